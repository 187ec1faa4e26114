"""-m gpu: the device-resident submission writer (csrc/submission_rays.hip through ext.submission_rays, metrics.SubmissionWriter,
io.format_submission_device and test_loop.run_test) against
  * the reference's own submission content (tests/golden/datasets.npz, keys sub_*) and per-ray rows
    (tests/golden/ray_metrics.npz, keys pcd_pred_*),
  * the numpy restatement on the reference-pinned caster (tests/submission_ref.py) and the rows of RayMetrics.update,
    converted by numpy, on small grids where the kernel can go wrong.
Every comparison is bit for bit; a NaN flow is compared with isnan only (its payload bits are unspecified)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from occnet_amd import io as oio
from tests import submission_ref as sref
from tests.golden_cases import METRIC_SEEDS, metric_scene
from tests.test_submission_device_host import F16_EDGES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.5
PC_MIN = (-1.5, -1.0, -0.5)
IDS_U8 = [0, 3, 7, 15, 17, 127, 128, 200, 255]
IDS_I64 = IDS_U8 + [300, -3]
FILL = 0xA5


def _pc_range(shape, voxel=VOXEL, pc_min=PC_MIN):
    return list(pc_min) + [pc_min[k] + shape[k] * voxel for k in range(3)]


def _metres(vox, voxel=VOXEL, pc_min=PC_MIN):
    """voxel coordinates -> ego metres (exact: voxel sizes here are powers of two)"""
    return [pc_min[k] + vox[k] * voxel for k in range(3)]


@pytest.fixture(scope='module')
def hand_rays():
    """300 directions = two blocks of 256, the second partial: the six axis directions, four in-plane diagonals (one component
    exactly zero), 290 seeded random unit vectors (from an origin outside the grid about half of them point away)."""
    rng = np.random.default_rng(5)
    axis = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    diag = np.array([[1, 1, 0], [1, -1, 0], [0, 1, 1], [-1, 0, -1]], np.float64) / np.sqrt(2.0)
    rnd = rng.normal(size=(290, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    return torch.from_numpy(np.concatenate([axis, diag, rnd]).astype(np.float32))


def _grid(shape, dtype, seed, ids, density=0.25):
    rng = np.random.default_rng(seed)
    sem = np.full(shape, 16, dtype)
    occ = rng.random(shape) < density
    sem[occ] = rng.choice(np.array(ids, dtype=np.int64), int(occ.sum())).astype(dtype)
    sem[0, 0, 0] = 5                      # the voxel that a ray which never enters the grid reports
    sem[2, 2, 1] = 3                      # an origin sits inside this one
    flow = (rng.normal(size=shape + (2,)) * 3).astype(np.float32)
    return sem, flow


def _origins3(shape, dtype=torch.float32):
    """(3, 3, 3) origins in metres with counts [3, 1, 2]: inside an occupied voxel, on a voxel face, outside beside the grid |
    outside above it | on a voxel edge, inside at a general position.  Slots beyond the counts hold 1e3: never to be cast."""
    o = torch.full((3, 3, 3), 1e3, dtype=torch.float64)
    o[0, 0] = torch.tensor(_metres((2.5, 2.5, 1.5)))
    o[0, 1] = torch.tensor(_metres((3.0, 1.5, 0.5)))
    o[0, 2] = torch.tensor(_metres((-2.5, 1.3, 0.7)))
    o[1, 0] = torch.tensor(_metres((2.2, 2.2, shape[2] + 3.5)))
    o[2, 0] = torch.tensor(_metres((1.0, 2.0, 0.5)))
    o[2, 1] = torch.tensor(_metres((1.3, 3.4, 1.6)))
    return o.to(dtype), [3, 1, 2]


def _want(sems, flows, origins, counts, rays, voxel=VOXEL, pc_min=PC_MIN):
    """per sample (cls, dist, flow) of submission_ref for its first counts[b] origins"""
    out = []
    for b, n in enumerate(counts):
        labels, rows = sref.rows(sems[b], flows[b], origins[b, :n], rays, pc_min, voxel)
        with np.errstate(over='ignore'):
            out.append(sref.pack(labels, rows))
    return out


def _run(sems, flows, origins, counts, rays, voxel=VOXEL, pc_min=PC_MIN, **kw):
    from occnet_amd import ext
    B, T, R = len(sems), origins.shape[1], rays.shape[0]
    out = torch.full((ext.submission_rays_bytes(B, T, R),), FILL, dtype=torch.uint8, device='cuda')
    sem = torch.from_numpy(np.stack(sems)).cuda()
    flow = torch.from_numpy(np.stack(flows)).cuda()
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32).cuda()
    views = ext.submission_rays(sem, flow, origins.cuda().contiguous(), rays.cuda(), pc_min, voxel, 16, origin_counts=cnt,
                                out=out, **kw)
    return out, views


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _assert_rows(got, want, what=''):
    """(cls int8, dist fp16, flow fp16 (n, 2)) bit for bit; NaN flows by isnan"""
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
    assert np.array_equal(got[0], want[0]), (what, 'cls', int((got[0] != want[0]).sum()))
    assert not np.isnan(want[1]).any()
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, 'dist', int((_bits(got[1]) != _bits(want[1])).sum()))
    nan = np.isnan(want[2])
    assert np.array_equal(np.isnan(got[2]), nan), (what, 'flow nan')
    assert np.array_equal(_bits(got[2])[~nan], _bits(want[2])[~nan]), (what, 'flow')


def _check_batch(out, views, want, counts, T, R):
    cls, dist, flow = (v.cpu().numpy() for v in views)
    for b, n in enumerate(counts):
        got = (cls[b, :n].reshape(-1), dist[b, :n].reshape(-1), flow[b, :n].reshape(-1, 2))
        _assert_rows(got, want[b], f'sample {b}')
        # rows beyond the counts keep the byte they were pre-filled with
        assert (cls[b, n:].view(np.uint8) == FILL).all()
        assert (dist[b, n:].view(np.uint8) == FILL).all() and (flow[b, n:].view(np.uint8) == FILL).all()
    # and so does the padding between the sections
    n_rows, _, off_dist, off_flow, total = sref.layout(len(counts), T, R)
    raw = out.cpu().numpy()
    assert raw.shape == (total,)
    for lo, hi in ((n_rows, off_dist), (off_dist + 2 * n_rows, off_flow), (off_flow + 4 * n_rows, total)):
        assert (raw[lo:hi] == FILL).all()


def _from_metric_rows(rows, counts):
    """RayMetrics.update(return_rays=True) prediction rows (B, T, R, 4) -> per sample (cls, dist, flow) by numpy"""
    rows = rows.cpu().numpy()
    out = []
    for b, n in enumerate(counts):
        r = rows[b, :n].reshape(-1, 4)
        with np.errstate(over='ignore'):
            out.append(sref.pack(r[:, 0].astype(np.int64), r))
    return out


SHAPES = {'u8_6x5x3': ((6, 5, 3), np.uint8, IDS_U8), 'i64_7x9x20': ((7, 9, 20), np.int64, IDS_I64)}


@pytest.fixture(scope='module')
def cases(hand_rays):
    """the B = 3 batch of each small shape with its reference rows, computed once"""
    out = {}
    for name, (shape, dtype, ids) in SHAPES.items():
        grids = [_grid(shape, dtype, 100 + b, ids) for b in range(3)]
        sems, flows = [g[0] for g in grids], [g[1] for g in grids]
        origins, counts = _origins3(shape)
        out[name] = dict(shape=shape, sems=sems, flows=flows, origins=origins, counts=counts,
                         want=_want(sems, flows, origins, counts, hand_rays))
    return out


# ---- the reference's own runs ---------------------------------------------------------------------------------------------
def test_file_equals_reference_submission_and_host_path(tmp_path):
    from tests.test_io_golden import GOLD, _check_submission, _samples
    gold = dict(np.load(GOLD))
    path = oio.format_submission_device(_samples(), str(tmp_path / 'dev'), batch=2)       # 3 samples: a batch of 2 and one of 1
    assert path == str(tmp_path / 'dev' / 'submission.gz')
    _check_submission(gold, oio.read_submission(path))                                   # dtype, shape and bits of sub_*
    host = oio.format_submission(_samples(), str(tmp_path / 'host'))
    with open(path, 'rb') as a, open(host, 'rb') as b:
        assert a.read() == b.read()
    # device tensors in, one batch of all three, a header of the caller's
    dev = [(t, torch.as_tensor(s).cuda(), torch.as_tensor(f).cuda(), o) for t, s, f, o in _samples()]
    sub = oio.read_submission(oio.format_submission_device(dev, str(tmp_path / 'dev8'), header={'method': 'm'}))
    assert sorted(sub) == ['method', 'results']
    assert sub['method'] == 'm'
    _check_submission(gold, dict(oio.SUBMISSION_HEADER, results=sub['results']))


def test_packed_rows_equal_reference_rows():
    from occnet_amd import ext
    from occnet_amd.metrics import generate_lidar_rays
    gold = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'ray_metrics.npz')))
    scenes = [metric_scene(s) for s in METRIC_SEEDS]
    rays = torch.from_numpy(generate_lidar_rays()).cuda()
    for dtype in (np.uint8, np.int64):
        sem = torch.from_numpy(np.stack([s[0].astype(dtype) for s in scenes])).cuda()
        flow = torch.from_numpy(np.stack([s[2] for s in scenes])).cuda()
        origins = torch.cat([s[4] for s in scenes]).cuda()
        assert origins.dtype == torch.float32 and tuple(origins.shape) == (2, 2, 3)
        cls, dist, fl = (v.cpu().numpy() for v in ext.submission_rays(sem, flow, origins, rays, [-40, -40, -1.0], 0.4))
        for i in range(len(scenes)):
            p = gold[f'pcd_pred_{i}']
            want = (p[:, 0].astype(np.int8), p[:, 1].astype(np.float16), p[:, 2:4].astype(np.float16))
            _assert_rows((cls[i].reshape(-1), dist[i].reshape(-1), fl[i].reshape(-1, 2)), want, f'scene {i} {dtype}')


# ---- small shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_small_shapes_ragged_batch(cases, hand_rays, name):
    from occnet_amd.metrics import RayMetrics
    c = cases[name]
    T, R = 3, hand_rays.shape[0]
    assert R == 300
    out, views = _run(c['sems'], c['flows'], c['origins'], c['counts'], hand_rays)
    _check_batch(out, views, c['want'], c['counts'], T, R)
    # what the cases are there for
    cls0, dist0, _ = c['want'][0]
    never = _bits(dist0[2 * R:]) == _bits(np.float16(-VOXEL))                  # third origin of sample 0: outside the grid
    assert 50 < int(never.sum()) < R and (cls0[2 * R:][never] == 5).all()
    assert (cls0[:R] == 3).all()                                               # origin inside an occupied voxel: every ray
    assert (np.concatenate([w[0] for w in c['want']]) < 0).any()               # class ids above 127 were met
    # the evaluator's rows of the same casts, converted by numpy
    m = RayMetrics(_pc_range(c['shape']), VOXEL, rays=hand_rays)
    assert m.occ_size == list(c['shape'])
    sem = torch.from_numpy(np.stack(c['sems'])).cuda()
    flow = torch.from_numpy(np.stack(c['flows'])).cuda()
    cnt = torch.tensor(c['counts'], dtype=torch.int32).cuda()
    rows_pred, _ = m.update(sem, flow, sem, flow, c['origins'].cuda(), return_rays=True, origin_counts=cnt)
    _check_batch(out, views, _from_metric_rows(rows_pred, c['counts']), c['counts'], T, R)


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_small_shapes_float64_origins(cases, hand_rays, name):
    """float64 origins: the conversion to voxel units runs in float64, as process_one_sample's does for them"""
    c = cases[name]
    origins, counts = _origins3(c['shape'], torch.float64)
    origins[:, :, :] += torch.tensor([1e-9, -3e-10, 7e-10], dtype=torch.float64)        # not representable in float32
    want = _want(c['sems'], c['flows'], origins, counts, hand_rays)
    out, views = _run(c['sems'], c['flows'], origins, counts, hand_rays)
    _check_batch(out, views, want, counts, 3, hand_rays.shape[0])
    # no origin_counts: every slot is cast (the junk ones report voxel (0, 0, 0) for every ray)
    full = [3, 3, 3]
    out, views = _run(c['sems'], c['flows'], origins, None, hand_rays)
    _check_batch(out, views, _want(c['sems'], c['flows'], origins, full, hand_rays), full, 3, hand_rays.shape[0])


# ---- rounding -------------------------------------------------------------------------------------------------------------
def test_float16_rounding_edges(hand_rays):
    shape, voxel, pc_min = (7, 9, 20), 8192.0, (0.0, 0.0, 0.0)
    sem, flow = _grid(shape, np.int64, 7, IDS_I64, density=0.08)
    edges = np.array([v for v, _ in F16_EDGES] + [np.nan], np.float32)
    flow.reshape(-1)[:] = edges[np.arange(flow.size) % edges.size]
    origins = torch.tensor([[_metres((3.5, 4.5, 10.5), voxel, pc_min), _metres((-1.5, 4.2, 9.1), voxel, pc_min)]],
                           dtype=torch.float32)
    labels, rows = sref.rows(sem, flow, origins[0], hand_rays, pc_min, voxel)
    with np.errstate(over='ignore'):
        want = sref.pack(labels, rows)
    # the inputs reach every edge: each value was read at a hit voxel, depths on both sides of the float16 range
    seen = rows[:, 2:4].reshape(-1)
    for v in edges[:-1]:
        assert ((seen == v) & (np.signbit(seen) == np.signbit(v))).any(), v
    assert np.isnan(seen).any()
    assert (rows[:, 1] > 65520).any() and ((rows[:, 1] > 0) & (rows[:, 1] < 65504)).any()
    assert np.isinf(want[1]).any() and np.isnan(want[2]).any()
    out, views = _run([sem], [flow], origins, [2], hand_rays, voxel, pc_min)
    _check_batch(out, views, [want], [2], 2, hand_rays.shape[0])
    # and the table itself, value by value, where the row's float32 flow is the edge
    got_flow = views[2].cpu().numpy().reshape(-1)
    for v, b in F16_EDGES:
        sel = (seen == np.float32(v)) & (np.signbit(seen) == np.signbit(np.float32(v)))
        assert (_bits(got_flow)[sel] == b).all(), (v, hex(b))


# ---- determinism and entry points -----------------------------------------------------------------------------------------
def test_determinism_workspace_c_abi_and_stream(cases, hand_rays):
    from occnet_amd import _lib, ext
    c = cases['i64_7x9x20']
    B, T, R = 3, 3, hand_rays.shape[0]
    X, Y, Z = c['shape']
    first, _ = _run(c['sems'], c['flows'], c['origins'], c['counts'], hand_rays)
    first = first.cpu().numpy()
    again, _ = _run(c['sems'], c['flows'], c['origins'], c['counts'], hand_rays)
    assert np.array_equal(again.cpu().numpy(), first)
    ws = torch.full((ext.submission_rays_workspace_bytes(B, X, Y, Z) + 512,), 0xFF, dtype=torch.uint8, device='cuda')
    assert torch.isnan(ws[:1024].view(torch.float32)).all()
    nan_ws, _ = _run(c['sems'], c['flows'], c['origins'], c['counts'], hand_rays, workspace=ws)
    assert np.array_equal(nan_ws.cpu().numpy(), first)
    assert (ws[-512:] == 0xFF).all()                                           # nothing written past the size the query gives
    # the C ABI, called directly
    sem = torch.from_numpy(np.stack(c['sems'])).cuda()
    flow = torch.from_numpy(np.stack(c['flows'])).cuda()
    origins, rays = c['origins'].cuda().contiguous(), hand_rays.cuda()
    cnt = torch.tensor(c['counts'], dtype=torch.int32).cuda()
    out = torch.full((ext.submission_rays_bytes(B, T, R),), FILL, dtype=torch.uint8, device='cuda')
    ws = torch.empty(ext.submission_rays_workspace_bytes(B, X, Y, Z), dtype=torch.uint8, device='cuda')
    p, f = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_float
    rc = _lib.lib().occ_submission_rays(p(sem), 1, p(flow), p(origins), 0, p(cnt), p(rays), f(PC_MIN[0]), f(PC_MIN[1]),
                                        f(PC_MIN[2]), f(VOXEL), 16, p(out), ctypes.c_int64(out.numel()), p(ws),
                                        ctypes.c_int64(ws.numel()), B, T, X, Y, Z, R,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert np.array_equal(out.cpu().numpy(), first)
    # a stream of the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out2 = torch.full_like(out, FILL)
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(side):
        ext.submission_rays(sem, flow, origins, rays, PC_MIN, VOXEL, 16, origin_counts=cnt, out=out2)
    side.synchronize()
    assert np.array_equal(out2.cpu().numpy(), first)


def test_unsupported_depth():
    from occnet_amd import ext
    from occnet_amd._lib import OccAmdUnsupported
    sem = torch.full((1, 4, 4, 33), 16, dtype=torch.uint8).cuda()
    out = torch.full((1024,), FILL, dtype=torch.uint8, device='cuda')
    with pytest.raises(OccAmdUnsupported):
        ext.submission_rays(sem, torch.zeros(1, 4, 4, 33, 2).cuda(), torch.zeros(1, 1, 3).cuda(), torch.zeros(8, 3).cuda(),
                            PC_MIN, VOXEL, out=out)
    assert (out == FILL).all()


# ---- the writer -----------------------------------------------------------------------------------------------------------
def _stream_batches(shape, seed=21):
    """five batches B = 1, 2, 3, 1, 2 with ragged origin counts, uint8 and int64 grids, float32 and float64 origins"""
    rng = np.random.default_rng(seed)
    batches, k = [], 0
    for i, B in enumerate((1, 2, 3, 1, 2)):
        dtype, ids = ((np.uint8, IDS_U8), (np.int64, IDS_I64))[i % 2]
        T = (3, 2, 3, 1, 2)[i]
        counts = [int(rng.integers(1, T + 1)) for _ in range(B)]
        counts[0] = T
        grids = [_grid(shape, dtype, 300 + k + b, ids) for b in range(B)]
        vox = rng.uniform([-2, -2, -2], [shape[0] + 2, shape[1] + 2, shape[2] + 2], size=(B, T, 3))
        origins = torch.tensor(np.asarray(PC_MIN) + vox * VOXEL, dtype=(torch.float32, torch.float64)[i % 3 == 1])
        batches.append(dict(tokens=[f'tok{k + b}' for b in range(B)], sems=[g[0] for g in grids], flows=[g[1] for g in grids],
                            origins=origins, counts=counts))
        k += B
    return batches


def _results_equal(a, b):
    assert list(a) == list(b)
    for tok in a:
        assert sorted(a[tok]) == ['pcd_cls', 'pcd_dist', 'pcd_flow']
        _assert_rows(tuple(a[tok][k] for k in ('pcd_cls', 'pcd_dist', 'pcd_flow')),
                     tuple(b[tok][k] for k in ('pcd_cls', 'pcd_dist', 'pcd_flow')), tok)


def test_writer_streams_batches_in_order(hand_rays, tmp_path):
    from occnet_amd.metrics import SubmissionWriter
    shape = (7, 9, 20)
    batches = _stream_batches(shape)
    w = SubmissionWriter(_pc_range(shape), VOXEL, rays=hand_rays, depth=2)
    one = SubmissionWriter(_pc_range(shape), VOXEL, rays=hand_rays.numpy(), depth=1)
    R = hand_rays.shape[0]
    for i, bt in enumerate(batches):
        sem = torch.from_numpy(np.stack(bt['sems'])).cuda()
        flow = torch.from_numpy(np.stack(bt['flows'])).cuda()
        origins = bt['origins'].cuda() if i % 2 else bt['origins']                      # device and host origins
        w.add(bt['tokens'], sem, flow, origins, origin_counts=bt['counts'])
        for b, tok in enumerate(bt['tokens']):
            one.add(tok, sem[b], flow[b], bt['origins'][b:b + 1, :bt['counts'][b]])
    with pytest.raises(ValueError, match='tok4'):
        w.add(['fresh', 'tok4'], sem, flow, origins)                                    # a token of an earlier batch
    with pytest.raises(ValueError, match='twice|duplicate'):
        w.add(['x', 'x'], sem, flow, origins)
    with pytest.raises(ValueError, match='origin_counts'):
        w.add(['y', 'z'], sem, flow, origins, origin_counts=[1, origins.shape[1] + 1])
    res = w.results()
    assert list(res) == [f'tok{k}' for k in range(9)]                                   # insertion order, nothing from the refused calls
    _results_equal(res, one.results())
    for bt in batches:
        for b, tok in enumerate(bt['tokens']):
            assert res[tok]['pcd_cls'].shape == (bt['counts'][b] * R,) and res[tok]['pcd_flow'].shape == (bt['counts'][b] * R, 2)
    # one sample against the restatement, so that the two writers are not merely wrong alike
    bt = batches[2]
    want = _want(bt['sems'], bt['flows'], bt['origins'], bt['counts'], hand_rays)
    for b, tok in enumerate(bt['tokens']):
        _assert_rows(tuple(res[tok][k] for k in ('pcd_cls', 'pcd_dist', 'pcd_flow')), want[b], tok)
    # the file, and the parts of a two-rank run merged back into it
    path = w.write(str(tmp_path / 'sub'))
    sub = oio.read_submission(path)
    assert {k: v for k, v in sub.items() if k != 'results'} == oio.SUBMISSION_HEADER
    _results_equal(sub['results'], res)
    ranks = [SubmissionWriter(_pc_range(shape), VOXEL, rays=hand_rays) for _ in range(2)]
    flat = [(tok, bt['sems'][b], bt['flows'][b], bt['origins'][b:b + 1, :bt['counts'][b]])
            for bt in batches for b, tok in enumerate(bt['tokens'])][:8]
    for i, (tok, s, f, o) in enumerate(flat):
        ranks[i % 2].add(tok, torch.from_numpy(s).cuda(), torch.from_numpy(f).cuda(), o)
    parts = [r.save_part(str(tmp_path / f'part{k}.gz')) for k, r in enumerate(ranks)]
    merged = oio.read_submission(oio.merge_submission_parts(parts, str(tmp_path / 'merged')))
    _results_equal(merged['results'], {t: res[t] for t in list(res)[:8]})


# ---- the loop -------------------------------------------------------------------------------------------------------------
class _StubModel:
    """simple_test returns prepared device tensors, as BEVFormerOcc.simple_test does: (bev_embed, occ_cls, flow)"""

    def __init__(self, outs):
        self.outs, self.calls = outs, []

    def simple_test(self, img_metas, img):
        self.calls.append((img_metas, img))
        occ_cls, flow = self.outs[len(self.calls) - 1]
        return None, occ_cls, flow


def test_run_test_feeds_metric_and_writer(hand_rays):
    from occnet_amd.metrics import RayMetrics, SubmissionWriter
    from occnet_amd.test_loop import run_test
    shape = (7, 9, 20)
    pc_range = _pc_range(shape)
    rng = np.random.default_rng(31)
    samples, outs = [], []
    for i in range(3):
        sp, fp = _grid(shape, np.int64, 400 + i, IDS_U8[:5])
        sg, fg = _grid(shape, np.uint8, 500 + i, IDS_U8[:5])
        sg[sp < 16] = sp[sp < 16]                                                       # mostly agreeing with the prediction
        vox = rng.uniform([1, 1, 1], [6, 8, 19], size=(1, 2, 3))
        origins = torch.tensor(np.asarray(PC_MIN) + vox * VOXEL, dtype=torch.float32)
        outs.append((torch.from_numpy(sp)[None].cuda(), torch.from_numpy(fp)[None].cuda()))
        samples.append(dict(token=f's{i}', img_metas=[{'i': i}], img=i, lidar_origins=origins,
                            voxel_semantics=torch.from_numpy(sg)[None].cuda(), voxel_flow=torch.from_numpy(fg)[None].cuda()))
    model = _StubModel(outs)
    metric = RayMetrics(pc_range, VOXEL, rays=hand_rays)
    writer = SubmissionWriter(pc_range, VOXEL, rays=hand_rays)
    assert run_test(model, iter(samples), metric=metric, writer=writer) == 3
    assert [c[1] for c in model.calls] == [0, 1, 2] and model.calls[1][0] == [{'i': 1}]
    direct_m = RayMetrics(pc_range, VOXEL, rays=hand_rays)
    direct_w = SubmissionWriter(pc_range, VOXEL, rays=hand_rays)
    for s, (occ_cls, flow) in zip(samples, outs):
        direct_m.update(occ_cls, flow, s['voxel_semantics'], s['voxel_flow'], s['lidar_origins'])
        direct_w.add(s['token'], occ_cls, flow, s['lidar_origins'])
    assert int(metric.state[:17].sum()) > 0
    assert torch.equal(metric.state, direct_m.state)
    _results_equal(writer.results(), direct_w.results())
    # one consumer at a time, and none at all
    only_w = SubmissionWriter(pc_range, VOXEL, rays=hand_rays)
    assert run_test(_StubModel(outs), samples, writer=only_w) == 3
    _results_equal(only_w.results(), direct_w.results())
    only_m = RayMetrics(pc_range, VOXEL, rays=hand_rays)
    run_test(_StubModel(outs), samples, metric=only_m)
    assert torch.equal(only_m.state, direct_m.state)
    with pytest.raises(ValueError):
        run_test(_StubModel(outs), samples)
