"""-m gpu: the server-side scorer on the device (csrc/submission_score.hip through ext.submission_score_accumulate,
metrics.SubmissionScore, SubmissionWriter.add_scored, io.score_submission and test_loop.run_test) against the numpy restatement
of the reference's tools/ray_iou/metric.py (tests/submission_score_ref.py) and the numbers metric.py itself left in
tests/golden/ray_metrics.npz.  Every case compares all 17 * ncls state words for equality."""
import os

import numpy as np
import pytest
import torch

from occnet_amd import io as oio
from tests import submission_ref as sref
from tests import submission_score_ref as ssr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ray_metrics.npz')
COUNTS = [1, 63, 64, 65, 255, 257, 1025]
STRIDE = 1100                 # > every count; 2 blocks per sample by the launcher's rule, 5 steps of one block at 1025 rows
STRANGERS = [-128, -1, 17, 127]


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def _side(samples, stride, fmt):
    """samples: list of (cls, dist, flow) -> what ext.submission_score_accumulate takes; the padding rows hold class 0 and
    NaN flow, which must not show"""
    B = len(samples)
    if fmt == 0:
        cls = np.zeros((B, stride), np.int8)
        dist = np.zeros((B, stride), np.float16)
        flow = np.full((B, stride, 2), np.nan, np.float16)
        for b, (c, d, f) in enumerate(samples):
            assert c.dtype == np.int8 and d.dtype == np.float16 and f.dtype == np.float16
            cls[b, :len(c)], dist[b, :len(c)], flow[b, :len(c)] = c, d, f
        return tuple(torch.from_numpy(a).cuda() for a in (cls, dist, flow))
    rows = np.zeros((B, stride, 4), np.float32)
    rows[:, :, 2:] = np.nan
    for b, (c, d, f) in enumerate(samples):
        assert c.dtype == np.float32 and d.dtype == np.float32 and f.dtype == np.float32
        rows[b, :len(c), 0], rows[b, :len(c), 1], rows[b, :len(c), 2:] = c, d, f
    return torch.from_numpy(rows).cuda()


def _as(samples, fmt):
    """samples of values exact in int8 / float16 -> the arrays of format fmt"""
    types = (np.int8, np.float16, np.float16) if fmt == 0 else (np.float32,) * 3
    return [tuple(np.asarray(a).astype(t) for a, t in zip(s, types)) for s in samples]


def _device_state(pred, gt, free_id, fmts=(1, 1), stride=None, state=None, **kw):
    from occnet_amd import ext
    counts = [len(s[0]) for s in gt]
    stride = max(counts) if stride is None else stride
    if state is None:
        state = torch.zeros(ext.submission_score_state_words(free_id), dtype=torch.int64, device='cuda')
    ext.submission_score_accumulate(state, _side(_as(pred, fmts[0]), stride, fmts[0]), _side(_as(gt, fmts[1]), stride, fmts[1]),
                                    torch.tensor(counts, dtype=torch.int32).cuda(), stride, free_id, **kw)
    return state


def _ref(pred, gt, free_id, fmts=(1, 1)):
    ref = ssr.Ref(free_id)
    for p, g in zip(_as(pred, fmts[0]), _as(gt, fmts[1])):
        ref.add(p, g)
    return ref


def _equal(state, ref, what=''):
    got, want = state.cpu().numpy(), ref.words()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, [(int(i) // ref.ncls, int(i) % ref.ncls, int(got[i]), int(want[i])) for i in bad[:8]])


# ---- the reference's own rows -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope='module')
def gold_samples(gold):
    n = sum(1 for k in gold if k.startswith('pcd_pred_'))
    return ([ssr.split_rows(gold[f'pcd_pred_{i}']) for i in range(n)], [ssr.split_rows(gold[f'pcd_gt_{i}']) for i in range(n)])


def test_golden_rows_as_float32_rows(gold, gold_samples):
    from occnet_amd.metrics import SubmissionScore
    pred, gt = gold_samples
    ref = _ref(pred, gt, 16)
    m = SubmissionScore()
    m.update_rows(torch.from_numpy(np.stack([gold[f'pcd_pred_{i}'] for i in range(len(pred))])),
                  np.stack([gold[f'pcd_gt_{i}'] for i in range(len(gt))]))
    _equal(m.state, ref, 'rows')
    out = m.compute()
    assert np.array_equal(np.stack(out['iou_list']), gold['metric_py_iou'], equal_nan=True)
    want = gold['metric_py_ave']
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(out['ave_list']), ~ok) and ok.sum() >= 2
    rel = np.abs(out['ave_list'][ok] - want[ok]) / want[ok]
    print('AVE against metric_py_ave, relative:', rel)
    assert (rel < 2e-6).all()            # metric.py's float32 pairwise sum: about 26 roundings of 2^-24 (tests/test_submission_score_host.py)
    res = ref.compute()
    assert np.array_equal(out['ave_list'], res['ave_fixed'], equal_nan=True)
    want_out = ssr.output(res['iou_list'], res['ave_fixed'])
    assert all(out[k] == want_out[k] for k in want_out)


@pytest.mark.parametrize('fmts', [(0, 0), (0, 1), (1, 0)])
def test_golden_rows_packed_on_the_host_and_mixed(gold, fmts):
    n = sum(1 for k in gold if k.startswith('pcd_pred_'))
    sides = []
    for name, fmt in (('pcd_pred', fmts[0]), ('pcd_gt', fmts[1])):
        rows = [gold[f'{name}_{i}'] for i in range(n)]
        sides.append([ssr.pack_rows(r) if fmt == 0 else tuple(np.ascontiguousarray(a) for a in ssr.split_rows(r)) for r in rows])
    pred, gt = sides
    ref = ssr.Ref(16)
    for p, g in zip(pred, gt):
        ref.add(p, g)
    _equal(_device_state(pred, gt, 16, fmts), ref, str(fmts))
    if fmts == (0, 0):                   # the rounding moved rays across a threshold: this is not the float32 score
        flt = _ref([ssr.split_rows(gold[f'pcd_pred_{i}']) for i in range(n)],
                   [ssr.split_rows(gold[f'pcd_gt_{i}']) for i in range(n)], 16)
        assert ref.tp != flt.tp


# ---- edge shapes ----------------------------------------------------------------------------------------------------------
def _random_sample(rng, n, free_id):
    """values exact in int8 / float16, so that one sample can travel in either format"""
    ids = np.array(list(range(free_id + 1)) + STRANGERS)
    w = np.ones(len(ids))
    w[free_id] = 3                                              # a good share of free ground truth
    gc = rng.choice(ids, n, p=w / w.sum())
    pc = np.where(rng.random(n) < 0.6, gc, rng.choice(ids, n))
    gd = rng.integers(0, 80, n) * 0.25
    pd = gd + rng.choice([0, 0.25, 0.75, 1, 1.25, 2, 2.5, 4, 6], n) * rng.choice([-1, 1], n)
    gf = rng.integers(-40, 40, (n, 2)) * 0.125
    pf = rng.integers(-40, 40, (n, 2)) * 0.125
    return (pc, pd, pf), (gc, gd, gf)


def _set(side, i, cls, dist, flow=(0.0, 0.0)):
    side[0][i], side[1][i], side[2][i] = cls, dist, flow


def _edge_batch(free_id):
    rng = np.random.default_rng(100 + free_id)
    pred, gt = [], []
    for n in COUNTS:
        p, g = _random_sample(rng, n, free_id)
        pred.append(p)
        gt.append(g)
    a, b = 0, 1                                                 # two flow classes that exist for ncls = 3 and 17
    # sample 0 (1 row): ground truth all free, prediction not
    _set(gt[0], 0, free_id, 3.0)
    _set(pred[0], 0, a, 3.0, (1.0, 2.0))
    # sample 1 (63 rows): valid rays, no true positive: the classes never meet
    gt[1][0][:] = a
    pred[1][0][:] = np.where(np.arange(63) % 2, b, free_id)
    # sample 2 (64 rows): class `a` has its only true positive at threshold 4; class b none at all
    gt[2][0][:] = np.where(np.arange(64) % 2, b, free_id)
    pred[2][0][:] = a
    _set(gt[2], 5, a, 10.0, (1.0, 0.0))
    _set(pred[2], 5, a, 13.0, (0.0, 1.0))
    # sample 3 (65 rows): depth differences of exactly 1, 2 and 4 are no hits; one float16 step below they are
    gt[3][0][:] = free_id
    for i, (d, hit) in enumerate([(1.0, 0), (2.0, 0), (4.0, 0), (1.0 - 2.0 ** -7, 1), (2.0 - 2.0 ** -7, 1), (4.0 - 2.0 ** -7, 1)]):
        _set(gt[3], i, b, 10.0, (0.5, 0.5))
        _set(pred[3], i, b, 10.0 + d if i % 2 else 10.0 - d, (0.25, -0.5))
    # sample 4 (255 rows): the classes no table has, on either side and on both
    for i, c in enumerate(STRANGERS):
        _set(gt[4], i, c, 5.0)
        _set(pred[4], i, c, 5.0)                                # equal and close, but a true positive of no class
        _set(gt[4], 10 + i, c, 5.0)
        _set(pred[4], 10 + i, a, 5.0)
        _set(gt[4], 20 + i, a, 5.0)
        _set(pred[4], 20 + i, c, 5.0)
    _set(gt[4], 30, a, 5.0)
    _set(pred[4], 30, a, 5.5)                                   # one true positive of class a, so that the sample's AVE terms count
    # samples 5, 6 (257, 1025 rows): ground truth free under a non-free prediction, in the last row of the last block too
    for s in (5, 6):
        _set(gt[s], COUNTS[s] - 1, free_id, 2.0)
        _set(pred[s], COUNTS[s] - 1, b, 2.0, (3.0, 3.0))
    return pred, gt


@pytest.fixture(scope='module', params=[16, 2])
def edge(request):
    free_id = request.param
    pred, gt = _edge_batch(free_id)
    return dict(free_id=free_id, pred=pred, gt=gt, ref=_ref(pred, gt, free_id))


def test_edge_batch_is_what_it_is_for(edge):
    free_id, pred, gt = edge['free_id'], edge['pred'], edge['gt']
    one = [_ref(pred[i:i + 1], gt[i:i + 1], free_id) for i in range(len(COUNTS))]
    assert not one[0].words().any()                                                  # all free: nothing at all
    assert one[1].gt_cnt[0] == 63 and not np.array(one[1].tp).any() and not np.array(one[1].ave_cnt).any()
    assert [one[2].tp[j][0] for j in range(3)] == [0, 0, 1]
    assert [one[2].ave_cnt[j][0] for j in range(3)] == [0, 0, int((gt[2][0] != free_id).sum())]
    assert not np.array(one[2].ave_cnt)[:, 1].any()
    assert [one[3].tp[j][1] for j in range(3)] == [1, 3, 5] and one[3].gt_cnt[1] == 6   # of differences 1-, 1, 2-, 2, 4-, 4
    assert sum(one[4].gt_cnt) < int((gt[4][0] != free_id).sum())                     # valid rays of no class
    assert one[4].ave_cnt[1][0] == int((gt[4][0] != free_id).sum())                  # ... still count in the AVE
    assert (np.array(edge['ref'].ave_cnt) > np.array(edge['ref'].tp)).any()


@pytest.mark.parametrize('fmts', [(1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize('max_chunks', [0, 1])
def test_edge_shapes_ragged_batch(edge, fmts, max_chunks):
    state = _device_state(edge['pred'], edge['gt'], edge['free_id'], fmts, stride=STRIDE, max_chunks=max_chunks)
    _equal(state, edge['ref'], f'{fmts} {max_chunks}')


# ---- non-finite errors ------------------------------------------------------------------------------------------------------
def test_non_finite_errors():
    from occnet_amd.metrics import SubmissionScore
    inf = np.inf

    def sample(cls, pflow, gflow, n=40):
        """n valid rays of ground-truth class 9 (no flow class, never predicted) and one true positive of class `cls`"""
        gc, pc = np.full(n, 9.0), np.full(n, 10.0)
        gc[3] = pc[3] = cls
        d = np.full(n, 7.0)
        pf, gf = np.full((n, 2), 0.5), np.full((n, 2), 0.25)
        pf[7], gf[7] = pflow, gflow
        return (pc, d, pf), (gc, d.copy(), gf)

    packed = [sample(0, (inf, 0.0), (1.0, 1.0)),                 # fp16 inf flow: an infinite error
              sample(1, (inf, 0.0), (inf, 0.0))]                 # inf - inf = NaN
    with np.errstate(all='ignore'):
        rows = [sample(2, (3e38, 0.0), (0.0, 0.0)),              # ux * ux overflows float32: numpy's error is inf
                sample(3, (2.0 ** 34, 0.0), (0.0, 0.0)),         # a finite error at the fixed-point limit: counted as infinite
                sample(4, (2.0 ** 34 - 1024.0, 0.0), (0.0, 0.0))]   # the largest error that is still added
    ref = ssr.Ref(16)
    m = SubmissionScore()
    for batch, fmt in ((packed, 0), (rows, 1)):
        pred, gt = _as([s[0] for s in batch], fmt), _as([s[1] for s in batch], fmt)
        for p, g in zip(pred, gt):
            ref.add(p, g)
        _device_state(pred, gt, 16, (fmt, fmt), state=m.state)
    _equal(m.state, ref)
    assert [ref.ave_inf[1][c] for c in range(5)] == [1, 0, 1, 1, 0] and [ref.ave_nan[1][c] for c in range(5)] == [0, 1, 0, 0, 0]
    assert ref.ave_sum[1][4] > 2 ** 61 and ref.ave_inf[1][4] == 0
    out, res = m.compute(), ref.compute()
    ave = out['ave_list']
    assert ave[0] == inf and np.isnan(ave[1]) and ave[2] == inf and np.isnan(ave[5:]).all()
    for c in (0, 1, 2):                                           # inf where numpy gives inf, NaN where it gives NaN
        assert np.array_equal(ave[c], res['ave_np'][c], equal_nan=True) and np.array_equal(ave[c], res['ave_f64'][c], equal_nan=True)
    assert ave[3] == inf and np.isfinite(res['ave_np'][3])        # the documented limit: >= 2^34 m/s reports inf
    assert abs(ave[4] - res['ave_f64'][4]) <= 1e-12 * res['ave_f64'][4]
    assert np.array_equal(ave, res['ave_fixed'], equal_nan=True)
    assert out['mAVE'] == inf and out['final_Occ_Score'] == out['RayIoU'] * 0.9


# ---- accumulation and order -------------------------------------------------------------------------------------------------
def test_accumulation_order_and_workspace(edge):
    from occnet_amd import ext
    from occnet_amd.metrics import SubmissionScore
    free_id, pred, gt, ref = edge['free_id'], edge['pred'], edge['gt'], edge['ref']
    whole = _device_state(pred, gt, free_id, stride=STRIDE)
    _equal(whole, ref)
    assert torch.equal(_device_state(pred, gt, free_id, stride=STRIDE), whole)                      # two runs
    # two updates into one state = the sum of both, each checked on its own as well
    first = _device_state(pred[:3], gt[:3], free_id)
    _equal(first, _ref(pred[:3], gt[:3], free_id))
    second = _device_state(pred[3:], gt[3:], free_id)
    both = _device_state(pred[3:], gt[3:], free_id, state=first.clone())
    assert torch.equal(both, first + second) and torch.equal(both, whole)
    # another split, sample by sample in reverse order, through SubmissionScore.update_rows and merge
    parts = [SubmissionScore(free_id=free_id) for _ in range(2)]
    for i in reversed(range(len(COUNTS))):
        p, g = (np.concatenate([np.asarray(a, np.float32).reshape(COUNTS[i], -1) for a in s], 1) for s in (pred[i], gt[i]))
        parts[i % 2].update_rows(p, g)
    assert not torch.equal(parts[0].state, whole)
    assert torch.equal(parts[0].merge(parts[1]).state, whole)
    assert int(parts[0].reset().state.abs().sum()) == 0
    # counts given to update_rows, padding rows that must not show
    m = SubmissionScore(free_id=free_id)
    m.update_rows(_side(_as(pred, 1), STRIDE, 1), _side(_as(gt, 1), STRIDE, 1), counts=COUNTS)
    assert torch.equal(m.state, whole)
    # the workspace is scratch: 0xFF-filled it changes nothing, and nothing is written past the size the query gives
    need = ext.submission_score_workspace_bytes(len(COUNTS))
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device='cuda')
    assert torch.equal(_device_state(pred, gt, free_id, stride=STRIDE, workspace=ws), whole)
    assert (ws[-512:] == 0xFF).all()


# ---- the writer, the file and the loop --------------------------------------------------------------------------------------
VOXEL = 0.5
PC_MIN = (-1.5, -1.0, -0.5)
SHAPE = (24, 20, 8)


def _grids(dtype_pred, dtype_gt, seed):
    rng = np.random.default_rng(seed)
    sg = np.full(SHAPE, 16, dtype_gt)
    occ = rng.random(SHAPE) < 0.2
    sg[occ] = rng.integers(0, 16, int(occ.sum())).astype(dtype_gt)
    sp = sg.astype(dtype_pred)
    flip = rng.random(SHAPE) < 0.15
    sp[flip] = rng.choice(np.array([0, 1, 2, 7, 9, 16, 16, 16, 100, 200]), int(flip.sum())).astype(dtype_pred)
    fg = (rng.normal(size=SHAPE + (2,)) * 2).astype(np.float32)
    fp = (fg + rng.normal(size=SHAPE + (2,)) * 0.5).astype(np.float32)
    return sp, fp, sg, fg


class _StubModel:
    def __init__(self, outs):
        self.outs, self.k = outs, 0

    def simple_test(self, img_metas, img):
        self.k += 1
        return (None,) + self.outs[self.k - 1]


@pytest.mark.parametrize('dtypes', [(np.uint8, np.int64), (np.int64, np.uint8)])
def test_add_scored_end_to_end(dtypes, tmp_path):
    from occnet_amd.metrics import SubmissionScore, SubmissionWriter
    from occnet_amd.test_loop import run_test
    rng = np.random.default_rng(7)
    rays = rng.normal(size=(130, 3))
    rays = torch.from_numpy((rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32))
    counts, T, B = [3, 1, 2], 3, 3
    vox = rng.uniform([1, 1, 1], [SHAPE[0] - 1, SHAPE[1] - 1, SHAPE[2] - 1], size=(B, T, 3))
    origins = torch.tensor(np.asarray(PC_MIN) + vox * VOXEL, dtype=torch.float32)
    grids = [_grids(dtypes[0], dtypes[1], 40 + b) for b in range(B)]
    pc_range = list(PC_MIN) + [PC_MIN[k] + SHAPE[k] * VOXEL for k in range(3)]
    # the existing host route: the reference-pinned caster per origin, numpy look-up, numpy casts
    ref, want_rows = ssr.Ref(16), []
    for b, (sp, fp, sg, fg) in enumerate(grids):
        lp, rp = sref.rows(sp, fp, origins[b, :counts[b]], rays, PC_MIN, VOXEL)
        lg, rg = sref.rows(sg, fg, origins[b, :counts[b]], rays, PC_MIN, VOXEL)
        with np.errstate(over='ignore'):
            p, g = sref.pack(lp, rp), sref.pack(lg, rg)
        ref.add(p, g)
        want_rows.append(p)
    assert sum(ref.tp[0]) > 20 and sum(ref.ave_cnt[1]) > 0 and sum(ref.pred_cnt) < sum(ref.gt_cnt)
    dev = [tuple(torch.from_numpy(np.stack([g[k] for g in grids])).cuda() for k in range(4))]
    sp, fp, sg, fg = dev[0]
    tokens = ['a', 'b', 'c']
    score = SubmissionScore()
    scored = SubmissionWriter(pc_range, VOXEL, rays=rays)
    scored.add_scored(tokens, sp, fp, sg, fg, origins, score, origin_counts=counts)
    _equal(score.state, ref, 'add_scored')
    plain = SubmissionWriter(pc_range, VOXEL, rays=rays)
    plain.add(tokens, sp, fp, origins, origin_counts=counts)
    got, want = scored.results(), plain.results()
    assert list(got) == list(want) == tokens
    for b, tok in enumerate(tokens):
        for k, name in enumerate(('pcd_cls', 'pcd_dist', 'pcd_flow')):
            assert got[tok][name].dtype == want[tok][name].dtype and got[tok][name].tobytes() == want[tok][name].tobytes()
            assert got[tok][name].tobytes() == want_rows[b][k].tobytes()
    with pytest.raises(ValueError, match='free_id'):
        plain.add_scored(['z'], sp[:1], fp[:1], sg[:1], fg[:1], origins[:1], SubmissionScore(free_id=2))
    # the loop: sample by sample, a second batch into a slot already used; the same state, the same rows
    samples = [dict(token=tok, img_metas=None, img=None, lidar_origins=origins[b:b + 1, :counts[b]],
                    voxel_semantics=sg[b:b + 1] if b else sg[b:b + 1].cpu().numpy(), voxel_flow=fg[b:b + 1])
               for b, tok in enumerate(tokens)]
    loop_score, loop_writer = SubmissionScore(), SubmissionWriter(pc_range, VOXEL, rays=rays, depth=1)
    assert run_test(_StubModel([(sp[b:b + 1], fp[b:b + 1]) for b in range(B)]), samples, writer=loop_writer, score=loop_score) == 3
    assert torch.equal(loop_score.state, score.state)
    assert all(loop_writer.results()[t]['pcd_dist'].tobytes() == want[t]['pcd_dist'].tobytes() for t in tokens)
    with pytest.raises(ValueError, match='writer'):
        run_test(_StubModel([]), samples, metric=object(), score=loop_score)
    # the two files, scored as the server scores them
    gt_writer = SubmissionWriter(pc_range, VOXEL, rays=rays)          # the ground-truth rows file: a writer fed the ground truth
    gt_writer.add(tokens, sg, fg, origins, origin_counts=counts)
    pred_path = scored.write(str(tmp_path / 'pred'))
    gt_path = gt_writer.write(str(tmp_path / 'gt'))
    out = oio.score_submission(pred_path, gt_path)
    res = ref.compute()
    want_out = ssr.output(res['iou_list'], res['ave_fixed'])
    assert all(out[k] == want_out[k] for k in want_out) and np.isfinite(out['final_Occ_Score'])
    assert np.array_equal(np.stack(out['iou_list']), np.stack(res['iou_list']), equal_nan=True)
    assert np.array_equal(out['ave_list'], res['ave_fixed'], equal_nan=True)
    rel = np.abs(out['ave_list'] - res['ave_np']) / res['ave_np']
    assert (rel[~np.isnan(rel)] < 2e-6).all()


def test_score_submission_files_and_dicts(tmp_path):
    pred, gt = _edge_batch(16)
    ref = _ref(pred, gt, 16, (0, 0))
    names = ('pcd_cls', 'pcd_dist', 'pcd_flow')
    res_p = {f't{i}': dict(zip(names, s)) for i, s in enumerate(_as(pred, 0))}
    res_g = {f't{i}': dict(zip(names, s)) for i, s in enumerate(_as(gt, 0))}
    res_p['stranger'] = res_p['t2']                              # an extra prediction is ignored
    out = oio.score_submission(oio.write_submission(res_p, str(tmp_path / 'pred')),
                               oio.write_submission(res_g, str(tmp_path / 'gt')), batch=3)
    res = ref.compute()
    want = ssr.output(res['iou_list'], res['ave_fixed'])
    assert all(out[k] == want[k] for k in want)
    assert np.array_equal(np.stack(out['iou_list']), np.stack(res['iou_list']), equal_nan=True)
    assert np.array_equal(out['ave_list'], res['ave_fixed'], equal_nan=True)
    # result dicts instead of paths, bare or under 'results'; ground truth that is not in the file's types
    wide = {t: {'pcd_cls': r['pcd_cls'].astype(np.int64), 'pcd_dist': r['pcd_dist'].astype(np.float64),
                'pcd_flow': r['pcd_flow'].astype(np.float32)} for t, r in res_g.items()}
    again = oio.score_submission({'method': 'm', 'results': res_p}, wide)
    assert all(again[k] == want[k] for k in want)
    del res_p['t4']
    with pytest.raises(RuntimeError, match='t4'):
        oio.score_submission(res_p, res_g)
