"""-m gpu: the fused, device-resident RayIoU / mAVE evaluator (csrc/ray_metrics_fused.hip through occnet_amd.metrics.RayMetrics)
against the reference's own per-ray rows and scores (tests/golden/ray_metrics.npz), the CPU oracle (oracle/ray_metrics_ref.py
+ oracle/dvr_ref.c) and the numpy restatement of the accumulation (tests/ray_metrics_restate.py).

Bounds: per-ray rows and every integer counter bit for bit; IoU exactly; AVE within 2e-6 relative of the reference's float32
pairwise sums (derivation: tests/test_ray_metrics_device_host.py); each fixed-point sum within count * quantum / 2 of the
float64 sum of the same flow errors (round to nearest per term); OccScore within 1e-6."""
import os

import numpy as np
import pytest
import torch

from oracle import ray_metrics_ref as oref
from tests.golden_cases import METRIC_SEEDS, metric_scene
from tests.ray_metrics_restate import QUANTUM, ROWS, flow_errors, restate_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC_RANGE = [-40, -40, -1.0, 40, 40, 5.4]


def _lib_or_skip():
    try:
        oref.dvr_lib()
    except FileNotFoundError:
        pytest.skip("oracle/_build/libdvr_ref.so not built (make -C oracle)")


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'ray_metrics.npz')))


@pytest.fixture(scope='module')
def rays():
    from occnet_amd.metrics import generate_lidar_rays
    return torch.from_numpy(generate_lidar_rays())


def _metric(pc_range=PC_RANGE, voxel=0.4):
    from occnet_amd.metrics import RayMetrics
    return RayMetrics(pc_range, voxel)


def _dev(*arrays):
    return [torch.as_tensor(a).cuda() for a in arrays]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(t):
    """(B, T, R, 4) device rows of ONE sample -> (T * R, 4) numpy, process_one_sample's order."""
    assert t.shape[0] == 1
    return t[0].reshape(-1, 4).cpu().numpy()


def _state(m):
    return m.state.cpu().numpy()


def _check_ave_sums(state, pairs):
    """each fixed-point sum vs the float64 sum of the same rows' flow errors: within count * quantum / 2"""
    s = state.reshape(ROWS, -1)
    for j, thr in enumerate((1, 2, 4)):
        want = np.zeros(8)
        for p, g in pairs:
            v = g[:, 0].astype(np.int32) != 16
            p, g = p[v], g[v]
            tp = (p[:, 0] == g[:, 0]) & (np.abs(p[:, 1] - g[:, 1]) < thr)
            err = flow_errors(p, g).astype(np.float64)
            for c in range(8):
                want[c] += err[tp & (g[:, 0] == c)].sum()
        got = s[8 + j][:8].astype(np.float64) * QUANTUM
        bound = s[5 + j][:8] * QUANTUM / 2
        print(f'thr {thr} m: |fixed-point sum - float64 sum| max {np.abs(got - want).max():.3e}, bound max {bound.max():.3e}')
        assert (np.abs(got - want) <= bound + 1e-12 * np.abs(want)).all(), (j, got - want, bound)


def test_golden_scenes_rows_counters_and_scores(gold):
    m = _metric()
    want_state = 0
    pairs = []
    for i, seed in enumerate(METRIC_SEEDS):
        sp, sg, fp, fg, org = metric_scene(seed)
        rp, rg = m.update(*_dev(sp, fp, sg, fg, org), return_rays=True)
        rp, rg = _rows(rp), _rows(rg)
        for nm, got in (('pcd_pred', rp), ('pcd_gt', rg)):
            want = gold[f'{nm}_{i}']
            neq = int((_bits(got) != _bits(want)).any(axis=1).sum())
            print(f'scene {seed} {nm}: {neq} of {want.shape[0]} rows differ')
            assert got.shape == want.shape and neq == 0, (nm, i, neq)
        want_state = want_state + restate_state(gold[f'pcd_pred_{i}'], gold[f'pcd_gt_{i}'])
        pairs.append((gold[f'pcd_pred_{i}'], gold[f'pcd_gt_{i}']))
    state = _state(m)
    assert np.array_equal(state, want_state), np.nonzero(state != want_state)
    res = m.compute()
    assert np.array_equal(np.stack(res['iou_list']), gold['iou'], equal_nan=True)
    ave, want = np.asarray(res['ave_list']), gold['ave']
    assert np.array_equal(np.isnan(ave), np.isnan(want))
    ok = ~np.isnan(want)
    rel = np.abs(ave[ok] - want[ok]) / np.abs(want[ok])
    print('AVE relative difference to the reference:', rel.max())
    assert rel.max() <= 2e-6
    _check_ave_sums(state, pairs)
    print('occ_score', res['occ_score'], 'reference', float(gold['occ_score']))
    assert abs(res['occ_score'] - float(gold['occ_score'])) < 1e-6


def test_main_device_matches_reference_golden(gold):
    from occnet_amd.metrics import main_device
    scenes = [metric_scene(s) for s in METRIC_SEEDS]
    res = main_device([s[0].reshape(-1) for s in scenes], [s[1].reshape(-1) for s in scenes],
                      [s[2].reshape(-1) for s in scenes], [s[3].reshape(-1) for s in scenes], [s[4] for s in scenes],
                      verbose=False)
    assert np.array_equal(np.stack(res['iou_list']), gold['iou'], equal_nan=True)
    assert res['miou'] == float(gold['miou'])
    assert abs(res['occ_score'] - float(gold['occ_score'])) < 1e-6


def test_skipped_prediction_casts_change_nothing():
    a, b = _metric(), _metric()
    for seed in METRIC_SEEDS:
        sp, sg, fp, fg, org = metric_scene(seed)
        args = _dev(sp, fp, sg, fg, org)
        assert a.update(*args) is None
        b.update(*args, return_rays=True)
    assert int(_state(a)[:17].sum()) > 0
    assert np.array_equal(_state(a), _state(b))


def _noisy_scene():
    """the scene of tests/test_gpu_dvr.py::test_process_one_sample_and_score_match_oracle"""
    rng = np.random.default_rng(3)
    sem_gt = np.full((200, 200, 16), 16, dtype=np.uint8)
    sem_gt[:, :, :2] = rng.integers(10, 14, (200, 200, 2))
    boxes = rng.integers(0, 180, (60, 2))
    for i, (x, y) in enumerate(boxes):
        sem_gt[x:x + 8, y:y + 5, 2:6] = i % 10
    sem_pred = sem_gt.copy()
    noise = rng.random(sem_gt.shape) < 0.02
    sem_pred[noise] = rng.integers(0, 17, int(noise.sum()))
    flow_gt = rng.normal(size=(200, 200, 16, 2)).astype(np.float32)
    flow_pred = flow_gt + rng.normal(scale=0.2, size=flow_gt.shape).astype(np.float32)
    origins = torch.tensor([[[0.98, 0.0, 1.84], [3.0, -1.5, 1.9]]])
    return sem_pred, sem_gt, flow_pred, flow_gt, origins


def _check_against_oracle(m, sp, sg, fp, fg, org, rays):
    """rows, state and scores of one sample against oref.process_one_sample + oref.calc_metrics"""
    before = _state(m).copy()
    rp, rg = m.update(*_dev(sp, fp, sg, fg, org), return_rays=True)
    op = oref.process_one_sample(sp, rays, org, fp)
    og = oref.process_one_sample(sg, rays, org, fg)
    for nm, got, want in (('pred', _rows(rp), op), ('gt', _rows(rg), og)):
        neq = int((_bits(got) != _bits(want)).any(axis=1).sum())
        print(f'{nm}: {neq} of {want.shape[0]} rows differ from the oracle')
        assert got.shape == want.shape and neq == 0, (nm, neq)
    assert np.array_equal(_state(m) - before, restate_state(op, og))
    return op, og


def test_noisy_scene_matches_oracle(rays):
    _lib_or_skip()
    sp, sg, fp, fg, org = _noisy_scene()
    m = _metric()
    op, og = _check_against_oracle(m, sp, sg, fp, fg, org, rays)
    valid = og[:, 0].astype(np.int32) != 16
    iou, ave = oref.calc_metrics([op[valid]], [og[valid]])
    res = m.compute()
    assert np.array_equal(np.stack(res['iou_list']), np.stack(iou), equal_nan=True)
    ave_got = np.asarray(res['ave_list'])
    assert np.array_equal(np.isnan(ave_got), np.isnan(ave))
    ok = ~np.isnan(ave)
    rel = np.abs(ave_got[ok] - ave[ok]) / np.abs(ave[ok])
    print('AVE relative difference to the oracle:', rel.max())
    assert rel.max() <= 2e-6
    _check_ave_sums(_state(m), [(op, og)])
    miou, mave = float(np.nanmean(iou)), float(np.nanmean(ave))
    assert abs(res['occ_score'] - (miou * 0.9 + max(1 - mave, 0.0) * 0.1)) < 1e-6


def test_batching_and_determinism():
    s0, s1 = metric_scene(METRIC_SEEDS[0]), _noisy_scene()
    o0 = s0[4][:, :1]                                                    # 1 origin
    o1 = torch.cat([s1[4], torch.tensor([[[-2.0, 4.0, 1.7]]])], 1)       # 3 origins
    singles = []
    for order in ((0, 1), (1, 0)):
        m = _metric()
        for k in order:
            sp, sg, fp, fg, _ = (s0, s1)[k]
            m.update(*_dev(sp, fp, sg, fg, (o0, o1)[k]))
        singles.append(_state(m))
    assert np.array_equal(singles[0], singles[1])
    origins = torch.zeros(2, 3, 3)
    origins[0, :1] = o0[0]
    origins[0, 1:] = 1e3                                                 # must not be cast: beyond origin_counts[0]
    origins[1] = o1[0]
    counts = torch.tensor([1, 3], dtype=torch.int32).cuda()
    batch = [torch.as_tensor(np.stack([a, b])).cuda() for a, b in zip(s0[:4], s1[:4])]
    runs = []
    for _ in range(2):
        m = _metric()
        rows = m.update(batch[0], batch[2], batch[1], batch[3], origins.cuda(), return_rays=True, origin_counts=counts)
        runs.append(_state(m))
        assert rows[0].shape == (2, 3, 14040, 4) and float(rows[0][0, 1:].abs().sum()) == 0.0
    assert np.array_equal(runs[0], runs[1])
    assert np.array_equal(runs[0], singles[0])
    m = _metric()
    m.update(batch[0], batch[2], batch[1], batch[3], origins.cuda(), origin_counts=counts)
    assert np.array_equal(_state(m), singles[0])


def test_input_types_and_class_above_free(rays):
    _lib_or_skip()
    sp, sg, fp, fg, org = _noisy_scene()
    sp, sg = sp.copy(), sg.copy()
    sp[100:104, 90:110, 2:5] = 17                                        # occupied, counted in no class
    sg[80:84, 90:110, 2:5] = 17
    states = []
    for tp, tg in ((np.uint8, np.uint8), (np.int64, np.uint8), (np.int64, np.int64)):
        m = _metric()
        m.update(*_dev(sp.astype(tp), fp, sg.astype(tg), fg, org))
        states.append(_state(m))
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[0], states[2])
    m = _metric()
    op, og = _check_against_oracle(m, sp, sg, fp, fg, org, rays)
    assert (op[:, 0] == 17).any() and (og[:, 0] == 17).any()
    assert np.array_equal(_state(m), states[0])


def test_origin_outside_small_grid(rays, monkeypatch):
    _lib_or_skip()
    pc_range = [-10.0, -8.0, -1.0, 10.0, 8.0, 0.6]                       # 50 x 40 x 4 voxels of 0.4 m
    monkeypatch.setattr(oref, '_pc_range', pc_range)
    rng = np.random.default_rng(7)
    sg = np.full((50, 40, 4), 16, np.uint8)
    sg[:, :, 0] = 10
    sg[rng.random(sg.shape) < 0.05] = 3
    sg[0, 0, 0] = 5                                                      # the voxel a ray that never enters reports
    sp = sg.copy()
    flip = rng.random(sg.shape) < 0.05
    sp[flip] = rng.integers(0, 17, int(flip.sum()))
    fg = rng.normal(size=(50, 40, 4, 2)).astype(np.float32)
    fp = fg + rng.normal(scale=0.3, size=fg.shape).astype(np.float32)
    org = torch.tensor([[[14.0, 3.0, 1.84], [-12.5, -9.0, -2.0], [0.3, 0.2, 0.1]]])   # two outside, one inside
    m = _metric(pc_range, 0.4)
    assert m.occ_size == [50, 40, 4]
    op, og = _check_against_oracle(m, sp, sg, fp, fg, org, rays)
    never = int((og[:, 1] < 0).sum())
    print('rays that never enter the grid:', never)
    assert never > 1000 and int(_state(m)[5]) > 0


def test_hires_grid_rows(rays, monkeypatch):
    _lib_or_skip()
    monkeypatch.setattr(oref, '_voxel_size', 0.2)
    rng = np.random.default_rng(11)
    shape = (400, 400, 32)
    sg = np.full(shape, 16, np.uint8)
    occ = rng.random(shape) < 0.002
    sg[occ] = rng.integers(0, 16, int(occ.sum()))
    sg[:, :, 0] = 10
    sp = np.full(shape, 16, np.uint8)
    occ = rng.random(shape) < 0.002
    sp[occ] = rng.integers(0, 16, int(occ.sum()))
    sp[:, :, 0] = 10
    fg = rng.normal(size=shape + (2,)).astype(np.float32)
    fp = rng.normal(size=shape + (2,)).astype(np.float32)
    org = torch.tensor([[[0.9858, 0.0, 1.8402]]])
    m = _metric(PC_RANGE, 0.2)
    assert m.occ_size == [400, 400, 32]
    _check_against_oracle(m, sp, sg, fp, fg, org, rays)


def test_unsupported_depth():
    from occnet_amd._lib import OccAmdUnsupported
    m = _metric([-40, -40, -1.0, 40, 40, 12.2], 0.4)
    assert m.occ_size == [200, 200, 33]
    sem = torch.full((1, 200, 200, 33), 16, dtype=torch.uint8).cuda()
    flow = torch.zeros(1, 200, 200, 33, 2).cuda()
    with pytest.raises(OccAmdUnsupported):
        m.update(sem, flow, sem, flow, torch.zeros(1, 1, 3).cuda())
    assert int(m.state.abs().sum()) == 0


def test_non_finite_flow_flags_only_its_class(gold, rays):
    _lib_or_skip()
    k = 1                                          # the golden scene that has true positives of class 0 (car)
    sp, sg, fp, fg, org = metric_scene(METRIC_SEEDS[k])
    clean = _metric()
    clean.update(*_dev(sp, fp, sg, fg, org))
    # which voxel does each prediction ray report?  cast the oracle with the voxel index in the flow channel
    marker = np.zeros_like(fp)
    marker[..., 0] = np.arange(sp.size, dtype=np.float32).reshape(sp.shape)
    vox = oref.process_one_sample(sp, rays, org, marker)[:, 2].astype(np.int64)
    p, g = gold[f'pcd_pred_{k}'], gold[f'pcd_gt_{k}']
    tp = (p[:, 0] == 0) & (g[:, 0] == 0) & (np.abs(p[:, 1] - g[:, 1]) < 1)
    assert tp.any()
    target = int(vox[np.nonzero(tp)[0][0]])
    fp_bad = fp.copy()
    fp_bad.reshape(-1, 2)[target, 0] = np.nan
    m = _metric()
    op, og = _check_against_oracle(m, sp, sg, fp_bad, fg, org, rays)
    s, c = _state(m).reshape(ROWS, 17), _state(clean).reshape(ROWS, 17)
    assert np.array_equal(s[:8], c[:8])                                  # every counter
    assert np.array_equal(s[8:11, 1:], c[8:11, 1:]) and np.array_equal(s[11:, 1:], c[11:, 1:])
    assert (s[11:, 0] > 0).all() and (c[11:] == 0).all()
    assert (s[8:11, 0] < c[8:11, 0]).all()
    res, ref = m.compute(), clean.compute()
    assert np.isnan(res['ave_list'][0]) and not np.isnan(ref['ave_list'][0])
    assert np.array_equal(res['ave_list'][1:], ref['ave_list'][1:], equal_nan=True)
    assert np.array_equal(np.stack(res['iou_list']), np.stack(ref['iou_list']), equal_nan=True)
