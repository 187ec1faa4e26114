"""not-gpu: the device-resident RayIoU evaluator's host side — C-ABI symbols and argument checks, and RayMetrics.compute() /
merge(), which are pure host arithmetic, on a state rebuilt in numpy from the reference's own per-ray rows
(tests/golden/ray_metrics.npz).

The AVE bound (2e-6 relative): the reference sums float32 flow errors with numpy's pairwise np.sum, whose worst-case
relative error for n <= 112 320 non-negative terms is about (19 + log2(n / 128)) * 2^-24 = 1.7e-6; the fixed-point sum is
exact to n * 2^-29 m/s, far below it."""
import ctypes
import os

import numpy as np
import pytest
import torch

from occnet_amd import _lib
from occnet_amd.metrics import RayMetrics
from tests.golden_cases import METRIC_SEEDS
from tests.ray_metrics_restate import QUANTUM, ROWS, restate_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC_RANGE = [-40, -40, -1.0, 40, 40, 5.4]


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'ray_metrics.npz')))


def test_symbols_declared_and_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ('occ_ray_metrics_accumulate', 'occ_ray_metrics_state_words', 'occ_ray_metrics_workspace_bytes'):
        assert name in declared and hasattr(lib, name), name
    assert lib.occ_abi_version() == _lib.ABI == 3
    assert lib.occ_ray_metrics_state_words(16) == ROWS * 17
    assert lib.occ_ray_metrics_state_words(0) == 0 and lib.occ_ray_metrics_state_words(32) == 0
    assert lib.occ_ray_metrics_workspace_bytes(1, 200, 200, 16) == 2 * 200 * 200 * 2          # uint16 masks, both grids
    assert lib.occ_ray_metrics_workspace_bytes(2, 400, 400, 32) == 2 * 2 * 400 * 400 * 4      # uint32 masks
    assert lib.occ_ray_metrics_workspace_bytes(1, 50, 40, 4) == (2 * 50 * 40 * 2 + 255) // 256 * 256
    assert lib.occ_ray_metrics_workspace_bytes(1, 200, 200, 33) == 0


def test_argument_checks_without_gpu():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f, i64 = ctypes.c_float, ctypes.c_int64

    def call(sem_pred=p, dt_pred=0, dt_gt=1, state=p, rows_pred=null, rows_gt=null, ws=p, ws_bytes=1 << 20, B=1, T=2, X=4,
             Y=4, Z=4, R=8, free_id=16, voxel=0.4, origins=p):
        return lib.occ_ray_metrics_accumulate(sem_pred, dt_pred, p, p, dt_gt, p, origins, null, p, f(-40.0), f(-40.0),
                                              f(-1.0), f(voxel), free_id, state, rows_pred, rows_gt, ws, i64(ws_bytes),
                                              B, T, X, Y, Z, R, null)

    assert call(sem_pred=null) == -1 and b'null' in lib.occ_last_error()
    assert call(state=null) == -1 and call(ws=null) == -1 and call(origins=null) == -1
    assert call(rows_pred=p) == -1 and b'together' in lib.occ_last_error()
    assert call(B=0) == -1 and call(X=0) == -1 and call(R=0) == -1 and b'dimension' in lib.occ_last_error()
    assert call(Z=33) == -3 and b'Z = 33' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'ray_metrics_accumulate')
    assert call(T=0) == -1 and call(T=9) == -1 and b'1..8' in lib.occ_last_error()
    assert call(dt_pred=2) == -1 and call(dt_gt=-1) == -1 and b'dtype' in lib.occ_last_error()
    assert call(free_id=0) == -1 and call(free_id=32) == -1
    assert call(voxel=0.0) == -1
    assert call(ws_bytes=16) == -1 and b'workspace too small' in lib.occ_last_error()


def _gold_states(gold):
    return [restate_state(gold[f'pcd_pred_{i}'], gold[f'pcd_gt_{i}']) for i in range(len(METRIC_SEEDS))]


def _metric(state):
    m = RayMetrics(PC_RANGE, 0.4, device='cpu')
    assert m.state.shape == state.shape and m.state.dtype == torch.int64 and m.occ_size == [200, 200, 16]
    m.state += torch.from_numpy(state)
    return m


def test_compute_reproduces_reference_scores(gold):
    res = _metric(sum(_gold_states(gold))).compute()
    assert np.array_equal(np.stack(res['iou_list']), gold['iou'], equal_nan=True)
    ave, want = np.asarray(res['ave_list']), gold['ave']
    assert ave.shape == want.shape and np.array_equal(np.isnan(ave), np.isnan(want))
    ok = ~np.isnan(want)
    rel = np.abs(ave[ok] - want[ok]) / np.abs(want[ok])
    print('AVE relative difference to the reference:', rel.max())
    assert rel.max() <= 2e-6
    assert res['miou'] == float(gold['miou'])
    assert abs(res['mave'] - float(gold['mave'])) <= 2e-6 * float(gold['mave'])
    assert abs(res['occ_score'] - float(gold['occ_score'])) < 1e-6


def test_merge_equals_concatenated_input(gold):
    a, b = _gold_states(gold)
    both = restate_state(np.concatenate([gold['pcd_pred_0'], gold['pcd_pred_1']]),
                         np.concatenate([gold['pcd_gt_0'], gold['pcd_gt_1']]))
    assert np.array_equal(a + b, both)
    for first, second in ((a, b), (b, a)):
        m = _metric(first).merge(_metric(second))
        assert np.array_equal(m.state.numpy(), both)
    m.reset()
    assert int(m.state.abs().sum()) == 0
    assert np.isnan(m.compute()['miou'])


def test_non_finite_flow_error_flags_its_class():
    """A non-finite flow error never enters the fixed-point sum: it is counted in ave_bad and the class reports NaN."""
    pred = np.array([[0, 10.0, np.nan, 0.0], [0, 10.0, 1.0, 0.0], [1, 5.0, 0.5, 0.0]], np.float32)
    gt = np.array([[0, 10.5, 0.0, 0.0], [0, 10.5, 0.0, 0.0], [1, 5.0, 0.0, 0.0]], np.float32)
    s = restate_state(pred, gt).reshape(ROWS, 17)
    assert s[6][0] == 2 and s[12][0] == 1 and s[9][0] == round(1.0 / QUANTUM) and s[9][1] == round(0.5 / QUANTUM)
    res = _metric(s.reshape(-1)).compute()
    assert np.isnan(res['ave_list'][0]) and res['ave_list'][1] == 0.5
    assert res['iou_list'][0][0] == 1.0


def test_update_refuses_host_tensors():
    m = RayMetrics(PC_RANGE, 0.4, device='cpu')
    sem = np.full((200, 200, 16), 16, np.uint8)
    flow = np.zeros((200, 200, 16, 2), np.float32)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        m.update(sem, flow, sem, flow, torch.zeros(1, 1, 3))
