"""not-gpu: the server-side scorer's host side — the numpy restatement (tests/submission_score_ref.py) against the numbers the
reference's own tools/ray_iou/metric.py left in tests/golden/ray_metrics.npz, the rounding path of the file's types, every
argument check of occ_submission_score_accumulate through the C ABI (each returns its code before any launch: this machine may
have no GPU at all), SubmissionScore.compute() on hand-written states and update_results' token rules."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from occnet_amd import _lib
from tests import submission_score_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ray_metrics.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _scenes(gold):
    n = sum(1 for k in gold if k.startswith('pcd_pred_'))
    return [(gold[f'pcd_pred_{i}'], gold[f'pcd_gt_{i}']) for i in range(n)]


def test_restatement_equals_metric_py_on_golden_rows(gold):
    ref = ssr.Ref(16)
    for p, g in _scenes(gold):
        ref.add(ssr.split_rows(p), ssr.split_rows(g))
    res = ref.compute()
    assert np.array_equal(np.stack(res['iou_list']), gold['metric_py_iou'], equal_nan=True)
    want = gold['metric_py_ave']
    assert np.array_equal(np.isnan(res['ave_np']), np.isnan(want)) and (~np.isnan(want)).sum() >= 2
    ok = ~np.isnan(want)
    # metric.py adds float32 errors with numpy's pairwise sum: leaves of 128 in 8 accumulators, about 26 roundings for
    # n ~ 14 000 -> 26 * 2^-24 ~ 1.6e-6 relative
    for name in ('ave_np', 'ave_f64', 'ave_fixed'):
        rel = np.abs(res[name][ok] - want[ok]) / want[ok]
        print(name, 'max relative difference to metric_py_ave', rel.max())
        assert (rel < 2e-6).all(), (name, rel)
    rel = np.abs(res['ave_fixed'][ok] - res['ave_f64'][ok]) / res['ave_f64'][ok]
    print('fixed point against float64', rel.max())
    assert (rel < 1e-12).all()
    assert not any(v for row in ref.ave_inf + ref.ave_nan for v in row)
    # the AVE rule: every valid ray of a sample counts once the class has a true positive there
    assert max(ref.ave_cnt[1]) > max(ref.tp[1][:8])


def test_rounding_path_is_live(gold):
    """the same rows through astype(int8 / float16), as the file holds them, move rays across a depth threshold"""
    as_float, as_file = ssr.Ref(16), ssr.Ref(16)
    for p, g in _scenes(gold):
        as_float.add(ssr.split_rows(p), ssr.split_rows(g))
        as_file.add(ssr.pack_rows(p), ssr.pack_rows(g))
    assert as_float.gt_cnt == as_file.gt_cnt and as_float.pred_cnt == as_file.pred_cnt       # classes 0..16 survive int8
    moved = sum(abs(a - b) for ra, rb in zip(as_float.tp, as_file.tp) for a, b in zip(ra, rb))
    print('true positives moved by the rounding:', moved)
    assert as_float.tp != as_file.tp and moved > 0
    assert not np.array_equal(as_float.words(), as_file.words())


def _lib64():
    lib = _lib.lib()
    return lib


def test_symbols_and_size_queries():
    lib = _lib64()
    declared = _lib.declared_symbols()
    for name in ('occ_submission_score_accumulate', 'occ_submission_score_state_words',
                 'occ_submission_score_workspace_bytes'):
        assert name in declared and hasattr(lib, name), name
    assert lib.occ_abi_version() == _lib.ABI == 3                  # entries were added, no signature changed
    assert lib.occ_submission_score_state_words(16) == 17 * 17
    assert lib.occ_submission_score_state_words(2) == 17 * 3 and lib.occ_submission_score_state_words(31) == 17 * 32
    assert lib.occ_submission_score_state_words(0) == 0 and lib.occ_submission_score_state_words(32) == 0
    assert lib.occ_submission_score_workspace_bytes(0) == 0 and lib.occ_submission_score_workspace_bytes(-1) == 0
    one = lib.occ_submission_score_workspace_bytes(1)
    assert one >= (5 * 32 + 4) * 8 and one % 256 == 0 and lib.occ_submission_score_workspace_bytes(8) == 8 * one


def test_argument_checks_without_gpu():
    lib = _lib64()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    i64 = ctypes.c_int64

    def call(pf=0, pc=p, pd=p, pfl=p, gf=0, gc=p, gd=p, gfl=p, counts=p, free_id=16, state=p, ws=p, ws_bytes=1 << 30, B=1,
             stride=8, max_chunks=0):
        return lib.occ_submission_score_accumulate(pf, pc, pd, pfl, gf, gc, gd, gfl, counts, free_id, state, ws, i64(ws_bytes),
                                                   B, i64(stride), max_chunks, null)

    for name in ('pc', 'pd', 'pfl', 'gc', 'gd', 'gfl', 'counts', 'state', 'ws'):
        assert call(**{name: null}) == -1 and b'null' in lib.occ_last_error(), name
    for name in ('pc', 'gc'):                                      # float32 rows: the section pointers are not needed ...
        assert call(pf=1, gf=1, **{name: null}) == -1 and b'null' in lib.occ_last_error(), name
    for fmt in (-1, 2, 7):
        assert call(pf=fmt) == -1 and b'format' in lib.occ_last_error()
        assert call(gf=fmt) == -1 and b'format' in lib.occ_last_error()
    for free_id in (0, -1, 32, 200):
        assert call(free_id=free_id) == -1 and b'1..31' in lib.occ_last_error(), free_id
    for B in (0, -3, 65536):
        assert call(B=B) == -1 and b'dimension' in lib.occ_last_error(), B
    assert call(stride=0) == -1 and b'dimension' in lib.occ_last_error()
    assert call(max_chunks=-1) == -1 and b'max_chunks' in lib.occ_last_error()
    need = lib.occ_submission_score_workspace_bytes(1)
    assert call(ws_bytes=need - 1) == -1 and b'workspace too small' in lib.occ_last_error()
    odd = ctypes.c_void_p(p.value + 1)
    for kw in (dict(pd=odd), dict(gfl=ctypes.c_void_p(p.value + 2)), dict(pf=1, pc=ctypes.c_void_p(p.value + 4)),
               dict(state=odd), dict(ws=odd)):
        assert call(**kw) == -1 and b'aligned' in lib.occ_last_error(), kw


def test_ext_refuses_host_tensors():
    from occnet_amd import ext
    assert ext.submission_score_state_words(16) == 289
    with pytest.raises(_lib.OccAmdError, match='free_id'):
        ext.submission_score_state_words(32)
    state = torch.zeros(289, dtype=torch.int64)
    rows = torch.zeros(1, 4, 4)
    with pytest.raises(_lib.OccAmdError, match='counts'):
        ext.submission_score_accumulate(state, rows, rows, torch.tensor([4], dtype=torch.int32), 4)


def _state(ncls, **rows):
    s = np.zeros((17, ncls), np.int64)
    for name, v in rows.items():
        s[int(name[1:])] = v
    return torch.from_numpy(s.reshape(-1))


def test_compute_on_hand_written_state():
    from occnet_amd.metrics import SubmissionScore
    m = SubmissionScore(free_id=2, device='cpu')
    assert m.state.numel() == 17 * 3 and m.ncls == 3
    # classes 0, 1 and free; thresholds 1 / 2 / 4
    m.state = _state(3, r0=[10, 6, 0], r1=[8, 8, 0], r2=[2, 0, 0], r3=[4, 3, 0], r4=[8, 6, 0],
                     r5=[16, 0, 0], r6=[32, 16, 0], r7=[48, 16, 0],
                     r8=[3 << 28, 0, 0], r9=[(8 << 28) + (1 << 27), 4 << 28, 0], r10=[1, 1, 0])
    out = m.compute()
    assert sorted(out) == sorted(['RayIoU@1', 'RayIoU@2', 'RayIoU@4', 'RayIoU', 'mAVE', 'final_Occ_Score', 'iou_list',
                                  'ave_list'])
    iou = [np.array([2 / 16, 0 / 14]), np.array([4 / 14, 3 / 11]), np.array([8 / 10, 6 / 8])]
    for j in range(3):
        assert out['iou_list'][j].shape == (2,) and np.array_equal(out['iou_list'][j], iou[j])
    assert np.array_equal(out['ave_list'], np.array([8.5 / 32, 4 / 16]))                 # threshold 2 m only
    assert out['RayIoU@1'] == np.mean(iou[0]) and out['RayIoU@2'] == np.mean(iou[1]) and out['RayIoU@4'] == np.mean(iou[2])
    assert out['RayIoU'] == np.mean(iou) and out['mAVE'] == np.mean([8.5 / 32, 0.25])
    assert out['final_Occ_Score'] == out['RayIoU'] * 0.9 + (1 - out['mAVE']) * 0.1
    want = ssr.output(iou, np.array([8.5 / 32, 0.25]))
    assert all(out[k] == want[k] for k in want)
    # an infinite error makes the class's AVE inf, a NaN one NaN (also next to an infinite one); the score's AVE term is then 0
    m.state[12 * 3 + 1] = 1
    out = m.compute()
    assert out['ave_list'][1] == np.inf and out['mAVE'] == np.inf and out['final_Occ_Score'] == out['RayIoU'] * 0.9
    m.state[15 * 3 + 1] = 2
    out = m.compute()
    assert np.isnan(out['ave_list'][1]) and out['ave_list'][0] == 8.5 / 32 and out['mAVE'] == 8.5 / 32
    # the words of the other thresholds do not reach the AVE
    m.state[11 * 3 + 0] = m.state[16 * 3 + 0] = 5
    assert m.compute()['ave_list'][0] == 8.5 / 32
    # seventeen classes: AVE is NaN beyond the eight flow classes, whatever the words say
    m = SubmissionScore(device='cpu')
    s = np.zeros((17, 17), np.int64)
    s[0], s[1], s[3], s[6], s[9] = 4, 4, 2, 10, 5 << 28
    m.state = torch.from_numpy(s.reshape(-1))
    out = m.compute()
    assert out['ave_list'].shape == (16,) and np.array_equal(out['ave_list'][:8], np.full(8, 0.5))
    assert np.isnan(out['ave_list'][8:]).all() and out['mAVE'] == 0.5
    assert np.array_equal(out['iou_list'][1], np.full(16, 2 / 6)) and np.isnan(out['iou_list'][0]).sum() == 0


def test_empty_state_gives_nans_without_warning():
    from occnet_amd.metrics import SubmissionScore
    m = SubmissionScore(device='cpu')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        out = m.compute()
    for k in ('RayIoU@1', 'RayIoU@2', 'RayIoU@4', 'RayIoU', 'mAVE', 'final_Occ_Score'):
        assert np.isnan(out[k]), k
    assert all(np.isnan(a).all() and a.shape == (16,) for a in out['iou_list']) and np.isnan(out['ave_list']).all()
    assert m.reset() is m and m.merge(SubmissionScore(device='cpu')) is m and m.all_reduce() is m
    with pytest.raises(ValueError):
        m.merge(SubmissionScore(free_id=2, device='cpu'))
    with pytest.raises(ValueError):
        SubmissionScore(free_id=32, device='cpu')


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    return {'pcd_cls': rng.integers(0, 17, n).astype(np.int8), 'pcd_dist': rng.uniform(0, 50, n).astype(np.float16),
            'pcd_flow': rng.normal(size=(n, 2)).astype(np.float16)}


class _Recorder:
    """a SubmissionScore whose device step only records what update_results hands it"""

    def __init__(self):
        from occnet_amd.metrics import SubmissionScore
        self.m = SubmissionScore(device='cpu')
        self.calls = []
        self.m._accumulate = lambda pred, gt, counts, stride, max_chunks=0: self.calls.append((pred, gt, counts, stride))


def test_update_results_tokens_and_batches():
    gt = {f't{i}': _rows(5 + i, i) for i in range(5)}
    pred = {f't{i}': _rows(5 + i, 10 + i) for i in range(5)}
    missing = {k: v for k, v in pred.items() if k != 't3'}
    r = _Recorder()
    with pytest.raises(RuntimeError, match='t3'):
        r.m.update_results(missing, gt)
    assert not r.calls                                             # refused before anything was enqueued
    extra = dict(pred, stranger=_rows(4, 99))
    assert r.m.update_results(extra, gt, batch=2) == 5             # an extra prediction is ignored
    assert [int(c[2].numel()) for c in r.calls] == [2, 2, 1] and [c[3] for c in r.calls] == [6, 8, 9]
    assert [c[2].tolist() for c in r.calls] == [[5, 6], [7, 8], [9]]
    p0, g0 = r.calls[0][0], r.calls[0][1]
    assert isinstance(p0, tuple) and p0[0].dtype == torch.int8 and p0[1].dtype == torch.float16 and tuple(p0[2].shape) == (2, 6, 2)
    assert np.array_equal(p0[0][1].numpy(), pred['t1']['pcd_cls']) and np.array_equal(g0[1][0, :5].numpy(), gt['t0']['pcd_dist'])
    assert int(p0[0][0, 5]) == 0                                   # the padding row of the shorter sample
    # rows that are not in the file's types travel as float32 rows, cast as metric.py casts them
    wide = {k: {'pcd_cls': v['pcd_cls'].astype(np.int64), 'pcd_dist': v['pcd_dist'].astype(np.float64),
                'pcd_flow': v['pcd_flow'].astype(np.float32)} for k, v in gt.items()}
    r = _Recorder()
    r.m.update_results(pred, wide, batch=8)
    (p, g, counts, stride), = r.calls
    assert isinstance(p, tuple) and g.dtype == torch.float32 and tuple(g.shape) == (5, 9, 4) and stride == 9
    assert np.array_equal(g[2, :7, 0].numpy(), gt['t2']['pcd_cls'].astype(np.float32))
    assert np.array_equal(g[2, :7, 1].numpy(), gt['t2']['pcd_dist'].astype(np.float32))
    short = dict(pred, t1=_rows(3, 5))
    with pytest.raises(ValueError, match='t1'):
        _Recorder().m.update_results(short, gt)
