"""RayIoU / mAVE / OccScore pinned to the reference (VERDICT r1 missing #4).

tests/golden/ray_metrics.npz was written by oracle/gen_golden.py running the reference's OWN
projects/mmdet3d_plugin/datasets/ray_metrics.py (process_one_sample :89-143, calc_metrics :146-197, main :200-257)
and tools/ray_iou/metric.py (calc_metrics :6-81) in place, on the seeded scenes of tests/golden_cases.metric_scene,
with the reference's ray-casting kernel body (dvr.cu:69-319) compiled for the host (oracle/build_ref.py).
Checked against it:
  not gpu   oracle/ray_metrics_ref.py (the restatement) + oracle/dvr_ref.c (plain-C ray caster): bit-exact rays,
            identical scores;  occnet_amd.metrics.calc_metrics (vectorised product mirror): identical scores;
            oracle/dvr_ref.c vs the reference kernel on random / adversarial rays (its results stored in
            tests/golden/dvr_reference_kernel.npz; live as well where oracle/_ref is built);
  gpu       the HIP pipeline (occ_dvr_render_forward_f32 + occnet_amd.metrics) end to end: bit-exact rays, same score.
"""
import os

import numpy as np
import pytest
import torch

from tests.golden_cases import DVR_FIELDS, DVR_KERNEL_CASES, METRIC_SEEDS, metric_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ray_metrics.npz')
DVR_GOLD = os.path.join(ROOT, 'tests', 'golden', 'dvr_reference_kernel.npz')
REF_SO = os.path.join(ROOT, 'oracle', '_ref', 'libdvr_reference.so')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _valid_lists(pcd_pred, pcd_gt):
    valid = [g[:, 0].astype(np.int32) != 16 for g in pcd_gt]
    return [p[v] for p, v in zip(pcd_pred, valid)], [g[v] for g, v in zip(pcd_gt, valid)]


def _check_scores(gold, iou_list, ave_list):
    assert np.array_equal(np.stack(iou_list), gold['iou'], equal_nan=True)
    assert np.array_equal(np.asarray(ave_list), gold['ave'], equal_nan=True)
    miou, mave = np.nanmean(iou_list), np.nanmean(ave_list)
    assert miou == gold['miou'] and mave == gold['mave']
    assert abs(miou * 0.9 + max(1 - mave, 0.0) * 0.1 - gold['occ_score']) < 1e-12     # ray_metrics.py:253


def test_oracle_pipeline_matches_reference_golden(gold):
    from oracle import ray_metrics_ref as oref
    try:
        oref.dvr_lib()
    except FileNotFoundError:
        pytest.skip("oracle/_build/libdvr_ref.so not built (make -C oracle)")
    from occnet_amd.metrics import generate_lidar_rays
    rays = torch.from_numpy(generate_lidar_rays())
    preds, gts = [], []
    for i, seed in enumerate(METRIC_SEEDS):
        sp, sg, fp, fg, org = metric_scene(seed)
        p = oref.process_one_sample(sp, rays, org, fp)
        g = oref.process_one_sample(sg, rays, org, fg)
        for nm, got in (('pcd_pred', p), ('pcd_gt', g)):
            want = gold[f'{nm}_{i}']
            assert got.shape == want.shape == (2 * 14040, 4)
            assert np.array_equal(got, want), (nm, i, int((got != want).sum()))     # rays bit-exact
        preds.append(p)
        gts.append(g)
    with np.errstate(divide='ignore', invalid='ignore'):
        _check_scores(gold, *oref.calc_metrics(*_valid_lists(preds, gts)))


def test_product_calc_metrics_matches_reference_golden(gold):
    """The vectorised calc_metrics of the product on the reference's per-ray arrays: the reference's scores, and
    tools/ray_iou/metric.py's (which takes unmasked per-field lists, metric.py:31-48) agree with them."""
    from occnet_amd.metrics import calc_metrics
    preds = [gold[f'pcd_pred_{i}'] for i in range(len(METRIC_SEEDS))]
    gts = [gold[f'pcd_gt_{i}'] for i in range(len(METRIC_SEEDS))]
    _check_scores(gold, *calc_metrics(*_valid_lists(preds, gts)))
    # metric.py sums the flow error over ALL valid rays of a sample once any true positive of the class exists
    # (metric.py:70-73: `flow_error = np.linalg.norm(gt_flow - pred_flow)` is not masked by tp_mask), so its AVE
    # differs from ray_metrics.py's by construction; its IoU is the same quantity
    assert np.array_equal(gold['metric_py_iou'], gold['iou'], equal_nan=True)
    assert gold['metric_py_ave'].shape == gold['ave'].shape


@pytest.fixture(scope='module')
def dvr_gold():
    return dict(np.load(DVR_GOLD))


def _dvr_case(name, args):
    from tests.test_gpu_dvr import _case
    seed, N, T, Z, Y, X, M, occ = args
    return _case(seed, N, T, Z, Y, X, M, occ, outside=name == "origin_outside"), [T, Z, Y, X]


@pytest.mark.parametrize("phase", ["test", "train"])
def test_c_oracle_matches_reference_kernel(dvr_gold, phase):
    """oracle/dvr_ref.c (the restatement the HIP kernel is held to, bit for bit) vs the reference's own kernel body
    compiled for the host: random occupancy, time-indexed grids, origins outside, padded / axis-aligned /
    near-zero-length rays (the cases of tests/test_gpu_dvr.py).  The kernel's results are stored in
    tests/golden/dvr_reference_kernel.npz (oracle/gen_golden.py); where oracle/_ref is built, the kernel runs live too."""
    from oracle import ray_metrics_ref as oref
    try:
        oref.dvr_lib()
    except FileNotFoundError:
        pytest.skip("oracle/_build/libdvr_ref.so not built (make -C oracle)")
    ref = None
    if os.path.exists(REF_SO):
        from oracle.refshim import _reference_dvr
        ref = _reference_dvr()
    for name, args in DVR_KERNEL_CASES:
        (sigma, origin, points, tindex), grid = _dvr_case(name, args)
        got = oref.render_forward(sigma, origin, points, tindex, phase)
        wants = [[torch.from_numpy(dvr_gold[f'{name}_{phase}_{nm}']) for nm in DVR_FIELDS]]
        if ref is not None:
            wants.append(ref.render_forward(sigma, origin, points, tindex, grid, phase))
        for want in wants:
            for nm, a, b in zip(DVR_FIELDS, got, want):
                assert torch.equal(a, b), (name, phase, nm, int((a != b).sum()))


def test_fma_contraction_moves_no_voxel_and_distances_by_ulps(dvr_gold):
    """nvcc contracts a*b+c into fused multiply-adds by default; the oracle and the HIP kernel do not.  On the
    nuScenes-sized case the reference kernel built with contraction (stored in tests/golden/dvr_reference_kernel.npz,
    live as well where oracle/_ref is built) picks the same voxel for every ray as the oracle (= the reference kernel
    without contraction, test_c_oracle_matches_reference_kernel) and its distances agree to a few float32 ulps — far
    below the metric's 1 m threshold."""
    from oracle import ray_metrics_ref as oref
    try:
        oref.dvr_lib()
    except FileNotFoundError:
        pytest.skip("oracle/_build/libdvr_ref.so not built (make -C oracle)")
    (sigma, origin, points, tindex), grid = _dvr_case("nuscenes_grid", dict(DVR_KERNEL_CASES)["nuscenes_grid"])
    a = oref.render_forward(sigma, origin, points, tindex, "test")
    fmas = [[torch.from_numpy(dvr_gold[f'nuscenes_grid_fma_test_{nm}']) for nm in DVR_FIELDS]]
    if os.path.exists(REF_SO.replace('.so', '_fma.so')):
        from oracle.refshim import _reference_dvr
        fmas.append(_reference_dvr('libdvr_reference_fma.so').render_forward(sigma, origin, points, tindex, grid, "test"))
    for b in fmas:
        assert torch.equal(a[2], b[2])
        assert float((a[0] - b[0]).abs().max()) < 1e-4


@pytest.mark.gpu
def test_hip_pipeline_matches_reference_golden(gold):
    from occnet_amd.metrics import ray_metrics as prm
    rays = torch.from_numpy(prm.generate_lidar_rays())
    scenes = [metric_scene(s) for s in METRIC_SEEDS]
    for i, (sp, sg, fp, fg, org) in enumerate(scenes):
        for nm, sem, fl in (('pcd_pred', sp, fp), ('pcd_gt', sg, fg)):
            got = prm.process_one_sample(sem, rays, org, fl)
            want = gold[f'{nm}_{i}']
            assert np.array_equal(got, want), (nm, i, int((got != want).sum()))
    res = prm.main([s[0].reshape(-1) for s in scenes], [s[1].reshape(-1) for s in scenes],
                   [s[2].reshape(-1) for s in scenes], [s[3].reshape(-1) for s in scenes],
                   [s[4] for s in scenes], verbose=False)
    _check_scores(gold, res['iou_list'], res['ave_list'])
    assert abs(res['occ_score'] - float(gold['occ_score'])) < 1e-12
