"""numpy restatement of the accumulation of csrc/ray_metrics_fused.hip, from per-ray rows (label, depth, flow_x, flow_y) as
process_one_sample returns them: main()'s non-free filter, calc_metrics' terms as integers, the flow-error sums in fixed
point.  Shared by tests/test_ray_metrics_device_host.py and tests/test_gpu_ray_metrics_device.py (helper, no tests)."""
import numpy as np

ROWS = 14
QUANTUM = 2.0 ** -28
ERR_LIMIT = 2.0 ** 34
N_FLOW = 8


def flow_errors(pcd_pred, pcd_gt):
    """float32 flow error per ray, as the reference computes it (ray_metrics.py:185)."""
    return np.linalg.norm(pcd_gt[:, 2:4] - pcd_pred[:, 2:4], axis=1)


def restate_state(pcd_pred, pcd_gt, free_id=16):
    """-> (14 * ncls) int64 state of the rows of ONE sample (all rays, unfiltered)."""
    ncls = free_id + 1
    s = np.zeros((ROWS, ncls), np.int64)
    valid = pcd_gt[:, 0].astype(np.int32) != free_id
    p, g = pcd_pred[valid], pcd_gt[valid]
    lp, lg = p[:, 0], g[:, 0]
    in_p = (lp >= 0) & (lp < ncls)
    in_g = (lg >= 0) & (lg < ncls)
    s[0] += np.bincount(lg[in_g].astype(np.int64), minlength=ncls)
    s[1] += np.bincount(lp[in_p].astype(np.int64), minlength=ncls)
    l1 = np.abs(p[:, 1] - g[:, 1])
    with np.errstate(invalid='ignore', over='ignore'):
        err = flow_errors(p, g)
    assert l1.dtype == np.float32 and err.dtype == np.float32
    same = (lp == lg) & in_g
    for j, thr in enumerate((1, 2, 4)):
        tp = same & (l1 < thr)
        s[2 + j] += np.bincount(lg[tp].astype(np.int64), minlength=ncls)
        fl = tp & (lg < N_FLOW)
        cls, e = lg[fl].astype(np.int64), err[fl]
        s[5 + j] += np.bincount(cls, minlength=ncls)
        with np.errstate(invalid='ignore'):
            ok = e < ERR_LIMIT                      # False for NaN and inf
        np.add.at(s[8 + j], cls[ok], np.rint(e[ok].astype(np.float64) / QUANTUM).astype(np.int64))
        s[11 + j] += np.bincount(cls[~ok], minlength=ncls)
    return s.reshape(-1)
