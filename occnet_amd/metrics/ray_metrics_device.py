"""RayIoU / mAVE / OccScore with the state on the device (csrc/ray_metrics_fused.hip).

`ray_metrics.main()` mirrors the reference's host loop: per sample and per lidar origin it uploads a float occupancy
grid, launches the ray caster, copies the hits back and scores in numpy.  `RayMetrics` takes the model's outputs and the
ground truth as device tensors, runs ONE fused pass per update (occupancy bit masks, both ray casts, the non-free
filter, the per-class terms) and keeps 14 x 17 int64 words on the device; nothing is copied or synchronised until
`compute()`.  The state is integer throughout (the flow-error sums are fixed point, quantum 2^-28 m/s), so it does not
depend on the order of arrival: partial states of batches or ranks add up exactly (`merge`, `all_reduce`).

State layout (ncls = free_id + 1 = 17 words per row; j = depth threshold 1 / 2 / 4 m):

    row 0        gt_cnt[c]        rays whose ground truth is class c
    row 1        pred_cnt[c]      scored rays whose prediction is class c
    rows 2-4     tp_cnt[j][c]     same class and |depth_pred - depth_gt| < thr_j
    rows 5-7     ave_cnt[j][c]    those true positives, flow classes (c < 8) only
    rows 8-10    ave_sum[j][c]    their flow errors |flow_gt - flow_pred|, in units of 2^-28 m/s
    rows 11-13   ave_bad[j][c]    their NON-FINITE flow errors (not in ave_sum): the class's AVE is reported as NaN
"""
import warnings

import numpy as np
import torch

from .device_common import DeviceRays, IntState, class_grid, flow_grid, occ_size
from .ray_metrics import flow_class_names, occ_class_names

QUANTUM = 2.0 ** -28          # m/s per unit of ave_sum
ROWS = 14


class RayMetrics(IntState):
    def __init__(self, pc_range, voxel_size, free_id=16, rays=None, device='cuda'):
        super().__init__(ROWS, free_id, device)
        self.pc_range = [float(v) for v in pc_range]
        self.voxel_size = float(voxel_size)
        self.occ_size = occ_size(self.pc_range, self.voxel_size)
        self._rays_dev = DeviceRays(rays, self.device)

    # ---- accumulation --------------------------------------------------------------------------------------------
    def update(self, sem_pred, flow_pred, sem_gt, flow_gt, lidar_origins, return_rays=False, origin_counts=None):
        """Add a batch (or one sample) to the state.  sem_* (B, X, Y, Z) uint8 / int64 — or any shape with X*Y*Z
        elements per sample, as main() takes them —, flow_* (B, X, Y, Z, 2) float32, lidar_origins (B, T, 3) ego metres
        (T <= 8; for one sample (1, T, 3) as main() takes it).  origin_counts: None (every sample has T origins) or a (B)
        int32 device tensor.  Device tensors are used as they are; the call enqueues two kernels and never synchronises.
        -> None, or with return_rays (rows_pred, rows_gt) (B, T, R, 4) device tensors in process_one_sample's order."""
        from .. import ext
        sem_pred, sem_gt = (class_grid(n, t, self.occ_size, self.device, convert=True)
                            for n, t in (('sem_pred', sem_pred), ('sem_gt', sem_gt)))
        flow_pred, flow_gt = (flow_grid(n, t, self.occ_size, self.device, convert=True)
                              for n, t in (('flow_pred', flow_pred), ('flow_gt', flow_gt)))
        origins = torch.as_tensor(lidar_origins).to(self.device, torch.float32).reshape(sem_pred.shape[0], -1, 3)
        B, X, Y, Z = sem_pred.shape
        return ext.ray_metrics_accumulate(self.state, sem_pred, flow_pred, sem_gt, flow_gt, origins.contiguous(),
                                          self._rays_dev(), self.pc_range[:3], self.voxel_size, self.free_id,
                                          origin_counts=origin_counts, return_rays=return_rays,
                                          workspace=self._grown_workspace(ext.ray_metrics_workspace_bytes(B, X, Y, Z)))

    # ---- scores --------------------------------------------------------------------------------------------------
    def compute(self):
        """One copy of the state to the host -> dict(miou, mave, occ_score, iou_list, ave_list) as main() returns."""
        s = self.state.cpu().numpy().reshape(ROWS, self.ncls)
        gt_cnt, pred_cnt = s[0].astype(np.float64), s[1].astype(np.float64)
        tp_cnt = s[2:5].astype(np.float64)
        n_flow = min(len(flow_class_names), self.ncls)
        with np.errstate(divide='ignore', invalid='ignore'):
            iou_list = [(tp_cnt[j] / (gt_cnt + pred_cnt - tp_cnt[j]))[:-1] for j in range(3)]
            ave = np.full(self.ncls, np.nan)
            ave[:n_flow] = (s[9][:n_flow].astype(np.float64) * QUANTUM) / s[6][:n_flow].astype(np.float64)
            ave[s[12] != 0] = np.nan
            ave_list = ave[:-1]
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)      # an empty state: every class is NaN
                miou = float(np.nanmean(iou_list))
                mave = float(np.nanmean(ave_list))
        occ_score = miou * 0.9 + max(1 - mave, 0.0) * 0.1
        return dict(miou=miou, mave=mave, occ_score=occ_score, iou_list=iou_list, ave_list=ave_list)


def main_device(sem_pred_list, sem_gt_list, flow_pred_list, flow_gt_list, lidar_origin_list, device='cuda',
                verbose=True):
    """ray_metrics.main() on the device-resident evaluator: same arguments (numpy arrays or device tensors per sample),
    same dict, same table."""
    from . import ray_metrics as rm
    metric = RayMetrics(rm._pc_range, rm._voxel_size, free_id=len(occ_class_names) - 1, device=device)
    for sem_pred, sem_gt, flow_pred, flow_gt, origins in zip(sem_pred_list, sem_gt_list, flow_pred_list, flow_gt_list,
                                                             lidar_origin_list):
        metric.update(sem_pred, flow_pred, sem_gt, flow_gt, origins)
    res = metric.compute()
    if verbose:
        iou_list, ave_list = res['iou_list'], res['ave_list']
        print(f"{'Class Names':22s} {'IoU@1':>7s} {'IoU@2':>7s} {'IoU@4':>7s} {'AVE':>7s}")
        for i in range(len(occ_class_names) - 1):
            print(f"{occ_class_names[i]:22s} {iou_list[0][i]:7.3f} {iou_list[1][i]:7.3f} "
                  f"{iou_list[2][i]:7.3f} {ave_list[i]:7.3f}")
        print(f"{'MEAN':22s} {np.nanmean(iou_list[0]):7.3f} {np.nanmean(iou_list[1]):7.3f} "
              f"{np.nanmean(iou_list[2]):7.3f} {np.nanmean(ave_list):7.3f}")
        print(' --- Occ score:', res['occ_score'])
    return res
