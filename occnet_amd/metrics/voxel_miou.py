"""Per-class voxel IoU over the voxels a mask admits, with the confusion counts on the device (csrc/visibility.hip).

The plain occupancy metric: of the voxels the cameras observed (`mask`, e.g. visibility.CameraVisibility), how many of class c
in the ground truth or the prediction are class c in both.  `update` is one launch and copies nothing; the state is
(ncls + 1) x ncls int64 words — row g, column p: admitted voxels with ground truth g and prediction p; last row: [skipped,
admitted] — so partial states of batches or ranks add up exactly."""
import warnings

import numpy as np

from .device_common import IntState, class_grid, occ_size


def iou_from_confusion(conf, free_id):
    """conf (ncls, ncls) counts, row = ground truth, column = prediction -> (iou (ncls) float64 = TP / (TP + FP + FN) with NaN
    where the denominator is 0, miou = nanmean over classes 0..free_id-1, iou_occupied = occupied vs free)."""
    conf = np.asarray(conf).astype(np.float64)
    tp = np.diag(conf)
    with np.errstate(divide='ignore', invalid='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                  # no class present: the mean of nothing is NaN
        iou = tp / (conf.sum(1) + conf.sum(0) - tp)
        miou = float(np.nanmean(iou[:free_id]))
        occ = conf[:free_id, :free_id].sum()                             # occupied in both
        union = conf.sum() - conf[free_id, free_id]
        iou_occupied = float(occ / union) if union > 0 else float('nan')
    return iou, miou, iou_occupied


class VoxelMIoU(IntState):
    def __init__(self, pc_range, voxel_size, free_id=16, device='cuda'):
        """pc_range and voxel_size give the [X, Y, Z] of the grids `update` takes, as for RayMetrics."""
        if not 1 <= int(free_id) <= 31:
            raise ValueError(f"VoxelMIoU: free_id must be 1..31, got {free_id}")
        super().__init__(int(free_id) + 2, free_id, device)
        self.occ_size = occ_size(pc_range, voxel_size)

    def update(self, sem_pred, sem_gt, mask=None):
        """Add B samples: sem_pred / sem_gt anything class_grid accepts (host data and other integer types are converted),
        mask: None (every voxel) or a bool / uint8 tensor of as many elements, non-zero = admitted.  One launch."""
        import torch
        from .. import ext
        pred = class_grid('sem_pred', sem_pred, self.occ_size, self.device, convert=True)
        gt = class_grid('sem_gt', sem_gt, self.occ_size, self.device, B=pred.shape[0], convert=True)
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype not in (torch.bool, torch.uint8):
                mask = mask != 0
            mask = mask.to(self.device).reshape(pred.shape).contiguous()
        ext.confusion_accumulate(self.state, pred, gt, mask=mask, free_id=self.free_id)

    def compute(self):
        """One copy of the state to the host -> {'iou' (ncls) float64 (NaN: class absent from both grids), 'miou' over classes
        0..free_id-1, 'iou_occupied', 'voxels' (admitted), 'skipped' (admitted, a class id outside 0..free_id), 'confusion'}."""
        s = self.state.cpu().numpy().reshape(self.ncls + 1, self.ncls)
        iou, miou, iou_occupied = iou_from_confusion(s[:self.ncls], self.free_id)
        return {'iou': iou, 'miou': miou, 'iou_occupied': iou_occupied, 'voxels': int(s[self.ncls, 1]),
                'skipped': int(s[self.ncls, 0]), 'confusion': s[:self.ncls].copy()}
