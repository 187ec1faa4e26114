"""The score a submission file gets from the challenge server, with the state on the device (csrc/submission_score.hip).

The reference has two scorers.  `RayMetrics` mirrors projects/mmdet3d_plugin/datasets/ray_metrics.py: unrounded float32 rays, a
flow error counted on true-positive rays only.  The leaderboard runs tools/ray_iou/metric.py on the rows of the file (pcd_cls
int8, pcd_dist float16, pcd_flow float16), and its AVE rule is different: once a flow class has any true positive in a sample
at a threshold, the flow error of EVERY valid ray of that sample is added, with the count of all those rays (metric.py:70-73).
`SubmissionScore` restates that scorer: rows in — the packed buffers of `ext.submission_rays`, float32 rows, or the dicts of a
file —, 17 x ncls int64 words on the device, nothing copied or synchronised until `compute()`.  The state is integer throughout
(the flow-error sums are fixed point, quantum 2^-28 m/s), so partial states of batches or ranks add up exactly.

State layout (ncls = free_id + 1 words per row; j = depth threshold 1 / 2 / 4 m):

    row 0        gt_cnt[c]        valid rays (ground truth not free) whose ground truth is class c
    row 1        pred_cnt[c]      valid rays whose prediction is class c
    rows 2-4     tp[j][c]         same class and |depth_pred - depth_gt| < thr_j
    rows 5-7     ave_cnt[j][c]    valid rays of the samples in which flow class c (< 8) had a true positive at thr_j
    rows 8-10    ave_sum[j][c]    the flow errors |flow_gt - flow_pred| of those rays, in units of 2^-28 m/s
    rows 11-13   ave_inf[j][c]    those of them that are infinite (or >= 2^34 m/s), left out of ave_sum: the AVE is inf
    rows 14-16   ave_nan[j][c]    those that are NaN, left out of ave_sum: the AVE is NaN
"""
import warnings

import numpy as np
import torch

from .device_common import IntState

QUANTUM = 2.0 ** -28          # m/s per unit of ave_sum
ROWS = 17
FLOW_CLASSES = 8
_FIELDS = ('pcd_cls', 'pcd_dist', 'pcd_flow')


class SubmissionScore(IntState):
    def __init__(self, free_id=16, device='cuda'):
        if not 1 <= int(free_id) <= 31:
            raise ValueError(f"SubmissionScore: free_id must be 1..31, got {free_id}")
        super().__init__(ROWS, free_id, device)

    # ---- accumulation ------------------------------------------------------------------------------------------------
    def _accumulate(self, pred, gt, counts, stride, max_chunks=0):
        from .. import ext
        workspace = self._grown_workspace(ext.submission_score_workspace_bytes(int(counts.numel())))
        ext.submission_score_accumulate(self.state, pred, gt, counts, stride, self.free_id, workspace=workspace,
                                        max_chunks=max_chunks)

    def _counts(self, counts, B, n):
        if counts is None:
            return torch.full((B,), n, dtype=torch.int32, device=self.device)
        counts = torch.as_tensor(counts)
        if counts.numel() != B:
            raise ValueError(f"SubmissionScore: counts must have {B} entries, got {counts.numel()}")
        return counts.to(self.device, torch.int32, non_blocking=True).reshape(B).contiguous()

    def update_packed(self, pred_buf, gt_buf, B, Tmax, R, counts):
        """Add B samples held in two packed device buffers of ext.submission_rays(B, Tmax, R) (prediction, ground truth).
        counts: (B) int32 device tensor of ROWS per sample (origin_counts[b] * R).  Two launches, no synchronisation."""
        from .. import ext
        pred = ext.submission_rays_views(pred_buf, B, Tmax, R)
        gt = ext.submission_rays_views(gt_buf, B, Tmax, R)
        self._accumulate(pred, gt, self._counts(counts, B, Tmax * R), Tmax * R)

    def update_rows(self, rows_pred, rows_gt, counts=None):
        """Add B samples of float32 rows (B, n, 4) = [class, dist, flow_x, flow_y] (process_one_sample's rows, or those of
        RayMetrics.update(return_rays=True) reshaped to (B, T * R, 4)); counts: None (n rows each) or B row counts."""
        rows_pred = torch.as_tensor(rows_pred).to(self.device, torch.float32)
        rows_gt = torch.as_tensor(rows_gt).to(self.device, torch.float32)
        if rows_pred.dim() == 2:
            rows_pred, rows_gt = rows_pred[None], rows_gt[None]
        if rows_pred.dim() != 3 or rows_pred.shape[2] != 4 or rows_gt.shape != rows_pred.shape:
            raise ValueError("SubmissionScore.update_rows: expected two (B, n, 4) tensors of the same shape, got "
                             f"{tuple(rows_pred.shape)} and {tuple(rows_gt.shape)}")
        B, n = rows_pred.shape[:2]
        if B == 0 or n == 0:
            return
        self._accumulate(rows_pred.contiguous(), rows_gt.contiguous(), self._counts(counts, B, n), n)

    def _upload(self, samples, stride):
        """Host rows of a batch -> what ext.submission_score_accumulate takes.  Rows in the file's own types travel as they
        are (7 bytes per ray); anything else is cast as metric.py casts it (int32 / float32) and travels as float32 rows."""
        B = len(samples)
        packed = all(np.asarray(s['pcd_cls']).dtype == np.int8 and np.asarray(s['pcd_dist']).dtype == np.float16
                     and np.asarray(s['pcd_flow']).dtype == np.float16 for s in samples)
        if packed:
            cls = np.zeros((B, stride), np.int8)
            dist = np.zeros((B, stride), np.float16)
            flow = np.zeros((B, stride, 2), np.float16)
            for b, s in enumerate(samples):
                n = len(s['pcd_cls'])
                cls[b, :n], dist[b, :n], flow[b, :n] = s['pcd_cls'], s['pcd_dist'], np.reshape(s['pcd_flow'], (n, 2))
            return tuple(torch.from_numpy(a).to(self.device, non_blocking=True) for a in (cls, dist, flow))
        rows = np.zeros((B, stride, 4), np.float32)
        for b, s in enumerate(samples):
            n = len(s['pcd_cls'])
            with np.errstate(invalid='ignore', over='ignore'):
                rows[b, :n, 0] = np.asarray(s['pcd_cls']).astype(np.int32)
                rows[b, :n, 1] = np.asarray(s['pcd_dist']).astype(np.float32)
                rows[b, :n, 2:4] = np.reshape(np.asarray(s['pcd_flow']).astype(np.float32), (n, 2))
        return torch.from_numpy(rows).to(self.device, non_blocking=True)

    def update_results(self, pred_results, gt_results, batch=8):
        """Add the samples of two host dicts {token: {pcd_cls, pcd_dist, pcd_flow}} (the `results` of two files), uploaded
        `batch` samples at a time.  Walks the ground truth's tokens; a token missing from the prediction raises RuntimeError
        (metric.py:100-114); extra prediction tokens are ignored.  -> number of samples."""
        tokens = list(gt_results)
        for tok in tokens:
            if tok not in pred_results:
                raise RuntimeError(f'OpenOcc: prediction is not found for token: {tok}')
        for tok in tokens:
            n_p, n_g = len(pred_results[tok]['pcd_cls']), len(gt_results[tok]['pcd_cls'])
            if n_p != n_g:
                raise ValueError(f"SubmissionScore.update_results: token {tok!r} has {n_p} predicted and {n_g} ground-truth "
                                 "rows")
        for k in range(0, len(tokens), int(batch)):
            toks = [t for t in tokens[k:k + int(batch)] if len(gt_results[t]['pcd_cls'])]
            if not toks:
                continue
            counts = [len(gt_results[t]['pcd_cls']) for t in toks]
            stride = max(counts)
            pred = self._upload([pred_results[t] for t in toks], stride)
            gt = self._upload([gt_results[t] for t in toks], stride)
            self._accumulate(pred, gt, self._counts(counts, len(toks), stride), stride)
        return len(tokens)

    # ---- scores ------------------------------------------------------------------------------------------------------
    def compute(self):
        """One copy of the state to the host -> metric.py's `output` keys (RayIoU@1, RayIoU@2, RayIoU@4, RayIoU, mAVE,
        final_Occ_Score) plus iou_list (3 arrays over the non-free classes) and ave_list (threshold 2 m; NaN for the classes
        without flow and, as 0 / 0, for a flow class without a true positive; inf / NaN where numpy's sum is)."""
        s = self.state.cpu().numpy().reshape(ROWS, self.ncls)
        gt_cnt, pred_cnt = s[0].astype(np.float64), s[1].astype(np.float64)
        tp = s[2:5].astype(np.float64)
        n_flow = min(FLOW_CLASSES, self.ncls)
        with np.errstate(divide='ignore', invalid='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)              # an empty state: every class is NaN
            iou_list = [(tp[j] / (gt_cnt + pred_cnt - tp[j]))[:-1] for j in range(3)]
            ave = np.full(self.ncls, np.nan)
            ave[:n_flow] = (s[9][:n_flow].astype(np.float64) * QUANTUM) / s[6][:n_flow].astype(np.float64)
            ave[:n_flow][s[12][:n_flow] != 0] = np.inf
            ave[:n_flow][s[15][:n_flow] != 0] = np.nan
            ave_list = ave[:-1]
            miou = np.nanmean(iou_list)
            mave = np.nanmean(ave_list)
            out = {f'RayIoU@{t}': float(np.nanmean(iou_list[j])) for j, t in enumerate((1, 2, 4))}
        score = miou * 0.9 + max(1 - mave, 0.0) * 0.1                    # metric.py:120
        out.update({'RayIoU': float(miou), 'mAVE': float(mave), 'final_Occ_Score': float(score), 'iou_list': iou_list,
                    'ave_list': ave_list})
        return out
