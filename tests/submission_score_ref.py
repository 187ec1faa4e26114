"""numpy restatement of the challenge server's scorer (test infrastructure for csrc/submission_score.hip).

`Ref.add` is the reference's tools/ray_iou/metric.py:calc_metrics (:31-73) for one sample, statement by statement — the casts to
int32 / float32, the non-free filter, the L1 depth test, the per-class masks and the AVE rule that adds the flow error of EVERY
valid ray of a sample once the class has a true positive in it — with exact Python-int counters instead of float64 ones.  The
flow-error sum is carried three ways: as the fixed-point integer of the kernel (rint(float64(err) * 2^28) per ray, non-finite
errors and errors >= 2^34 counted in `ave_inf` / `ave_nan` instead), as a float64 sum, and as metric.py's own float32 pairwise
`np.sum`.  `compute` is metric.py:75-81 and :118-132.  Nothing is imported from the reference."""
import numpy as np

QUANTUM = 2.0 ** -28
ERR_LIMIT = np.float32(2.0 ** 34)
THRESHOLDS = (1, 2, 4)
FLOW_CLASSES = 8
ROWS = 17


class Ref:
    def __init__(self, free_id=16):
        self.free_id = free_id
        self.ncls = n = free_id + 1
        self.gt_cnt = [0] * n
        self.pred_cnt = [0] * n
        self.tp = [[0] * n for _ in THRESHOLDS]
        self.ave_cnt = [[0] * n for _ in THRESHOLDS]
        self.ave_sum = [[0] * n for _ in THRESHOLDS]          # fixed point, units of 2^-28
        self.ave_inf = [[0] * n for _ in THRESHOLDS]
        self.ave_nan = [[0] * n for _ in THRESHOLDS]
        self.ave_f64 = np.zeros((3, n))                       # float64 sum of the float32 errors
        self.ave_np = np.zeros((3, n))                        # metric.py: ave[j][i] += np.sum(flow_error) (float32 pairwise)

    def add(self, pred, gt):
        """pred, gt: (cls, dist, flow (n, 2)) arrays of one sample, of any dtype"""
        n_flow = min(FLOW_CLASSES, self.ncls)
        with np.errstate(all='ignore'):
            pred_cls, gt_cls = np.asarray(pred[0]).astype(np.int32), np.asarray(gt[0]).astype(np.int32)
            pred_dist, gt_dist = np.asarray(pred[1]).astype(np.float32), np.asarray(gt[1]).astype(np.float32)
            pred_flow, gt_flow = np.asarray(pred[2]).astype(np.float32), np.asarray(gt[2]).astype(np.float32)
            valid = gt_cls != self.free_id
            pred_cls, pred_dist, pred_flow = pred_cls[valid], pred_dist[valid], pred_flow[valid].reshape(-1, 2)
            gt_cls, gt_dist, gt_flow = gt_cls[valid], gt_dist[valid], gt_flow[valid].reshape(-1, 2)
            l1 = np.abs(pred_dist - gt_dist)
            flow_error = np.linalg.norm(gt_flow - pred_flow, axis=1)
            assert flow_error.dtype == np.float32
            is_nan = np.isnan(flow_error)
            is_inf = ~is_nan & ~(flow_error < ERR_LIMIT)
            fin = flow_error[~is_nan & ~is_inf]
            fixed = int(np.rint(fin.astype(np.float64) * 2.0 ** 28).astype(np.int64).sum())
            f64 = flow_error.astype(np.float64).sum()
            f32 = np.sum(flow_error)
        for c in range(self.ncls):
            self.gt_cnt[c] += int((gt_cls == c).sum())
            self.pred_cnt[c] += int((pred_cls == c).sum())
        for j, thr in enumerate(THRESHOLDS):
            hit = l1 < thr
            for c in range(self.ncls):
                tp = int(((gt_cls == c) & (pred_cls == c) & hit).sum())
                self.tp[j][c] += tp
                if c < n_flow and tp > 0:
                    self.ave_cnt[j][c] += int(flow_error.shape[0])
                    self.ave_sum[j][c] += fixed
                    self.ave_inf[j][c] += int(is_inf.sum())
                    self.ave_nan[j][c] += int(is_nan.sum())
                    with np.errstate(all='ignore'):
                        self.ave_f64[j][c] += f64
                        self.ave_np[j][c] += f32
        return self

    def words(self):
        """the kernel's state: int64 (17 * ncls)"""
        rows = [self.gt_cnt, self.pred_cnt] + self.tp + self.ave_cnt + self.ave_sum + self.ave_inf + self.ave_nan
        return np.array(rows, dtype=np.int64).reshape(-1)

    def compute(self):
        """-> dict(iou_list, ave_fixed, ave_f64, ave_np): metric.py:75-79, the AVE at threshold 2 m from each of the three
        sums (ave_np is what the server itself computes)"""
        n, n_flow = self.ncls, min(FLOW_CLASSES, self.ncls)
        gt_cnt, pred_cnt = np.array(self.gt_cnt, np.float64), np.array(self.pred_cnt, np.float64)
        tp = np.array(self.tp, np.float64)
        with np.errstate(all='ignore'):
            iou_list = [(tp[j] / (gt_cnt + pred_cnt - tp[j]))[:-1] for j in range(3)]
            cnt = np.array(self.ave_cnt[1], np.float64)
            mask = np.full(n, np.nan)
            mask[:n_flow] = 0.0
            ave_fixed = (np.array(self.ave_sum[1], np.float64) * QUANTUM + mask) / cnt
            ave_fixed[np.array(self.ave_inf[1]) != 0] = np.inf
            ave_fixed[np.array(self.ave_nan[1]) != 0] = np.nan
            ave_f64 = (self.ave_f64[1] + mask) / cnt
            ave_np = (self.ave_np[1] + mask) / cnt
        return dict(iou_list=iou_list, ave_fixed=ave_fixed[:-1], ave_f64=ave_f64[:-1], ave_np=ave_np[:-1])


def output(iou_list, ave_list):
    """metric.py:118-132"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        miou, mave = np.nanmean(iou_list), np.nanmean(ave_list)
        out = {f'RayIoU@{t}': np.nanmean(iou_list[j]) for j, t in enumerate(THRESHOLDS)}
    out.update({'RayIoU': miou, 'mAVE': mave, 'final_Occ_Score': miou * 0.9 + max(1 - mave, 0.0) * 0.1})
    return out


def split_rows(rows):
    """float32 rows (n, 4) -> (cls, dist, flow)"""
    rows = np.asarray(rows)
    return rows[:, 0], rows[:, 1], rows[:, 2:4]


def pack_rows(rows):
    """float32 rows -> the file's types, as nuscenes_occ.py:232-234 converts them"""
    rows = np.asarray(rows)
    with np.errstate(all='ignore'):
        return rows[:, 0].astype(np.int8), rows[:, 1].astype(np.float16), rows[:, 2:4].astype(np.float16)
