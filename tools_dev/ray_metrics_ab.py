"""A/B timing of the evaluation path: metrics.main (host loop around the ray caster, numpy inputs) against
metrics.main_device (fused device-resident evaluator, device tensors as input — how each is used).

    python -m tools_dev.ray_metrics_ab [--samples 8] [--origins 8] [--passes 5] [--json OUT]

Same process, alternating A / B / A / B, one warm-up pass of each, median of the timed passes; 8 seeded
tests/golden_cases.metric_scene samples with 8 lidar origins each.  A pass is timed on the host clock from the call to the
returned scores (both paths end with their results on the host; the device is synchronised before the clock starts).
Prints one JSON line with both medians, the per-pass values and the scores' agreement."""
import argparse
import json
import statistics
import time

import numpy as np
import torch

from occnet_amd import metrics
from tests.golden_cases import metric_scene


def scenes(n, origins):
    out = []
    for k in range(n):
        sp, sg, fp, fg, org = metric_scene(100 + k)
        rng = np.random.default_rng(1000 + k)
        extra = torch.from_numpy(rng.uniform([-3.0, -1.5, 1.7], [3.0, 1.5, 1.95], (1, origins, 3)).astype(np.float32))
        extra[:, :min(2, origins)] = org[:, :min(2, origins)]
        out.append((sp, sg, fp, fg, extra))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=8)
    ap.add_argument('--origins', type=int, default=8)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sc = scenes(a.samples, a.origins)
    host = [[s[i].reshape(-1) for s in sc] for i in range(4)] + [[s[4] for s in sc]]
    dev = [[torch.as_tensor(s[i]).cuda() for s in sc] for i in range(4)] + [[s[4].cuda() for s in sc]]

    def run_a():
        return metrics.main(host[0], host[1], host[2], host[3], host[4], verbose=False)

    def run_b():
        return metrics.main_device(dev[0], dev[1], dev[2], dev[3], dev[4], verbose=False)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    timed(run_a), timed(run_b)                      # warm-up
    ta, tb = [], []
    for _ in range(a.passes):
        t, ra = timed(run_a)
        ta.append(t)
        t, rb = timed(run_b)
        tb.append(t)
    same_iou = bool(np.array_equal(np.stack(ra['iou_list']), np.stack(rb['iou_list']), equal_nan=True))
    ave_a, ave_b = np.asarray(ra['ave_list']), np.asarray(rb['ave_list'])
    ok = ~np.isnan(ave_a)
    rec = dict(samples=a.samples, origins=a.origins, rays=int(a.samples * a.origins * 14040),
               main_ms=[round(t, 3) for t in ta], main_device_ms=[round(t, 3) for t in tb],
               main_median_ms=round(statistics.median(ta), 3), main_device_median_ms=round(statistics.median(tb), 3),
               speedup=round(statistics.median(ta) / statistics.median(tb), 2), iou_identical=same_iou,
               ave_max_rel_diff=float((np.abs(ave_a[ok] - ave_b[ok]) / np.abs(ave_a[ok])).max()) if ok.any() else 0.0,
               occ_score_main=ra['occ_score'], occ_score_main_device=rb['occ_score'])
    line = json.dumps(rec)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
