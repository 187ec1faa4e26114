"""A/B timing of scoring a submission as the challenge server does: the host route (the packed rows copied out as
SubmissionWriter.results() does, then the numpy restatement of tools/ray_iou/metric.py, tests/submission_score_ref.py — the
only route before SubmissionScore) against the device update (metrics.SubmissionScore.update_packed on the packed buffers
where they lie, csrc/submission_score.hip).

    python -m tools_dev.submission_score_ab [--origins 8] [--passes 5] [--json OUT]

One full-size sample (8 origins x 14 040 rays) and a batch of 8, seeded tests/golden_cases.metric_scene grids.  Same process,
alternating A / B, one warm-up pass of each, median of the timed passes.  A pass is timed on the host clock from the packed
device buffers to the score dict (the device is synchronised before the clock starts; both routes end in a host value).  Then
the kernels alone, by HIP events over 20 back-to-back calls: the score launch pair with the launcher's grid, with one block per
sample (max_chunks = 1), and the cast launch pair (ext.submission_rays) that precedes it in SubmissionWriter.add_scored.
Prints every pass, then one JSON line per batch size."""
import argparse
import json
import statistics
import time

import numpy as np
import torch

from occnet_amd import ext
from occnet_amd.metrics import SubmissionScore, ray_metrics as rm
from tests import submission_score_ref as ssr
from tests.golden_cases import metric_scene


def batch(n, origins):
    sp, sg, fp, fg, org = [], [], [], [], []
    for k in range(n):
        a, b, c, d, o = metric_scene(100 + k)
        rng = np.random.default_rng(1000 + k)
        oo = torch.from_numpy(rng.uniform([-3.0, -1.5, 1.7], [3.0, 1.5, 1.95], (1, origins, 3)).astype(np.float32))
        oo[:, :min(2, origins)] = o[:, :min(2, origins)]
        sp.append(a.astype(np.int64)), sg.append(b.astype(np.int64)), fp.append(c), fg.append(d), org.append(oo)
    dev = lambda xs: torch.from_numpy(np.stack(xs)).cuda()
    return dev(sp), dev(fp), dev(sg), dev(fg), torch.cat(org).cuda()


def events_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--origins', type=int, default=8)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    free_id = len(rm.occ_class_names) - 1
    rays = torch.from_numpy(rm.generate_lidar_rays()).cuda()
    R, T = rays.shape[0], a.origins
    lines = []
    for B in (1, 8):
        sp, fp, sg, fg, origins = batch(B, T)
        nbytes = ext.submission_rays_bytes(B, T, R)
        pbuf = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        gbuf = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        cast_ws = torch.empty(max(ext.submission_rays_workspace_bytes(B, 200, 200, 16), 256), dtype=torch.uint8, device='cuda')

        def cast(sem, flow, out):
            ext.submission_rays(sem, flow, origins, rays, rm._pc_range[:3], rm._voxel_size, free_id, out=out, workspace=cast_ws)

        cast(sp, fp, pbuf), cast(sg, fg, gbuf)
        counts = torch.full((B,), T * R, dtype=torch.int32, device='cuda')
        score = SubmissionScore(free_id=free_id)

        def run_host():
            ref = ssr.Ref(free_id)
            p = [v.numpy() for v in ext.submission_rays_views(pbuf.cpu(), B, T, R)]
            g = [v.numpy() for v in ext.submission_rays_views(gbuf.cpu(), B, T, R)]
            for b in range(B):
                ref.add((p[0][b].reshape(-1), p[1][b].reshape(-1), p[2][b].reshape(-1, 2)),
                        (g[0][b].reshape(-1), g[1][b].reshape(-1), g[2][b].reshape(-1, 2)))
            res = ref.compute()
            return ref, ssr.output(res['iou_list'], res['ave_fixed'])

        def run_device():
            score.reset()
            score.update_packed(pbuf, gbuf, B, T, R, counts)
            return score.compute()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res

        timed(run_host), timed(run_device)              # warm-up
        ta, tb = [], []
        for i in range(a.passes):
            t, (ref, want) = timed(run_host)
            ta.append(t)
            t, got = timed(run_device)
            tb.append(t)
            print(f'B={B} pass {i}: host route {ta[-1]:.3f} ms, device update + compute {tb[-1]:.3f} ms', flush=True)
        same_state = bool(np.array_equal(score.state.cpu().numpy(), ref.words()))
        same_score = all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in want)

        state = torch.zeros(ext.submission_score_state_words(free_id), dtype=torch.int64, device='cuda')
        ws = torch.empty(ext.submission_score_workspace_bytes(B), dtype=torch.uint8, device='cuda')
        pv, gv = ext.submission_rays_views(pbuf, B, T, R), ext.submission_rays_views(gbuf, B, T, R)

        def kernels(max_chunks):
            return lambda: ext.submission_score_accumulate(state, pv, gv, counts, T * R, free_id, workspace=ws,
                                                           max_chunks=max_chunks)

        k_grid, k_one = events_ms(kernels(0)), events_ms(kernels(1))
        k_cast = events_ms(lambda: cast(sp, fp, pbuf))
        print(f'B={B} kernels: score pair {k_grid * 1e3:.1f} us, score pair with one block per sample {k_one * 1e3:.1f} us, '
              f'cast pair {k_cast * 1e3:.1f} us', flush=True)
        rec = dict(samples=B, origins=T, rays=int(B * T * R), host_route_ms=[round(t, 3) for t in ta],
                   device_update_compute_ms=[round(t, 3) for t in tb], host_route_median_ms=round(statistics.median(ta), 3),
                   device_update_compute_median_ms=round(statistics.median(tb), 3), state_equal=same_state,
                   score_equal=bool(same_score), score_pair_us=round(k_grid * 1e3, 1),
                   score_pair_one_block_per_sample_us=round(k_one * 1e3, 1), cast_pair_us=round(k_cast * 1e3, 1),
                   final_Occ_Score=got['final_Occ_Score'], mAVE=got['mAVE'])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
