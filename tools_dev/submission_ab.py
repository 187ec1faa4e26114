"""A/B timing of the submission path: io.format_submission (host loop around the ray caster, numpy inputs as forward_test
hands them over) against io.format_submission_device (metrics.SubmissionWriter on device tensors — how each is used).

    python -m tools_dev.submission_ab [--samples 8] [--origins 8] [--passes 5] [--out DIR] [--json OUT]

Same process, alternating A / B / A / B, one warm-up pass of each, median of the timed passes; 8 seeded
tests/golden_cases.metric_scene samples with 8 float64 lidar origins each (the type io.lidar_origins returns).  A pass is timed
on the host clock from the call to the written file (the device is synchronised before the clock starts and after the call).
Then the device path's own split, per pass: HIP events around the two kernels alone and around SubmissionWriter.add (kernels +
the copy into the pinned slot), host clock around results() (waiting is excluded: the device is synchronised first — what is
left are the per-sample numpy slices) and around the pickle + gzip + write that both paths share.
Prints every pass, then one JSON line."""
import argparse
import json
import os
import statistics
import tempfile
import time

import numpy as np
import torch

from occnet_amd import ext, io as oio
from occnet_amd.metrics import SubmissionWriter, ray_metrics as rm
from tests.golden_cases import metric_scene


def scenes(n, origins):
    out = []
    for k in range(n):
        sp, _, fp, _, org = metric_scene(100 + k)
        rng = np.random.default_rng(1000 + k)
        o = torch.from_numpy(rng.uniform([-3.0, -1.5, 1.7], [3.0, 1.5, 1.95], (1, origins, 3)))
        o[:, :min(2, origins)] = org[:, :min(2, origins)].double()
        out.append((f'sample{k}', sp.astype(np.int64), fp, o))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=8)
    ap.add_argument('--origins', type=int, default=8)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    out = a.out or tempfile.mkdtemp(prefix='submission_ab_')
    host = scenes(a.samples, a.origins)
    dev = [(t, torch.from_numpy(s).cuda(), torch.from_numpy(f).cuda(), o) for t, s, f, o in host]

    def run_a():
        return oio.format_submission(host, os.path.join(out, 'a'))

    def run_b():
        return oio.format_submission_device(dev, os.path.join(out, 'b'), batch=a.samples)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    timed(run_a), timed(run_b)                      # warm-up
    ta, tb = [], []
    for i in range(a.passes):
        t, pa = timed(run_a)
        ta.append(t)
        t, pb = timed(run_b)
        tb.append(t)
        print(f'pass {i}: format_submission {ta[-1]:.3f} ms, format_submission_device {tb[-1]:.3f} ms', flush=True)
    with open(pa, 'rb') as fa, open(pb, 'rb') as fb:
        identical = fa.read() == fb.read()

    # the device path's own split
    sem = torch.stack([s for _, s, _, _ in dev])
    flow = torch.stack([f for _, _, f, _ in dev])
    origins = torch.cat([o for _, _, _, o in dev])
    tokens = [t for t, _, _, _ in dev]
    free_id = len(rm.occ_class_names) - 1
    rays = torch.from_numpy(rm.generate_lidar_rays()).cuda()
    buf = torch.empty(ext.submission_rays_bytes(a.samples, a.origins, rays.shape[0]), dtype=torch.uint8, device='cuda')
    origins_dev = origins.cuda()
    split = dict(kernels_ms=[], add_ms=[], slices_ms=[], pickle_gzip_write_ms=[])
    w = SubmissionWriter(rm._pc_range, rm._voxel_size, free_id=free_id, depth=1)
    for i in range(a.passes + 1):                   # pass 0 warms up (and allocates the writer's slot)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        w.reset()
        torch.cuda.synchronize()
        ev[0].record()
        ext.submission_rays(sem, flow, origins_dev, rays, rm._pc_range[:3], rm._voxel_size, free_id, out=buf)
        ev[1].record()
        ev[2].record()
        w.add(tokens, sem, flow, origins)
        ev[3].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = w.results()
        t1 = time.perf_counter()
        oio.write_submission(res, os.path.join(out, 'split'))
        t2 = time.perf_counter()
        if i == 0:
            continue                                # warm-up
        split['kernels_ms'].append(ev[0].elapsed_time(ev[1]))
        split['add_ms'].append(ev[2].elapsed_time(ev[3]))
        split['slices_ms'].append((t1 - t0) * 1e3)
        split['pickle_gzip_write_ms'].append((t2 - t1) * 1e3)
        print(f'split {i - 1}: kernels {split["kernels_ms"][-1]:.3f} ms, add (kernels + copy) '
              f'{split["add_ms"][-1]:.3f} ms, slices {split["slices_ms"][-1]:.3f} ms, '
              f'pickle + gzip + write {split["pickle_gzip_write_ms"][-1]:.3f} ms', flush=True)
    med = statistics.median
    rec = dict(samples=a.samples, origins=a.origins, rays=int(a.samples * a.origins * rays.shape[0]),
               format_submission_ms=[round(t, 3) for t in ta], format_submission_device_ms=[round(t, 3) for t in tb],
               format_submission_median_ms_per_sample=round(med(ta) / a.samples, 3),
               format_submission_device_median_ms_per_sample=round(med(tb) / a.samples, 3),
               files_identical=bool(identical),
               split_median_ms={k: round(med(v), 3) for k, v in split.items()},
               split_ms={k: [round(x, 3) for x in v] for k, v in split.items()})
    line = json.dumps(rec)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
