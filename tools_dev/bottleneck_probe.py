"""Dev probe: time the whole-bottleneck kernels on the ResNet-50 layer1 shape (6 x 232 x 400) against the
HBM floor (x read once + out written once).

    python tools_dev/bottleneck_probe.py [--variants 1,2,3,4,5] [--iters 20] [--rounds 3]

variants are those of ext.bottleneck64_nhwc (1 = first kernel, 2 = second kernel, 3 / 4 / 5 = second kernel with tile
order 0 / 1 / 2); they are timed alternately, `rounds` times each.  Under `rocprofv3 --pmc` use --iters 2 --rounds 1 and
one variant per run: the counters are then per launch of that variant."""
import argparse
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from occnet_amd import ext


def setup(cin, ds):
    g = torch.Generator().manual_seed(0)
    N, H, W = 6, 232, 400
    x = torch.randn(N, cin, H, W, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    mk = lambda *s: torch.randn(*s, generator=g).cuda() * 0.05
    pack = ext.bottleneck64_pack(mk(64, cin, 1, 1), mk(64), mk(64, 64, 3, 3), mk(64), mk(256, 64, 1, 1), mk(256),
                                 mk(256, cin, 1, 1) if ds else None, mk(256) if ds else None)
    return x, pack


def run(cin, ds, variants, iters, rounds):
    x, pack = setup(cin, ds)
    N, _, H, W = x.shape
    mb = N * H * W * (cin + 256) * 2 / 1e6
    ref = ext.bottleneck64_nhwc(x, pack, variant=1)
    out = torch.empty_like(ref)
    for v in variants:
        same = torch.equal(ext.bottleneck64_nhwc(x, pack, variant=v), ref)
        print(f"bottleneck64 cin={cin} ds={ds} variant {v}: bits equal to variant 1: {same}")
    for r in range(rounds):
        for v in variants:
            for _ in range(3):
                ext.bottleneck64_nhwc(x, pack, variant=v, out=out)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); a.record()
            for _ in range(iters):
                ext.bottleneck64_nhwc(x, pack, variant=v, out=out)
            b.record(); torch.cuda.synchronize()
            us = a.elapsed_time(b) * 1e3 / iters
            print(f"bottleneck64 cin={cin} ds={ds} variant {v} round {r}: {us:.1f} us  "
                  f"({mb:.0f} MB min traffic -> {mb / us:.2f} TB/s)", flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--variants', default='1,2')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', choices=['256', '64'], default=None)
    a = ap.parse_args()
    vs = [int(v) for v in a.variants.split(',')]
    if a.only != '64':
        run(256, False, vs, a.iters, a.rounds)
    if a.only != '256':
        run(64, True, vs, a.iters, a.rounds)
