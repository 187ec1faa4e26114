"""The image-scale input on the GPU, three measurements ("Image scale on the device"):
  1. the launch time of ext.input_u8_scaled on 6 x 900 x 1600 frames at scale 1.0 / 0.8 / 0.5, next to ext.train_input_u8 on
     the same frames (every photometric stage on, GridMask on);
  2. images -> voxels per step of the base config under the inference plan at the same scales, uint8 frames resident:
     model.simple_test(scaled metas, img_u8=..., img_scale=s); the scale 1.0 row is the comparison line, and the plan's own
     uint8 stem route (no img_scale) is printed next to it;
  3. per scale, which launcher every backbone convolution of the plan went to, by input shape: the wrappers of ext that the
     plan calls and torch's conv2d (MIOpen), noted during one forward.
Same process for every figure; 3 warm-up passes, median of 7 timed passes, HIP events on the current stream, the candidates
alternating inside a pass.  A timed window of (1) holds 50 launches into a preallocated output, of (2) 5 steps.

    python -m tools_dev.input_scale_probe [--steps-per-pass 5]
"""
import argparse
import os
import statistics
from collections import Counter

import numpy as np
import torch

from occnet_amd import ext, io, synthetic
from occnet_amd.plugin import backbone_plan

NI, HS, WS = 6, 900, 1600
SCALES = (1.0, 0.8, 0.5)
NORM = dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False)
WARMUP, PASSES = 3, 7
LAUNCHES = 50          # per timed window of the launch-time figures: 3 to 8 ms of work between the two events


def timed(fn, n=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def medians(candidates, n=1):
    """{name: fn} -> {name: (median ms, [runs])}, the candidates alternating inside every pass."""
    runs = {k: [] for k in candidates}
    for i in range(WARMUP + PASSES):
        for k, fn in candidates.items():
            ms = timed(fn, n)
            if i >= WARMUP:
                runs[k].append(ms)
    return {k: (statistics.median(v), [round(t, 4) for t in v]) for k, v in runs.items()}


def launch_times(u8):
    np.random.seed(1)
    rec = io.sample_photometric(NI)
    rec[:, :5] = [[13.25, 1.2, 0.8, 9.5, 1.0], [-7.75, 1.0, 1.3, -12.5, 0.7]] * 3       # every stage on
    rec[:, 5:] = [[2, 0, 1], [1, 2, 0]] * 3
    rec_d = torch.from_numpy(rec).cuda()
    gm = (117, 59, 100, 20, 1, 1, 1)
    norm = (NORM['mean'], NORM['std'], NORM['to_rgb'])
    full = torch.empty(NI, 3, 928, 1600, device='cuda')
    cand = {'train_input_u8': lambda: ext.train_input_u8(u8, rec_d, *norm, grid_mask=gm, out=full)}
    for s in SCALES:
        hd, wd = io.scaled_size(HS, WS, s)
        out = torch.empty(NI, 3, (hd + 31) // 32 * 32, (wd + 31) // 32 * 32, device='cuda')
        cand[f'input_u8_scaled {s}'] = lambda s=s, out=out: ext.input_u8_scaled(u8, rec_d, *norm, s, grid_mask=gm, out=out)
    print(f"1. launch time, 6 x 900 x 1600 uint8 frames, every photometric stage and GridMask on, output preallocated, "
          f"{LAUNCHES} launches per timed window")
    for k, (ms, runs) in medians(cand, LAUNCHES).items():
        print(f"   {k:22s} {ms:.4f} ms   min {min(runs):.4f}  max {max(runs):.4f}   runs {runs}")


def build_model():
    from occnet_amd.plugin import Config, build_model, import_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_base_200x200x16.py'))
    import_plugin(cfg)
    torch.manual_seed(0)
    model = build_model(cfg.model)
    model.init_weights()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():           # query-dependent sampling pattern, as bench.py sets it up
        for n, p in model.named_parameters():
            if n.endswith("sampling_offsets.weight") or n.endswith("attention_weights.weight"):
                p.add_(torch.randn(p.shape, generator=g) * 0.02)
    model = model.cuda().eval()
    model.enable_fused_backbone(dtype=torch.bfloat16, use_graph=False)
    return model


def step_times(model, u8, steps):
    geo = dict(synthetic.BASE)
    (plain,) = synthetic.make_img_metas(geo, batch=1)
    frames = u8[None]
    cand, metas = {}, {}
    for s in SCALES:
        metas[s] = [io.scale_img_metas(plain, s, (HS, WS))]
        cand[f'img_scale {s}'] = lambda s=s: model.simple_test(metas[s], img_u8=frames, img_norm_cfg=NORM, img_scale=s)
    cand['no img_scale (uint8 stem)'] = lambda: model.simple_test([plain], img_u8=frames, img_norm_cfg=NORM)
    print(f"2. images -> voxels, base config, inference plan, uint8 frames resident, {steps} steps per pass")
    with torch.no_grad():
        res = medians(cand, steps)
    for k, (ms, runs) in res.items():
        print(f"   {k:26s} {ms:.3f} ms / step   runs {runs}")
    return metas


LAUNCHERS = ('stem_conv7x7_pool', 'stem_conv7x7_pool_u8', 'bottleneck64_nhwc', 'bottleneck64_next_nhwc', 'conv1x1_nhwc',
             'conv3x3_nhwc', 'conv3x3_conv1x1_nhwc')


def routing(model, u8, metas):
    """One forward per scale with every launcher the plan calls wrapped: (launcher, input shape (N, C, H, W)) counts."""
    print("3. where the plan's convolutions went, per scale: launcher, input (N, C, H, W), launches")
    seen = Counter()
    saved = {n: getattr(ext, n) for n in LAUNCHERS}
    conv2d = backbone_plan.F.conv2d

    def note(name, fn):
        def wrapped(x, *a, **k):
            seen[(name, tuple(x.shape))] += 1
            return fn(x, *a, **k)
        return wrapped
    try:
        for n, fn in saved.items():
            setattr(ext, n, note(n, fn))
        backbone_plan.F.conv2d = note('MIOpen conv2d', conv2d)
        for s in SCALES:
            seen.clear()
            with torch.no_grad():
                model.simple_test(metas[s], img_u8=u8[None], img_norm_cfg=NORM, img_scale=s)
            torch.cuda.synchronize()
            print(f"   scale {s}:")
            for (name, shape), count in sorted(seen.items(), key=lambda kv: (-kv[0][1][2], kv[0][0])):
                print(f"     {name:24s} {str(shape):24s} x{count}")
            fell = sorted({shape for (name, shape) in seen if name == 'MIOpen conv2d'})
            print(f"     fell back to MIOpen: {fell if fell else 'none'}")
    finally:
        for n, fn in saved.items():
            setattr(ext, n, fn)
        backbone_plan.F.conv2d = conv2d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps-per-pass', type=int, default=5)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    u8 = torch.from_numpy(rng.randint(0, 256, size=(NI, HS, WS, 3)).astype(np.uint8)).cuda()
    launch_times(u8)
    model = build_model()
    metas = step_times(model, u8, args.steps_per_pass)
    routing(model, u8, metas)


if __name__ == '__main__':
    main()
