"""A/B of the uint8 training input at the base shape (NI = 6, 900 x 1600 -> 928 x 1600), on the GPU:
  (a) ext.train_input_u8, every photometric stage on, GridMask on: one launch
  (b) the torch-op training branch of BEVFormerOcc.extract_feat_u8 (float, flip, subtract, multiply, permute, pad — it has
      no augmentation) followed by the GridMask module's forward (host-built mask, upload, multiply)
Alternating, 2 warm-ups, median of 5, HIP events on the current stream (for (b) the interval includes the host's mask
construction, during which the stream idles: that is the route's cost per step).

    python -m tools_dev.train_input_ab
"""
import statistics

import numpy as np
import torch

from occnet_amd import ext, io
from occnet_amd.plugin.grid_mask import GridMask

NI, HS, WS = 6, 900, 1600
MEAN, STD, TO_RGB = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375], True


def torch_chain(u8, size_divisor=32):
    x = u8.float()
    if TO_RGB:
        x = x.flip(-1)
    stdinv = [float(1.0 / float(torch.tensor(v, dtype=torch.float32))) for v in STD]
    x = (x - x.new_tensor(MEAN)) * x.new_tensor(stdinv)
    d = size_divisor
    H, W = (HS + d - 1) // d * d, (WS + d - 1) // d * d
    return torch.nn.functional.pad(x.permute(0, 3, 1, 2), (0, W - WS, 0, H - HS)).contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    rng = np.random.RandomState(0)
    u8 = torch.from_numpy(rng.randint(0, 256, size=(NI, HS, WS, 3)).astype(np.uint8)).cuda()
    np.random.seed(1)
    rec = io.sample_photometric(NI)
    rec[:, :5] = [[13.25, 1.2, 0.8, 9.5, 1.0], [-7.75, 1.0, 1.3, -12.5, 0.7]] * 3       # every stage on
    rec[:, 5:] = [[2, 0, 1], [1, 2, 0]] * 3
    rec_d = torch.from_numpy(rec).cuda()
    module = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=1.0).train()
    gm = (417, 209, 100, 200, 1, 1, 1)
    out = torch.empty(NI, 3, 928, 1600, device='cuda')

    def a():
        return ext.train_input_u8(u8, rec_d, MEAN, STD, TO_RGB, grid_mask=gm, out=out)

    def b_chain():
        return torch_chain(u8)

    def b():
        return module(torch_chain(u8))
    ta, tb, tc = [], [], []
    for i in range(7):
        np.random.seed(100 + i)
        for name, fn, acc in (('a', a, ta), ('b', b, tb), ('b_chain', b_chain, tc)):
            ms, _ = timed(fn)
            if i >= 2:
                acc.append(ms)
    ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
    nbytes = NI * HS * WS * 3 + NI * 3 * 928 * 1600 * 4
    print(f"(a) train_input_u8, all stages + GridMask: {ma:.3f} ms (runs {[round(t, 3) for t in ta]}), "
          f"{nbytes / 1e6:.1f} MB -> {nbytes / ma / 1e6:.0f} GB/s")
    print(f"(b) torch chain + GridMask module: {mb:.3f} ms (runs {[round(t, 3) for t in tb]}); chain alone {mc:.3f} ms "
          f"(runs {[round(t, 3) for t in tc]})")
    print(f"(a) / (b) = {ma / mb:.4f}; (a) / (b, chain alone) = {ma / mc:.4f}")


if __name__ == '__main__':
    main()
