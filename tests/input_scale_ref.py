"""Shared by tests/test_input_scale_host.py and tests/test_gpu_input_scale.py: the float64 restatement of the scaled uint8
input chain (photometric distortion -> normalise -> bilinear rescale -> pad -> GridMask; csrc/input_scale_u8.hip and
include/occnet_amd_input.h state the arithmetic), the float32 host chain built from occnet_amd.io, and the bound.

The resize is the project's own definition ("Image scale on the device"): no reference run pins it.  The
restatement here takes the tap indices and the weights from the float32-exact statements (they are part of the definition:
a weight that differs in its last bit is another resize) and makes the blends in float64, on top of
train_input_ref.chain64(..., size_divisor=1), which returns the unpadded normalised image.  It is written as loops over the
destination index, not from io.resize_taps.

The bound of every comparison against it:
    max|got - ref|  <=  max(4 * E32, 24 * 2^-23 * max|ref|)
E32 = max|float32 host chain - ref| on the same inputs; the floor is train_input_ref's sixteen rounded operations plus
eight: the two weight formations (1 - fx, 1 - fy) and, along any one path to an output, the three operations of the
horizontal blend and the three of the vertical one.  The conditioning assertion min_abs_v >= 0.1 of train_input_ref is kept
and no pixel is excluded."""
import functools

import numpy as np

from occnet_amd import io
from occnet_amd.plugin.grid_mask import GridMask
from tests import train_input_ref as R

SHAPES = [(37, 53), (32, 64), (5, 9)]           # odd sizes, Ws % 4 != 0, pad in rows and columns; round sizes; a frame of a few pixels
SCALES = [0.5, 0.8, 1.25, 0.3]                  # 1.25 reaches all four clamps on 37 x 53, the others none
GRIDS = ['off', 'both_mode1']


def sizes(hs, ws, scale, d=32):
    """-> (Hd, Wd), (H, W): truncation after a double multiply, then the next multiples of d."""
    hd, wd = int(hs * scale), int(ws * scale)
    return (hd, wd), R.padded(hd, wd, d)


def taps(n_src, n_dst, columns):
    """One axis, one destination index at a time -> (i0, i1, w0, w1, clamps): indices as ints, weights as float32, and how
    many destination indices hit the low and the high clamp."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    i0, i1, w0, w1, low, high = [], [], [], [], 0, 0
    for d in range(n_dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if columns:
            if s < 0:
                s, f, low = 0, np.float32(0), low + 1
            if s >= n_src - 1:
                s, f, high = n_src - 1, np.float32(0), high + 1
            a, b = s, min(s + 1, n_src - 1)
        else:
            low += s < 0
            high += s + 1 > n_src - 1
            a, b = min(max(s, 0), n_src - 1), min(max(s + 1, 0), n_src - 1)
        i0.append(a)
        i1.append(b)
        w0.append(np.float32(1) - f)
        w1.append(f)
    return np.array(i0), np.array(i1), np.array(w0, np.float32), np.array(w1, np.float32), (low, high)


def resize64(x, hd, wd):
    """x (..., hs, ws) float64 -> ((..., hd, wd) float64, clamp counts): the blends in float64."""
    hs, ws = x.shape[-2:]
    r0, r1, b0, b1, row_clamps = taps(hs, hd, columns=False)
    c0, c1, a0, a1, col_clamps = taps(ws, wd, columns=True)
    a0, a1, b0, b1 = (w.astype(np.float64) for w in (a0, a1, b0, b1))
    h0 = x[..., r0, :][..., c0] * a0 + x[..., r0, :][..., c1] * a1
    h1 = x[..., r1, :][..., c0] * a0 + x[..., r1, :][..., c1] * a1
    return h0 * b0[:, None] + h1 * b1[:, None], dict(rows=row_clamps, columns=col_clamps)


def chain64(fr, records, mean, std, to_rgb, scale, gm=None, size_divisor=32):
    """-> ((NI, 3, H, W) float64, info): train_input_ref.chain64's info plus the clamp counts and the sizes."""
    n64, info = R.chain64(fr, records, mean, std, to_rgb, size_divisor=1)
    (hd, wd), (H, W) = sizes(fr.shape[1], fr.shape[2], scale, size_divisor)
    y, clamps = resize64(n64, hd, wd)
    out = np.zeros((len(fr), 3, H, W))
    out[:, :, :hd, :wd] = y
    info = dict(info, clamps=clamps, resized=(hd, wd), padded=(H, W))
    return out * R.mask64(H, W, gm), info


def chain32(fr, records, mean, std, to_rgb, scale, gm=None, size_divisor=32):
    """The float32 host chain of occnet_amd.io + GridMask.mask_from_params -> (NI, 3, H, W) float32."""
    imgs = io.photometric_distort(list(fr), records)
    imgs, _ = io.normalize_multiview(imgs, mean, std, to_rgb)
    imgs, _ = io.random_scale_multiview(imgs, scale)
    imgs, _ = io.pad_multiview(imgs, size_divisor=size_divisor)
    x = np.stack(imgs).transpose(0, 3, 1, 2)
    if gm is not None:
        d, l, st_h, st_w, use_h, use_w, mode = gm
        x = x * GridMask.mask_from_params(x.shape[2], x.shape[3], d, l, st_h, st_w, bool(use_h), bool(use_w), mode)
    return np.ascontiguousarray(x, dtype=np.float32)


def bound(e32, ref):
    return max(4.0 * e32, 24.0 * 2.0 ** -23 * float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def case(shape, norm, scale):
    """The unmasked float64 reference and float32 chain of one (shape, norm, scale) under R.RECORDS; computed once."""
    mean, std, to_rgb = R.NORMS[norm]
    fr = R.frames(*shape)
    ref, info = chain64(fr, R.RECORDS, mean, std, to_rgb, scale)
    f32 = chain32(fr, R.RECORDS, mean, std, to_rgb, scale)
    for a in (ref, f32):
        a.setflags(write=False)
    return dict(frames=fr, ref=ref, f32=f32, info=info, mean=mean, std=std, to_rgb=to_rgb)


def grey_frames(hs, ws):
    """(NI, hs, ws, 3) uint8 with b == g == r in every pixel, all 256 levels where the frame has that many pixels: the HSV
    round trip, which the kernel always makes, returns such pixels exactly (s == 0), so identity records leave float(u8)
    and only the normalisation and the resize are on trial."""
    lv = np.random.RandomState(hs * ws).permutation(np.arange(R.NI * hs * ws) % 256).astype(np.uint8)
    return np.repeat(lv.reshape(R.NI, hs, ws, 1), 3, -1)
