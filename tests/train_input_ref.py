"""Shared by tests/test_train_input_host.py and tests/test_gpu_train_input.py: the float64 restatement of the uint8
training-input chain (photometric distortion -> normalise -> pad -> GridMask; csrc/train_input_u8.hip states the
arithmetic), the float32 host chain built from occnet_amd.io, the hand-written decision set and the bound.

The bound of every comparison against the float64 restatement:
    max|got - ref|  <=  max(4 * E32, 16 * 2^-23 * max|ref|)
E32 = max|float32 numpy chain - ref| on the same inputs (that chain is the reference's own arithmetic; the factor 4 and
the max-of-two form follow tests/test_gpu_bn3d_relu_train.py), the floor is sixteen rounded operations.

Conditioning (a condition, not a tolerance): s = diff / (|v| + eps) is ill-conditioned for 0 < |v| << 1, in the
reference too.  Every hand-written brightness delta lies >= 0.25 from the nearest integer and chain64's info['min_abs_v'] is
the smallest non-zero |v| of the float64 reference, which the tests assert to be >= 0.1.  No pixel is excluded."""
import functools

import numpy as np

from occnet_amd import io
from occnet_amd.plugin.grid_mask import GridMask

EPS = float(np.finfo(np.float32).eps)
SHAPES = [(33, 50), (32, 64), (5, 9)]           # -> (64, 64) pad rows + columns, Ws % 4 != 0, 150-byte rows; (32, 64) no pad;
NI = 6                                           #    (32, 32) a frame smaller than one block's row of threads
NORMS = {'imagenet_rgb': ([123.675, 116.28, 103.53], [58.395, 57.12, 57.375], True),
         'base_bgr': ([103.530, 116.280, 123.675], [1.0, 1.0, 1.0], False)}

# delta, alpha_pre, sat, hue, alpha_post, perm: every stage on and off, contrast before (the reference's mode 1) and after
# (mode 0) the HSV round trip, all six permutations, hue shifts of both signs large enough to wrap at 360 and at 0
RECORDS = np.array([
    [0.0, 1.0, 1.0, 0.0, 1.0, 0, 1, 2],
    [17.25, 1.3, 1.4, 17.5, 1.0, 2, 0, 1],
    [-20.75, 1.0, 1.0, -17.5, 0.6, 1, 2, 0],
    [0.0, 1.0, 0.55, 0.0, 1.0, 0, 2, 1],
    [0.0, 0.5, 1.0, 10.5, 1.0, 1, 0, 2],
    [31.75, 1.0, 1.5, -3.25, 1.5, 2, 1, 0]], dtype=np.float32)


def padded(hs, ws, d=32):
    return (hs + d - 1) // d * d, (ws + d - 1) // d * d


def grid_cases(H, W):
    """name -> None | (d, l, st_h, st_w, use_h, use_w, mode) for an (H, W) output."""
    dn = H - 1                                   # d near h: GridMask draws d from [2, h)
    df = H - 7                                   # hh // d == 1: the second period starts INSIDE the crop and holds no band
    return {
        'off': None,
        'both_mode1': (7, 4, 3, 5, 1, 1, 1),     # what BEVFormerOcc builds; at H = 64 bands start beyond the crop
        'd_near_h': (dn, (dn + 1) // 2, dn - 1, 0, 1, 1, 1),      # st_h > Y at the top rows: no band there
        'one_period': (df, (df + 1) // 2, 0, 2, 1, 1, 0),
        'use_h_mode0': (5, 2, 4, 1, 1, 0, 0),
        'use_w_mode0': (9, 3, 8, 8, 0, 1, 0),
    }


@functools.lru_cache(maxsize=None)
def frames(hs, ws):
    """(NI, hs, ws, 3) uint8: seeded noise, then all 256 levels, grey pixels, black, white and argmax ties in each pair
    of channels (both as the two largest and with the third on top)."""
    rng = np.random.RandomState(1000 * hs + ws)
    f = rng.randint(0, 256, size=(NI * hs * ws, 3)).astype(np.uint8)
    special = [[0, 0, 0], [255, 255, 255], [128, 128, 128], [1, 1, 1], [200, 200, 10], [200, 10, 200], [10, 200, 200],
               [90, 90, 200], [90, 200, 90], [200, 90, 90], [255, 0, 0], [0, 255, 0], [0, 0, 255], [30, 10, 250], [10, 30, 250]]
    per = hs * ws
    free = np.ones(NI * per, bool)
    for i in range(NI):                          # the same special pixels in every image: under every record
        f[i * per + per - len(special):(i + 1) * per] = special
        free[i * per + per - len(special):(i + 1) * per] = False
    levels = f[free].reshape(-1)                 # (a copy) every level once, in the pixels that are not special
    levels[:256] = np.arange(256)
    f[free] = levels.reshape(-1, 3)
    return f.reshape(NI, hs, ws, 3)


def mask64(H, W, gm):
    """Step 7 on the host, written out independently of GridMask.mask_from_params."""
    if gm is None:
        return np.ones((H, W))
    d, l, st_h, st_w, use_h, use_w, mode = gm
    hh, ww = int(1.5 * H), int(1.5 * W)
    band = np.zeros((H, W), bool)
    for y in range(H):
        t = y + (hh - H) // 2 - st_h
        if use_h and t >= 0 and t // d < hh // d and t % d < l:
            band[y, :] = True
    for x in range(W):
        t = x + (ww - W) // 2 - st_w
        if use_w and t >= 0 and t // d < ww // d and t % d < l:
            band[:, x] = True
    m = np.where(band, 0.0, 1.0)
    return 1.0 - m if mode == 1 else m


def chain64(fr, records, mean, std, to_rgb, gm=None, size_divisor=32):
    """Steps 1-7 in float64 on float32-exact parameters -> ((NI, 3, H, W) float64, info dict)."""
    n, hs, ws, _ = fr.shape
    H, W = padded(hs, ws, size_divisor)
    rec = np.asarray(records, dtype=np.float32).astype(np.float64)
    x = fr.astype(np.float64)
    x = (x + rec[:, 0, None, None, None]) * rec[:, 1, None, None, None]
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = diff / (np.abs(v) + EPS)
    k = 60.0 / (diff + EPS)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + 120.0, (r - g) * k + 240.0))
    h = np.where(h < 0, h + 360.0, h)
    s = s * rec[:, 2, None, None]
    hue = np.broadcast_to(rec[:, 3, None, None], h.shape)
    h = h + hue
    over = (h > 360) & (hue != 0)
    h = np.where(over, h - 360.0, h)
    under = (h < 0) & (hue != 0)
    h = np.where(under, h + 360.0, h)
    h6 = h * (1.0 / 60.0)
    h6 = np.where(h6 < 0, h6 + 6.0, h6)
    h6 = np.where(h6 >= 6, h6 - 6.0, h6)
    assert (h6 >= 0).all() and (h6 < 6).all()
    sec = np.floor(h6).astype(np.int64)
    f = h6 - sec
    tab = np.stack([v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))], -1)
    idx = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    bgr = np.where((s == 0)[..., None], v[..., None], np.take_along_axis(tab, idx[sec], -1))
    bgr = bgr * rec[:, 4, None, None, None]
    perm = rec[:, 5:8].astype(np.int64)
    bgr = np.stack([bgr[i][..., perm[i]] for i in range(n)])
    if to_rgb:
        bgr = bgr[..., ::-1]
    mean32 = np.asarray(mean, dtype=np.float32)
    stdinv32 = (1 / np.float64(np.asarray(std, dtype=np.float32))).astype(np.float32)
    y = (bgr - mean32.astype(np.float64)) * stdinv32.astype(np.float64)
    out = np.zeros((n, 3, H, W))
    out[:, :, :hs, :ws] = y.transpose(0, 3, 1, 2)
    out = out * mask64(H, W, gm)
    nz = np.abs(v)[v != 0]
    info = dict(min_abs_v=float(nz.min()) if nz.size else np.inf, wrap_over=int(over.sum()), wrap_under=int(under.sum()),
                grey=int((diff == 0).sum()), sectors=sorted(set(sec[s != 0].tolist())), negative_v=int((v < 0).sum()),
                ties=[int(((b == g) & (v == b)).sum()), int(((b == r) & (v == b)).sum()), int(((g == r) & (v == g)).sum())])
    return out, info


def chain32(fr, records, mean, std, to_rgb, gm=None, size_divisor=32):
    """The float32 host chain of occnet_amd.io + GridMask.mask_from_params -> (NI, 3, H, W) float32."""
    imgs = io.photometric_distort(list(fr), records)
    imgs, _ = io.normalize_multiview(imgs, mean, std, to_rgb)
    imgs, _ = io.pad_multiview(imgs, size_divisor=size_divisor)
    x = np.stack(imgs).transpose(0, 3, 1, 2)
    if gm is not None:
        d, l, st_h, st_w, use_h, use_w, mode = gm
        x = x * GridMask.mask_from_params(x.shape[2], x.shape[3], d, l, st_h, st_w, bool(use_h), bool(use_w), mode)
    return np.ascontiguousarray(x, dtype=np.float32)


def bound(e32, ref):
    return max(4.0 * e32, 16.0 * 2.0 ** -23 * float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def case(shape, norm):
    """The unmasked float64 reference and float32 chain of one (shape, norm) under RECORDS; computed once."""
    mean, std, to_rgb = NORMS[norm]
    fr = frames(*shape)
    ref, info = chain64(fr, RECORDS, mean, std, to_rgb)
    f32 = chain32(fr, RECORDS, mean, std, to_rgb)
    for a in (ref, f32):
        a.setflags(write=False)
    return dict(frames=fr, ref=ref, f32=f32, info=info, mean=mean, std=std, to_rgb=to_rgb)
