"""GridMask train-time image augmentation (reference: projects/mmdet3d_plugin/models/utils/grid_mask.py:70-124,
instantiated by BEVFormerOcc as GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7),
bevformer_occ.py:52-53, applied in extract_img_feat when `use_grid_mask`, :81-82).

Draws from numpy's global RNG in the reference's order (apply?, period d, row start, column start, angle), so
a run seeded like the reference masks the same pixels.  The mask is built on the host (one (1.5h, 1.5w) byte
plane per call) and applied on the device.  For rotate == 1 and offset == False (what BEVFormerOcc builds) the mask
has a closed form in four integers: sample_params draws them without building the plane, mask_from_params evaluates
the form on the host, and ext.train_input_u8 evaluates it inside the uint8 training-input kernel."""
import numpy as np
import torch
import torch.nn as nn


class GridMask(nn.Module):
    def __init__(self, use_h, use_w, rotate=1, offset=False, ratio=0.5, mode=0, prob=1.):
        super().__init__()
        self.use_h, self.use_w, self.rotate, self.offset = use_h, use_w, rotate, offset
        self.ratio, self.mode, self.st_prob, self.prob = ratio, mode, prob, prob
        self.fp16_enable = False

    def set_prob(self, epoch, max_epoch):
        self.prob = self.st_prob * epoch / max_epoch

    @staticmethod
    def _rotate_nearest(mask, degrees):
        """Counter-clockwise rotation about the image centre, nearest neighbour, zero fill (PIL's
        Image.rotate defaults)."""
        if degrees % 360 == 0:
            return mask
        hh, ww = mask.shape
        a = np.deg2rad(degrees)
        cy, cx = hh / 2.0, ww / 2.0
        y, x = np.mgrid[0:hh, 0:ww].astype(np.float64)
        xs, ys = x + 0.5 - cx, y + 0.5 - cy
        sx = np.cos(a) * xs - np.sin(a) * ys + cx
        sy = np.sin(a) * xs + np.cos(a) * ys + cy
        ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        ok = (ix >= 0) & (ix < ww) & (iy >= 0) & (iy < hh)
        out = np.zeros_like(mask)
        out[ok] = mask[iy[ok], ix[ok]]
        return out

    def make_mask(self, h, w):
        """The (h, w) float32 multiplier of one call (host array), consuming the RNG like the reference."""
        hh, ww = int(1.5 * h), int(1.5 * w)
        d = np.random.randint(2, h)
        self.l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        mask = np.ones((hh, ww), np.float32)
        st_h, st_w = np.random.randint(d), np.random.randint(d)
        if self.use_h:
            for i in range(hh // d):
                s = d * i + st_h
                mask[s:min(s + self.l, hh), :] = 0
        if self.use_w:
            for i in range(ww // d):
                s = d * i + st_w
                mask[:, s:min(s + self.l, ww)] = 0
        r = np.random.randint(self.rotate)
        mask = self._rotate_nearest(np.uint8(mask), r).astype(np.float32)
        mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]
        return 1 - mask if self.mode == 1 else mask

    def sample_params(self, h, w):
        """The draws of one forward() call on an (h, w) image without building the mask: None when the mask is not
        applied, else (d, l, st_h, st_w).  Consumes numpy's global RNG exactly as forward() + make_mask() do (apply?,
        d, st_h, st_w, the randint(rotate) angle), so either route leaves the generator in the same state.  The
        parameters describe the whole mask only for rotate == 1 (the angle is then always 0) and offset == False: that
        is what mask_from_params and the device route (ext.train_input_u8) evaluate."""
        if np.random.rand() > self.prob or not self.training:
            return None
        d = np.random.randint(2, h)
        self.l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        st_h, st_w = np.random.randint(d), np.random.randint(d)
        np.random.randint(self.rotate)
        return int(d), int(self.l), int(st_h), int(st_w)

    @staticmethod
    def mask_from_params(h, w, d, l, st_h, st_w, use_h=True, use_w=True, mode=0):
        """make_mask's (h, w) float32 multiplier for rotate == 1 in closed form.  With hh = int(1.5 h) and
        Y = y + (hh - h) // 2, row y lies in a band iff use_h, Y - st_h >= 0, (Y - st_h) // d < hh // d and
        (Y - st_h) % d < l; columns alike.  0 inside a band, 1 outside, inverted for mode == 1."""
        def bands(n, st, use):
            nn = int(1.5 * n)
            t = np.arange(n) + (nn - n) // 2 - st
            return (t >= 0) & (t // d < nn // d) & (t % d < l) if use else np.zeros(n, bool)
        band = bands(h, st_h, use_h)[:, None] | bands(w, st_w, use_w)[None, :]
        mask = np.where(band, np.float32(0), np.float32(1))
        return 1 - mask if mode == 1 else mask

    def forward(self, x):
        if np.random.rand() > self.prob or not self.training:
            return x
        n, c, h, w = x.size()
        mask = torch.from_numpy(np.ascontiguousarray(self.make_mask(h, w))).to(device=x.device, dtype=x.dtype)
        if self.offset:
            off = torch.from_numpy(2 * (np.random.rand(h, w) - 0.5)).to(device=x.device, dtype=x.dtype)
            return x * mask + off * (1 - mask)
        return x * mask
