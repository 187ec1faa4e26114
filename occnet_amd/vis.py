"""Pictures of a prediction: camera views and a bird's-eye view rendered on the device (csrc/occ_render.hip).

A pin-hole camera is one more bundle of rays through the caster the evaluator and the submission writer use (csrc/ray_cast.h):
per pixel, which voxel the camera sees, its class, its distance, and — with a ground truth — whether the two agree, drawn over
the uint8 frame the model was fed.  `view_rays` turns the img_metas the model already takes into the 12 floats per camera the
kernel wants; `OccRenderer` holds palette, geometry and a ring of pinned host slots (the scheme of metrics.SubmissionWriter: two
launch pairs, non-blocking copies, one event per batch; a slot is read only when it is about to be reused); `save_png` writes an
image with the standard library alone.

    python -m occnet_amd.vis GRID.npz --out DIR [--gt GT.npz] [--size 232 400]     # six cameras + BEV -> DIR/mosaic.png ...
    python -m occnet_amd.vis --bench                                                # one JSON line: render vs. the per-view loop
"""
import os
import struct
import zlib

import numpy as np
import torch

from .metrics.device_common import SlotRing, class_grid, occ_size

# this project's own colour table: classes 0..15 of the occupancy benchmark, 16 = free, 17 = the spare id some label sets add
_CLASS_RGB = (
    (66, 135, 245),    # 0 car
    (38, 70, 160),     # 1 truck
    (120, 90, 200),    # 2 trailer
    (20, 160, 170),    # 3 bus
    (200, 120, 30),    # 4 construction vehicle
    (235, 80, 150),    # 5 bicycle
    (190, 40, 90),     # 6 motorcycle
    (230, 40, 40),     # 7 pedestrian
    (250, 160, 20),    # 8 traffic cone
    (150, 150, 160),   # 9 barrier
    (90, 90, 100),     # 10 driveable surface
    (125, 115, 110),   # 11 other flat
    (170, 150, 190),   # 12 sidewalk
    (150, 185, 110),   # 13 terrain
    (215, 205, 185),   # 14 manmade
    (40, 140, 60),     # 15 vegetation
    (250, 250, 250),   # 16 free (never drawn: a free voxel is no hit)
    (240, 230, 60),    # 17
)
# agreement categories of the diff mode: 0 both miss (never drawn), 1 agree (drawn in the class colour), 2 depth off, 3 class
# differs, 4 prediction only, 5 ground truth only
_CATEGORY_RGB = ((0, 0, 0), (255, 255, 255), (250, 200, 40), (170, 60, 220), (230, 50, 40), (40, 110, 240))


def default_palette():
    """(256, 3) uint8: the table above, then a fixed spread of hues for ids this project has no name for."""
    pal = np.zeros((256, 3), np.uint8)
    pal[:len(_CLASS_RGB)] = np.array(_CLASS_RGB, np.uint8)
    k = np.arange(len(_CLASS_RGB), 256)
    pal[len(_CLASS_RGB):] = np.stack([(k * 67 + 40) % 200 + 40, (k * 131 + 90) % 200 + 40, (k * 29 + 150) % 200 + 40],
                                     -1).astype(np.uint8)
    return pal


def category_palette():
    return np.array(_CATEGORY_RGB, np.uint8)


def view_rays(img_metas, render_hw, img_hw=None):
    """img_metas: one dict per sample with `lidar2img` (V 4x4), `ego2lidar` (4x4) and `img_shape`; render_hw = (h, w) of the
    rendered image; img_hw = (H, W) of the image the matrices project into (default: img_shape of each camera).
    -> (B, V, 12) float32: per camera the centre o (3) in ego metres and the row-major 3x3 D with
    ego point = o + depth * D (px, py, 1)^T for pixel centre (px, py) of the RENDERED image.
    M = lidar2img @ ego2lidar is the product point_sampling projects with; it must be affine (last row 0 0 0 1 within 1e-6).
    The inverse is taken in float64 (view_rays64) and rounded to float32 once."""
    return torch.from_numpy(view_rays64(img_metas, render_hw, img_hw).astype(np.float32))


def view_rays64(img_metas, render_hw, img_hw=None):
    """view_rays before its one rounding -> (B, V, 12) float64 numpy."""
    h, w = int(render_hw[0]), int(render_hw[1])
    out = []
    for meta in img_metas:
        ego2lidar = np.asarray(meta['ego2lidar'], np.float64)
        rows = []
        for v, l2i in enumerate(meta['lidar2img']):
            M = np.asarray(l2i, np.float64) @ ego2lidar
            if M.shape != (4, 4) or np.abs(M[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > 1e-6:
                raise ValueError(f"view_rays: camera {v}: lidar2img @ ego2lidar is not affine (last row {M[3].tolist()})")
            H_img, W_img = (img_hw if img_hw is not None else meta['img_shape'][v])[:2]
            inv = np.linalg.inv(M)
            D = inv[:3, :3].copy()
            D[:, 0] *= float(W_img) / w
            D[:, 1] *= float(H_img) / h
            rows.append(np.concatenate([inv[:3, 3], D.reshape(-1)]))
        out.append(np.stack(rows))
    return np.stack(out)


def save_png(path, rgb):
    """rgb: (H, W, 3) or (H, W) uint8 (numpy or tensor) -> an 8-bit PNG (truecolour or greyscale) at `path`."""
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError(f"save_png: expected a non-empty (H, W, 3) or (H, W) uint8 image, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    raw = np.zeros((H, 1 + a[0].size), np.uint8)                      # filter byte 0 (None) in front of every row
    raw[:, 1:] = a.reshape(H, -1)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)

    png = (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0))
           + chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) + chunk(b'IEND', b''))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as f:
        f.write(png)
    return path


class OccRenderer:
    def __init__(self, pc_range, voxel_size, free_id=16, size=(232, 400), palette=None, far=100., alpha=160, tol=2.,
                 device='cuda', depth=2, bg_rgb=0x101418):
        """size = (h, w) of a rendered camera view; palette: None (default_palette()) or (256, 3) uint8; far, tol in metres;
        alpha 0..256: the weight of the rendering over the frame; depth: the number of host slots of enqueue; bg_rgb: the
        background (0xRRGGBB) where no frame is given."""
        self.pc_range = [float(v) for v in pc_range]
        self.voxel_size = float(voxel_size)
        self.free_id = int(free_id)
        self.occ_size = occ_size(self.pc_range, self.voxel_size)
        self.size = (int(size[0]), int(size[1]))
        self.far, self.alpha, self.tol, self.bg_rgb = float(far), int(alpha), float(tol), int(bg_rgb)
        self.device = torch.device(device)
        pal = default_palette() if palette is None else np.asarray(palette)
        if pal.dtype != np.uint8 or pal.shape != (256, 3):
            raise ValueError(f"OccRenderer: palette must be (256, 3) uint8, got {pal.dtype} {pal.shape}")
        self._palette_host = torch.from_numpy(np.ascontiguousarray(pal))
        self._tables = None
        # a slot: device images `views` and `bev`, mask `workspace`, their pinned copies `host_views` and `host_bev`, the pinned
        # staging of the cameras `cams`
        self._ring = SlotRing("OccRenderer", depth, self._finish)

    def _dev_tables(self):
        if self._tables is None:
            self._tables = (self._palette_host.to(self.device), torch.from_numpy(category_palette()).to(self.device))
        return self._tables

    def _grid(self, name, t, B=None):
        return class_grid(name, t, self.occ_size, self.device, B)

    # ---- direct calls --------------------------------------------------------------------------------------------------
    def views(self, sem, img_metas, frames=None, sem_gt=None, want=('label', 'depth', 'rgb'), out=None, workspace=None,
              cams=None):
        """sem (B, X, Y, Z) uint8 / int64 device tensor (any shape with X*Y*Z elements per sample), img_metas: B dicts (view_rays),
        frames: None or (B, V, Hs, Ws, 3) uint8, sem_gt: None or the ground truth as sem (`label` then holds the agreement
        categories) -> {'label' (B, V, h, w) uint8, 'depth' (B, V, h, w) float32, 'rgb' (B, V, h, w, 3) uint8} on the device."""
        from . import ext
        sem = self._grid('sem', sem)
        sem_gt = None if sem_gt is None else self._grid('sem_gt', sem_gt, sem.shape[0])
        if cams is None:
            cams = view_rays(img_metas, self.size).to(self.device)
        if frames is not None:
            frames = torch.as_tensor(frames).to(self.device)
            frames = (frames[None] if frames.dim() == 4 else frames).contiguous()      # (V, Hs, Ws, 3): one sample
        pal, cat = self._dev_tables()
        return ext.render_views(sem, cams, self.pc_range[:3], self.voxel_size, self.size, free_id=self.free_id, sem_gt=sem_gt,
                                frames=frames, palette=pal, cat_palette=cat, far=self.far, tol=self.tol, alpha=self.alpha,
                                bg_rgb=self.bg_rgb, want=want, out=out, workspace=workspace)

    def bev(self, sem, sem_gt=None, want=('label', 'rgb'), out=None, workspace=None):
        """-> {'label' (B, X, Y) uint8, 'rgb' (B, X, Y, 3) uint8} on the device, in GRID order (mosaic() turns ego x up)."""
        from . import ext
        sem = self._grid('sem', sem)
        sem_gt = None if sem_gt is None else self._grid('sem_gt', sem_gt, sem.shape[0])
        pal, cat = self._dev_tables()
        return ext.render_bev(sem, free_id=self.free_id, sem_gt=sem_gt, palette=pal, cat_palette=cat, bg_rgb=self.bg_rgb,
                              want=want, out=out, workspace=workspace)

    @staticmethod
    def mosaic(views_rgb, bev_rgb, layout=((2, 0, 1), (4, 3, 5))):
        """views_rgb (V, h, w, 3), bev_rgb (X, Y, 3) uint8 tensors of ONE sample (device or host: torch ops only) -> one image
        (rows * h, cols * w + bev_w, 3): the camera views tiled as `layout` says (rows of view indices; None leaves a tile
        black), and right of them the BEV with ego x up and ego y to the left, scaled (nearest) to the mosaic's height."""
        views_rgb, bev_rgb = torch.as_tensor(views_rgb), torch.as_tensor(bev_rgb)
        V, h, w = views_rgb.shape[:3]
        rows, cols = len(layout), max(len(r) for r in layout)
        H = rows * h
        X, Y = bev_rgb.shape[:2]
        bw = max(1, (H * Y + X // 2) // X)
        out = torch.zeros((H, cols * w + bw, 3), dtype=torch.uint8, device=views_rgb.device)
        for r, row in enumerate(layout):
            for c, v in enumerate(row):
                if v is not None:
                    if not 0 <= int(v) < V:
                        raise ValueError(f"mosaic: layout names view {v}, there are {V}")
                    out[r * h:(r + 1) * h, c * w:(c + 1) * w] = views_rgb[int(v)]
        top = torch.flip(bev_rgb.to(out.device), (0, 1))                 # row 0 = largest x, column 0 = largest y
        ri = ((2 * torch.arange(H, device=out.device) + 1) * X) // (2 * H)
        ci = ((2 * torch.arange(bw, device=out.device) + 1) * Y) // (2 * bw)
        out[:, cols * w:] = top[ri][:, ci]
        return out

    # ---- the ring ------------------------------------------------------------------------------------------------------
    def enqueue(self, tokens, sem, img_metas, frames=None, sem_gt=None):
        """Render a batch (views and BEV, rgb only) and start its copy into a pinned host slot: two launch pairs, two
        non-blocking copies, one event.  The call waits only for the slot it is about to reuse (the batch enqueued `depth`
        calls ago).  tokens: one per sample (a single str for one sample)."""
        from . import ext
        tokens = self._ring.claim("OccRenderer.enqueue", tokens)
        B = len(tokens)
        sem = self._grid('sem', sem, B)
        sem_gt = None if sem_gt is None else self._grid('sem_gt', sem_gt, B)
        cams_host = view_rays(img_metas, self.size)
        if cams_host.shape[0] != B:
            raise ValueError(f"OccRenderer.enqueue: {B} tokens, {cams_host.shape[0]} img_metas")
        V = cams_host.shape[1]
        h, w = self.size
        X, Y, Z = self.occ_size
        slot = self._ring.take()
        dev = self.device
        nv, nb = B * V * h * w * 3, B * X * Y * 3
        views = slot.grown('views', nv, dtype=torch.uint8, device=dev)
        bev = slot.grown('bev', nb, dtype=torch.uint8, device=dev)
        workspace = slot.grown('workspace', max(ext.render_workspace_bytes(B, X, Y, Z, True), 256), dtype=torch.uint8, device=dev)
        host_views = slot.grown('host_views', nv, dtype=torch.uint8, pin_memory=True)
        host_bev = slot.grown('host_bev', nb, dtype=torch.uint8, pin_memory=True)
        staged = slot.grown('cams', B * V * 12, dtype=torch.float32, pin_memory=True)[:B * V * 12].view(B, V, 12)
        staged.copy_(cams_host)
        cams = staged.to(dev, non_blocking=True)                      # through the slot's pinned memory: does not block
        self.views(sem, None, frames=frames, sem_gt=sem_gt, want=('rgb',), out={'rgb': views}, workspace=workspace, cams=cams)
        self.bev(sem, sem_gt=sem_gt, want=('rgb',), out={'rgb': bev}, workspace=workspace)               # same stream
        host_views[:nv].copy_(views[:nv], non_blocking=True)
        host_bev[:nb].copy_(bev[:nb], non_blocking=True)
        self._ring.record(slot, tokens, (tokens, host_views[:nv].view(B, V, h, w, 3), host_bev[:nb].view(B, X, Y, 3)))

    @staticmethod
    def _finish(pending):
        tokens, views, bev = pending
        views, bev = views.numpy(), bev.numpy()
        for b, tok in enumerate(tokens):
            yield tok, {'views': views[b].copy(), 'bev': bev[b].copy()}

    def drain(self):
        """Wait for every enqueued batch, oldest first."""
        self._ring.results()
        return self

    def results(self):
        """-> {token: {'views' (V, h, w, 3) uint8, 'bev' (X, Y, 3) uint8 numpy}} in the order the samples were enqueued."""
        return self._ring.results()


# ---- command line -----------------------------------------------------------------------------------------------------------
def demo_grid(seed=0, shape=(200, 200, 16), free_id=16):
    """A seeded scene for runs without a dataset -> (pred, gt) uint8: ground, a sidewalk strip, a wall and boxes of several
    classes; the prediction shifts, relabels or drops some of them."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    gt = np.full(shape, free_id, np.uint8)
    gt[:, :, 0:max(1, Z // 8)] = 10
    gt[:, :int(Y * 0.3), 0:max(1, Z // 8)] = 12
    gt[:, int(Y * 0.92):, 0:max(2, (3 * Z) // 4)] = 14
    pred = gt.copy()
    z0 = max(1, Z // 8)
    for i in range(28):
        cls = int(rng.choice([0, 1, 3, 5, 6, 7, 8, 9, 15]))
        sx, sy = (int(v) for v in rng.integers(2, max(3, X // 22), 2))
        sz = int(rng.integers(1, max(2, Z // 2)))
        x0, y0 = int(rng.integers(X // 5, X - X // 5 - sx)), int(rng.integers(Y // 5, Y - Y // 5 - sy))
        gt[x0:x0 + sx, y0:y0 + sy, z0:z0 + sz] = cls
        if i % 4 == 3:
            continue
        dx, dy = (int(v) for v in rng.integers(-4, 5, 2)) if i % 4 == 1 else (0, 0)
        pred[x0 + dx:x0 + dx + sx, y0 + dy:y0 + dy + sy, z0:z0 + sz] = int(rng.choice([0, 1, 7])) if i % 4 == 2 else cls
    return pred, gt


def _bench(args):
    """Device-event medians of (a) render_views + render_bev and (b) the per-view loop over ext.dvr_render_forward with host
    colouring (tests/render_ref.py: the only way to the same images without the render kernel), alternating, in one process."""
    import json
    from . import synthetic
    try:
        from tests import render_ref
    except ImportError as e:
        raise SystemExit(f"--bench compares against tests/render_ref.py: run it from a checkout's root ({e})")
    cfg = synthetic.BASE
    pc_range, voxel = list(cfg['pc_range']), 0.4
    pred, _ = demo_grid(args.seed)
    metas = synthetic.make_img_metas(cfg, batch=1)
    r = OccRenderer(pc_range, voxel, size=tuple(args.size), device='cuda')
    sem = torch.from_numpy(pred)[None].cuda()
    g = torch.Generator().manual_seed(args.seed)
    frames_host = torch.randint(0, 256, (1, cfg['num_cams'], cfg['img_h'], cfg['img_w'], 3), generator=g, dtype=torch.uint8)
    frames = frames_host.cuda()
    cams_host = view_rays(metas, r.size)
    cams = cams_host.cuda()
    pal = default_palette()

    def new():
        v = r.views(sem, None, frames=frames, cams=cams)
        b = r.bev(sem)
        return v, b

    def loop():
        v = render_ref.views(pred, cams_host[0].numpy(), pc_range[:3], voxel, r.size, frames=frames_host[0].numpy(),
                             palette=pal, far=r.far, alpha=r.alpha, bg_rgb=r.bg_rgb)
        b = render_ref.bev(pred, palette=pal, bg_rgb=r.bg_rgb)
        return v, b

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    (_, (nv, nb)), (_, (lv, lb)) = timed(new), timed(loop)            # warm-up, and the two paths' images agree
    same = bool(np.array_equal(nv['rgb'][0].cpu().numpy(), lv['rgb']) and np.array_equal(nb['rgb'][0].cpu().numpy(), lb['rgb'])
                and np.array_equal(nv['depth'][0].cpu().numpy().view(np.uint32), lv['depth'].view(np.uint32)))
    t_new, t_loop = [], []
    for _ in range(5):
        t_new.append(timed(new)[0])
        t_loop.append(timed(loop)[0])
    line = dict(bench='occ_render', size=list(r.size), views=cfg['num_cams'], grid=list(pred.shape), images_equal=same,
                render_ms=float(np.median(t_new)), loop_ms=float(np.median(t_loop)),
                speedup=float(np.median(t_loop) / np.median(t_new)), share_of_5p6ms_step=float(np.median(t_new) / 5.6))
    if args.full_size:
        full = OccRenderer(pc_range, voxel, size=(cfg['img_h'], cfg['img_w']), device='cuda')
        cams_full = view_rays(metas, full.size).cuda()
        fn = lambda: (full.views(sem, None, frames=frames, cams=cams_full), full.bev(sem))      # noqa: E731
        timed(fn)
        line['render_full_size_ms'] = float(np.median([timed(fn)[0] for _ in range(5)]))
        line['full_size'] = list(full.size)
    print(json.dumps(line))
    return 0


def main(argv=None):
    import argparse
    from . import io as oio, synthetic
    ap = argparse.ArgumentParser(prog='python -m occnet_amd.vis', description=__doc__.split('\n\n')[0])
    ap.add_argument('grid', nargs='?', help='saved grid (io.save_occ_gt format); default: a seeded demo scene')
    ap.add_argument('--gt', help='ground truth in the same format: renders the agreement categories too')
    ap.add_argument('--out', default='vis_out', help='output directory')
    ap.add_argument('--size', type=int, nargs=2, default=(232, 400), metavar=('H', 'W'))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--bench', action='store_true', help='time the render against the per-view loop; one JSON line')
    ap.add_argument('--full-size', action='store_true', help='with --bench: add the 928 x 1600 figure')
    args = ap.parse_args(argv)
    if args.bench:
        return _bench(args)
    cfg = synthetic.BASE
    if args.grid:
        pred = oio.load_occ_gt(args.grid)[0]
        gt = oio.load_occ_gt(args.gt)[0] if args.gt else None
    else:
        pred, gt = demo_grid(args.seed)
    voxel = (cfg['pc_range'][3] - cfg['pc_range'][0]) / pred.shape[0]
    pc_range = list(cfg['pc_range'][:3]) + [cfg['pc_range'][k] + pred.shape[k] * voxel for k in range(3)]
    r = OccRenderer(pc_range, voxel, size=tuple(args.size), device='cuda')
    metas = synthetic.make_img_metas(cfg, batch=1)
    sem = torch.from_numpy(np.ascontiguousarray(pred))[None].cuda()
    written = []
    for name, g in (('mosaic', None),) + ((('diff', gt),) if gt is not None else ()):
        sg = None if g is None else torch.from_numpy(np.ascontiguousarray(g))[None].cuda()
        v, b = r.views(sem, metas, sem_gt=sg), r.bev(sem, sem_gt=sg)
        written.append(save_png(os.path.join(args.out, f'{name}.png'), r.mosaic(v['rgb'][0], b['rgb'][0])))
        if g is None:
            for k in range(v['rgb'].shape[1]):
                written.append(save_png(os.path.join(args.out, f'cam{k}.png'), v['rgb'][0, k]))
            written.append(save_png(os.path.join(args.out, 'bev.png'), torch.flip(b['rgb'][0], (0, 1))))
    print('\n'.join(written))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
