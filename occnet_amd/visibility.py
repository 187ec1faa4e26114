"""Camera visibility masks: which voxels of a class grid the cameras of a sample can see (csrc/visibility.hip).

`BEVFormerOccHead(use_mask=True)` averages its cross-entropy over the voxels of `mask_camera`, and a per-class voxel IoU
(metrics.VoxelMIoU) only means something over the voxels the cameras observed — but the challenge's ground-truth files carry
`semantics` and `flow` alone.  `CameraVisibility` makes the mask from what a sample does carry: the ground-truth grid and the
`img_metas` the model already takes.  A voxel is seen when a pixel ray of one of the cameras (vis.view_rays: the rays
`vis.OccRenderer` renders) passes through it before the first occupied voxel stops the ray, that voxel included.  Lidar
visibility (`mask_lidar`, which the model does not use) is not built.

    python -m occnet_amd.visibility --bench          # one JSON line: mask vs. render at two rasters, and the confusion counts
"""
import numpy as np
import torch

from .metrics.device_common import class_grid, occ_size
from .vis import view_rays


class CameraVisibility:
    def __init__(self, pc_range, voxel_size, free_id=16, size=(464, 800), far=100., device='cuda'):
        """size = (h, w) of the raster of pixel rays per camera — half the 928 x 1600 frames by default: at base geometry the
        renderer's default (232, 400) under-samples the far field, 2.6 % of the marked voxels differ between the two rasters
        (DESIGN.md 11d); far in metres scales the ray directions as the renderer's does (the walk is not cut there)."""
        self.pc_range = [float(v) for v in pc_range]
        self.voxel_size = float(voxel_size)
        self.free_id = int(free_id)
        self.occ_size = occ_size(self.pc_range, self.voxel_size)
        self.size = (int(size[0]), int(size[1]))
        self.far = float(far)
        self.device = torch.device(device)
        self._workspace = None

    def _grown_workspace(self, nbytes):
        need = max(nbytes, 256)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def __call__(self, sem_gt, img_metas, out=None, cams=None):
        """sem_gt: B class grids, anything class_grid accepts (host data is moved to the device); img_metas: B dicts
        (vis.view_rays), or cams (B, V, 12) float32 on the device in their place -> mask_camera (B, X, Y, Z) uint8 on the
        device.  Three launches on the current stream, no synchronisation."""
        from . import ext
        sem = class_grid('sem_gt', sem_gt, self.occ_size, self.device, convert=True)
        if cams is None:
            cams = view_rays(img_metas, self.size).to(self.device)
        B, X, Y, Z = sem.shape
        return ext.visibility_views(sem, cams, self.pc_range[:3], self.voxel_size, self.size, free_id=self.free_id,
                                    far=self.far, out=out,
                                    workspace=self._grown_workspace(ext.visibility_workspace_bytes(B, X, Y, Z)))


# ---- command line -----------------------------------------------------------------------------------------------------------
def _bench(args):
    """Device-event medians at base geometry (vis.demo_grid, 200 x 200 x 16, B = 1, the synthetic six-camera rig): the mask at
    two rasters, each beside render_views(want=('label',)) on the same inputs and rays — the same traversal without the
    marking —, the share of voxels whose mark differs between the rasters, and the confusion counts over 640 000 voxels."""
    import json
    from . import ext, synthetic
    from .vis import OccRenderer, demo_grid
    cfg = synthetic.BASE
    pc_range, voxel = list(cfg['pc_range']), 0.4
    pred, gt = demo_grid(args.seed)
    metas = synthetic.make_img_metas(cfg, batch=1)
    sem = torch.from_numpy(gt)[None].cuda()
    sem_pred = torch.from_numpy(pred)[None].cuda()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def median_ms(fn):
        timed(fn)                                                        # warm-up
        return float(np.median([timed(fn)[0] for _ in range(5)]))

    line = dict(bench='visibility', grid=list(gt.shape), views=cfg['num_cams'])
    masks = {}
    for size in ((232, 400), (464, 800)):
        cv = CameraVisibility(pc_range, voxel, size=size, device='cuda')
        r = OccRenderer(pc_range, voxel, size=size, device='cuda')
        cams = view_rays(metas, size).cuda()
        out = torch.empty(sem.shape, dtype=torch.uint8, device='cuda')
        ws = torch.empty(ext.render_workspace_bytes(*sem.shape), dtype=torch.uint8, device='cuda')
        label = {'label': torch.empty((1, cfg['num_cams']) + size, dtype=torch.uint8, device='cuda')}
        t_vis = median_ms(lambda: cv(sem, None, out=out, cams=cams))
        t_render = median_ms(lambda: r.views(sem, None, want=('label',), out=label, workspace=ws, cams=cams))
        masks[size] = out.clone()
        key = f'{size[0]}x{size[1]}'
        line[f'visibility_ms_{key}'] = t_vis
        line[f'render_label_ms_{key}'] = t_render
        line[f'ratio_{key}'] = t_vis / t_render
        line[f'marked_share_{key}'] = float(masks[size].float().mean())
    lo, hi = masks[(232, 400)], masks[(464, 800)]
    differ = int((lo != hi).sum())
    line['marks_differ'] = differ
    line['marks_differ_share_of_marked'] = differ / max(1, int(hi.sum()))
    state = torch.zeros(ext.confusion_state_words(16), dtype=torch.int64, device='cuda')
    line['confusion_ms'] = median_ms(lambda: ext.confusion_accumulate(state, sem_pred, sem, mask=lo, free_id=16))
    line['confusion_voxels'] = int(sem.numel())
    line['confusion_bytes_read'] = int(sem.numel() * 3)                  # two uint8 grids and the mask
    print(json.dumps(line))
    return 0


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m occnet_amd.visibility', description=__doc__.split('\n\n')[0])
    ap.add_argument('--bench', action='store_true', help='time the mask against the renderer; one JSON line')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    if not args.bench:
        ap.error('nothing to do: give --bench')
    return _bench(args)


if __name__ == '__main__':
    raise SystemExit(main())
