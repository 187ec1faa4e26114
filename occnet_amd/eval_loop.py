"""`test_loop.run_test` with one more consumer: the voxel mIoU over the voxels the cameras saw.

`run_test` here takes everything `test_loop.run_test` takes and, with `miou=` (metrics.VoxelMIoU), also feeds
`miou.update(occ_cls, gt, mask)` per sample from the same `model.simple_test` call — the mask being
`visibility(gt, img_metas)` with a `visibility` (visibility.CameraVisibility) and None, every voxel, without one.  Beside
other consumers the loop that runs is test_loop's, as it is: the model goes into it behind `_Tap`, which is the model in
every other respect and passes each `occ_cls` on.  With the mIoU as the only consumer, which that loop refuses, the samples
are walked here.

A sample may carry `img_u8` + `img_norm_cfg` (+ `img_scale`) instead of `img`: raw uint8 device frames, handed to
`model.simple_test(img_metas, img_u8=..., img_norm_cfg=..., img_scale=...)` under these names (with a scale the sample's metas
are those of the scaled images: io.scale_img_metas).  test_loop's loop reads `s['img']` and passes it on, so such a sample goes
into it with `img=None` and the same tap swaps the keywords in.  Without `miou` and without such samples this is
`test_loop.run_test`."""
import torch

from . import test_loop
from .metrics.device_common import class_grid


class _Tap:
    """The model with a tapped `simple_test`, which finds the sample whose `img_metas` the call was given: a sample that
    carries `img_u8` is handed to the model under its uint8 keywords, and with a `miou` the model's `occ_cls` goes to it with the
    sample's ground truth.  `watch` notes the samples by that object as the loop takes them, so it does not matter how far ahead
    of `simple_test` a loop takes samples; every other attribute is the model's own."""

    def __init__(self, model, miou=None, visibility=None):
        self._model, self._miou, self._visibility, self._taken = model, miou, visibility, {}

    def __getattr__(self, name):
        return getattr(self._model, name)

    def watch(self, samples):
        for s in samples:
            self._taken[id(s['img_metas'])] = s
            yield s if 'img' in s else dict(s, img=None)

    def simple_test(self, img_metas, img, **kw):
        s = self._taken.pop(id(img_metas))
        if 'img_u8' in s:
            kw.update(img_u8=s['img_u8'], img_norm_cfg=s['img_norm_cfg'], img_scale=s.get('img_scale'))
        out = self._model.simple_test(img_metas, img, **kw)
        sem_gt = s.get('voxel_semantics')
        if self._miou is not None and sem_gt is not None:
            miou, visibility = self._miou, self._visibility
            gt = class_grid('voxel_semantics', sem_gt, miou.occ_size, miou.device, convert=True)
            miou.update(out[1], gt, None if visibility is None else visibility(gt, img_metas))
        return out


def run_test(model, samples, metric=None, writer=None, score=None, renderer=None, out_dir=None, every=1, miou=None,
             visibility=None):
    """test_loop.run_test(model, samples, metric, writer, score, renderer, out_dir, every) — same samples, same consumers, same
    refusals, same return value — and for every sample that carries `voxel_semantics`, with `miou`,
    `miou.update(occ_cls, gt, mask)`.  `miou` may be the only consumer.  A sample may carry `img_u8`, `img_norm_cfg` and an
    optional `img_scale` instead of `img` (uint8 device frames; the module's docstring).  No `.cpu()`, no synchronisation: the caller reads
    `miou.compute()` afterwards."""
    if visibility is not None and miou is None:
        raise ValueError("run_test: a visibility needs a miou (it masks the miou's voxels)")
    others = dict(metric=metric, writer=writer, score=score, renderer=renderer, out_dir=out_dir, every=every)
    tap = _Tap(model, miou, visibility)
    if miou is None or any(c is not None for c in (metric, writer, score, renderer)):
        return test_loop.run_test(tap, tap.watch(samples), **others)
    n = 0
    with torch.no_grad():
        for s in tap.watch(samples):
            tap.simple_test(s['img_metas'], s['img'])
            n += 1
    return n
