"""`scored_loop.run_test` with pictures: model step -> metric / writer / score as there, and the prediction rendered into camera
views and a BEV by a `vis.OccRenderer`, nothing copied to the host inside the loop but the renderer's own non-blocking copies.

`run_test` here takes the arguments of `scored_loop.run_test` and a `renderer`; without one it is `scored_loop.run_test` itself.
The model runs once per sample: the loop underneath calls `simple_test` through a thin proxy that hands `occ_cls`, the sample's
metas and its optional uint8 `frames` and ground truth to `renderer.enqueue` before returning the model's outputs unchanged."""
import os

import torch

from . import scored_loop


class _Tap:
    """simple_test of the wrapped model, plus renderer.enqueue for every `every`-th sample."""

    def __init__(self, model, renderer, every):
        self.model, self.renderer, self.every = model, renderer, max(1, int(every))
        self.sample, self.n = None, 0

    def samples(self, samples):
        for s in samples:
            self.sample = s
            yield s

    def simple_test(self, img_metas, img):
        out = self.model.simple_test(img_metas, img)
        s, k = self.sample, self.n
        self.n += 1
        if k % self.every == 0:
            gt = s.get('voxel_semantics')
            if gt is not None:
                gt = scored_loop._gt_grid(gt, self.renderer.device, False)
            self.renderer.enqueue(s.get('token', f'sample{k}'), out[1], img_metas, frames=s.get('frames'), sem_gt=gt)
        return out


def run_test(model, samples, metric=None, writer=None, score=None, renderer=None, out_dir=None, every=1):
    """samples: the dicts of scored_loop.run_test, each optionally with `frames` ((1, V, Hs, Ws, 3) uint8: the frames the model
    was fed, drawn under the rendering) — `voxel_semantics`, where present, turns the rendering into the agreement categories.
    Every `every`-th sample is rendered.  out_dir: write `<out_dir>/<token>.png` (renderer.mosaic) for each rendered sample,
    after the loop.  Without metric, writer and score the loop only renders.  -> number of samples."""
    if renderer is None:
        return scored_loop.run_test(model, samples, metric=metric, writer=writer, score=score)
    tap = _Tap(model, renderer, every)
    if metric is None and writer is None:
        if score is not None:
            raise ValueError("run_test: a score needs a writer (it scores the writer's rows)")
        n = 0
        with torch.no_grad():
            for s in tap.samples(samples):
                tap.simple_test(s['img_metas'], s['img'])
                n += 1
    else:
        n = scored_loop.run_test(tap, tap.samples(samples), metric=metric, writer=writer, score=score)
    if out_dir is not None:
        from .vis import save_png
        for tok, res in renderer.results().items():
            save_png(os.path.join(out_dir, f'{tok}.png'),
                     renderer.mosaic(torch.from_numpy(res['views']), torch.from_numpy(res['bev']),
                                     layout=_layout(res['views'].shape[0])))
    return n


def _layout(V):
    """six cameras: front-left, front, front-right over back-left, back, back-right; otherwise one row"""
    return ((2, 0, 1), (4, 3, 5)) if V == 6 else (tuple(range(V)),)
