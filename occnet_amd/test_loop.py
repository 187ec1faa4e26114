"""The test-split loop: model step -> device-resident scoring, submission rows, the server's score of those rows and pictures,
nothing copied to the host inside it.

`run_test` is the counterpart of `train.train_step` for evaluation and submission runs: `forward_test` copies 10 MB of int64
classes and float32 flow to the host per sample for the reference's host-side consumers; here the model's `occ_cls` and `flow`
stay on the device and go straight into `metrics.RayMetrics.update` (two launches), `metrics.SubmissionWriter.add` (two
launches and one non-blocking copy of the packed rows) — or `add_scored`, which also hands the rows to a
`metrics.SubmissionScore` — and `vis.OccRenderer.enqueue` (camera views and a BEV, with the renderer's own non-blocking copies)."""
import os

import torch

from .metrics.device_common import class_grid, flow_grid


def run_test(model, samples, metric=None, writer=None, score=None, renderer=None, out_dir=None, every=1):
    """samples: iterable of dicts
        token            sample token (needed with `writer`; names the picture)
        img_metas, img   what model.simple_test(img_metas, img) takes
        lidar_origins    (1, T, 3) lidar origins in ego metres (io.lidar_origins)
        voxel_semantics, voxel_flow   ground truth (needed with `metric`, used with `score` and `renderer`): device tensors or
                         anything RayMetrics.update takes
        frames           optional (1, V, Hs, Ws, 3) uint8: the frames the model was fed, drawn under the rendering
    For every sample: `_, occ_cls, flow = model.simple_test(img_metas, img)` once, then on the device tensors as they are
      * every `every`-th sample `renderer.enqueue(token, occ_cls, img_metas, ...)` — with `voxel_semantics` the picture holds
        the agreement categories;
      * `metric.update(occ_cls, flow, gt ...)`;
      * `writer.add_scored(token, occ_cls, flow, gt ..., lidar_origins, score)` where a writer, a score and the sample's ground
        truth are all there, otherwise `writer.add(token, occ_cls, flow, lidar_origins)`.
    No `.cpu()`, no synchronisation: the caller reads `metric.compute()` / `score.compute()` / `writer.write(prefix)` /
    `renderer.results()` afterwards.  out_dir: write `<out_dir>/<token>.png` (renderer.mosaic) for each rendered sample, after
    the loop.  -> number of samples."""
    if score is not None and writer is None:
        raise ValueError("run_test: a score needs a writer (it scores the writer's rows)")
    if metric is None and writer is None and renderer is None:
        raise ValueError("run_test: give a metric, a writer, a renderer or several of them")
    every = max(1, int(every))
    n = 0
    with torch.no_grad():
        for s in samples:
            _, occ_cls, flow = model.simple_test(s['img_metas'], s['img'])
            sem_gt, flow_gt = s.get('voxel_semantics'), s.get('voxel_flow')
            if renderer is not None and n % every == 0:
                gt = None if sem_gt is None else class_grid('voxel_semantics', sem_gt, renderer.occ_size, renderer.device,
                                                            convert=True)
                renderer.enqueue(s.get('token', f'sample{n}'), occ_cls, s['img_metas'], frames=s.get('frames'), sem_gt=gt)
            if metric is not None:
                metric.update(occ_cls, flow, s['voxel_semantics'], s['voxel_flow'], s['lidar_origins'])
            if writer is not None and score is not None and sem_gt is not None and flow_gt is not None:
                writer.add_scored(s['token'], occ_cls, flow,
                                  class_grid('voxel_semantics', sem_gt, writer.occ_size, writer.device, convert=True),
                                  flow_grid('voxel_flow', flow_gt, writer.occ_size, writer.device, convert=True),
                                  s['lidar_origins'], score)
            elif writer is not None:
                writer.add(s['token'], occ_cls, flow, s['lidar_origins'])
            n += 1
    if renderer is not None and out_dir is not None:
        from .vis import save_png
        for tok, res in renderer.results().items():
            save_png(os.path.join(out_dir, f'{tok}.png'),
                     renderer.mosaic(torch.from_numpy(res['views']), torch.from_numpy(res['bev']),
                                     layout=_layout(res['views'].shape[0])))
    return n


def _layout(V):
    """six cameras: front-left, front, front-right over back-left, back, back-right; otherwise one row"""
    return ((2, 0, 1), (4, 3, 5)) if V == 6 else (tuple(range(V)),)
