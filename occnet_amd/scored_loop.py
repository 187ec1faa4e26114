"""`test_loop.run_test` with the server's score of the rows it writes: model step -> `SubmissionWriter.add_scored`, nothing copied
to the host inside the loop.

`test_loop.run_test(model, samples, metric=None, writer=None)` feeds `RayMetrics` and / or a `SubmissionWriter`.  `run_test` here
takes the same arguments and a `score` (`metrics.SubmissionScore`): where a writer, a score and the sample's ground truth are all
there, `writer.add_scored(...)` takes the place of `writer.add(...)` — the same rows in the file, and what the challenge server
will give them.  Without a score it is `test_loop.run_test` itself."""
import torch

from . import test_loop


def _gt_grid(t, device, floating):
    t = torch.as_tensor(t)
    if floating:
        return t.to(device, torch.float32)
    if t.dtype not in (torch.uint8, torch.int64):
        t = t.to(torch.int64)
    return t.to(device)


def run_test(model, samples, metric=None, writer=None, score=None):
    """samples: the dicts of test_loop.run_test; `voxel_semantics` / `voxel_flow` (device tensors or anything
    RayMetrics.update takes) are needed with `metric` and used with `score`.  For every sample: `_, occ_cls, flow =
    model.simple_test(img_metas, img)`, `metric.update(...)` if a metric is given, then `writer.add_scored(token, occ_cls, flow,
    gt ..., lidar_origins, score)` — or `writer.add(...)` for a sample without ground truth.  No `.cpu()`, no synchronisation:
    the caller reads `score.compute()` / `metric.compute()` / `writer.write(prefix)` afterwards.  -> number of samples."""
    if score is None:
        return test_loop.run_test(model, samples, metric=metric, writer=writer)
    if writer is None:
        raise ValueError("run_test: a score needs a writer (it scores the writer's rows)")
    n = 0
    with torch.no_grad():
        for s in samples:
            _, occ_cls, flow = model.simple_test(s['img_metas'], s['img'])
            if metric is not None:
                metric.update(occ_cls, flow, s['voxel_semantics'], s['voxel_flow'], s['lidar_origins'])
            if s.get('voxel_semantics') is not None and s.get('voxel_flow') is not None:
                writer.add_scored(s['token'], occ_cls, flow, _gt_grid(s['voxel_semantics'], writer.device, False),
                                  _gt_grid(s['voxel_flow'], writer.device, True), s['lidar_origins'], score)
            else:
                writer.add(s['token'], occ_cls, flow, s['lidar_origins'])
            n += 1
    return n
