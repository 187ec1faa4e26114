"""The test-split loop: model step -> device-resident scoring and / or submission rows, nothing copied to the host inside it.

`run_test` is the counterpart of `train.train_step` for evaluation and submission runs: `forward_test` copies 10 MB of int64
classes and float32 flow to the host per sample for the reference's host-side consumers; here the model's `occ_cls` and `flow`
stay on the device and go straight into `metrics.RayMetrics.update` (two launches) and `metrics.SubmissionWriter.add` (two
launches and one non-blocking copy of the packed rows)."""
import torch


def run_test(model, samples, metric=None, writer=None):
    """samples: iterable of dicts
        token            sample token (needed with `writer`)
        img_metas, img   what model.simple_test(img_metas, img) takes
        lidar_origins    (1, T, 3) lidar origins in ego metres (io.lidar_origins)
        voxel_semantics, voxel_flow   ground truth (needed with `metric`): device tensors or anything RayMetrics.update takes
    For every sample: `_, occ_cls, flow = model.simple_test(img_metas, img)`, then `metric.update(occ_cls, flow, gt ...)`
    and / or `writer.add(token, occ_cls, flow, lidar_origins)` on the device tensors as they are.  No `.cpu()`, no
    synchronisation: the caller reads `metric.compute()` / `writer.write(prefix)` afterwards.  -> number of samples."""
    if metric is None and writer is None:
        raise ValueError("run_test: give a metric, a writer or both")
    n = 0
    with torch.no_grad():
        for s in samples:
            _, occ_cls, flow = model.simple_test(s['img_metas'], s['img'])
            if metric is not None:
                metric.update(occ_cls, flow, s['voxel_semantics'], s['voxel_flow'], s['lidar_origins'])
            if writer is not None:
                writer.add(s['token'], occ_cls, flow, s['lidar_origins'])
            n += 1
    return n
