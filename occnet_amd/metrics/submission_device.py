"""submission.gz rows with the ray cast, the class / flow look-up and the int8 / float16 packing on the device
(csrc/submission_rays.hip).

`io.format_submission` mirrors the reference's host loop: per sample and per lidar origin it builds a float occupancy grid on
the host, uploads it, launches the ray caster, copies the hit voxels back with a synchronising copy and indexes class and flow
in numpy.  `SubmissionWriter` takes the model's outputs as device tensors, runs ONE launch pair per batch that writes the rows
already in the file's types into one packed buffer, and copies that buffer (7 bytes per ray) into a pinned host slot without
blocking.  A slot is read — `event.synchronize()`, then per-sample numpy slices — only when it is about to be reused, so with
`depth` slots the host never waits for the batch it has just enqueued.

Origins keep their type: float64 origins (what `io.lidar_origins` returns, and what `process_one_sample` then computes in) are
converted to voxel units in float64 on the device, float32 origins in float32 — the file is the one `io.format_submission`
writes, bit for bit.
"""
import gzip
import os
import pickle

import torch

from .device_common import DeviceRays, SlotRing, class_grid, flow_grid, occ_size


class SubmissionWriter:
    def __init__(self, pc_range, voxel_size, free_id=16, rays=None, device='cuda', depth=2):
        self.pc_range = [float(v) for v in pc_range]
        self.voxel_size = float(voxel_size)
        self.free_id = int(free_id)
        self.occ_size = occ_size(self.pc_range, self.voxel_size)
        self.device = torch.device(device)
        # a slot: packed device buffer `dev` (and the ground truth's `dev_gt`, for add_scored), mask `workspace`, pinned `host`
        # copy, pinned staging of `origins` and `counts`
        self._ring = SlotRing("SubmissionWriter", depth, self._finish)
        self._rays_dev = DeviceRays(rays, self.device)

    # ---- accumulation ------------------------------------------------------------------------------------------------
    def add(self, tokens, sem_pred, flow_pred, lidar_origins, origin_counts=None):
        """Enqueue a batch.  tokens: one per sample (a single str for one sample); sem_pred (B, X, Y, Z) uint8 / int64 — or any
        shape with X*Y*Z elements per sample —, flow_pred (B, X, Y, Z, 2) float32: device tensors, used as they are;
        lidar_origins (B, T, 3) float32 or float64 ego metres (T <= 8; host or device); origin_counts: None (every sample has
        T origins) or a HOST list of B ints in 1..T.  Two kernels, one non-blocking copy into a pinned slot, one event; the
        call waits only for the slot it is about to reuse (the batch enqueued `depth` calls ago)."""
        self._enqueue(tokens, sem_pred, flow_pred, lidar_origins, origin_counts)

    def add_scored(self, tokens, sem_pred, flow_pred, sem_gt, flow_gt, lidar_origins, score, origin_counts=None):
        """`add`, and the score the server will give these rows: the prediction's rows go exactly as in `add`; the ground truth
        (sem_gt, flow_gt: as sem_pred, flow_pred) goes through the same ext.submission_rays into a second device buffer of the
        slot, and `score` (metrics.SubmissionScore) takes both packed buffers in one update_packed.  Two more launch
        pairs (cast, score), nothing more copied, no synchronisation."""
        self._enqueue(tokens, sem_pred, flow_pred, lidar_origins, origin_counts, gt=(sem_gt, flow_gt), score=score)

    def _enqueue(self, tokens, sem_pred, flow_pred, lidar_origins, origin_counts, gt=None, score=None):
        from .. import ext
        tokens = self._ring.claim("SubmissionWriter.add", tokens)
        B = len(tokens)
        sem_pred = class_grid("sem_pred", sem_pred, self.occ_size, self.device, B)
        flow_pred = flow_grid("flow_pred", flow_pred, self.occ_size, self.device, B)
        if gt is not None:
            if score is None or score.free_id != self.free_id:
                raise ValueError("SubmissionWriter.add_scored: score must be a SubmissionScore of the writer's free_id")
            sem_gt = class_grid("sem_gt", gt[0], self.occ_size, self.device, B)
            flow_gt = flow_grid("flow_gt", gt[1], self.occ_size, self.device, B)
        origins = torch.as_tensor(lidar_origins)
        if origins.dtype not in (torch.float32, torch.float64):
            origins = origins.to(torch.float64)
        origins = origins.reshape(B, -1, 3)
        Tmax = origins.shape[1]
        if not 1 <= Tmax <= 8:
            raise ValueError(f"SubmissionWriter.add: origins per sample must be 1..8, got {Tmax}")
        if origin_counts is None:
            counts = [Tmax] * B
        else:
            counts = [int(c) for c in origin_counts]
            if len(counts) != B or any(c < 1 or c > Tmax for c in counts):
                raise ValueError(f"SubmissionWriter.add: origin_counts must be {B} ints in 1..{Tmax}, got {counts}")
        rays = self._rays_dev()
        R = rays.shape[0]
        X, Y, Z = self.occ_size
        slot = self._ring.take()
        nbytes = ext.submission_rays_bytes(B, Tmax, R)
        dev = self.device
        packed = slot.grown('dev', nbytes, dtype=torch.uint8, device=dev)
        workspace = slot.grown('workspace', max(ext.submission_rays_workspace_bytes(B, X, Y, Z), 256), dtype=torch.uint8,
                               device=dev)
        host = slot.grown('host', nbytes, dtype=torch.uint8, pin_memory=True)
        counts_host = slot.grown('counts', B, dtype=torch.int32, pin_memory=True)
        counts_host[:B] = torch.tensor(counts, dtype=torch.int32)
        counts_dev = counts_host[:B].to(dev, non_blocking=True)
        if not origins.is_cuda:                      # staged through the slot's pinned memory: the upload does not block
            staging = slot.grown('origins', B * Tmax * 3, dtype=torch.float64, pin_memory=True)
            staged = staging[:B * Tmax * 3].view(B, Tmax, 3) if origins.dtype == torch.float64 else \
                staging.view(torch.float32)[:B * Tmax * 3].view(B, Tmax, 3)
            staged.copy_(origins)
            origins = staged.to(dev, non_blocking=True)
        ext.submission_rays(sem_pred, flow_pred, origins.contiguous(), rays, self.pc_range[:3], self.voxel_size, self.free_id,
                            origin_counts=counts_dev, out=packed, workspace=workspace)
        if gt is not None:                           # same stream: the masks' workspace is free again when this cast starts
            packed_gt = slot.grown('dev_gt', nbytes, dtype=torch.uint8, device=dev)
            ext.submission_rays(sem_gt, flow_gt, origins.contiguous(), rays, self.pc_range[:3], self.voxel_size, self.free_id,
                                origin_counts=counts_dev, out=packed_gt, workspace=workspace)
            score.update_packed(packed, packed_gt, B, Tmax, R, counts_dev * R)
        host[:nbytes].copy_(packed[:nbytes], non_blocking=True)
        self._ring.record(slot, tokens, (tokens, counts, host, B, Tmax, R))

    @staticmethod
    def _finish(pending):
        from .. import ext
        tokens, counts, host, B, Tmax, R = pending
        cls, dist, flow = (v.numpy() for v in ext.submission_rays_views(host, B, Tmax, R))
        for b, (tok, n) in enumerate(zip(tokens, counts)):
            yield tok, {'pcd_cls': cls[b, :n].reshape(-1).copy(), 'pcd_dist': dist[b, :n].reshape(-1).copy(),
                        'pcd_flow': flow[b, :n].reshape(-1, 2).copy()}

    # ---- output ------------------------------------------------------------------------------------------------------
    def results(self):
        """Wait for every enqueued batch -> {token: {pcd_cls int8 (T*R), pcd_dist float16 (T*R), pcd_flow float16 (T*R, 2)}}
        in the order the samples were added."""
        return self._ring.results()

    def reset(self):
        """Forget every sample (waiting for the enqueued ones first); the slots' buffers are kept."""
        self._ring.reset()
        return self

    def write(self, submission_prefix, header=None):
        """`<prefix>/submission.gz` exactly as io.format_submission writes it -> path."""
        from ..io import write_submission
        return write_submission(self.results(), submission_prefix, header)

    def save_part(self, path):
        """This rank's results (a pickled {token: rows} dict in insertion order) for io.merge_submission_parts."""
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, 'wb') as f:
            f.write(gzip.compress(pickle.dumps(self.results()), mtime=0))
        return path
