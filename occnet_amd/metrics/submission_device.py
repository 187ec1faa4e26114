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

import numpy as np
import torch

from .ray_metrics import generate_lidar_rays


class _Slot:
    """One in-flight batch: packed device buffer (and the ground truth's, for add_scored), mask workspace, pinned host copy, pinned staging of origins and counts."""

    def __init__(self):
        self.dev = self.dev_gt = self.workspace = self.host = self.origins = self.counts = None
        self.event = None
        self.pending = None          # (tokens, counts, B, Tmax, R) of the batch whose copy `event` marks


def _grown(t, n, **kw):
    return t if t is not None and t.numel() >= n else torch.empty(n, **kw)


class SubmissionWriter:
    def __init__(self, pc_range, voxel_size, free_id=16, rays=None, device='cuda', depth=2):
        self.pc_range = [float(v) for v in pc_range]
        self.voxel_size = float(voxel_size)
        self.free_id = int(free_id)
        self.occ_size = [int(round((self.pc_range[3 + k] - self.pc_range[k]) / self.voxel_size)) for k in range(3)]
        self.device = torch.device(device)
        if int(depth) < 1:
            raise ValueError("SubmissionWriter: depth must be at least 1")
        self._rays_host = generate_lidar_rays() if rays is None else rays
        self._rays = None
        self._slots = [_Slot() for _ in range(int(depth))]
        self._next = 0
        self._tokens = set()
        self._results = {}

    def _rays_dev(self):
        if self._rays is None:
            r = self._rays_host
            r = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)) if isinstance(r, np.ndarray) else r
            self._rays = r.to(self.device, torch.float32).contiguous()
        return self._rays

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
        tokens = [tokens] if isinstance(tokens, str) else list(tokens)
        B = len(tokens)
        if len(set(tokens)) != B or any(t in self._tokens for t in tokens):
            dup = sorted({t for t in tokens if t in self._tokens or tokens.count(t) > 1})
            raise ValueError(f"SubmissionWriter.add: duplicate token(s) {dup}")
        grids = (("sem_pred", sem_pred), ("flow_pred", flow_pred)) + \
            ((("sem_gt", gt[0]), ("flow_gt", gt[1])) if gt is not None else ())
        for name, t in grids:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ext.OccAmdError(f"{name} must be a device (HIP) tensor: the MI355X path has no CPU fallback")
        for name, t in grids[::2]:
            if t.dtype not in (torch.uint8, torch.int64):
                raise ext.OccAmdError(f"{name} must be uint8 or int64, got {t.dtype}")
        sem_pred = sem_pred.reshape([B] + self.occ_size).contiguous()
        flow_pred = flow_pred.reshape([B] + self.occ_size + [2]).contiguous()
        if gt is not None:
            if score is None or score.free_id != self.free_id:
                raise ValueError("SubmissionWriter.add_scored: score must be a SubmissionScore of the writer's free_id")
            sem_gt = gt[0].reshape([B] + self.occ_size).contiguous()
            flow_gt = gt[1].reshape([B] + self.occ_size + [2]).contiguous()
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
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        self._drain(slot)
        nbytes = ext.submission_rays_bytes(B, Tmax, R)
        dev = self.device
        slot.dev = _grown(slot.dev, nbytes, dtype=torch.uint8, device=dev)
        slot.workspace = _grown(slot.workspace, max(ext.submission_rays_workspace_bytes(B, X, Y, Z), 256), dtype=torch.uint8,
                                device=dev)
        slot.host = _grown(slot.host, nbytes, dtype=torch.uint8, pin_memory=True)
        slot.counts = _grown(slot.counts, B, dtype=torch.int32, pin_memory=True)
        slot.counts[:B] = torch.tensor(counts, dtype=torch.int32)
        counts_dev = slot.counts[:B].to(dev, non_blocking=True)
        if not origins.is_cuda:                      # staged through the slot's pinned memory: the upload does not block
            slot.origins = _grown(slot.origins, B * Tmax * 3, dtype=torch.float64, pin_memory=True)
            staged = slot.origins[:B * Tmax * 3].view(B, Tmax, 3) if origins.dtype == torch.float64 else \
                slot.origins.view(torch.float32)[:B * Tmax * 3].view(B, Tmax, 3)
            staged.copy_(origins)
            origins = staged.to(dev, non_blocking=True)
        ext.submission_rays(sem_pred, flow_pred, origins.contiguous(), rays, self.pc_range[:3], self.voxel_size, self.free_id,
                            origin_counts=counts_dev, out=slot.dev, workspace=slot.workspace)
        if gt is not None:                           # same stream: the masks' workspace is free again when this cast starts
            slot.dev_gt = _grown(slot.dev_gt, nbytes, dtype=torch.uint8, device=dev)
            ext.submission_rays(sem_gt, flow_gt, origins.contiguous(), rays, self.pc_range[:3], self.voxel_size, self.free_id,
                                origin_counts=counts_dev, out=slot.dev_gt, workspace=slot.workspace)
            score.update_packed(slot.dev, slot.dev_gt, B, Tmax, R, counts_dev * R)
        slot.host[:nbytes].copy_(slot.dev[:nbytes], non_blocking=True)
        slot.event = torch.cuda.Event()
        slot.event.record()
        slot.pending = (tokens, counts, B, Tmax, R)
        self._tokens.update(tokens)

    def _drain(self, slot):
        if slot.pending is None:
            return
        from .. import ext
        tokens, counts, B, Tmax, R = slot.pending
        slot.event.synchronize()
        cls, dist, flow = (v.numpy() for v in ext.submission_rays_views(slot.host, B, Tmax, R))
        for b, (tok, n) in enumerate(zip(tokens, counts)):
            self._results[tok] = {'pcd_cls': cls[b, :n].reshape(-1).copy(), 'pcd_dist': dist[b, :n].reshape(-1).copy(),
                                  'pcd_flow': flow[b, :n].reshape(-1, 2).copy()}
        slot.pending = None

    # ---- output ------------------------------------------------------------------------------------------------------
    def results(self):
        """Wait for every enqueued batch -> {token: {pcd_cls int8 (T*R), pcd_dist float16 (T*R), pcd_flow float16 (T*R, 2)}}
        in the order the samples were added."""
        n = len(self._slots)
        for k in range(n):                           # oldest batch first: the dict keeps insertion order
            self._drain(self._slots[(self._next + k) % n])
        return self._results

    def reset(self):
        """Forget every sample (waiting for the enqueued ones first); the slots' buffers are kept."""
        self.results()
        self._tokens, self._results = set(), {}
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
