"""What the device-resident evaluation classes share (RayMetrics, SubmissionScore, SubmissionWriter, vis.OccRenderer): the
grid geometry, the lidar rays on the device, "make this a (B, X, Y, Z) grid", the int64 state with its merge / all_reduce /
reset, and the ring of pinned host slots behind SubmissionWriter.add and OccRenderer.enqueue."""
import numpy as np
import torch


def occ_size(pc_range, voxel_size):
    """[X, Y, Z] voxels of pc_range = [x0, y0, z0, x1, y1, z1] at voxel_size."""
    return [int(round((float(pc_range[3 + k]) - float(pc_range[k])) / float(voxel_size))) for k in range(3)]


class DeviceRays:
    """The lidar rays (R, 3) float32 on `device`, copied there at the first call (None: generate_lidar_rays())."""

    def __init__(self, rays, device):
        from .ray_metrics import generate_lidar_rays
        self._host = generate_lidar_rays() if rays is None else rays
        self._device, self._dev = device, None

    def __call__(self):
        if self._dev is None:
            r = self._host
            r = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)) if isinstance(r, np.ndarray) else r
            self._dev = r.to(self._device, torch.float32).contiguous()
        return self._dev


def _need_device(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        from .. import ext
        raise ext.OccAmdError(f"{name} must be a device (HIP) tensor: the MI355X path has no CPU fallback")


def class_grid(name, t, size, device, B=None, convert=False):
    """-> contiguous (B, X, Y, Z) uint8 / int64 device tensor of class ids (size = [X, Y, Z]; B None: as many samples as t
    holds).  convert: t is anything torch.as_tensor takes, other integer types become int64 and host data moves to `device`;
    otherwise t must be a uint8 / int64 device tensor already (OccAmdError: there is no CPU fallback)."""
    if convert:
        t = torch.as_tensor(t)
        if t.dtype not in (torch.uint8, torch.int64):
            t = t.to(torch.int64)
        t = t.to(device)
    else:
        _need_device(name, t)
        if t.dtype not in (torch.uint8, torch.int64):
            from .. import ext
            raise ext.OccAmdError(f"{name} must be uint8 or int64, got {t.dtype}")
    return t.reshape([-1 if B is None else B] + list(size)).contiguous()


def flow_grid(name, t, size, device, B=None, convert=False):
    """-> contiguous (B, X, Y, Z, 2) device tensor of flow; convert as class_grid (to float32), otherwise a device tensor."""
    if convert:
        t = torch.as_tensor(t).to(device, torch.float32)
    else:
        _need_device(name, t)
    return t.reshape([-1 if B is None else B] + list(size) + [2]).contiguous()


class IntState:
    """`rows` x (free_id + 1) int64 words on the device and a grow-only byte workspace: partial states of batches or ranks add
    up exactly, in any order."""

    def __init__(self, rows, free_id, device):
        self.free_id = int(free_id)
        self.ncls = self.free_id + 1
        self.device = torch.device(device)
        self._workspace = None
        self.state = torch.zeros(rows * self.ncls, dtype=torch.int64, device=self.device)

    def _grown_workspace(self, nbytes):
        need = max(nbytes, 256)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def merge(self, other):
        """Add another state of the same classes: integer addition, exact in any order."""
        if other.state.numel() != self.state.numel():
            raise ValueError(f"{type(self).__name__}.merge: states of different class counts")
        self.state += other.state.to(self.state.device)
        return self

    def all_reduce(self):
        """Sum the state over the ranks of the default process group (no-op without one)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.state, op=dist.ReduceOp.SUM)
        return self

    def reset(self):
        self.state.zero_()
        return self


class _Slot:
    """One in-flight batch: named grow-only buffers (device, or pinned host), the event that marks its copies, and what
    `finish` needs to read them back."""

    def __init__(self):
        self._buffers = {}
        self.event = None
        self.pending = None

    def grown(self, name, n, **kw):
        """Buffer `name` with at least n elements (torch.empty(n, **kw) when it has to grow)."""
        t = self._buffers.get(name)
        if t is None or t.numel() < n:
            t = self._buffers[name] = torch.empty(n, **kw)
        return t


class SlotRing:
    """`depth` slots used round-robin.  A slot is read back — event.synchronize(), then finish(pending) -> (token,
    result) pairs — only when it is about to be reused or when everything is drained, so the host never waits for the batch it
    has just enqueued."""

    def __init__(self, owner, depth, finish):
        if int(depth) < 1:
            raise ValueError(f"{owner}: depth must be at least 1")
        self._slots = [_Slot() for _ in range(int(depth))]
        self._next = 0
        self._finish = finish
        self._tokens = set()
        self._results = {}

    def claim(self, caller, tokens):
        """-> the list of tokens (a single str is one sample), none of them seen before."""
        tokens = [tokens] if isinstance(tokens, str) else list(tokens)
        if len(set(tokens)) != len(tokens) or any(t in self._tokens for t in tokens):
            dup = sorted({t for t in tokens if t in self._tokens or tokens.count(t) > 1})
            raise ValueError(f"{caller}: duplicate token(s) {dup}")
        return tokens

    def take(self):
        """The next slot, read back if a batch is still in it: the one wait of an enqueue."""
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        self._drain(slot)
        return slot

    def record(self, slot, tokens, pending):
        """Mark the end of the slot's copies on the current stream; `pending` goes to `finish` when the slot is read."""
        slot.event = torch.cuda.Event()
        slot.event.record()
        slot.pending = pending
        self._tokens.update(tokens)

    def _drain(self, slot):
        if slot.pending is None:
            return
        slot.event.synchronize()
        self._results.update(self._finish(slot.pending))
        slot.pending = None

    def results(self):
        """Wait for every enqueued batch, oldest first -> {token: result} in the order the samples were enqueued."""
        n = len(self._slots)
        for k in range(n):
            self._drain(self._slots[(self._next + k) % n])
        return self._results

    def reset(self):
        """Forget every sample (waiting for the enqueued ones first); the slots' buffers are kept."""
        self.results()
        self._tokens, self._results = set(), {}
