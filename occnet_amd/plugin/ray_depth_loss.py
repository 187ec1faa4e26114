"""Ray-depth supervision: the expected depth of lidar-like rays through the predicted occupancy, against the depth at which
the same rays hit the ground truth — the quantity RayIoU scores (class and depth within 1 / 2 / 4 m), which the voxel losses
do not see.  Opt-in: `loss_depth=dict(type='RayDepthLoss', ...)` in the head's config.

  DvrRenderLoss   autograd node over ext.dvr_render (csrc/dvr_render_train.hip): the kernel returns the depths and the
                  analytic gradient of the summed loss in one pass, backward scales it
  RayDepthLoss    logits -> density -> DvrRenderLoss; pseudo-lidar targets from the ground-truth grid

Everything stays on the device: no host synchronisation (the count of rendered rays is a 0-d device tensor).
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .registry import LOSSES


def _ulp(t):
    """Spacing of the float32 values in t (np.spacing of |t|), same dtype."""
    _, e = torch.frexp(t)
    return torch.ldexp(torch.ones_like(t), e - 24)


def end_points_at(origin, end, dist):
    """The float32 points p on the rays origin -> end (origin (B, 1, 3), end (B, R, 3), voxel units) with |p - origin| = dist
    (B, R) to half a float32 ulp OF THE DISTANCE — the renderer's target is that norm, taken in double from the float32
    coordinates.  Rounding origin + dir * dist alone does not give it: a coordinate near 25 has an ulp of 1.9e-6, a distance
    of 2 one of 2.4e-7 (measured: one ray in five beyond one ulp, the worst 12 ulp).  So 82 float32 candidates around the
    rounded point are tried: for each axis, the two other coordinates moved by -1, 0, +1 ulp and the axis solved from
    dist^2 - (the others)^2, with its float32 neighbours; of those within half an ulp the one nearest the exact point is
    taken (measured: all of 24 596 rays of two scenes within half an ulp, at most 7e-4 voxels off the ray), the best one
    otherwise."""
    o64 = origin.double()
    d64 = end.double() - o64
    D = dist.double()
    ideal = o64 + d64 / d64.norm(dim=-1, keepdim=True) * D[..., None]
    p0 = ideal.float()
    step = _ulp(p0).double()
    k = torch.tensor([(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)], dtype=torch.float64, device=end.device)     # (9, 2)
    cands = [p0[..., None, :].double()]
    for ax in range(3):
        oth = [a for a in range(3) if a != ax]
        cand = p0[..., None, :].double().repeat(1, 1, 9, 1)                                   # (B, R, 9, 3)
        for j, a in enumerate(oth):
            cand[..., a] = (p0[..., a].double()[..., None] + k[:, j] * step[..., a][..., None]).float().double()
        r = cand - o64[..., None, :]
        rest = (D[..., None] ** 2 - r[..., oth[0]] ** 2 - r[..., oth[1]] ** 2).clamp(min=0)
        sign = torch.where(d64[..., ax] >= 0, 1.0, -1.0)[..., None]
        solved = (o64[..., None, ax] + sign * rest.sqrt()).float()
        for dz in (-1.0, 0.0, 1.0):
            c = cand.clone()
            c[..., ax] = (solved.double() + dz * _ulp(solved).double()).float().double()
            cands.append(c)
    c = torch.cat(cands, 2)                                                                   # float32 values held in float64
    err = ((c - o64[..., None, :]).norm(dim=-1) - D[..., None]).abs()
    off_ray = (c - ideal[..., None, :]).norm(dim=-1)
    score = torch.where(err <= 0.5 * _ulp(dist)[..., None].double(), off_ray, 1e6 + err)
    pick = score.argmin(-1)
    return torch.gather(c, 2, pick[..., None, None].expand(-1, -1, 1, 3))[:, :, 0].float()


class DvrRenderLoss(torch.autograd.Function):
    """apply(sigma (N, T, Z, Y, X), origin (N, T, 3), points (N, M, >=3), tindex (N, M), loss_name) ->
    (loss_sum, n_valid), 0-d device tensors: the loss summed over the rays the kernel rendered (pred_dist >= 0) and their
    number.  loss_sum is formed in torch from the float32 distances — sum |p - g| (l1, bce), sum (p - g)^2 / 2 (l2),
    sum |p - g| / g (absrel) — the losses whose derivatives the kernel bakes into grad_sigma.  Gradient for sigma only."""

    @staticmethod
    def forward(ctx, sigma, origin, points, tindex, loss_name):
        from .. import ext
        pred, gt, grad_sigma = ext.dvr_render(sigma.contiguous(), origin.contiguous(), points.contiguous(),
                                              tindex.contiguous(), loss_name)
        valid = pred >= 0
        diff = torch.where(valid, pred - gt, torch.zeros_like(pred))
        if loss_name == "l2":
            loss_sum = (0.5 * diff * diff).sum()
        elif loss_name == "absrel":
            loss_sum = (diff.abs() / torch.where(valid, gt, torch.ones_like(gt))).sum()
        else:
            loss_sum = diff.abs().sum()
        n_valid = valid.sum()
        ctx.save_for_backward(grad_sigma)
        ctx.mark_non_differentiable(n_valid)
        return loss_sum, n_valid

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_n):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        (grad_sigma,) = ctx.saved_tensors
        return grad_loss * grad_sigma, None, None, None, None


@LOSSES.register_module()
class RayDepthLoss(nn.Module):
    """loss_weight * mean over the rendered rays of the depth loss, in metres (l1), metres^2 (l2) or relative (absrel).

    Density rule: with head logits occ (B, X, Y, Z, C), sigma = logsumexp(occ, -1) - occ[..., free_id] = -log p_free >= 0 per
    voxel length: one voxel length of path through a voxel leaves the transmittance p_free.  Layout: (B, T, Z, Y, X) — the
    evaluator's mapping sigma[z][y][x] = grid[x][y][z] (metrics.process_one_sample's permute(2, 1, 0)), one copy of the grid per
    lidar origin (the C ABI indexes sigma and origin by the same T; autograd sums the copies' gradients).  Distances inside the
    kernel are in voxel units: the loss is scaled by voxel_size (l1), voxel_size^2 (l2), nothing (absrel)."""

    def __init__(self, loss='l1', loss_weight=1.0, free_id=None, pc_range=(-40, -40, -1.0, 40, 40, 5.4), voxel_size=0.4):
        super().__init__()
        if loss not in ('l1', 'l2', 'absrel'):
            raise ValueError(f"loss must be 'l1', 'l2' or 'absrel', got {loss!r}")
        self.loss = loss
        self.loss_weight = loss_weight
        self.free_id = free_id
        self.pc_range = [float(v) for v in pc_range]
        self.voxel_size = float(voxel_size)
        self._rays = {}         # device -> (14040, 3) float32 unit directions; not a buffer: no state_dict entry

    def _check_grid(self, X, Y, Z):
        r, s = self.pc_range, self.voxel_size
        for n, lo, hi in ((X, r[0], r[3]), (Y, r[1], r[4]), (Z, r[2], r[5])):
            if abs((hi - lo) / n - s) > 1e-6 * s:
                raise ValueError(f"RayDepthLoss: a {X}x{Y}x{Z} grid over pc_range {r} does not have voxel_size {s}")

    def lidar_rays(self, device):
        rays = self._rays.get(device)
        if rays is None:
            from ..metrics import generate_lidar_rays
            rays = self._rays[device] = torch.from_numpy(generate_lidar_rays()).to(device)
        return rays

    @torch.no_grad()
    def targets_from_occupancy(self, voxel_semantics, lidar_origins, rays=None):
        """Pseudo-lidar targets from the ground-truth grid alone: voxel_semantics (B, X, Y, Z) class ids on the device,
        lidar_origins (B, T, 3) ego metres, rays (R, 3) unit directions (None: metrics.generate_lidar_rays()).  Every ray is
        cast from every origin through the ground truth with the evaluator's hard caster (ext.dvr_render_forward, "test"
        phase, process_one_sample's float32 conversion to voxel units).
        -> (origin_vox (B, T, 3), points_vox (B, T * R, 3), tindex (B, T * R)) float32: the end point of ray r of origin t, row
        t * R + r, lies on the ray at the hit distance — the exit distance of the first occupied voxel, the same d_i the
        renderer averages; |point - origin| carries it to a float32 ulp (end_points_at) — and tindex = t; tindex = -1 (a padded ray) where the ray hits nothing or never enters the grid:
        the evaluator's `valid` rule, with static shapes."""
        from .. import ext
        sem = voxel_semantics
        B, X, Y, Z = sem.shape
        self._check_grid(X, Y, Z)
        dev = sem.device
        if self.free_id is None:
            raise ValueError("RayDepthLoss.targets_from_occupancy: class ids do not tell the free class; pass free_id")
        free_id = int(self.free_id)
        rays = self.lidar_rays(dev) if rays is None else rays.to(dev, torch.float32)
        R = rays.shape[0]
        origins = torch.as_tensor(lidar_origins).to(dev, torch.float32).reshape(B, -1, 3)
        T = origins.shape[1]
        offset = torch.tensor(self.pc_range[:3], dtype=torch.float32, device=dev)
        scaler = torch.tensor([self.voxel_size] * 3, dtype=torch.float32, device=dev)
        origin_vox = ((origins - offset) / scaler).contiguous()
        end_vox = ((rays[None, None] + origins[:, :, None]) - offset) / scaler               # (B, T, R, 3)
        occ = (sem != free_id).permute(0, 3, 2, 1)[:, None].float().contiguous()             # (B, 1, Z, Y, X)
        zeros = torch.zeros((B, R), dtype=torch.float32, device=dev)
        points, tindex = [], []
        for t in range(T):
            o = origin_vox[:, t:t + 1].contiguous()
            dist, _, coord = ext.dvr_render_forward(occ, o, end_vox[:, t].contiguous(), zeros, None, "test")
            c = coord.long()
            cls = sem[torch.arange(B, device=dev)[:, None], c[..., 0], c[..., 1], c[..., 2]]
            hit = (dist >= 0) & (cls != free_id)
            p = end_points_at(o, end_vox[:, t], dist.clamp(min=0))
            points.append(torch.where(hit[..., None], p, end_vox[:, t]))
            tindex.append(torch.where(hit, torch.full_like(dist, float(t)), torch.full_like(dist, -1.0)))
        return origin_vox, torch.cat(points, 1).contiguous(), torch.cat(tindex, 1).contiguous()

    def density(self, occ):
        """Head logits (B, X, Y, Z, C) -> sigma (B, 1, Z, Y, X) = -log p_free."""
        free_id = occ.shape[-1] - 1 if self.free_id is None else int(self.free_id)
        sigma = torch.logsumexp(occ, -1) - occ[..., free_id]
        return sigma.permute(0, 3, 2, 1)[:, None]

    def forward(self, occ, origin_vox, points_vox, tindex):
        """occ (B, X, Y, Z, C) logits; origin_vox (B, T, 3), points_vox (B, M, >=3), tindex (B, M) in voxel units
        (targets_from_occupancy).  -> 0-d loss."""
        B, X, Y, Z, _ = occ.shape
        self._check_grid(X, Y, Z)
        T = origin_vox.shape[1]
        sigma = self.density(occ.float()).expand(B, T, Z, Y, X).contiguous()
        loss_sum, n_valid = DvrRenderLoss.apply(sigma, origin_vox, points_vox, tindex, self.loss)
        unit = {'l1': self.voxel_size, 'l2': self.voxel_size ** 2, 'absrel': 1.0}[self.loss]
        return (self.loss_weight * unit) * loss_sum / n_valid.clamp(min=1)
