"""Reference for the fused spatial cross-attention gather (ext.sca_fused_forward, csrc/sca_fused.hip: sca_fused_kernel,
sca_fused_h_kernel, sca_fused_hm_kernel) and the inputs its tests run on.  A plain helper: no pytest code, CPU torch ops only,
differentiable.

`sca_gather_ref` restates what the kernels' header cites of the reference module's spatial_cross_attention.py: softmax over the
L*P logits of a head, offsets / (W_l, H_l), + the camera's z-anchor (point p pairs with anchor p % Z), the oracle's
multi_scale_deformable_attn_pytorch per camera, batch 0's mask picks the cameras of every batch element, the sum is divided by
the number of cameras the own batch element's mask holds (at least 1).  tests/test_sca_fused_host.py holds it against
oracle.model.SpatialCrossAttention; tests/test_gpu_sca_fused_backward.py differentiates it.
"""
import torch

from oracle.msda import multi_scale_deformable_attn_pytorch

M, D = 8, 32            # the only head shape the fused kernels exist for
SEED = 3
GPU_TOL = 2e-5          # max |hip - float64 reference| of an fp32 gather on unit-variance values: tsa_ref.GPU_TOL, test_gpu_msda.py
# A coordinate this close (in pixels) to an integer that decides a corner may fall either way in fp32.  The kernels evaluate
# x = (ref + off / W) * W - 0.5 from the same fp32 inputs: off / W to 1 ulp (6e-8 at |off / W| < 1), the sum to half an ulp of
# |loc| < 2 (1.2e-7), together 1.8e-7 * W <= 2.7e-6 px at W <= 15, and the product and the difference each to half an ulp of
# |x| < 16 (4.8e-7): 3.7e-6 px in all at the deciding integers of these maps.  1e-5 is 2.7 times that.  (A window of 1e-4
# holds up to 31 coordinates of a B = 2 case; this one at most 8: tests/test_sca_fused_host.py.)
NEAR_PX = 1e-5


def level_starts(shapes):
    hw = shapes[:, 0] * shapes[:, 1]
    return torch.cat([hw.new_zeros(1), hw.cumsum(0)[:-1]])


def sca_locations_weights(offs, logits, ref_cam, shapes, P, Z):
    """offs (B, Nq, M*L*P*2) pixels, logits (B, Nq, M*L*P), ref_cam (NC, B, Nq, Z, 2), shapes (L, 2) (h, w) ->
    sampling_locations (NC, B, Nq, M, L, P, 2), attention_weights (B, Nq, M, L, P)."""
    B, Nq = offs.shape[:2]
    L = shapes.shape[0]
    aw = logits.reshape(B, Nq, M, L * P).softmax(-1).reshape(B, Nq, M, L, P)
    norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(offs.dtype)                 # (W, H)
    off = offs.reshape(B, Nq, M, L, P // Z, Z, 2) / norm[None, None, None, :, None, None, :]
    loc = ref_cam[:, :, :, None, None, None, :, :] + off[None]                          # point p pairs with anchor p % Z
    return loc.reshape(ref_cam.shape[0], B, Nq, M, L, P, 2), aw


def sca_camera_outputs(value, shapes, loc, aw):
    """value (B*NC, S, M, D) in row order, entry b*NC + c; loc (NC, B, Nq, M, L, P, 2); aw (B, Nq, M, L, P) ->
    (NC, B, Nq, M*D): every camera's deformable attention for every query, seen or not.
    A sample whose location is not finite contributes nothing: the reference's device kernel fails its admission test
    (-1 < h_im < H is false for NaN and +-Inf; oracle/msda.py::msda_scalar_f64), while grid_sample would return NaN."""
    NC = loc.shape[0]
    dead = ~torch.isfinite(loc).all(-1)
    loc = torch.where(dead[..., None], torch.zeros_like(loc), loc)
    outs = []
    for cam in range(NC):
        w = torch.where(dead[cam], torch.zeros_like(aw), aw)
        outs.append(multi_scale_deformable_attn_pytorch(value[cam::NC], shapes, loc[cam], w))
    return torch.stack(outs)


def popcount(vis, NC):
    return sum((vis.to(torch.int64) >> cam) & 1 for cam in range(NC))


def sca_camera_mean(per_cam, select, divide):
    """per_cam (NC, B, Nq, M*D); select / divide: int (B, Nq) camera bit masks (or (Nq,), for every batch element) ->
    (B, Nq, M*D): the cameras of `select` summed, divided by the number of cameras in `divide` (at least 1)."""
    NC = per_cam.shape[0]
    select, divide = select.to(torch.int64), divide.to(torch.int64)
    slots = 0
    for cam in range(NC):
        slots = slots + per_cam[cam] * ((select >> cam) & 1).to(per_cam.dtype)[..., None]
    return slots / popcount(divide, NC).clamp(min=1).to(per_cam.dtype)[..., None]


def sca_gather_ref(value, shapes, offs, logits, ref_cam, vis, P, Z, dtype=torch.float64):
    """What ext.sca_fused_forward computes, in `dtype` on the CPU.  value (B*NC, S, M, D) in ROW order (S = the maps' pixels,
    no pad row), shapes (L, 2) int64, offs (B, Nq, M*L*P*2), logits (B, Nq, M*L*P), ref_cam (NC, B, Nq, Z, 2), vis (B, Nq)
    int32 camera bits -> (B, Nq, M*D)."""
    value, offs, logits, ref_cam = (t.to(dtype) for t in (value, offs, logits, ref_cam))
    loc, aw = sca_locations_weights(offs, logits, ref_cam, shapes, P, Z)
    per_cam = sca_camera_outputs(value, shapes, loc, aw)
    return sca_camera_mean(per_cam, vis[0], vis)          # batch 0's mask picks the cameras, the own one divides


def sca_counts(shapes, offs, logits, ref_cam, vis, P, Z):
    """What the kernels' `stats` pair counts, in float64 -> (rows, corners, near).
    rows: visible (b, q, camera) triples, batch 0's mask applied to every batch element (= stats[0]).
    corners: bilinear corners inside their map over all samples of those rows (oracle.msda.count_inbounds_corners on float64
    locations; = stats[1] up to fp32 rounding of the locations).
    near: coordinates of those samples within NEAR_PX of an integer that DECIDES a corner: -1 and W (the admission test), 0
    (w_low = -1 or 0: the left corners) and W - 1 (the right corners), likewise in y.  Around any other integer k the floor
    falls to k - 1 or k with all four corners inside either way.  Only such a coordinate can be counted differently by the
    kernels (NEAR_PX), and each decides at most two corners of its sample: |stats[1] - corners| <= 2 * near."""
    B, Nq = offs.shape[:2]
    NC = ref_cam.shape[0]
    loc, _ = sca_locations_weights(offs.double(), logits.double(), ref_cam.double(), shapes, P, Z)
    seen = torch.stack([(vis[0].to(torch.int64) >> cam) & 1 for cam in range(NC)]).bool()          # (NC, Nq)
    rows = int(seen.sum()) * B
    live = seen[:, None, :].expand(NC, B, Nq)
    loc = loc[live]                                                                                 # (rows, M, L, P, 2)
    loc = torch.where(torch.isfinite(loc).all(-1, keepdim=True), loc, torch.full_like(loc, -1e9))
    corners = _count_corners_f64(shapes, loc)
    near = 0
    for l, (H, W) in enumerate(shapes.tolist()):
        for axis, n in ((0, W), (1, H)):
            x = loc[:, :, l, :, axis] * n - 0.5
            for k in {-1, 0, n - 1, n}:
                near += int(((x - k).abs() < NEAR_PX).sum())
    return rows, corners, near


def _count_corners_f64(shapes, loc):
    """oracle.msda.count_inbounds_corners evaluates in float32 (`.float()`): the same count on float64 locations."""
    n = 0
    for l, (H, W) in enumerate(shapes.tolist()):
        x = loc[:, :, l, :, 0] * W - 0.5
        y = loc[:, :, l, :, 1] * H - 0.5
        ok = (y > -1) & (x > -1) & (y < H) & (x < W)
        xl, yl = torch.floor(x), torch.floor(y)
        t, btm = yl >= 0, (yl + 1) <= H - 1
        lft, rgt = xl >= 0, (xl + 1) <= W - 1
        n += int((ok & t & lft).sum() + (ok & t & rgt).sum() + (ok & btm & lft).sum() + (ok & btm & rgt).sum())
    return n


def outside_share(shapes, offs, logits, ref_cam, P, Z):
    """Share of all (camera, b, q, head, level, point) samples that fail the admission test -1 < h_im < H, -1 < w_im < W."""
    loc, _ = sca_locations_weights(offs.double(), logits.double(), ref_cam.double(), shapes, P, Z)
    bad = tot = 0
    for l, (H, W) in enumerate(shapes.tolist()):
        x, y = loc[..., l, :, 0] * W - 0.5, loc[..., l, :, 1] * H - 0.5
        ok = (x > -1) & (x < W) & (y > -1) & (y < H)
        bad += int((~ok).sum())
        tot += ok.numel()
    return bad / tot


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# Tiny maps (at most 177 pixels) and offsets of 1.5 px keep float32 rounding of the restatement below GPU_TOL / 4.
# L4P8: S = 177 is odd (the 16-bit rows get a pad pixel) and levels 2 and 3 start at the odd pixels 161 and 173: a pixel pair
# of the pair layout straddles two levels.  L4P4: odd widths and a 1x1 level.
MAPS = {"L4P8": ((9, 14), (5, 7), (3, 4), (2, 2)), "L4P4": ((9, 13), (5, 7), (3, 4), (1, 1)),
        "L2P8": ((9, 15), (5, 7)), "L1P8": ((7, 9),)}
POINTS = {"L4P8": 8, "L4P4": 4, "L2P8": 8, "L1P8": 8}
ZS = {"L4P8": (8, 4, 2, 1), "L4P4": (4, 2, 1), "L2P8": (8, 2), "L1P8": (8, 1)}
NQ = 77                 # 2 * 32 + 13: the head-major kernel's last block has one full wave, one 5-query wave, two idle waves

# (maps, Z, B, NC, Nq)
CASES = [(k, z, b, 6, NQ) for k in MAPS for z in ZS[k] for b in (1, 2)]
CASES += [("L4P8", 4, 2, 1, NQ)]                                        # one camera
CASES += [("L4P8", 8, 2, 6, 1), ("L4P8", 2, 2, 6, 7), ("L4P8", 4, 2, 6, 33)]       # tails


def case_id(c):
    k, z, b, nc, nq = c
    return f"{k}_Z{z}_B{b}" + (f"_NC{nc}" if nc != 6 else "") + (f"_Nq{nq}" if nq != NQ else "")


CASE_IDS = [case_id(c) for c in CASES]
TAILS = [i for i, c in enumerate(CASES) if c[4] != NQ]


def _edge_targets(H, W):
    """The placed samples of tsa_ref.tsa_case for one level, in normalised (x, y).  The two pixel centres are those of pixel
    (1, 1) and of its mirror image in x where the level has an interior (a pixel centre is an integer coordinate, and one
    at a border pixel would decide corners: sca_counts), a quarter pixel off the border pixel's centre otherwise."""
    far = 1.0 / max(H, W)
    c = 1.5 if min(H, W) >= 3 else 0.75
    return [(0.0, 0.0), (1.0, 1.0), (c / W, c / H), (-far, -far), (1e7, 1e7), (-1e7, -1e7), (1.0 - c / W, c / H),
            (1.0 + 0.49 * far, 1.0 + 0.49 * far)]


def sca_case(maps, Z, B, NC, Nq, seed=SEED, amp=1.0):
    """float32 CPU inputs of one case, as a dict: value (B*NC, S, M, D) = amp * N(0, 1) in row order, shapes, starts, offs,
    logits, ref_cam (NC, B, Nq, Z, 2), vis (B, Nq) int32, and B, NC, Nq, S, L, P, Z, amp.
    Visibility, Nq >= 24: queries 0-7 no camera in any batch element (a whole head-major wave with an empty union); 8-23 every
    camera in batch element 0; B = 2: 24-27 seen in element 0 and by nobody in element 1 (divisor 1), 28-31 the other way
    round (no camera loop: exactly 0); every other bit drawn at p = 0.35.  Nq < 24: query 0 unseen (Nq > 1), query 1 / 2 the
    two B = 2 kinds.  Queries 8-15 of batch element 0 hold the placed edge samples at the even points of every head and level
    (anchor 0 for every camera, so the offsets put every camera's sample on the target; the odd points keep their drawn
    offsets, so that no such row is all zero), 16-18 the extreme logits rows.  A few anchors of queries every camera sees
    lie at +-3e4 / +-7e4: points behind a camera."""
    g = torch.Generator().manual_seed(seed * 1000 + 17 * Z + 5 * B + NC + Nq + len(MAPS[maps]))
    shapes = torch.tensor(MAPS[maps], dtype=torch.int64)
    L, P = shapes.shape[0], POINTS[maps]
    starts = level_starts(shapes)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    value = torch.randn(B * NC, S, M, D, generator=g) * amp
    offs = torch.randn(B, Nq, M * L * P * 2, generator=g) * 1.5
    logits = torch.randn(B, Nq, M * L * P, generator=g) * 3.0
    ref_cam = torch.rand(NC, B, Nq, Z, 2, generator=g) * 1.3 - 0.15
    bits = (torch.rand(B, Nq, NC, generator=g) < 0.35).to(torch.int64)
    one = lambda q: q % NC                                   # a camera for a query that needs at least one
    if Nq >= 24:
        bits[:, :8] = 0
        bits[0, 8:24] = 1
        b0_only, b1_only, far_q = range(24, 28), range(28, 32), [q for q in (32, 40, 47, 54) if q < Nq]
    else:
        if Nq > 1:
            bits[:, 0] = 0
        b0_only, b1_only, far_q = [min(1, Nq - 1)], ([2] if Nq > 2 else []), ([5] if Nq > 5 else [])
    if B == 2:
        for q in b0_only:                                    # two cameras: the divisor 1 differs from batch 0's count
            bits[0, q, one(q)] = bits[0, q, one(q + 1)] = 1
            bits[1, q] = 0
        for q in b1_only:
            bits[0, q] = 0
            bits[1, q, one(q)] = 1
    elif Nq == 1:
        bits[0, 0, 0] = 1
    for i, q in enumerate(far_q):
        bits[0, q] = 1
        v = (3e4, -3e4, 7e4, -7e4)[i % 4]
        ref_cam[q % NC, q % B, q, q % Z] = torch.tensor([v, -v / 2])
    vis = (bits << torch.arange(NC)).sum(-1).to(torch.int32)
    if Nq >= 24:
        o = offs.view(B, Nq, M, L, P, 2)
        lg = logits.view(B, Nq, M, L * P)
        ref_cam[:, 0, 8:16] = 0.0
        for l, (H, W) in enumerate(MAPS[maps]):
            for t, target in enumerate(_edge_targets(H, W)):
                o[0, 8 + t, :, l, 0::2] = torch.tensor(target) * torch.tensor([float(W), float(H)])
        lg[0, 16] = 0.0
        lg[0, 16, :, 0], lg[0, 16, :, 1] = 100.0, -100.0
        lg[0, 17] = 1e4
        lg[0, 18] = -1e4
    return dict(maps=maps, B=B, NC=NC, Nq=Nq, S=S, L=L, P=P, Z=Z, amp=amp, shapes=shapes, starts=starts, value=value,
                offs=offs, logits=logits, ref_cam=ref_cam, vis=vis)


def case_ref(c, value=None, dtype=torch.float64):
    """sca_gather_ref on a case dict (optionally on other value rows: the stored fp16 / q16 values)."""
    return sca_gather_ref(c['value'] if value is None else value, c['shapes'], c['offs'], c['logits'], c['ref_cam'], c['vis'],
                          c['P'], c['Z'], dtype=dtype)
