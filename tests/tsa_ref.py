"""Reference for the fused temporal self-attention gather (occ_tsa_fused_forward_f32, csrc/tsa_fused.hip) and the inputs its
tests run on.  A plain helper: no pytest code, CPU torch ops only, differentiable.

`tsa_gather_ref` restates the reference module's temporal_self_attention.py:206-262 (the lines the kernel's header cites):
view + softmax of the two Linear outputs, the (bs*2) permutes, sampling_locations = ref_2d + offsets / (W, H),
multi_scale_deformable_attn_pytorch on the (bs*2) value maps, mean over the two queue entries.  tests/test_tsa_fused_host.py
holds it against oracle.model.TemporalSelfAttention.
"""
import torch

from oracle.msda import multi_scale_deformable_attn_pytorch

M, D, P = 8, 32, 4          # the only shape the fused kernel exists for


def tsa_locations_weights(offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points):
    """offs (B, Nq, M*2*P*2) pixels, logits (B, Nq, M*2*P), ref_2d (B*2, Nq, 1, 2) ->
    sampling_locations (B*2, Nq, M, 1, P, 2), attention_weights (B*2, Nq, M, 1, P): lines :206-228."""
    B, Nq = offs.shape[:2]
    m, p = num_heads, num_points
    o = offs.reshape(B, Nq, m, 2, 1, p, 2)
    aw = logits.reshape(B, Nq, m, 2, p).softmax(-1).reshape(B, Nq, m, 2, 1, p)
    aw = aw.permute(0, 3, 1, 2, 4, 5).reshape(B * 2, Nq, m, 1, p)
    o = o.permute(0, 3, 1, 2, 4, 5, 6).reshape(B * 2, Nq, m, 1, p, 2)
    normalizer = torch.tensor([bev_w, bev_h], dtype=offs.dtype)
    loc = ref_2d[:, :, None, :, None, :] + o / normalizer
    return loc, aw


def tsa_gather_weighted(value, loc, aw, bev_h, bev_w, reduce="mean"):
    """value (B*2, bev_h*bev_w, M, D) and the (B*2, Nq, ...) locations / weights -> (B, Nq, M*D): lines :240-262.
    A sample whose location is not finite contributes nothing: the reference's device kernel fails its admission test
    (-1 < h_im < H is false for NaN and +-Inf; oracle/msda.py::msda_scalar_f64), while grid_sample would return NaN."""
    B2, Nq = loc.shape[:2]
    dead = ~torch.isfinite(loc).all(-1)
    aw = torch.where(dead, torch.zeros_like(aw), aw)
    loc = torch.where(dead[..., None], torch.zeros_like(loc), loc)
    shapes = torch.tensor([[bev_h, bev_w]], dtype=torch.long)
    out = multi_scale_deformable_attn_pytorch(value, shapes, loc, aw)          # (B*2, Nq, M*D)
    out = out.permute(1, 2, 0).reshape(Nq, out.shape[-1], B2 // 2, 2)
    out = out.mean(-1) if reduce == "mean" else out.sum(-1)
    return out.permute(2, 0, 1)


def tsa_gather_ref(value, offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points, dtype=torch.float64):
    """What ext.tsa_fused_forward computes, in `dtype` on the CPU.  value (B*2, bev_h*bev_w, M, D); offs / logits / ref_2d
    cover Nq queries: all bev_h*bev_w of them, or fewer (the band form: some rows of the BEV against the whole map)."""
    value, offs, logits, ref_2d = (t.to(dtype) for t in (value, offs, logits, ref_2d))
    loc, aw = tsa_locations_weights(offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points)
    return tsa_gather_weighted(value, loc, aw, bev_h, bev_w)


# (B, bev_h, bev_w, spread): tiny, non-square maps.  9x7 at B = 1 (63 waves), 5x31 (155) and 1x1 leave a partial last
# block of the kernel's four waves.
CASES = [(1, 12, 14, 4.0), (2, 9, 7, 3.0), (1, 9, 7, 3.0), (1, 5, 31, 3.0), (1, 1, 1, 0.4), (1, 1, 5, 1.0)]
CASE_IDS = [f"B{b}_{h}x{w}" for b, h, w, _ in CASES]
SEED = 7
GPU_TOL = 2e-5          # max |hip - float64 reference|: the bound tests/test_gpu_msda.py holds the generic fp32 gather to


def tsa_case(B, bev_h, bev_w, seed, spread):
    """float32 CPU inputs of one case: value (B*2, Nq, M, D), offs (B, Nq, M*2*P*2), logits (B, Nq, M*2*P),
    ref_2d (B*2, Nq, 1, 2), Nq = bev_h*bev_w.  With Nq >= 10, queries 0-9 of batch 0 hold the edge cases."""
    g = torch.Generator().manual_seed(seed)
    H, W = bev_h, bev_w
    Nq = H * W
    value = torch.randn(B * 2, Nq, M, D, generator=g)
    offs = torch.randn(B, Nq, M * 2 * P * 2, generator=g) * spread
    logits = torch.randn(B, Nq, M * 2 * P, generator=g) * 3.0
    ref_2d = torch.rand(B * 2, Nq, 1, 2, generator=g)
    if Nq >= 10:
        o = offs.view(B, Nq, M, 2, P, 2)
        lg = logits.view(B, Nq, M, 2, P)
        wh = torch.tensor([float(W), float(H)])
        far = 1.0 / max(H, W)
        targets = {0: (0.0, 0.0),                          # exact top-left corner
                   1: (1.0, 1.0),                          # exact bottom-right corner
                   2: (0.5 / W, 0.5 / H),                  # a pixel centre
                   3: (-far, -far),                        # just outside
                   4: (1e7, 1e7),                          # absurdly far
                   5: (-1e7, -1e7),
                   6: (1.0 - 0.5 / W, 0.5 / H),
                   7: (1.0 + 0.49 * far, 1.0 + 0.49 * far)}   # the last admitted half pixel
        for q, target in targets.items():
            for t in range(2):
                o[0, q, :, t] = (torch.tensor(target) - ref_2d[t, q, 0]) * wh
        lg[0, 8, :, 0] = torch.tensor([100.0, -100.0, 0.0, 0.0])
        lg[0, 8, :, 1] = 1e4
        lg[0, 9] = -1e4
    return value, offs, logits, ref_2d
