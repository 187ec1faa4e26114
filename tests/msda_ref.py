"""Closed-form float64 reference of multi-scale deformable attention, forward and backward, with the input sets that make
it the arbiter where torch.autograd is not one (test infrastructure; imports nothing from the package).

The arithmetic is mmcv's ms_deformable_im2col / col2im, per sample (b, q, m, l, p):
    h_im = loc_y * H - 0.5,  w_im = loc_x * W - 0.5,   admitted iff -1 < h_im < H and -1 < w_im < W  (a NaN is not),
    h_low = floor(h_im), w_low = floor(w_im), lh = h_im - h_low, lw = w_im - w_low, hh = 1 - lh, hw = 1 - lw,
    corners v1 (h_low, w_low), v2 (h_low, w_low + 1), v3 (h_low + 1, w_low), v4 (h_low + 1, w_low + 1), each used only if it
    lies inside the map, with weights w1 = hh hw, w2 = hh lw, w3 = lh hw, w4 = lh lw;
    out[b, q, m, :]   = sum_{l, p} attn * sum_k w_k v_k
    grad_attn         = sum_c top_c * sum_k w_k v_k
    grad_loc (x, y)   = (W, H) * attn * sum_c top_c * (hh (v2 - v1) + lh (v4 - v3),  hw (v3 - v1) + lw (v4 - v2))
    grad_value[k]    += top * attn * w_k
and a sample that is not admitted contributes zero everywhere.  At an integer pixel coordinate and on the admission boundary
the operator is not differentiable; the formulas above are the kernels' DEFINED answer there (right-sided floor, strict
admission), which is where torch.autograd through grid_sample answers differently (tests/test_msda_ref_host.py measures it).

Every decision (admission, floor, the four corner tests) is taken on the exact float64 image of the location that is passed
in: pass the float32 tensor the kernel gets (or its .double()).  Written in torch, vectorised, so it also runs in float64 on
the device for the one case whose value tensor does not fit a host copy.

`mut` restates a wrong kernel (the mutants of tests/test_msda_ref_host.py):
    'adm_ge'         admission with >= / <= for > / <
    'floor_left'     the left cell at an integer coordinate (h_low = ceil(h_im) - 1, lh = 1)
    'drop_last_col'  the corner in the last column is dropped when it is the LEFT corner (w_low = W - 1)
    'skip_lane0'     the zero-item skip decided from channels 0..3 only (one lane of the 8-lane group instead of its ballot)
    'skip_neighbour' the zero-item skip read from the neighbouring item's byte (count and fill disagreeing on the item)
"""
import itertools

import torch

MUTANTS = ('adm_ge', 'floor_left', 'drop_last_col', 'skip_lane0', 'skip_neighbour')


def level_starts(shapes):
    st, out = 0, []
    for H, W in shapes:
        out.append(st)
        st += H * W
    return out


def shape_tensors(shapes):
    """(spatial_shapes, level_start_index) int64 tensors of a list of [H, W]."""
    return torch.tensor(shapes, dtype=torch.long), torch.tensor(level_starts(shapes), dtype=torch.long)


def _level_terms(loc_l, H, W, mut):
    """loc_l (..., 2) -> adm, then per corner k: (ok_k, pixel index in the level, weight), and lh, lw, hh, hw."""
    x = loc_l[..., 0].double() * W - 0.5
    y = loc_l[..., 1].double() * H - 0.5
    if mut == 'adm_ge':
        adm = (y >= -1) & (x >= -1) & (y <= H) & (x <= W)
    else:
        adm = (y > -1) & (x > -1) & (y < H) & (x < W)
    zero = torch.zeros_like(x)
    x, y = torch.where(adm, x, zero), torch.where(adm, y, zero)       # a sample that is not admitted: finite stand-ins
    if mut == 'floor_left':
        h_low, w_low = torch.ceil(y) - 1, torch.ceil(x) - 1
    else:
        h_low, w_low = torch.floor(y), torch.floor(x)
    lh, lw = y - h_low, x - w_low
    hh, hw = 1 - lh, 1 - lw
    corners = []
    for dy, dx, wgt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
        hy, wx = h_low + dy, w_low + dx
        ok = adm & (hy >= 0) & (hy <= H - 1) & (wx >= 0) & (wx <= W - 1)
        if mut == 'drop_last_col' and dx == 0:
            ok = ok & (w_low != W - 1)
        pix = torch.where(ok, hy * W + wx, zero).long()
        corners.append((ok, pix, wgt))
    return adm, corners, lh, lw, hh, hw


def _live_items(top, mut):
    """(B, Lq, M) bool: the items a kernel with this (wrong) skip rule would process; None = all of them."""
    if mut == 'skip_lane0':
        return (top[..., :4] != 0).any(-1)
    if mut == 'skip_neighbour':
        nz = (top != 0).any(-1).flatten()
        idx = torch.arange(nz.numel(), device=nz.device) ^ 1
        idx = torch.where(idx < nz.numel(), idx, idx ^ 1)
        return nz[idx].view(top.shape[:3])
    return None


def closed_form(value, shapes, loc, attn, grad_out=None, mut=None):
    """value (B, S, M, D), shapes [[H, W], ...], loc (B, Lq, M, L, P, 2), attn (B, Lq, M, L, P), grad_out (B, Lq, M * D) or None
    -> dict of float64 tensors: out (B, Lq, M * D), adm (B, Lq, M, L, P) bool, and with grad_out: grad_value, grad_loc,
    grad_attn in the shapes of value, loc, attn.  value may be float32 (gathered as it is, widened after)."""
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    dev = value.device
    vflat = value.permute(0, 2, 1, 3)                                   # (B, M, S, D), a view
    a = attn.double()
    out = torch.zeros(B, Lq, M, D, dtype=torch.float64, device=dev)
    adm_all = torch.zeros(B, Lq, M, L, P, dtype=torch.bool, device=dev)
    res = {}
    if grad_out is not None:
        top = grad_out.double().view(B, Lq, M, D)
        live = _live_items(top, mut)
        if live is not None:
            top = torch.where(live[..., None], top, torch.zeros_like(top))
        gv = torch.zeros(B * M * S, D, dtype=torch.float64, device=dev)
        gl = torch.zeros(B, Lq, M, L, P, 2, dtype=torch.float64, device=dev)
        ga = torch.zeros(B, Lq, M, L, P, dtype=torch.float64, device=dev)
        bm = (torch.arange(B, device=dev)[:, None, None, None] * M + torch.arange(M, device=dev)[None, None, :, None]) * S
    for l, ((H, W), st) in enumerate(zip(shapes, level_starts(shapes))):
        adm, corners, lh, lw, hh, hw = _level_terms(loc[:, :, :, l], H, W, mut)        # (B, Lq, M, P) each
        adm_all[:, :, :, l] = adm
        v = []
        for ok, pix, _ in corners:
            idx = (st + pix).permute(0, 2, 1, 3).reshape(B, M, Lq * P, 1).expand(B, M, Lq * P, D)
            g = torch.gather(vflat, 2, idx).double().view(B, M, Lq, P, D).permute(0, 2, 1, 3, 4)
            v.append(torch.where(ok[..., None], g, torch.zeros_like(g)))             # (B, Lq, M, P, D)
        bil = sum(c[2][..., None] * vk for c, vk in zip(corners, v))
        al = a[:, :, :, l]
        out += (al[..., None] * bil).sum(3)
        if grad_out is None:
            continue
        t = top[:, :, :, None, :]                                                      # (B, Lq, M, 1, D)
        ga[:, :, :, l] = (t * bil).sum(-1)
        gx = (t * (hh[..., None] * (v[1] - v[0]) + lh[..., None] * (v[3] - v[2]))).sum(-1)
        gy = (t * (hw[..., None] * (v[2] - v[0]) + lw[..., None] * (v[3] - v[1]))).sum(-1)
        gl[:, :, :, l, :, 0] = W * al * gx
        gl[:, :, :, l, :, 1] = H * al * gy
        for ok, pix, wgt in corners:
            contrib = torch.where(ok[..., None], t * (al * wgt)[..., None], torch.zeros_like(bil))
            gv.index_add_(0, (bm + st + pix).reshape(-1), contrib.reshape(-1, D))
    res['out'] = out.view(B, Lq, M * D)
    res['adm'] = adm_all
    if grad_out is not None:
        res['grad_value'] = gv.view(B, M, S, D).permute(0, 2, 1, 3).contiguous()
        res['grad_loc'] = gl
        res['grad_attn'] = ga
    return res


def grads(res):
    return res['grad_value'], res['grad_loc'], res['grad_attn']


# ---- the decision set --------------------------------------------------------------------------------------------------------
DECISION_SHAPES = [[8, 8], [4, 8], [2, 2], [1, 2], [1, 1]]
SPECIALS = (1e7, -1e7, float('nan'), float('inf'), float('-inf'))


def axis_coords(n):
    """Pixel coordinates of one axis of size n where a decision changes: the admission boundary on both sides, integer
    coordinates (floor side), the first and the last cell, the half-cells outside the map that are still admitted."""
    return sorted({-1.0, -0.75, -0.5, 0.0, 0.5, 1.0, n - 2.0, n - 1.0, n - 0.5, n - 0.25, float(n)})


def decision_points(H, W):
    """float32 (N, 2) locations (x, y) of one level: the Cartesian product of the axis coordinates, then the far and
    non-finite ones (both coordinates, and each alone beside a coordinate in the middle of the map)."""
    pts = [((x + 0.5) / W, (y + 0.5) / H) for y, x in itertools.product(axis_coords(H), axis_coords(W))]
    mid = (0.5, 0.5)
    for s in SPECIALS:
        pts += [(s, s), (s, mid[1]), (mid[0], s)]
    return torch.tensor(pts, dtype=torch.float64).float()


def check_exact(loc, shapes):
    """The precondition that makes a decision case independent of FMA contraction and of the precision of the arithmetic:
    for every finite |loc| < 4, loc32 * n and loc32 * n - 0.5 are float32 numbers (checked in float64), so the kernel's
    h_im / w_im, its floor, its weights and every comparison are exact."""
    for l, (H, W) in enumerate(shapes):
        for d, n in ((0, W), (1, H)):
            c = loc[:, :, :, l, :, d].double()
            c = c[torch.isfinite(c) & (c.abs() < 4)]
            for e in (c * n, c * n - 0.5):
                assert torch.equal(e.float().double(), e), (l, d)


def decision_set(shapes=DECISION_SHAPES, B=2, M=3, D=32, P=4, seed=31):
    """-> value, spatial_shapes, level_start_index, loc, attn, grad_out (float32 / int64, host).  Every level's point list is
    laid over the (query, point) slots of a (batch, head), cycled to the common length and ROTATED from head to head and batch
    entry to batch entry, so that the 8-lane groups of a wave (consecutive (b, q, m) items) hold different samples."""
    g = torch.Generator().manual_seed(seed)
    lists = [decision_points(H, W) for H, W in shapes]
    n = max(len(p) for p in lists)
    Lq = (n + P - 1) // P
    L = len(shapes)
    loc = torch.empty(B, Lq, M, L, P, 2)
    for b in range(B):
        for m in range(M):
            for l, pts in enumerate(lists):
                idx = (torch.arange(Lq * P) + 37 * m + 11 * b + 5 * l) % len(pts)
                loc[b, :, m, l] = pts[idx].view(Lq, P, 2)
    check_exact(loc, shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(B, S, M, D, generator=g)
    attn = torch.rand(B, Lq, M, L, P, generator=g) + 1e-3
    attn = attn / attn.flatten(-2).sum(-1)[..., None, None]
    grad_out = torch.randn(B, Lq, M * D, generator=g)
    shapes_t, start = shape_tensors(shapes)
    return value, shapes_t, start, loc, attn, grad_out


def dyadic_loc(size, gen, lo=-0.1, hi=1.1, bits=12):
    """Random float32 locations j / 2^bits in [lo, hi): for every map side n with n * 2^bits * hi < 2^24 the products
    loc * n and loc * n - 0.5 are float32 numbers, so check_exact holds on maps of ANY size (not only powers of two) and the
    closed form needs no window around integer coordinates for them either; some of them ARE integer coordinates."""
    j = torch.randint(int(lo * 2 ** bits), int(hi * 2 ** bits), size, generator=gen)
    return j.float() / 2 ** bits


def dyadic_inputs(B, shapes, M, D, Lq, P, seed, value=True):
    """-> value, spatial_shapes, level_start_index, loc, attn, grad_out like decision_set, random locations on the dyadic
    grid (value=False: None in its place, for a value tensor the caller makes elsewhere)."""
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    v = torch.randn(B, S, M, D, generator=g) if value else None
    loc = dyadic_loc((B, Lq, M, L, P, 2), g)
    check_exact(loc, shapes)
    attn = torch.rand(B, Lq, M, L, P, generator=g) + 1e-3
    attn = attn / attn.flatten(-2).sum(-1)[..., None, None]
    grad_out = torch.randn(B, Lq, M * D, generator=g)
    shapes_t, start = shape_tensors(shapes)
    return v, shapes_t, start, loc, attn, grad_out


# ---- sparse output gradients --------------------------------------------------------------------------------------------------
SPARSE_PATTERNS = ('every_4th_query', 'one_head', 'one_channel', 'neg_zero_rows', 'zero_run', 'all_zero')
ONE_CHANNELS = (0, 3, 4, 31)


def sparse_grad(grad_out, M, pattern):
    """A copy of grad_out (B, Lq, M * D) with the pattern's items (b, q, m) zeroed -> (gradient, (B, Lq, M) bool mask of the
    items that are all zero).  The skip of msda_bwd_d32_kernel is per ITEM: the patterns put zero items beside live ones
    inside an 8-item wave, leave single channels alive in each of the 8 lanes' corners (0, 3 | 4 | 31), and empty whole
    waves and whole launches."""
    B, Lq, MD = grad_out.shape
    D = MD // M
    g = grad_out.clone().view(B, Lq, M, D)
    if pattern == 'every_4th_query':
        g[:, ::4] = 0.0
    elif pattern == 'one_head':
        g[:, :, M // 2] = 0.0
    elif pattern == 'one_channel':
        item = torch.arange(B * Lq * M).view(B, Lq, M)
        for i, c in enumerate(ONE_CHANNELS):
            if c >= D:
                continue
            sel = item % 8 == 2 * i                      # every other item of a wave, one channel each
            keep = g[..., c].clone()
            g[sel] = 0.0
            g[..., c] = torch.where(sel, keep, g[..., c])
    elif pattern == 'neg_zero_rows':
        g[:, 1::3] = -0.0
    elif pattern == 'zero_run':
        q0, nq = Lq // 3, (64 + M - 1) // M + 2         # >= 64 consecutive items (b, q, m), not aligned to a wave
        assert q0 + nq <= Lq
        g[:, q0:q0 + nq] = 0.0
        g[:, q0 - 1, M - 1] = 0.0
    elif pattern == 'all_zero':
        g.zero_()
    else:
        raise ValueError(pattern)
    zero_items = (g == 0).all(-1)
    return g.view(B, Lq, MD).contiguous(), zero_items
