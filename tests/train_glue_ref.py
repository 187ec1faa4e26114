"""float64 restatements, case generators, mutants and assertion functions for the small kernels that join the training
step: csrc/ln_dropout_train.hip, csrc/rows_index.hip, csrc/sca_prep.hip and csrc/point_sampling.hip.
CPU only: nothing here imports the package or touches a GPU.

The manner of tests/exact_cases.py and tests/ln_bound.py: seeded generators, a Case with inputs and a float64 ref(mut=None),
bit comparison wherever the arithmetic is exact, and bounds counted from the kernel sources (tests/ln_bound.py for the
LayerNorm, C_POINT below for the projection).  The assertion functions here are the ones tests/test_gpu_train_glue.py
applies to the device results; tests/test_train_glue_host.py applies the same functions to the mutants of the
restatements, which must fail them.

DropoutAddLayerNorm.  z = x keep scale + residual is built backwards: the wanted z (the four row kinds of ln_bound,
integers) and a non-zero integer x are drawn, the keep mask follows from the seed the node will draw, and
residual = z - x keep scale.  With p in {0, 0.5, 0.75} scale is 1, 2 or 4 and every value is an exact integer; one wrong
keep decision moves an element of z by |x| scale >= 1.  Row r is served by wave r % 4 of block (r / 4) % blocks, so the
row kinds go by (r + r / 4) % 4: every wave slot and every grid-stride iteration meets all four.

rows_gather_sum.  |x| < 2^20 and K <= 8 summands: every sum is exact.

SCAPrep.  The exact half: level shapes that are powers of two, offsets in sixteenths, dyadic anchors and logits equal
within a softmax group, so exp(x - max) = 1, the sum is 32 and attn = 1/32: fdiv is faithful, hence exact where the quotient
is representable.  The general half keeps the bounds of tests/grad_bounds.py.

point_sampling.  Per point, from the fp32 inputs in float64: cam = (lidar2img @ ego2lidar) @ [ref * range + min, 1],
u = cam_x / max(cam_z, eps) / img_w, v likewise.  C_POINT counts the kernel's roundings in front of a comparison, each
relative to the same expression evaluated on absolute values (cam_a):
    an element of T = lidar2img @ ego2lidar: a 4-term chain (one product, three fmas):          4
    ref * range + min:                                                                          2
    cam = T @ [X, 1]: a 4-term chain:                                                           4
  so |cam - computed cam| <= 10 U cam_a, and for z against eps that is all.  u and v take two divisions more (2), and to
  first order the quotient x / z inherits 10 U cam_a_x / z + |x| / z * 10 U cam_a_z / z:
    |u - computed u| <= C_POINT U (cam_a_x / z + |cam_x| / z * cam_a_z / z) / img_w,            c = 12 -> C_POINT = 13.
  A point is undecidable when cam_z - eps, or (in front of the camera) one of u, 1 - u, v, 1 - v, is within that bound of
  zero.  Behind the camera, decidably, the mask is False whatever u and v are."""
import functools

import numpy as np
import torch

from tests import exact_cases as ec
from tests import ln_bound as lb
from tests.exact_cases import Case

U = lb.U


def _ratio(got, want, bound):
    """max |got - want| / bound (inf where a zero bound is missed or the result is not finite)."""
    err = (got.detach().cpu().double() - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, 0.0, float("inf")))
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- DropoutAddLayerNorm ---------------------------------------------------------------------------------------------------

C = 256
LN_P = (0.0, 0.5, 0.75)
LN_SCALE = {0.0: 1.0, 0.5: 2.0, 0.75: 4.0}
# 4097: the first second iteration of a wave; 8197: waves with two and with three iterations
LN_ROWS = (1, 3, 4, 5, 4096, 4097, 8197)
# block counts on either side of every boundary of ln_colsum_reduce_kernel's two loops (b + 24 < blocks, step 32; tail step 8)
LN_BLOCKS = (1, 2, 7, 8, 9, 24, 25, 31, 32, 33, 57, 64, 65, 1024)
LN_BLOCK_ROWS = tuple(4 * b - b % 4 for b in LN_BLOCKS if b not in (1, 2, 1024))          # full and ragged last blocks
LN_GY_AMP = 8
LN_MUTANTS = ("skip_ge_4096", "drop_last_block", "unroll_le")


def ln_train_blocks(rows):
    """csrc/ln_dropout_train.hip::ln_train_blocks."""
    return min(max((rows + 3) // 4, 1), 1024)


def keep_mask(n, seed, p):
    """numpy restatement of csrc/ln_dropout_train.hip's keep decision for elements 0 .. n-1."""
    i = np.arange(n, dtype=np.uint32)
    s0, s1 = np.uint32(seed & 0xffffffff), np.uint32(seed >> 32)
    with np.errstate(over='ignore'):
        h = i ^ s0
        h ^= h >> np.uint32(16); h *= np.uint32(0x85ebca6b); h ^= h >> np.uint32(13); h *= np.uint32(0xc2b2ae35); h ^= h >> np.uint32(16)
        h += s1
        h ^= h >> np.uint32(15); h *= np.uint32(0x2c1b3c6d); h ^= h >> np.uint32(12)
    return h >= np.uint32(int(p * 4294967296.0))


def drawn_seed(torch_seed):
    """The seed DropoutAddLayerNormFunction.forward draws from torch's CPU generator right after torch.manual_seed(torch_seed)."""
    g = torch.Generator().manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=g).item())


def ln_row_kinds(rows):
    i = torch.arange(rows)
    return (i + i // 4) % 4


def colsum_reduce(partial, mut=None):
    """ln_colsum_reduce_kernel, loop for loop, in the dtype of `partial` (blocks, columns).  MUTANT unroll_le: the unrolled
    loop runs while b + 24 <= blocks and reads the row behind the buffer, modelled as a row of ones (anything but zeros)."""
    blocks, ncol = partial.shape
    pad = torch.cat([partial, torch.ones(1, ncol, dtype=partial.dtype)])
    zero = torch.zeros(ncol, dtype=partial.dtype)
    red = []
    for rg in range(8):
        s, b = [zero, zero, zero, zero], rg
        while (b + 24 <= blocks) if mut == "unroll_le" else (b + 24 < blocks):
            s = [s[j] + pad[b + 8 * j] for j in range(4)]
            b += 32
        while b < blocks:
            s[0] = s[0] + pad[b]
            b += 8
        red.append((s[0] + s[1]) + (s[2] + s[3]))
    out = red[0]
    for r in range(1, 8):
        out = out + red[r]
    return out


def block_partials(terms, mut=None):
    """(rows, columns) per-row terms -> (blocks, columns): row r belongs to block (r / 4) % blocks.  MUTANTS: the rows from
    4096 on (all that only the grid-stride loop reaches) are skipped; the last block's partial sums are dropped."""
    rows = terms.shape[0]
    blocks = ln_train_blocks(rows)
    r = torch.arange(rows)
    if mut == "skip_ge_4096":
        terms = terms * (r < 4096).to(terms.dtype)[:, None]
    part = torch.zeros(blocks, terms.shape[1], dtype=terms.dtype).index_add_(0, (r // 4) % blocks, terms)
    if mut == "drop_last_block":
        part[blocks - 1] = 0.0
    return part


class LnTrainRef:
    """float64: ln (the LnRef of z), gres and dgamma with the sums of magnitudes their bounds are counted on, dbeta."""

    def __init__(self, c, mut=None):
        self.ln = ln = lb.LnRef(c["z"], c["gamma"], c["beta"])
        gy, gamma = c["gy"], c["gamma"].double()
        self.zh = zh = ln.d * ln.rstd
        w = gy * gamma
        c1, c2 = w.mean(1, keepdim=True), (w * zh).mean(1, keepdim=True)
        self.gres = ln.rstd * (w - c1 - zh * c2)
        self.gres_mag = ln.rstd * (w.abs() + w.abs().mean(1, keepdim=True) + zh.abs() * (w * zh).abs().mean(1, keepdim=True))
        self.dgamma = colsum_reduce(block_partials(gy * zh, mut), mut)
        self.dgamma_mag = (gy * zh).abs().sum(0)
        self.dbeta = colsum_reduce(block_partials(gy, mut), mut)
        self.keep, self.scale = c["keep"], c["scale"]


def _ln_train_fn(c, mut=None):
    return LnTrainRef(c, mut)


@functools.lru_cache(maxsize=4)
def ln_train_case(rows, p):
    """-> Case; inp: x, res, gy, z (float64 integers), keep (bool), gamma / beta (float32), kind, scale, p, torch_seed (what to
    pass to torch.manual_seed in front of the node) and seed (what the node then draws)."""
    g = ec._gen("ln_train", rows, p)
    torch_seed = 1000 + rows
    seed = drawn_seed(torch_seed) if p > 0 else 0
    scale = LN_SCALE[p]
    kind = ln_row_kinds(rows)
    i = torch.arange(rows)
    z = ec.ints(g, (rows, C), 50000)
    off = ec.ints(g, (rows, C), 50) + 30000.0
    const = ec.ints(g, (rows, 1), 30000, lo=1000).expand(rows, C).clone()
    const[i, torch.randint(0, C, (rows,), generator=g)] += (kind == lb.NEAR_CONSTANT).double()
    z = torch.where((kind == lb.OFFSET)[:, None], off, torch.where((kind >= lb.NEAR_CONSTANT)[:, None], const, z))
    keep = torch.from_numpy(keep_mask(rows * C, seed, p)).view(rows, C) if p > 0 else torch.ones(rows, C, dtype=torch.bool)
    x = ec.ints(g, (rows, C), 8, lo=1)
    res = z - x * keep.double() * scale
    gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
    beta = torch.randn(C, generator=g)
    beta = torch.where(beta == 0, torch.ones_like(beta), beta)
    inp = dict(x=x, res=res, z=z, gy=ec.ints(g, (rows, C), LN_GY_AMP), keep=keep, gamma=gamma, beta=beta, kind=kind,
               scale=scale, p=p, torch_seed=torch_seed, seed=seed, rows=rows)
    return Case(("ln_train", rows, p), inp, _ln_train_fn)


def ln_train_cases():
    """(rows, p): every p at the grid-stride row counts, p = 0.5 at the row counts that walk the reduce's block counts."""
    return [(rows, p) for rows in LN_ROWS for p in LN_P] + [(rows, 0.5) for rows in LN_BLOCK_ROWS]


def assert_ln_train_inputs(c):
    """The preconditions: integer x / residual / gy, z = x keep scale + residual an integer inside ln_bound's precondition,
    and |gy| <= 8 with no more than 8197 rows, so that every partial column sum of gy is an integer below 2^24."""
    for k in ("x", "res", "gy", "z"):
        assert torch.equal(c[k], c[k].round()) and float(c[k].abs().max()) < ec.LIMIT
    assert torch.equal(c["x"] * c["keep"].double() * c["scale"] + c["res"], c["z"]) and float(c["x"].abs().min()) >= 1
    lb.assert_ln_inputs(c["z"])
    assert float(c["gy"].abs().max()) <= LN_GY_AMP and c["rows"] <= 8197
    assert float(c["gy"].abs().sum(0).max()) < ec.LIMIT
    assert bool((c["gamma"] > 0).any()) and bool((c["gamma"] < 0).any()) and bool((c["beta"] != 0).all())


def assert_ln_train_forward(y, ref):
    """y under LnRef.bound(C_TRAIN_LN) -> worst err / bound."""
    r = lb.worst_ratio(y, ref.ln, ref.ln.bound(lb.C_TRAIN_LN))
    assert r <= 1.0, f"y: worst err / bound = {r:.3g}"
    return r


def assert_ln_train_backward(gx, gres, dgamma, dbeta, ref):
    """dbeta bit for bit; g_residual and dgamma under their counted bounds; g_x = where(keep, scale * g_residual, 0) bit for
    bit (gx is None for p = 0, where the node returns g_residual itself) -> (worst ratio of g_residual, of dgamma)."""
    ec.assert_bit_equal(dbeta, ref.dbeta, "dbeta")
    r_g = _ratio(gres, ref.gres, lb.C_TRAIN_GRES * U * ref.gres_mag)
    assert r_g <= 1.0, f"g_residual: worst err / bound = {r_g:.3g}"
    r_d = _ratio(dgamma, ref.dgamma, lb.C_TRAIN_DGAMMA * U * ref.dgamma_mag)
    assert r_d <= 1.0, f"dgamma: worst err / bound = {r_d:.3g}"
    if gx is not None:
        want = torch.where(ref.keep, gres.detach().cpu().double() * ref.scale, torch.zeros((), dtype=torch.float64))
        ec.assert_bit_equal(gx, want + 0.0, "g_x against keep * scale * g_residual")
    return r_g, r_d


def _butterfly(v):
    """wave_sum: v += shfl_xor(v, d) for d = 32 .. 1 over the 64 lanes of the last dim."""
    lanes = torch.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ d]
    return v


def _quad(t):
    return (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])


def _rsqrt32(var, g):
    """rsqrtf off by -1, 0 or +1 ulp at random."""
    s = var.double().rsqrt().float()
    ulps = torch.randint(-1, 2, s.shape, generator=g).to(torch.int32)
    return torch.where(torch.isfinite(s) & (s > 0), (s.view(torch.int32) + ulps).view(torch.float32), s)


def emulate_train_ln(z, gamma, beta, g, form="two_pass", eps=lb.EPS):
    """fp32 LayerNorm in the form of dropout_add_ln_fwd_kernel: 64 lanes x 4 columns, wave_sum as a butterfly.  form: 'two_pass'
    (the kernel), or the wrong kernels 'one_pass' (var = E[z^2] - mean^2), 'bessel' (division by N - 1), 'no_eps'.
    -> y, mean, rstd (fp32)."""
    rows = z.shape[0]
    v = z.float().view(rows, 64, 4)
    mean = _butterfly(_quad(v)) * (1.0 / C)
    d = v - mean[..., None]
    if form == "one_pass":
        var = _butterfly(_quad(v * v)) * (1.0 / C) - mean * mean
    else:
        var = _butterfly(_quad(d * d)) * (1.0 / (C - 1 if form == "bessel" else C))
    if form != "no_eps":
        var = var + torch.tensor(eps, dtype=torch.float32)
    rstd = _rsqrt32(var, g)
    y = lb._fma32(d * rstd[..., None], gamma.float().view(1, 64, 4), beta.float().view(1, 64, 4))
    return y.view(rows, C), mean[:, 0], rstd[:, 0]


def emulate_train_ln_bwd(gy, z, mean, rstd, gamma):
    """fp32 dropout_add_ln_bwd_kernel + ln_colsum_reduce_kernel from the forward's fp32 statistics: the row quantities on
    64 lanes x 4, the column sums as an fma chain over a wave's rows, the block's four waves and the two-stage reduce.
    -> g_residual, dgamma, dbeta (fp32)."""
    rows = z.shape[0]
    g, v = gy.float().view(rows, 64, 4), z.float().view(rows, 64, 4)
    st_x, st_y = mean.view(rows, 1, 1), rstd.view(rows, 1, 1)
    h = (v - st_x) * st_y
    w = g * gamma.float().view(1, 64, 4)
    c1 = (_butterfly(_quad(w)) * (1.0 / C))[..., None]
    c2 = (_butterfly(_quad(w * h)) * (1.0 / C))[..., None]
    t = st_y * (w - c1 - h * c2)
    blocks = ln_train_blocks(rows)
    dg, db = torch.zeros(blocks * 4, C), torch.zeros(blocks * 4, C)
    gf, hf = g.view(rows, C), h.view(rows, C)
    for r0 in range(0, rows, blocks * 4):                       # one grid-stride iteration of every wave
        n = min(blocks * 4, rows - r0)
        dg[:n] = lb._fma32(gf[r0:r0 + n], hf[r0:r0 + n], dg[:n])
        db[:n] = db[:n] + gf[r0:r0 + n]
    part = lambda a: (a.view(blocks, 4, C)[:, 0] + a.view(blocks, 4, C)[:, 1]) + (a.view(blocks, 4, C)[:, 2] + a.view(blocks, 4, C)[:, 3])
    return t.view(rows, C), colsum_reduce(part(dg)), colsum_reduce(part(db))


# ---- rows_gather_sum -------------------------------------------------------------------------------------------------------

GATHER_AMP = 2 ** 20 - 1
# (B, rows_in, rows_out, F, K): rows_out * F / 4 threads, below 256 and no multiple of 256
GATHER_SHAPES = [(1, 5, 7, 4, 1), (3, 9, 11, 4, 3), (1, 37, 300, 4, 6), (3, 6, 3, 64, 6), (1, 37, 21, 64, 3), (3, 10, 5, 64, 1),
                 (3, 13, 5, 256, 6), (1, 10, 3, 256, 1), (1, 9, 7, 256, 3), (3, 7, 3, 768, 3), (1, 9, 3, 768, 6), (3, 4, 5, 768, 1)]
# (B, Q, cameras, F): a row_to_query map and its inverse
GATHER_PAIRS = [(3, 13, 5, 64), (1, 300, 4, 768), (2, 40, 3, 4)]
GATHER_MUTANTS = ("batch_stride", "drop_last_k", "pad_row0")


def gather_sum_ref(x, index, mut=None):
    """out[b, r] = sum over k with 0 <= index[r, k] < rows_in of x[b, index[r, k]] (float64).  MUTANTS: every batch reads
    batch 0; the last k is dropped; padding (-1) reads row 0."""
    B, rows_in, F = x.shape
    rows_out, K = index.shape
    out = torch.zeros(B, rows_out, F, dtype=torch.float64)
    src_x = x[:1].expand(B, rows_in, F) if mut == "batch_stride" else x
    for k in range(K - (1 if mut == "drop_last_k" else 0)):
        src = index[:, k]
        ok = (src >= 0) & (src < rows_in)
        if mut == "pad_row0":
            ok = ok | (src < 0)
        out += src_x[:, src.clamp(0, rows_in - 1)] * ok.double().view(1, -1, 1)
    return out


def _gather_fn(c, mut=None):
    return gather_sum_ref(c["x"], c["index"], mut)


@functools.lru_cache(maxsize=None)
def gather_case(B, rows_in, rows_out, F, K):
    """Row 0 holds an index equal to rows_in (skipped), row 1 is all padding, row 2 repeats its first index in its last
    column (K > 1: that row of x is summed twice)."""
    g = ec._gen("rows_gather", B, rows_in, rows_out, F, K)
    index = torch.randint(-1, rows_in, (rows_out, K), generator=g)
    index[0, 0] = rows_in
    index[1] = -1
    index[2, 0] = rows_in - 1
    index[2, K - 1] = rows_in - 1
    inp = dict(x=ec.ints(g, (B, rows_in, F), GATHER_AMP), index=index)
    return Case(("rows_gather", B, rows_in, rows_out, F, K), inp, _gather_fn)


def row_maps(g, Q, cams, kq, empty_cam, odd_len=False):
    """row_to_query (cams * max_len, 1) and its inverse query_to_rows (Q, kq), -1 = padding, as SpatialCrossAttention builds
    them: camera c's visible queries, ascending, in rows c * max_len ..; a query's rows in camera order.  Query q is seen by
    q % (kq + 1) cameras (so some by none, some by kq), never by `empty_cam`, whose rows are all padding."""
    live = [c for c in range(cams) if c != empty_cam]
    assert kq <= len(live)
    lists = [[] for _ in range(cams)]
    for q in range(Q):
        for c in torch.randperm(len(live), generator=g)[:q % (kq + 1)].tolist():
            lists[live[c]].append(q)
    max_len = max(len(l) for l in lists)
    if odd_len and max_len % 2 == 0:
        max_len += 1
    r2q = torch.full((cams * max_len, 1), -1, dtype=torch.long)
    q2r = torch.full((Q, kq), -1, dtype=torch.long)
    fill = [0] * Q
    for c, l in enumerate(lists):
        for j, q in enumerate(l):
            r2q[c * max_len + j, 0] = q
            q2r[q, fill[q]] = c * max_len + j
            fill[q] += 1
    return r2q, q2r


def scatter_rows(rows, r2q, Q):
    """The adjoint of the rebatch, from row_to_query alone: (B, R, F) -> (B, Q, F), padded rows dropped."""
    valid = (r2q[:, 0] >= 0).double().view(1, -1, 1)
    return torch.zeros(rows.shape[0], Q, rows.shape[2], dtype=torch.float64).index_add_(1, r2q[:, 0].clamp(min=0), rows * valid)


@functools.lru_cache(maxsize=None)
def gather_pair_case(B, Q, cams, F):
    """x (B, Q, F) gathered through row_to_query; its gradient for an integer gout is the gather-sum over query_to_rows.
    ref(): (out, grad), the gradient computed by scattering through row_to_query, not through the inverse map."""
    g = ec._gen("rows_gather_pair", B, Q, cams, F)
    r2q, q2r = row_maps(g, Q, cams, min(3, cams - 1), cams - 2)
    inp = dict(x=ec.ints(g, (B, Q, F), GATHER_AMP), gout=ec.ints(g, (B, r2q.shape[0], F), GATHER_AMP), r2q=r2q, q2r=q2r)
    return Case(("rows_gather_pair", B, Q, cams, F), inp,
                lambda c, mut=None: (gather_sum_ref(c["x"], c["r2q"], mut), scatter_rows(c["gout"], c["r2q"], Q)))


def assert_gather_inputs(x, K):
    assert torch.equal(x, x.round()) and K <= 8 and float(x.abs().max()) * K < ec.LIMIT


# ---- SCAPrep ---------------------------------------------------------------------------------------------------------------

PREP_M, PREP_L, PREP_P = 8, 4, 8
PREP_LP = PREP_L * PREP_P
PREP_NOFF = PREP_M * PREP_LP * 2
PREP_W = PREP_M * PREP_LP * 3
PREP_Q, PREP_CAMS, PREP_EMPTY_CAM = 13, 5, 2
PREP_Z = (1, 2, 4, 8)
PREP_COMBOS = [(1, 768, 1), (2, 776, 3), (1, 776, 3), (2, 768, 1)]          # (bs, proj_ld, Kq)
PREP_SHAPES_EXACT = ((16, 32), (8, 16), (4, 8), (2, 4))
PREP_SHAPES_REAL = ((20, 30), (10, 15), (5, 8), (3, 4))
PREP_MUTANTS = ("anchor_div", "swap_wh", "softmax_p", "no_max")


class PrepRef:
    def __init__(self, loc, attn, dproj):
        self.loc, self.attn, self.dproj = loc, attn, dproj


def _prep_fn(c, mut=None):
    """loc (bs, R, M, L, P, 2), attn (bs, R, M, L, P) and dproj (bs, Q, ld) in float64.  MUTANTS: point p pairs with anchor
    p // (P / Z); the offsets are divided by (H, W); the softmax runs over P alone; no max subtraction (in fp32, where it
    matters)."""
    M, L, P, LP = PREP_M, PREP_L, PREP_P, PREP_LP
    proj, r2q, ref_rb, shapes = c["proj"], c["r2q"], c["ref_rb"], c["shapes"]
    bs, Q, ld = proj.shape
    R, Z = r2q.shape[0], ref_rb.shape[2]
    q = r2q[:, 0]
    valid = (q >= 0).double().view(1, R, 1)
    rb = proj[:, q.clamp(min=0)] * valid
    off = rb[..., :PREP_NOFF].reshape(bs, R, M, L, P, 2)
    logit = rb[..., PREP_NOFF:PREP_W].reshape(bs, R, M, LP)
    if mut == "softmax_p":
        attn = logit.view(bs, R, M, L, P).softmax(-1)
    elif mut == "no_max":
        e = logit.float().exp()
        attn = (e / e.sum(-1, keepdim=True)).double().view(bs, R, M, L, P)
    else:
        attn = logit.softmax(-1).view(bs, R, M, L, P)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    if mut == "swap_wh":
        wh = wh.flip(1)
    p = torch.arange(P)
    anchor = ref_rb[:, :, (p // (P // Z)) if mut == "anchor_div" else (p % Z)]          # (bs, R, P, 2)
    loc = anchor[:, :, None, None] + off / wh.view(1, 1, 1, L, 1, 2)
    ga = c["g_attn"].view(bs, R, M, LP)
    a = attn.reshape(bs, R, M, LP)
    d_logit = a * (ga - (a * ga).sum(-1, keepdim=True))
    d_off = c["g_loc"] / wh.view(1, 1, 1, L, 1, 2)
    rows = torch.cat([d_off.reshape(bs, R, PREP_NOFF), d_logit.reshape(bs, R, M * LP)], -1)
    dproj = torch.zeros(bs, Q, ld, dtype=torch.float64)
    dproj[..., :PREP_W] = scatter_rows(rows, r2q, Q)
    return PrepRef(loc, attn, dproj)


@functools.lru_cache(maxsize=None)
def prep_case(Z, bs, ld, kq, exact):
    """Q = 13 queries on 5 cameras of an odd number of rows each (bs R and bs Q are no multiples of 4: the last block of
    either kernel has early-returning waves), camera 2 without a visible query, every (kq + 1)-th query seen by no camera.
    The columns of proj from 768 on (ld = 776) hold values the kernels must not use.
    exact: see the module docstring.  Otherwise real level shapes and random fp32 values; the logits of one softmax group
    of a visible query are spread over +-90, and another group has one logit 1e4 above the rest."""
    g = ec._gen("sca_prep", Z, bs, ld, kq, exact)
    M, L, P, LP, Q = PREP_M, PREP_L, PREP_P, PREP_LP, PREP_Q
    r2q, q2r = row_maps(g, Q, PREP_CAMS, kq, PREP_EMPTY_CAM, odd_len=True)
    R = r2q.shape[0]
    seen = int((q2r[:, 0] >= 0).nonzero()[0])
    if exact:
        proj = ec.ints(g, (bs, Q, ld), 64) / 16
        proj[..., PREP_NOFF:PREP_W] = (ec.ints(g, (bs, Q, M, 1), 40) / 8).expand(bs, Q, M, LP).reshape(bs, Q, M * LP)
        ref_rb = torch.randint(0, 65, (bs, R, Z, 2), generator=g).double() / 64
        g_loc, g_attn = ec.ints(g, (bs, R, M, L, P, 2), 8), ec.ints(g, (bs, R, M, L, P), 8)
    else:
        f = lambda *s: torch.randn(*s, generator=g).double()
        proj, g_loc, g_attn = f(bs, Q, ld), f(bs, R, M, L, P, 2), f(bs, R, M, L, P)
        proj[0, seen, PREP_NOFF:PREP_NOFF + LP] = ((torch.rand(LP, generator=g) * 180 - 90).float()).double()
        proj[bs - 1, seen, PREP_NOFF + LP + 5] += 1e4
        proj = proj.float().double()
        ref_rb = torch.rand(bs, R, Z, 2, generator=g).double()
    inp = dict(proj=proj, r2q=r2q, q2r=q2r, ref_rb=ref_rb, shapes=PREP_SHAPES_EXACT if exact else PREP_SHAPES_REAL,
               g_loc=g_loc, g_attn=g_attn, exact=exact, seen=seen, Z=Z)
    return Case(("sca_prep", Z, bs, ld, kq, "exact" if exact else "general"), inp, _prep_fn)


def prep_cases(exact):
    return [(Z, bs, ld, kq, exact) for Z in PREP_Z for (bs, ld, kq) in PREP_COMBOS]


def assert_prep_exact(loc, attn, dproj, ref, c):
    """Forward bit for bit (a padded row is loc = anchor, attn = 1/32); backward bit for bit, with exactly zero rows for
    unseen queries and exactly zero tail columns."""
    ec.assert_bit_equal(loc, ref.loc, "loc")
    ec.assert_bit_equal(attn, ref.attn, "attn")
    pad = c["r2q"][:, 0] < 0
    assert pad.any() and bool((ref.attn[:, pad] == 1.0 / PREP_LP).all())
    if dproj is not None:
        d = dproj.detach().cpu()
        ec.assert_bit_equal(d[..., :PREP_NOFF], ref.dproj[..., :PREP_NOFF] + 0.0, "dproj (offsets)")
        ec.assert_bit_equal(d[..., PREP_NOFF:PREP_W], ref.dproj[..., PREP_NOFF:PREP_W] + 0.0, "dproj (logits)")
        unseen = c["q2r"][:, 0] < 0
        assert unseen.sum() >= 2 and bool((d[:, unseen] == 0).all()), "rows of unseen queries are not exactly zero"
        assert bool((d[..., PREP_W:] == 0).all()), "tail columns are not exactly zero"


def assert_prep_general(loc, attn, dproj, ref):
    """Finite, and within the bounds of tests/grad_bounds.py of float64 -> the three errors."""
    from tests.grad_bounds import SCA_PREP_ATTN_ABS, SCA_PREP_GRAD_REL, SCA_PREP_LOC_ABS
    out = []
    for name, got, want, bound, rel in (("loc", loc, ref.loc, SCA_PREP_LOC_ABS, False), ("attn", attn, ref.attn, SCA_PREP_ATTN_ABS, False),
                                        ("dproj", dproj, ref.dproj, SCA_PREP_GRAD_REL, True)):
        if got is None:
            continue
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all()), f"{name} is not finite"
        e = float((got - want).abs().max())
        if rel:
            e /= float(want.abs().max())
        assert e < bound, f"{name}: {e:.3e} (bound {bound:.1e})"
        out.append(e)
    return out


# ---- point_sampling --------------------------------------------------------------------------------------------------------

C_POINT = 13
EPS_Z = float(np.float32(1e-5))
POINT_CAP = 1e-4                       # the largest undecidable share of a case's points
# (bev_h, bev_w, points per pillar, batch, ego2lidar moved): 300 or 299 queries; with a batch of 2, 600 threads (a ragged block)
POINT_GRIDS = [(20, 15, 4, 2, False), (13, 23, 8, 1, False), (12, 25, 8, 2, True)]
POINT_MUTANTS = ("ge", "swap_hw", "no_ego", "bit_shift")


def pillar_points(H, W, pillar_h, n, bs):
    """(bs, n, H * W, 3) normalised pillar points, query q = y * W + x (BEVFormerEncoder.get_reference_points, '3d')."""
    zs = torch.linspace(0.5, pillar_h - 0.5, n) / pillar_h
    xs = torch.linspace(0.5, W - 0.5, W) / W
    ys = torch.linspace(0.5, H - 0.5, H) / H
    ref = torch.stack((xs.view(1, 1, W).expand(n, H, W), ys.view(1, H, 1).expand(n, H, W), zs.view(-1, 1, 1).expand(n, H, W)), -1)
    return ref.reshape(n, H * W, 3)[None].repeat(bs, 1, 1, 1).contiguous()


def moved_ego2lidar():
    """A rigid transform that is not the identity (2 degrees of yaw and a small offset), in fp32."""
    a = np.radians(2.0)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = [0.3, -0.2, 0.1]
    return torch.from_numpy(m.astype(np.float32))


def _wrap32(bits):
    return ((bits + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


class PointRef:
    """float64 from the fp32 inputs: uv (NC, B, Nq, Z, 2), mask and front (z > eps) (NC, B, Nq, Z), vis (B, Nq) int32, and
    the decision set: z_dec (z is not within its bound of eps), decidable (the mask cannot be flipped by the kernel's
    roundings), uv_bound."""


def point_sampling_ref(ref_3d, lidar2img, ego2lidar, pc_range, img_h, img_w, mut=None, exact=False):
    """MUTANTS: 'ge' (the comparisons admit equality), 'swap_hw', 'no_ego' (ego2lidar dropped), 'bit_shift' (camera c sets
    bit c + 1).  exact: asserts that every product and partial sum of the kernel's chains is an fp32 value."""
    f32 = lambda v: float(np.float32(v))
    rng = torch.tensor([f32(pc_range[3] - pc_range[0]), f32(pc_range[4] - pc_range[1]), f32(pc_range[5] - pc_range[2])], dtype=torch.float64)
    org = torch.tensor([f32(pc_range[0]), f32(pc_range[1]), f32(pc_range[2])], dtype=torch.float64)
    A, E, p = lidar2img.double(), ego2lidar.double(), ref_3d.double()
    if mut == "no_ego":
        E = torch.eye(4, dtype=torch.float64)
    if mut == "swap_hw":
        img_h, img_w = img_w, img_h
    is32 = lambda t: torch.equal(t.float().double(), t)
    T, Ta = A @ E, A.abs() @ E.abs()                                                          # (B, NC, 4, 4)
    X, Xa = p * rng + org, p.abs() * rng.abs() + org.abs()                                    # (B, Z, Nq, 3)
    one = torch.ones_like(X[..., :1])
    X4, X4a = torch.cat([X, one], -1), torch.cat([Xa, one], -1)
    if exact:
        assert is32(T) and is32(p * rng) and is32(X)
        for i in range(3):
            s = torch.zeros(())
            for j in range(4):
                s = s + T[:, :, None, None, i, j] * X4[:, None, :, :, j]
                assert is32(s), "a partial sum of the projection is not an fp32 value"
    cam = torch.einsum('bcij,bzqj->cbqzi', T[:, :, :3], X4)
    cam_a = torch.einsum('bcij,bzqj->cbqzi', Ta[:, :, :3], X4a)
    r = PointRef()
    z = cam[..., 2]
    den = z.clamp(min=EPS_Z)
    wh = torch.tensor([float(img_w), float(img_h)], dtype=torch.float64)
    if exact:
        qd = cam[..., :2] / den[..., None]
        low = qd.contiguous().view(torch.int64) & ((1 << 29) - 1)                  # a double this close to a tie of the fp32
        assert not bool(((low - (1 << 28)).abs() <= 1).any())                      # grid could round twice: none is
        r.uv = qd.float().double() / wh
        assert is32(r.uv)
    else:
        r.uv = cam[..., :2] / den[..., None] / wh
    u, v = r.uv[..., 0], r.uv[..., 1]
    if mut == "ge":
        r.front = z >= EPS_Z
        r.mask = r.front & (v >= 0) & (v <= 1) & (u <= 1) & (u >= 0)
    else:
        r.front = z > EPS_Z
        r.mask = r.front & (v > 0) & (v < 1) & (u < 1) & (u > 0)
    NC = A.shape[1]
    bits = sum(r.mask[c].any(-1).long() << (c + 1 if mut == "bit_shift" else c) for c in range(NC))
    r.vis = _wrap32(bits)
    cu = C_POINT * U
    r.z_dec = (z - EPS_Z).abs() > cu * cam_a[..., 2]
    r.uv_bound = cu * (cam_a[..., :2] / den[..., None] + cam[..., :2].abs() / den[..., None] * (cam_a[..., 2] / den)[..., None]) / wh
    margin = torch.minimum(r.uv.abs(), (1 - r.uv).abs())
    uv_dec = (margin > r.uv_bound).all(-1)
    r.decidable = r.z_dec & (~r.front | uv_dec)
    return r


def assert_point_sampling(ref_cam, mask, vis, r):
    """bev_mask equals float64 at every decidable point, vis_bits wherever all of the query's points are decidable, ref_cam
    within the bound wherever the point is (decidably) in front of the camera -> worst err / bound of ref_cam."""
    ref_cam, mask, vis = ref_cam.detach().cpu(), mask.detach().cpu().bool(), vis.detach().cpu()
    bad = (mask != r.mask) & r.decidable
    assert not bool(bad.any()), f"{int(bad.sum())} decidable points with a wrong mask, first at {tuple(int(i) for i in bad.nonzero()[0])}"
    q_ok = r.decidable.all(-1).all(0)
    badv = (vis != r.vis) & q_ok
    assert not bool(badv.any()), f"{int(badv.sum())} visibility words differ, first at {tuple(int(i) for i in badv.nonzero()[0])}"
    front = r.front & r.z_dec
    ratio = _ratio(ref_cam[front], r.uv[front], r.uv_bound[front])
    assert ratio <= 1.0, f"ref_cam: worst err / bound = {ratio:.3g}"
    return ratio


def assert_point_sampling_exact(ref_cam, mask, vis, r):
    ref_cam, mask, vis = ref_cam.detach().cpu(), mask.detach().cpu().bool(), vis.detach().cpu()
    assert torch.equal(mask, r.mask), f"{int((mask != r.mask).sum())} mask bits differ"
    ec.assert_bit_equal(ref_cam, r.uv, "ref_cam")
    assert torch.equal(vis, r.vis), "vis_bits differ"


BOUNDARY_PC_RANGE = (-32.0, -32.0, -4.0, 32.0, 32.0, 4.0)
BOUNDARY_IMG = (256, 512)              # img_h, img_w
BOUNDARY_NC = (1, 6, 32)
# queries of batch 0, by name: (Y, Zm, which reference coordinate moves by how many ulps); X = 4 metres in front
_UV_POINTS = [("u0", -4.0, 0.0, 1, 0), ("u0_in", -4.0, 0.0, 1, 1), ("u0_out", -4.0, 0.0, 1, -1),
              ("u1", 4.0, 0.0, 1, 0), ("u1_in", 4.0, 0.0, 1, -1), ("u1_out", 4.0, 0.0, 1, 1),
              ("v0", 0.0, -2.0, 2, 0), ("v0_in", 0.0, -2.0, 2, 1), ("v0_out", 0.0, -2.0, 2, -2),
              ("v1", 0.0, 2.0, 2, 0), ("v1_in", 0.0, 2.0, 2, -1), ("v1_out", 0.0, 2.0, 2, 1),
              ("centre", 0.0, 0.0, 1, 0), ("behind", 0.0, 0.0, 1, 0)]
BOUNDARY_QUERIES = [n for n, *_ in _UV_POINTS]
# queries of batch 1: cam_z = eps + k ulp(eps)
_Z_POINTS = [("z_eps", 0.0), ("z_in", 1.0), ("z_out", -1.0)]


def _ulp_step(v, k):
    a = np.float32(v)
    for _ in range(abs(k)):
        a = np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return float(a)


@functools.lru_cache(maxsize=None)
def point_boundary_case(NC):
    """Every product and sum of the projection exact.  pc_range (-32, -32, -4, 32, 32, 4), a 512 x 256 image, ego2lidar = I.
    Batch 0, camera kinds by c % 3: 0 looks along +x with focal length 256 and principal point (256, 128); 1 the same with
    focal length 128; 2 is kind 0 negated (every point in front of kind 0 has z < 0 there: masked, ref_cam = xy / eps).
    Its queries sit 4 m in front (a power of two: the quotients are exact), anchor 0 on u = 0, u = 1, v = 0, v = 1 of kind 0
    or with ONE reference coordinate one fp32 ulp inside or outside (v0_out: two ulps, 0.25 being a power of two); anchor 1
    of every query is behind kinds 0 and 1, whose visibility bits are therefore anchor 0's.  Batch 1: cam_z = eps + k ulp(eps) for k = 0, 1, -1 through a z row (1, 0, ulp, eps) at
    X = 0, with cam_x = 256 cam_z and cam_y = 128 cam_z (kind 1: 128 and 64).
    -> dict(ref_3d (2, 2, Nq, 3), lidar2img (2, NC, 4, 4), ego2lidar, pc_range, img_h, img_w) in fp32."""
    img_h, img_w = BOUNDARY_IMG
    Nq = len(_UV_POINTS)
    ref = torch.zeros(2, 2, Nq, 3, dtype=torch.float64)
    ref[:, 1] = torch.tensor([28 / 64, 0.5, 0.5])                                  # anchor 1: X = -4
    for q, (name, Y, Zm, axis, k) in enumerate(_UV_POINTS):
        pt = [36 / 64 if name != "behind" else 28 / 64, (Y + 32) / 64, (Zm + 4) / 8]
        pt[axis] = _ulp_step(pt[axis], k)
        ref[0, 0, q] = torch.tensor(pt, dtype=torch.float64)
    ref[1, 0] = torch.tensor([0.5, 0.5, 5 / 8])                                    # batch 1 filler: z one ulp inside
    for q, (name, k) in enumerate(_Z_POINTS):
        ref[1, 0, q] = torch.tensor([0.5, 0.5, (k + 4) / 8])
    ref[1, 1] = ref[1, 0, 2]                                                       # batch 1, anchor 1: z one ulp outside
    ulp = float(np.spacing(np.float32(EPS_Z)))
    A = torch.zeros(2, NC, 4, 4, dtype=torch.float64)
    for c in range(NC):
        f = 256.0 if c % 3 != 1 else 128.0
        sign = -1.0 if c % 3 == 2 else 1.0
        A[0, c, 0, :2] = torch.tensor([256.0, f]) * sign
        A[0, c, 1, 0], A[0, c, 1, 2] = 128.0 * sign, f * sign
        A[0, c, 2, 0] = sign
        zrow = torch.tensor([1.0, 0.0, ulp, EPS_Z]) * sign
        A[1, c, 2] = zrow
        A[1, c, 0], A[1, c, 1] = zrow * f, zrow * (f / 2)
        A[:, c, 3, 3] = 1.0
    assert torch.equal(ref.float().double(), ref) and torch.equal(A.float().double(), A)
    return dict(ref_3d=ref.float(), lidar2img=A.float(), ego2lidar=torch.eye(4), pc_range=BOUNDARY_PC_RANGE,
                img_h=img_h, img_w=img_w)
