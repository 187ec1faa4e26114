"""The LayerNorms of the Linear kernels on exact integer inputs, under an error bound counted from the kernel sources.
CPU only: nothing here imports the package or touches a GPU.

The input x of the LayerNorm (x = a . Wo^T + bo + residual, or the FFN's pre2 of tests/exact_cases.ffn_case) is an exact
integer in every kernel: the contraction meets the 2^24 precondition of tests/exact_cases.py.  Every row also has
sum |x| < 2^24 and |x - mean| < 2^16, so for a power-of-two N the row sum (any order), the mean (a multiple of 1/N) and
the deviations d = x - mean (multiples of 1/N below 2^16: at most 24 bits) are fp32 values: a correct kernel computes them
without any rounding.  What is left are the LayerNorm's own roundings, and the float64 reference differs from a correct
kernel by those alone.  With t = d * rstd * gamma and y = t + beta from float64, per element

    |got - y|  <=  c * U * |t|  +  U * |y|,          U = 2^-24, the unit roundoff of fp32 (half an ulp, relative).

U |y| is the final rounding (of the fma, or of the addition of beta), which no implementation avoids.  c counts every
rounding in front of it, to first order; each count is rounded up to the next integer, which covers the higher-order
terms (c^2 U^2 / 2 < 1e-11 U) and the difference between U |y| and U |computed y|.

rsqrtf: no statement of its accuracy was found in the HIP math documentation of the ROCm tree the library is built with
(none is installed with it), so 2 ulp = 4 U is taken.

ch_layernorm (csrc/linear_chain_x3.hip; linear_ln_chain and both LayerNorms of encoder_ffn_chain), N = 256:
    variance: a lane sums its 32 squared deviations with v = fmaf(d, d, v): 32 roundings, each at most U of a partial sum
      of non-negative terms, so at most U of the total;  v += shfl_xor(v, 32): 1;  the four-wave exchange
      (r0 + r1) + (r2 + r3): 2 on any path;  * (1 / 256): exact;  + eps: 1.   36 U on var + eps, which enters
      rstd = (var + eps)^(-1/2) at half weight:                                                         18 U
    rsqrtf:                                                                                                 4 U
    d * rstd:                                                                                               1 U
    fmaf(., gamma, beta): its one rounding is the U |y| term.
    c = 23 -> C_CHAIN = 24.

The ln= epilogue of linear (csrc/linear_mfma.hip and csrc/linear_bf16x3.hip, the same code), N <= 256 on 64 lanes x 4:
    variance: (dx dx + dy dy) + (dz dz + dw dw), contracted to fmas or not: at most 3 roundings on any path;  wave_sum:
      6 shuffle additions;  * inv_n: exact for a power-of-two N;  + eps: 1.   10 U, at half weight:      5 U
    rsqrtf:                                                                                                 4 U
    d * rstd:                                                                                               1 U
    * gamma (a rounding of its own unless it is contracted with + beta):                                    1 U
    c = 11 -> C_LINEAR = 12.
  N = 100: inv_n = fdiv(1, 100) is not exact.  fdiv is faithful (1 ulp = 2 U), the products S * inv_n and
  ssq * inv_n round once more (3 U each), and x - mean is no longer exact (1 U of |d|):
    variance 13 U at half weight 6.5 U, rsqrtf 4 U, x - mean 1 U, d * rstd 1 U, * gamma 1 U:   13.5 -> C_LINEAR_INEXACT = 14.
  The computed mean itself is off by up to delta = 3 U |mean| (MEAN_ROUNDINGS): no fp32 LayerNorm over 100 columns
  holds the mean of a row exactly.  It moves every deviation by delta and, as sum d = 0, the variance by exactly
  delta^2, so for such N the bound has two more terms:
      + delta * rstd * |gamma|  +  delta^2 / (2 (var + eps)) * |t|.
  Both vanish for a power-of-two N, where the bound is the one above.

dropout_add_ln_fwd_kernel (csrc/ln_dropout_train.hip), N = 256 on 64 lanes x 4.  z = x keep scale + residual is an exact
integer (tests/train_glue_ref.py), the row sum, the mean and d = z - mean are exact as above:
    variance: (dx dx + dy dy) + (dz dz + dw dw), contracted to fmas or not: at most 3 roundings on any path;  wave_sum:
      6 shuffle additions;  * (1 / 256): exact;  + eps: 1.   10 U, at half weight:                          5 U
    rsqrtf:                                                                                                 4 U
    d * rstd:                                                                                               1 U
    fmaf(., gamma, beta): its one rounding is the U |y| term.
    c = 10 -> C_TRAIN_LN = 11.
  The stored rstd is off by the first two lines, 9 U: RSTD_ROUNDINGS.

dropout_add_ln_bwd_kernel, per element, with zh = d rstd, w = gy gamma, c1 = mean_c(w), c2 = mean_c(w zh) in float64:
  g_residual = rstd (w - c1 - zh c2).  The kernel's h = d * rstd: 9 U + its product 1 U = 10 U |zh|.
    w = gy * gamma:                                                                       1 U |w|
    c1: the terms 1 U each, (wx + wy) + (wz + ww) 2 additions, wave_sum 6:                9 U mean|w|
    c2: a term w h is 1 + 10 + 1 (its product) = 12 U, the same 8 additions:             20 U mean|w zh|
    h * c2: 10 + 20 + 1 (the product, unless contracted):                                31 U |zh| mean|w zh|
    (w - c1) - h c2: two roundings, each at most U (|w| + mean|w| + |zh| mean|w zh|)
    rstd * (.): 9 U of rstd + 1 for the product, on the same sum of magnitudes:          10 U
  |w|: 1 + 2 + 10 = 13, mean|w|: 9 + 2 + 10 = 21, |zh| mean|w zh|: 31 + 2 + 10 = 43.  The largest covers all three:
    |got - g_residual|  <=  C_TRAIN_GRES U rstd (|w| + mean|w| + |zh| mean|w zh|),   c = 43 -> C_TRAIN_GRES = 44.
  dgamma = sum_rows gy zh.  A term gy * h carries the 10 U of h.  The longest addition chain on any path, at no more than
  8197 rows (1024 blocks of 4 waves, at most 3 rows per wave):
    dg = fmaf(gy, h, dg) per row of the wave:                                             3
    (red[0] + red[1]) + (red[2] + red[3]) of the block:                                   2
    ln_colsum_reduce_kernel: s0 takes 1024 / 32 = 32 terms in the unrolled loop and up to 3 in its tail:  35
    (s0 + s1) + (s2 + s3):                                                                2
    the 8 row groups, one after the other:                                                7
    49 additions, each at most U of a partial sum of magnitudes, and the 10 U of h:
    |got - dgamma|  <=  C_TRAIN_DGAMMA U sum_rows |gy zh|,                             c = 59 -> C_TRAIN_DGAMMA = 60.
  dbeta = sum_rows gy has no bound: with |gy| <= 8 every partial sum is an integer below 2^24, the sum is exact."""
import torch

from tests import exact_cases as ec

U = 2.0 ** -24
RSQRT_ULPS = 2
C_CHAIN = 24
C_LINEAR = 12
C_LINEAR_INEXACT = 14
MEAN_ROUNDINGS = 3
C_TRAIN_LN = 11
RSTD_ROUNDINGS = 9
C_TRAIN_GRES = 44
C_TRAIN_DGAMMA = 60
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # the fp32 value the kernels add

ORDINARY, OFFSET, NEAR_CONSTANT, CONSTANT = 0, 1, 2, 3


class LnRef:
    """float64: x (M, N), mean, var, rstd (M, 1), t = d rstd gamma, y = t + beta."""

    def __init__(self, x, gamma, beta, eps=EPS):
        self.x, self.gamma, self.beta, self.eps = x, gamma.double(), beta.double(), eps
        self.mean = x.mean(1, keepdim=True)
        self.d = x - self.mean
        self.var = (self.d * self.d).mean(1, keepdim=True)
        self.rstd = (self.var + eps).rsqrt()
        self.t = self.d * self.rstd * self.gamma
        self.y = self.t + self.beta

    def bound(self, c, mean_roundings=0):
        b = c * U * self.t.abs() + U * self.y.abs()
        if mean_roundings:
            delta = mean_roundings * U * self.mean.abs()
            b = b + delta * self.rstd * self.gamma.abs() + delta * delta / (2.0 * (self.var + self.eps)) * self.t.abs()
        return b


def linear_c(N):
    """(c, roundings of the mean) of the ln= epilogue of linear for N columns."""
    return (C_LINEAR, 0) if N & (N - 1) == 0 else (C_LINEAR_INEXACT, MEAN_ROUNDINGS)


def worst_ratio(got, ref, bound):
    """max err / bound over the elements (inf where a zero bound is missed or the result is not finite)."""
    err = (got.detach().cpu().double() - ref.y).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, 0.0, float("inf")))
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def assert_ln_inputs(x):
    """The precondition on the LayerNorm's input: integers with row sums below 2^24 and, for a power-of-two N, deviations
    from the mean that are fp32 values."""
    N = x.shape[1]
    assert torch.equal(x, x.round()) and float(x.abs().sum(1).max()) < ec.LIMIT
    d = x - x.mean(1, keepdim=True)
    assert float(d.abs().max()) < 2.0 ** 16
    if N & (N - 1) == 0:
        assert torch.equal(d.float().double(), d)


def ln_case(M, N, K=256):
    """x = a . Wo^T + bo + res with the four row kinds interleaved (row i is of kind i % 4, so every tile holds several of
    each): ordinary rows (|x| up to 6e4), offset rows (mean 3e4, std about 70: |mean| / std > 100; narrow a and a residual
    of 30000 +- 50), constant rows (a = 0 and a residual of C - bo: x = C in every column, with a bias that is not zero)
    and near-constant rows (as constant, one element off by 1: eps is 0.25 % of the variance).
    -> dict(a, wo, bo, res, gamma, beta, kind, x, abs): float64 tensors, gamma / beta float32."""
    g = ec._gen("ln", M, N, K)
    kind = torch.arange(M) % 4
    a, wo, bo = ec.ints(g, (M, K), 8), ec.ints(g, (N, K), 8), ec.ints(g, (N,), 32)
    a[kind == OFFSET] = ec.ints(g, (int((kind == OFFSET).sum()), K), 1)
    a[kind >= NEAR_CONSTANT] = 0.0
    res = ec.ints(g, (M, N), 58000)
    off = ec.ints(g, (M, N), 50) + 30000.0
    const = ec.ints(g, (M, 1), 30000, lo=1000) - bo
    const[torch.arange(M), torch.randint(0, N, (M,), generator=g)] += (kind == NEAR_CONSTANT).double()
    res = torch.where((kind == OFFSET)[:, None], off, torch.where((kind >= NEAR_CONSTANT)[:, None], const, res))
    gamma = (torch.rand(N, generator=g) + 0.5) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1).float()
    beta = torch.randn(N, generator=g)
    x = a @ wo.t() + bo + res
    ab = a.abs() @ wo.abs().t() + bo.abs() + res.abs()
    return dict(a=a, wo=wo, bo=bo, res=res, gamma=gamma, beta=beta, kind=kind, x=x, abs=ab)


# ---- fp32 emulations of the kernels' form, and of three wrong ones ----------------------------------------------------------

def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _tree_sum(terms, squares):
    """The summation tree of ch_layernorm over (M, 256) fp32 terms: 8 chains of 32 (fmaf(d, d, v) when `squares`), a
    pairwise addition (the shuffle), then (r0 + r1) + (r2 + r3)."""
    M = terms.shape[0]
    ch = terms.view(M, 8, 32)
    v = torch.zeros(M, 8)
    for k in range(32):
        v = _fma32(ch[:, :, k], ch[:, :, k], v) if squares else v + ch[:, :, k]
    w = v[:, 0::2] + v[:, 1::2]
    return ((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]))[:, None]


def emulate(x, gamma, beta, g, form="two_pass", eps=EPS):
    """fp32 LayerNorm over 256 columns in the form of ch_layernorm, the columns dealt to the summation chains in a
    random order, rsqrt off by -1, 0 or +1 ulp at random.  form: 'two_pass' (the kernel), or one of the wrong kernels
    'one_pass' (var = E[x^2] - mean^2), 'bessel' (division by N - 1), 'no_eps'."""
    M, N = x.shape
    assert N == 256
    perm = torch.randperm(N, generator=g)
    xs = x.float()[:, perm]
    mean = _tree_sum(xs, False) * (1.0 / N)
    d = xs - mean
    if form == "one_pass":
        var = _tree_sum(xs, True) * (1.0 / N) - mean * mean
    else:
        var = _tree_sum(d, True) * (1.0 / (N - 1 if form == "bessel" else N))
    if form != "no_eps":
        var = var + torch.tensor(eps, dtype=torch.float32)
    s = var.double().rsqrt().float()
    ulps = torch.randint(-1, 2, s.shape, generator=g).to(torch.int32)
    s = torch.where(torch.isfinite(s) & (s > 0), (s.view(torch.int32) + ulps).view(torch.float32), s)
    y = torch.empty(M, N)
    y[:, perm] = _fma32(d * s, gamma.float()[perm][None], beta.float()[perm][None])
    return y
