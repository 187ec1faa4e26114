"""Exact-arithmetic cases for the matrix-core kernels: generators, float64 references, mutants and the bit comparator.
CPU only: nothing here imports the package or touches a GPU.

The idea.  Operands are integers (or integers times a power of two) chosen so that for every contraction of a case
    sum |a| |b| + |bias| + |residual|  <  2^24   in units of the smallest operand bit.
Then every partial sum, in any order and on any MFMA shape, split-K or tile walk, is an integer below 2^24 and the fp32
accumulator holds the mathematically exact value.  A correct kernel therefore returns exactly rne_bf16(float64 result)
for a bf16 output and exactly the float64 result for an fp32 output: no tolerance is chosen anywhere.
`assert_exact_inputs` asserts the precondition, `rounding_profile` shows that the rounding itself is exercised (values
that are not bf16-representable, exact ties, negative pre-activations), the mutants show that the oracle notices wrong
kernels, and `diff_report` / `assert_bit_equal` compare bit patterns.

The bf16x3 kernels compute Ah.Bh + Ah.Bl + Al.Bh on hi/lo bf16 planes (hi = rne(x), lo = rne(x - hi)) and drop Al.Bl.
Their cases come in flavours: one operand is "wide" (integers of up to 12 bits, which need the low plane and are exactly
hi + lo), the others are bf16-exact (|int| <= 8, low plane zero), so the dropped product is zero and the result is exact.
Each flavour fails exactly when the low-part product of ITS wide operand is missing.  The precondition of these cases is
taken on |hi| + |lo| of the wide operand (the planes the kernel really multiplies).

The linear_*_chain kernels are covered stage by stage: linear_pair_chain as it stands, the tails of linear_ln_chain and
encoder_ffn_chain and the latter's FFN behind a LayerNorm whose gamma is zero (its output is then the row beta, exactly).
A LayerNorm itself is not exact: the chains' LayerNorms and the ln= epilogue of linear are checked on exact integer
inputs under an error bound counted from the kernel source (tests/ln_bound.py).

Out of scope (their transcendentals, divisions or square roots are not exact): the Softplus epilogue, occ_heads, the
BatchNorm statistics kernels and the heads-loss kernels.  The gather kernels already have float64 tests in every mode;
bias_relu_maxpool_nhwc and bias_act_nhwc_ are already compared bit for bit."""
import functools

import torch

F = torch.nn.functional
LIMIT = float(2 ** 24)

MUTANTS = ("trunc", "half_away", "drop_k", "edge_pad", "skip_mid_round", "drop_low", "stride_off", "up_off", "trunc_in",
           "term_last_group", "term_on_zv", "bias_pass0", "tile_copy", "no_relu", "no_x2")


# ---- number formats --------------------------------------------------------------------------------------------------

def _f32(t64):
    f = t64.float()
    assert torch.equal(f.double(), t64), "a float64 reference value does not survive .float(): the case is not exact"
    return f


def rne_bf16(t64):
    """float64 -> the bf16 value nearest-even, as float64 (through .float().to(bfloat16), the value fp32-exact)."""
    return _f32(t64).to(torch.bfloat16).double()


def to_bf16(t64):
    """float64 -> bfloat16 tensor (RNE)."""
    return _f32(t64).to(torch.bfloat16)


def _bits(t64):
    return _f32(t64).contiguous().view(torch.int32)


def trunc_bf16(t64):
    """MUTANT rounding: drop the low 16 bits."""
    return (_bits(t64) & -65536).view(torch.float32).double()


def half_away_bf16(t64):
    """MUTANT rounding: nearest, ties away from zero."""
    b = _bits(t64)
    mag = ((b & 0x7fffffff) + 0x8000) & -65536
    return (mag | (b & -2147483648)).view(torch.float32).double()


def is_bf16(t64):
    return rne_bf16(t64) == t64


def bf16_split(t64):
    """The bf16x3 operand split of the kernels: hi = rne(x), lo = rne(x - hi) (float64 tensors)."""
    hi = rne_bf16(t64)
    lo = rne_bf16(t64 - hi)
    return hi, lo


def split_abs(t64):
    """|hi| + |lo|: what the absolute-value contraction of a bf16x3 kernel sees; asserts hi + lo == x."""
    hi, lo = bf16_split(t64)
    assert torch.equal(hi + lo, t64), "operand is not exactly hi + lo"
    return hi.abs() + lo.abs()


def rounding_profile(pre, relu=False):
    """pre: the float64 pre-activation.  -> (share of the values to be rounded that are not bf16-representable, share
    that are exact ties (low 16 bits of the fp32 pattern == 0x8000), share of negative pre-activations).  With relu the
    first two are taken on relu(pre), the values the kernel rounds."""
    v = pre.relu() if relu else pre
    low = _bits(v) & 0xffff
    n = float(v.numel())
    return float((low != 0).sum()) / n, float((low == 0x8000).sum()) / n, float((pre < 0).sum()) / n


# ---- comparator ------------------------------------------------------------------------------------------------------

def diff_report(got, want):
    """None when `got` equals `want` bit for bit, else a description.  bf16: int16 patterns of got against the bf16
    reference; fp32: got.double() == want (float64).  Both on the CPU, same shape."""
    got = got.detach().cpu()
    if tuple(got.shape) != tuple(want.shape):
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    if want.dtype == torch.bfloat16:
        assert got.dtype == torch.bfloat16
        ne = got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)
    else:
        assert want.dtype == torch.float64 and got.dtype in (torch.float32, torch.float64)
        ne = got.double() != want
    n = int(ne.sum())
    if n == 0:
        return None
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return (f"{n} of {ne.numel()} elements differ; first at {idx}: got {float(got[idx]):.10g}, "
            f"want {float(want[idx]):.10g}")


def assert_bit_equal(got, want, what=""):
    rep = diff_report(got, want)
    assert rep is None, f"{what}: {rep}"


# ---- references: result container and the mutant hooks -----------------------------------------------------------------

class Ref:
    """pre: float64 pre-activation of the (last) stage; value: what is rounded / returned (float64, after ReLU and any
    fp32 tail); out: the expected output (bfloat16 tensor, or float64 for fp32 outputs); stages: [(name, abs-value
    contraction in units of the smallest operand bit)]; extra: further expected outputs by name."""

    def __init__(self, pre, value, out, stages, relu, extra=None):
        self.pre, self.value, self.out, self.stages, self.relu, self.extra = pre, value, out, stages, relu, extra or {}


def _round(v, mut):
    v = v + 0.0          # a zero sum is +0 (IEEE round-to-nearest; the accumulators start at +0), also where float64 summed only -0 terms
    if mut == "trunc":
        return trunc_bf16(v).float().to(torch.bfloat16)
    if mut == "half_away":
        return half_away_bf16(v).float().to(torch.bfloat16)
    return to_bf16(v)


def _mid(v, mut):
    return v if mut == "skip_mid_round" else rne_bf16(v)


def _drop_k(w, mut):
    """MUTANT: one contraction element whose weight is +-1 is dropped."""
    if mut != "drop_k":
        return w
    flat = w.clone().reshape(-1)
    hit = (flat.abs() == 1).nonzero()
    assert hit.numel(), "no weight of magnitude 1 in this case"
    flat[int(hit[0])] = 0.0
    return flat.view_as(w)


def _pad2(x, p, mut):
    """Zero padding of the two last dims; MUTANT edge_pad: the left border replicates the first column."""
    xp = F.pad(x, (p, p, p, p))
    if mut == "edge_pad":
        xp[..., p:-p, :p] = x[..., :, :1]
    return xp


def _shift2(x, mut):
    """MUTANT stride_off: the map seen one pixel down-right (zeros enter at the end), so a stride-2 walk samples the
    pixel next to the right one."""
    if mut != "stride_off":
        return x
    out = torch.zeros_like(x)
    out[..., :-1, :-1] = x[..., 1:, 1:]
    return out


def _sample(x, s, mut):
    if s == 1:
        return x
    return _shift2(x, mut)[..., ::s, ::s]


def _up2(r, Ho, Wo, mut):
    """Nearest x2 upsampling; MUTANT up_off: the source pixel one further right (clamped)."""
    iy = torch.arange(Ho) // 2
    ix = torch.arange(Wo) // 2
    if mut == "up_off":
        ix = (ix + 1).clamp(max=r.shape[-1] - 1)
    return r[..., iy, :][..., :, ix]


def _wide(t, mut):
    """MUTANT drop_low: the wide operand loses its low plane."""
    return bf16_split(t)[0] if mut == "drop_low" else t


def _finish_bf16(pre, relu, stages, mut):
    value = pre.relu() if relu else pre
    return Ref(pre, value, _round(value, mut), stages, relu)


def _bc(b):
    return b.view(1, -1, 1, 1)


# ---- generators ------------------------------------------------------------------------------------------------------

def _gen(*key):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % (2 ** 31))


def ints(g, shape, amp, lo=0, keep=None):
    """Integer-valued float64 tensor, magnitudes uniform in [lo, amp], random sign; keep: one element in `keep` stays,
    the others are zero (a sparse weight: a smaller sum at the same K)."""
    if keep is not None:
        return ints(g, shape, amp, lo) * (torch.randint(0, keep, tuple(shape), generator=g) == 0).double()
    if lo == 0:
        return torch.randint(-amp, amp + 1, tuple(shape), generator=g).double()
    mag = torch.randint(lo, amp + 1, tuple(shape), generator=g).double()
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return mag * sign


def amp_for_k(K):
    """Operand amplitude of the bf16 convolutions by contraction length: +-8 gives sums of a few hundred (beyond 256,
    where integers stop being bf16-representable) from K = 128 on; shorter contractions need +-16."""
    return 8 if K >= 128 else 16


class Case:
    def __init__(self, key, inp, fn):
        self.key, self.inp, self._fn, self._cache = key, inp, fn, {}

    def ref(self, mut=None, **kw):
        k = (mut,) + tuple(sorted(kw.items()))
        if k not in self._cache:
            self._cache[k] = self._fn(self.inp, mut=mut, **kw)
        return self._cache[k]

    def __repr__(self):
        return "-".join(str(k) for k in self.key)


def assert_exact_inputs(ref):
    """The precondition that makes the summation order irrelevant: every stage's absolute-value contraction (plus |bias|
    and |residual|), in units of the smallest operand bit, stays below 2^24, and is an integer in those units."""
    assert ref.stages
    for name, a in ref.stages:
        m = float(a.max())
        assert m < LIMIT, f"stage {name}: abs-sum bound {m:.4g} reaches 2^24"
        assert torch.equal(a, a.round()), f"stage {name}: operands are not multiples of the unit"
    return max(float(a.max()) for _, a in ref.stages)


# ---- conv1x1_nhwc (and its data gradient) ----------------------------------------------------------------------------

CONV1X1_GEOMETRIES = [(1, 5, 7, 1), (2, 13, 11, 1), (2, 27, 35, 2), (3, 9, 15, 2)]
CONV1X1_RESIDENT = [(ci, co) for ci in (128, 256, 512) for co in (128, 1024)]
CONV1X1_TILED_ONLY = [(1024, 256), (2048, 512), (96, 160), (224, 96), (32, 32)]
CONV1X1_TILED_GEOMETRIES = [(2, 13, 11, 1), (3, 9, 15, 2)]
CONV1X1_UP2_GEOMETRIES = [(2, 12, 22), (1, 4, 6)]
CONV1X1_UP2_CHANNELS = [(128, 1024), (512, 128), (96, 160)]
CONV1X1_DGRAD = (2, 7, 9, 256, 128)          # N, H, W, Cout (channels of g), Cin


def _conv1x1_fn(c, mut=None, relu=False):
    s = c["stride"]
    xs = _sample(c["x"], s, mut)
    w = _drop_k(c["w"], mut)
    pre = F.conv2d(xs, w[:, :, None, None]) + _bc(c["b"])
    a = F.conv2d(_sample(c["x"], s, None).abs(), c["w"].abs()[:, :, None, None]) + _bc(c["b"].abs())
    if c["r"] is not None:
        r = _up2(c["r"], pre.shape[2], pre.shape[3], mut) if c["up"] else c["r"]
        pre = pre + r
        a = a + (_up2(c["r"], pre.shape[2], pre.shape[3], None) if c["up"] else c["r"]).abs()
    return _finish_bf16(pre, relu, [("conv1x1", a)], mut)


@functools.lru_cache(maxsize=None)
def conv1x1_case(N, H, W, stride, Cin, Cout, res):
    """res: 0 none, 1 plain, 2 the half-resolution map added nearest-upsampled (stride 1, even sizes)."""
    g = _gen("conv1x1", N, H, W, stride, Cin, Cout, res)
    amp = amp_for_k(Cin)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    inp = dict(x=ints(g, (N, Cin, H, W), amp), w=ints(g, (Cout, Cin), amp), b=ints(g, (Cout,), 64), stride=stride,
               r=None, up=res == 2)
    if res == 1:
        inp["r"] = ints(g, (N, Cout, Ho, Wo), 100)
    elif res == 2:
        inp["r"] = ints(g, (N, Cout, Ho // 2, Wo // 2), 100)
    return Case(("conv1x1", N, H, W, stride, Cin, Cout, res), inp, _conv1x1_fn)


def conv1x1_cases():
    out = [conv1x1_case(N, H, W, s, ci, co, res) for (ci, co) in CONV1X1_RESIDENT for (N, H, W, s) in CONV1X1_GEOMETRIES
           for res in (0, 1)]
    out += [conv1x1_case(N, H, W, s, ci, co, res) for (ci, co) in CONV1X1_TILED_ONLY
            for (N, H, W, s) in CONV1X1_TILED_GEOMETRIES for res in (0, 1)]
    out += [conv1x1_case(N, H, W, 1, ci, co, 2) for (ci, co) in CONV1X1_UP2_CHANNELS for (N, H, W) in CONV1X1_UP2_GEOMETRIES]
    return out


def _conv1x1_dgrad_fn(c, mut=None):
    w = _drop_k(c["w"], mut)
    pre = F.conv2d(c["g"], w.t()[:, :, None, None])
    a = F.conv2d(c["g"].abs(), c["w"].abs().t()[:, :, None, None])
    return _finish_bf16(pre, False, [("conv1x1_dgrad", a)], mut)


@functools.lru_cache(maxsize=None)
def conv1x1_dgrad_case():
    N, H, W, O, I = CONV1X1_DGRAD
    g = _gen("conv1x1_dgrad")
    return Case(("conv1x1_dgrad", N, H, W, O, I), dict(g=ints(g, (N, O, H, W), 8), w=ints(g, (O, I), 8)),
                _conv1x1_dgrad_fn)


# ---- conv3x3_nhwc (and its data gradient) ----------------------------------------------------------------------------

CONV3X3_TILES = {1: (12, 13, 14, 16, 18, 22, 23, 24), 2: (12, 13, 22)}
# (N, C, Cout, H, W, stride)
CONV3X3_SHAPES = [(2, 128, 128, 9, 21, 1), (1, 32, 128, 1, 1, 1), (1, 64, 256, 8, 16, 1),
                  (1, 256, 256, 7, 9, 2), (1, 32, 128, 2, 3, 2), (2, 64, 128, 1, 1, 2)]
CONV3X3_DGRAD = (1, 6, 10, 64, 128)          # N, H, W, Cout (channels of g), Cin


def _conv3x3_core(x, w, b, stride, mut):
    xp = _pad2(_shift2(x, mut) if stride == 2 else x, 1, mut)
    pre = F.conv2d(xp, _drop_k(w, mut), stride=stride) + _bc(b)
    a = F.conv2d(x.abs(), w.abs(), stride=stride, padding=1) + _bc(b.abs())
    return pre, a


def _conv3x3_fn(c, mut=None, relu=False):
    pre, a = _conv3x3_core(c["x"], c["w"], c["b"], c["stride"], mut)
    return _finish_bf16(pre, relu, [("conv3x3", a)], mut)


@functools.lru_cache(maxsize=None)
def conv3x3_case(N, C, Cout, H, W, stride):
    g = _gen("conv3x3", N, C, Cout, H, W, stride)
    amp = 16 if C <= 64 else 8          # maps of one pixel contract the centre tap only (K = C)
    inp = dict(x=ints(g, (N, C, H, W), amp), w=ints(g, (Cout, C, 3, 3), amp), b=ints(g, (Cout,), 64), stride=stride)
    return Case(("conv3x3", N, C, Cout, H, W, stride), inp, _conv3x3_fn)


def conv3x3_cases():
    return [conv3x3_case(*s) for s in CONV3X3_SHAPES]


def _conv3x3_dgrad_fn(c, mut=None):
    wd = c["w"].flip(2, 3).transpose(0, 1).contiguous()
    pre, a = _conv3x3_core(c["g"], wd, torch.zeros(wd.shape[0], dtype=torch.float64), 1, mut)
    return _finish_bf16(pre, False, [("conv3x3_dgrad", a)], mut)


@functools.lru_cache(maxsize=None)
def conv3x3_dgrad_case():
    N, H, W, O, I = CONV3X3_DGRAD
    g = _gen("conv3x3_dgrad")
    return Case(("conv3x3_dgrad", N, H, W, O, I), dict(g=ints(g, (N, O, H, W), 8), w=ints(g, (O, I, 3, 3), 8)),
                _conv3x3_dgrad_fn)


# ---- conv3x3_conv1x1_nhwc ---------------------------------------------------------------------------------------------

FUSED_TILES = {(128, 1): (12,), (128, 2): (12, 13), (256, 1): (22, 23, 24), (256, 2): (22,)}
# (N, H, W, stride): one ragged map (tiles cut by the edge in both directions) and one map smaller than a tile, per stride
FUSED_GEOMETRIES = [(2, 13, 11, 1), (1, 5, 7, 1), (2, 27, 35, 2), (3, 9, 15, 2)]
FUSED_CMID = (128, 256)


def _fused_fn(c, mut=None):
    """relu(conv1x1(rne_bf16(relu(conv3x3(x) + b2))) + b3 + residual), one rounding at the mid tensor, one at the end."""
    pre2, a2 = _conv3x3_core(c["x"], c["w2"], c["b2"], c["stride"], mut)
    mid = _mid(pre2.relu(), mut)
    pre = F.conv2d(mid, c["w3"][:, :, None, None]) + _bc(c["b3"]) + c["r"]
    mid_true = rne_bf16(_conv3x3_core(c["x"], c["w2"], c["b2"], c["stride"], None)[0].relu())
    a3 = F.conv2d(mid_true, c["w3"].abs()[:, :, None, None]) + _bc(c["b3"].abs()) + c["r"].abs()
    ref = _finish_bf16(pre, True, [("conv3x3", a2), ("conv1x1", a3)], mut)
    ref.extra["mid_pre"] = pre2
    return ref


@functools.lru_cache(maxsize=None)
def fused_case(N, H, W, stride, cmid):
    g = _gen("fused", N, H, W, stride, cmid)
    cout = 4 * cmid
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    inp = dict(x=ints(g, (N, cmid, H, W), 4), w2=ints(g, (cmid, cmid, 3, 3), 4), b2=ints(g, (cmid,), 32),
               w3=ints(g, (cout, cmid), 2 if cmid == 128 else 1), b3=ints(g, (cout,), 64),
               r=ints(g, (N, cout, Ho, Wo), 100), stride=stride, cmid=cmid, cout=cout)
    return Case(("conv3x3_conv1x1", N, H, W, stride, cmid), inp, _fused_fn)


def fused_cases():
    return [fused_case(N, H, W, s, cmid) for cmid in FUSED_CMID for (N, H, W, s) in FUSED_GEOMETRIES]


# ---- bottleneck64_nhwc ------------------------------------------------------------------------------------------------

BOTTLENECK_SHAPES = [(256, False, 1, 13, 21), (64, True, 1, 9, 17), (256, False, 1, 3, 5), (256, False, 2, 24, 48)]
BOTTLENECK_VARIANTS = (0, 1, 2, 3, 4, 5)


def _bottleneck_fn(c, mut=None):
    """c1 = rne(relu(conv1x1(x, w1) + b1)); c2 = rne(relu(conv3x3(c1, w2) + b2));
    out = rne(relu(conv1x1(c2, w3) + b3 + identity)), identity = x, or conv1x1(x, wds) + bds contracted in the same
    accumulator as the third convolution."""
    x = c["x"]
    w1 = _drop_k(c["w1"], mut)

    def chain(w1_, m):
        p1 = F.conv2d(x, w1_[:, :, None, None]) + _bc(c["b1"])
        c1 = _mid(p1.relu(), m)
        p2 = F.conv2d(_pad2(c1, 1, m), c["w2"]) + _bc(c["b2"])
        c2 = _mid(p2.relu(), m)
        idn = x if c["wds"] is None else F.conv2d(x, c["wds"][:, :, None, None]) + _bc(c["bds"])
        return p1, c1, p2, c2, F.conv2d(c2, c["w3"][:, :, None, None]) + _bc(c["b3"]) + idn

    p1, c1, p2, c2, pre = chain(w1, mut)
    _, t1, _, t2, _ = chain(c["w1"], None) if mut else (p1, c1, p2, c2, pre)
    ab = lambda t, w, b: F.conv2d(t.abs(), w.abs(), padding=w.shape[-1] // 2) + _bc(b.abs())
    a1 = ab(x, c["w1"][:, :, None, None], c["b1"])
    a2 = ab(t1, c["w2"], c["b2"])
    a3 = ab(t2, c["w3"][:, :, None, None], c["b3"])
    a3 = a3 + (x.abs() if c["wds"] is None else ab(x, c["wds"][:, :, None, None], c["bds"]))
    ref = _finish_bf16(pre, True, [("conv1", a1), ("conv2", a2), ("conv3+identity", a3)], mut)
    ref.extra.update(p1=p1, p2=p2)
    return ref


@functools.lru_cache(maxsize=None)
def bottleneck_case(cin, ds, N, H, W):
    g = _gen("bottleneck64", cin, ds, N, H, W)
    # K = 64 (projection block): conv1 needs +-8 for its outputs to pass 256, where rounding starts; sparse w2 / w3 then
    # keep the block's output small enough (a few thousand) for ties to stay frequent
    a1, a2, keep = (6, 2, None) if cin == 256 else (8, 1, 4)
    inp = dict(x=ints(g, (N, cin, H, W), a1), w1=ints(g, (64, cin), a1), b1=ints(g, (64,), 32),
               w2=ints(g, (64, 64, 3, 3), a2, keep=keep), b2=ints(g, (64,), 32),
               w3=ints(g, (256, 64), 1, keep=keep), b3=ints(g, (256,), 64),
               wds=ints(g, (256, cin), 2) if ds else None, bds=ints(g, (256,), 64) if ds else None)
    return Case(("bottleneck64", cin, ds, N, H, W), inp, _bottleneck_fn)


def bottleneck_cases():
    return [bottleneck_case(*s) for s in BOTTLENECK_SHAPES]


# ---- stem -------------------------------------------------------------------------------------------------------------

STEM_SHAPES = [(1, 9, 7), (1, 37, 53), (2, 64, 96)]
# (N, Hs, Ws, to_rgb, mean, std): integer means, power-of-two std: (x - mean) * (1 / std) is exact and bf16-representable
STEM_U8_CASES = [(1, 37, 53, False, (104.0, 116.0, 124.0), (1.0, 2.0, 4.0)),
                 (2, 64, 90, True, (124.0, 116.0, 104.0), (4.0, 1.0, 2.0))]


def _stem_fn(c, mut=None):
    """max_pool2d(rne_bf16(relu(conv7x7_s2_p3(rne_bf16(x), w) + b)), 3, 2, 1): the kernel rounds its fp32 input and the
    convolution output to bf16; the pooling picks among rounded values."""
    x = trunc_bf16(c["x"]) if mut == "trunc_in" else rne_bf16(c["x"])
    xp = _pad2(_shift2(x, mut), 3, mut)
    pre = F.conv2d(xp, _drop_k(c["w"], mut), stride=2) + _bc(c["b"])
    a = (F.conv2d(rne_bf16(c["x"]).abs(), c["w"].abs(), stride=2, padding=3) + _bc(c["b"].abs())) / c["unit"]
    conv = _round(pre.relu(), mut)
    out = F.max_pool2d(conv.float(), 3, 2, 1).to(torch.bfloat16)
    return Ref(pre, pre.relu(), out, [("conv7x7", a)], True)


@functools.lru_cache(maxsize=None)
def stem_case(N, H, W):
    g = _gen("stem", N, H, W)
    # the range of a uint8 image, [-128, 128), in eighths: 11 significant bits, so the kernel's own rounding of its fp32
    # input to bf16 has work to do (half the values need it, a quarter are ties); the rounded values are still multiples
    # of 1/8
    x = torch.randint(-1024, 1024, (N, 3, H, W), generator=g).double() / 8
    inp = dict(x=x, w=ints(g, (64, 3, 7, 7), 4), b=ints(g, (64,), 64), unit=0.125)
    return Case(("stem", N, H, W), inp, _stem_fn)


@functools.lru_cache(maxsize=None)
def stem_u8_case(N, Hs, Ws, to_rgb, mean, std):
    """Raw uint8 HWC images; the float64 reference normalises ((x[2 - c if to_rgb else c] - mean[c]) / std[c]), pads
    with zeros to the next multiple of 32 and runs the stem reference: not the float stem kernel."""
    g = _gen("stem_u8", N, Hs, Ws, to_rgb)
    raw = torch.randint(0, 256, (N, Hs, Ws, 3), generator=g).to(torch.uint8)
    x = raw.double().permute(0, 3, 1, 2)
    if to_rgb:
        x = x.flip(1)
    x = (x - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    H, W = (Hs + 31) // 32 * 32, (Ws + 31) // 32 * 32
    x = F.pad(x, (0, W - Ws, 0, H - Hs))
    inp = dict(x=x.contiguous(), raw=raw, w=ints(g, (64, 3, 7, 7), 4), b=ints(g, (64,), 64), unit=1.0 / max(std),
               mean=mean, std=std, to_rgb=to_rgb, hw=(H, W))
    return Case(("stem_u8", N, Hs, Ws, to_rgb), inp, _stem_fn)


def stem_cases():
    return [stem_case(*s) for s in STEM_SHAPES] + [stem_u8_case(*s) for s in STEM_U8_CASES]


# ---- conv3d_bn_relu and conv3d_autograd ---------------------------------------------------------------------------------

# name, B, Z, Y, X, Cin: the named cases of tests/test_gpu_decoder.CONV_CASES
CONV3D_SHAPES = [("one_pillar", 1, 16, 1, 1, 16), ("z16_c8", 1, 16, 7, 11, 8), ("z8_c8", 1, 8, 3, 18, 8),
                 ("z16_c24", 1, 16, 3, 9, 24), ("tiny_z4", 1, 4, 13, 37, 64), ("hires_z32_c8_b2", 2, 32, 3, 9, 8),
                 ("base_conv2", 2, 16, 7, 10, 32)]
CONV3D_FLAVOURS = ("w", "x")           # which operand is wide (+-1023); the other is |int| <= 8
CONV3D_AUTOGRAD_SHAPES = [(1, 16, 5, 7, 16, 1), (1, 4, 6, 9, 64, 0)]          # B, Z, Y, X, Cin, layout
CONV3D_AUTOGRAD_FLAVOURS = ("w", "x", "g")
WIDE3D, NARROW = 1023, 8


def _pad3(x, mut):
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    if mut == "edge_pad":
        xp[..., 1:-1, 1:-1, :1] = x[..., :, :, :1]
    return xp


def _conv3d_fn(c, mut=None, relu=True):
    """relu(conv3d(x, w, padding 1) * scale + shift) on (B, Cin, Z, Y, X); scale a power of two, shift an integer."""
    wide = c["wide"]
    x = _wide(c["x"], mut) if wide == "x" else c["x"]
    w = _wide(c["w"], mut) if wide == "w" else c["w"]
    if wide == "x":
        w = _drop_k(w, mut)
    sc, sh = c["scale"].view(1, -1, 1, 1, 1), c["shift"].view(1, -1, 1, 1, 1)
    pre = F.conv3d(_pad3(x, mut), w) * sc + sh
    a = F.conv3d(split_abs(c["x"]), split_abs(c["w"]), padding=1)
    a = (a * sc + sh.abs()) / sc.clamp(max=1.0)
    value = pre.relu() if relu else pre
    _f32(value)
    return Ref(pre, value, value, [("conv3d", a)], relu)


@functools.lru_cache(maxsize=None)
def conv3d_case(name, B, Z, Y, X, Cin, wide):
    g = _gen("conv3d", name, wide)
    x = ints(g, (B, Cin, Z, Y, X), WIDE3D if wide == "x" else NARROW)
    w = ints(g, (32, Cin, 3, 3, 3), WIDE3D if wide == "w" else NARROW)
    scale = 2.0 ** torch.randint(-2, 2, (32,), generator=g).double()
    inp = dict(x=x, w=w, scale=scale, shift=ints(g, (32,), 1000), wide=wide, geom=(B, Z, Y, X, Cin))
    return Case(("conv3d", name, wide), inp, _conv3d_fn)


def conv3d_cases():
    return [conv3d_case(*s, wide) for s in CONV3D_SHAPES for wide in CONV3D_FLAVOURS]


def _conv3d_autograd_fn(c, mut=None):
    """out = conv3d(x, w); dx = conv3d(go, flipped transposed w); dW[o, i, taps] = sum over positions of go * x."""
    x, w, go = c["x"], c["w"], c["go"]
    wide = c["wide"]
    xw, ww, gw = (_wide(t, mut) if wide == n else t for t, n in ((x, "x"), (w, "w"), (go, "g")))
    out = F.conv3d(xw, ww, padding=1)
    wt = lambda t: t.flip(2, 3, 4).transpose(0, 1).contiguous()
    dx = F.conv3d(gw, wt(ww), padding=1)
    # dW through the convolution of x (channels as batch) with go as the filter
    dwf = lambda xx, gg: F.conv3d(xx.transpose(0, 1), gg.transpose(0, 1), padding=1).transpose(0, 1)
    dw = dwf(xw, gw)
    sx, sw, sg = split_abs(x), split_abs(w), split_abs(go)
    stages = [("forward", F.conv3d(sx, sw, padding=1)), ("dx", F.conv3d(sg, wt(sw), padding=1)), ("dW", dwf(sx, sg))]
    for t in (out, dx, dw):
        _f32(t)
    return Ref(out, out, out, stages, False, extra=dict(dx=dx, dw=dw))


@functools.lru_cache(maxsize=None)
def conv3d_autograd_case(B, Z, Y, X, Cin, layout, wide):
    g = _gen("conv3d_autograd", B, Z, Y, X, Cin, layout, wide)
    amp = lambda n: WIDE3D if wide == n else NARROW
    inp = dict(x=ints(g, (B, Cin, Z, Y, X), amp("x")), w=ints(g, (32, Cin, 3, 3, 3), amp("w")),
               go=ints(g, (B, 32, Z, Y, X), amp("g")), wide=wide, geom=(B, Z, Y, X, Cin), layout=layout)
    return Case(("conv3d_autograd", B, Z, Y, X, Cin, layout, wide), inp, _conv3d_autograd_fn)


def conv3d_autograd_cases():
    return [conv3d_autograd_case(*s, wide) for s in CONV3D_AUTOGRAD_SHAPES for wide in CONV3D_AUTOGRAD_FLAVOURS]


# ---- linear, value_proj, linear_wgrad -----------------------------------------------------------------------------------

LINEAR_M = (1, 31, 33, 300)
# (K1, K2, N): K = 256 and 48 in one segment and split into a | a2 (+ a2_add).  Both kernels need K1 % 16 == 0 and
# K2 % 16 == 0 (a K that is no multiple of 16 is OccAmdUnsupported on the f32 path too); 48 is the K that is no multiple
# of 32
LINEAR_KN = [(256, 0, 256), (256, 0, 96), (48, 0, 64), (192, 64, 256), (192, 64, 96), (32, 16, 64)]
LINEAR_FLAVOURS = ("w", "a")           # which operand is wide (12-bit integers); the other is |int| <= 8
WIDE12 = 2047


def _linear_fn(c, mut=None):
    """relu?([a | a2 + a2_add] @ W^T + bias) + residual, fp32 output (the ReLU before the residual)."""
    wide = c["wide"]
    a = c["a"] if c["a2"] is None else torch.cat([c["a"], c["a2"] + c["a2_add"]], 1)
    aw = _wide(a, mut) if wide == "a" else a
    ww = _wide(c["w"], mut) if wide == "w" else c["w"]
    if wide == "a":
        ww = _drop_k(ww, mut)
    pre = aw @ ww.t()
    ab = split_abs(a) @ split_abs(c["w"]).t()
    if c["b"] is not None:
        pre, ab = pre + c["b"], ab + c["b"].abs()
    value = pre.relu() if c["relu"] else pre
    if c["res"] is not None:
        value, ab = value + c["res"], ab + c["res"].abs()
    _f32(value)
    return Ref(pre, value, value, [("linear", ab)], c["relu"])


@functools.lru_cache(maxsize=None)
def linear_case(M, K1, K2, N, wide):
    """Split cases (K2 > 0) carry the whole epilogue: a2 + a2_add, bias, ReLU, residual; single-segment ones are plain."""
    g = _gen("linear", M, K1, K2, N, wide)
    aamp = WIDE12 if wide == "a" else NARROW
    full = K2 > 0
    inp = dict(a=ints(g, (M, K1), aamp), a2=None, a2_add=None, w=ints(g, (N, K1 + K2), WIDE12 if wide == "w" else NARROW),
               b=None, res=None, relu=full, wide=wide)
    if full:
        half = aamp // 2
        inp.update(a2=ints(g, (M, K2), half), a2_add=ints(g, (M, K2), half), b=ints(g, (N,), 1000),
                   res=ints(g, (M, N), 100000))
    return Case(("linear", M, K1, K2, N, wide), inp, _linear_fn)


def linear_cases():
    return [linear_case(M, *kn, wide) for M in LINEAR_M for kn in LINEAR_KN for wide in LINEAR_FLAVOURS]


# value_proj_bf16: the activations are bf16 tensors, so only the weight can be wide.  (G, rpg, K, N, ogr, row0, nbias):
# the two smallest group layouts of test_value_proj_bf16_matches_torch
VALUE_PROJ_LAYOUTS = [(4, 33, 64, 128, 40, 0, 2), (2, 70, 32, 36, 70, 0, 0)]
# value_proj_bf16_planes: cams, K, N, P, rows per segment (the multi-segment layout of the same module, N % 256 == 0)
VALUE_PROJ_PLANES = (3, 64, 256, 2, (130, 37, 9, 2))


def _value_proj_fn(c, mut=None):
    w = _wide(c["w"], mut)
    pre = c["a"] @ w.t()
    ab = c["a"].abs() @ split_abs(c["w"]).t()
    if c["gb"] is not None:
        idx = (torch.arange(c["a"].shape[0]) // c["rpg"]) % c["gb"].shape[0]
        pre, ab = pre + c["gb"][idx], ab + c["gb"][idx].abs()
    _f32(pre)
    return Ref(pre, pre, pre, [("value_proj", ab)], False)


@functools.lru_cache(maxsize=None)
def value_proj_case(G, rpg, K, N, ogr, row0, nbias):
    g = _gen("value_proj", G, rpg, K, N)
    inp = dict(a=ints(g, (G * rpg, K), NARROW), w=ints(g, (N, K), WIDE12), gb=ints(g, (nbias, N), 1000) if nbias else None,
               rpg=rpg, G=G, ogr=ogr, row0=row0)
    return Case(("value_proj", G, rpg, K, N, ogr, row0, nbias), inp, _value_proj_fn)


@functools.lru_cache(maxsize=None)
def value_proj_planes_cases():
    """One Case per (plane, segment): rows of segment s are cams groups of hws[s] rows, bias row g of table [s]."""
    cams, K, N, P, hws = VALUE_PROJ_PLANES
    g = _gen("value_proj_planes")
    a_list = [ints(g, (cams * hw, K), NARROW) for hw in hws]
    ws = [ints(g, (N, K), WIDE12) for _ in range(P)]
    gbs = [ints(g, (len(hws), cams, N), 1000) for _ in range(P)]
    return [[Case(("value_proj_planes", p, s), dict(a=a_list[s], w=ws[p], gb=gbs[p][s], rpg=hws[s]), _value_proj_fn)
             for s in range(len(hws))] for p in range(P)]


def value_proj_cases():
    return [value_proj_case(*l) for l in VALUE_PROJ_LAYOUTS] + [c for row in value_proj_planes_cases() for c in row]


LINEAR_WGRAD_M = (1, 257, 1000)
LINEAR_WGRAD_NK = [(100, 48), (64, 256)]
LINEAR_WGRAD_FLAVOURS = ("dy", "x")


def _linear_wgrad_fn(c, mut=None):
    """dW = dy^T @ x, db = column sums of dy; fp32 outputs."""
    wide = c["wide"]
    dy = _wide(c["dy"], mut) if wide == "dy" else c["dy"]
    x = _wide(c["x"], mut) if wide == "x" else c["x"]
    if mut == "drop_k":
        x = x.clone()
        x[0] = 0.0                          # one contraction element (row 0) dropped from dW
    dw = dy.t() @ x
    stages = [("dW", split_abs(c["dy"]).t() @ split_abs(c["x"])), ("db", split_abs(c["dy"]).sum(0))]
    db = c["dy"].sum(0)
    _f32(dw), _f32(db)
    return Ref(dw, dw, dw, stages, False, extra=dict(db=db))


@functools.lru_cache(maxsize=None)
def linear_wgrad_case(M, N, K, wide):
    g = _gen("linear_wgrad", M, N, K, wide)
    inp = dict(dy=ints(g, (M, N), WIDE12 if wide == "dy" else NARROW), x=ints(g, (M, K), WIDE12 if wide == "x" else NARROW),
               wide=wide)
    return Case(("linear_wgrad", M, N, K, wide), inp, _linear_wgrad_fn)


def linear_wgrad_cases():
    return [linear_wgrad_case(M, N, K, wide) for M in LINEAR_WGRAD_M for (N, K) in LINEAR_WGRAD_NK
            for wide in LINEAR_WGRAD_FLAVOURS]


# ---- linear_pair_chain, and the exact stages of linear_ln_chain / encoder_ffn_chain -------------------------------------------
# Program C (linear_pair_chain) has no LayerNorm and is exact as it stands.  Programs A and B are exact behind a LayerNorm
# whose gamma is zero: fmaf(d * rstd, 0, beta) = beta for any finite row, so the LayerNorm'd tile is the row beta, whatever
# the (arbitrary, finite) operands in front of it.  That row is the operand of the next stage: the tail of A, the tail of
# B (gamma2 = 0) and B's FFN (gamma1 = 0, up to the second LayerNorm: its input pre2 is an exact integer, its output is
# checked under the derived bound of tests/ln_bound.py).  The references of the gamma = 0 cases are one row, broadcast.

CHAIN_M_SMALL = (1, 63, 65)            # one ragged tile, and one row into the second
CHAIN_M_FULL = 8229                    # 128 full 64-row tiles + a ragged one: blockIdx >> 3 takes all 16 k-step rotations
CHAIN_NQ = (64, 128, 192, 256)
CHAIN_N2 = (32, 96, 224, 288, 768, 1280)          # n2 % 64 == 32 (half-wave store masks), one .. five passes
CHAIN_PAIR_FLAVOURS = ("a", "w")
CHAIN_TAIL_FLAVOURS = ("beta", "w")
WIDE10 = 1023                          # weights against the 256 DISTINCT bf16-exact beta values (-128 .. 127)
CHAIN_MUTANTS = ("term_last_group", "term_on_zv", "bias_pass0", "tile_copy")


def chain_m_half(cus=256):
    """Rows that reach the 32-row tiles of the chain kernels on a device of `cus` CUs (two resident blocks each):
    2 * cus full tiles, then 129 half tiles, the last with one row: all 16 rotations on 32-row tiles."""
    return 64 * 2 * cus + 32 * 128 + 1


def _distinct(g, wide):
    """256 distinct integers: 12-bit ones (wide), or a permutation of -128 .. 127 (all bf16-exact)."""
    if wide:
        return (torch.randperm(2 * WIDE12 + 1, generator=g)[:256] - WIDE12).double()
    return (torch.randperm(256, generator=g) - 128).double()


def _noise(g, *shape):
    """Arbitrary finite fp32 operands of the stages in front of a gamma = 0 LayerNorm."""
    return torch.randint(-50, 51, tuple(shape), generator=g).float()


def _pair_core(x, c, mut, x_name):
    """[x . Wq^T (+ term) | x . Wv^T + bv] for x (R, 256), R = 1 (broadcast) or M -> (zq | zv, abs-sum)."""
    wide, nq, term = c["wide"], c["wq"].shape[0], c["term"]
    xw = _wide(x, mut) if wide == x_name else x
    wq, wv = c["wq"], c["wv"]
    if wide == "w":
        wq, wv = _wide(wq, mut), _wide(wv, mut)
    else:
        wv = _drop_k(wv, mut)
    zq, zv = xw @ wq.t(), xw @ wv.t() + c["bv"]
    sx = split_abs(x)
    aq, av = sx @ split_abs(c["wq"]).t(), sx @ split_abs(c["wv"]).t() + c["bv"].abs()
    if term is not None:
        t = term
        if mut == "term_last_group":                 # MUTANT: the last 64-column group of zq misses its term
            t = term.clone()
            t[:, nq - 64:] = 0.0
        zq, aq = zq + t, aq + term.abs()
        if mut == "term_on_zv":                      # MUTANT: the term is added to the value columns as well
            zv = zv.expand(term.shape[0], 256).clone()
            zv[:, :nq] += term
    M = c["M"]
    return torch.cat([zq.expand(M, nq), zv.expand(M, 256)], 1), torch.cat([aq.expand(M, nq), av.expand(M, 256)], 1)


def _pair_fn(c, mut=None):
    z, ab = _pair_core(c["a"], c, mut, "a")
    _f32(z)
    return Ref(z, z, z, [("pair", ab)], False)


def pair_chain_case(M, nq, term, wide):
    """Program C.  Expected output: [zq | zv] (M, nq + 256)."""
    g = _gen("pair_chain", M, nq, term, wide)
    wamp = WIDE12 if wide == "w" else NARROW
    inp = dict(a=ints(g, (M, 256), WIDE12 if wide == "a" else NARROW), wq=ints(g, (nq, 256), wamp),
               wv=ints(g, (256, 256), wamp), bv=ints(g, (256,), 1000), term=ints(g, (M, nq), 100000) if term else None,
               wide=wide, M=M)
    return Case(("pair_chain", M, nq, int(term), wide), inp, _pair_fn)


def _tail_b_fn(c, mut=None):
    z, ab = _pair_core(c["beta"][None], c, mut, "beta")
    _f32(z)
    return Ref(z, z, z, [("tail", ab)], False, extra=dict(y=c["beta"][None].expand(c["M"], 256)))


def tail_b_case(M, nq, term, wide):
    """Program B with gamma2 = 0: y = beta2 in every row, [zq | zv] = [beta2 . Wq^T + term | beta2 . Wv^T + bv].  The
    stages in front (output_proj, LayerNorm 1, FFN) run on arbitrary finite operands."""
    g = _gen("tail_b", M, nq, term, wide)
    wamp = WIDE10 if wide == "w" else NARROW
    inp = dict(beta=_distinct(g, wide == "beta"), wq=ints(g, (nq, 256), wamp), wv=ints(g, (256, 256), wamp),
               bv=ints(g, (256,), 1000), term=ints(g, (M, nq), 100000) if term else None, wide=wide, M=M,
               a=_noise(g, M, 256), res=_noise(g, M, 256), wo=ints(g, (256, 256), 2).float(), bo=_noise(g, 256),
               g1=torch.randint(1, 4, (256,), generator=g).float(), be1=_noise(g, 256) / 16,
               w1=ints(g, (512, 256), 2).float(), b1=_noise(g, 512), w2=ints(g, (256, 512), 2).float(), b2=_noise(g, 256))
    return Case(("tail_b", M, nq, int(term), wide), inp, _tail_b_fn)


def _tail_a_fn(c, mut=None, relu=False):
    wide, n2 = c["wide"], c["w2"].shape[0]
    beta = c["beta"][None]
    bw = _wide(beta, mut) if wide == "beta" else beta
    w2 = _wide(c["w2"], mut) if wide == "w" else _drop_k(c["w2"], mut)
    b2 = c["b2"]
    if mut == "bias_pass0":                          # MUTANT: the passes behind the first take the first pass's biases
        b2 = b2.clone()
        b2[256:] = torch.cat([c["b2"][:256]] * 5)[:n2 - 256]
    pre = bw @ w2.t() + b2
    ab = split_abs(beta) @ split_abs(c["w2"]).t() + c["b2"].abs()
    value = pre.relu() if relu else pre
    if mut == "tile_copy":                           # MUTANT: the last stored 32-column tile is a copy of the one before it
        value = value.clone()
        value[:, n2 - 32:] = value[:, n2 - 64:n2 - 32]
    _f32(value)
    M = c["M"]
    return Ref(pre, value, value.expand(M, n2), [("tail", ab)], relu, extra=dict(y=beta.expand(M, 256)))


def tail_a_case(M, n2, wide):
    """Program A with gamma = 0: y = beta in every row, z = act2(beta . W2^T + b2)."""
    g = _gen("tail_a", M, n2, wide)
    inp = dict(beta=_distinct(g, wide == "beta"), w2=ints(g, (n2, 256), WIDE10 if wide == "w" else NARROW),
               b2=ints(g, (n2,), 1000), wide=wide, M=M, a=_noise(g, M, 256), res=_noise(g, M, 256),
               w1=ints(g, (256, 256), 2).float(), b1=_noise(g, 256))
    return Case(("tail_a", M, n2, wide), inp, _tail_a_fn)


FFN_B1_SHIFT = 300           # b1 = +-1000 + 300: 40 % negative pre-activations, and a third of h = relu(.) needs its low plane


def _ffn_fn(c, mut=None):
    """x2 = beta1;  h = relu(x2 . W1^T + b1);  pre2 = h . W2^T + b2 + x2: the exact input of the second LayerNorm."""
    x2 = c["beta1"][None]
    hpre = x2 @ c["w1"].t() + c["b1"]
    h_true = hpre.relu()
    h = hpre if mut == "no_relu" else h_true          # MUTANT no_relu: the hidden activation keeps its negative values
    h = _wide(h, mut)
    w2 = c["w2"]
    if mut == "drop_k":                              # MUTANT: the first live contraction element of output column 0 is dropped
        w2 = w2.clone()
        w2[0, int(((h_true[0] > 0) & (w2[0] != 0)).nonzero()[0])] = 0.0
    pre2 = h @ w2.t() + c["b2"]
    if mut != "no_x2":                               # MUTANT no_x2: the FFN's residual is missing
        pre2 = pre2 + x2
    a1 = x2.abs() @ c["w1"].abs().t() + c["b1"].abs()
    a2 = split_abs(h_true) @ c["w2"].abs().t() + c["b2"].abs() + x2.abs()
    _f32(pre2)
    return Ref(hpre, pre2, pre2.expand(c["M"], 256), [("ffn1", a1), ("ffn2", a2)], True, extra=dict(h=h_true))


def ffn_case(M):
    """Program B with gamma1 = 0 and no tail, exact up to the second LayerNorm.  W2 is +-2: |pre2| stays below 2^16, so
    the deviations from the row mean (multiples of 2^-8) are fp32 values too."""
    g = _gen("ffn_b", M)
    inp = dict(beta1=ints(g, (256,), NARROW), w1=ints(g, (512, 256), NARROW), b1=ints(g, (512,), 1000) + FFN_B1_SHIFT,
               w2=ints(g, (256, 512), 2), b2=ints(g, (256,), 1000), M=M,
               g2=(torch.rand(256, generator=g) + 0.5) * (torch.randint(0, 2, (256,), generator=g) * 2 - 1).float(),
               be2=torch.randn(256, generator=g), a=_noise(g, M, 256), res=_noise(g, M, 256),
               wo=ints(g, (256, 256), 2).float(), bo=_noise(g, 256))
    return Case(("ffn_b", M), inp, _ffn_fn)


@functools.lru_cache(maxsize=None)
def chain_host_cases():
    """(case, reference keywords) the host tests build: every flavour / width / term combination at the small M, and one
    case per program at the two tall M (the operands of a row do not depend on M; the references of the gamma = 0
    programs are one row)."""
    tall = (CHAIN_M_FULL, chain_m_half())
    out = []
    for M in (1, 65):
        out += [(pair_chain_case(M, nq, t, w), {}) for nq in CHAIN_NQ for t in (False, True) for w in CHAIN_PAIR_FLAVOURS]
        out += [(tail_b_case(M, nq, t, w), {}) for nq in CHAIN_NQ for t in (False, True) for w in CHAIN_TAIL_FLAVOURS]
        out += [(tail_a_case(M, n2, w), dict(relu=r)) for n2 in CHAIN_N2 for w in CHAIN_TAIL_FLAVOURS for r in (False, True)]
        out.append((ffn_case(M), {}))
    out += [(pair_chain_case(M, 192, True, "a"), {}) for M in tall]
    out += [(tail_b_case(M, 192, True, "beta"), {}) for M in tall]
    out += [(tail_a_case(M, 288, "beta"), dict(relu=True)) for M in tall]
    return out


# ---- conv1x1_wgrad_nhwc, conv3x3_wgrad_nhwc, bias_act_bwd_nhwc --------------------------------------------------------------

CONV_WGRAD_CHANNELS = [(32, 32), (128, 64), (64, 256)]          # (Cin, Cout)
CONV_WGRAD_MAPS = [(2, 9, 13), (1, 1, 1)]
CONV_WGRAD_SPLITS = (None, 1, 3)


def _conv_wgrad_fn(c, mut=None, bf16=False):
    """dw[o, i, ky, kx] = sum over output pixels of g[n, o, yo, xo] * x[n, i, yo*s + ky - p, xo*s + kx - p] (zero outside
    the map); fp32 result = the float64 sum, bf16 result = its RNE."""
    k, s = c["k"], c["stride"]
    p = k // 2
    g = _drop_k(c["g"], mut)
    x = _shift2(c["x"], mut) if s == 2 else c["x"]

    def contract(xx, gg, m):
        xp = _pad2(xx, p, m) if p else xx
        cols = F.unfold(xp, k, stride=s)                                  # (N, Cin*k*k, L)
        return torch.einsum("nol,nkl->ok", gg.flatten(2), cols).view(gg.shape[1], xx.shape[1], k, k)

    dw = contract(x, g, mut)
    a = contract(c["x"].abs(), c["g"].abs(), None)
    return Ref(dw, dw, _round(dw, mut) if bf16 else _f32(dw).double(), [("wgrad", a)], False)


@functools.lru_cache(maxsize=None)
def conv_wgrad_case(k, stride, Cin, Cout, N, H, W):
    gen = _gen("conv_wgrad", k, stride, Cin, Cout, N, H, W)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    # one-pixel maps: a single product per element (and only the centre tap of a 3x3 sees it); magnitudes in [33, 45] put
    # it in [1024, 2048), where bf16 keeps multiples of 8: most products need rounding, those = 4 mod 8 are ties
    lo, amp = (33, 45) if N * Ho * Wo == 1 else (0, 8)
    inp = dict(g=ints(gen, (N, Cout, Ho, Wo), amp, lo), x=ints(gen, (N, Cin, H, W), amp, lo), k=k, stride=stride)
    return Case((f"conv{k}x{k}_wgrad", stride, Cin, Cout, N, H, W), inp, _conv_wgrad_fn)


def conv_wgrad_cases(k):
    return [conv_wgrad_case(k, s, ci, co, *m) for s in (1, 2) for (ci, co) in CONV_WGRAD_CHANNELS for m in CONV_WGRAD_MAPS]


BIAS_ACT_BWD_SHAPES = [(2, 64, 7, 9), (1, 256, 5, 3), (3, 8, 1, 1), (2, 192, 6, 5), (1, 2048, 3, 4)]


def _bias_act_bwd_fn(c, mut=None, relu=True):
    g = torch.where(c["y"] > 0, c["gy"], torch.zeros_like(c["gy"])) if relu else c["gy"]
    db = g.sum((0, 2, 3))
    a = c["gy"].abs().sum((0, 2, 3))
    return Ref(db, db, _f32(db).double(), [("bias_grad", a)], False, extra=dict(g=to_bf16(g)))


@functools.lru_cache(maxsize=None)
def bias_act_bwd_case(N, C, H, W):
    g = _gen("bias_act_bwd", N, C, H, W)
    y = ints(g, (N, C, H, W), 8).relu()
    y.view(-1)[::7] = -0.0                   # a negative zero is not > 0
    return Case(("bias_act_bwd", N, C, H, W), dict(gy=ints(g, (N, C, H, W), 200), y=y), _bias_act_bwd_fn)


def bias_act_bwd_cases():
    return [bias_act_bwd_case(*s) for s in BIAS_ACT_BWD_SHAPES]


# ---- which case of a family the mutants run on, and which mutants a family has -----------------------------------------
# The smallest case of the family on which the mutant is defined (a one-pixel map has no neighbour to sample, a case
# without ReLU-free large values no rounding to get wrong): (case, reference keywords, mutants).

def mutant_table():
    rounding = ("trunc", "half_away")
    return [
        (conv1x1_case(1, 5, 7, 1, 128, 128, 0), dict(relu=False), rounding + ("drop_k",)),
        (conv1x1_case(3, 9, 15, 2, 128, 128, 0), dict(relu=True), rounding + ("drop_k", "stride_off")),
        (conv1x1_case(1, 4, 6, 1, 128, 1024, 2), dict(relu=False), rounding + ("up_off",)),
        (conv1x1_dgrad_case(), {}, rounding + ("drop_k",)),
        (conv3x3_case(1, 32, 128, 2, 3, 2), dict(relu=False), rounding + ("drop_k", "edge_pad", "stride_off")),
        (conv3x3_case(1, 64, 256, 8, 16, 1), dict(relu=True), rounding + ("drop_k", "edge_pad")),
        (conv3x3_dgrad_case(), {}, rounding + ("drop_k", "edge_pad")),
        (fused_case(1, 5, 7, 1, 128), {}, rounding + ("drop_k", "edge_pad", "skip_mid_round")),
        (fused_case(3, 9, 15, 2, 128), {}, rounding + ("drop_k", "edge_pad", "skip_mid_round", "stride_off")),
        (bottleneck_case(256, False, 1, 3, 5), {}, rounding + ("drop_k", "edge_pad", "skip_mid_round")),
        (bottleneck_case(64, True, 1, 9, 17), {}, rounding + ("drop_k", "edge_pad", "skip_mid_round")),
        (stem_case(1, 9, 7), {}, rounding + ("edge_pad", "stride_off", "trunc_in")),
        (stem_case(1, 37, 53), {}, ("drop_k",)),         # 9 x 7 pools to 3 x 2 pixels: one tap rarely reaches the maximum
        (stem_u8_case(*STEM_U8_CASES[0]), {}, rounding + ("drop_k", "edge_pad", "stride_off")),
        (conv3d_case(*CONV3D_SHAPES[0], "w"), {}, ("drop_low",)),
        (conv3d_case(*CONV3D_SHAPES[0], "x"), {}, ("drop_low",)),          # one pillar: most taps lie in the padding
        (conv3d_case(*CONV3D_SHAPES[2], "x"), {}, ("drop_low", "drop_k", "edge_pad")),
        (conv3d_autograd_case(*CONV3D_AUTOGRAD_SHAPES[0], "w"), {}, ("drop_low",)),
        (conv3d_autograd_case(*CONV3D_AUTOGRAD_SHAPES[0], "x"), {}, ("drop_low",)),
        (conv3d_autograd_case(*CONV3D_AUTOGRAD_SHAPES[0], "g"), {}, ("drop_low",)),
        (linear_case(1, 48, 0, 64, "w"), {}, ("drop_low",)),
        (linear_case(1, 48, 0, 64, "a"), {}, ("drop_low", "drop_k")),
        (linear_case(1, 32, 16, 64, "a"), {}, ("drop_low",)),
        (linear_case(31, 32, 16, 64, "a"), {}, ("drop_k",)),          # one row: the ReLU can hide the one output it changes
        (value_proj_case(*VALUE_PROJ_LAYOUTS[1]), {}, ("drop_low",)),
        (linear_wgrad_case(1, 100, 48, "dy"), {}, ("drop_low",)),
        (linear_wgrad_case(1, 100, 48, "x"), {}, ("drop_low",)),
        (linear_wgrad_case(257, 100, 48, "x"), {}, ("drop_low", "drop_k")),
        (pair_chain_case(1, 64, True, "a"), {}, ("drop_low", "drop_k", "term_last_group", "term_on_zv")),
        (pair_chain_case(1, 64, True, "w"), {}, ("drop_low",)),
        (tail_b_case(1, 64, True, "beta"), {}, ("drop_low", "drop_k", "term_last_group", "term_on_zv")),
        (tail_b_case(1, 64, True, "w"), {}, ("drop_low",)),
        (tail_a_case(1, 32, "beta"), dict(relu=False), ("drop_low", "drop_k")),
        (tail_a_case(1, 32, "w"), dict(relu=False), ("drop_low",)),
        (tail_a_case(1, 96, "beta"), dict(relu=True), ("tile_copy",)),          # n2 % 64 == 32 with a tile in front of the last
        (tail_a_case(1, 288, "beta"), dict(relu=False), ("bias_pass0",)),       # the smallest n2 with a second pass
        # encoder_ffn_chain's FFN: pre2, the input of the second LayerNorm, is what these change.  The kernel's output is
        # LayerNorm(pre2), so on the device drop_low and drop_k, like no_relu and no_x2 (the hidden ReLU or the FFN's
        # residual missing), are killed through the derived bound on y, not bit-wise: tests/test_ln_bound_host.py
        (ffn_case(1), {}, ("drop_low", "drop_k", "no_relu", "no_x2")),
        (conv_wgrad_case(1, 1, 32, 32, 1, 1, 1), dict(bf16=True), rounding),
        (conv_wgrad_case(1, 2, 32, 32, 2, 9, 13), dict(bf16=True), rounding + ("drop_k", "stride_off")),
        (conv_wgrad_case(3, 1, 32, 32, 1, 1, 1), dict(bf16=True), rounding + ("edge_pad",)),
        (conv_wgrad_case(3, 2, 32, 32, 2, 9, 13), dict(bf16=True), rounding + ("drop_k", "edge_pad", "stride_off")),
        (conv_wgrad_case(3, 2, 32, 32, 2, 9, 13), dict(bf16=False), ("drop_k", "edge_pad", "stride_off")),
    ]


def bf16_profile_cases():
    """(case, reference keywords) of every case with a bf16 output, ReLU on and off where the GPU test runs both."""
    out = []
    for c in conv1x1_cases() + conv3x3_cases():
        out += [(c, dict(relu=True)), (c, dict(relu=False))]
    out += [(c, {}) for c in [conv1x1_dgrad_case(), conv3x3_dgrad_case()] + fused_cases() + bottleneck_cases() + stem_cases()]
    out += [(c, dict(bf16=True)) for k in (1, 3) for c in conv_wgrad_cases(k)]
    return out


def fp32_cases():
    """(case, reference keywords) of every case with an fp32 output."""
    out = [(c, dict(relu=True)) for c in conv3d_cases()] + [(conv3d_case(*CONV3D_SHAPES[-1], "w"), dict(relu=False))]
    out += [(c, {}) for c in conv3d_autograd_cases() + linear_cases() + value_proj_cases() + linear_wgrad_cases()]
    out += [(c, dict(bf16=False)) for k in (1, 3) for c in conv_wgrad_cases(k)]
    out += [(c, dict(relu=r)) for c in bias_act_bwd_cases() for r in (True, False)]
    out += chain_host_cases()
    return out


def wide_operands():
    """(case, the operand the kernel has to round or split itself) of every bf16x3 case and of the float stem: at least
    30 % of it must not be bf16-representable."""
    out = []
    for c in conv3d_cases() + conv3d_autograd_cases():
        out.append((c, c.inp[{"w": "w", "x": "x", "g": "go"}[c.inp["wide"]]]))
    out += [(c, c.inp["x"]) for c in stem_cases() if c.key[0] == "stem"]          # the stem rounds its fp32 input itself
    for c in linear_cases():
        a = c.inp["a"] if c.inp["a2"] is None else torch.cat([c.inp["a"], c.inp["a2"] + c.inp["a2_add"]], 1)
        out.append((c, c.inp["w"] if c.inp["wide"] == "w" else a))
    out += [(c, c.inp["w"]) for c in value_proj_cases()]
    out += [(c, c.inp[c.inp["wide"]]) for c in linear_wgrad_cases()]
    for c, kw in chain_host_cases():
        if c.key[0] == "ffn_b":
            out.append((c, c.ref().extra["h"]))          # the hidden activation: the kernel splits it itself
        elif kw.get("relu", False) is False:             # (the ReLU twin of a tail case has the same operands)
            w = c.inp["wide"]
            out.append((c, torch.cat([c.inp["wq"], c.inp["wv"]]) if w == "w" and "wq" in c.inp else
                        c.inp["w2"] if w == "w" else c.inp[w]))
    return out
