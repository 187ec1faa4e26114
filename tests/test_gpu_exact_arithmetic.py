"""-m gpu: every convolution and GEMM kernel of the matrix cores against the float64 reference, BIT FOR BIT.

The operands (tests/exact_cases.py) are small integers, or integers times a power of two, for which every partial sum of
every contraction is exactly representable in fp32 (tests/test_exact_cases_host.py asserts it for each case used here).
The fp32 accumulator then holds the mathematically exact value whatever the summation order, MFMA shape, split-K or tile
walk, so a correct kernel returns exactly rne_bf16(float64 result) for a bf16 output and exactly the float64 result for
an fp32 output.  Nothing is measured and no tolerance is chosen; the sums land on bf16 ties and on values that bf16
cannot hold, so the epilogues' rounding is exercised as well.  Shapes are the smallest at which each kernel's tiling can
still go wrong (ragged tiles, maps below one tile, several blocks, every forced tile / variant id of the existing variant
tests).  Weights go through the device packers, which are part of what is tested.

The contracts the references state: the two 64-channel intermediates of bottleneck64_nhwc and the mid tensor of
conv3x3_conv1x1_nhwc are rounded to bf16 (RNE); the stem rounds its fp32 input and its convolution output (before the
pooling) to bf16; a projection shortcut is contracted in the accumulator of the third convolution (no rounding between);
linear applies the ReLU before the residual.  The bf16x3 kernels (linear, value_proj, linear_wgrad, conv3d and its
gradients) run once per flavour: one operand wide (needs its low plane), the others bf16-exact.

The linear chains (csrc/linear_chain_x3.hip): linear_pair_chain is exact as it stands; the tails of linear_ln_chain and
encoder_ffn_chain run behind a LayerNorm with gamma = 0, whose output is the row beta exactly, and are exact from there.
A LayerNorm itself is not exact: those of the chains (encoder_ffn_chain's second one on the exact integer output of its
FFN) and the ln= epilogue of linear get exact integer inputs, at rows with |mean| >> std and with variance near eps,
and must stay inside an error bound counted from the kernel source, never fitted to a result (tests/ln_bound.py).

Out of scope: the Softplus epilogue and occ_heads (transcendentals and divisions are not exact), the BatchNorm
statistics and heads-loss kernels, and the gather kernels (float64 tests in every mode already).  bias_relu_maxpool_nhwc and bias_act_nhwc_ are compared bit for bit in tests/test_gpu_backbone.py.  Both
Linear kernels need K1 % 16 == 0 and K2 % 16 == 0 (anything else is OccAmdUnsupported, tests/test_gpu_linear.py), so the
odd K here is 48 = 32 + 16."""
import pytest
import torch

from tests import exact_cases as ec

pytestmark = pytest.mark.gpu


def _cl(t64):
    """float64 (N, C, H, W) -> channels_last bf16 on the device (the values are bf16-exact by construction)."""
    b = ec.to_bf16(t64)
    assert torch.equal(b.double(), t64)
    return b.cuda().contiguous(memory_format=torch.channels_last)


def _f(t64):
    return None if t64 is None else ec._f32(t64).cuda().contiguous()


def _same(got, want, what):
    assert got.dtype == torch.bfloat16 and got.is_contiguous(memory_format=torch.channels_last), what
    ec.assert_bit_equal(got, want, what)


# ---- conv1x1_nhwc ------------------------------------------------------------------------------------------------------

def _run_conv1x1(case, variants):
    from occnet_amd import ext
    c = case.inp
    x, wp, b = _cl(c["x"]), ext.conv1x1_pack_weight(_f(c["w"])), _f(c["b"])
    r = None if c["r"] is None else _cl(c["r"])
    for relu in (True, False):
        want = case.ref(relu=relu).out
        for v in variants:
            got = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=relu, stride=c["stride"], residual_upsample2=c["up"], variant=v)
            _same(got, want, f"{case!r} relu={relu} variant={v}")


@pytest.mark.parametrize("Cin,Cout", ec.CONV1X1_RESIDENT)
def test_conv1x1_every_variant(Cin, Cout):
    from tests.test_gpu_conv1x1_variants import _variants
    for (N, H, W, s) in ec.CONV1X1_GEOMETRIES:
        for res in (0, 1):
            _run_conv1x1(ec.conv1x1_case(N, H, W, s, Cin, Cout, res), _variants(Cin, Cout))


@pytest.mark.parametrize("Cin,Cout", ec.CONV1X1_TILED_ONLY)
def test_conv1x1_tiled_only_shapes(Cin, Cout):
    for (N, H, W, s) in ec.CONV1X1_TILED_GEOMETRIES:
        for res in (0, 1):
            _run_conv1x1(ec.conv1x1_case(N, H, W, s, Cin, Cout, res), (None, 1))


@pytest.mark.parametrize("Cin,Cout", ec.CONV1X1_UP2_CHANNELS)
def test_conv1x1_upsampled_residual(Cin, Cout):
    from tests.test_gpu_conv1x1_variants import _variants
    variants = _variants(Cin, Cout) if Cin in (128, 256, 512) else (None, 1)
    for (N, H, W) in ec.CONV1X1_UP2_GEOMETRIES:
        _run_conv1x1(ec.conv1x1_case(N, H, W, 1, Cin, Cout, 2), variants)


def test_conv1x1_dgrad():
    from occnet_amd import ext
    case = ec.conv1x1_dgrad_case()
    got = ext.conv1x1_dgrad_nhwc(_cl(case.inp["g"]), _f(case.inp["w"]))
    _same(got, case.ref().out, repr(case))


# ---- conv3x3_nhwc ------------------------------------------------------------------------------------------------------

def _pattern_max(t):
    return int((t.contiguous().view(torch.int16).to(torch.int32) & 0x7fff).max())


@pytest.mark.parametrize("N,C,Cout,H,W,stride", ec.CONV3X3_SHAPES)
def test_conv3x3_every_tile(N, C, Cout, H, W, stride):
    from occnet_amd import ext
    case = ec.conv3x3_case(N, C, Cout, H, W, stride)
    c = case.inp
    x, wp, b = _cl(c["x"]), ext.conv3x3_pack_weight(_f(c["w"])), _f(c["b"])
    for relu in (True, False):
        want = case.ref(relu=relu).out
        for v in ec.CONV3X3_TILES[stride] + (0, None):
            if v and Cout % (128 * (v // 10)):
                continue
            got = ext.conv3x3_nhwc(x, wp, b, Cout, relu=relu, stride=stride, variant=v)
            _same(got, want, f"{case!r} relu={relu} tile={v}")
            # with the amax words: the same output, and the decoded maximum is max|out| of the reference exactly
            words = ext.new_absmax_words(x.device)
            got_a = ext.conv3x3_nhwc(x, wp, b, Cout, relu=relu, stride=stride, amax=words, variant=v)
            _same(got_a, want, f"{case!r} relu={relu} tile={v} amax")
            assert int(words.max()) == _pattern_max(want) and int(words.min()) >= 0, (v, relu)


def test_conv3x3_dgrad():
    from occnet_amd import ext
    case = ec.conv3x3_dgrad_case()
    got = ext.conv3x3_dgrad_nhwc(_cl(case.inp["g"]), _f(case.inp["w"]))
    _same(got, case.ref().out, repr(case))


# ---- conv3x3_conv1x1_nhwc ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cmid", ec.FUSED_CMID)
@pytest.mark.parametrize("N,H,W,stride", ec.FUSED_GEOMETRIES)
def test_conv3x3_conv1x1_every_tile(N, H, W, stride, cmid):
    """One rounding at the mid tensor, one at the output: relu(conv1x1(rne(relu(conv3x3(x) + b2))) + b3 + residual)."""
    from occnet_amd import ext
    case = ec.fused_case(N, H, W, stride, cmid)
    c = case.inp
    x, p2, b2 = _cl(c["x"]), ext.conv3x3_pack_weight(_f(c["w2"])), _f(c["b2"])
    p3, b3, r = ext.conv1x1_pack_weight(_f(c["w3"])), _f(c["b3"]), _cl(c["r"])
    want = case.ref().out
    for v in ec.FUSED_TILES[(cmid, stride)]:
        got = ext.conv3x3_conv1x1_nhwc(x, p2, b2, cmid, p3, b3, r, stride=stride, variant=v)
        _same(got, want, f"{case!r} tile={v}")
        # the two launches it replaces obey the same contract
        mid = ext.conv3x3_nhwc(x, p2, b2, cmid, relu=True, stride=stride, variant=v)
        _same(ext.conv1x1_nhwc(mid, p3, b3, residual=r, relu=True), want, f"{case!r} pair tile={v}")


# ---- bottleneck64_nhwc -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,ds,N,H,W", ec.BOTTLENECK_SHAPES)
def test_bottleneck64_every_variant(cin, ds, N, H, W):
    """The two 64-channel intermediates are rounded to bf16; the identity (or the projection, contracted in the third
    convolution's accumulator with the biases added in fp32) joins before the one rounding of the output."""
    from occnet_amd import ext
    case = ec.bottleneck_case(cin, ds, N, H, W)
    c = case.inp
    pack = ext.bottleneck64_pack(_f(c["w1"]), _f(c["b1"]), _f(c["w2"]), _f(c["b2"]), _f(c["w3"]), _f(c["b3"]),
                                 _f(c["wds"]), _f(c["bds"]))
    x = _cl(c["x"])
    want = case.ref().out
    for v in ec.BOTTLENECK_VARIANTS:
        _same(ext.bottleneck64_nhwc(x, pack, variant=v), want, f"{case!r} variant={v}")


# ---- stem --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,W", ec.STEM_SHAPES)
def test_stem_conv7x7_pool(N, H, W):
    from occnet_amd import ext
    case = ec.stem_case(N, H, W)
    c = case.inp
    got = ext.stem_conv7x7_pool(_f(c["x"]), ext.stem_pack_weight(_f(c["w"])), _f(c["b"]))
    _same(got, case.ref().out, repr(case))


@pytest.mark.parametrize("N,Hs,Ws,to_rgb,mean,std", ec.STEM_U8_CASES)
def test_stem_conv7x7_pool_u8(N, Hs, Ws, to_rgb, mean, std):
    """Raw uint8 images against float64 normalise -> pad -> stem: a reference that is not the float stem kernel."""
    from occnet_amd import ext
    case = ec.stem_u8_case(N, Hs, Ws, to_rgb, mean, std)
    c = case.inp
    frag, b = ext.stem_pack_weight(_f(c["w"])), _f(c["b"])
    got, hw = ext.stem_conv7x7_pool_u8(c["raw"].cuda(), frag, b, mean, std, to_rgb=to_rgb)
    assert hw == c["hw"]
    _same(got, case.ref().out, repr(case))
    # and the float kernel on the normalised, padded tensor
    _same(ext.stem_conv7x7_pool(_f(c["x"]), frag, b), case.ref().out, f"{case!r} float path")


# ---- conv3d_bn_relu, conv3d_autograd -----------------------------------------------------------------------------------

def _conv3d_in(x, layout):
    B, Cin, Z, Y, X = x.shape
    if layout == 0:
        return x.permute(0, 3, 4, 2, 1).contiguous()                            # (B, Y, X, Z, Cin)
    return x.permute(0, 3, 4, 1, 2).reshape(B, Y * X, Cin * Z).contiguous()          # BEV embedding (lifter view)


@pytest.mark.parametrize("wide", ec.CONV3D_FLAVOURS)
@pytest.mark.parametrize("name,B,Z,Y,X,Cin", ec.CONV3D_SHAPES, ids=[s[0] for s in ec.CONV3D_SHAPES])
def test_conv3d_bn_relu(name, B, Z, Y, X, Cin, wide):
    from occnet_amd import ext
    case = ec.conv3d_case(name, B, Z, Y, X, Cin, wide)
    c = case.inp
    scale, shift = _f(c["scale"]), _f(c["shift"])
    relus = (True, False) if (name == "base_conv2" and wide == "w") else (True,)
    for precision in ("f32", "bf16x3"):
        wp = ext.conv3d_pack_weight(_f(c["w"]), precision=precision)
        for layout in (0, 1):
            xin = _f(_conv3d_in(c["x"], layout))
            for xy_major in (False, True):
                for relu in relus:
                    ref = case.ref(relu=relu).out
                    want = (ref.permute(0, 4, 3, 2, 1) if xy_major else ref.permute(0, 3, 4, 2, 1)).contiguous()
                    got = ext.conv3d_bn_relu(xin, wp, scale, shift, Z, Y, X, Cin, 32, in_layout=layout,
                                             out_xy_major=xy_major, relu=relu)
                    ec.assert_bit_equal(got, want, f"{case!r} {precision} layout={layout} xy_major={xy_major} relu={relu}")


@pytest.mark.parametrize("wide", ec.CONV3D_AUTOGRAD_FLAVOURS)
@pytest.mark.parametrize("B,Z,Y,X,Cin,layout", ec.CONV3D_AUTOGRAD_SHAPES)
def test_conv3d_autograd(B, Z, Y, X, Cin, layout, wide):
    """Forward, dx and dW of the decoder's training convolution; the wide operand is x, the weight or the output gradient."""
    from occnet_amd import ext
    case = ec.conv3d_autograd_case(B, Z, Y, X, Cin, layout, wide)
    c, ref = case.inp, case.ref()
    xin = _f(_conv3d_in(c["x"], layout)).requires_grad_(True)
    w = _f(c["w"]).requires_grad_(True)
    out = ext.conv3d_autograd(xin, w, Z, Y, X, in_layout=layout)
    out.backward(_f(c["go"].permute(0, 3, 4, 2, 1)))
    ec.assert_bit_equal(out, ref.out.permute(0, 3, 4, 2, 1).contiguous(), f"{case!r} forward")
    ec.assert_bit_equal(xin.grad, _conv3d_in(ref.extra["dx"], layout), f"{case!r} dx")
    ec.assert_bit_equal(w.grad, ref.extra["dw"].contiguous(), f"{case!r} dW")


# ---- linear, value_proj, linear_wgrad ----------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", ec.LINEAR_FLAVOURS)
@pytest.mark.parametrize("K1,K2,N", ec.LINEAR_KN)
def test_linear(K1, K2, N, wide):
    from occnet_amd import ext
    for M in ec.LINEAR_M:
        case = ec.linear_case(M, K1, K2, N, wide)
        c = case.inp
        for precision in ("f32", "bf16x3"):
            got = ext.linear(_f(c["a"]), _f(c["w"]), _f(c["b"]), a2=_f(c["a2"]), a2_add=_f(c["a2_add"]),
                             act="relu" if c["relu"] else None, residual=_f(c["res"]), precision=precision)
            ec.assert_bit_equal(got, case.ref().out, f"{case!r} {precision}")


@pytest.mark.parametrize("G,rpg,K,N,ogr,row0,nbias", ec.VALUE_PROJ_LAYOUTS)
def test_value_proj_bf16(G, rpg, K, N, ogr, row0, nbias):
    from occnet_amd import ext
    case = ec.value_proj_case(G, rpg, K, N, ogr, row0, nbias)
    c = case.inp
    out = torch.full(((G - 1) * ogr + row0 + rpg + 5, N), float("nan"), device="cuda")
    ext.value_proj_bf16(ec.to_bf16(c["a"]).cuda(), _f(c["w"]), _f(c["gb"]), out, rows_per_group=rpg, out_group_rows=ogr,
                        out_row0=row0)
    want = case.ref().out
    for gi in range(G):
        ec.assert_bit_equal(out[gi * ogr + row0: gi * ogr + row0 + rpg], want[gi * rpg:(gi + 1) * rpg], f"{case!r} group {gi}")


def test_value_proj_bf16_planes():
    from occnet_amd import ext
    cams, K, N, P, hws = ec.VALUE_PROJ_PLANES
    cases = ec.value_proj_planes_cases()
    starts = [sum(hws[:i]) for i in range(len(hws))]
    total = sum(hws)
    a_list = [ec.to_bf16(cases[0][s].inp["a"]).cuda() for s in range(len(hws))]
    ws = [_f(cases[p][0].inp["w"]) for p in range(P)]
    gbs = [torch.stack([_f(cases[p][s].inp["gb"]) for s in range(len(hws))]) for p in range(P)]
    out = torch.full((P, cams * total, N), float("nan"), device="cuda")
    ext.value_proj_bf16_planes(a_list, ws, gbs, out, rows_per_group=list(hws), out_group_rows=total, out_row0=starts)
    for p in range(P):
        single = torch.full((cams * total, N), float("nan"), device="cuda")
        ext.value_proj_bf16(a_list, ws[p], gbs[p], single, rows_per_group=list(hws), out_group_rows=total, out_row0=starts)
        for s, hw in enumerate(hws):
            want = cases[p][s].ref().out.view(cams, hw, N)
            for name, o in (("planes", out[p]), ("one launch", single)):
                ec.assert_bit_equal(o.view(cams, total, N)[:, starts[s]:starts[s] + hw], want, f"{name} plane {p} segment {s}")


@pytest.mark.parametrize("wide", ec.LINEAR_WGRAD_FLAVOURS)
@pytest.mark.parametrize("N,K", ec.LINEAR_WGRAD_NK)
def test_linear_wgrad(N, K, wide):
    from occnet_amd import ext
    for M in ec.LINEAR_WGRAD_M:
        case = ec.linear_wgrad_case(M, N, K, wide)
        dw, db = ext.linear_wgrad(_f(case.inp["dy"]), _f(case.inp["x"]))
        ec.assert_bit_equal(dw, case.ref().out, f"{case!r} dW")
        ec.assert_bit_equal(db, case.ref().extra["db"], f"{case!r} db")


# ---- conv1x1_wgrad_nhwc, conv3x3_wgrad_nhwc, bias_act_bwd_nhwc -----------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cin,Cout", ec.CONV_WGRAD_CHANNELS)
def test_conv_wgrad(Cin, Cout, stride, k):
    """The fp32 weight gradient is the float64 sum, the bf16 one its RNE, for every split count."""
    from occnet_amd import ext
    fn = ext.conv1x1_wgrad_nhwc if k == 1 else ext.conv3x3_wgrad_nhwc
    for (N, H, W) in ec.CONV_WGRAD_MAPS:
        case = ec.conv_wgrad_case(k, stride, Cin, Cout, N, H, W)
        g, x = _cl(case.inp["g"]), _cl(case.inp["x"])
        for splits in ec.CONV_WGRAD_SPLITS:
            for dtype in (torch.float32, torch.bfloat16):
                got = fn(g, x, stride=stride, out_dtype=dtype, splits=splits)
                want = case.ref(bf16=dtype == torch.bfloat16).out
                ec.assert_bit_equal(got, want, f"{case!r} splits={splits} {dtype}")


@pytest.mark.parametrize("N,C,H,W", ec.BIAS_ACT_BWD_SHAPES)
def test_bias_act_bwd_bias_gradient_is_the_exact_column_sum(N, C, H, W):
    from occnet_amd import ext
    case = ec.bias_act_bwd_case(N, C, H, W)
    gy = _cl(case.inp["gy"])
    y = ec.to_bf16(case.inp["y"]).cuda().contiguous(memory_format=torch.channels_last)
    assert bool((y.view(torch.int16) == -32768).any())                     # the negative zeros survive the trip
    for relu in (True, False):
        ref = case.ref(relu=relu)
        got_g, got_b = ext.bias_act_bwd_nhwc(gy, y if relu else None, relu=relu)
        ec.assert_bit_equal(got_g, ref.extra["g"], f"{case!r} relu={relu} g")
        ec.assert_bit_equal(got_b, ref.out, f"{case!r} relu={relu} bias gradient")


# ---- the linear chains (csrc/linear_chain_x3.hip): exact stages ---------------------------------------------------------------

@pytest.fixture
def x3(monkeypatch):
    """The chain programs exist in the bf16x3 precision mode only (the environment could set the other one)."""
    from occnet_amd import ext
    monkeypatch.setattr(ext, "LINEAR_PRECISION", "bf16x3")
    return ext


def _chain_tall():
    """The tall M: all 16 k-step rotations on 64-row tiles and, from the device's CU count, on 32-row tiles."""
    return ec.CHAIN_M_FULL, ec.chain_m_half(torch.cuda.get_device_properties(0).multi_processor_count)


def _chain_runs(flavours):
    """(M, flavour): both flavours at the small M; the tall M walk the tiles, which does not depend on the flavour: one
    each."""
    return [(M, w) for M in ec.CHAIN_M_SMALL for w in flavours] + list(zip(_chain_tall(), flavours))


def _ln0(beta):
    """A LayerNorm with gamma = 0: its output is the row beta."""
    return torch.zeros(256, device="cuda"), _f(beta), 1e-5


def _rows_equal(y, beta, what):
    """Every row of y is the row beta, bit for bit (the columns are distinct integers: a permuted store shows)."""
    assert tuple(y.shape) == (y.shape[0], 256)
    bad = (y != _f(beta)[None]).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements of y differ from beta, first at {tuple(int(i) for i in bad[0])}"


@pytest.mark.parametrize("term", [False, True])
@pytest.mark.parametrize("nq", ec.CHAIN_NQ)
def test_linear_pair_chain(nq, term, x3):
    for M, wide in _chain_runs(ec.CHAIN_PAIR_FLAVOURS):
        case = ec.pair_chain_case(M, nq, term, wide)
        c = case.inp
        zq, zv = x3.linear_pair_chain(_f(c["a"]), _f(c["wq"]), _f(c["term"]), _f(c["wv"]), _f(c["bv"]))
        assert zq.shape == (M, nq) and zv.shape == (M, 256)
        ec.assert_bit_equal(torch.cat([zq, zv], 1), case.ref().out, f"{case!r}")


@pytest.mark.parametrize("wide", ec.CHAIN_TAIL_FLAVOURS)
@pytest.mark.parametrize("n2", ec.CHAIN_N2)
def test_linear_ln_chain_tail(n2, wide, x3):
    """Program A behind gamma = 0: y is beta in every row and z = act2(beta . W2^T + b2), ReLU on and off."""
    for M, relu in [(M, r) for M in ec.CHAIN_M_SMALL for r in (False, True)] + list(zip(_chain_tall(), (True, False))):
        case = ec.tail_a_case(M, n2, wide)
        c = case.inp
        y, z = x3.linear_ln_chain(c["a"].cuda(), c["res"].cuda(), c["w1"].cuda(), c["b1"].cuda(), _ln0(c["beta"]),
                                  _f(c["w2"]), _f(c["b2"]), act2="relu" if relu else None)
        _rows_equal(y, c["beta"], f"{case!r}")
        ec.assert_bit_equal(z, case.ref(relu=relu).out, f"{case!r} relu={relu}")


@pytest.mark.parametrize("term", [False, True])
@pytest.mark.parametrize("nq", ec.CHAIN_NQ)
def test_encoder_ffn_chain_tail(nq, term, x3):
    """Program B behind gamma2 = 0: y (which parks x2 until x3 overwrites it) is beta2 in every row, and the tail is
    [beta2 . Wq^T + term | beta2 . Wv^T + bv]."""
    for M, wide in _chain_runs(ec.CHAIN_TAIL_FLAVOURS):
        case = ec.tail_b_case(M, nq, term, wide)
        c = case.inp
        d = {k: c[k].cuda() for k in ("a", "res", "wo", "bo", "g1", "be1", "w1", "b1", "w2", "b2")}
        y, zq, zv = x3.encoder_ffn_chain(d["a"], d["res"], d["wo"], d["bo"], (d["g1"], d["be1"], 1e-5), d["w1"], d["b1"],
                                         d["w2"], d["b2"], _ln0(c["beta"]),
                                         tail=(_f(c["wq"]), _f(c["term"]), _f(c["wv"]), _f(c["bv"])))
        _rows_equal(y, c["beta"], f"{case!r}")
        assert zq.shape == (M, nq) and zv.shape == (M, 256)
        ec.assert_bit_equal(torch.cat([zq, zv], 1), case.ref().out, f"{case!r}")


# ---- LayerNorm on exact integer inputs, under the bound counted from the kernel sources (tests/ln_bound.py) -------------------

LN_M = (65, 8229)


def _check_ln(got, ref, c, mean_roundings, what, constant=None):
    from tests import ln_bound as lb
    ratio = lb.worst_ratio(got, ref, ref.bound(c, mean_roundings))
    print(f"{what}: c = {c}, worst err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: err / bound = {ratio:.4g} with c = {c}"
    if constant is not None:                           # a constant row is beta, exactly
        rows = got.detach().cpu()[constant]
        assert torch.equal(rows, ref.beta.float()[None].expand_as(rows)), f"{what}: a constant row is not beta"


@pytest.mark.parametrize("M", LN_M)
def test_linear_ln_chain_layernorm(M, x3):
    """y of linear_ln_chain on the four row kinds.  |y - ref| <= 24 U |t| + U |y|: the count is in tests/ln_bound.py."""
    from tests import ln_bound as lb
    c = lb.ln_case(M, 256)
    ref = lb.LnRef(c["x"], c["gamma"], c["beta"])
    w2 = torch.zeros(32, 256, device="cuda")
    y, _ = x3.linear_ln_chain(_f(c["a"]), _f(c["res"]), _f(c["wo"]), _f(c["bo"]), (c["gamma"].cuda(), c["beta"].cuda(), 1e-5),
                              w2, None)
    _check_ln(y, ref, lb.C_CHAIN, 0, f"linear_ln_chain M={M}", c["kind"] == lb.CONSTANT)


@pytest.mark.parametrize("M", LN_M)
def test_encoder_ffn_chain_layernorm(M, x3):
    """gamma1 = 0 makes x2 the row beta1 and pre2 = relu(x2 . W1^T + b1) . W2^T + b2 + x2 an exact integer
    (tests/exact_cases.ffn_case); y = LayerNorm2(pre2) under the bound of ch_layernorm.  A missing ReLU, a missing x2, a
    lost low plane of h or a dropped k element miss it by factors of 1e4 and more (tests/test_ln_bound_host.py)."""
    from tests import ln_bound as lb
    case = ec.ffn_case(M)
    c = case.inp
    ref = lb.LnRef(case.ref().value, c["g2"], c["be2"])
    y, zq, zv = x3.encoder_ffn_chain(c["a"].cuda(), c["res"].cuda(), c["wo"].cuda(), c["bo"].cuda(), _ln0(c["beta1"]),
                                     _f(c["w1"]), _f(c["b1"]), _f(c["w2"]), _f(c["b2"]), (c["g2"].cuda(), c["be2"].cuda(), 1e-5))
    assert zq is None and zv is None and y.shape == (M, 256)
    _check_ln(y, ref, lb.C_CHAIN, 0, f"encoder_ffn_chain M={M}")


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("N", [256, 128, 100])
def test_linear_layernorm_epilogue(N, precision):
    """linear(..., residual=, ln=) on the four row kinds: c = 12, and for N = 100 (1 / N and the mean are not exact) c = 14
    with the two terms of the inexact mean (tests/ln_bound.py)."""
    from occnet_amd import ext
    from tests import ln_bound as lb
    cc, mr = lb.linear_c(N)
    for M in LN_M:
        c = lb.ln_case(M, N)
        ref = lb.LnRef(c["x"], c["gamma"], c["beta"])
        y = ext.linear(_f(c["a"]), _f(c["wo"]), _f(c["bo"]), residual=_f(c["res"]), ln=(c["gamma"].cuda(), c["beta"].cuda(), 1e-5),
                       precision=precision)
        _check_ln(y, ref, cc, mr, f"linear ln= N={N} {precision} M={M}", c["kind"] == lb.CONSTANT)
