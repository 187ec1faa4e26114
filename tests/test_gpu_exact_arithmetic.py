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

Out of scope: the LayerNorm and Softplus epilogues, the linear_*_chain kernels and occ_heads (transcendentals and
divisions are not exact), the BatchNorm statistics and heads-loss kernels, and the gather kernels (float64 tests in every
mode already).  bias_relu_maxpool_nhwc and bias_act_nhwc_ are compared bit for bit in tests/test_gpu_backbone.py.  Both
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
