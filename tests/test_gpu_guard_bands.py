"""-m gpu: every kernel reads and writes only its own tensors (tests/guard_bands.py).

Each test runs an entry point twice on a case of the existing suites: plainly, and with every input inside a poisoned arena
(NaN bands for floats, 0xA5 bytes for integers and uint8 frames, an out-of-range value for indices) while every allocation the
wrapper makes -- outputs, workspaces, packed weights -- is framed too.  It then asserts that the C-ABI function it claims to
cover was launched, that no band changed, and that the framed result equals the plain one bit for bit (so no NaN came in from
a band, not even times zero).  The families whose sums go through float atomics are compared with their float64 reference
under the bound their own suite uses instead, and checked for new non-finite elements separately.

The shapes are the small ones of the existing lists: below one tile, ragged with batch >= 2 (the neighbour is then another
image as well as the band), and one ragged case per forced tile or variant.  A line "GUARD <family> <arenas>" is printed per run."""
import pytest
import torch

from tests import exact_cases as ec
from tests import guard_bands as gb

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(autouse=True)
def _leave_the_process_as_found():
    """After every test: the derived-weight caches (which pin the framed weights they packed) hold what they held before,
    torch's CPU generator is where it was, and every arena is zeroed before its memory goes back to the caching allocator -- no
    later test finds NaN in a fresh torch.empty because this file ran first."""
    from occnet_amd import derived
    caches = derived.snapshot()
    rng = torch.get_rng_state()
    yield
    torch.cuda.synchronize()
    derived.restore(caches)
    torch.set_rng_state(rng)
    gb.release()


def _cl(t64):
    return ec.to_bf16(t64).cuda().contiguous(memory_format=CL)


def _f(t64):
    return None if t64 is None else ec._f32(t64).cuda().contiguous()


def _guard(family, fn, inputs, *entries, defined=None):
    """run_guarded + the three assertions every bit-equal family shares."""
    r = gb.run_guarded(fn, inputs)
    r.record.require(*entries)
    gb.assert_bit_equal(r.plain, r.framed, defined)
    print(f"GUARD {family} {r.n_arenas}")
    return r


def _direct(name, *args):
    """A C-ABI launcher no wrapper of occnet_amd.ext calls, on the current stream."""
    from occnet_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


# ---- backbone: conv1x1_nhwc ----------------------------------------------------------------------------------------------------

def _conv1x1(case, variant, relu=True):
    from occnet_amd import ext
    c = case.inp

    def fn(x, w, b, r):
        return ext.conv1x1_nhwc(x, ext.conv1x1_pack_weight(w), b, residual=r, relu=relu, stride=c["stride"],
                                residual_upsample2=c["up"], variant=variant)
    r = _guard("conv1x1", fn, [_cl(c["x"]), _f(c["w"]), _f(c["b"]), None if c["r"] is None else _cl(c["r"])],
               "occ_conv1x1_nhwc_bf16_variant", "occ_mfma_pack_b_frag_bf16")
    ec.assert_bit_equal(r.framed, case.ref(relu=relu).out, f"{case!r} variant={variant}")


@pytest.mark.parametrize("Cin,Cout", [(128, 1024), (256, 128), (512, 128)])
def test_conv1x1_resident_variants(Cin, Cout):
    """Below one tile with the launcher's choice; every variant id on a ragged two-image map with a residual and on a ragged
    three-image stride-2 map."""
    from tests.test_gpu_conv1x1_variants import _variants
    _conv1x1(ec.conv1x1_case(1, 5, 7, 1, Cin, Cout, 0), None, relu=False)
    for v in _variants(Cin, Cout):
        _conv1x1(ec.conv1x1_case(2, 13, 11, 1, Cin, Cout, 1), v)
        _conv1x1(ec.conv1x1_case(3, 9, 15, 2, Cin, Cout, 0), v)


@pytest.mark.parametrize("Cin,Cout", [(1024, 256), (96, 160), (32, 32)])
def test_conv1x1_tiled_kernel(Cin, Cout):
    for (N, H, W, s) in ec.CONV1X1_TILED_GEOMETRIES:
        for v in (None, 1):
            _conv1x1(ec.conv1x1_case(N, H, W, s, Cin, Cout, 1), v)


@pytest.mark.parametrize("Cin,Cout", [(128, 1024), (96, 160)])
def test_conv1x1_upsampled_residual(Cin, Cout):
    from tests.test_gpu_conv1x1_variants import _variants
    for (N, H, W) in ec.CONV1X1_UP2_GEOMETRIES:
        for v in (_variants(Cin, Cout) if Cin == 128 else (None, 1)):
            _conv1x1(ec.conv1x1_case(N, H, W, 1, Cin, Cout, 2), v)


def test_conv1x1_plain_entry_point_and_dgrad():
    """occ_conv1x1_nhwc_bf16 (the entry point without a variant, bound by the backbone plan) and the data gradient."""
    from occnet_amd import ext
    case = ec.conv1x1_case(2, 13, 11, 1, 128, 128, 1)
    c = case.inp

    def fn(x, w, b, r):
        N, Cin, H, W = x.shape
        out = torch.empty((N, b.numel(), H, W), dtype=torch.bfloat16, device=x.device, memory_format=CL)
        _direct("occ_conv1x1_nhwc_bf16", x, ext.conv1x1_pack_weight(w), b, r, out, N, H, W, Cin, b.numel(), 1, 1, 0)
        return out
    r = _guard("conv1x1", fn, [_cl(c["x"]), _f(c["w"]), _f(c["b"]), _cl(c["r"])], "occ_conv1x1_nhwc_bf16")
    ec.assert_bit_equal(r.framed, case.ref(relu=True).out, repr(case))
    d = ec.conv1x1_dgrad_case()
    r = _guard("conv1x1", ext.conv1x1_dgrad_nhwc, [_cl(d.inp["g"]), _f(d.inp["w"])], "occ_conv1x1_nhwc_bf16_variant")
    ec.assert_bit_equal(r.framed, d.ref().out, repr(d))


# ---- backbone: conv3x3_nhwc, conv3x3_conv1x1_nhwc ----------------------------------------------------------------------------

@pytest.mark.parametrize("N,C,Cout,H,W,stride", ec.CONV3X3_SHAPES)
def test_conv3x3_every_tile(N, C, Cout, H, W, stride):
    """Every forced tile of the shape, with and without the amax words (framed like any other input: 8 words between bands)."""
    from occnet_amd import ext
    case = ec.conv3x3_case(N, C, Cout, H, W, stride)
    c = case.inp
    for v in ec.CONV3X3_TILES[stride] + (None,):
        if v and Cout % (128 * (v // 10)):
            continue
        for with_amax in (False, True):
            def fn(x, w, b, words):
                words = None if words is None else torch.empty_like(words).copy_(words)
                out = ext.conv3x3_nhwc(x, ext.conv3x3_pack_weight(w), b, Cout, relu=True, stride=stride, amax=words, variant=v)
                return out, words
            words = ext.new_absmax_words("cuda") if with_amax else None
            r = _guard("conv3x3", fn, [_cl(c["x"]), _f(c["w"]), _f(c["b"]), words],
                       "occ_conv3x3_nhwc_bf16_variant", "occ_conv3x3_pack_weight_bf16")
            ec.assert_bit_equal(r.framed[0], case.ref(relu=True).out, f"{case!r} tile={v} amax={with_amax}")


def test_conv3x3_plain_entry_points_and_dgrad():
    """occ_conv3x3_nhwc_bf16 and occ_conv3x3_nhwc_bf16_amax, which ext reaches only through the variant entry point."""
    from occnet_amd import ext
    case = ec.conv3x3_case(2, 128, 128, 9, 21, 1)
    c = case.inp

    def fn(x, w, b, words):
        N, Cin, H, W = x.shape
        outs = [torch.empty((N, 128, H, W), dtype=torch.bfloat16, device=x.device, memory_format=CL) for _ in range(2)]
        wp, words = ext.conv3x3_pack_weight(w), torch.empty_like(words).copy_(words)
        _direct("occ_conv3x3_nhwc_bf16", x, wp, b, outs[0], N, H, W, Cin, 128, 1, 0)
        _direct("occ_conv3x3_nhwc_bf16_amax", x, wp, b, outs[1], N, H, W, Cin, 128, 1, 0, words)
        return outs, words
    r = _guard("conv3x3", fn, [_cl(c["x"]), _f(c["w"]), _f(c["b"]), ext.new_absmax_words("cuda")],
               "occ_conv3x3_nhwc_bf16", "occ_conv3x3_nhwc_bf16_amax")
    for o in r.framed[0]:
        ec.assert_bit_equal(o, case.ref(relu=False).out, repr(case))
    d = ec.conv3x3_dgrad_case()
    r = _guard("conv3x3", ext.conv3x3_dgrad_nhwc, [_cl(d.inp["g"]), _f(d.inp["w"])], "occ_conv3x3_nhwc_bf16_variant")
    ec.assert_bit_equal(r.framed, d.ref().out, repr(d))


@pytest.mark.parametrize("cmid", ec.FUSED_CMID)
@pytest.mark.parametrize("N,H,W,stride", ec.FUSED_GEOMETRIES)
def test_conv3x3_conv1x1_every_tile(N, H, W, stride, cmid):
    from occnet_amd import ext
    case = ec.fused_case(N, H, W, stride, cmid)
    c = case.inp
    for v in ec.FUSED_TILES[(cmid, stride)]:
        def fn(x, w2, b2, w3, b3, r):
            return ext.conv3x3_conv1x1_nhwc(x, ext.conv3x3_pack_weight(w2), b2, cmid, ext.conv1x1_pack_weight(w3), b3, r,
                                            stride=stride, variant=v)
        r = _guard("conv3x3_conv1x1", fn, [_cl(c["x"]), _f(c["w2"]), _f(c["b2"]), _f(c["w3"]), _f(c["b3"]), _cl(c["r"])],
                   "occ_conv3x3_conv1x1_nhwc_bf16")
        ec.assert_bit_equal(r.framed, case.ref().out, f"{case!r} tile={v}")


# ---- backbone: bottleneck64, stem, pointwise --------------------------------------------------------------------------------

def _bottleneck_inputs(c):
    return [_cl(c["x"])] + [_f(c[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "wds", "bds")]


@pytest.mark.parametrize("cin,ds,N,H,W", ec.BOTTLENECK_SHAPES)
def test_bottleneck64_every_variant(cin, ds, N, H, W):
    """Identity and projection blocks, below one tile (3 x 5) and ragged with two images, every variant id; the entry point
    without a variant once per shape."""
    from occnet_amd import ext
    case = ec.bottleneck_case(cin, ds, N, H, W)
    for v in ec.BOTTLENECK_VARIANTS:
        def fn(x, *ws):
            return ext.bottleneck64_nhwc(x, ext.bottleneck64_pack(*ws), variant=v)
        r = _guard("bottleneck64", fn, _bottleneck_inputs(case.inp), "occ_bottleneck64_nhwc_bf16_variant")
        ec.assert_bit_equal(r.framed, case.ref().out, f"{case!r} variant={v}")

    def plain_entry(x, *ws):
        p = ext.bottleneck64_pack(*ws)
        out = torch.empty((N, 256, H, W), dtype=torch.bfloat16, device=x.device, memory_format=CL)
        _direct("occ_bottleneck64_nhwc_bf16", x, p["w1"], p["b1"], p["w2"], p["b2"], p["w3"], p["b3"], out, N, H, W, cin,
                1 if ds else 0)
        return out
    r = _guard("bottleneck64", plain_entry, _bottleneck_inputs(case.inp), "occ_bottleneck64_nhwc_bf16")
    ec.assert_bit_equal(r.framed, case.ref().out, f"{case!r} plain entry point")


@pytest.mark.parametrize("N,H,W", [(1, 3, 5), (2, 13, 21), (1, 16, 24)])
def test_bottleneck64_next(N, H, W):
    """The block that emits the next stage's conv1 and shortcut: its inputs framed as well as its two outputs."""
    from occnet_amd import ext
    case = ec.bottleneck_case(256, False, N, H, W)
    g = ec._gen("guard_bottleneck64_next", N, H, W)
    w1n, b1n = ec.ints(g, (128, 256), 1, keep=8), ec.ints(g, (128,), 64)
    wds, bds = ec.ints(g, (512, 256), 1, keep=8), ec.ints(g, (512,), 64)

    def fn(x, w1, b1, w2, b2, w3, b3, w1n, b1n, wds, bds):
        pack = ext.bottleneck64_pack(w1, b1, w2, b2, w3, b3)
        fused = ext.bottleneck64_next_nhwc(x, pack, ext.conv1x1_pack_weight(w1n), b1n, ext.conv1x1_pack_weight(wds), bds)
        return fused
    inputs = _bottleneck_inputs(case.inp)[:7] + [_f(w1n), _f(b1n), _f(wds), _f(bds)]
    r = _guard("bottleneck64", fn, inputs, "occ_bottleneck64_next_nhwc_bf16")
    # the three launches it replaces, on the plain tensors
    x, pack = inputs[0], ext.bottleneck64_pack(*inputs[1:7])
    mid = ext.bottleneck64_nhwc(x, pack, variant=2)
    y = ext.conv1x1_nhwc(mid, ext.conv1x1_pack_weight(inputs[7]), inputs[8], relu=True, variant=2)
    sc = ext.conv1x1_nhwc(mid, ext.conv1x1_pack_weight(inputs[9]), inputs[10], stride=2, variant=2)
    gb.assert_bit_equal((y, sc), r.framed)


@pytest.mark.parametrize("N,H,W", ec.STEM_SHAPES[:2] + [(2, 9, 7)])
def test_stem_f32(N, H, W):
    from occnet_amd import ext
    case = ec.stem_case(N, H, W)
    c = case.inp

    def fn(x, w, b):
        return ext.stem_conv7x7_pool(x, ext.stem_pack_weight(w), b)
    r = _guard("stem", fn, [_f(c["x"]), _f(c["w"]), _f(c["b"])], "occ_stem_conv7x7_pool_f32_bf16")
    ec.assert_bit_equal(r.framed, case.ref().out, repr(case))


@pytest.mark.parametrize("N,Hs,Ws,to_rgb,mean,std", ec.STEM_U8_CASES)
def test_stem_u8(N, Hs, Ws, to_rgb, mean, std):
    """The frames sit between bands of 0xA5 bytes; 37 x 53 and 64 x 90 are padded at the bottom and the right, where the
    kernel clamps: a byte taken from a band would be normalised into the sum as (165 - mean) / std."""
    from occnet_amd import ext
    case = ec.stem_u8_case(N, Hs, Ws, to_rgb, mean, std)
    c = case.inp

    def fn(raw, w, b):
        return ext.stem_conv7x7_pool_u8(raw, ext.stem_pack_weight(w), b, mean, std, to_rgb=to_rgb)[0]
    r = _guard("stem", fn, [c["raw"].cuda(), _f(c["w"]), _f(c["b"])], "occ_stem_conv7x7_pool_u8_bf16")
    ec.assert_bit_equal(r.framed, case.ref().out, repr(case))


@pytest.mark.parametrize("N,C,H,W", [(2, 64, 12, 20), (1, 8, 7, 9), (1, 16, 1, 1), (3, 64, 5, 2)])
def test_bias_relu_maxpool_and_bias_act(N, C, H, W):
    """The shapes of tests/test_gpu_backbone.py.  bias_act_nhwc_ works in place: its target is a framed copy of x."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(3)
    y = torch.randn(N, C, H, W, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    res = torch.randn(N, C, H, W, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=CL)
    b = torch.randn(C, generator=g).cuda()
    r = _guard("pointwise", ext.bias_relu_maxpool_nhwc, [y, b], "occ_bias_relu_maxpool_nhwc_bf16")
    want = torch.nn.functional.max_pool2d((y.float() + b.view(1, -1, 1, 1)).relu(), 3, 2, 1)
    assert torch.equal(r.framed, want.to(torch.bfloat16))
    for with_res, relu in ((False, True), (True, True), (False, False)):
        def fn(x, bias, residual):
            out = torch.empty_like(x)               # framed under guarded_allocations: the in-place target has bands
            out.copy_(x)
            return ext.bias_act_nhwc_(out, bias, residual=residual, relu=relu)
        r = _guard("pointwise", fn, [y, b, res if with_res else None], "occ_bias_act_nhwc_bf16")
        want = y.float() + b.view(1, -1, 1, 1) + (res.float() if with_res else 0)
        assert torch.equal(r.framed, (want.relu() if relu else want).to(torch.bfloat16))


@pytest.mark.parametrize("N,C,H,W", ec.BIAS_ACT_BWD_SHAPES[:4])
def test_bias_act_bwd(N, C, H, W):
    from occnet_amd import ext
    case = ec.bias_act_bwd_case(N, C, H, W)
    gy, y = _cl(case.inp["gy"]), ec.to_bf16(case.inp["y"]).cuda().contiguous(memory_format=CL)
    for relu in (True, False):
        def fn(gy, y):
            g, db = ext.bias_act_bwd_nhwc(gy, y if relu else None, relu=relu)
            return (g, db) if relu else db          # without ReLU g is grad_y itself
        r = _guard("pointwise", fn, [gy, y], "occ_bias_act_bwd_nhwc_bf16")
        ec.assert_bit_equal(r.framed[1] if relu else r.framed, case.ref(relu=relu).out, f"{case!r} relu={relu}")


# ---- decoder: conv3d_bn_relu, heads -------------------------------------------------------------------------------------------

GUARD_CONV3D = [("one_pillar", 1, 16, 1, 1, 16), ("z4_c8", 1, 4, 5, 33, 8), ("hires_z32_c8_b2", 2, 32, 3, 9, 8),
                ("z16_c24", 1, 16, 3, 9, 24), ("base_conv2", 2, 16, 7, 10, 32)]


def _conv3d_in(x, layout):
    B, Cin, Z, Y, X = x.shape
    if layout == 0:
        return x.permute(0, 3, 4, 2, 1).contiguous()
    return x.permute(0, 3, 4, 1, 2).reshape(B, Y * X, Cin * Z).contiguous()


@pytest.mark.parametrize("name,B,Z,Y,X,Cin", GUARD_CONV3D, ids=[s[0] for s in GUARD_CONV3D])
def test_conv3d_bn_relu(name, B, Z, Y, X, Cin):
    """Both precisions, both input layouts, both output orders.  The halo taps and the weight tiles are clamped loads."""
    from occnet_amd import ext
    case = ec.conv3d_case(name, B, Z, Y, X, Cin, "x")
    c = case.inp
    ref = case.ref(relu=True).out
    for precision in ("f32", "bf16x3"):
        x3 = precision == "bf16x3" and (Cin % 16 == 0 or Cin == 8)          # any other Cin has the f32 kernel only
        entry = "occ_conv3d_bn_relu_bf16x3_f32" if x3 else "occ_conv3d_bn_relu_f32"
        pack = "occ_conv3d_pack_weight_bf16x3" if x3 else "occ_conv3d_pack_weight_f32"
        for layout in (0, 1):
            for xy_major in (False, True):
                def fn(x, w, scale, shift):
                    return ext.conv3d_bn_relu(x, ext.conv3d_pack_weight(w, precision=precision), scale, shift, Z, Y, X, Cin, 32,
                                              in_layout=layout, out_xy_major=xy_major)
                r = _guard("conv3d", fn, [_f(_conv3d_in(c["x"], layout)), _f(c["w"]), _f(c["scale"]), _f(c["shift"])],
                           entry, pack)
                want = (ref.permute(0, 4, 3, 2, 1) if xy_major else ref.permute(0, 3, 4, 2, 1)).contiguous()
                ec.assert_bit_equal(r.framed, want, f"{case!r} {precision} layout={layout} xy_major={xy_major}")


def _heads_weights(g, ncls, C=32):
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).cuda()
    return [mk(64, C), mk(64), mk(ncls, 64), mk(ncls), mk(64, C), mk(64), mk(2, 64), mk(2)]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("n_rows,ncls", [(1, 17), (31, 17), (77, 3)])
def test_occ_heads(n_rows, ncls, precision):
    """The cases of tests/test_gpu_decoder.py::test_occ_heads_match_oracle below one 32-row tile, one row short of it and
    ragged over three; with and without the decoded classes, and the entry point without them."""
    from occnet_amd import ext
    from oracle import decoder as odec
    g = torch.Generator().manual_seed(40 + n_rows)
    feat = torch.randn(n_rows, 32, generator=g) * 2.0
    feat[0, :] = 30.0
    ws = _heads_weights(g, ncls)
    for decode in (False, True):
        r = _guard("heads", lambda feat, *ws: ext.occ_heads(feat, *ws, decode=decode, precision=precision),
                   [feat.cuda()] + ws, "occ_occ_heads_decode_f32")
    occ_ref, flow_ref = odec.heads(feat.double(), *[t.cpu().double() for t in ws])
    tol = 2e-5 if precision == "f32" else 1e-4          # the tolerances of test_occ_heads_match_oracle
    assert float((r.framed[0].cpu().double() - occ_ref).abs().max()) / max(1.0, float(occ_ref.abs().max())) < tol
    assert float((r.framed[1].cpu().double() - flow_ref).abs().max()) / max(1.0, float(flow_ref.abs().max())) < tol
    if precision == "f32":
        def plain_entry(feat, *ws):
            occ = torch.empty((n_rows, ncls), dtype=torch.float32, device=feat.device)
            flow = torch.empty((n_rows, 2), dtype=torch.float32, device=feat.device)
            _direct("occ_occ_heads_f32", feat, *ws, occ, flow, n_rows, 32, 64, ncls)
            return occ, flow
        p = _guard("heads", plain_entry, [feat.cuda()] + ws, "occ_occ_heads_f32")
        gb.assert_bit_equal(p.framed, r.framed[:2])


@pytest.mark.parametrize("B,Y,X,Z,ncls", [(1, 1, 1, 16, 17), (2, 3, 4, 32, 17), (1, 3, 9, 16, 5)])
def test_conv3d_heads_decode(B, Y, X, Z, ncls):
    """Cases of tests/test_gpu_decoder.py::FUSED_CASES: one pillar, two ragged images at Z = 32, a run-time class count."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(61)
    x = torch.randn(B, Y, X, Z, 32, generator=g).cuda()
    w = (torch.randn(32, 32, 3, 3, 3, generator=g) * (2.0 / (32 * 27)) ** 0.5).cuda()
    scale, shift = (torch.rand(32, generator=g) + 0.5).cuda(), (torch.randn(32, generator=g) * 0.1).cuda()
    hw = [t * (0.6 if t.dim() == 2 else 0.3) for t in _heads_weights(g, ncls)]

    def fn(x, w, scale, shift, *hw):
        return ext.conv3d_heads_decode(x, ext.conv3d_pack_weight(w, precision="bf16x3"), scale, shift,
                                       ext.conv3d_heads_pack(*hw), Z, Y, X, ncls)
    r = _guard("heads", fn, [x, w, scale, shift] + hw, "occ_conv3d_heads_decode_bf16x3_f32", "occ_conv3d_heads_pack")
    occ, flow, cls = r.framed
    assert torch.equal(cls, occ.softmax(-1).argmax(-1))
    feat = ext.conv3d_bn_relu(x, ext.conv3d_pack_weight(w, precision="bf16x3"), scale, shift, Z, Y, X, 32, 32, in_layout=0,
                              out_xy_major=True)
    occ2, flow2 = ext.occ_heads(feat, *hw, precision="bf16x3")
    assert float((occ - occ2).abs().max()) < 2e-5 and float((flow - flow2).abs().max()) < 2e-5      # as the decoder suite


@pytest.mark.parametrize("wide", ["x", "g"])
@pytest.mark.parametrize("B,Z,Y,X,Cin,layout", ec.CONV3D_AUTOGRAD_SHAPES)
def test_conv3d_autograd(B, Z, Y, X, Cin, layout, wide):
    """Conv3dX3Function forward and backward; then the weight-gradient kernel again on framed copies of the padded tensors
    the node builds with F.pad (which guarded_allocations does not frame)."""
    from occnet_amd import _lib, ext
    case = ec.conv3d_autograd_case(B, Z, Y, X, Cin, layout, wide)
    c, ref = case.inp, case.ref()

    def fn(x, w, go):
        x, w = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
        out = ext.conv3d_autograd(x, w, Z, Y, X, in_layout=layout)
        out.backward(go)
        return out.detach(), x.grad, w.grad
    r = _guard("conv3d_train", fn, [_f(_conv3d_in(c["x"], layout)), _f(c["w"]), _f(c["go"].permute(0, 3, 4, 2, 1))],
               "occ_conv3d_bn_relu_bf16x3_f32", "occ_conv3d_wgrad_bf16x3_f32")
    ec.assert_bit_equal(r.framed[0], ref.out.permute(0, 3, 4, 2, 1).contiguous(), f"{case!r} forward")
    ec.assert_bit_equal(r.framed[1], _conv3d_in(ref.extra["dx"], layout), f"{case!r} dx")
    ec.assert_bit_equal(r.framed[2], ref.extra["dw"].contiguous(), f"{case!r} dW")

    pad = lambda t: torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1, 1, 1)).contiguous()

    def wgrad(gp, xp):
        nbytes = int(_lib.lib().occ_conv3d_wgrad_workspace_bytes(B, Z, Y, X, Cin))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=gp.device)
        dw = torch.empty((32, 27, Cin), dtype=torch.float32, device=gp.device)
        _direct("occ_conv3d_wgrad_bf16x3_f32", gp, xp, dw, ws, nbytes, B, Z, Y, X, Cin)
        return dw.permute(0, 2, 1).reshape(32, Cin, 3, 3, 3)
    r = _guard("conv3d_train", wgrad, [pad(_f(c["go"].permute(0, 3, 4, 2, 1))), pad(_f(c["x"].permute(0, 3, 4, 2, 1)))],
               "occ_conv3d_wgrad_bf16x3_f32")
    ec.assert_bit_equal(r.framed, ref.extra["dw"].contiguous(), f"{case!r} dW, framed padded operands")


@pytest.mark.parametrize("geom", [(1, 1, 2, 1), (1, 1, 7, 1), (1, 3, 5, 4), (2, 6, 7, 8)])
def test_bn3d_relu_train(geom):
    """Statistics, forward and backward of the decoder's training BatchNorm at the smallest geometries of
    tests/test_gpu_bn3d_relu_train.py (two rows, seven rows, a halo, two images), both output orders, with the padded
    gradient; the running statistics are updated in place, so they are framed copies."""
    from occnet_amd import ext
    from tests import test_gpu_bn3d_relu_train as bn
    c = bn._case(geom)
    B, Y, X, Z = geom

    def fn(y, go, gamma, beta, rm, rv):
        rm, rv = torch.empty_like(rm).copy_(rm), torch.empty_like(rv).copy_(rv)
        mean_rstd = ext.bn3d_relu_train_stats(y, rm, rv, 0.1, bn.EPS)
        outs = [ext.bn3d_relu_train_fwd(y, mean_rstd, gamma, beta, Z, Y, X, out_xy_major=m) for m in (False, True)]
        gy, gp, dgamma, dbeta = ext.bn3d_relu_train_bwd(go, y, mean_rstd, gamma, beta, Z, Y, X, want_grad_y_pad=True)
        return mean_rstd, rm, rv, outs, gy, gp, dgamma, dbeta
    y, go = (c[k].cuda().view(B, Y, X, Z, 32) for k in ("y", "go"))
    r = _guard("bn3d", fn, [y, go] + [c[k].cuda() for k in ("gamma", "beta", "rm", "rv")],
               "occ_bn3d_relu_train_stats_f32", "occ_bn3d_relu_train_fwd_f32", "occ_bn3d_relu_train_bwd_f32")
    mean_rstd, _, _, outs, gy, gp, dgamma, dbeta = r.framed
    assert all(bool(torch.isfinite(t).all()) for t in (mean_rstd, outs[0], gy, dgamma, dbeta))
    assert torch.equal(outs[1], outs[0].permute(0, 2, 1, 3, 4)) and torch.equal(gp[:, 1:-1, 1:-1, 1:-1], gy)
    assert float(gp.abs().sum()) == float(gy.abs().sum())               # the halo is zero


# ---- GEMMs -------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def x3(monkeypatch):
    """The chain programs and the q16 epilogue exist in the bf16x3 precision mode only."""
    from occnet_amd import ext
    monkeypatch.setattr(ext, "LINEAR_PRECISION", "bf16x3")
    return ext


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("K1,K2,N", [(192, 64, 256), (32, 16, 64), (256, 0, 96), (48, 0, 64)])
def test_linear(K1, K2, N, precision):
    """One row, and 33 rows (one past the 32-row tile); the split cases carry a2 + a2_add, bias, ReLU and residual; N = 96 is no
    multiple of 64, K = 48 none of 32."""
    from occnet_amd import ext
    entry = "occ_linear_bf16x3_f32" if precision == "bf16x3" else "occ_linear_f32"
    for M in (1, 33):
        case = ec.linear_case(M, K1, K2, N, "a")
        c = case.inp

        def fn(a, w, b, a2, a2_add, res):
            return ext.linear(a, w, b, a2=a2, a2_add=a2_add, act="relu" if c["relu"] else None, residual=res,
                              precision=precision)
        r = _guard("linear", fn, [_f(c[k]) for k in ("a", "w", "b", "a2", "a2_add", "res")], entry)
        ec.assert_bit_equal(r.framed, case.ref().out, f"{case!r} {precision}")


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("N", [256, 100])
def test_linear_layernorm_epilogue(N, precision):
    """residual + LayerNorm epilogue on the rows of tests/ln_bound.py; N = 100 is no multiple of 32.  Under that suite's bound."""
    from occnet_amd import ext
    from tests import ln_bound as lb
    cc, mr = lb.linear_c(N)
    for M in (1, 65):
        c = lb.ln_case(M, N)
        ref = lb.LnRef(c["x"], c["gamma"], c["beta"])

        def fn(a, wo, bo, res, gamma, beta):
            return ext.linear(a, wo, bo, residual=res, ln=(gamma, beta, 1e-5), precision=precision)
        r = _guard("linear", fn, [_f(c["a"]), _f(c["wo"]), _f(c["bo"]), _f(c["res"]), c["gamma"].cuda(), c["beta"].cuda()],
                   "occ_linear_bf16x3_f32" if precision == "bf16x3" else "occ_linear_f32")
        assert lb.worst_ratio(r.framed, ref, ref.bound(cc, mr)) <= 1.0


@pytest.mark.parametrize("S,groups", [(1, 1), (63, 1), (65, 2)])
def test_linear_q16rows_and_rows_encode(S, groups, x3):
    """The q16 epilogue and the stand-alone encoder it must equal (tests/test_gpu_tsa_fused_q16.py's smallest shapes: one row,
    an odd S, an odd S with two maps).  The pad pixel of an odd S is zeroed by the wrapper, so the whole output is defined."""
    from tests import test_gpu_tsa_fused_q16 as tq
    w, b = tq._weights()
    a = torch.randn(S * groups, 256, generator=torch.Generator().manual_seed(S)).cuda() * 3.0
    a[::7] *= 1e-3
    y = x3.linear(a, w, b)
    s = tq._pow2_scale(y)
    r = _guard("linear", lambda a, w, b, s: x3.linear_q16rows(a, w, b, s, groups), [a, w, b, s], "occ_linear_bf16x3_q16rows")
    e = _guard("linear", x3.sca_rows_encode_q16, [y.view(groups, S, 256), s], "occ_sca_rows_encode_q16")
    gb.assert_bit_equal(e.framed, r.framed)
    _guard("linear", lambda a, w: x3.linear_q16rows(a, w, None, None, groups), [a, w], "occ_linear_bf16x3_q16rows")


@pytest.mark.parametrize("G,rpg,K,N,ogr,row0,nbias", ec.VALUE_PROJ_LAYOUTS)
def test_value_proj_bf16(G, rpg, K, N, ogr, row0, nbias):
    """fp32 and fp16-pair outputs (q16 rows come from the activation-resident kernel only: test_value_proj_resident_q16); the
    output is NaN-filled inside its frame, so the rows between the groups must stay NaN and the bands behind the last group
    untouched."""
    from occnet_amd import ext
    case = ec.value_proj_case(G, rpg, K, N, ogr, row0, nbias)
    c = case.inp
    rows = (G - 1) * ogr + row0 + rpg + 5
    rows += rows & 1
    for dtype, entry in ((torch.float32, "occ_value_proj_bf16_f32"), (torch.float16, "occ_value_proj_bf16_f16pairs")):
        if dtype == torch.float16 and (ogr & 1 or N % 32):
            continue

        def fn(a, w, gbias, scale):
            out = torch.empty((rows, N), dtype=dtype, device=a.device)
            out.fill_(float("nan"))
            ext.value_proj_bf16(a, w, gbias, out, rows_per_group=rpg, out_group_rows=ogr, out_row0=row0,
                                out_scale=None if dtype == torch.float32 else scale)
            return out
        r = _guard("value_proj", fn, [ec.to_bf16(c["a"]).cuda(), _f(c["w"]), _f(c["gb"]),
                                      torch.full((1,), 2.0 ** -8, device="cuda")], entry, "occ_linear_pack_weight_bf16x3")
        if dtype == torch.float32:
            for gi in range(G):
                ec.assert_bit_equal(r.framed[gi * ogr + row0: gi * ogr + row0 + rpg], case.ref().out[gi * rpg:(gi + 1) * rpg],
                                    f"{case!r} group {gi}")
            assert bool(torch.isnan(r.framed[(G - 1) * ogr + row0 + rpg:]).all())


def test_value_proj_bf16_planes():
    from occnet_amd import ext
    cams, K, N, P, hws = ec.VALUE_PROJ_PLANES
    cases = ec.value_proj_planes_cases()
    starts = [sum(hws[:i]) for i in range(len(hws))]
    total = sum(hws)

    def fn(a_list, ws, gbs):
        out = torch.empty((P, cams * total, N), dtype=torch.float32, device="cuda")
        out.fill_(float("nan"))
        return ext.value_proj_bf16_planes(a_list, ws, gbs, out, rows_per_group=list(hws), out_group_rows=total, out_row0=starts)
    a_list = [ec.to_bf16(cases[0][s].inp["a"]).cuda() for s in range(len(hws))]
    ws = [_f(cases[p][0].inp["w"]) for p in range(P)]
    gbs = [torch.stack([_f(cases[p][s].inp["gb"]) for s in range(len(hws))]) for p in range(P)]
    r = _guard("value_proj", fn, [a_list, ws, gbs], "occ_value_proj_bf16_planes")
    for p in range(P):
        for s, hw in enumerate(hws):
            ec.assert_bit_equal(r.framed[p].view(cams, total, N)[:, starts[s]:starts[s] + hw],
                                cases[p][s].ref().out.view(cams, hw, N), f"plane {p} segment {s}")


@pytest.mark.parametrize("rows,K,strided", [((1, 7, 300), 64, False), ((513, 64), 256, True)])
def test_value_range_scale_pair(rows, K, strided):
    """The maps of tests/test_gpu_value_range.py::test_value_range_scale_matches_torch (same seed, same draws): three small
    maps, and two maps that are column slices of wider ones (the columns behind a strided row hold 1e30 in the plain run and
    NaN in the frame); then value_range_scale_from_amax on the words a producer would have left for the same maps."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(5)
    maps = []
    for i, r in enumerate(rows):
        t = (torch.randn(r, 2 * K if strided else K, generator=g) * (3.0 + i)).to(torch.bfloat16).cuda()
        if strided:
            t[:, K:] = 1e30
        maps.append(t[:, :K] if strided else t)
    maps[-1][rows[-1] // 2, K - 3] = -777.0
    l1, bm = [13.5, 0.25, 40.0, 7.0], [0.5, 3.0, 0.0, 100.0]
    r = _guard("value_range", lambda maps: ext.value_range_scale(maps, l1, bm), [maps], "occ_value_range_scale_bf16")
    assert r.framed.shape == (9,) and float(r.framed[4]) == 776.0          # bf16(777) = 776
    words = ext.feature_absmax_words(maps)
    p = _guard("value_range", lambda w: ext.value_range_scale_from_amax(w, l1, bm), [words], "occ_value_range_scale_from_amax")
    gb.assert_bit_equal(p.framed, r.framed)


@pytest.mark.parametrize("N,K", ec.LINEAR_WGRAD_NK)
def test_linear_wgrad(N, K):
    """One row and 257 rows (ragged against every chunk), with and without the bias gradient."""
    from occnet_amd import ext
    for M in (1, 257):
        case = ec.linear_wgrad_case(M, N, K, "dy")
        for with_bias in (True, False):
            r = _guard("wgrad", lambda dy, x: ext.linear_wgrad(dy, x, with_bias=with_bias),
                       [_f(case.inp["dy"]), _f(case.inp["x"])], "occ_linear_wgrad_bf16x3_f32")
            ec.assert_bit_equal(r.framed[0], case.ref().out, f"{case!r} dW")
            assert (r.framed[1] is None) == (not with_bias)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_wgrad(stride, k):
    """The ragged two-image map and the one-pixel map, per split count, both output types."""
    from occnet_amd import ext
    fn = ext.conv1x1_wgrad_nhwc if k == 1 else ext.conv3x3_wgrad_nhwc
    for (Cin, Cout) in ec.CONV_WGRAD_CHANNELS[:2]:
        for (N, H, W) in ec.CONV_WGRAD_MAPS:
            case = ec.conv_wgrad_case(k, stride, Cin, Cout, N, H, W)
            for splits in ec.CONV_WGRAD_SPLITS:
                for dtype in (torch.float32, torch.bfloat16):
                    r = _guard("wgrad", lambda g, x: fn(g, x, stride=stride, out_dtype=dtype, splits=splits),
                               [_cl(case.inp["g"]), _cl(case.inp["x"])], f"occ_conv{k}x{k}_wgrad_nhwc_bf16")
                    ec.assert_bit_equal(r.framed, case.ref(bf16=dtype == torch.bfloat16).out, f"{case!r} splits={splits}")


@pytest.mark.parametrize("M", [1, 65])
def test_linear_chains(M, x3):
    """The three chain programs with their inputs framed (their outputs already are in tests/test_gpu_linear.py): the pair
    chain as it stands, the other two behind a gamma = 0 LayerNorm, where they are exact."""
    zero = torch.zeros(256, device="cuda")
    case = ec.pair_chain_case(M, 192, True, "a")
    c = case.inp
    r = _guard("chains", x3.linear_pair_chain, [_f(c[k]) for k in ("a", "wq", "term", "wv", "bv")],
               "occ_linear_pair_chain_bf16x3_f32", "occ_linear_chain_pack_bf16x3")
    ec.assert_bit_equal(torch.cat(r.framed, 1), case.ref().out, repr(case))

    case = ec.tail_a_case(M, 288, "beta")
    c = case.inp
    r = _guard("chains", lambda a, res, w1, b1, g, beta, w2, b2: x3.linear_ln_chain(a, res, w1, b1, (g, beta, 1e-5), w2, b2),
               [c["a"].cuda(), c["res"].cuda(), c["w1"].cuda(), c["b1"].cuda(), zero, _f(c["beta"]), _f(c["w2"]), _f(c["b2"])],
               "occ_linear_ln_chain_bf16x3_f32")
    ec.assert_bit_equal(r.framed[1], case.ref(relu=False).out, repr(case))

    case = ec.tail_b_case(M, 192, True, "beta")
    c = case.inp

    def ffn(a, res, wo, bo, g1, be1, w1, b1, w2, b2, g2, beta, wq, term, wv, bv):
        return x3.encoder_ffn_chain(a, res, wo, bo, (g1, be1, 1e-5), w1, b1, w2, b2, (g2, beta, 1e-5), tail=(wq, term, wv, bv))
    inputs = [c[k].cuda() for k in ("a", "res", "wo", "bo", "g1", "be1", "w1", "b1", "w2", "b2")]
    inputs += [zero, _f(c["beta"])] + [_f(c[k]) for k in ("wq", "term", "wv", "bv")]
    r = _guard("chains", ffn, inputs, "occ_encoder_ffn_chain_bf16x3_f32")
    ec.assert_bit_equal(torch.cat(r.framed[1:], 1), case.ref().out, repr(case))


def test_value_proj_resident_q16():
    """The q16 and fp16 epilogues of the activation-resident projection (K = 256, N = 256, groups of 240 and 160 rows, two
    groups): the case of tests/test_gpu_q16.py, one projection, scales from the range kernel."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(11)
    hws, G, K, N = [(12, 20), (16, 10)], 2, 256, 256
    a_list = [torch.randn(G * h * w, K, generator=g).to(torch.bfloat16).cuda() for h, w in hws]
    w = ((torch.rand(N, K, generator=g) * 2 - 1) * 0.1).cuda()
    gbias = torch.randn(len(hws), G, N, generator=g).cuda()
    rpg = [h * w for h, w in hws]
    total = sum(rpg)
    t = ext.value_range_scale(a_list, [float(w.abs().sum(1).max())], [float(gbias.abs().max())])
    for dtype, entry in ((torch.int16, "occ_value_proj_bf16_q16pairs"), (torch.float16, "occ_value_proj_bf16_f16pairs")):
        def fn(a_list, w, gbias, scale):
            out = torch.empty((G * total, N), dtype=dtype, device="cuda")
            return ext.value_proj_bf16(a_list, w, gbias, out, rows_per_group=rpg, out_group_rows=total, out_row0=[0, rpg[0]],
                                       out_scale=scale)
        _guard("value_proj", fn, [a_list, w, gbias, t[:1].clone()], entry)


# ---- gathers -----------------------------------------------------------------------------------------------------------------

from tests.test_gpu_msda import CASES as _MSDA_CASES          # noqa: E402

MSDA_FWD = [c for c in _MSDA_CASES if c[0] in ("single", "ragged_items", "scalar_d16", "sca_like")]


@pytest.mark.parametrize("name,B,shapes,M,D,Lq,P", MSDA_FWD, ids=[c[0] for c in MSDA_FWD])
def test_ms_deform_attn_forward(name, B, shapes, M, D, Lq, P):
    """Sampling locations on the corners, just outside and 1e7 away (tests/test_gpu_msda.py::_inputs): the bands say whether
    such a sample reads anything.  The level shape and start tensors are framed with -1: no size and no row of any map (a
    sample measured against a map of that size is admitted nowhere, so even a stray read of the band stays inside the arenas)."""
    from occnet_amd import ext
    from oracle import msda as omsda
    from tests.test_gpu_msda import _inputs
    value, shapes_t, start, loc, attn = _inputs(B, shapes, M, D, Lq, P, seed=1)
    r = _guard("msda", lambda v, sh, st, l, a: ext.ms_deform_attn_forward(v, sh, st, l, a, im2col_step=64),
               [value.cuda(), gb.Poisoned(shapes_t.cuda(), -1), gb.Poisoned(start.cuda(), -1), loc.cuda(), attn.cuda()],
               "occ_ms_deform_attn_forward_f32")
    ref = omsda.multi_scale_deformable_attn_pytorch(value.double(), shapes_t, loc.double(), attn.double()).float()
    assert float((r.framed.cpu() - ref).abs().max()) < 2e-5          # the bound of test_forward_matches_oracle


def _msda_backward(value, shapes_t, start, loc, attn, grad_out):
    from occnet_amd import ext
    gv, gl, ga = torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(attn)
    ext.ms_deform_attn_backward(value, shapes_t, start, loc, attn, grad_out, gv, gl, ga, im2col_step=64)
    return gv, gl, ga


def _msda_inputs(name):
    from tests import test_gpu_backward as tb
    (value, shapes_t, start, loc, attn, grad_out), refs = tb._case_of(name)
    return [value.cuda(), gb.Poisoned(shapes_t.cuda(), -1), gb.Poisoned(start.cuda(), -1), loc.cuda(), attn.cuda(),
            grad_out.cuda()], refs


@pytest.mark.parametrize("name", ["single", "ragged_items", "sca_like"])
def test_ms_deform_attn_backward_workspace_path(name, monkeypatch):
    """The binned path with its scratch, bins and gradient tensors framed.  Under the deterministic replay the framed run
    equals the plain one bit for bit; in the default mode grad_value has no promised last bits and is held to the oracle."""
    from tests import test_gpu_backward as tb
    inputs, refs = _msda_inputs(name)
    monkeypatch.delenv("OCC_MSDA_BWD_ATOMICS", raising=False)
    monkeypatch.setenv("OCC_MSDA_BWD_DETERMINISTIC", "1")
    r = _guard("msda", _msda_backward, inputs, "occ_ms_deform_attn_backward_ws_f32")
    tb._assert_within_bound(f"{name} framed, deterministic", r.framed, refs)
    monkeypatch.delenv("OCC_MSDA_BWD_DETERMINISTIC")
    r = gb.run_guarded(_msda_backward, inputs)
    r.record.require("occ_ms_deform_attn_backward_ws_f32")
    gb.assert_bit_equal(r.plain[1:], r.framed[1:])                   # grad_loc and grad_attn are bit-reproducible
    tb._assert_within_bound(f"{name} framed", r.framed, refs)
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    print(f"GUARD msda {r.n_arenas}")


@pytest.mark.parametrize("name", ["ragged_items", "sca_like"])
def test_ms_deform_attn_backward_atomic_fallback(name, monkeypatch):
    """OCC_MSDA_BWD_ATOMICS=1, the kernel test_float_atomic_fallback_matches_autograd_oracle selects: float atomics, so the
    framed run is held to the float64 oracle under that file's bound, and must not gain a non-finite element."""
    from tests import test_gpu_backward as tb
    inputs, refs = _msda_inputs(name)
    monkeypatch.delenv("OCC_MSDA_BWD_DETERMINISTIC", raising=False)
    monkeypatch.setenv("OCC_MSDA_BWD_ATOMICS", "1")
    r = gb.run_guarded(_msda_backward, inputs)
    r.record.require("occ_ms_deform_attn_backward_ws_f32")
    tb._assert_within_bound(f"{name} framed (float atomics)", r.framed, refs)
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    print(f"GUARD msda {r.n_arenas}")


@pytest.mark.parametrize("name", ["generic_d16", "generic_d24"])
def test_ms_deform_attn_backward_plain_entry_point(name):
    """occ_ms_deform_attn_backward_f32, the reference interface without a caller's workspace, at head dimensions that take
    float atomics throughout (no scratch is allocated behind the caller's back)."""
    from tests import test_gpu_backward as tb
    inputs, refs = _msda_inputs(name)

    def fn(value, shapes_t, start, loc, attn, grad_out):
        B, S, M, D = value.shape
        _, Lq, _, L, P, _ = loc.shape
        gv, gl, ga = torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(attn)
        _direct("occ_ms_deform_attn_backward_f32", value, shapes_t, start, loc, attn, grad_out, gv, gl, ga, B, S, M, D, L, Lq,
                P, 64)
        return gv, gl, ga
    r = gb.run_guarded(fn, inputs)
    r.record.require("occ_ms_deform_attn_backward_f32")
    tb._assert_within_bound(f"{name} framed (plain entry point)", r.framed, refs)
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    print(f"GUARD msda {r.n_arenas}")


@pytest.mark.parametrize("case", ["L4P8_Z4_B2", "L4P8_Z2_B2_Nq7", "L4P8_Z8_B2_Nq1"])
@pytest.mark.parametrize("kernel", ["f32", "f16", "q16", "f16-hm", "q16-hm"])
def test_sca_fused_forward(kernel, case, monkeypatch):
    """Every value format, query-major and head-major, on the main two-image case and the 7- and 1-query tails; 16-bit rows go
    in already in pixel-pair order, so that the tensor the kernel reads is the framed one."""
    from occnet_amd import ext
    from tests import test_gpu_sca_fused as sf
    fmt = sf._select(kernel, monkeypatch)
    i = sf.CASE_IDS.index(case)
    c, dev = sf._case(i)
    rows, kw, ref = sf._rows(i, fmt)
    if fmt == "f16":
        rows, kw = ext.sca_pair_layout(rows), dict(value_layout="pairs")
    entry = {"f32": "occ_sca_fused_forward_f32", "f16": "occ_sca_fused_forward_f16v", "q16": "occ_sca_fused_forward_q16v"}[fmt]

    def fn(rows, shapes, starts, offs, logits, ref_cam, vis):
        return ext.sca_fused_forward(rows, shapes, starts, offs, logits, ref_cam, vis, sf.M, c["L"], c["P"], **kw)
    r = _guard("sca", fn, [rows, gb.Poisoned(dev["shapes"], -1), gb.Poisoned(dev["starts"], -1), dev["offs"],
                           dev["logits"], dev["ref_cam"], dev["vis"]], entry)
    assert sf._err(r.framed, ref) < sf.GPU_TOL


@pytest.mark.parametrize("B,LP", [(1, (4, 8)), (2, (4, 4)), (2, (1, 8))])
def test_sca_fused_backward(B, LP, monkeypatch):
    """tests/test_gpu_sca_fused_backward.py's case generator at 37 queries (anchors and offsets across and beyond the borders,
    offs / logits as slices of one wider tensor).  Deterministic replay: bit for bit; default scatter: grad_value under the
    suite's bound against float64 autograd."""
    from occnet_amd import ext
    from tests import test_gpu_sca_fused_backward as sb
    c = sb._case(B, *LP, Nq=37, seed=B * 10 + LP[0] + LP[1])

    def fn(value, shapes, starts, lin, ref_cam, vis, grad_slots):
        return ext.sca_fused_backward(value, shapes, starts, lin[..., :c["n_off"]], lin[..., c["n_off"]:c["n_off"] + c["n_att"]],
                                      ref_cam, vis, grad_slots, sb.M, c["L"], c["P"])
    inputs = [c["value"].cuda(), gb.Poisoned(c["shapes"].cuda(), -1), gb.Poisoned(c["starts"].cuda(), -1),
              c["lin"].cuda(), c["ref_cam"].cuda(), c["vis"].cuda(), c["grad_slots"].cuda()]
    ref = sb._restated(c)

    def within(got):
        for name, a, rr in zip(("grad_value", "grad_offs", "grad_logits"), got, ref):
            scale = float(rr.abs().max())
            assert float((a.cpu().double() - rr).abs().max()) <= sb.SCA_FUSED_GRAD_REL * scale + sb.SCA_FUSED_GRAD_ABS, name
    monkeypatch.setenv("OCC_MSDA_BWD_DETERMINISTIC", "1")
    r = _guard("sca", fn, inputs, "occ_sca_fused_backward_f32")
    within(r.framed)
    monkeypatch.delenv("OCC_MSDA_BWD_DETERMINISTIC")
    r = gb.run_guarded(fn, inputs)
    r.record.require("occ_sca_fused_backward_f32")
    gb.assert_bit_equal(r.plain[1:], r.framed[1:])
    within(r.framed)
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    print(f"GUARD sca {r.n_arenas}")


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 9, 7), (2, 9, 7)])
def test_tsa_fused_forward(B, H, W):
    """fp32 and q16 rows, the two queue entries separate and shared (B = 1: one map read through stride 0), on the one-query
    map, an odd map (q16: a pad row) and the two-image one."""
    from occnet_amd import ext
    from tests import test_gpu_tsa_fused as tf
    from tests import tsa_ref as tr
    i = tf._idx(B, H, W)
    _, (value, offs, logits, ref_2d), ref = tf._case(i)
    Nq = H * W

    def f32(value, offs, logits, ref_2d, shared):
        return ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, tr.M, tr.P, shared_queue=shared)
    r = _guard("tsa", lambda *a: f32(*a, False), [value, offs, logits, ref_2d], "occ_tsa_fused_forward_f32")
    assert tf._err(r.framed, ref) < tr.GPU_TOL
    one = value.view(B, 2, Nq, tr.M, tr.D)[:, 1].contiguous()
    _guard("tsa", lambda *a: f32(*a, True), [one, offs, logits, ref_2d], "occ_tsa_fused_forward_f32")

    def q16(value, scale, offs, logits, ref_2d, shared):
        rows = ext.sca_rows_encode_q16(value.view(value.shape[0], Nq, tr.M * tr.D), scale)
        return ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, tr.M, tr.P, shared_queue=shared, value_scale=scale)
    scale = torch.full((1,), 2.0 ** 11, device="cuda")          # max|N(0, 1)| < 16 on these maps
    assert float(value.abs().max()) * 2.0 ** 11 <= 2.0 ** 15
    r = _guard("tsa", lambda *a: q16(*a, False), [value, scale, offs, logits, ref_2d], "occ_tsa_fused_forward_q16v")
    assert bool(torch.isfinite(r.framed).all())
    _guard("tsa", lambda *a: q16(*a, True), [one, scale, offs, logits, ref_2d], "occ_tsa_fused_forward_q16v")


@pytest.mark.parametrize("B,H,W", [(2, 9, 7), (1, 1, 5)])
def test_tsa_fused_backward(B, H, W, monkeypatch):
    from occnet_amd import ext
    from tests import test_gpu_tsa_fused_backward as tb
    (value, offs, logits, ref_2d, G), ref, kink = tb._case(tb._idx(B, H, W))
    inputs = [t.cuda() for t in (value, offs, logits, ref_2d, G)]
    monkeypatch.setattr(ext, "_TSA_LEVEL_TENSORS", {})          # the cached level tensors: a dict of this test's own

    def fn(value, offs, logits, ref_2d, G):
        ext._TSA_LEVEL_TENSORS.clear()          # rebuilt in either run, so that the framed run frames them
        return ext.tsa_fused_backward(value, offs, logits, ref_2d, G, H, W, tb.M, tb.P)
    monkeypatch.setenv("OCC_MSDA_BWD_DETERMINISTIC", "1")
    r = _guard("tsa", fn, inputs, "occ_tsa_fused_backward_f32")
    tb._compare(f"B{B}_{H}x{W} framed, deterministic", r.framed, ref, kink)
    monkeypatch.delenv("OCC_MSDA_BWD_DETERMINISTIC")
    r = gb.run_guarded(fn, inputs)
    r.record.require("occ_tsa_fused_backward_f32")
    gb.assert_bit_equal(r.plain[1:], r.framed[1:])
    tb._compare(f"B{B}_{H}x{W} framed", r.framed, ref, kink)
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    print(f"GUARD tsa {r.n_arenas}")


# ---- training glue ------------------------------------------------------------------------------------------------------------

def test_point_sampling_boundaries():
    from occnet_amd import ext
    from tests import train_glue_ref as tg
    for NC in tg.BOUNDARY_NC[:2]:
        inp = tg.point_boundary_case(NC)
        r = _guard("glue", lambda ref_3d, l2i, e2l: ext.point_sampling(ref_3d, l2i, e2l, inp["pc_range"], inp["img_h"],
                                                                      inp["img_w"]),
                   [inp["ref_3d"].cuda(), inp["lidar2img"].cuda(), inp["ego2lidar"].cuda()], "occ_point_sampling_f32")
        tg.assert_point_sampling_exact(*r.framed, tg.point_sampling_ref(**inp, exact=True))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("Z,bs,ld,kq", [(1, 1, 768, 1), (4, 2, 776, 3)])
def test_sca_prep(Z, bs, ld, kq, exact):
    """Forward and backward; the row maps are framed with -1, the row no query and no rebatched row has; proj with ld = 776
    has columns the kernels must not use."""
    from occnet_amd import ext
    from tests import train_glue_ref as tg
    case = tg.prep_case(Z, bs, ld, kq, exact)
    c = case.inp

    def fn(proj, r2q, q2r, ref_rb, shapes, g_loc, g_attn):
        proj = proj.detach().requires_grad_()
        loc, attn = ext.SCAPrepFunction.apply(proj, r2q, q2r, ref_rb, shapes, tg.PREP_M, tg.PREP_L, tg.PREP_P)
        torch.autograd.backward([loc, attn], [g_loc, g_attn])
        return loc.detach(), attn.detach(), proj.grad
    f = lambda t: t.float().cuda()
    r = _guard("glue", fn, [f(c["proj"]), gb.Poisoned(c["r2q"].cuda(), -1), gb.Poisoned(c["q2r"].cuda(), -1),
                            f(c["ref_rb"]), gb.Poisoned(torch.tensor(c["shapes"], device="cuda"), -1), f(c["g_loc"]),
                            f(c["g_attn"])], "occ_sca_prep_forward_f32", "occ_sca_prep_backward_f32")
    if exact:
        tg.assert_prep_exact(*r.framed, case.ref(), c)
    else:
        tg.assert_prep_general(*r.framed, case.ref())


@pytest.mark.parametrize("shape", [(1, 5, 7, 4, 1), (3, 9, 11, 4, 3), (3, 6, 3, 64, 6), (3, 7, 3, 768, 3)])
def test_rows_gather_sum(shape):
    """The index band is a row far out of range: an index read from it is skipped and its row missing from the sum; the case's
    own index already holds rows_in (skipped) and -1 (padding)."""
    from occnet_amd import ext
    from tests import train_glue_ref as tg
    case = tg.gather_case(*shape)
    c = case.inp
    r = _guard("glue", ext.rows_gather_sum, [c["x"].float().cuda(), gb.Poisoned(c["index"].cuda(), 1 << 40)],
               "occ_rows_gather_sum_f32")
    ec.assert_bit_equal(r.framed, case.ref(), repr(case))


@pytest.mark.parametrize("shape", [(3, 13, 5, 64), (2, 40, 3, 4)])
def test_rows_gather_sum_function(shape):
    from occnet_amd import ext
    from tests import train_glue_ref as tg
    case = tg.gather_pair_case(*shape)
    c = case.inp

    def fn(x, r2q, q2r, gout):
        x = x.detach().requires_grad_()
        out = ext.RowsGatherSumFunction.apply(x, r2q, q2r)
        out.backward(gout)
        return out.detach(), x.grad
    r = _guard("glue", fn, [c["x"].float().cuda(), gb.Poisoned(c["r2q"].cuda(), 1 << 40), gb.Poisoned(c["q2r"].cuda(), 1 << 40),
                            c["gout"].float().cuda()], "occ_rows_gather_sum_f32")
    want_out, want_grad = case.ref()
    ec.assert_bit_equal(r.framed[0], want_out, "rebatch")
    ec.assert_bit_equal(r.framed[1], want_grad, "gradient")


@pytest.mark.parametrize("rows,p", [(5, 0.0), (5, 0.1), (5, 0.5), (1, 0.75)])
def test_dropout_add_layernorm(rows, p):
    """Five rows: one block of four and one row into the next.  The keep mask is a hash of (seed, element index); the seed is
    drawn from torch's CPU generator, reseeded in front of either run.  p = 0.1 has no exact reference: its keep scale 1 / 0.9
    is no power of two, so tg.ln_train_case has no case for it.  That leg runs on the tensors of the p = 0.5 case and keeps the
    assertions that need no reference: both entry points ran, no band moved, framed == plain bit for bit, nothing non-finite."""
    from occnet_amd import ext
    from tests import train_glue_ref as tg
    exact = p in tg.LN_SCALE
    case = tg.ln_train_case(rows, p if exact else 0.5)
    c = case.inp

    def fn(x, res, gamma, beta, gy):
        x, res, gamma, beta = (t.detach().requires_grad_() for t in (x, res, gamma, beta))
        torch.manual_seed(c["torch_seed"])
        y = ext.DropoutAddLayerNormFunction.apply(x, res, gamma, beta, 1e-5, p)
        y.backward(gy)
        return y.detach(), x.grad, res.grad, gamma.grad, beta.grad
    f = lambda t: t.float().cuda()
    r = _guard("glue", fn, [f(c["x"]), f(c["res"]), c["gamma"].cuda(), c["beta"].cuda(), f(c["gy"])],
               "occ_dropout_add_ln_fwd_f32", "occ_dropout_add_ln_bwd_f32")
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    y, gx, gres, dgamma, dbeta = r.framed
    assert all(bool(torch.isfinite(t).all()) for t in r.framed)
    if exact:
        ref = case.ref()
        tg.assert_ln_train_forward(y, ref)
        tg.assert_ln_train_backward(gx if p > 0 else None, gres, dgamma, dbeta, ref)
    else:
        live = gres != 0                             # some elements dropped, most kept, the kept ones scaled by 1 / 0.9:
        dropped = (gx == 0) & live                   # the rounded scale and one product, 2^-23 each, stay below 1e-6
        assert 0.0 < float(dropped.sum()) / float(live.sum()) < 0.3
        kept = live & ~dropped
        assert float(((gx[kept] - gres[kept] / (1.0 - p)).abs() / gres[kept].abs()).max()) < 1e-6


@pytest.mark.parametrize("O,I,k", [(128, 256, 1), (128, 128, 3), (64, 3, 7)])
def test_conv_bn_fold(O, I, k):
    """The draws and the assertions of tests/test_gpu_backbone.py::test_conv_bn_fold_kernels_match_torch at its three small
    shapes: the fold bit for bit, its chain rule with the bf16 weight gradient in both memory formats."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(O + I + k)
    W = torch.randn(O, I, k, k, generator=g).cuda()
    gamma, beta = (torch.rand(O, generator=g) + 0.5).cuda(), torch.randn(O, generator=g).cuda()
    rstd, mean_rstd = (torch.rand(O, generator=g) + 0.5).cuda(), torch.randn(O, generator=g).cuda()
    r = _guard("glue", ext.conv_bn_fold_fwd, [W, gamma, beta, rstd, mean_rstd], "occ_conv_bn_fold_fwd_f32")
    wf, w16, b = r.framed
    sc = gamma * rstd
    assert torch.equal(wf, W * sc.view(-1, 1, 1, 1))
    assert w16.is_contiguous(memory_format=CL) and torch.equal(w16, wf.to(torch.bfloat16))
    assert float((b - (beta - gamma * mean_rstd)).abs().max()) <= 1e-6 * float(b.abs().max() + 1)
    gbias = torch.randn(O, generator=g).cuda()
    for fmt in (torch.contiguous_format, CL):
        gw = torch.randn(O, I, k, k, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=fmt)
        r = _guard("glue", ext.conv_bn_fold_bwd, [gw, W, gamma, rstd, mean_rstd, gbias], "occ_conv_bn_fold_bwd_f32")
        dW, dgamma = r.framed
        assert torch.equal(dW, gw.float() * sc.view(-1, 1, 1, 1))
        want = rstd.double() * (gw.double() * W.double()).sum((1, 2, 3)) - mean_rstd.double() * gbias.double()
        assert float((dgamma.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_selftest_fdiv():
    """The numerators and divisors of tests/test_gpu_value_range.py's fdiv test (same seed and mix) at 4 x 259 elements, held to
    its bound: within one ulp of the correctly rounded quotient."""
    n = 4 * 259
    g = torch.Generator().manual_seed(77)
    a = torch.cat([torch.rand(n // 4, generator=g), (torch.rand(n // 4, generator=g) - 0.5) * 600,
                   torch.randn(n // 4, generator=g) * 1e3, torch.randn(n // 4, generator=g) * 1e5]).cuda()
    d = torch.cat([1 + 31 * torch.rand(n // 4, generator=g), torch.randint(1, 4097, (n // 4,), generator=g).float(),
                   torch.randint(1, 7, (n // 4,), generator=g).float(), 1 + 31 * torch.rand(n // 4, generator=g)]).cuda()

    def fn(a, d):
        q = torch.empty_like(a)
        _direct("occ_selftest_fdiv_f32", a, d, q, n)
        return q
    r = _guard("glue", fn, [a, d], "occ_selftest_fdiv_f32")
    want = a.double() / d.double()
    ieee = want.float()
    ulp = torch.maximum(torch.abs(torch.nextafter(ieee, ieee * 2) - ieee), torch.full_like(ieee, 1e-45))
    assert float(((r.framed.double() - want).abs() / ulp.double()).max()) <= 1.0


# ---- loss and input ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["r60_c3", "r280_c18_tile", "r280_c30_mb1"])
def test_heads_loss(name):
    """Forward and backward through the wrappers, so that the incoming loss gradients and the occ denominator are framed too:
    60 rows without a mask, 280 rows over two images with a tile mask, class weights and uint8 labels holding 255 (the label
    band is 0xA5 = 165, no class), and the capped grid."""
    from occnet_amd import ext
    from tests import test_gpu_heads_loss as hl
    c = hl.CASES[name]
    feat, params, labels, flow_gt, mask, cw = hl._inputs(name)
    gos = torch.tensor([1.0 if v is None else v for v in c["gos"]])

    def fn(feat, params, labels, flow_gt, mask, cw, gos):
        losses = ext.heads_loss_forward(feat, *params, labels, flow_gt, mask, cw, c["ignore"], c["reduction"], c["max_blocks"])
        dfeat, grads = ext.heads_loss_backward(feat, *params, labels, flow_gt, mask, cw, c["ignore"], c["reduction"], gos,
                                               losses[2:], max_blocks=c["max_blocks"])
        return losses, dfeat, grads
    d = hl._dev
    r = _guard("loss", fn, [d(feat), [d(p) for p in params], d(labels), d(flow_gt), d(mask), d(cw), d(gos)],
               "occ_heads_loss_fwd_f32", "occ_heads_loss_bwd_f32")
    if None not in c["gos"]:                  # the bound of test_node_matches_float64_restatement, on losses and gradients
        ref_losses, ref_grads = hl._reference(name)
        for k in (0, 1):
            assert hl._rel(r.framed[0][k], ref_losses[k]) <= hl.gb.LINEAR_X3_REL, k
        for got, ref in zip([r.framed[1]] + list(r.framed[2]), ref_grads):
            assert hl._rel(got, ref) <= hl.gb.LINEAR_X3_REL


@pytest.mark.parametrize("name,args", [("small_dense", (1, 2, 1, 4, 6, 8, 300, 0.3)), ("time_indexed", (2, 2, 3, 8, 20, 24, 2000, 0.05)),
                                       ("origin_outside", (5, 1, 1, 16, 40, 40, 800, 0.1))])
def test_dvr_render_forward(name, args):
    from occnet_amd import ext
    from tests.test_gpu_dvr import _case
    seed, N, T, Z, Y, X, M, occ = args
    inputs = [t.cuda() for t in _case(seed, N, T, Z, Y, X, M, occ, outside=name == "origin_outside")]
    for phase in ("test", "train"):
        _guard("dvr", lambda s, o, p, t: ext.dvr_render_forward(s, o, p, t, [T, Z, Y, X], phase), inputs,
               "occ_dvr_render_forward_f32")


@pytest.mark.parametrize("loss", ["l1", "l2", "absrel"])
@pytest.mark.parametrize("name", ["small_dense", "degenerate"])
def test_dvr_render(name, loss):
    """pred and gt are bit-reproducible; grad_sigma is summed with float atomics and is held to the float64 restatement under
    dvr_render_ref.grad_bound, as tests/test_gpu_dvr_render.py holds the plain run."""
    from occnet_amd import ext
    from tests import test_gpu_dvr_render as dr
    inputs = [t.cuda() for t in dr._inputs(name)]
    r = gb.run_guarded(lambda s, o, p, t: ext.dvr_render(s, o, p, t, loss), inputs)
    r.record.require("occ_dvr_render_f32")
    gb.assert_bit_equal(r.plain[:2], r.framed[:2])
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    got = tuple(t.cpu().numpy() for t in r.framed)
    if name == "degenerate":
        assert (got[0] == -1).all() and (got[1] == -1).all() and not got[2].any()
    else:
        dr._compare(f"{name} {loss} framed", got, dr._reference(name, loss))
    print(f"GUARD dvr {r.n_arenas}")


@pytest.mark.parametrize("shape", [(37, 53), (5, 9)])
def test_input_u8(shape):
    """input_u8_scaled at a scale that reaches all four clamps (1.25 on 37 x 53) and at 0.5, and train_input_u8 on the same
    frames: uint8 frames between 0xA5 bands, the records framed too, GridMask on."""
    import numpy as np
    from occnet_amd import ext
    from tests import input_scale_ref as S
    from tests import train_input_ref as R
    rec = torch.from_numpy(np.ascontiguousarray(R.RECORDS, dtype=np.float32)).cuda()
    for scale in (1.25, 0.5, None):
        c = R.case(shape, "imagenet_rgb") if scale is None else S.case(shape, "imagenet_rgb", scale)
        frames = torch.from_numpy(np.ascontiguousarray(c["frames"])).cuda()
        H, W = R.padded(*shape) if scale is None else S.sizes(*shape, scale)[1]
        gm = R.grid_cases(H, W)["both_mode1"]
        if scale is None:
            _guard("input", lambda fr, rec: ext.train_input_u8(fr, rec, c["mean"], c["std"], c["to_rgb"], grid_mask=gm),
                   [frames, rec], "occ_train_input_u8_f32")
        else:
            _guard("input", lambda fr, rec: ext.input_u8_scaled(fr, rec, c["mean"], c["std"], c["to_rgb"], scale, grid_mask=gm),
                   [frames, rec], "occ_input_u8_scaled_f32")


# ---- evaluation ----------------------------------------------------------------------------------------------------------------

def _framed_copy(t):
    """A copy made with torch.empty_like: inside guarded_allocations it is framed, so a state a kernel adds to has bands."""
    return torch.empty_like(t).copy_(t)


from tests.test_gpu_submission_device import hand_rays          # noqa: E402,F401  (the fixture, for the ray casters below)


def _small_batch(name, hand_rays):
    import numpy as np
    from tests import test_gpu_submission_device as sd
    shape, dtype, ids = sd.SHAPES[name]
    grids = [sd._grid(shape, dtype, 100 + b, ids) for b in range(3)]
    gts = [sd._grid(shape, dtype, 200 + b, ids) for b in range(3)]
    origins, counts = sd._origins3(shape)
    st = lambda k, gs: torch.from_numpy(np.stack([g[k] for g in gs])).cuda()
    return dict(sem=st(0, grids), flow=st(1, grids), sem_gt=st(0, gts), flow_gt=st(1, gts), origins=origins.cuda(),
                counts=torch.tensor(counts, dtype=torch.int32).cuda(), rays=hand_rays.cuda())


@pytest.mark.parametrize("name", ["u8_6x5x3", "i64_7x9x20"])
def test_ray_metrics_accumulate_and_submission_rays(name, hand_rays):
    """The ragged B = 3 batch of tests/test_gpu_submission_device.py (origins inside, on faces, outside; unused origin slots)
    through both ray casters.  The state words are a framed zero tensor: a counter that lands one word off shows in a band."""
    from occnet_amd import ext
    from tests import test_gpu_submission_device as sd
    b = _small_batch(name, hand_rays)
    state = torch.zeros(ext.ray_metrics_state_words(16), dtype=torch.int64, device="cuda")

    def metrics(state, sem, flow, sem_gt, flow_gt, origins, counts, rays):
        state = _framed_copy(state)
        rows = ext.ray_metrics_accumulate(state, sem, flow, sem_gt, flow_gt, origins, rays, sd.PC_MIN, sd.VOXEL, 16,
                                          origin_counts=counts, return_rays=True)
        return state, rows
    r = _guard("eval", metrics, [state, b["sem"], b["flow"], b["sem_gt"], b["flow_gt"], b["origins"], b["counts"], b["rays"]],
               "occ_ray_metrics_accumulate")
    assert int(r.framed[0].abs().sum()) > 0

    def rays(sem, flow, origins, counts, rays):
        return ext.submission_rays(sem, flow, origins, rays, sd.PC_MIN, sd.VOXEL, 16, origin_counts=counts)
    for origins in (b["origins"], b["origins"].double()):
        _guard("eval", rays, [b["sem"], b["flow"], origins, b["counts"], b["rays"]], "occ_submission_rays")


@pytest.mark.parametrize("fmts", [(1, 1), (0, 0)])
def test_submission_score_accumulate(fmts):
    from occnet_amd import ext
    from tests import test_gpu_submission_score as ss
    pred, gt = ss._edge_batch(16)
    counts = torch.tensor([len(s[0]) for s in gt], dtype=torch.int32).cuda()
    state = torch.zeros(ext.submission_score_state_words(16), dtype=torch.int64, device="cuda")

    def fn(state, pred, gt, counts):
        state = _framed_copy(state)
        ext.submission_score_accumulate(state, pred, gt, counts, ss.STRIDE, 16)
        return state
    r = _guard("eval", fn, [state, ss._side(ss._as(pred, fmts[0]), ss.STRIDE, fmts[0]),
                            ss._side(ss._as(gt, fmts[1]), ss.STRIDE, fmts[1]), counts], "occ_submission_score_accumulate")
    ss._equal(r.framed, ss._ref(pred, gt, 16, fmts), str(fmts))


@pytest.mark.parametrize("dtype", ["uint8", "int64"])
def test_confusion_accumulate(dtype):
    import numpy as np
    from occnet_amd import ext
    from tests import test_gpu_visibility as tv
    from tests import visibility_ref as vr
    for n in (1, 4097):
        pred, gt, mask = tv._grids(n, dtype, 7 + n % 5, tv.U8_IDS if dtype == "uint8" else tv.I64_IDS)
        for m in (None, mask):
            def fn(state, pred, gt, m):
                state = _framed_copy(state)
                ext.confusion_accumulate(state, pred, gt, mask=m, free_id=16)
                return state
            r = _guard("eval", fn, [tv._state(), tv._dev(pred), tv._dev(gt), None if m is None else tv._dev(m)],
                       "occ_confusion_accumulate")
            assert np.array_equal(r.framed.cpu().numpy().reshape(18, 17), vr.confusion(pred, gt, m, 16))


@pytest.mark.parametrize("name,size", [("5x6x4", (7, 13)), ("4x4x32", (1, 1)), ("3x9x1", (9, 70))])
def test_visibility_views(name, size):
    import numpy as np
    from tests import render_cases as rc
    from tests import test_gpu_visibility as tv
    from tests import visibility_ref as vr
    for dtype in tv.DTYPES:
        sem, cams = tv._scene(name, dtype, size)
        r = _guard("eval", lambda sem, cams: tv._views(sem, cams, size), [sem, cams], "occ_visibility_views")
        assert np.array_equal(r.framed.cpu().numpy(), vr.case_mask(name, dtype, size))


@pytest.mark.parametrize("name,size", [("5x6x4", (7, 13)), ("7x5x17", (1, 1))])
def test_render_views_and_bev(name, size):
    """The renderer with its inputs framed as well (tests/test_gpu_render.py guards the outputs): grids, cameras, frames of
    another size than the raster, both palettes."""
    import numpy as np
    from occnet_amd import ext
    from tests import render_cases as rc
    from tests import test_gpu_render as tr
    c = tr._case(name, np.int64, size)
    d = c.dev
    frames = torch.from_numpy(np.ascontiguousarray(c.frames("other"))).cuda()
    for diff in (False, True):
        def views(sem, gt, cams, frames, pal, cat):
            return ext.render_views(sem, cams, rc.PC_MIN, rc.VOXEL, size, free_id=rc.FREE, sem_gt=gt if diff else None,
                                    frames=frames, palette=pal, cat_palette=cat, far=rc.FAR, tol=rc.TOL, alpha=100, bg_rgb=rc.BG)
        r = _guard("eval", views, [d["sem"], d["gt"], d["cams"], frames, d["pal"], d["cat"]], "occ_render_views")
        want = c.want(diff, c.frames("other"), 100)
        for key in ("label", "rgb"):
            assert np.array_equal(r.framed[key].cpu().numpy(), np.stack([w[key] for w in want])), (diff, key)

        def bev(sem, gt, pal, cat):
            return ext.render_bev(sem, free_id=rc.FREE, sem_gt=gt if diff else None, palette=pal, cat_palette=cat, bg_rgb=rc.BG)
        _guard("eval", bev, [d["sem"], d["gt"], d["pal"], d["cat"]], "occ_render_bev")
