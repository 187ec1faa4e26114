"""The backbone's 3x3 convolution gradients on this library's kernels: ext.conv3x3_wgrad_nhwc (csrc/conv3x3_wgrad_bf16.hip) and
ext.conv3x3_dgrad_nhwc (the forward kernel on the flipped, transposed weight) against float64, and ConvBNActFunction / the
whole backbone under ConvBNActFunction.own_conv3x3_backward."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, H, W, stride, splits)
WGRAD_CASES = [
    (2, 128, 128, 12, 20, 1, None),      # a bottleneck conv2
    (1, 256, 256, 7, 11, 1, None),       # 77 px: less than one pixel tile
    (3, 128, 256, 9, 13, 1, None),       # ragged, batch seams
    (1, 512, 512, 3, 4, 1, None),        # the widest operands, every pixel on a border
    (2, 96, 160, 5, 5, 1, None),         # 32-multiples that are not tile multiples; W < 8: a lane's run spans rows
    (2, 128, 128, 12, 20, 2, None),      # stride 2, even sizes
    (1, 256, 256, 7, 9, 2, None),        # stride 2, odd sizes
    (1, 128, 128, 1, 9, 1, None),        # one row: the ky != 1 taps are exactly zero
    (1, 128, 128, 9, 1, 1, None),        # one column: the kx != 1 taps are exactly zero
    (1, 128, 128, 2, 2, 2, None),        # stride 2 to a single output pixel
    (1, 128, 128, 37, 53, 1, 7),         # 37 rows in seven splits, the last ones short
    (1, 128, 128, 37, 53, 1, 1),         # the same input as one split
]


def _cl(t):
    return t.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _wgrad_problem(N, Cin, Cout, H, W, stride):
    """bf16-valued g and x, the float64 weight gradient over the same values (CPU, torch.nn.grad.conv2d_weight) and its
    magnitude sum |g| (*) |x|, both (Cout, Cin, 3, 3) on the device (computed once per shape)."""
    gen = torch.Generator().manual_seed(1000 * Cin + Cout + 7 * H + W + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.randn(N, Cout, Ho, Wo, generator=gen).to(torch.bfloat16)
    x = torch.randn(N, Cin, H, W, generator=gen).to(torch.bfloat16)
    size = (Cout, Cin, 3, 3)
    want = torch.nn.grad.conv2d_weight(x.double(), size, g.double(), stride=stride, padding=1)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), size, g.double().abs(), stride=stride, padding=1)
    assert want.shape == size
    return _cl(g), _cl(x), want.cuda(), mag.cuda(), N * Ho * Wo


def _poisoned_allocator_blocks(nbytes, device):
    """Fill a block of the size the next workspace request takes with NaN and hand it back to torch's caching allocator."""
    junk = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=device)
    del junk


@pytest.mark.parametrize("N,Cin,Cout,H,W,stride,splits", WGRAD_CASES)
def test_wgrad_matches_float64(N, Cin, Cout, H, W, stride, splits):
    """|got - want| <= B = P * 2^-23 * (|g| (*) |x|) for the fp32 output (the worst-case bound of an fp32 sum of exact
    products in any order, doubled; P = output pixels), 2^-8 |want| + 2 B for the bf16 output (one round-to-nearest on top).
    dw and the workspace hold NaN before the call and dw is finite after it; the C ABI and ext give the same bits, twice."""
    from occnet_amd import _lib, ext
    from occnet_amd._lib import i32, ptr, stream_ptr
    g, x, want, mag, P = _wgrad_problem(N, Cin, Cout, H, W, stride)
    B = P * 2.0 ** -23 * mag
    lib = _lib.lib()
    sp = 0 if splits is None else splits
    nbytes = int(lib.occ_conv3x3_wgrad_workspace_bytes(i32(N), i32(H), i32(W), i32(Cin), i32(Cout), i32(stride), i32(sp)))
    assert nbytes > 0 and nbytes % (9 * Cout * Cin * 4) == 0
    if splits is not None:
        assert nbytes == splits * 9 * Cout * Cin * 4
    for dtype, bound in ((torch.float32, B), (torch.bfloat16, 2.0 ** -8 * want.abs() + 2 * B)):
        # the C ABI with a NaN-filled output and a NaN-filled workspace: overwritten, no stale partial read
        dw = torch.full((Cout, 3, 3, Cin), float('nan'), dtype=dtype, device='cuda')
        ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device='cuda')
        rc = lib.occ_conv3x3_wgrad_nhwc_bf16(ptr(g), ptr(x), ptr(dw), i32(1 if dtype == torch.bfloat16 else 0), ptr(ws), i32(N),
                                             i32(H), i32(W), i32(Cin), i32(Cout), i32(stride), i32(sp), stream_ptr(g.device))
        _lib.check(rc, "conv3x3_wgrad")
        assert bool(torch.isfinite(dw).all())
        dw = dw.permute(0, 3, 1, 2)                                      # [Cout][3][3][Cin] in memory -> (Cout, Cin, 3, 3)
        err = (dw.double() - want).abs()
        print(f"wgrad {dtype}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
        if H == 1:                                                       # no input row above or below: exact zeros, not small numbers
            assert not bool(dw[:, :, 0, :].any()) and not bool(dw[:, :, 2, :].any())
        if W == 1:
            assert not bool(dw[:, :, :, 0].any()) and not bool(dw[:, :, :, 2].any())
        # the Python entry point: the same bits, twice (its workspace comes from the caching allocator, poisoned here)
        _poisoned_allocator_blocks(nbytes, g.device)
        got = ext.conv3x3_wgrad_nhwc(g, x, stride=stride, out_dtype=dtype, splits=splits)
        _poisoned_allocator_blocks(nbytes, g.device)
        again = ext.conv3x3_wgrad_nhwc(g, x, stride=stride, out_dtype=dtype, splits=splits)
        assert got.shape == (Cout, Cin, 3, 3) and got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, again) and torch.equal(got, dw)


def test_wgrad_split_count_changes_only_the_summation_order():
    """37 rows of 53 pixels as one range and as seven: both inside the bound above, and not required to be the same bits."""
    from occnet_amd import ext
    g, x, want, mag, P = _wgrad_problem(1, 128, 128, 37, 53, 1)
    one = ext.conv3x3_wgrad_nhwc(g, x, splits=1).double()
    seven = ext.conv3x3_wgrad_nhwc(g, x, splits=7).double()
    B = P * 2.0 ** -23 * mag
    assert bool(((one - seven).abs() <= 2 * B).all())


@pytest.mark.parametrize("W,stride", [(11, 1), (10, 2)])
def test_wgrad_non_finite_x_stays_in_the_taps_that_read_it(W, stride):
    """x = Inf in the last column: the kx = 0 tap reads columns xo * stride - 1 <= W - 2 only, so it has the bits of the
    same call with that column zeroed (a pixel past the row's end, whose kx = 0 tap would sit on column W - 1, takes no
    tap); x = Inf in the first row leaves the ky = 2 tap alone in the same way at stride 1."""
    from occnet_amd import ext
    gen = torch.Generator().manual_seed(W)
    N, C, H = 1, 128, 5
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = _cl(torch.randn(N, C, Ho, Wo, generator=gen))
    x = torch.randn(N, C, H, W, generator=gen)
    clean, hot = x.clone(), x.clone()
    clean[:, :, :, W - 1] = 0.0
    hot[:, :, :, W - 1] = float('inf')
    want = ext.conv3x3_wgrad_nhwc(g, _cl(clean), stride=stride)
    got = ext.conv3x3_wgrad_nhwc(g, _cl(hot), stride=stride)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got[:, :, :, 0], want[:, :, :, 0])
    assert not bool(torch.isfinite(got[:, :, 1, 2]).all())             # the taps that do read the column see it
    if stride == 1:
        clean, hot = x.clone(), x.clone()
        clean[:, :, 0, :] = 0.0
        hot[:, :, 0, :] = float('inf')
        want = ext.conv3x3_wgrad_nhwc(g, _cl(clean), stride=1)
        got = ext.conv3x3_wgrad_nhwc(g, _cl(hot), stride=1)
        assert torch.equal(got[:, :, 2, :], want[:, :, 2, :])


def _hand_built_dgrad_weight(w):
    """Wd[i][o][ky][kx] = W[o][i][2 - ky][2 - kx], tap by tap."""
    O, I = w.shape[:2]
    wd = torch.empty((I, O, 3, 3), dtype=w.dtype, device=w.device)
    for ky in range(3):
        for kx in range(3):
            wd[:, :, ky, kx] = w[:, :, 2 - ky, 2 - kx].t()
    return wd


# every stride-1 shape of WGRAD_CASES the forward kernel takes as a data gradient (Cin % 128 == 0), once
DGRAD_CASES = list(dict.fromkeys(c[:5] for c in WGRAD_CASES if c[5] == 1 and c[1] % 128 == 0))


@pytest.mark.parametrize("N,Cin,Cout,H,W", DGRAD_CASES)
def test_dgrad_helper_matches_float64(N, Cin, Cout, H, W):
    """gx = g (*) Wd through the forward kernel: |got - want| <= 2^-8 |want| + 2 (9 Cout) 2^-23 (|g| (*) |W|); two calls give
    the same bits, which are those of ext.conv3x3_nhwc on the hand-built Wd."""
    from occnet_amd import ext
    g, _, _, _, P = _wgrad_problem(N, Cin, Cout, H, W, 1)
    gen = torch.Generator().manual_seed(Cin + Cout)
    w16 = (torch.randn(Cout, Cin, 3, 3, generator=gen) * (9 * Cout) ** -0.5).cuda().to(torch.bfloat16)
    got = ext.conv3x3_dgrad_nhwc(g, w16)
    assert got.shape == (N, Cin, H, W) and got.dtype == torch.bfloat16 and got.is_contiguous(memory_format=torch.channels_last)
    gd, wd = g.double().cpu(), w16.double().cpu()
    want = torch.nn.grad.conv2d_input((N, Cin, H, W), wd, gd, stride=1, padding=1).cuda()
    mag = torch.nn.grad.conv2d_input((N, Cin, H, W), wd.abs(), gd.abs(), stride=1, padding=1).cuda()
    bound = 2.0 ** -8 * want.abs() + 2 * (9 * Cout) * 2.0 ** -23 * mag
    err = (got.double() - want).abs()
    print(f"dgrad: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got, ext.conv3x3_dgrad_nhwc(g, w16))
    packed = ext.conv3x3_pack_weight(_hand_built_dgrad_weight(w16).float().contiguous())
    direct = ext.conv3x3_nhwc(g, packed, torch.zeros(Cin, device='cuda'), Cin)
    assert torch.equal(got, direct)


def test_device_tensors_of_the_wrong_dtype_or_layout_are_refused():
    """fp32 and NCHW tensors on the device (the host test can only offer CPU tensors, which the device check alone refuses)."""
    from occnet_amd import ext
    from occnet_amd.ext import OccAmdUnsupported
    g = _cl(torch.randn(1, 64, 4, 6))
    x = _cl(torch.randn(1, 128, 4, 6))
    w = torch.randn(64, 128, 3, 3, device='cuda').to(torch.bfloat16)
    assert ext.conv3x3_wgrad_nhwc(g, x).shape == (64, 128, 3, 3) and ext.conv3x3_dgrad_nhwc(g, w).shape == (1, 128, 4, 6)
    nchw = lambda t: t.contiguous(memory_format=torch.contiguous_format)
    for bad_g, bad_x in ((g.float(), x), (g, x.float()), (nchw(g), x), (g, nchw(x))):
        assert not (bad_g.is_contiguous(memory_format=torch.channels_last) and bad_g.dtype == torch.bfloat16
                    and bad_x.is_contiguous(memory_format=torch.channels_last) and bad_x.dtype == torch.bfloat16)
        with pytest.raises(OccAmdUnsupported):
            ext.conv3x3_wgrad_nhwc(bad_g, bad_x)
    for bad_g in (g.float(), nchw(g)):
        with pytest.raises(OccAmdUnsupported):
            ext.conv3x3_dgrad_nhwc(bad_g, w)
    with pytest.raises(OccAmdUnsupported):
        ext.conv3x3_wgrad_nhwc(g, x, out_dtype=torch.float16)
    with pytest.raises(OccAmdUnsupported):
        ext.conv3x3_wgrad_nhwc(g, x, stride=3)
    with pytest.raises(OccAmdUnsupported):                               # the forward kernel has no Cout % 128 != 0 shape
        ext.conv3x3_dgrad_nhwc(g, torch.randn(64, 96, 3, 3, device='cuda').to(torch.bfloat16))
    with pytest.raises(OccAmdUnsupported):                               # a 1x1 weight
        ext.conv3x3_dgrad_nhwc(g, torch.randn(64, 128, 1, 1, device='cuda').to(torch.bfloat16))


# ---- the node under the switch ------------------------------------------------------------------------------------------

def _node_setup(cin, cout, k, stride, bn, res):
    g = torch.Generator().manual_seed(cin + cout + k)
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=not bn).cuda()
    norm = None
    if bn:
        norm = torch.nn.BatchNorm2d(cout).cuda().eval()
        with torch.no_grad():
            norm.running_mean.copy_(torch.randn(cout, generator=g).cuda() * 0.1)
            norm.running_var.copy_(torch.rand(cout, generator=g).cuda() * 0.5 + 0.75)
            norm.weight.copy_(torch.rand(cout, generator=g).cuda() * 0.5 + 0.75)
            norm.bias.copy_(torch.randn(cout, generator=g).cuda() * 0.1)
    N, H, W = 2, 12, 20
    x0 = _cl(torch.randn(N, cin, H, W, generator=g))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r0 = _cl(torch.randn(N, cout, Ho, Wo, generator=g)) if res else None
    gy = _cl(torch.randn(N, cout, Ho, Wo, generator=g))
    params = [conv.weight] + ([conv.bias] if conv.bias is not None else []) + ([norm.weight, norm.bias] if bn else [])
    return conv, norm, x0, r0, gy, params


def _run_node(mode, conv, norm, x0, r0, gy, params, relu, own, x_grad=True, train=None):
    """One forward + backward of the node (`fused`), the bf16 autocast chain (`chain`) or the fp32 chain (`fp32`) ->
    [y, dx, (dres), dparams ...] as float32; `train` = the indices of `params` that require a gradient (None = all)."""
    from occnet_amd.plugin.backbone import ConvBNActFunction, conv_bn_act, conv_bn_folded
    bn = norm is not None
    x = (x0.float() if mode == "fp32" else x0.clone(memory_format=torch.channels_last)).requires_grad_(x_grad)
    r = None if r0 is None else (r0.float() if mode == "fp32" else r0.clone(memory_format=torch.channels_last)).requires_grad_(True)
    for i, p in enumerate(params):
        p.grad = None
        p.requires_grad_(train is None or i in train)
    was = ConvBNActFunction.own_conv3x3_backward
    ConvBNActFunction.own_conv3x3_backward = own
    try:
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=mode != "fp32"):
            if mode == "fused":
                y = conv_bn_act(x, conv, norm, relu=relu, residual=r)
            else:
                y = conv_bn_folded(x, conv, norm) if bn else conv(x)
                if r is not None:
                    y = y + r
                if relu:
                    y = torch.relu(y)
        y.backward(gy.float() if mode == "fp32" else gy)
    finally:
        ConvBNActFunction.own_conv3x3_backward = was
        for p in params:
            p.requires_grad_(True)
    grads = [None if x.grad is None else x.grad.float()] + ([] if r is None else [r.grad.float()])
    return [y.detach().float()] + grads + [None if p.grad is None else p.grad.float().clone() for p in params], y.detach()


@pytest.fixture
def deterministic_convolutions():
    """MIOpen's deterministic mode, as in test_gpu_autograd_contract: in its default mode two identical calls of
    aten.convolution_backward need not give the same bits, so a bit comparison across calls that reach MIOpen (the stride-2
    data gradient, the nodes that pass through) says something about this repository's code only with that mode on."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


# (cin, cout, stride, bn, res, relu)
NODE_CASES = [
    (128, 128, 1, True, False, True),      # bottleneck conv2
    (256, 256, 2, True, False, True),      # the first block of a stage: stride 2, ATen data gradient
    (256, 256, 1, False, False, False),    # FPN output: bias, no norm, no ReLU
    (96, 128, 1, True, False, True),       # '3x3' route with Cin % 128 != 0: own weight gradient, ATen data gradient
]


@pytest.mark.parametrize("cin,cout,stride,bn,res,relu", NODE_CASES)
def test_node_with_own_backward_matches_the_chains(cin, cout, stride, bn, res, relu, monkeypatch):
    """test_conv_bn_act_function_matches_the_autocast_chain's comparison with the switch on (same bounds); the forward is
    untouched (same bits on and off); the difference to MIOpen's gradients is printed, not asserted.  Under the switch the
    own weight gradient runs once, and the own data gradient exactly where the forward kernel has the shape (stride 1 and
    Cin % 128 == 0)."""
    from occnet_amd import ext
    from tests.grad_bounds import conv_bn_act_within_bound
    calls = []
    for name in ("conv3x3_wgrad_nhwc", "conv3x3_dgrad_nhwc"):
        real = getattr(ext, name)
        monkeypatch.setattr(ext, name, lambda *a, _real=real, _name=name, **kw: (calls.append(_name), _real(*a, **kw))[1])
    setup = _node_setup(cin, cout, 3, stride, bn, res)
    out = {}
    out["own"], y_on = _run_node("fused", *setup, relu, True)
    assert calls == ["conv3x3_wgrad_nhwc"] + (["conv3x3_dgrad_nhwc"] if stride == 1 and cin % 128 == 0 else [])
    del calls[:]
    out["aten"], y_off = _run_node("fused", *setup, relu, False)
    out["chain"], _ = _run_node("chain", *setup, relu, False)
    out["fp32"], _ = _run_node("fp32", *setup, relu, False)
    assert not calls                                                     # nothing of it with the switch off
    assert torch.equal(y_on, y_off)
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-12))
    for i, (f, m, c, ref) in enumerate(zip(out["own"], out["aten"], out["chain"], out["fp32"])):
        ef, ec = rel(f, ref), rel(c, ref)
        print(f"tensor {i} {tuple(ref.shape)}: own vs fp32 {ef:.3e}, chain vs fp32 {ec:.3e}, own vs MIOpen {rel(f, m):.3e}")
        assert f.shape == ref.shape and conv_bn_act_within_bound(ef, ec), (i, tuple(ref.shape), ef, ec)


@pytest.mark.parametrize("cin,cout,stride,bn,res,relu", NODE_CASES)
def test_node_partial_masks_give_the_full_mask_bits(cin, cout, stride, bn, res, relu, deterministic_convolutions):
    """x only / weight only / gamma only / beta only with the switch on: the same bits as under the full mask (the stride-2
    data gradient is MIOpen's under either mask)."""
    setup = _node_setup(cin, cout, 3, stride, bn, res)
    params = setup[5]
    full, _ = _run_node("fused", *setup, relu, True)
    first = 2 + (1 if res else 0)                     # index of the first parameter gradient in the result list
    got, _ = _run_node("fused", *setup, relu, True, x_grad=True, train=())
    assert torch.equal(got[1], full[1]) and all(t is None for t in got[first:])
    for i in range(len(params)):                      # weight, then (bias) or (gamma, beta)
        got, _ = _run_node("fused", *setup, relu, True, x_grad=False, train=(i,))
        assert got[1] is None
        assert all((t is None) == (j != i) for j, t in enumerate(got[first:]))
        assert torch.equal(got[first + i], full[first + i]), i


@pytest.mark.parametrize("cin,cout,k", [(256, 128, 1), (48, 64, 3)])
def test_other_nodes_pass_through(cin, cout, k, deterministic_convolutions, monkeypatch):
    """A 1x1 node and a 3x3 node without the '3x3' route (48 -> 64 channels): neither new entry point is called, and the
    gradients are bit-identical with the switch on and off."""
    from occnet_amd import ext
    calls = []
    for name in ("conv3x3_wgrad_nhwc", "conv3x3_dgrad_nhwc"):
        real = getattr(ext, name)
        monkeypatch.setattr(ext, name, lambda *a, _real=real, _name=name, **kw: (calls.append(_name), _real(*a, **kw))[1])
    setup = _node_setup(cin, cout, k, 1, True, False)
    on, _ = _run_node("fused", *setup, True, True)
    off, _ = _run_node("fused", *setup, True, False)
    assert not calls
    assert len(on) == len(off) and all(torch.equal(a, b) for a, b in zip(on, off))


def test_whole_backbone_with_own_3x3_backward_matches_the_module_graph(monkeypatch):
    """ResNet-50 (norm_eval, frozen_stages=1) + FPN under bf16 autocast: fused nodes with the own 3x3 backward against the
    module graph; the bounds of test_training_backbone_fused_nodes_match_the_autocast_modules.  The ten stride-1 conv2 of
    layers 2-4 and the three stride-1 FPN outputs take both own gradients; the four stride-2 convolutions
    (layer{2,3,4}.0.conv2, the FPN's extra convolution) take the own weight gradient only where the node routes them."""
    from occnet_amd import ext
    from occnet_amd.plugin.backbone import FPN, Bottleneck, ConvBNActFunction
    from tests.grad_bounds import BACKBONE_FUSED_GRAD_MEDIAN_REL, BACKBONE_FUSED_GRAD_WORST_REL, BACKBONE_FUSED_OUT_REL
    from tests.test_gpu_backbone import _train_backbone
    bb, g = _train_backbone()
    neck = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output', num_outs=4,
               relu_before_extra_convs=True).cuda().train()
    x = (torch.randn(2, 3, 96, 160, generator=g) * 50.0).cuda()
    res = {}
    calls = {"conv3x3_wgrad_nhwc": [], "conv3x3_dgrad_nhwc": []}
    state = {"own": None}
    for name in calls:
        real = getattr(ext, name)
        monkeypatch.setattr(ext, name, lambda *a, _real=real, _name=name, **kw: (calls[_name].append(state["own"]),
                                                                                  _real(*a, **kw))[1])
    was3, was1 = ConvBNActFunction.own_conv3x3_backward, ConvBNActFunction.own_conv1x1_backward
    for own in (True, False):
        Bottleneck.fused_train_nodes = own
        ConvBNActFunction.own_conv3x3_backward = own
        state["own"] = own
        try:
            bb.zero_grad(set_to_none=True)
            neck.zero_grad(set_to_none=True)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                outs = neck(bb(x))
            assert len(outs) == 4
            sum((o.float() ** 2).mean() for o in outs).backward()
            grads = {n: p.grad.detach().float().clone() for m, pre in ((bb, 'bb.'), (neck, 'neck.'))
                     for n, p in ((pre + k, v) for k, v in m.named_parameters()) if p.grad is not None}
            res[own] = ([o.detach().float() for o in outs], grads)
        finally:
            Bottleneck.fused_train_nodes = True
            ConvBNActFunction.own_conv3x3_backward = was3
    assert ConvBNActFunction.own_conv1x1_backward == was1                 # the 1x1 switch is left as found
    nw, nd = len(calls["conv3x3_wgrad_nhwc"]), len(calls["conv3x3_dgrad_nhwc"])
    print(f"own 3x3 backward, whole backbone: {nw} weight gradients, {nd} data gradients")
    assert all(calls["conv3x3_wgrad_nhwc"]) and all(calls["conv3x3_dgrad_nhwc"])      # only under the switch
    assert nw == 17 and nd == 13                  # stride 2 is routed to the own weight gradient (EXPERIMENTS.md 8o)
    assert res[True][1].keys() == res[False][1].keys() and len(res[True][1]) > 120
    for a, b in zip(res[True][0], res[False][0]):
        assert float((a - b).abs().max() / b.abs().max()) < BACKBONE_FUSED_OUT_REL
    rel = sorted(float((res[True][1][n] - gb).abs().max() / (gb.abs().max() + 1e-12)) for n, gb in res[False][1].items())
    print(f"own 3x3 backward, whole backbone: relative gradient difference worst {rel[-1]:.2e}, median {rel[len(rel) // 2]:.2e}")
    assert rel[len(rel) // 2] < BACKBONE_FUSED_GRAD_MEDIAN_REL and rel[-1] < BACKBONE_FUSED_GRAD_WORST_REL
