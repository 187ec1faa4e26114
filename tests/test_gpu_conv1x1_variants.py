"""-m gpu: the two kernels of the backbone's 1x1 convolution (tiled / activation-resident, forced through
occ_conv1x1_nhwc_bf16_variant) and the launcher's own choice on ragged shapes and on the 13 shapes of one base-config
step, against torch's conv2d in f32 on the bf16-rounded operands; repeat calls bit-identical; the inference plan with
the launcher's choice against the same plan forced onto the tiled kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, stride): M below one 128-row tile; M = 286 (not a multiple of the tile, the second tile spans both images);
# stride 2 on odd sizes (M = 504); stride 2, three images, M = 120
GEOMETRIES = [(1, 5, 7, 1), (2, 13, 11, 1), (2, 27, 35, 2), (3, 9, 15, 2)]

# one base-config step (6 cameras, 928 x 1600): (Cin, Cout, H, W, stride, residual: 0 none / 1 plain / 2 upsampled, relu)
BASE_SHAPES = [(256, 128, 232, 400, 1, 0, 1), (512, 128, 116, 200, 1, 0, 1), (128, 512, 116, 200, 1, 1, 1),
               (256, 512, 232, 400, 2, 0, 0), (512, 256, 116, 200, 1, 0, 1), (512, 256, 116, 200, 1, 2, 0),
               (256, 1024, 58, 100, 1, 1, 1), (512, 1024, 116, 200, 2, 0, 0), (512, 2048, 29, 50, 1, 1, 1),
               (1024, 256, 58, 100, 1, 0, 1), (1024, 256, 58, 100, 1, 2, 0), (1024, 512, 58, 100, 1, 0, 1),
               (2048, 512, 29, 50, 1, 0, 1), (1024, 2048, 58, 100, 2, 0, 0), (2048, 256, 29, 50, 1, 0, 0)]


def _cl(t):
    return t.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _case(N, Cin, Cout, H, W, stride, res, seed):
    g = torch.Generator().manual_seed(seed)
    x = _cl(torch.randn(N, Cin, H, W, generator=g))
    w = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).cuda().to(torch.bfloat16)
    b = torch.randn(Cout, generator=g).cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = None
    if res == 1:
        r = _cl(torch.randn(N, Cout, Ho, Wo, generator=g))
    elif res == 2:
        r = _cl(torch.randn(N, Cout, Ho // 2, Wo // 2, generator=g))
    return x, w, b, r


def _want(x, w, b, r, relu, stride, up):
    F = torch.nn.functional
    want = F.conv2d(x.float(), w.float().view(*w.shape, 1, 1), b, stride=stride)
    if r is not None:
        want = want + (F.interpolate(r.float(), size=want.shape[-2:]) if up else r.float())
    return want.relu() if relu else want


def _check(got, want):
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    d, scale = float((got.float() - want).abs().max()), float(want.abs().max())
    assert d <= scale * 2 ** -8 + 1e-6, (d, scale)          # one bf16 rounding of the f32-accumulated result
    return d


def _variants(Cin, Cout):
    np_ = Cout // (256 if Cout % 256 == 0 else 128)          # column passes of the resident kernel
    vs = [0, 1, 2, 24, 124, 100 * np_ + 24]                  # 124: one block walks every pass; the last: one pass per block
    if Cin == 512:
        vs += [22, 122]
    return vs


@pytest.mark.parametrize("Cout", [128, 256, 512, 1024])
@pytest.mark.parametrize("Cin", [128, 256, 512])
def test_every_variant_matches_torch(Cin, Cout):
    from occnet_amd import ext
    for gi, (N, H, W, stride) in enumerate(GEOMETRIES):
        for res in (0, 1):
            x, w, b, r = _case(N, Cin, Cout, H, W, stride, res, seed=Cin * 7 + Cout + gi)
            wp = ext.conv1x1_pack_weight(w)
            for relu in (True, False):
                want = _want(x, w, b, r, relu, stride, False)
                for v in _variants(Cin, Cout):
                    got = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=relu, stride=stride, variant=v)
                    _check(got, want)
                    again = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=relu, stride=stride, variant=v)
                    assert torch.equal(got, again), (v, N, H, W, stride, res, relu)


@pytest.mark.parametrize("Cin,Cout", [(128, 256), (256, 128), (256, 512), (512, 256), (512, 128), (512, 1024)])
def test_every_variant_matches_torch_with_upsampled_residual(Cin, Cout):
    """The FPN top-down step: the residual is the map of half the resolution, added nearest-upsampled x2."""
    from occnet_amd import ext
    for gi, (N, H, W, stride) in enumerate([(2, 12, 22, 1), (1, 4, 6, 1), (2, 27, 35, 2), (3, 18, 10, 1)]):
        x, w, b, r = _case(N, Cin, Cout, H, W, stride, 2, seed=Cin * 5 + Cout + gi)
        wp = ext.conv1x1_pack_weight(w)
        for relu in (True, False):
            want = _want(x, w, b, r, relu, stride, True)
            for v in _variants(Cin, Cout):
                got = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=relu, stride=stride, residual_upsample2=True, variant=v)
                _check(got, want)
                again = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=relu, stride=stride, residual_upsample2=True,
                                         variant=v)
                assert torch.equal(got, again), (v, N, H, W, stride, relu)


def test_resident_grid_does_not_change_the_result():
    """The column split and the dealing of the blocks change which block computes what, never a value."""
    from occnet_amd import ext
    x, w, b, r = _case(2, 256, 1024, 37, 43, 1, 1, seed=11)          # M = 3182: 25 row tiles, the last group of 8 padded
    wp = ext.conv1x1_pack_weight(w)
    ref = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=True, variant=124)
    _check(ref, _want(x, w, b, r, True, 1, False))
    for v in (2, 24, 224, 424):
        assert torch.equal(ext.conv1x1_nhwc(x, wp, b, residual=r, relu=True, variant=v), ref), v
    x, w, b, r = _case(3, 512, 2048, 19, 23, 2, 1, seed=12)          # stride 2: M = 360
    wp = ext.conv1x1_pack_weight(w)
    ref = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=False, stride=2, variant=124)
    _check(ref, _want(x, w, b, r, False, 2, False))
    for v in (2, 224, 824):
        assert torch.equal(ext.conv1x1_nhwc(x, wp, b, residual=r, relu=False, stride=2, variant=v), ref), v
    ref = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=False, stride=2, variant=122)
    for v in (22, 422, 822):
        assert torch.equal(ext.conv1x1_nhwc(x, wp, b, residual=r, relu=False, stride=2, variant=v), ref), v


def test_unsupported_variant_is_an_error():
    from occnet_amd import ext
    x, w, b, r = _case(1, 1024, 256, 6, 6, 1, 0, seed=3)
    with pytest.raises(ext.OccAmdUnsupported):                        # K = 1024 has the tiled kernel only
        ext.conv1x1_nhwc(x, ext.conv1x1_pack_weight(w), b, variant=2)
    x, w, b, r = _case(1, 256, 256, 6, 6, 1, 0, seed=4)
    for v in (22, 3, 324):                        # the 64-row tile is K = 512's; no such kernel; 3 blocks for 1 pass
        with pytest.raises(ext.OccAmdUnsupported):
            ext.conv1x1_nhwc(x, ext.conv1x1_pack_weight(w), b, variant=v)


@pytest.mark.parametrize("Cin,Cout,H,W,stride,res,relu", BASE_SHAPES)
def test_base_config_shapes_default_dispatch(Cin, Cout, H, W, stride, res, relu):
    """Full-size launches through the default entry point: torch reference, two calls bit-identical."""
    from occnet_amd import ext
    x, w, b, r = _case(6, Cin, Cout, H, W, stride, res, seed=Cin + Cout + H)
    wp = ext.conv1x1_pack_weight(w)
    got = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=bool(relu), stride=stride, residual_upsample2=res == 2)
    d = _check(got, _want(x, w, b, r, bool(relu), stride, res == 2))
    print(f"conv1x1 {Cin}->{Cout} {H}x{W} s{stride} res{res}: max diff {d:.3e}")
    again = ext.conv1x1_nhwc(x, wp, b, residual=r, relu=bool(relu), stride=stride, residual_upsample2=res == 2)
    assert torch.equal(again, got)


def test_plan_with_resident_kernels_matches_plan_on_tiled_kernels(monkeypatch):
    """FusedInferenceBackbone as it is (the launcher's choice) against the same plan with every 1x1 convolution forced
    onto the tiled kernel.  The image is large enough that layer2 and layer3 take the resident kernel: for their
    shapes variant 2 exists and the default launch returns variant 2's bits."""
    from occnet_amd import ext
    from occnet_amd.plugin.backbone import FPN, FusedInferenceBackbone, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_eval=True).eval()
    bb.init_weights()
    nk = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    bb, nk = bb.cuda(), nk.cuda()
    x = torch.randn(2, 3, 256, 384).cuda() * 50.0
    real = ext.conv1x1_nhwc
    seen = []

    def recording(x, weight_frag, bias, residual=None, relu=False, stride=1, residual_upsample2=False):
        out = real(x, weight_frag, bias, residual=residual, relu=relu, stride=stride,
                   residual_upsample2=residual_upsample2)
        Cin, M = x.shape[1], out.shape[0] * out.shape[2] * out.shape[3]
        # the launcher's rule: K <= 512 and at least a few row tiles
        if Cin in (128, 256, 512) and M >= 512:
            forced = real(x, weight_frag, bias, residual=residual, relu=relu, stride=stride,
                          residual_upsample2=residual_upsample2, variant=2)          # exists: no error
            assert torch.equal(out, forced)
            seen.append((Cin, bias.numel(), M))
        return out

    def tiled(x, weight_frag, bias, residual=None, relu=False, stride=1, residual_upsample2=False):
        return real(x, weight_frag, bias, residual=residual, relu=relu, stride=stride,
                    residual_upsample2=residual_upsample2, variant=1)

    with torch.no_grad():
        plan = FusedInferenceBackbone(bb, nk)
        monkeypatch.setattr(ext, 'conv1x1_nhwc', recording)
        a = plan(x)
        monkeypatch.setattr(ext, 'conv1x1_nhwc', tiled)
        b = plan(x)
    # layer2: 128 -> 512 (conv3), 512 -> 128 (conv1), 256 -> 512 (downsample); layer3: 512 -> 256 (first conv1),
    # 256 -> 1024 (conv3), 512 -> 1024 (downsample)
    for shape in ((128, 512), (512, 128), (256, 512), (512, 256), (256, 1024), (512, 1024)):
        assert any(s[:2] == shape for s in seen), (shape, seen)
    for u, v in zip(a, b):
        rel = float((u.float() - v.float()).abs().max() / v.float().abs().max())
        print(f"level {tuple(u.shape)}: resident vs tiled max rel diff {rel:.3e}")
        assert rel < 0.03
