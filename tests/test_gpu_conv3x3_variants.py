"""-m gpu: every tile of the 3x3 implicit GEMM (forced through occ_conv3x3_nhwc_bf16_variant) on ragged shapes, and the
launcher's own choice on the 17 convolutions of one base-config step, against torch's conv2d with bf16-rounded weights;
repeat calls bit-identical; the amax words equal the largest pattern stored."""
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = {1: (12, 13, 14, 16, 18, 22, 23, 24), 2: (12, 13, 22)}      # 10 * channel blocks of 128 + row tiles per wave

# ResNet-50 layer2..4 conv2 and the FPN output / extra-level convolutions of the base config (6 cameras, 928 x 1600):
# (Cin, Cout, H, W, stride, launches per step)
BASE_SHAPES = [(128, 128, 232, 400, 2, 1), (128, 128, 116, 200, 1, 3), (256, 256, 116, 200, 2, 1),
               (256, 256, 58, 100, 1, 6), (512, 512, 58, 100, 2, 1), (512, 512, 29, 50, 1, 2),
               (256, 256, 116, 200, 1, 1), (256, 256, 29, 50, 1, 1),
               (256, 256, 29, 50, 2, 1)]


def _case(N, C, Cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, H, W, generator=g) * 2).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    return x, w, b


def _check(got, x, w, b, relu, stride):
    want = torch.nn.functional.conv2d(x.float(), w.to(torch.bfloat16).float(), b, padding=1, stride=stride)
    if relu:
        want = want.relu()
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    d = float((got.float() - want).abs().max())
    scale = float(want.abs().max())
    assert d <= scale * 2 ** -8 + 1e-5, (d, scale)          # one bf16 rounding of the f32-accumulated result
    return d


def _pattern_max(t):
    return int((t.contiguous().view(torch.int16).to(torch.int32) & 0x7fff).max())


@pytest.mark.parametrize("N,C,Cout,H,W,stride", [
    (2, 64, 128, 13, 37, 1), (1, 96, 256, 29, 21, 1), (3, 32, 128, 5, 3, 1), (1, 128, 128, 1, 1, 1),
    (2, 64, 128, 27, 35, 2), (1, 96, 256, 11, 50, 2), (2, 32, 128, 2, 3, 2), (1, 64, 128, 1, 1, 2)])
@pytest.mark.parametrize("relu", [True, False])
def test_every_variant_matches_torch(N, C, Cout, H, W, stride, relu):
    from occnet_amd import ext
    x, w, b = _case(N, C, Cout, H, W, seed=N * 7919 + C * 31 + H * W + stride)
    wp = ext.conv3x3_pack_weight(w)
    for v in VARIANTS[stride] + (0,):
        if Cout % (128 * (v // 10 or 1)):
            continue
        got = ext.conv3x3_nhwc(x, wp, b, Cout, relu=relu, stride=stride, variant=v)
        _check(got, x, w, b, relu, stride)
        # amax on: the same output, the words hold the largest sign-stripped pattern stored
        words = ext.new_absmax_words(x.device)
        got_a = ext.conv3x3_nhwc(x, wp, b, Cout, relu=relu, stride=stride, amax=words, variant=v)
        assert torch.equal(got_a, got), v
        assert int(words.max()) == _pattern_max(got) and int(words.min()) >= 0, v


@pytest.mark.parametrize("stride", [1, 2])
def test_unsupported_variant_is_an_error(stride):
    from occnet_amd import ext
    x, w, b = _case(1, 32, 128, 6, 6, seed=3)
    with pytest.raises(ext.OccAmdUnsupported):
        ext.conv3x3_nhwc(x, ext.conv3x3_pack_weight(w), b, 128, stride=stride, variant=15)
    with pytest.raises(ext.OccAmdUnsupported):                    # 256-channel blocks on 128 channels
        ext.conv3x3_nhwc(x, ext.conv3x3_pack_weight(w), b, 128, stride=stride, variant=22)


@pytest.mark.parametrize("C,Cout,H,W,stride,n", BASE_SHAPES)
def test_base_config_shapes_default_dispatch(C, Cout, H, W, stride, n):
    """Full-size launches through the default entry points: torch reference, two calls bit-identical, the amax entry
    stores the same output and its words equal the largest pattern stored."""
    from occnet_amd import ext
    x, w, b = _case(6, C, Cout, H, W, seed=C + H * W + stride)
    wp = ext.conv3x3_pack_weight(w)
    got = ext.conv3x3_nhwc(x, wp, b, Cout, relu=True, stride=stride)
    d = _check(got, x, w, b, True, stride)
    print(f"conv3x3 {C}->{Cout} {H}x{W} s{stride} (x{n} per step): max diff {d:.3e}")
    assert torch.equal(ext.conv3x3_nhwc(x, wp, b, Cout, relu=True, stride=stride), got)
    words = ext.new_absmax_words(x.device)
    got_a = ext.conv3x3_nhwc(x, wp, b, Cout, relu=True, stride=stride, amax=words)
    assert torch.equal(got_a, got)
    assert int(words.max()) == _pattern_max(got)
