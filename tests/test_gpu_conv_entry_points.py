"""-m gpu: ext.conv3x3_nhwc and ext.conv1x1_nhwc make one call to their `_variant` entry point whatever the arguments; the
launcher's choice (variant None / 0), with and without amax words, gives the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_default_amax_and_variant0_agree_bit_for_bit(stride):
    """The words are atomic maxima spread over 8 slots: their maximum is the value feature_absmax_words replicates."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(11 + stride)
    x = (torch.randn(1, 32, 5, 7, generator=g) * 2).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(128, 32, 3, 3, generator=g) / (9 * 32) ** 0.5).cuda()
    b = torch.randn(128, generator=g).cuda()
    wp = ext.conv3x3_pack_weight(w)
    plain = ext.conv3x3_nhwc(x, wp, b, 128, relu=True, stride=stride)
    want = torch.nn.functional.conv2d(x.float(), w.to(torch.bfloat16).float(), b, padding=1, stride=stride).relu()
    assert plain.shape == want.shape and plain.is_contiguous(memory_format=torch.channels_last)
    assert float((plain.float() - want).abs().max()) <= float(want.abs().max()) * 2 ** -8 + 1e-5
    words = ext.new_absmax_words(x.device)
    with_amax = ext.conv3x3_nhwc(x, wp, b, 128, relu=True, stride=stride, amax=words)
    forced0 = ext.conv3x3_nhwc(x, wp, b, 128, relu=True, stride=stride, variant=0)
    words0 = ext.new_absmax_words(x.device)
    forced0_amax = ext.conv3x3_nhwc(x, wp, b, 128, relu=True, stride=stride, amax=words0, variant=0)
    assert torch.equal(with_amax, plain) and torch.equal(forced0, plain) and torch.equal(forced0_amax, plain)
    ref = ext.feature_absmax_words(plain)
    assert int(ref.min()) == int(ref.max()) > 0
    assert int(words.max()) == int(ref[0]) and int(words.min()) >= 0
    assert torch.equal(words0, words)


def test_conv1x1_default_and_variant0_agree_bit_for_bit():
    from occnet_amd import ext
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 64, 5, 7, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(32, 64, generator=g) / 8).cuda()
    b = torch.randn(32, generator=g).cuda()
    wp = ext.conv1x1_pack_weight(w)
    for stride in (1, 2):
        plain = ext.conv1x1_nhwc(x, wp, b, relu=True, stride=stride)
        want = torch.nn.functional.conv2d(x.float(), w.to(torch.bfloat16).float()[:, :, None, None], b, stride=stride).relu()
        assert plain.shape == want.shape
        assert float((plain.float() - want).abs().max()) <= float(want.abs().max()) * 2 ** -8 + 1e-5
        assert torch.equal(ext.conv1x1_nhwc(x, wp, b, relu=True, stride=stride, variant=0), plain)
        assert torch.equal(ext.conv1x1_nhwc(x, wp, b, relu=True, stride=stride, variant=None), plain)
