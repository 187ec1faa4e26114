"""-m gpu: the second whole-bottleneck kernel (identity from the staged tile, XCD-local tile order) computes the first
kernel's bits: every forced variant against variant 1 on the smallest shapes at which the kernel can go wrong, into an
output buffer pre-filled with NaN, twice; and the backbone plan with the default routing against OCC_BOTTLENECK64_V2=0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 3, 5),       # smaller than one tile
    (1, 9, 17),      # four partial tiles, fewer blocks than XCDs
    (3, 20, 40),     # 27 tiles, 27 % 8 = 3, every border case, several images
    (2, 40, 80),     # 50 tiles, two bands of 4 tile rows and one of 1 per image
]


def _case(cin, ds, N, H, W):
    g = torch.Generator().manual_seed(cin + H * W)
    x = torch.randn(N, cin, H, W, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w1 = (torch.randn(64, cin, 1, 1, generator=g) / cin ** 0.5).cuda()
    w2 = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).cuda()
    w3 = (torch.randn(256, 64, 1, 1, generator=g) / 8.0).cuda()
    b1, b2, b3 = (torch.randn(n, generator=g).cuda() * 0.3 for n in (64, 64, 256))
    wds = (torch.randn(256, cin, 1, 1, generator=g) / cin ** 0.5).cuda() if ds else None
    bds = torch.randn(256, generator=g).cuda() * 0.3 if ds else None
    return x, (w1, b1, w2, b2, w3, b3, wds, bds)


def _reference(x, w1, b1, w2, b2, w3, b3, wds=None, bds=None):
    """fp32 torch restatement of what the fused kernels compute (as tests/test_gpu_backbone.py: bf16 weights, f32
    accumulation, the two 64-channel intermediates rounded to bf16)."""
    r = lambda t: t.to(torch.bfloat16).float()
    F = torch.nn.functional
    xf = x.float()
    c1 = r(F.conv2d(xf, r(w1), b1).relu())
    c2 = r(F.conv2d(c1, r(w2), b2, padding=1).relu())
    idn = xf if wds is None else F.conv2d(xf, r(wds), bds)
    return (F.conv2d(c2, r(w3), b3) + idn).relu()


@pytest.mark.parametrize("N,H,W", SHAPES)
@pytest.mark.parametrize("cin,ds", [(256, False), (64, True)])
def test_second_kernel_computes_the_first_kernels_bits(cin, ds, N, H, W):
    from occnet_amd import ext
    x, ws = _case(cin, ds, N, H, W)
    pack = ext.bottleneck64_pack(*ws)

    def poisoned():
        return torch.full((N, 256, H, W), float('nan'), dtype=torch.bfloat16, device=x.device).contiguous(
            memory_format=torch.channels_last)

    # the new kernel first, into NaN: a tile no block computes shows as NaN and not as a leftover of the allocator
    got = {}
    for v in (2, 3, 4, 5, 0):
        buf = poisoned()
        res = ext.bottleneck64_nhwc(x, pack, variant=v, out=buf)
        assert res is buf
        got[v] = buf
        assert not bool(torch.isnan(buf).any()), f"variant {v} left elements unwritten"
    again = ext.bottleneck64_nhwc(x, pack, variant=2, out=poisoned())
    first = ext.bottleneck64_nhwc(x, pack, variant=1, out=poisoned())
    assert first.is_contiguous(memory_format=torch.channels_last)
    for v, t in got.items():
        assert torch.equal(t, first), f"variant {v} differs from the first kernel in " \
                                      f"{int((t != first).sum())} of {t.numel()} elements"
    assert torch.equal(again, got[2])                                    # repeating the call gives identical bits
    # and the tolerances of test_bottleneck64_fused_matches_torch against the torch restatement
    want = _reference(x, *ws)
    d = float((got[2].float() - want).abs().max())
    scale = float(want.abs().max())
    print(f"bottleneck64 v2 cin={cin} ds={ds} {N}x{H}x{W}: max diff {d:.3e} (scale {scale:.2f})")
    assert d <= scale * 2 ** -7 + 1e-5
    assert float((got[2].float() - want).abs().mean()) <= scale * 2 ** -11


def test_out_argument_is_checked():
    from occnet_amd import ext
    x, ws = _case(256, False, 1, 3, 5)
    pack = ext.bottleneck64_pack(*ws)
    with pytest.raises(ext.OccAmdError):
        ext.bottleneck64_nhwc(x, pack, out=torch.empty(1, 256, 3, 6, dtype=torch.bfloat16, device=x.device).contiguous(
            memory_format=torch.channels_last))
    with pytest.raises(ext.OccAmdError):
        ext.bottleneck64_nhwc(x, pack, out=x)
    with pytest.raises(ext.OccAmdUnsupported):
        ext.bottleneck64_nhwc(x, pack, variant=6)


def test_plan_default_routing_matches_first_kernel(monkeypatch):
    """FusedInferenceBackbone on a small image: the FPN maps with the default routing are the maps with
    OCC_BOTTLENECK64_V2=0, bit for bit."""
    from occnet_amd.plugin.backbone import FPN, FusedInferenceBackbone, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_eval=True).eval()
    bb.init_weights()
    nk = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    bb, nk = bb.cuda(), nk.cuda()
    x = torch.randn(2, 3, 96, 160).cuda() * 50.0
    with torch.no_grad():
        plan = FusedInferenceBackbone(bb, nk, fused_bottleneck=True)
        assert len(plan._bneck) == 3
        monkeypatch.delenv('OCC_BOTTLENECK64_V2', raising=False)
        new = [t.clone() for t in plan(x)]
        monkeypatch.setenv('OCC_BOTTLENECK64_V2', '0')
        old = plan(x)
    assert len(new) == len(old) == 4
    for u, v in zip(new, old):
        assert torch.equal(u, v)
