"""-m gpu: the third whole-bottleneck kernel (the last layer1 block with the next block's conv1 and stride-2 shortcut computed
on the tile) returns the bits of the three launches it replaces, on the smallest shapes at which it can go wrong, into
interior slices of NaN-filled buffers, twice; the torch restatement within the tolerances of the bottleneck64 and 1x1 tests;
argument checks; and the backbone plan takes the fused route exactly where its rule says, with the same FPN maps."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 3, 5),       # smaller than one tile; shortcut 2 x 3
    (1, 9, 17),      # four partial tiles, odd sizes: the stride-2 edge (H - 1) // 2 + 1 = 5, 9 lies in a tile of its own
    (3, 20, 40),     # 27 tiles, several images, every border case
    (2, 40, 80),     # 50 full tiles
]
CMID = 128


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(N, H, W):
    """Inputs, packs, and the three-launch route's outputs (computed once per shape, never modified)."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(256 + H * W)
    x = _cl(torch.randn(N, 256, H, W, generator=g).cuda().to(torch.bfloat16))
    w1 = (torch.randn(64, 256, 1, 1, generator=g) / 16.0).cuda()
    w2 = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).cuda()
    w3 = (torch.randn(256, 64, 1, 1, generator=g) / 8.0).cuda()
    b1, b2, b3 = (torch.randn(n, generator=g).cuda() * 0.3 for n in (64, 64, 256))
    wn = (torch.randn(CMID, 256, generator=g) / 16.0).cuda()
    wd = (torch.randn(4 * CMID, 256, generator=g) / 16.0).cuda()
    bn, bd = (torch.randn(n, generator=g).cuda() * 0.3 for n in (CMID, 4 * CMID))
    ws = (w1, b1, w2, b2, w3, b3)
    pack = ext.bottleneck64_pack(*ws)
    wnp, wdp = ext.conv1x1_pack_weight(wn), ext.conv1x1_pack_weight(wd)
    # the route the fused launch replaces, every kernel forced: tiny maps default to the tiled 1x1, whose K order rotates
    mid = ext.bottleneck64_nhwc(x, pack, variant=2)
    y = ext.conv1x1_nhwc(mid, wnp, bn, relu=True, variant=2)
    sc = ext.conv1x1_nhwc(mid, wdp, bd, stride=2, variant=2)
    return dict(x=x, ws=ws, pack=pack, wn=wn, bn=bn, wd=wd, bd=bd, wnp=wnp, wdp=wdp, mid=mid, y=y, sc=sc)


def _guarded(N, C, H, W):
    """An (N, C, H, W) channels_last output as the interior of a NaN-filled buffer with one guard image on either side (the
    interior stays contiguous); -> (whole buffer, interior)."""
    buf = _cl(torch.full((N + 2, C, H, W), float('nan'), dtype=torch.bfloat16, device='cuda'))
    return buf, buf[1:N + 1]


def _run(c, N, H, W):
    from occnet_amd import ext
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ybuf, y = _guarded(N, CMID, H, W)
    sbuf, sc = _guarded(N, 4 * CMID, Ho, Wo)
    got = ext.bottleneck64_next_nhwc(c['x'], c['pack'], c['wnp'], c['bn'], c['wdp'], c['bd'], out=(y, sc))
    assert got[0] is y and got[1] is sc
    for name, buf in (("y", ybuf), ("shortcut", sbuf)):
        assert not bool(torch.isnan(buf[1:N + 1]).any()), f"{name}: elements left unwritten"
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[N + 1]).all()), f"{name}: a store outside the output"
    return y, sc


def _reference(c):
    """fp32 torch restatement: _reference of tests/test_gpu_bottleneck64_v2.py, its map rounded to bf16, then the two 1x1s
    on bf16 weights with f32 accumulation."""
    r = lambda t: t.to(torch.bfloat16).float()
    F = torch.nn.functional
    w1, b1, w2, b2, w3, b3 = c['ws']
    xf = c['x'].float()
    c1 = r(F.conv2d(xf, r(w1), b1).relu())
    c2 = r(F.conv2d(c1, r(w2), b2, padding=1).relu())
    mid = r((F.conv2d(c2, r(w3), b3) + xf).relu())
    return (F.conv2d(mid, r(c['wn'])[:, :, None, None], c['bn']).relu(),
            F.conv2d(mid, r(c['wd'])[:, :, None, None], c['bd'], stride=2))


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_fused_launch_returns_the_bits_of_the_three_launches(N, H, W):
    c = _case(N, H, W)
    y, sc = _run(c, N, H, W)
    assert y.shape == c['y'].shape and sc.shape == c['sc'].shape
    assert torch.equal(y, c['y']), f"y differs in {int((y != c['y']).sum())} of {y.numel()} elements"
    assert torch.equal(sc, c['sc']), f"shortcut differs in {int((sc != c['sc']).sum())} of {sc.numel()} elements"
    y2, sc2 = _run(c, N, H, W)                                            # repeating the call gives identical bits
    assert torch.equal(y2, y) and torch.equal(sc2, sc)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_fused_launch_matches_torch(N, H, W):
    from occnet_amd import ext
    c = _case(N, H, W)
    y, sc = ext.bottleneck64_next_nhwc(c['x'], c['pack'], c['wnp'], c['bn'], c['wdp'], c['bd'])
    assert y.is_contiguous(memory_format=torch.channels_last) and sc.is_contiguous(memory_format=torch.channels_last)
    # the whole chain: the tolerances of test_second_kernel_computes_the_first_kernels_bits
    for name, got, want in zip(("y", "shortcut"), (y, sc), _reference(c)):
        d, scale = float((got.float() - want).abs().max()), float(want.abs().max())
        mean = float((got.float() - want).abs().mean())
        print(f"bottleneck64_next {name} {N}x{H}x{W}: max diff {d:.3e} mean {mean:.3e} (scale {scale:.2f})")
        assert d <= scale * 2 ** -7 + 1e-5
        assert mean <= scale * 2 ** -11
    # each 1x1 on the map the second kernel stores: the tolerance of tests/test_gpu_conv1x1_variants.py (one bf16 rounding)
    F = torch.nn.functional
    r = lambda t: t.to(torch.bfloat16).float()
    mid = c['mid'].float()
    for name, got, want in (("y", y, F.conv2d(mid, r(c['wn'])[:, :, None, None], c['bn']).relu()),
                            ("shortcut", sc, F.conv2d(mid, r(c['wd'])[:, :, None, None], c['bd'], stride=2))):
        d, scale = float((got.float() - want).abs().max()), float(want.abs().max())
        print(f"bottleneck64_next {name} {N}x{H}x{W} on the stored map: max diff {d:.3e} (scale {scale:.2f})")
        assert d <= scale * 2 ** -8 + 1e-6, (d, scale)


def test_arguments_are_checked_before_any_launch():
    from occnet_amd import ext
    N, H, W = 1, 3, 5
    c = _case(N, H, W)
    args = (c['x'], c['pack'], c['wnp'], c['bn'], c['wdp'], c['bd'])
    bf = dict(dtype=torch.bfloat16, device='cuda')
    good_y, good_s = _cl(torch.empty(N, CMID, H, W, **bf)), _cl(torch.empty(N, 4 * CMID, 2, 3, **bf))
    with pytest.raises(ext.OccAmdError):                                   # dtype
        ext.bottleneck64_next_nhwc(c['x'].float(), *args[1:])
    with pytest.raises(ext.OccAmdError):                                   # layout: NCHW-contiguous
        ext.bottleneck64_next_nhwc(c['x'].contiguous(), *args[1:])
    with pytest.raises(ext.OccAmdError):                                   # f16 output
        ext.bottleneck64_next_nhwc(*args, out=(good_y.to(torch.float16), good_s))
    with pytest.raises(ext.OccAmdError):                                   # NCHW-contiguous output
        ext.bottleneck64_next_nhwc(*args, out=(torch.empty(N, CMID, H, W, **bf), good_s))
    with pytest.raises(ext.OccAmdError):                                   # y of another width
        ext.bottleneck64_next_nhwc(*args, out=(_cl(torch.empty(N, CMID, H, W + 1, **bf)), good_s))
    with pytest.raises(ext.OccAmdError):                                   # shortcut at floor(H / 2) instead of (H - 1) // 2 + 1
        ext.bottleneck64_next_nhwc(*args, out=(good_y, _cl(torch.empty(N, 4 * CMID, 1, 2, **bf))))
    with pytest.raises(ext.OccAmdError):                                   # shortcut with cmid channels
        ext.bottleneck64_next_nhwc(*args, out=(good_y, _cl(torch.empty(N, CMID, 2, 3, **bf))))
    with pytest.raises(ext.OccAmdError):                                   # a downsample weight of another size
        ext.bottleneck64_next_nhwc(c['x'], c['pack'], c['wnp'], c['bn'], c['wnp'], c['bd'])
    # a cmid_next without a kernel: consistent operands, refused by the entry point
    g = torch.Generator().manual_seed(1)
    for cm in (64, 256):
        wn, wd = torch.randn(cm, 256, generator=g).cuda(), torch.randn(4 * cm, 256, generator=g).cuda()
        with pytest.raises(ext.OccAmdUnsupported, match="no kernel for cmid_next"):
            ext.bottleneck64_next_nhwc(c['x'], c['pack'], ext.conv1x1_pack_weight(wn), torch.zeros(cm).cuda(),
                                       ext.conv1x1_pack_weight(wd), torch.zeros(4 * cm).cuda())
    # and the good call still goes through
    y, sc = ext.bottleneck64_next_nhwc(*args, out=(good_y, good_s))
    assert torch.equal(y, c['y']) and torch.equal(sc, c['sc'])


def _resnet_fpn(out_indices):
    from occnet_amd.plugin.backbone import FPN, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=out_indices, frozen_stages=1, norm_eval=True).eval()
    bb.init_weights()
    chans = [256, 512, 1024, 2048]
    nk = FPN(in_channels=[chans[i] for i in out_indices], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    return bb.cuda(), nk.cuda()


def _count_fused(monkeypatch):
    from occnet_amd import ext
    real, calls = ext.bottleneck64_next_nhwc, []

    def counting(x, *a, **kw):
        calls.append(tuple(x.shape))
        return real(x, *a, **kw)

    monkeypatch.setattr(ext, 'bottleneck64_next_nhwc', counting)
    return calls


def test_plan_takes_the_fused_route_once_and_returns_the_same_maps(monkeypatch):
    """2 x 3 x 128 x 256 images: a 32 x 64 layer1 map, M = 4096 and 1024 at stride 2, so the rule fuses."""
    from occnet_amd import ext
    from occnet_amd.plugin.backbone import FusedInferenceBackbone
    bb, nk = _resnet_fpn((1, 2, 3))
    x = torch.randn(2, 3, 128, 256).cuda() * 50.0
    assert ext.bottleneck64_next_pick(2, 32, 64, 128)
    calls = _count_fused(monkeypatch)
    with torch.no_grad():
        plan = FusedInferenceBackbone(bb, nk, fuse_next_stage=True)
        monkeypatch.delenv('OCC_BOTTLENECK64_NEXT', raising=False)
        new = [t.clone() for t in plan(x)]
        assert calls == [(2, 256, 32, 64)]                                # exactly once per forward
        monkeypatch.setenv('OCC_BOTTLENECK64_NEXT', '0')
        old = [t.clone() for t in plan(x)]
        assert len(calls) == 1                                            # the switch keeps the three launches
        monkeypatch.delenv('OCC_BOTTLENECK64_NEXT')
        plain = FusedInferenceBackbone(bb, nk)(x)                         # a plan built without fuse_next_stage
        assert len(calls) == 1
        for u, v in zip(plain, old):
            assert torch.equal(u, v)
    assert len(new) == len(old) == 4
    for u, v in zip(new, old):
        assert torch.equal(u, v), float((u.float() - v.float()).abs().max())


def test_plan_keeps_the_map_where_something_else_reads_it(monkeypatch):
    from occnet_amd.plugin.backbone import FusedInferenceBackbone
    monkeypatch.delenv('OCC_BOTTLENECK64_NEXT', raising=False)
    x = torch.randn(2, 3, 128, 256).cuda() * 50.0
    calls = _count_fused(monkeypatch)
    with torch.no_grad():
        bb, nk = _resnet_fpn((0, 1, 2, 3))                                # layer1's output is an FPN input
        outs = FusedInferenceBackbone(bb, nk, fuse_next_stage=True)(x)
        assert len(outs) == 4 and tuple(outs[0].shape) == (2, 256, 32, 64)
        assert calls == []
        bb, _ = _resnet_fpn((1, 2, 3))
        for k in (1, 2):                                                  # the plan ends at layer1; forward_prefix keeps every map
            out = FusedInferenceBackbone(bb, None, prefix_stages=k, fuse_next_stage=True).forward_prefix(x)
            assert tuple(out.shape) == (2, 256 * k, 32 // k, 64 // k)
        assert calls == []
