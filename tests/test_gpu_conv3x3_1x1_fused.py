"""gpu: ext.conv3x3_conv1x1_nhwc (conv2 + conv3 of a layer2 / layer3 bottleneck in one launch) returns the bits of the two
launches it replaces, for every tile id it has; both agree with torch within the bound of the project's other
multi-rounding fused block; the plan takes the fused launch exactly where occ_conv3x3_conv1x1_pick says so."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# input geometries (N, H, W, stride) of tests/test_gpu_conv1x1_variants.py: a map smaller than one tile; ragged in both
# directions with tiles cut by the image edge; odd sizes at stride 2; three images at stride 2
GEOMETRIES = [(1, 5, 7, 1), (2, 13, 11, 1), (2, 27, 35, 2), (3, 9, 15, 2)]
CHANNELS = [(128, 512), (256, 1024)]
# every tile id the fused kernel is built for, by (Cmid, stride)
TILES = {(128, 1): (12,), (128, 2): (12, 13), (256, 1): (22, 23, 24), (256, 2): (22,)}
# conv2 inputs of one base-config step (6 cameras, 928 x 1600): (Cmid, H, W, stride)
BASE_SHAPES = [(128, 116, 200, 1), (128, 232, 400, 2), (256, 58, 100, 1), (256, 116, 200, 2)]


def _cl(t):
    return t.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(N, cmid, cout, H, W, stride):
    """Inputs seeded as test_gpu_conv1x1_variants._case, weights scaled by fan-in^-0.5; shared and never modified."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(cmid + 31 * H + W + stride)
    x = _cl(torch.randn(N, cmid, H, W, generator=g))
    w2 = (torch.randn(cmid, cmid, 3, 3, generator=g) / (9 * cmid) ** 0.5).cuda().to(torch.bfloat16)
    b2 = torch.randn(cmid, generator=g).cuda() * 0.3
    w3 = (torch.randn(cout, cmid, generator=g) / cmid ** 0.5).cuda().to(torch.bfloat16)
    b3 = torch.randn(cout, generator=g).cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = _cl(torch.randn(N, cout, Ho, Wo, generator=g))
    return dict(x=x, w2=w2, b2=b2, w3=w3, b3=b3, r=r, p2=ext.conv3x3_pack_weight(w2.float().contiguous()),
                p3=ext.conv1x1_pack_weight(w3.float()), cmid=cmid, cout=cout, stride=stride)


def _pair(c, v):
    from occnet_amd import ext
    mid = ext.conv3x3_nhwc(c['x'], c['p2'], c['b2'], c['cmid'], relu=True, stride=c['stride'], variant=v)
    return ext.conv1x1_nhwc(mid, c['p3'], c['b3'], residual=c['r'], relu=True, variant=2)


def _fused(c, v):
    from occnet_amd import ext
    return ext.conv3x3_conv1x1_nhwc(c['x'], c['p2'], c['b2'], c['cmid'], c['p3'], c['b3'], c['r'], stride=c['stride'],
                                    variant=v)


@functools.lru_cache(maxsize=None)
def _torch_reference(N, cmid, cout, H, W, stride):
    """conv2d in f32 on the bf16 operands, rounded to bf16, then conv2d + residual + ReLU in f32."""
    c = _case(N, cmid, cout, H, W, stride)
    F = torch.nn.functional
    mid = F.conv2d(c['x'].float(), c['w2'].float(), c['b2'], stride=stride, padding=1).relu().to(torch.bfloat16)
    want = F.conv2d(mid.float(), c['w3'].float().view(cout, cmid, 1, 1), c['b3']) + c['r'].float()
    return want.relu()


def _check_against_torch(got, want, what):
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    d = (got.float() - want).abs()
    scale = float(want.abs().max())
    print(f"{what}: max diff {float(d.max()):.3e} mean {float(d.mean()):.3e} (scale {scale:.2f})")
    # the bound of test_bottleneck64_fused_matches_torch: one bf16 rounding of the output + rounding flips of the bf16
    # intermediate (f32 summation order differs from torch's)
    assert float(d.max()) <= scale * 2 ** -7 + 1e-5
    assert float(d.mean()) <= scale * 2 ** -11


@pytest.mark.parametrize("cmid,cout", CHANNELS)
@pytest.mark.parametrize("N,H,W,stride", GEOMETRIES)
def test_fused_equals_the_two_launches_on_small_maps(N, H, W, stride, cmid, cout):
    """The default rule does not fuse maps this small: every tile id is forced."""
    from occnet_amd import ext
    c = _case(N, cmid, cout, H, W, stride)
    assert ext.conv3x3_conv1x1_pick(N, H, W, cmid, cout, stride) == 0
    with pytest.raises(ext.OccAmdUnsupported):
        _fused(c, None)
    want = _torch_reference(N, cmid, cout, H, W, stride)
    for v in TILES[(cmid, stride)]:
        pair, got = _pair(c, v), _fused(c, v)
        assert got.shape == pair.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, pair), (v, float((got.float() - pair.float()).abs().max()))
        assert torch.equal(_fused(c, v), got), v                      # a second call is bit-identical
        _check_against_torch(pair, want, f"pair  v{v} {cmid} {N}x{H}x{W} s{stride}")
        _check_against_torch(got, want, f"fused v{v} {cmid} {N}x{H}x{W} s{stride}")


@pytest.mark.parametrize("cmid,cout", CHANNELS)
@pytest.mark.parametrize("N,H,W,stride", [(2, 13, 11, 1), (2, 27, 35, 2)])
def test_fused_stores_nothing_outside_the_map(N, H, W, stride, cmid, cout, monkeypatch):
    """The output lies inside a larger poisoned allocation: tiles cut by the image edge must not write past the map."""
    from occnet_amd import ext
    c = _case(N, cmid, cout, H, W, stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    n_out = N * Ho * Wo * cout
    pad = 64 * cout
    real_empty = torch.empty
    for v in TILES[(cmid, stride)]:
        big = torch.full((n_out + 2 * pad,), -7.0, dtype=torch.bfloat16, device='cuda')

        def empty(shape, *a, **kw):
            if isinstance(shape, (tuple, list)) and tuple(shape) == (N, cout, Ho, Wo):
                return big[pad:pad + n_out].view(N, Ho, Wo, cout).permute(0, 3, 1, 2)
            return real_empty(shape, *a, **kw)

        monkeypatch.setattr(torch, 'empty', empty)
        got = _fused(c, v)
        monkeypatch.setattr(torch, 'empty', real_empty)
        assert got.data_ptr() == big.data_ptr() + 2 * pad
        assert bool((big[:pad] == -7.0).all()) and bool((big[pad + n_out:] == -7.0).all()), v
        assert torch.equal(got, _pair(c, v)), v


@pytest.mark.parametrize("cmid,H,W,stride", BASE_SHAPES)
def test_full_size_default_launch_equals_the_pair_at_the_picked_tile(cmid, H, W, stride):
    from occnet_amd import ext
    cout = 4 * cmid
    c = _case(6, cmid, cout, H, W, stride)
    v = ext.conv3x3_conv1x1_pick(6, H, W, cmid, cout, stride)
    print(f"pick {cmid}/{cout} {H}x{W} s{stride}: {v}")
    if v == 0:
        with pytest.raises(ext.OccAmdUnsupported):
            _fused(c, None)
        return
    assert v in TILES[(cmid, stride)]
    got = _fused(c, None)
    assert torch.equal(got, _pair(c, v))
    assert torch.equal(got, _fused(c, v))
    torch.cuda.synchronize()
    _case.cache_clear()                                               # the full-size operands are not shared further


def test_plan_takes_the_fused_launch_where_pick_says_so(monkeypatch):
    """FusedInferenceBackbone on one base-config input (6 x 3 x 928 x 1600, the size at which pick fuses the layer2 and
    layer3 maps) with the fused dispatch and with OCC_CONV3X3_FUSE_1X1=0.

    Of the ten layer2 / layer3 bottlenecks nine take the fused launch: the rule keeps 256 -> 1024 at stride 2 (the first
    block of layer3) on the pair, where the fused launch measured no faster in the plan (EXPERIMENTS.md section 8i).  Every
    fused launch runs the tile the 3x3 launcher picks, so the two plans return the same bits."""
    from occnet_amd import ext
    from occnet_amd.plugin.backbone import FPN, FusedInferenceBackbone, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_eval=True).eval()
    bb.init_weights()
    nk = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    bb, nk = bb.cuda(), nk.cuda()
    x = torch.randn(6, 3, 928, 1600).cuda() * 50.0
    real = ext.conv3x3_conv1x1_nhwc
    calls = []

    def counting(x, *a, **kw):
        calls.append((x.shape[1], x.shape[2], x.shape[3], kw.get('stride', 1)))
        return real(x, *a, **kw)

    # blocks per shape: layer2 = 1 at stride 2 + 3 at stride 1, layer3 = 1 + 5
    blocks = dict(zip(BASE_SHAPES, (3, 1, 5, 1)))
    picks = {s: ext.conv3x3_conv1x1_pick(6, s[1], s[2], s[0], 4 * s[0], s[3]) for s in BASE_SHAPES}
    assert [bool(picks[s]) for s in BASE_SHAPES] == [True, True, True, False], picks
    with torch.no_grad():
        plan = FusedInferenceBackbone(bb, nk)
        monkeypatch.setattr(ext, 'conv3x3_conv1x1_nhwc', counting)
        a = [t.clone() for t in plan(x)]
        n_fused = len(calls)
        monkeypatch.setenv('OCC_CONV3X3_FUSE_1X1', '0')
        b = plan(x)
        assert len(calls) == n_fused                                  # the switch keeps the pair
    assert n_fused == 9, calls
    for s in BASE_SHAPES:
        assert calls.count(s) == (blocks[s] if picks[s] else 0), (s, calls)
    for u, v in zip(a, b):
        assert torch.equal(u, v), float((u.float() - v.float()).abs().max())
