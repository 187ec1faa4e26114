"""-m gpu: the fused TSA gather's backward (csrc/tsa_fused_backward.hip, ext.tsa_fused_backward / ext.TSAFusedFunction) and
training through it (TemporalSelfAttention.train_fused, OCC_TSA_TRAIN_FUSED=1).

The operator is checked against float64 autograd through tests/tsa_ref.py::tsa_gather_ref on the CPU, at the tiny shapes of
tsa_ref.CASES.  The offset gradient of bilinear interpolation jumps where a pixel coordinate is an integer, and tsa_case puts
queries exactly there: the offset pairs of samples within 1e-3 of such a kink are left out of the grad_offs comparison (at
most 5 % of the pairs per case, asserted).  The float32 floor — the same reference run in float32 on the CPU against float64,
on these inputs and this grad_out, worst of the six cases with and without a shared queue — is 1.83e-5 on grad_offs off the
kinks (max|ref| 3 to 13.5), 2.45e-6 on grad_value and 3.75e-6 on grad_logits; the tests print the measured GPU maxima next to it.
(The figures of the issue that asked for this test, 1.5e-5 and 2.7e-6, were taken with another grad_out.)"""
import functools

import pytest
import torch

from occnet_amd import ext, synthetic
from occnet_amd._lib import OccAmdUnsupported
from tests.grad_bounds import LINEAR_X3_REL, SCA_FUSED_GRAD_ABS, SCA_FUSED_GRAD_REL
from tests.tsa_ref import CASE_IDS, CASES, SEED, D, M, P, tsa_case, tsa_gather_ref, tsa_locations_weights
from tests.util import build_pair, small_cfg

pytestmark = pytest.mark.gpu

KINK = 1e-3                 # |x_im - round(x_im)| below this: the sample's offset pair is not compared
KINK_SHARE = 0.05
FLOOR_VALUE, FLOOR_OFFS, FLOOR_LOGITS = 2.45e-6, 1.83e-5, 3.75e-6      # float32 CPU reference against float64 (module docstring)
N_OFF, N_ATT = M * 2 * P * 2, M * 2 * P


def _grad_out(B, Nq):
    return torch.randn(B, Nq, M * D, generator=torch.Generator().manual_seed(SEED + 100))


def _kink_pairs(offs, logits, ref_2d, H, W):
    """(B, Nq, M*2*P*2) bool: offset elements of samples whose pixel coordinate is within KINK of an integer (float64)."""
    B, Nq = offs.shape[:2]
    loc, _ = tsa_locations_weights(offs.double(), logits.double(), ref_2d.double(), H, W, M, P)    # (B*2, Nq, M, 1, P, 2)
    im = loc * torch.tensor([W, H], dtype=torch.float64) - 0.5
    near = ((im - im.round()).abs() < KINK).any(-1)                          # (B*2, Nq, M, 1, P)
    near = near.view(B, 2, Nq, M, P).permute(0, 2, 3, 1, 4)                  # (B, Nq, M, 2, P): the offsets' memory order
    return near[..., None].expand(B, Nq, M, 2, P, 2).reshape(B, Nq, N_OFF)


def _f64_grads(value, offs, logits, ref_2d, G, H, W, shared):
    """float64 autograd of (out * G).sum() -> (grad_value, grad_offs, grad_logits); `shared`: value is the single map."""
    v = value.double().requires_grad_(True)
    o = offs.double().requires_grad_(True)
    l = logits.double().requires_grad_(True)
    B, Nq = offs.shape[:2]
    vv = torch.stack([v.view(B, Nq, M, D)] * 2, 1).reshape(B * 2, Nq, M, D) if shared else v
    out = tsa_gather_ref(vv, o, l, ref_2d, H, W, M, P)
    (out * G.double()).sum().backward()
    return v.grad, o.grad, l.grad


@functools.lru_cache(maxsize=None)
def _case(i, shared=False):
    """CPU inputs of case i (with `shared`: the single map = queue entry 1), the grad_out, the float64 reference gradients and
    the kink mask: computed once and never written to."""
    B, H, W, spread = CASES[i]
    value, offs, logits, ref_2d = tsa_case(B, H, W, SEED, spread)
    if shared:
        value = value.view(B, 2, H * W, M, D)[:, 1].contiguous()
    G = _grad_out(B, H * W)
    ref = _f64_grads(value, offs, logits, ref_2d, G, H, W, shared)
    kink = _kink_pairs(offs, logits, ref_2d, H, W)
    return (value, offs, logits, ref_2d, G), ref, kink


def _idx(B, H, W):
    return next(i for i, c in enumerate(CASES) if c[:3] == (B, H, W))


def _run_node(value, offs, logits, ref_2d, G, H, W, shared=False, order=None, need=(True, True, True)):
    """TSAFusedFunction on device leaves -> (out, grad_value, grad_offs, grad_logits), None where not required."""
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip((value, offs, logits), need)]
    out = ext.TSAFusedFunction.apply(*leaves, ref_2d, H, W, M, P, shared, order)
    (out * G).sum().backward()
    return (out.detach(),) + tuple(t.grad for t in leaves)


def _compare(tag, got, ref, kink):
    """The issue's bound on all three gradients (grad_offs off the kinks); prints the maxima next to the float32 floor."""
    share = float(kink.float().mean())
    print(f"{tag}: {share * 100:.2f} % of the offset elements within {KINK} of a kink")
    assert share <= KINK_SHARE, (tag, share)
    for name, a, r, floor in (("grad_value", got[0], ref[0], FLOOR_VALUE), ("grad_offs", got[1], ref[1], FLOOR_OFFS),
                              ("grad_logits", got[2], ref[2], FLOOR_LOGITS)):
        a = a.detach().double().cpu().reshape(r.shape)
        diff = (a - r).abs()
        if name == "grad_offs":
            diff = diff.masked_fill(kink, 0.0)
        scale = float(r.abs().max())
        d = float(diff.max())
        print(f"{tag} {name}: max|hip - f64| = {d:.3e} (max|ref| {scale:.3e}; float32 CPU floor {floor:.1e})")
        assert bool(torch.isfinite(a).all()), (tag, name)
        assert d <= SCA_FUSED_GRAD_REL * scale + SCA_FUSED_GRAD_ABS, (tag, name, d, scale)


@pytest.mark.parametrize("mode", ["separate", "shared", "slices", "order"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_op_matches_float64_autograd(i, mode):
    B, H, W, _ = CASES[i]
    Nq = H * W
    shared = mode == "shared"
    (value, offs, logits, ref_2d, G), ref, kink = _case(i, shared)
    value, offs, logits, ref_2d, G = (t.cuda() for t in (value, offs, logits, ref_2d, G))
    tag = f"{CASE_IDS[i]} {mode}"
    if mode == "slices":            # offs / logits as column slices of one wider leaf: autograd routes both gradients into it
        lin = torch.full((B, Nq, 200), 0.25, device='cuda')
        lin[..., :N_OFF] = offs
        lin[..., N_OFF:N_OFF + N_ATT] = logits
        lin.requires_grad_(True)
        v = value.clone().requires_grad_(True)
        o, l = lin[..., :N_OFF], lin[..., N_OFF:N_OFF + N_ATT]
        assert o.stride(1) == 200 and l.data_ptr() == lin.data_ptr() + 4 * N_OFF
        out = ext.TSAFusedFunction.apply(v, o, l, ref_2d, H, W, M, P)
        (out * G).sum().backward()
        got = (v.grad, lin.grad[..., :N_OFF], lin.grad[..., N_OFF:N_OFF + N_ATT])
        assert float(lin.grad[..., N_OFF + N_ATT:].abs().max()) == 0.0
        plain = ext.tsa_fused_forward(value, o.detach(), l.detach(), ref_2d, H, W, M, P)
    else:
        order = None
        if mode == "order":         # steers the forward's locality only; the backward ignores it
            order = torch.randperm(Nq, generator=torch.Generator().manual_seed(11)).to(torch.int32).cuda()
        out, *got = _run_node(value, offs, logits, ref_2d, G, H, W, shared=shared, order=order)
        plain = ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, M, P, shared_queue=shared, order=order)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), plain)                  # the node's forward IS the inference gather
    assert got[0].shape == value.shape
    _compare(tag, got, ref, kink)


def test_non_finite_offsets():
    """The forward test's construction: samples at +-Inf / NaN.  All three gradients finite, grad_offs exactly zero for the
    dead samples, and the live points of a group with a dead member match the reference."""
    B, H, W = 1, 12, 14
    Nq = H * W
    (value, offs, logits, ref_2d, G), _, _ = _case(_idx(B, H, W))
    offs = offs.clone()
    o = offs.view(B, Nq, M, 2, P, 2)
    inf, nan = float('inf'), float('nan')
    o[0, 20, 0:4] = inf                                   # heads 0-3: all 8 samples
    o[0, 20, 5, 0, 1, 0] = inf                            # head 5: one sample, x only
    o[0, 77, 2] = -inf
    o[0, 77, 6, 1] = -inf                                 # head 6: every sample of queue entry 1
    o[0, 150, 7] = nan
    o[0, 150, 1, 0, 2, 1] = nan
    o[0, 150, 3, :, :, 0] = nan                           # head 3: all 8 samples through x alone
    dead = ~torch.isfinite(o).all(-1)                     # (B, Nq, M, 2, P)
    assert int(dead.sum()) == 4 * 8 + 1 + 8 + 4 + 8 + 1 + 8
    ref = _f64_grads(value, offs, logits, ref_2d, G, H, W, False)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    kink = _kink_pairs(offs, logits, ref_2d, H, W)
    _, *got = _run_node(*(t.cuda() for t in (value, offs, logits, ref_2d, G)), H, W)
    torch.cuda.synchronize()
    _compare("non-finite offsets", got, ref, kink)
    go = got[1].cpu().view(B, Nq, M, 2, P, 2)
    gl = got[2].cpu().view(B, Nq, M, 2, P)
    assert float(go[dead].abs().max()) == 0.0
    assert float(ref[1].view(B, Nq, M, 2, P, 2)[dead].abs().max()) == 0.0
    # groups with one dead member: the live points keep their gradients, the dead point its softmax-backward term
    rl = ref[2].view(B, Nq, M, 2, P)
    ro = ref[1].view(B, Nq, M, 2, P, 2)
    for q, m, t, p_dead in ((20, 5, 0, 1), (150, 1, 0, 2)):
        live = [p for p in range(P) if p != p_dead]
        assert float(ro[0, q, m, t, live].abs().max()) > 0.0 and float(go[0, q, m, t, live].abs().max()) > 0.0
        scale = float(ref[2].abs().max())
        assert float((gl[0, q, m, t].double() - rl[0, q, m, t]).abs().max()) <= SCA_FUSED_GRAD_REL * scale + SCA_FUSED_GRAD_ABS
        assert float(rl[0, q, m, t, p_dead].abs()) > 0.0 and float(gl[0, q, m, t, p_dead].abs()) > 0.0


def test_contract_partial_requires_grad(monkeypatch):
    """needs_input_grad is honoured: what needs no gradient is not computed and comes back as None; what is computed equals
    the all-on run bit for bit (grad_value under the deterministic replay)."""
    monkeypatch.setenv("OCC_MSDA_BWD_DETERMINISTIC", "1")
    B, H, W = 2, 9, 7
    (value, offs, logits, ref_2d, G), _, _ = _case(_idx(B, H, W))
    dev = tuple(t.cuda() for t in (value, offs, logits, ref_2d, G))
    seen = []
    real = ext.tsa_fused_backward

    def recorded(*a, **k):
        r = real(*a, **k)
        seen.append(tuple(x is not None for x in r))
        return r
    monkeypatch.setattr(ext, "tsa_fused_backward", recorded)
    _, gv, go, gl = _run_node(*dev, H, W)
    assert seen == [(True, True, True)]
    _, gv1, go1, gl1 = _run_node(*dev, H, W, need=(True, False, False))
    assert seen[-1] == (True, False, False) and go1 is None and gl1 is None
    assert torch.equal(gv1, gv)
    _, gv2, go2, gl2 = _run_node(*dev, H, W, need=(False, True, True))
    assert seen[-1] == (False, True, True) and gv2 is None
    assert torch.equal(go2, go) and torch.equal(gl2, gl)
    _, gv3, go3, gl3 = _run_node(*dev, H, W, need=(False, False, True))
    assert gv3 is None and go3 is None and torch.equal(gl3, gl)
    # torch.autograd.grad on the all-on graph
    leaves = [t.detach().clone().requires_grad_(True) for t in dev[:3]]
    out = ext.TSAFusedFunction.apply(*leaves, dev[3], H, W, M, P)
    g3 = torch.autograd.grad((out * dev[4]).sum(), leaves)
    assert torch.equal(g3[0], gv) and torch.equal(g3[1], go) and torch.equal(g3[2], gl)
    torch.cuda.synchronize()


def test_unsupported_raises_before_any_launch(monkeypatch):
    B, H, W = 1, 12, 14
    Nq = H * W
    (value, offs, logits, ref_2d, _), _, _ = _case(_idx(B, H, W))
    value, offs, logits, ref_2d = (t.cuda() for t in (value, offs, logits, ref_2d))
    launches = []
    monkeypatch.setattr(ext, "tsa_fused_forward", lambda *a, **k: launches.append(1))
    monkeypatch.setattr(ext, "_tsa_fused_forward", lambda *a, **k: launches.append(1))
    with pytest.raises(OccAmdUnsupported, match="value_rows"):        # a row band: the row pipeline is an inference device
        ext.TSAFusedFunction.apply(value, offs[:, :28], logits[:, :28], ref_2d[:, :28].contiguous(), H, W, M, P, False,
                                   None, Nq)
    with pytest.raises(OccAmdUnsupported):                            # P = 8
        ext.TSAFusedFunction.apply(value, torch.zeros(B, Nq, M * 2 * 8 * 2, device='cuda'),
                                   torch.zeros(B, Nq, M * 2 * 8, device='cuda'), ref_2d, H, W, M, 8)
    with pytest.raises(OccAmdUnsupported):                            # D = 64
        ext.TSAFusedFunction.apply(torch.zeros(B * 2, Nq, M, 64, device='cuda'), offs, logits, ref_2d, H, W, M, P)
    with pytest.raises(OccAmdUnsupported):                            # M = 4
        ext.TSAFusedFunction.apply(torch.zeros(B * 2, Nq, 4, D, device='cuda'), offs[..., :N_OFF // 2],
                                   logits[..., :N_ATT // 2], ref_2d, H, W, 4, P)
    with pytest.raises(OccAmdUnsupported):
        ext.tsa_fused_backward(value, torch.zeros(B, Nq, M * 2 * 8 * 2, device='cuda'),
                               torch.zeros(B, Nq, M * 2 * 8, device='cuda'), ref_2d,
                               torch.zeros(B, Nq, M * D, device='cuda'), H, W, M, 8)
    assert not launches


@pytest.mark.parametrize("B,H,W", [(1, 12, 14), (2, 9, 7)], ids=["B1_12x14", "B2_9x7"])
def test_backward_is_bit_reproducible(B, H, W, monkeypatch):
    """grad_offs / grad_logits bit-identical across calls in every mode; grad_value too under OCC_MSDA_BWD_DETERMINISTIC=1, and
    within 1e-5 * max|ref| of the default mode's."""
    (value, offs, logits, ref_2d, G), ref, _ = _case(_idx(B, H, W))
    args = tuple(t.cuda() for t in (value, offs, logits, ref_2d, G))
    run = lambda: ext.tsa_fused_backward(*args, H, W, M, P)
    monkeypatch.delenv("OCC_MSDA_BWD_DETERMINISTIC", raising=False)
    a, b = run(), run()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    scale = float(ref[0].abs().max())
    assert float((a[0] - b[0]).abs().max()) <= 1e-5 * scale
    monkeypatch.setenv("OCC_MSDA_BWD_DETERMINISTIC", "1")
    c, d = run(), run()
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and torch.equal(c[2], d[2])
    assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])
    assert float((c[0] - a[0]).abs().max()) <= 1e-5 * scale
    torch.cuda.synchronize()


def _count_backward(monkeypatch):
    calls = []
    real = ext.tsa_fused_backward

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ext, "tsa_fused_backward", counted)
    return calls


@functools.lru_cache(maxsize=None)
def _module():
    from occnet_amd.plugin.temporal_self_attention import TemporalSelfAttention
    torch.manual_seed(3)
    mod = TemporalSelfAttention(embed_dims=256, num_levels=1)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():               # the reference initialises both query Linears' weights to zero: give them a slope
        mod.sampling_offsets.weight.copy_(torch.randn(mod.sampling_offsets.weight.shape, generator=g) * 0.05)
        mod.attention_weights.weight.copy_(torch.randn(mod.attention_weights.weight.shape, generator=g) * 0.1)
    return mod.cuda().eval()            # eval: no dropout noise between the two paths; gradients still flow


@pytest.mark.parametrize("history", [False, True], ids=["no_history", "history"])
@pytest.mark.parametrize("bs", [1, 2])
def test_module_train_fused_equals_default_path(bs, history, monkeypatch):
    from occnet_amd.plugin.temporal_self_attention import TemporalSelfAttention
    H, W, C = 12, 14, 256
    Nq = H * W
    mod = _module()
    g = torch.Generator().manual_seed(20 + bs * 2 + history)
    query0 = torch.randn(bs, Nq, C, generator=g).cuda()
    pos = (torch.randn(bs, Nq, C, generator=g) * 0.5).cuda()
    prev0 = torch.randn(bs, Nq, C, generator=g).cuda() if history else None
    ref_2d = torch.rand(bs * 2, Nq, 1, 2, generator=g).cuda()
    Gout = torch.randn(bs, Nq, C, generator=g).cuda()
    shapes = torch.tensor([[H, W]], dtype=torch.int64, device='cuda')
    start = torch.zeros(1, dtype=torch.int64, device='cuda')
    calls = _count_backward(monkeypatch)
    res = {}
    for flag in (False, True):
        monkeypatch.setattr(TemporalSelfAttention, "train_fused", flag)
        mod.zero_grad(set_to_none=True)
        query = query0.clone().requires_grad_(True)
        prev = prev0.clone().requires_grad_(True) if history else None
        value = torch.stack([prev, query], 1).reshape(bs * 2, Nq, C) if history else None
        n0 = len(calls)
        out = mod(query, value=value, query_pos=pos, reference_points=ref_2d, spatial_shapes=shapes,
                  level_start_index=start, bev_h=H, bev_w=W)
        (out * Gout).sum().backward()
        torch.cuda.synchronize()
        assert len(calls) - n0 == (1 if flag else 0)      # the default path never calls it, the fused path exactly once
        grads = {n: p.grad.detach().clone() for n, p in mod.named_parameters()}
        grads["query"] = query.grad.detach().clone()
        if history:
            grads["prev_bev"] = prev.grad.detach().clone()
        res[flag] = (out.detach(), grads)
    d = float((res[True][0] - res[False][0]).abs().max())
    scale = float(res[False][0].abs().max())
    print(f"bs={bs} history={history}: output max diff {d:.3e} (max {scale:.3e})")
    assert d <= LINEAR_X3_REL * scale
    assert res[True][1].keys() == res[False][1].keys()
    for n, gr in res[False][1].items():
        d = float((res[True][1][n] - gr).abs().max())
        scale = float(gr.abs().max())
        print(f"bs={bs} history={history} {n}: gradient max diff {d:.3e} (max {scale:.3e})")
        assert scale > 0.0, n
        assert d <= SCA_FUSED_GRAD_REL * scale + 1e-5, (n, d, scale)


def _train_step(g, seed, feats, metas, targets):
    prod, _ = build_pair(g, seed=seed)
    out = prod([f.cuda() for f in feats], metas, prev_bev=None)
    sem, flow, mask = targets
    lp = prod.loss(sem.cuda(), flow.cuda(), mask.cuda(), out)
    (lp['loss_occ'] + lp['loss_flow']).backward()
    torch.cuda.synchronize()
    return prod, lp


def test_train_fused_equals_default_path(monkeypatch):
    """One training step with the switch on against off, under the tolerances of
    test_gpu_sca_fused_backward.py::test_train_fused_equals_default_path."""
    from occnet_amd.plugin.temporal_self_attention import TemporalSelfAttention
    from occnet_amd.train import synthetic_targets
    calls = _count_backward(monkeypatch)
    g = small_cfg(bev=(20, 20), num_layers=2)
    feats = synthetic.make_features(g, seed=5)
    metas = synthetic.make_img_metas(g)
    targets = synthetic_targets(g['bev_h'], g['bev_w'], g['pillar_h'], num_classes=17, batch=1, seed=0)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(TemporalSelfAttention, "train_fused", flag)
        prod, lp = _train_step(g, 5, feats, metas, targets)
        res[flag] = ({k: float(v.detach()) for k, v in lp.items()},
                     {n: p.grad.detach().clone() for n, p in prod.named_parameters() if p.grad is not None})
    assert len(calls) == g['num_layers']                  # one fused backward per encoder layer, none with the switch off
    for k in res[True][0]:
        assert abs(res[True][0][k] - res[False][0][k]) < 1e-5, k
    assert res[True][1].keys() == res[False][1].keys()
    worst = 0.0
    for n, gr in res[False][1].items():
        d = float((res[True][1][n] - gr).abs().max())
        floor = 3e-5 if n.endswith('conv.weight') and '.decoder.' in n else 1e-5
        assert d < 1e-3 * float(gr.abs().max()) + floor, (n, d)
        worst = max(worst, d / (float(gr.abs().max()) + 1e-12))
    print(f"TSA train_fused vs default training path: worst relative gradient difference {worst:.2e}")
