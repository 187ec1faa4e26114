"""The decoder's training BatchNorm3d + ReLU kernels (csrc/bn3d_relu_train.hip), the combined Conv3d + BatchNorm3d + ReLU
autograd node (ext.Conv3dBNReLUFunction) and the opt-in decoder path of TransformerOcc built on it.

The bound of every float64 comparison here is
    max|got - ref| / (max|ref| + 1e-12)  <=  max(4 * e_aten, DROPOUT_LN_REL = 2e-5)
where e_aten is the same quantity for ATen's own float32 chain, run on the GPU on the same inputs inside the test: the kernels
are judged against the reference implementation's float32 floor (the factor 4 allows another, still legitimate, summation
order), never against themselves.

The ReLU mask is discontinuous: one element whose pre-activation changes sign between float32 and float64 moves dbeta by
1 / sqrt(rows).  The op-level inputs are therefore conditioned on the CPU, in float64: no pre-activation within 1e-3 of zero
(offenders are nudged by 4e-3 sigma / |gamma| away from it, at most 4 rounds, at most 0.2 % of the elements); the node and
module tests, whose pre-activations come out of a convolution, use seeds chosen on the CPU so that the float64
pre-activations keep 1e-4 clear of zero, and assert that from the float64 reference."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import autograd_contract as ac
from tests import grad_bounds as gb

pytestmark = pytest.mark.gpu

EPS = 1e-5
GEOMS = [(1, 1, 2, 1), (1, 1, 7, 1), (1, 1, 61, 1), (1, 1, 1031, 1), (1, 1, 40009, 1),      # row-count tails, 1 / many blocks
         (1, 3, 5, 4), (2, 6, 7, 8), (2, 19, 24, 16)]                                        # halo, strides, B > 1
SEED = 100          # of the op-level inputs; checked on the CPU: the conditioning below touches at most 0.11 % of the elements


def _rows(geom):
    B, Y, X, Z = geom
    return B * Y * X * Z


def _pre64(y, gamma, beta):
    y64 = y.double()
    sigma = torch.sqrt(y64.var(0, unbiased=False) + EPS)
    return (y64 - y64.mean(0)) / sigma * gamma.double() + beta.double(), sigma


def _condition(y, gamma, beta, clear=1e-3):
    """-> (y with no float64 pre-activation within `clear` of zero, share of elements that were nudged)"""
    y = y.clone()
    touched = torch.zeros(y.shape, dtype=torch.bool)
    for _ in range(4):
        pre, sigma = _pre64(y, gamma, beta)
        bad = pre.abs() < clear
        if not bool(bad.any()):
            break
        away = torch.where(pre >= 0, 1.0, -1.0).double() * torch.sign(gamma.double())
        y = torch.where(bad, (y.double() + away * 4e-3 * sigma / gamma.double().abs()).float(), y)
        touched |= bad
    return y, float(touched.float().mean())


@functools.lru_cache(maxsize=None)
def _case(geom, offset=False):
    """Inputs of one geometry (CPU, float32) and the float64 reference of everything the kernels produce; computed once."""
    rows = _rows(geom)
    g = torch.Generator().manual_seed(SEED + (5000 if offset else 0))
    scale = torch.linspace(0.05, 3.0, 32)[torch.randperm(32, generator=g)]
    y = torch.randn(rows, 32, generator=g) * scale
    if offset:
        y[:, 5] = 300.0 + 0.5 * torch.randn(rows, generator=g)
        y[:, 9] = -40.0 + 0.01 * torch.randn(rows, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(32, generator=g)
    gamma[3] = -gamma[3].abs() - 0.2                        # one negative channel
    beta = 0.5 * torch.randn(32, generator=g)
    go = torch.randn(rows, 32, generator=g)
    rm, rv = 0.1 * torch.randn(32, generator=g), 0.75 + 0.5 * torch.rand(32, generator=g)
    y, share = _condition(y, gamma, beta)
    pre, _ = _pre64(y, gamma, beta)
    y64, g64, b64 = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    rm64, rv64 = rm.double(), rv.double()
    out = torch.relu(F.batch_norm(y64, rm64, rv64, g64, b64, True, 0.1, EPS))
    out.backward(go.double())
    yd = y.double()
    ref = dict(out=out.detach(), mean=yd.mean(0), rstd=1.0 / torch.sqrt(yd.var(0, unbiased=False) + EPS), rm=rm64, rv=rv64,
               dy=y64.grad, dgamma=g64.grad, dbeta=b64.grad)
    return dict(geom=geom, rows=rows, y=y, gamma=gamma, beta=beta, go=go, rm=rm, rv=rv, ref=ref, share=share,
                clear=float(pre.abs().min()))


def _rel(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-12))


def _within(e, e_aten):
    return e <= max(4.0 * e_aten, gb.DROPOUT_LN_REL)


def _aten_leg(c):
    """ATen's float32 chain on the GPU on the case's inputs -> the same quantities as c['ref']"""
    y, g, b = (c[k].cuda().requires_grad_(True) for k in ('y', 'gamma', 'beta'))
    rm, rv = c['rm'].cuda(), c['rv'].cuda()
    o, mean, rstd = torch.native_batch_norm(y, g, b, rm, rv, True, 0.1, EPS)
    out = torch.relu(o)
    out.backward(c['go'].cuda())
    return dict(out=out, mean=mean, rstd=rstd, rm=rm, rv=rv, dy=y.grad, dgamma=g.grad, dbeta=b.grad)


def _ours(c):
    from occnet_amd import ext
    B, Y, X, Z = c['geom']
    y = c['y'].cuda().view(B, Y, X, Z, 32)
    g, b, rm, rv = (c[k].cuda() for k in ('gamma', 'beta', 'rm', 'rv'))
    mean_rstd = ext.bn3d_relu_train_stats(y, rm, rv, 0.1, EPS)
    out = ext.bn3d_relu_train_fwd(y, mean_rstd, g, b, Z, Y, X)
    gy, _, dgamma, dbeta = ext.bn3d_relu_train_bwd(c['go'].cuda().view(B, Y, X, Z, 32), y, mean_rstd, g, b, Z, Y, X)
    torch.cuda.synchronize()
    return dict(out=out, mean=mean_rstd[0], rstd=mean_rstd[1], rm=rm, rv=rv, dy=gy, dgamma=dgamma, dbeta=dbeta)


def _compare_with_float64(c, label):
    assert c['clear'] >= 1e-3, f"a float64 pre-activation lies {c['clear']:.2e} from zero after conditioning"
    assert c['share'] <= 0.002, f"{100 * c['share']:.3f} % of the elements were nudged"
    ours, aten, ref = _ours(c), _aten_leg(c), c['ref']
    bad = []
    for k in ('out', 'mean', 'rstd', 'rm', 'rv', 'dy', 'dgamma', 'dbeta'):
        e, ea = _rel(ours[k].reshape(ref[k].shape), ref[k]), _rel(aten[k].reshape(ref[k].shape), ref[k])
        print(f"{label} {c['geom']} rows {c['rows']:6d} {k:7s}: kernel {e:.2e}  ATen fp32 {ea:.2e}  (nudged {100 * c['share']:.3f} %)")
        if not _within(e, ea):
            bad.append((k, e, ea))
    assert not bad, bad


@pytest.mark.parametrize("geom", GEOMS)
def test_forward_and_backward_match_float64_autograd(geom):
    """1. out, mean, rstd, the updated running buffers, dy, dgamma, dbeta against relu(F.batch_norm(...)) in float64."""
    _compare_with_float64(_case(geom), "plain")


@pytest.mark.parametrize("geom", [g for g in GEOMS if _rows(g) >= 7])
def test_offset_channels(geom):
    """2. A channel at 300 +- 0.5 and one at -40 +- 0.01: a variance taken as E[y^2] - mean^2 in float32 loses every digit of
    the spread here (errors near 1e-2); ATen float32 itself sits at a few 1e-5 (the mean is a float32 number)."""
    _compare_with_float64(_case(geom, True), "offset")


@pytest.mark.parametrize("rows", [2, 7])
def test_running_statistics(rows):
    """3. momentum 0.1, momentum None (cumulative average) and no tracking, two calls each, against nn.BatchNorm1d in
    float64; the unbiased variance rows / (rows - 1) enters the running buffer."""
    from occnet_amd import ext
    c = _case((1, 1, rows, 1))
    g = torch.Generator().manual_seed(rows)
    batches = [c['y'], c['y'] * 0.7 + 0.3 * torch.randn(rows, 32, generator=g)]
    # the unbiasing on its own: one call with factor 1 leaves running_var = biased variance * rows / (rows - 1)
    rm, rv = torch.zeros(32, device='cuda'), torch.ones(32, device='cuda')
    ext.bn3d_relu_train_stats(batches[0].cuda(), rm, rv, 1.0, EPS)
    var = batches[0].double().var(0, unbiased=False)
    assert _rel(rv, var * rows / (rows - 1)) <= gb.DROPOUT_LN_REL and _rel(rm, batches[0].double().mean(0)) <= gb.DROPOUT_LN_REL
    assert _rel(rv, var) > 0.1          # and it is not the biased one
    for momentum in (0.1, None):
        bn = nn.BatchNorm1d(32, eps=EPS, momentum=momentum).double().train()
        with torch.no_grad():
            bn.running_mean.copy_(c['rm'])
            bn.running_var.copy_(c['rv'])
        rm, rv = c['rm'].cuda(), c['rv'].cuda()
        v0 = rm._version
        for k, y in enumerate(batches):
            bn(y.double())
            eaf = 0.1 if momentum is not None else 1.0 / (k + 1)           # the host's rule (TransformerOcc._bn_eaf)
            ext.bn3d_relu_train_stats(y.cuda(), rm, rv, eaf, EPS)
            e_m, e_v = _rel(rm, bn.running_mean), _rel(rv, bn.running_var)
            print(f"rows {rows} momentum {momentum} call {k}: running_mean {e_m:.2e} running_var {e_v:.2e}")
            assert e_m <= gb.DROPOUT_LN_REL and e_v <= gb.DROPOUT_LN_REL
        assert rm._version > v0 and rv._version > v0      # version-keyed caches (the inference decoder's pack) see the update
    # no tracking: no buffers, the same statistics
    a = ext.bn3d_relu_train_stats(batches[0].cuda(), None, None, 0.0, EPS)
    b = ext.bn3d_relu_train_stats(batches[0].cuda(), torch.zeros(32, device='cuda'), torch.ones(32, device='cuda'), 0.1, EPS)
    assert torch.equal(a, b)
    with pytest.raises(Exception):
        ext.bn3d_relu_train_stats(batches[0].cuda(), torch.zeros(32, device='cuda'), None, 0.1, EPS)


def _raw_bwd(c, xy_major, want_gy, want_gp, mean_rstd):
    """occ_bn3d_relu_train_bwd_f32 on buffers that all start NaN-filled -> (grad_y, grad_y_pad, grad_gamma_beta)"""
    from occnet_amd import _lib
    from occnet_amd._lib import i32, i64, ptr, stream_ptr
    B, Y, X, Z = c['geom']
    dev = torch.device('cuda')
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    y = c['y'].cuda().view(B, Y, X, Z, 32)
    go = c['go'].cuda().view(B, Y, X, Z, 32)
    sb, sy, sx = Y * X * Z * 32, X * Z * 32, Z * 32
    if xy_major:
        go = go.permute(0, 2, 1, 3, 4).contiguous()
        sy, sx = Z * 32, Y * Z * 32
    lib = _lib.lib()
    partial = nan(int(lib.occ_bn3d_relu_train_partial_floats(i64(c['rows']), i32(32))))
    ggb = nan(2, 32)
    gy = nan(B, Y, X, Z, 32) if want_gy else None
    gp = nan(B, Y + 2, X + 2, Z + 2, 32) if want_gp else None
    g, b = c['gamma'].cuda(), c['beta'].cuda()
    rc = lib.occ_bn3d_relu_train_bwd_f32(ptr(go), i64(sb), i64(sy), i64(sx), ptr(y), ptr(mean_rstd), ptr(g), ptr(b), ptr(partial),
                                         ptr(ggb), ptr(gy), ptr(gp), i32(B), i32(Z), i32(Y), i32(X), i32(32), stream_ptr(dev))
    _lib.check(rc, "bn3d_relu_train_bwd")
    torch.cuda.synchronize()
    return gy, gp, ggb


@pytest.mark.parametrize("geom", [(1, 1, 1031, 1), (1, 3, 5, 4), (2, 6, 7, 8), (2, 19, 24, 16)])
def test_layouts_and_completeness(geom):
    """4. The (X, Y)-major output is the permuted contiguous one bit for bit; grad_y_pad is F.pad(grad_y) bit for bit with
    every buffer NaN-filled beforehand; each of grad_y / grad_y_pad is the same without the other; two calls, the same bits."""
    from occnet_amd import _lib, ext
    from occnet_amd._lib import i32, i64, ptr, stream_ptr
    c = _case(geom)
    B, Y, X, Z = geom
    y = c['y'].cuda().view(B, Y, X, Z, 32)
    g, b = c['gamma'].cuda(), c['beta'].cuda()
    mean_rstd = ext.bn3d_relu_train_stats(y, None, None, 0.0, EPS)
    assert torch.equal(mean_rstd, ext.bn3d_relu_train_stats(y, None, None, 0.0, EPS))
    # forward into NaN-filled buffers, both orders
    outs = {}
    for xy in (False, True):
        out = torch.full((B, X, Y, Z, 32) if xy else (B, Y, X, Z, 32), float('nan'), dtype=torch.float32, device='cuda')
        sy, sx = (Z * 32, Y * Z * 32) if xy else (X * Z * 32, Z * 32)
        rc = _lib.lib().occ_bn3d_relu_train_fwd_f32(ptr(y), ptr(mean_rstd), ptr(g), ptr(b), ptr(out), i32(B), i32(Z), i32(Y),
                                                    i32(X), i32(32), i64(Y * X * Z * 32), i64(sy), i64(sx),
                                                    stream_ptr(out.device))
        _lib.check(rc, "bn3d_relu_train_fwd")
        outs[xy] = out
    torch.cuda.synchronize()
    assert not bool(torch.isnan(outs[False]).any())
    assert torch.equal(outs[True], outs[False].permute(0, 2, 1, 3, 4).contiguous())
    assert torch.equal(outs[False], ext.bn3d_relu_train_fwd(y, mean_rstd, g, b, Z, Y, X))
    # backward
    gy, gp, ggb = _raw_bwd(c, False, True, True, mean_rstd)
    for t in (gy, gp, ggb):
        assert not bool(torch.isnan(t).any())
    assert torch.equal(gp, F.pad(gy, (0, 0, 1, 1, 1, 1, 1, 1)))
    gy1, none, ggb1 = _raw_bwd(c, False, True, False, mean_rstd)
    assert none is None and torch.equal(gy1, gy) and torch.equal(ggb1, ggb)
    none, gp1, ggb2 = _raw_bwd(c, False, False, True, mean_rstd)
    assert none is None and torch.equal(gp1, gp) and torch.equal(ggb2, ggb)
    gy2, gp2, ggb3 = _raw_bwd(c, False, True, True, mean_rstd)
    assert torch.equal(gy2, gy) and torch.equal(gp2, gp) and torch.equal(ggb3, ggb)
    # the incoming gradient in the (X, Y)-major order of such an output: the same bits
    gy3, gp3, ggb4 = _raw_bwd(c, True, True, True, mean_rstd)
    assert torch.equal(gy3, gy) and torch.equal(gp3, gp) and torch.equal(ggb4, ggb)


# ---------------------------------------------------------------------------------------------------------- 5. the node

NODE_GEOM = (1, 3, 5, 4)        # (B, Y, X, Z), Cin = 16
NODE_SEED = 0                   # chosen on the CPU: the float64 pre-activations keep 1e-4 clear of zero (asserted below)


def _node_inputs():
    B, Y, X, Z = NODE_GEOM
    g = torch.Generator().manual_seed(NODE_SEED)
    x = torch.randn(B, Y, X, Z, 16, generator=g)
    w = torch.randn(32, 16, 3, 3, 3, generator=g) * (2.0 / (16 * 27)) ** 0.5
    gamma = 1.0 + 0.3 * torch.randn(32, generator=g)
    gamma[3] = -gamma[3].abs() - 0.2
    beta = 0.5 * torch.randn(32, generator=g)
    return x, w, gamma, beta


def _node_ref(l64, return_pre=False):
    x, w, gamma, beta = l64
    y = F.conv3d(x.permute(0, 4, 3, 1, 2), w, padding=1)                        # (B, 32, Z, Y, X)
    pre = F.batch_norm(y, None, None, gamma, beta, True, 0.1, EPS)
    return pre if return_pre else torch.relu(pre).permute(0, 3, 4, 2, 1)       # (B, Y, X, Z, 32)


def _node_run(leaves):
    from occnet_amd import ext
    B, Y, X, Z = NODE_GEOM
    x, w, gamma, beta = leaves
    rm, rv = torch.zeros(32, device=x.device), torch.ones(32, device=x.device)
    return ext.conv3d_bn_relu_autograd(x, w, gamma, beta, rm, rv, 0.1, EPS, Z, Y, X, in_layout=0)


def _node_chain(leaves):
    """the ATen leg: today's decoder layer, Conv3dX3Function -> F.batch_norm -> relu"""
    from occnet_amd import ext
    B, Y, X, Z = NODE_GEOM
    x, w, gamma, beta = leaves
    y = ext.conv3d_autograd(x, w, Z, Y, X, in_layout=0)
    return torch.relu(F.batch_norm(y.view(-1, 32), None, None, gamma, beta, True, 0.1, EPS)).view(B, Y, X, Z, 32)


def _node_spec():
    spec = None

    def make_leaves():
        return [t.clone().cuda() for t in _node_inputs()]

    def chain_leg(what, mask, grad_outs):
        leaves = make_leaves()
        for i in range(4):
            leaves[i].requires_grad_(i in mask)
        out = _node_chain(leaves)
        if what[0] == 'out':
            return out.detach()
        gos = ac.default_grad_outs(spec, [out]) if grad_outs is None else grad_outs
        out.backward(gos[0])
        return leaves[what[1]].grad

    def truth(what, got, ref, mask, grad_outs):
        d, scale = float((got - ref).abs().max()), float(ref.abs().max())
        if len(mask) == 4 and grad_outs is None:
            print(f"node {what}: max abs {d:.2e}, relative {d / (scale + 1e-12):.2e} (max|ref| {scale:.3f})")
        if what == ('grad', 0):
            assert d < gb.CONV3D_DX_ABS, (what, d)
        elif what == ('grad', 1):
            assert d < gb.CONV3D_DW_ABS * max(1.0, scale), (what, d, scale)
        else:
            e, ea = d / (scale + 1e-12), _rel(chain_leg(what, mask, grad_outs), ref)
            if len(mask) == 4 and grad_outs is None:
                print(f"node {what}: today's chain {ea:.2e}")
            assert _within(e, ea), (what, mask, e, ea)

    spec = ac.NodeSpec('Conv3dBNReLUFunction', make_leaves, _node_run, _node_ref, diff=(0, 1, 2, 3), truth=truth,
                       node_name='Conv3dBNReLUFunction')
    return spec


def test_node_seed_keeps_the_mask_stable():
    pre = _node_ref([t.double() for t in _node_inputs()], return_pre=True)
    assert float(pre.abs().min()) >= 1e-4, float(pre.abs().min())


def test_node_contract_masks():
    """5. every requires_grad mask over (x, weight, gamma, beta): truth, presence, mask independence"""
    report = ac.check_masks(_node_spec())
    assert len(report) == 15, report


def test_node_contract_layouts_and_retain_graph():
    spec = _node_spec()
    ac.check_grad_layouts(spec)
    assert ac.check_retain_graph(spec) == 6         # x, weight, y, mean_rstd, gamma, beta: the activation is NOT saved


# ---------------------------------------------------------------------------------------------------------- 6. the module

MODULE_SEED = 109       # of the BEV tensor; chosen on the CPU (see _module_ref)


@functools.lru_cache(maxsize=None)
def _module_parts():
    """A TransformerOcc with a (6, 6) BEV grid and Z = 16 on the CPU, decoder norms with non-trivial affine parameters."""
    from occnet_amd.plugin import build_head
    from tests.util import head_cfg, randomize, small_cfg
    head = build_head(copy.deepcopy(head_cfg(small_cfg(bev=(6, 6), num_layers=1))))
    randomize(head, 4)
    tr = head.transformer
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for m in (tr.decoder[0], tr.decoder[1]):
            m.norm.weight.copy_(1.0 + 0.3 * torch.randn(32, generator=g))
            m.norm.bias.copy_(0.5 * torch.randn(32, generator=g))
        tr.decoder[0].norm.weight[3] = -1.1
    return tr


def _module_inputs(seed=MODULE_SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 36, 256, generator=g), torch.randn(2, 6, 6, 16, 32, generator=g)


def _module_ref(tr, bev, go):
    """float64 restatement of the training decoder on the CPU -> dict of outputs / gradients / buffers, and the smallest
    |pre-activation| of the two layers."""
    Z, H, W = 16, 6, 6
    ps = {}
    for k, m in enumerate((tr.decoder[0], tr.decoder[1])):
        ps[f'w{k}'] = m.conv.weight.detach().double().cpu().requires_grad_(True)
        ps[f'gamma{k}'] = m.norm.weight.detach().double().cpu().requires_grad_(True)
        ps[f'beta{k}'] = m.norm.bias.detach().double().cpu().requires_grad_(True)
        ps[f'rm{k}'] = m.norm.running_mean.detach().double().cpu().clone()
        ps[f'rv{k}'] = m.norm.running_var.detach().double().cpu().clone()
    b64 = bev.double().requires_grad_(True)
    x = b64.view(2, H, W, 256 // Z, Z).permute(0, 3, 4, 1, 2)                   # (B, Cin, Z, H, W): the lifter view
    clear = float('inf')
    for k in range(2):
        pre = F.batch_norm(F.conv3d(x, ps[f'w{k}'], padding=1), ps[f'rm{k}'], ps[f'rv{k}'], ps[f'gamma{k}'], ps[f'beta{k}'],
                           True, 0.1, EPS)
        clear = min(clear, float(pre.detach().abs().min()))
        x = torch.relu(pre)
    out = x.permute(0, 4, 3, 2, 1)                                               # (B, W, H, Z, C)
    out.backward(go.double())
    res = {'out': out.detach(), 'bev': b64.grad}
    for k in range(2):
        res.update({f'w{k}': ps[f'w{k}'].grad, f'gamma{k}': ps[f'gamma{k}'].grad, f'beta{k}': ps[f'beta{k}'].grad,
                    f'rm{k}': ps[f'rm{k}'], f'rv{k}': ps[f'rv{k}']})
    return res, clear


def _module_run(tr_cpu, bev, go, switch, prepare=None):
    tr = copy.deepcopy(tr_cpu).cuda().train()
    tr.train_decoder_fused_bn = switch
    if prepare is not None:
        prepare(tr)
        tr = tr.cuda()
    b = bev.cuda().requires_grad_(True)
    assert tr._train_decoder_ok(b)
    out = tr._train_decoder(b, 6, 6)
    out.backward(go.cuda())
    torch.cuda.synchronize()
    res = {'out': out.detach(), 'bev': b.grad}
    for k, m in enumerate((tr.decoder[0], tr.decoder[1])):
        res.update({f'w{k}': m.conv.weight.grad, f'gamma{k}': getattr(m.norm.weight, 'grad', None),
                    f'beta{k}': getattr(m.norm.bias, 'grad', None),
                    f'rm{k}': m.norm.running_mean, f'rv{k}': m.norm.running_var, f'nbt{k}': m.norm.num_batches_tracked})
    return res, out


def test_module_switch_matches_todays_path():
    """6. TransformerOcc._train_decoder with the switch on against float64, judged by the switch-off path's own error."""
    tr = _module_parts()
    bev, go = _module_inputs()
    ref, clear = _module_ref(tr, bev, go)
    assert clear >= 1e-4, f"a float64 pre-activation lies {clear:.2e} from zero: choose another MODULE_SEED"
    off, out_off = _module_run(tr, bev, go, False)
    on, out_on = _module_run(tr, bev, go, True)
    ac.find_node(out_on, 'Conv3dBNReLUFunction')
    with pytest.raises(AssertionError):
        ac.find_node(out_off, 'Conv3dBNReLUFunction')
    assert out_on.is_contiguous() and out_on.shape == out_off.shape == (2, 6, 6, 16, 32)
    bad = []
    for k in ref:
        e, ea = _rel(on[k], ref[k]), _rel(off[k], ref[k])
        print(f"module {k:7s}: switch on {e:.2e}  switch off {ea:.2e}")
        if not _within(e, ea):
            bad.append((k, e, ea))
    assert not bad, bad
    for k in range(2):          # the statistics updated exactly once
        assert int(on[f'nbt{k}']) == int(off[f'nbt{k}']) == int(tr.decoder[k].norm.num_batches_tracked) + 1


def _eval_second_norm(tr):
    tr.decoder[1].norm.eval()


def _first_norm_without_affine(tr):
    old = tr.decoder[0].norm
    new = nn.BatchNorm3d(32, eps=old.eps, momentum=old.momentum, affine=False)
    new.load_state_dict({k: v for k, v in old.state_dict().items() if k not in ('weight', 'bias')})
    setattr(tr.decoder[0], tr.decoder[0].norm_name, new.train())       # `norm` itself is a read-only property
    assert tr.decoder[0].norm is new


@pytest.mark.parametrize("prepare", [_eval_second_norm, _first_norm_without_affine])
def test_module_switch_leaves_other_norms_to_todays_path(prepare):
    """A norm in eval mode, or one without affine parameters: the switch-on call IS today's path, bit for bit, and the
    statistics update once."""
    tr = _module_parts()
    bev, go = _module_inputs()
    off, _ = _module_run(tr, bev, go, False, prepare)
    on, out_on = _module_run(tr, bev, go, True, prepare)
    with pytest.raises(AssertionError):
        ac.find_node(out_on, 'Conv3dBNReLUFunction')
    for k in off:
        if off[k] is None:
            assert on[k] is None, k
        else:
            assert torch.equal(on[k], off[k]), k
    base = [int(m.norm.num_batches_tracked) for m in (tr.decoder[0], tr.decoder[1])]
    assert int(on['nbt0']) == base[0] + 1
    assert int(on['nbt1']) == base[1] + (0 if prepare is _eval_second_norm else 1)


# ---------------------------------------------------------------------------------------------------------- 7. the step

def test_two_training_steps_with_the_switch_on():
    """7. Two optimiser steps of the reduced head (test_gpu_heads_loss.py's geometry) with the switch on, and with the fused
    heads + loss node on as well: finite losses within 1e-4 relative of the switch-off steps, finite parameters."""
    from occnet_amd import synthetic
    from occnet_amd.plugin import build_head
    from occnet_amd.train import synthetic_targets
    from tests.util import head_cfg, randomize, small_cfg
    g = small_cfg(bev=(20, 20), num_layers=2)
    base = build_head(copy.deepcopy(head_cfg(g)))
    randomize(base, 3)
    feats = [f.cuda() for f in synthetic.make_features(g, seed=3)]
    metas = synthetic.make_img_metas(g)
    sem, flow, mask = (t.cuda() for t in synthetic_targets(g['bev_h'], g['bev_w'], g['pillar_h'], num_classes=17, batch=1,
                                                           seed=0))

    def steps(fused_bn, fused_loss):
        head = copy.deepcopy(base).cuda().train()
        head.fused_loss = fused_loss
        head.transformer.train_decoder_fused_bn = fused_bn
        opt = torch.optim.SGD(head.parameters(), lr=1e-3)
        losses = []
        for k in range(2):
            torch.manual_seed(20 + k)           # dropout masks
            opt.zero_grad(set_to_none=True)
            lp = head.forward_loss(feats, metas, None, sem, flow, mask)
            if k == 0:
                names = _graph_names(lp['loss_occ'].grad_fn)
                assert any(n.startswith('Conv3dBNReLUFunction') for n in names) == fused_bn
            (lp['loss_occ'] + lp['loss_flow']).backward()
            opt.step()
            losses.append({n: float(v.detach()) for n, v in lp.items()})
        assert all(bool(torch.isfinite(p).all()) for p in head.parameters())
        assert all(int(m.norm.num_batches_tracked) == int(b.norm.num_batches_tracked) + 2
                   for m, b in zip(head.transformer.decoder, base.transformer.decoder))
        return losses

    off = steps(False, False)
    for fused_loss in (False, True):
        on = steps(True, fused_loss)
        for k in range(2):
            for n in ('loss_occ', 'loss_flow'):
                a, b = on[k][n], off[k][n]
                print(f"step {k} {n}: switch on (fused_loss {fused_loss}) {a:.7f}  off {b:.7f}")
                assert a == a and abs(a) < float('inf') and abs(a - b) <= 1e-4 * abs(b), (k, n, a, b)


def _graph_names(fn):
    seen, names, queue = set(), [], [fn]
    while queue:
        f = queue.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        queue += [nf for nf, _ in f.next_functions]
    return names
