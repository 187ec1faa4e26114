"""-m gpu: the autograd contract (tests/autograd_contract.py) applied to every hand-written autograd node of the training step.

The per-node parity tests set requires_grad on all inputs at once, so each backward runs one path through its
`ctx.needs_input_grad` branches.  Here every node is run under every requires_grad mask (ConvBNActFunction: every single leaf,
every pair of {weight, gamma, beta}, all-but-one, all — every subset where a case has at most four leaves), against a float64
restatement differentiated under the SAME mask, under the bound that node's own parity test asserts (tests/grad_bounds.py).
Then, full mask: the incoming gradient in other layouts, backward twice over a retained graph, one of two outputs without a
gradient (SCAPrepFunction), inputs that are views of one parent (SCAFusedFunction).  Shapes are small: this file tests the
control flow around the kernels; the kernels' parity at size stays in the per-node tests.

Bit-identity across masks is asserted for every node: the atomic-scatter backward of MSDA / SCA runs in its deterministic mode
(OCC_MSDA_BWD_DETERMINISTIC=1, as tests/test_gpu_backward.py does), MIOpen in its deterministic mode for ConvBNActFunction.

What the sweep ran and found on an MI355X (every mask under the reference bound as well, never bit-identity instead of it;
"bits" = output and gradients bit-identical across masks):

  ConvBNActFunction: 15 masks per case (x, W, gamma, beta), 14 with a residual, 7 without a norm, 16 with all six inputs; bits.  FOUND, in every case
      with a BatchNorm (one-launch fold): W without gamma lost the gamma * rstd factor (relative L2 error 0.44 - 0.49 where the
      autocast chain's is 0.002 - 0.06) and gamma without W got no gradient: 8 of 15 masks (6 of 14) per case.  Fixed in
      ConvBNActFunction.backward.  Also found: ResNet ignored norm_cfg's requires_grad=False.  Fixed.
  SCAFusedFunction: 7 masks (value, offs, logits), 3 with offs / logits as slices of one leaf; bits.  Nothing found.
  MultiScaleDeformableAttnFunction_fp32 / _fp16: 7 masks each (fp16 under autocast; its bound here is the fp32 node's plus one fp16
      rounding, 2^-11; its parity test is tests/test_gpu_msda_edges.py: .half() of the fp32 node bit for bit); bits.  Nothing found.
  Conv3dX3Function: 3 masks, both input layouts, x also as a view of a wider leaf; bits.  Nothing found.
  LinearX3Function: 7 masks with a bias, 3 without, with and without ReLU; bits.  Nothing found.
  LinearWgradFunction: 7 masks with a bias, 3 without (the output and dx are library GEMMs no parity test bounds: the fp32
      dot-product rounding bound); bits.  Nothing found.
  RowsGatherSumFunction: its one mask.  Nothing found.
  SCAPrepFunction: its one mask, with both outputs, loc only and attn only; bits.  Nothing found.
  DropoutAddLayerNormFunction: 15 masks, p = 0 and p = 0.1; bits.  Nothing found in the node; its predicate let misaligned and
      other-device operands through.  Fixed (ext.dropout_add_layernorm_ok), tested at the end of this file.

Gradient layouts (contiguous, stride-0 expansion, permuted, column slice, channels_last) and two backward passes over a retained
graph: bit-identical gradients for every case of every node, saved tensors and outputs unchanged.

Run time, each file in a process of its own, alternating on one MI355X: this file 11.1 / 6.2 / 5.7 s, tests/test_gpu_backbone.py
13.7 / 6.5 / 4.7 s (first pair with cold MIOpen caches); the test bodies of this file sum to under 4 s."""
import pytest
import torch
import torch.nn.functional as F

from tests import autograd_contract as ac
from tests import grad_bounds as gb

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def _max_rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _max_abs(a, b):
    return float((a - b).abs().max())


# ---- ConvBNActFunction

CONV_CASES = [
    # cin, cout, k, stride, bn, res, relu: the cases of test_gpu_backbone.py::test_conv_bn_act_function_matches_the_autocast_chain
    (256, 128, 1, 1, True, False, True),      # bottleneck conv1: own 1x1 kernel
    (128, 128, 3, 2, True, False, True),      # conv2, stride 2: own 3x3 kernel
    (128, 512, 1, 1, True, True, True),       # conv3 + identity + ReLU: own 1x1 kernel with residual
    (256, 512, 1, 2, True, False, False),     # downsample projection
    (64, 64, 3, 1, True, False, True),        # a shape without an own kernel: MIOpen + the fused tail
    (512, 256, 1, 1, False, False, False),    # FPN lateral: bias, no norm
    (256, 256, 3, 1, False, False, False),    # FPN output convolution
    # beyond those seven: a biased convolution WITH a norm and a residual — all six differentiable inputs at once, and the
    # node's other fold (ATen expressions instead of the one-launch kernels, forward and backward)
    (64, 128, 1, 1, True, True, True, True)]
CONV_IDS = ["conv1_1x1", "conv2_3x3_s2", "conv3_residual", "downsample_s2", "no_own_kernel", "fpn_lateral", "fpn_output",
            "norm_and_bias_all_six_leaves"]


def _conv_spec(cin, cout, k, stride, bn, res, relu, conv_bias=None):
    """gamma from U(0.5, 2) and the running variance from U(0.25, 4): a missing gamma * rstd factor is an O(1) relative error,
    nowhere near a bf16-sized bound."""
    from occnet_amd.plugin.backbone import ConvBNActFunction
    conv_bias = (not bn) if conv_bias is None else conv_bias
    g = torch.Generator().manual_seed(cin + cout + k)
    cl = lambda t: t.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    N, H, W = 2, 12, 20
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    eps = 1e-5
    base = [cl(torch.randn(N, cin, H, W, generator=g)),
            (torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5).to(DEV),
            (torch.rand(cout, generator=g) * 1.5 + 0.5).to(DEV) if bn else None,
            (torch.randn(cout, generator=g) * 0.1).to(DEV) if bn else None,
            (torch.randn(cout, generator=g) * 0.1).to(DEV) if conv_bias else None,
            cl(torch.randn(N, cout, Ho, Wo, generator=g)) if res else None]
    mean = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    var = (torch.rand(cout, generator=g) * 3.75 + 0.25).to(DEV)
    rstd = torch.rsqrt(var + eps)
    mean_rstd = mean * rstd
    stride2, pad2 = (stride, stride), (k // 2, k // 2)
    diff = tuple(i for i, t in enumerate(base) if t is not None)

    def make_leaves():
        return [None if t is None else t.clone(memory_format=torch.preserve_format) for t in base]

    def run(l):
        with torch.autocast('cuda', dtype=torch.bfloat16):
            return ConvBNActFunction.apply(l[0], l[1], l[2], l[3], rstd if bn else None, mean_rstd if bn else None, l[4], l[5],
                                           stride2, pad2, relu)

    def chain(l, mean_, var_):
        """The function the node replaces: conv_bn_folded (or the biased convolution) -> + residual -> ReLU."""
        y = ac.folded_conv_bn(l[0], l[1], l[2], l[3], l[4], mean_, var_, eps, stride2, pad2)
        if l[5] is not None:
            y = y + l[5]
        return torch.relu(y) if relu else y

    def ref(l64):
        return chain(l64, mean.double().cpu(), var.double().cpu())

    chain_runs = {}

    def autocast_chain(mask, grad_outs):
        """The same chain under torch.autocast(bf16) on the device, same mask, same incoming gradient: its error against the
        float64 chain is the yardstick of the node's bound."""
        key = (mask, None if grad_outs is None else id(grad_outs))
        if key not in chain_runs:
            l = make_leaves()
            for i in diff:
                l[i].requires_grad_(i in mask)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                y = chain(l, mean, var)
            assert y.dtype == torch.bfloat16
            go = ac.default_grad_outs(spec, [y])[0] if grad_outs is None else grad_outs[0]
            y.backward(go.to(torch.bfloat16))
            chain_runs[key] = (grad_outs, y.detach(), {i: l[i].grad for i in diff})
        return chain_runs[key][1:]

    def truth(what, got, ref_, mask, grad_outs):
        y, grads = autocast_chain(mask, grad_outs)
        c = (y if what[0] == 'out' else grads[what[1]]).double().cpu()
        ef, ec = _rel_l2(got, ref_), _rel_l2(c, ref_)
        print(f"    conv_bn_act {what} mask {mask}: fused {ef:.3e}  autocast chain {ec:.3e}")
        assert gb.conv_bn_act_within_bound(ef, ec), f"relative L2 error {ef:.3e} (the autocast chain's: {ec:.3e})"

    spec = ac.NodeSpec(f"ConvBNAct({cin}->{cout} k{k} s{stride} bn={bn} res={res} relu={relu})", make_leaves, run, ref, diff, truth,
                       node_name='ConvBNActFunction')
    return spec


@pytest.fixture
def deterministic_convolutions():
    """MIOpen's deterministic mode: the data / weight gradients of one problem are the same bits whichever of them a mask
    asks for."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv_bn_act_masks(case, deterministic_convolutions):
    spec = _conv_spec(*case)
    masks = ac.conv_bn_act_masks(spec.diff)
    assert len(masks) == {3: 7, 4: 15, 5: 1 + 5 + 3 + 5, 6: 1 + 6 + 3 + 6}[len(spec.diff)]
    report = ac.check_masks(spec, masks)
    assert len(report) == len(masks) and set(report.values()) == {'full mask', 'bit-identical'}


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv_bn_act_gradient_layouts_and_retained_graph(case, deterministic_convolutions):
    """bias_act_nhwc_ works in place on the convolution output that the node then saves for its ReLU mask: nothing may write it
    again (the retained-graph check compares the saved tensors and the output before and after two backward passes)."""
    spec = _conv_spec(*case)
    ac.check_grad_layouts(spec)
    n_saved = ac.check_retain_graph(spec)
    assert n_saved >= 3


# ---- the other nine nodes: one spec factory per case

def _msda_spec(half, B, shapes, M, D, Lq, P):
    from occnet_amd.plugin import functions
    from oracle.msda import multi_scale_deformable_attn_pytorch
    from tests.test_gpu_backward import _interior
    from tests.test_gpu_msda import _inputs
    Fn = functions.MultiScaleDeformableAttnFunction_fp16 if half else functions.MultiScaleDeformableAttnFunction_fp32
    value, shapes_t, start, loc, attn = _inputs(B, shapes, M, D, Lq, P, seed=8, adversarial=False)
    loc = _interior(loc, shapes)
    if half:        # keep the interior property after the cast the node applies
        loc = _interior(loc.half().float(), shapes).half().float()
    base = [value.to(DEV), loc.to(DEV), attn.to(DEV)]
    sd, st = shapes_t.to(DEV), start.to(DEV)

    def run(l):
        if not half:
            return Fn.apply(l[0], sd, st, l[1], l[2], 64)
        with torch.autocast('cuda', dtype=torch.float16):       # custom_fwd(cast_inputs=float16) casts under autocast only
            out = Fn.apply(l[0], sd, st, l[1], l[2], 64)
        assert out.dtype == torch.float16
        return out

    def ref(l):
        if half:    # the node sees the inputs rounded to fp16 (straight-through: the cast's derivative is the identity)
            l = [t + (t.detach().half().double() - t.detach()) for t in l]
        return multi_scale_deformable_attn_pytorch(l[0], shapes_t, l[1], l[2])

    # fp16: every tensor the node returns is rounded to fp16 once (2^-11 relative) on top of the fp32 node's bound
    tol = gb.MSDA_GRAD_TOL + (2.0 ** -11 if half else 0.0)

    def truth(what, got, ref_, mask, grad_outs):
        d = _max_abs(got, ref_) / max(1.0, float(ref_.abs().max()))
        assert d < tol, f"max diff / max(1, max|ref|) = {d:.3e}"
    return ac.NodeSpec(f"MSDA_{'fp16' if half else 'fp32'}", lambda: [t.clone() for t in base], run, ref, (0, 1, 2), truth,
                       node_name='MultiScaleDeformableAttnFunction')


def _sca_case(B, L, P):
    from tests.test_gpu_sca_fused_backward import _case
    return _case(B, L, P, Nq=64, NC=3, seed=B * 10 + L + P)


def _sca_reference(c, value, offs, logits):
    """The restatement of tests/test_gpu_sca_fused_backward.py (per-camera multi_scale_deformable_attn_pytorch, softmax, offset
    normalisation, z-anchor pairing, batch 0's camera choice, mean over each batch's own visible cameras) on given leaves."""
    from oracle.msda import multi_scale_deformable_attn_pytorch
    from tests.test_gpu_sca_fused_backward import D, M
    B, L, P, Nq, NC, Z = c['B'], c['L'], c['P'], c['Nq'], c['NC'], c['Z']
    offs = offs.reshape(B, Nq, M, L, P // Z, Z, 2)
    aw = logits.reshape(B, Nq, M, L * P).softmax(-1).view(B, Nq, M, L, P)
    norm = torch.stack([c['shapes'][:, 1], c['shapes'][:, 0]], -1).double()      # (W, H)
    off = offs / norm[None, None, None, :, None, None, :]
    vis = c['vis'].to(torch.int64)
    slots = 0
    for cam in range(NC):
        ref_c = c['ref_cam'][cam].double()
        loc = (ref_c[:, :, None, None, None, :, :] + off).view(B, Nq, M, L, P, 2)
        out = multi_scale_deformable_attn_pytorch(value[cam::NC], c['shapes'], loc, aw)
        slots = slots + out * ((vis[0] >> cam) & 1).double()[None, :, None]
    count = sum(((vis >> cam) & 1).double() for cam in range(NC))
    return slots / count.clamp(min=1.0)[..., None]


def _sca_truth(what, got, ref_, mask, grad_outs):
    d, scale = _max_abs(got, ref_), float(ref_.abs().max())
    assert scale > 0.0 and d <= gb.SCA_FUSED_GRAD_REL * scale + gb.SCA_FUSED_GRAD_ABS, f"max diff {d:.3e}, max|ref| {scale:.3e}"


def _sca_spec(B, L, P, views=False):
    """views: offs and logits are column slices of ONE leaf (a wider Linear output, 8 spare columns), as the node's docstring
    promises: the leaf's gradient is what autograd assembles from the two slices' gradients."""
    from occnet_amd import ext
    from tests.test_gpu_sca_fused_backward import M
    c = _sca_case(B, L, P)
    n_off, n_att = c['n_off'], c['n_att']
    lin = c['lin'].to(DEV)
    consts = [c[k].to(DEV) for k in ('ref_cam', 'vis', 'shapes', 'starts')]
    if views:
        base = [c['value'].to(DEV), lin]
        split = lambda l: (l[0], l[1][..., :n_off], l[1][..., n_off:n_off + n_att])
    else:
        base = [c['value'].to(DEV), lin[..., :n_off].contiguous(), lin[..., n_off:n_off + n_att].contiguous()]
        split = lambda l: tuple(l)

    def run(l):
        value, offs, logits = split(l)
        if views:
            assert not offs.is_contiguous() and not logits.is_contiguous()
        return ext.SCAFusedFunction.apply(value, offs, logits, *consts, M, L, P)
    return ac.NodeSpec(f"SCAFused(B={B} L={L} P={P}{' views' if views else ''})", lambda: [t.clone() for t in base], run,
                       lambda l: _sca_reference(c, *split(l)), tuple(range(len(base))), _sca_truth, node_name='SCAFusedFunction')


def _conv3d_spec(B, Z, Y, X, Cin, layout, view_input=False):
    """view_input (layout 1): x is a column slice of a wider leaf, so the node saves a non-contiguous tensor."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(71)
    x = torch.randn(B, Cin, Z, Y, X, generator=g)
    w = torch.randn(32, Cin, 3, 3, 3, generator=g) * (2.0 / (Cin * 27)) ** 0.5
    xin = x.permute(0, 3, 4, 2, 1).contiguous() if layout == 0 else x.permute(0, 3, 4, 1, 2).reshape(B, Y * X, Cin * Z).contiguous()
    base = [xin.to(DEV), w.to(DEV)]
    if view_input:
        assert layout == 1
        base[0] = torch.cat([base[0], torch.randn(B, Y * X, 8, generator=g).to(DEV)], -1)
    cut = (lambda t: t[..., :Cin * Z]) if view_input else (lambda t: t)

    def ref(l):
        x5 = cut(l[0])
        x5 = x5.permute(0, 4, 3, 1, 2) if layout == 0 else x5.reshape(B, Y, X, Cin, Z).permute(0, 3, 4, 1, 2)   # (B, Cin, Z, Y, X)
        return F.conv3d(x5, l[1], padding=1).permute(0, 3, 4, 2, 1)                                           # (B, Y, X, Z, 32)

    def truth(what, got, ref_, mask, grad_outs):
        d = _max_abs(got, ref_)
        bound = gb.CONV3D_OUT_ABS if what[0] == 'out' else gb.CONV3D_DX_ABS if what[1] == 0 else \
            gb.CONV3D_DW_ABS * max(1.0, float(ref_.abs().max()))
        assert d < bound, f"max diff {d:.3e} (bound {bound:.1e})"
    return ac.NodeSpec(f"Conv3dX3(Z={Z} Cin={Cin} layout={layout})", lambda: [t.clone() for t in base],
                       lambda l: ext.conv3d_autograd(cut(l[0]), l[1], Z, Y, X, in_layout=layout), ref, (0, 1), truth,
                       node_name='Conv3dX3Function')


def _linear_x3_spec(rows, K, N, act, bias):
    from occnet_amd import ext
    g = torch.Generator().manual_seed(63 + rows)
    base = [torch.randn(rows, K, generator=g).to(DEV), (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV),
            (torch.randn(N, generator=g) * 0.1).to(DEV) if bias else None]
    state = {}

    def run(l):
        y = ext.linear_autograd(l[0], l[1], l[2], act=act)
        assert type(y.grad_fn).__name__.startswith("LinearX3Function")
        state['y'] = y.detach()
        return y

    def ref(l):
        yr = F.linear(l[0], l[1], l[2])
        if act == 'relu':
            # the node's contract: the backward masks with the forward's own output (test_gpu_linear.py, same reference)
            mask = (state['y'].cpu() > 0).double()
            flips = int((mask - (yr.detach() > 0).double()).abs().sum())
            assert flips <= max(2, int(1e-4 * mask.numel())), flips
            yr = yr * mask
        return yr

    def truth(what, got, ref_, mask, grad_outs):
        e = _max_rel(got, ref_)
        assert e < gb.LINEAR_X3_REL, f"max-norm relative error {e:.3e}"
    return ac.NodeSpec(f"LinearX3(rows={rows} {K}->{N} act={act} bias={bias})", lambda: [None if t is None else t.clone() for t in base],
                       run, ref, (0, 1, 2) if bias else (0, 1), truth, node_name='LinearX3Function')


def _linear_wgrad_spec(rows, K, N, bias):
    """The weight / bias gradients come from linear_wgrad (its bounds); the output and dx are fp32 library GEMMs, which no parity
    test bounds: for those, the rounding-error bound of an n-term fp32 dot product in any order, |err| <= n * 2^-23 * sum |terms|
    per element (twice the textbook gamma_n = n * 2^-24 / (1 - n * 2^-24))."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(64 + rows)
    base = [torch.randn(rows, K, generator=g).to(DEV), (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV),
            (torch.randn(N, generator=g) * 0.1).to(DEV) if bias else None]
    x64, w64 = base[0].double().cpu(), base[1].double().cpu()

    def truth(what, got, ref_, mask, grad_outs):
        if what == ('grad', 1) or what == ('grad', 2):
            e, tol = _max_rel(got, ref_), gb.LINEAR_WGRAD_DW_REL if what[1] == 1 else gb.LINEAR_WGRAD_DB_REL
            assert e < tol, f"max-norm relative error {e:.3e}"
            return
        if what[0] == 'out':
            mag, n = x64.abs() @ w64.abs().t() + (0.0 if not bias else base[2].double().cpu().abs()), K + 1
        else:
            go = ac.default_grad_outs(spec, [ref_.new_zeros(rows, N)])[0] if grad_outs is None else grad_outs[0].double().cpu()
            mag, n = go.abs() @ w64.abs(), N
        excess = float(((got - ref_).abs() - n * 2.0 ** -23 * mag).max())
        assert excess <= 0.0, f"an element exceeds the fp32 dot-product bound by {excess:.3e}"
    spec = ac.NodeSpec(f"LinearWgrad(rows={rows} {K}->{N} bias={bias})", lambda: [None if t is None else t.clone() for t in base],
                       lambda l: ext.LinearWgradFunction.apply(l[0], l[1], l[2]), lambda l: F.linear(l[0], l[1], l[2]),
                       (0, 1, 2) if bias else (0, 1), truth, node_name='LinearWgradFunction')
    return spec


def _row_maps(g, Q, nc, keep):
    """The rebatch maps of the SCA training path (tests/test_gpu_training.py): row -> query with -1 padding, query -> rows."""
    lists = [torch.nonzero(torch.rand(Q, generator=g) > keep).squeeze(-1) for _ in range(nc)]
    max_len = max(len(l) for l in lists)
    r2q = torch.full((nc * max_len, 1), -1, dtype=torch.long)
    for i, l in enumerate(lists):
        r2q[i * max_len:i * max_len + len(l), 0] = l
    kmax = max(int(torch.bincount(torch.cat(lists), minlength=Q).max()), 1)
    q2r = torch.full((Q, kmax), -1, dtype=torch.long)
    fill = [0] * Q
    for i, l in enumerate(lists):
        for j, q in enumerate(l.tolist()):
            q2r[q, fill[q]] = i * max_len + j
            fill[q] += 1
    return r2q, q2r


def _rows_gather_spec():
    from occnet_amd import ext
    g = torch.Generator().manual_seed(11)
    Q, nc, Fdim = 120, 4, 64
    r2q, q2r = _row_maps(g, Q, nc, 0.55)
    base = [torch.randn(2, Q, Fdim, generator=g).to(DEV)]
    valid = (r2q[:, 0] >= 0).double().view(1, -1, 1)
    r2q_d, q2r_d = r2q.to(DEV), q2r.to(DEV)

    def truth(what, got, ref_, mask, grad_outs):
        d = _max_abs(got, ref_)
        assert (d == gb.ROWS_GATHER_OUT_ABS) if what[0] == 'out' else (d < gb.ROWS_GATHER_GRAD_ABS), f"max diff {d:.3e}"
    return ac.NodeSpec("RowsGatherSum", lambda: [t.clone() for t in base],
                       lambda l: ext.RowsGatherSumFunction.apply(l[0], r2q_d, q2r_d),
                       lambda l: l[0].index_select(1, r2q[:, 0].clamp(min=0)) * valid, (0,), truth,
                       node_name='RowsGatherSumFunction')


def _sca_prep_spec():
    from occnet_amd import ext
    g = torch.Generator().manual_seed(12)
    bs, Q, nc, M, L, P, Z = 2, 60, 3, 8, 4, 8, 4
    r2q, q2r = _row_maps(g, Q, nc, 0.5)
    R = r2q.shape[0]
    shapes = torch.tensor([[20, 30], [10, 15], [5, 8], [3, 4]])
    base = [torch.randn(bs, Q, 3 * M * L * P, generator=g).to(DEV)]
    ref_rb = torch.rand(bs, R, Z, 2, generator=g)
    consts = [r2q.to(DEV), q2r.to(DEV), ref_rb.to(DEV), shapes.to(DEV)]
    valid = (r2q[:, 0] >= 0).double().view(1, R, 1)
    n_off = M * L * P * 2

    def ref(l):
        rb = l[0].index_select(1, r2q[:, 0].clamp(min=0)) * valid
        off = rb[..., :n_off].reshape(bs, R, M, L, P, 2)
        att = rb[..., n_off:].reshape(bs, R, M, L * P).softmax(-1).view(bs, R, M, L, P)
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
        off = off / norm[None, None, None, :, None, :]
        loc = ref_rb.double()[:, :, None, None, None, :, :] + off.view(bs, R, M, L, P // Z, Z, 2)
        return loc.view(bs, R, M, L, P, 2), att

    def truth(what, got, ref_, mask, grad_outs):
        if what[0] == 'out':
            d, tol = _max_abs(got, ref_), (gb.SCA_PREP_LOC_ABS, gb.SCA_PREP_ATTN_ABS)[what[1]]
        else:
            d, tol = _max_rel(got, ref_), gb.SCA_PREP_GRAD_REL
        assert d < tol, f"{d:.3e} (bound {tol:.1e})"
    return ac.NodeSpec("SCAPrep", lambda: [t.clone() for t in base], lambda l: ext.SCAPrepFunction.apply(l[0], *consts, M, L, P), ref,
                       (0,), truth, node_name='SCAPrepFunction')


def _dropout_ln_spec(rows, p):
    """The keep mask is a counter-based hash of (seed, element index); the seed comes from torch's CPU generator, so seeding it
    before every run gives every mask the same dropout pattern, restated on the host by tests/test_gpu_training.py::_keep_mask."""
    from occnet_amd import ext
    from tests.test_gpu_training import _keep_mask
    g = torch.Generator().manual_seed(rows)
    C = 256
    base = [torch.randn(1, rows, C, generator=g).to(DEV), torch.randn(1, rows, C, generator=g).to(DEV),
            (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)]
    eps = 1e-5
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())      # the draw the node makes after manual_seed(77)
    keep = torch.ones(1, rows, C, dtype=torch.float64)
    if p > 0:
        keep = torch.from_numpy(_keep_mask(rows * C, seed, p).astype('float64')).view(1, rows, C) / (1 - p)

    def truth(what, got, ref_, mask, grad_outs):
        e = _max_rel(got, ref_)
        assert e < gb.DROPOUT_LN_REL, f"max-norm relative error {e:.3e}"
    return ac.NodeSpec(f"DropoutAddLayerNorm(rows={rows} p={p})", lambda: [t.clone() for t in base],
                       lambda l: ext.DropoutAddLayerNormFunction.apply(l[0], l[1], l[2], l[3], eps, p),
                       lambda l: F.layer_norm(l[0] * keep + l[1], (C,), l[2], l[3], eps), (0, 1, 2, 3), truth,
                       node_name='DropoutAddLayerNormFunction', before_run=lambda: torch.manual_seed(77))


NODE_CASES = {
    "msda_fp32_two_levels": lambda: _msda_spec(False, 2, [[10, 14], [5, 7]], 8, 32, 64, 4),
    "msda_fp32_ragged_items": lambda: _msda_spec(False, 1, [[5, 7], [3, 4]], 3, 32, 13, 5),
    "msda_fp16_two_levels": lambda: _msda_spec(True, 2, [[10, 14], [5, 7]], 8, 32, 64, 4),
    "sca_fused_b1_l4_p8": lambda: _sca_spec(1, 4, 8),
    "sca_fused_b1_l2_p8": lambda: _sca_spec(1, 2, 8),
    "sca_fused_views_b2_l4_p4": lambda: _sca_spec(2, 4, 4, views=True),
    "conv3d_layout1_cin16": lambda: _conv3d_spec(1, 16, 5, 7, 16, 1),
    "conv3d_layout1_cin16_view_input": lambda: _conv3d_spec(1, 16, 5, 7, 16, 1, view_input=True),
    "conv3d_layout0_cin32": lambda: _conv3d_spec(2, 16, 4, 6, 32, 0),
    "conv3d_layout1_cin8": lambda: _conv3d_spec(1, 32, 3, 5, 8, 1),
    "conv3d_layout0_cin64": lambda: _conv3d_spec(1, 4, 6, 9, 64, 0),
    "linear_x3_rows5_relu_bias": lambda: _linear_x3_spec(5, 256, 64, 'relu', True),
    "linear_x3_rows4003_bias": lambda: _linear_x3_spec(4003, 256, 64, None, True),
    "linear_x3_rows4099_relu_nobias": lambda: _linear_x3_spec(4099, 64, 256, 'relu', False),
    "linear_x3_rows5_nobias": lambda: _linear_x3_spec(5, 64, 256, None, False),
    "linear_wgrad_rows4099_bias": lambda: _linear_wgrad_spec(4099, 64, 17, True),
    "linear_wgrad_rows4003_nobias": lambda: _linear_wgrad_spec(4003, 64, 2, False),
    "linear_wgrad_rows5_bias": lambda: _linear_wgrad_spec(5, 64, 17, True),
    "rows_gather_sum": _rows_gather_spec,
    "sca_prep": _sca_prep_spec,
    "dropout_ln_rows5_p0.1": lambda: _dropout_ln_spec(5, 0.1),
    "dropout_ln_rows4003_p0": lambda: _dropout_ln_spec(4003, 0.0),
    "dropout_ln_rows4099_p0.1": lambda: _dropout_ln_spec(4099, 0.1),
}


@pytest.fixture
def deterministic_scatter(monkeypatch):
    monkeypatch.setenv("OCC_MSDA_BWD_DETERMINISTIC", "1")


@pytest.mark.parametrize("case", list(NODE_CASES), ids=list(NODE_CASES))
def test_node_masks(case, deterministic_scatter):
    """Every non-empty requires_grad subset: truth under the same mask, presence, bit-identical output and gradients."""
    spec = NODE_CASES[case]()
    report = ac.check_masks(spec)
    assert len(report) == 2 ** len(spec.diff) - 1
    assert set(report.values()) <= {'full mask', 'bit-identical'}


@pytest.mark.parametrize("case", list(NODE_CASES), ids=list(NODE_CASES))
def test_node_gradient_layouts_and_retained_graph(case, deterministic_scatter):
    spec = NODE_CASES[case]()
    ac.check_grad_layouts(spec)
    ac.check_retain_graph(spec)


@pytest.mark.parametrize("use", [(0,), (1,)], ids=["loss_on_loc_only", "loss_on_attn_only"])
def test_sca_prep_with_one_output_unused(use):
    """A loss that reads one of the node's two outputs: the other's gradient never arrives; the gradient of proj is the
    reference's (loc only: the logit columns get exactly zero; attn only: the offset columns do)."""
    spec = _sca_prep_spec()
    ac.check_masks(spec, use_outputs=use)
    _, grads = ac.run_node(spec, (0,), use_outputs=use)
    n_off = 8 * 4 * 8 * 2
    dead = grads[0][..., n_off:] if use == (0,) else grads[0][..., :n_off]
    assert float(dead.abs().max()) == 0.0


# ---- module level: ResNet-50 + FPN with part of the parameters frozen

def _frozen_backbone(kind):
    from occnet_amd.plugin.backbone import ResNet
    torch.manual_seed(0)
    norm_cfg = dict(type='BN', requires_grad=kind != 'frozen_norm_affine')
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_cfg=norm_cfg, norm_eval=True)
    bb.init_weights()
    g = torch.Generator().manual_seed(1)
    for m in bb.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.75)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    if kind == 'frozen_layer3_conv_weights':
        for m in bb.layer3.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.requires_grad_(False)
    return bb.to(DEV).train(), g


@pytest.mark.parametrize("kind", ["frozen_norm_affine", "frozen_layer3_conv_weights"])
def test_partly_frozen_backbone_fused_nodes_match_the_autocast_modules(kind):
    """test_gpu_backbone.py::test_training_backbone_fused_nodes_match_the_autocast_modules with (a) norm_cfg=dict(type='BN',
    requires_grad=False), the frozen-BN-affine fine-tuning set-up, and (b) every convolution weight of layer3 frozen, the norms
    trainable: the fused nodes against the module graph they replace, same bounds; exactly the parameters with requires_grad
    have a gradient, on both sides."""
    from occnet_amd.plugin.backbone import FPN, Bottleneck
    bb, g = _frozen_backbone(kind)
    neck = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output', num_outs=4,
               relu_before_extra_convs=True).to(DEV).train()
    named = {pre + k: v for m, pre in ((bb, 'bb.'), (neck, 'neck.')) for k, v in m.named_parameters()}
    want = {n for n, p in named.items() if p.requires_grad}
    bn_affine = {n for n in named if '.bn' in n or 'downsample.1.' in n or n.startswith('bb.bn1.')}
    if kind == 'frozen_norm_affine':
        assert bn_affine and not (bn_affine & want) and len(want) > 40
    else:
        assert 'bb.layer3.0.conv1.weight' not in want and 'bb.layer3.0.bn1.weight' in want and 'bb.layer2.0.conv1.weight' in want
    x = (torch.randn(2, 3, 96, 160, generator=g) * 50.0).to(DEV)
    res = {}
    for fused in (True, False):
        Bottleneck.fused_train_nodes = fused
        try:
            bb.zero_grad(set_to_none=True)
            neck.zero_grad(set_to_none=True)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                outs = neck(bb(x))
            sum((o.float() ** 2).mean() for o in outs).backward()
            res[fused] = ([o.detach().float() for o in outs],
                          {n: p.grad.detach().float().clone() for n, p in named.items() if p.grad is not None})
        finally:
            Bottleneck.fused_train_nodes = True
    assert set(res[True][1]) == want and set(res[False][1]) == want
    for a, b in zip(res[True][0], res[False][0]):
        assert float((a - b).abs().max() / b.abs().max()) < gb.BACKBONE_FUSED_OUT_REL
    rel = sorted((float((res[True][1][n] - gr).abs().max() / (gr.abs().max() + 1e-12)), n) for n, gr in res[False][1].items())
    print(f"{kind}: relative gradient difference worst {rel[-1][0]:.2e} ({rel[-1][1]}), median {rel[len(rel) // 2][0]:.2e}")
    assert rel[len(rel) // 2][0] < gb.BACKBONE_FUSED_GRAD_MEDIAN_REL and rel[-1][0] < gb.BACKBONE_FUSED_GRAD_WORST_REL


# ---- ext.dropout_add_layernorm_ok on the device: the sites it refuses keep their ATen tail

def test_layernorm_tail_falls_back_for_operands_the_kernel_cannot_read(monkeypatch):
    """gamma / beta as an offset view of a flat parameter buffer (flat[1:257]: dense, 4 bytes off a float4 boundary), a strided
    weight, a residual on the host: the predicate says no, the FFN site takes its ATen tail (the fused node is never entered:
    the misaligned operands are not shown to the kernel) and the layer's result is torch.nn.functional.layer_norm's."""
    from occnet_amd import ext
    from occnet_amd.plugin.bricks import FFN
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 37, 256, generator=g).to(DEV).requires_grad_(True)
    good = torch.nn.LayerNorm(256).to(DEV)
    assert ext.dropout_add_layernorm_ok(x, x, good)
    flat = torch.randn(1024, generator=g).to(DEV)
    offset = torch.nn.LayerNorm(256).to(DEV)
    offset.weight = torch.nn.Parameter(flat[1:257])
    offset.bias = torch.nn.Parameter(flat[513:769])
    assert offset.weight.is_contiguous() and offset.weight.data_ptr() % 16 == 4
    strided = torch.nn.LayerNorm(256).to(DEV)
    strided.weight = torch.nn.Parameter(flat[::2][:256])
    assert not strided.weight.is_contiguous()
    assert not ext.dropout_add_layernorm_ok(x, x, offset)
    assert not ext.dropout_add_layernorm_ok(x, x, strided)
    assert not ext.dropout_add_layernorm_ok(x, x.detach().cpu(), good)
    bias_only = torch.nn.LayerNorm(256).to(DEV)
    bias_only.bias = torch.nn.Parameter(flat[513:769])
    assert not ext.dropout_add_layernorm_ok(x, x, bias_only)
    assert not ext.dropout_add_layernorm_ok(flat[1:257].view(1, 256), flat[:256].view(1, 256), good)     # x itself misaligned

    def never(*a, **k):
        raise AssertionError("the fused LayerNorm node was entered for operands it cannot read")
    ffn = FFN(embed_dims=256, feedforward_channels=512, ffn_drop=0.0).to(DEV).train()
    out_good, normed = ffn(x, post_norm_train=good)
    assert normed is True
    monkeypatch.setattr(ext.DropoutAddLayerNormFunction, "apply", never)
    for ln in (offset, strided):
        out, normed = ffn(x, post_norm_train=ln)
        assert normed is False                                   # the caller applies its norm: the ATen tail
        y = ln(out)
        h = ffn.layers[1](ffn.layers[0][0](x, act='relu'))
        want = F.layer_norm((x + h).double(), (256,), ln.weight.double(), ln.bias.double(), ln.eps)
        assert _max_rel(y.detach().double(), want.detach()) < gb.DROPOUT_LN_REL
        y.sum().backward()
        assert ln.weight.grad is not None and bool(torch.isfinite(ln.weight.grad).all())
