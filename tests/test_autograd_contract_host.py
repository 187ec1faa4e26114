"""No GPU needed: the pieces the autograd contract sweep (tests/test_gpu_autograd_contract.py) stands on.

 - conv_bn_folded, the restatement the ConvBNActFunction truth is built on, against nn.Conv2d -> nn.BatchNorm2d.eval() in
   float64 autograd under every requires_grad mask the sweep uses;
 - the harness itself on a toy autograd.Function: the correct node passes, each planted fault is reported by the check meant
   for it;
 - the alignment / density half of ext.dropout_add_layernorm_ok."""
import pytest
import torch

from tests import autograd_contract as ac


# ---- conv_bn_folded under partial masks

def _conv_bn_case(cin, cout, k, stride, conv_bias, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, dtype=torch.float64) * (hi - lo) + lo
    return dict(x=r(2, cin, 9, 11), weight=r(cout, cin, k, k) * (cin * k * k) ** -0.5, gamma=u(0.5, 2.0, cout),
                beta=r(cout) * 0.1, conv_bias=r(cout) * 0.1 if conv_bias else None, mean=r(cout) * 0.1,
                var=u(0.25, 4.0, cout), gy=r(2, cout, (9 - 1) // stride + 1, (11 - 1) // stride + 1), stride=stride, k=k)


@pytest.mark.parametrize("cin,cout,k,stride,conv_bias", [(32, 64, 3, 2, False), (16, 24, 1, 1, True)])
def test_conv_bn_folded_matches_conv_then_batchnorm_under_every_mask(cin, cout, k, stride, conv_bias):
    """Same function, different association, float64: outputs and gradients to 1e-10 relative, and both sides leave exactly the
    frozen leaves without a gradient.  Three ways: the modules, conv_bn_folded on the modules, and conv_bn_folded on bare
    tensors (ac.folded_conv_bn, what the GPU sweep differentiates)."""
    c = _conv_bn_case(cin, cout, k, stride, conv_bias, seed=cin + cout)
    from occnet_amd.plugin.backbone import conv_bn_folded
    names = ['x', 'weight', 'gamma', 'beta'] + (['conv_bias'] if conv_bias else [])
    present = [ac.CONV_BN_ACT_LEAVES.index(n) for n in names]
    masks = ac.conv_bn_act_masks(present)
    assert len(masks) == (15 if not conv_bias else 1 + 5 + 3 + 5)
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-300))
    worst = 0.0
    for mask in masks:
        on = {ac.CONV_BN_ACT_LEAVES[i] for i in mask}
        res = {}
        for mode in ("modules", "folded_modules", "folded_tensors"):
            t = {n: c[n].clone().requires_grad_(n in on) for n in names}
            if mode == "folded_tensors":
                y = ac.folded_conv_bn(t['x'], t['weight'], t['gamma'], t['beta'], t.get('conv_bias'), c['mean'], c['var'], 1e-5,
                                      (stride, stride), (k // 2, k // 2))
                leaves = t
            else:
                conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=conv_bias).double()
                bn = torch.nn.BatchNorm2d(cout).double().eval()
                with torch.no_grad():
                    conv.weight.copy_(c['weight']), bn.weight.copy_(c['gamma']), bn.bias.copy_(c['beta'])
                    bn.running_mean.copy_(c['mean']), bn.running_var.copy_(c['var'])
                    if conv_bias:
                        conv.bias.copy_(c['conv_bias'])
                leaves = dict(x=t['x'], weight=conv.weight, gamma=bn.weight, beta=bn.bias)
                if conv_bias:
                    leaves['conv_bias'] = conv.bias
                for n, p in leaves.items():
                    p.requires_grad_(n in on)
                y = bn(conv(t['x'])) if mode == "modules" else conv_bn_folded(t['x'], conv, bn)
            y.backward(c['gy'])
            res[mode] = (y.detach(), {n: leaves[n].grad for n in names})
        y0, g0 = res["modules"]
        for mode in ("folded_modules", "folded_tensors"):
            y1, g1 = res[mode]
            worst = max(worst, rel(y1, y0))
            for n in names:
                assert (g0[n] is None) == (n not in on) and (g1[n] is None) == (n not in on), (mask, mode, n)
                if n in on:
                    assert float(g0[n].abs().max()) > 0.0
                    worst = max(worst, rel(g1[n], g0[n]))
    print(f"conv_bn_folded vs Conv2d -> BatchNorm2d.eval(), {len(masks)} masks: worst relative L2 difference {worst:.2e}")
    assert worst <= 1e-10


def test_conv_bn_act_mask_lists():
    six = ac.conv_bn_act_masks(range(6))
    assert six[0] == tuple(range(6)) and len(six) == len(set(six)) == 1 + 6 + 3 + 6
    assert {(1,), (2,), (1, 2), (1, 3), (2, 3), (0, 2, 3, 4, 5), (0, 1, 3, 4, 5)} <= set(six)
    assert len(ac.conv_bn_act_masks((0, 1, 4))) == 7 and len(ac.all_masks(range(4))) == 15


# ---- the harness on a toy node: y = 3 * a * b + c

def _toy(fault=None):
    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b, c):
            h = 3.0 * b
            scratch = torch.zeros_like(a)
            ctx.save_for_backward(a, h, scratch)
            return a * h + c

        @staticmethod
        def backward(ctx, gy):
            a, h, scratch = ctx.saved_tensors
            need = ctx.needs_input_grad
            if fault == 'assumes_contiguous':
                gy = gy.view(-1).view(gy.shape)
            ga = gy * h
            gb = gy * a * 3.0
            gc = gy
            if fault == 'drops_scale' and not need[1]:
                ga = gy * (h / 3.0)                  # the frozen-partner path forgets the factor
            if fault == 'none_for_required' and not need[0]:
                gb = None                            # the partner's gradient exists only on the all-inputs path
            if fault == 'mask_dependent' and not need[2]:
                ga = ga * (1.0 + 1e-13)              # another code path: right to any bound, not the same bits
            if fault == 'mutates_unused_saved':
                scratch.data.add_(1.0)
            if fault == 'mutates_used_saved':
                h.data.mul_(2.0)
            return ga, gb, gc
    return Toy


def _toy_spec(fault=None):
    Toy = _toy(fault)
    g = torch.Generator().manual_seed(3)
    base = [torch.randn(4, 6, generator=g, dtype=torch.float64) for _ in range(3)]

    def truth(what, got, ref, mask, grad_outs):
        assert float((got - ref).norm()) <= 1e-10 * float(ref.norm()), f"relative L2 {float((got - ref).norm() / ref.norm()):.2e}"
    return ac.NodeSpec('toy', lambda: [t.clone() for t in base], lambda l: Toy.apply(*l), lambda l: 3.0 * l[0] * l[1] + l[2],
                       diff=(0, 1, 2), truth=truth, node_name='Toy')


def test_harness_passes_a_correct_node():
    spec = _toy_spec()
    report = ac.check_masks(spec)
    assert len(report) == 7 and report[(0, 1, 2)] == 'full mask' and set(report.values()) == {'full mask', 'bit-identical'}
    ac.check_grad_layouts(spec)
    assert ac.check_retain_graph(spec) == 3


@pytest.mark.parametrize("fault,check,failing_masks", [
    ('drops_scale', 'truth', {(0,), (0, 2)}),
    ('none_for_required', 'presence', {(1,), (1, 2)}),
    ('mask_dependent', 'mask_independence', {(0,), (0, 1)}),
])
def test_harness_reports_a_planted_mask_fault_by_its_check(fault, check, failing_masks):
    with pytest.raises(ac.ContractViolation) as e:
        ac.check_masks(_toy_spec(fault))
    assert {m for m, _ in e.value.violations} == failing_masks
    assert {v.check for _, v in e.value.violations} == {check}
    ac.check_grad_layouts(_toy_spec(fault))          # full mask only: these faults do not show there
    ac.check_retain_graph(_toy_spec(fault))


@pytest.mark.parametrize("fault,check", [('mutates_unused_saved', 'saved'), ('mutates_used_saved', 'retain')])
def test_harness_reports_a_saved_tensor_written_in_backward(fault, check):
    ac.check_masks(_toy_spec(fault))                 # one backward per graph: invisible to the mask sweep
    with pytest.raises(ac.ContractViolation) as e:
        ac.check_retain_graph(_toy_spec(fault))
    assert e.value.check == check


def test_harness_reports_a_backward_that_assumes_a_contiguous_gradient():
    ac.check_masks(_toy_spec('assumes_contiguous'))
    with pytest.raises(ac.ContractViolation) as e:
        ac.check_grad_layouts(_toy_spec('assumes_contiguous'))
    assert e.value.check == 'layout'


def test_grad_layouts_are_equal_in_value_and_differ_in_strides():
    g = torch.randn(2, 8, 3, 5)
    lay = ac.grad_layouts(g)
    assert set(lay) == {'contiguous', 'permuted', 'sliced', 'channels_last'}
    assert all(torch.equal(t, g) for t in lay.values())
    assert len({t.stride() for t in lay.values()}) == 4 and not lay['sliced'].is_contiguous()


# ---- ext.dropout_add_layernorm_ok: what can be decided without a device

def test_layernorm_operand_predicate_refuses_offset_views_and_strided_weights():
    """gamma / beta are read as float4: an offset view of a flat parameter buffer (4 bytes off) and a strided weight are refused;
    the whole predicate refuses a site on the host (it needs device rows), whatever else holds."""
    from occnet_amd import ext
    flat = torch.zeros(1024)
    assert flat.data_ptr() % 16 == 0
    assert ext._float4_rows_ok(flat[:256]) and ext._float4_rows_ok(flat[256:512])
    assert not ext._float4_rows_ok(flat[1:257])                      # dense, misaligned
    assert not ext._float4_rows_ok(flat[::2][:256])                  # aligned, strided
    ln = torch.nn.LayerNorm(256)
    x = torch.zeros(3, 256)
    assert not ext.dropout_add_layernorm_ok(x, x, ln)
