"""Host: the closed-form float64 reference of tests/msda_ref.py, float64 against float64.

(a) where the operator is smooth it equals torch.autograd through the restated mmcv function; (b) on the decision set its
forward equals the scalar restatement and grad_value / grad_attn still equal autograd; (c) its grad_loc on the decision set is
the right-sided slope of grad_attn inside the cell, exactly 0 for a sample that is not admitted; (d) autograd's grad_loc is far
from it there, which is why this reference exists; and it kills the mutants: wrong kernels restated in float64 move a
decision-set or sparse-gradient comparison beyond the bounds the GPU tests hold (tests/test_gpu_msda_edges.py).

Bounds: 1e-12 of the reference's scale for float64 against float64 (observed: at most 5e-15), 1e-9 for the difference quotient
over d = 2^-10 px (rounding 1e-16 / d)."""
import functools

import pytest
import torch

from oracle import msda as omsda
from tests import msda_ref as mr

F64_BOUND, SLOPE_BOUND = 1e-12, 1e-9
GPU_GRAD_BOUND, GPU_FWD_BOUND = 1e-4, 2e-5          # tests/test_gpu_backward.py, tests/test_gpu_msda.py

INTERIOR_CASES = [
    ("sca_like", 2, [[12, 20], [6, 10], [3, 5], [2, 3]], 4, 32, 50, 8),
    ("ragged_items", 1, [[5, 7], [3, 4]], 3, 32, 13, 5),
    ("generic_d16", 2, [[9, 11], [4, 6]], 4, 16, 57, 3),
    ("single", 1, [[1, 1]], 1, 32, 1, 1),
]


def _rel(got, ref):
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _interior_inputs(B, shapes, M, D, Lq, P, seed=5):
    """The inputs of tests/test_gpu_backward.py's cases, from its own helpers (the module imports without a GPU)."""
    from tests.test_gpu_backward import _interior
    from tests.test_gpu_msda import _inputs
    value, shapes_t, start, loc, attn = _inputs(B, shapes, M, D, Lq, P, seed=seed, adversarial=False)
    loc = _interior(loc, shapes)
    grad_out = torch.randn(B, Lq, M * D, generator=torch.Generator().manual_seed(6))
    return value, shapes_t, start, loc, attn, grad_out


@pytest.mark.parametrize("name,B,shapes,M,D,Lq,P", INTERIOR_CASES, ids=[c[0] for c in INTERIOR_CASES])
def test_closed_form_equals_autograd_where_smooth(name, B, shapes, M, D, Lq, P):
    value, shapes_t, start, loc, attn, grad_out = _interior_inputs(B, shapes, M, D, Lq, P)
    res = mr.closed_form(value.double(), shapes, loc, attn, grad_out)
    fwd = omsda.multi_scale_deformable_attn_pytorch(value.double(), shapes_t, loc.double(), attn.double())
    refs = omsda.msda_backward_autograd(value.double(), shapes_t, loc.double(), attn.double(), grad_out.double())
    d = _rel(res['out'], fwd)
    print(f"{name} forward: {d:.3e}")
    assert d < F64_BOUND
    for nm, got, ref in zip(("grad_value", "grad_loc", "grad_attn"), mr.grads(res), refs):
        d = _rel(got, ref)
        print(f"{name} {nm}: {d:.3e}")
        assert d < F64_BOUND, (name, nm, d)


@functools.lru_cache(maxsize=None)
def _decision():
    inputs = mr.decision_set()
    value, shapes_t, start, loc, attn, grad_out = inputs
    return inputs, mr.closed_form(value.double(), mr.DECISION_SHAPES, loc, attn, grad_out)


def _finite_stand_in(loc):
    """grid_sample has no answer for a non-finite location; a location far outside has the same one as the closed form gives
    them (not admitted: zero), so the autograd oracle gets 1e7 in their place.  The closed form keeps the original."""
    return torch.where(torch.isfinite(loc), loc, torch.full_like(loc, 1e7))


def test_decision_set_covers_every_decision():
    (value, shapes_t, start, loc, attn, grad_out), res = _decision()
    adm = res['adm']
    print(f"decision set: {adm.numel()} samples, {int(adm.sum())} admitted, {int((~torch.isfinite(loc)).any(-1).sum())} non-finite")
    assert not adm[(~torch.isfinite(loc)).any(-1)].any() and not adm[(loc.abs() > 1e6).any(-1)].any()
    for l, (H, W) in enumerate(mr.DECISION_SHAPES):
        x = loc[:, :, :, l, :, 0].double() * W - 0.5
        y = loc[:, :, :, l, :, 1].double() * H - 0.5
        for c, n in ((x, W), (y, H)):
            for want in mr.axis_coords(n):
                assert (c == want).any(), (l, n, want)
        a = adm[:, :, :, l]
        assert a[(x == W - 0.25) & (y == H - 0.25)].all() and not a[(x == W) & (y == 0)].any()
        assert not a[(x == -1) & (y == 0)].any() and a[(x == -0.75) & (y == -0.75)].all()
        assert not a[(x == 0) & (y == -1)].any() and not a[(x == 0) & (y == H)].any()
    # the rotation: the 8 items of a wave do not hold the same sample list
    flat = loc.view(-1, *loc.shape[3:])
    assert not torch.equal(torch.nan_to_num(flat[0]), torch.nan_to_num(flat[1]))


def test_decision_set_forward_value_and_attn_gradients():
    (value, shapes_t, start, loc, attn, grad_out), res = _decision()
    scalar, _ = omsda.msda_scalar_f64(value.numpy(), mr.DECISION_SHAPES, start.tolist(), loc.numpy(), attn.numpy())
    d = _rel(res['out'], torch.from_numpy(scalar))
    print(f"decision set forward vs scalar restatement: {d:.3e}")
    assert d < F64_BOUND
    gv, gl, ga = omsda.msda_backward_autograd(value.double(), shapes_t, _finite_stand_in(loc).double(), attn.double(),
                                              grad_out.double())
    for nm, got, ref in (("grad_value", res['grad_value'], gv), ("grad_attn", res['grad_attn'], ga)):
        d = _rel(got, ref)
        print(f"decision set {nm} vs autograd: {d:.3e}")
        assert d < F64_BOUND, (nm, d)
    for t in (res['out'], *mr.grads(res)):
        assert torch.isfinite(t).all()
    # (d) the reason this reference exists
    scale = max(1.0, float(res['grad_loc'].abs().max()))
    far = float((gl - res['grad_loc']).abs().max())
    print(f"decision set grad_loc: autograd differs from the closed form by {far:.3f} on a scale of {scale:.3f}")
    assert far / scale > 1e-2


def test_decision_set_grad_loc_is_the_right_sided_slope():
    (value, shapes_t, start, loc, attn, grad_out), res = _decision()
    adm, gl = res['adm'], res['grad_loc']
    assert float(gl[~adm].abs().max()) == 0.0 and float(res['grad_attn'][~adm].abs().max()) == 0.0
    scale = max(1.0, float(gl.abs().max()))
    d_px = 2.0 ** -10
    safe = torch.where(adm[..., None], loc.double(), torch.full_like(loc, 0.5).double())
    for axis in (0, 1):
        step = torch.zeros_like(safe)
        for l, (H, W) in enumerate(mr.DECISION_SHAPES):
            step[:, :, :, l, :, axis] = d_px / (W, H)[axis]
        moved = mr.closed_form(value.double(), mr.DECISION_SHAPES, safe + step, attn, grad_out)
        base = mr.closed_form(value.double(), mr.DECISION_SHAPES, safe, attn, grad_out)
        assert torch.equal(moved['adm'][adm], base['adm'][adm]) and base['adm'][adm].all()     # same cell, still admitted
        slope = attn.double() * (moved['grad_attn'] - base['grad_attn']) / step[..., axis]
        d = float((slope - gl[..., axis])[adm].abs().max()) / scale
        print(f"decision set grad_loc axis {axis}: slope of grad_attn over 2^-10 px differs by {d:.3e} of scale {scale:.2f}")
        assert d < SLOPE_BOUND


# ---- the mutants ---------------------------------------------------------------------------------------------------------------
SPARSE_SHAPES, SPARSE_DIMS = [[12, 20], [3, 5]], (2, 3, 32, 300, 4)        # the shape of the GPU test


@functools.lru_cache(maxsize=None)
def _sparse_inputs():
    B, M, D, Lq, P = SPARSE_DIMS
    return mr.dyadic_inputs(B, SPARSE_SHAPES, M, D, Lq, P, seed=41)


def _moved(true, wrong):
    """The comparisons of the GPU tests that the wrong result fails: name -> distance in units of its bound."""
    out = {}
    d = float((wrong['out'] - true['out']).abs().max()) / GPU_FWD_BOUND
    if d > 1:
        out['forward'] = d
    for nm in ('grad_value', 'grad_loc', 'grad_attn'):
        d = _rel(wrong[nm], true[nm]) / GPU_GRAD_BOUND
        if d > 1:
            out[nm] = d
    return out


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_closed_form_kills_the_mutant(mutant):
    moved = {}
    (value, shapes_t, start, loc, attn, grad_out), true = _decision()
    wrong = mr.closed_form(value.double(), mr.DECISION_SHAPES, loc, attn, grad_out, mut=mutant)
    moved.update({f"decision set {k}": v for k, v in _moved(true, wrong).items()})
    value, shapes_t, start, loc, attn, grad_out = _sparse_inputs()
    for pattern in mr.SPARSE_PATTERNS:
        g, _ = mr.sparse_grad(grad_out, SPARSE_DIMS[1], pattern)
        true = mr.closed_form(value.double(), SPARSE_SHAPES, loc, attn, g)
        wrong = mr.closed_form(value.double(), SPARSE_SHAPES, loc, attn, g, mut=mutant)
        moved.update({f"{pattern} {k}": v for k, v in _moved(true, wrong).items()})
    print(f"{mutant}: beyond the GPU bound by a factor of " + ", ".join(f"{k}: {v:.3g}" for k, v in moved.items()))
    assert moved, f"mutant {mutant} survives every decision-set and sparse-gradient comparison"
    if mutant.startswith('skip'):
        assert any(not k.startswith('decision') for k in moved)
    else:
        assert any(k.startswith('decision') for k in moved)


@pytest.mark.parametrize("pattern", mr.SPARSE_PATTERNS)
def test_sparse_patterns_are_what_they_say(pattern):
    B, M, D, Lq, P = SPARSE_DIMS
    grad_out = _sparse_inputs()[5]
    g, zero = mr.sparse_grad(grad_out, M, pattern)
    gi = g.view(B, Lq, M, D)
    assert torch.equal(zero, (gi == 0).all(-1))
    live = ~zero
    assert torch.equal(gi[live & ((gi != 0).sum(-1) == D)], grad_out.view(B, Lq, M, D)[live & ((gi != 0).sum(-1) == D)])
    if pattern == 'every_4th_query':
        assert zero[:, ::4].all() and not zero[:, 1::4].any()
    elif pattern == 'one_head':
        assert zero[:, :, M // 2].all() and int(zero.sum()) == B * Lq
    elif pattern == 'one_channel':
        single = (gi != 0).sum(-1) == 1
        assert not zero.any()
        for c in mr.ONE_CHANNELS:
            assert (single & (gi[..., c] != 0)).any(), c
    elif pattern == 'neg_zero_rows':
        assert zero[:, 1::3].all() and torch.signbit(gi[:, 1::3]).all()
    elif pattern == 'zero_run':
        run = best = 0
        for z in zero[0].flatten().tolist():
            run = run + 1 if z else 0
            best = max(best, run)
        assert best >= 64 and best % 8 != 0
    elif pattern == 'all_zero':
        assert zero.all()
