"""-m gpu: the kernels that join the training step (csrc/ln_dropout_train.hip, csrc/rows_index.hip, csrc/sca_prep.hip,
csrc/point_sampling.hip) against the float64 restatements of tests/train_glue_ref.py: bit for bit wherever the arithmetic is
exact, under bounds counted from the kernel sources elsewhere (tests/ln_bound.py, train_glue_ref.C_POINT), at the row
counts where the grid-stride loops make a second and third iteration, at every block count on either side of the column
reduce's loop boundaries, and at the padded, repeated, unseen and on-the-boundary inputs the one-shape tests never held.
tests/test_train_glue_host.py shows on the CPU that the cases meet their preconditions and that the assertion functions
used here reject the listed wrong kernels.  Every printed ratio is err / bound, for information."""
import pytest
import torch

from tests import exact_cases as ec
from tests import train_glue_ref as tg
from tests.test_train_glue_host import _grid_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return t.float().to(DEV)


# ---- DropoutAddLayerNorm ---------------------------------------------------------------------------------------------------

def _run_ln(c, torch_seed=None):
    from occnet_amd import ext
    x, r = _dev(c["x"]).requires_grad_(), _dev(c["res"]).requires_grad_()
    gamma, beta = c["gamma"].to(DEV).requires_grad_(), c["beta"].to(DEV).requires_grad_()
    torch.manual_seed(c["torch_seed"] if torch_seed is None else torch_seed)
    y = ext.DropoutAddLayerNormFunction.apply(x, r, gamma, beta, 1e-5, c["p"])
    y.backward(_dev(c["gy"]))
    torch.cuda.synchronize()
    return y.detach(), x.grad, r.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("rows,p", tg.ln_train_cases())
def test_dropout_add_layernorm_on_exact_rows(rows, p):
    case = tg.ln_train_case(rows, p)
    c, ref = case.inp, case.ref()
    y, gx, gres, dgamma, dbeta = _run_ln(c)
    r_y = tg.assert_ln_train_forward(y, ref)
    if p == 0:
        assert torch.equal(gx, gres)
    r_g, r_d = tg.assert_ln_train_backward(gx if p > 0 else None, gres, dgamma, dbeta, ref)
    print(f"rows {rows} p {p}: err / bound  y {r_y:.3f}  g_residual {r_g:.3f}  dgamma {r_d:.3f};  dbeta and the mask exact")


def test_dropout_mask_follows_the_seed():
    c = tg.ln_train_case(131, 0.5).inp
    a, b, other = _run_ln(c), _run_ln(c), _run_ln(c, torch_seed=77)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert tg.drawn_seed(77) != c["seed"] and not torch.equal(a[1] == 0, other[1] == 0)


# ---- rows_gather_sum -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", tg.GATHER_SHAPES)
def test_rows_gather_sum_is_exact(shape):
    from occnet_amd import ext
    case = tg.gather_case(*shape)
    c = case.inp
    out = ext.rows_gather_sum(_dev(c["x"]), c["index"].to(DEV))
    ec.assert_bit_equal(out, case.ref(), repr(case))


@pytest.mark.parametrize("shape", tg.GATHER_PAIRS)
def test_rows_gather_sum_function_and_its_gradient_are_exact(shape):
    from occnet_amd import ext
    case = tg.gather_pair_case(*shape)
    c = case.inp
    want_out, want_grad = case.ref()
    x = _dev(c["x"]).requires_grad_()
    r2q, q2r = c["r2q"].to(DEV), c["q2r"].to(DEV)
    out = ext.RowsGatherSumFunction.apply(x, r2q, q2r)
    out.backward(_dev(c["gout"]))
    ec.assert_bit_equal(out, want_out, "rebatch")
    ec.assert_bit_equal(x.grad, want_grad, "gradient")
    # the other direction: the scatter back is the gather-sum over the inverse map, and the rebatch is ITS gradient
    rows = _dev(c["gout"]).requires_grad_()
    back = ext.RowsGatherSumFunction.apply(rows, q2r, r2q)
    back.backward(_dev(c["x"]))
    ec.assert_bit_equal(back, want_grad, "scatter back")
    ec.assert_bit_equal(rows.grad, want_out, "gradient of the scatter back")


def test_index_arguments_are_checked_before_any_launch():
    """Only the raise is asserted: no call here reaches a kernel."""
    from occnet_amd import ext
    from occnet_amd._lib import OccAmdError
    x = torch.zeros(2, 6, 8, device=DEV)
    idx = torch.zeros(4, 2, dtype=torch.long, device=DEV)
    inv = torch.zeros(6, 2, dtype=torch.long, device=DEV)
    bad = lambda t: (t.int(), t.cpu(), t.repeat_interleave(2, dim=0)[::2], t.float())          # dtype, device, strides
    assert not bad(idx)[2].is_contiguous() and not bad(torch.zeros(5, 1))[2].is_contiguous()
    for w in bad(idx):
        with pytest.raises(OccAmdError):
            ext.rows_gather_sum(x, w)
        with pytest.raises(OccAmdError):
            ext.RowsGatherSumFunction.apply(x, w, inv)
    for w in bad(inv) + (inv[:5],):
        with pytest.raises(OccAmdError):
            ext.RowsGatherSumFunction.apply(x, idx, w)
    M, L, P = tg.PREP_M, tg.PREP_L, tg.PREP_P
    proj = torch.zeros(2, 6, 768, device=DEV)
    r2q = torch.zeros(5, 1, dtype=torch.long, device=DEV)
    q2r = torch.zeros(6, 2, dtype=torch.long, device=DEV)
    ref_rb = torch.zeros(2, 5, 4, 2, device=DEV)
    shapes = torch.tensor(tg.PREP_SHAPES_REAL, device=DEV)
    good = [proj, r2q, q2r, ref_rb, shapes]
    for pos in (1, 2, 4):
        for w in bad(good[pos]):
            args = list(good)
            args[pos] = w
            with pytest.raises(OccAmdError):
                ext.SCAPrepFunction.apply(*args, M, L, P)
    for w in (torch.zeros(2, 4, 4, 2, device=DEV), torch.zeros(1, 5, 4, 2, device=DEV), torch.zeros(2, 5, 4, 3, device=DEV),
              torch.zeros(2, 5, 8, device=DEV), ref_rb.cpu(), ref_rb.double()):
        with pytest.raises(OccAmdError):
            ext.SCAPrepFunction.apply(proj, r2q, q2r, w, shapes, M, L, P)
    for args in ([proj, r2q, q2r, ref_rb, shapes[:3]], [proj, r2q, q2r[:5], ref_rb, shapes], [proj, r2q.view(1, 5), q2r, ref_rb, shapes]):
        with pytest.raises(OccAmdError):
            ext.SCAPrepFunction.apply(*args, M, L, P)


# ---- SCAPrep ---------------------------------------------------------------------------------------------------------------

def _run_prep(c):
    from occnet_amd import ext
    proj = _dev(c["proj"]).requires_grad_()
    loc, attn = ext.SCAPrepFunction.apply(proj, c["r2q"].to(DEV), c["q2r"].to(DEV), _dev(c["ref_rb"]),
                                          torch.tensor(c["shapes"], device=DEV), tg.PREP_M, tg.PREP_L, tg.PREP_P)
    torch.autograd.backward([loc, attn], [_dev(c["g_loc"]), _dev(c["g_attn"])])
    torch.cuda.synchronize()
    return loc.detach(), attn.detach(), proj.grad


@pytest.mark.parametrize("combo", tg.prep_cases(True), ids=lambda c: "Z%d-bs%d-ld%d-Kq%d" % c[:4])
def test_sca_prep_exact_half(combo):
    case = tg.prep_case(*combo)
    loc, attn, dproj = _run_prep(case.inp)
    tg.assert_prep_exact(loc, attn, dproj, case.ref(), case.inp)


@pytest.mark.parametrize("combo", tg.prep_cases(False), ids=lambda c: "Z%d-bs%d-ld%d-Kq%d" % c[:4])
def test_sca_prep_general_half(combo):
    case = tg.prep_case(*combo)
    loc, attn, dproj = _run_prep(case.inp)
    e = tg.assert_prep_general(loc, attn, dproj, case.ref())
    d = dproj.cpu()
    assert bool((d[:, case.inp["q2r"][:, 0] < 0] == 0).all()) and bool((d[..., tg.PREP_W:] == 0).all())
    print("sca_prep %s: loc %.2e attn %.2e grad rel %.2e" % (case, *e))


# ---- point_sampling --------------------------------------------------------------------------------------------------------

def _run_points(inp):
    from occnet_amd import ext
    out = ext.point_sampling(inp["ref_3d"].to(DEV), inp["lidar2img"].to(DEV), inp["ego2lidar"].to(DEV), inp["pc_range"],
                             inp["img_h"], inp["img_w"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("grid", tg.POINT_GRIDS)
def test_point_sampling_on_its_decision_set(grid):
    inp = _grid_inputs(*grid)
    r = tg.point_sampling_ref(**inp)
    ratio = tg.assert_point_sampling(*_run_points(inp), r)
    n = r.decidable.numel()
    print(f"grid {grid}: {n - int(r.decidable.sum())} of {n} points undecidable; ref_cam worst err / bound = {ratio:.3f}")


@pytest.mark.parametrize("NC", tg.BOUNDARY_NC)
def test_point_sampling_on_the_boundaries(NC):
    inp = tg.point_boundary_case(NC)
    r = tg.point_sampling_ref(**inp, exact=True)
    ref_cam, mask, vis = _run_points(inp)
    assert vis.dtype == torch.int32
    tg.assert_point_sampling_exact(ref_cam, mask, vis, r)
    if NC == 32:                                               # camera 31 is the sign bit of the word
        centre = tg.BOUNDARY_QUERIES.index("centre")
        assert bool(mask[31, 0, centre, 0]) and int(vis[0, centre]) < 0
