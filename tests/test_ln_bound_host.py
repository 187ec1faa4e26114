"""Host side of the LayerNorm tests of tests/test_gpu_exact_arithmetic.py (no GPU): the cases meet their precondition, an
fp32 emulation of the kernel's own form stays inside the derived bound of tests/ln_bound.py, and wrong kernels break it:
a one-pass variance on the offset rows, a division by N - 1, an omitted eps on the near-constant rows, and, through
encoder_ffn_chain's second LayerNorm, a hidden layer without its ReLU or an FFN without its residual."""
import pytest
import torch

from tests import exact_cases as ec
from tests import ln_bound as lb

LN_N = (256, 128, 100)
LN_M = (65, 8229)


@pytest.mark.parametrize("N", LN_N)
def test_ln_case_meets_the_precondition_and_holds_every_row_kind(N):
    c = lb.ln_case(65, N)
    assert float(c["abs"].max()) < ec.LIMIT
    lb.assert_ln_inputs(c["x"])
    ref = lb.LnRef(c["x"], c["gamma"], c["beta"])
    k = c["kind"]
    std = ref.var.sqrt()[:, 0]
    assert float(c["x"][k == lb.ORDINARY].abs().max()) > 5e4
    assert float((ref.mean[:, 0].abs() / std)[k == lb.OFFSET].min()) >= 100.0
    assert bool((ref.var[k == lb.CONSTANT] == 0).all()) and bool((ref.y[k == lb.CONSTANT] == c["beta"].double()).all())
    share = lb.EPS / (ref.var[k == lb.NEAR_CONSTANT] + lb.EPS)
    if N == 256:                                       # var = 255 / 256^2: eps is a quarter of a per cent of var + eps
        assert 0.002 < float(share.min()) and float(share.max()) < 0.003
    for tile in range(0, 64, 32):                      # several rows of each kind in every 32-row tile
        assert all(int((k[tile:tile + 32] == kind).sum()) >= 4 for kind in range(4))


def test_emulated_kernel_stays_inside_the_bound_and_wrong_kernels_break_it():
    c = lb.ln_case(8229, 256)
    ref = lb.LnRef(c["x"], c["gamma"], c["beta"])
    bound = ref.bound(lb.C_CHAIN)
    k = c["kind"]
    g = torch.Generator().manual_seed(7)
    worst = max(lb.worst_ratio(lb.emulate(c["x"], c["gamma"], c["beta"], g), ref, bound) for _ in range(4))
    print(f"two-pass emulation: worst err / bound = {worst:.3f}")
    assert worst <= 1.0

    def ratio_on(form, kind):
        y = lb.emulate(c["x"], c["gamma"], c["beta"], g, form=form)
        sub = lb.LnRef(c["x"][k == kind], c["gamma"], c["beta"])
        return lb.worst_ratio(y[k == kind], sub, sub.bound(lb.C_CHAIN))
    for form, kind in (("one_pass", lb.OFFSET), ("bessel", lb.ORDINARY), ("bessel", lb.OFFSET), ("no_eps", lb.NEAR_CONSTANT)):
        r = ratio_on(form, kind)
        print(f"{form} on rows of kind {kind}: worst err / bound = {r:.3g}")
        assert r > 1.0, (form, kind, r)
    # the constant rows are beta exactly in the kernel's form
    y = lb.emulate(c["x"], c["gamma"], c["beta"], g)
    assert torch.equal(y[k == lb.CONSTANT], c["beta"][None].expand(int((k == lb.CONSTANT).sum()), 256))


@pytest.mark.parametrize("mutant", ["no_relu", "no_x2", "drop_low", "drop_k"])
def test_ffn_mutants_break_the_bound_behind_the_second_layernorm(mutant):
    """encoder_ffn_chain shows pre2 only through LayerNorm 2: the wrong pre2 of each mutant, normalised in float64 (no
    rounding error at all), already misses the bound around the true y."""
    case = ec.ffn_case(1)
    c = case.inp
    true = lb.LnRef(case.ref().value, c["g2"], c["be2"])
    lb.assert_ln_inputs(true.x)
    wrong = lb.LnRef(case.ref(mut=mutant).value, c["g2"], c["be2"])
    r = lb.worst_ratio(wrong.y, true, true.bound(lb.C_CHAIN))
    print(f"{mutant}: worst err / bound = {r:.3g}")
    assert r > 1.0


@pytest.mark.parametrize("N", LN_N)
def test_bound_terms(N):
    """A power-of-two N has the plain bound; 100 columns add the two terms of the inexact mean."""
    c, m = lb.linear_c(N)
    assert (c, m) == ((lb.C_LINEAR, 0) if N != 100 else (lb.C_LINEAR_INEXACT, lb.MEAN_ROUNDINGS))
    case = lb.ln_case(65, N)
    ref = lb.LnRef(case["x"], case["gamma"], case["beta"])
    plain = c * lb.U * ref.t.abs() + lb.U * ref.y.abs()
    assert bool((ref.bound(c, m) >= plain).all()) and (m > 0 or torch.equal(ref.bound(c, m), plain))
