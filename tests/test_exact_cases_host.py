"""Host side of the exact-arithmetic tests (no GPU): every case tests/test_gpu_exact_arithmetic.py runs is built here from
the same lists and must (1) meet the exactness precondition — every stage's absolute-value contraction below 2^24 units,
so the fp32 accumulator is exact in any summation order; (2) exercise the rounding — bf16 outputs: at least 5 % of the
values need rounding, at least 1 % are exact ties, ReLU cases have 25 % .. 75 % negative pre-activations; bf16x3 cases: at
least 30 % of the wide operand needs its low plane; and (3) kill the mutants — a wrong kernel restated in float64
(truncation, ties away from zero, a dropped K element, edge-replicated padding, an unrounded intermediate, a missing low
plane, a stride or upsampling source off by one, the stem's input truncated) differs from the true reference under the bit comparator.

These are conditions on the inputs: where one fails, the amplitudes or shapes of the case are too tame, and the case is
what gets fixed."""
import pytest
import torch

from tests import exact_cases as ec


def _ids(pairs):
    return [repr(c) + "".join(f"-{k}{int(v)}" for k, v in sorted(kw.items())) for c, kw in pairs]


BF16 = ec.bf16_profile_cases()
FP32 = ec.fp32_cases()
WIDE = ec.wide_operands()
MUTANTS = [(c, kw, m) for c, kw, ms in ec.mutant_table() for m in ms]


@pytest.mark.parametrize("case,kw", BF16 + FP32, ids=_ids(BF16 + FP32))
def test_exactness_precondition(case, kw):
    ref = case.ref(**kw)
    worst = ec.assert_exact_inputs(ref)
    print(f"{case!r}: abs-sum bound {worst:.4g} of {ec.LIMIT:.4g}")
    # the expected output itself is an fp32 value (bf16 outputs by construction)
    if ref.out.dtype == torch.float64:
        assert torch.equal(ref.out.float().double(), ref.out)
        for t in ref.extra.values():
            if t.dtype == torch.float64:
                assert torch.equal(t.float().double(), t)


@pytest.mark.parametrize("case,kw", BF16, ids=_ids(BF16))
def test_rounding_profile(case, kw):
    ref = case.ref(**kw)
    inexact, ties, negative = ec.rounding_profile(ref.pre, relu=ref.relu)
    print(f"{case!r} {kw}: inexact {inexact:.3f} ties {ties:.3f} negative {negative:.3f}")
    assert inexact >= 0.05 and ties >= 0.01, (inexact, ties)
    if ref.relu:
        assert 0.25 <= negative <= 0.75, negative
    # chains: the rounded intermediates must need their rounding too
    for name in ("mid_pre", "p1", "p2"):
        if name in ref.extra:
            i2, t2, n2 = ec.rounding_profile(ref.extra[name], relu=True)
            print(f"    {name}: inexact {i2:.3f} ties {t2:.3f} negative {n2:.3f}")
            assert i2 >= 0.01 and t2 >= 0.01 and 0.25 <= n2 <= 0.75, (name, i2, t2, n2)


CHAIN_RELU = [(c, kw) for c, kw in ec.chain_host_cases() if c.ref(**kw).relu]


@pytest.mark.parametrize("case,kw", CHAIN_RELU, ids=_ids(CHAIN_RELU))
def test_chain_relu_sees_negative_preactivations(case, kw):
    """The ReLU of linear_ln_chain's tail and of encoder_ffn_chain's hidden layer (fp32 outputs: no rounding to profile)."""
    negative = ec.rounding_profile(case.ref(**kw).pre)[2]
    print(f"{case!r}: negative {negative:.3f}")
    assert 0.25 <= negative <= 0.75, negative


@pytest.mark.parametrize("case,wide", WIDE, ids=[repr(c) for c, _ in WIDE])
def test_wide_operand_needs_its_low_plane(case, wide):
    share = float((~ec.is_bf16(wide)).double().mean())
    if case.key[0] != "stem":
        hi, lo = ec.bf16_split(wide)
        assert torch.equal(hi + lo, wide)               # and two planes hold it exactly
    assert share >= 0.30, share


@pytest.mark.parametrize("case,kw,mutant", MUTANTS, ids=[f"{c!r}-{m}" for c, _, m in MUTANTS])
def test_oracle_kills_the_mutant(case, kw, mutant):
    true, wrong = case.ref(**kw), case.ref(mut=mutant, **kw)
    outs = [(wrong.out, true.out)] + [(wrong.extra[k], true.extra[k]) for k in true.extra
                                      if k in ("dx", "dw", "db") and true.extra[k].dtype == true.out.dtype]
    reports = [ec.diff_report(w if w.dtype == torch.bfloat16 else w.float(), t) for w, t in outs]
    assert any(r is not None for r in reports), f"mutant {mutant} survives on {case!r}"
    print(f"{case!r} {mutant}: {[r for r in reports if r][0]}")


def test_comparator_reports_the_first_difference_and_ignores_nothing():
    want = torch.tensor([[1.0, 2.0], [3.0, 258.0]], dtype=torch.float64)
    assert ec.diff_report(want.float(), want) is None
    got = want.float().clone()
    got[1, 0] = 3.0000002
    rep = ec.diff_report(got, want)
    assert rep.startswith("1 of 4") and "(1, 0)" in rep
    wb = want.float().to(torch.bfloat16)
    gb = wb.clone()
    assert ec.diff_report(gb, wb) is None
    gb[0, 1] = -2.0
    gb[1, 1] = 260.0                                   # one bf16 ulp
    rep = ec.diff_report(gb, wb)
    assert rep.startswith("2 of 4") and "(0, 1)" in rep
    with pytest.raises(AssertionError):
        ec.assert_bit_equal(gb, wb, "demo")
    # -0.0 against +0.0 is a bit difference for bf16 outputs
    assert ec.diff_report(torch.tensor([-0.0], dtype=torch.bfloat16), torch.tensor([0.0], dtype=torch.bfloat16)) is not None


def test_rounding_helpers():
    t = torch.tensor([257.0, 259.0, 258.0, -257.0, -259.0, 3.0, 1025.0], dtype=torch.float64)
    assert ec.rne_bf16(t).tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 3.0, 1024.0]
    assert ec.trunc_bf16(t).tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 3.0, 1024.0]
    assert ec.half_away_bf16(t).tolist() == [258.0, 260.0, 258.0, -258.0, -260.0, 3.0, 1024.0]
    inexact, ties, negative = ec.rounding_profile(t)
    assert (round(inexact * 7), round(ties * 7), round(negative * 7)) == (5, 4, 2)
    hi, lo = ec.bf16_split(torch.tensor([2047.0, -1023.0, 255.0], dtype=torch.float64))
    assert hi.tolist() == [2048.0, -1024.0, 255.0] and lo.tolist() == [-1.0, 1.0, 0.0]
    with pytest.raises(AssertionError):
        ec.rne_bf16(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64))      # not an fp32 value
