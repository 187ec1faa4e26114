"""-m gpu: every fused spatial cross-attention gather kernel (ext.sca_fused_forward -> sca_fused_kernel for fp32 rows,
sca_fused_h_kernel / sca_fused_hm_kernel for fp16 and q16 rows) against the float64 reference of tests/sca_ref.py, in every
calling mode of the wrapper.  Every test is a handful of launches on maps of at most 177 pixels; the properties of the cases
themselves are asserted on the CPU in tests/test_sca_fused_host.py.

The kernel is chosen by the value rows' dtype and OCC_SCA_HEAD_MAJOR (read per call).  16-bit rows are compared with the
reference on the STORED values (fp16: value.half(); q16: the numpy decoder of tests/q16_ref.py on what the HIP encoder wrote), so
what is measured is the gather's fp32 arithmetic, not the rows' rounding.  The result is linear in the values: a case whose
values are amp * N(0, 1) is held to GPU_TOL * amp, whether amp lies above 1 or below (measured: profiles/sca_forward_reference.txt)."""
import functools

import numpy as np
import pytest
import torch

from tests import q16_ref
from tests.sca_ref import CASE_IDS, CASES, GPU_TOL, TAILS, D, M, case_ref, sca_case, sca_counts, sca_gather_ref

pytestmark = pytest.mark.gpu

KERNELS = ["f32", "f16", "q16", "f16-hm", "q16-hm"]
HALF_KERNELS = KERNELS[1:]
MAIN = CASE_IDS.index("L4P8_Z4_B2")          # 16-byte logits / offsets loads, the head-major kernel's 16-byte anchor loads


def _select(kernel, monkeypatch):
    monkeypatch.setenv("OCC_SCA_HEAD_MAJOR", "1" if kernel.endswith("-hm") else "0")
    return kernel.split("-")[0]


def _decode_q16(enc, S, scale):
    """int16 pixel pairs (BN, S_pad, M*D) as the HIP encoder wrote them -> the float64 values they stand for, row order."""
    from occnet_amd import ext
    BN = enc.shape[0]
    rows = ext.sca_unpair_layout(enc.view(BN, -1, M, D), S).cpu().numpy()
    return torch.from_numpy(q16_ref.decode(rows.reshape(BN, S, M * D), scale)).view(BN, S, M, D)


@functools.lru_cache(maxsize=None)
def _case(i, amp=1.0):
    """CPU inputs of case i and their device copies, made once and never written to."""
    c = sca_case(*CASES[i], amp=amp)
    dev = {k: c[k].cuda() for k in ('value', 'shapes', 'starts', 'offs', 'logits', 'ref_cam', 'vis')}
    return c, dev


@functools.lru_cache(maxsize=None)
def _stored(i, fmt, amp=1.0, scaled=False):
    """The value rows of case i in one storage format -> (device rows, wrapper keywords, the float64 values they store in row
    order).  scaled: under the power-of-two range scale of ext.f16_range_scaled / ext.q16_range_scaled."""
    from occnet_amd import ext
    c, dev = _case(i, amp)
    if fmt == "f32":
        return dev['value'], {}, c['value'].double()
    if fmt == "f16":
        if scaled:
            rows, s = ext.f16_range_scaled(dev['value'])
            return rows, dict(value_scale=s), rows.cpu().double() / float(s)
        rows = dev['value'].half()
        return rows, {}, rows.cpu().double()
    BN, S = c['value'].shape[:2]
    flat = dev['value'].view(BN, S, M * D)
    enc, s = ext.q16_range_scaled(flat) if scaled else (ext.sca_rows_encode_q16(flat), None)
    kw = dict(value_layout="pairs", value_scale=s)
    return enc.view(BN, -1, M, D), kw, _decode_q16(enc, S, 1.0 if s is None else float(s))


@functools.lru_cache(maxsize=None)
def _rows(i, fmt, amp=1.0, scaled=False):
    """-> (device rows, wrapper keywords, float64 reference on the stored values), computed once and never written to."""
    rows, kw, stored = _stored(i, fmt, amp, scaled)
    return rows, kw, case_ref(_case(i, amp)[0], stored)


def _run(c, dev, rows, kw, **over):
    from occnet_amd import ext
    a = dict(dev, **{k: over.pop(k) for k in ('offs', 'logits', 'ref_cam') if k in over})
    return ext.sca_fused_forward(rows, a['shapes'], a['starts'], a['offs'], a['logits'], a['ref_cam'], a['vis'], M, c['L'],
                                 c['P'], **kw, **over)


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


def _nan_prefill(c):
    """The result's future storage holds NaN: a row that no wave writes cannot pass by luck."""
    junk = torch.full((c['B'], c['Nq'], M * D), float('nan'), device='cuda')
    del junk


def _perm32(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(torch.int32)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_matches_reference(kernel, i, monkeypatch):
    fmt = _select(kernel, monkeypatch)
    c, dev = _case(i)
    rows, kw, ref = _rows(i, fmt)
    _nan_prefill(c)
    out = _run(c, dev, rows, kw)
    d = _err(out, ref)
    print(f"{kernel} {CASE_IDS[i]}: max|hip - reference(f64)| = {d:.3e}")
    assert out.shape == (c['B'], c['Nq'], M * D) and out.dtype == torch.float32
    assert d < GPU_TOL


@pytest.mark.parametrize("amp", [1e-3, 1e3])
@pytest.mark.parametrize("kernel", HALF_KERNELS)
def test_range_scaled_rows_match_reference(kernel, amp, monkeypatch):
    """Rows stored under the range scale s (max|s v| in [2^14, 2^15]) against the reference on the stored rows / s."""
    fmt = _select(kernel, monkeypatch)
    c, dev = _case(MAIN, amp)
    rows, kw, ref = _rows(MAIN, fmt, amp, True)
    s = float(kw['value_scale'])
    assert 2.0 ** 14 <= float(c['value'].abs().max()) * s <= 2.0 ** 15
    out = _run(c, dev, rows, kw)
    d = _err(out, ref)
    print(f"{kernel} amp {amp:g} (s = 2^{int(np.log2(s))}): max|hip - reference(f64)| = {d:.3e} (bound {GPU_TOL * amp:.1e})")
    assert float(ref.abs().max()) > 0.5 * amp
    assert d < GPU_TOL * amp


@pytest.mark.parametrize("k", [-7, 9])
@pytest.mark.parametrize("kernel", HALF_KERNELS)
def test_gather_under_the_range_scale_is_exact(kernel, k, monkeypatch):
    """test_gpu_value_range.py::test_gather_under_the_range_scale_is_exact on all four 16-bit kernels.  fp16 rows: rows
    holding value * 2^k under value_scale = 2^k give the unscaled rows' result bit for bit.  q16 rows carry their piece's
    exponent in the low bits of two mantissas, so a rescaled plane is another set of values; what is exact is the divisor:
    the same rows under value_scale = s and s * 2^k give results that differ by the factor 2^k, bit for bit."""
    from occnet_amd import ext
    fmt = _select(kernel, monkeypatch)
    c, dev = _case(MAIN)
    g = torch.Generator().manual_seed(21)
    shape = c['value'].shape
    sign = (torch.rand(shape, generator=g) < 0.5).float() * 2 - 1
    value = (sign * (0.5 + 3.5 * torch.rand(shape, generator=g))).half().cuda()       # exponents -1 .. 1: exact both ways
    s = torch.tensor([2.0 ** k], device='cuda')
    if fmt == "f16":
        want = _run(c, dev, value, {})
        scaled = (value.float() * s).half()
        assert torch.equal(scaled.float() / s, value.float())
        got = _run(c, dev, scaled, dict(value_scale=s))
    else:
        s0 = torch.tensor([16.0], device='cuda')
        enc = ext.sca_rows_encode_q16(value.float().view(shape[0], shape[1], M * D), s0).view(shape[0], -1, M, D)
        want = _run(c, dev, enc, dict(value_layout="pairs", value_scale=s0))
        got = _run(c, dev, enc, dict(value_layout="pairs", value_scale=s0 * s)) * s
    assert float(want.abs().max()) > 0.1
    assert torch.equal(got, want)


@pytest.mark.parametrize("kernel", ["f16", "f16-hm"])
def test_fp16_subnormal_rows(kernel, monkeypatch):
    """fp16 rows below 2^-14 without a range scale: v_fma_mix_f32 widens the subnormal halves exactly (the kernels are compiled
    in the default mode, which keeps fp16 denormals), so the result matches the reference on the stored values."""
    fmt = _select(kernel, monkeypatch)
    amp = 2.0 ** -14 / 6
    c, dev = _case(MAIN, amp)
    rows = dev['value'].clamp(-(2.0 ** -14 - 2.0 ** -24), 2.0 ** -14 - 2.0 ** -24).half()
    stored = rows.cpu().double()
    assert float(stored.abs().max()) < 2.0 ** -14 and float((stored != 0).double().mean()) > 0.95
    ref = case_ref(c, stored)
    out = _run(c, dev, rows, {})
    d = _err(out, ref)
    print(f"{kernel} fp16 subnormal rows (max|v| {float(stored.abs().max()):.3e}): max|hip - reference(f64)| = {d:.3e}, "
          f"max|reference| {float(ref.abs().max()):.3e}, max|hip| {float(out.abs().max()):.3e} (bound {GPU_TOL * amp:.1e})")
    assert float(ref.abs().max()) > 0.5 * amp
    assert d < GPU_TOL * amp


@pytest.mark.parametrize("kind", ["random", "reversed"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_order_only_decides_which_wave_computes_a_row(kernel, kind, monkeypatch):
    """On the head-major kernel the permutation changes which 8 queries share a wave, so every query meets another union of
    cameras: the dead samples of the cameras it does not see must add exactly nothing."""
    fmt = _select(kernel, monkeypatch)
    c, dev = _case(MAIN)
    rows, kw, _ = _rows(MAIN, fmt)
    Nq = c['Nq']
    order = _perm32(Nq, 11) if kind == "random" else torch.arange(Nq - 1, -1, -1, dtype=torch.int32)
    assert order.dtype == torch.int32 and torch.equal(order.long().sort().values, torch.arange(Nq))
    plain = _run(c, dev, rows, kw)
    order = order.cuda()
    assert order.is_contiguous()
    _nan_prefill(c)
    out = _run(c, dev, rows, kw, order=order)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, plain)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("case", ["L4P8_Z4_B2", "L4P4_Z2_B2"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_column_slices_of_one_linear_output(kernel, case, pad, monkeypatch):
    """offs / logits as the column slices 0 and 2*M*L*P of one wider Linear output (how the production callers pass them),
    without and with trailing pad columns."""
    fmt = _select(kernel, monkeypatch)
    i = CASE_IDS.index(case)
    c, dev = _case(i)
    rows, kw, _ = _rows(i, fmt)
    n = M * c['L'] * c['P']
    lin = torch.full((c['B'], c['Nq'], 3 * n + pad), float('nan'), device='cuda')
    lin[..., :2 * n] = dev['offs']
    lin[..., 2 * n:3 * n] = dev['logits']
    o, l = lin[..., :2 * n], lin[..., 2 * n:3 * n]
    assert not o.is_contiguous() and o.stride(1) == 3 * n + pad and l.data_ptr() == lin.data_ptr() + 8 * n
    out = _run(c, dev, rows, kw, offs=o, logits=l)
    assert torch.equal(out, _run(c, dev, rows, kw))


@pytest.mark.parametrize("kernel", KERNELS)
def test_non_finite_locations_contribute_nothing(kernel, monkeypatch):
    """A sample whose location is +-Inf or NaN — through its anchor or its offset — fails the admission test (csrc/common.h
    bilinear_terms): weight 0 and the dead offset on all four corners, no load."""
    fmt = _select(kernel, monkeypatch)
    c, dev = _case(MAIN)
    rows, kw, _ = _rows(MAIN, fmt)
    B, Nq, L, P = c['B'], c['Nq'], c['L'], c['P']
    inf, nan = float('inf'), float('nan')
    ref_cam, offs = c['ref_cam'].clone(), c['offs'].clone()
    o = offs.view(B, Nq, M, L, P, 2)
    # queries 19-23: every camera sees them in batch element 0, and they hold no placed sample
    assert all(int(c['vis'][0, q]) == 63 for q in range(19, 24))
    ref_cam[2, 0, 19, 1] = inf                             # one anchor of one camera: points 1 and 5 of every head and level
    ref_cam[3, 1, 20, 0, 0] = nan                          # x alone, batch element 1
    ref_cam[0, 0, 21] = -inf                               # a whole camera of a query
    ref_cam[5, 1, 21, 2, 1] = inf
    o[0, 22, 3] = nan                                      # head 3: every sample, in every camera
    o[1, 23, 5, 1, 2, 1] = inf                             # one sample, y alone
    o[0, 19, 0, 0, 0, 0] = -inf
    o[0, 23, 6, :, :, 0] = nan                             # head 6: every sample through x alone
    stored = _stored(MAIN, fmt)[2]
    ref = sca_gather_ref(stored, c['shapes'], offs, c['logits'], ref_cam, c['vis'], P, c['Z'])
    assert bool(torch.isfinite(ref).all())
    out = _run(c, dev, rows, kw, offs=offs.cuda(), ref_cam=ref_cam.cuda())
    assert bool(torch.isfinite(out).all())
    d = _err(out, ref)
    print(f"{kernel} non-finite anchors and offsets: max|hip - reference(f64)| = {d:.3e}")
    assert d < GPU_TOL
    got, want = out.view(B, Nq, M, D).cpu(), ref.view(B, Nq, M, D)
    for b, q, m in [(0, 22, 3), (0, 23, 6)]:               # dead heads
        assert float(got[b, q, m].abs().max()) == 0.0 and float(want[b, q, m].abs().max()) == 0.0, (b, q, m)
    for b, q, m in [(0, 19, 0), (1, 23, 5), (0, 21, 0), (1, 20, 2)]:          # partly dead heads still gather their live samples
        assert float(want[b, q, m].abs().max()) > 0.0 and float(got[b, q, m].abs().max()) > 0.0, (b, q, m)


@pytest.mark.parametrize("ordered", [False, True], ids=["plain", "order"])
@pytest.mark.parametrize("i", TAILS, ids=[CASE_IDS[i] for i in TAILS])
@pytest.mark.parametrize("kernel", KERNELS)
def test_tails(kernel, i, ordered, monkeypatch):
    """Nq = 1, 7, 33: a partly filled wave of 8 queries (head-major) and a partly filled block of 4 (query-major).  Every row
    is written and matches the reference."""
    fmt = _select(kernel, monkeypatch)
    c, dev = _case(i)
    rows, kw, ref = _rows(i, fmt)
    order = torch.arange(c['Nq'] - 1, -1, -1, dtype=torch.int32).cuda() if ordered else None
    _nan_prefill(c)
    out = _run(c, dev, rows, kw, order=order)
    assert out.shape == (c['B'], c['Nq'], M * D) and not bool(torch.isnan(out).any())
    d = _err(out, ref)
    print(f"{kernel} {CASE_IDS[i]} {'order' if ordered else 'plain'}: max|hip - reference(f64)| = {d:.3e}")
    assert d < GPU_TOL


@pytest.mark.parametrize("case", ["L4P8_Z8_B2", "L4P8_Z2_B1", "L4P4_Z2_B2", "L2P8_Z8_B2", "L1P8_Z1_B2", "L4P8_Z4_B2_NC1",
                                  "L4P8_Z2_B2_Nq7", "L4P8_Z8_B2_Nq1"])
def test_stats(case, monkeypatch):
    """stats = (visible (b, q, camera) rows, bilinear corners inside their map): the five kernels evaluate the same fp32
    locations and agree exactly; the rows equal the reference's count, the corners the float64 count up to the coordinates
    that fp32 may put on the other side of a deciding integer (sca_ref.sca_counts: two corners each)."""
    i = CASE_IDS.index(case)
    c, dev = _case(i)
    want_rows, want_corners, near = sca_counts(c['shapes'], c['offs'], c['logits'], c['ref_cam'], c['vis'], c['P'], c['Z'])
    seen = {}
    for kernel in KERNELS:
        fmt = _select(kernel, monkeypatch)
        rows, kw, _ = _rows(i, fmt)
        stats = torch.zeros(2, dtype=torch.int64, device='cuda')
        _run(c, dev, rows, kw, stats=stats)
        seen[kernel] = tuple(stats.tolist())
    print(f"{case}: stats {seen['f32']}, reference rows {want_rows}, corners(f64) {want_corners}, near a deciding integer {near}")
    assert all(v == seen['f32'] for v in seen.values()), seen
    assert seen['f32'][0] == want_rows
    assert abs(seen['f32'][1] - want_corners) <= 2 * near


def test_refusals_launch_nothing(monkeypatch):
    """ext.sca_fused_forward raises the library's alignment conditions from the tensors themselves."""
    from occnet_amd import ext
    from occnet_amd._lib import OccAmdError
    c, dev = _case(MAIN)
    B, Nq, n = c['B'], c['Nq'], M * c['L'] * c['P']
    half, _, _ = _rows(MAIN, "f16")
    monkeypatch.setenv("OCC_SCA_HEAD_MAJOR", "1")
    f = lambda rows=dev['value'], **over: _run(c, dev, rows, {}, **over)
    wide = torch.zeros(B, Nq, 2 * n + 6, device='cuda')
    odd = torch.zeros(B, Nq, 2 * n + 1, device='cuda')
    with pytest.raises(OccAmdError, match="even row stride"):
        f(offs=odd[..., :2 * n])
    with pytest.raises(OccAmdError, match="8-byte aligned"):
        f(offs=wide[..., 1:2 * n + 1])
    assert f(offs=wide[..., 2:2 * n + 2]).shape == (B, Nq, M * D)       # fp32 rows: an even column of an even-stride buffer
    with pytest.raises(OccAmdError, match="multiples of 4"):
        f(half, offs=wide[..., 2:2 * n + 2])                           # 16-bit rows, L*P = 32: 16-byte loads
    with pytest.raises(OccAmdError, match="multiples of 4"):
        f(half, offs=wide[..., :2 * n])                                # row stride 2 n + 6
    lw = torch.zeros(B, Nq, n + 4, device='cuda')
    with pytest.raises(OccAmdError, match="multiples of 4"):
        f(half, logits=lw[..., 2:n + 2])
    assert f(half, logits=lw[..., 4:]).shape == (B, Nq, M * D)
    flat = torch.zeros(dev['value'].numel() + 4, device='cuda')
    with pytest.raises(OccAmdError, match="value must be 16-byte aligned"):
        f(flat[1:1 + dev['value'].numel()].view(dev['value'].shape))
    rflat = torch.zeros(dev['ref_cam'].numel() + 4, device='cuda')
    with pytest.raises(OccAmdError, match="ref_cam must be 8-byte aligned"):
        f(ref_cam=rflat[1:1 + dev['ref_cam'].numel()].view(dev['ref_cam'].shape))
    r8 = rflat[2:2 + dev['ref_cam'].numel()].view(dev['ref_cam'].shape)
    with pytest.raises(OccAmdError, match="ref_cam must be 16-byte aligned"):
        f(half, ref_cam=r8)                                            # the head-major kernel's 16-byte anchor loads (Z = 4)
    monkeypatch.setenv("OCC_SCA_HEAD_MAJOR", "0")
    assert f(half, ref_cam=r8).shape == (B, Nq, M * D)                 # the query-major kernel reads float2 anchors
    torch.cuda.synchronize()
