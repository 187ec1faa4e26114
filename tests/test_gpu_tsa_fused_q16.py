"""-m gpu: the q16 value rows of the fused temporal self-attention gather (OCC_TSA_VALUES=q16) — the gather kernel
(ext.tsa_fused_forward on int16 rows -> occ_tsa_fused_forward_q16v), the value projection that writes them
(ext.linear_q16rows -> occ_linear_bf16x3_q16rows), their range scale (ext.tsa_value_scale) and the switch in
TemporalSelfAttention.fused_gather.

The gather is held to the float64 reference of tests/tsa_ref.py on the STORED values — what tests/q16_ref.decode makes of the
int16 the device encoder wrote (the method of tests/test_gpu_sca_fused.py) — under the project's bound for a gather that
accumulates in fp32, GPU_TOL times the value amplitude: storage error is the encoder's business and is measured apart
(test_module_*).  Maps of at most 168 pixels; one Linear of 33 k rows for the 64-row tile choice."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from tests import q16_ref
from tests.tsa_q16_ref import pattern_value
from tests.tsa_ref import CASE_IDS, CASES, GPU_TOL, SEED, D, M, P, tsa_case, tsa_gather_ref

pytestmark = pytest.mark.gpu

AMPS = (1.0, 1e-3, 1e4)


@functools.lru_cache(maxsize=None)
def _case(i):
    """CPU inputs of case i and their device copies, made once and never written to."""
    B, H, W, spread = CASES[i]
    inp = tsa_case(B, H, W, SEED, spread)
    return inp, tuple(t.cuda() for t in inp)


def _idx(B, H, W):
    return next(i for i, c in enumerate(CASES) if c[:3] == (B, H, W))


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


def _scale_of(s):
    return 1.0 if s is None else float(s.item())


def _stored(rows, s, S):
    """int16 pixel pairs (maps, S_pad, M*D) as the device wrote them -> the float64 values they hold, (maps, S, M, D)."""
    from occnet_amd import ext
    q = ext.sca_unpair_layout(rows.cpu().view(rows.shape[0], rows.shape[1], M, D), S)
    return torch.from_numpy(q16_ref.decode(q.contiguous().numpy(), _scale_of(s)))


@functools.lru_cache(maxsize=None)
def _encoded(i, amp, scaled):
    """Case i's value maps times amp as q16 rows on the device (+ their scale), and the float64 reference on what they hold."""
    from occnet_amd import ext
    B, H, W, _ = CASES[i]
    (value, offs, logits, ref_2d), (value_d, _, _, _) = _case(i)
    v = (value_d * amp).view(B * 2, H * W, M * D)
    if scaled:
        rows, s = ext.q16_range_scaled(v)
    else:
        rows, s = ext.sca_rows_encode_q16(v, None), None
    assert rows.dtype == torch.int16 and tuple(rows.shape) == (B * 2, H * W + (H * W & 1), M * D)
    stored = _stored(rows, s, H * W)
    return rows, s, stored, tsa_gather_ref(stored, offs, logits, ref_2d, H, W, M, P)


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "range_scaled"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_matches_reference_on_stored_values(i, scaled):
    from occnet_amd import ext
    B, H, W, _ = CASES[i]
    (value, _, _, _), (_, offs, logits, ref_2d) = _case(i)
    for amp in AMPS:
        rows, s, stored, ref = _encoded(i, amp, scaled)
        out = ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, M, P, value_scale=s)
        d = _err(out, ref)
        # how far the stored values are from the fp32 ones (not asserted here: the encoder's tests and test_module_* own it)
        sd = float((stored - (value * amp).double()).abs().max())
        print(f"{CASE_IDS[i]} amp {amp:g} s {_scale_of(s):g}: max|hip - reference(f64 on stored)| = {d:.3e} "
              f"(bound {GPU_TOL * amp:.1e}); max|stored - fp32| = {sd:.3e}")
        assert out.shape == (B, H * W, M * D) and out.dtype == torch.float32
        assert float(ref.abs().max()) > 0.1 * amp
        assert d < GPU_TOL * amp


@pytest.mark.parametrize("B,H,W", [(1, 9, 7), (2, 9, 7)], ids=["B1_stride0_alias", "B2_stack"])
def test_shared_queue(B, H, W):
    from occnet_amd import ext
    i = _idx(B, H, W)
    (_, offs, logits, ref_2d), (_, offs_d, logits_d, ref_d) = _case(i)
    rows, s, stored, _ = _encoded(i, 1.0, True)
    S, Sp = H * W, rows.shape[1]
    one = rows.view(B, 2, Sp, M * D)[:, 1].contiguous()                        # (B, S_pad, C): queue entry 1 of every batch
    st = stored.view(B, 2, S, M, D)[:, 1]
    ref = tsa_gather_ref(torch.stack([st, st], 1).reshape(B * 2, S, M, D), offs, logits, ref_2d, H, W, M, P)
    out = ext.tsa_fused_forward(one, offs_d, logits_d, ref_d, H, W, M, P, shared_queue=True, value_scale=s)
    d = _err(out, ref)
    print(f"shared_queue B={B}: max|hip - reference(f64 on stored)| = {d:.3e}")
    assert d < GPU_TOL
    # the same numbers read through one buffer (stride 0) or through two copies of it
    twice = torch.stack([one, one], 1).reshape(B * 2, Sp, M * D).contiguous()
    assert torch.equal(out, ext.tsa_fused_forward(twice, offs_d, logits_d, ref_d, H, W, M, P, value_scale=s))


@pytest.mark.parametrize("B,H,W", [(1, 12, 14), (2, 9, 7), (1, 5, 31)], ids=["B1_12x14", "B2_9x7", "B1_5x31"])
def test_order_only_decides_which_wave_computes_a_row(B, H, W):
    from occnet_amd import ext
    i = _idx(B, H, W)
    _, (_, offs, logits, ref_2d) = _case(i)
    rows, s, _, ref = _encoded(i, 1.0, True)
    Nq = H * W
    order = torch.randperm(Nq, generator=torch.Generator().manual_seed(11)).to(torch.int32).cuda()
    plain = ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, M, P, value_scale=s)
    junk = torch.full((B, Nq, M * D), float('nan'), device='cuda')      # the result's future storage holds NaN
    del junk
    out = ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, M, P, order=order, value_scale=s)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, plain)
    assert _err(out, ref) < GPU_TOL


@pytest.mark.parametrize("B,H,W", [(1, 12, 14), (2, 9, 7)], ids=["B1", "B2"])
@pytest.mark.parametrize("cols", [192, 200])
def test_column_slices_of_one_linear_output(B, H, W, cols):
    from occnet_amd import ext
    i = _idx(B, H, W)
    _, (_, offs, logits, ref_2d) = _case(i)
    rows, s, _, ref = _encoded(i, 1.0, True)
    lin = torch.full((B, H * W, cols), float('nan'), device='cuda')
    lin[..., :128] = offs
    lin[..., 128:192] = logits
    o, l = lin[..., :128], lin[..., 128:192]
    assert not o.is_contiguous() and o.stride(1) == cols
    out = ext.tsa_fused_forward(rows, o, l, ref_2d, H, W, M, P, value_scale=s)
    assert torch.equal(out, ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, M, P, value_scale=s))
    assert _err(out, ref) < GPU_TOL


@pytest.mark.parametrize("r0,r1", [(3, 8), (5, 6)], ids=["rows_3_to_7", "one_row"])
def test_row_band(r0, r1):
    """value_rows: the queries are rows r0 .. r1-1 of the BEV, the value maps the whole BEV."""
    from occnet_amd import ext
    B, H, W = 1, 12, 14
    i = _idx(B, H, W)
    (_, offs_c, logits_c, ref_c), (_, offs, logits, ref_2d) = _case(i)
    rows, s, stored, _ = _encoded(i, 1.0, True)
    q0, q1 = r0 * W, r1 * W
    full = ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, M, P, value_scale=s)
    band = (offs[:, q0:q1], logits[:, q0:q1], ref_2d[:, q0:q1].contiguous())
    out = ext.tsa_fused_forward(rows, *band, H, W, M, P, value_rows=H * W, value_scale=s)
    assert out.shape == (1, q1 - q0, M * D)
    assert torch.equal(out, full[:, q0:q1])
    order = torch.randperm(q1 - q0, generator=torch.Generator().manual_seed(12)).to(torch.int32).cuda()
    assert torch.equal(ext.tsa_fused_forward(rows, *band, H, W, M, P, value_rows=H * W, order=order, value_scale=s), out)
    ref = tsa_gather_ref(stored, offs_c[:, q0:q1], logits_c[:, q0:q1], ref_c[:, q0:q1], H, W, M, P)
    d = _err(out, ref)
    print(f"band rows {r0}..{r1 - 1}: max|hip - reference(f64 on stored)| = {d:.3e}")
    assert d < GPU_TOL


def _capi(value_ptr, stride, rows, offs, logits, ref_2d, out, B, Nq, H, W, m=M, d=D, p=P, scale=None):
    from occnet_amd import _lib
    from occnet_amd._lib import i32, i64, ptr, stream_ptr
    return _lib.lib().occ_tsa_fused_forward_q16v(
        ctypes.c_void_p(value_ptr), i64(stride), i32(rows), ptr(offs), i64(offs.stride(1)), ptr(logits),
        i64(logits.stride(1)), ptr(ref_2d), ptr(None), ptr(out), i32(B), i32(Nq), i32(H), i32(W), i32(m), i32(d), i32(p),
        ptr(scale), stream_ptr(out.device))


@pytest.mark.parametrize("B,H,W", [(1, 9, 7), (2, 9, 7), (1, 12, 14)], ids=["B1_9x7_pad_row", "B2_9x7_pad_row", "B1_12x14"])
def test_never_reads_outside_the_map(B, H, W):
    """Corners outside the map are not loaded: int16 patterns that decode to the largest value q16 rows can hold (0x7fff in
    every element: E = 15, mantissas 32767 — twice the bound of the plane under its scale) in front of, between and behind the padded maps — the maps of a batch entry lie a guard apart
    inside the ONE descriptor the kernel builds over both — and in the pad row of the odd maps change nothing."""
    i = _idx(B, H, W)
    _, (_, offs, logits, ref_2d) = _case(i)
    rows, s, _, ref = _encoded(i, 1.0, True)
    S, Sp = H * W, rows.shape[1]
    per, guard = Sp * M * D, 2048                                           # elements; the guard keeps 16-byte alignment
    outs = []
    for fill in (0, 0x7fff):
        buf = torch.full((guard + B * 2 * (per + guard),), fill, dtype=torch.int16, device='cuda')
        maps = buf[guard:].view(B * 2, per + guard)[:, :per]
        maps.copy_(rows.view(B * 2, per))
        if S & 1:      # the pad pixel: second slot of the last pair, every head
            maps.view(B * 2, Sp // 2, M, 2, D)[:, -1, :, 1, :] = fill
        out = torch.full((B, S, M * D), float('nan'), device='cuda')
        assert _capi(buf.data_ptr() + guard * 2, per + guard, Sp, offs, logits, ref_2d, out, B, S, H, W, scale=s) == 0
        outs.append(out)
    assert bool(torch.isfinite(outs[1]).all())
    assert torch.equal(outs[0], outs[1])
    assert _err(outs[1], ref) < GPU_TOL
    # the hostile pattern is the largest value the format holds under this scale: twice the plane's bound
    assert float(q16_ref.decode(np.full(8, 0x7fff, np.int16), _scale_of(s)).max()) > float(ref.abs().max())


def test_non_finite_locations_contribute_nothing():
    from occnet_amd import ext
    B, H, W = 1, 12, 14
    i = _idx(B, H, W)
    (_, offs_c, logits_c, ref_c), (_, _, logits, ref_2d) = _case(i)
    rows, s, stored, _ = _encoded(i, 1.0, True)
    offs_c = offs_c.clone()
    o = offs_c.view(B, H * W, M, 2, P, 2)
    inf, nan = float('inf'), float('nan')
    o[0, 20, 0:4] = inf                                   # heads 0-3: all 8 samples
    o[0, 20, 5, 0, 1, 0] = inf                            # head 5: one sample, x only
    o[0, 77, 2] = -inf
    o[0, 77, 6, 1] = -inf                                 # head 6: every sample of queue entry 1
    o[0, 150, 7] = nan
    o[0, 150, 1, 0, 2, 1] = nan
    o[0, 150, 3, :, :, 0] = nan                           # head 3: all 8 samples through x alone
    dead = [(20, 0), (20, 1), (20, 2), (20, 3), (77, 2), (150, 7), (150, 3)]
    ref = tsa_gather_ref(stored, offs_c, logits_c, ref_c, H, W, M, P)
    assert bool(torch.isfinite(ref).all())
    out = ext.tsa_fused_forward(rows, offs_c.cuda(), logits, ref_2d, H, W, M, P, value_scale=s)
    assert bool(torch.isfinite(out).all())
    assert _err(out, ref) < GPU_TOL
    got, want = out.view(H * W, M, D), ref.view(H * W, M, D)
    for q, m in dead:
        assert float(got[q, m].abs().max()) == 0.0 and float(want[q, m].abs().max()) == 0.0, (q, m)
    for q, m in [(20, 5), (77, 6), (150, 1)]:             # partly dead heads still gather their live samples
        assert float(want[q, m].abs().max()) > 0.0 and float(got[q, m].abs().max()) > 0.0, (q, m)


def test_refusals_launch_nothing():
    from occnet_amd import _lib, ext
    from occnet_amd._lib import OccAmdError, OccAmdUnsupported
    B, H, W = 1, 9, 7
    i = _idx(B, H, W)
    _, (_, offs, logits, ref_2d) = _case(i)
    rows, s, _, _ = _encoded(i, 1.0, True)
    S, Sp = H * W, rows.shape[1]
    per = Sp * M * D
    out = torch.full((B, S, M * D), float('nan'), device='cuda')
    last = lambda: _lib.lib().occ_last_error()
    big = torch.zeros(2 * per + 64, dtype=torch.int16, device='cuda')
    call = lambda ptr_=big.data_ptr(), stride=per, rows_=Sp, **kw: _capi(ptr_, stride, rows_, offs, logits, ref_2d, out,
                                                                        B, S, H, W, **kw)
    assert call(ptr_=big.data_ptr() + 8) == -1 and b'16-byte aligned' in last()             # misaligned value
    assert call(ptr_=big.data_ptr() + 2) == -1 and b'16-byte aligned' in last()
    assert call(rows_=S, stride=S * M * D) == -1 and b'rounded up to even' in last()        # odd padded row count
    assert call(stride=per - 8) == -1 and b'value stride' in last()                         # a stride smaller than a map
    assert call(stride=S * M * D) == -1 and b'value stride' in last()                       # (the unpadded map's size)
    # shapes without a kernel (consistent buffers: every argument check passes)
    z = lambda *shape: torch.zeros(*shape, device='cuda')
    for m, d, p in ((4, 32, 4), (8, 64, 4), (8, 32, 8)):
        o, l = z(B, S, m * 2 * p * 2), z(B, S, m * 2 * p)
        v = torch.zeros(2 * Sp * m * d, dtype=torch.int16, device='cuda')
        o2 = torch.full((B, S, m * d), float('nan'), device='cuda')
        assert _capi(v.data_ptr(), Sp * m * d, Sp, o, l, ref_2d, o2, B, S, H, W, m=m, d=d, p=p) == -3
        assert bool(torch.isnan(o2).all())
        with pytest.raises(OccAmdUnsupported):
            ext.tsa_fused_forward(v.view(2, Sp, m, d), o, l, ref_2d, H, W, m, p)
    # the wrapper's own checks
    with pytest.raises(OccAmdError, match="rounded up to even"):
        ext.tsa_fused_forward(rows[:, :S].contiguous(), offs, logits, ref_2d, H, W, M, P)
    with pytest.raises(OccAmdError, match="16-byte aligned"):
        ext.tsa_fused_forward(big[4:4 + 2 * per].view(2, Sp, M * D), offs, logits, ref_2d, H, W, M, P)
    with pytest.raises(OccAmdError, match="value_scale"):
        ext.tsa_fused_forward(rows, offs, logits, ref_2d, H, W, M, P, value_scale=torch.ones(1))      # on the CPU
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(scale=s) == 0                                                               # and the good call does launch
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


# ---- the value projection that writes the rows ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(sign=False):
    g = torch.Generator().manual_seed(31)
    w = torch.randn(256, 256, generator=g) / 16.0
    b = torch.randn(256, generator=g)
    if sign:
        w, b = w.abs(), b.abs()
    return w.cuda(), b.cuda()


def _pow2_scale(y):
    amax = y.abs().amax()
    _, e = torch.frexp(amax)
    return torch.ldexp(torch.ones_like(amax), 15 - e).reshape(1)


# S rows per map x maps: one row; odd S; odd S with two maps; even S with two maps; 512 64-row blocks and more (the 64-row
# tile choice of occ_linear_bf16x3_f32: ceil(M / 64) >= 512), odd S, a partial last block
LINEAR_SHAPES = [(1, 1), (63, 1), (65, 2), (200, 2), (16417, 2)]


@pytest.mark.parametrize("S,groups", LINEAR_SHAPES, ids=[f"{s}x{g}" for s, g in LINEAR_SHAPES])
def test_linear_epilogue_is_the_encoder_bit_for_bit(S, groups):
    from occnet_amd import ext
    w, b = _weights()
    Mrows = S * groups
    assert (Mrows + 63) // 64 >= 512 if S > 10000 else (Mrows + 63) // 64 < 512
    a = torch.randn(Mrows, 256, generator=torch.Generator().manual_seed(S)).cuda() * 3.0
    a[:: 7] *= 1e-3                                                       # pieces far below the plane's maximum: small exponents
    y = ext.linear(a, w, b)
    for s in (_pow2_scale(y), None):
        out = ext.linear_q16rows(a, w, b, s, groups)
        assert out.dtype == torch.int16 and tuple(out.shape) == (groups, S + (S & 1), 256)
        want = q16_ref.pair_layout(q16_ref.encode(y.cpu().numpy().reshape(groups, S, 8, 32), _scale_of(s), 8))
        got = out.cpu().numpy().reshape(want.shape)
        bad = int((got != want).sum())
        print(f"{S}x{groups} scale {_scale_of(s):g}: {bad} of {want.size} int16 differ from q16_ref.encode(ext.linear)")
        assert bad == 0
        if S & 1:
            assert not out.view(groups, (S + 1) // 2, 8, 2, 32)[:, -1, :, 1, :].any()
        assert torch.equal(out, ext.linear_q16rows(a, w, b, s, groups))
        if s is not None:                                                 # and the stand-alone encoder agrees
            assert torch.equal(out, ext.sca_rows_encode_q16(y.view(groups, S, 256), s))
    if S == 200:
        assert torch.equal(ext.linear_q16rows(a.view(2, 200, 256), w, None, None, 2),
                           ext.sca_rows_encode_q16(ext.linear(a, w, None).view(2, 200, 256), None))


def test_linear_epilogue_refusals_launch_nothing():
    from occnet_amd import ext
    from occnet_amd._lib import OccAmdError, OccAmdUnsupported
    w, b = _weights()
    a = torch.randn(64, 256, device='cuda')
    with pytest.raises(OccAmdUnsupported, match="N=128"):
        ext.linear_q16rows(a, w[:128].contiguous(), b[:128].contiguous(), None, 1)
    with pytest.raises(OccAmdUnsupported, match="residual"):
        ext.linear_q16rows(a, w, b, None, 1, residual=torch.zeros(64, 256, device='cuda'))
    with pytest.raises(OccAmdUnsupported):
        ext.linear_q16rows(a[:, :248], w[:, :248].contiguous(), b, None, 1)             # K % 16
    with pytest.raises(OccAmdError, match="split"):
        ext.linear_q16rows(a, w, b, None, 3)
    torch.cuda.synchronize()


def test_scale_from_the_layernorm_bound_never_wraps():
    """The worst case of the range rule: max|a| IS the attached bound, in a row where every element has it with the sign of
    its weights, so the L1 bound is reached.  No mantissa wraps — every stored element stays within the half step of its piece
    of the fp32 Linear output (two steps for the two tagged elements, whose step is four units)."""
    from occnet_amd import ext
    w, b = _weights(sign=True)
    g = torch.Generator().manual_seed(41)
    ln = torch.nn.LayerNorm(256)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(256, generator=g))
        ln.bias.copy_(torch.randn(256, generator=g) * 0.3)
    ln = ln.cuda()
    words = ext.layernorm_bound_words(ln)
    bound = float(pattern_value(np.int64(int(words[0].item()))))
    a = (torch.rand(130, 256, generator=g) * 2 - 1) * bound
    a[0] = bound
    a[1] = -bound
    a[2, ::2] = bound
    a = a.cuda()
    assert float(a.abs().max()) == bound

    s = ext.tsa_value_scale(types.SimpleNamespace(weight=w, bias=b), words)
    sv = float(s.item())
    assert np.frexp(sv)[0] == 0.5
    y = ext.linear(a, w, b).cpu()
    top = float(y.abs().max()) * sv
    print(f"bound {bound:.4f}, s = 2^{int(np.log2(sv))}, max|y| * s = 2^{np.log2(top):.3f}")
    assert 2.0 ** 13 < top <= 2.0 ** 15
    rows = ext.linear_q16rows(a, w, b, s, 2)
    assert torch.equal(rows, ext.sca_rows_encode_q16(y.cuda().view(2, 65, 256), s))
    q = ext.sca_unpair_layout(rows.cpu().view(2, 66, 8, 32), 65).contiguous().numpy().reshape(-1, 8)
    E = (q[:, 0].astype(np.int64) & 3) | ((q[:, 1].astype(np.int64) & 3) << 2)
    unit = np.ldexp(1.0, E - 15) / (sv * 0.5)                               # value of one mantissa step, per piece
    dev = np.abs(q16_ref.decode(q, sv) - y.numpy().astype(np.float64).reshape(-1, 8)) / unit[:, None]
    print(f"largest deviation in mantissa steps: tagged {dev[:, :2].max():.3f}, others {dev[:, 2:].max():.3f}")
    assert dev[:, 2:].max() <= 0.5 and dev[:, :2].max() <= 2.0
    assert int(np.abs(q.astype(np.int64)).max()) < 32768 and int(E.max()) >= 13


# ---- the switch in the module --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _module():
    from occnet_amd.plugin.temporal_self_attention import TemporalSelfAttention
    torch.manual_seed(51)
    m = TemporalSelfAttention(embed_dims=256, num_heads=8, num_levels=1, num_points=4)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0.0, 0.02)
        m.attention_weights.weight.normal_(0.0, 0.05)
    return m.cuda().eval()


def _module_inputs(history):
    g = torch.Generator().manual_seed(52)
    H, W = 12, 14
    q = torch.randn(1, H * W, 256, generator=g)
    pos = torch.randn(1, H * W, 256, generator=g) * 0.5
    ref = torch.rand(2, H * W, 1, 2, generator=g)
    value = torch.stack([torch.randn(1, H * W, 256, generator=g) * 2.0, q], 1).reshape(2, H * W, 256) if history else None
    return q, pos, ref, value, H, W


@pytest.mark.parametrize("history", [False, True], ids=["no_history", "history"])
def test_module_switch(history, monkeypatch):
    """fused_gather under OCC_TSA_VALUES=q16 against the same call on fp32 rows.  Tolerance: twice the deviation that storing
    THESE value rows as q16 causes in the float64 reference (measured here on the CPU), plus GPU_TOL.  With the switch unset
    the call is the parent's: bit-identical to a direct ext.tsa_fused_forward on the fp32 rows.  (The measured figures are
    printed, and recorded in DESIGN.md.)"""
    from occnet_amd import ext
    m = _module()
    q, pos, ref, value, H, W = _module_inputs(history)
    qd, posd, refd = q.cuda(), pos.cuda(), ref.cuda()
    vd = None if value is None else value.cuda()
    seen = []
    real = ext.tsa_fused_forward
    monkeypatch.setattr(ext, "tsa_fused_forward", lambda v, *a, **k: (seen.append(v.dtype), real(v, *a, **k))[1])

    monkeypatch.setattr(ext, "TSA_VALUES", "f32")
    out32 = m.fused_gather(qd, vd, posd, refd, H, W)
    # the parent's computation, spelled out
    n_off = m.sampling_offsets.out_features
    wcat, bcat = m._qcat.get((m.sampling_offsets, m.attention_weights))
    if history:
        lin = ext.linear(vd[:1].contiguous(), wcat, bcat, a2=qd, a2_add=posd)
        v32 = ext.linear(vd, m.value_proj.weight, m.value_proj.bias)
    else:
        w_sum, pos_term = m._folded_query_weights(wcat, bcat, posd)
        lin, v32 = ext.linear_pair_chain(qd, w_sum, pos_term, m.value_proj.weight, m.value_proj.bias)
    direct = real(v32.view(v32.shape[0], H * W, M, D), lin[..., :n_off], lin[..., n_off:], refd, H, W, M, P,
                  shared_queue=not history)
    assert torch.equal(out32, direct)
    assert seen == [torch.float32]

    monkeypatch.setattr(ext, "TSA_VALUES", "q16")
    outq = m.fused_gather(qd, vd, posd, refd, H, W)
    assert seen == [torch.float32, torch.int16]

    # storage-induced deviation of the float64 reference for these exact inputs
    src = qd if vd is None else vd
    sv = float(ext.tsa_value_scale(m.value_proj, ext.absmax_words_f32(src)).item())
    v = v32.cpu().view(-1, H * W, M, D)
    if not history:
        v = torch.cat([v, v], 0)
    stored = torch.from_numpy(q16_ref.decode(q16_ref.encode(v.numpy(), sv, 8), sv))
    offs, logits = lin[..., :n_off].cpu().contiguous(), lin[..., n_off:].cpu().contiguous()
    ref32 = tsa_gather_ref(v, offs, logits, ref, H, W, M, P)
    refq = tsa_gather_ref(stored, offs, logits, ref, H, W, M, P)
    storage = float((ref32 - refq).abs().max())
    tol = 2.0 * storage + GPU_TOL
    d = float((outq - out32).abs().max())
    print(f"history={history}: s = {sv:g}, storage deviation (f64 reference) {storage:.3e}, tolerance {tol:.3e}, "
          f"max|q16 - f32| on the device {d:.3e}, max|out| {float(out32.abs().max()):.3f}")
    assert float(ref32.abs().max()) > 0.1 and storage > 0.0
    assert _err(out32, ref32) < GPU_TOL
    assert d <= tol


def test_layernorm_words_ride_along_and_an_in_place_write_drops_them(monkeypatch):
    from occnet_amd import ext
    m = _module()
    g = torch.Generator().manual_seed(61)
    ln = torch.nn.LayerNorm(256)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(256, generator=g) * 0.5 + 1.0)
        ln.bias.copy_(torch.randn(256, generator=g) * 0.1)
    ln = ln.cuda()
    a = torch.randn(1, 168, 256, generator=g).cuda()
    r = torch.randn(1, 168, 256, generator=g).cuda()
    w, b = _weights()
    monkeypatch.setattr(ext, "TSA_VALUES", "f32")
    assert ext.absmax_of(ext.linear(a, w, b, residual=r, ln=ln)) is None            # nothing rides along by default
    monkeypatch.setattr(ext, "TSA_VALUES", "q16")
    x = ext.linear(a, w, b, residual=r, ln=ln)
    words = ext.absmax_of(x)
    assert words is not None and torch.equal(words, ext.layernorm_bound_words(ln))
    y, _ = ext.linear_ln_chain(a, r, w, b, ln, w, b)
    assert torch.equal(ext.absmax_of(y), words)
    bound = float(pattern_value(np.int64(int(words[0].item()))))
    assert float(x.abs().max()) <= bound and float(y.abs().max()) <= bound
    rows_ln, s_ln = m._q16_rows(x, None)
    assert torch.equal(s_ln, ext.tsa_value_scale(m.value_proj, words))
    x.add_(0.0)                                                                     # an in-place write: the side band is stale
    assert ext.absmax_of(x) is None
    rows_m, s_m = m._q16_rows(x, None)
    measured = ext.tsa_value_scale(m.value_proj, ext.absmax_words_f32(x))
    assert torch.equal(s_m, measured)
    assert torch.equal(ext.absmax_of(x), ext.absmax_words_f32(x))                   # kept for the next layer
    assert float(s_ln.item()) <= float(s_m.item())                                  # the analytic bound is the safe side
    assert torch.equal(rows_m, ext.linear_q16rows(x, m.value_proj.weight, m.value_proj.bias, measured, 1))
