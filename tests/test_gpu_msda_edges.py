"""-m gpu: `ms_deform_attn_forward` / `ms_deform_attn_backward` against the closed-form float64 reference (tests/msda_ref.py)
where the other operator tests do not go: the decision set (integer pixel coordinates, the admission boundary, non-finite
locations), sparse output gradients (the zero-item skip of the D = 32 backward), the dispatch branches no other test
launches, generic head dims, the accumulation contract and the fp16 autograd node.

Bounds: the two the operator's files already hold - forward 2e-5 absolute (tests/test_gpu_msda.py), gradients 1e-4 of
max(1, max|ref|) (tests/test_gpu_backward.py).  On the decision set and on the dyadic location grid every decision and every
bilinear weight is exact in float32 (msda_ref.check_exact), so no sample is kept away from integer coordinates and none is
masked out of a comparison.  Observed values: EXPERIMENTS.md section 8w."""
import functools

import pytest
import torch

from tests import msda_ref as mr

pytestmark = pytest.mark.gpu

FWD_BOUND, GRAD_BOUND = 2e-5, 1e-4
ENV = ("OCC_MSDA_BWD_BIN", "OCC_MSDA_BWD_DETERMINISTIC", "OCC_MSDA_BWD_ATOMICS")
# the four D = 32 routes of occ_ms_deform_attn_backward_ws_f32 (msda_backward.hip): block-aggregated binning + float replay,
# wave-aggregated binning, fixed-point replay, msda_bwd_d32_kernel<true>
PATHS = {"block": {}, "wave": {"OCC_MSDA_BWD_BIN": "wave"}, "deterministic": {"OCC_MSDA_BWD_DETERMINISTIC": "1"},
         "atomics": {"OCC_MSDA_BWD_ATOMICS": "1"}}


def _set_path(monkeypatch, path):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _forward(inputs):
    from occnet_amd import ext
    value, shapes_t, start, loc, attn = inputs[:5]
    out = ext.ms_deform_attn_forward(value.cuda(), shapes_t.cuda(), start.cuda(), loc.cuda(), attn.cuda(), im2col_step=64)
    torch.cuda.synchronize()
    return out


def _backward(inputs, grad_out=None, prefill=None):
    from occnet_amd import ext
    value, shapes_t, start, loc, attn = inputs[:5]
    grad_out = inputs[5] if grad_out is None else grad_out
    if prefill is None:
        gv, gl, ga = (torch.zeros_like(t).cuda() for t in (value, loc, attn))
    else:
        gv, gl, ga = (t.clone().cuda() for t in prefill)
    ext.ms_deform_attn_backward(value.cuda(), shapes_t.cuda(), start.cuda(), loc.cuda(), attn.cuda(), grad_out.cuda(),
                                gv, gl, ga, im2col_step=64)
    torch.cuda.synchronize()
    return gv, gl, ga


def _check_forward(name, out, ref):
    d = float((out.cpu().double() - ref['out'].cpu()).abs().max())
    print(f"{name} forward: max|hip - closed form| = {d:.3e}")
    assert torch.isfinite(out).all()
    assert d < FWD_BOUND, (name, d)


def _check_grads(name, got, ref, skip=()):
    for nm, g in zip(("grad_value", "grad_loc", "grad_attn"), got):
        if nm in skip:
            continue
        r = ref[nm]
        scale = max(1.0, float(r.abs().max()))
        d = float((g.cpu().double() - r).abs().max()) / scale
        print(f"{name} {nm}: max rel diff = {d:.3e} (scale {scale:.2f})")
        assert torch.isfinite(g).all(), (name, nm)
        assert d < GRAD_BOUND, (name, nm, d)


def _check_dead_samples(name, got, dead):
    """grad_loc / grad_attn of the samples in `dead` (B, Lq, M, L, P): exactly 0.0 (and not NaN)."""
    gv, gl, ga = got
    dead = dead.cuda()
    n = int(dead.sum())
    worst = max(float(gl[dead].abs().max()), float(ga[dead].abs().max())) if n else 0.0
    print(f"{name}: {n} samples that must have zero grad_loc / grad_attn, largest magnitude {worst}")
    assert n > 0 and worst == 0.0 and not torch.isnan(gl[dead]).any() and not torch.isnan(ga[dead]).any()


# ---- the decision set ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decision(D):
    inputs = mr.decision_set(D=D)
    value, shapes_t, start, loc, attn, grad_out = inputs
    return inputs, mr.closed_form(value.double(), mr.DECISION_SHAPES, loc, attn, grad_out)


@pytest.mark.parametrize("D", [32, 16], ids=["d32_buffer", "d16_scalar"])
def test_decision_set_forward(D):
    inputs, ref = _decision(D)
    _check_forward(f"decision set D={D}", _forward(inputs), ref)


@pytest.mark.parametrize("path", list(PATHS))
def test_decision_set_backward_d32(path, monkeypatch):
    inputs, ref = _decision(32)
    _set_path(monkeypatch, path)
    got = _backward(inputs)
    _check_grads(f"decision set ({path})", got, ref)
    _check_dead_samples(f"decision set ({path})", got, ~ref['adm'])


def test_decision_set_backward_generic(monkeypatch):
    inputs, ref = _decision(16)
    _set_path(monkeypatch, "block")
    got = _backward(inputs)
    _check_grads("decision set (generic D=16)", got, ref)
    _check_dead_samples("decision set (generic D=16)", got, ~ref['adm'])


def test_decision_set_block_and_wave_binning_bit_identical(monkeypatch):
    """Fixed-point accumulation is order-independent: the two binning forms agree bit for bit exactly when they emit the
    same row items (tests/test_gpu_backward.py holds this on interior locations; here on every decision)."""
    inputs, ref = _decision(32)
    _set_path(monkeypatch, "deterministic")
    block = _backward(inputs)
    monkeypatch.setenv("OCC_MSDA_BWD_BIN", "wave")
    wave = _backward(inputs)
    for nm, a, b in zip(("grad_value", "grad_loc", "grad_attn"), wave, block):
        print(f"decision set {nm}: wave vs block binning, elements that differ: {int((a != b).sum())}")
        assert torch.equal(a, b), nm


# ---- sparse output gradients ---------------------------------------------------------------------------------------------------
# two binning blocks per (batch, head, level): Lq * P = 1200 > 1024; the 15-pixel level is one hot bin; M = 3 makes the
# 8-item groups of a wave ragged against the queries
SPARSE_SHAPES, SPARSE_B, SPARSE_M, SPARSE_LQ, SPARSE_P = [[12, 20], [3, 5]], 2, 3, 300, 4


@functools.lru_cache(maxsize=None)
def _sparse_inputs(D):
    return mr.dyadic_inputs(SPARSE_B, SPARSE_SHAPES, SPARSE_M, D, SPARSE_LQ, SPARSE_P, seed=41)


@functools.lru_cache(maxsize=None)
def _sparse_case(D, pattern):
    value, shapes_t, start, loc, attn, grad_out = _sparse_inputs(D)
    g, zero = mr.sparse_grad(grad_out, SPARSE_M, pattern)
    return g, zero, mr.closed_form(value.double(), SPARSE_SHAPES, loc, attn, g)


@pytest.mark.parametrize("pattern", mr.SPARSE_PATTERNS)
@pytest.mark.parametrize("path", list(PATHS) + ["generic_d16"])
def test_sparse_output_gradient(path, pattern, monkeypatch):
    D = 16 if path == "generic_d16" else 32
    assert SPARSE_LQ * SPARSE_P > 1024                                   # kBinBlockThreads: more than one binning block
    g, zero, ref = _sparse_case(D, pattern)
    _set_path(monkeypatch, "block" if D == 16 else path)
    got = _backward(_sparse_inputs(D), grad_out=g)
    name = f"sparse {pattern} ({path})"
    _check_grads(name, got, ref)
    if bool(zero.any()):
        dead = zero[..., None, None].expand_as(ref['adm'])
        _check_dead_samples(name, got, dead)
    if pattern == 'all_zero':                                            # an empty work list
        for nm, t in zip(("grad_value", "grad_loc", "grad_attn"), got):
            assert float(t.abs().max()) == 0.0 and not torch.isnan(t).any(), (name, nm)


# ---- dispatch branches ---------------------------------------------------------------------------------------------------------
SAMPLE_PARAM_BYTES, FWD_WAVES_PER_BLOCK, FWD_LDS_LIMIT = 32, 4, 64 * 1024      # msda_forward.hip: SampleParam, kWavesPerBlock
OOB_OFFSET = 0x7fffff00                                                        # common.h: kOobOffset
BIN_PIX, BIN_LDS_LIMIT, SCAN_BLOCK = 32, 48 * 1024, 1024                       # msda_backward.hip


def _fwd_lds_bytes(L, P):
    return FWD_WAVES_PER_BLOCK * 8 * (L * P + 1) * SAMPLE_PARAM_BYTES


@pytest.mark.parametrize("L,P,lds_kernel", [(3, 21, True), (4, 16, False)], ids=["LP63_lds_kernel_at_64KiB", "LP64_scalar_kernel"])
def test_forward_d32_at_the_lds_limit(L, P, lds_kernel):
    """D = 32 takes the LDS kernel while 4 * 8 * (L * P + 1) * 32 bytes fit 64 KiB: L * P = 63 asks for exactly 64 KiB of dynamic
    LDS, L * P = 64 is the scalar kernel at D = 32."""
    assert (_fwd_lds_bytes(L, P) <= FWD_LDS_LIMIT) == lds_kernel
    assert not lds_kernel or _fwd_lds_bytes(L, P) == FWD_LDS_LIMIT
    shapes = [[6, 9], [4, 5], [3, 3], [2, 2]][:L]
    inputs = mr.dyadic_inputs(2, shapes, 3, 32, 77, P, seed=43)
    value, shapes_t, start, loc, attn, _ = inputs
    ref = mr.closed_form(value.double(), shapes, loc, attn)
    _check_forward(f"L*P = {L * P}", _forward(inputs), ref)


def test_forward_pointer_form_above_2gib():
    """msda_fwd_d32_kernel<false>: taken when the whole value tensor has >= 0x7fffff00 bytes (a buffer descriptor cannot span it).
    B = 2 entries of one 2900 x 2900 level: the B = 2 call is the pointer form, a B = 1 call on either entry the buffer form."""
    from occnet_amd import ext
    B, H, W, M, D, Lq, P = 2, 2900, 2900, 1, 32, 257, 4
    S = H * W
    assert B * S * M * D * 4 == 2152960000 >= OOB_OFFSET > S * M * D * 4 and S * M * D < 2 ** 31
    assert _fwd_lds_bytes(1, P) <= FWD_LDS_LIMIT
    _, shapes_t, start, loc, attn, _ = mr.dyadic_inputs(B, [[H, W]], M, D, Lq, P, seed=44, value=False)
    # the first and the last row and column of both entries, clipped corners included: pixel 0 and pixel S - 1
    for q, (x, y) in enumerate(((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0))):
        loc[:, q, ..., 0], loc[:, q, ..., 1] = x, y
    mr.check_exact(loc, [[H, W]])
    gen = torch.Generator(device="cuda").manual_seed(45)
    value = torch.randn(B, S, M, D, device="cuda", generator=gen)
    try:
        dev = [t.cuda() for t in (shapes_t, start, loc, attn)]
        both = ext.ms_deform_attn_forward(value, *dev, im2col_step=64)
        torch.cuda.synchronize()
        for b in range(B):
            one = ext.ms_deform_attn_forward(value[b:b + 1], dev[0], dev[1], dev[2][b:b + 1].contiguous(),
                                             dev[3][b:b + 1].contiguous(), im2col_step=64)
            d = float((both[b:b + 1] - one).abs().max())
            print(f"entry {b}: pointer form vs buffer form: max diff {d:.3e}, bit-equal: {torch.equal(both[b:b + 1], one)}")
            assert d < FWD_BOUND
        ref = mr.closed_form(value[1:2], [[H, W]], dev[2][1:2], dev[3][1:2])       # float64 on the device, gathered rows only
        used = ref['adm'][0, :4]
        assert used.all()
        _check_forward("entry 1, buffer form", one, ref)
        _check_forward("entry 1, pointer form", both[1:2], ref)
    finally:
        del value
        torch.cuda.empty_cache()


def _bins(B, shapes, M):
    S = sum(h * w for h, w in shapes)
    return S, B * M * (S // BIN_PIX + len(shapes) + 1)                  # bwd_ws_layout: bins_per_bm = S / 32 + L + 1


@functools.lru_cache(maxsize=None)
def _dispatch_case(B, shapes, M, Lq, P, seed):
    shapes = [list(s) for s in shapes]
    inputs = mr.dyadic_inputs(B, shapes, M, 32, Lq, P, seed=seed)
    value, shapes_t, start, loc, attn, grad_out = inputs
    return inputs, mr.closed_form(value, shapes, loc, attn, grad_out)


@pytest.mark.parametrize("path", ["block", "deterministic"])
def test_backward_wave_binning_by_rule(path, monkeypatch):
    """No switch: the block-aggregated binning needs (S / 32 + 2) * 2 ints of LDS; above 48 KiB the call falls to the
    wave-aggregated kernels by itself.  One 444 x 444 level: 6 162 bins, 7 blocks in the scan."""
    B, shapes, M, Lq, P = 1, ((444, 444),), 1, 300, 4
    S, n_bins = _bins(B, shapes, M)
    assert (S // BIN_PIX + 2) * 2 * 4 > BIN_LDS_LIMIT and S == 197136
    assert n_bins == 6162 and (n_bins + SCAN_BLOCK - 1) // SCAN_BLOCK == 7
    inputs, ref = _dispatch_case(B, shapes, M, Lq, P, 46)
    _set_path(monkeypatch, path)
    _check_grads(f"444 x 444, wave binning by rule ({path} replay)", _backward(inputs), ref)


@pytest.mark.parametrize("path", ["block", "deterministic"])
def test_backward_multi_block_scan_on_the_default_path(path, monkeypatch):
    """More than 1 024 bins: the scan runs as several blocks plus the block of their totals."""
    B, shapes, M, Lq, P = 2, ((48, 48),), 8, 200, 4
    S, n_bins = _bins(B, shapes, M)
    assert n_bins == 1184 > SCAN_BLOCK and (S // BIN_PIX + 2) * 2 * 4 <= BIN_LDS_LIMIT
    inputs, ref = _dispatch_case(B, shapes, M, Lq, P, 47)
    _set_path(monkeypatch, path)
    _check_grads(f"1184 bins ({path})", _backward(inputs), ref)


def test_backward_mmcv_argument_list_allocates_its_own_scratch(monkeypatch):
    """occ_ms_deform_attn_backward_f32 - mmcv's exact argument list, no workspace: the library takes the scratch of the binned
    path from hipMallocAsync and frees it behind the replay.  A second call right after returns the same grad_loc / grad_attn
    bits: the freed scratch (flags, counts) left nothing behind."""
    from occnet_amd import _lib
    from occnet_amd.ext import i32, ptr, stream_ptr          # the operator module's own pointer helpers
    from tests.test_gpu_backward import _case_of
    _set_path(monkeypatch, "block")
    (value, shapes_t, start, loc, attn, grad_out), _ = _case_of("sca_like")
    ref = mr.closed_form(value.double(), shapes_t.tolist(), loc, attn, grad_out)
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    assert int(_lib.lib().occ_ms_deform_attn_backward_workspace_bytes(i32(B), i32(S), i32(M), i32(D), i32(L), i32(Lq), i32(P))) > 0
    dev = [t.cuda() for t in (value, shapes_t, start, loc, attn, grad_out)]

    def run():
        gv, gl, ga = (torch.zeros_like(t) for t in (dev[0], dev[3], dev[4]))
        with torch.cuda.device(dev[0].device):
            rc = _lib.lib().occ_ms_deform_attn_backward_f32(
                *[ptr(t) for t in dev], ptr(gv), ptr(gl), ptr(ga), i32(B), i32(S), i32(M), i32(D), i32(L), i32(Lq), i32(P),
                i32(64), stream_ptr(dev[0].device))
        _lib.check(rc, "ms_deform_attn_backward (no workspace)")
        return gv, gl, ga
    first, second = run(), run()
    torch.cuda.synchronize()
    _check_grads("sca_like, library-owned scratch, call 1", first, ref)
    _check_grads("sca_like, library-owned scratch, call 2", second, ref)
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])


# ---- generic head dims, accumulation, the fp16 node ----------------------------------------------------------------------------
GENERIC_SHAPES = [[5, 7], [3, 4]]


@pytest.mark.parametrize("D", [1, 8, 48, 64, 200, 256])
def test_generic_head_dims(D, monkeypatch):
    """The generic backward's block is (256 / D) items x D threads: 240 threads at D = 48, one item per block and a thread count
    that is no multiple of 64 at D = 200."""
    inputs = mr.dyadic_inputs(2, GENERIC_SHAPES, 2, D, 13, 3, seed=48)
    value, shapes_t, start, loc, attn, grad_out = inputs
    ref = mr.closed_form(value.double(), GENERIC_SHAPES, loc, attn, grad_out)
    _set_path(monkeypatch, "block")
    _check_forward(f"generic D={D}", _forward(inputs), ref)
    _check_grads(f"generic D={D}", _backward(inputs), ref)


def test_backward_refuses_257_channels_before_any_launch(monkeypatch):
    from occnet_amd._lib import OccAmdError
    inputs = mr.dyadic_inputs(1, GENERIC_SHAPES, 2, 257, 13, 3, seed=49)
    _set_path(monkeypatch, "block")
    marks = tuple(torch.full_like(t, 3.0) for t in (inputs[0], inputs[3], inputs[4]))
    with pytest.raises(OccAmdError, match="above 256"):
        _backward(inputs, prefill=marks)


@functools.lru_cache(maxsize=None)
def _dense_ref(D):
    value, shapes_t, start, loc, attn, grad_out = _sparse_inputs(D)
    assert bool((grad_out.view(SPARSE_B, SPARSE_LQ, SPARSE_M, D) != 0).any(-1).all())
    return mr.closed_form(value.double(), SPARSE_SHAPES, loc, attn, grad_out)


@pytest.mark.parametrize("path", list(PATHS) + ["generic_d16"])
def test_grad_value_is_accumulated_the_other_two_are_written(path, monkeypatch):
    """The contract in msda_backward.hip's header: grad_value += , grad_loc / grad_attn = (every sample has one writer; no item
    is skipped here, the output gradient has no zero row)."""
    D = 16 if path == "generic_d16" else 32
    inputs, ref = _sparse_inputs(D), _dense_ref(D)
    g = torch.Generator().manual_seed(50)
    G0 = torch.randn(inputs[0].shape, generator=g)
    marks = (G0, torch.full_like(inputs[3], 7.0), torch.full_like(inputs[4], -7.0))
    _set_path(monkeypatch, "block" if D == 16 else path)
    gv, gl, ga = _backward(inputs, prefill=marks)
    scale = max(1.0, float((G0.double() + ref['grad_value']).abs().max()))
    d = float(((gv.cpu().double() - G0.double()) - ref['grad_value']).abs().max()) / scale
    print(f"accumulation ({path}): (grad_value - G0) vs closed form = {d:.3e} (scale {scale:.2f})")
    assert torch.isfinite(gv).all() and d < GRAD_BOUND
    _check_grads(f"accumulation ({path}), written over the marks", (gv, gl, ga), ref, skip=("grad_value",))


def test_fp16_node_is_the_fp32_node_behind_a_cast(monkeypatch):
    """MultiScaleDeformableAttnFunction_fp16 on half inputs: output and gradients are .half() of what the fp32 node gives on the
    same half-rounded inputs, bit for bit - the same kernels behind a cast.  (grad_value in the default mode follows the slot
    order of integer atomics in its last bits; the fixed-point replay makes both runs the same sum.)"""
    from occnet_amd.plugin import functions as fn
    _set_path(monkeypatch, "deterministic")
    shapes = [[10, 14], [5, 7]]
    value, shapes_t, start, loc, attn, grad_out = mr.dyadic_inputs(2, shapes, 4, 32, 64, 4, seed=51)
    half = [t.cuda().half() for t in (value, loc, attn)]
    w = grad_out.cuda().half()
    st = (shapes_t.cuda(), start.cuda())

    def run(node, cast, w_):
        v, l, a = (cast(t).detach().requires_grad_(True) for t in half)
        out = node.apply(v, st[0], st[1], l, a, 64)
        out.backward(w_)
        return out.detach(), v.grad, l.grad, a.grad
    got = run(fn.MultiScaleDeformableAttnFunction_fp16, lambda t: t.clone(), w)
    want = run(fn.MultiScaleDeformableAttnFunction_fp32, lambda t: t.float(), w.float())
    for nm, g, r in zip(("output", "grad_value", "grad_loc", "grad_attn"), got, want):
        assert g.dtype == torch.float16 and r.dtype == torch.float32
        differ = int((g != r.half()).sum())
        print(f"fp16 node {nm}: elements that differ from .half() of the fp32 node: {differ} of {g.numel()}")
        assert torch.equal(g, r.half()), nm
    assert float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0
