"""Guard bands: run a kernel with every tensor it can see placed inside a poisoned arena, then look at the poison.

A value test cannot see a kernel that leaves its tensors where the neighbouring memory is harmless: a clamp that is off by one
loads from the next allocation, a 0/1 mask multiplies what it loaded by zero, and every value is right -- until the neighbour holds
a NaN.  A store one row past the end lands in the allocator's slack.  Here every input (`framed`) and every allocation a wrapper
makes (`guarded_allocations`: outputs, workspaces, packed weights) is the interior of a one-dimensional arena

    [ band: poison | interior, 256-byte aligned | band: poison ]

whose bands are at least BAND_MIN bytes and at least as large as the tensor.  Floating-point bands are NaN, so a value read out of
one reaches the result as NaN even through a multiplication by zero; integer bands are the byte POISON_BYTE, or a value the case
names (an index out of range).  `check()` compares every band with a copy taken when it was written, as raw bytes.

A GPU test file that uses this ends every test with release() (and puts back the package's weight caches, which pin the
framed weights they were built from), so that it leaves the process, and the allocator's pool, as it found them.

What this cannot see: an overreach larger than a band, and a read whose value is discarded (a clamped in-tensor address, a
`select` that drops the lane).  Neither moves a band nor poisons a result.  Nor is an operand framed that a wrapper derives
with another torch op than the six patched here (`.float().permute().reshape()`, `torch.cat`, `b3 + bds` in
ext.bottleneck64_pack; F.pad in the conv3d training node; `.contiguous()` of a strided input): it lies in plain pool memory, so
what the kernel reads of it has no bands.  A test that needs those bands builds the operand itself and calls the launcher.

`COVERED` / `EXEMPT` at the end of this file list every function of the C ABI; tests/test_guard_bands_host.py keeps them complete.
"""
import contextlib
import sys

import torch

BAND_MIN = 64 * 1024
ALIGN = 256
POISON_BYTE = 0xA5


class GuardBandError(AssertionError):
    """A band changed, a claimed entry point was not launched, or a framed result differs from the plain one."""


class Arena:
    """One framed tensor: the arena's bytes, where the interior lies in them, and a copy of both bands as written."""

    def __init__(self, label, raw, lo, span_bytes, band, itemsize):
        self.label, self.raw, self.lo, self.span_bytes, self.band, self.itemsize = label, raw, lo, span_bytes, band, itemsize
        self.before = raw[lo - band:lo].clone()
        self.after = raw[lo + span_bytes:lo + span_bytes + band].clone()

    def touched(self):
        """[(side, first byte offset, first element offset)]: 'before' counts back from the tensor's first byte (1 = the byte
        just in front of it), 'after' counts from the first byte behind its last element (0 = that byte)."""
        out = []
        now_before = self.raw[self.lo - self.band:self.lo]
        now_after = self.raw[self.lo + self.span_bytes:self.lo + self.span_bytes + self.band]
        if not torch.equal(now_before, self.before):
            bad = (now_before != self.before).nonzero()
            off = self.band - int(bad[-1])                  # the touched byte nearest to the tensor
            out.append(("before", off, (off + self.itemsize - 1) // self.itemsize))
        if not torch.equal(now_after, self.after):
            off = int((now_after != self.after).nonzero()[0])
            out.append(("after", off, off // self.itemsize))
        return out


_ARENAS = []
_LIVE = []          # the allocation behind every arena since the last release()


def reset():
    """Forget every arena made so far (check() then looks at later ones only)."""
    del _ARENAS[:]


def release():
    """Overwrite every arena made since the last release() with zeros and let go of it: the memory that returns to the
    allocator's pool holds no poison for a later test's torch.empty to find.  The tensors handed out are zeros afterwards."""
    for alloc in _LIVE:
        alloc.zero_()
    del _LIVE[:]
    del _ARENAS[:]


def arenas():
    return list(_ARENAS)


def _span(shape, strides):
    """Elements from the first to the last addressed one, inclusive (0 for an empty tensor)."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((n - 1) * st for n, st in zip(shape, strides))


def _fill(flat, poison):
    """Fill a flat typed view with the poison of its dtype: NaN for floats, `poison` (a value) or POISON_BYTE bytes otherwise."""
    if flat.numel() == 0:
        return
    if poison is not None:
        flat.fill_(poison)
    elif flat.dtype.is_floating_point:
        flat.fill_(float("nan"))
    else:
        flat.view(torch.uint8).fill_(POISON_BYTE)


def _arena(shape, strides, dtype, device, poison, label, interior_fill):
    """A tensor of the given geometry inside a fresh arena.  interior_fill: 'poison' (as the bands) or 'zero'."""
    itemsize = _REAL["empty"]((), dtype=dtype).element_size()
    span = _span(shape, strides)
    span_bytes = span * itemsize
    band = max(BAND_MIN, -(-span_bytes // ALIGN) * ALIGN)
    total = band + span_bytes + band
    total = -(-total // 8) * 8
    alloc = _REAL["empty"](total + ALIGN, dtype=torch.uint8, device=device)
    shift = (-alloc.data_ptr()) % ALIGN
    raw = alloc[shift:shift + total]                        # 256-byte aligned; every offset below is a multiple of itemsize
    flat = raw[:(total // itemsize) * itemsize].view(dtype)
    lo = band
    _fill(flat[:lo // itemsize], poison)
    _fill(flat[lo // itemsize + span:], poison)
    inner = flat[lo // itemsize:lo // itemsize + span]
    if interior_fill == "zero":
        inner.view(torch.uint8).zero_()
    else:
        _fill(inner, poison)
    t = flat.as_strided(tuple(shape), tuple(strides), flat.storage_offset() + lo // itemsize)
    assert t.numel() == 0 or t.data_ptr() % ALIGN == 0
    _ARENAS.append(Arena(label, raw, lo, span_bytes, band, itemsize))
    _LIVE.append(alloc)
    return t


def framed(t, poison=None, label=None):
    """`t` again -- values, shape, dtype, strides (so memory format), requires_grad -- as the interior of a poisoned arena.
    poison: None = NaN for floating types and POISON_BYTE bytes for the others; a number = that value in t's dtype (an index out
    of range for the case)."""
    src = t.detach()
    out = _arena(src.shape, src.stride(), src.dtype, src.device, poison,
                 label or f"input {tuple(src.shape)} {src.dtype}", "poison")
    out.copy_(src)
    if t.requires_grad:
        out.requires_grad_(True)
    return out


class Poisoned:
    """An input of run_guarded with a poison of its own: Poisoned(index, 1 << 40)."""

    def __init__(self, tensor, poison):
        self.tensor, self.poison = tensor, poison


def _map_inputs(x, on_tensor, path="in"):
    if isinstance(x, Poisoned):
        return on_tensor(x.tensor, x.poison, path)
    if isinstance(x, torch.Tensor):
        return on_tensor(x, None, path)
    if isinstance(x, (list, tuple)):
        return type(x)(_map_inputs(v, on_tensor, f"{path}[{i}]") for i, v in enumerate(x))
    if isinstance(x, dict):
        return {k: _map_inputs(v, on_tensor, f"{path}[{k!r}]") for k, v in x.items()}
    return x


# ---- every allocation framed ------------------------------------------------------------------------------------------------

_REAL = {"empty": torch.empty, "empty_like": torch.empty_like, "zeros": torch.zeros, "zeros_like": torch.zeros_like,
         "new_empty": torch.Tensor.new_empty, "new_zeros": torch.Tensor.new_zeros}


class LaunchRecord(list):
    """Names of the C-ABI functions called while guarded_allocations() was active, in order."""

    def require(self, *names):
        missing = [n for n in names if n not in self]
        if missing:
            raise GuardBandError(f"not launched: {missing}; launched: {sorted(set(self))}")


def _caller():
    f = sys._getframe(2)
    return f"{f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno}"


class _RecordingLib:
    """The ctypes library with every function call written into the record."""

    def __init__(self, real, record):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_record", record)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn) or not name.startswith("occ_"):
            return fn
        record = self._record

        def call(*args):
            record.append(name)
            return fn(*args)
        call.__name__ = name
        call._guard_band_recorded = True
        return call


@contextlib.contextmanager
def guarded_allocations(device_type="cuda"):
    """While active: every torch.empty / empty_like / zeros / zeros_like / Tensor.new_empty / new_zeros on a `device_type` device
    returns the interior of an arena (same shape, dtype, strides -- so memory_format= -- and requires_grad as the real call's
    result), and every C-ABI call through occnet_amd.ext._launch or occnet_amd._lib.lib() is written into the LaunchRecord this
    yields.  `empty` interiors hold the poison, `zeros` interiors zeros."""
    record = LaunchRecord()

    def wrap(name, interior_fill):
        real = _REAL[name]

        def alloc(*args, **kw):
            if kw.get("out") is not None:
                return real(*args, **kw)
            proto = real(*args, **kw)            # the real call decides shape, dtype, device and strides
            if proto.device.type != device_type or proto.layout != torch.strided or proto.is_quantized:
                return proto
            out = _arena(proto.shape, proto.stride(), proto.dtype, proto.device, None,
                         f"{name} {tuple(proto.shape)} {proto.dtype} at {_caller()}", interior_fill)
            return out.requires_grad_(True) if proto.requires_grad else out
        alloc.__name__ = name
        return alloc

    patches = [(torch, "empty", wrap("empty", "poison")), (torch, "empty_like", wrap("empty_like", "poison")),
               (torch, "zeros", wrap("zeros", "zero")), (torch, "zeros_like", wrap("zeros_like", "zero")),
               (torch.Tensor, "new_empty", wrap("new_empty", "poison")), (torch.Tensor, "new_zeros", wrap("new_zeros", "zero"))]
    undo = []
    try:
        ext = _lib = None
        try:
            from occnet_amd import _lib, ext
        except Exception:                       # the helper's own host tests run without the package's library
            pass
        if _lib is not None:
            real_lib, real_launch = _lib.lib, ext._launch

            def lib():
                return _RecordingLib(real_lib(), record)

            def launch(fn, dev, what, *args, **kw):
                if not getattr(fn, "_guard_band_recorded", False):      # a function taken from the library before we got here
                    record.append(fn.__name__)
                return real_launch(fn, dev, what, *args, **kw)
            patches += [(_lib, "lib", lib), (ext, "_launch", launch)]
        for obj, name, new in patches:
            had = name in vars(obj)
            undo.append((obj, name, had, vars(obj).get(name)))
            setattr(obj, name, new)
        yield record
    finally:
        for obj, name, had, old in reversed(undo):
            if had:
                setattr(obj, name, old)
            else:
                delattr(obj, name)


def check():
    """Every band of every arena since reset() must hold what was written into it.  Returns the number of arenas checked."""
    bad = []
    for a in _ARENAS:
        for side, off, el in a.touched():
            where = (f"{off} byte(s) = element -{el} in front of its first element" if side == "before"
                     else f"byte +{off} = element +{el} behind its last element")
            bad.append(f"{a.label}: band {side} the tensor changed, nearest at {where}")
    if bad:
        raise GuardBandError("guard band touched:\n  " + "\n  ".join(bad))
    return len(_ARENAS)


class Guarded:
    """What run_guarded returns: the plain result, the framed one, the launch record, and how many arenas were checked."""

    def __init__(self, plain, framed_result, record, n_arenas):
        self.plain, self.framed, self.record, self.n_arenas = plain, framed_result, record, n_arenas


def run_framed(fn, inputs, device_type="cuda"):
    """fn(*framed inputs) under guarded_allocations(), synchronised, bands checked: (result, launch record, arenas checked)."""
    reset()
    fr = _map_inputs(list(inputs), lambda t, p, path: framed(t, p, f"{path} {tuple(t.shape)} {t.dtype}"))
    with guarded_allocations(device_type) as record:
        out = fn(*fr)
        if device_type == "cuda":
            torch.cuda.synchronize()
    return out, record, check()


def run_guarded(fn, inputs, device_type="cuda"):
    """fn(*inputs) plainly, then run_framed(fn, inputs).  `inputs` is a sequence whose tensors -- also inside lists, tuples and
    dicts, also wrapped in Poisoned -- are framed; anything else is passed as it is.  fn must not modify its inputs (clone
    inside fn for an in-place kernel)."""
    plain = fn(*_map_inputs(list(inputs), lambda t, p, path: t))
    if device_type == "cuda":
        torch.cuda.synchronize()
    out, record, n = run_framed(fn, inputs, device_type)
    return Guarded(plain, out, record, n)


# ---- comparing the two runs --------------------------------------------------------------------------------------------------

def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32,
                                                                      8: torch.int64}[t.element_size()])


def _pairs(plain, got, path="out"):
    if isinstance(plain, torch.Tensor):
        if not isinstance(got, torch.Tensor):
            raise GuardBandError(f"{path}: plain run gave a tensor, framed run {type(got).__name__}")
        yield path, plain, got
    elif isinstance(plain, (list, tuple)):
        if not isinstance(got, (list, tuple)) or len(got) != len(plain):
            raise GuardBandError(f"{path}: structure differs")
        for i, (p, g) in enumerate(zip(plain, got)):
            yield from _pairs(p, g, f"{path}[{i}]")
    elif isinstance(plain, dict):
        if not isinstance(got, dict) or set(got) != set(plain):
            raise GuardBandError(f"{path}: keys differ")
        for k in plain:
            yield from _pairs(plain[k], got[k], f"{path}[{k!r}]")
    elif plain != got:
        raise GuardBandError(f"{path}: {plain!r} != {got!r}")


def assert_bit_equal(plain, got, defined=None):
    """The framed result equals the plain one bit for bit (raw bytes: NaN == NaN, -0 != +0), and therefore has no non-finite
    element the plain one lacks.  defined: {path: bool mask or index} for outputs only partly defined by contract."""
    n = 0
    for path, p, g in _pairs(plain, got):
        if p.shape != g.shape or p.dtype != g.dtype:
            raise GuardBandError(f"{path}: {tuple(p.shape)} {p.dtype} vs {tuple(g.shape)} {g.dtype}")
        if defined is not None and path in defined:
            p, g = p[defined[path]], g[defined[path]]
        if p.numel() and not torch.equal(_bits(p), _bits(g)):
            bad = (_bits(p) != _bits(g)).reshape(-1).nonzero()
            i = int(bad[0])
            raise GuardBandError(f"{path}: framed run differs from the plain run in {bad.numel()} of {p.numel()} elements, first "
                                 f"at flat index {i}: plain {p.contiguous().reshape(-1)[i].item()!r}, framed "
                                 f"{g.contiguous().reshape(-1)[i].item()!r}")
        n += 1
    if n == 0:
        raise GuardBandError("nothing was compared")


def assert_no_new_nonfinite(plain, got):
    """For the families without promised last bits: no Inf / NaN in the framed result where the plain one is finite."""
    for path, p, g in _pairs(plain, got):
        if p.dtype.is_floating_point:
            new = torch.isfinite(p) & ~torch.isfinite(g)
            if bool(new.any()):
                raise GuardBandError(f"{path}: {int(new.sum())} non-finite element(s) only in the framed run, first at flat index "
                                     f"{int(new.reshape(-1).nonzero()[0])}")


# ---- the C ABI, function by function ------------------------------------------------------------------------------------------
# Every `int occ_*(` of include/occnet_amd.h, occnet_amd_dvr.h, occnet_amd_visibility.h and occnet_amd_input.h is in exactly one
# table.  COVERED names the test that frames its inputs and outputs; EXEMPT is for functions that launch nothing.

_G = "tests/test_gpu_guard_bands.py::"

COVERED = {
    # backbone
    "occ_conv1x1_nhwc_bf16_variant": _G + "test_conv1x1_resident_variants",
    "occ_conv1x1_nhwc_bf16": _G + "test_conv1x1_plain_entry_point_and_dgrad",
    "occ_mfma_pack_b_frag_bf16": _G + "test_conv1x1_resident_variants",
    "occ_conv3x3_nhwc_bf16_variant": _G + "test_conv3x3_every_tile",
    "occ_conv3x3_pack_weight_bf16": _G + "test_conv3x3_every_tile",
    "occ_conv3x3_nhwc_bf16": _G + "test_conv3x3_plain_entry_points_and_dgrad",
    "occ_conv3x3_nhwc_bf16_amax": _G + "test_conv3x3_plain_entry_points_and_dgrad",
    "occ_conv3x3_conv1x1_nhwc_bf16": _G + "test_conv3x3_conv1x1_every_tile",
    "occ_bottleneck64_nhwc_bf16_variant": _G + "test_bottleneck64_every_variant",
    "occ_bottleneck64_nhwc_bf16": _G + "test_bottleneck64_every_variant",
    "occ_bottleneck64_next_nhwc_bf16": _G + "test_bottleneck64_next",
    "occ_stem_conv7x7_pool_f32_bf16": _G + "test_stem_f32",
    "occ_stem_conv7x7_pool_u8_bf16": _G + "test_stem_u8",
    "occ_bias_relu_maxpool_nhwc_bf16": _G + "test_bias_relu_maxpool_and_bias_act",
    "occ_bias_act_nhwc_bf16": _G + "test_bias_relu_maxpool_and_bias_act",
    "occ_bias_act_bwd_nhwc_bf16": _G + "test_bias_act_bwd",
    # decoder
    "occ_conv3d_bn_relu_f32": _G + "test_conv3d_bn_relu",
    "occ_conv3d_bn_relu_bf16x3_f32": _G + "test_conv3d_bn_relu",
    "occ_conv3d_pack_weight_f32": _G + "test_conv3d_bn_relu",
    "occ_conv3d_pack_weight_bf16x3": _G + "test_conv3d_bn_relu",
    "occ_occ_heads_decode_f32": _G + "test_occ_heads",
    "occ_occ_heads_f32": _G + "test_occ_heads",
    "occ_conv3d_heads_decode_bf16x3_f32": _G + "test_conv3d_heads_decode",
    "occ_conv3d_heads_pack": _G + "test_conv3d_heads_decode",
    "occ_conv3d_wgrad_bf16x3_f32": _G + "test_conv3d_autograd",
    "occ_bn3d_relu_train_stats_f32": _G + "test_bn3d_relu_train",
    "occ_bn3d_relu_train_fwd_f32": _G + "test_bn3d_relu_train",
    "occ_bn3d_relu_train_bwd_f32": _G + "test_bn3d_relu_train",
    # GEMMs
    "occ_linear_f32": _G + "test_linear",
    "occ_linear_bf16x3_f32": _G + "test_linear",
    "occ_linear_pack_weight_bf16x3": _G + "test_value_proj_bf16",
    "occ_linear_bf16x3_q16rows": _G + "test_linear_q16rows_and_rows_encode",
    "occ_sca_rows_encode_q16": _G + "test_linear_q16rows_and_rows_encode",
    "occ_value_proj_bf16_f32": _G + "test_value_proj_bf16",
    "occ_value_proj_bf16_f16pairs": _G + "test_value_proj_resident_q16",
    "occ_value_proj_bf16_q16pairs": _G + "test_value_proj_resident_q16",
    "occ_value_proj_bf16_planes": _G + "test_value_proj_bf16_planes",
    "occ_value_range_scale_bf16": _G + "test_value_range_scale_pair",
    "occ_value_range_scale_from_amax": _G + "test_value_range_scale_pair",
    "occ_linear_wgrad_bf16x3_f32": _G + "test_linear_wgrad",
    "occ_conv1x1_wgrad_nhwc_bf16": _G + "test_conv_wgrad",
    "occ_conv3x3_wgrad_nhwc_bf16": _G + "test_conv_wgrad",
    "occ_linear_chain_pack_bf16x3": _G + "test_linear_chains",
    "occ_linear_pair_chain_bf16x3_f32": _G + "test_linear_chains",
    "occ_linear_ln_chain_bf16x3_f32": _G + "test_linear_chains",
    "occ_encoder_ffn_chain_bf16x3_f32": _G + "test_linear_chains",
    # gathers
    "occ_ms_deform_attn_forward_f32": _G + "test_ms_deform_attn_forward",
    "occ_ms_deform_attn_backward_ws_f32": _G + "test_ms_deform_attn_backward_workspace_path",
    "occ_ms_deform_attn_backward_f32": _G + "test_ms_deform_attn_backward_plain_entry_point",
    "occ_sca_fused_forward_f32": _G + "test_sca_fused_forward",
    "occ_sca_fused_forward_f16v": _G + "test_sca_fused_forward",
    "occ_sca_fused_forward_q16v": _G + "test_sca_fused_forward",
    "occ_sca_fused_backward_f32": _G + "test_sca_fused_backward",
    "occ_tsa_fused_forward_f32": _G + "test_tsa_fused_forward",
    "occ_tsa_fused_forward_q16v": _G + "test_tsa_fused_forward",
    "occ_tsa_fused_backward_f32": _G + "test_tsa_fused_backward",
    # training glue
    "occ_point_sampling_f32": _G + "test_point_sampling_boundaries",
    "occ_sca_prep_forward_f32": _G + "test_sca_prep",
    "occ_sca_prep_backward_f32": _G + "test_sca_prep",
    "occ_rows_gather_sum_f32": _G + "test_rows_gather_sum",
    "occ_dropout_add_ln_fwd_f32": _G + "test_dropout_add_layernorm",
    "occ_dropout_add_ln_bwd_f32": _G + "test_dropout_add_layernorm",
    "occ_conv_bn_fold_fwd_f32": _G + "test_conv_bn_fold",
    "occ_conv_bn_fold_bwd_f32": _G + "test_conv_bn_fold",
    "occ_selftest_fdiv_f32": _G + "test_selftest_fdiv",
    # loss and input
    "occ_heads_loss_fwd_f32": _G + "test_heads_loss",
    "occ_heads_loss_bwd_f32": _G + "test_heads_loss",
    "occ_dvr_render_forward_f32": _G + "test_dvr_render_forward",
    "occ_dvr_render_f32": _G + "test_dvr_render",
    "occ_input_u8_scaled_f32": _G + "test_input_u8",
    "occ_train_input_u8_f32": "tests/test_gpu_train_input.py::test_memory_discipline",       # and again in test_input_u8
    # evaluation
    "occ_ray_metrics_accumulate": _G + "test_ray_metrics_accumulate_and_submission_rays",
    "occ_submission_rays": _G + "test_ray_metrics_accumulate_and_submission_rays",
    "occ_submission_score_accumulate": _G + "test_submission_score_accumulate",
    "occ_confusion_accumulate": _G + "test_confusion_accumulate",
    "occ_visibility_views": _G + "test_visibility_views",
    "occ_render_views": _G + "test_render_views_and_bev",
    "occ_render_bev": _G + "test_render_views_and_bev",
}

EXEMPT = {
    "occ_abi_version": "returns a constant",
    "occ_conv3d_channel_block": "host query of the shape, no stream",
    "occ_linear_chain_tile_split": "pure host function (its header says so), no stream",
    "occ_conv3x3_conv1x1_pick": "host query of the shape, no stream",
    "occ_bottleneck64_tile_of_block": "pure host function, no stream",
    "occ_bottleneck64_next_pick": "host query of the shape, no stream",
}
