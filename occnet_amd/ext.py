"""The operator module: mirror of the reference's `mmcv._ext` surface for this path.

`ms_deform_attn_forward` / `ms_deform_attn_backward` keep mmcv's exact Python signatures
(reference call sites: projects/mmdet3d_plugin/bevformer/modules/
multi_scale_deformable_attn_function.py:42-48, 74-84, 118-124, 150-160): tensors are torch-owned and
device resident, `im2col_step` is passed as a keyword, the op runs on the current stream without
synchronising, failures raise Python exceptions.  Underneath, each call hands raw device pointers to
the C ABI (include/occnet_amd.h) of libocc_amd.so.

The remaining functions expose the fused MI355X kernels (no counterpart in mmcv._ext).
"""
import ctypes
import os

import torch

from . import _lib
from .derived import DerivedCache
from .io import check_scale, scaled_size
from ._lib import OccAmdError, OccAmdUnsupported, f32, i32
from ._lib import i64, ptr, stream_ptr  # noqa: F401  (not used here any more; callers import them from this module)


_TIMING = None   # None, or {kernel name: [(start_event, end_event), ...]} (bench.py roofline leg)
_TIMING_ONLY = None   # None = every instrumented launch, or the set of kernel names still timed


def kernel_timing(enable=True):
    """Turn HIP-event timing of the instrumented launches on/off.  Events are recorded on the
    stream the kernel is launched on (torch's current stream).  Returns the record dict."""
    global _TIMING, _TIMING_ONLY
    _TIMING = {} if enable else None
    _TIMING_ONLY = None
    return _TIMING


def kernel_timing_only(names):
    """Restrict the timing to the given kernel names (None = all again): two event records per launch cost
    ~4 us of queue time each, 0.3 ms per step when every Linear is timed."""
    global _TIMING_ONLY
    _TIMING_ONLY = None if names is None else set(names)


def _timing_on(name):
    """True when launches booked under `name` are being timed (None: a launch that is not instrumented)."""
    return name is not None and _TIMING is not None and (_TIMING_ONLY is None or name in _TIMING_ONLY)


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = _timing_on(self.name)
        if self.on:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def __exit__(self, *exc):
        if self.on:
            self.ev[1].record()
            _TIMING.setdefault(self.name, []).append(self.ev)
        return False


def _note_flops(name, flops):
    """bench.py's backbone roofline: the FLOPs of an instrumented launch, next to its event pair."""
    if _timing_on(name):
        _TIMING.setdefault(name + '_flops', []).append(float(flops))


def _launch(fn, dev, what, *args, timing=None, flops=None):
    """The one way into a kernel launcher of the C ABI: fn(*args, stream) on `dev` and its current stream, timed under the
    kernel_timing name `timing` (None: not instrumented) with `flops` booked next to the event pair (whether or not the call
    succeeded), then the return code checked under the name `what`.  Tensors go in as they are (_lib.DevicePtr); a wrong
    argument count or kind raises on the host, from the argtypes the binding read out of the header."""
    with torch.cuda.device(dev), _timed(timing):
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
    if flops is not None:
        _note_flops(timing, flops)
    _lib.check(rc, what)


def kernel_times_ms(record):
    """{name: [ms per launch]} from a kernel_timing() record (call after a device synchronize); entries
    that are plain numbers (e.g. 'linear_flops') pass through."""
    return {k: [a.elapsed_time(b) for a, b in v] if v and isinstance(v[0], tuple) else list(v)
            for k, v in record.items()}


def _need_cuda_f32(name, t, contiguous=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise OccAmdError(f"{name} must be a device (HIP) tensor: the MI355X path has no CPU fallback")
    if t.dtype != torch.float32:
        raise OccAmdError(f"{name} must be float32, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise OccAmdError(f"{name} must be contiguous")


def _need_cuda_i64(name, t, device=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
        raise OccAmdError(f"{name} must be a contiguous int64 device tensor")
    if device is not None and t.device != device:
        raise OccAmdError(f"{name} must be on the device of the data ({device}), got {t.device}")


def ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index,
                           sampling_locations, attention_weights, im2col_step=64):
    """-> Tensor (B, Lq, M*D).  Same contract as mmcv._ext.ms_deform_attn_forward."""
    for n, t in (("value", value), ("sampling_locations", sampling_locations),
                 ("attention_weights", attention_weights)):
        _need_cuda_f32(n, t)
    _need_cuda_i64("value_spatial_shapes", value_spatial_shapes)
    _need_cuda_i64("value_level_start_index", value_level_start_index)
    if value.dim() != 4 or sampling_locations.dim() != 6 or attention_weights.dim() != 5:
        raise OccAmdError("ms_deform_attn_forward: expected value (B,S,M,D), sampling_locations "
                          "(B,Lq,M,L,P,2), attention_weights (B,Lq,M,L,P)")
    B, S, M, D = value.shape
    _, Lq, M2, L, P, two = sampling_locations.shape
    if (M2 != M or two != 2 or sampling_locations.shape[0] != B or
            tuple(attention_weights.shape) != (B, Lq, M, L, P) or
            tuple(value_spatial_shapes.shape) != (L, 2) or value_level_start_index.numel() != L):
        raise OccAmdError("ms_deform_attn_forward: inconsistent shapes")
    out = torch.empty((B, Lq, M * D), dtype=torch.float32, device=value.device)
    _launch(_lib.lib().occ_ms_deform_attn_forward_f32, value.device, "ms_deform_attn_forward", value, value_spatial_shapes,
            value_level_start_index, sampling_locations, attention_weights, out, B, S, M, D, L, Lq, P, int(im2col_step))
    return out


def ms_deform_attn_backward(value, value_spatial_shapes, value_level_start_index,
                            sampling_locations, attention_weights, grad_output, grad_value,
                            grad_sampling_loc, grad_attn_weight, im2col_step=64):
    """Writes into the three pre-zeroed grad tensors; returns None (mmcv contract)."""
    for n, t in (("value", value), ("sampling_locations", sampling_locations),
                 ("attention_weights", attention_weights), ("grad_output", grad_output),
                 ("grad_value", grad_value), ("grad_sampling_loc", grad_sampling_loc),
                 ("grad_attn_weight", grad_attn_weight)):
        _need_cuda_f32(n, t)
    _need_cuda_i64("value_spatial_shapes", value_spatial_shapes)
    _need_cuda_i64("value_level_start_index", value_level_start_index)
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_locations.shape
    if (grad_value.shape != value.shape or grad_sampling_loc.shape != sampling_locations.shape or
            grad_attn_weight.shape != attention_weights.shape or
            grad_output.numel() != B * Lq * M * D):
        raise OccAmdError("ms_deform_attn_backward: inconsistent shapes")
    lib = _lib.lib()
    # scratch of the atomic-free grad_value path from torch's caching allocator (not hipMallocAsync behind its back);
    # freed back to the pool when this call returns — stream-ordered, the kernels are already enqueued
    need = lib.occ_ms_deform_attn_backward_workspace_bytes(B, S, M, D, L, Lq, P)
    ws = torch.empty(need, dtype=torch.uint8, device=value.device) if need > 0 else None
    _launch(lib.occ_ms_deform_attn_backward_ws_f32, value.device, "ms_deform_attn_backward", value, value_spatial_shapes,
            value_level_start_index, sampling_locations, attention_weights, grad_output, grad_value, grad_sampling_loc,
            grad_attn_weight, B, S, M, D, L, Lq, P, int(im2col_step), ws, need)


def point_sampling(ref_3d, lidar2img, ego2lidar, pc_range, img_h, img_w):
    """ref_3d (B,Z,Nq,3), lidar2img (B,NC,4,4), ego2lidar (4,4) ->
    ref_cam (NC,B,Nq,Z,2) f32, bev_mask (NC,B,Nq,Z) bool, vis_bits (B,Nq) int32 bit field."""
    for n, t in (("ref_3d", ref_3d), ("lidar2img", lidar2img), ("ego2lidar", ego2lidar)):
        _need_cuda_f32(n, t)
    B, Z, Nq, three = ref_3d.shape
    NC = lidar2img.shape[1]
    if three != 3 or tuple(lidar2img.shape) != (B, NC, 4, 4) or tuple(ego2lidar.shape) != (4, 4):
        raise OccAmdError("point_sampling: inconsistent shapes")
    dev = ref_3d.device
    ref_cam = torch.empty((NC, B, Nq, Z, 2), dtype=torch.float32, device=dev)
    mask = torch.empty((NC, B, Nq, Z), dtype=torch.uint8, device=dev)
    vis = torch.empty((B, Nq), dtype=torch.int32, device=dev)
    pcr = (f32 * 6)(*[float(v) for v in pc_range])
    _launch(_lib.lib().occ_point_sampling_f32, dev, "point_sampling", ref_3d, lidar2img, ego2lidar, pcr, float(img_h),
            float(img_w), ref_cam, mask, vis, B, NC, Nq, Z)
    return ref_cam, mask.view(torch.bool), vis


# Storage type of the projected value maps the fused SCA gather reads (the reference keeps them in fp32:
# spatial_cross_attention.py:75,387-390).  All three keep sampling arithmetic, attention weights and accumulation in fp32.
#   'q16' (default since round 6): block floating point, 16 bits per element — one head row of a pixel = 64 bytes = 4 lanes x
#         16 bytes, so a wave load fetches 16 rows instead of 8 (csrc/sca_fused.hip); every 16-byte piece of 8 channels holds
#         int16 mantissas under one shared 4-bit exponent (csrc/common.h fma8q): the elements that dominate the gather's sums
#         are rounded to 2^-16 relative.  Against the CPU oracle: 7e-5 at the synthetic feature scale, < 6e-4 at ANY scale
#         (tests/test_gpu_value_range.py);
#   'f16' (OCC_SCA_VALUES=f16, the default of rounds 3-5): fp16 rows of the same geometry, 2^-12 relative on every element:
#         2.2e-4 at the synthetic scale, up to 1.4e-3 when the camera term dominates the residual; 2 % faster per step
#         (the q16 decode costs 17 VALU instructions per 16-byte load against 9, its encode 10 us per projection launch);
#   'f32' (OCC_SCA_VALUES=f32): the reference's storage, 8 lanes per 128-byte row (round-1/2 kernel): 3e-5, +15 % per step.
SCA_VALUES = os.environ.get("OCC_SCA_VALUES", "q16")
if SCA_VALUES not in ("f16", "f32", "q16"):
    raise OccAmdError(f"OCC_SCA_VALUES={SCA_VALUES!r}: expected f16, f32 or q16")

# Storage type of the projected BEV maps the fused TSA gather reads at INFERENCE (TemporalSelfAttention.fused_gather; the
# reference keeps them in fp32; the training node always reads fp32 rows).  Sampling arithmetic, softmax and accumulation are
# fp32 either way.
#   'f32' (default): 128-byte head rows, 8 lanes per row, 32 16-byte loads per lane (csrc/tsa_fused.hip tsa_fused_kernel);
#   'q16' (OCC_TSA_VALUES=q16, opt-in): the block-floating-point rows of the SCA gather in its pixel-pair layout — 64-byte head
#         rows, 4 lanes per row, 16 loads per lane (tsa_fused_q16_kernel).  The rows are written by the value projection
#         itself where it is a stand-alone Linear (linear_q16rows: history BEV, bs > 1) and by one sca_rows_encode_q16 pass
#         over the fp32 rows where they come out of a chain kernel (no history); their range scale comes from the LayerNorm
#         bound of the producer of the BEV rows (layernorm_bound_words) or one amax pass (tsa_value_scale).  Measured step
#         times and the storage error: DESIGN.md (TSA q16 rows), EXPERIMENTS.md.
TSA_VALUES = os.environ.get("OCC_TSA_VALUES", "f32")
if TSA_VALUES not in ("f32", "q16"):
    raise OccAmdError(f"OCC_TSA_VALUES={TSA_VALUES!r}: expected f32 or q16")


def sca_head_major():
    """The 16-bit-row SCA gather runs on the head-major kernel (one wave = 8 queries x one head, heads dealt to the XCDs;
    csrc/sca_fused.hip — the default since round 6); OCC_SCA_HEAD_MAJOR=0 selects the query-major kernel.  Read per call, like
    the library does.  (fp32 rows always take the query-major fp32 kernel.)"""
    return os.environ.get("OCC_SCA_HEAD_MAJOR", "1") != "0" and sca_rows_16bit()


def sca_rows_16bit():
    """True when the fused gather's value maps are 16-bit rows in the pixel-pair layout with a range scale (f16, q16)."""
    return SCA_VALUES in ("f16", "q16")


def sca_rows_dtype():
    return {"f16": torch.float16, "q16": torch.int16, "f32": torch.float32}[SCA_VALUES]


def sca_variant_name():
    hm = sca_head_major()
    return {"f16": "sca_fused_hm_kernel<4,8> (head-major, fp16 value rows)" if hm else "sca_fused_h_kernel<4,8> (query-major, fp16 value rows)",
            "q16": ("sca_fused_hm_kernel<4,8,Q> (head-major, q16 block-floating-point value rows)" if hm
                    else "sca_fused_h_kernel<4,8,Q> (query-major, q16 block-floating-point value rows)"),
            "f32": "sca_fused_kernel<4,8> (query-major, fp32 value rows)"}[SCA_VALUES]


def sca_value_bytes():
    return 2 if sca_rows_16bit() else 4


def sca_pair_layout(value):
    """(B*NC, S, M, D) fp16 value maps in row order -> the fused gather's pixel-PAIR order: a contiguous
    (B*NC, S_pad, M, D) tensor, S_pad = S rounded up to even, whose memory is [b][pix >> 1][head][pix & 1][D] — the two
    x-neighbours (2k, 2k+1) of one head share one 128-byte line (csrc/sca_fused.hip).  The value projection's fp16
    outputs are written in this order directly; this helper is for tests and for maps that were projected in fp32."""
    BN, S, M, D = value.shape
    if S & 1:
        value = torch.cat([value, value.new_zeros(BN, 1, M, D)], 1)
    return value.reshape(BN, -1, 2, M, D).permute(0, 1, 3, 2, 4).contiguous().view(BN, -1, M, D)


def sca_unpair_layout(value_pairs, S=None):
    """Inverse of sca_pair_layout: pixel-pair-ordered (B*NC, S_pad, M, D) [or (B*NC * S_pad, M*D) with M = cols / 32]
    -> row order, first S rows."""
    BN, S_pad, M, D = value_pairs.shape
    v = value_pairs.reshape(BN, S_pad // 2, M, 2, D).permute(0, 1, 3, 2, 4).reshape(BN, S_pad, M, D)
    return v if S is None else v[:, :S]


def sca_fused_forward(value, spatial_shapes, level_start_index, offs, logits, ref_cam, vis_bits,
                      num_heads, num_levels, num_points, order=None, stats=None, value_layout="rows", value_scale=None,
                      _timing='sca_fused_forward'):
    """Fused SCA gather.  value (B*NC, S, M, D) float32 or float16; offs (B, Nq, M*L*P*2) / logits (B, Nq, M*L*P) may
    be column slices of one wider Linear output (last dim contiguous); ref_cam (NC,B,Nq,Z,2);
    vis_bits (B,Nq) int32.  -> slots (B, Nq, M*D) float32.
    fp16 maps reach the kernel in pixel-pair order (sca_pair_layout): value_layout="pairs" says the tensor already is
    (what value_proj_bf16 / value_proj_bf16_planes write into an fp16 output); "rows" (default) converts a row-ordered
    fp16 tensor first (a copy: tests and the fp32-projection path only).
    value_scale (fp16 maps only): 1-element float32 device tensor s, a power of two — the maps hold s * value
    (value_range_scale / f16_range_scaled), the kernel divides its fp32 sums by count * s: the same result, whatever s.
    Alignment (refused before any launch): value 16 bytes; ref_cam 8 bytes; offs 8 bytes with an even row stride.  With 16-bit
    rows and L*P = 32: offs and logits 16 bytes with row strides that are multiples of 4, and ref_cam 16 bytes on the
    head-major kernel when Z % 4 == 0.  Slices of one Linear output at columns that are multiples of 4 satisfy all of it."""
    q16 = value.dtype == torch.int16
    half = value.dtype == torch.float16 or q16
    if q16 and value_layout != "pairs":
        raise OccAmdError("sca_fused_forward: q16 value maps exist in the pixel-pair layout only (sca_rows_encode_q16)")
    if value_scale is not None:
        if not half:
            raise OccAmdError("sca_fused_forward: value_scale goes with 16-bit value maps")
        if not (value_scale.is_cuda and value_scale.dtype == torch.float32 and value_scale.numel() == 1
                and value_scale.device == value.device):
            raise OccAmdError("sca_fused_forward: value_scale must be a 1-element float32 tensor on the value's device")
    if half:
        if value_layout not in ("rows", "pairs"):
            raise OccAmdError(f"sca_fused_forward: unknown value_layout {value_layout!r}")
        if not value.is_cuda:
            raise OccAmdError("sca_fused_forward: fp16 value must be a contiguous device tensor")
        if value_layout == "rows":
            value = sca_pair_layout(value)
        if not value.is_contiguous() or value.shape[1] % 2:
            raise OccAmdError("sca_fused_forward: pixel-pair fp16 value must be contiguous with an even number of rows")
    else:
        _need_cuda_f32("value", value)
    _need_cuda_f32("ref_cam", ref_cam)
    _need_cuda_f32("offs", offs, contiguous=False)
    _need_cuda_f32("logits", logits, contiguous=False)
    _need_cuda_i64("spatial_shapes", spatial_shapes)
    _need_cuda_i64("level_start_index", level_start_index)
    NC, B, Nq, Z, _ = ref_cam.shape
    BN, S, M, D = value.shape
    L, P = int(num_levels), int(num_points)
    if BN != B * NC or M != num_heads:
        raise OccAmdError("sca_fused_forward: value batch must equal B*num_cams")
    for n, t, w in (("offs", offs, M * L * P * 2), ("logits", logits, M * L * P)):
        if tuple(t.shape[:2]) != (B, Nq) or t.shape[-1] != w or t.stride(-1) != 1 \
                or t.stride(0) != Nq * t.stride(1):
            raise OccAmdError(f"sca_fused_forward: {n} must be (B,Nq,{w}) with unit inner stride")
    if vis_bits.dtype != torch.int32 or tuple(vis_bits.shape) != (B, Nq) or not vis_bits.is_contiguous():
        raise OccAmdError("sca_fused_forward: vis_bits must be contiguous int32 (B,Nq)")
    if order is not None and (order.dtype != torch.int32 or order.numel() != Nq):
        raise OccAmdError("sca_fused_forward: order must be int32 (Nq)")
    # the library refuses the same (sca_dispatch): float2 reads of offset pairs and anchors, 16-byte pieces of value rows; the
    # 16-bit-row kernels with L*P = 32 read four logits / four offset pairs (head-major: four anchors) as 16-byte loads
    if value.data_ptr() % 16:
        raise OccAmdError("sca_fused_forward: value must be 16-byte aligned")
    if ref_cam.data_ptr() % 8:
        raise OccAmdError("sca_fused_forward: ref_cam must be 8-byte aligned")
    if offs.data_ptr() % 8 or offs.stride(1) % 2:
        raise OccAmdError("sca_fused_forward: offs must be 8-byte aligned with an even row stride (float2 reads)")
    if half and L * P == 32:
        if offs.data_ptr() % 16 or logits.data_ptr() % 16 or offs.stride(1) % 4 or logits.stride(1) % 4:
            raise OccAmdError("sca_fused_forward: offs and logits must be 16-byte aligned with row strides that are multiples "
                              "of 4 for 16-bit value rows with L*P = 32")
        if Z % 4 == 0 and not os.environ.get("OCC_SCA_HEAD_MAJOR", "1").startswith("0") and ref_cam.data_ptr() % 16:
            raise OccAmdError("sca_fused_forward: ref_cam must be 16-byte aligned for the head-major kernel with L*P = 32 "
                              "and Z % 4 == 0")
    slots = torch.empty((B, Nq, M * D), dtype=torch.float32, device=value.device)
    fn = (_lib.lib().occ_sca_fused_forward_q16v if q16 else _lib.lib().occ_sca_fused_forward_f16v if half
          else _lib.lib().occ_sca_fused_forward_f32)
    _launch(fn, value.device, "sca_fused_forward", value, spatial_shapes, level_start_index, offs, offs.stride(1), logits,
            logits.stride(1), ref_cam, vis_bits, order, slots, stats, B, NC, S, M, D, L, P, Z, Nq,
            *((value_scale,) if half else ()), timing=_timing)
    return slots


def sca_fused_backward_workspace_bytes(B, NC, S, M, D, L, P, Nq):
    """Bytes of scratch sca_fused_backward takes for these shapes (0: no backward kernel for them)."""
    return _lib.lib().occ_sca_fused_backward_workspace_bytes(B, NC, S, M, D, L, P, Nq)


def sca_fused_backward(value, spatial_shapes, level_start_index, offs, logits, ref_cam, vis_bits, grad_slots,
                       num_heads, num_levels, num_points):
    """Gradient of sca_fused_forward over fp32 value rows (csrc/sca_fused_backward.hip).  Same inputs as the forward
    (value (B*NC, S, M, D) float32 row order; offs / logits may be column slices of one wider Linear output) plus
    grad_slots (B, Nq, M*D) -> (grad_value (B*NC, S, M, D), grad_offs (B, Nq, M*L*P*2), grad_logits (B, Nq, M*L*P)).
    grad_offs / grad_logits are bit-reproducible; grad_value too under OCC_MSDA_BWD_DETERMINISTIC=1.  Raises
    OccAmdUnsupported for shapes without a backward kernel."""
    _need_cuda_f32("value", value)
    _need_cuda_f32("ref_cam", ref_cam)
    _need_cuda_f32("offs", offs, contiguous=False)
    _need_cuda_f32("logits", logits, contiguous=False)
    _need_cuda_f32("grad_slots", grad_slots)
    _need_cuda_i64("spatial_shapes", spatial_shapes)
    _need_cuda_i64("level_start_index", level_start_index)
    if value.dim() != 4 or ref_cam.dim() != 5:
        raise OccAmdError("sca_fused_backward: expected value (B*NC, S, M, D) and ref_cam (NC, B, Nq, Z, 2)")
    NC, B, Nq, Z, _ = ref_cam.shape
    BN, S, M, D = value.shape
    L, P = int(num_levels), int(num_points)
    if BN != B * NC or M != num_heads:
        raise OccAmdError("sca_fused_backward: value batch must equal B*num_cams")
    for n, t, w in (("offs", offs, M * L * P * 2), ("logits", logits, M * L * P)):
        if t.dim() != 3 or tuple(t.shape[:2]) != (B, Nq) or t.shape[-1] != w or t.stride(-1) != 1 \
                or t.stride(0) != Nq * t.stride(1):
            raise OccAmdError(f"sca_fused_backward: {n} must be (B,Nq,{w}) with unit inner stride")
    if vis_bits.dtype != torch.int32 or tuple(vis_bits.shape) != (B, Nq) or not vis_bits.is_contiguous():
        raise OccAmdError("sca_fused_backward: vis_bits must be contiguous int32 (B,Nq)")
    if tuple(grad_slots.shape) != (B, Nq, M * D):
        raise OccAmdError(f"sca_fused_backward: grad_slots must be (B,Nq,{M * D})")
    need = sca_fused_backward_workspace_bytes(B, NC, S, M, D, L, P, Nq)
    if need <= 0:
        raise OccAmdUnsupported(f"sca_fused_backward: no backward kernel for M={M} D={D} L={L} P={P} "
                                f"(or shapes beyond the binned grad_value path)")
    # scratch from torch's caching allocator, freed back to the pool when this call returns (stream-ordered)
    ws = torch.empty(need, dtype=torch.uint8, device=value.device)
    grad_value = torch.zeros_like(value)
    grad_offs = torch.empty((B, Nq, M * L * P * 2), dtype=torch.float32, device=value.device)
    grad_logits = torch.empty((B, Nq, M * L * P), dtype=torch.float32, device=value.device)
    _launch(_lib.lib().occ_sca_fused_backward_f32, value.device, "sca_fused_backward", value, spatial_shapes,
            level_start_index, offs, offs.stride(1), logits, logits.stride(1), ref_cam, vis_bits, grad_slots, grad_value,
            grad_offs, grad_offs.stride(1), grad_logits, grad_logits.stride(1), B, NC, S, M, D, L, P, Z, Nq, ws, need,
            timing='sca_fused_backward')
    return grad_value, grad_offs, grad_logits


class SCAFusedFunction(torch.autograd.Function):
    """The fused SCA gather as an autograd node: forward = occ_sca_fused_forward_f32 on fp32 value rows (training always
    takes fp32 rows, whatever OCC_SCA_VALUES says), backward = occ_sca_fused_backward_f32.
    value (B*NC, S, M, D) float32; offs / logits (B, Nq, ...) — column slices of one Linear output are fine, autograd
    routes both gradients into it; ref_cam (NC, B, Nq, Z, 2) and vis_bits (B, Nq) are constants -> slots (B, Nq, M*D).
    Raises OccAmdUnsupported (before anything runs) for shapes without a backward kernel."""

    @staticmethod
    def forward(ctx, value, offs, logits, ref_cam, vis_bits, spatial_shapes, level_start_index, num_heads, num_levels,
                num_points):
        value = value.contiguous()
        NC, B, Nq = ref_cam.shape[:3]
        BN, S, M, D = value.shape
        if sca_fused_backward_workspace_bytes(B, NC, S, M, D, int(num_levels), int(num_points), Nq) <= 0:
            raise OccAmdUnsupported(f"SCAFusedFunction: no backward kernel for M={M} D={D} L={num_levels} "
                                    f"P={num_points}")
        # timed under a name of its own: 'sca_fused_forward' is the inference gather's (bench.py's roofline leg)
        slots = sca_fused_forward(value, spatial_shapes, level_start_index, offs, logits, ref_cam, vis_bits,
                                  num_heads, num_levels, num_points, _timing='sca_fused_forward_train')
        ctx.save_for_backward(value, offs, logits, ref_cam, vis_bits, spatial_shapes, level_start_index)
        ctx.dims = (int(num_heads), int(num_levels), int(num_points))
        return slots

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_slots):
        value, offs, logits, ref_cam, vis_bits, spatial_shapes, level_start_index = ctx.saved_tensors
        gv, go, gl = sca_fused_backward(value, spatial_shapes, level_start_index, offs, logits, ref_cam, vis_bits,
                                        grad_slots.contiguous(), *ctx.dims)
        return gv, go, gl, None, None, None, None, None, None, None


def tsa_fused_forward(value, offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points,
                      shared_queue=False, order=None, value_rows=None, value_scale=None):
    """Fused TSA gather.  value: (B*2, Nq, M, D), or (B, Nq, M, D) with shared_queue=True when both
    queue entries are the same projected BEV (no history).  offs (B,Nq,M*2*P*2), logits
    (B,Nq,M*2*P), ref_2d (B*2,Nq,1,2).  -> (B, Nq, M*D).
    An int16 value holds q16 rows in the pixel-pair layout (linear_q16rows / sca_rows_encode_q16): (B*2 or B, S_pad, M, D)
    with S_pad = bev_h*bev_w rounded up to even, value_scale the 1-element float32 device tensor they were encoded with
    (None = 1) — occ_tsa_fused_forward_q16v; everything else as for fp32 rows.
    value_rows (B == 1 only): the queries are a ROW BAND of the BEV — offs / logits / ref_2d / order / the result cover
    Nq < bev_h*bev_w queries (order holds band-local indices) while `value` is the whole (bev_h*bev_w = value_rows)-pixel
    map: the encoder's row pipeline (plugin/encoder.py).
    order: None, or a contiguous int32 (Nq) tensor on value's device that must be a PERMUTATION of arange(Nq): wave r of a
    batch entry computes query order[r], so only locality depends on it.  Its values are not range-checked (that would cost
    a device sync): a repeated index leaves another row of the result unwritten, an index outside [0, Nq) reads and writes
    out of range.
    The kernel reads float2 offset pairs and 16-byte pieces of value rows: offs must start 8-byte aligned with an even row
    stride, value 16-byte aligned (any slice of a Linear output at an even column is)."""
    return _tsa_fused_forward(value, offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points, shared_queue, order,
                              value_rows, 'tsa_fused_forward', value_scale)


def _tsa_fused_forward(value, offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points, shared_queue, order, value_rows,
                       timing, value_scale=None):
    """tsa_fused_forward under the timing label `timing` (the training node keeps its launches apart from the inference
    gather's)."""
    q16 = isinstance(value, torch.Tensor) and value.dtype == torch.int16
    if q16:
        if not (value.is_cuda and value.is_contiguous() and value.dim() in (3, 4)):
            raise OccAmdError("tsa_fused_forward: q16 value must be a contiguous int16 device tensor (B*2 or B, S_pad, M, D)")
        if value_scale is not None and not (isinstance(value_scale, torch.Tensor) and value_scale.dtype == torch.float32
                                            and value_scale.numel() == 1 and value_scale.device == value.device):
            raise OccAmdError("tsa_fused_forward: value_scale must be a 1-element float32 tensor on value's device")
    else:
        if value_scale is not None:
            raise OccAmdError("tsa_fused_forward: value_scale goes with q16 (int16) value rows")
        _need_cuda_f32("value", value)
    _need_cuda_f32("ref_2d", ref_2d)
    _need_cuda_f32("offs", offs, contiguous=False)
    _need_cuda_f32("logits", logits, contiguous=False)
    if offs.dim() != 3 or logits.dim() != 3:
        raise OccAmdError("tsa_fused_forward: offs and logits must be (B,Nq,...)")
    B, Nq = offs.shape[:2]
    M, P = int(num_heads), int(num_points)
    Nv = Nq if value_rows is None else int(value_rows)
    if Nv != bev_h * bev_w or (value_rows is not None and B != 1):
        raise OccAmdError("tsa_fused_forward: the value map must have bev_h*bev_w rows (a query band needs B == 1)")
    # rows of one stored map: q16 maps are pixel pairs, padded to an even row count
    Nr = value.shape[1] if q16 else Nv
    D = value.shape[-1] // M if q16 and value.dim() == 3 else value.shape[-1]      # the encoders return (maps, S_pad, M*D)
    if q16 and Nr != Nv + (Nv & 1):
        raise OccAmdError("tsa_fused_forward: a q16 value map must have bev_h*bev_w rows rounded up to even")
    per = Nr * M * D
    if shared_queue:
        if value.numel() != B * per:
            raise OccAmdError("tsa_fused_forward: shared value must be (B,Nq,M,D)")
        if B != 1:
            # entry (b,t) lives at (b*2+t)*stride: aliasing both entries needs stride 0 -> B == 1
            value = torch.stack([value.view(B, Nr, M, D)] * 2, 1).reshape(B * 2, Nr, M, D).contiguous()
            stride = per
        else:
            stride = 0
    else:
        if value.numel() != 2 * B * per:
            raise OccAmdError("tsa_fused_forward: value must be (B*2,Nq,M,D)")
        stride = per
    if tuple(ref_2d.shape) != (B * 2, Nq, 1, 2):
        raise OccAmdError("tsa_fused_forward: ref_2d must be (B*2,Nq,1,2)")
    for n, t, w in (("offs", offs, M * 2 * P * 2), ("logits", logits, M * 2 * P)):
        # (the batch stride of a B == 1 tensor addresses nothing: a row band sliced out of a full-map Linear output keeps
        # the full map's)
        if tuple(t.shape[:2]) != (B, Nq) or t.shape[-1] != w or t.stride(-1) != 1 \
                or (B > 1 and t.stride(0) != Nq * t.stride(1)):
            raise OccAmdError(f"tsa_fused_forward: {n} must be (B,Nq,{w}) with unit inner stride")
    if offs.data_ptr() % 8 or offs.stride(1) % 2:
        raise OccAmdError("tsa_fused_forward: offs must be 8-byte aligned with an even row stride (float2 reads)")
    if value.data_ptr() % 16 or ref_2d.data_ptr() % 8:
        raise OccAmdError("tsa_fused_forward: value must be 16-byte aligned (and ref_2d 8-byte aligned)")
    if order is not None and not (isinstance(order, torch.Tensor) and order.dtype == torch.int32 and order.numel() == Nq
                                  and order.device == value.device and order.is_contiguous()):
        raise OccAmdError("tsa_fused_forward: order must be a contiguous int32 (Nq) tensor on value's device")
    out = torch.empty((B, Nq, M * D), dtype=torch.float32, device=value.device)
    if q16:
        _launch(_lib.lib().occ_tsa_fused_forward_q16v, value.device, "tsa_fused_forward", value, stride, Nr, offs,
                offs.stride(1), logits, logits.stride(1), ref_2d, order, out, B, Nq, bev_h, bev_w, M, D, P, value_scale,
                timing=timing)
    else:
        _launch(_lib.lib().occ_tsa_fused_forward_f32, value.device, "tsa_fused_forward", value, stride, offs, offs.stride(1),
                logits, logits.stride(1), ref_2d, order, out, B, Nq, bev_h, bev_w, M, D, P, timing=timing)
    return out


def tsa_fused_backward_workspace_bytes(B, Nq, bev_h, bev_w, M, D, P):
    """Bytes of scratch tsa_fused_backward takes for these shapes (0: no backward kernel for them)."""
    return _lib.lib().occ_tsa_fused_backward_workspace_bytes(B, Nq, bev_h, bev_w, M, D, P)


_TSA_LEVEL_TENSORS = {}


def _tsa_level_tensors(device, bev_h, bev_w):
    """spatial_shapes ((1, 2) int64) and level_start_index ((1,) int64) of the one BEV level on `device`, built by fill
    kernels (no host-to-device copy, so no device sync) and kept."""
    key = (str(device), int(bev_h), int(bev_w))
    hit = _TSA_LEVEL_TENSORS.get(key)
    if hit is None:
        shapes = torch.empty((1, 2), dtype=torch.int64, device=device)
        shapes[:, 0].fill_(int(bev_h))
        shapes[:, 1].fill_(int(bev_w))
        hit = _TSA_LEVEL_TENSORS[key] = (shapes, torch.zeros(1, dtype=torch.int64, device=device))
    return hit


def tsa_fused_backward(value, offs, logits, ref_2d, grad_out, bev_h, bev_w, num_heads, num_points, shared_queue=False,
                       want_value=True, want_query=True):
    """Gradient of tsa_fused_forward (csrc/tsa_fused_backward.hip).  Same inputs as the forward (no query bands, no `order`:
    it only steers locality) plus grad_out (B, Nq, M*D) -> (grad_value in value's layout, grad_offs (B, Nq, M*2*P*2),
    grad_logits (B, Nq, M*2*P)).  With shared_queue the kernel still writes one gradient map per queue entry and their sum
    is returned as the gradient of the single map.  want_value / want_query = False: that part is not computed and comes
    back as None.  grad_offs / grad_logits are bit-reproducible; grad_value too under OCC_MSDA_BWD_DETERMINISTIC=1.  Raises
    OccAmdUnsupported for shapes without a backward kernel."""
    _need_cuda_f32("value", value)
    _need_cuda_f32("ref_2d", ref_2d)
    _need_cuda_f32("offs", offs, contiguous=False)
    _need_cuda_f32("logits", logits, contiguous=False)
    _need_cuda_f32("grad_out", grad_out)
    if offs.dim() != 3 or logits.dim() != 3:
        raise OccAmdError("tsa_fused_backward: offs and logits must be (B,Nq,...)")
    if not (want_value or want_query):
        return None, None, None
    B, Nq = offs.shape[:2]
    M, D, P = int(num_heads), value.shape[-1], int(num_points)
    need = tsa_fused_backward_workspace_bytes(B, Nq, bev_h, bev_w, M, D, P)
    if need <= 0:
        raise OccAmdUnsupported(f"tsa_fused_backward: no backward kernel for M={M} D={D} P={P}, {Nq} queries on a "
                                f"{bev_h}x{bev_w} map")
    per = Nq * M * D
    if value.numel() != (B if shared_queue else 2 * B) * per:
        raise OccAmdError("tsa_fused_backward: value must be (B*2,Nq,M,D), or (B,Nq,M,D) with shared_queue")
    if shared_queue and B != 1:         # entry (b,t) lives at (b*2+t)*stride: the forward stacked the map as well
        src = torch.stack([value.view(B, Nq, M, D)] * 2, 1).reshape(B * 2, Nq, M, D).contiguous()
    else:
        src = value
    stride = 0 if shared_queue and B == 1 else per
    if tuple(ref_2d.shape) != (B * 2, Nq, 1, 2):
        raise OccAmdError("tsa_fused_backward: ref_2d must be (B*2,Nq,1,2)")
    for n, t, w in (("offs", offs, M * 2 * P * 2), ("logits", logits, M * 2 * P)):
        if tuple(t.shape[:2]) != (B, Nq) or t.shape[-1] != w or t.stride(-1) != 1 \
                or (B > 1 and t.stride(0) != Nq * t.stride(1)):
            raise OccAmdError(f"tsa_fused_backward: {n} must be (B,Nq,{w}) with unit inner stride")
    if tuple(grad_out.shape) != (B, Nq, M * D):
        raise OccAmdError(f"tsa_fused_backward: grad_out must be (B,Nq,{M * D})")
    if offs.data_ptr() % 8 or offs.stride(1) % 2:
        raise OccAmdError("tsa_fused_backward: offs must be 8-byte aligned with an even row stride (float2 reads)")
    if src.data_ptr() % 16 or grad_out.data_ptr() % 16 or ref_2d.data_ptr() % 8:
        raise OccAmdError("tsa_fused_backward: value and grad_out must be 16-byte aligned (and ref_2d 8-byte aligned)")
    dev = value.device
    shapes, lstart = _tsa_level_tensors(dev, bev_h, bev_w)
    # scratch from torch's caching allocator, freed back to the pool when this call returns (stream-ordered)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    # one gradient map per queue entry, also where the forward read one map twice: no aliasing writes in the launch
    gv2 = torch.zeros((B * 2, Nq, M, D), dtype=torch.float32, device=dev) if want_value else None
    grad_offs = torch.empty((B, Nq, M * 2 * P * 2), dtype=torch.float32, device=dev) if want_query else None
    grad_logits = torch.empty((B, Nq, M * 2 * P), dtype=torch.float32, device=dev) if want_query else None
    _launch(_lib.lib().occ_tsa_fused_backward_f32, dev, "tsa_fused_backward", src, stride, offs, offs.stride(1), logits,
            logits.stride(1), ref_2d, grad_out, shapes, lstart, gv2, grad_offs, M * 2 * P * 2, grad_logits, M * 2 * P, B, Nq,
            bev_h, bev_w, M, D, P, ws, need, timing='tsa_fused_backward')
    grad_value = None
    if want_value:
        grad_value = (gv2.view(B, 2, Nq, M, D).sum(1) if shared_queue else gv2).view(value.shape)
    return grad_value, grad_offs, grad_logits


class TSAFusedFunction(torch.autograd.Function):
    """The fused TSA gather as an autograd node: forward = occ_tsa_fused_forward_f32, backward = occ_tsa_fused_backward_f32.
    value (B*2, Nq, M, D) float32, or (B, Nq, M, D) with shared_queue; offs / logits (B, Nq, ...) — column slices of one
    Linear output are fine, autograd routes both gradients into it; ref_2d (B*2, Nq, 1, 2) is a constant -> (B, Nq, M*D).
    `order` steers the forward's locality only and is ignored in the backward.  Raises OccAmdUnsupported (before anything
    runs) for shapes without a backward kernel and for value_rows: the row pipeline is an inference device."""

    @staticmethod
    def forward(ctx, value, offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points, shared_queue=False, order=None,
                value_rows=None):
        if value_rows is not None:
            raise OccAmdUnsupported("TSAFusedFunction: no backward for a query band (value_rows)")
        if offs.dim() != 3:
            raise OccAmdError("TSAFusedFunction: offs and logits must be (B,Nq,...)")
        B, Nq = offs.shape[:2]
        M, D, P = int(num_heads), value.shape[-1], int(num_points)
        if tsa_fused_backward_workspace_bytes(B, Nq, int(bev_h), int(bev_w), M, D, P) <= 0:
            raise OccAmdUnsupported(f"TSAFusedFunction: no backward kernel for M={M} D={D} P={P}, {Nq} queries on a "
                                    f"{bev_h}x{bev_w} map")
        value = value.contiguous()
        # timed under a name of its own: 'tsa_fused_forward' is the inference gather's
        out = _tsa_fused_forward(value, offs, logits, ref_2d, bev_h, bev_w, num_heads, num_points, shared_queue, order, None,
                                 'tsa_fused_forward_train')
        ctx.save_for_backward(value, offs, logits, ref_2d)
        ctx.args = (int(bev_h), int(bev_w), M, P, bool(shared_queue))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        value, offs, logits, ref_2d = ctx.saved_tensors
        need_v, need_o, need_l = ctx.needs_input_grad[:3]
        bev_h, bev_w, M, P, shared = ctx.args
        gv, go, gl = tsa_fused_backward(value, offs, logits, ref_2d, grad_out.contiguous(), bev_h, bev_w, M, P,
                                        shared_queue=shared, want_value=need_v, want_query=need_o or need_l)
        return (gv, go if need_o else None, gl if need_l else None) + (None,) * 8


def conv3d_channel_block(cin):
    """Input channels contracted per LDS phase by the MFMA Conv3d kernel (0 = unsupported)."""
    return int(_lib.lib().occ_conv3d_channel_block(int(cin)))


CONV3D_PRECISION = os.environ.get("OCC_CONV3D_PRECISION", "bf16x3")   # 'bf16x3' (default) or 'f32'
# int16 elements of the packed bf16x3 weight for Cin = 8 (Cout = 32): that kernel contracts two taps per MFMA step, so the
# 27 taps are 14 steps (the 28th tap is zero weights) x (hi, lo) planes x 2 lane halves x 32 output channels x 8 channels
CONV3D_C8_PACKED_INT16 = 14 * 2 * 2 * 32 * 8


def conv3d_pack_weight(weight, precision=None):
    """torch Conv3d weight (Cout, Cin, 3, 3, 3) f32 -> packed MFMA B-fragment order (flat tensor): float32 for
    the exact-f32 kernel, int16 (bf16 hi/lo planes) for the bf16x3 kernel (Cin % 16 == 0, else f32)."""
    _need_cuda_f32("weight", weight)
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise OccAmdError("conv3d_pack_weight: expected a (Cout, Cin, 3, 3, 3) weight")
    cout, cin = weight.shape[:2]
    precision = precision or CONV3D_PRECISION
    if precision == 'bf16x3' and (cin % 16 == 0 or (cin == 8 and cout == 32)):
        n16 = CONV3D_C8_PACKED_INT16 if cin == 8 else weight.numel() * 2
        packed = torch.empty(n16, dtype=torch.int16, device=weight.device)
        _launch(_lib.lib().occ_conv3d_pack_weight_bf16x3, weight.device, "conv3d_pack_weight", weight, packed, cin, cout)
        return packed
    packed = torch.empty(weight.numel(), dtype=torch.float32, device=weight.device)
    _launch(_lib.lib().occ_conv3d_pack_weight_f32, weight.device, "conv3d_pack_weight", weight, packed, cin, cout)
    return packed


def conv3d_bn_relu(x, w_packed, scale, shift, Z, Y, X, cin, cout, in_layout, out_xy_major=False,
                   relu=True):
    """Lifter/Conv3d(k3,p1)+BN(eval)+ReLU on the matrix cores; the kernel (exact f32, or bf16x3: operands split
    into hi + lo bf16, f32 accumulation) follows the dtype of `w_packed` (conv3d_pack_weight).

    x: in_layout 0 -> (B, Y, X, Z, cin); in_layout 1 -> (B, Y*X, cin*Z) BEV embedding (lifter view).
    -> (B, Y, X, Z, cout), or (B, X, Y, Z, cout) with out_xy_major (the reference's
    permute(0,4,3,2,1) order, transformer_occ.py:308)."""
    for n, t in (("x", x), ("scale", scale), ("shift", shift)):
        _need_cuda_f32(n, t)
    x3 = w_packed.dtype == torch.int16
    if not (w_packed.is_cuda and w_packed.is_contiguous() and (x3 or w_packed.dtype == torch.float32)):
        raise OccAmdError("conv3d_bn_relu: w_packed must come from conv3d_pack_weight")
    B = x.shape[0]
    n_w = (CONV3D_C8_PACKED_INT16 if cin == 8 else cout * cin * 27 * 2) if x3 else cout * cin * 27
    if x.numel() != B * Y * X * Z * cin or w_packed.numel() != n_w \
            or scale.numel() != cout or shift.numel() != cout:
        raise OccAmdError("conv3d_bn_relu: inconsistent shapes")
    if out_xy_major:
        out = torch.empty((B, X, Y, Z, cout), dtype=torch.float32, device=x.device)
        sy, sx = Z * cout, Y * Z * cout
    else:
        out = torch.empty((B, Y, X, Z, cout), dtype=torch.float32, device=x.device)
        sy, sx = X * Z * cout, Z * cout
    fn = _lib.lib().occ_conv3d_bn_relu_bf16x3_f32 if x3 else _lib.lib().occ_conv3d_bn_relu_f32
    _launch(fn, x.device, "conv3d_bn_relu", x, w_packed, scale, shift, out, B, Z, Y, X, cin, cout, int(in_layout),
            Y * X * Z * cout, sy, sx, 1 if relu else 0, timing='conv3d_bn_relu')
    return out


def conv3d_heads_pack(w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow):
    """The eight head tensors (C = 32, hidden = 64) -> the operand buffer of conv3d_heads_decode (bf16 hi/lo MFMA
    fragments + biases; uint8 tensor)."""
    ts = (w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow)
    for n, t in zip(("w1_occ", "b1_occ", "w2_occ", "b2_occ", "w1_flow", "b1_flow", "w2_flow", "b2_flow"), ts):
        _need_cuda_f32(n, t)
    hidden, C = w1_occ.shape
    ncls = w2_occ.shape[0]
    if (tuple(w1_flow.shape) != (hidden, C) or tuple(w2_occ.shape) != (ncls, hidden) or tuple(w2_flow.shape) != (2, hidden)
            or b1_occ.numel() != hidden or b1_flow.numel() != hidden or b2_occ.numel() != ncls or b2_flow.numel() != 2):
        raise OccAmdError("conv3d_heads_pack: inconsistent weight shapes")
    lib = _lib.lib()
    packed = torch.empty(int(lib.occ_conv3d_heads_pack_bytes()), dtype=torch.uint8, device=w1_occ.device)
    _launch(lib.occ_conv3d_heads_pack, w1_occ.device, "conv3d_heads_pack", *ts, packed, C, hidden, ncls)
    packed._occ_heads_meta = (int(C), int(hidden), int(ncls))     # the fragment layout bakes these in: checked at use
    return packed


def conv3d_heads_decode(x, w_packed, scale, shift, heads_packed, Z, Y, X, num_classes):
    """Second decoder convolution + BN(eval) + ReLU + both occupancy heads + argmax decode in one launch: x
    (B, Y, X, Z, 32) fp32 -> occ (B, X, Y, Z, num_classes), flow (B, X, Y, Z, 2), occ_cls (B, X, Y, Z) int64 — what
    conv3d_bn_relu(out_xy_major=True) + occ_heads(decode=True) produce, without the 82 MB round trip of the
    convolution's output.  w_packed: conv3d_pack_weight (bf16x3); heads_packed: conv3d_heads_pack."""
    for n, t in (("x", x), ("scale", scale), ("shift", shift)):
        _need_cuda_f32(n, t)
    if w_packed.dtype != torch.int16:
        raise OccAmdUnsupported("conv3d_heads_decode: needs the bf16x3 packed weight")
    meta = getattr(heads_packed, '_occ_heads_meta', None)
    if meta is not None and meta[2] != int(num_classes):
        raise OccAmdError(f"conv3d_heads_decode: heads were packed for {meta[2]} classes, called with {num_classes}")
    B = x.shape[0]
    cin = x.numel() // (B * Y * X * Z)
    if x.numel() != B * Y * X * Z * cin or w_packed.numel() != 32 * cin * 27 * 2:
        raise OccAmdError("conv3d_heads_decode: inconsistent shapes")
    occ = torch.empty((B, X, Y, Z, num_classes), dtype=torch.float32, device=x.device)
    flow = torch.empty((B, X, Y, Z, 2), dtype=torch.float32, device=x.device)
    cls = torch.empty((B, X, Y, Z), dtype=torch.int64, device=x.device)
    _launch(_lib.lib().occ_conv3d_heads_decode_bf16x3_f32, x.device, "conv3d_heads_decode", x, w_packed, scale, shift,
            heads_packed, occ, flow, cls, B, Z, Y, X, cin, num_classes, timing='conv3d_heads')
    return occ, flow, cls


HEADS_PRECISION = os.environ.get("OCC_HEADS_PRECISION", "bf16x3")    # 'bf16x3' (default) or 'f32'


def occ_heads(feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, decode=False,
              precision=None):
    """feat (..., C) -> occ (..., num_classes), flow (..., 2): both decoder MLP heads in one kernel.  With `decode`
    the same pass also writes argmax_c occ (int64, first index on ties): -> (occ, flow, occ_cls)."""
    ts = (feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow)
    for n, t in zip(("feat", "w1_occ", "b1_occ", "w2_occ", "b2_occ", "w1_flow", "b1_flow", "w2_flow",
                     "b2_flow"), ts):
        _need_cuda_f32(n, t)
    C = feat.shape[-1]
    hidden, ncls = w1_occ.shape[0], w2_occ.shape[0]
    if (tuple(w1_occ.shape) != (hidden, C) or tuple(w1_flow.shape) != (hidden, C) or
            tuple(w2_occ.shape) != (ncls, hidden) or tuple(w2_flow.shape) != (2, hidden) or
            b1_occ.numel() != hidden or b1_flow.numel() != hidden or b2_occ.numel() != ncls or
            b2_flow.numel() != 2):
        raise OccAmdError("occ_heads: inconsistent weight shapes")
    n_rows = feat.numel() // C
    occ = torch.empty(feat.shape[:-1] + (ncls,), dtype=torch.float32, device=feat.device)
    flow = torch.empty(feat.shape[:-1] + (2,), dtype=torch.float32, device=feat.device)
    cls = torch.empty(feat.shape[:-1], dtype=torch.int64, device=feat.device) if decode else None
    _launch(_lib.lib().occ_occ_heads_decode_f32, feat.device, "occ_heads", feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow,
            b1_flow, w2_flow, b2_flow, occ, flow, cls, n_rows, C, hidden, ncls,
            1 if (precision or HEADS_PRECISION) == "f32" else 0, timing='occ_heads')
    return (occ, flow, cls) if decode else (occ, flow)


def _rows2d(name, t, k=None):
    """(…, K) tensor -> (data tensor, M, K, row stride) for the Linear kernel: rows must be uniformly
    strided, unit inner stride, 16-byte aligned."""
    _need_cuda_f32(name, t, contiguous=False)
    K = t.shape[-1]
    if k is not None and K != k:
        raise OccAmdError(f"linear: {name} has {K} columns, expected {k}")
    if t.dim() == 2 and t.stride(1) == 1:
        ld = t.stride(0)
    elif t.is_contiguous():
        ld = K
    else:
        raise OccAmdError(f"linear: {name} must be contiguous or a 2-D row-strided view")
    M = t.numel() // K
    if t.data_ptr() % 16 or ld % 4:
        raise OccAmdUnsupported(f"linear: {name} rows are not 16-byte aligned")
    return t, M, K, ld


# Precision of the MFMA Linear kernel: 'f32' = v_mfma_f32_32x32x2_f32 (exact fp32, bitwise an fmaf
# chain), 'bf16x3' = three bf16 MFMAs on hi/lo-split operands with f32 accumulation (relative error of a
# product <= 2^-16; 2-3x faster).  The default can be overridden with OCC_LINEAR_PRECISION.
LINEAR_PRECISION = os.environ.get("OCC_LINEAR_PRECISION", "bf16x3")
_PACKED_W = DerivedCache("linear_pack_weight_bf16x3", 256, register=True)


def linear_pack_weight_bf16x3(weight):
    """(N, K) float32 Linear weight -> bf16 hi/lo split in MFMA fragment order
    packed[K/16][ceil(N/32)][hi, lo][lane][8] (int16 storage, columns zero-padded to a multiple of 32), cached.
    Temporaries (a transposed weight in a backward pass, a concatenation rebuilt every forward) are marked `_occ_no_cache`
    by their producer and packed without entering the cache."""
    def build():
        _need_cuda_f32("weight", weight)
        N, K = weight.shape
        packed = torch.empty((N + 31) // 32 * 32 * K * 2, dtype=torch.int16, device=weight.device)
        _launch(_lib.lib().occ_linear_pack_weight_bf16x3, weight.device, "linear_pack_weight_bf16x3", weight, packed, N, K)
        return packed
    return _PACKED_W.get((weight,), build)


def _check_out_scale(what, out_scale, planes, out):
    if out_scale is None:
        return
    if not (out_scale.is_cuda and out_scale.dtype == torch.float32 and out_scale.dim() == 1 and out_scale.is_contiguous()
            and out_scale.numel() >= planes and out_scale.device == out.device):
        raise OccAmdError(f"{what}: out_scale must be a contiguous float32 device vector of >= {planes} entries")


def _range_terms_dev(row_l1, bias_max, dev):
    """(P,) float32 device vectors of the two weight-side terms: device tensors pass through, host floats are uploaded."""
    def one(v):
        if isinstance(v, torch.Tensor):
            t = v.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        else:
            t = torch.tensor([float(x) for x in v], dtype=torch.float32, device=dev)
        return t
    r, b = one(row_l1), one(bias_max)
    if r.numel() != b.numel() or r.numel() == 0:
        raise OccAmdError("value_range_scale: row_l1 and bias_max must have one entry per plane")
    return r, b


def value_range_scale(a_list, row_l1, bias_max):
    """Per-plane power-of-two scales for fp16 storage of the projections of the bf16 feature rows `a_list` (csrc/value_range.hip):
    -> float32 device vector t of 2 P + 1 entries, t[:P] = s_p with  (max|x| * row_l1[p] * (1 + 2^-8) + bias_max[p]) * s_p <= 2^15,
    t[P] = max|x| over every map, t[P + 1 + p] = the bound of plane p (diagnostics).  row_l1[p] = max_n sum_k |W_p[n][k]|,
    bias_max[p] = max |group bias of p| — (P,) float32 DEVICE tensors (round 6; host sequences are uploaded: tests).  No host
    synchronisation; a memset node + one launch on the current stream.  Pass t[:P] as value_proj_bf16*(out_scale=) and
    t[p:p+1] as sca_fused_forward(value_scale=)."""
    if isinstance(a_list, torch.Tensor):
        a_list = [a_list]
    S = len(a_list)
    K = a_list[0].shape[1]
    for a in a_list:
        if not (a.is_cuda and a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and a.shape[1] == K):
            raise OccAmdUnsupported("value_range_scale: every a must be a (M, K) bfloat16 device matrix with unit column stride")
    dev = a_list[0].device
    r, b = _range_terms_dev(row_l1, bias_max, dev)
    P = r.numel()
    # 2 P + 1 result floats + the kernel's two work words in ONE allocation of the caller's pool (the launcher zeroes the
    # words: nothing is cached across calls, streams or graph captures)
    buf = torch.empty(2 * P + 3, dtype=torch.float32, device=dev)
    out, work = buf[:2 * P + 1], buf[2 * P + 1:]
    arr64 = lambda v: (ctypes.c_int64 * S)(*[int(x) for x in v])
    a_ptrs = (ctypes.c_void_p * S)(*[a.data_ptr() for a in a_list])
    _launch(_lib.lib().occ_value_range_scale_bf16, dev, "value_range_scale", S, a_ptrs, arr64([a.stride(0) for a in a_list]),
            arr64([a.shape[0] for a in a_list]), K, P, r, b, out, work, timing='value_range')
    return out


def new_absmax_words(device):
    """8 zeroed device words for conv3x3_nhwc(amax=...): the producer side of value_range_scale_from_amax."""
    return torch.zeros(8, dtype=torch.int32, device=device)


def attach_absmax(t, words):
    """Hang the producer's max|x| words on a feature-map tensor (or a view of one) together with the tensor's version counter:
    an in-place write to the map afterwards invalidates the side band (absmax_of returns None, the consumer measures)."""
    t._occ_absmax = words
    t._occ_absmax_version = t._version
    return t


def absmax_of(t):
    """The words attach_absmax hung on `t`, or None (none attached, or the map was written in place since)."""
    w = getattr(t, '_occ_absmax', None)
    if w is None or getattr(t, '_occ_absmax_version', None) != t._version:
        return None
    return w


def feature_absmax_words(a_list):
    """The 8 words a producer would have accumulated, for maps that did not come from this library's backbone plan (bench
    set-up, tests): max of the sign-stripped bf16 patterns of every element, replicated."""
    if isinstance(a_list, torch.Tensor):
        a_list = [a_list]
    m = torch.stack([(a.detach().contiguous().view(torch.int16).to(torch.int32) & 0x7fff).amax() for a in a_list]).amax()
    return m.to(torch.int32).reshape(1).repeat(8)


def value_range_scale_from_amax(amax8, row_l1, bias_max):
    """value_range_scale when the producer of the maps accumulated max|x| itself (conv3x3_nhwc(amax=...) of the backbone plan's
    FPN output convolutions): one 64-thread launch instead of a pass over the maps.  Same result vector."""
    if not (isinstance(amax8, torch.Tensor) and amax8.is_cuda and amax8.dtype == torch.int32 and amax8.numel() == 8
            and amax8.is_contiguous()):
        raise OccAmdError("value_range_scale_from_amax: amax8 must be 8 contiguous int32 device words")
    return _range_scale_from_amax(amax8, row_l1, bias_max, 'value_range')


def _range_scale_from_amax(amax8, row_l1, bias_max, timing):
    """The launch of value_range_scale_from_amax, under the timing label `timing` (tsa_value_scale keeps its launches out of
    the SCA planes' 'value_range' figure)."""
    dev = amax8.device
    r, b = _range_terms_dev(row_l1, bias_max, dev)
    P = r.numel()
    out = torch.empty(2 * P + 1, dtype=torch.float32, device=dev)
    _launch(_lib.lib().occ_value_range_scale_from_amax, dev, "value_range_scale_from_amax", amax8, P, r, b, out, timing=timing)
    return out


def f16_range_scaled(v):
    """fp32 value rows -> (fp16 rows holding s * v, s as a 1-element float32 device tensor), s the power of two that puts
    max|v| into [2^14, 2^15]: the ATen counterpart of value_range_scale for value tensors that were projected in fp32 (the
    non-LazyFeatures inputs of the fused SCA gather).  No host synchronisation; Inf / NaN / all-zero rows: s = 1."""
    amax = v.detach().abs().amax().float()
    _, e = torch.frexp(amax)
    ok = torch.isfinite(amax) & (amax > 0)
    s = torch.where(ok, torch.ldexp(torch.ones_like(amax), (15 - e).clamp(-100, 100)), torch.ones_like(amax))
    return (v * s).clamp(-65504.0, 65504.0).half(), s.reshape(1)


def sca_rows_encode_q16(v, scale=None):
    """fp32 value rows (BN, S, C) [or (BN, S, M, D)], C = heads * 32 -> q16 pixel pairs: int16 (BN, S + (S & 1), C) in the fused
    gather's pair order, each 16-byte piece of 8 channels holding int16 mantissas of scale * v under one 4-bit exponent
    (csrc/common.h; numpy restatement: tests/q16_ref.py).  scale: 1-element float32 device tensor, a power of two with
    max|v| * scale <= 2^15 (q16_range_scaled derives it), None = 1."""
    _need_cuda_f32("v", v)
    BN, S = v.shape[0], v.shape[1]
    C = v.numel() // (BN * S)
    out = torch.empty((BN, S + (S & 1), C), dtype=torch.int16, device=v.device)
    if S & 1:                                    # the pad pixel (second slot of the last pair, every head): never sampled, kept defined
        out.view(BN, (S + 1) // 2, C // 32, 2, 32)[:, -1, :, 1, :].zero_()
    _launch(_lib.lib().occ_sca_rows_encode_q16, v.device, "sca_rows_encode_q16", v, out, scale, BN, S, C)
    return out


def q16_range_scaled(v):
    """fp32 value rows -> (q16 pixel pairs, s): the q16 counterpart of f16_range_scaled (same power-of-two rule for s)."""
    amax = v.detach().abs().amax().float()
    _, e = torch.frexp(amax)
    ok = torch.isfinite(amax) & (amax > 0)
    s = torch.where(ok, torch.ldexp(torch.ones_like(amax), (15 - e).clamp(-100, 100)), torch.ones_like(amax)).reshape(1)
    return sca_rows_encode_q16(v.contiguous(), s), s


# ---- range scale of the q16 TSA value rows (OCC_TSA_VALUES=q16) from fp32 inputs, without a scale kernel of its own ---------
def absmax_words_f32(a_or_bound):
    """A float32 tensor (its max|a| is taken) or scalar bound -> the 8 int32 words value_range_scale_from_amax reads: the
    bf16 pattern of the bound ROUNDED UP, (bits + 0xffff) >> 16 on the sign-stripped fp32 bits, so the pattern never decodes to
    less than the bound (and to less than bound * (1 + 2^-7) for a normal number).  ATen ops on the tensor's device, no host
    synchronisation.  Inf / NaN give an Inf / NaN pattern: the scale kernel then returns s = 1, as q16_range_scaled does."""
    m = a_or_bound.detach().to(torch.float32).abs().reshape(-1).amax()
    bits = m.view(torch.int32).to(torch.int64) & 0x7fffffff
    pattern = ((bits + 0xffff) >> 16).clamp(max=0x7fff)           # (0x7fff: a NaN pattern, not the sign bit)
    return pattern.to(torch.int32).reshape(1).repeat(8)


_LN_BOUND = DerivedCache("layernorm_bound_words", 64, register=True)        # (gamma, beta) -> words
_TSA_RANGE_TERMS = DerivedCache("tsa_value_scale", 64, register=True)       # (weight, bias) -> (row_l1, bias_max)


def layernorm_bound_words(ln):
    """absmax_words_f32 of the analytic bound of a LayerNorm's output over N channels (ln: nn.LayerNorm or (gamma, beta, eps)):
    sum_c (x_c - mean) = 0 gives (x_c - mean)^2 <= (N - 1) var, so |y_c| <= |gamma_c| sqrt(N - 1) + |beta_c| for any input row
    and any eps >= 0; 2^-8 of slack covers the fp32 arithmetic of the kernels: both LayerNorm epilogues (csrc/linear_bf16x3.hip,
    csrc/linear_chain_x3.hip) square the very deviations d_c they normalise, so |d_c| rstd <= sqrt(N) holds whatever the
    rounding of the mean, and sqrt(N) / sqrt(N - 1) is inside the slack from N = 129 on (they run at N = 256).  Cached on
    (gamma, beta) identity."""
    g, b = (ln.weight, ln.bias) if isinstance(ln, torch.nn.LayerNorm) else (ln[0], ln[1])
    def build():
        n = g.numel()
        bound = g.detach().float().abs().amax() * (float(max(n - 1, 0)) ** 0.5 * 1.00390625)
        if b is not None:
            bound = bound + b.detach().float().abs().amax()
        return absmax_words_f32(bound)
    return _LN_BOUND.get((g, b), build)


def _attach_ln_bound(t, gamma, beta):
    """A LayerNorm output leaves linear(ln=) / linear_ln_chain / encoder_ffn_chain with its analytic bound attached
    (attach_absmax: an in-place write drops it), for the q16 value projection that may consume it.  Only under
    OCC_TSA_VALUES=q16: nobody reads the words otherwise, and the default path stays free of even the cache lookup."""
    if TSA_VALUES == "q16":
        attach_absmax(t, layernorm_bound_words((gamma, beta, 0.0)))


def tsa_value_scale(value_proj, words):
    """The power-of-two range scale s (1-element float32 device tensor) of the q16 rows of value_proj(x) for inputs with
    max|x| <= the bound in `words` (absmax_words_f32 / layernorm_bound_words / absmax_of):
    (bound * row_l1 * (1 + 2^-8) + bias_max) * s <= 2^15 with row_l1 = max_n sum_k |W_nk|, bias_max = max|b| (device tensors,
    cached per weight version) — occ_value_range_scale_from_amax, one 64-thread launch."""
    w, b = value_proj.weight, value_proj.bias
    def build():
        row_l1 = w.detach().float().abs().sum(1).amax().reshape(1)
        bias_max = (b.detach().float().abs().amax() if b is not None else torch.zeros((), device=w.device)).reshape(1)
        return row_l1, bias_max
    row_l1, bias_max = _TSA_RANGE_TERMS.get((w, b), build)
    if not (isinstance(words, torch.Tensor) and words.is_cuda and words.dtype == torch.int32 and words.numel() == 8
            and words.is_contiguous()):
        raise OccAmdError("tsa_value_scale: words must be 8 contiguous int32 device words")
    return _range_scale_from_amax(words, row_l1, bias_max, 'tsa_value_range')[:1]


def linear_q16rows(a, weight, bias, scale, groups, act=None, residual=None, ln=None):
    """The plain bf16x3 Linear a @ weight^T + bias with a q16 epilogue (csrc/linear_bf16x3.hip): the M rows of `a` are
    `groups` maps of S = M / groups rows; -> int16 (groups, S + (S & 1), 256) q16 pixel pairs, bit for bit what
    sca_rows_encode_q16(linear(a, weight, bias).view(groups, S, 256), scale) returns, without the fp32 round trip.  scale: the
    1-element float32 device tensor s (tsa_value_scale), None = 1.  Covers N == 256, K % 16 == 0, the bf16x3 precision mode and
    no activation / residual / LayerNorm: OccAmdUnsupported otherwise (nothing is launched)."""
    if act is not None or residual is not None or ln is not None:
        raise OccAmdUnsupported("linear_q16rows: the q16 epilogue takes no activation, residual or LayerNorm")
    if LINEAR_PRECISION != "bf16x3":
        raise OccAmdUnsupported("linear_q16rows: bf16x3 precision mode only")
    a_, M, K, lda = _rows2d("a", a)
    _need_cuda_f32("weight", weight)
    if weight.dim() != 2 or weight.shape[1] != K or not weight.is_contiguous():
        raise OccAmdError("linear_q16rows: weight must be a contiguous (N, K) matrix")
    N = weight.shape[0]
    if N != 256 or K % 16:
        raise OccAmdUnsupported(f"linear_q16rows: no kernel for N={N} K={K} (need N == 256, K % 16 == 0)")
    if bias is not None:
        _need_cuda_f32("bias", bias)
        if bias.numel() != N:
            raise OccAmdError("linear_q16rows: bias must have N entries")
    groups = int(groups)
    if groups <= 0 or M % groups:
        raise OccAmdError(f"linear_q16rows: {M} rows do not split into {groups} maps")
    if scale is not None and not (isinstance(scale, torch.Tensor) and scale.is_cuda and scale.dtype == torch.float32
                                  and scale.numel() == 1 and scale.device == a.device):
        raise OccAmdError("linear_q16rows: scale must be a 1-element float32 tensor on a's device")
    S = M // groups
    wp = linear_pack_weight_bf16x3(weight)
    out = torch.empty((groups, S + (S & 1), N), dtype=torch.int16, device=a.device)
    if S & 1:                                    # the pad pixel of every map: never sampled, kept defined (sca_rows_encode_q16)
        out.view(groups, (S + 1) // 2, N // 32, 2, 32)[:, -1, :, 1, :].zero_()
    _launch(_lib.lib().occ_linear_bf16x3_q16rows, a.device, "linear_q16rows", a_, lda, K, wp, bias, scale, out, M, N, groups,
            timing='linear', flops=2.0 * M * N * K)
    return out


def value_proj_bf16(a_list, weight, group_bias, out, rows_per_group, out_group_rows, out_row0, out_scale=None):
    """For every segment s (FPN level) and row m = g*rows_per_group[s] + i of a_list[s]:
        out[g*out_group_rows + out_row0[s] + i] = a_list[s][m] @ weight.T + group_bias[s][g % G]   (fp32 out),
    all segments in one launch.  An fp16 `out` is the fused SCA gather's operand and is written in its pixel-PAIR
    order (sca_pair_layout: row r of a group's block lands at [r >> 1][head][r & 1][32]; out_group_rows must be even,
    N a multiple of 32, rows contiguous) — read it back in row order with sca_unpair_layout.  a_list[s] (M_s, K) bf16 with unit column stride (an NHWC feature map seen as
    pixels x channels); weight (N, K) fp32 Linear weight (packed hi/lo once, cached); group_bias (S, G, N) fp32
    contiguous or None; out fp32 2-D (rows, N); rows_per_group / out_row0: one int per segment.
    out_scale (fp16 out only): float32 device vector, out = fp16(out_scale[0] * (...)) — value_range_scale()."""
    if isinstance(a_list, torch.Tensor):
        a_list, rows_per_group, out_row0 = [a_list], [rows_per_group], [out_row0]
        if group_bias is not None:
            group_bias = group_bias.unsqueeze(0)
    S = len(a_list)
    out_q16 = out.dtype == torch.int16
    out_half = out.dtype == torch.float16 or out_q16
    if not out_half:
        _need_cuda_f32("out", out)
    if not out.is_cuda or out.dim() != 2 or out.stride(1) != 1:
        raise OccAmdError("value_proj_bf16: out must be a 2-D fp32 (or fp16) device matrix with unit column stride")
    N, K = weight.shape
    if out.shape[1] != N or len(rows_per_group) != S or len(out_row0) != S:
        raise OccAmdError("value_proj_bf16: inconsistent shapes")
    for a, rpg, r0 in zip(a_list, rows_per_group, out_row0):
        if not (a.is_cuda and a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1
                and a.shape[1] == K):
            raise OccAmdUnsupported("value_proj_bf16: every a must be a (M, K) bfloat16 device matrix with unit "
                                    "column stride")
        groups = (a.shape[0] + rpg - 1) // rpg
        if (groups - 1) * out_group_rows + r0 + min(rpg, a.shape[0]) > out.shape[0]:
            raise OccAmdError("value_proj_bf16: output rows out of range")
    G = 0
    gb_ptrs = None
    if group_bias is not None:
        _need_cuda_f32("group_bias", group_bias)
        if group_bias.dim() != 3 or group_bias.shape[0] != S or group_bias.shape[2] != N \
                or not group_bias.is_contiguous():
            raise OccAmdError("value_proj_bf16: group_bias must be a contiguous (S, G, N) tensor")
        G = group_bias.shape[1]
        gb_ptrs = (ctypes.c_void_p * S)(*[group_bias[s].data_ptr() for s in range(S)])
    if out_scale is not None and not out_half:
        raise OccAmdError("value_proj_bf16: out_scale goes with an fp16 out")
    _check_out_scale("value_proj_bf16", out_scale, 1, out)
    packed = linear_pack_weight_bf16x3(weight)
    arr64 = lambda v: (ctypes.c_int64 * S)(*[int(x) for x in v])
    a_ptrs = (ctypes.c_void_p * S)(*[a.data_ptr() for a in a_list])
    fn = (_lib.lib().occ_value_proj_bf16_q16pairs if out_q16 else _lib.lib().occ_value_proj_bf16_f16pairs if out_half
          else _lib.lib().occ_value_proj_bf16_f32)
    _launch(fn, out.device, "value_proj_bf16", S, a_ptrs, arr64([a.stride(0) for a in a_list]),
            arr64([a.shape[0] for a in a_list]), arr64(rows_per_group), arr64(out_row0), gb_ptrs, G, packed, out,
            out.stride(0), K, N, out_group_rows, *((out_scale,) if out_half else ()), timing='value_proj')
    return out


_STACKED_VP = DerivedCache("value_proj_planes_prepare", 8, register=True)    # weights -> (stacked weight, its pack, weights)
_STACKED_GB = DerivedCache("value_proj_bf16_planes bias", 8, register=True)  # bias tables -> their concatenation


def value_proj_planes_prepare(weights):
    """The stacked + packed weight of value_proj_bf16_planes for this list of projections (cached on the weights'
    identities): built on the CURRENT stream.  A caller that launches value_proj_bf16_planes on a side stream calls this
    on the main stream first, so that no main-stream reader of the cache entry can race its construction."""
    def build():
        stacked = torch.cat([w.detach() for w in weights], 0).contiguous()
        stacked._occ_no_cache = True
        return stacked, linear_pack_weight_bf16x3(stacked), list(weights)
    return _STACKED_VP.get(weights, build)


def value_proj_bf16_planes(a_list, weights, group_biases, out, rows_per_group, out_group_rows, out_row0, out_scale=None):
    """The same rows through SEVERAL projections in one launch (the encoder layers' SCA value projections):
    out[p] = value_proj_bf16(a_list, weights[p], group_biases[p], ...) for every p, feature rows read from HBM once.
    weights: list of P (N, K) fp32 Linear weights (N % 256 == 0); group_biases: list of P (S, G, N) fp32 or None;
    out (P, rows, N) fp32 or fp16, contiguous.  out_scale: float32 device vector of P per-plane factors
    (value_range_scale()), plane p = out_scale[p] * (...)."""
    P, S = len(weights), len(a_list)
    N, K = weights[0].shape
    if any(tuple(w.shape) != (N, K) for w in weights) or N % 256:
        raise OccAmdUnsupported("value_proj_bf16_planes: equal (N, K) weights with N % 256 == 0 needed")
    out_q16 = out.dtype == torch.int16
    out_half = out.dtype == torch.float16 or out_q16
    if not (out.is_cuda and out.dim() == 3 and out.shape[0] == P and out.shape[2] == N and out.is_contiguous()
            and (out_half or out.dtype == torch.float32)):
        raise OccAmdError("value_proj_bf16_planes: out must be a contiguous (P, rows, N) fp32 / fp16 / int16 (q16) device tensor")
    for a, rpg, r0 in zip(a_list, rows_per_group, out_row0):
        if not (a.is_cuda and a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and a.shape[1] == K):
            raise OccAmdUnsupported("value_proj_bf16_planes: every a must be a (M, K) bfloat16 device matrix with unit "
                                    "column stride")
        groups = (a.shape[0] + rpg - 1) // rpg
        if (groups - 1) * out_group_rows + r0 + min(rpg, a.shape[0]) > out.shape[1]:
            raise OccAmdError("value_proj_bf16_planes: output rows out of range")
    _check_out_scale("value_proj_bf16_planes", out_scale, P, out)
    hit = value_proj_planes_prepare(weights)
    gb_ptrs, G, gb_keep = None, 0, None
    if group_biases is not None and group_biases[0] is not None:
        # (S, G, P*N), cached on the per-projection bias tables' identities: it was a cat kernel per step in front of the
        # side stream's projection launch
        gb_keep = _STACKED_GB.get(group_biases, lambda: torch.cat(list(group_biases), 2).contiguous())
        G = gb_keep.shape[1]
        gb_ptrs = (ctypes.c_void_p * S)(*[gb_keep[s].data_ptr() for s in range(S)])
    arr64 = lambda v: (ctypes.c_int64 * S)(*[int(x) for x in v])
    a_ptrs = (ctypes.c_void_p * S)(*[a.data_ptr() for a in a_list])
    _launch(_lib.lib().occ_value_proj_bf16_planes, out.device, "value_proj_bf16_planes", S, a_ptrs,
            arr64([a.stride(0) for a in a_list]), arr64([a.shape[0] for a in a_list]), arr64(rows_per_group), arr64(out_row0),
            gb_ptrs, G, hit[1], out, 2 if out_q16 else 1 if out_half else 0, N, K, P, N, out.stride(0), out_group_rows,
            out_scale, timing='value_proj')
    return out


def linear(a, weight, bias=None, a2=None, a2_add=None, act=None, residual=None, ln=None,
           precision=None):
    """out = LayerNorm(residual + act([a | a2 (+ a2_add)] @ weight^T + bias)) on the f32 matrix cores.

    a (…, K1); a2 / a2_add (…, K2) optional second K segment (+ addend); weight (N, K1+K2) and bias (N)
    in torch Linear layout; act None | 'relu'; residual (…, N); ln = (gamma, beta, eps) or an
    nn.LayerNorm; precision 'f32' | 'bf16x3' (None = LINEAR_PRECISION).  -> (…, N) float32.  Raises
    OccAmdUnsupported for shapes without an MFMA kernel."""
    precision = precision or LINEAR_PRECISION
    if precision not in ("f32", "bf16x3"):
        raise OccAmdError(f"linear: unknown precision {precision!r}")
    a_, M, K1, lda1 = _rows2d("a", a)
    K2, lda2 = 0, 0
    if a2 is not None:
        a2_, M2, K2, lda2 = _rows2d("a2", a2)
        if M2 != M:
            raise OccAmdError("linear: a and a2 differ in rows")
        if a2_add is not None:
            _, M3, _, lda3 = _rows2d("a2_add", a2_add, K2)
            if M3 != M or lda3 != lda2:
                raise OccAmdError("linear: a2_add must match a2's shape and row stride")
    elif a2_add is not None:
        raise OccAmdError("linear: a2_add without a2")
    _need_cuda_f32("weight", weight)
    N = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K1 + K2:
        raise OccAmdError("linear: weight must be (N, K1+K2)")
    if bias is not None:
        _need_cuda_f32("bias", bias)
        if bias.numel() != N:
            raise OccAmdError("linear: bias must have N entries")
    ldres = 0
    if residual is not None:
        _, Mr, _, ldres = _rows2d("residual", residual, N)
        if Mr != M:
            raise OccAmdError("linear: residual differs in rows")
    g = b = None
    eps = 0.0
    if ln is not None:
        if isinstance(ln, torch.nn.LayerNorm):
            if tuple(ln.normalized_shape) != (N,) or ln.weight is None or ln.bias is None:
                raise OccAmdUnsupported("linear: LayerNorm must be affine over the N outputs")
            g, b, eps = ln.weight, ln.bias, ln.eps
        else:
            g, b, eps = ln
        _need_cuda_f32("ln_gamma", g)
        _need_cuda_f32("ln_beta", b)
    if act not in (None, 'relu'):
        raise OccAmdError("linear: act must be None or 'relu'")
    if not weight.is_contiguous():
        raise OccAmdError("linear: weight must be contiguous")
    wdev = linear_pack_weight_bf16x3(weight) if precision == "bf16x3" and (K1 + K2) % 16 == 0 else weight
    out = torch.empty(a.shape[:-1] + (N,), dtype=torch.float32, device=a.device)
    fn = _lib.lib().occ_linear_f32 if wdev is weight else _lib.lib().occ_linear_bf16x3_f32
    _launch(fn, a.device, "linear", a_, lda1, K1, a2, a2_add, lda2, K2, wdev, bias, 1 if act == 'relu' else 0, residual, ldres,
            g, b, float(eps), out, N, M, N, timing='linear', flops=2.0 * M * N * (K1 + K2))
    if g is not None:
        _attach_ln_bound(out, g, b)
    return out


# ---- row-local Linear chains (csrc/linear_chain_x3.hip) ---------------------------------------------------------------
# OCC_LINEAR_CHAIN=0 keeps the encoder on one launch per Linear (the round-3 path); the chain kernels need
# embed_dims = 256 and the bf16x3 precision mode
LINEAR_CHAIN = os.environ.get("OCC_LINEAR_CHAIN", "1") != "0"
_CHAIN_PACKS = DerivedCache("linear chain packs", 128, register=True)   # stage weights ("w") / biases ("b") -> packed buffer


def linear_chain_pack(weights):
    """[(N_i, K_i) float32 weights in consumption order] -> one int16 buffer: every weight packed by
    occ_linear_chain_pack_bf16x3 (256-row groups, 16 KB per k-step, zero rows beyond N), concatenated.  Cached on the
    weights' identities."""
    def build():
        lib = _lib.lib()
        sizes = []
        for w in weights:
            _need_cuda_f32("weight", w)
            if w.dim() != 2 or w.shape[1] % 16:
                raise OccAmdUnsupported("linear_chain_pack: weights must be (N, K) with K % 16 == 0")
            sizes.append(int(lib.occ_linear_chain_packed_bytes(w.shape[0], w.shape[1])) // 2)
        packed = torch.empty(sum(sizes), dtype=torch.int16, device=weights[0].device)
        off = 0
        for w, n in zip(weights, sizes):
            _launch(lib.occ_linear_chain_pack_bf16x3, packed.device, "linear_chain_pack_bf16x3", w, packed[off:], w.shape[0],
                    w.shape[1])
            off += n
        return packed
    return _CHAIN_PACKS.get(weights, build, ("w",))


def _chain_bias(parts, device):
    """[(bias tensor or None, padded length)] -> one float32 vector (zeros where a bias is None / beyond its length)."""
    def build():
        out = torch.zeros(sum(n for _, n in parts), dtype=torch.float32, device=device)
        off = 0
        for b, n in parts:
            if b is not None:
                _need_cuda_f32("bias", b)
                out[off:off + b.numel()] = b.detach().reshape(-1)
            off += n
        return out
    return _CHAIN_PACKS.get([b for b, _ in parts], build, ("b", device) + tuple(n for _, n in parts))


def _ln_params(ln, n=256):
    if isinstance(ln, torch.nn.LayerNorm):
        if tuple(ln.normalized_shape) != (n,) or ln.weight is None or ln.bias is None:
            raise OccAmdUnsupported("linear chain: LayerNorm must be affine over the 256 outputs")
        g, b, eps = ln.weight, ln.bias, ln.eps
    else:
        g, b, eps = ln
    _need_cuda_f32("ln_gamma", g)
    _need_cuda_f32("ln_beta", b)
    if g.numel() != n or b.numel() != n:
        raise OccAmdUnsupported("linear chain: LayerNorm must span the 256 outputs")
    return g, b, float(eps)


def _chain_rows(name, t):
    t_, M, K, ld = _rows2d(name, t)
    if K != 256:
        raise OccAmdUnsupported(f"linear chain: {name} must have 256 columns (embed_dims = 256), got {K}")
    return t_, M, ld


def linear_ln_chain(a, residual, w1, b1, ln, w2, b2, act2=None):
    """Program A of csrc/linear_chain_x3.hip in ONE launch:  y = LayerNorm(a @ w1^T + b1 + residual),
    z = act2(y @ w2^T + b2).  a, residual (…, 256) float32 device tensors; w1 (256, 256); w2 (n2, 256) with
    n2 % 32 == 0; ln = nn.LayerNorm(256) or (gamma, beta, eps); act2 None | 'relu'.  -> (y (…, 256), z (…, n2)).
    Raises OccAmdUnsupported for other shapes (the caller keeps occ `linear`)."""
    if LINEAR_PRECISION != "bf16x3":
        raise OccAmdUnsupported("linear chain: bf16x3 precision mode only")
    a_, M, lda = _chain_rows("a", a)
    r_, Mr, ldres = _chain_rows("residual", residual)
    if Mr != M:
        raise OccAmdError("linear_ln_chain: residual differs in rows")
    if tuple(w1.shape) != (256, 256) or w2.dim() != 2 or w2.shape[1] != 256 or w2.shape[0] % 32:
        raise OccAmdUnsupported("linear_ln_chain: w1 must be (256, 256) and w2 (n2 % 32 == 0, 256)")
    if act2 not in (None, 'relu'):
        raise OccAmdError("linear_ln_chain: act2 must be None or 'relu'")
    g, b, eps = _ln_params(ln)
    n2 = w2.shape[0]
    wp = linear_chain_pack([w1, w2])
    bias = _chain_bias([(b1, 256), (b2, (n2 + 255) // 256 * 256)], a.device)
    y = torch.empty(a.shape[:-1] + (256,), dtype=torch.float32, device=a.device)
    z = torch.empty(a.shape[:-1] + (n2,), dtype=torch.float32, device=a.device)
    _launch(_lib.lib().occ_linear_ln_chain_bf16x3_f32, a.device, "linear_ln_chain", a_, lda, r_, ldres, wp, bias, g, b, eps, y,
            256, z, n2, n2, 1 if act2 == 'relu' else 0, M, timing='linear', flops=2.0 * M * 256 * (256 + n2))
    _attach_ln_bound(y, g, b)
    return y, z


def _chain_out(name, t, M, ncols):
    """caller-provided output rows (a row band of a larger buffer): -> leading dimension"""
    _, Mo, _, ld = _rows2d(name, t, ncols)
    if Mo != M:
        raise OccAmdError(f"linear chain: {name} differs in rows")
    return ld


def encoder_ffn_chain(a, residual, wo, bo, ln1, w1, b1, w2, b2, ln2, tail=None, out=None):
    """Program B of csrc/linear_chain_x3.hip in ONE launch:
        x2 = LayerNorm1(a @ wo^T + bo + residual);  y = LayerNorm2(relu(x2 @ w1^T + b1) @ w2^T + b2 + x2)
    and, with tail = (wq (nq, 256), q_term (…, nq) or None, wv (256, 256), bv):  zq = y @ wq^T + q_term,
    zv = y @ wv^T + bv.  a, residual (…, 256); wo (256, 256); w1 (512, 256); w2 (256, 512).
    -> (y, zq, zv)  (zq = zv = None without a tail).  Raises OccAmdUnsupported for other shapes.
    out = (y, zq, zv) caller-provided result rows (zq / zv None without a tail), e.g. row bands of full-size buffers."""
    if LINEAR_PRECISION != "bf16x3":
        raise OccAmdUnsupported("linear chain: bf16x3 precision mode only")
    a_, M, lda = _chain_rows("a", a)
    r_, Mr, ldres = _chain_rows("residual", residual)
    if Mr != M:
        raise OccAmdError("encoder_ffn_chain: residual differs in rows")
    if tuple(wo.shape) != (256, 256) or tuple(w1.shape) != (512, 256) or tuple(w2.shape) != (256, 512):
        raise OccAmdUnsupported("encoder_ffn_chain: needs output_proj (256, 256) and a 256 -> 512 -> 256 FFN")
    g1, be1, eps1 = _ln_params(ln1)
    g2, be2, eps2 = _ln_params(ln2)
    weights = [wo, w1, w2]
    biases = [(bo, 256), (b1, 512), (b2, 256)]
    zq = zv = q_term = None
    nq, ldq = 0, 0
    if tail is not None:
        wq, q_term, wv, bv = tail
        nq = wq.shape[0]
        if wq.dim() != 2 or wq.shape[1] != 256 or nq > 256 or nq % 64 or tuple(wv.shape) != (256, 256):
            raise OccAmdUnsupported("encoder_ffn_chain: tail needs wq (nq <= 256, nq % 64 == 0, 256) and wv (256, 256)")
        if q_term is not None:
            _, Mq, _, ldq = _rows2d("q_term", q_term, nq)
            if Mq != M:
                raise OccAmdError("encoder_ffn_chain: q_term differs in rows")
        weights += [wq, wv]
        biases += [(None, 256), (bv, 256)]
        if out is None:
            zq = torch.empty(a.shape[:-1] + (nq,), dtype=torch.float32, device=a.device)
            zv = torch.empty(a.shape[:-1] + (256,), dtype=torch.float32, device=a.device)
    wp = linear_chain_pack(weights)
    bias = _chain_bias(biases, a.device)
    ldy, ldzq, ldzv = 256, nq, 256
    if out is None:
        y = torch.empty(a.shape[:-1] + (256,), dtype=torch.float32, device=a.device)
    else:
        y = out[0]
        ldy = _chain_out("out y", y, M, 256)
        if tail is not None:
            zq, zv = out[1], out[2]
            ldzq, ldzv = _chain_out("out zq", zq, M, nq), _chain_out("out zv", zv, M, 256)
    _launch(_lib.lib().occ_encoder_ffn_chain_bf16x3_f32, a.device, "encoder_ffn_chain", a_, lda, r_, ldres, wp, bias, g1, be1,
            eps1, g2, be2, eps2, y, ldy, q_term, ldq, zq, ldzq, nq, zv, ldzv, M, timing='linear',
            flops=2.0 * M * 256 * (256 + 512 + 512 + (nq + 256 if tail is not None else 0)))
    _attach_ln_bound(y, g2, be2)
    return y, zq, zv


def linear_pair_chain(a, wq, q_term, wv, bv):
    """Program C of csrc/linear_chain_x3.hip: zq = a @ wq^T (+ q_term), zv = a @ wv^T + bv in ONE launch (the rows are
    read once).  a (…, 256); wq (nq <= 256, nq % 64 == 0, 256); wv (256, 256).  -> (zq, zv)."""
    if LINEAR_PRECISION != "bf16x3":
        raise OccAmdUnsupported("linear chain: bf16x3 precision mode only")
    a_, M, lda = _chain_rows("a", a)
    nq = wq.shape[0]
    if wq.dim() != 2 or wq.shape[1] != 256 or nq > 256 or nq % 64 or tuple(wv.shape) != (256, 256):
        raise OccAmdUnsupported("linear_pair_chain: needs wq (nq <= 256, nq % 64 == 0, 256) and wv (256, 256)")
    ldq = 0
    if q_term is not None:
        _, Mq, _, ldq = _rows2d("q_term", q_term, nq)
        if Mq != M:
            raise OccAmdError("linear_pair_chain: q_term differs in rows")
    wp = linear_chain_pack([wq, wv])
    bias = _chain_bias([(None, 256), (bv, 256)], a.device)
    zq = torch.empty(a.shape[:-1] + (nq,), dtype=torch.float32, device=a.device)
    zv = torch.empty(a.shape[:-1] + (256,), dtype=torch.float32, device=a.device)
    _launch(_lib.lib().occ_linear_pair_chain_bf16x3_f32, a.device, "linear_pair_chain", a_, lda, wp, bias, q_term, ldq, zq, nq,
            nq, zv, 256, M, timing='linear', flops=2.0 * M * 256 * (nq + 256))
    return zq, zv


def linear_wgrad(dy, x, with_bias=True):
    """Weight / bias gradient of out = x @ W^T + b on the bf16x3 matrix-core kernel (csrc/linear_wgrad.hip):
    dW (N, K) = dy^T @ x, db (N) = dy.sum(rows).  dy (…, N), x (…, K) float32 device tensors with the same leading
    shape and unit column stride.  Deterministic (chunked reduction, fixed order)."""
    def rows(name, t):          # dword loads: any row stride / alignment, unit column stride
        _need_cuda_f32(name, t, contiguous=False)
        if t.dim() == 2 and t.stride(1) == 1:
            return t, t.shape[0], t.shape[1], t.stride(0)
        if t.is_contiguous():
            return t, t.numel() // t.shape[-1], t.shape[-1], t.shape[-1]
        raise OccAmdError(f"linear_wgrad: {name} must be contiguous or a 2-D row-strided view")
    dy_, M, N, lddy = rows("dy", dy)
    x_, Mx, K, ldx = rows("x", x)
    if Mx != M:
        raise OccAmdError("linear_wgrad: dy and x differ in rows")
    dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if with_bias else None
    lib = _lib.lib()
    nbytes = int(lib.occ_linear_wgrad_workspace_bytes(M, N, K))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dy.device)
    _launch(lib.occ_linear_wgrad_bf16x3_f32, dy.device, "linear_wgrad", dy_, lddy, x_, ldx, dw, db, ws, nbytes, M, N, K,
            timing='linear_wgrad')
    return dw, db


class Conv3dX3Function(torch.autograd.Function):
    """3x3x3 / stride 1 / pad 1 Conv3d (no bias, Cout = 32) with forward AND backward on this library's kernels — the
    training-mode replacement for the decoder's nn.Conv3d (reference transformer_occ.py:106-126; round 3 trained it on
    MIOpen under bf16 autocast, narrower than the reference's fp32):
      forward  occ_conv3d_bn_relu_bf16x3_f32 with scale 1 / shift 0 / no ReLU (BatchNorm and ReLU stay autograd ops);
      dx       the same kernel on the flipped, transposed weight (rows beyond Cin zero: the kernel writes 32 channels);
      dW       occ_conv3d_wgrad_bf16x3_f32 on zero-padded copies of x and dy: in the padded grid a tap is a constant
               row offset, so dW = dy_pad^T @ im2col(x_pad) is ONE launch of the N = 32 wgrad kernel (deterministic).
    x: in_layout 0 (B, Y, X, Z, Cin) or 1 (B, Y*X, Cin*Z) (the lifter view of the BEV embedding); -> (B, Y, X, Z, 32)."""

    @staticmethod
    def forward(ctx, x, weight, Z, Y, X, in_layout):
        cout, cin = weight.shape[:2]
        one = torch.ones(cout, dtype=torch.float32, device=x.device)
        zero = torch.zeros(cout, dtype=torch.float32, device=x.device)
        out = conv3d_bn_relu(x.contiguous(), conv3d_pack_weight(weight.detach().contiguous()), one, zero, Z, Y, X, cin, cout,
                             in_layout, relu=False)
        ctx.save_for_backward(x, weight)
        ctx.geom = (int(Z), int(Y), int(X), int(in_layout))
        return out

    @staticmethod
    def backward(ctx, gout):
        x, weight = ctx.saved_tensors
        Z, Y, X, in_layout = ctx.geom
        gout = gout.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _conv3d_x3_dgrad(gout, weight, x.shape[0], Z, Y, X, in_layout)
        if ctx.needs_input_grad[1]:
            gp = torch.nn.functional.pad(gout, (0, 0, 1, 1, 1, 1, 1, 1)).contiguous()    # (B, Y+2, X+2, Z+2, 32)
            gw = _conv3d_x3_wgrad(gp, x, weight, Z, Y, X, in_layout)
        return gx, gw, None, None, None, None


def _conv3d_x3_dgrad(gout, weight, B, Z, Y, X, in_layout):
    """Data gradient of Conv3dX3Function's convolution: gout (B, Y, X, Z, 32) contiguous -> the gradient in x's layout."""
    cout, cin = weight.shape[:2]
    one = torch.ones(32, dtype=torch.float32, device=gout.device)
    zero = torch.zeros(32, dtype=torch.float32, device=gout.device)
    wt = weight.detach().flip(2, 3, 4).transpose(0, 1)               # (cin, cout, 3, 3, 3): dY -> dX
    parts = []
    for c0 in range(0, cin, 32):                                     # the kernel writes 32 channels per launch
        wg = wt[c0:c0 + 32]
        if wg.shape[0] < 32:
            wg = torch.cat([wg, wg.new_zeros((32 - wg.shape[0],) + tuple(wg.shape[1:]))], 0)
        g32 = conv3d_bn_relu(gout, conv3d_pack_weight(wg.contiguous()), one, zero, Z, Y, X, cout, 32, 0, relu=False)
        parts.append(g32[..., :min(32, cin - c0)])
    gx = parts[0] if len(parts) == 1 else torch.cat(parts, -1)
    return gx.permute(0, 1, 2, 4, 3).reshape(B, Y * X, cin * Z) if in_layout == 1 else gx.contiguous()


def _conv3d_x3_wgrad(gp, x, weight, Z, Y, X, in_layout):
    """Weight gradient of Conv3dX3Function's convolution: gp (B, Y+2, X+2, Z+2, 32) the zero-padded output gradient, x the
    node's input in its own layout (padded here) -> (32, cin, 3, 3, 3)."""
    cout, cin = weight.shape[:2]
    B = x.shape[0]
    xc = x.detach()
    if in_layout == 1:
        xc = xc.view(B, Y, X, cin, Z).permute(0, 1, 2, 4, 3)                # (B, Y, X, Z, cin) view
    xp = torch.nn.functional.pad(xc, (0, 0, 1, 1, 1, 1, 1, 1)).contiguous()      # (B, Y+2, X+2, Z+2, cin)
    lib = _lib.lib()
    nbytes = int(lib.occ_conv3d_wgrad_workspace_bytes(B, Z, Y, X, cin))
    if nbytes <= 0:
        raise OccAmdUnsupported("conv3d wgrad: grid beyond the kernel's 32-bit row range")
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((cout, 27, cin), dtype=torch.float32, device=x.device)
    _launch(lib.occ_conv3d_wgrad_bf16x3_f32, x.device, "conv3d_wgrad", gp, xp, dw, ws, nbytes, B, Z, Y, X, cin,
            timing='conv3d_wgrad')
    return dw.permute(0, 2, 1).reshape(cout, cin, 3, 3, 3)


def conv3d_autograd(x, weight, Z, Y, X, in_layout=0):
    """Differentiable Conv3d(k3, s1, p1, no bias, Cout = 32) on the bf16x3 kernels (Conv3dX3Function)."""
    cout, cin = weight.shape[:2]
    if cout != 32 or not (cin % 16 == 0 or cin == 8) or Z not in (4, 8, 16, 32) or CONV3D_PRECISION != "bf16x3":
        raise OccAmdUnsupported("conv3d_autograd: needs Cout = 32, Cin % 16 == 0 or Cin == 8, Z in {4, 8, 16, 32}")
    return Conv3dX3Function.apply(x, weight, Z, Y, X, in_layout)


def bn3d_relu_train_partial(rows, C, device):
    """Scratch of bn3d_relu_train_stats / bn3d_relu_train_bwd for (rows, C) rows; OccAmdUnsupported outside C = 32,
    rows >= 2, fewer than 2^31 elements."""
    n = int(_lib.lib().occ_bn3d_relu_train_partial_floats(rows, C))
    if n <= 0:
        raise OccAmdUnsupported(f"bn3d_relu_train: rows={rows} C={C}: needs C = 32, rows >= 2, fewer than 2^31 elements")
    return torch.empty(n, dtype=torch.float32, device=device)


def bn3d_relu_train_stats(y, running_mean, running_var, eaf, eps):
    """Batch statistics of y (..., 32) over all leading dimensions (csrc/bn3d_relu_train.hip) -> mean_rstd (2, 32) = mean |
    1 / sqrt(biased var + eps).  running_mean / running_var (both or neither; fp32 device tensors) are updated in place as
    nn.BatchNorm3d does in training, with the exponential average factor eaf."""
    _need_cuda_f32("y", y)
    if (running_mean is None) != (running_var is None):
        raise OccAmdError("bn3d_relu_train_stats: running_mean and running_var come together or not at all")
    C = y.shape[-1]
    for n, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None:
            _need_cuda_f32(n, t)
            if t.numel() != C:
                raise OccAmdError(f"bn3d_relu_train_stats: {n} must have {C} elements")
    rows = y.numel() // C
    partial = bn3d_relu_train_partial(rows, C, y.device)
    mean_rstd = torch.empty((2, C), dtype=torch.float32, device=y.device)
    _launch(_lib.lib().occ_bn3d_relu_train_stats_f32, y.device, "bn3d_relu_train_stats", y, partial, mean_rstd, running_mean,
            running_var, eaf, eps, rows, C, timing='bn3d_relu_train')
    if running_mean is not None:        # written through raw pointers: tell autograd (and every version-keyed cache)
        torch._C._increment_version((running_mean, running_var))
    return mean_rstd


def _bn3d_strides(Z, Y, X, C, xy_major):
    """(batch, y, x) element strides of a (B, Y, X, Z, C) tensor, or of its (B, X, Y, Z, C) arrangement"""
    return (Y * X * Z * C,) + ((Z * C, Y * Z * C) if xy_major else (X * Z * C, Z * C))


def bn3d_relu_train_fwd(y, mean_rstd, gamma, beta, Z, Y, X, out_xy_major=False):
    """relu((y - mean) * rstd * gamma + beta) of y (B, Y, X, Z, 32) -> (B, Y, X, Z, 32), or (B, X, Y, Z, 32) with out_xy_major
    (the reference's permute(0, 4, 3, 2, 1) order, written directly)."""
    for n, t in (("y", y), ("mean_rstd", mean_rstd), ("gamma", gamma), ("beta", beta)):
        _need_cuda_f32(n, t)
    C = y.shape[-1]
    B = y.numel() // (Z * Y * X * C)
    if y.numel() != B * Z * Y * X * C or mean_rstd.numel() != 2 * C or gamma.numel() != C or beta.numel() != C:
        raise OccAmdError("bn3d_relu_train_fwd: inconsistent shapes")
    out = torch.empty((B, X, Y, Z, C) if out_xy_major else (B, Y, X, Z, C), dtype=torch.float32, device=y.device)
    sb, sy, sx = _bn3d_strides(Z, Y, X, C, out_xy_major)
    _launch(_lib.lib().occ_bn3d_relu_train_fwd_f32, y.device, "bn3d_relu_train_fwd", y, mean_rstd, gamma, beta, out, B, Z, Y,
            X, C, sb, sy, sx, timing='bn3d_relu_train')
    return out


def bn3d_relu_train_bwd(grad_out, y, mean_rstd, gamma, beta, Z, Y, X, grad_xy_major=False, want_grad_y=True,
                        want_grad_y_pad=False):
    """Backward of bn3d_relu_train_fwd.  grad_out: contiguous in the forward output's own shape ((B, X, Y, Z, 32) with
    grad_xy_major).  -> (grad_y (B, Y, X, Z, 32) or None, grad_y_pad (B, Y+2, X+2, Z+2, 32) with its zero halo or None,
    dgamma (32), dbeta (32))."""
    for n, t in (("grad_out", grad_out), ("y", y), ("mean_rstd", mean_rstd), ("gamma", gamma), ("beta", beta)):
        _need_cuda_f32(n, t)
    C = y.shape[-1]
    B = y.numel() // (Z * Y * X * C)
    if (y.numel() != B * Z * Y * X * C or grad_out.numel() != y.numel() or mean_rstd.numel() != 2 * C or gamma.numel() != C
            or beta.numel() != C):
        raise OccAmdError("bn3d_relu_train_bwd: inconsistent shapes")
    partial = bn3d_relu_train_partial(B * Z * Y * X, C, y.device)
    ggb = torch.empty((2, C), dtype=torch.float32, device=y.device)
    gy = torch.empty((B, Y, X, Z, C), dtype=torch.float32, device=y.device) if want_grad_y else None
    gp = torch.empty((B, Y + 2, X + 2, Z + 2, C), dtype=torch.float32, device=y.device) if want_grad_y_pad else None
    sb, sy, sx = _bn3d_strides(Z, Y, X, C, grad_xy_major)
    _launch(_lib.lib().occ_bn3d_relu_train_bwd_f32, y.device, "bn3d_relu_train_bwd", grad_out, sb, sy, sx, y, mean_rstd, gamma,
            beta, partial, ggb, gy, gp, B, Z, Y, X, C, timing='bn3d_relu_train')
    return gy, gp, ggb[0], ggb[1]


class Conv3dBNReLUFunction(torch.autograd.Function):
    """One decoder layer in training, Conv3d(k3, s1, p1, no bias, Cout = 32) -> BatchNorm3d (batch statistics) -> ReLU, as ONE
    autograd node (reference: ConvModule, transformer_occ.py:106-126, under ATen autograd).  The convolution, its data and
    weight gradients are Conv3dX3Function's; statistics, normalise + ReLU and their backward are csrc/bn3d_relu_train.hip.  Saves
    the convolution's output y, not the activation: the backward recomputes the ReLU mask from y with the forward's own
    expression, and writes dy both as the contiguous tensor of the data-gradient convolution and as the zero-padded tensor of
    the weight-gradient kernel.  running_mean / running_var (or None, None) are updated in place with the exponential average
    factor eaf.  -> (B, Y, X, Z, 32), or (B, X, Y, Z, 32) with out_xy_major."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, eaf, eps, Z, Y, X, in_layout, out_xy_major):
        cout, cin = weight.shape[:2]
        one = torch.ones(cout, dtype=torch.float32, device=x.device)
        zero = torch.zeros(cout, dtype=torch.float32, device=x.device)
        y = conv3d_bn_relu(x.contiguous(), conv3d_pack_weight(weight.detach().contiguous()), one, zero, Z, Y, X, cin, cout,
                           in_layout, relu=False)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        mean_rstd = bn3d_relu_train_stats(y, running_mean, running_var, eaf, eps)
        out = bn3d_relu_train_fwd(y, mean_rstd, g, b, Z, Y, X, out_xy_major)
        ctx.save_for_backward(x, weight, y, mean_rstd, gamma, beta)
        ctx.geom = (int(Z), int(Y), int(X), int(in_layout), bool(out_xy_major))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, weight, y, mean_rstd, gamma, beta = ctx.saved_tensors
        Z, Y, X, in_layout, xy_major = ctx.geom
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gy, gp, dgamma, dbeta = bn3d_relu_train_bwd(gout.contiguous(), y, mean_rstd, gamma.detach().contiguous(),
                                                    beta.detach().contiguous(), Z, Y, X, grad_xy_major=xy_major,
                                                    want_grad_y=need_x, want_grad_y_pad=need_w)
        gx = _conv3d_x3_dgrad(gy, weight, x.shape[0], Z, Y, X, in_layout) if need_x else None
        gw = _conv3d_x3_wgrad(gp, x, weight, Z, Y, X, in_layout) if need_w else None
        return (gx, gw, dgamma.view(gamma.shape) if ctx.needs_input_grad[2] else None,
                dbeta.view(beta.shape) if ctx.needs_input_grad[3] else None) + (None,) * 9


def conv3d_bn_relu_autograd(x, weight, gamma, beta, running_mean, running_var, eaf, eps, Z, Y, X, in_layout=0,
                            out_xy_major=False):
    """Differentiable Conv3d(k3, s1, p1, no bias, Cout = 32) -> BatchNorm3d(training) -> ReLU (Conv3dBNReLUFunction)."""
    cout, cin = weight.shape[:2]
    if cout != 32 or not (cin % 16 == 0 or cin == 8) or Z not in (4, 8, 16, 32) or CONV3D_PRECISION != "bf16x3":
        raise OccAmdUnsupported("conv3d_bn_relu_autograd: needs Cout = 32, Cin % 16 == 0 or Cin == 8, Z in {4, 8, 16, 32}")
    return Conv3dBNReLUFunction.apply(x, weight, gamma, beta, running_mean, running_var, eaf, eps, Z, Y, X, in_layout,
                                      out_xy_major)


class LinearX3Function(torch.autograd.Function):
    """y = act(x @ W^T + b) with forward AND backward on the bf16x3 kernels: forward = linear(), dx = linear(dy, W^T),
    dW / db = linear_wgrad().  The training-mode replacement for F.linear at the encoder's Linear call sites
    (reference: nn.Linear + ATen autograd; temporal_self_attention.py:197-209, spatial_cross_attention.py:334-341,
    mmcv FFN)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        out = linear(x, weight, bias, act=act, precision='bf16x3')
        ctx.act = act
        ctx.save_for_backward(x, weight, out if act == 'relu' else None)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, weight, out = ctx.saved_tensors
        gout = gout.contiguous()
        if ctx.act == 'relu':
            gout = gout * (out > 0)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wt = weight.t().contiguous()
            wt._occ_no_cache = True                 # a temporary: packed for this call only
            gx = linear(gout, wt, None, precision='bf16x3')
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = linear_wgrad(gout, x, with_bias=ctx.has_bias)
        return gx, gw, gb, None


def rows_gather_sum(x, index):
    """out[b, r] = sum_k x[b, index[r, k]] over the entries with 0 <= index < rows_in (csrc/rows_index.hip).  x (B, rows_in, F)
    float32 contiguous, index (rows_out, K) int64, contiguous, on x's device -> (B, rows_out, F).  An entry outside
    [0, rows_in) contributes nothing: -1 is the padding of the rebatch maps, and an entry >= rows_in is skipped in the same
    way, never read.  A row index that occurs twice in a row of `index` is summed twice."""
    _need_cuda_f32("x", x)
    if x.dim() != 3 or not isinstance(index, torch.Tensor) or index.dim() != 2:
        raise OccAmdError("rows_gather_sum: x must be (B, rows, F), index a contiguous (rows_out, K) int64 device "
                          "tensor")
    _need_cuda_i64("rows_gather_sum: index", index, x.device)
    B, rows_in, F = x.shape
    rows_out, K = index.shape
    out = torch.empty((B, rows_out, F), dtype=torch.float32, device=x.device)
    _launch(_lib.lib().occ_rows_gather_sum_f32, x.device, "rows_gather_sum", x, rows_in * F, index, K, out, B, rows_out,
            rows_in, F, timing='rows_gather_sum')
    return out


class RowsGatherSumFunction(torch.autograd.Function):
    """rows_gather_sum with its gradient expressed as the gather-sum over the INVERSE index (the caller supplies
    both maps; they must be each other's transpose as relations)."""

    @staticmethod
    def forward(ctx, x, index, inverse_index):
        _need_cuda_f32("x", x, contiguous=False)
        if x.dim() != 3 or not isinstance(inverse_index, torch.Tensor) or inverse_index.dim() != 2 \
                or inverse_index.shape[0] != x.shape[1]:
            raise OccAmdError("RowsGatherSumFunction: inverse_index must be (rows_in, K'), one row per row of x")
        _need_cuda_i64("RowsGatherSumFunction: inverse_index", inverse_index, x.device)
        ctx.save_for_backward(inverse_index)
        return rows_gather_sum(x.contiguous(), index)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        (inverse_index,) = ctx.saved_tensors
        return rows_gather_sum(gout.contiguous(), inverse_index), None, None


class SCAPrepFunction(torch.autograd.Function):
    """(loc, attn) of SpatialCrossAttention's training path from the per-query Linear outputs: rebatch + softmax +
    offset normalisation + anchor add as one kernel, and its gradient as one kernel (csrc/sca_prep.hip).
    proj (B, Q, 3*M*L*P) float32, row_to_query (R, 1) / query_to_rows (Q, K) int64 (the maps of
    RowsGatherSumFunction), ref_rb (B, R, Z, 2), spatial_shapes (L, 2) int64 ->
    loc (B, R, M, L, P, 2), attn (B, R, M, L, P)."""

    @staticmethod
    def forward(ctx, proj, row_to_query, query_to_rows, ref_rb, spatial_shapes, M, L, P):
        _need_cuda_f32("proj", proj)
        _need_cuda_f32("ref_rb", ref_rb)
        if proj.dim() != 3 or ref_rb.device != proj.device:
            raise OccAmdError("SCAPrepFunction: proj must be (B, Q, ld), ref_rb on its device")
        for n, t in (("row_to_query", row_to_query), ("query_to_rows", query_to_rows), ("spatial_shapes", spatial_shapes)):
            _need_cuda_i64("SCAPrepFunction: " + n, t, proj.device)
        B, Q, ld = proj.shape
        if row_to_query.dim() != 2 or row_to_query.shape[1] != 1 or query_to_rows.dim() != 2 \
                or query_to_rows.shape[0] != Q or query_to_rows.shape[1] < 1 or tuple(spatial_shapes.shape) != (L, 2):
            raise OccAmdError("SCAPrepFunction: expected row_to_query (R, 1), query_to_rows (Q, K) and spatial_shapes (L, 2)")
        R = row_to_query.shape[0]
        if ref_rb.dim() != 4 or ref_rb.shape[0] != B or ref_rb.shape[1] != R or ref_rb.shape[2] < 1 or ref_rb.shape[3] != 2:
            raise OccAmdError(f"SCAPrepFunction: ref_rb must be ({B}, {R}, Z, 2), got {tuple(ref_rb.shape)}")
        Z = ref_rb.shape[2]
        loc = torch.empty((B, R, M, L, P, 2), dtype=torch.float32, device=proj.device)
        attn = torch.empty((B, R, M, L, P), dtype=torch.float32, device=proj.device)
        _launch(_lib.lib().occ_sca_prep_forward_f32, proj.device, "sca_prep_forward", proj, Q * ld, ld, row_to_query, ref_rb,
                spatial_shapes, loc, attn, B, R, M, L, P, Z, timing='sca_prep')
        ctx.save_for_backward(attn, query_to_rows, spatial_shapes)
        ctx.dims = (B, Q, ld, R, M, L, P)
        return loc, attn

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loc, g_attn):
        attn, query_to_rows, spatial_shapes = ctx.saved_tensors
        B, Q, ld, R, M, L, P = ctx.dims
        g_loc = (torch.zeros_like(attn).unsqueeze(-1).expand(*attn.shape, 2) if g_loc is None else g_loc).contiguous()
        g_attn = (torch.zeros_like(attn) if g_attn is None else g_attn).contiguous()
        dproj = torch.empty((B, Q, ld), dtype=torch.float32, device=attn.device)
        if ld > 3 * M * L * P:
            dproj.zero_()
        _launch(_lib.lib().occ_sca_prep_backward_f32, attn.device, "sca_prep_backward", g_loc, g_attn, attn, query_to_rows,
                query_to_rows.shape[1], spatial_shapes, dproj, ld, B, R, Q, M, L, P, timing='sca_prep_bwd')
        return dproj, None, None, None, None, None, None, None


class LinearWgradFunction(torch.autograd.Function):
    """y = x @ W^T + b for the shapes linear_bf16x3 does not cover (the occupancy heads' 64 -> 17 and 64 -> 2 layers:
    N not a multiple of 16) but whose WEIGHT gradient is the expensive part: 640 000 voxels reduced into a 17 x 64
    matrix is a 1.0-1.5 ms fp32 library GEMM plus a 1.6 ms column reduction for the bias in ATen; linear_wgrad does
    both in one pass.  Forward and dx stay library GEMMs (thin, fast)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, weight = ctx.saved_tensors
        gout = gout.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = gout.matmul(weight)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = linear_wgrad(gout, x if x.is_contiguous() else x.contiguous(), with_bias=ctx.has_bias)
        return gx, gw, gb


TRAIN_LINEAR = os.environ.get("OCC_TRAIN_LINEAR", "x3")      # 'x3' (own kernels) or 'torch' (F.linear + ATen autograd)
TRAIN_WGRAD_ONLY = os.environ.get("OCC_TRAIN_WGRAD_ONLY", "1") != "0"   # LinearWgradFunction for the other shapes


class DropoutAddLayerNormFunction(torch.autograd.Function):
    """y = LayerNorm(dropout(x, p) + residual) as ONE autograd node (csrc/ln_dropout_train.hip): the tail of every attention /
    FFN block of a BEVFormerLayer in training (reference: encoder.py:377-404, spatial_cross_attention.py:173-175,
    temporal_self_attention.py:270-272, mmcv FFN).  One launch forward, one (+ a small fixed-order reduce) backward instead
    of ATen's dropout + add + LayerNorm and masked scale + two LayerNorm kernels + the residual fork's add.  The keep mask is
    a counter-based hash of (seed, element index): never stored, regenerated in backward; the seed comes from torch's CPU
    generator (reproducible under torch.manual_seed, no device sync)."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, p):
        shape = x.shape
        C = shape[-1]
        x2, r2 = x.reshape(-1, C).contiguous(), residual.reshape(-1, C).contiguous()
        rows = x2.shape[0]
        z, y = torch.empty_like(x2), torch.empty_like(x2)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if p > 0 else 0
        _launch(_lib.lib().occ_dropout_add_ln_fwd_f32, x.device, "dropout_add_ln_fwd", x2, r2, weight, bias, eps, p, seed, z,
                y, stats, rows, C)
        ctx.save_for_backward(z, stats, weight)
        ctx.cfg = (float(p), seed, tuple(shape), tuple(residual.shape))
        return y.view(shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        z, stats, weight = ctx.saved_tensors
        p, seed, shape, rshape = ctx.cfg
        rows, C = z.shape
        gy2 = gy.reshape(rows, C).contiguous()
        lib = _lib.lib()
        partial = torch.empty(int(lib.occ_dropout_add_ln_bwd_partial_floats(rows, C)), dtype=torch.float32,
                              device=z.device)
        gres = torch.empty_like(z)
        gx = torch.empty_like(z) if p > 0 else gres
        ggb = torch.empty(2 * C, dtype=torch.float32, device=z.device)
        _launch(lib.occ_dropout_add_ln_bwd_f32, z.device, "dropout_add_ln_bwd", gy2, z, stats, weight, p, seed,
                gx if p > 0 else None, gres, partial, ggb, rows, C)
        return gx.view(shape), gres.view(rshape), ggb[:C], ggb[C:], None, None


def _float4_rows_ok(t):
    """The LayerNorm kernels read their operands as float4: dense rows starting on a 16-byte boundary.  (x and residual are
    made contiguous by the node, and a copy is aligned; a tensor that already is contiguous is passed as it stands.)"""
    return t.is_contiguous() and t.data_ptr() % 16 == 0


def dropout_add_layernorm_ok(x, residual, norm):
    """True when DropoutAddLayerNormFunction covers this site: fp32 rows of 256 columns and an affine LayerNorm over them, all
    on ONE device, gamma / beta dense and 16-byte aligned (an offset view of a flat parameter buffer is not), x / residual
    aligned where the node passes them on without a copy.  False: the site keeps its ATen tail."""
    if not (isinstance(norm, torch.nn.LayerNorm) and norm.elementwise_affine and norm.bias is not None
            and tuple(norm.normalized_shape) == (256,) and x.is_cuda and x.dtype == torch.float32
            and residual.dtype == torch.float32 and x.shape == residual.shape and x.shape[-1] == 256
            and x.numel() < (1 << 32) and norm.weight.dtype == torch.float32 and norm.bias.dtype == torch.float32):
        return False
    if not all(t.device == x.device for t in (residual, norm.weight, norm.bias)):
        return False
    if not (_float4_rows_ok(norm.weight) and _float4_rows_ok(norm.bias)):
        return False
    return all(not t.is_contiguous() or t.data_ptr() % 16 == 0 for t in (x, residual))


def dropout_add_layernorm(x, residual, norm, p, training):
    """LayerNorm(dropout(x) + residual) on the fused training node."""
    return DropoutAddLayerNormFunction.apply(x, residual, norm.weight, norm.bias, float(norm.eps),
                                             float(p) if training else 0.0)


def linear_autograd(x, weight, bias=None, act=None):
    """F.linear(+ReLU) that is differentiable: on a float32 device tensor with supported shapes the forward and the
    backward run on the bf16x3 kernels; shapes the forward kernel does not cover keep the library forward and take
    only the weight/bias gradient kernel (many rows); anything else is F.linear (still on the device: no CPU
    branch here)."""
    dev_ok = (TRAIN_LINEAR == "x3" and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
              and weight.is_contiguous() and torch.is_grad_enabled() and not torch.is_autocast_enabled())
    if dev_ok and weight.shape[1] % 16 == 0 and weight.shape[0] % 16 == 0:
        if not (x.is_contiguous() or (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0)):
            x = x.contiguous()
        return LinearX3Function.apply(x, weight, bias, act)
    if dev_ok and TRAIN_WGRAD_ONLY and act is None and x.numel() // x.shape[-1] >= 4096:
        return LinearWgradFunction.apply(x, weight, bias)
    y = torch.nn.functional.linear(x, weight, bias)
    return torch.relu(y) if act == 'relu' else y


def dvr_render_forward(sigma, origin, points, tindex, grid=None, phase_name="test"):
    """Same call shape as the reference's `dvr.render_forward(sigma, origin, points, tindex, grid,
    phase_name)` (tools/ray_iou/lib/dvr/dvr.cpp:68-72; used at ray_metrics.py:116-123):
    sigma (N, T, Z, Y, X), origin (N, T, 3), points (N, M, >=3) in voxel units, tindex (N, M), all float32
    device tensors; grid = [T, Z, Y, X] (checked against sigma when given).
    -> (pred_dist (N, M), gt_dist (N, M), coord_index (N, M, 3)) float32."""
    for n, t in (("sigma", sigma), ("origin", origin), ("points", points), ("tindex", tindex)):
        _need_cuda_f32(n, t)
    if sigma.dim() != 5 or origin.dim() != 3 or points.dim() != 3 or tindex.dim() != 2:
        raise OccAmdError("dvr_render_forward: expected sigma (N,T,Z,Y,X), origin (N,T,3), points "
                          "(N,M,>=3), tindex (N,M)")
    N, T, Z, Y, X = sigma.shape
    M = points.shape[1]
    if grid is not None and [int(v) for v in grid] != [T, Z, Y, X]:
        raise OccAmdError(f"dvr_render_forward: grid {list(grid)} does not match sigma {[T, Z, Y, X]}")
    if (points.shape[0] != N or tuple(tindex.shape) != (N, M) or origin.shape[0] != N or
            origin.shape[2] != 3 or points.shape[2] < 3):
        raise OccAmdError("dvr_render_forward: inconsistent shapes")
    if phase_name not in ("test", "train"):
        raise OccAmdError(f"UNKNOWN PHASE NAME: {phase_name}")
    dev = sigma.device
    pred = torch.empty((N, M), dtype=torch.float32, device=dev)
    gt = torch.empty((N, M), dtype=torch.float32, device=dev)
    coord = torch.empty((N, M, 3), dtype=torch.float32, device=dev)
    _launch(_lib.lib().occ_dvr_render_forward_f32, dev, "dvr_render_forward", sigma, origin, points, tindex, pred, gt, coord,
            N, T, Z, Y, X, M, points.shape[2], 1 if phase_name == "train" else 0, timing='dvr_render_forward')
    return pred, gt, coord


_DVR_LOSS_CODES = {"l1": 0, "l2": 1, "absrel": 2, "bce": 0}     # "bce" is l1 in the reference too (dvr.cu:676-677)


def dvr_render(sigma, origin, points, tindex, loss_name):
    """Same call shape as the reference's `dvr.render(sigma, origin, points, tindex, loss_name)` (tools/ray_iou/lib/dvr/dvr.cu:
    648-703): sigma (N, T, Z, Y, X) densities, origin (N, T, 3), points (N, M, >=3) in voxel units, tindex (N, M), all float32
    device tensors; loss_name "l1", "l2", "absrel" or "bce" (= l1).
    -> (pred_dist (N, M), gt_dist (N, M), grad_sigma (N, T, Z, Y, X)) float32: the expected depth of every ray, its clamped
    target, and d(sum of the per-ray losses) / d sigma, accumulated with float atomics (last bits vary from run to run).
    Rays that are not rendered (include/occnet_amd_dvr.h: padded rays) keep -1 and add nothing."""
    if loss_name not in _DVR_LOSS_CODES:
        raise OccAmdError(f"UNKNOWN LOSS TYPE: {loss_name}")       # the reference prints this and calls exit(1)
    for n, t in (("sigma", sigma), ("origin", origin), ("points", points), ("tindex", tindex)):
        _need_cuda_f32(n, t)
    if sigma.dim() != 5 or origin.dim() != 3 or points.dim() != 3 or tindex.dim() != 2:
        raise OccAmdError("dvr_render: expected sigma (N,T,Z,Y,X), origin (N,T,3), points (N,M,>=3), tindex (N,M)")
    N, T, Z, Y, X = sigma.shape
    M = points.shape[1]
    if (points.shape[0] != N or tuple(tindex.shape) != (N, M) or tuple(origin.shape) != (N, T, 3) or points.shape[2] < 3):
        raise OccAmdError("dvr_render: inconsistent shapes")
    dev = sigma.device
    if any(t.device != dev for t in (origin, points, tindex)):
        raise OccAmdError("dvr_render: all tensors must be on one device")
    pred = torch.empty((N, M), dtype=torch.float32, device=dev)
    gt = torch.empty((N, M), dtype=torch.float32, device=dev)
    grad = torch.empty_like(sigma)
    _launch(_lib.lib().occ_dvr_render_f32, dev, "dvr_render", sigma, origin, points, tindex, pred, gt, grad,
            N, T, Z, Y, X, M, points.shape[2], _DVR_LOSS_CODES[loss_name], timing='dvr_render')
    return pred, gt, grad


_SEM_DTYPE_CODES = {torch.uint8: 0, torch.int64: 1}
_ORIGIN_DTYPE_CODES = {torch.float32: 0, torch.float64: 1}


# ---- the argument checks shared by the evaluation wrappers (ray metrics, submission rows and score, renderer) ----
def _eval_grid(what, name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise OccAmdError(f"{what}: {name} must be a device (HIP) tensor: the MI355X path has no CPU fallback")
    if t.dtype not in _SEM_DTYPE_CODES or not t.is_contiguous() or t.dim() != 4:
        raise OccAmdError(f"{what}: {name} must be a contiguous (B, X, Y, Z) uint8 or int64 tensor, got {t.dtype} "
                          f"{tuple(t.shape)}")


def _eval_origin_counts(what, origin_counts, B):
    if origin_counts is not None and not (origin_counts.is_cuda and origin_counts.dtype == torch.int32
                                          and origin_counts.is_contiguous() and origin_counts.numel() == B):
        raise OccAmdError(f"{what}: origin_counts must be a contiguous int32 device tensor of B entries")


def _eval_state(what, state, words):
    if not (state.is_cuda and state.dtype == torch.int64 and state.is_contiguous() and state.numel() == words):
        raise OccAmdError(f"{what}: state must be a contiguous int64 device tensor of {words} words")


def _eval_workspace(what, workspace, need, dev):
    """The caller's uint8 device workspace once it is seen to hold `need` bytes, or a fresh one."""
    need = max(need, 256)                                             # Z > 32 answers 0: the call itself reports it
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.numel() >= need):
        raise OccAmdError(f"{what}: workspace must be a uint8 device tensor of >= {need} bytes")
    return workspace


def ray_metrics_state_words(free_id=16):
    """int64 words of the RayIoU / mAVE state for classes 0..free_id (14 per class; layout: include/occnet_amd.h)."""
    n = int(_lib.lib().occ_ray_metrics_state_words(free_id))
    if n <= 0:
        raise OccAmdError(f"ray_metrics_state_words: free_id must be 1..31, got {free_id}")
    return n


def ray_metrics_workspace_bytes(B, X, Y, Z):
    return int(_lib.lib().occ_ray_metrics_workspace_bytes(B, X, Y, Z))


def ray_metrics_accumulate(state, sem_pred, flow_pred, sem_gt, flow_gt, origins, rays, pc_min, voxel_size, free_id=16,
                           origin_counts=None, return_rays=False, workspace=None):
    """Cast `rays` from every lidar origin through the ground-truth and the predicted grid and add the RayIoU / mAVE terms of
    the rays whose ground truth is not free to `state` (int64 device tensor of ray_metrics_state_words(free_id) words), in two
    launches on the current stream: no synchronisation, no copy (csrc/ray_metrics_fused.hip).
    sem_pred / sem_gt (B, X, Y, Z) uint8 or int64, flow_pred / flow_gt (B, X, Y, Z, 2) float32, origins (B, Tmax, 3) float32 in
    ego metres (Tmax <= 8), origin_counts None or (B) int32 DEVICE tensor, rays (R, 3) float32, pc_min = pc_range[:3].
    workspace: None, or a uint8 device tensor of at least ray_metrics_workspace_bytes(B, X, Y, Z) bytes.
    -> None, or with return_rays (rows_pred, rows_gt), each (B, Tmax, R, 4) float32 (label, depth, flow_x, flow_y); rows of
    origins beyond origin_counts stay zero."""
    what = "ray_metrics_accumulate"
    for n, t in (("flow_pred", flow_pred), ("flow_gt", flow_gt), ("origins", origins), ("rays", rays)):
        _need_cuda_f32(n, t)
    _eval_grid(what, "sem_pred", sem_pred)
    _eval_grid(what, "sem_gt", sem_gt)
    _eval_state(what, state, ray_metrics_state_words(free_id))
    if sem_gt.shape != sem_pred.shape or origins.dim() != 3 or rays.dim() != 2:
        raise OccAmdError("ray_metrics_accumulate: expected sem (B,X,Y,Z), flow (B,X,Y,Z,2), origins (B,T,3), rays (R,3)")
    B, X, Y, Z = sem_pred.shape
    Tmax, R = origins.shape[1], rays.shape[0]
    if (tuple(flow_pred.shape) != (B, X, Y, Z, 2) or flow_gt.shape != flow_pred.shape or origins.shape[0] != B
            or origins.shape[2] != 3 or rays.shape[1] != 3):
        raise OccAmdError("ray_metrics_accumulate: inconsistent shapes")
    _eval_origin_counts(what, origin_counts, B)
    dev = sem_pred.device
    workspace = _eval_workspace(what, workspace, ray_metrics_workspace_bytes(B, X, Y, Z), dev)
    rows_pred = rows_gt = None
    if return_rays:
        rows_pred = torch.zeros((B, Tmax, R, 4), dtype=torch.float32, device=dev)
        rows_gt = torch.zeros((B, Tmax, R, 4), dtype=torch.float32, device=dev)
    _launch(_lib.lib().occ_ray_metrics_accumulate, dev, what, sem_pred, _SEM_DTYPE_CODES[sem_pred.dtype], flow_pred, sem_gt,
            _SEM_DTYPE_CODES[sem_gt.dtype], flow_gt, origins, origin_counts, rays, pc_min[0], pc_min[1], pc_min[2], voxel_size,
            free_id, state, rows_pred, rows_gt, workspace, workspace.numel(), B, Tmax, X, Y, Z, R,
            timing='ray_metrics_accumulate')
    return (rows_pred, rows_gt) if return_rays else None


def _align256(n):
    return (int(n) + 255) // 256 * 256


def submission_rays_layout(B, Tmax, R):
    """Byte offsets of the packed submission buffer's sections -> (N, off_cls, off_dist, off_flow, total); N = B * Tmax * R
    rows, every section on a 256-byte boundary (include/occnet_amd.h)."""
    n = int(B) * int(Tmax) * int(R)
    off_dist = _align256(n)
    off_flow = off_dist + _align256(2 * n)
    return n, 0, off_dist, off_flow, off_flow + _align256(4 * n)


def submission_rays_bytes(B, Tmax, R):
    return int(_lib.lib().occ_submission_rays_bytes(B, Tmax, R))


def submission_rays_workspace_bytes(B, X, Y, Z):
    return int(_lib.lib().occ_submission_rays_workspace_bytes(B, X, Y, Z))


def submission_rays_views(packed, B, Tmax, R):
    """(cls int8 (B, Tmax, R), dist float16 (B, Tmax, R), flow float16 (B, Tmax, R, 2)) views into a packed uint8 buffer
    (a device tensor, or the pinned host copy of one)."""
    n, _, off_dist, off_flow, _ = submission_rays_layout(B, Tmax, R)
    cls = packed[:n].view(torch.int8).view(B, Tmax, R)
    dist = packed[off_dist:off_dist + 2 * n].view(torch.float16).view(B, Tmax, R)
    flow = packed[off_flow:off_flow + 4 * n].view(torch.float16).view(B, Tmax, R, 2)
    return cls, dist, flow


def submission_rays(sem_pred, flow_pred, origins, rays, pc_min, voxel_size, free_id=16, origin_counts=None, out=None,
                    workspace=None):
    """Cast `rays` from every lidar origin through the predicted grid and pack class / depth / flow per ray in the types of
    submission.gz (int8 / float16 / float16 x 2), in two launches on the current stream: no synchronisation, no copy
    (csrc/submission_rays.hip).
    sem_pred (B, X, Y, Z) uint8 or int64, flow_pred (B, X, Y, Z, 2) float32, origins (B, Tmax, 3) float32 or float64 in ego
    metres (Tmax <= 8; the conversion to voxel units runs in the origins' type, as process_one_sample's does), origin_counts
    None or (B) int32 DEVICE tensor, rays (R, 3) float32, pc_min = pc_range[:3].
    out: None, or a uint8 device tensor of at least submission_rays_bytes(B, Tmax, R) bytes; workspace: None, or one of at least
    submission_rays_workspace_bytes(B, X, Y, Z) bytes.
    -> (cls, dist, flow): (B, Tmax, R) int8, (B, Tmax, R) float16, (B, Tmax, R, 2) float16 views into the packed buffer; rows
    of origins beyond origin_counts are not written (zero when `out` is None)."""
    what = "submission_rays"
    for n, t in (("flow_pred", flow_pred), ("rays", rays)):
        _need_cuda_f32(n, t)
    _eval_grid(what, "sem_pred", sem_pred)
    if not isinstance(origins, torch.Tensor) or not origins.is_cuda:
        raise OccAmdError("origins must be a device (HIP) tensor: the MI355X path has no CPU fallback")
    if origins.dtype not in _ORIGIN_DTYPE_CODES or not origins.is_contiguous():
        raise OccAmdError(f"origins must be a contiguous float32 or float64 tensor, got {origins.dtype}")
    if origins.dim() != 3 or rays.dim() != 2:
        raise OccAmdError("submission_rays: expected sem (B,X,Y,Z), flow (B,X,Y,Z,2), origins (B,T,3), rays (R,3)")
    B, X, Y, Z = sem_pred.shape
    Tmax, R = origins.shape[1], rays.shape[0]
    if (tuple(flow_pred.shape) != (B, X, Y, Z, 2) or origins.shape[0] != B or origins.shape[2] != 3 or rays.shape[1] != 3):
        raise OccAmdError("submission_rays: inconsistent shapes")
    _eval_origin_counts(what, origin_counts, B)
    dev = sem_pred.device
    workspace = _eval_workspace(what, workspace, submission_rays_workspace_bytes(B, X, Y, Z), dev)
    need_out = max(submission_rays_bytes(B, Tmax, R), 256)            # Tmax = 0 answers 0: the call itself reports it
    if out is None:
        out = torch.zeros(need_out, dtype=torch.uint8, device=dev)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= need_out):
        raise OccAmdError(f"submission_rays: out must be a contiguous uint8 device tensor of >= {need_out} bytes")
    _launch(_lib.lib().occ_submission_rays, dev, what, sem_pred, _SEM_DTYPE_CODES[sem_pred.dtype], flow_pred, origins,
            _ORIGIN_DTYPE_CODES[origins.dtype], origin_counts, rays, pc_min[0], pc_min[1], pc_min[2], voxel_size, free_id, out,
            out.numel(), workspace, workspace.numel(), B, Tmax, X, Y, Z, R, timing='submission_rays')
    return submission_rays_views(out, B, Tmax, R)


def render_workspace_bytes(B, X, Y, Z, diff=False):
    """Bytes of the pillar-mask workspace of render_views / render_bev (both grids with diff); 0 for Z > 32."""
    return int(_lib.lib().occ_render_workspace_bytes(B, X, Y, Z, 1 if diff else 0))


def _render_u8(what, name, t, shape):
    if t is None:
        return
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
            and tuple(t.shape) == tuple(shape)):
        raise OccAmdError(f"{what}: {name} must be a contiguous uint8 device tensor of shape {tuple(shape)}")


def _render_out(what, name, out, want, shape, dtype, dev):
    """One optional output: `want` False -> None; `out` given -> a view of its first elements (it may be larger)."""
    if not want:
        return None
    n = 1
    for s in shape:
        n *= int(s)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype and out.is_contiguous()
            and out.numel() >= n):
        raise OccAmdError(f"{what}: out[{name!r}] must be a contiguous {dtype} device tensor of >= {n} elements")
    return out.reshape(-1)[:n].view(shape)


def render_views(sem, cams, pc_min, voxel_size, size, free_id=16, sem_gt=None, frames=None, palette=None, cat_palette=None,
                 far=100.0, tol=2.0, alpha=160, bg_rgb=0, want=('label', 'depth', 'rgb'), out=None, workspace=None):
    """Pin-hole views of a batch of class grids, in two launches on the current stream: no synchronisation, no copy
    (csrc/occ_render.hip; the per-pixel arithmetic is written out in include/occnet_amd.h).
    sem (B, X, Y, Z) uint8 or int64; cams (B, V, 12) float32 (vis.view_rays); size = (h, w); sem_gt: None, or the ground truth
    as sem -> `label` holds the six agreement categories; frames: None or (B, V, Hs, Ws, 3) uint8; palette (256, 3) uint8 and,
    with sem_gt, cat_palette (6, 3) uint8 — needed when 'rgb' is wanted.  want: which of 'label', 'depth', 'rgb' to produce;
    out: None, or a dict of preallocated contiguous device tensors by those names (each may be larger than needed); workspace:
    None, or a uint8 device tensor of at least render_workspace_bytes(B, X, Y, Z, sem_gt is not None) bytes.
    -> dict of the wanted images: label (B, V, h, w) uint8, depth (B, V, h, w) float32, rgb (B, V, h, w, 3) uint8."""
    what = "render_views"
    _eval_grid(what, "sem", sem)
    if sem_gt is not None:
        _eval_grid(what, "sem_gt", sem_gt)
        if sem_gt.shape != sem.shape:
            raise OccAmdError(f"{what}: sem_gt {tuple(sem_gt.shape)} does not match sem {tuple(sem.shape)}")
    _need_cuda_f32("cams", cams)
    B, X, Y, Z = sem.shape
    if cams.dim() != 3 or cams.shape[0] != B or cams.shape[2] != 12 or not cams.is_contiguous():
        raise OccAmdError(f"{what}: cams must be a contiguous (B, V, 12) tensor, got {tuple(cams.shape)}")
    V = cams.shape[1]
    h, w = int(size[0]), int(size[1])
    want = tuple(want)
    if not want or any(k not in ('label', 'depth', 'rgb') for k in want):
        raise OccAmdError(f"{what}: want must name at least one of 'label', 'depth', 'rgb', got {want}")
    Hs = Ws = 0
    if frames is not None:
        if not isinstance(frames, torch.Tensor) or frames.dim() != 5:
            raise OccAmdError(f"{what}: frames must be a (B, V, Hs, Ws, 3) uint8 device tensor")
        Hs, Ws = int(frames.shape[2]), int(frames.shape[3])
        _render_u8(what, "frames", frames, (B, V, Hs, Ws, 3))
    _render_u8(what, "palette", palette, (256, 3))
    _render_u8(what, "cat_palette", cat_palette, (6, 3))
    dev = sem.device
    out = out or {}
    label = _render_out(what, 'label', out.get('label'), 'label' in want, (B, V, h, w), torch.uint8, dev)
    depth = _render_out(what, 'depth', out.get('depth'), 'depth' in want, (B, V, h, w), torch.float32, dev)
    rgb = _render_out(what, 'rgb', out.get('rgb'), 'rgb' in want, (B, V, h, w, 3), torch.uint8, dev)
    workspace = _eval_workspace(what, workspace, render_workspace_bytes(B, X, Y, Z, sem_gt is not None), dev)
    _launch(_lib.lib().occ_render_views, dev, what, sem, _SEM_DTYPE_CODES[sem.dtype], sem_gt,
            0 if sem_gt is None else _SEM_DTYPE_CODES[sem_gt.dtype], cams, frames, Hs, Ws, palette, cat_palette, pc_min[0],
            pc_min[1], pc_min[2], voxel_size, free_id, far, tol, alpha, bg_rgb, label, depth, rgb, workspace,
            workspace.numel(), B, V, X, Y, Z, h, w, timing='render_views')
    return {k: v for k, v in (('label', label), ('depth', depth), ('rgb', rgb)) if v is not None}


def render_bev(sem, free_id=16, sem_gt=None, palette=None, cat_palette=None, bg_rgb=0, want=('label', 'rgb'), out=None,
               workspace=None):
    """Bird's-eye view of a batch of class grids — the top occupied voxel of every pillar, in grid order — in two launches on
    the current stream (csrc/occ_render.hip).  Arguments as render_views.
    -> dict of the wanted images: label (B, X, Y) uint8 (with sem_gt: the agreement categories), rgb (B, X, Y, 3) uint8."""
    what = "render_bev"
    _eval_grid(what, "sem", sem)
    if sem_gt is not None:
        _eval_grid(what, "sem_gt", sem_gt)
        if sem_gt.shape != sem.shape:
            raise OccAmdError(f"{what}: sem_gt {tuple(sem_gt.shape)} does not match sem {tuple(sem.shape)}")
    B, X, Y, Z = sem.shape
    want = tuple(want)
    if not want or any(k not in ('label', 'rgb') for k in want):
        raise OccAmdError(f"{what}: want must name at least one of 'label', 'rgb', got {want}")
    _render_u8(what, "palette", palette, (256, 3))
    _render_u8(what, "cat_palette", cat_palette, (6, 3))
    dev = sem.device
    out = out or {}
    label = _render_out(what, 'label', out.get('label'), 'label' in want, (B, X, Y), torch.uint8, dev)
    rgb = _render_out(what, 'rgb', out.get('rgb'), 'rgb' in want, (B, X, Y, 3), torch.uint8, dev)
    workspace = _eval_workspace(what, workspace, render_workspace_bytes(B, X, Y, Z, sem_gt is not None), dev)
    _launch(_lib.lib().occ_render_bev, dev, what, sem, _SEM_DTYPE_CODES[sem.dtype], sem_gt,
            0 if sem_gt is None else _SEM_DTYPE_CODES[sem_gt.dtype], palette, cat_palette, free_id, bg_rgb, label, rgb,
            workspace, workspace.numel(), B, X, Y, Z, timing='render_bev')
    return {k: v for k, v in (('label', label), ('rgb', rgb)) if v is not None}


def visibility_workspace_bytes(B, X, Y, Z):
    """Bytes of the workspace of visibility_views (pillar masks + one visibility word per pillar); 0 for Z > 32."""
    return int(_lib.lib().occ_visibility_workspace_bytes(B, X, Y, Z))


def visibility_views(sem, cams, pc_min, voxel_size, size, free_id=16, far=100.0, out=None, workspace=None):
    """The voxels seen by the cameras, in three launches on the current stream: no synchronisation, no copy
    (csrc/visibility.hip; the definition is written out in include/occnet_amd_visibility.h).  A voxel is marked when a pixel ray
    of render_views — same cams, same size = (h, w), same far — passes through it before it is stopped, the first occupied
    voxel included.
    sem (B, X, Y, Z) uint8 or int64; cams (B, V, 12) float32 (vis.view_rays); out: None, or a contiguous uint8 device tensor
    of at least B * X * Y * Z elements (every byte of the mask is written); workspace: None, or a uint8 device tensor of at
    least visibility_workspace_bytes(B, X, Y, Z) bytes, reusable from call to call as it is.
    -> mask (B, X, Y, Z) uint8: 1 seen, 0 not."""
    what = "visibility_views"
    _eval_grid(what, "sem", sem)
    _need_cuda_f32("cams", cams)
    B, X, Y, Z = sem.shape
    if cams.dim() != 3 or cams.shape[0] != B or cams.shape[2] != 12 or not cams.is_contiguous():
        raise OccAmdError(f"{what}: cams must be a contiguous (B, V, 12) tensor, got {tuple(cams.shape)}")
    V = cams.shape[1]
    h, w = int(size[0]), int(size[1])
    dev = sem.device
    mask = _render_out(what, 'mask', out, True, (B, X, Y, Z), torch.uint8, dev)
    workspace = _eval_workspace(what, workspace, visibility_workspace_bytes(B, X, Y, Z), dev)
    for name, t in (("cams", cams), ("out", mask), ("workspace", workspace)):
        if t.device != dev:
            raise OccAmdError(f"{what}: {name} must be on the device of sem ({dev}), got {t.device}")
    _launch(_lib.lib().occ_visibility_views, dev, what, sem, _SEM_DTYPE_CODES[sem.dtype], cams, pc_min[0], pc_min[1],
            pc_min[2], voxel_size, free_id, far, mask, workspace, workspace.numel(), B, V, X, Y, Z, h, w,
            timing='visibility_views')
    return mask


def confusion_state_words(free_id=16):
    """int64 words of the confusion state for classes 0..free_id: (ncls + 1) * ncls, ncls = free_id + 1 (layout:
    include/occnet_amd_visibility.h)."""
    n = int(_lib.lib().occ_confusion_state_words(free_id))
    if n <= 0:
        raise OccAmdError(f"confusion_state_words: free_id must be 1..31, got {free_id}")
    return n


def confusion_accumulate(state, sem_pred, sem_gt, mask=None, free_id=16):
    """Add the confusion counts of two class grids over the voxels `mask` admits (None: all) to `state` (int64 device tensor of
    confusion_state_words(free_id) words), in one launch on the current stream (csrc/visibility.hip).
    sem_pred / sem_gt: contiguous uint8 or int64 device tensors of the same shape; mask: None, or a contiguous bool / uint8
    device tensor of as many elements."""
    what = "confusion_accumulate"
    for name, t in (("sem_pred", sem_pred), ("sem_gt", sem_gt)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise OccAmdError(f"{what}: {name} must be a device (HIP) tensor: the MI355X path has no CPU fallback")
        if t.dtype not in _SEM_DTYPE_CODES or not t.is_contiguous():
            raise OccAmdError(f"{what}: {name} must be a contiguous uint8 or int64 tensor, got {t.dtype}")
    if sem_gt.shape != sem_pred.shape:
        raise OccAmdError(f"{what}: sem_gt {tuple(sem_gt.shape)} does not match sem_pred {tuple(sem_pred.shape)}")
    if mask is not None and not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype in (torch.bool, torch.uint8)
                                 and mask.is_contiguous() and mask.numel() == sem_pred.numel()):
        raise OccAmdError(f"{what}: mask must be a contiguous bool or uint8 device tensor of {sem_pred.numel()} elements")
    if not isinstance(state, torch.Tensor):
        raise TypeError(f"{what}: state must be a torch.Tensor")
    dev = sem_pred.device
    if sem_gt.device != dev or state.device != dev or (mask is not None and mask.device != dev):
        raise OccAmdError(f"{what}: sem_pred, sem_gt, mask and state must be on one device")
    _eval_state(what, state, confusion_state_words(free_id))
    _launch(_lib.lib().occ_confusion_accumulate, dev, what, sem_pred, _SEM_DTYPE_CODES[sem_pred.dtype], sem_gt,
            _SEM_DTYPE_CODES[sem_gt.dtype], mask, free_id, state, sem_pred.numel(), timing='confusion_accumulate')


def submission_score_state_words(free_id=16):
    """int64 words of the submission score's state for classes 0..free_id (17 per class; layout: include/occnet_amd.h)."""
    n = int(_lib.lib().occ_submission_score_state_words(free_id))
    if n <= 0:
        raise OccAmdError(f"submission_score_state_words: free_id must be 1..31, got {free_id}")
    return n


def submission_score_workspace_bytes(B):
    return int(_lib.lib().occ_submission_score_workspace_bytes(B))


def _score_side(name, side, B, stride):
    """One side of submission_score_accumulate -> (format code, cls / rows, dist, flow): a float32 (B, stride, 4) tensor of
    rows, or the (cls int8, dist float16, flow float16) sections of a packed buffer with B * stride rows each."""
    if isinstance(side, torch.Tensor):
        if not (side.is_cuda and side.dtype == torch.float32 and side.is_contiguous()):
            raise OccAmdError(f"{name} rows must be a contiguous float32 device (HIP) tensor: the MI355X path has no CPU "
                              "fallback")
        if side.numel() != B * stride * 4 or side.shape[-1] != 4:
            raise OccAmdError(f"submission_score_accumulate: {name} rows must hold B * stride = {B * stride} rows of 4")
        return 1, side, None, None
    cls, dist, flow = side
    for t, dt, per in ((cls, torch.int8, 1), (dist, torch.float16, 1), (flow, torch.float16, 2)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise OccAmdError(f"{name} sections must be contiguous int8 / float16 / float16 device (HIP) tensors: the MI355X "
                              "path has no CPU fallback")
        if t.numel() != B * stride * per:
            raise OccAmdError(f"submission_score_accumulate: {name} sections must hold B * stride = {B * stride} rows")
    return 0, cls, dist, flow


def submission_score_accumulate(state, pred, gt, counts, stride, free_id=16, workspace=None, max_chunks=0):
    """Add the terms of tools/ray_iou/metric.py:calc_metrics for B samples of per-ray rows to `state` (int64 device tensor of
    submission_score_state_words(free_id) words), in two launches on the current stream: no synchronisation, no copy
    (csrc/submission_score.hip).
    pred / gt: each either a float32 (B, stride, 4) tensor of rows [class, dist, flow_x, flow_y], or the tuple (cls int8, dist
    float16, flow float16) of a packed buffer's sections with B * stride rows (ext.submission_rays_views); counts (B) int32
    DEVICE tensor: sample b owns rows [b * stride, b * stride + counts[b]).
    workspace: None, or a uint8 device tensor of at least submission_score_workspace_bytes(B) bytes (uninitialised);
    max_chunks: 0, or a cap on the blocks per sample (the state does not depend on it)."""
    if not (isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous()):
        raise OccAmdError("submission_score_accumulate: counts must be a contiguous int32 device tensor of B entries")
    B, stride = int(counts.numel()), int(stride)
    if B < 1 or stride < 1:
        raise OccAmdError(f"submission_score_accumulate: bad dimension (B={B} stride={stride})")
    _eval_state("submission_score_accumulate", state, submission_score_state_words(free_id))
    pf, pc, pd, pfl = _score_side("pred", pred, B, stride)
    gf, gc, gd, gfl = _score_side("gt", gt, B, stride)
    dev = state.device
    workspace = _eval_workspace("submission_score_accumulate", workspace, submission_score_workspace_bytes(B), dev)
    _launch(_lib.lib().occ_submission_score_accumulate, dev, "submission_score_accumulate", pf, pc, pd, pfl, gf, gc, gd, gfl,
            counts, free_id, state, workspace, workspace.numel(), B, stride, max_chunks, timing='submission_score_accumulate')


_HEADS_LOSS_PARAMS = ("w1_occ", "b1_occ", "w2_occ", "b2_occ", "w1_flow", "b1_flow", "w2_flow", "b2_flow")


def _heads_loss_check(what, feat, params, labels, flow_gt, mask, class_weight, reduction):
    """Device, dtype, contiguity, shape and alignment conditions of the fused heads + loss node -> (n_rows, num_classes);
    OccAmdUnsupported otherwise (the caller then runs the module chain)."""
    def bad(msg):
        raise OccAmdUnsupported(f"{what}: {msg}")
    for n, t in (("feat", feat), ("flow_gt", flow_gt)) + tuple(zip(_HEADS_LOSS_PARAMS, params)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            bad(f"{n} must be a contiguous float32 device tensor")
    if reduction not in ('mean', 'sum'):
        bad(f"reduction {reduction!r} is not covered (mean, sum)")
    w1o, b1o, w2o, b2o, w1f, b1f, w2f, b2f = params
    C = feat.shape[-1] if feat.dim() else 0
    ncls = w2o.shape[0] if w2o.dim() == 2 else 0
    if (C != 32 or tuple(w1o.shape) != (64, 32) or tuple(w1f.shape) != (64, 32) or ncls < 1 or ncls > 30
            or tuple(w2o.shape) != (ncls, 64) or tuple(w2f.shape) != (2, 64) or b1o.numel() != 64 or b1f.numel() != 64
            or b2o.numel() != ncls or b2f.numel() != 2):
        bad("needs C = 32, hidden = 64 and num_classes <= 30")
    n_rows = feat.numel() // 32
    if n_rows < 1:
        bad("no rows")
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype in _SEM_DTYPE_CODES
            and labels.is_contiguous() and labels.numel() == n_rows):
        bad("labels must be a contiguous uint8 or int64 device tensor with one entry per row")
    if flow_gt.numel() != 2 * n_rows:
        bad("flow_gt must hold (n_rows, 2) values")
    if mask is not None and not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype in (torch.bool, torch.uint8)
                                 and mask.is_contiguous() and mask.numel() == n_rows):
        bad("mask must be a contiguous bool or uint8 device tensor with one entry per row")
    if class_weight is not None and not (isinstance(class_weight, torch.Tensor) and class_weight.is_cuda
                                         and class_weight.dtype == torch.float32 and class_weight.is_contiguous()
                                         and class_weight.numel() == ncls):
        bad("class_weight must be a contiguous float32 device tensor of num_classes entries")
    if feat.data_ptr() % 16 or flow_gt.data_ptr() % 8:
        bad("feat must be 16-byte aligned, flow_gt 8-byte aligned")
    return n_rows, ncls


def _heads_loss_workspace(n_rows, ncls, max_blocks, device):
    nbytes = int(_lib.lib().occ_heads_loss_workspace_bytes(n_rows, ncls, max_blocks))
    if nbytes <= 0:
        raise OccAmdUnsupported(f"heads_loss: no kernel for num_classes={ncls}, max_blocks={max_blocks}")
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device), nbytes


def heads_loss_forward(feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, labels, flow_gt,
                       mask=None, class_weight=None, ignore_index=-100, reduction='mean', max_blocks=0):
    """Both decoder heads + CrossEntropyLoss + L1Loss in one launch and a one-wave finalise (csrc/occ_heads_loss.hip):
    feat (..., 32), labels (...) uint8 / int64, flow_gt (..., 2), mask None or (...) bool, class_weight None or (ncls)
    -> 3 device floats: loss_occ, loss_flow (both WITHOUT loss_weight), the occ denominator."""
    params = (w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow)
    n_rows, ncls = _heads_loss_check("heads_loss_forward", feat, params, labels, flow_gt, mask, class_weight, reduction)
    ws, nbytes = _heads_loss_workspace(n_rows, ncls, max_blocks, feat.device)
    losses = torch.empty(3, dtype=torch.float32, device=feat.device)
    _launch(_lib.lib().occ_heads_loss_fwd_f32, feat.device, "heads_loss_forward", feat, *params, labels,
            _SEM_DTYPE_CODES[labels.dtype], flow_gt, mask, class_weight, int(ignore_index), 1 if reduction == 'mean' else 0,
            losses, ws, nbytes, n_rows, 32, 64, ncls, max_blocks, timing='heads_loss_fwd')
    return losses


def heads_loss_backward(feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, labels, flow_gt,
                        mask, class_weight, ignore_index, reduction, grad_losses, occ_denom, need_feat=True,
                        need_params=(True,) * 8, max_blocks=0):
    """Gradients of heads_loss_forward: grad_losses (2) and occ_denom (1) device floats (no host read) ->
    (dfeat or None, [the eight parameter gradients, None where need_params is False]).  One launch + a small reduce."""
    params = (w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow)
    n_rows, ncls = _heads_loss_check("heads_loss_backward", feat, params, labels, flow_gt, mask, class_weight, reduction)
    for n, t, k in (("grad_losses", grad_losses, 2), ("occ_denom", occ_denom, 1)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == k):
            raise OccAmdUnsupported(f"heads_loss_backward: {n} must be {k} contiguous float32 device value(s)")
    ws, nbytes = _heads_loss_workspace(n_rows, ncls, max_blocks, feat.device)
    dfeat = torch.empty_like(feat) if need_feat else None
    grads = [torch.empty_like(p) if need else None for p, need in zip(params, need_params)]
    _launch(_lib.lib().occ_heads_loss_bwd_f32, feat.device, "heads_loss_backward", feat, *params, labels,
            _SEM_DTYPE_CODES[labels.dtype], flow_gt, mask, class_weight, int(ignore_index), 1 if reduction == 'mean' else 0,
            grad_losses, occ_denom, dfeat, *grads, ws, nbytes, n_rows, 32, 64, ncls, max_blocks,
            timing='heads_loss_bwd')
    return dfeat, grads


class OccHeadsLossFunction(torch.autograd.Function):
    """(loss_occ, loss_flow) = CrossEntropyLoss / L1Loss of the two decoder heads applied to feat, as ONE autograd node
    (csrc/occ_heads_loss.hip): the training-mode replacement for predicter / flow_predicter (reference
    transformer_occ.py:132-141,318-319) followed by BEVFormerOccHead.loss_single (bevformer_occ_head.py:163-196).  Saves its
    tensor inputs and the occ denominator, nothing else: the backward recomputes the hidden layers tile by tile.  The losses
    carry no loss_weight.  A label outside [0, num_classes) other than ignore_index contributes nothing (torch asserts)."""

    @staticmethod
    def forward(ctx, feat, w1o, b1o, w2o, b2o, w1f, b1f, w2f, b2f, labels, flow_gt, mask, class_weight, ignore_index,
                reduction, max_blocks=0):
        losses = heads_loss_forward(feat, w1o, b1o, w2o, b2o, w1f, b1f, w2f, b2f, labels, flow_gt, mask, class_weight,
                                    ignore_index, reduction, max_blocks)
        ctx.save_for_backward(feat, w1o, b1o, w2o, b2o, w1f, b1f, w2f, b2f, labels, flow_gt, mask, class_weight, losses[2:])
        ctx.args = (int(ignore_index), reduction, int(max_blocks))
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_occ, g_flow):
        *ins, denom = ctx.saved_tensors
        ignore_index, reduction, max_blocks = ctx.args
        dev = ins[0].device
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        g = torch.stack([zero if t is None else t.to(device=dev, dtype=torch.float32).reshape(()) for t in (g_occ, g_flow)])
        need = ctx.needs_input_grad
        dfeat, grads = heads_loss_backward(*ins, ignore_index, reduction, g, denom, need_feat=need[0],
                                           need_params=tuple(need[1:9]), max_blocks=max_blocks)
        return (dfeat, *grads, None, None, None, None, None, None, None)


def heads_loss(feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, labels, flow_gt, mask=None,
               class_weight=None, ignore_index=-100, reduction='mean', max_blocks=0):
    """Differentiable (loss_occ, loss_flow) of the decoder features (OccHeadsLossFunction); max_blocks caps the grids."""
    return OccHeadsLossFunction.apply(feat, w1_occ, b1_occ, w2_occ, b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, labels,
                                      flow_gt, mask, class_weight, ignore_index, reduction, max_blocks)


def _is_cl_bf16(t):
    """True for a channels_last bfloat16 (N, C, H, W) device tensor."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4
            and t.is_contiguous(memory_format=torch.channels_last))


def _need_cl_bf16(what, name, t):
    if not _is_cl_bf16(t):
        raise OccAmdUnsupported(f"{what}: {name} must be a channels_last bfloat16 device tensor")


def bias_act_nhwc_(x, bias, residual=None, relu=True):
    """In place x = relu?(x + bias[c] (+ residual)) on a channels_last bf16 (N, C, H, W) tensor (memory
    order N, H, W, C).  bias (C) float32.  Returns x."""
    _need_cl_bf16("bias_act_nhwc_", "x", x)
    _need_cuda_f32("bias", bias)
    N, C, H, W = x.shape
    if bias.numel() != C:
        raise OccAmdError("bias_act_nhwc_: bias must have C entries")
    if residual is not None and not (_is_cl_bf16(residual) and residual.shape == x.shape):
        raise OccAmdUnsupported("bias_act_nhwc_: residual must match x (channels_last bfloat16)")
    _launch(_lib.lib().occ_bias_act_nhwc_bf16, x.device, "bias_act_nhwc_", x, bias, residual, N * H * W, C, 1 if relu else 0)
    return x


def bias_act_bwd_nhwc(grad_y, y=None, relu=True):
    """Backward of bias_act_nhwc_ in one pass: -> (g, bias_grad) with g = grad_y * (y > 0) (grad_y itself when not relu) and
    bias_grad (C) float32 = sum of g over N, H, W.  grad_y / y: channels_last bfloat16 (N, C, H, W) device tensors."""
    if not _is_cl_bf16(grad_y) or (relu and not (_is_cl_bf16(y) and y.shape == grad_y.shape)):
        raise OccAmdUnsupported("bias_act_bwd_nhwc: grad_y / y must be matching channels_last bfloat16 device tensors")
    N, C, H, W = grad_y.shape
    rows = N * H * W
    nfl = _lib.lib().occ_bias_act_bwd_partial_floats(rows, C)
    if nfl <= 0:
        raise OccAmdUnsupported(f"bias_act_bwd_nhwc: no kernel for C={C}")
    partial = torch.empty(nfl, dtype=torch.float32, device=grad_y.device)
    bias_grad = torch.empty(C, dtype=torch.float32, device=grad_y.device)
    g = torch.empty_like(grad_y) if relu else grad_y
    _launch(_lib.lib().occ_bias_act_bwd_nhwc_bf16, grad_y.device, "bias_act_bwd_nhwc", grad_y, y if relu else None,
            g if relu else None, partial, bias_grad, rows, C, 1 if relu else 0)
    return g, bias_grad


def conv_bn_fold_fwd(weight, gamma, beta, rstd, mean_rstd):
    """Eval-mode BatchNorm folded into a convolution weight, one launch: -> (w_folded fp32 (O, I, kh, kw) contiguous,
    w16 = the same as bfloat16 channels_last, bias (O) fp32)."""
    for n, t in (("weight", weight), ("gamma", gamma), ("beta", beta), ("rstd", rstd), ("mean_rstd", mean_rstd)):
        _need_cuda_f32(n, t)
    O, I, KH, KW = weight.shape
    wf = torch.empty_like(weight, memory_format=torch.contiguous_format)
    w16 = torch.empty((O, I, KH, KW), dtype=torch.bfloat16, device=weight.device, memory_format=torch.channels_last)
    b = torch.empty(O, dtype=torch.float32, device=weight.device)
    _launch(_lib.lib().occ_conv_bn_fold_fwd_f32, weight.device, "conv_bn_fold_fwd", weight, gamma, beta, rstd, mean_rstd, wf,
            w16, b, O, I, KH, KW)
    return wf, w16, b


def conv_bn_fold_bwd(grad_w16, weight, gamma, rstd, mean_rstd, grad_bias):
    """Chain rule of conv_bn_fold_fwd, one launch: grad_w16 (O, I, kh, kw) bfloat16 (any strides) -> (grad_weight fp32,
    grad_gamma fp32); grad_beta is grad_bias."""
    if not (grad_w16.is_cuda and grad_w16.dtype == torch.bfloat16 and grad_w16.shape == weight.shape):
        raise OccAmdUnsupported("conv_bn_fold_bwd: grad_w16 must be a bfloat16 device tensor of the weight's shape")
    for n, t in (("weight", weight), ("gamma", gamma), ("rstd", rstd), ("mean_rstd", mean_rstd), ("grad_bias", grad_bias)):
        _need_cuda_f32(n, t)
    O, I, KH, KW = weight.shape
    dW = torch.empty_like(weight, memory_format=torch.contiguous_format)
    dgamma = torch.empty(O, dtype=torch.float32, device=weight.device)
    so, si, sh, sw = grad_w16.stride()
    _launch(_lib.lib().occ_conv_bn_fold_bwd_f32, weight.device, "conv_bn_fold_bwd", grad_w16, so, si, sh, sw, weight, gamma,
            rstd, mean_rstd, grad_bias, dW, dgamma, O, I, KH, KW)
    return dW, dgamma


def stem_pack_weight(weight):
    """(64, 3, 7, 7) stem weight (BatchNorm folded) -> the fragment-ordered (64, 224) operand of stem_conv7x7_pool:
    column ky*32 + kx*4 + c holds weight[:, c, ky, kx]; the pad columns (kx = 7, c = 3) are zero."""
    if tuple(weight.shape) != (64, 3, 7, 7):
        raise OccAmdUnsupported("stem_pack_weight: expected a (64, 3, 7, 7) weight")
    w2 = torch.zeros(64, 7, 8, 4, dtype=torch.float32, device=weight.device)
    w2[:, :, :7, :3] = weight.float().permute(0, 2, 3, 1)
    return mfma_pack_b_frag(w2.reshape(64, 224))


def stem_conv7x7_pool(x, weight_frag, bias):
    """max_pool2d(relu(conv2d(x, W, stride 2, padding 3) + bias), 3, 2, 1) in one launch.
    x (N, 3, H, W) fp32 contiguous (NCHW); weight_frag from stem_pack_weight; bias (64) fp32
    -> (N, 64, Hp, Wp) channels_last bf16."""
    _need_cuda_f32("x", x)
    _need_cuda_f32("bias", bias)
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise OccAmdUnsupported("stem_conv7x7_pool: x must be a contiguous (N, 3, H, W) fp32 tensor")
    if weight_frag.numel() != 64 * 224 or bias.numel() != 64:
        raise OccAmdError("stem_conv7x7_pool: inconsistent shapes")
    N, _, H, W = x.shape
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.empty((N, 64, Hp, Wp), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    _launch(_lib.lib().occ_stem_conv7x7_pool_f32_bf16, x.device, "stem_conv7x7_pool", x, weight_frag, bias, out, N, H, W,
            timing='bb_stem7x7_pool', flops=2.0 * N * Hc * Wc * 64 * 147)
    return out


def stem_conv7x7_pool_u8(x_u8, weight_frag, bias, mean, std, to_rgb=False, size_divisor=32):
    """The stem fed with RAW camera images: x_u8 (N, Hs, Ws, 3) uint8 HWC on the device.  NormalizeMultiviewImage
    ((x[to_rgb ? 2-c : c] - mean[c]) / std[c]) and PadMultiViewImage (zeros to the next multiple of `size_divisor`;
    reference transform_3d.py:31-45,82-94) are applied while the input tile is staged.
    -> (N, 64, Hp, Wp) channels_last bf16, and the padded (H, W)."""
    if not (x_u8.is_cuda and x_u8.dtype == torch.uint8 and x_u8.dim() == 4 and x_u8.shape[-1] == 3
            and x_u8.is_contiguous()):
        raise OccAmdUnsupported("stem_conv7x7_pool_u8: x must be a contiguous (N, H, W, 3) uint8 device tensor")
    _need_cuda_f32("bias", bias)
    if weight_frag.numel() != 64 * 224 or bias.numel() != 64:
        raise OccAmdError("stem_conv7x7_pool_u8: inconsistent shapes")
    N, Hs, Ws, _ = x_u8.shape
    d = int(size_divisor)
    H, W = (Hs + d - 1) // d * d, (Ws + d - 1) // d * d
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.empty((N, 64, Hp, Wp), dtype=torch.bfloat16, device=x_u8.device, memory_format=torch.channels_last)
    mean_c = (f32 * 3)(*[float(v) for v in mean])
    std_c = (f32 * 3)(*[float(v) for v in std])
    _launch(_lib.lib().occ_stem_conv7x7_pool_u8_bf16, x_u8.device, "stem_conv7x7_pool_u8", x_u8, weight_frag, bias, out, N, Hs,
            Ws, H, W, mean_c, std_c, 1 if to_rgb else 0)
    return out, (H, W)


def train_input_u8(frames_u8, records, mean, std, to_rgb, size_divisor=32, grid_mask=None, out=None):
    """The reference's training input in one launch: frames_u8 (NI, Hs, Ws, 3) uint8 HWC on the device, channels as
    loaded (BGR) -> (NI, 3, H, W) float32, H x W the next multiples of `size_divisor`, the pad area 0.
    PhotoMetricDistortionMultiViewImage with the draws in `records` ((NI, 8) float32, io.sample_photometric /
    io.identity_photometric; a numpy array is uploaded, a device tensor is taken as it is), NormalizeMultiviewImage(mean,
    std, to_rgb), PadMultiViewImage(size_divisor) and GridMask (reference transform_3d.py:141-188, :91, :31-43,
    grid_mask.py:84-124).  grid_mask: None (not applied) or (d, l, st_h, st_w, use_h, use_w, mode) — the draws of
    GridMask.sample_params and the module's use_h / use_w / mode; rotate == 1 and offset == False only.
    out: optional (NI, 3, H, W) float32 contiguous device tensor to write into."""
    return _u8_input("train_input_u8", frames_u8, records, mean, std, to_rgb, None, size_divisor, grid_mask, out)[0]


def input_u8_scaled(frames_u8, records, mean, std, to_rgb, scale, size_divisor=32, grid_mask=None, out=None):
    """train_input_u8 with RandomScaleImageMultiViewImage(scales=[scale]) between normalise and pad, in one launch:
    frames_u8 (NI, Hs, Ws, 3) uint8 -> photometric distortion (records) -> normalise -> bilinear rescale to
    (Hd, Wd) = (int(Hs * scale), int(Ws * scale)) -> pad to the next multiples of `size_divisor` -> GridMask of the padded
    size.  The resize is the project's float32 definition (include/occnet_amd_input.h; io.random_scale_multiview is its host
    twin); scale == 1.0 gives train_input_u8's tensor.  Arguments as train_input_u8's.
    -> ((NI, 3, H, W) float32, (Hd, Wd))."""
    _as_occ_error(check_scale, scale)         # a bad scale is refused before anything else is looked at
    return _u8_input("input_u8_scaled", frames_u8, records, mean, std, to_rgb, scale, size_divisor, grid_mask, out)


def _as_occ_error(fn, *args):
    """fn(*args) of io's scale helpers, their ValueError as this module's error type."""
    try:
        return fn(*args)
    except ValueError as e:
        raise OccAmdError(f"input_u8_scaled: {e}") from None


def _u8_input(what, frames_u8, records, mean, std, to_rgb, scale, size_divisor, grid_mask, out):
    """The checks and the launch of train_input_u8 (scale None) and input_u8_scaled -> (out, (Hd, Wd))."""
    if not (isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda):
        raise OccAmdError(f"{what}: frames must be a device (HIP) tensor: the MI355X path has no CPU fallback")
    if not (frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[-1] == 3
            and frames_u8.is_contiguous()):
        raise OccAmdUnsupported(f"{what}: frames must be a contiguous (NI, Hs, Ws, 3) uint8 device tensor")
    NI, Hs, Ws, _ = frames_u8.shape
    Hd, Wd = (Hs, Ws) if scale is None else _as_occ_error(scaled_size, Hs, Ws, scale)
    if not isinstance(records, torch.Tensor):
        import numpy as np
        records = torch.from_numpy(np.ascontiguousarray(records, dtype=np.float32)).to(frames_u8.device)
    _need_cuda_f32("records", records)
    if tuple(records.shape) != (NI, 8):
        raise OccAmdError(f"{what}: records must be ({NI}, 8), got {tuple(records.shape)}")
    d = int(size_divisor)
    H, W = (Hd + d - 1) // d * d, (Wd + d - 1) // d * d
    if out is None:
        out = torch.empty((NI, 3, H, W), dtype=torch.float32, device=frames_u8.device)
    else:
        _need_cuda_f32("out", out)
        if tuple(out.shape) != (NI, 3, H, W):
            raise OccAmdError(f"{what}: out must be ({NI}, 3, {H}, {W}), got {tuple(out.shape)}")
    mean_c = (f32 * 3)(*[float(v) for v in mean])
    std_c = (f32 * 3)(*[float(v) for v in std])
    gm_c = None
    if grid_mask is not None:
        if len(grid_mask) != 7:
            raise OccAmdError(f"{what}: grid_mask must be (d, l, st_h, st_w, use_h, use_w, mode)")
        gm_c = (i32 * 8)(1, *[int(v) for v in grid_mask])
    tail = (H, W, mean_c, std_c, 1 if to_rgb else 0, gm_c)
    if scale is None:
        _launch(_lib.lib().occ_train_input_u8_f32, frames_u8.device, what, frames_u8, records, out, NI, Hs, Ws, *tail,
                timing=what)
    else:
        _launch(_lib.lib().occ_input_u8_scaled_f32, frames_u8.device, what, frames_u8, records, out, NI, Hs, Ws, Hd, Wd, *tail,
                timing=what)
    return out, (Hd, Wd)


def bias_relu_maxpool_nhwc(y, bias):
    """max_pool2d(relu(y + bias), 3, stride 2, padding 1) in one launch on a channels_last bf16 activation
    (the ResNet stem's tail).  y (N, C, H, W) channels_last bf16 raw convolution output; bias (C) f32."""
    _need_cl_bf16("bias_relu_maxpool_nhwc", "y", y)
    _need_cuda_f32("bias", bias)
    N, C, H, W = y.shape
    if bias.numel() != C:
        raise OccAmdError("bias_relu_maxpool_nhwc: bias must have C entries")
    out = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.bfloat16, device=y.device,
                      memory_format=torch.channels_last)
    _launch(_lib.lib().occ_bias_relu_maxpool_nhwc_bf16, y.device, "bias_relu_maxpool_nhwc", y, bias, out, N, H, W, C)
    return out


def conv1x1_pack_weight(weight2d):
    """(Cout, Cin) weight matrix (any float dtype, on the device) -> bf16 in MFMA B-fragment order (what
    conv1x1_nhwc takes; see mfma_pack_b_frag): a wave reads its operand straight from global memory."""
    cout, cin = weight2d.shape
    if cin % 32 or cout % 32:
        raise OccAmdUnsupported("conv1x1_pack_weight: Cin and Cout must be multiples of 32")
    return mfma_pack_b_frag(weight2d.float().contiguous())


def conv1x1_nhwc(x, weight_frag, bias, residual=None, relu=False, stride=1, residual_upsample2=False, variant=None,
                 _timing='bb_conv1x1'):
    """1x1 convolution + bias (+ residual) (+ ReLU) on a channels_last bf16 activation, one launch.
    x (N, Cin, H, W) channels_last bf16; weight_frag = conv1x1_pack_weight((Cout, Cin) matrix); bias (Cout) f32;
    residual (N, Cout, Ho, Wo) channels_last bf16 or None -> (N, Cout, Ho, Wo) channels_last bf16.
    residual_upsample2: residual is (N, Cout, Ho/2, Wo/2) and is added nearest-upsampled x2 (FPN top-down).
    variant: None = the launcher's choice; an int forces the kernel (occ_conv1x1_nhwc_bf16_variant: 1 = tiled, 2 =
    activation-resident, 22 / 24 = resident with the 64- / 128-row tile); OccAmdUnsupported where the shape has none.
    _timing: the kernel_timing entry the launch is booked under (conv1x1_dgrad_nhwc books the whole call under its own)."""
    _need_cl_bf16("conv1x1_nhwc", "x", x)
    _need_cuda_f32("bias", bias)
    N, Cin, H, W = x.shape
    Cout = bias.numel()
    if not (weight_frag.dtype == torch.int16 and weight_frag.dim() == 1 and weight_frag.is_contiguous()
            and weight_frag.numel() == Cout * Cin):
        raise OccAmdError("conv1x1_nhwc: weight must come from conv1x1_pack_weight (Cout*Cin bf16, fragment order)")
    s = int(stride)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    out = torch.empty((N, Cout, Ho, Wo), dtype=torch.bfloat16, device=x.device,
                      memory_format=torch.channels_last)
    want = (N, Cout, Ho // 2, Wo // 2) if residual_upsample2 else tuple(out.shape)
    if residual_upsample2 and (residual is None or Ho % 2 or Wo % 2):
        raise OccAmdUnsupported("conv1x1_nhwc: an upsampled residual needs even output sizes")
    if residual is not None and not (_is_cl_bf16(residual) and tuple(residual.shape) == want):
        raise OccAmdUnsupported("conv1x1_nhwc: residual must match the output (channels_last bfloat16)")
    _launch(_lib.lib().occ_conv1x1_nhwc_bf16_variant, x.device, "conv1x1_nhwc", x, weight_frag, bias, residual, out, N, H, W,
            Cin, Cout, s, 1 if relu else 0, 1 if residual_upsample2 else 0, 0 if variant is None else int(variant),
            timing=_timing, flops=2.0 * N * Ho * Wo * Cin * Cout)
    return out


def _conv_wgrad_nhwc(k, g, x, stride, out_dtype, splits):
    """The body of conv1x1_wgrad_nhwc (k = 1) and conv3x3_wgrad_nhwc (k = 3): they differ in their name, their two entry
    points, the shape and memory format of dw, the kernel_timing name and the k * k taps in the FLOPs."""
    what = f"conv{k}x{k}_wgrad_nhwc"
    _need_cl_bf16(what, "g", g)
    _need_cl_bf16(what, "x", x)
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise OccAmdUnsupported(f"{what}: out_dtype must be float32 or bfloat16")
    N, Cin, H, W = x.shape
    s = int(stride)
    Cout = g.shape[1]
    if s not in (1, 2) or tuple(g.shape) != (N, Cout, (H - 1) // s + 1, (W - 1) // s + 1) or g.device != x.device:
        raise OccAmdUnsupported(f"{what}: g must be (N, Cout, (H-1)//stride+1, (W-1)//stride+1) on x's device, "
                                "stride 1 or 2")
    sp = 0 if splits is None else int(splits)
    if sp < 0 or (splits is not None and sp == 0):
        raise OccAmdError(f"{what}: splits must be None or a positive int")
    lib = _lib.lib()
    query, fn = ((lib.occ_conv1x1_wgrad_workspace_bytes, lib.occ_conv1x1_wgrad_nhwc_bf16) if k == 1 else
                 (lib.occ_conv3x3_wgrad_workspace_bytes, lib.occ_conv3x3_wgrad_nhwc_bf16))
    nbytes = query(N, H, W, Cin, Cout, s, sp)
    if nbytes <= 0:
        raise OccAmdUnsupported(f"{what}: needs Cin % 32 == 0, Cout % 32 == 0, both <= 2048 "
                                f"(Cin={Cin}, Cout={Cout})")
    dw = torch.empty((Cout, Cin, k, k), dtype=out_dtype, device=x.device,
                     memory_format=torch.channels_last if k == 3 else torch.contiguous_format)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)     # torch's caching allocator
    _launch(fn, x.device, what, g, x, dw, 1 if out_dtype == torch.bfloat16 else 0, ws, N, H, W, Cin, Cout, s, sp,
            timing=f"bb_conv{k}x{k}_wgrad", flops=2.0 * N * g.shape[2] * g.shape[3] * k * k * Cin * Cout)
    return dw


def conv1x1_wgrad_nhwc(g, x, stride=1, out_dtype=torch.float32, splits=None):
    """Weight gradient of conv1x1_nhwc (csrc/conv1x1_wgrad_bf16.hip): dw[o, i] = sum over output pixels of
    g[n, o, yo, xo] * x[n, i, yo * stride, xo * stride], f32 accumulation on the matrix cores, deterministic.
    g (N, Cout, Ho, Wo) and x (N, Cin, H, W) channels_last bf16 with Ho = (H - 1) // stride + 1 -> (Cout, Cin, 1, 1) in
    out_dtype (float32 or bfloat16).  Cin % 32 == 0, Cout % 32 == 0, both <= 2048, stride 1 or 2: OccAmdUnsupported
    otherwise.  splits: None = the launcher's choice of pixel ranges; an int forces it (tests, probes)."""
    return _conv_wgrad_nhwc(1, g, x, stride, out_dtype, splits)


def conv1x1_dgrad_nhwc(g, w16):
    """Data gradient of a stride-1 conv1x1_nhwc: gx[n, i, y, x] = sum_o g[n, o, y, x] * w16[o, i] — the forward kernel on
    the transposed weight (zero bias, no residual, no ReLU); no kernel of its own.
    g (N, Cout, H, W) channels_last bf16; w16 (Cout, Cin, 1, 1) or (Cout, Cin) device weight -> (N, Cin, H, W) channels_last
    bf16.  Cin % 32 == 0 and Cout % 32 == 0: OccAmdUnsupported otherwise."""
    _need_cl_bf16("conv1x1_dgrad_nhwc", "g", g)
    if not (isinstance(w16, torch.Tensor) and w16.is_cuda and w16.is_floating_point() and w16.dim() in (2, 4)
            and w16.shape[0] == g.shape[1] and w16.numel() == w16.shape[0] * w16.shape[1] and w16.device == g.device):
        raise OccAmdUnsupported("conv1x1_dgrad_nhwc: w16 must be a (Cout, Cin, 1, 1) device weight matching g's channels")
    O, I = w16.shape[0], w16.shape[1]
    # one kernel_timing entry for the whole call: the transpose + pack of the weight and the zero bias are paid per call, and the
    # launch is not booked as a forward bb_conv1x1 launch as well
    with torch.cuda.device(g.device), _timed('bb_conv1x1_dgrad'):
        frag = conv1x1_pack_weight(w16.reshape(O, I).t())
        gx = conv1x1_nhwc(g, frag, torch.zeros(I, dtype=torch.float32, device=g.device), _timing=None)
    _note_flops('bb_conv1x1_dgrad', 2.0 * g.shape[0] * g.shape[2] * g.shape[3] * I * O)
    return gx


def mfma_pack_b_frag(weight2d):
    """(N, K) float32 device matrix -> bf16 in MFMA B-fragment order (int16 storage, N*K elements): what the
    fused bottleneck kernel streams straight from global memory."""
    _need_cuda_f32("weight", weight2d)
    if weight2d.dim() != 2:
        raise OccAmdError("mfma_pack_b_frag: expected a (N, K) matrix")
    weight2d = weight2d.contiguous()
    n, k = weight2d.shape
    packed = torch.empty(n * k, dtype=torch.int16, device=weight2d.device)
    _launch(_lib.lib().occ_mfma_pack_b_frag_bf16, weight2d.device, "mfma_pack_b_frag", weight2d, packed, n, k)
    return packed


def bottleneck64_pack(w1, b1, w2, b2, w3, b3, wds=None, bds=None):
    """Folded (BatchNorm already merged) weights of one 64-mid-channel bottleneck -> the operand set of
    bottleneck64_nhwc.  w1 (64, Cin[,1,1]), w2 (64, 64, 3, 3), w3 (256, 64[,1,1]), optional projection
    wds (256, Cin[,1,1]) / bds; biases float32.  Cin = 256 without projection, 64 with."""
    w1 = w1.float().reshape(w1.shape[0], -1)
    w3 = w3.float().reshape(w3.shape[0], -1)
    if tuple(w2.shape) != (64, 64, 3, 3) or w1.shape[0] != 64 or tuple(w3.shape) != (256, 64):
        raise OccAmdUnsupported("bottleneck64_pack: only 64 mid / 256 output channels")
    ds = wds is not None
    cin = w1.shape[1]
    if (ds and cin != 64) or (not ds and cin != 256):
        raise OccAmdUnsupported("bottleneck64_pack: Cin must be 256 (identity) or 64 (projection)")
    w2m = w2.float().permute(0, 2, 3, 1).reshape(64, 9 * 64)          # k = (ky*3 + kx)*64 + ci
    b3 = b3.float()
    if ds:
        w3 = torch.cat([w3, wds.float().reshape(256, 64)], dim=1)
        b3 = b3 + bds.float()
    return dict(w1=mfma_pack_b_frag(w1), b1=b1.float().contiguous(), w2=mfma_pack_b_frag(w2m),
                b2=b2.float().contiguous(), w3=mfma_pack_b_frag(w3), b3=b3.contiguous(), cin=cin, ds=ds)


def bottleneck64_nhwc(x, pack, variant=0, out=None):
    """One whole stride-1 ResNet bottleneck (64 mid channels) on a channels_last bf16 activation, one launch.
    x (N, Cin, H, W) channels_last bf16; pack from bottleneck64_pack -> (N, 256, H, W) channels_last bf16.
    variant: 0 = the launcher's choice; an int forces the kernel (occ_bottleneck64_nhwc_bf16_variant: 1 = first kernel,
    2 = second kernel, 3 / 4 / 5 = second kernel with tile order 0 / 1 / 2); every variant computes the same bits.
    out: a (N, 256, H, W) channels_last bf16 tensor on x's device to write into (every element is written), or None."""
    _need_cl_bf16("bottleneck64_nhwc", "x", x)
    N, Cin, H, W = x.shape
    if Cin != pack['cin']:
        raise OccAmdError("bottleneck64_nhwc: x has %d channels, the pack was built for %d" % (Cin, pack['cin']))
    if out is None:
        out = torch.empty((N, 256, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    else:
        _need_cl_bf16("bottleneck64_nhwc", "out", out)
        if tuple(out.shape) != (N, 256, H, W) or out.device != x.device or out.data_ptr() == x.data_ptr():
            raise OccAmdError("bottleneck64_nhwc: out must be a (N, 256, H, W) tensor on x's device, not x itself")
    _launch(_lib.lib().occ_bottleneck64_nhwc_bf16_variant, x.device, "bottleneck64_nhwc", x, pack['w1'], pack['b1'],
            pack['w2'], pack['b2'], pack['w3'], pack['b3'], out, N, H, W, Cin, 1 if pack['ds'] else 0, int(variant),
            timing='bb_bottleneck64',
            flops=2.0 * N * H * W * (Cin * 64 + 9 * 64 * 64 + 64 * 256 + (Cin * 256 if pack['ds'] else 0)))
    return out


def bottleneck64_next_pick(batch, H, W, cmid_next):
    """True where bottleneck64_next_nhwc replaces bottleneck64_nhwc + the two conv1x1_nhwc launches behind it for a
    (batch, 256, H, W) map (occ_bottleneck64_next_pick: a kernel for cmid_next, and both 1x1 launches on the resident
    kernel by the launcher's default rule; a pure function of the shape, needs no GPU)."""
    return bool(_lib.lib().occ_bottleneck64_next_pick(batch, H, W, int(cmid_next)))


def bottleneck64_next_nhwc(x, pack, w1_frag, b1, wds_frag, bds, out=None):
    """The last identity bottleneck of a stage and the two pointwise readers of its output in the next stage's first
    block, one launch; the 256-channel map stays on chip.
    x (N, 256, H, W) channels_last bf16; pack from bottleneck64_pack (identity block); w1_frag = conv1x1_pack_weight of the
    next conv1 (cmid, 256), b1 (cmid) f32; wds_frag = conv1x1_pack_weight of the next downsample (4 cmid, 256), bds (4 cmid)
    f32; cmid = 128
    -> (y, shortcut): y = relu(conv1(block(x))) (N, cmid, H, W), shortcut = downsample(block(x)) at stride 2
    (N, 4 cmid, (H-1)//2+1, (W-1)//2+1), both channels_last bf16.
    out: a (y, shortcut) pair of such tensors on x's device to write into (every element is written), or None.
    Bit-identical to bottleneck64_nhwc(x, pack, variant=2), then conv1x1_nhwc(., w1_frag, b1, relu=True, variant=2) and
    conv1x1_nhwc(., wds_frag, bds, stride=2, variant=2)."""
    _need_cl_bf16("bottleneck64_next_nhwc", "x", x)
    _need_cuda_f32("b1", b1)
    _need_cuda_f32("bds", bds)
    N, Cin, H, W = x.shape
    if Cin != 256 or pack['cin'] != 256 or pack['ds']:
        raise OccAmdError("bottleneck64_next_nhwc: x must have 256 channels and the pack be an identity block's")
    cmid = b1.numel()
    for name, wf, cout in (("w1_frag", w1_frag, cmid), ("wds_frag", wds_frag, 4 * cmid)):
        if not (isinstance(wf, torch.Tensor) and wf.is_cuda and wf.dtype == torch.int16 and wf.dim() == 1
                and wf.is_contiguous() and wf.numel() == cout * 256):
            raise OccAmdError(f"bottleneck64_next_nhwc: {name} must come from conv1x1_pack_weight ({cout}*256 bf16, "
                              "fragment order)")
    if bds.numel() != 4 * cmid:
        raise OccAmdError("bottleneck64_next_nhwc: bds must have 4 * cmid entries")
    shapes = ((N, cmid, H, W), (N, 4 * cmid, (H - 1) // 2 + 1, (W - 1) // 2 + 1))
    if out is None:
        y, sc = (torch.empty(s, dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last) for s in shapes)
    else:
        y, sc = out
        for name, t, s in (("out[0]", y, shapes[0]), ("out[1]", sc, shapes[1])):
            _need_cl_bf16("bottleneck64_next_nhwc", name, t)
            if tuple(t.shape) != s or t.device != x.device:
                raise OccAmdError(f"bottleneck64_next_nhwc: {name} must be a {s} tensor on x's device")
        if len({y.data_ptr(), sc.data_ptr(), x.data_ptr()}) != 3:
            raise OccAmdError("bottleneck64_next_nhwc: x and the two outputs must be distinct tensors")
    _launch(_lib.lib().occ_bottleneck64_next_nhwc_bf16, x.device, "bottleneck64_next_nhwc", x, pack['w1'], pack['b1'],
            pack['w2'], pack['b2'], pack['w3'], pack['b3'], w1_frag, b1, wds_frag, bds, y, sc, N, H, W, cmid,
            timing='bb_bottleneck64', flops=2.0 * N * H * W * (256 * 64 + 9 * 64 * 64 + 64 * 256 + 256 * cmid)
            + 2.0 * N * shapes[1][2] * shapes[1][3] * 256 * 4 * cmid)
    return y, sc


def conv3x3_pack_weight(weight):
    """torch Conv2d weight (Cout, Cin, 3, 3) float32 -> packed bf16 [Cin/32][tap][co][32] (int16 storage)."""
    _need_cuda_f32("weight", weight)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise OccAmdError("conv3x3_pack_weight: expected a (Cout, Cin, 3, 3) weight")
    cout, cin = weight.shape[:2]
    packed = torch.empty(weight.numel(), dtype=torch.int16, device=weight.device)
    _launch(_lib.lib().occ_conv3x3_pack_weight_bf16, weight.device, "conv3x3_pack_weight", weight, packed, cout, cin)
    return packed


def conv3x3_nhwc(x, w_packed, bias, cout, relu=False, stride=1, amax=None, variant=None):
    """3x3 / pad 1 / stride 1 or 2 convolution + bias (+ ReLU) on a channels_last bf16 activation, one launch.
    x (N, Cin, H, W) channels_last bf16; w_packed from conv3x3_pack_weight; bias (Cout) f32
    -> (N, Cout, (H-1)//stride+1, (W-1)//stride+1) channels_last bf16.
    amax: 8 int32 device words (new_absmax_words) the launch folds max|out| into (atomic maxima of the sign-stripped bf16
    patterns; they accumulate over launches) — the input of value_range_scale_from_amax.
    variant: None = the launcher's choice; an int forces the tile (occ_conv3x3_nhwc_bf16_variant: 10 * NT + RT for
    (2 * RT) x 16 pixels x (128 * NT) channels per block; stride 1: 12, 13, 14, 16, 18, 22, 23, 24; stride 2: 12, 13,
    22; 0 = the launcher's choice through the same entry point)."""
    return _conv3x3_nhwc(x, w_packed, bias, cout, relu, stride, amax, variant, 'bb_conv3x3')


def _conv3x3_nhwc(x, w_packed, bias, cout, relu, stride, amax, variant, timing):
    """conv3x3_nhwc booked under the kernel_timing entry `timing` (None: not booked; conv3x3_dgrad_nhwc books the whole call
    under its own)."""
    _need_cl_bf16("conv3x3_nhwc", "x", x)
    _need_cuda_f32("bias", bias)
    N, Cin, H, W = x.shape
    if w_packed.numel() != cout * Cin * 9 or bias.numel() != cout:
        raise OccAmdError("conv3x3_nhwc: inconsistent shapes")
    st = int(stride)
    if st not in (1, 2):
        raise OccAmdUnsupported("conv3x3_nhwc: stride must be 1 or 2")
    if amax is not None and not (amax.is_cuda and amax.dtype == torch.int32 and amax.numel() == 8 and amax.is_contiguous()):
        raise OccAmdError("conv3x3_nhwc: amax must be 8 contiguous int32 device words")
    out = torch.empty((N, cout, (H - 1) // st + 1, (W - 1) // st + 1), dtype=torch.bfloat16, device=x.device,
                      memory_format=torch.channels_last)
    _launch(_lib.lib().occ_conv3x3_nhwc_bf16_variant, x.device, "conv3x3_nhwc", x, w_packed, bias, out, N, H, W, Cin, cout, st,
            1 if relu else 0, amax, 0 if variant is None else int(variant), timing=timing,
            flops=2.0 * N * out.shape[2] * out.shape[3] * 9 * Cin * cout)
    return out


def conv3x3_wgrad_nhwc(g, x, stride=1, out_dtype=torch.float32, splits=None):
    """Weight gradient of conv3x3_nhwc (csrc/conv3x3_wgrad_bf16.hip): dw[o, i, ky, kx] = sum over output pixels of
    g[n, o, yo, xo] * x[n, i, yo * stride + ky - 1, xo * stride + kx - 1] (zero outside the map), f32 accumulation on the
    matrix cores, deterministic.
    g (N, Cout, Ho, Wo) and x (N, Cin, H, W) channels_last bf16 with Ho = (H - 1) // stride + 1 -> (Cout, Cin, 3, 3) in
    out_dtype (float32 or bfloat16), channels_last strides (memory order [Cout][3][3][Cin]).  Cin % 32 == 0, Cout % 32 == 0,
    both <= 2048, stride 1 or 2: OccAmdUnsupported otherwise.  splits: None = the launcher's choice of row ranges; an int
    forces it (tests, probes)."""
    return _conv_wgrad_nhwc(3, g, x, stride, out_dtype, splits)


def conv3x3_dgrad_weight(weight):
    """(Cout, Cin, 3, 3) weight -> the weight of the stride-1 data gradient as a convolution of g:
    Wd[i, o, ky, kx] = weight[o, i, 2 - ky, 2 - kx] (spatially flipped, input and output channels transposed).  A view."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise OccAmdError("conv3x3_dgrad_weight: expected a (Cout, Cin, 3, 3) weight")
    return weight.flip(2, 3).transpose(0, 1)


def conv3x3_dgrad_nhwc(g, w16):
    """Data gradient of a stride-1 conv3x3_nhwc: gx[n, i, y, x] = sum over (o, ky, kx) of g[n, o, y + 1 - ky, x + 1 - kx] *
    w16[o, i, ky, kx] — the forward kernel on conv3x3_dgrad_weight(w16) (zero bias, no ReLU); no kernel of its own.
    g (N, Cout, H, W) channels_last bf16; w16 (Cout, Cin, 3, 3) device weight (any strides) -> (N, Cin, H, W) channels_last
    bf16.  Cin % 128 == 0 and Cout % 32 == 0 (the forward kernel's shapes with the channels swapped): OccAmdUnsupported
    otherwise."""
    _need_cl_bf16("conv3x3_dgrad_nhwc", "g", g)
    if not (isinstance(w16, torch.Tensor) and w16.is_cuda and w16.is_floating_point() and w16.dim() == 4
            and tuple(w16.shape[2:]) == (3, 3) and w16.shape[0] == g.shape[1] and w16.device == g.device):
        raise OccAmdUnsupported("conv3x3_dgrad_nhwc: w16 must be a (Cout, Cin, 3, 3) device weight matching g's channels")
    O, I = w16.shape[0], w16.shape[1]
    if I % 128 or O % 32:
        raise OccAmdUnsupported(f"conv3x3_dgrad_nhwc: needs Cin % 128 == 0 and Cout % 32 == 0 (Cin={I}, Cout={O})")
    # one kernel_timing entry for the whole call: the flip + transpose + pack of the weight and the zero bias are paid per call,
    # and the launch is not booked as a forward bb_conv3x3 launch as well
    with torch.cuda.device(g.device), _timed('bb_conv3x3_dgrad'):
        packed = conv3x3_pack_weight(conv3x3_dgrad_weight(w16).float().contiguous())
        gx = _conv3x3_nhwc(g, packed, torch.zeros(I, dtype=torch.float32, device=g.device), I, False, 1, None, None, None)
    _note_flops('bb_conv3x3_dgrad', 2.0 * g.shape[0] * g.shape[2] * g.shape[3] * 9 * I * O)
    return gx


def conv3x3_conv1x1_pick(batch, H, W, cmid, cout, stride=1):
    """Tile id (10 * NT + RT) conv3x3_conv1x1_nhwc uses for an input of (batch, cmid, H, W), or 0 when the shape stays on
    conv3x3_nhwc + conv1x1_nhwc (occ_conv3x3_conv1x1_pick: a pure function of the shape, needs no GPU)."""
    return int(_lib.lib().occ_conv3x3_conv1x1_pick(batch, H, W, cmid, cout, int(stride)))


def conv3x3_conv1x1_nhwc(x, w3_packed, b2, cmid, w1_frag, b3, residual, stride=1, variant=None):
    """relu(conv1x1(relu(conv3x3(x) + b2) rounded to bf16) + b3 + residual) in one launch: conv2 + conv3 of a ResNet
    bottleneck with 128 or 256 mid channels; the mid tensor stays on chip.
    x (N, cmid, H, W) channels_last bf16; w3_packed from conv3x3_pack_weight((cmid, cmid, 3, 3)); b2 (cmid) f32; w1_frag from
    conv1x1_pack_weight((Cout, cmid)); b3 (Cout) f32, Cout = 4 * cmid; residual (N, Cout, Ho, Wo) channels_last bf16
    -> (N, Cout, Ho, Wo) channels_last bf16, Ho = (H-1)//stride + 1.
    variant: None = the tile conv3x3_conv1x1_pick returns (OccAmdUnsupported where that is 0); an int forces the 3x3 tile
    id.  Bit-identical to conv1x1_nhwc(conv3x3_nhwc(x, ..., relu=True, variant=v), ..., relu=True, variant=2)."""
    _need_cl_bf16("conv3x3_conv1x1_nhwc", "x", x)
    _need_cuda_f32("b2", b2)
    _need_cuda_f32("b3", b3)
    N, Cin, H, W = x.shape
    Cout = b3.numel()
    if Cin != cmid or w3_packed.numel() != cmid * Cin * 9 or b2.numel() != cmid:
        raise OccAmdError("conv3x3_conv1x1_nhwc: inconsistent 3x3 shapes")
    if not (w1_frag.dtype == torch.int16 and w1_frag.dim() == 1 and w1_frag.is_contiguous()
            and w1_frag.numel() == Cout * cmid):
        raise OccAmdError("conv3x3_conv1x1_nhwc: w1_frag must come from conv1x1_pack_weight (Cout*cmid bf16, fragment order)")
    st = int(stride)
    if st not in (1, 2):
        raise OccAmdUnsupported("conv3x3_conv1x1_nhwc: stride must be 1 or 2")
    Ho, Wo = (H - 1) // st + 1, (W - 1) // st + 1
    out = torch.empty((N, Cout, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    if not (_is_cl_bf16(residual) and tuple(residual.shape) == tuple(out.shape)):
        raise OccAmdUnsupported("conv3x3_conv1x1_nhwc: residual must match the output (channels_last bfloat16)")
    # timed under the 3x3 family (bench.py --full sums four fixed family names), with the FLOPs of both convolutions
    _launch(_lib.lib().occ_conv3x3_conv1x1_nhwc_bf16, x.device, "conv3x3_conv1x1_nhwc", x, w3_packed, b2, w1_frag, b3,
            residual, out, N, H, W, cmid, Cout, st, 0 if variant is None else int(variant), timing='bb_conv3x3',
            flops=2.0 * N * Ho * Wo * (9 * Cin * cmid + cmid * Cout))
    return out
