/*
 * occnet_amd.h — C ABI of the MI355X (gfx950) OccNet / BEVFormer-occ forward hot path.
 *
 * Every entry point takes plain device pointers + sizes (no torch types) and a
 * hipStream_t passed as void*.  All tensors are device-resident, contiguous, row-major.
 * Work is enqueued on `stream`; no call synchronises the device.  Every function returns
 * 0 on success and a negative OCC_E_* code on failure; occ_last_error() returns a
 * thread-local human readable message (the Python mirror turns it into RuntimeError, the
 * analogue of the TORCH_CHECK exceptions the reference's extension raises).
 *
 * Reference interfaces replaced (paths relative to the OccNet tree,
 *   P/ = projects/mmdet3d_plugin/):
 *   occ_ms_deform_attn_forward_f32   <- mmcv._ext.ms_deform_attn_forward, bound at
 *        P/bevformer/modules/multi_scale_deformable_attn_function.py:10-12, called :42-48,:118-124
 *   occ_ms_deform_attn_backward_f32  <- mmcv._ext.ms_deform_attn_backward, same file :74-84,:150-160
 *   occ_point_sampling_f32           <- BEVFormerEncoder.point_sampling, P/bevformer/modules/encoder.py:92-151
 *   occ_sca_fused_forward_f32        <- SpatialCrossAttention.forward :136-173 (rebatch, scatter-add,
 *        visible-camera mean) fused with MSDeformableAttention3D.forward :338-396 (softmax,
 *        offset normalisation, z-anchor add, deformable gather), P/bevformer/modules/spatial_cross_attention.py
 *   occ_sca_fused_backward_f32       <- the autograd backward of that same block (ms_deform_attn_backward on the
 *        padded rebatch + the softmax / normalisation / rebatch / camera-mean gradients) for fp32 value rows
 *   occ_tsa_fused_forward_f32        <- TemporalSelfAttention.forward :206-262 (softmax, locations,
 *        gather, mean over the 2-deep BEV queue), P/bevformer/modules/temporal_self_attention.py
 *   occ_tsa_fused_forward_q16v       <- the same lines over q16 value rows; occ_linear_bf16x3_q16rows <- self.value_proj
 *        (:198) writing them
 *   occ_conv3d_pack_weight_f32, occ_conv3d_bn_relu_f32 <- TransformerOcc.forward lifter view +
 *        decoder ConvModule(Conv3d k3 + BN3d + ReLU) x2 + permute, P/bevformer/modules/transformer_occ.py
 *        :305-308 (modules :106-126)
 *   occ_occ_heads_f32                <- predicter / flow_predicter MLPs, transformer_occ.py:132-141,318-319
 *   occ_linear_f32                   <- the nn.Linear / FFN / LayerNorm call sites of a BEVFormerLayer
 *   occ_dvr_render_forward_f32       <- dvr.render_forward, tools/ray_iou/lib/dvr/dvr.cu:70-388
 *   occ_ray_metrics_accumulate       <- process_one_sample + main + calc_metrics, P/datasets/ray_metrics.py:89-257
 *   occ_submission_rays              <- NuSceneOcc.format_results' per-sample loop (process_one_sample + the int8 / float16
 *        casts), P/datasets/nuscenes_occ.py:217-241
 *   occ_submission_score_accumulate  <- calc_metrics of the stand-alone scorer, tools/ray_iou/metric.py:31-73
 *   occ_heads_loss_fwd_f32 / _bwd_f32 <- the heads (transformer_occ.py:132-141,318-319) + BEVFormerOccHead.loss /
 *        loss_single, P/bevformer/dense_heads/bevformer_occ_head.py:163-196, and their autograd backward
 */
#ifndef OCCNET_AMD_H_
#define OCCNET_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCC_OK 0
#define OCC_E_INVALID (-1)     /* bad argument / unsupported shape                */
#define OCC_E_LAUNCH (-2)      /* hipLaunch / runtime error                       */
#define OCC_E_UNSUPPORTED (-3) /* shape is valid but has no fused kernel: caller  */
                               /* must use the unfused HIP path (never a CPU one) */

/* ABI version: bumped whenever a signature below changes. */
int occ_abi_version(void);
/* Thread-local message describing the last failure in this thread ("" if none). */
const char* occ_last_error(void);
/* Test hook: q[i] = the quotient a[i] / d[i] as the gather kernels compute it (reciprocal + Newton step + residual correction,
 * csrc/common.h occ::fdiv — NOT the compiler's IEEE division expansion, whose results are unreliable on gfx950 while an
 * MFMA-issuing wave shares the SIMD: DESIGN.md section 8d).  a, d, q: n DEVICE floats; d normal and non-zero. */
int occ_selftest_fdiv_f32(const float* a, const float* d, float* q, int64_t n, void* stream);

/* ==========================================================================================
 * PART I — THE REFERENCE INTERFACE.  The entry points a maintainer of the reference binds: one per interface the
 * reference itself loads from native code (mmcv._ext for the model, the dvr extension for the metric).  INTEGRATION.md
 * section 3 shows the binding stubs; nothing else in this header is needed for a drop-in.
 *   occ_ms_deform_attn_forward_f32, occ_ms_deform_attn_backward_f32 (+ _workspace_bytes / _ws_f32), occ_dvr_render_forward_f32
 * ========================================================================================== */

/* ------------------------------------------------------------------------------------------
 * Multi-scale deformable attention, forward (mmcv op semantics).
 *   value            (B, S, M, D)        f32   S = sum_l H_l*W_l
 *   spatial_shapes   (L, 2)              i64   (H_l, W_l), device memory
 *   level_start_index(L)                 i64   device memory
 *   sampling_loc     (B, Lq, M, L, P, 2) f32   (x, y) in [0,1] image-normalised
 *   attn_weight      (B, Lq, M, L, P)    f32
 *   out              (B, Lq, M*D)        f32   fully overwritten
 * out[b,q,m,:] = sum_l sum_p attn[b,q,m,l,p] * bilinear(value_l[b,:,m,:], loc*(W,H)-0.5),
 * zero padding, align_corners=False.  im2col_step keeps mmcv's contract:
 * step = min(B, im2col_step) must divide B (otherwise OCC_E_INVALID).
 */
int occ_ms_deform_attn_forward_f32(const float* value, const int64_t* spatial_shapes,
                                   const int64_t* level_start_index, const float* sampling_loc,
                                   const float* attn_weight, float* out, int B, int S, int M, int D,
                                   int L, int Lq, int P, int im2col_step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-scale deformable attention, backward (mmcv op semantics).  Shapes as in the forward;
 *   grad_output (B, Lq, M*D) f32 in;  grad_value (B, S, M, D), grad_sampling_loc (B, Lq, M, L, P, 2),
 *   grad_attn_weight (B, Lq, M, L, P) f32 out — PRE-ZEROED BY THE CALLER (the reference's autograd
 *   Function allocates them with zeros_like, multi_scale_deformable_attn_function.py:146-148);
 *   grad_value: for D == 32 (almost) WITHOUT floating-point atomics (counting sort of the bilinear row items into
 *   32-pixel bins, replayed by owner blocks from a device-built work list, csrc/msda_backward.hip): a bin with
 *   more than 2048 items is split over several blocks that combine with f32 atomics (a few dozen per bin); the
 *   item order inside a bin follows integer-atomic slot order.  The f32 summation order — and the last bits of
 *   grad_value — may therefore differ from run to run, as they do with mmcv's atomicAdd.  Other D (and
 *   OCC_MSDA_BWD_ATOMICS=1): f32 atomics throughout.
 */
int occ_ms_deform_attn_backward_f32(const float* value, const int64_t* spatial_shapes,
                                    const int64_t* level_start_index, const float* sampling_loc,
                                    const float* attn_weight, const float* grad_output,
                                    float* grad_value, float* grad_sampling_loc,
                                    float* grad_attn_weight, int B, int S, int M, int D, int L,
                                    int Lq, int P, int im2col_step, void* stream);
/* The same with CALLER-PROVIDED scratch for the atomic-free grad_value path (D == 32): `workspace` of at least
 * occ_ms_deform_attn_backward_workspace_bytes(...) bytes, 256-byte aligned, uninitialised (1.0-1.2 GB per SCA call
 * at the base config: the Python operator module takes it from torch's caching allocator).  workspace == NULL: the
 * library uses hipMallocAsync and, if that fails, falls back to float atomics with ONE warning on stderr.
 * ..._workspace_bytes returns 0 when the path does not apply (D != 32 / index ranges): workspace is then ignored. */
int64_t occ_ms_deform_attn_backward_workspace_bytes(int B, int S, int M, int D, int L, int Lq, int P);
int occ_ms_deform_attn_backward_ws_f32(const float* value, const int64_t* spatial_shapes,
                                       const int64_t* level_start_index, const float* sampling_loc,
                                       const float* attn_weight, const float* grad_output,
                                       float* grad_value, float* grad_sampling_loc,
                                       float* grad_attn_weight, int B, int S, int M, int D, int L,
                                       int Lq, int P, int im2col_step, void* workspace,
                                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray casting through an occupancy grid (RayIoU metric) — replaces the reference's `dvr.render_forward`
 * (tools/ray_iou/lib/dvr/dvr.cpp:68-72 binding, dvr.cu:70-388), called at
 * projects/mmdet3d_plugin/datasets/ray_metrics.py:116-123.
 *   sigma (N, T, Z, Y, X) f32 occupancy ; origin (N, T, 3) f32 and points (N, M, point_stride >= 3) f32
 *   in VOXEL units ; tindex (N, M) f32 time index per ray (< 0 = padded ray, skipped)
 *   pred_dist, gt_dist (N, M) f32 and coord_index (N, M, 3) f32 out, fully written
 *   (-1, -1, (0,0,0) for rays that never enter the grid) ; train_phase 0 = "test", 1 = "train".
 */
int occ_dvr_render_forward_f32(const float* sigma, const float* origin, const float* points,
                               const float* tindex, float* pred_dist, float* gt_dist,
                               float* coord_index, int N, int T, int Z, int Y, int X, int M,
                               int point_stride, int train_phase, void* stream);

/* ==========================================================================================
 * PART II — FUSED MI355X ENTRY POINTS.  No counterpart in mmcv._ext: each replaces a stretch of the reference's
 * Python / ATen code on the hot path with a gfx950 kernel (cited per entry); occnet_amd/plugin/ calls them behind the
 * reference's module / registry surface.  Grouped: (a) the encoder — projection of the pillars, the two fused gathers,
 * the Linear kernels and chains; (b) the decoder — Conv3d, heads, decode; (c) training partners; (d) the inference
 * plan of the stock image backbone (outside the SURVEY.md section 8 scope; builder conveniences such as
 * occ_mfma_pack_b_frag_bf16 / occ_bias_act_nhwc_bf16 live here).
 * ========================================================================================== */

/* ------------------------------------------------------------------------------------------
 * Pillar reference points -> per-camera image coordinates + visibility.
 *   ref_3d     (B, Z, Nq, 3) f32  normalised (x, y, z) in [0,1]
 *   lidar2img  (B, NC, 4, 4) f32 ; ego2lidar (4, 4) f32 ; pc_range[6] host floats
 *   ref_cam    (NC, B, Nq, Z, 2) f32 out ; bev_mask (NC, B, Nq, Z) u8 out (0/1)
 *   vis_bits   (B, Nq) u32 out: bit c set iff any z-anchor of query q is visible in camera c
 *              (may be NULL).  NC <= 32.
 */
int occ_point_sampling_f32(const float* ref_3d, const float* lidar2img, const float* ego2lidar,
                           const float* pc_range, float img_h, float img_w, float* ref_cam,
                           uint8_t* bev_mask, uint32_t* vis_bits, int B, int NC, int Nq, int Z,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused spatial cross-attention gather (one encoder layer, all cameras):
 *   slots[b,q,:] = (1/max(1,count[b,q])) * sum_{c : query q visible in camera c (batch 0's mask)}
 *                  MSDA( value[b*NC+c], softmax(logits[b,q]), ref_cam[c,b,q,z(p)] + offs[b,q]/(W_l,H_l) )
 *   value     (B*NC, S, M, D) f32 ; spatial_shapes (L,2) i64 ; level_start_index (L) i64
 *   offs      (B, Nq, M*L*P*2) f32 raw sampling_offsets Linear output, row stride offs_stride floats
 *   logits    (B, Nq, M*L*P)   f32 raw attention_weights Linear output, row stride logits_stride
 *   ref_cam   (NC, B, Nq, Z, 2) f32 ; vis_bits (B, Nq) u32 (see occ_point_sampling_f32)
 *   order     (Nq) i32 processing order of the queries (permutation; NULL = identity); only
 *             affects cache locality, never results
 *   slots     (B, Nq, M*D) f32 out, fully overwritten
 *   stats     NULL, or 2 x u64 device counters (pre-zeroed): [0] += visible (camera,query) rows,
 *             [1] += bilinear corners that fall inside their map (the N_in of the roofline formula)
 * Fused kernels exist for M=8, D=32, (L,P) in {(4,8),(4,4),(2,8),(1,8)}, Z | P; other shapes
 * return OCC_E_UNSUPPORTED.
 * Alignment (OCC_E_INVALID before any launch; the same for the f16v / q16v entries): value and slots 16 bytes; ref_cam
 * 8 bytes; offs 8 bytes with an even offs_stride.  16-bit value rows with L*P = 32 read a lane's four logits and offset
 * pairs as 16-byte loads: offs and logits 16 bytes, both strides multiples of 4, and — on the head-major kernel with
 * Z % 4 == 0 — ref_cam 16 bytes.
 */
int occ_sca_fused_forward_f32(const float* value, const int64_t* spatial_shapes,
                              const int64_t* level_start_index, const float* offs,
                              int64_t offs_stride, const float* logits, int64_t logits_stride,
                              const float* ref_cam, const uint32_t* vis_bits, const int32_t* order,
                              float* slots, uint64_t* stats, int B, int NC, int S, int M, int D,
                              int L, int P, int Z, int Nq, void* stream);

/* The same gather over fp16 VALUE maps (SURVEY.md §8d's e_v = 2 variant), as written by occ_value_proj_bf16_f16pairs /
 * occ_value_proj_bf16_planes.  One head row of a pixel is 64 bytes = 4 lanes x 16 bytes, so a wave load fetches 16 rows
 * instead of 8 (the texture path retires wave loads, not bytes: csrc/sca_fused.hip).  LAYOUT: pixel PAIRS —
 * value_f16[b * NC + c][pix >> 1][head (M)][pix & 1][D] fp16, pix = level_start + y * W + x, so the two x-neighbours
 * (2k, 2k + 1) of one head share one 128-byte line; S = pixel rows per camera entry INCLUDING padding to an even count.
 * Sampling arithmetic, attention weights and accumulation stay fp32 (v_fma_mix_f32); the value elements carry 11
 * significant bits.  value_scale: NULL, or a DEVICE float s (a power of two): the maps hold s * value (what the value
 * projections write under out_scale = occ_value_range_scale_bf16's result, so that no finite feature map can pass the
 * fp16 limit); the kernel divides its fp32 sums by count * s — exact, the result does not depend on s.  (abi 2) */
int occ_sca_fused_forward_f16v(const void* value_f16, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const float* offs, int64_t offs_stride,
                               const float* logits, int64_t logits_stride, const float* ref_cam,
                               const uint32_t* vis_bits, const int32_t* order, float* slots, uint64_t* stats,
                               int B, int NC, int S, int M, int D, int L, int P, int Z, int Nq,
                               const float* value_scale, void* stream);

/* The same gather over q16 VALUE maps (round 6): the fp16 maps' geometry, pair layout and byte count, but BLOCK FLOATING
 * POINT — every 16-byte piece (8 channels of one head of one pixel) holds 8 two's-complement int16 mantissas q_j under one
 * 4-bit exponent E:  value_j * s = q_j * 2^(E - 15), E = the binary exponent of the piece's largest |value * s| (0 .. 15),
 * stored in the two low bits of elements 0 and 1 (E & 3, E >> 2; those two are rounded to the nearest value with these
 * low bits, i.e. to 14 bits).  The reference keeps these rows in fp32 (spatial_cross_attention.py:75,387-390); fp16 rows
 * round every element to 2^-12 relative, q16 rounds the elements that dominate the gather's sums to 2^-16 relative —
 * measured against the CPU oracle: DESIGN.md section 2.  Written by occ_value_proj_bf16_planes(out_f16 = 2),
 * occ_value_proj_bf16_q16pairs or occ_sca_rows_encode_q16.  value_scale: the plane's range scale s (or NULL = 1). */
int occ_sca_fused_forward_q16v(const void* value_q16, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const float* offs, int64_t offs_stride,
                               const float* logits, int64_t logits_stride, const float* ref_cam,
                               const uint32_t* vis_bits, const int32_t* order, float* slots, uint64_t* stats,
                               int B, int NC, int S, int M, int D, int L, int P, int Z, int Nq,
                               const float* value_scale, void* stream);
/* Backward of occ_sca_fused_forward_f32 (fp32 value rows; same geometry and arguments).  grad_slots (B, Nq, M*D) f32 is the
 * gradient of `slots`.  Outputs:
 *   grad_value  (B*NC, S, M, D) f32, ACCUMULATED into (the caller zeroes it), like occ_ms_deform_attn_backward_f32's;
 *   grad_offs   (B, Nq, M*L*P*2) f32, row stride grad_offs_stride floats, every element overwritten;
 *   grad_logits (B, Nq, M*L*P)   f32, row stride grad_logits_stride floats, every element overwritten.
 * grad_offs / grad_logits have one writer per element and a fixed summation order: bit-identical run to run.  grad_value runs
 * through the binned, atomic-free path of the msda backward with the items of the visible (query, camera) rows only; with
 * OCC_MSDA_BWD_DETERMINISTIC=1 (read per call) it is bit-identical run to run as well.  `workspace`: CALLER-OWNED scratch of at
 * least occ_sca_fused_backward_workspace_bytes(...) bytes, 256-byte aligned, uninitialised.  Kernels exist for M=8, D=32,
 * (L,P) in {(4,8),(4,4),(2,8),(1,8)}, Z | P; other shapes (and ..._workspace_bytes() == 0) return OCC_E_UNSUPPORTED. */
int64_t occ_sca_fused_backward_workspace_bytes(int B, int NC, int S, int M, int D, int L, int P, int Nq);
int occ_sca_fused_backward_f32(const float* value, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const float* offs, int64_t offs_stride,
                               const float* logits, int64_t logits_stride, const float* ref_cam,
                               const uint32_t* vis_bits, const float* grad_slots, float* grad_value,
                               float* grad_offs, int64_t grad_offs_stride, float* grad_logits,
                               int64_t grad_logits_stride, int B, int NC, int S, int M, int D, int L, int P,
                               int Z, int Nq, void* workspace, int64_t workspace_bytes, void* stream);
/* fp32 value rows -> q16 pixel pairs.  v (groups, S, C) f32 contiguous, C % 32 == 0; out (groups, S + (S & 1), C) int16 in
 * the pair order (the pad row of an odd S is not written); scale: NULL or one DEVICE float s, a power of two with
 * max|v| * s <= 2^15. */
int occ_sca_rows_encode_q16(const float* v, void* out, const float* scale, int64_t groups, int S, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused temporal self-attention gather over the 2-deep BEV queue (single level):
 *   out[b,q,:] = 0.5 * sum_{t in {0,1}} MSDA( value[b*2+t], softmax_p(logits[b,q,m,t,:]),
 *                                            ref_2d[b*2+t,q] + offs[b,q,m,t,p]/(W,H) )
 *   value    f32, queue entry t of batch b at value + (b*2+t)*value_bt_stride floats, each (Nq_v, M, D)
 *            with Nq_v = bev_h*bev_w (pass value_bt_stride such that both entries alias one buffer
 *            when there is no history BEV: the reference stacks the same tensor twice)
 *   offs     (B, Nq, M*2*P*2) f32, row stride offs_stride ; logits (B, Nq, M*2*P), stride logits_stride
 *   ref_2d   (B*2, Nq, 1, 2) f32
 *   out      (B, Nq, M*D) f32
 *   order    NULL, or Nq int32: a permutation of 0..Nq-1, the query that wave r of a batch entry computes (locality
 *            only; the values are NOT range-checked: anything but a permutation leaves rows unwritten or reads out of range)
 * Alignment (checked, OCC_E_INVALID): value and out 16 bytes (value_bt_stride a multiple of 4 floats), offs and ref_2d
 * 8 bytes, offs_stride even: the kernel reads float2 offset pairs and 16-byte pieces of value rows.
 * Fused kernel exists for M=8, D=32, P=4, one level; otherwise OCC_E_UNSUPPORTED.
 */
int occ_tsa_fused_forward_f32(const float* value, int64_t value_bt_stride, const float* offs,
                              int64_t offs_stride, const float* logits, int64_t logits_stride,
                              const float* ref_2d, const int32_t* order, float* out, int B, int Nq,
                              int bev_h, int bev_w, int M, int D, int P, void* stream);
/* The same gather over q16 VALUE maps (opt-in: OCC_TSA_VALUES=q16): block floating point as for occ_sca_fused_forward_q16v,
 * in the pixel-pair layout occ_sca_rows_encode_q16 / occ_linear_bf16x3_q16rows write — queue entry t of batch b at
 * value_q16 + (b*2+t)*value_bt_stride int16 elements, each [pix >> 1][head][pix & 1][32] with pix = y*bev_w + x and
 * value_rows = bev_h*bev_w rounded up to even rows (the pad row of an odd map is never sampled).  value_bt_stride is 0 (both
 * entries alias one map) or at least one padded map (value_rows*M*D), and a multiple of 8.  value_scale: NULL (= 1) or one
 * DEVICE float s, the power-of-two range scale the rows were encoded with (stored under s / 2); the kernel divides
 * 2^15 * s / 2 out together with the queue mean, so the result depends on s only through the encoder's rounding.  offs, logits,
 * ref_2d, order, out, the alignment rules and the M=8, D=32, P=4 restriction (OCC_E_UNSUPPORTED) are those of
 * occ_tsa_fused_forward_f32; softmax, sampling arithmetic and accumulation are fp32.  One buffer descriptor spans both maps of a
 * batch entry: (value_bt_stride + value_rows*M*D) * 2 bytes must stay below 2^31 - 1280 (OCC_E_INVALID). */
int occ_tsa_fused_forward_q16v(const void* value_q16, int64_t value_bt_stride, int value_rows, const float* offs,
                               int64_t offs_stride, const float* logits, int64_t logits_stride,
                               const float* ref_2d, const int32_t* order, float* out, int B, int Nq,
                               int bev_h, int bev_w, int M, int D, int P, const float* value_scale, void* stream);
/* Backward of occ_tsa_fused_forward_f32 (same geometry and arguments; Nq = bev_h*bev_w: no query bands; `order` only steers
 * locality and has no counterpart here).  grad_out (B, Nq, M*D) f32 is the gradient of `out`.  spatial_shapes = {bev_h, bev_w}
 * and level_start_index = {0} as int64 in DEVICE memory (the grad_value replay reads them).  Outputs:
 *   grad_value  (B*2, Nq, M, D) f32 contiguous, one map per queue entry (also when value_bt_stride made the forward's entries
 *               alias: the caller adds the two), ACCUMULATED into (the caller zeroes it);
 *   grad_offs   (B, Nq, M*2*P*2) f32, row stride grad_offs_stride floats, every element overwritten;
 *   grad_logits (B, Nq, M*2*P)   f32, row stride grad_logits_stride floats, every element overwritten.
 * An output that is not wanted is NULL — grad_value, or grad_offs AND grad_logits together — and nothing is computed for it.
 * A sample whose location is not finite contributes nothing, as in the forward.  grad_offs / grad_logits have one writer per
 * element and a fixed summation order: bit-identical run to run.  grad_value runs through the binned, atomic-free path of the
 * msda backward; with OCC_MSDA_BWD_DETERMINISTIC=1 (read per call) it is bit-identical run to run as well.  `workspace`:
 * CALLER-OWNED scratch of at least occ_tsa_fused_backward_workspace_bytes(...) bytes, 256-byte aligned, uninitialised.
 * Alignment (checked, OCC_E_INVALID): value, grad_out and grad_value 16 bytes (value_bt_stride a multiple of 4 floats), offs,
 * grad_offs and ref_2d 8 bytes, offs_stride and grad_offs_stride even.  Kernel exists for M=8, D=32, P=4; other shapes (and
 * ..._workspace_bytes() == 0) return OCC_E_UNSUPPORTED. */
int64_t occ_tsa_fused_backward_workspace_bytes(int B, int Nq, int bev_h, int bev_w, int M, int D, int P);
int occ_tsa_fused_backward_f32(const float* value, int64_t value_bt_stride, const float* offs, int64_t offs_stride,
                               const float* logits, int64_t logits_stride, const float* ref_2d, const float* grad_out,
                               const int64_t* spatial_shapes, const int64_t* level_start_index, float* grad_value,
                               float* grad_offs, int64_t grad_offs_stride, float* grad_logits,
                               int64_t grad_logits_stride, int B, int Nq, int bev_h, int bev_w, int M, int D, int P,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Lifter + Conv3d(k=3, pad=1, stride=1, no bias) + BatchNorm3d(eval) + ReLU, implicit GEMM on the f32
 * matrix cores (exact f32).  Voxel grid (Z, Y, X) = torch's (D, H, W).
 *   in        in_layout 0: (B, Y, X, Z, Cin) f32, channels innermost (the layout this op writes)
 *             in_layout 1: (B, Y, X, Cin, Z) f32 = the lifter view of a (B, Y*X, Cin*Z) BEV embedding,
 *                          channel c = ci*Z + z (transformer_occ.py:305-307)
 *   w_packed  weight packed by occ_conv3d_pack_weight_f32 from torch's (Cout, Cin, 3, 3, 3) layout
 *             (Cout*Cin*27 floats)
 *   scale, shift (Cout) f32: y = conv*scale + shift  (BN eval: scale = gamma/sqrt(var+eps),
 *             shift = beta - mean*scale; a conv bias folds into shift)
 *   out       element (b, y, x, z, co) at b*out_stride_b + y*out_stride_y + x*out_stride_x + z*Cout + co
 *             (strides in floats): (Y,X)-major for the next conv, (X,Y)-major for the reference's
 *             permute(0,4,3,2,1) output order (transformer_occ.py:308)
 * Kernels exist for Cout = 32, Cin % 8 == 0, Z in {4, 8, 16, 32}; otherwise OCC_E_UNSUPPORTED.
 * occ_conv3d_channel_block(Cin) = input channels contracted per LDS phase (16, 8, or 0 = unsupported).
 */
int occ_conv3d_channel_block(int Cin);
int occ_conv3d_pack_weight_f32(const float* weight, float* packed, int Cin, int Cout, void* stream);
int occ_conv3d_bn_relu_f32(const float* in, const float* w_packed, const float* scale,
                           const float* shift, float* out, int B, int Z, int Y, int X, int Cin,
                           int Cout, int in_layout, int64_t out_stride_b, int64_t out_stride_y,
                           int64_t out_stride_x, int relu, void* stream);

/* bf16x3 variant of the two calls above (the default decoder kernel): operands split into hi + lo bf16,
 * a.w ~= al.wh + ah.wl + ah.wh accumulated in f32 by v_mfma_f32_32x32x16_bf16 (product error <= 2^-16; 5.3x less
 * matrix-pipe time than the exact-f32 instruction).  Same arguments; packed = 2 * Cout*Cin*27 16-bit words
 * ([phase][tap][hi, lo][k half][co][8]); needs Cout == 32, Cin % 16 == 0, Z in {4, 8, 16, 32}.
 * Cin == 8 (BASELINE configs[4]: 256 / 32 channels per voxel; round 4): two TAPS per 16-k MFMA step — lanes 0-31
 * contract tap 2s, lanes 32-63 tap 2s + 1, 14 steps; packed = 14 * 2 * 2 * 32 * 8 16-bit words
 * ([step][hi, lo][tap parity][co][8], the 28th tap zero).
 */
int occ_conv3d_pack_weight_bf16x3(const float* weight, void* packed, int Cin, int Cout, void* stream);
int occ_conv3d_bn_relu_bf16x3_f32(const float* in, const void* w_packed, const float* scale, const float* shift,
                                  float* out, int B, int Z, int Y, int X, int Cin, int Cout, int in_layout,
                                  int64_t out_stride_b, int64_t out_stride_y, int64_t out_stride_x, int relu,
                                  void* stream);

/* Second decoder convolution + BatchNorm(eval) + ReLU + BOTH occupancy heads + the class decode in ONE kernel
 * (csrc/conv3d_mfma.hip conv3d_heads_x3_kernel; reference transformer_occ.py:304-321, bevformer_occ_head.py:210-212):
 * the (B, Y, X, Z, 32) activations of the second convolution never reach HBM.  in (B, Y, X, Z, Cin = 32) f32 (layout 0 of
 * occ_conv3d_bn_relu_*), w_packed = occ_conv3d_pack_weight_bf16x3, scale / shift (32) as there; heads_packed =
 * occ_conv3d_heads_pack(...) (occ_conv3d_heads_pack_bytes() bytes: the eight head tensors of occ_occ_heads_f32 as bf16
 * hi/lo MFMA fragments + biases, C = 32, hidden = 64).  Outputs in the reference's (B, X, Y, Z, .) order:
 * occ_out (.., num_classes), flow_out (.., 2), occ_cls_out (..) int64 or NULL — the same values occ_conv3d_bn_relu_bf16x3_f32
 * (out (X, Y)-major) followed by occ_occ_heads_decode_f32(exact_f32 = 0) produce.  Cin == 32; Z == 16 (2 x 8 pillars per
 * block) or Z == 32 (2 x 4 pillars, BASELINE configs[4]; round 4). */
int64_t occ_conv3d_heads_pack_bytes(void);
int occ_conv3d_heads_pack(const float* w1_occ, const float* b1_occ, const float* w2_occ, const float* b2_occ,
                          const float* w1_flow, const float* b1_flow, const float* w2_flow, const float* b2_flow,
                          void* packed, int C, int hidden, int num_classes, void* stream);
int occ_conv3d_heads_decode_bf16x3_f32(const float* in, const void* w_packed, const float* scale, const float* shift,
                                       const void* heads_packed, float* occ_out, float* flow_out,
                                       int64_t* occ_cls_out, int B, int Z, int Y, int X, int Cin, int num_classes,
                                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Occupancy heads on every voxel feature row:
 *   occ  = Linear(hidden, num_classes)( Softplus( Linear(C, hidden)(feat) ) )     (predicter)
 *   flow = Linear(hidden, 2)( ReLU( Linear(C, hidden)(feat) ) )                   (flow_predicter)
 *   feat (n_rows, C) f32; weights in torch Linear layout (out_features, in_features), f32
 *   occ_out (n_rows, num_classes) f32 ; flow_out (n_rows, 2) f32
 * Fused kernel for C = 32, hidden = 64, num_classes <= 30; otherwise OCC_E_UNSUPPORTED.
 */
int occ_occ_heads_f32(const float* feat, const float* w1_occ, const float* b1_occ,
                      const float* w2_occ, const float* b2_occ, const float* w1_flow,
                      const float* b1_flow, const float* w2_flow, const float* b2_flow,
                      float* occ_out, float* flow_out, int64_t n_rows, int C, int hidden,
                      int num_classes, void* stream);
/* same + the decoded class per voxel, occ_cls[row] = argmax_c occ[row, c] (first index on ties) as int64 — the
 * reference's get_occ, P/bevformer/dense_heads/bevformer_occ_head.py:210-212 (softmax(-1).argmax(-1); softmax is
 * monotonic) — written by the same pass; occ_cls_out may be NULL.  exact_f32 != 0: the f32 matrix instruction
 * (occ_occ_heads_f32's kernel); 0: bf16x3 arithmetic (hi/lo-split operands on the bf16 MFMA, f32 accumulation,
 * product error <= 2^-16) — 5x less matrix-pipe time. */
int occ_occ_heads_decode_f32(const float* feat, const float* w1_occ, const float* b1_occ, const float* w2_occ,
                             const float* b2_occ, const float* w1_flow, const float* b1_flow,
                             const float* w2_flow, const float* b2_flow, float* occ_out, float* flow_out,
                             int64_t* occ_cls_out, int64_t n_rows, int C, int hidden, int num_classes,
                             int exact_f32, void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.Linear on the f32 matrix cores (exact f32) with the encoder's elementwise tail fused:
 *   out = LayerNorm( residual + act( [A1 | A2 (+ A2add)] @ W^T + bias ) )
 *   a1 (M, K1) row stride lda1 ; optional second K segment a2 (M, K2) row stride lda2 with an optional
 *   addend a2_add of the same shape/stride (the TSA query `cat([value, query + query_pos], -1)`,
 *   temporal_self_attention.py:197) ; weight (N, K1+K2) torch Linear layout ; bias (N) or NULL ;
 *   act 0 = none, 1 = ReLU ; residual (M, N) row stride ldres or NULL (added after act) ;
 *   ln_gamma / ln_beta (N) or both NULL, ln_eps: LayerNorm over the N outputs ; out (M, N) row stride ldo.
 * Requires K1, K2 multiples of 16, N % 4 == 0, 16-byte aligned rows, N <= 256 with LayerNorm;
 * otherwise OCC_E_UNSUPPORTED (the caller keeps the library GEMM).
 * Call sites replaced: value_proj / sampling_offsets / attention_weights / output_proj Linears
 * (spatial_cross_attention.py:334-341,173 ; temporal_self_attention.py:198-209,266), mmcv FFN + the three
 * LayerNorms of a BEVFormerLayer (encoder.py:377-404).
 */
int occ_linear_f32(const float* a1, int64_t lda1, int K1, const float* a2, const float* a2_add,
                   int64_t lda2, int K2, const float* weight, const float* bias, int act,
                   const float* residual, int64_t ldres, const float* ln_gamma, const float* ln_beta,
                   float ln_eps, float* out, int64_t ldo, int M, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * occ_linear_f32's fast variant on the bf16 matrix cores ("bf16x3"): every f32 operand is split into
 * hi + lo bf16 and A.W^T ~= Ah.Wh^T + Ah.Wl^T + Al.Wh^T is accumulated in f32 (relative error of a product
 * <= 2^-16).  Same arguments, except that the weight is given PACKED by occ_linear_pack_weight_bf16x3 in
 * MFMA fragment order: packed[K/16][ceil(N/32)][hi, lo][lane][8] bf16 = ceil(N/32)*32 * K * 2 16-bit words
 * (columns zero-padded to a multiple of 32; K % 16 == 0).
 */
int occ_linear_pack_weight_bf16x3(const float* weight, void* packed, int N, int K, void* stream);
int occ_linear_bf16x3_f32(const float* a1, int64_t lda1, int K1, const float* a2, const float* a2_add,
                          int64_t lda2, int K2, const void* weight_packed, const float* bias, int act,
                          const float* residual, int64_t ldres, const float* ln_gamma,
                          const float* ln_beta, float ln_eps, float* out, int64_t ldo, int M, int N,
                          void* stream);
/* The plain Linear out = a.W^T + bias of occ_linear_bf16x3_f32 (same kernel, same tile choice: the SAME fp32 values) stored
 * as q16 value rows for occ_tsa_fused_forward_q16v instead of fp32: the M rows are `groups` maps of S = M / groups rows
 * (M % groups == 0), row r of map g goes to the pixel-pair position
 *     out[(g*S_pad + (r & ~1))*256 + (n/32)*64 + (r & 1)*32 + n%32]     (int16, S_pad = S + (S & 1); pad rows are not written)
 * with one exponent per 16-byte piece of 8 channels, exactly what occ_sca_rows_encode_q16 makes of the fp32 result — without
 * the pass over it.  a (M, K) f32 with row stride lda; scale: NULL (= 1) or one DEVICE float s, a power of two with
 * max|out| * s <= 2^15.  Covers N == 256 and K % 16 == 0 (lda % 4 == 0); no residual, activation or LayerNorm; anything
 * else returns OCC_E_UNSUPPORTED. */
int occ_linear_bf16x3_q16rows(const float* a, int64_t lda, int K, const void* weight_packed, const float* bias,
                              const float* scale, void* out, int M, int N, int groups, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row-local Linear CHAINS of a BEVFormerLayer, one launch each (csrc/linear_chain_x3.hip; bf16x3 arithmetic as
 * occ_linear_bf16x3_f32; embed_dims = 256).  A 64-row block keeps the LayerNorm'd tile in LDS as the next Linear's
 * operand; the weights of all stages of a chain are ONE buffer in consumption order:
 *   occ_linear_chain_pack_bf16x3(W (N, K)) -> for every 256-row group of W: [K/16][8 tiles][hi | lo][lane][8 bf16]
 *   (rows beyond N are zero), occ_linear_chain_packed_bytes(N, K) bytes; the caller concatenates the packs of the stages.
 *
 * occ_linear_ln_chain_bf16x3_f32 — "program A":   y = LayerNorm(a.W1^T + b1 + residual)      (N = K = 256)
 *                                                 z = act2(y.W2^T + b2)                      (n2 columns, n2 % 32 == 0)
 *   w_chain = [pack(W1) | pack(W2)], bias_chain = [b1 (256) | b2 zero-padded to ceil(n2 / 256) * 256].
 *   Call sites replaced: TemporalSelfAttention.output_proj + residual (temporal_self_attention.py:266-272) + the layer's
 *   first LayerNorm (encoder.py:377-404 `norm`) + MSDeformableAttention3D.sampling_offsets | attention_weights
 *   (spatial_cross_attention.py:334-341) — z is what occ_sca_fused_forward_* reads.
 *
 * occ_encoder_ffn_chain_bf16x3_f32 — "program B": x2 = LayerNorm1(a.Wo^T + bo + residual)
 *                                                 y  = LayerNorm2(relu(x2.W1^T + b1).W2^T + b2 + x2)   (hidden = 512)
 *                                   optional tail: zq = y.Wq^T + q_term (nq <= 256 columns, nq % 64 == 0),
 *                                                  zv = y.Wv^T + bv     (256 columns)
 *   w_chain = [pack(Wo) | pack(W1) | pack(W2) | pack(Wq) | pack(Wv)] (the last two only with a tail),
 *   bias_chain = [bo | b1 (512) | b2 | 256 zeros | bv].  zq == zv == NULL: no tail.  `y` doubles as scratch (x2 is parked
 *   in the block's own rows before y is written).
 *   Call sites replaced: SpatialCrossAttention.output_proj + residual (spatial_cross_attention.py:173-175), the second
 *   LayerNorm, mmcv FFN (custom_base_transformer_layer.py:144-160) + the third LayerNorm, and — tail — the NEXT layer's
 *   TemporalSelfAttention sampling_offsets | attention_weights on cat([query, query + pos]) (temporal_self_attention.py
 *   :197-209; without history Wq = W[:, :256] + W[:, 256:], q_term = pos.W[:, 256:]^T + b) and its value_proj (:198).
 */
int64_t occ_linear_chain_packed_bytes(int N, int K);
int occ_linear_chain_pack_bf16x3(const float* weight, void* packed, int N, int K, void* stream);
int occ_linear_ln_chain_bf16x3_f32(const float* a, int64_t lda, const float* residual, int64_t ldres,
                                   const void* w_chain, const float* bias_chain, const float* ln_gamma,
                                   const float* ln_beta, float ln_eps, float* y, int64_t ldy, float* z,
                                   int64_t ldz, int n2, int act2, int M, void* stream);
int occ_encoder_ffn_chain_bf16x3_f32(const float* a, int64_t lda, const float* residual, int64_t ldres,
                                     const void* w_chain, const float* bias_chain, const float* ln1_gamma,
                                     const float* ln1_beta, float ln1_eps, const float* ln2_gamma,
                                     const float* ln2_beta, float ln2_eps, float* y, int64_t ldy,
                                     const float* q_term, int64_t ldq_term, float* zq, int64_t ldzq, int nq,
                                     float* zv, int64_t ldzv, int M, void* stream);

/* Program C: the tail stage alone — two Linears of the SAME 256-wide rows in one launch (the first encoder layer's TSA
 * query Linears and value projection, temporal_self_attention.py:197-209,239-240, straight from the BEV queries):
 *   zq (M, nq) = a . Wq^T + q_term (or + 0),   zv (M, 256) = a . Wv^T + bv.
 * w_chain = chain packs of [Wq (nq <= 256 rows, zero-padded to 256), Wv]; bias_chain = [256 zeros | bv].
 * nq % 64 == 0; rows 16-byte aligned. */
int occ_linear_pair_chain_bf16x3_f32(const float* a, int64_t lda, const void* w_chain, const float* bias_chain,
                                     const float* q_term, int64_t ldq_term, float* zq, int64_t ldzq, int nq,
                                     float* zv, int64_t ldzv, int M, void* stream);
/* The tile split of the three chain programs, a pure host function: M rows on `slots` resident blocks (the launchers
 * pass 2 x the CU count) -> blocks [0, nfull) own 64-row tiles, blocks [nfull, ntiles) 32-row tiles of the rows behind
 * them.  32-row tiles appear only when the last round of 64-row tiles would fill at most half of the slots. */
int occ_linear_chain_tile_split(int M, int slots, int* nfull, int* ntiles);

/* Training path of SpatialCrossAttention, query side (csrc/sca_prep.hip; reference spatial_cross_attention.py:338-373
 * applied to the per-camera rebatched rows): from proj (B, Q, >= 3*M*L*P) = [sampling_offsets | attention_weights]
 * Linear outputs per BEV query, row_to_query (R) (-1 = padded row) and the rebatched reference points ref_rb
 * (B, R, Z, 2):  attn (B, R, M, L, P) = softmax over L*P,  loc (B, R, M, L, P, 2) = ref_rb[.., p % Z, :] +
 * offsets / (W_l, H_l) — the layouts ms_deform_attn_forward takes.  The backward accumulates, per BEV query over the
 * <= Kq rows of query_to_rows (Q, Kq) (-1 = none), d proj (B, Q, proj_ld) from grad_loc / grad_attn (every row of
 * dproj is written).  M = 8, L = 4, P = 8 only (OCC_E_UNSUPPORTED otherwise: the caller keeps the ATen ops). */
int occ_sca_prep_forward_f32(const float* proj, int64_t proj_batch_stride, int proj_ld, const int64_t* row_to_query,
                             const float* ref_rb, const int64_t* spatial_shapes, float* loc, float* attn, int B,
                             int64_t R, int M, int L, int P, int Z, void* stream);
int occ_sca_prep_backward_f32(const float* grad_loc, const float* grad_attn, const float* attn,
                              const int64_t* query_to_rows, int Kq, const int64_t* spatial_shapes, float* dproj,
                              int proj_ld, int B, int64_t R, int64_t Q, int M, int L, int P, void* stream);

/* Row gather-sum (csrc/rows_index.hip): out[b][r][:] = sum over k < K with index[r*K + k] >= 0 of x[b][index[r*K + k]][:].
 * x (B, rows_in, F) with batch stride x_batch_stride (floats), index (rows_out, K) int64 (-1 = no row), out
 * (B, rows_out, F) contiguous; F % 4 == 0, 16-byte aligned.  K = 1: SpatialCrossAttention's per-camera rebatch of the
 * visible BEV queries (spatial_cross_attention.py:145-153); index = the inverse map: the scatter back into the BEV
 * slots (:165-167); each is the other's gradient, so the training path needs no float-atomic index_add. */
int occ_rows_gather_sum_f32(const float* x, int64_t x_batch_stride, const int64_t* index, int K, float* out, int B,
                            int64_t rows_out, int64_t rows_in, int F, void* stream);

/* Training partner of occ_linear_bf16x3_f32 (csrc/linear_wgrad.hip): weight and bias gradient of a Linear,
 *     dw[n][k] = sum_m dy[m][n] * x[m][k]      db[n] = sum_m dy[m][n]      (db may be NULL)
 * on the bf16 matrix cores with the same hi/lo operand split (product error <= 2^-16), f32 accumulation.
 * The row dimension is reduced in chunks into `workspace` (occ_linear_wgrad_workspace_bytes(M, N, K) bytes, owned by
 * the caller, 16-byte aligned) and summed in a fixed order: the result is deterministic, no float atomics.
 * dy (M, N) with row stride lddy, x (M, K) with row stride ldx, dw (N, K) contiguous (overwritten, not accumulated).
 * Replaces: ATen's addmm backward behind the nn.Linear call sites listed at occ_linear_f32.  The input gradient
 * needs no entry point: dx = occ_linear_bf16x3_f32(dy, pack(W^T)). */
int64_t occ_linear_wgrad_workspace_bytes(int M, int N, int K);
int occ_linear_wgrad_bf16x3_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dw, float* db,
                                void* workspace, int64_t workspace_bytes, int M, int N, int K, void* stream);

/* Training partner of occ_conv3d_bn_relu_bf16x3_f32 (csrc/linear_wgrad.hip linear_wgrad_n32_kernel; round 4): weight
 * gradient of a 3x3x3 / stride 1 / pad 1 Conv3d with 32 output channels — the decoder's two convolutions, reference
 * transformer_occ.py:106-126 (autograd of nn.Conv3d).  dy_pad (B, Y+2, X+2, Z+2, 32) and x_pad (B, Y+2, X+2, Z+2, Cin) are
 * ZERO-PADDED channels-last copies of the output gradient and the input: in the padded grid a tap is a constant row
 * offset, dW = dy_pad^T . im2col(x_pad) in one launch.  dw (32, 27, Cin): dW[co][kz*9 + ky*3 + kx][ci].  The input
 * gradient needs no entry point: dx = occ_conv3d_bn_relu_bf16x3_f32(dy, pack(flipped, transposed W), scale 1, shift 0). */
int64_t occ_conv3d_wgrad_workspace_bytes(int B, int Z, int Y, int X, int Cin);
int occ_conv3d_wgrad_bf16x3_f32(const float* dy_pad, const float* x_pad, float* dw, void* workspace,
                                int64_t workspace_bytes, int B, int Z, int Y, int X, int Cin, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backbone tail (outside the hand-written hot path): in place x = relu?(x + bias[c] (+ residual)) on an
 * NHWC bf16 activation of `rows` = N*H*W pixels x C channels (C % 8 == 0, 16-byte aligned).  Replaces the
 * BatchNorm / ReLU / residual-add launches after each MIOpen convolution of the ResNet-50 bottlenecks once
 * eval-mode BatchNorm is folded into the convolution weights.
 */
int occ_bias_act_nhwc_bf16(void* x, const float* bias, const void* residual, int64_t rows, int C, int relu,
                           void* stream);

/* Backward of that tail for the training step's autocast backbone (the reference trains its ResNet with eval-mode
 * BatchNorm, bevformer_base_occ.py:55; conv -> + bias (+ residual) -> ReLU is one autograd node in plugin/backbone.py):
 *   g = relu ? (y > 0 ? grad_y : 0) : grad_y   (bf16 NHWC; relu == 0: g is not written and may be NULL, y is not read)
 *   bias_grad[c] = sum over rows of g[., c]     (fp32, deterministic: per-block partial sums added in a fixed order)
 * in one pass over the activation.  partial: occ_bias_act_bwd_partial_floats(rows, C) floats of scratch (0 = unsupported C:
 * C % 8 != 0 or C > 2048). */
int64_t occ_bias_act_bwd_partial_floats(int64_t rows, int C);
int occ_bias_act_bwd_nhwc_bf16(const void* grad_y, const void* y, void* g, float* partial, float* bias_grad,
                               int64_t rows, int C, int relu, void* stream);

/* Weight side of the same training nodes: eval-mode BatchNorm folded into a convolution weight, and the fold's chain rule,
 * one launch each (conv_bn_folded's arithmetic, plugin/backbone.py; rstd = 1 / sqrt(running_var + eps), mean_rstd =
 * running_mean * rstd are constants of the frozen statistics).  weight / w_folded / grad_weight: (Cout, Cin, KH, KW) fp32
 * contiguous; w_folded_bf16_nhwc: the same values as bf16 in channels_last order [Cout][KH][KW][Cin]; bias[o] = beta[o] -
 * gamma[o] * mean_rstd[o].  Backward: grad_w_bf16 = the convolution's bf16 weight gradient with the given ELEMENT strides;
 * grad_weight = grad_w * gamma * rstd; grad_gamma[o] = rstd[o] * sum(grad_w[o] * weight[o]) - mean_rstd[o] * grad_bias[o]
 * (grad_beta = grad_bias). */
int occ_conv_bn_fold_fwd_f32(const float* weight, const float* gamma, const float* beta, const float* rstd,
                             const float* mean_rstd, float* w_folded, void* w_folded_bf16_nhwc, float* bias, int Cout,
                             int Cin, int KH, int KW, void* stream);
int occ_conv_bn_fold_bwd_f32(const void* grad_w_bf16, int64_t stride_o, int64_t stride_i, int64_t stride_h, int64_t stride_w,
                             const float* weight, const float* gamma, const float* rstd, const float* mean_rstd,
                             const float* grad_bias, float* grad_weight, float* grad_gamma, int Cout, int Cin, int KH, int KW,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step glue of a BEVFormerLayer (reference: encoder.py:377-404 with the module tails
 * spatial_cross_attention.py:173-175, temporal_self_attention.py:270-272 and mmcv's FFN): y = LayerNorm(dropout(x) +
 * residual) and its backward, one launch each, C = 256 (OCC_E_UNSUPPORTED otherwise).
 *   forward : z = x * keep / (1 - p) + residual ; y = (z - mean) * rstd * gamma + beta ; stats[r] = (mean, rstd)
 *   backward: grad_residual = LayerNorm's input gradient ; grad_x = grad_residual * keep / (1 - p) (p == 0: not written, may
 *             be NULL — it IS grad_residual) ; grad_gamma_beta = (sum_rows gy * zhat | sum_rows gy), 2 C floats, by a fixed-order
 *             two-stage sum (partial: occ_dropout_add_ln_bwd_partial_floats(rows, C) floats of scratch).
 * keep = occ_ln_dropout_hash(element index, seed_lo, seed_hi) >= (uint32)(p * 2^32): the mask is a pure function of (seed,
 * index) and is never stored; the caller draws `seed` per call and hands the same one to the backward. */
unsigned occ_ln_dropout_hash(unsigned index, unsigned seed_lo, unsigned seed_hi);
int64_t occ_dropout_add_ln_bwd_partial_floats(int64_t rows, int C);
int occ_dropout_add_ln_fwd_f32(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                               float p_drop, uint64_t seed, float* z, float* y, float* stats, int64_t rows, int C,
                               void* stream);
int occ_dropout_add_ln_bwd_f32(const float* grad_y, const float* z, const float* stats, const float* gamma, float p_drop,
                               uint64_t seed, float* grad_x, float* grad_residual, float* partial, float* grad_gamma_beta,
                               int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm3d + ReLU of the voxel decoder on the convolution's channels-last output (reference:
 * ConvModule(Conv3d -> BatchNorm3d -> ReLU), transformer_occ.py:106-126, and ATen's autograd of it: batch_norm's statistics /
 * normalise kernels, relu, threshold_backward, batch_norm_backward's two kernels, the permute copies of layer 2).  C = 32
 * only; OCC_E_UNSUPPORTED for another C, for fewer than 2 rows (torch raises there too) and for 2^31 elements or more
 * (counted on the zero-haloed grid for the calls that take one).  y: (rows, 32) = (B, Y, X, Z, 32) contiguous fp32.
 *   stats   : mean_rstd (2, 32) = per-channel mean | 1 / sqrt(biased variance + eps) over the rows (shifted sums, fp64 second
 *             stage).  running_mean / running_var: both NULL (nothing is written) or both given, updated in place:
 *             running_mean = (1 - eaf) running_mean + eaf mean ; running_var = (1 - eaf) running_var + eaf var rows / (rows - 1).
 *   fwd     : out = max(0, (y - mean) rstd gamma + beta); element (b, y, x, z, c) of out at b out_sb + y out_sy + x out_sx +
 *             32 z + c (as occ_conv3d_bn_relu_*: the (B, X, Y, Z, C) order of the reference's permute is a choice of strides).
 *   bwd     : dz = grad_out [pre-activation > 0] with grad_out read through go_sb / go_sy / go_sx; grad_gamma_beta (2, 32) =
 *             sum dz xhat | sum dz; dy = gamma rstd (dz - sum dz / rows - xhat sum(dz xhat) / rows) written to grad_y
 *             (B, Y, X, Z, 32) contiguous and / or grad_y_pad (B, Y+2, X+2, Z+2, 32) INCLUDING its zero halo (no pre-zeroing;
 *             the operand occ_conv3d_wgrad_bf16x3_f32 takes).  Either may be NULL.
 * partial: occ_bn3d_relu_train_partial_floats(rows, C) floats of scratch (0: unsupported), shared by stats and bwd.  Sums are
 * taken in a fixed order: every output is the same bits run to run. */
int64_t occ_bn3d_relu_train_partial_floats(int64_t rows, int C);
int occ_bn3d_relu_train_stats_f32(const float* y, float* partial, float* mean_rstd, float* running_mean, float* running_var,
                                  float eaf, float eps, int64_t rows, int C, void* stream);
int occ_bn3d_relu_train_fwd_f32(const float* y, const float* mean_rstd, const float* gamma, const float* beta, float* out, int B,
                                int Z, int Y, int X, int C, int64_t out_sb, int64_t out_sy, int64_t out_sx, void* stream);
int occ_bn3d_relu_train_bwd_f32(const float* grad_out, int64_t go_sb, int64_t go_sy, int64_t go_sx, const float* y,
                                const float* mean_rstd, const float* gamma, const float* beta, float* partial,
                                float* grad_gamma_beta, float* grad_y, float* grad_y_pad, int B, int Z, int Y, int X, int C,
                                void* stream);

/* SCA value projection straight off the backbone's bf16 feature maps (rows A3/A8: replaces the reference's
 * fp32 feature flatten + embedding adds, transformer_occ.py:204-222, AND MSDeformableAttention3D.value_proj,
 * spatial_cross_attention.py:366), all FPN levels in one launch.  For segment (= level) s, row m = g*rpg_s + i:
 *   out[(g*out_group_rows + out_row0[s] + i)*ldo + n] = sum_k a[s][m*lda[s] + k] * W[n][k]
 *                                                      + group_bias[s][(g % bias_groups)*N + n]
 * n_segments <= 8 ; a[s] (rows[s], K) bf16 device pointers, lda[s] row strides ; the arrays a / lda / rows /
 * rows_per_group / out_row0 / group_bias are HOST arrays of n_segments entries (read at launch) ;
 * weight_packed = occ_linear_pack_weight_bf16x3(W (N, K)) (hi/lo split: products exact to 2^-17, two MFMAs per
 * k-step) ; group_bias[s] (bias_groups, N) f32 device pointers, or group_bias == NULL — for the SCA:
 * (cams_embeds[cam] + level_embeds[s]) . W^T + b, one row per camera ; out f32.
 * Needs K % 32 == 0, N % 4 == 0, lda % 8 == 0, ldo % 4 == 0.
 */
int occ_value_proj_bf16_f32(int n_segments, const void* const* a, const int64_t* lda, const int64_t* rows,
                            const int64_t* rows_per_group, const int64_t* out_row0,
                            const float* const* group_bias, int bias_groups, const void* weight_packed,
                            float* out, int64_t ldo, int K, int N, int64_t out_group_rows, void* stream);
/* same with the output written as fp16 for occ_sca_fused_forward_f16v, IN ITS PIXEL-PAIR ORDER: row r = out_row0[s] + i of
 * group g's block lands at out[(g*out_group_rows + (r & ~1)) * ldo + (n / 32) * 64 + (r & 1) * 32 + n % 32].  Needs
 * ldo == N, N % 32 == 0, out_group_rows even (pad an odd pixel count by one row).  out_scale: NULL, or a DEVICE float:
 * out = fp16(out_scale[0] * (a . W^T + group_bias)) — the range scale of occ_value_range_scale_bf16 (abi 2). */
int occ_value_proj_bf16_f16pairs(int n_segments, const void* const* a, const int64_t* lda, const int64_t* rows,
                            const int64_t* rows_per_group, const int64_t* out_row0,
                            const float* const* group_bias, int bias_groups, const void* weight_packed,
                            void* out, int64_t ldo, int K, int N, int64_t out_group_rows, const float* out_scale,
                            void* stream);
/* same with q16 pixel pairs (occ_sca_fused_forward_q16v); exists on the activation-resident kernel only (K == 256,
 * N % 256 == 0, rows_per_group >= 128): OCC_E_UNSUPPORTED otherwise — project to f32 and use occ_sca_rows_encode_q16. */
int occ_value_proj_bf16_q16pairs(int n_segments, const void* const* a, const int64_t* lda, const int64_t* rows,
                            const int64_t* rows_per_group, const int64_t* out_row0,
                            const float* const* group_bias, int bias_groups, const void* weight_packed,
                            void* out, int64_t ldo, int K, int N, int64_t out_group_rows, const float* out_scale,
                            void* stream);

/* Range-safe fp16 value rows (csrc/value_range.hip).  The reference keeps the SCA value rows in fp32
 * (spatial_cross_attention.py:75,387-390, @force_fp32); stored as fp16 a plane whose values pass 65 504 would be clamped.
 * This call derives, on the device and per call, one POWER-OF-TWO scale per projection plane from an a-priori bound:
 *     |a . W_p^T + gb_p|  <=  max|a| * row_l1[p] + bias_max[p],      row_l1[p] = max_n sum_k |W_p[n][k]|,
 *     scale_out[p] = 2^(15 - e) with bound_p = m 2^e, m in [0.5, 1)   (bound_p * scale <= 2^15 = half of the fp16 limit)
 * so no finite input can saturate; a zero / Inf / NaN bound gives 1.  max|a| is measured over every segment (bf16 rows,
 * K % 8 == 0, lda % 8 == 0); row_l1 / bias_max: DEVICE arrays of n_planes (<= 8) floats (abi 3: no host round trip, the
 * call is graph-safe and follows the live weights).
 * scale_out: DEVICE floats [0, n_planes) scales, [n_planes] max|a|, [n_planes + 1, 2 n_planes + 1) the bounds.
 * work: two DEVICE words of scratch, zeroed by the call itself (calls sharing `work` must be stream-ordered).  Scaling by
 * a power of two is exact both ways: results equal the unscaled fp16-row path's wherever that one does not saturate. */
int occ_value_range_scale_bf16(int n_segments, const void* const* a, const int64_t* lda, const int64_t* rows, int K,
                               int n_planes, const float* row_l1, const float* bias_max, float* scale_out,
                               uint32_t* work, void* stream);
/* The same scales when the PRODUCER of the maps already holds max|a|: amax8 = 8 DEVICE words, the largest sign-stripped
 * bf16 pattern each shard of the producer's blocks stored (occ_conv3x3_nhwc_bf16_amax; the maximum over the 8 words is
 * max|a|).  One 64-thread launch instead of a pass over the maps (52 us at the base config). */
int occ_value_range_scale_from_amax(const uint32_t* amax8, int n_planes, const float* row_l1, const float* bias_max,
                                    float* scale_out, void* stream);

/* Several projections of the SAME rows in one launch — the four encoder layers' SCA value projections depend on the
 * camera features only (spatial_cross_attention.py:366 in each of the 4 layers): weight_packed = pack of the
 * (n_planes * plane_cols, K) stacked weights, group_bias[s] (bias_groups, n_planes * plane_cols); projection p writes
 * plane p of `out` (planes plane_stride elements apart, rows of ldo elements, plane_cols columns; fp16 when out_f16) just
 * as the single-projection calls above would.  The column blocks of a row block are dealt to one XCD back to back: the
 * feature maps are read from HBM once instead of once per layer.  plane_cols % 256 == 0, otherwise OCC_E_UNSUPPORTED.
 * out_scale: NULL, or n_planes DEVICE floats: plane p is multiplied by out_scale[p] before it is stored (abi 2).
 * out_f16: 0 = f32 rows, 1 = fp16 pixel pairs, 2 = q16 pixel pairs (abi 3). */
int occ_value_proj_bf16_planes(int n_segments, const void* const* a, const int64_t* lda, const int64_t* rows,
                               const int64_t* rows_per_group, const int64_t* out_row0,
                               const float* const* group_bias, int bias_groups, const void* weight_packed, void* out,
                               int out_f16, int64_t ldo, int K, int n_planes, int plane_cols, int64_t plane_stride,
                               int64_t out_group_rows, const float* out_scale, void* stream);

/* ResNet stem in one launch (outside the hand-written hot path):
 *   out = max_pool2d(relu(conv2d(x, W 7x7, stride 2, pad 3) + bias), kernel 3, stride 2, pad 1)
 * x (batch, 3, H, W) f32 NCHW (rounded to bf16 while staged) ; weight_frag = occ_mfma_pack_b_frag_bf16 of the
 * (64, 224) matrix W2[co][ky*32 + kx*4 + c] = W[co][c][ky][kx] (zero at kx = 7 and c = 3) ; bias (64) f32 ;
 * out (batch, Hp, Wp, 64) bf16 NHWC with Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (same for W).
 */
int occ_stem_conv7x7_pool_f32_bf16(const float* x, const void* weight_frag, const float* bias, void* out,
                                   int batch, int H, int W, void* stream);
/* The same stem fed with the RAW camera images: x (batch, Hs, Ws, 3) uint8 HWC; the pipeline's
 * NormalizeMultiviewImage ((x[to_rgb ? 2-c : c] - mean[c]) / std[c], float32) and PadMultiViewImage (zeros to
 * H x W) — reference P/datasets/pipelines/transform_3d.py:31-45,82-94 — run while the input tile is staged.
 * mean, std: 3 HOST floats each (network channel order). */
int occ_stem_conv7x7_pool_u8_bf16(const uint8_t* x, const void* weight_frag, const float* bias, void* out,
                                  int batch, int Hs, int Ws, int H, int W, const float* mean,
                                  const float* std, int to_rgb, void* stream);

/* The reference's TRAINING input from raw frames in one pass (bevformer_base_occ.py:153-164 and use_grid_mask):
 * PhotoMetricDistortionMultiViewImage -> NormalizeMultiviewImage -> PadMultiViewImage -> GridMask
 * (P/datasets/pipelines/transform_3d.py:141-188, :91, :31-43; P/models/utils/grid_mask.py:84-124), float32 throughout.
 *   x        (n_images, Hs, Ws, 3) uint8 HWC on the device, channels as loaded (BGR); any byte alignment
 *   records  n_images x 8 DEVICE floats, one row per image, the draws of the distortion made on the host:
 *              [0] brightness delta (0 = off)   [1] contrast alpha applied BEFORE the HSV round trip (1 = off)
 *              [2] saturation factor (1 = off)  [3] hue shift in degrees (0 = off)
 *              [4] contrast alpha applied AFTER the round trip (1 = off)
 *              [5..7] perm[3] as 0.f / 1.f / 2.f: output channel c takes channel perm[c] (0 1 2 = off)
 *   out      (n_images, 3, H, W) f32 NCHW, 16-byte aligned; every element is written, rows >= Hs and columns >= Ws are 0
 *   mean, std: 3 HOST floats each, network channel order; to_rgb reverses the channels first; 1 / std is formed in
 *            double and rounded to float, as occ_stem_conv7x7_pool_u8_bf16 forms it
 *   grid_mask: NULL (not applied) or 8 HOST ints (apply, d, l, st_h, st_w, use_h, use_w, mode): GridMask with rotate = 1
 *            and offset = False: the multiplier is 0 inside a band (1 outside), inverted when mode == 1.  With
 *            hh = 3H/2, Y = y + (hh - H)/2 a row is in a band iff use_h, Y - st_h >= 0, (Y - st_h) / d < hh / d and
 *            (Y - st_h) % d < l; columns alike with W, st_w, use_w.
 * The BGR <-> HSV steps restate OpenCV's float path (s = diff / (|v| + FLT_EPSILON), h in degrees, sector table).
 * OCC_E_INVALID before any launch: null / misaligned pointers, H < Hs, W < Ws, zero std, more than 65 535 images,
 * d < 2, l outside [1, d-1], st_h / st_w outside [0, d).  OCC_E_UNSUPPORTED: W % 4 != 0 (one thread stores 4 pixels). */
int occ_train_input_u8_f32(const uint8_t* x, const void* records, float* out, int n_images, int Hs, int Ws, int H,
                           int W, const float* mean, const float* std, int to_rgb, const int32_t* grid_mask,
                           void* stream);

/* Stem tail in one pass: out = max_pool2d(relu(y + bias), kernel 3, stride 2, padding 1) on NHWC bf16
 * (outside the hand-written hot path).  y (batch, H, W, C) bf16 raw convolution output ; bias (C) f32 ;
 * out (batch, (H-1)/2+1, (W-1)/2+1, C) bf16.  Needs C % 8 == 0.
 */
int occ_bias_relu_maxpool_nhwc_bf16(const void* y, const float* bias, void* out, int batch, int H, int W, int C,
                                    void* stream);

/* Backbone 1x1 convolution on NHWC bf16 (outside the hand-written hot path, like the call above):
 * out[(n,yo,xo), co] = relu?( sum_ci x[(n, yo*stride, xo*stride), ci] * weight[co, ci] + bias[co]
 *                             (+ residual[(n,yo,xo), co]) ), bf16 in, f32 accumulate, bf16 out.
 *   x (batch, Hin, Win, Cin) bf16 ; weight = occ_mfma_pack_b_frag_bf16 of the (Cout, Cin) matrix (MFMA
 *   B-fragment order, read straight from global memory) ; bias (Cout) f32 ; residual / out
 *   (batch, Hout, Wout, Cout) bf16 with Hout = (Hin-1)/stride + 1.  Needs Cin % 32 == 0, Cout % 32 == 0.
 *   residual_upsample2 != 0: residual is (batch, Hout/2, Wout/2, Cout) and is added nearest-upsampled x2 (the FPN
 *   top-down path: lateral conv + F.interpolate(coarser, nearest) in one launch; Hout, Wout even).
 */
int occ_conv1x1_nhwc_bf16(const void* x, const void* weight, const float* bias, const void* residual,
                          void* out, int batch, int Hin, int Win, int Cin, int Cout, int stride, int relu,
                          int residual_upsample2, void* stream);

/* The same convolution with the kernel forced (tests, probes).  variant: 0 = the launcher's choice from the arguments, as
 * the entry point above; 1 = the tiled kernel (64 pixels x 256 channels per block, K staged in 32-channel chunks);
 * 2 = the activation-resident kernel (the block's pixel tile x Cin stays in LDS for all its output channels: Cin 128, 256
 * or 512, Cout % 128 == 0, Cout <= 4096) with its default tile; 22 / 24 = resident with the 64- / 128-row
 * tile (22: Cin 512 only); 100 * ncb + 22 / 24 also fixes the column blocks per row tile (ncb must
 * divide the number of column passes).  A variant the arguments have no kernel for returns OCC_E_UNSUPPORTED ("no
 * variant") before any launch.  The kernels differ only in f32 summation order; each is deterministic. */
int occ_conv1x1_nhwc_bf16_variant(const void* x, const void* weight, const float* bias, const void* residual,
                                  void* out, int batch, int Hin, int Win, int Cin, int Cout, int stride, int relu,
                                  int residual_upsample2, int variant, void* stream);

/* Training partner of occ_conv1x1_nhwc_bf16 (csrc/conv1x1_wgrad_bf16.hip): weight gradient of the 1x1 convolution,
 *     dw[o][i] = sum over (n, yo, xo) of g[(n, yo, xo), o] * x[(n, yo*stride, xo*stride), i]
 * bf16 in, f32 accumulation on the matrix cores.  g (N, Ho, Wo, Cout) bf16 NHWC with Ho = (H-1)/stride + 1, x (N, H, W, Cin)
 * bf16 NHWC, both 4-byte aligned; dw (Cout, Cin) contiguous, f32 or (dw_bf16 != 0) bf16, overwritten, not accumulated.
 * Needs Cin % 32 == 0, Cout % 32 == 0, both <= 2048, stride 1 or 2, otherwise OCC_E_UNSUPPORTED (and
 * ..._workspace_bytes() == 0): the caller keeps ATen's convolution_backward.
 * The pixel dimension is reduced in `splits` ranges into `workspace` (occ_conv1x1_wgrad_workspace_bytes(...) bytes for the
 * SAME arguments, owned by the caller, 8-byte aligned; every byte of it that is read has been written by this call) and
 * the partial sums are added in a fixed order: the result is deterministic, no float atomics.  splits: 0 = the launcher's
 * choice (enough blocks for 256 CUs), > 0 = at most that many equal ranges (ceil(pixels / splits) pixels each, as many as cover the pixels; at most
 * min(pixels, 4096); tests, probes), < 0 OCC_E_INVALID.
 * Argument checks run before any launch.  Replaces: the weight half of ATen's convolution_backward (MIOpen / CK) behind
 * ConvBNActFunction.  The input gradient needs no entry point at stride 1: gx = occ_conv1x1_nhwc_bf16(g, pack(W^T)). */
int64_t occ_conv1x1_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride, int splits);
int occ_conv1x1_wgrad_nhwc_bf16(const void* g, const void* x, void* dw, int dw_bf16, void* workspace, int N, int H, int W,
                                int Cin, int Cout, int stride, int splits, void* stream);

/* Training partner of occ_conv3x3_nhwc_bf16 (csrc/conv3x3_wgrad_bf16.hip): weight gradient of the 3x3 / pad 1 convolution,
 *     dw[o][ky][kx][i] = sum over (n, yo, xo) of g[(n, yo, xo), o] * x[(n, yo*stride + ky - 1, xo*stride + kx - 1), i]
 * (terms outside the map are zero).  bf16 in, f32 accumulation on the matrix cores.  g (N, Ho, Wo, Cout) bf16 NHWC with
 * Ho = (H-1)/stride + 1, x (N, H, W, Cin) bf16 NHWC, both 4-byte aligned; dw in memory order [Cout][3][3][Cin] (torch: a
 * (Cout, Cin, 3, 3) tensor in channels_last strides), f32 or (dw_bf16 != 0) bf16, overwritten, not accumulated.
 * Needs Cin % 32 == 0, Cout % 32 == 0, both <= 2048, stride 1 or 2, otherwise OCC_E_UNSUPPORTED (and
 * ..._workspace_bytes() == 0): the caller keeps ATen's convolution_backward.
 * The output rows (n, yo) are reduced in `splits` ranges of whole rows into `workspace` (occ_conv3x3_wgrad_workspace_bytes(...)
 * bytes for the SAME arguments, owned by the caller, 8-byte aligned; every byte of it that is read has been written by this
 * call) and the partial sums are added in a fixed order: the result is deterministic, no float atomics.  splits: 0 = the
 * launcher's choice (about one block per CU), > 0 = that many balanced ranges, splits * 9 * Cout * Cin * 4 bytes (at most
 * min(N * Ho, 4096) ranges; tests, probes), < 0 OCC_E_INVALID.
 * A non-finite x value enters only the taps whose exact sum contains it; a non-finite g value at a pixel next to the map's
 * border also makes the taps that fall outside the map there NaN (they are g * 0): exact border taps need finite g.
 * Argument checks run before any launch.  Replaces: the weight half of ATen's convolution_backward (MIOpen / CK) behind
 * ConvBNActFunction.  The input gradient needs no entry point at stride 1: gx = occ_conv3x3_nhwc_bf16(g, pack(Wd)) with
 * Wd[i][o][ky][kx] = W[o][i][2-ky][2-kx]. */
int64_t occ_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride, int splits);
int occ_conv3x3_wgrad_nhwc_bf16(const void* g, const void* x, void* dw, int dw_bf16, void* workspace, int N, int H, int W,
                                int Cin, int Cout, int stride, int splits, void* stream);

/* Backbone 3x3 pad-1 convolution, stride 1 or 2, on NHWC bf16 with bias (+ ReLU) fused (outside the
 * hand-written hot path).  x (batch, H, W, Cin) bf16 ; weight packed by occ_conv3x3_pack_weight_bf16 from
 * torch's (Cout, Cin, 3, 3) f32 layout to [Cin/32][tap][co][32] bf16 ; bias (Cout) f32 ;
 * out (batch, (H-1)/stride+1, (W-1)/stride+1, Cout) bf16.
 * Needs Cin % 32 == 0, Cout % 128 == 0, stride in {1, 2}, otherwise OCC_E_UNSUPPORTED (the caller keeps MIOpen).
 */
int occ_conv3x3_pack_weight_bf16(const float* weight, void* packed, int Cout, int Cin, void* stream);
int occ_conv3x3_nhwc_bf16(const void* x, const void* weight_packed, const float* bias, void* out, int batch,
                          int H, int W, int Cin, int Cout, int stride, int relu, void* stream);
/* The same convolution; additionally folds max|out| (the sign-stripped bf16 pattern of every element it stores) into the
 * 8 DEVICE words amax8 with atomic maxima.  The words ACCUMULATE across launches: zero them once in front of the FPN's
 * output convolutions (the maps the reference flattens at transformer_occ.py:204-222), then hand them to
 * occ_value_range_scale_from_amax. */
int occ_conv3x3_nhwc_bf16_amax(const void* x, const void* weight_packed, const float* bias, void* out, int batch,
                               int H, int W, int Cin, int Cout, int stride, int relu, uint32_t* amax8, void* stream);
/* Either of the two with the tile forced (tests, probes): variant = 10 * NT + RT, a block of 4 waves computes
 * (2 * RT) x 16 output pixels x (128 * NT) channels; stride 1 has 12, 13, 14, 16, 18, 22, 23, 24, stride 2 has 12, 13,
 * 22 (NT 2 needs Cout % 256 == 0); 0 lets the launcher choose from the shape as the two entry points above do.  amax8
 * may be NULL (no max|out|).  A variant the shape lacks returns OCC_E_UNSUPPORTED.  Variants differ from each other only
 * in f32 summation order. */
int occ_conv3x3_nhwc_bf16_variant(const void* x, const void* weight_packed, const float* bias, void* out, int batch,
                                  int H, int W, int Cin, int Cout, int stride, int relu, uint32_t* amax8, int variant,
                                  void* stream);

/* A 3x3 convolution and the 1x1 expansion after it (ResNet bottleneck conv2 + conv3) in one launch; the mid tensor stays
 * in LDS (csrc/conv3x3_conv1x1_fused_bf16.hip):
 *   out = relu( conv1x1( bf16( relu(conv3x3(x, W2, pad 1, stride) + b2) ), W3 ) + b3 + residual )
 *   x (batch, H, W, Cmid) bf16 ; w3x3_packed = occ_conv3x3_pack_weight_bf16 of W2 (Cmid, Cmid, 3, 3) ; b2 (Cmid) f32 ;
 *   w1x1_frag = occ_mfma_pack_b_frag_bf16 of W3 (Cout, Cmid) ; b3 (Cout) f32 ; residual / out (batch, Ho, Wo, Cout) bf16,
 *   Ho = (H-1)/stride + 1.  Needs Cmid 128 or 256, Cout = 4 Cmid, stride 1 or 2, otherwise OCC_E_UNSUPPORTED.
 * variant: the 3x3 tile id (10 * NT + RT, as occ_conv3x3_nhwc_bf16_variant) the block uses; it must hold all mid channels
 * (Cmid 128: 12, and 13 at stride 2; Cmid 256: 22, and 23, 24 at stride 1).  0 = the tile occ_conv3x3_conv1x1_pick returns, and
 * OCC_E_UNSUPPORTED where that is 0.  For a tile id the result is bit-identical to occ_conv3x3_nhwc_bf16_variant with that
 * id followed by occ_conv1x1_nhwc_bf16_variant 2.  Argument checks run before any launch. */
int occ_conv3x3_conv1x1_nhwc_bf16(const void* x, const void* w3x3_packed, const float* b2, const void* w1x1_frag,
                                  const float* b3, const void* residual, void* out, int batch, int H, int W, int Cmid,
                                  int Cout, int stride, int variant, void* stream);
/* The tile id the entry point above uses for a shape at variant 0, or 0 when the shape should stay on the two launches
 * (no fused kernel, or too few tiles to give every CU a block).  A pure function of its arguments; needs no GPU. */
int occ_conv3x3_conv1x1_pick(int batch, int H, int W, int Cmid, int Cout, int stride);

/* MFMA B-operand packing: f32 row-major (N, K) matrix -> bf16 in v_mfma_f32_32x32x16_bf16 fragment order
 * packed[((ks * N/32 + nt) * 64 + lane) * 8 + j] = w[nt*32 + (lane & 31)][ks*16 + (lane >> 5)*8 + j], so a wave
 * loads its operand of (k-step ks, column tile nt) as one coalesced 1 KB read.  Needs N % 32 == 0, K % 16 == 0.
 */
int occ_mfma_pack_b_frag_bf16(const float* weight, void* packed, int N, int K, void* stream);

/* One whole 64-mid-channel ResNet bottleneck (mmdet Bottleneck, style='pytorch', stride 1, eval BatchNorm
 * folded; outside the hand-written hot path) on NHWC bf16 in ONE launch — the 64-channel intermediates stay in
 * LDS:  out = relu( conv1x1( relu(conv3x3( relu(conv1x1(x,W1)+b1), W2)+b2), W3) + b3 + identity ).
 *   x (batch, H, W, Cin) bf16 ; out (batch, H, W, 256) bf16 ; b1, b2 (64) f32 ; b3 (256) f32
 *   w1_frag = pack_b_frag(W1 (64, Cin)) ; w2_frag = pack_b_frag(W2 as (64, 9*64) with k = (ky*3+kx)*64 + ci)
 *   downsample == 0 (Cin == 256): identity = x,  w3_frag = pack_b_frag(W3 (256, 64))
 *   downsample == 1 (Cin == 64):  identity = conv1x1(x, Wds) + bds,  w3_frag = pack_b_frag([W3 | Wds] (256, 128)),
 *                                 b3 := b3 + bds
 * Other channel counts: OCC_E_UNSUPPORTED (the caller keeps the per-layer kernels).
 */
int occ_bottleneck64_nhwc_bf16(const void* x, const void* w1_frag, const float* b1, const void* w2_frag,
                               const float* b2, const void* w3_frag, const float* b3, void* out, int batch,
                               int H, int W, int Cin, int downsample, void* stream);

/* The same bottleneck with the kernel forced (tests, probes).  variant: 0 = the launcher's choice, as the entry point above
 * (the second kernel; OCC_BOTTLENECK64_V2=0 in the environment, read once, keeps the first); 1 = the first kernel (f32 LDS
 * transpose in the epilogue, identity read from x a second time, block b computes tile b); 2 = the second kernel
 * (csrc/bottleneck64_v2_nhwc_bf16.hip: identity kept in registers from the staged tile, x read once) with its default
 * tile order, 0 (OCC_BOTTLENECK64_ORDER=0 / 1 / 2, read once, overrides it); 3 / 4 / 5 = the second kernel with tile
 * order 0 / 1 / 2 of occ_bottleneck64_tile_of_block (1, 2: XCD-local, fewer bytes fetched, measured slower).  Every
 * variant computes the same bits.  An unknown variant returns OCC_E_UNSUPPORTED ("no variant"); argument checks run
 * before any launch. */
int occ_bottleneck64_nhwc_bf16_variant(const void* x, const void* w1_frag, const float* b1, const void* w2_frag,
                                       const float* b2, const void* w3_frag, const float* b3, void* out, int batch,
                                       int H, int W, int Cin, int downsample, int variant, void* stream);
/* The tile (row-major linear index over image, tile row, tile column; 8 x 16 pixel tiles) that block `block` of a grid of
 * n_blocks = batch * tiles_y * tiles_x blocks computes in the second kernel.  Blocks b, b + 8, b + 16, ... run on one XCD
 * (one L2).  order 0: tile = block.  order 1: group b % 8 takes a contiguous range of the row-major walk, position
 * x*q + min(x, r) + b / 8 with x = b % 8, q = n / 8, r = n % 8.  order 2: the same ranges of a walk that goes through each
 * image in bands of 4 tile rows, column by column inside a band.  A permutation of 0 .. n_blocks - 1 for every order; a
 * pure function, needs no GPU.  Bad arguments: OCC_E_INVALID (negative). */
int occ_bottleneck64_tile_of_block(int block, int n_blocks, int tiles_x, int tiles_y, int order);

/* The last identity bottleneck (Cin 256) of a stage whose output only feeds the next stage's first block, with that block's
 * two pointwise readers computed on the tile before it leaves the CU (csrc/bottleneck64_next_nhwc_bf16.hip); the
 * 256-channel map out = bottleneck64(x) is NOT written:
 *   y        = relu( conv1x1(out, W1n) + b1n )            (batch, H, W, cmid_next) bf16
 *   shortcut = conv1x1(out, Wds, stride 2) + bds          (batch, (H-1)/2+1, (W-1)/2+1, 4 cmid_next) bf16
 *   x (batch, H, W, 256) bf16 ; w1_frag .. b3 as occ_bottleneck64_nhwc_bf16 with downsample == 0 ;
 *   next_w1_frag = occ_mfma_pack_b_frag_bf16 of W1n (cmid_next, 256) ; next_b1 (cmid_next) f32 ;
 *   next_wds_frag = occ_mfma_pack_b_frag_bf16 of Wds (4 cmid_next, 256) ; next_bds (4 cmid_next) f32.
 * cmid_next must be 128, otherwise OCC_E_UNSUPPORTED.  Bit-identical to occ_bottleneck64_nhwc_bf16_variant 2 followed by
 * occ_conv1x1_nhwc_bf16_variant 2 with relu = 1 and by occ_conv1x1_nhwc_bf16_variant 2 with stride = 2, for every shape.
 * Argument checks run before any launch. */
int occ_bottleneck64_next_nhwc_bf16(const void* x, const void* w1_frag, const float* b1, const void* w2_frag,
                                    const float* b2, const void* w3_frag, const float* b3, const void* next_w1_frag,
                                    const float* next_b1, const void* next_wds_frag, const float* next_bds, void* y,
                                    void* shortcut, int batch, int H, int W, int cmid_next, void* stream);
/* Non-zero where a plan should take the entry point above for a (batch, H, W, 256) map: a kernel exists for cmid_next and
 * BOTH 1x1 launches it replaces would run the activation-resident kernel under occ_conv1x1_nhwc_bf16's default rule
 * (M >= 512 at full resolution and at stride 2), so that the fused launch returns the bits of the route it replaces.
 * A pure function of its arguments; needs no GPU. */
int occ_bottleneck64_next_pick(int batch, int H, int W, int cmid_next);

/* ------------------------------------------------------------------------------------------
 * (e) Evaluation: RayIoU / mAVE counters of a batch of samples in one fused pass (csrc/ray_metrics_fused.hip) — the
 * reference's process_one_sample + main's non-free filter + calc_metrics (projects/mmdet3d_plugin/datasets/
 * ray_metrics.py:89-257) without a host round trip: occupancy bit masks per pillar, the "test"-phase ray cast of
 * occ_dvr_render_forward_f32 on the ground-truth and on the predicted grid, and the per-class scoring.
 *   sem_pred, sem_gt (B, X, Y, Z) class ids, dtype code 0 = uint8, 1 = int64 (each grid its own); a voxel is occupied
 *                    iff its class != free_id; classes outside 0..free_id are occupied and counted in no class
 *   flow_pred, flow_gt (B, X, Y, Z, 2) f32
 *   origins (B, Tmax, 3) f32 lidar origins in ego metres, 1 <= Tmax <= 8; origin_counts (B) i32 DEVICE, origins of
 *                    sample b beyond origin_counts[b] are not cast (NULL: every sample has Tmax)
 *   rays (R, 3) f32 unit directions; off_x/y/z = pc_range[:3], voxel_size: (p - off) / voxel_size in float32
 *   state            occ_ray_metrics_state_words(free_id) = 14 * (free_id + 1) int64 words, ACCUMULATED into (the
 *                    caller zeroes them once): gt_cnt[c] | pred_cnt[c] | tp_cnt[j][c] | ave_cnt[j][c] | ave_sum[j][c] |
 *                    ave_bad[j][c], c = class, j = depth threshold 1 / 2 / 4 m.  ave_sum: flow errors of the true
 *                    positives of classes 0..7 in fixed point, quantum 2^-28 m/s (sums below 2^35 m/s); ave_bad counts
 *                    the non-finite (or >= 2^34 m/s) errors, which are left out of ave_sum.  Integer atomics only: the
 *                    state is bit-identical run to run and for any split of the samples over calls.
 *   rows_pred, rows_gt NULL, or (B, Tmax, R, 4) f32 out: (label, depth [m], flow_x, flow_y) per ray in
 *                    process_one_sample's order; rows of origins beyond origin_counts[b] are not written.  When given,
 *                    every ray is cast on both grids; otherwise the prediction cast of a ray whose ground truth is free
 *                    is skipped (the state is the same).
 *   workspace        occ_ray_metrics_workspace_bytes(B, X, Y, Z) bytes, 256-byte aligned, uninitialised: the pillar masks
 *                    (uint16 for Z <= 16, uint32 for Z <= 32) of both grids.  Z > 32: OCC_E_UNSUPPORTED (query: 0).
 * free_id in 1..31.  Two launches, no synchronisation, no allocation, no copy.
 */
int64_t occ_ray_metrics_state_words(int free_id);
int64_t occ_ray_metrics_workspace_bytes(int B, int X, int Y, int Z);
int occ_ray_metrics_accumulate(const void* sem_pred, int sem_pred_dtype, const float* flow_pred,
                               const void* sem_gt, int sem_gt_dtype, const float* flow_gt,
                               const float* origins, const int32_t* origin_counts, const float* rays,
                               float off_x, float off_y, float off_z, float voxel_size, int free_id,
                               int64_t* state, float* rows_pred, float* rows_gt, void* workspace,
                               int64_t workspace_bytes, int B, int Tmax, int X, int Y, int Z, int R,
                               void* stream);

/* Submission rows of a batch of predictions in one launch pair (csrc/submission_rays.hip) — the per-sample loop of the
 * reference's format_results (projects/mmdet3d_plugin/datasets/nuscenes_occ.py:217-241: process_one_sample, then
 * astype(np.int8) / astype(np.float16)) without a host round trip: occupancy bit masks of the prediction, the ray cast of
 * occ_ray_metrics_accumulate (the same text: csrc/ray_cast.h), class / flow read at the reported voxel, packed.
 *   sem_pred (B, X, Y, Z) class ids, dtype code 0 = uint8, 1 = int64; flow_pred (B, X, Y, Z, 2) f32
 *   origins (B, Tmax, 3) lidar origins in ego metres, 1 <= Tmax <= 8, origins_dtype 0 = float32, 1 = float64.  The
 *                    conversion to voxel units follows the type as process_one_sample's tensor arithmetic does: float32
 *                    origins -> float32 `ray + origin` and `(p - off) / voxel_size`, exactly as occ_ray_metrics_accumulate;
 *                    float64 origins (what the reference's EgoPoseDataset yields) -> those statements in float64, rounded to
 *                    float32 once.
 *   origin_counts (B) i32 DEVICE or NULL, rays (R, 3) f32, off_x/y/z, voxel_size, free_id in 1..31: as above
 *   out              occ_submission_rays_bytes(B, Tmax, R) bytes, 4-byte aligned: three sections, each starting on a
 *                    256-byte boundary, N = B * Tmax * R rows, row (b * Tmax + t) * R + r (process_one_sample's order):
 *                      cls  int8[N]     at 0                             low 8 bits of the class id: ids 0..127 are what
 *                                       the host path defines; above that the C cast behind numpy's astype(np.int8) is
 *                                       undefined — the rule HERE is two's-complement wrap (200 -> -56)
 *                      dist fp16[N]     at align256(N)                   float32(distance * voxel_size) rounded to nearest
 *                                       even, overflow -> inf; a ray that never enters the grid: -1 * voxel_size, voxel (0,0,0)
 *                      flow fp16[N][2]  at align256(N) + align256(2 N)   rounded the same way
 *                    rows of origins beyond origin_counts[b] are NOT written.
 *   workspace        occ_submission_rays_workspace_bytes(B, X, Y, Z) bytes, 4-byte aligned, uninitialised: the prediction's
 *                    pillar masks (uint16 for Z <= 16, uint32 for Z <= 32).  Z > 32: OCC_E_UNSUPPORTED (both queries that
 *                    take Z answer 0).
 * Two launches on `stream`, no synchronisation, no allocation, no copy.  Every argument is checked before the first launch.
 */
int64_t occ_submission_rays_bytes(int B, int Tmax, int R);
int64_t occ_submission_rays_workspace_bytes(int B, int X, int Y, int Z);
int occ_submission_rays(const void* sem_pred, int sem_pred_dtype, const float* flow_pred, const void* origins,
                        int origins_dtype, const int32_t* origin_counts, const float* rays, float off_x, float off_y,
                        float off_z, float voxel_size, int free_id, void* out, int64_t out_bytes, void* workspace,
                        int64_t workspace_bytes, int B, int Tmax, int X, int Y, int Z, int R, void* stream);

/* Score of submission rows as the challenge server computes it (csrc/submission_score.hip) — the reference's stand-alone
 * scorer tools/ray_iou/metric.py:calc_metrics (:31-73) over B samples of per-ray rows, without a host round trip.  It differs
 * from occ_ray_metrics_accumulate's scorer in what it reads (the rows of the file: int8 class, float16 depth and flow) and in
 * its AVE rule: once a flow class (c < 8) has any true positive in a sample at a threshold, the flow error of EVERY valid ray
 * of that sample is added, and the count of all those rays (metric.py:70-73).
 *   pred_format, gt_format   0 = the packed sections of occ_submission_rays: *_cls int8[N], *_dist fp16[N] (2-byte aligned),
 *                    *_flow fp16[N][2] (4-byte aligned);  1 = float32 rows (N, 4) = [class, dist, flow_x, flow_y] in *_cls,
 *                    16-byte aligned (*_dist / *_flow are not read): the class is truncated toward zero as astype(np.int32)
 *                    does; a class value that is NaN, infinite or beyond int32 counts as an out-of-range class.
 *   counts (B) i32 DEVICE: sample b owns rows [b * stride, b * stride + counts[b]) of both sides (for the writer's buffers
 *                    stride = Tmax * R, counts[b] = origin_counts[b] * R); clamped to 0 .. stride; rows beyond are never read
 *                    into the score.  Both sides hold B * stride rows.
 *   a ray is valid iff gt_cls != free_id; classes outside 0..free_id match no class (the ray stays valid); depth thresholds
 *   1 / 2 / 4 m on the float32 |pred_dist - gt_dist|, strictly below; err = sqrtf(ux * ux + uy * uy) in float32, uncontracted.
 *   state            occ_submission_score_state_words(free_id) = 17 * (free_id + 1) int64 words, ACCUMULATED into (the caller
 *                    zeroes them once): gt_cnt[c] | pred_cnt[c] | tp[j][c] | ave_cnt[j][c] | ave_sum[j][c] | ave_inf[j][c] |
 *                    ave_nan[j][c].  ave_sum: fixed point, quantum 2^-28 m/s (sums below 2^35 m/s: the full validation split
 *                    fits while the mean flow error over its valid rays stays below 50 m/s).  A NaN error adds 1 to ave_nan,
 *                    an infinite one (or one >= 2^34 m/s) 1 to ave_inf, instead of to ave_sum; both count in ave_cnt.  Integer
 *                    atomics only: the state is bit-identical run to run and for any split of the samples over calls.
 *   workspace        occ_submission_score_workspace_bytes(B) bytes, 8-byte aligned, uninitialised: the per-block records.
 *   max_chunks       0 = the launcher's grid (one block per 1024 rows of stride, at most 128 per sample); > 0 caps the blocks
 *                    per sample (1: one block per sample); < 0 OCC_E_INVALID.  The state does not depend on it.
 * free_id in 1..31, 1 <= B <= 65535.  Two launches on `stream`, no synchronisation, no allocation, no copy.  Every argument is
 * checked before the first launch.
 */
int64_t occ_submission_score_state_words(int free_id);
int64_t occ_submission_score_workspace_bytes(int B);
int occ_submission_score_accumulate(int pred_format, const void* pred_cls, const void* pred_dist, const void* pred_flow,
                                    int gt_format, const void* gt_cls, const void* gt_dist, const void* gt_flow,
                                    const int32_t* counts, int free_id, int64_t* state, void* workspace,
                                    int64_t workspace_bytes, int B, int64_t stride, int max_chunks, void* stream);

/* Pictures of a batch of class grids, rendered on the device (csrc/occ_render.hip): pin-hole camera views and a bird's-eye
 * view as label / depth / colour images.  No counterpart in the reference that runs (its utils/vis.py needs Open3D and stops on
 * an undefined name).  A camera pixel is one ray through the caster of occ_ray_metrics_accumulate / occ_submission_rays (the
 * same text: csrc/ray_cast.h), so it reports the voxel and the distance those report for that ray.
 *   sem (B, X, Y, Z) class ids, dtype code 0 = uint8, 1 = int64; sem_gt NULL, or the ground truth in the same layout (its own
 *                    dtype code): DIFF MODE, below
 *   cams (B, V, 12) f32: per view the camera centre o[3] in ego metres, then a row-major 3 x 3 matrix D with
 *                    ego point = o + depth * D (px, py, 1)^T for the pixel centre (px, py) of the RENDERED image
 *   frames NULL, or (B, V, Hs, Ws, 3) u8 HWC: the background, sampled nearest; Hs, Ws are read only with frames
 *   palette (256, 3) u8 DEVICE (needed with rgb); cat_palette (6, 3) u8 DEVICE (needed with rgb and sem_gt)
 *   off_x/y/z = pc_range[:3], voxel_size > 0, free_id in 1..31, far > 0 (metres: the length of a ray in units of (px, py, 1)
 *                    depth), tol >= 0 (metres), alpha in 0..256, bg_rgb = 0xRRGGBB (the background without frames)
 *   label u8 (B, V, h, w), depth f32 (B, V, h, w), rgb u8 (B, V, h, w, 3): each may be NULL, not all three
 * ARITHMETIC CONTRACT of pixel (i, j), float32, uncontracted, in this order:
 *   px = (float)j + 0.5f, py = (float)i + 0.5f;  dir_k = (D[k][0] * px + D[k][1] * py) + D[k][2];  ray_k = dir_k * far;
 *   end = ray + o, origin and end to voxel units as (p - off) / voxel_size (float32, as occ_ray_metrics_accumulate); the
 *   "test"-phase traversal -> voxel (x, y, z), dist;  depth = dist * voxel_size;  class = sem[b][x][y][z].
 *   HIT iff dist >= 0 and class != free_id (a ray that never enters the grid reports voxel (0, 0, 0), dist -1: a miss).
 *   label = hit ? class & 0xff : free_id;  depth = hit ? depth : -1
 *   rgb[k]: bg = frames ? frames[b][v][((2 i + 1) Hs) / (2 h)][((2 j + 1) Ws) / (2 w)][k] : byte k of bg_rgb;
 *           shade = 256 - (int)fminf((depth * 192.0f) / far, 192.0f);  lit = (palette[label][k] * shade) >> 8;
 *           hit ? (lit * alpha + bg * (256 - alpha)) >> 8 : bg            (integer arithmetic after the one truncation)
 * DIFF MODE: the ray is cast through both grids; `label` holds a category: 0 both miss, 1 both hit with the same class and
 *   fabsf(depth_pred - depth_gt) < tol, 2 same class but depth off, 3 both hit and the class differs, 4 only the prediction
 *   hits, 5 only the ground truth hits.  `depth` stays the prediction's.  rgb: category 0 -> bg; 1 -> palette[class_gt & 0xff],
 *   2..5 -> cat_palette[category]; shaded by the prediction's depth (category 5: the ground truth's), blended as above.
 * occ_render_bev: one pixel per pillar in grid order, label u8 (B, X, Y), rgb u8 (B, X, Y, 3), each may be NULL, not both.
 *   top = highest occupied z of the pillar; label = class(x, y, top) & 0xff, rgb[k] = (palette[label][k] * (128 + (128 * (top +
 *   1)) / Z)) >> 8; an empty pillar: label = free_id, rgb = bg_rgb.  With sem_gt the categories are 0 both empty, 1 same class
 *   and same top, 2 same class and another top, 3 class differs, 4 prediction only, 5 ground truth only, coloured as above
 *   (shade from the prediction's top, category 5: the ground truth's).
 *   workspace        occ_render_workspace_bytes(B, X, Y, Z, diff) bytes, 4-byte aligned, uninitialised: the pillar masks (uint16
 *                    for Z <= 16, uint32 for Z <= 32) of the prediction and, with diff != 0, of the ground truth.  Z > 32:
 *                    OCC_E_UNSUPPORTED, reported before the pointer checks (query: 0).
 * OCC_E_INVALID with a message that names the argument: a NULL sem / cams / workspace, no output, a missing palette, a
 * non-positive size (B * V <= 65535; h, w, Hs, Ws <= 16384), a dtype code, free_id, bg_rgb, voxel_size, far <= 0, tol < 0, alpha
 * outside 0..256, a workspace that is too small or misaligned.  Each call: one mask launch + one render launch on `stream`, no
 * synchronisation, no allocation, no copy; every argument is checked before the first launch.
 */
int64_t occ_render_workspace_bytes(int B, int X, int Y, int Z, int diff);
int occ_render_views(const void* sem, int sem_dtype, const void* sem_gt, int sem_gt_dtype, const float* cams,
                     const uint8_t* frames, int Hs, int Ws, const uint8_t* palette, const uint8_t* cat_palette,
                     float off_x, float off_y, float off_z, float voxel_size, int free_id, float far, float tol,
                     int alpha, int bg_rgb, uint8_t* label, float* depth, uint8_t* rgb, void* workspace,
                     int64_t workspace_bytes, int B, int V, int X, int Y, int Z, int h, int w, void* stream);
int occ_render_bev(const void* sem, int sem_dtype, const void* sem_gt, int sem_gt_dtype, const uint8_t* palette,
                   const uint8_t* cat_palette, int free_id, int bg_rgb, uint8_t* label, uint8_t* rgb, void* workspace,
                   int64_t workspace_bytes, int B, int X, int Y, int Z, void* stream);

/* ------------------------------------------------------------------------------------------
 * (f) Training tail: both occupancy heads AND their losses as one node (csrc/occ_heads_loss.hip) — the reference's
 * predicter / flow_predicter (transformer_occ.py:132-141,318-319) followed by BEVFormerOccHead.loss / loss_single
 * (bevformer_occ_head.py:163-196: CrossEntropyLoss on the logits, L1Loss on the flow) and the autograd graph between
 * them.  Nothing but the inputs is kept between forward and backward: the backward recomputes each 32-voxel tile.
 *   feat (n_rows, 32) f32, 16-byte aligned; the eight head tensors of occ_occ_heads_f32
 *   labels (n_rows) class ids, dtype code 0 = uint8, 1 = int64; flow_gt (n_rows, 2) f32
 *   mask NULL or (n_rows) bool bytes: multiplies the cross-entropy terms; class_weight NULL or (num_classes) f32
 *   a voxel whose label equals ignore_index contributes 0 to loss_occ — and so does a label outside [0, num_classes)
 *   (DEVIATION: torch raises a device assert there; nothing is read through such a label).  The flow term is unmasked.
 *   Denominators (bricks.CrossEntropyLoss / L1Loss): occ — mask.sum() when a mask is given (either reduction: the
 *   avg_factor rule; 0 / 0 stays NaN), else n_rows for reduction_mean = 1 and 1 for 0; flow — 2 n_rows or 1.
 *   Loss weights stay with the caller.
 * forward:  losses[0] = loss_occ, losses[1] = loss_flow, losses[2] = the occ denominator (three DEVICE floats; heads in
 *   bf16x3 arithmetic as occ_occ_heads_decode_f32(exact_f32 = 0)); one launch + a one-wave finalise.
 * backward: grad_losses = the two incoming gradient scalars, occ_denom = losses + 2 of the forward, both DEVICE
 *   pointers (no host synchronisation); dfeat (n_rows, 32) fully written, or NULL; each of the eight parameter gradients
 *   fully written, or NULL (all NULL: the weight-gradient products are skipped).  Exact f32 (v_mfma_f32_32x32x2_f32); one
 *   launch + a small reduce; no float atomics: bit-identical run to run.
 * workspace: occ_heads_loss_workspace_bytes(n_rows, num_classes, max_blocks) bytes, 16-byte aligned, uninitialised (0:
 *   unsupported or invalid arguments).  max_blocks: 0 = the launcher's grid, > 0 caps the grid of every launch (a small
 *   cap makes each wave walk several tiles: tests), < 0 OCC_E_INVALID.  The grids depend on n_rows and max_blocks only.
 * C == 32, hidden == 64, num_classes + 2 <= 32, otherwise OCC_E_UNSUPPORTED.  Argument checks precede every launch; no
 * allocation; everything on `stream`.
 */
int64_t occ_heads_loss_workspace_bytes(int64_t n_rows, int num_classes, int max_blocks);
int occ_heads_loss_fwd_f32(const float* feat, const float* w1_occ, const float* b1_occ, const float* w2_occ,
                           const float* b2_occ, const float* w1_flow, const float* b1_flow, const float* w2_flow,
                           const float* b2_flow, const void* labels, int labels_dtype, const float* flow_gt,
                           const uint8_t* mask, const float* class_weight, int64_t ignore_index, int reduction_mean,
                           float* losses, void* workspace, int64_t workspace_bytes, int64_t n_rows, int C, int hidden,
                           int num_classes, int max_blocks, void* stream);
int occ_heads_loss_bwd_f32(const float* feat, const float* w1_occ, const float* b1_occ, const float* w2_occ,
                           const float* b2_occ, const float* w1_flow, const float* b1_flow, const float* w2_flow,
                           const float* b2_flow, const void* labels, int labels_dtype, const float* flow_gt,
                           const uint8_t* mask, const float* class_weight, int64_t ignore_index, int reduction_mean,
                           const float* grad_losses, const float* occ_denom, float* dfeat, float* dw1_occ,
                           float* db1_occ, float* dw2_occ, float* db2_occ, float* dw1_flow, float* db1_flow,
                           float* dw2_flow, float* db2_flow, void* workspace, int64_t workspace_bytes, int64_t n_rows,
                           int C, int hidden, int num_classes, int max_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCCNET_AMD_H_ */
