// Backward of the fused temporal self-attention gather (tsa_fused.hip) for gfx950: M = 8, D = 32, P = 4, one BEV level,
// 2-deep queue, no row bands (Nq = bev_h * bev_w).
//
// The forward, per (batch b, BEV query q), head m, sample s = (queue entry t, point p):
//   a_s = softmax over the 4 logits of (m, t),   loc_s = ref_2d[b*2+t][q] + off_s / (W, H)
//   out[b][q][m] = 0.5 * sum_s a_s * bilinear(value[b*2+t][m], loc_s)
// Its gradients for top = 0.5 * grad_out[b][q][m] (the 0.5 is the queue mean), per sample, with the corner rows v1..v4 of
// queue entry t and the bilinear terms of sca_fused_backward.hip's header (out-of-map corners read as 0):
//   dA_s        = sum_ch top_ch * (hh hw v1 + hh lw v2 + lh hw v3 + lh lw v4)
//   grad_off_x  = a_s * sum_ch top_ch * (hh (v2 - v1) + lh (v4 - v3))       (1 / W of the normalisation cancels the W of the
//   grad_off_y  = a_s * sum_ch top_ch * (hw (v3 - v1) + lw (v4 - v2))        pixel coordinate: no scale left)
//   grad_logit  = a_s * (dA_s - sum_p' a_p' dA_p')                          (over the 4 points of the sample's own (m, t))
//   grad_value[b*2+t][corner k][m] += top * a_s * w_k                        (in-range corners)
// A sample whose location is not finite contributes nothing in the forward (it fails the admission test): its dA, its offset
// gradients and its grad_value items are 0, while the other points of its softmax group keep their softmax-backward term.
//
// grad_offs / grad_logits: tsa_bwd_sample_kernel, one 64-lane wave per (b, q).  Set-up lane map of the forward:
// lane = m*8 + t*4 + p owns one sample (softmax = 4-lane shuffle), its corner offsets and fractional weights go to LDS.  Then
// every 8-lane group (one head, 4 channels per lane) walks its head's 8 samples — samples 0-3 in queue entry 0's map, 4-7 in
// entry 1's — takes the dot products of the grad row with the four corner rows and folds the 8 lanes' 3 x 8 partial sums by the
// reduce-scatter shared with sca_fused_backward.hip (gather_pieces.h; xor 4, 2, 1), which leaves lane c4 of the group with
// sample c4 = t*4 + p: the lane that owns that sample's logit and offset pair.  One writer per element, fixed order of every sum: bit-reproducible.
// `order` of the forward only steers locality and is ignored here.
//
// grad_value: no scatter of its own.  The sample kernel writes loc (B*2, Nq, M, 1, P, 2) and attn (B*2, Nq, M, 1, P) in
// ms_deform_attn layout into the workspace, attn = 0.5 * a_s (a dead sample: attn = 0 and the finite out-of-map location
// (-2, -2), so the binning passes never see a NaN or Inf), marks every (b*2+t, q, m) item live, and bwd_bins_replay
// (msda_bwd_bins.h) bins and replays them into grad_value (B*2, S, M, D), reading grad_out rows directly: the grad row of value
// batch entry bv is that of batch bv / 2.  OCC_MSDA_BWD_DETERMINISTIC=1 (read per call) takes the fixed-point replay.
//
// Buffer offsets.  Every value read goes through a buffer resource of exactly map_bytes = bev_h * bev_w * M * D * 4 bytes
// over one queue entry's map (the host checks map_bytes < kOobOffset).  A corner flag c[k] of bilinear_terms is set only if
// the sample is admitted and pixel (h, w) of corner k has 0 <= h < bev_h and 0 <= w < bev_w, so its offset is
// (h * bev_w + w) * 1024 + lane_off with lane_off = (g * 32 + c4 * 4) * 4 <= 1008: the 16 bytes read end at most at
// (bev_h * bev_w - 1) * 1024 + 1024 = map_bytes.  Every other corner carries kOobOffset + lane_off >= map_bytes (no 32-bit
// wrap: 0x7fffff00 + 1008 < 2^32): the load returns 0 and requests nothing.  All other accesses are plain pointers indexed by
// (b, q, lane) inside the documented extents.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 110 VGPRs with all outputs wanted (114 for grad_offs /
// grad_logits alone, 24 and no LDS for the grad_value planes alone), 0 AGPRs, no scratch, 9216 bytes of LDS per 256-thread
// block, 4 waves per SIMD.
#include <cstdlib>
#include "gather_pieces.h"
#include "msda_bwd_bins.h"

namespace occ {

constexpr int kTsaBwdWaves = 4;

// WANT_Q: grad_offs / grad_logits; WANT_V: the loc / attn / flag planes the grad_value replay reads
template <bool WANT_Q, bool WANT_V>
__global__ __launch_bounds__(64 * kTsaBwdWaves) void tsa_bwd_sample_kernel(
    const float* __restrict__ value, long value_bt_stride, const float* __restrict__ offs, long offs_stride,
    const float* __restrict__ logits, long logits_stride, const float* __restrict__ ref_2d,
    const float* __restrict__ grad_out, float* __restrict__ grad_offs, long goffs_stride, float* __restrict__ grad_logits,
    long glogits_stride, float* __restrict__ ws_loc, float* __restrict__ ws_attn, unsigned char* __restrict__ ws_flags,
    int B, int Nq, int bev_h, int bev_w) {
  constexpr int M = 8, D = 32, P = 4, NS = 2 * P;
  constexpr int NSp = NS + 1;
  __shared__ BwdSampleParam smem[kTsaBwdWaves * M * NSp];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long wg = (long)blockIdx.x * kTsaBwdWaves + wave;
  if (wg >= (long)B * Nq) return;
  const int b = (int)(wg / Nq);
  const int q = (int)(wg - (long)b * Nq);
  const long bq = (long)b * Nq + q;
  BwdSampleParam* sp = smem + wave * M * NSp;
  constexpr int row_stride = M * D;

  // ---- set-up map: lane = m*8 + t*4 + p, the memory order of both Linear outputs ------------------------------------------
  const int m = lane >> 3, t = (lane >> 2) & 1, p = lane & 3;
  float aw, lx, ly;
  tsa_lane_setup(logits, logits_stride, offs, offs_stride, ref_2d, bq, lane, b, t, q, Nq, bev_h, bev_w, aw, lx, ly);
  const int finite = lane_flag(fabsf(lx) < __builtin_huge_valf()) & lane_flag(fabsf(ly) < __builtin_huge_valf());
  if (WANT_V) {
    const long item = (((long)b * 2 + t) * Nq + q) * M + m;       // (b*2+t, q, m): ms_deform_attn order, L = 1
    *reinterpret_cast<float2*>(ws_loc + (item * P + p) * 2) = make_float2(finite ? lx : -2.f, finite ? ly : -2.f);
    ws_attn[item * P + p] = finite ? 0.5f * aw : 0.f;
    if (p == 0) ws_flags[item] = 1;
  }
  if (!WANT_Q) return;

  const BilinearTerms bt = bilinear_terms(lx, ly, bev_h, bev_w, finite);
  sp[m * NSp + (lane & 7)] = bwd_sample_param(bt, 0, bev_w, row_stride);
  wave_lds_sync();

  // ---- gradient map: lane = (head g, channel piece c4); ends with sample c4 = t*4 + p of head g ---------------------------
  const int g = lane >> 3, c4 = lane & 7;
  const int b2 = lane_flag((c4 & 4) != 0), b1 = lane_flag((c4 & 2) != 0), b0 = lane_flag((c4 & 1) != 0);
  float4 top = *reinterpret_cast<const float4*>(grad_out + bq * row_stride + g * D + c4 * 4);
  top.x *= 0.5f; top.y *= 0.5f; top.z *= 0.5f; top.w *= 0.5f;
  const unsigned lane_off = (unsigned)(g * D + c4 * 4) * 4u;
  const unsigned map_bytes = (unsigned)bev_h * (unsigned)bev_w * (unsigned)row_stride * 4u;
  // queue entry h holds samples 4 h .. 4 h + 3; the reduce-scatter leaves lane c4 with the channel sums of sample c4
  OCC_BWD_GRAD_CHUNK8(g * NSp, uniform_rsrc(value + ((long)b * 2 + h) * value_bt_stride, map_bytes), dA, gX, gY)

  // ---- softmax backward over the sample's 4-lane group (lane g*8 + c4 = m*8 + t*4 + p: `aw` is this sample's) -------------
  float dot = aw * dA;
  dot += __shfl_xor(dot, 1);
  dot += __shfl_xor(dot, 2);
  grad_logits[bq * glogits_stride + lane] = aw * (dA - dot);
  *reinterpret_cast<float2*>(grad_offs + bq * goffs_stride + 2 * lane) = make_float2(aw * gX, aw * gY);
}

struct TsaBwdWs { BwdWsLayout w; size_t off_loc, off_attn, bytes; bool ok; };
static TsaBwdWs tsa_bwd_ws_layout(int B, int Nq, int M, int P) {
  TsaBwdWs r;
  r.w = bwd_ws_layout(B * 2, Nq, M, 1, Nq, P);
  const size_t n = (size_t)B * 2 * Nq * M * P;
  r.off_loc = (r.w.bytes + 255) & ~(size_t)255;
  r.off_attn = (r.off_loc + n * 8 + 255) & ~(size_t)255;
  r.bytes = r.off_attn + n * 4;
  r.ok = r.w.ok;
  return r;
}

static bool tsa_bwd_shape(int B, int Nq, int bev_h, int bev_w, int M, int D, int P) {
  return B > 0 && B < (1 << 30) && Nq > 0 && bev_h > 0 && bev_w > 0 && (long)bev_h * bev_w == (long)Nq && M == 8 &&
         D == 32 && P == 4 && (long)Nq * M * D * 4 < (long)kOobOffset;
}

}  // namespace occ

// Bytes of caller-owned scratch occ_tsa_fused_backward_f32 needs for these shapes; 0 = no backward kernel for them.
extern "C" int64_t occ_tsa_fused_backward_workspace_bytes(int B, int Nq, int bev_h, int bev_w, int M, int D, int P) {
  using namespace occ;
  if (!tsa_bwd_shape(B, Nq, bev_h, bev_w, M, D, P)) return 0;
  const TsaBwdWs w = tsa_bwd_ws_layout(B, Nq, M, P);
  return w.ok ? (int64_t)w.bytes : 0;
}

extern "C" int occ_tsa_fused_backward_f32(const float* value, int64_t value_bt_stride, const float* offs,
                                          int64_t offs_stride, const float* logits, int64_t logits_stride,
                                          const float* ref_2d, const float* grad_out, const int64_t* spatial_shapes,
                                          const int64_t* level_start_index, float* grad_value, float* grad_offs,
                                          int64_t grad_offs_stride, float* grad_logits, int64_t grad_logits_stride, int B,
                                          int Nq, int bev_h, int bev_w, int M, int D, int P, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(value && offs && logits && ref_2d && grad_out && spatial_shapes && level_start_index && workspace,
                "tsa_fused_backward: null pointer argument");
  const bool want_v = grad_value != nullptr, want_q = grad_offs != nullptr;
  OCC_CHECK_ARG((grad_offs != nullptr) == (grad_logits != nullptr) && (want_v || want_q),
                "tsa_fused_backward: null pointer argument (outputs: grad_value, or grad_offs AND grad_logits, or all three)");
  OCC_CHECK_ARG(B > 0 && Nq > 0 && bev_h > 0 && bev_w > 0 && M > 0 && D > 0 && P > 0,
                "tsa_fused_backward: bad dimension (B=%d Nq=%d bev_h=%d bev_w=%d)", B, Nq, bev_h, bev_w);
  if (M != 8 || D != 32 || P != 4) {
    set_error("tsa_fused_backward: no backward kernel for M=%d D=%d P=%d", M, D, P);
    return OCC_E_UNSUPPORTED;
  }
  if ((long)bev_h * bev_w != (long)Nq) {
    set_error("tsa_fused_backward: no backward kernel for a query band (Nq=%d, map %dx%d)", Nq, bev_h, bev_w);
    return OCC_E_UNSUPPORTED;
  }
  OCC_CHECK_ARG((long)bev_h * bev_w * M * D * 4 < (long)kOobOffset, "tsa_fused_backward: BEV map too large");
  OCC_CHECK_ARG(value_bt_stride >= 0, "tsa_fused_backward: negative value stride");
  const long n_off = (long)M * 2 * P * 2, n_att = (long)M * 2 * P;
  OCC_CHECK_ARG(offs_stride >= n_off && logits_stride >= n_att &&
                    (!want_q || (grad_offs_stride >= n_off && grad_logits_stride >= n_att)),
                "tsa_fused_backward: row strides smaller than a row");
  // float2 offset pairs and reference points, float4 pieces of value / grad_out rows; the replay adds float4 pieces
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(offs) % 8 == 0 && offs_stride % 2 == 0 &&
                    (!want_q || (reinterpret_cast<uintptr_t>(grad_offs) % 8 == 0 && grad_offs_stride % 2 == 0)),
                "tsa_fused_backward: offs and grad_offs must be 8-byte aligned with an even row stride");
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(value) % 16 == 0 && value_bt_stride % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(grad_out) % 16 == 0 && reinterpret_cast<uintptr_t>(grad_value) % 16 == 0,
                "tsa_fused_backward: value, grad_out and grad_value must be 16-byte aligned");
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(ref_2d) % 8 == 0, "tsa_fused_backward: ref_2d must be 8-byte aligned");
  const TsaBwdWs w = tsa_bwd_ws_layout(B, Nq, M, P);
  if (B >= (1 << 30) || !w.ok) {
    set_error("tsa_fused_backward: shapes beyond the binned grad_value path (B=%d Nq=%d)", B, Nq);
    return OCC_E_UNSUPPORTED;
  }
  OCC_CHECK_ARG(workspace_bytes >= (int64_t)w.bytes && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                "tsa_fused_backward: workspace too small (%ld < %ld bytes) or not 256-byte aligned", (long)workspace_bytes,
                (long)w.bytes);
  const bool deterministic = bwd_deterministic();                  // read per call, as the msda backward does
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  float* ws_loc = reinterpret_cast<float*>(ws + w.off_loc);
  float* ws_attn = reinterpret_cast<float*>(ws + w.off_attn);
  unsigned char* ws_flags = reinterpret_cast<unsigned char*>(ws);
  if (want_v) {
    const hipError_t e = hipMemsetAsync(ws, 0, w.w.off_cur, st);    // flags + counts of the binning passes
    if (e != hipSuccess) {
      set_error("tsa_fused_backward: workspace clear failed: %s", hipGetErrorString(e));
      return OCC_E_LAUNCH;
    }
  }
  const long blocks = ((long)B * Nq + kTsaBwdWaves - 1) / kTsaBwdWaves;
  const dim3 grid((unsigned)blocks), block(64 * kTsaBwdWaves);
#define OCC_TSA_BWD_LAUNCH(WQ, WV)                                                                                          \
  hipLaunchKernelGGL((tsa_bwd_sample_kernel<WQ, WV>), grid, block, 0, st, value, (long)value_bt_stride, offs,               \
                     (long)offs_stride, logits, (long)logits_stride, ref_2d, grad_out, grad_offs, (long)grad_offs_stride,  \
                     grad_logits, (long)grad_logits_stride, ws_loc, ws_attn, ws_flags, B, Nq, bev_h, bev_w)
  if (want_q && want_v) OCC_TSA_BWD_LAUNCH(true, true);
  else if (want_q) OCC_TSA_BWD_LAUNCH(true, false);
  else OCC_TSA_BWD_LAUNCH(false, true);
#undef OCC_TSA_BWD_LAUNCH
  OCC_CHECK_LAUNCH("tsa_fused_backward (samples)");
  if (want_v) {
    const int rc = bwd_bins_replay(w.w, ws, deterministic, spatial_shapes, level_start_index, ws_loc, ws_attn, nullptr,
                                   grad_out, (long)B * Nq * M * D, grad_value, B * 2, Nq, M, 1, Nq, P, st, 2);
    if (rc != OCC_OK) return rc;
    OCC_CHECK_LAUNCH("tsa_fused_backward (grad_value)");
  }
  return OCC_OK;
}
