// Backward of the fused spatial cross-attention gather (sca_fused.hip, fp32 value rows) for gfx950.
//
// The forward, per (batch b, BEV query q), head m, sample s = (level l, point p), over the cameras c that batch 0's mask
// marks for q (the reference's quirk), divided by the number of cameras q's OWN mask marks (clamped to >= 1):
//   a_s   = softmax over the head's L*P logits,  loc_s(c) = ref_cam[c][b][q][p % Z] + off_s / (W_l, H_l)
//   slots[b][q][m] = sum_c sum_s a_s * bilinear(value[b * NC + c][m], loc_s(c)) / count
// Its gradients for top = grad_slots[b][q][m] / count, per sample, with the in-range corner rows v1..v4 of camera c and the
// bilinear weights of mmcv's ms_deformable_col2im (out-of-range corners read as 0):
//   dA_s        = sum_c sum_ch top_ch * (hh hw v1 + hh lw v2 + lh hw v3 + lh lw v4)
//   grad_off_x  = a_s * sum_c sum_ch top_ch * (hh (v2 - v1) + lh (v4 - v3))     (d loc_x / d off_x = 1 / W_l cancels the W_l
//   grad_off_y  = a_s * sum_c sum_ch top_ch * (hw (v3 - v1) + lw (v4 - v2))      of d h_im / d loc: no scale left)
//   grad_logit  = a_s * (dA_s - sum_s' a_s' dA_s')                              (softmax backward over the head's L*P)
//   grad_value[b * NC + c][corner k][m] += top * a_s * w_k                       (in-range corners)
//
// grad_offs / grad_logits: sca_bwd_sample_kernel, one 64-lane wave per (b, q) like the forward.  Per visible camera the wave
// resolves the head's samples into LDS (set-up map: lane + 64 k = m * LP + s, the fp32 forward's: gather_pieces.h), then every 8-lane group
// (one head, 4 channels per lane) reads its head's samples 8 at a time, takes the dot products of the grad row with the four
// corner rows, and folds the 8 lanes' partial sums of those 8 samples by a REDUCE-SCATTER (xor 4, 2, 1: 21 shuffles for 24
// values) that leaves lane c4 of the group with sample 8 j + c4 — summed over the cameras in registers.  The softmax, the 1 / count
// and the attention weight are applied once at the end, in the same lane map.  Every output element has one writer and the
// order of every sum is fixed: grad_offs and grad_logits are bit-reproducible.
// The kernel also leaves the camera-independent sampling terms (a_s / count, off_s / (W_l, H_l)) in the workspace.
//
// grad_value: the binned count -> scan -> fill -> replay of msda_backward.hip (msda_bwd_bins.h), fed with the items of the
// VISIBLE (query, camera) rows only: a sample's location is recomputed from the camera's anchor and the saved offset term, its
// weight is a_s / count, and the replay reads the query's grad_slots row directly (no padded per-camera grad_out).  No float
// atomics outside the few split bins of the default mode; OCC_MSDA_BWD_DETERMINISTIC=1 takes the order-independent fixed-point
// replay, so grad_value is bit-identical run to run as well.
#include <cstdlib>
#include "gather_pieces.h"
#include "msda_bwd_bins.h"

namespace occ {

constexpr int kScaBwdWaves = 4;

// BwdSampleParam, the sample builder, the 8-sample gradient chunk: gather_pieces.h (shared with tsa_fused_backward.hip)

template <int L, int P>
__global__ __launch_bounds__(64 * kScaBwdWaves) void sca_bwd_sample_kernel(
    const float* __restrict__ value, const int64_t* __restrict__ shapes, const int64_t* __restrict__ lstart,
    const float* __restrict__ offs, long offs_stride, const float* __restrict__ logits, long logits_stride,
    const float* __restrict__ ref_cam, const uint32_t* __restrict__ vis_bits, const float* __restrict__ grad_slots,
    float* __restrict__ grad_offs, long goffs_stride, float* __restrict__ grad_logits, long glogits_stride,
    float* __restrict__ pre_aw, float* __restrict__ pre_oxy, int B, int NC, int S, int Z, int Nq) {
  constexpr int M = 8, D = 32, LP = L * P;
  constexpr int K = M * LP / 64;       // samples resolved per lane (set-up map)
  constexpr int J = LP / 8;            // samples per lane at the end (gradient map)
  static_assert(LP >= 8 && LP <= 32 && (LP & (LP - 1)) == 0, "L*P must be a power of two in [8,32]");
  constexpr int LPp = LP + 1;
  __shared__ BwdSampleParam smem[kScaBwdWaves * M * LPp];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long wg = (long)blockIdx.x * kScaBwdWaves + wave;
  if (wg >= (long)B * Nq) return;
  const int b = (int)(wg / Nq);
  const int q = (int)(wg - (long)b * Nq);
  const long bq = (long)b * Nq + q;
  BwdSampleParam* sp = smem + wave * M * LPp;
  constexpr int row_stride = M * D;
  const uint32_t vis = vis_bits[q];                   // batch 0's mask picks the cameras
  const uint32_t own = vis_bits[bq];                  // this batch's mask gives the divisor
  const float inv = (float)(own != 0u ? __builtin_popcount(own) : 1);

  // ---- set-up map: normalised offsets of the lane's K samples (idx = lane + 64 k = m * LP + s) ---------------------------
  OCC_SCA32_LEVEL
  float ox[K], oy[K];
  const float* orow = offs + bq * offs_stride;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int idx = lane + 64 * k;
    OCC_SCA32_OFFSET(k)
    *reinterpret_cast<float2*>(pre_oxy + (bq * M * LP + idx) * 2) = make_float2(ox[k], oy[k]);
  }

  // ---- gradient map: lane = (head g, channel piece c4); owns samples s = 8 j + c4 of head g at the end ------------------
  const int g = lane >> 3, c4 = lane & 7;
  const int b2 = lane_flag((c4 & 4) != 0), b1 = lane_flag((c4 & 2) != 0), b0 = lane_flag((c4 & 1) != 0);
  const float4 top = *reinterpret_cast<const float4*>(grad_slots + bq * row_stride + g * D + c4 * 4);
  const unsigned lane_off = (unsigned)(g * D + c4 * 4) * 4u;
  float accA[J], accX[J], accY[J];
#pragma unroll
  for (int j = 0; j < J; ++j) accA[j] = accX[j] = accY[j] = 0.f;

  for (int c = 0; c < NC; ++c) {
    if (!((vis >> c) & 1u)) continue;  // wave-uniform
    const float* rp = ref_cam + (((long)c * B + b) * Nq + q) * Z * 2;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      OCC_SCA32_ANCHOR(k)
      const BilinearTerms t = bilinear_terms(rxy.x + ox[k], rxy.y + oy[k], lvH, lvW, 1);
      sp[m * LPp + s] = bwd_sample_param(t, lvS, lvW, row_stride);
    }
    wave_lds_sync();
    const __amdgpu_buffer_rsrc_t rsrc =
        uniform_rsrc(value + ((long)b * NC + c) * S * row_stride, (unsigned)S * row_stride * 4u);
    // a rolled loop over the head's 8-sample chunks (unrolled, hipcc keeps the corner rows of several chunks live: 256 VGPRs
    // and spills); the chunk's result is added to its accumulator by selects
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
      // two groups of 4 samples (16 corner loads in flight), then the reduce-scatter: lane c4 ends with the channel sums of
      // sample 8 j + c4
      OCC_BWD_GRAD_CHUNK8(g * LPp + 8 * j, rsrc, rA, rX, rY)
#pragma unroll
      for (int jj = 0; jj < J; ++jj) {
        if (jj == j) { accA[jj] += rA; accX[jj] += rX; accY[jj] += rY; }
      }
    }
    wave_lds_sync();  // WAR: next camera rewrites the LDS slab
  }

  // ---- softmax of the head's logits in the gradient map, its backward, the outputs --------------------------------------
  const float* lrow = logits + bq * logits_stride + g * LP;
  float x[J];
  float mx = -__builtin_huge_valf();
#pragma unroll
  for (int j = 0; j < J; ++j) { x[j] = lrow[8 * j + c4]; mx = fmaxf(mx, x[j]); }
#pragma unroll
  for (int d = 4; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) { x[j] = expf(x[j] - mx); sum += x[j]; }
#pragma unroll
  for (int d = 4; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  float dot = 0.f, a[J], dA[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    a[j] = fdiv(x[j], sum);
    dA[j] = fdiv(accA[j], inv);
    dot = fmaf(a[j], dA[j], dot);
  }
#pragma unroll
  for (int d = 4; d >= 1; d >>= 1) dot += __shfl_xor(dot, d);
  float* glrow = grad_logits + bq * glogits_stride + g * LP;
  float* gorow = grad_offs + bq * goffs_stride + 2 * g * LP;
  float* awrow = pre_aw + bq * M * LP + g * LP;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int s = 8 * j + c4;
    glrow[s] = a[j] * (dA[j] - dot);
    *reinterpret_cast<float2*>(gorow + 2 * s) = make_float2(fdiv(a[j] * accX[j], inv), fdiv(a[j] * accY[j], inv));
    awrow[s] = fdiv(a[j], inv);
  }
}

struct ScaBwdWs { BwdWsLayout w; size_t off_aw, off_oxy, bytes; bool ok; };
static ScaBwdWs sca_bwd_ws_layout(int B, int NC, int S, int M, int L, int P, int Nq) {
  ScaBwdWs r;
  r.w = bwd_ws_layout(B * NC, S, M, L, Nq, P);
  const size_t n = (size_t)B * Nq * M * L * P;
  r.off_aw = (r.w.bytes + 255) & ~(size_t)255;
  r.off_oxy = (r.off_aw + n * 4 + 255) & ~(size_t)255;
  r.bytes = r.off_oxy + n * 8;
  r.ok = r.w.ok && bwd_block_bins_fit(B * NC, S, M, L, Nq, P);
  return r;
}

static bool sca_bwd_shape(int L, int P) {
  return (L == 4 && P == 8) || (L == 4 && P == 4) || (L == 2 && P == 8) || (L == 1 && P == 8);
}

template <int L, int P>
static void launch_sca_bwd_sample(const float* value, const int64_t* shapes, const int64_t* lstart, const float* offs,
                                  long offs_stride, const float* logits, long logits_stride, const float* ref_cam,
                                  const uint32_t* vis_bits, const float* grad_slots, float* grad_offs, long goffs_stride,
                                  float* grad_logits, long glogits_stride, float* pre_aw, float* pre_oxy, int B, int NC,
                                  int S, int Z, int Nq, hipStream_t st) {
  const long blocks = ((long)B * Nq + kScaBwdWaves - 1) / kScaBwdWaves;
  hipLaunchKernelGGL((sca_bwd_sample_kernel<L, P>), dim3((unsigned)blocks), dim3(64 * kScaBwdWaves), 0, st, value, shapes,
                     lstart, offs, offs_stride, logits, logits_stride, ref_cam, vis_bits, grad_slots, grad_offs,
                     goffs_stride, grad_logits, glogits_stride, pre_aw, pre_oxy, B, NC, S, Z, Nq);
}

}  // namespace occ

// Bytes of caller-owned scratch occ_sca_fused_backward_f32 needs for these shapes; 0 = no backward kernel for them.
extern "C" int64_t occ_sca_fused_backward_workspace_bytes(int B, int NC, int S, int M, int D, int L, int P, int Nq) {
  using namespace occ;
  if (B <= 0 || NC <= 0 || NC > 32 || S <= 0 || Nq <= 0 || M != 8 || D != 32 || !sca_bwd_shape(L, P)) return 0;
  const ScaBwdWs w = sca_bwd_ws_layout(B, NC, S, M, L, P, Nq);
  return w.ok ? (int64_t)w.bytes : 0;
}

extern "C" int occ_sca_fused_backward_f32(const float* value, const int64_t* spatial_shapes,
                                          const int64_t* level_start_index, const float* offs, int64_t offs_stride,
                                          const float* logits, int64_t logits_stride, const float* ref_cam,
                                          const uint32_t* vis_bits, const float* grad_slots, float* grad_value,
                                          float* grad_offs, int64_t grad_offs_stride, float* grad_logits,
                                          int64_t grad_logits_stride, int B, int NC, int S, int M, int D, int L, int P,
                                          int Z, int Nq, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(value && spatial_shapes && level_start_index && offs && logits && ref_cam && vis_bits && grad_slots &&
                    grad_value && grad_offs && grad_logits && workspace,
                "sca_fused_backward: null pointer argument");
  OCC_CHECK_ARG(B > 0 && NC > 0 && NC <= 32 && S > 0 && Nq > 0 && Z > 0 && L > 0 && P > 0,
                "sca_fused_backward: bad dimension (B=%d NC=%d S=%d Nq=%d Z=%d L=%d P=%d)", B, NC, S, Nq, Z, L, P);
  OCC_CHECK_ARG(P % Z == 0, "sca_fused_backward: num_points(%d) must be a multiple of Z(%d)", P, Z);
  if (M != 8 || D != 32) {
    set_error("sca_fused_backward: no backward kernel for M=%d D=%d", M, D);
    return OCC_E_UNSUPPORTED;
  }
  if (!sca_bwd_shape(L, P)) {
    set_error("sca_fused_backward: no backward kernel for L=%d P=%d", L, P);
    return OCC_E_UNSUPPORTED;
  }
  const long n_off = (long)M * L * P * 2, n_att = (long)M * L * P;
  OCC_CHECK_ARG(offs_stride >= n_off && logits_stride >= n_att && grad_offs_stride >= n_off && grad_logits_stride >= n_att,
                "sca_fused_backward: row strides smaller than a row");
  OCC_CHECK_ARG((long)S * M * D * 4 < (long)kOobOffset, "sca_fused_backward: value batch entry too large");
  const ScaBwdWs w = sca_bwd_ws_layout(B, NC, S, M, L, P, Nq);
  if (!w.ok) {
    set_error("sca_fused_backward: shapes beyond the binned grad_value path (B=%d NC=%d S=%d Nq=%d)", B, NC, S, Nq);
    return OCC_E_UNSUPPORTED;
  }
  OCC_CHECK_ARG(workspace_bytes >= (int64_t)w.bytes && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                "sca_fused_backward: workspace too small (%ld < %ld bytes) or not 256-byte aligned", (long)workspace_bytes,
                (long)w.bytes);
  const bool deterministic = bwd_deterministic();                  // read per call, as the msda backward does
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  float* pre_aw = reinterpret_cast<float*>(ws + w.off_aw);
  float* pre_oxy = reinterpret_cast<float*>(ws + w.off_oxy);
  const hipError_t e = hipMemsetAsync(ws, 0, w.w.off_cur, st);    // flags + counts of the binning passes
  if (e != hipSuccess) {
    set_error("sca_fused_backward: workspace clear failed: %s", hipGetErrorString(e));
    return OCC_E_LAUNCH;
  }
#define OCC_SCA_BWD_CASE(LL, PP)                                                                                          \
  if (L == LL && P == PP)                                                                                                 \
    launch_sca_bwd_sample<LL, PP>(value, spatial_shapes, level_start_index, offs, (long)offs_stride, logits,              \
                                  (long)logits_stride, ref_cam, vis_bits, grad_slots, grad_offs, (long)grad_offs_stride,  \
                                  grad_logits, (long)grad_logits_stride, pre_aw, pre_oxy, B, NC, S, Z, Nq, st);
  OCC_SCA_BWD_CASE(4, 8)
  else OCC_SCA_BWD_CASE(4, 4)
  else OCC_SCA_BWD_CASE(2, 8)
  else OCC_SCA_BWD_CASE(1, 8)
#undef OCC_SCA_BWD_CASE
  OCC_CHECK_LAUNCH("sca_fused_backward (samples)");
  const ScaBinSource src{ref_cam, pre_oxy, pre_aw, vis_bits, NC, B, Z};
  const int rc = bwd_bins_replay(w.w, ws, deterministic, spatial_shapes, level_start_index, nullptr, nullptr, &src,
                                 grad_slots, (long)B * Nq * M * D, grad_value, B * NC, S, M, L, Nq, P, st);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_LAUNCH("sca_fused_backward (grad_value)");
  return OCC_OK;
}
