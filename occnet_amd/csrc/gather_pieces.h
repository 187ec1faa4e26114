// The blocks that two or more deformable-gather kernels must keep the same, once.  A backward resolves exactly the sample its
// forward resolved (the fused training paths, OCC_TSA_TRAIN_FUSED and the fused SCA step, rest on that), and the two 16-bit
// SCA kernels that OCC_SCA_HEAD_MAJOR selects between per call compute the same sums in the same order.  Included by
// sca_fused.hip, sca_fused_backward.hip, tsa_fused.hip, tsa_fused_backward.hip and msda_backward.hip only.
// A piece is a __forceinline__ function where that leaves every kernel's device code the parent's (tsa_lane_setup,
// bwd_sample_param, next to dot4 / rs_step), and TEXT otherwise: a macro on the enclosing kernel's locals, for the reason
// given in conv3x3_kloop.h — hipcc simplifies a callee before it inlines it (EXPERIMENTS.md section 8s lists, piece by piece,
// what each one did as a function: the gradient chunk took sca_bwd_sample_kernel<4, 4> from 132 to 160 VGPRs).  Every set-up
// piece goes through bilinear_terms / bilinear_setup_b (common.h), so the predicates keep the 0 / 1 lane_flag form; no piece
// has a `bool` predicate of its own.  What differs between two kernels stays written out in them: the lane maps, `live`, the
// camera loop, the slab row, the head-major kernel's two-float4 anchor load, the workspace planes of the TSA backward and the
// softmax-backward tails.  Macro arguments that are index sums are pasted WITHOUT parentheses (HEAD, ROW0, SP0 below), so
// that the sum keeps the parent's flat association: it decides the address instructions.
//
// The functions:
//   tsa_lane_setup(...)            lane = m*8 + t*4 + p of tsa_fused_kernel / tsa_bwd_sample_kernel: aw = softmax over the lane's
//                                  4-lane group, (lx, ly) = reference point + offset / (W, H).  The wave must be converged.
//   bwd_sample_param(t, lvs, w, row_stride)   the BwdSampleParam of BilinearTerms t in a level starting at pixel lvs, w wide
// The text pieces, and the locals each expects in scope:
//   OCC_SCA16_PROLOGUE(HEAD)       sca_fused_h / _hm: fills aw, ox, oy [K] of head HEAD: the lane's K logits / offset pairs as one
//                                  / two vector loads (K == 4) or scalars, softmax = K-term local reduction + 3 shuffle steps
//                                  over the head's 8 lanes, offsets / (W_l, H_l).  logits, logits_stride, offs, offs_stride, b,
//                                  Nq, q, LP, K, sK, lvH, lvW
//   OCC_SCA16_ANCHORS              rxy_k[k] = anchor of sample sK K + k.  rp, rxy_k [K], K, P, Z, sK
//   OCC_SCA16_RESOLVE(ROW0, LIVE)  sched_barrier, then the lane's K samples -> slab entries ROW0 + k * 8 + sK in the pixel-pair
//                                  layout; n_in += corners inside the map.  rxy_k, aw, ox, oy, lvH, lvW, lvS, row_stride, EV, sp,
//                                  sK, n_in
//   OCC_SCA16_EPILOGUE(STORES, DST)  inv = count * value_scale * (Q ? 2^14 : 1), the eight half merges, and for the lanes with
//                                  STORES the two float4 stores of fdiv(acc, inv) to DST.  count, value_scale, Q, acc, acc2
//   OCC_SCA_STATS(SUM_ROWS)        stats[0] += n_rows (summed over the lanes when SUM_ROWS, and then added only if non-zero),
//                                  stats[1] += sum of n_in.  stats, lane, n_in, n_rows
//   OCC_SCA32_LEVEL                fp32 SCA map idx = lane + 64 k = m * LP + s (sca_fused_kernel, sca_bwd_sample_kernel):
//                                  declares lane_l, lvH, lvW, lvS.  lane, LP, P, shapes, lstart
//   OCC_SCA32_OFFSET(k)            ox[k], oy[k] = the offset pair of idx / (W_l, H_l); declares o.  orow, idx, lvW, lvH
//   OCC_SCA32_ANCHOR(k)            declares idx, m, s, z and rxy = the anchor (s % P) % Z.  lane, LP, P, Z, rp
//   OCC_BWD_GRAD_CHUNK8(SP0, RSRC, DA, GX, GY)  samples sp[SP0 .. SP0 + 7] of the lane's head, RSRC (may name h) = the map of
//                                  samples 4 h .. 4 h + 3: declares DA, GX, GY = sample c4's sums over the group's 32 channels
//                                  (also v, r1, r2).  sp, lane_off, top, b2, b1, b0 (lane_flag of bits 2, 1, 0 of c4)
//   OCC_D32_CORNER_GRAD(EXTRA)     msda_bwd_d32_kernel: g_attn, g_x, g_y += one sample's sums over the lane's four channels;
//                                  EXTRA runs per channel k (with ta, w1 .. w4).  top, v1 .. v4 (0 outside the map), lh, lw, hh,
//                                  hw, a
#pragma once
#include "common.h"

namespace occ {

// ---- 16-bit SCA kernels ----------------------------------------------------------------------------------------------------
#define OCC_SCA16_PROLOGUE(HEAD)                                                                                       \
  {                                                                                                                    \
    const float* lp = logits + ((long)b * Nq + q) * logits_stride + HEAD * LP + sK * K;                                \
    const float* op = offs + ((long)b * Nq + q) * offs_stride + 2 * (HEAD * LP + sK * K);                              \
    float x[K], o[2 * K];                                                                                              \
    if constexpr (K == 4) {                                                                                            \
      const float4 tt = *reinterpret_cast<const float4*>(lp);                                                          \
      x[0] = tt.x; x[1] = tt.y; x[2] = tt.z; x[3] = tt.w;                                                              \
      const float4 u0 = *reinterpret_cast<const float4*>(op), u1 = *reinterpret_cast<const float4*>(op + 4);           \
      o[0] = u0.x; o[1] = u0.y; o[2] = u0.z; o[3] = u0.w; o[4] = u1.x; o[5] = u1.y; o[6] = u1.z; o[7] = u1.w;          \
    } else {                                                                                                           \
      _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                  \
        x[k] = lp[k];                                                                                                  \
        const float2 tt = *reinterpret_cast<const float2*>(op + 2 * k);                                                \
        o[2 * k] = tt.x; o[2 * k + 1] = tt.y;                                                                          \
      }                                                                                                                \
    }                                                                                                                  \
    float mx = x[0];                                                                                                   \
    _Pragma("unroll") for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);                                                \
    _Pragma("unroll") for (int d = 4; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));                              \
    float sum = 0.f;                                                                                                   \
    _Pragma("unroll") for (int k = 0; k < K; ++k) { x[k] = expf(x[k] - mx); sum += x[k]; }                             \
    _Pragma("unroll") for (int d = 4; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);                                      \
    _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                    \
      aw[k] = fdiv(x[k], sum); /* (fdiv, not `/`: see common.h) */                                                     \
      ox[k] = fdiv(o[2 * k], (float)lvW);                                                                              \
      oy[k] = fdiv(o[2 * k + 1], (float)lvH);                                                                          \
    }                                                                                                                  \
  }

// point p pairs with z-anchor p % Z (view(.., P//Z, Z, 2))
#define OCC_SCA16_ANCHORS                                                                                              \
  _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                      \
    const int z = ((sK * K + k) % P) % Z;                                                                              \
    rxy_k[k] = *reinterpret_cast<const float2*>(rp + 2 * z);                                                           \
  }

// Pixel-pair layout (sca_fused.hip's header): byte offset pix * 512 -> (pix >> 1) * 1024 + (pix & 1) * 64; the out-of-range
// marker stays out of range.  Slot k * 8 + sK, not s: the 8 lanes of a row write consecutive 32-byte entries (conflict-free);
// the gather sums a row's LP entries, so their order in the slab is free.
#define OCC_SCA16_RESOLVE(ROW0, LIVE)                                                                                  \
  __builtin_amdgcn_sched_barrier(0);                                                                                   \
  _Pragma("unroll") for (int k = 0; k < K; ++k) {                                                                      \
    SampleParamB p;                                                                                                    \
    n_in += bilinear_setup_b(rxy_k[k].x + ox[k], rxy_k[k].y + oy[k], aw[k], lvH, lvW, lvS,                             \
                             (unsigned)row_stride * EV, kOobOffset, LIVE, p);                                          \
    _Pragma("unroll") for (int kk = 0; kk < 4; ++kk) p.o[kk] = (p.o[kk] & ~1023u) | ((p.o[kk] >> 3) & 64u);            \
    sp[ROW0 + k * 8 + sK] = p;                                                                                         \
  }

// value_scale: the power-of-two range scale s the projection stored the 16-bit rows with (value_range.hip); dividing by
// count * s undoes it exactly (q16 rows: the mantissas additionally carry 2^15 / 2 — stored under s / 2 —, common.h fma8q).
// The two sample halves of a row sit 32 lanes apart.
#define OCC_SCA16_EPILOGUE(STORES, DST)                                                                                \
  const float inv = (float)(count > 0 ? count : 1) * (value_scale != nullptr ? *value_scale : 1.f) * (Q ? 16384.f : 1.f); \
  acc.x += __shfl_xor(acc.x, 32); acc.y += __shfl_xor(acc.y, 32); acc.z += __shfl_xor(acc.z, 32);                      \
  acc.w += __shfl_xor(acc.w, 32);                                                                                      \
  acc2.x += __shfl_xor(acc2.x, 32); acc2.y += __shfl_xor(acc2.y, 32); acc2.z += __shfl_xor(acc2.z, 32);                \
  acc2.w += __shfl_xor(acc2.w, 32);                                                                                    \
  if (STORES) {                                                                                                        \
    float* dst = DST;                                                                                                  \
    *reinterpret_cast<float4*>(dst) = make_float4(fdiv(acc.x, inv), fdiv(acc.y, inv), fdiv(acc.z, inv), fdiv(acc.w, inv)); \
    *reinterpret_cast<float4*>(dst + 4) = make_float4(fdiv(acc2.x, inv), fdiv(acc2.y, inv), fdiv(acc2.z, inv), fdiv(acc2.w, inv)); \
  }

#define OCC_SCA_STATS(SUM_ROWS)                                                                                        \
  if (stats) {                                                                                                         \
    _Pragma("unroll") for (int d = 32; d >= 1; d >>= 1) {                                                              \
      n_in += __shfl_xor(n_in, d);                                                                                     \
      if (SUM_ROWS) n_rows += __shfl_xor(n_rows, d);                                                                   \
    }                                                                                                                  \
    if (lane == 0) {                                                                                                   \
      if (!SUM_ROWS || n_rows) atomicAdd(&stats[0], (unsigned long long)n_rows);                                       \
      atomicAdd(&stats[1], (unsigned long long)n_in);                                                                  \
    }                                                                                                                  \
  }

// ---- fp32 SCA forward and backward: set-up map idx = lane + 64 k = m * LP + s ---------------------------------------------
// sample index s = (lane + 64 k) % LP does not depend on k (64 % LP == 0): one level per lane
#define OCC_SCA32_LEVEL                                                                                                \
  static_assert(64 % LP == 0, "the lane's level must not depend on k");                                                \
  const int lane_l = (lane % LP) / P;                                                                                  \
  const int lvH = (int)shapes[2 * lane_l], lvW = (int)shapes[2 * lane_l + 1], lvS = (int)lstart[lane_l];
#define OCC_SCA32_OFFSET(k)                                                                                            \
  const float2 o = *reinterpret_cast<const float2*>(orow + 2 * idx);                                                   \
  ox[k] = fdiv(o.x, (float)lvW);                                                                                       \
  oy[k] = fdiv(o.y, (float)lvH);
// point p pairs with z-anchor p % Z (view(.., P//Z, Z, 2))
#define OCC_SCA32_ANCHOR(k)                                                                                            \
  const int idx = lane + 64 * k;                                                                                       \
  const int m = idx / LP, s = idx % LP;                                                                                \
  const int z = (s % P) % Z;                                                                                           \
  const float2 rxy = *reinterpret_cast<const float2*>(rp + 2 * z);

// ---- TSA forward and backward: lane = m*8 + t*4 + p owns one sample, exactly the memory order of both Linear outputs --------
// softmax weight over the lane's 4-lane group (the 4 points of (m, t)), location = reference point + offset / (W, H); bq = b * Nq + q
__device__ __forceinline__ void tsa_lane_setup(const float* logits, long logits_stride, const float* offs, long offs_stride,
                                               const float* ref_2d, long bq, int lane, int b, int t, int q, int Nq, int bev_h,
                                               int bev_w, float& aw, float& lx, float& ly) {
  const float x = logits[bq * logits_stride + lane];
  float mx = fmaxf(x, __shfl_xor(x, 1));
  mx = fmaxf(mx, __shfl_xor(mx, 2));
  const float e = expf(x - mx);
  float sum = e + __shfl_xor(e, 1);
  sum += __shfl_xor(sum, 2);
  aw = fdiv(e, sum);                 // (fdiv, not `/`: see common.h)
  float2 o = *reinterpret_cast<const float2*>(offs + bq * offs_stride + 2 * lane);
  o.x = fdiv(o.x, (float)bev_w);
  o.y = fdiv(o.y, (float)bev_h);
  const float2 rf = *reinterpret_cast<const float2*>(ref_2d + (((long)b * 2 + t) * Nq + q) * 2);
  lx = rf.x + o.x;
  ly = rf.y + o.y;
}

// ---- the fused gathers' backward kernels (sca_bwd_sample_kernel, tsa_bwd_sample_kernel) ------------------------------------
// one resolved sample for the gradient: byte offsets of the four corner rows (kOobOffset outside the map: the buffer load
// returns 0, which is mmcv's "only in-range corners"), the fractional weights (0 for a sample outside its map)
struct __attribute__((aligned(16))) BwdSampleParam {
  unsigned o[4];
  float lh, lw, pad0, pad1;
};

// the sample of BilinearTerms t in a level that starts at pixel lvs and is w pixels wide; rows of row_stride floats
__device__ __forceinline__ BwdSampleParam bwd_sample_param(const BilinearTerms& t, int lvs, int w, int row_stride) {
  const unsigned base = (unsigned)(lvs + t.h_low * w + t.w_low);
  BwdSampleParam p;
  p.o[0] = t.c[0] ? base * (unsigned)row_stride * 4u : kOobOffset;
  p.o[1] = t.c[1] ? (base + 1u) * (unsigned)row_stride * 4u : kOobOffset;
  p.o[2] = t.c[2] ? (base + (unsigned)w) * (unsigned)row_stride * 4u : kOobOffset;
  p.o[3] = t.c[3] ? (base + (unsigned)w + 1u) * (unsigned)row_stride * 4u : kOobOffset;
  p.lh = t.adm ? t.lh : 0.f;       // a sample outside its map (or dead): 0, not 0 * NaN
  p.lw = t.adm ? t.lw : 0.f;
  p.pad0 = p.pad1 = 0.f;
  return p;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}

// One step of the reduce-scatter that folds 8 lanes' partial sums of 8 samples (xor 4, 2, 1) so that lane c of the group ends
// with sample c: x (lane's copy) + the value held `mask` lanes away, where each lane keeps one half and sends the other; hi
// (0 / 1 lane flag) selects which half this lane keeps
__device__ __forceinline__ float rs_step(float lo, float hi_v, int hi, int mask) {
  const float keep = hi ? hi_v : lo, send = hi ? lo : hi_v;
  return keep + __shfl_xor(send, mask);
}

// two groups of 4 samples x 4 corner loads (16 in flight), the dot products of the grad row with the corner rows, the three
// bilinear combinations, and the reduce-scatter over the group's 8 lanes (21 shuffles for 24 values)
#define OCC_BWD_GRAD_CHUNK8(SP0, RSRC, DA, GX, GY)                                                                     \
  float v[8][3];                                                                                                       \
  _Pragma("unroll") for (int h = 0; h < 2; ++h) {                                                                      \
    const __amdgpu_buffer_rsrc_t rsrc_h = RSRC;                                                                        \
    float4 r[4][4];                                                                                                    \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                    \
      const occ_u32x4 o = *reinterpret_cast<const occ_u32x4*>(sp[SP0 + 4 * h + u].o);                                  \
      _Pragma("unroll") for (int kk = 0; kk < 4; ++kk) r[u][kk] = buf_load16(rsrc_h, o[kk] + lane_off);                \
    }                                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                    \
      const BwdSampleParam& pp = sp[SP0 + 4 * h + u];                                                                  \
      const float lh = pp.lh, lw = pp.lw, hh = 1.f - lh, hw = 1.f - lw;                                                \
      const float d1 = dot4(top, r[u][0]), d2 = dot4(top, r[u][1]), d3 = dot4(top, r[u][2]), d4 = dot4(top, r[u][3]);  \
      v[4 * h + u][0] = hh * hw * d1 + hh * lw * d2 + lh * hw * d3 + lh * lw * d4;                                     \
      v[4 * h + u][1] = hh * (d2 - d1) + lh * (d4 - d3);                                                               \
      v[4 * h + u][2] = hw * (d3 - d1) + lw * (d4 - d2);                                                               \
    }                                                                                                                  \
  }                                                                                                                    \
  float r1[4][3], r2[2][3];                                                                                            \
  _Pragma("unroll") for (int u = 0; u < 4; ++u)                                                                        \
    _Pragma("unroll") for (int e = 0; e < 3; ++e) r1[u][e] = rs_step(v[u][e], v[4 + u][e], b2, 4);                     \
  _Pragma("unroll") for (int u = 0; u < 2; ++u)                                                                        \
    _Pragma("unroll") for (int e = 0; e < 3; ++e) r2[u][e] = rs_step(r1[u][e], r1[2 + u][e], b1, 2);                   \
  const float DA = rs_step(r2[0][0], r2[1][0], b0, 1);                                                                 \
  const float GX = rs_step(r2[0][1], r2[1][1], b0, 1);                                                                 \
  const float GY = rs_step(r2[0][2], r2[1][2], b0, 1);

// ---- msda_bwd_d32_kernel: one sample's corner gradients over the lane's four channels ---------------------------------------
#define OCC_D32_CORNER_GRAD(EXTRA)                                                                                     \
  const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;                                                  \
  const float tx[4] = {top.x, top.y, top.z, top.w};                                                                    \
  const float a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};                                      \
  const float a3[4] = {v3.x, v3.y, v3.z, v3.w}, a4[4] = {v4.x, v4.y, v4.z, v4.w};                                      \
  _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                      \
    const float ta = tx[k] * a;                                                                                        \
    g_attn += tx[k] * (w1 * a1[k] + w2 * a2[k] + w3 * a3[k] + w4 * a4[k]);                                             \
    g_x += ta * (hh * (a2[k] - a1[k]) + lh * (a4[k] - a3[k]));                                                         \
    g_y += ta * (hw * (a3[k] - a1[k]) + lw * (a4[k] - a2[k]));                                                         \
    EXTRA                                                                                                              \
  }

}  // namespace occ
