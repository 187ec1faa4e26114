// The occupancy heads (semantics + flow MLPs, occ_heads.hip's header) on the bf16 matrix cores, as the pieces that
// occ_heads_x3_kernel (occ_heads.hip: rows from memory) and conv3d_heads_x3_kernel (conv3d_mfma.hip: rows straight from
// the convolution's D registers) share: the fragment packing of the weights, one 32-voxel tile from operand words to
// transposed logits, and the class decode of one voxel.  How a kernel loads its operands and stores its outputs stays
// in the kernel.
#pragma once
#include "common.h"

namespace occ {

constexpr int kHeadsC = 32, kHeadsHid = 64;      // input channels, hidden units per head

// Element e in [0, 4096) of the packed weights: one (hi, lo) pair of W1cat and one of W2cat, into
//   w1s [(a*2 + s)*2 + plane][lane][8 bf16]      W1cat = [predicter.0 ; flow_predicter.0]  (128 x 32), A operand of layer 1
//   w2s [(kk*2 + plane)][lane][8 bf16]           W2cat block diagonal (32 x 128), A operand of layer 2
// W1cat's k-slot (s, g, j) of a lane stands for input channel
//   K_FROM_D = false:  16 s + 8 g + j                       (a lane's 8 consecutive floats of a row in memory)
//   K_FROM_D = true:   16 s + 8 (j / 4) + 4 g + j % 4       (a lane's D registers of the transposed convolution)
// The two orders sum the same products in a different order: each kernel keeps its own, and with it its bits.
// W2cat's k-slot is always the D-register order: hidden unit 32 a + 16 ks + 8 (j / 4) + 4 g + j % 4.
template <bool K_FROM_D>
__device__ __forceinline__ void heads_pack_weights(int e, const float* w1o, const float* w2o, const float* w1f,
                                                   const float* w2f, int ncls,
                                                   unsigned short* w1s, unsigned short* w2s) {
  constexpr int C = kHeadsC, HID = kHeadsHid;
  const int j = e & 7, l = (e >> 3) & 63, f = e >> 9;      // f: 0..7
  const int m = l & 31, gg = l >> 5;
  {   // W1cat: f = a*2 + s
    const int a = f >> 1, sk = f & 1, u = 32 * a + m;
    const int k = K_FROM_D ? 16 * sk + 8 * (j >> 2) + 4 * gg + (j & 3) : 16 * sk + 8 * gg + j;
    const float w = u < HID ? w1o[u * C + k] : w1f[(u - HID) * C + k];
    unsigned short hi, lo;
    bf16_split(w, hi, lo);
    w1s[((f * 2 + 0) * 64 + l) * 8 + j] = hi;
    w1s[((f * 2 + 1) * 64 + l) * 8 + j] = lo;
  }
  {   // W2cat: f = kk = 2a + ks; output row m, hidden unit u
    const int a = f >> 1, ks = f & 1, u = 32 * a + 16 * ks + 8 * (j >> 2) + 4 * gg + (j & 3);
    float w = 0.f;
    if (m < ncls) { if (u < HID) w = w2o[m * HID + u]; }
    else if (m < ncls + 2) { if (u >= HID) w = w2f[(m - ncls) * HID + (u - HID)]; }
    unsigned short hi, lo;
    bf16_split(w, hi, lo);
    w2s[((f * 2 + 0) * 64 + l) * 8 + j] = hi;
    w2s[((f * 2 + 1) * 64 + l) * 8 + j] = lo;
  }
}
// b1cat (128) and b2cat (32, zero beyond ncls + 2), element e of each
__device__ __forceinline__ void heads_pack_bias(int e, const float* b1o, const float* b2o, const float* b1f,
                                                const float* b2f, int ncls,
                                                float* b1s, float* b2s) {
  if (e < 128) b1s[e] = e < kHeadsHid ? b1o[e] : b1f[e - kHeadsHid];
  if (e < 32) b2s[e] = e < ncls ? b2o[e] : (e < ncls + 2 ? b2f[e - ncls] : 0.f);
}

// One 32-voxel tile: lane (voxel vi, half g) supplies its voxel's two 16-k steps as hi / lo operand words xh[s], xl[s] (in
// the k order W1cat was packed for); W1 / W2 point at this lane's fragment in LDS, b1s / b2s at the biases in LDS.
// Leaves the logits transposed in sm[voxel][33]: occupancy classes [0, ncls), flow ncls, ncls + 1.
__device__ __forceinline__ void heads_tile(const uint4 (&xh)[2], const uint4 (&xl)[2], const bf16x8* W1, const bf16x8* W2,
                                           const float* b1s, const float* b2s, float* sm, int vi, int g) {
  // ---- H^T = W1cat . X^T : 4 hidden tiles, the MFMAs of different tiles interleaved (no back-to-back MFMAs on one
  // accumulator)
  f32x16 h[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) h[a][r] = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 bxh = __builtin_bit_cast(bf16x8, xh[s]), bxl = __builtin_bit_cast(bf16x8, xl[s]);
#pragma unroll
    for (int a = 0; a < 4; ++a)
      h[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1[((a * 2 + s) * 2 + 1) * 64], bxh, h[a], 0, 0, 0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
      h[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1[((a * 2 + s) * 2 + 0) * 64], bxl, h[a], 0, 0, 0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
      h[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(W1[((a * 2 + s) * 2 + 0) * 64], bxh, h[a], 0, 0, 0);
  }
  // ---- bias + activation (hidden [0,64): Softplus, [64,128): ReLU), then O^T = W2cat . act(H^T); one accumulator
  // per bf16x3 term
  f32x16 o0, o1, o2;
#pragma unroll
  for (int r = 0; r < 16; ++r) o0[r] = o1[r] = o2[r] = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float v[16];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const float4 bb = *reinterpret_cast<const float4*>(b1s + 32 * a + 8 * q4 + 4 * g);
      const float t0 = h[a][4 * q4 + 0] + bb.x, t1 = h[a][4 * q4 + 1] + bb.y;
      const float t2 = h[a][4 * q4 + 2] + bb.z, t3 = h[a][4 * q4 + 3] + bb.w;
      if (a < 2) {
        v[4 * q4 + 0] = softplus(t0); v[4 * q4 + 1] = softplus(t1);
        v[4 * q4 + 2] = softplus(t2); v[4 * q4 + 3] = softplus(t3);
      } else {
        v[4 * q4 + 0] = fmaxf(t0, 0.f); v[4 * q4 + 1] = fmaxf(t1, 0.f);
        v[4 * q4 + 2] = fmaxf(t2, 0.f); v[4 * q4 + 3] = fmaxf(t3, 0.f);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 hh, hl;
      bf16_split2(v[8 * ks + 0], v[8 * ks + 1], hh.x, hl.x); bf16_split2(v[8 * ks + 2], v[8 * ks + 3], hh.y, hl.y);
      bf16_split2(v[8 * ks + 4], v[8 * ks + 5], hh.z, hl.z); bf16_split2(v[8 * ks + 6], v[8 * ks + 7], hh.w, hl.w);
      const int kk = 2 * a + ks;
      const bf16x8 wh = W2[(kk * 2 + 0) * 64], wl = W2[(kk * 2 + 1) * 64];
      o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, __builtin_bit_cast(bf16x8, hh), o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, __builtin_bit_cast(bf16x8, hl), o1, 0, 0, 0);
      o2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, __builtin_bit_cast(bf16x8, hh), o2, 0, 0, 0);
    }
  }
  // O^T (row = output channel, col = voxel) + bias -> sm[voxel][channel]
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const float4 bb = *reinterpret_cast<const float4*>(b2s + 8 * q4 + 4 * g);
    const float bq[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * q4 + i;
      sm[vi * 33 + 8 * q4 + 4 * g + i] = ((o0[r] + o1[r]) + o2[r]) + bq[i];
    }
  }
}

// Class decode of one voxel's row of sm[voxel][33] (reference bevformer_occ_head.py:210-212: softmax(-1).argmax(-1)): softmax is
// monotonic, so the class is the argmax of the logits, first index on ties as torch.argmax resolves them.
__device__ __forceinline__ int heads_argmax(const float* sm, int voxel, int ncls) {
  float best = sm[voxel * 33];
  int arg = 0;
  bool nan = best != best;
  for (int ch = 1; ch < ncls; ++ch) {
    const float x = sm[voxel * 33 + ch];
    nan |= x != x;
    if (x > best) { best = x; arg = ch; }
  }
  // a NaN logit makes the reference's whole softmax row NaN, whose argmax torch resolves to index 0
  return nan ? 0 : arg;
}

}  // namespace occ
