// Phases A and B of the whole 64-mid-channel bottleneck (bottleneck64_nhwc_bf16.hip says what the block computes), as TEXT:
// bottleneck64_nhwc_bf16_kernel and bottleneck64_v2_nhwc_bf16_kernel both expand these macros, so c1 and c2 are the same
// sums in the same order, rounded at the same place, by construction.  Every variant of occ_bottleneck64_nhwc_bf16_variant
// is tested torch.equal to variant 1 on that footing.  Macros on the kernel's locals and not __device__ functions, for the
// reason given in conv3x3_kloop.h (EXPERIMENTS.md sections 8m, 8r: phase B as a __forceinline__ function took the second
// kernel from 254 to 253 VGPRs with another register assignment throughout).
//
// Block = 4 waves x (8 x 16 output pixels).  All three weight matrices are pre-packed in MFMA B-fragment order
// (occ_mfma_pack_b_frag_bf16: [k-step][32-col tile][lane][8 bf16]), so a wave's operand is ONE coalesced 1 KB global load per
// (k-step, column tile) that never touches LDS (L1/L2 hits: 0.2 MB of weights shared by every block); LDS carries only
// activations:
//   lds                 two x chunk buffers of kBnXA bytes: 192 pixel slots x 32 channels, 80-byte slots (chunk step ci in
//                       buffer ci & 1)
//   sH1 = lds + 2 kBnXA the c1 halo: 10 x 18 pixel slots of 144 B, pixel p = hy * 18 + hx at p * 144, zero outside the image
//                       (= conv2's padding)
//   sC2 = sH1 + kBnH1   the c2 tile: 128 pixel slots of 144 B
//   phase A  x halo chunk -> c1 halo; GEMM 192 x 64 x Cin, wave = 3 row tiles x 1 column tile
//   phase B  9 taps x 4 k-steps straight out of the c1 halo -> c2 tile; wave = 2 x 1 tiles
//   phase C  c2 (+ x centre pixels when downsampling) x W3 -> 128 x 256: each kernel's own, on OCC_BN_C_AFRAG
// kBnStageBytes = 75 072 B of LDS -> two blocks per CU, so one block's loads overlap the other's MFMAs.
// The MFMAs of phases A and B are issued with the WEIGHTS as the row operand: D[channel][pixel], so a lane ends up with ONE
// pixel (column = lane & 31) and four groups of 4 consecutive channels (8g + 4*(lane>>5) + 0..3): the bf16 intermediates go
// to LDS as 8-byte stores of v_cvt_pk pairs and the per-pixel bookkeeping (in-image test) is done once per row tile, not
// once per element.
//
// The pieces, in the order a kernel places them (each kernel keeps its own statement order, which its registers depend
// on: 182 / 208 VGPRs for the first kernel's <64, true> / <256, false>, 174 / 254 for the second's, no scratch):
//   OCC_BN_TILE_DECODE(TILE)    tile (row-major over image, tile row, tile column) -> img, y0, x0
//   OCC_BN_STAGING              the three x staging roles of a thread (hofs*, hdst*, hlive*), the masks hm*, the four
//                               register sets vh*_S of the x prefetch
//   OCC_BN_WAVE_TILES           ntA, mtA0, ntB, mtB0: the wave's column tile and first row tile in phases A and B
//   OCC_BN_ISSUE_BIASES         requests bA, bB (float4 [4], the kernel's): b1 / b2 of this lane's channels
//   OCC_BN_ZERO_ACC(ACC, N)     f32x16 ACC[N] = 0
//   OCC_BN_ISSUE_X(S, CH)       requests the thread's three pieces of chunk CH into register set S
//   OCC_BN_ISSUE_W1(SLOT, CH)   requests the wave's two W1 fragments of chunk CH into wa[SLOT] (uint4 [.][2], the kernel's)
//   OCC_BN_CH(CI)               the chunk of step CI under the kernel's `rot`
//   inside a step:  OCC_BN_STAGE_STORE(S, SX)   register set S -> chunk buffer SX, zero outside the image
//                   OCC_BN_W1_FRAGS(SLOT)       declares wf0, wf1 from wa[SLOT]
//                   OCC_BN_STEP_MFMA(SX)        acc1 += W1 chunk x the wave's three row tiles of SX
//   OCC_BN_W2_PROLOGUE          declares the W2 ring wr[PFB = 12] and fills it
//   OCC_BN_WRITE_C1             acc1 + bA, ReLU, in-image mask, one RNE rounding -> sH1
//   OCC_BN_PHASE_B              declares acc2 and runs the 36 k-steps out of sH1 under the ring
//   OCC_BN_WRITE_C2             acc2 + bB, ReLU, one RNE rounding -> sC2
//   OCC_BN_C_AFRAG(AF, RT, KS)  phase C's activation fragment of row tile RT, k-step KS: sC2 for KS < 4, else (downsample)
//                               the centre pixels of x chunk (KS - 4) / 2, which still sits in its buffer
// They expect in scope
//   x, w1p, w2p                 const uint4* __restrict__: the NHWC input, the packed W1 and W2
//   b1, b2                      const float*
//   H, W, tiles_x, tiles_y      the map and its tiles
//   NCH, CQ, DS                 CIN / 32, CIN / 8, the projection instance
//   lds, sH1, sC2               char*: kBnStageBytes of LDS, 16-byte aligned, as laid out above
//   tid, lane, wave, vi, kb     threadIdx.x, tid & 63, tid >> 6, lane & 31, lane >> 5
//   rot                         const int: the chunk rotation, 0 when DS (chunk c must stay in buffer c for phase C); else
//                               keyed on what the kernel says (L2 channel hot-spotting, see conv1x1_nhwc_bf16.hip)
//   bA, bB, acc1, wa            the kernel's declarations, see above
// What a kernel spells out for itself: the rotation key, the depth of the W1 ring and where its request stands against the
// x request, when the biases are requested, the step skeleton made of the pieces above, and all of phase C.
#pragma once
#include "common.h"

namespace occ {

constexpr int kBnTH = 8, kBnTW = 16, kBnHH = 10, kBnHW = 18, kBnNP = kBnHH * kBnHW;   // 180 halo pixels
constexpr int kBnXS = 80;                    // bytes per x-chunk pixel slot (32 bf16 + 16 pad)
constexpr int kBnXA = 192 * kBnXS;           // one x chunk buffer (6 row tiles of 32 halo pixels)
constexpr int kBnMS = 144;                   // bytes per 64-channel pixel slot (128 + 16 pad)
constexpr int kBnH1ROW = kBnHW * kBnMS;      // 2592
constexpr int kBnH1 = kBnHH * kBnH1ROW;      // 25 920
constexpr int kBnC2 = 128 * kBnMS;           // 18 432
constexpr int kBnStageBytes = 2 * kBnXA + kBnH1 + kBnC2;              // 75 072

// the second kernel (bottleneck64_v2_nhwc_bf16.hip) on `st`: the first kernel's arguments, already checked, the same bits;
// order = its block -> tile map
void bottleneck64_v2_launch(const void* x, const void* w1_frag, const float* b1, const void* w2_frag, const float* b2,
                            const void* w3_frag, const float* b3, void* out, int batch, int H, int W, int downsample,
                            int order, hipStream_t st);
constexpr int kBnOrderDefault = 0;           // tile order of the second kernel where nothing else is asked for: 1 and 2 fetch
                                             // less and run slower (EXPERIMENTS.md section 8q)

// One launch of either kernel: the projection instance <64, true> or the identity instance <256, false>, one block per
// 8 x 16 tile; `tail` = what the kernel takes behind tiles_y.
template <typename Kernel, typename... Tail>
inline void bn64_launch(Kernel k_ds, Kernel k_id, const void* x, const void* w1_frag, const float* b1, const void* w2_frag,
                        const float* b2, const void* w3_frag, const float* b3, void* out, int batch, int H, int W,
                        int downsample, hipStream_t st, Tail... tail) {
  const int tiles_x = (W + kBnTW - 1) / kBnTW, tiles_y = (H + kBnTH - 1) / kBnTH;
  const unsigned gx = (unsigned)((long)batch * tiles_x * tiles_y);
  hipLaunchKernelGGL(downsample ? k_ds : k_id, dim3(gx), dim3(256), 0, st, reinterpret_cast<const uint4*>(x),
                     reinterpret_cast<const uint4*>(w1_frag), b1, reinterpret_cast<const uint4*>(w2_frag), b2,
                     reinterpret_cast<const uint4*>(w3_frag), b3, reinterpret_cast<unsigned short*>(out), H, W, tiles_x,
                     tiles_y, tail...);
}

}  // namespace occ

#define OCC_BN_TILE_DECODE(TILE)                                                                  \
  int bid = (TILE);                                                                               \
  const int tx_i = bid % tiles_x; bid /= tiles_x;                                                 \
  const int ty_i = bid % tiles_y;                                                                 \
  const int img = bid / tiles_y;                                                                  \
  const int y0 = ty_i * kBnTH, x0 = tx_i * kBnTW;

// x staging role K of a thread: 180 pixels x 4 pieces of 16 B per chunk = 720 items over 256 threads (clamped loads)
#define OCC_BN_ROLE(K, OFS, DST, IN, LIVE)                                                        \
  {                                                                                               \
    const int idx = tid + 256 * (K);                                                              \
    LIVE = idx < kBnNP * 4;                                                                       \
    const int p = LIVE ? idx >> 2 : 0, piece = idx & 3;                                           \
    const int hy = p / kBnHW, hx = p % kBnHW;                                                     \
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;                                                 \
    IN = LIVE && iy >= 0 && iy < H && ix >= 0 && ix < W;                                          \
    const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);                           \
    OFS = (((long)img * H + cy) * W + cx) * CQ + piece;                                           \
    DST = p * kBnXS + piece * 16;                                                                 \
  }
// four register sets: the x prefetch runs four chunks ahead (two blocks per CU and ~2 us of HBM latency under load: with
// two chunks in flight the phase was latency-bound)
#define OCC_BN_STAGING                                                                            \
  long hofs0, hofs1, hofs2;                                                                       \
  int hdst0, hdst1, hdst2;                                                                        \
  bool hin0, hin1, hin2, hlive0, hlive1, hlive2;                                                  \
  OCC_BN_ROLE(0, hofs0, hdst0, hin0, hlive0)                                                      \
  OCC_BN_ROLE(1, hofs1, hdst1, hin1, hlive1)                                                      \
  OCC_BN_ROLE(2, hofs2, hdst2, hin2, hlive2)                                                      \
  const unsigned hm0 = hin0 ? 0xffffffffu : 0u, hm1 = hin1 ? 0xffffffffu : 0u, hm2 = hin2 ? 0xffffffffu : 0u; \
  uint4 vh0_0, vh1_0, vh2_0, vh0_1, vh1_1, vh2_1, vh0_2, vh1_2, vh2_2, vh0_3, vh1_3, vh2_3;
#define OCC_BN_ISSUE_X(S, CH)                                                                     \
  {                                                                                               \
    const long cq = (long)(CH) * 4;                                                               \
    vh0_##S = x[hofs0 + cq]; vh1_##S = x[hofs1 + cq]; vh2_##S = x[hofs2 + cq];                    \
  }
#define OCC_BN_CH(CI) (((CI) + rot) % NCH)

#define OCC_BN_WAVE_TILES                                                                         \
  const int ntA = wave & 1, mtA0 = 3 * (wave >> 1);                                               \
  const int ntB = wave & 1, mtB0 = 2 * (wave >> 1);
#define OCC_BN_ISSUE_BIASES                                                                       \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                 \
    bA[g] = *reinterpret_cast<const float4*>(b1 + ntA * 32 + 8 * g + 4 * kb);                     \
    bB[g] = *reinterpret_cast<const float4*>(b2 + ntB * 32 + 8 * g + 4 * kb);                     \
  }
#define OCC_BN_ZERO_ACC(ACC, N)                                                                   \
  f32x16 ACC[N];                                                                                  \
  _Pragma("unroll") for (int j = 0; j < N; ++j)                                                   \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) ACC[j][r] = 0.f;
#define OCC_BN_ISSUE_W1(SLOT, CH)                                                                 \
  {                                                                                               \
    wa[SLOT][0] = w1p[(((long)(CH) * 2 + 0) * 2 + ntA) * 64 + lane];                              \
    wa[SLOT][1] = w1p[(((long)(CH) * 2 + 1) * 2 + ntA) * 64 + lane];                              \
  }

// out-of-image pixels are zero: AND with an all-ones / all-zeros mask
#define OCC_BN_STAGE_STORE(S, SX)                                                                 \
  if (hlive0) *reinterpret_cast<uint4*>(SX + hdst0) = make_uint4(vh0_##S.x & hm0, vh0_##S.y & hm0, vh0_##S.z & hm0, vh0_##S.w & hm0); \
  if (hlive1) *reinterpret_cast<uint4*>(SX + hdst1) = make_uint4(vh1_##S.x & hm1, vh1_##S.y & hm1, vh1_##S.z & hm1, vh1_##S.w & hm1); \
  if (hlive2) *reinterpret_cast<uint4*>(SX + hdst2) = make_uint4(vh2_##S.x & hm2, vh2_##S.y & hm2, vh2_##S.z & hm2, vh2_##S.w & hm2);
#define OCC_BN_W1_FRAGS(SLOT)                                                                     \
  const bf16x8 wf0 = __builtin_bit_cast(bf16x8, wa[SLOT][0]), wf1 = __builtin_bit_cast(bf16x8, wa[SLOT][1]);
#define OCC_BN_STEP_MFMA(SX)                                                                      \
  _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                                 \
    const bf16x8 af0 = *reinterpret_cast<const bf16x8*>(SX + ((mtA0 + j) * 32 + vi) * kBnXS + kb * 16);      \
    const bf16x8 af1 = *reinterpret_cast<const bf16x8*>(SX + ((mtA0 + j) * 32 + vi) * kBnXS + 32 + kb * 16); \
    acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf0, af0, acc1[j], 0, 0, 0);                \
    acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf1, af1, acc1[j], 0, 0, 0);                \
  }

// first W2 fragments in flight while c1 is written
#define OCC_BN_W2_PROLOGUE                                                                        \
  constexpr int PFB = 12;                                                                         \
  uint4 wr[PFB];                                                                                  \
  _Pragma("unroll") for (int s = 0; s < PFB; ++s) wr[s] = w2p[((long)s * 2 + ntB) * 64 + lane];
// c1 halo: bias + ReLU, zero outside the image (conv2's zero padding applies to c1, not to x)
#define OCC_BN_WRITE_C1                                                                           \
  _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                                 \
    const int p = (mtA0 + j) * 32 + vi;                                                           \
    const int hy = p / kBnHW, hx = p - hy * kBnHW;                                                \
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;                                                 \
    const float m = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? 1.f : 0.f;                         \
    if (p < kBnNP) {                                                                              \
      char* dst = sH1 + p * kBnMS + (ntA * 32 + 4 * kb) * 2;                                      \
      _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                             \
        const float v0 = fmaxf(acc1[j][4 * g + 0] + bA[g].x, 0.f) * m, v1 = fmaxf(acc1[j][4 * g + 1] + bA[g].y, 0.f) * m; \
        const float v2 = fmaxf(acc1[j][4 * g + 2] + bA[g].z, 0.f) * m, v3 = fmaxf(acc1[j][4 * g + 3] + bA[g].w, 0.f) * m; \
        *reinterpret_cast<uint2*>(dst + 16 * g) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3)); \
      }                                                                                           \
    }                                                                                             \
  }

// phase B: c2 = relu(conv3x3(c1) + b2), K = 9 taps x 64.  The ring keeps PFB weight loads in flight; the scheduling barrier
// keeps hipcc from sinking them behind the MFMAs (it would otherwise run the phase with two loads in flight,
// L2-latency-bound).  The next k-step's pixel fragments are read while this step's MFMAs run.
#define OCC_BN_PHASE_B                                                                            \
  OCC_BN_ZERO_ACC(acc2, 2)                                                                        \
  const int ab0 = (2 * mtB0 + (vi >> 4)) * kBnH1ROW + (vi & 15) * kBnMS + kb * 16;                \
  const int ab1 = ab0 + 2 * kBnH1ROW;                                                             \
  {                                                                                               \
    bf16x8 a0 = *reinterpret_cast<const bf16x8*>(sH1 + ab0), a1 = *reinterpret_cast<const bf16x8*>(sH1 + ab1); \
    _Pragma("unroll") for (int s = 0; s < 36; ++s) {                                              \
      const bf16x8 wf = __builtin_bit_cast(bf16x8, wr[s % PFB]);                                  \
      if (s + PFB < 36) wr[s % PFB] = w2p[((long)(s + PFB) * 2 + ntB) * 64 + lane];               \
      bf16x8 a0n = a0, a1n = a1;                                                                  \
      if (s + 1 < 36) {                                                                           \
        const int tap = (s + 1) >> 2, ks = (s + 1) & 3;                                           \
        const int toff = (tap / 3) * kBnH1ROW + (tap % 3) * kBnMS + ks * 32;                      \
        a0n = *reinterpret_cast<const bf16x8*>(sH1 + ab0 + toff);                                 \
        a1n = *reinterpret_cast<const bf16x8*>(sH1 + ab1 + toff);                                 \
      }                                                                                           \
      acc2[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, a0, acc2[0], 0, 0, 0);                \
      acc2[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, a1, acc2[1], 0, 0, 0);                \
      __builtin_amdgcn_sched_barrier(0);                                                          \
      a0 = a0n; a1 = a1n;                                                                         \
    }                                                                                             \
  }
#define OCC_BN_WRITE_C2                                                                           \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                 \
    char* dst = sC2 + ((mtB0 + j) * 32 + vi) * kBnMS + (ntB * 32 + 4 * kb) * 2;                   \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                               \
      const float v0 = fmaxf(acc2[j][4 * g + 0] + bB[g].x, 0.f), v1 = fmaxf(acc2[j][4 * g + 1] + bB[g].y, 0.f); \
      const float v2 = fmaxf(acc2[j][4 * g + 2] + bB[g].z, 0.f), v3 = fmaxf(acc2[j][4 * g + 3] + bB[g].w, 0.f); \
      *reinterpret_cast<uint2*>(dst + 16 * g) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3)); \
    }                                                                                             \
  }

#define OCC_BN_C_AFRAG(AF, RT, KS)                                                                \
  if ((KS) < 4) {                                                                                 \
    AF = *reinterpret_cast<const bf16x8*>(sC2 + ((RT) * 32 + vi) * kBnMS + (KS) * 32 + kb * 16);  \
  } else {                                                                                        \
    const int p = (2 * (RT) + (vi >> 4) + 1) * kBnHW + (vi & 15) + 1;                             \
    AF = *reinterpret_cast<const bf16x8*>(lds + (((KS) - 4) >> 1) * kBnXA + p * kBnXS + (((KS) - 4) & 1) * 32 + kb * 16); \
  }
