// The K loop of the backbone 3x3 convolutions (conv3x3_nhwc_bf16.hip has the GEMM view), as TEXT: conv3x3_nhwc_bf16_kernel
// and phase 1 of conv3x3_conv1x1_kernel both expand OCC_C3_KLOOP, so the two sum the same products in the same order by
// construction.  Macros on the kernel's locals and not __device__ functions: a function, even a __forceinline__ template,
// changes the register allocation of every instance (EXPERIMENTS.md section 8m); the preprocessor changes nothing.
//
// OCC_C3_KLOOP expects in scope
//   x, wp                       const uint4* __restrict__: the NHWC input and the conv3x3_pack_weight buffer
//   lds                         char*: 2 * HALO_BYTES of LDS, 16-byte aligned
//   acc                         f32x16 [RT][NT], zeroed
//   tid, lane, vi, kb           thread index, tid & 63, lane & 31, lane >> 5
//   img, y0, x0, H, W           the image and the first output pixel of the block's tile, the input map's size
//   CQ, NCH                     Cin / 8, Cin / 32
//   S, NT, PF, G, RT            stride, 32-column tiles per wave, weight ring depth, C3Geom<S, RT>, G::RT
//   kC3ROW, HALO_BYTES          G::ROW, G::HH * kC3ROW
// and three macros of the kernel's own, expanded where the statements stand:
//   OCC_C3_NT32                 Cout / 32 of the packed weight
//   OCC_C3_WTILE(T)             the wave's T-th 32-column tile (T = 0, NT - 1); clamped where the grid can overhang Cout
//   OCC_C3_ROT                  unsigned: the block's chunk rotation before the reduction mod NCH
// It declares its own locals (halo roles, weight ring, abase, rot, ...): expand it inside a block of its own.
#pragma once
#include "common.h"

namespace occ {

constexpr int kC3TW = 16;                             // output tile width (one MFMA row tile = 2 x 16 pixels)
constexpr int kC3PX = 80;                             // bytes per halo pixel slot (32 bf16 + 16 pad)
// Tile geometry per stride S: output tile TH x 16, input halo HH x HW.  Stride 2 keeps the halo columns
// DE-INTERLEAVED in LDS (17 even columns, then 17 odd-column slots): for a fixed tap the 16 output pixels of a
// row then read 16 CONSECUTIVE 80-byte slots, conflict-free like stride 1 (a 160-byte lane stride is not).
template <int S, int RT_> struct C3Geom {
  static constexpr int RT = RT_, TH = 2 * RT;
  static constexpr int HH = (TH - 1) * S + 3, HW = (kC3TW - 1) * S + 3;     // RT 4: 10 x 18  /  RT 2: 9 x 33
  // bytes per halo row: the two image rows of an MFMA row tile lie S rows apart, and S * ROW must be a multiple of the
  // 256-byte bank cycle for their 16-lane halves to share no bank in a ds_read_b128 lane group (stride 2 with 34
  // slots = 2720 B had 48 % bank-conflict cycles)
  static constexpr int ROW = S == 1 ? 1536 : 2816;
  static constexpr int ITEMS = HH * HW * 4, NR = (ITEMS + 255) / 256;       // 16-byte staging items / roles
  __device__ static constexpr int slot(int hx) { return S == 1 ? hx : (hx & 1) * 17 + (hx >> 1); }
};

// The tiles: variant = 10 * NT + RT (NT x 128 output channels, 4 waves x 32 * NT, 2 * RT x 16 output pixels per block)
// and the waves per SIMD each is compiled for (launch_bounds: what its registers, or at stride 2 its LDS, allow).
struct C3Variant { int stride, id, minw; };
constexpr C3Variant kC3Variants[] = {{1, 12, 3}, {1, 13, 3}, {1, 14, 3}, {1, 16, 2}, {1, 18, 2}, {1, 22, 2}, {1, 23, 2},
                                     {1, 24, 2}, {2, 12, 3}, {2, 13, 2}, {2, 22, 2}};
constexpr int c3_minw(int s, int id) {
  for (const C3Variant& v : kC3Variants)
    if (v.stride == s && v.id == id) return v.minw;
  return 0;
}

int c3_pick(long batch, int Ho, int Wo, int Cout, int stride);     // conv3x3_nhwc_bf16.hip

}  // namespace occ

// halo staging role K of a thread: which 16-byte piece of which halo pixel it loads (clamped) and where it goes in LDS
#define OCC_C3_HALO_ROLE(K, OFS, DST, IN, LIVE)                                                   \
  {                                                                                               \
    const int idx = tid + 256 * (K);                                                              \
    LIVE = idx < G::ITEMS;                                                                        \
    const int p = LIVE ? idx >> 2 : 0, piece = idx & 3;                                           \
    const int hy = p / G::HW, hx = p % G::HW;                                                     \
    const int iy = y0 * S - 1 + hy, ix = x0 * S - 1 + hx;                                         \
    IN = LIVE && iy >= 0 && iy < H && ix >= 0 && ix < W;                                          \
    const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);                           \
    OFS = (((long)img * H + cy) * W + cx) * CQ + piece;                                           \
    DST = hy * kC3ROW + G::slot(hx) * kC3PX + piece * 16;                                         \
  }
// request the halo of chunk CH (32 input channels = 4 pieces further along every pixel)
#define OCC_C3_ISSUE_HALO(CH)                                                                     \
  {                                                                                               \
    const long cq = (long)(CH) * 4;                                                               \
    vh0 = x[hofs0 + cq]; vh1 = x[hofs1 + cq];                                                     \
    if (NR > 2) vh2 = x[hofs2 + cq];                                                              \
    if (NR > 3) vh3 = x[hofs3 + cq];                                                              \
    if (NR > 4) vh4 = x[hofs4 + cq];                                                              \
    if (NR > 5) vh5 = x[hofs5 + cq];                                                              \
    if (NR > 6) vh6 = x[hofs6 + cq];                                                              \
    if (NR > 7) vh7 = x[hofs7 + cq];                                                              \
  }
// the wave's weight fragment of k-step T18 = (tap, ks) of chunk CHK, column tile T
#define OCC_C3_W(CHK, T18, T) wp[(((long)(CHK) * 18 + (T18)) * NT32) * 64 + ((T) == 0 ? wl0 : wl1)]
// the CI-th chunk the block visits: the chunk order is rotated per block (L2 channel hot-spotting, see
// conv1x1_nhwc_bf16.hip); past the end it repeats the last one (the ring and the halo request run one chunk ahead)
#define OCC_C3_CH(CI) ((((CI) < NCH ? (CI) : NCH - 1) + rot) % NCH)
// one chunk of 32 input channels: halo registers -> LDS buffer PAR, barrier, next chunk's halo requested,
// 18 k-steps straight out of the halo with compile-time tap offsets
#define OCC_C3_CHUNK(PAR, CI)                                                                     \
  {                                                                                               \
    char* sH = lds + (PAR) * HALO_BYTES;                                                          \
    /* out-of-image pixels are zero (the convolution's padding): AND with an all-ones / all-zeros mask */ \
    if (hlive0) *reinterpret_cast<uint4*>(sH + hdst0) = make_uint4(vh0.x & hm0, vh0.y & hm0, vh0.z & hm0, vh0.w & hm0); \
    if (hlive1) *reinterpret_cast<uint4*>(sH + hdst1) = make_uint4(vh1.x & hm1, vh1.y & hm1, vh1.z & hm1, vh1.w & hm1); \
    if (NR > 2 && hlive2) *reinterpret_cast<uint4*>(sH + hdst2) = make_uint4(vh2.x & hm2, vh2.y & hm2, vh2.z & hm2, vh2.w & hm2); \
    if (NR > 3 && hlive3) *reinterpret_cast<uint4*>(sH + hdst3) = make_uint4(vh3.x & hm3, vh3.y & hm3, vh3.z & hm3, vh3.w & hm3); \
    if (NR > 4 && hlive4) *reinterpret_cast<uint4*>(sH + hdst4) = make_uint4(vh4.x & hm4, vh4.y & hm4, vh4.z & hm4, vh4.w & hm4); \
    if (NR > 5 && hlive5) *reinterpret_cast<uint4*>(sH + hdst5) = make_uint4(vh5.x & hm5, vh5.y & hm5, vh5.z & hm5, vh5.w & hm5); \
    if (NR > 6 && hlive6) *reinterpret_cast<uint4*>(sH + hdst6) = make_uint4(vh6.x & hm6, vh6.y & hm6, vh6.z & hm6, vh6.w & hm6); \
    if (NR > 7 && hlive7) *reinterpret_cast<uint4*>(sH + hdst7) = make_uint4(vh7.x & hm7, vh7.y & hm7, vh7.z & hm7, vh7.w & hm7); \
    __syncthreads();   /* halo chunk visible; the other halo buffer is free for the next chunk */ \
    OCC_C3_ISSUE_HALO(OCC_C3_CH((CI) + 1))                                                        \
    const int ch_cur = OCC_C3_CH(CI), ch_nxt = OCC_C3_CH((CI) + 1);                               \
    bf16x8 af[RT], an[RT];                                                                        \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                             \
      af[rt] = *reinterpret_cast<const bf16x8*>(sH + abase[rt]);                                  \
    _Pragma("unroll") for (int s = 0; s < 18; ++s) {                                              \
      const int slot = ((PAR) * 18 + s) % PF;                                                     \
      bf16x8 wf[NT];                                                                              \
      _Pragma("unroll") for (int t = 0; t < NT; ++t) wf[t] = __builtin_bit_cast(bf16x8, wr[slot][t]); \
      {                                                                                           \
        const int sn = s + PF;                                                                    \
        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                            \
          wr[slot][t] = OCC_C3_W(sn < 18 ? ch_cur : ch_nxt, sn % 18, t);                          \
      }                                                                                           \
      if (s + 1 < 18) {                                                                           \
        const int tap = (s + 1) >> 1, ks = (s + 1) & 1;                                           \
        const int toff = (tap / 3) * kC3ROW + G::slot(tap % 3) * kC3PX + ks * 32;                 \
        _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                         \
          an[rt] = *reinterpret_cast<const bf16x8*>(sH + abase[rt] + toff);                       \
      }                                                                                           \
      _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                           \
        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                            \
          acc[rt][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[rt], wf[t], acc[rt][t], 0, 0, 0); \
      __builtin_amdgcn_sched_barrier(0);                                                          \
      if (s + 1 < 18) { _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) af[rt] = an[rt]; }      \
    }                                                                                             \
  }

// The loop.  In order:
//  * halo staging roles: HH x HW pixels x 4 pieces of 16 B over 256 threads (RT 4: 3 per thread at stride 1, RT 2: 5 at
//    stride 2; at most 8; clamped + zero-masked, unconditional loads).  Named scalars: small per-thread arrays written in
//    a loop end up in scratch with hipcc / ROCm 7.2;
//  * wl0, wl1: this wave's 32-column tiles in the packed weight, the uint4 index of (tile, lane) inside one
//    (chunk, tap, ks);
//  * abase: the A fragment base offsets (bytes) of this lane's pixel in each row tile, tap (0,0), k-step 0;
//  * weights: MFMA-fragment-ordered, global -> registers, a ring of PF k-steps in flight (k-step = (tap, ks), 18 per
//    chunk; the ring runs on across chunk boundaries).  Each wave owns its columns, so there is nothing to share through
//    LDS; the scheduling barrier per k-step keeps hipcc from sinking the prefetch;
//  * the chunks, two per trip: the halo is double buffered.
#define OCC_C3_KLOOP                                                                              \
  constexpr int NR = G::NR;                                                                       \
  static_assert(NR >= 2 && NR <= 8, "halo staging register budget");                              \
  long hofs0, hofs1, hofs2 = 0, hofs3 = 0, hofs4 = 0, hofs5 = 0, hofs6 = 0, hofs7 = 0;            \
  int hdst0, hdst1, hdst2 = 0, hdst3 = 0, hdst4 = 0, hdst5 = 0, hdst6 = 0, hdst7 = 0;             \
  bool hin0, hin1, hin2 = false, hin3 = false, hin4 = false, hin5 = false, hin6 = false, hin7 = false; \
  bool hlive0, hlive1, hlive2 = false, hlive3 = false, hlive4 = false, hlive5 = false, hlive6 = false, hlive7 = false; \
  OCC_C3_HALO_ROLE(0, hofs0, hdst0, hin0, hlive0)                                                 \
  OCC_C3_HALO_ROLE(1, hofs1, hdst1, hin1, hlive1)                                                 \
  if (NR > 2) OCC_C3_HALO_ROLE(2, hofs2, hdst2, hin2, hlive2)                                     \
  if (NR > 3) OCC_C3_HALO_ROLE(3, hofs3, hdst3, hin3, hlive3)                                     \
  if (NR > 4) OCC_C3_HALO_ROLE(4, hofs4, hdst4, hin4, hlive4)                                     \
  if (NR > 5) OCC_C3_HALO_ROLE(5, hofs5, hdst5, hin5, hlive5)                                     \
  if (NR > 6) OCC_C3_HALO_ROLE(6, hofs6, hdst6, hin6, hlive6)                                     \
  if (NR > 7) OCC_C3_HALO_ROLE(7, hofs7, hdst7, hin7, hlive7)                                     \
  const int NT32 = OCC_C3_NT32;                                                                   \
  static_assert(NT <= 2, "weight ring register budget");                                          \
  const long wl0 = (long)(OCC_C3_WTILE(0)) * 64 + lane;                                           \
  const long wl1 = (long)(OCC_C3_WTILE(NT - 1)) * 64 + lane;                                      \
  int abase[RT];                                                                                  \
  _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                               \
    abase[rt] = (2 * rt + (vi >> 4)) * S * kC3ROW + (vi & 15) * kC3PX + kb * 16;                  \
  uint4 vh0, vh1, vh2, vh3, vh4, vh5, vh6, vh7;                                                   \
  const unsigned hm0 = hin0 ? 0xffffffffu : 0u, hm1 = hin1 ? 0xffffffffu : 0u, hm2 = hin2 ? 0xffffffffu : 0u; \
  const unsigned hm3 = hin3 ? 0xffffffffu : 0u, hm4 = hin4 ? 0xffffffffu : 0u, hm5 = hin5 ? 0xffffffffu : 0u; \
  const unsigned hm6 = hin6 ? 0xffffffffu : 0u, hm7 = hin7 ? 0xffffffffu : 0u;                    \
  static_assert(36 % PF == 0 && PF <= 18, "ring slot pattern repeats every two chunks");          \
  uint4 wr[PF][NT];                                                                               \
  const int rot = (int)((OCC_C3_ROT) % (unsigned)NCH);                                            \
  OCC_C3_ISSUE_HALO(OCC_C3_CH(0))                                                                 \
  _Pragma("unroll") for (int s = 0; s < PF; ++s)                                                  \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) wr[s][t] = OCC_C3_W(OCC_C3_CH(0), s, t);       \
  for (int ch = 0; ch < NCH; ch += 2) {                                                           \
    OCC_C3_CHUNK(0, ch)                                                                           \
    if (ch + 1 < NCH) OCC_C3_CHUNK(1, ch + 1)                                                     \
  }
