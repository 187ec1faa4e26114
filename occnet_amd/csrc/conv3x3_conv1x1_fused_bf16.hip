// ResNet bottleneck tail in ONE launch (NHWC bf16): the 3x3 convolution (conv2) and the 1x1 expansion after it (conv3),
//   out = relu( conv1x1( bf16( relu(conv3x3(x, W2, stride s) + b2) ), W3 ) + b3 + residual ),
// for Cmid in {128, 256}, Cout = 4 Cmid, stride 1 or 2, residual of the output's size.  The pair of launches it replaces
// (conv3x3_nhwc_bf16.hip, then conv1x1_resident_bf16.hip) runs a matrix-pipe-bound kernel that leaves HBM idle and then an
// HBM-bound kernel that leaves the matrix cores idle, and writes the mid tensor to HBM only to read it back.  Here the mid
// tile never leaves the CU, and with two or three blocks per CU the residual loads and row stores of one block travel under
// the 3x3 MFMAs of another.
//
// A block = 4 waves = one 3x3 tile that holds ALL mid channels: variant id 10 NT + RT with 128 NT = Cmid, (2 RT) x 16 output
// pixels.  Two phases:
//   1. the body of conv3x3_nhwc_bf16_kernel, COPIED from conv3x3_nhwc_bf16.hip (halo chunks double buffered in LDS, weight
//      ring of 6 k-steps on the conv3x3_pack_weight buffer, chunk rotation from the tile index exactly as that kernel derives
//      it from blockIdx.x with blockIdx.y = 0), so the f32 sums are the same bits.  Its epilogue adds the bias in f32, applies
//      the ReLU, rounds ONCE and writes the bf16 tile into LDS - over the halo buffers, which are dead by then - in the
//      row-swizzled 16-byte-piece layout of conv1x1_resident_kernel (rows = the pixels of the patch in MFMA row-tile order,
//      32 rt + 16 (y & 1) + x).  Pixels outside the map are written as zeros and never stored.
//   2. the pass loop of conv1x1_resident_kernel, COPIED from conv1x1_resident_bf16.hip, on that tile (transposed MFMAs on the
//      conv1x1_pack_weight buffer, 4-deep weight ring across k-steps and passes, accumulators start at the bias staged in
//      LDS, K ascending, residual prefetched RD tiles ahead as 16-byte row segments, add / ReLU / one rounding in the
//      per-wave scratch, 16-byte row-segment stores).  Output and residual addresses come from (oy, ox) of the row with a
//      bounds mask; the block walks all Cout / 256 column passes itself.
// The copies (instead of shared __device__ pieces) keep the two parent kernels' code generation untouched.
// For a given tile id the result is bit-identical to conv3x3 (that tile) followed by the resident conv1x1.
#include "common.h"

namespace occ {

int c3_pick(long batch, int Ho, int Wo, int Cout, int stride);     // conv3x3_nhwc_bf16.hip

namespace {

constexpr int kF31TW = 16, kF31PX = 80;                          // = kC3TW, kC3PX
constexpr int kF31Pitch = 80, kF31Scratch = 32 * kF31Pitch;      // = kC1rPitch, kC1rScratch

template <int S, int RT_> struct F31Geom {                       // = C3Geom
  static constexpr int RT = RT_, TH = 2 * RT;
  static constexpr int HH = (TH - 1) * S + 3, HW = (kF31TW - 1) * S + 3;
  static constexpr int ROW = S == 1 ? 1536 : 2816;
  static constexpr int ITEMS = HH * HW * 4, NR = (ITEMS + 255) / 256;
  __device__ static constexpr int slot(int hx) { return S == 1 ? hx : (hx & 1) * 17 + (hx >> 1); }
};

// LDS of a block: the two halo buffers of phase 1, overlaid in phase 2 by mid tile + the four waves' scratch + the bias
constexpr int f31_lds_bytes(int nt, int s, int rt) {
  const int hh = (2 * rt - 1) * s + 3;
  const int halo = 2 * hh * (s == 1 ? 1536 : 2816);
  const int p2 = 32 * rt * (128 * nt) * 2 + 4 * kF31Scratch + 512 * nt * 4;
  return halo > p2 ? halo : p2;
}

template <int NT, int S, int RT_, int MINW, int RD>
__global__ __launch_bounds__(256, MINW) void conv3x3_conv1x1_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ wp, const float* __restrict__ bias2,
    const uint4* __restrict__ wp3, const float* __restrict__ bias3, const unsigned short* __restrict__ residual,
    unsigned short* __restrict__ out, int H, int W, int Ho, int Wo, int tiles_x, int tiles_y) {
  using G = F31Geom<S, RT_>;
  constexpr int PF = 6;
  constexpr int RT = G::RT, WR = 32 * NT;
  constexpr int Cin = 128 * NT, Cmid = 128 * NT, N = 4 * Cmid;
  constexpr int kC3ROW = G::ROW, kC3TH = G::TH;
  constexpr int HALO_BYTES = G::HH * kC3ROW;
  extern __shared__ __attribute__((aligned(16))) char flds[];
  char* const lds = flds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  int bid = blockIdx.x;
  const int tx_i = bid % tiles_x; bid /= tiles_x;
  const int ty_i = bid % tiles_y;
  const int img = bid / tiles_y;
  const int y0 = ty_i * kC3TH, x0 = tx_i * kF31TW;
  const int nw0 = wave * WR;
  constexpr int CQ = Cin / 8, NCH = Cin / 32;

  f32x16 acc[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][t][r] = 0.f;

  // ---- phase 1: conv3x3_nhwc_bf16_kernel's K loop (see there for the commentary) ----------------------------------------
  constexpr int NR = G::NR;
  static_assert(NR >= 2 && NR <= 8, "halo staging register budget");
  long hofs0, hofs1, hofs2 = 0, hofs3 = 0, hofs4 = 0, hofs5 = 0, hofs6 = 0, hofs7 = 0;
  int hdst0, hdst1, hdst2 = 0, hdst3 = 0, hdst4 = 0, hdst5 = 0, hdst6 = 0, hdst7 = 0;
  bool hin0, hin1, hin2 = false, hin3 = false, hin4 = false, hin5 = false, hin6 = false, hin7 = false;
  bool hlive0, hlive1, hlive2 = false, hlive3 = false, hlive4 = false, hlive5 = false, hlive6 = false, hlive7 = false;
#define OCC_F31_HALO_ROLE(K, OFS, DST, IN, LIVE)                                                  \
  {                                                                                               \
    const int idx = tid + 256 * (K);                                                              \
    LIVE = idx < G::ITEMS;                                                                        \
    const int p = LIVE ? idx >> 2 : 0, piece = idx & 3;                                           \
    const int hy = p / G::HW, hx = p % G::HW;                                                     \
    const int iy = y0 * S - 1 + hy, ix = x0 * S - 1 + hx;                                         \
    IN = LIVE && iy >= 0 && iy < H && ix >= 0 && ix < W;                                          \
    const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);                           \
    OFS = (((long)img * H + cy) * W + cx) * CQ + piece;                                           \
    DST = hy * kC3ROW + G::slot(hx) * kF31PX + piece * 16;                                        \
  }
  OCC_F31_HALO_ROLE(0, hofs0, hdst0, hin0, hlive0)
  OCC_F31_HALO_ROLE(1, hofs1, hdst1, hin1, hlive1)
  if (NR > 2) OCC_F31_HALO_ROLE(2, hofs2, hdst2, hin2, hlive2)
  if (NR > 3) OCC_F31_HALO_ROLE(3, hofs3, hdst3, hin3, hlive3)
  if (NR > 4) OCC_F31_HALO_ROLE(4, hofs4, hdst4, hin4, hlive4)
  if (NR > 5) OCC_F31_HALO_ROLE(5, hofs5, hdst5, hin5, hlive5)
  if (NR > 6) OCC_F31_HALO_ROLE(6, hofs6, hdst6, hin6, hlive6)
  if (NR > 7) OCC_F31_HALO_ROLE(7, hofs7, hdst7, hin7, hlive7)
#undef OCC_F31_HALO_ROLE
  constexpr int NT32 = Cmid / 32;
  static_assert(NT <= 2, "weight ring register budget");
  const long wl0 = (long)(nw0 / 32) * 64 + lane;
  const long wl1 = (long)(nw0 / 32 + NT - 1) * 64 + lane;
  int abase[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    abase[rt] = (2 * rt + (vi >> 4)) * S * kC3ROW + (vi & 15) * kF31PX + kb * 16;

  uint4 vh0, vh1, vh2, vh3, vh4, vh5, vh6, vh7;
  const unsigned hm0 = hin0 ? 0xffffffffu : 0u, hm1 = hin1 ? 0xffffffffu : 0u, hm2 = hin2 ? 0xffffffffu : 0u;
  const unsigned hm3 = hin3 ? 0xffffffffu : 0u, hm4 = hin4 ? 0xffffffffu : 0u, hm5 = hin5 ? 0xffffffffu : 0u;
  const unsigned hm6 = hin6 ? 0xffffffffu : 0u, hm7 = hin7 ? 0xffffffffu : 0u;
#define OCC_F31_ISSUE_HALO(CH)                                                                    \
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
  static_assert(36 % PF == 0 && PF <= 18, "ring slot pattern repeats every two chunks");
  uint4 wr[PF][NT];
#define OCC_F31_W(CHK, T18, T) wp[(((long)(CHK) * 18 + (T18)) * NT32) * 64 + ((T) == 0 ? wl0 : wl1)]

  const int rot = (int)((blockIdx.x * 5u) % (unsigned)NCH);
#define OCC_F31_CH(CI) ((((CI) < NCH ? (CI) : NCH - 1) + rot) % NCH)
  OCC_F31_ISSUE_HALO(OCC_F31_CH(0))
#pragma unroll
  for (int s = 0; s < PF; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) wr[s][t] = OCC_F31_W(OCC_F31_CH(0), s, t);

#define OCC_F31_CHUNK(PAR, CI)                                                                    \
  {                                                                                               \
    char* sH = lds + (PAR) * HALO_BYTES;                                                          \
    if (hlive0) *reinterpret_cast<uint4*>(sH + hdst0) = make_uint4(vh0.x & hm0, vh0.y & hm0, vh0.z & hm0, vh0.w & hm0); \
    if (hlive1) *reinterpret_cast<uint4*>(sH + hdst1) = make_uint4(vh1.x & hm1, vh1.y & hm1, vh1.z & hm1, vh1.w & hm1); \
    if (NR > 2 && hlive2) *reinterpret_cast<uint4*>(sH + hdst2) = make_uint4(vh2.x & hm2, vh2.y & hm2, vh2.z & hm2, vh2.w & hm2); \
    if (NR > 3 && hlive3) *reinterpret_cast<uint4*>(sH + hdst3) = make_uint4(vh3.x & hm3, vh3.y & hm3, vh3.z & hm3, vh3.w & hm3); \
    if (NR > 4 && hlive4) *reinterpret_cast<uint4*>(sH + hdst4) = make_uint4(vh4.x & hm4, vh4.y & hm4, vh4.z & hm4, vh4.w & hm4); \
    if (NR > 5 && hlive5) *reinterpret_cast<uint4*>(sH + hdst5) = make_uint4(vh5.x & hm5, vh5.y & hm5, vh5.z & hm5, vh5.w & hm5); \
    if (NR > 6 && hlive6) *reinterpret_cast<uint4*>(sH + hdst6) = make_uint4(vh6.x & hm6, vh6.y & hm6, vh6.z & hm6, vh6.w & hm6); \
    if (NR > 7 && hlive7) *reinterpret_cast<uint4*>(sH + hdst7) = make_uint4(vh7.x & hm7, vh7.y & hm7, vh7.z & hm7, vh7.w & hm7); \
    __syncthreads();                                                                              \
    OCC_F31_ISSUE_HALO(OCC_F31_CH((CI) + 1))                                                      \
    const int ch_cur = OCC_F31_CH(CI), ch_nxt = OCC_F31_CH((CI) + 1);                             \
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
          wr[slot][t] = OCC_F31_W(sn < 18 ? ch_cur : ch_nxt, sn % 18, t);                         \
      }                                                                                           \
      if (s + 1 < 18) {                                                                           \
        const int tap = (s + 1) >> 1, ks = (s + 1) & 1;                                           \
        const int toff = (tap / 3) * kC3ROW + G::slot(tap % 3) * kF31PX + ks * 32;                \
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
  for (int ch = 0; ch < NCH; ch += 2) {
    OCC_F31_CHUNK(0, ch)
    if (ch + 1 < NCH) OCC_F31_CHUNK(1, ch + 1)
  }
#undef OCC_F31_CHUNK
#undef OCC_F31_ISSUE_HALO
#undef OCC_F31_W
#undef OCC_F31_CH

  // ---- phase 2 set-up that can travel under the hand-over: weight ring and residual requests ----------------------------
  constexpr int K = Cmid, NTW = 2;
  constexpr int PCS = K / 8, PITCH = K * 2, KS = K / 16, NP = N / (128 * NTW);
  constexpr int MASK = (PCS < 32 ? PCS : 32) - 1;
  constexpr int TILE_BYTES = 32 * RT * PITCH;
  constexpr int NTILES = RT * NTW;
  constexpr int N32 = N / 32;
  static_assert(KS % 4 == 0 && NTILES >= 2 && RD >= 1 && RD <= NTILES, "tile geometry");
  static_assert(2 * HALO_BYTES <= f31_lds_bytes(NT, S, RT) && TILE_BYTES + 4 * kF31Scratch + N * 4 <= f31_lds_bytes(NT, S, RT),
                "LDS overlay");

  occ_u32x4 w[4][NTW];
  const __amdgpu_buffer_rsrc_t wrs = uniform_rsrc(wp3, (unsigned)K * (unsigned)N * 2u);
  const int wv = (wave * NTW * 64 + lane) * 16;
  constexpr int kstep_bytes = N32 * 1024;
#define OCC_F31_LOAD(SLOT, PASS, KSTEP)                                                            \
  {                                                                                               \
    const int so = (KSTEP) * kstep_bytes + (PASS) * (4 * NTW * 1024);                             \
    _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                               \
      w[SLOT][t] = __builtin_amdgcn_raw_buffer_load_b128(wrs, wv + t * 1024, so, 0);              \
  }
  OCC_F31_LOAD(0, 0, 0)
  OCC_F31_LOAD(1, 0, 1)
  OCC_F31_LOAD(2, 0, 2)

  // residual row segments of tile (rt, t) of the pass whose first column (for this wave) is NW: lane -> tile rows
  // (lane >> 2) and + 16 = image rows y0 + 2 rt and + 1 at column x0 + (lane >> 2), 16-byte piece lane & 3 (clamped loads)
  const long img_row0 = (long)img * Ho;
#define OCC_F31_RES(DST, NW, RTI, TI)                                                              \
  {                                                                                               \
    const int rx = min(x0 + (rlane >> 2), Wo - 1);                                                \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                               \
      const int ry = min(y0 + 2 * (RTI) + j, Ho - 1);                                             \
      DST[j] = *reinterpret_cast<const uint4*>(residual + ((img_row0 + ry) * Wo + rx) * N + (NW) + (TI) * 32 + (rlane & 3) * 8); \
    }                                                                                             \
  }
  uint4 rq[RD][2];
  int rlane = lane;
  {
    const int nwf = wave * (32 * NTW);
#pragma unroll
    for (int i = 0; i < RD; ++i) OCC_F31_RES(rq[i], nwf, i / NTW, i % NTW)
  }

  // ---- phase 1 epilogue: bias, ReLU, one rounding; the bf16 tile goes over the halo buffers ----------------------------
  __syncthreads();                                  // every wave is done reading the halo
  float* const sbias = reinterpret_cast<float*>(lds + TILE_BYTES + 4 * kF31Scratch);
  for (int i = tid; i < N / 4; i += 256)
    *reinterpret_cast<float4*>(sbias + 4 * i) = *reinterpret_cast<const float4*>(bias3 + 4 * i);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = nw0 + t * 32 + vi;                // the lane's mid channel; register r = tile row (r & 3) + 8 (r >> 2) + 4 kb
    const float bv = bias2[c];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * kb;
        const int oy = y0 + 2 * rt + (row >> 4), ox = x0 + (row & 15);
        const float v = fmaxf(acc[rt][t][r] + bv, 0.f);
        const unsigned short h = (oy < Ho && ox < Wo) ? bf16_rne(v) : (unsigned short)0;
        const int trow = rt * 32 + row;
        *reinterpret_cast<unsigned short*>(lds + trow * PITCH + (((c >> 3) ^ (trow & MASK)) << 4) + (c & 7) * 2) = h;
      }
  }
  __syncthreads();                                  // the mid tile and the bias are in LDS; no block barrier after this

  // ---- phase 2: conv1x1_resident_kernel's pass loop (see there for the commentary) -------------------------------------
  char* const scratch = lds + TILE_BYTES + wave * kF31Scratch;
  bf16x8 af[2][RT];
  unsigned abase2 = (unsigned)(vi * PITCH + ((kb ^ vi) & MASK) * 16);
#define OCC_F31_AFRAG(BUF, KSTEP)                                                                  \
  {                                                                                               \
    asm volatile("" : "+v"(abase2));                                                              \
    const char* ap = lds + (abase2 ^ (unsigned)((KSTEP) * 32));                                   \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                             \
      af[BUF][rt] = *reinterpret_cast<const bf16x8*>(ap + rt * (32 * PITCH));                     \
  }
  OCC_F31_AFRAG(0, 0)
#pragma unroll 1
  for (int p = 0; p < NP; ++p) {
    const int nw = p * (128 * NTW) + wave * (32 * NTW);
    int elane = lane;
    asm volatile("" : "+v"(elane));
    f32x16 acc2[RT][NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 c0 = *reinterpret_cast<const float4*>(sbias + nw + t * 32 + 8 * q + 4 * kb);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          acc2[rt][t][4 * q + 0] = c0.x;
          acc2[rt][t][4 * q + 1] = c0.y;
          acc2[rt][t][4 * q + 2] = c0.z;
          acc2[rt][t][4 * q + 3] = c0.w;
        }
      }
    const int pn = p + 1 < NP ? p + 1 : p;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 3 < KS) OCC_F31_LOAD((ks + 3) & 3, p, ks + 3)
      else OCC_F31_LOAD((ks + 3) & 3, pn, ks + 3 - KS)
      OCC_F31_AFRAG((ks + 1) & 1, (ks + 1) & (KS - 1))
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
          acc2[rt][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[ks & 3][t]), af[ks & 1][rt],
                                                                acc2[rt][t], 0, 0, 0);
      {
        constexpr int MQ = NTILES / 4, MR = NTILES - 3 * MQ;
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, (RT + 1) / 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, MR, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, RT / 2, 0);
      }
    }

    const int erow = elane >> 2, epiece = elane & 3;
    const int ex = x0 + erow;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        const int e = rt * NTW + t;
        {
          const uint4 r0 = rq[0][0], r1 = rq[0][1];
#pragma unroll
          for (int i = 0; i + 1 < RD; ++i) { rq[i][0] = rq[i + 1][0]; rq[i][1] = rq[i + 1][1]; }
          asm volatile("" : "+v"(rlane));
          if (e + RD < NTILES) OCC_F31_RES(rq[RD - 1], nw, (e + RD) / NTW, (e + RD) % NTW)
          else if (p + 1 < NP) OCC_F31_RES(rq[RD - 1], nw + 128 * NTW, (e + RD - NTILES) / NTW, (e + RD - NTILES) % NTW)
          *reinterpret_cast<uint4*>(scratch + erow * kF31Pitch + epiece * 16) = r0;
          *reinterpret_cast<uint4*>(scratch + (erow + 16) * kF31Pitch + epiece * 16) = r1;
          wave_lds_sync();
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          char* const sp = scratch + vi * kF31Pitch + 16 * q + 8 * kb;
          float v0 = acc2[rt][t][4 * q + 0], v1 = acc2[rt][t][4 * q + 1], v2 = acc2[rt][t][4 * q + 2],
                v3 = acc2[rt][t][4 * q + 3];
          const uint2 r = *reinterpret_cast<const uint2*>(sp);
          v0 += bf16_lo_to_f32(r.x); v1 += bf16_hi_to_f32(r.x); v2 += bf16_lo_to_f32(r.y); v3 += bf16_hi_to_f32(r.y);
          v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
          *reinterpret_cast<uint2*>(sp) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int row = erow + 16 * j;
          const int oy = y0 + 2 * rt + j;
          const uint4 v = *reinterpret_cast<const uint4*>(scratch + row * kF31Pitch + epiece * 16);
          if (oy < Ho && ex < Wo)
            *reinterpret_cast<uint4*>(out + ((img_row0 + oy) * Wo + ex) * N + nw + t * 32 + epiece * 8) = v;
        }
        wave_lds_sync();
      }
    }
  }
#undef OCC_F31_RES
#undef OCC_F31_AFRAG
#undef OCC_F31_LOAD
}

// The tiles the fused kernel is built for (a 3x3 tile that holds all Cmid channels: 128 NT = Cmid) and the waves per SIMD
// each is compiled for - those of the 3x3 variant of the same id.
struct F31Variant { int stride, id, minw; };
constexpr F31Variant kF31Variants[] = {{1, 12, 3}, {1, 22, 2}, {1, 23, 2}, {1, 24, 2},
                                       {2, 12, 3}, {2, 13, 2}, {2, 22, 2}};
constexpr int f31_minw(int s, int id) {
  for (const F31Variant& v : kF31Variants)
    if (v.stride == s && v.id == id) return v.minw;
  return 0;
}
bool f31_has(int Cmid, int stride, int id) { return f31_minw(stride, id) != 0 && (id / 10) * 128 == Cmid; }

bool f31_shape_ok(int Cmid, int Cout, int stride) {
  return (Cmid == 128 || Cmid == 256) && Cout == 4 * Cmid && (stride == 1 || stride == 2);
}

}  // namespace
}  // namespace occ

// Tile id (10 NT + RT) the fused launch uses for a shape, or 0 when the shape stays on the two launches.  A pure function.
// The rule: the tile is the one the 3x3 launcher picks for conv2 (c3_pick), so that the fused launch returns the bits of
// the pair it replaces; it must hold all mid channels in one block and have a fused kernel; and the grid must give every
// CU at least one block - a fused block walks all column passes of conv3 itself, so a small map cannot be spread over the
// machine the way the resident 1x1 kernel spreads it by splitting the passes.  Of the four layer2 / layer3 shapes of a
// base-config step this keeps one on the pair: 256 -> 1024 at stride 2, where c3_pick takes tile 12 (two column blocks)
// and the fused launch at tile 22, the only one it has there, measured no faster in the plan than that pair
// (EXPERIMENTS.md section 8i).
extern "C" int occ_conv3x3_conv1x1_pick(int batch, int H, int W, int Cmid, int Cout, int stride) {
  using namespace occ;
  if (batch <= 0 || H <= 0 || W <= 0 || !f31_shape_ok(Cmid, Cout, stride)) return 0;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int id = c3_pick(batch, Ho, Wo, Cmid, stride);
  if (!f31_has(Cmid, stride, id)) return 0;
  const int rt = id % 10;
  const long blocks = (long)batch * ((Wo + kF31TW - 1) / kF31TW) * ((Ho + 2 * rt - 1) / (2 * rt));
  if (blocks < 256) return 0;
  return id;
}

extern "C" int occ_conv3x3_conv1x1_nhwc_bf16(const void* x, const void* w3x3_packed, const float* b2,
                                             const void* w1x1_frag, const float* b3, const void* residual, void* out,
                                             int batch, int H, int W, int Cmid, int Cout, int stride, int variant,
                                             void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(x && w3x3_packed && b2 && w1x1_frag && b3 && residual && out,
                "conv3x3_conv1x1_nhwc_bf16: null pointer argument");
  OCC_CHECK_ARG(batch > 0 && H > 0 && W > 0 && Cmid > 0 && Cout > 0, "conv3x3_conv1x1_nhwc_bf16: bad dimension");
  if (!f31_shape_ok(Cmid, Cout, stride)) {
    set_error("conv3x3_conv1x1_nhwc_bf16: no kernel for Cmid=%d Cout=%d stride=%d (need Cmid 128 or 256, Cout = 4 Cmid, "
              "stride 1 or 2)", Cmid, Cout, stride);
    return OCC_E_UNSUPPORTED;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  int id = variant;
  if (id == 0) {
    id = occ_conv3x3_conv1x1_pick(batch, H, W, Cmid, Cout, stride);
    if (id == 0) {
      set_error("conv3x3_conv1x1_nhwc_bf16: shape %d x %d x %d (Cmid %d, stride %d) stays on the two launches "
                "(occ_conv3x3_conv1x1_pick returns 0)", batch, H, W, Cmid, stride);
      return OCC_E_UNSUPPORTED;
    }
  }
  if (!f31_has(Cmid, stride, id)) {
    set_error("conv3x3_conv1x1_nhwc_bf16: no variant %d at stride %d, Cmid %d (Cmid 128: 12, and 13 at stride 2; Cmid 256: "
              "22, and 23, 24 at stride 1)", variant, stride, Cmid);
    return OCC_E_UNSUPPORTED;
  }
  const long in_px = (long)batch * H * W, out_px = (long)batch * Ho * Wo;
  if (in_px * Cmid >= (1L << 40) || out_px * Cout >= (1L << 40)) {
    set_error("conv3x3_conv1x1_nhwc_bf16: tensor too large");
    return OCC_E_UNSUPPORTED;
  }
  const int rt = id % 10;
  const int tiles_x = (Wo + kF31TW - 1) / kF31TW, tiles_y = (Ho + 2 * rt - 1) / (2 * rt);
  const long blocks = (long)batch * tiles_x * tiles_y;
  if (blocks >= (1L << 31)) {
    set_error("conv3x3_conv1x1_nhwc_bf16: grid too large");
    return OCC_E_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  // RDD = residual tiles in flight per wave (8 VGPRs each): what the register budget of the instance leaves
#define OCC_F31_GO(SS, ID, RDD)                                                                     \
  {                                                                                               \
    auto kern = conv3x3_conv1x1_kernel<ID / 10, SS, ID % 10, f31_minw(SS, ID), RDD>;               \
    constexpr int lds = f31_lds_bytes(ID / 10, SS, ID % 10);                                      \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
    if (e == hipSuccess)                                                                          \
      hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, reinterpret_cast<const uint4*>(x), \
                         reinterpret_cast<const uint4*>(w3x3_packed), b2, reinterpret_cast<const uint4*>(w1x1_frag), b3, \
                         reinterpret_cast<const unsigned short*>(residual), reinterpret_cast<unsigned short*>(out), H, W, \
                         Ho, Wo, tiles_x, tiles_y);                                               \
  }
  if (stride == 1) {
    switch (id) {
      case 12: OCC_F31_GO(1, 12, 2) break;
      case 22: OCC_F31_GO(1, 22, 4) break;
      case 23: OCC_F31_GO(1, 23, 4) break;
      default: OCC_F31_GO(1, 24, 2) break;
    }
  } else {
    switch (id) {
      case 12: OCC_F31_GO(2, 12, 2) break;
      case 13: OCC_F31_GO(2, 13, 4) break;
      default: OCC_F31_GO(2, 22, 4) break;
    }
  }
#undef OCC_F31_GO
  if (e != hipSuccess) {
    set_error("conv3x3_conv1x1_nhwc_bf16: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    return OCC_E_LAUNCH;
  }
  OCC_CHECK_LAUNCH("conv3x3_conv1x1_nhwc_bf16");
  return OCC_OK;
}
