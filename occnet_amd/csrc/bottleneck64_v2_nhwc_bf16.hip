// Second kernel of the whole 64-mid-channel bottleneck (bottleneck64_nhwc_bf16.hip has the first one, the structure and the
// LDS layout; phases A and B are the same text).  It computes the same bits and differs in what it moves:
//
//   * identity from the staged tile.  Every centre pixel's 256 input channels pass through the two x chunk buffers during
//     phase A.  Phase C runs with the WEIGHTS as the row operand like phases A and B (D[channel][pixel]: a lane owns one
//     pixel and groups of 4 consecutive channels), wave w owns output channels 64w .. 64w+63 of all 128 pixels, and those
//     are exactly chunks 2w and 2w+1 of x: the wave copies them out of the chunk buffer at the two phase-A steps where they
//     are resident (32 ds_read_b64 per lane, 64 VGPRs of packed bf16) and the epilogue adds them from registers.  x is not
//     read a second time; the f32 LDS transpose, its eight block barriers and the identity prefetch queue are gone.  Rows
//     leave through a per-wave bf16 scratch (32 pixels x 128 B) as 16-byte pieces of whole 128-byte lines.
//   * block -> tile map.  Blocks b, b+8, b+16, ... share an XCD (one L2); bn64_tile_of_block hands each of the eight
//     groups a contiguous range of a walk over the tiles in which a tile's neighbours follow it closely, so a halo line is
//     fetched from memory once per L2 and not once per tile.  Measured (EXPERIMENTS.md section 8q): a fifth fewer bytes
//     fetched and 2 - 3 % MORE time than tile = block, which the launcher therefore keeps as the default order.
//
// Per output element the arithmetic is the first kernel's: conv1's chunk rotation is keyed on the TILE (the value
// blockIdx.x has there), the K order of every GEMM is unchanged (an MFMA with its operands swapped sums the same products
// in the same order), then acc + (b3 + identity), ReLU, one RNE rounding.
#include "common.h"

namespace occ {

constexpr int kB2TH = 8, kB2TW = 16, kB2HH = 10, kB2HW = 18, kB2NP = kB2HH * kB2HW;   // 180 halo pixels
constexpr int kB2XS = 80;                    // bytes per x-chunk pixel slot (32 bf16 + 16 pad)
constexpr int kB2XA = 192 * kB2XS;           // one x chunk buffer (6 row tiles of 32 halo pixels)
constexpr int kB2MS = 144;                   // bytes per 64-channel pixel slot (128 + 16 pad)
constexpr int kB2H1ROW = kB2HW * kB2MS;      // 2592
constexpr int kB2H1 = kB2HH * kB2H1ROW;      // 25 920
constexpr int kB2C2 = 128 * kB2MS;           // 18 432
constexpr int kB2OS = 32 * kB2MS;            // one wave's epilogue scratch: 32 pixels x 64 channels bf16, padded rows
constexpr int kB2Band = 4;                   // tile rows per band of the banded walk

// Tile (row-major linear index over image, tile row, tile column) of a block.
//   order 0: tile = block (the first kernel's map: neighbours lie on eight different L2s)
//   order 1: XCD-contiguous.  Group x = block % 8 takes positions x*q + min(x, r) + j, j = block / 8, of the row-major
//            walk (q = n / 8, r = n % 8: bijective for any n).  Horizontal neighbours follow each other, vertical ones
//            are tiles_x positions apart.
//   order 2: the same ranges over a walk in bands of kB2Band tile rows per image, column by column inside a band:
//            a vertical neighbour follows directly, a horizontal one kB2Band positions later; only the rows between
//            two bands (and between two groups' ranges) see their halo twice.
__host__ __device__ inline int bn64_tile_of_block(int block, int n_blocks, int tiles_x, int tiles_y, int order) {
  if (order == 0) return block;
  const int q = n_blocks >> 3, r = n_blocks & 7, x = block & 7, j = block >> 3;
  const int p = x * q + (x < r ? x : r) + j;
  if (order == 1) return p;
  const int per_img = tiles_x * tiles_y, img = p / per_img, pi = p - img * per_img;
  const int r0 = pi / (kB2Band * tiles_x) * kB2Band;
  const int h = tiles_y - r0 < kB2Band ? tiles_y - r0 : kB2Band;
  const int i = pi - r0 * tiles_x;
  return img * per_img + (r0 + i % h) * tiles_x + i / h;
}

template <int CIN, bool DS>
__global__ __launch_bounds__(256, 2) void bottleneck64_v2_nhwc_bf16_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ w1p, const float* __restrict__ b1,
    const uint4* __restrict__ w2p, const float* __restrict__ b2, const uint4* __restrict__ w3p,
    const float* __restrict__ b3, unsigned short* __restrict__ out, int H, int W, int tiles_x, int tiles_y, int order) {
  static_assert(CIN % 32 == 0 && (DS ? CIN == 64 : CIN == 256), "identity: 4 waves x 2 chunks; projection: both chunks in LDS");
  constexpr int NCH = CIN / 32, CQ = CIN / 8;
  constexpr int STAGE_BYTES = 2 * kB2XA + kB2H1 + kB2C2;              // 75 072
  __shared__ __attribute__((aligned(16))) char lds[STAGE_BYTES];
  static_assert(4 * kB2OS <= kB2H1, "the waves' epilogue scratch aliases the c1 halo");
  char* const sH1 = lds + 2 * kB2XA;
  char* const sC2 = sH1 + kB2H1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  const int tile = bn64_tile_of_block((int)blockIdx.x, (int)gridDim.x, tiles_x, tiles_y, order);
  int bid = tile;
  const int tx_i = bid % tiles_x; bid /= tiles_x;
  const int ty_i = bid % tiles_y;
  const int img = bid / tiles_y;
  const int y0 = ty_i * kB2TH, x0 = tx_i * kB2TW;

  // ================= phase A: c1 = relu(x . W1^T + b1) on the 180 halo pixels ==========================
  // x staging roles: 180 pixels x 4 pieces of 16 B per chunk = 720 items over 256 threads
  long hofs0, hofs1, hofs2;
  int hdst0, hdst1, hdst2;
  bool hin0, hin1, hin2, hlive0, hlive1, hlive2;
#define OCC_B2_ROLE(K, OFS, DST, IN, LIVE)                                                        \
  {                                                                                               \
    const int idx = tid + 256 * (K);                                                              \
    LIVE = idx < kB2NP * 4;                                                                       \
    const int p = LIVE ? idx >> 2 : 0, piece = idx & 3;                                           \
    const int hy = p / kB2HW, hx = p % kB2HW;                                                     \
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;                                                 \
    IN = LIVE && iy >= 0 && iy < H && ix >= 0 && ix < W;                                          \
    const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);                           \
    OFS = (((long)img * H + cy) * W + cx) * CQ + piece;                                           \
    DST = p * kB2XS + piece * 16;                                                                 \
  }
  OCC_B2_ROLE(0, hofs0, hdst0, hin0, hlive0)
  OCC_B2_ROLE(1, hofs1, hdst1, hin1, hlive1)
  OCC_B2_ROLE(2, hofs2, hdst2, hin2, hlive2)
#undef OCC_B2_ROLE
  const unsigned hm0 = hin0 ? 0xffffffffu : 0u, hm1 = hin1 ? 0xffffffffu : 0u, hm2 = hin2 ? 0xffffffffu : 0u;
  // four register sets: the x prefetch runs four chunks ahead
  uint4 vh0_0, vh1_0, vh2_0, vh0_1, vh1_1, vh2_1, vh0_2, vh1_2, vh2_2, vh0_3, vh1_3, vh2_3;
#define OCC_B2_ISSUE_X(S, CH)                                                                     \
  {                                                                                               \
    const long cq = (long)(CH) * 4;                                                               \
    vh0_##S = x[hofs0 + cq]; vh1_##S = x[hofs1 + cq]; vh2_##S = x[hofs2 + cq];                    \
  }
  // chunk order rotated per TILE: the summation order of conv1, and with it the bits of a tile, do not depend on which
  // block computes it; the downsample variant keeps chunk c in buffer c for phase C
  const int rot = DS ? 0 : (int)(((unsigned)tile * 5u) % (unsigned)NCH);
#define OCC_B2_CH(CI) (((CI) + rot) % NCH)

  const int ntA = wave & 1, mtA0 = 3 * (wave >> 1);
  const int ntB = wave & 1, mtB0 = 2 * (wave >> 1);
  // weights as the row operand in all three phases: D[channel][pixel], a lane holds ONE pixel (column = lane & 31) and
  // four groups of 4 consecutive channels (8g + 4*(lane>>5) + 0..3)
  // Biases of this lane's channels: requested in the last but one step of phase A, when the x prefetch has stopped and its
  // registers come free (the first kernel asks for them up front; here those 32 registers carry the identity)
  float4 bA[4], bB[4];
  f32x16 acc1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[j][r] = 0.f;
  // identity of this lane: pixel 32 rt + vi, channels 64 wave + 32 t + 8 q + 4 kb + 0..3 as idn[t][rt][q] (packed bf16).
  // Taken at the phase-A step whose chunk is 2 wave + t: the step is known only at run time (rot), so every step tests
  // the wave-uniform chunk index and copies into statically named registers.
  uint2 idn[2][4][4];
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int cbase = (((vi >> 4) + 1) * kB2HW + (vi & 15) + 1) * kB2XS + 8 * kb;
#define OCC_B2_CAPTURE(T, SX)                                                                     \
  _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                 \
      idn[T][rt][q] = *reinterpret_cast<const uint2*>((SX) + cbase + rt * (2 * kB2HW * kB2XS) + 16 * q);
  // W1 fragments: a ring of three chunks (the first kernel's fourth slot is 8 of the registers the identity needs).  The
  // fragments of chunk c + 3 are requested in FRONT of the x pieces of chunk c + 4, so the in-order vmcnt wait for the
  // fragments of a step still leaves the x pieces of the three chunks behind it in flight.
  constexpr int WD = 3;
  uint4 wa[WD][2];
#define OCC_B2_ISSUE_W1(SLOT, CH)                                                                 \
  {                                                                                               \
    wa[SLOT][0] = w1p[(((long)(CH) * 2 + 0) * 2 + ntA) * 64 + lane];                              \
    wa[SLOT][1] = w1p[(((long)(CH) * 2 + 1) * 2 + ntA) * 64 + lane];                              \
  }
  OCC_B2_ISSUE_W1(0, OCC_B2_CH(0))
  OCC_B2_ISSUE_X(0, OCC_B2_CH(0))
  OCC_B2_ISSUE_W1(1, OCC_B2_CH(NCH > 1 ? 1 : 0))
  OCC_B2_ISSUE_X(1, OCC_B2_CH(NCH > 1 ? 1 : 0))
  if (NCH > 2) {
    OCC_B2_ISSUE_W1(2, OCC_B2_CH(NCH > 2 ? 2 : 0))
    OCC_B2_ISSUE_X(2, OCC_B2_CH(NCH > 2 ? 2 : 0))
    OCC_B2_ISSUE_X(3, OCC_B2_CH(NCH > 3 ? 3 : 0))
  }
#define OCC_B2_STEP_A(S, CI)                                                                      \
  {                                                                                               \
    char* sX = lds + ((CI) & 1) * kB2XA;                                                          \
    if (hlive0) *reinterpret_cast<uint4*>(sX + hdst0) = make_uint4(vh0_##S.x & hm0, vh0_##S.y & hm0, vh0_##S.z & hm0, vh0_##S.w & hm0); \
    if (hlive1) *reinterpret_cast<uint4*>(sX + hdst1) = make_uint4(vh1_##S.x & hm1, vh1_##S.y & hm1, vh1_##S.z & hm1, vh1_##S.w & hm1); \
    if (hlive2) *reinterpret_cast<uint4*>(sX + hdst2) = make_uint4(vh2_##S.x & hm2, vh2_##S.y & hm2, vh2_##S.z & hm2, vh2_##S.w & hm2); \
    const bf16x8 wf0 = __builtin_bit_cast(bf16x8, wa[(CI) % WD][0]), wf1 = __builtin_bit_cast(bf16x8, wa[(CI) % WD][1]); \
    __syncthreads();                                                                              \
    if ((CI) + WD < NCH) OCC_B2_ISSUE_W1((CI) % WD, OCC_B2_CH((CI) + WD < NCH ? (CI) + WD : NCH - 1)) \
    if ((CI) + 4 < NCH) OCC_B2_ISSUE_X(S, OCC_B2_CH((CI) + 4 < NCH ? (CI) + 4 : NCH - 1))         \
    if ((CI) == NCH - 2) {                                                                        \
      _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                             \
        bA[g] = *reinterpret_cast<const float4*>(b1 + ntA * 32 + 8 * g + 4 * kb);                 \
        bB[g] = *reinterpret_cast<const float4*>(b2 + ntB * 32 + 8 * g + 4 * kb);                 \
      }                                                                                           \
    }                                                                                             \
    _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                               \
      const bf16x8 af0 = *reinterpret_cast<const bf16x8*>(sX + ((mtA0 + j) * 32 + vi) * kB2XS + kb * 16);      \
      const bf16x8 af1 = *reinterpret_cast<const bf16x8*>(sX + ((mtA0 + j) * 32 + vi) * kB2XS + 32 + kb * 16); \
      acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf0, af0, acc1[j], 0, 0, 0);              \
      acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf1, af1, acc1[j], 0, 0, 0);              \
    }                                                                                             \
    if (!DS) {                                                                                    \
      const int ch = OCC_B2_CH(CI);                                                               \
      if (ch == 2 * wave_u) { OCC_B2_CAPTURE(0, sX) }                                             \
      else if (ch == 2 * wave_u + 1) { OCC_B2_CAPTURE(1, sX) }                                    \
    }                                                                                             \
  }
#pragma unroll
  for (int ci = 0; ci < NCH; ci += 4) {
    OCC_B2_STEP_A(0, ci)
    if (ci + 1 < NCH) OCC_B2_STEP_A(1, ci + 1)
    if (ci + 2 < NCH) OCC_B2_STEP_A(2, ci + 2)
    if (ci + 3 < NCH) OCC_B2_STEP_A(3, ci + 3)
  }
#undef OCC_B2_STEP_A
#undef OCC_B2_ISSUE_W1
#undef OCC_B2_ISSUE_X
#undef OCC_B2_CAPTURE
#undef OCC_B2_CH

  // first W2 fragments in flight while c1 is written
  constexpr int PFB = 12;
  uint4 wr[PFB];
#pragma unroll
  for (int s = 0; s < PFB; ++s) wr[s] = w2p[((long)s * 2 + ntB) * 64 + lane];

  // c1 halo: bias + ReLU, zero outside the image (conv2's zero padding applies to c1, not to x); the halo
  // slot of pixel p = hy*18 + hx is simply p * 144 bytes
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int p = (mtA0 + j) * 32 + vi;
    const int hy = p / kB2HW, hx = p - hy * kB2HW;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const float m = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? 1.f : 0.f;
    if (p < kB2NP) {
      char* dst = sH1 + p * kB2MS + (ntA * 32 + 4 * kb) * 2;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float v0 = fmaxf(acc1[j][4 * g + 0] + bA[g].x, 0.f) * m, v1 = fmaxf(acc1[j][4 * g + 1] + bA[g].y, 0.f) * m;
        const float v2 = fmaxf(acc1[j][4 * g + 2] + bA[g].z, 0.f) * m, v3 = fmaxf(acc1[j][4 * g + 3] + bA[g].w, 0.f) * m;
        *reinterpret_cast<uint2*>(dst + 16 * g) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
      }
    }
  }
  __syncthreads();

  // ================= phase B: c2 = relu(conv3x3(c1) + b2), K = 9 taps x 64 ================================
  f32x16 acc2[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[j][r] = 0.f;
  const int ab0 = (2 * mtB0 + (vi >> 4)) * kB2H1ROW + (vi & 15) * kB2MS + kb * 16;
  const int ab1 = ab0 + 2 * kB2H1ROW;
  {
    bf16x8 a0 = *reinterpret_cast<const bf16x8*>(sH1 + ab0), a1 = *reinterpret_cast<const bf16x8*>(sH1 + ab1);
#pragma unroll
    for (int s = 0; s < 36; ++s) {
      const bf16x8 wf = __builtin_bit_cast(bf16x8, wr[s % PFB]);
      // the ring keeps PFB weight loads in flight; the scheduling barrier keeps hipcc from sinking them
      // behind the MFMAs
      if (s + PFB < 36) wr[s % PFB] = w2p[((long)(s + PFB) * 2 + ntB) * 64 + lane];
      bf16x8 a0n = a0, a1n = a1;
      if (s + 1 < 36) {   // next k-step's pixel fragments while this step's MFMAs run
        const int tap = (s + 1) >> 2, ks = (s + 1) & 3;
        const int toff = (tap / 3) * kB2H1ROW + (tap % 3) * kB2MS + ks * 32;
        a0n = *reinterpret_cast<const bf16x8*>(sH1 + ab0 + toff);
        a1n = *reinterpret_cast<const bf16x8*>(sH1 + ab1 + toff);
      }
      acc2[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, a0, acc2[0], 0, 0, 0);
      acc2[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, a1, acc2[1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      a0 = a0n; a1 = a1n;
    }
  }
  // every W3 fragment of the wave's two channel tiles and its bias in flight while c2 is written
  constexpr int KS3 = DS ? 8 : 4;
  uint4 w3f[KS3][2];
#pragma unroll
  for (int ks = 0; ks < KS3; ++ks)
#pragma unroll
    for (int t = 0; t < 2; ++t) w3f[ks][t] = w3p[((long)ks * 8 + 2 * wave + t) * 64 + lane];
  float4 bC[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) bC[t][q] = *reinterpret_cast<const float4*>(b3 + 64 * wave + 32 * t + 8 * q + 4 * kb);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    char* dst = sC2 + ((mtB0 + j) * 32 + vi) * kB2MS + (ntB * 32 + 4 * kb) * 2;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float v0 = fmaxf(acc2[j][4 * g + 0] + bB[g].x, 0.f), v1 = fmaxf(acc2[j][4 * g + 1] + bB[g].y, 0.f);
      const float v2 = fmaxf(acc2[j][4 * g + 2] + bB[g].z, 0.f), v3 = fmaxf(acc2[j][4 * g + 3] + bB[g].w, 0.f);
      *reinterpret_cast<uint2*>(dst + 16 * g) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
    }
  }
  __syncthreads();     // c2 complete; nothing reads the c1 halo any more: its bytes are the waves' scratch from here on

  // ================= phase C: out = relu(c2 . W3^T (+ x . Wds^T) + b3 (+ x)) ==============================
  // One 32-pixel tile (two image rows) at a time: the wave's 64 channels of it, D[channel][pixel]; no block barrier.
  char* const scr = sH1 + wave * kB2OS;
  const int orow = lane >> 3, opiece = lane & 7;       // the row leaves as 8 pieces of 16 B: pixel 8 j + orow of the tile
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    f32x16 acc3[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[t][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS3; ++ks) {
      bf16x8 af;
      if (ks < 4) {
        af = *reinterpret_cast<const bf16x8*>(sC2 + (rt * 32 + vi) * kB2MS + ks * 32 + kb * 16);
      } else {   // downsample: the centre pixels of the x halo, chunk (ks-4)/2 still sits in its buffer
        const int p = (2 * rt + (vi >> 4) + 1) * kB2HW + (vi & 15) + 1;
        af = *reinterpret_cast<const bf16x8*>(lds + ((ks - 4) >> 1) * kB2XA + p * kB2XS + ((ks - 4) & 1) * 32 + kb * 16);
      }
      acc3[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w3f[ks][0]), af, acc3[0], 0, 0, 0);
      acc3[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w3f[ks][1]), af, acc3[1], 0, 0, 0);
    }
    // bias, identity, ReLU, ONE rounding; the bf16 quads go to the wave's scratch, pixel rows of 128 B
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint2 id = DS ? make_uint2(0u, 0u) : idn[t][rt][q];
        float v0 = acc3[t][4 * q + 0], v1 = acc3[t][4 * q + 1], v2 = acc3[t][4 * q + 2], v3 = acc3[t][4 * q + 3];
        v0 += bC[t][q].x + bf16_lo_to_f32(id.x);
        v1 += bC[t][q].y + bf16_hi_to_f32(id.x);
        v2 += bC[t][q].z + bf16_lo_to_f32(id.y);
        v3 += bC[t][q].w + bf16_hi_to_f32(id.y);
        v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
        *reinterpret_cast<uint2*>(scr + vi * kB2MS + t * 64 + q * 16 + kb * 8) =
            make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
      }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 8 * j + orow;
      const int oy = y0 + 2 * rt + (row >> 4), ox = x0 + (row & 15);
      const uint4 v = *reinterpret_cast<const uint4*>(scr + row * kB2MS + opiece * 16);
      if (oy < H && ox < W)
        *reinterpret_cast<uint4*>(out + (((long)img * H + oy) * W + ox) * 256 + 64 * wave + opiece * 8) = v;
    }
    wave_lds_sync();
  }
}

// The second kernel on `st` (arguments already checked by the caller in bottleneck64_nhwc_bf16.hip).
void bottleneck64_v2_launch(const void* x, const void* w1_frag, const float* b1, const void* w2_frag, const float* b2,
                            const void* w3_frag, const float* b3, void* out, int batch, int H, int W, int downsample,
                            int order, hipStream_t st) {
  const int tiles_x = (W + kB2TW - 1) / kB2TW, tiles_y = (H + kB2TH - 1) / kB2TH;
  const unsigned gx = (unsigned)((long)batch * tiles_x * tiles_y);
#define OCC_B2_LAUNCH(CINN, DSS)                                                                     \
  hipLaunchKernelGGL((bottleneck64_v2_nhwc_bf16_kernel<CINN, DSS>), dim3(gx), dim3(256), 0, st,         \
                     reinterpret_cast<const uint4*>(x), reinterpret_cast<const uint4*>(w1_frag), b1,    \
                     reinterpret_cast<const uint4*>(w2_frag), b2, reinterpret_cast<const uint4*>(w3_frag), \
                     b3, reinterpret_cast<unsigned short*>(out), H, W, tiles_x, tiles_y, order)
  if (downsample) OCC_B2_LAUNCH(64, true); else OCC_B2_LAUNCH(256, false);
#undef OCC_B2_LAUNCH
}

}  // namespace occ

extern "C" int occ_bottleneck64_tile_of_block(int block, int n_blocks, int tiles_x, int tiles_y, int order) {
  using namespace occ;
  OCC_CHECK_ARG(tiles_x > 0 && tiles_y > 0 && n_blocks > 0 && n_blocks % (tiles_x * tiles_y) == 0,
                "bottleneck64_tile_of_block: n_blocks must be a positive multiple of tiles_x * tiles_y");
  OCC_CHECK_ARG(block >= 0 && block < n_blocks, "bottleneck64_tile_of_block: block outside 0 .. n_blocks - 1");
  OCC_CHECK_ARG(order >= 0 && order <= 2, "bottleneck64_tile_of_block: order must be 0, 1 or 2");
  return bn64_tile_of_block(block, n_blocks, tiles_x, tiles_y, order);
}
