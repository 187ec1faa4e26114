// Second kernel of the whole 64-mid-channel bottleneck (bottleneck64_nhwc_bf16.hip has the first one and says what the block
// computes; bottleneck64_phases.h has the structure, the LDS layout and phases A and B, which both kernels expand from the
// same text).  It computes the same bits and differs in what it moves:
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
//
// Its own in phase A, for the 64 registers of identity: the biases are requested in the last but one step, the W1 ring has
// three slots and is requested in front of x, and each step may capture the wave's identity chunk.
#include "bottleneck64_phases.h"

namespace occ {

constexpr int kBnOS = 32 * kBnMS;            // one wave's epilogue scratch: 32 pixels x 64 channels bf16, padded rows
constexpr int kBnBand = 4;                   // tile rows per band of the banded walk

// Tile (row-major linear index over image, tile row, tile column) of a block.
//   order 0: tile = block (the first kernel's map: neighbours lie on eight different L2s)
//   order 1: XCD-contiguous.  Group x = block % 8 takes positions x*q + min(x, r) + j, j = block / 8, of the row-major
//            walk (q = n / 8, r = n % 8: bijective for any n).  Horizontal neighbours follow each other, vertical ones
//            are tiles_x positions apart.
//   order 2: the same ranges over a walk in bands of kBnBand tile rows per image, column by column inside a band:
//            a vertical neighbour follows directly, a horizontal one kBnBand positions later; only the rows between
//            two bands (and between two groups' ranges) see their halo twice.
__host__ __device__ inline int bn64_tile_of_block(int block, int n_blocks, int tiles_x, int tiles_y, int order) {
  if (order == 0) return block;
  const int q = n_blocks >> 3, r = n_blocks & 7, x = block & 7, j = block >> 3;
  const int p = x * q + (x < r ? x : r) + j;
  if (order == 1) return p;
  const int per_img = tiles_x * tiles_y, img = p / per_img, pi = p - img * per_img;
  const int r0 = pi / (kBnBand * tiles_x) * kBnBand;
  const int h = tiles_y - r0 < kBnBand ? tiles_y - r0 : kBnBand;
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
  __shared__ __attribute__((aligned(16))) char lds[kBnStageBytes];
  static_assert(4 * kBnOS <= kBnH1, "the waves' epilogue scratch aliases the c1 halo");
  char* const sH1 = lds + 2 * kBnXA;
  char* const sC2 = sH1 + kBnH1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  const int tile = bn64_tile_of_block((int)blockIdx.x, (int)gridDim.x, tiles_x, tiles_y, order);
  OCC_BN_TILE_DECODE(tile)

  // ================= phase A: c1 = relu(x . W1^T + b1) on the 180 halo pixels ==========================
  OCC_BN_STAGING
  // chunk order rotated per TILE: the summation order of conv1, and with it the bits of a tile, do not depend on which
  // block computes it; the downsample variant keeps chunk c in buffer c for phase C
  const int rot = DS ? 0 : (int)(((unsigned)tile * 5u) % (unsigned)NCH);

  OCC_BN_WAVE_TILES
  // Biases of this lane's channels: requested in the last but one step of phase A, when the x prefetch has stopped and its
  // registers come free (the first kernel asks for them up front; here those 32 registers carry the identity)
  float4 bA[4], bB[4];
  OCC_BN_ZERO_ACC(acc1, 3)
  // identity of this lane: pixel 32 rt + vi, channels 64 wave + 32 t + 8 q + 4 kb + 0..3 as idn[t][rt][q] (packed bf16).
  // Taken at the phase-A step whose chunk is 2 wave + t: the step is known only at run time (rot), so every step tests
  // the wave-uniform chunk index and copies into statically named registers.
  uint2 idn[2][4][4];
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int cbase = (((vi >> 4) + 1) * kBnHW + (vi & 15) + 1) * kBnXS + 8 * kb;
#define OCC_B2_CAPTURE(T, SX)                                                                     \
  _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                 \
      idn[T][rt][q] = *reinterpret_cast<const uint2*>((SX) + cbase + rt * (2 * kBnHW * kBnXS) + 16 * q);
  // W1 fragments: a ring of three chunks (the first kernel's fourth slot is 8 of the registers the identity needs).  The
  // fragments of chunk c + 3 are requested in FRONT of the x pieces of chunk c + 4, so the in-order vmcnt wait for the
  // fragments of a step still leaves the x pieces of the three chunks behind it in flight.
  constexpr int WD = 3;
  uint4 wa[WD][2];
  OCC_BN_ISSUE_W1(0, OCC_BN_CH(0))
  OCC_BN_ISSUE_X(0, OCC_BN_CH(0))
  OCC_BN_ISSUE_W1(1, OCC_BN_CH(NCH > 1 ? 1 : 0))
  OCC_BN_ISSUE_X(1, OCC_BN_CH(NCH > 1 ? 1 : 0))
  if (NCH > 2) {
    OCC_BN_ISSUE_W1(2, OCC_BN_CH(NCH > 2 ? 2 : 0))
    OCC_BN_ISSUE_X(2, OCC_BN_CH(NCH > 2 ? 2 : 0))
    OCC_BN_ISSUE_X(3, OCC_BN_CH(NCH > 3 ? 3 : 0))
  }
#define OCC_B2_STEP_A(S, CI)                                                                      \
  {                                                                                               \
    char* sX = lds + ((CI) & 1) * kBnXA;                                                          \
    OCC_BN_STAGE_STORE(S, sX)                                                                     \
    OCC_BN_W1_FRAGS((CI) % WD)                                                                    \
    __syncthreads();                                                                              \
    if ((CI) + WD < NCH) OCC_BN_ISSUE_W1((CI) % WD, OCC_BN_CH((CI) + WD < NCH ? (CI) + WD : NCH - 1)) \
    if ((CI) + 4 < NCH) OCC_BN_ISSUE_X(S, OCC_BN_CH((CI) + 4 < NCH ? (CI) + 4 : NCH - 1))         \
    if ((CI) == NCH - 2) { OCC_BN_ISSUE_BIASES }                                                  \
    OCC_BN_STEP_MFMA(sX)                                                                          \
    if (!DS) {                                                                                    \
      const int ch = OCC_BN_CH(CI);                                                               \
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
#undef OCC_B2_CAPTURE

  OCC_BN_W2_PROLOGUE
  OCC_BN_WRITE_C1
  __syncthreads();

  OCC_BN_PHASE_B
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
  OCC_BN_WRITE_C2
  __syncthreads();     // c2 complete; nothing reads the c1 halo any more: its bytes are the waves' scratch from here on

  // ================= phase C: out = relu(c2 . W3^T (+ x . Wds^T) + b3 (+ x)) ==============================
  // One 32-pixel tile (two image rows) at a time: the wave's 64 channels of it, D[channel][pixel]; no block barrier.
  char* const scr = sH1 + wave * kBnOS;
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
      OCC_BN_C_AFRAG(af, rt, ks)
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
        *reinterpret_cast<uint2*>(scr + vi * kBnMS + t * 64 + q * 16 + kb * 8) =
            make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
      }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 8 * j + orow;
      const int oy = y0 + 2 * rt + (row >> 4), ox = x0 + (row & 15);
      const uint4 v = *reinterpret_cast<const uint4*>(scr + row * kBnMS + opiece * 16);
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
  bn64_launch(bottleneck64_v2_nhwc_bf16_kernel<64, true>, bottleneck64_v2_nhwc_bf16_kernel<256, false>, x, w1_frag, b1,
              w2_frag, b2, w3_frag, b3, out, batch, H, W, downsample, st, order);
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
