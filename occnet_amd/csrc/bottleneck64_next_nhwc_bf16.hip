// Third kernel of the whole 64-mid-channel bottleneck: the LAST identity block of a stage whose output has exactly two
// readers, both pointwise, both in the next stage's first block - its conv1 (256 -> CM, stride 1, ReLU) and its shortcut
// (256 -> 4 CM at stride 2).  The second kernel (bottleneck64_v2_nhwc_bf16.hip) writes the 256-channel map to HBM and two
// resident 1x1 launches read it back; here the 8 x 16 pixel tile never leaves the CU:
//   y    = relu(out . W1n^T + b1n)        (N, H, W, CM)                         every pixel
//   idn2 = out_even . Wds^T + bds         (N, (H-1)/2+1, (W-1)/2+1, 4 CM)       the pixels with even (y, x)
// and `out` itself is not stored.
//
// Phases A and B are bottleneck64_phases.h, placed as the second kernel places them (tile order 0).  Phase C is the second
// kernel's - wave w owns channels 64 w .. 64 w + 63, identity from idn[], one rounding - except that the bf16 quads go into
// an A tile in LDS in the resident 1x1 kernel's layout (rows of 512 B, 16-byte piece s of row r at slot s ^ (r & 31)) and
// not to global memory.  Phase D expands the resident kernel's pass loop (conv1x1_resident_pass.h) on that tile, so the K
// order and the rounding place of both 1x1s are conv1x1_resident_kernel's by construction: for every element the launch
// returns the bits of bottleneck64 (second kernel), then occ_conv1x1_nhwc_bf16_variant 2 twice.
//
// LDS.  The 128 x 256 tile (64 KB) does not fit beside c2, which is live until the last wave has left phase C.  The tile
// is therefore produced and consumed in two halves of 64 pixels (row tiles 0-1, then 2-3), and each half's 16 pixels
// with even (y, x) are also written to a 32-row tile of their own, on which the shortcut runs once, after the second half
// (no zero or duplicate rows: 64 MFMAs per wave and tile).  Everything phase D needs overlays the x chunk buffers and the
// c1 halo, which are dead from the barrier behind phase B on; c2 moves up behind the even tile:
//       0  half tile        64 rows x 512 B                     (phase A: x chunk buffers; phase B: c1 halo from 30 720)
//  32 768  scratch          4 waves x kC1rScratch
//  43 008  bias             b1n (CM) then bds (4 CM), f32
//  45 568  even tile        32 rows x 512 B: row 8 rt + x / 2
//  61 952  c2               128 pixel slots of 144 B             -> 80 384 B, two blocks per CU
// Block barriers behind phase B: half 0 written | half 0 read (its rows are overwritten) | half 1 written: three.
#include "bottleneck64_phases.h"
#include "conv1x1_resident_pass.h"

namespace occ {

// conv1x1_resident_bf16.hip: the resident 1x1 kernel's own shape rule (0 = no resident tile)
int conv1x1_resident_tile(int Cin, int Cout, long M, long in_pixels, int rt);

namespace {

constexpr int kBxHalf = 64 * 512;                                // half tile: 64 pixels x 256 channels bf16
constexpr int kBxScr = kBxHalf;                                  // the four waves' phase-D scratch
constexpr int bx_bias_ofs() { return kBxScr + 4 * kC1rScratch; }
constexpr int bx_even_ofs(int CM) { return bx_bias_ofs() + 5 * CM * 4; }
constexpr int bx_c2_ofs(int CM) { return bx_even_ofs(CM) + 32 * 512; }
constexpr int bx_lds_bytes(int CM) { return bx_c2_ofs(CM) + kBnC2; }

// What the pass loop takes from this kernel.  Neither 1x1 has a residual; the rows of the two tiles are spelled out in
// front of each expansion.
#define OCC_C1R_P_BEGIN 0
#define OCC_C1R_P_END NP
#define OCC_C1R_RESIDUAL 0
#define OCC_C1R_RELU D_RELU
#define OCC_C1R_RES_ROW(RTI, J) const long rpx = 0;
#define OCC_C1R_RES_PIXEL rpx

template <int CM>
__global__ __launch_bounds__(256, 2) void bottleneck64_next_nhwc_bf16_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ w1p, const float* __restrict__ b1,
    const uint4* __restrict__ w2p, const float* __restrict__ b2, const uint4* __restrict__ w3p,
    const float* __restrict__ b3, const uint4* __restrict__ wn1, const float* __restrict__ bn1,
    const uint4* __restrict__ wds, const float* __restrict__ bds, unsigned short* __restrict__ yout,
    unsigned short* __restrict__ sout, int H, int W, int Ho, int Wo, int tiles_x, int tiles_y) {
  constexpr int CIN = 256, NCH = CIN / 32, CQ = CIN / 8;
  constexpr bool DS = false;
  static_assert(CM % 64 == 0, "conv1: passes of 128 columns or one of CM; shortcut: passes of 256 columns");
  static_assert(bx_lds_bytes(CM) <= 81920, "two blocks per CU");
  static_assert(2 * kBnXA + kBnH1 <= bx_c2_ofs(CM), "c2 lies behind everything phase D overlays");
  __shared__ __attribute__((aligned(16))) char smem[bx_lds_bytes(CM)];
  char* const lds = smem;
  char* const sH1 = lds + 2 * kBnXA;
  char* const sC2 = lds + bx_c2_ofs(CM);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  const int tile = (int)blockIdx.x;
  OCC_BN_TILE_DECODE(tile)

  // ================= phase A: c1 = relu(x . W1^T + b1) on the 180 halo pixels (the second kernel's placement) =========
  OCC_BN_STAGING
  const int rot = (int)(((unsigned)tile * 5u) % (unsigned)NCH);

  OCC_BN_WAVE_TILES
  float4 bA[4], bB[4];
  OCC_BN_ZERO_ACC(acc1, 3)
  // identity of this lane: pixel 32 rt + vi, channels 64 wave + 32 t + 8 q + 4 kb + 0..3 as idn[t][rt][q] (packed bf16)
  uint2 idn[2][4][4];
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int cbase = (((vi >> 4) + 1) * kBnHW + (vi & 15) + 1) * kBnXS + 8 * kb;
#define OCC_BX_CAPTURE(T, SX)                                                                     \
  _Pragma("unroll") for (int rt = 0; rt < 4; ++rt)                                                \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                 \
      idn[T][rt][q] = *reinterpret_cast<const uint2*>((SX) + cbase + rt * (2 * kBnHW * kBnXS) + 16 * q);
  constexpr int WD = 3;
  uint4 wa[WD][2];
  OCC_BN_ISSUE_W1(0, OCC_BN_CH(0))
  OCC_BN_ISSUE_X(0, OCC_BN_CH(0))
  OCC_BN_ISSUE_W1(1, OCC_BN_CH(1))
  OCC_BN_ISSUE_X(1, OCC_BN_CH(1))
  OCC_BN_ISSUE_W1(2, OCC_BN_CH(2))
  OCC_BN_ISSUE_X(2, OCC_BN_CH(2))
  OCC_BN_ISSUE_X(3, OCC_BN_CH(3))
#define OCC_BX_STEP_A(S, CI)                                                                      \
  {                                                                                               \
    char* sX = lds + ((CI) & 1) * kBnXA;                                                          \
    OCC_BN_STAGE_STORE(S, sX)                                                                     \
    OCC_BN_W1_FRAGS((CI) % WD)                                                                    \
    __syncthreads();                                                                              \
    if ((CI) + WD < NCH) OCC_BN_ISSUE_W1((CI) % WD, OCC_BN_CH((CI) + WD < NCH ? (CI) + WD : NCH - 1)) \
    if ((CI) + 4 < NCH) OCC_BN_ISSUE_X(S, OCC_BN_CH((CI) + 4 < NCH ? (CI) + 4 : NCH - 1))         \
    if ((CI) == NCH - 2) { OCC_BN_ISSUE_BIASES }                                                  \
    OCC_BN_STEP_MFMA(sX)                                                                          \
    const int ch = OCC_BN_CH(CI);                                                                 \
    if (ch == 2 * wave_u) { OCC_BX_CAPTURE(0, sX) }                                               \
    else if (ch == 2 * wave_u + 1) { OCC_BX_CAPTURE(1, sX) }                                      \
  }
#pragma unroll
  for (int ci = 0; ci < NCH; ci += 4) {
    OCC_BX_STEP_A(0, ci)
    OCC_BX_STEP_A(1, ci + 1)
    OCC_BX_STEP_A(2, ci + 2)
    OCC_BX_STEP_A(3, ci + 3)
  }
#undef OCC_BX_STEP_A
#undef OCC_BX_CAPTURE

  OCC_BN_W2_PROLOGUE
  OCC_BN_WRITE_C1
  __syncthreads();

  OCC_BN_PHASE_B
  uint4 w3f[4][2];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int t = 0; t < 2; ++t) w3f[ks][t] = w3p[((long)ks * 8 + 2 * wave + t) * 64 + lane];
  float4 bC[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) bC[t][q] = *reinterpret_cast<const float4*>(b3 + 64 * wave + 32 * t + 8 * q + 4 * kb);
  OCC_BN_WRITE_C2
  __syncthreads();     // c2 complete; the x chunk buffers and the c1 halo are dead: tile, scratch, bias, even tile from here on

  // the biases of both 1x1s go through LDS (conv1x1_resident_bf16.hip says why); the barrier in front of the first
  // phase D covers them
  float* const sb = reinterpret_cast<float*>(lds + bx_bias_ofs());
  if (tid < 5 * CM / 4)
    *reinterpret_cast<float4*>(sb + 4 * tid) = tid < CM / 4 ? *reinterpret_cast<const float4*>(bn1 + 4 * tid)
                                                            : *reinterpret_cast<const float4*>(bds + 4 * tid - CM);
  char* const sEven = lds + bx_even_ofs(CM);
  char* const scratch = lds + kBxScr + wave * kC1rScratch;
  const unsigned short* const residual = nullptr;
  const long img_row0 = (long)img * H, img_row0s = (long)img * Ho;

#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 1) __syncthreads();     // every wave has read half 0 for the last time
    // ================= phase C: out = relu(c2 . W3^T + b3 + x), row tiles 2 h and 2 h + 1, into the half tile ==========
#pragma unroll
    for (int rh = 0; rh < 2; ++rh) {
      const int rt = 2 * h + rh;
      f32x16 acc3[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc3[t][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 afc;
        OCC_BN_C_AFRAG(afc, rt, ks)
        acc3[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w3f[ks][0]), afc, acc3[0], 0, 0, 0);
        acc3[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w3f[ks][1]), afc, acc3[1], 0, 0, 0);
      }
      // bias, identity, ReLU, ONE rounding; the lane's pixel is row 32 rh + vi of the half tile, and row 8 rt + x / 2 of
      // the even tile when it lies on an even image row (vi < 16: y0 is even) and an even column
      char* const trow = lds + (rh * 32 + vi) * 512 + 8 * kb;
      const bool even = (vi & 17) == 0;
      const int er = 8 * rt + (vi >> 1);
      char* const erow_p = sEven + er * 512 + 8 * kb;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint2 id = idn[t][rt][q];
          float v0 = acc3[t][4 * q + 0], v1 = acc3[t][4 * q + 1], v2 = acc3[t][4 * q + 2], v3 = acc3[t][4 * q + 3];
          v0 += bC[t][q].x + bf16_lo_to_f32(id.x);
          v1 += bC[t][q].y + bf16_hi_to_f32(id.x);
          v2 += bC[t][q].z + bf16_lo_to_f32(id.y);
          v3 += bC[t][q].w + bf16_hi_to_f32(id.y);
          v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
          const uint2 o = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
          const int piece = 8 * wave + 4 * t + q;                 // channels 8 piece .. 8 piece + 7
          *reinterpret_cast<uint2*>(trow + ((piece ^ vi) << 4)) = o;
          if (even) *reinterpret_cast<uint2*>(erow_p + ((piece ^ (er & 31)) << 4)) = o;
        }
    }

    // ================= phase D, conv1 of the next block on the half: y = relu(half . W1n^T + b1n) ======================
    {
      constexpr int K = 256, RT = 2, NTW = 1, RD = 1, N = CM;
      constexpr int PITCH = 2 * K, KS = K / 16, MASK = 31, NTILES = RT * NTW, NP = N / (128 * NTW), D_RELU = 1;
      float* const sbias = sb;
      unsigned short* const out = yout;
      OCC_C1R_RING(wn1)
      OCC_C1R_LOAD(0, 0, 0)
      OCC_C1R_LOAD(1, 0, 1)
      OCC_C1R_LOAD(2, 0, 2)
      OCC_C1R_RES_START
      __syncthreads();               // the half tile (h == 0: and the bias) is in LDS
      OCC_C1R_AFRAG_STATE
      // tile row 32 rt + 16 j + r = image row y0 + 4 h + 2 rt + j, column x0 + r
#define OCC_C1R_PASS_LOCALS const int ex = x0 + erow;
#define OCC_C1R_OUT_ROW(RTI, J)                                                                   \
      const int oy = y0 + 4 * h + 2 * (RTI) + (J);                                                \
      const bool olive = oy < H && ex < W;                                                        \
      const long orow = (img_row0 + oy) * W + ex;
      OCC_C1R_PASSES
#undef OCC_C1R_PASS_LOCALS
#undef OCC_C1R_OUT_ROW
    }
  }

  // ================= phase D, the next block's shortcut on the even tile: idn2 = even . Wds^T + bds =====================
  // (complete since the barrier in front of the second conv1; this wave's scratch is its own)
  {
    constexpr int K = 256, RT = 1, NTW = 2, RD = 1, N = 4 * CM;
    constexpr int PITCH = 2 * K, KS = K / 16, MASK = 31, NTILES = RT * NTW, NP = N / (128 * NTW), D_RELU = 0;
    char* const lds = sEven;
    float* const sbias = sb + CM;
    unsigned short* const out = sout;
    OCC_C1R_RING(wds)
    OCC_C1R_LOAD(0, 0, 0)
    OCC_C1R_LOAD(1, 0, 1)
    OCC_C1R_LOAD(2, 0, 2)
    OCC_C1R_RES_START
    OCC_C1R_AFRAG_STATE
    // tile row 16 j + r = shortcut pixel row y0 / 2 + 2 j + r / 8, column x0 / 2 + r % 8
#define OCC_C1R_PASS_LOCALS const int ex = (x0 >> 1) + (erow & 7), ey = (y0 >> 1) + (erow >> 3);
#define OCC_C1R_OUT_ROW(RTI, J)                                                                   \
    const int oy = ey + 2 * (J);                                                                  \
    const bool olive = oy < Ho && ex < Wo;                                                        \
    const long orow = (img_row0s + oy) * Wo + ex;
    OCC_C1R_PASSES
#undef OCC_C1R_PASS_LOCALS
#undef OCC_C1R_OUT_ROW
  }
}

bool bx_has(int cmid_next) { return cmid_next == 128; }

}  // namespace
}  // namespace occ

// Non-zero where the plan should take occ_bottleneck64_next_nhwc_bf16 for a (batch, 256, H, W) map in front of a block with
// cmid_next mid channels: a kernel exists, and BOTH 1x1 launches it replaces (256 -> cmid_next at full resolution,
// 256 -> 4 cmid_next at stride 2) would take the resident kernel by occ_conv1x1_nhwc_bf16's default rule, so that the
// fused launch returns the bits of the route it replaces.  A pure function of the shape; needs no GPU.
extern "C" int occ_bottleneck64_next_pick(int batch, int H, int W, int cmid_next) {
  using namespace occ;
  if (batch <= 0 || H <= 0 || W <= 0 || !bx_has(cmid_next)) return 0;
  static const bool resident_on = env_default_on("OCC_CONV1X1_RESIDENT");
  if (!resident_on) return 0;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long M = (long)batch * H * W, Ms = (long)batch * Ho * Wo;
  if (M < 512 || Ms < 512) return 0;
  if (!conv1x1_resident_tile(256, cmid_next, M, M, 0) || !conv1x1_resident_tile(256, 4 * cmid_next, Ms, M, 0)) return 0;
  return 1;
}

extern "C" int occ_bottleneck64_next_nhwc_bf16(const void* x, const void* w1_frag, const float* b1, const void* w2_frag,
                                               const float* b2, const void* w3_frag, const float* b3,
                                               const void* next_w1_frag, const float* next_b1, const void* next_wds_frag,
                                               const float* next_bds, void* y, void* shortcut, int batch, int H, int W,
                                               int cmid_next, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(x && w1_frag && b1 && w2_frag && b2 && w3_frag && b3 && next_w1_frag && next_b1 && next_wds_frag &&
                    next_bds && y && shortcut,
                "bottleneck64_next_nhwc_bf16: null pointer argument");
  OCC_CHECK_ARG(batch > 0 && H > 0 && W > 0, "bottleneck64_next_nhwc_bf16: bad dimension");
  OCC_CHECK_ARG(y != shortcut && x != y && x != shortcut, "bottleneck64_next_nhwc_bf16: x, y and shortcut must be distinct");
  if (!bx_has(cmid_next)) {
    set_error("bottleneck64_next_nhwc_bf16: no kernel for cmid_next=%d (128: the block after ResNet-50's layer1)", cmid_next);
    return OCC_E_UNSUPPORTED;
  }
  const int tiles_x = (W + kBnTW - 1) / kBnTW, tiles_y = (H + kBnTH - 1) / kBnTH;
  const long blocks = (long)batch * tiles_x * tiles_y;
  if (blocks >= (1L << 31) || (long)batch * H * W >= (1L << 30)) {
    set_error("bottleneck64_next_nhwc_bf16: tensor too large");
    return OCC_E_UNSUPPORTED;
  }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(bottleneck64_next_nhwc_bf16_kernel<128>, dim3((unsigned)blocks), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint4*>(x),
                     reinterpret_cast<const uint4*>(w1_frag), b1, reinterpret_cast<const uint4*>(w2_frag), b2,
                     reinterpret_cast<const uint4*>(w3_frag), b3, reinterpret_cast<const uint4*>(next_w1_frag), next_b1,
                     reinterpret_cast<const uint4*>(next_wds_frag), next_bds, reinterpret_cast<unsigned short*>(y),
                     reinterpret_cast<unsigned short*>(shortcut), H, W, Ho, Wo, tiles_x, tiles_y);
  OCC_CHECK_LAUNCH("bottleneck64_next_nhwc_bf16");
  return OCC_OK;
}
