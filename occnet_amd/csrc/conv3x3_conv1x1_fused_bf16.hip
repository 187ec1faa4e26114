// ResNet bottleneck tail in ONE launch (NHWC bf16): the 3x3 convolution (conv2) and the 1x1 expansion after it (conv3),
//   out = relu( conv1x1( bf16( relu(conv3x3(x, W2, stride s) + b2) ), W3 ) + b3 + residual ),
// for Cmid in {128, 256}, Cout = 4 Cmid, stride 1 or 2, residual of the output's size.  The pair of launches it replaces
// (conv3x3_nhwc_bf16.hip, then conv1x1_resident_bf16.hip) runs a matrix-pipe-bound kernel that leaves HBM idle and then an
// HBM-bound kernel that leaves the matrix cores idle, and writes the mid tensor to HBM only to read it back.  Here the mid
// tile never leaves the CU, and with two or three blocks per CU the residual loads and row stores of one block travel under
// the 3x3 MFMAs of another.
//
// A block = 4 waves = one 3x3 tile that holds ALL mid channels: variant id 10 NT + RT with 128 NT = Cmid, (2 RT) x 16 output
// pixels.  Two phases, each the text its parent kernel is made of (conv3x3_kloop.h, conv1x1_resident_pass.h), which is what
// makes the result for a given tile id the bits of conv3x3 (that tile) followed by the resident conv1x1:
//   1. the K loop of conv3x3_nhwc_bf16_kernel with one column block: the rotation is the one that kernel derives from
//      blockIdx.x with blockIdx.y = 0, and the wave's column tiles need no clamp.  The epilogue is this kernel's own: it adds
//      the bias in f32, applies the ReLU, rounds ONCE and writes the bf16 tile into LDS - over the halo buffers, which are
//      dead by then - in the row-swizzled 16-byte-piece layout of conv1x1_resident_kernel (rows = the pixels of the patch in
//      MFMA row-tile order, 32 rt + 16 (y & 1) + x).  Pixels outside the map are written as zeros and never stored.
//   2. the pass loop of conv1x1_resident_kernel on that tile, residual and ReLU always on; the block walks all Cout / 256
//      column passes itself.  Output and residual addresses come from (oy, ox) of the row: clamped for the residual's loads,
//      with a bounds mask for the stores.
#include "conv1x1_resident_pass.h"
#include "conv3x3_kloop.h"

namespace occ {
namespace {

// LDS of a block: the two halo buffers of phase 1, overlaid in phase 2 by mid tile + the four waves' scratch + the bias
template <int NT, int S, int RT> constexpr int f31_lds_bytes() {
  constexpr int halo = 2 * C3Geom<S, RT>::HH * C3Geom<S, RT>::ROW, p2 = c1r_lds_bytes(128 * NT, RT, 512 * NT);
  return halo > p2 ? halo : p2;
}

// What the two loops take from this kernel (see the headers)
#define OCC_C3_NT32 (Cmid / 32)
#define OCC_C3_WTILE(T) (nw0 / 32 + (T))
#define OCC_C3_ROT (blockIdx.x * 5u)
#define OCC_C1R_P_BEGIN 0
#define OCC_C1R_P_END NP
#define OCC_C1R_RESIDUAL 1
#define OCC_C1R_RELU 1
// tile row 32 rt + 16 j + r = image row y0 + 2 rt + j, column x0 + r
#define OCC_C1R_RES_ROW(RTI, J)                                                                   \
  const int rx = min(x0 + (rlane >> 2), Wo - 1), ry = min(y0 + 2 * (RTI) + (J), Ho - 1);
#define OCC_C1R_RES_PIXEL (img_row0 + ry) * Wo + rx
#define OCC_C1R_PASS_LOCALS const int ex = x0 + erow;
#define OCC_C1R_OUT_ROW(RTI, J)                                                                   \
  const int oy = y0 + 2 * (RTI) + (J);                                                            \
  const bool olive = oy < Ho && ex < Wo;                                                          \
  const long orow = (img_row0 + oy) * Wo + ex;

template <int NT, int S, int RT_, int MINW, int RD>
__global__ __launch_bounds__(256, MINW) void conv3x3_conv1x1_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ wp, const float* __restrict__ bias2,
    const uint4* __restrict__ wp3, const float* __restrict__ bias3, const unsigned short* __restrict__ residual,
    unsigned short* __restrict__ out, int H, int W, int Ho, int Wo, int tiles_x, int tiles_y) {
  using G = C3Geom<S, RT_>;
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
  const int y0 = ty_i * kC3TH, x0 = tx_i * kC3TW;
  const int nw0 = wave * WR;
  constexpr int CQ = Cin / 8, NCH = Cin / 32;

  f32x16 acc[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][t][r] = 0.f;

  // ---- phase 1: the 3x3 K loop -------------------------------------------------------------------------------------------
  { OCC_C3_KLOOP }

  // ---- phase 2 set-up that can travel under the hand-over: weight ring and residual requests ----------------------------
  constexpr int K = Cmid, NTW = 2;
  constexpr int PCS = K / 8, PITCH = K * 2, KS = K / 16, NP = N / (128 * NTW);
  constexpr int MASK = (PCS < 32 ? PCS : 32) - 1;
  constexpr int TILE_BYTES = 32 * RT * PITCH;
  constexpr int NTILES = RT * NTW;
  static_assert(KS % 4 == 0 && NTILES >= 2 && RD >= 1 && RD <= NTILES, "tile geometry");
  static_assert(2 * HALO_BYTES <= f31_lds_bytes<NT, S, RT>() && c1r_lds_bytes(K, RT, N) <= f31_lds_bytes<NT, S, RT>(),
                "LDS overlay");
  OCC_C1R_RING(wp3)
  OCC_C1R_LOAD(0, 0, 0)
  OCC_C1R_LOAD(1, 0, 1)
  OCC_C1R_LOAD(2, 0, 2)
  const long img_row0 = (long)img * Ho;
  OCC_C1R_RES_START

  // ---- phase 1 epilogue: bias, ReLU, one rounding; the bf16 tile goes over the halo buffers ----------------------------
  __syncthreads();                                  // every wave is done reading the halo
  float* const sbias = reinterpret_cast<float*>(lds + TILE_BYTES + 4 * kC1rScratch);
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

  // ---- phase 2: the resident 1x1 pass loop ---------------------------------------------------------------------------------
  char* const scratch = lds + TILE_BYTES + wave * kC1rScratch;
  OCC_C1R_AFRAG_STATE
  OCC_C1R_PASSES
}

// The (stride, tile id) the fused kernel is built for: 3x3 tiles that hold all Cmid channels (128 NT = Cmid).  The waves per
// SIMD each is compiled for are those of the 3x3 variant of the same id (c3_minw).
constexpr int kF31Tiles[][2] = {{1, 12}, {1, 22}, {1, 23}, {1, 24}, {2, 12}, {2, 13}, {2, 22}};
bool f31_has(int Cmid, int stride, int id) {
  for (const auto& t : kF31Tiles)
    if (t[0] == stride && t[1] == id) return (id / 10) * 128 == Cmid;
  return false;
}

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
  const long blocks = (long)batch * ((Wo + kC3TW - 1) / kC3TW) * ((Ho + 2 * rt - 1) / (2 * rt));
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
  const int tiles_x = (Wo + kC3TW - 1) / kC3TW, tiles_y = (Ho + 2 * rt - 1) / (2 * rt);
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
    auto kern = conv3x3_conv1x1_kernel<ID / 10, SS, ID % 10, c3_minw(SS, ID), RDD>;                \
    constexpr int lds = f31_lds_bytes<ID / 10, SS, ID % 10>();                                    \
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
