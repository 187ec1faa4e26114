// Backbone 1x1 convolutions (NHWC bf16), ACTIVATION-RESIDENT variant for Cin in {128, 256, 512}: the same function as
// conv1x1_nhwc_bf16.hip,  out = relu?( x . W^T + bias (+ residual) ), bf16 in / f32 accumulate / one RNE rounding / bf16 out,
// on the structure of value_proj_resident_kernel (value_proj_bf16.hip).
//
// The tiled kernel meets a block barrier every 32 input channels and runs its epilogue (residual loads, f32 LDS transpose, two
// barriers per 32 rows) after the K loop: loads, MFMAs and stores add up instead of overlapping.  Here a block owns 32 * RT
// output pixels (RT = 4, or 2 for the 64-row tile) and a run of column passes:
//   * its (32 RT) x K activation tile goes global -> LDS once, by LDS-DMA (no registers), 16-byte pieces XOR-swizzled by row
//     so the fragment reads (ds_read_b128, row pitch 2 K bytes) are bank-conflict-free; a strided convolution only changes
//     the source pixel of a tile row (the DMA takes a per-lane address);
//   * after that ONE barrier the four waves never synchronise again: wave w walks the passes (128 NTW columns per pass, the
//     wave's 32 NTW of them as NTW column tiles x RT row tiles), streaming its weight fragments from L2 through a 4-deep
//     register ring that runs ahead across k-steps AND passes.  The weights are the B-fragment pack conv1x1_pack_weight
//     makes for the tiled kernel: for v_mfma_f32_32x32x16_bf16 the row and the column operand have the same lane layout, so
//     the TRANSPOSED product (weights as the row operand) reads the same buffer;
//   * transposed, a lane ends up with 16 columns of ONE output row, four consecutive ones per register quad.  Epilogue per
//     32 x 32 tile, inside the wave: the residual (of the output's size, or of half the resolution and added nearest-
//     upsampled x2) arrives as 16-byte row segments, requested RD tiles ahead and across passes so that they travel under
//     the MFMAs, and is laid into the wave's 2.5 KB scratch; every lane adds its quads in f32, applies the ReLU, rounds
//     ONCE and writes the bf16 quad back in place; the rows leave as 16-byte segments.  The accumulators start at the
//     bias, which is staged in LDS with the tile (a global read at the start of a pass would drain the weight ring).
//   * small maps: the grid also splits the column passes (ncb column blocks per row tile, ppb passes each).  The column
//     blocks of a row tile are dealt to ONE XCD and dispatched together (linear id = (rb / 8) * 8 ncb + cb * 8 + rb % 8, as
//     the tiled value projection does), so the tile comes from HBM once and from that XCD's L2 afterwards.
// K is summed in a fixed order, independent of the grid: two launches on the same inputs are bit-identical.
#include <cstdlib>
#include "conv1x1_resident_pass.h"

namespace occ {

// output pixel m = (n, yo, xo) of a (Hout, Wout) map -> pixel (n, yo / 2, xo / 2) of the map of half the resolution
__device__ __forceinline__ int up2_row(int m, int Hout, int Wout) {
  const unsigned hw = (unsigned)(Hout * Wout);
  const unsigned n = (unsigned)m / hw, rem = (unsigned)m - n * hw;
  const unsigned yo = rem / (unsigned)Wout, xo = rem - yo * (unsigned)Wout;
  return (int)((n * (unsigned)(Hout >> 1) + (yo >> 1)) * (unsigned)(Wout >> 1) + (xo >> 1));
}

// What the pass loop (conv1x1_resident_pass.h) takes from this kernel: the block's run of passes, the switches, and rows
// that are flat pixel indices m0 + tile row, clamped to the last pixel for loads and masked by m < M for stores
#define OCC_C1R_P_BEGIN p0
#define OCC_C1R_P_END (p0 + ppb)
#define OCC_C1R_RESIDUAL RES
#define OCC_C1R_RELU relu
#define OCC_C1R_RES_ROW(RTI, J)                                                                   \
  int m = m0 + (RTI) * 32 + (rlane >> 2) + 16 * (J);                                              \
  if (m >= M) m = M - 1;                                                                          \
  if (RES == 2) m = up2_row(m, Hout, Wout);
#define OCC_C1R_RES_PIXEL (long)m
#define OCC_C1R_PASS_LOCALS
#define OCC_C1R_OUT_ROW(RTI, J)                                                                   \
  const int m = m0 + (RTI) * 32 + (erow + 16 * (J));                                              \
  const bool olive = m < M;                                                                       \
  const long orow = m;

// RES: 0 = no residual, 1 = residual of the output's size, 2 = residual of half the resolution, added nearest-upsampled x2
template <int K, int RT, int NTW, int RES, int MINB, int RD>
__global__ __launch_bounds__(256, MINB) void conv1x1_resident_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ wp, const float* __restrict__ bias,
    const unsigned short* __restrict__ residual, unsigned short* __restrict__ out, int M, int N, int Hin, int Win,
    int Hout, int Wout, int stride, int relu, int nrb, int ncb, int ppb) {
  extern __shared__ __attribute__((aligned(16))) char clds[];
  char* const lds = clds;
  constexpr int BM = 32 * RT, PCS = K / 8, PITCH = K * 2, KS = K / 16;
  constexpr int MASK = (PCS < 32 ? PCS : 32) - 1;            // swizzle: slot s of row r holds piece s ^ (r & MASK)
  constexpr int RPI = 64 / PCS;                              // tile rows per DMA instruction (1 KB of LDS each)
  constexpr int NINST = BM / RPI / 4;                        // DMA instructions per wave
  constexpr int TILE_BYTES = BM * PITCH;
  constexpr int NTILES = RT * NTW;                           // 32 x 32 tiles of a wave per pass
  static_assert(PCS <= 64 && KS % 4 == 0 && NTILES >= 2 && RT % 2 == 0 && RD >= 1 && RD <= NTILES, "tile geometry");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  int rb = (int)blockIdx.x, cb = 0;
  if (ncb > 1) {
    const int id = (int)blockIdx.x, grp = id / (8 * ncb), within = id % (8 * ncb);
    rb = grp * 8 + (within & 7);
    cb = within >> 3;
  }
  if (rb >= nrb) return;                                     // padding of the last group of 8 row tiles
  const int m0 = rb * BM;

  // activation tile
#pragma unroll
  for (int j = 0; j < NINST; ++j) {
    const int inst = wave * NINST + j;
    const int r = inst * RPI + lane / PCS, slot = lane % PCS;
    int m = m0 + r;
    if (m >= M) m = M - 1;
    int pix = m;
    if (stride != 1) {          // output pixel (n, yo, xo) reads input pixel (n, yo * stride, xo * stride)
      const unsigned hw = (unsigned)(Hout * Wout);
      const unsigned n = (unsigned)m / hw, rem = (unsigned)m - n * hw;
      const unsigned yo = rem / (unsigned)Wout, xo = rem - yo * (unsigned)Wout;
      pix = (int)((n * (unsigned)Hin + yo * (unsigned)stride) * (unsigned)Win + xo * (unsigned)stride);
    }
    __builtin_amdgcn_global_load_lds(x + (long)pix * PCS + (slot ^ (r & MASK)), (lds_ptr_t)(lds + inst * 1024), 16, 0, 0);
  }

  OCC_C1R_RING(wp)
  const int p0 = cb * ppb;
  // the bias of the block's columns goes through LDS: read from global memory at the start of a pass it would be the
  // youngest request and waiting for it would drain the weight ring
  float* const sbias = reinterpret_cast<float*>(lds + TILE_BYTES + 4 * kC1rScratch);
  for (int i = tid; i < ppb * (32 * NTW); i += 256)
    *reinterpret_cast<float4*>(sbias + 4 * i) = *reinterpret_cast<const float4*>(bias + p0 * (128 * NTW) + 4 * i);
  OCC_C1R_LOAD(0, p0, 0)
  OCC_C1R_LOAD(1, p0, 1)
  OCC_C1R_LOAD(2, p0, 2)
  __syncthreads();                                  // the tile and the bias have landed (the barrier waits for the DMA)

  char* const scratch = lds + TILE_BYTES + wave * kC1rScratch;
  OCC_C1R_AFRAG_STATE
  OCC_C1R_RES_START
  OCC_C1R_PASSES
}

// Which resident tile the arguments have a kernel for: 0 = none.  rt = 0 asks for the default tile of the shape, 2 / 4
// for the 64- / 128-row tile.  K > 512 (the tile does not fit LDS) stays on the tiled kernel.
int conv1x1_resident_tile(int Cin, int Cout, long M, long in_pixels, int rt) {
  if ((Cin != 128 && Cin != 256 && Cin != 512) || Cout % 128 || Cout > 4096) return 0;
  if (M >= (1L << 30) || in_pixels >= (1L << 30)) return 0;      // 32-bit row indices
  // default tile: at K = 512 the 128-row tile (128 KB) leaves one block per CU, whose load, MFMA and store phases no
  // other block covers; the 64-row tile runs two (sweep: EXPERIMENTS.md section 8g)
  if (rt == 0) rt = Cin == 512 ? 2 : 4;
  if (rt == 4) return 4;
  if (rt == 2 && Cin == 512) return 2;                               // the 64-row tile: two blocks per CU at K = 512
  return 0;
}

// ncb_force: 0 = column blocks chosen here; else the number of column blocks per row tile (must divide the passes)
int conv1x1_resident_launch(const void* x, const void* weight, const float* bias, const void* residual, void* out,
                            long M, int Hin, int Win, int Hout, int Wout, int Cin, int Cout, int stride, int relu,
                            int residual_upsample2, int rt, int ncb_force, hipStream_t st) {
  const int ntw = Cout % 256 == 0 ? 2 : 1;
  const int np = Cout / (128 * ntw);
  const int nrb = (int)((M + 32 * rt - 1) / (32 * rt));
  // column blocks per row tile: the smallest divisor of the passes that gives the grid four blocks per CU (eight at
  // K = 128, whose k loop is half as long) - the split every shape of the ResNet-50 table measured fastest with
  // (tools_dev/conv_probe.py c1x, EXPERIMENTS.md section 8g); fewer passes per block cost nothing because the column
  // blocks of a row tile share one XCD's L2
  const long want_blocks = Cin == 128 ? 2048 : 1024;
  int ncb = np;
  for (int d = 1; d <= np; ++d)
    if (np % d == 0 && (long)nrb * d >= want_blocks) { ncb = d; break; }
  if (ncb_force > 0) {
    if (np % ncb_force) {
      set_error("conv1x1_nhwc_bf16: no variant with %d column blocks for %d passes", ncb_force, np);
      return OCC_E_UNSUPPORTED;
    }
    ncb = ncb_force;
  }
  const int ppb = np / ncb;
  const unsigned grid = ncb > 1 ? (unsigned)((nrb + 7) / 8 * 8 * ncb) : (unsigned)nrb;
  hipError_t e = hipSuccess;
#define OCC_C1R_GO(KK, RTT, NTT, RR, MINB, RDD)                                                          \
  {                                                                                               \
    auto kern = conv1x1_resident_kernel<KK, RTT, NTT, RR, MINB, RR ? RDD : 1>;                                  \
    const int lds = c1r_lds_bytes(KK, RTT, ppb * 128 * NTT);                                                \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
    if (e == hipSuccess)                                                                          \
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, reinterpret_cast<const uint4*>(x),  \
                         reinterpret_cast<const uint4*>(weight), bias,                            \
                         reinterpret_cast<const unsigned short*>(residual),                       \
                         reinterpret_cast<unsigned short*>(out), (int)M, Cout, Hin, Win, Hout, Wout, stride, relu, nrb, \
                         ncb, ppb);                                                               \
  }
#define OCC_C1R_RES_(KK, RTT, NTT, MINB, RDD)                                                       \
  {                                                                                               \
    if (residual && residual_upsample2) OCC_C1R_GO(KK, RTT, NTT, 2, MINB, RDD)                    \
    else if (residual) OCC_C1R_GO(KK, RTT, NTT, 1, MINB, RDD)                                     \
    else OCC_C1R_GO(KK, RTT, NTT, 0, MINB, RDD)                                                   \
  }
// residual tiles in flight per wave (8 VGPRs each): what the register budget of the instance leaves
#define OCC_C1R_NT_(KK, RTT, MINB, RD2, RD1) { if (ntw == 2) OCC_C1R_RES_(KK, RTT, 2, MINB, RD2) else OCC_C1R_RES_(KK, RTT, 1, MINB, RD1) }
  if (Cin == 128) OCC_C1R_NT_(128, 4, 2, 6, 4)
  else if (Cin == 256) OCC_C1R_NT_(256, 4, 2, 4, 4)
  else if (rt == 2) OCC_C1R_NT_(512, 2, 2, 4, 2)
  else OCC_C1R_NT_(512, 4, 1, 8, 4)
#undef OCC_C1R_NT_
#undef OCC_C1R_RES_
#undef OCC_C1R_GO
  if (e != hipSuccess) {
    set_error("conv1x1_nhwc_bf16: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    return OCC_E_LAUNCH;
  }
  OCC_CHECK_LAUNCH("conv1x1_nhwc_bf16 (resident)");
  return OCC_OK;
}

}  // namespace occ
