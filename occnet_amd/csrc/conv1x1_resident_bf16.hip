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
#include "common.h"

namespace occ {

constexpr int kC1rPitch = 80, kC1rScratch = 32 * kC1rPitch;     // per-wave epilogue scratch: 32 rows x 64 B, padded

// LDS: activation tile + the four waves' scratch + the bias of the block's columns
// output pixel m = (n, yo, xo) of a (Hout, Wout) map -> pixel (n, yo / 2, xo / 2) of the map of half the resolution
__device__ __forceinline__ int up2_row(int m, int Hout, int Wout) {
  const unsigned hw = (unsigned)(Hout * Wout);
  const unsigned n = (unsigned)m / hw, rem = (unsigned)m - n * hw;
  const unsigned yo = rem / (unsigned)Wout, xo = rem - yo * (unsigned)Wout;
  return (int)((n * (unsigned)(Hout >> 1) + (yo >> 1)) * (unsigned)(Wout >> 1) + (xo >> 1));
}

constexpr int c1r_lds_bytes(int K, int RT, int bias_cols) { return 32 * RT * K * 2 + 4 * kC1rScratch + bias_cols * 4; }

// RES: 0 = no residual, 1 = residual of the output's size, 2 = residual of half the resolution, added nearest-upsampled x2
template <int K, int RT, int NTW, int RES, int MINB, int RD>
__global__ __launch_bounds__(256, MINB) void conv1x1_resident_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ wp, const float* __restrict__ bias,
    const unsigned short* __restrict__ residual, unsigned short* __restrict__ out, int M, int N, int Hin, int Win,
    int Hout, int Wout, int stride, int relu, int nrb, int ncb, int ppb) {
  extern __shared__ __attribute__((aligned(16))) char clds[];
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
  const int NT32 = N / 32;

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
    __builtin_amdgcn_global_load_lds(x + (long)pix * PCS + (slot ^ (r & MASK)), (lds_ptr_t)(clds + inst * 1024), 16, 0, 0);
  }

  // weight ring: slot (step & 3) = the wave's NTW column tiles of flat step = pass * KS + k-step (buffer loads: one
  // lane-offset VGPR for all of them, the step's offset in an SGPR, the tile in the immediate)
  occ_u32x4 w[4][NTW];
  const __amdgpu_buffer_rsrc_t wr = uniform_rsrc(wp, (unsigned)K * (unsigned)N * 2u);
  const int wv = (wave * NTW * 64 + lane) * 16;
  const int kstep_bytes = NT32 * 1024;
#define OCC_C1R_LOAD(SLOT, PASS, KSTEP)                                                            \
  {                                                                                               \
    const int so = (KSTEP) * kstep_bytes + (PASS) * (4 * NTW * 1024);                             \
    _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                               \
      w[SLOT][t] = __builtin_amdgcn_raw_buffer_load_b128(wr, wv + t * 1024, so, 0);               \
  }
  const int p0 = cb * ppb;
  // the bias of the block's columns goes through LDS: read from global memory at the start of a pass it would be the
  // youngest request and waiting for it would drain the weight ring
  float* const sbias = reinterpret_cast<float*>(clds + TILE_BYTES + 4 * kC1rScratch);
  for (int i = tid; i < ppb * (32 * NTW); i += 256)
    *reinterpret_cast<float4*>(sbias + 4 * i) = *reinterpret_cast<const float4*>(bias + p0 * (128 * NTW) + 4 * i);
  OCC_C1R_LOAD(0, p0, 0)
  OCC_C1R_LOAD(1, p0, 1)
  OCC_C1R_LOAD(2, p0, 2)
  __syncthreads();                                  // the tile and the bias have landed (the barrier waits for the DMA)

  char* const scratch = clds + TILE_BYTES + wave * kC1rScratch;

  // activation fragments of k-step ks (the same for every pass): double buffered, read one step ahead.  Slot of piece
  // 2 ks + kb in row vi = (2 ks) ^ ((kb ^ vi) & MASK): one XOR per step on an address the compiler cannot see through
  bf16x8 af[2][RT];
  unsigned abase = (unsigned)(vi * PITCH + ((kb ^ vi) & MASK) * 16);
#define OCC_C1R_AFRAG(BUF, KSTEP)                                                                  \
  {                                                                                               \
    asm volatile("" : "+v"(abase));                                                               \
    const char* ap = clds + (abase ^ (unsigned)((KSTEP) * 32));                                   \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                             \
      af[BUF][rt] = *reinterpret_cast<const bf16x8*>(ap + rt * (32 * PITCH));                     \
  }
  // residual row segments of tile (rt, t) of the pass whose first column (for this wave) is NW: lane -> rows (lane >> 2)
  // and + 16 of the tile, 16-byte piece lane & 3
#define OCC_C1R_RES(DST, NW, RTI, TI)                                                              \
  {                                                                                               \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                               \
      int m = m0 + (RTI) * 32 + (rlane >> 2) + 16 * j;                                            \
      if (m >= M) m = M - 1;                                                                      \
      if (RES == 2) m = up2_row(m, Hout, Wout);                                                   \
      DST[j] = *reinterpret_cast<const uint4*>(residual + (long)m * N + (NW) + (TI) * 32 + (rlane & 3) * 8); \
    }                                                                                             \
  }
  // the residual runs RD tiles ahead of the epilogue, across passes: rq[0] is the tile the epilogue takes next
  uint4 rq[RD][2];
  int rlane = lane;
  if (RES) {
    const int nw0 = p0 * (128 * NTW) + wave * (32 * NTW);
#pragma unroll
    for (int i = 0; i < RD; ++i) OCC_C1R_RES(rq[i], nw0, i / NTW, i % NTW)
  }
  OCC_C1R_AFRAG(0, 0)
#pragma unroll 1
  for (int p = p0; p < p0 + ppb; ++p) {
    const int nw = p * (128 * NTW) + wave * (32 * NTW);         // the wave's first column of this pass
    int elane = lane;                               // opaque per pass: the epilogue's offsets are recomputed here instead
    asm volatile("" : "+v"(elane));                 // of living across the k loop
    // D[column][row]: lane (vi, kb) holds row rt * 32 + vi, register 4 q + i = column 8 q + 4 kb + i of tile t.
    // The accumulators start at the bias.
    f32x16 acc[RT][NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 c0 = *reinterpret_cast<const float4*>(sbias + (nw - p0 * (128 * NTW)) + t * 32 + 8 * q + 4 * kb);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          acc[rt][t][4 * q + 0] = c0.x;
          acc[rt][t][4 * q + 1] = c0.y;
          acc[rt][t][4 * q + 2] = c0.z;
          acc[rt][t][4 * q + 3] = c0.w;
        }
      }
    const int pn = p + 1 < p0 + ppb ? p + 1 : p;     // the ring runs into the next pass (last pass: a harmless re-read)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 3 < KS) OCC_C1R_LOAD((ks + 3) & 3, p, ks + 3)
      else OCC_C1R_LOAD((ks + 3) & 3, pn, ks + 3 - KS)
      OCC_C1R_AFRAG((ks + 1) & 1, (ks + 1) & (KS - 1))
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
          acc[rt][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[ks & 3][t]), af[ks & 1][rt],
                                                               acc[rt][t], 0, 0, 0);
      // pin the software pipeline (hipcc otherwise sinks every ring request down to its use: load, vmcnt(0), MFMA)
      if (NTILES >= 4) {
        constexpr int MQ = NTILES / 4;
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);        // ring request of step s + 3
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, RT / 2, 0);   // A fragments of step s + 1
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        if (NTW > 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, RT / 2, 0);
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    }

    // ---- epilogue of the pass: one 32 x 32 tile at a time through the wave's scratch (row pitch 80 B) -------------------
    const int erow = elane >> 2, epiece = elane & 3;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        const int e = rt * NTW + t;
        if (RES) {
          const uint4 r0 = rq[0][0], r1 = rq[0][1];
#pragma unroll
          for (int i = 0; i + 1 < RD; ++i) { rq[i][0] = rq[i + 1][0]; rq[i][1] = rq[i + 1][1]; }
          asm volatile("" : "+v"(rlane));
          if (e + RD < NTILES) OCC_C1R_RES(rq[RD - 1], nw, (e + RD) / NTW, (e + RD) % NTW)
          else if (p + 1 < p0 + ppb) OCC_C1R_RES(rq[RD - 1], nw + 128 * NTW, (e + RD - NTILES) / NTW, (e + RD - NTILES) % NTW)
          *reinterpret_cast<uint4*>(scratch + erow * kC1rPitch + epiece * 16) = r0;
          *reinterpret_cast<uint4*>(scratch + (erow + 16) * kC1rPitch + epiece * 16) = r1;
          wave_lds_sync();
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          char* const sp = scratch + vi * kC1rPitch + 16 * q + 8 * kb;
          float v0 = acc[rt][t][4 * q + 0], v1 = acc[rt][t][4 * q + 1], v2 = acc[rt][t][4 * q + 2],
                v3 = acc[rt][t][4 * q + 3];
          if (RES) {
            const uint2 r = *reinterpret_cast<const uint2*>(sp);
            v0 += bf16_lo_to_f32(r.x); v1 += bf16_hi_to_f32(r.x); v2 += bf16_lo_to_f32(r.y); v3 += bf16_hi_to_f32(r.y);
          }
          if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
          *reinterpret_cast<uint2*>(sp) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3));
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int row = erow + 16 * j;
          const int m = m0 + rt * 32 + row;
          const uint4 v = *reinterpret_cast<const uint4*>(scratch + row * kC1rPitch + epiece * 16);
          if (m < M) *reinterpret_cast<uint4*>(out + (long)m * N + nw + t * 32 + epiece * 8) = v;
        }
        wave_lds_sync();
      }
    }
  }
#undef OCC_C1R_RES
#undef OCC_C1R_AFRAG
#undef OCC_C1R_LOAD
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
