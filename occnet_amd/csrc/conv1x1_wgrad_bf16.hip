// Weight gradient of a 1x1 convolution on NHWC bf16 activations (bf16 matrix cores, f32 accumulation) for gfx950.
//
//   dw[o][i] = sum over (n, yo, xo) of g[(n, yo, xo), o] * x[(n, yo * stride, xo * stride), i]
//
// The training-side partner of conv1x1_nhwc_bf16.hip: ConvBNActFunction's backward (plugin/backbone.py) took this product
// from ATen's convolution_backward (MIOpen / CK) for every shape.  The data gradient needs no kernel of its own: it is
// occ_conv1x1_nhwc_bf16(g, pack(W^T)).
//
// Shape of the problem: P = N * Ho * Wo = 8 700 .. 556 800 pixels is the REDUCTION dimension, the output is small
// (128 x 256 .. 512 x 2048).  As in linear_wgrad.hip the reduction is split over `splits` pixel ranges (grid.y); every
// block owns one 128 x 128 output tile of one range and writes its f32 partial tile to the workspace, and a second kernel
// adds the partials in a fixed order and rounds once to the requested output type (deterministic: no float atomics).
//
// Operand layout: the REGISTER-ONLY scheme of linear_wgrad.hip, adapted to 2-byte elements (the GEMM kernel uses no LDS and no
// transposed LDS read; the reduce kernel combines its four wave sums through 1 KB of it).  For v_mfma_f32_32x32x16_bf16 lane l holds, of the A operand, row l % 32 and the 8 reduction indices
// 8 * (l / 32) .. +7.  WHICH channel a row of the fragment stands for is free as long as the store uses the same map, so
// lane l loads ONE DWORD per pixel — channels 2 * (l % 32) and 2 * (l % 32) + 1 of a 64-channel group — for its 8
// consecutive pixels: the low halves of the 8 dwords are the fragment of the group's even channels, the high halves that
// of the odd channels (one v_perm_b32 per packed pair: 8 VALU ops per two fragments).  A wave instruction reads two fully
// used 128-byte segments (lanes 0-31: pixel m + j, lanes 32-63: pixel m + 8 + j); 16 dword loads feed 4 MFMAs of a wave's
// 64 x 64 tile, and the accumulator pair (even i, odd i) of a lane is one 8-byte store.  Chosen over staging pixel x
// channel tiles in LDS for the transposed read (ds_read_b64_tr_b16) because the global loads already arrive in
// fragment order: the LDS round trip would add a write, a barrier and a read per tile and remove no instruction, and this
// form keeps the ragged-end handling of linear_wgrad.hip (clamped rows, wave-uniform zeroing) unchanged.
//
// Ragged ends: a pixel index beyond P is clamped to P - 1 for the address (stride 2: the x row of the last valid pixel)
// and rows beyond the block's range are zeroed in BOTH operands under a wave-uniform condition; channel pairs beyond
// Cout / Cin (tiles of 128 over multiples of 32) are clamped for the load and dropped at the store.  No out-of-bounds
// address is formed.
//
// Compiler resource remarks (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   conv1x1_wgrad_kernel<true>  (stride 1)  180 VGPRs, 0 AGPRs, no scratch, no spills, 0 B LDS, 2 waves / SIMD
//   conv1x1_wgrad_kernel<false> (strided)   130 VGPRs, 0 AGPRs, no scratch, no spills, 0 B LDS
//   conv1x1_wgrad_reduce_kernel             32 VGPRs, 0 AGPRs, no scratch, no spills, 1 024 B LDS
#include "common.h"
#include "conv_wgrad.h"      // cw_frag, conv_wgrad_reduce_launch

namespace occ {

struct WgradGeo {       // pixel index -> x row, for the strided form
  int H, W, Ho, Wo, stride;
};

// pixels m .. m+15 of this wave's g channel group and x channel group -> raw registers.  Pixels are clamped to P - 1 so
// the load is always legal; `left` < 16 zeroes the pixels beyond the block's range (wave-uniform branch).
template <bool S1>
__device__ __forceinline__ void cw_load(const unsigned short* __restrict__ pg, const unsigned short* __restrict__ px,
                                        int Cin, int Cout, int m, int g, int P, int left, const WgradGeo& geo,
                                        unsigned (&a)[8], unsigned (&b)[8]) {
  const int p0 = m + 8 * g;
  int n = 0, yo = 0, xo = 0;
  long last = 0;
  if (!S1) {
    const int pc = p0 < P ? p0 : P - 1;
    const int q = pc / geo.Wo;
    xo = pc - q * geo.Wo;
    n = q / geo.Ho;
    yo = q - n * geo.Ho;
    last = ((long)n * geo.H + (long)yo * geo.stride) * geo.W + (long)xo * geo.stride;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = p0 + j;
    const long r = p < P ? p : P - 1;
    long xr = r;
    if (!S1) {
      if (p < P) last = ((long)n * geo.H + (long)yo * geo.stride) * geo.W + (long)xo * geo.stride;
      xr = last;
      if (++xo == geo.Wo) {
        xo = 0;
        if (++yo == geo.Ho) {
          yo = 0;
          ++n;
        }
      }
    }
    a[j] = *reinterpret_cast<const unsigned*>(pg + r * Cout);
    b[j] = *reinterpret_cast<const unsigned*>(px + xr * Cin);
  }
  if (left < 16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = 8 * g + j < left;
      a[j] = ok ? a[j] : 0u;
      b[j] = ok ? b[j] : 0u;
    }
  }
}

// acc[2 * t + u]: t = parity of the output channel, u = parity of the input channel
__device__ __forceinline__ void cw_step(const unsigned (&a)[8], const unsigned (&b)[8], f32x16 (&acc)[4]) {
  bf16x8 a0, a1, b0, b1;
  cw_frag(a, a0, a1);
  cw_frag(b, b0, b1);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[1], 0, 0, 0);
  acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[2], 0, 0, 0);
  acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[3], 0, 0, 0);
}

// grid (tiles_o * tiles_i, splits); block = 4 waves as 2 x 2 over a 128 (o) x 128 (i) tile
template <bool S1>
__global__ __launch_bounds__(256, 2) void conv1x1_wgrad_kernel(const unsigned short* __restrict__ gy,
                                                               const unsigned short* __restrict__ x,
                                                               float* __restrict__ part, int P, int Cin, int Cout,
                                                               int PC, int tiles_i, WgradGeo geo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, g = lane >> 5;
  const int tile_o = blockIdx.x / tiles_i, tile_i = blockIdx.x - tile_o * tiles_i;
  const int c = blockIdx.y;
  const int o0 = tile_o * 128 + (wave >> 1) * 64, i0 = tile_i * 128 + (wave & 1) * 64;
  const int m_begin = c * PC;
  const int m_end = m_begin + PC < P ? m_begin + PC : P;

  // this lane's channel pair; pairs beyond Cout / Cin are clamped for the load and dropped at the store
  const int og = o0 + 2 * col, ig = i0 + 2 * col;
  const unsigned short* pg = gy + (og < Cout ? og : Cout - 2);
  const unsigned short* px = x + (ig < Cin ? ig : Cin - 2);

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  unsigned a0[8], b0[8], a1[8], b1[8];
  int m = m_begin;
  if (S1) {
    // stride 1 (x row = pixel), the steps whose 16 pixels all lie inside the range: a wave-uniform base that moves with the
    // step plus this lane's eight constant 32-bit byte offsets (one 64-bit add per load, no multiply).  Two steps per
    // iteration: the next 16 pixels are requested before the current ones are consumed.
    unsigned oa[8], ob[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      oa[j] = (unsigned)((8 * g + j) * Cout + (og < Cout ? og : Cout - 2)) * 2u;
      ob[j] = (unsigned)((8 * g + j) * Cin + (ig < Cin ? ig : Cin - 2)) * 2u;
    }
    auto full = [&](const char* gb, const char* xb, unsigned (&a)[8], unsigned (&b)[8]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[j] = *reinterpret_cast<const unsigned*>(gb + oa[j]);
        b[j] = *reinterpret_cast<const unsigned*>(xb + ob[j]);
      }
    };
    const int n_full = (m_end - m_begin) / 16;
    const long sg = 32L * Cout, sx = 32L * Cin;        // bytes per step
    const char* gb = reinterpret_cast<const char*>(gy) + (long)m_begin * Cout * 2;
    const char* xb = reinterpret_cast<const char*>(x) + (long)m_begin * Cin * 2;
    if (n_full > 0) full(gb, xb, a0, b0);
    int s = 0;
    for (; s + 2 <= n_full; s += 2) {                  // a0 / b0 hold step s
      full(gb + sg, xb + sx, a1, b1);
      cw_step(a0, b0, acc);
      gb += 2 * sg;
      xb += 2 * sx;
      if (s + 2 < n_full) full(gb, xb, a0, b0);
      cw_step(a1, b1, acc);
    }
    if (s < n_full) cw_step(a0, b0, acc);              // an odd count: the last step is already loaded
    m = m_begin + 16 * n_full;
  }
  // the ragged last step of a range (clamped, zeroed: cw_load), and every step of the strided form
  if (m < m_end) cw_load<S1>(pg, px, Cin, Cout, m, g, P, m_end - m, geo, a0, b0);
  for (; m + 16 < m_end; m += 32) {                    // a0 / b0 hold the step at m
    cw_load<S1>(pg, px, Cin, Cout, m + 16, g, P, m_end - m - 16, geo, a1, b1);
    cw_step(a0, b0, acc);
    if (m + 32 < m_end) cw_load<S1>(pg, px, Cin, Cout, m + 32, g, P, m_end - m - 32, geo, a0, b0);
    cw_step(a1, b1, acc);
  }
  if (m < m_end) cw_step(a0, b0, acc);

  // partial tile: D[row][col] with row = 8 * (r / 4) + 4 * g + r % 4; fragment row a of parity t is channel o0 + 2 a + t,
  // fragment column `col` of parity u is channel i0 + 2 col + u: the (u = 0, u = 1) pair of a lane is one 8-byte store
  float* pw = part + (long)c * Cout * Cin;
  if (ig < Cin) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + 2 * (8 * (r >> 2) + 4 * g + (r & 3)) + t;
        if (o < Cout) *reinterpret_cast<float2*>(pw + (long)o * Cin + ig) = make_float2(acc[2 * t][r], acc[2 * t + 1][r]);
      }
    }
  }
}

// dw = sum_c partial[c] in a fixed order, rounded once to the output type: a block owns 64 consecutive outputs, its 4
// waves each add every 4th range (4 independent loads in flight per lane), and the four wave sums are combined in wave
// order through LDS (the scheme of linear_wgrad_reduce_kernel).
__global__ __launch_bounds__(256) void conv1x1_wgrad_reduce_kernel(const float* __restrict__ part, void* __restrict__ dw,
                                                                   long OI, int chunks, int dw_bf16) {
  __shared__ float red[4][64];
  const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + o;
  const bool ok = i < OI;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (ok) {
    int c = g;
    for (; c + 12 < chunks; c += 16) {
      s0 += part[(long)c * OI + i];
      s1 += part[(long)(c + 4) * OI + i];
      s2 += part[(long)(c + 8) * OI + i];
      s3 += part[(long)(c + 12) * OI + i];
    }
    for (; c < chunks; c += 4) s0 += part[(long)c * OI + i];
  }
  red[g][o] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && ok) {
    const float r = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    if (dw_bf16) reinterpret_cast<unsigned short*>(dw)[i] = bf16_rne(r);
    else reinterpret_cast<float*>(dw)[i] = r;
  }
}

struct WgradPlan {
  long P;
  int tiles_o, tiles_i, chunks, PC, Ho, Wo;
};

// false: no kernel for these arguments.  splits == 0: the launcher's choice; splits > 0: AT MOST that many ranges (and at most
// min(P, 4096)): the ranges are equal, ceil(P / splits) pixels each, and as many as cover P (P = 10, splits = 7: 5 ranges of 2).
// The workspace size and the launch both use the count computed here.
static bool cw_plan(int N, int H, int W, int Cin, int Cout, int stride, int splits, WgradPlan& pl) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || splits < 0) return false;
  if (Cin % 32 || Cout % 32 || Cin > 2048 || Cout > 2048 || (stride != 1 && stride != 2)) return false;
  pl.Ho = (H - 1) / stride + 1;
  pl.Wo = (W - 1) / stride + 1;
  pl.P = (long)N * pl.Ho * pl.Wo;
  if ((long)N * H * W >= (1L << 31) - 64) return false;      // pixel indices are ints (+ 16 of look-ahead)
  pl.tiles_o = (Cout + 127) / 128;
  pl.tiles_i = (Cin + 127) / 128;
  const int tiles = pl.tiles_o * pl.tiles_i;
  long want;
  if (splits > 0) {
    want = splits < 4096 ? splits : 4096;
    if (want > pl.P) want = pl.P;
  } else {
    // 512 blocks = two per CU, all resident at once; every range costs one Cout x Cin partial written and read back, so
    // small outputs take what fills the chip and no more, and a block keeps at least 8 MFMA steps
    want = (512 + tiles - 1) / tiles;
    const long max_chunks = (pl.P + 127) / 128;
    if (want > max_chunks) want = max_chunks;
    if (want < 1) want = 1;
  }
  pl.PC = (int)((pl.P + want - 1) / want);
  pl.chunks = (int)((pl.P + pl.PC - 1) / pl.PC);
  return true;
}

hipError_t conv_wgrad_reduce_launch(const float* part, void* dw, long OI, int chunks, int dw_bf16, hipStream_t st) {
  hipLaunchKernelGGL(conv1x1_wgrad_reduce_kernel, dim3((unsigned)((OI + 63) / 64)), dim3(256), 0, st, part, dw, OI, chunks,
                     dw_bf16 ? 1 : 0);
  return hipGetLastError();
}

}  // namespace occ

extern "C" int64_t occ_conv1x1_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride, int splits) {
  occ::WgradPlan pl;
  if (!occ::cw_plan(N, H, W, Cin, Cout, stride, splits, pl)) return 0;
  return (int64_t)pl.chunks * Cout * Cin * 4;
}

extern "C" int occ_conv1x1_wgrad_nhwc_bf16(const void* g, const void* x, void* dw, int dw_bf16, void* workspace, int N,
                                           int H, int W, int Cin, int Cout, int stride, int splits, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(g && x && dw && workspace, "conv1x1_wgrad: null pointer argument");
  OCC_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv1x1_wgrad: bad dimension (N=%d H=%d W=%d Cin=%d Cout=%d)",
                N, H, W, Cin, Cout);
  OCC_CHECK_ARG(splits >= 0, "conv1x1_wgrad: negative splits (%d)", splits);
  WgradPlan pl;
  if (!cw_plan(N, H, W, Cin, Cout, stride, splits, pl)) {
    set_error("conv1x1_wgrad: needs Cin %% 32 == 0, Cout %% 32 == 0, both <= 2048, stride 1 or 2 (Cin=%d Cout=%d stride=%d)",
              Cin, Cout, stride);
    return OCC_E_UNSUPPORTED;
  }
  OCC_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)x & 3) == 0 && ((uintptr_t)dw & 3) == 0 &&
                ((uintptr_t)workspace & 7) == 0,
                "conv1x1_wgrad: g / x / dw must be 4-byte aligned, the workspace 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned short* gp = reinterpret_cast<const unsigned short*>(g);
  const unsigned short* xp = reinterpret_cast<const unsigned short*>(x);
  float* part = reinterpret_cast<float*>(workspace);
  const WgradGeo geo = {H, W, pl.Ho, pl.Wo, stride};
  const dim3 grid((unsigned)(pl.tiles_o * pl.tiles_i), (unsigned)pl.chunks);
  if (stride == 1)
    hipLaunchKernelGGL(conv1x1_wgrad_kernel<true>, grid, dim3(256), 0, st, gp, xp, part, (int)pl.P, Cin, Cout, pl.PC,
                       pl.tiles_i, geo);
  else
    hipLaunchKernelGGL(conv1x1_wgrad_kernel<false>, grid, dim3(256), 0, st, gp, xp, part, (int)pl.P, Cin, Cout, pl.PC,
                       pl.tiles_i, geo);
  OCC_CHECK_LAUNCH("conv1x1_wgrad");
  const hipError_t e = conv_wgrad_reduce_launch(part, dw, (long)Cout * Cin, pl.chunks, dw_bf16, st);
  if (e != hipSuccess) {
    set_error("conv1x1_wgrad_reduce: launch failed: %s", hipGetErrorString(e));
    return OCC_E_LAUNCH;
  }
  return OCC_OK;
}
