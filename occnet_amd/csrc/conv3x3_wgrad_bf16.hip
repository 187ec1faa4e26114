// Weight gradient of a 3x3 / pad 1 convolution on NHWC bf16 activations (bf16 matrix cores, f32 accumulation) for gfx950.
//
//   dw[o][ky][kx][i] = sum over (n, yo, xo) of g[(n, yo, xo), o] * x[(n, yo * s + ky - 1, xo * s + kx - 1), i]
//                      (terms outside the map are zero; s = stride 1 or 2)
//
// The training-side partner of conv3x3_nhwc_bf16.hip: ConvBNActFunction's backward (plugin/backbone.py) took this product
// from ATen's convolution_backward (MIOpen / CK) for every 3x3 node.  The stride-1 data gradient needs no kernel of its own:
// it is occ_conv3x3_nhwc_bf16(g, pack(flipped, transposed W)).
//
// Operands: the register-only scheme of conv1x1_wgrad_bf16.hip (conv_wgrad.h: one dword per pixel = a channel pair, eight
// pixels per lane, v_perm_b32 into the even / odd channel fragments of v_mfma_f32_32x32x16_bf16; no LDS).  The output is
// [Cout][3][3][Cin] in memory, so the (even i, odd i) accumulator pair of a lane stays one 8-byte store, and the partials
// of the split reduction are Cout * 9 * Cin flat floats per range: conv1x1_wgrad_reduce_kernel adds them unchanged.
//
// Taps: nine taps x a 64 x 64 wave tile do not fit the accumulators (9 x 64 registers).  The grid carries ky (grid.z = 3)
// and a wave keeps the THREE kx taps of its 64 (o) x 64 (i) tile: 3 x 4 x 16 = 192 accumulator registers (AGPRs), and the g
// fragment pair built once per step feeds all three taps (12 MFMAs per 8 g dwords).  The three taps also share their x loads:
// tap kx of pixel j reads column s * j + kx of the lane's run, so a step loads 7 s + 3 distinct x dwords (10 at stride 1, 17
// at stride 2) instead of 24.  The price is one wave per SIMD (more than 256 registers); a block is 4 waves as 2 x 2 over a
// 128 x 128 tile and the launcher asks for about one block per CU.  With one wave per SIMD nothing but the wave itself hides
// memory latency: it keeps C3_DEPTH = 4 register buffers, i.e. the loads of three steps (54 / 75 dwords) in flight across
// the MFMAs of the current one.
//
// Pixel walk: the reduction is cut at WHOLE OUTPUT ROWS.  Range c of `chunks` owns the rows r = n * Ho + yo of
// [c R / chunks, (c + 1) R / chunks), R = N * Ho; a step is 16 consecutive xo of one row (lanes 0-31: xo .. xo + 7, lanes
// 32-63: xo + 8 .. xo + 15).  Everything about a row is wave-uniform and carried incrementally (++yo, wrap, ++n: no
// division in the loop): the g row starts at r * Wo pixels, the x row at (n * H + yo * s + ky - 1) * W, so the ky predicate
// is one scalar test per step.  A row whose input row lies outside the map keeps its steps and contributes zeros (one row in
// Ho for ky = 0 and, at stride 1 or odd H, ky = 2; the trip count stays a product and the loop has no data-dependent exit).
// Inside a row a lane adds 32-bit byte offsets to two uniform 64-bit row bases (global_load with an SGPR base).  Only a
// row's first and last step can touch the kx border or the row's end: those steps (a wave-uniform test, C3Walk::inner) clamp
// the pixel and the column into the row for the address and zero, before the fragments are built, the g dword of every pixel
// beyond Wo and the x dword of every (pixel, tap) whose pixel lies beyond Wo or whose column lies outside [0, W); every other
// step adds constants and masks nothing.  The zeroing happens where the registers are consumed, not where they are loaded,
// so it does not wait for loads in flight.  No out-of-bounds address is formed.  A row of Wo < 16 pixels still costs a whole
// step: narrow maps waste lanes, never correctness.
// No load sits under a branch (past the end of its range the walk repeats the last row and the look-ahead requests a few
// steps that are never consumed): s_waitcnt's counts are exact only when every path issues the same loads.
//
// Ragged channels: pairs beyond Cout / Cin (tiles of 128 over multiples of 32) are clamped for the load and dropped at the
// store.  A range whose rows all lie outside for this ky (H = 1 and ky != 1) stores exact zeros: every workspace float that
// the reduce reads has been written by the same call.
// Non-finite inputs: an x value enters only the taps whose exact sum contains it (a term outside the map has BOTH operands
// zero on the x side: a non-finite x next to the border does not leak into a tap that never reads it).  The g fragment is
// shared by the three taps, so a term outside the map is g * 0: a NON-FINITE g at a pixel of a row's first or last step, or
// of a row whose input row is outside, also makes the border taps of its output channel NaN, which the exact sum leaves
// finite.  Precondition for exact border taps: finite g.
//
// Compiler resource remarks (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   conv3x3_wgrad_kernel<1>  (stride 1)  122 VGPRs, 194 AGPRs, no scratch, no spills, 0 B LDS, 1 wave / SIMD
//   conv3x3_wgrad_kernel<2>  (stride 2)  162 VGPRs, 194 AGPRs, no scratch, no spills, 0 B LDS, 1 wave / SIMD
//   (the reduce is conv1x1_wgrad_reduce_kernel: conv1x1_wgrad_bf16.hip)
#include "common.h"
#include "conv_wgrad.h"      // cw_frag, conv_wgrad_reduce_launch

namespace occ {

// The wave-uniform walk over a block's steps: the rows of its range in order, 16 output pixels per step; (n, yo) follow r
// incrementally.  A row whose input row yo * S + ky - 1 lies outside the map keeps its steps (the trip count stays a product)
// and contributes zeros: ok() is false, the loads go to the clamped row and the step zeroes its registers.
template <int S>
struct C3Walk {
  int r, n, yo, xs;
  __device__ __forceinline__ int yi(int ky) const { return yo * S + ky - 1; }
  __device__ __forceinline__ bool ok(int H, int ky) const { return (unsigned)yi(ky) < (unsigned)H; }
  // a step that touches no border: nothing to clamp, nothing to zero (xs + 15 < Wo follows from the second condition)
  __device__ __forceinline__ bool inner(int H, int W, int ky) const { return ok(H, ky) && xs > 0 && (xs + 15) * S + 1 < W; }
  // the walk never leaves the range: past its last step it repeats the last row (the look-ahead requests a few steps beyond
  // the end without a branch around the loads; they are legal and never consumed)
  __device__ __forceinline__ void next(int Ho, int Wo, int r_end) {
    xs += 16;
    if (xs >= Wo) {
      xs = 0;
      if (r + 1 < r_end) {
        ++r;
        if (++yo == Ho) {
          yo = 0;
          ++n;
        }
      }
    }
  }
};

// One step's raw registers: a[j] = the g dword of pixel xo0 + j, b[c] = the x dword of column xo0 * S - 1 + c (xo0 = xs + 8 *
// (lane / 32)); tap kx of pixel j is b[S * j + kx].
template <int S>
struct C3Regs {
  static constexpr int NC = 7 * S + 3;
  unsigned a[8], b[NC];
};

// Request a step.  lg / lx: byte offset of this lane's channel pair inside a pixel.  Any step but an inner one clamps the
// pixel and the column into the row (c3_step zeroes what was clamped).
template <int S>
__device__ __forceinline__ void c3_load(const C3Walk<S>& w, const char* __restrict__ gy, const char* __restrict__ x, int H,
                                        int W, int Wo, int ky, int Cin, int Cout, unsigned lg, unsigned lx, int g,
                                        C3Regs<S>& q) {
  constexpr int NC = C3Regs<S>::NC;
  const int yc = w.yi(ky) < 0 ? 0 : w.yi(ky) > H - 1 ? H - 1 : w.yi(ky);
  const char* gb = gy + (long)w.r * Wo * Cout * 2;                                // uniform row bases
  const char* xb = x + ((long)w.n * H + yc) * W * Cin * 2;
  const int xo0 = w.xs + 8 * g, xi0 = xo0 * S - 1;
  const unsigned pg = (unsigned)Cout * 2u, px = (unsigned)Cin * 2u;              // bytes per pixel
  // 32-bit lane offsets from the uniform row bases: an inner step adds constants, any other step clamps first
  unsigned oa[8], ob[NC];
  if (w.inner(H, W, ky)) {
    const unsigned og = (unsigned)xo0 * pg + lg, ox = (unsigned)xi0 * px + lx;
#pragma unroll
    for (int j = 0; j < 8; ++j) oa[j] = og + (unsigned)j * pg;
#pragma unroll
    for (int c = 0; c < NC; ++c) ob[c] = ox + (unsigned)c * px;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int xo = xo0 + j;
      oa[j] = (unsigned)(xo < Wo ? xo : Wo - 1) * pg + lg;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int xi = xi0 + c;
      ob[c] = (unsigned)(xi < 0 ? 0 : xi < W ? xi : W - 1) * px + lx;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) q.a[j] = *reinterpret_cast<const unsigned*>(gb + oa[j]);
#pragma unroll
  for (int c = 0; c < NC; ++c) q.b[c] = *reinterpret_cast<const unsigned*>(xb + ob[c]);
}

// Consume the step that was requested at walk position `w`.  acc[kx][2 * t + u]: t = parity of the output channel, u = parity
// of the input channel.
template <int S>
__device__ __forceinline__ void c3_step(const C3Walk<S>& w, C3Regs<S>& q, int H, int W, int Wo, int ky, int g,
                                        f32x16 (&acc)[3][4]) {
  unsigned t[3][8];                                    // tap kx of pixel j
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int j = 0; j < 8; ++j) t[kx][j] = q.b[S * j + kx];
  if (!w.inner(H, W, ky)) {                            // wave-uniform: the first and last step of a row, and a skipped row
    const bool row = w.ok(H, ky);
    const int xo0 = w.xs + 8 * g, xi0 = xo0 * S - 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool pix = row && xo0 + j < Wo;            // a pixel past the row's end takes no tap, whatever column it would read
      q.a[j] = pix ? q.a[j] : 0u;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) t[kx][j] = pix && (unsigned)(xi0 + S * j + kx) < (unsigned)W ? t[kx][j] : 0u;
    }
  }
  bf16x8 a0, a1;
  cw_frag(q.a, a0, a1);
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    bf16x8 b0, b1;
    cw_frag(t[kx], b0, b1);
    acc[kx][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[kx][0], 0, 0, 0);
    acc[kx][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[kx][1], 0, 0, 0);
    acc[kx][2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[kx][2], 0, 0, 0);
    acc[kx][3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[kx][3], 0, 0, 0);
  }
}

constexpr int C3_DEPTH = 4;      // register buffers of a wave

// grid (tiles_o * tiles_i, chunks, 3 = ky); block = 4 waves as 2 x 2 over a 128 (o) x 128 (i) tile
template <int S>
__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_kernel(const unsigned short* __restrict__ gy,
                                                               const unsigned short* __restrict__ x,
                                                               float* __restrict__ part, int R, int H, int W, int Ho, int Wo,
                                                               int Cin, int Cout, int tiles_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, g = lane >> 5;
  const int tile_o = blockIdx.x / tiles_i, tile_i = blockIdx.x - tile_o * tiles_i;
  const int c = blockIdx.y, chunks = gridDim.y, ky = blockIdx.z;
  const int o0 = tile_o * 128 + (wave >> 1) * 64, i0 = tile_i * 128 + (wave & 1) * 64;

  // this lane's channel pair; pairs beyond Cout / Cin are clamped for the load and dropped at the store
  const int og = o0 + 2 * col, ig = i0 + 2 * col;
  const unsigned lg = (unsigned)(og < Cout ? og : Cout - 2) * 2u, lx = (unsigned)(ig < Cin ? ig : Cin - 2) * 2u;
  const char* gp = reinterpret_cast<const char*>(gy);
  const char* xp = reinterpret_cast<const char*>(x);

  f32x16 acc[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[k][t][r] = 0.f;

  const int r_begin = (int)((long)c * R / chunks), r_end = (int)((long)(c + 1) * R / chunks);
  const int T = (r_end - r_begin) * ((Wo + 15) / 16);          // steps of this block (>= 1: a range is never empty)
  C3Walk<S> wa;                                        // the next step to request
  wa.r = r_begin;
  wa.n = r_begin / Ho;
  wa.yo = r_begin - wa.n * Ho;
  wa.xs = 0;

  // D register buffers, D steps per iteration: buffer k holds step t + k, and the loads of step t + k + D - 1 are requested
  // before step t + k is consumed (D - 1 steps of loads in flight across the MFMAs: one wave per SIMD hides latency in depth).
  // No load sits under a branch: the s_waitcnt counts are exact only when every path issues the same loads.
  constexpr int D = C3_DEPTH;
  C3Regs<S> q[D];
  C3Walk<S> wq[D];                                     // where each buffer's step was requested
#pragma unroll
  for (int k = 0; k < D - 1; ++k) {
    wq[k] = wa;
    c3_load<S>(wa, gp, xp, H, W, Wo, ky, Cin, Cout, lg, lx, g, q[k]);
    wa.next(Ho, Wo, r_end);
  }
  int t = 0;
  for (; t + D <= T; t += D) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      wq[(k + D - 1) % D] = wa;
      c3_load<S>(wa, gp, xp, H, W, Wo, ky, Cin, Cout, lg, lx, g, q[(k + D - 1) % D]);
      wa.next(Ho, Wo, r_end);
      c3_step<S>(wq[k], q[k], H, W, Wo, ky, g, acc);
    }
  }
#pragma unroll
  for (int k = 0; k < D - 1; ++k)                      // the last T % D steps are already loaded
    if (t + k < T) c3_step<S>(wq[k], q[k], H, W, Wo, ky, g, acc);

  // partial tile: D[row][col] with row = 8 * (r / 4) + 4 * g + r % 4; fragment row a of parity t is channel o0 + 2 a + t,
  // fragment column `col` of parity u is channel i0 + 2 col + u: the (u = 0, u = 1) pair of a lane is one 8-byte store
  float* pw = part + (long)c * Cout * 9 * Cin + (long)ky * 3 * Cin;
  if (ig < Cin) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = o0 + 2 * (8 * (r >> 2) + 4 * g + (r & 3)) + t;
          if (o < Cout)
            *reinterpret_cast<float2*>(pw + ((long)o * 9 + kx) * Cin + ig) = make_float2(acc[kx][2 * t][r], acc[kx][2 * t + 1][r]);
        }
      }
    }
  }
}

struct C3WgradPlan {
  int Ho, Wo, R, tiles_o, tiles_i, chunks;
};

// false: no kernel for these arguments.  splits == 0: the launcher's choice; splits > 0: that many ranges (at most min(R, 4096),
// R = N * Ho output rows: a range is whole rows).  The ranges are balanced, range c = rows [c R / chunks, (c + 1) R / chunks).
// The workspace size and the launch both use the count computed here.
static bool c3_plan(int N, int H, int W, int Cin, int Cout, int stride, int splits, C3WgradPlan& pl) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || splits < 0) return false;
  if (Cin % 32 || Cout % 32 || Cin > 2048 || Cout > 2048 || (stride != 1 && stride != 2)) return false;
  if ((long)N * H * W >= (1L << 31) - 64) return false;      // row and pixel indices are ints
  if ((long)W * 2048 * 2 >= (1L << 31)) return false;         // byte offsets inside a row are 32-bit
  pl.Ho = (H - 1) / stride + 1;
  pl.Wo = (W - 1) / stride + 1;
  pl.R = N * pl.Ho;
  pl.tiles_o = (Cout + 127) / 128;
  pl.tiles_i = (Cin + 127) / 128;
  // one block per CU (one wave per SIMD): 256 blocks fill the chip once; every range costs one 9 x Cout x Cin partial
  // written and read back, so no more ranges than that
  long want = splits > 0 ? splits : 256 / (3 * pl.tiles_o * pl.tiles_i);
  if (want > 4096) want = 4096;
  if (want > pl.R) want = pl.R;
  if (want < 1) want = 1;
  pl.chunks = (int)want;
  return true;
}

}  // namespace occ

extern "C" int64_t occ_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride, int splits) {
  occ::C3WgradPlan pl;
  if (!occ::c3_plan(N, H, W, Cin, Cout, stride, splits, pl)) return 0;
  return (int64_t)pl.chunks * 9 * Cout * Cin * 4;
}

extern "C" int occ_conv3x3_wgrad_nhwc_bf16(const void* g, const void* x, void* dw, int dw_bf16, void* workspace, int N,
                                           int H, int W, int Cin, int Cout, int stride, int splits, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(g && x && dw && workspace, "conv3x3_wgrad: null pointer argument");
  OCC_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv3x3_wgrad: bad dimension (N=%d H=%d W=%d Cin=%d Cout=%d)",
                N, H, W, Cin, Cout);
  OCC_CHECK_ARG(splits >= 0, "conv3x3_wgrad: negative splits (%d)", splits);
  C3WgradPlan pl;
  if (!c3_plan(N, H, W, Cin, Cout, stride, splits, pl)) {
    set_error("conv3x3_wgrad: needs Cin %% 32 == 0, Cout %% 32 == 0, both <= 2048, stride 1 or 2 (Cin=%d Cout=%d stride=%d)",
              Cin, Cout, stride);
    return OCC_E_UNSUPPORTED;
  }
  OCC_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)x & 3) == 0 && ((uintptr_t)dw & 3) == 0 &&
                ((uintptr_t)workspace & 7) == 0,
                "conv3x3_wgrad: g / x / dw must be 4-byte aligned, the workspace 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned short* gp = reinterpret_cast<const unsigned short*>(g);
  const unsigned short* xp = reinterpret_cast<const unsigned short*>(x);
  float* part = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)(pl.tiles_o * pl.tiles_i), (unsigned)pl.chunks, 3);
  if (stride == 1)
    hipLaunchKernelGGL(conv3x3_wgrad_kernel<1>, grid, dim3(256), 0, st, gp, xp, part, pl.R, H, W, pl.Ho, pl.Wo, Cin, Cout,
                       pl.tiles_i);
  else
    hipLaunchKernelGGL(conv3x3_wgrad_kernel<2>, grid, dim3(256), 0, st, gp, xp, part, pl.R, H, W, pl.Ho, pl.Wo, Cin, Cout,
                       pl.tiles_i);
  OCC_CHECK_LAUNCH("conv3x3_wgrad");
  const hipError_t e = conv_wgrad_reduce_launch(part, dw, (long)Cout * 9 * Cin, pl.chunks, dw_bf16, st);
  if (e != hipSuccess) {
    set_error("conv3x3_wgrad_reduce: launch failed: %s", hipGetErrorString(e));
    return OCC_E_LAUNCH;
  }
  return OCC_OK;
}
