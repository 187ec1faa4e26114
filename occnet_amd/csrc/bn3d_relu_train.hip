// Training-mode BatchNorm3d + ReLU of the voxel decoder on channels-last rows, and its backward (C = 32).
//
// The reference's decoder layer is ConvModule(Conv3d -> BatchNorm3d -> ReLU) (transformer_occ.py:106-126) under ATen autograd:
// a batch-statistics kernel, a normalise kernel, a ReLU, and in backward threshold_backward plus batch norm's two backward
// kernels (and, for the second layer, a permute copy each way).  Here, on the convolution's own (rows, 32) output y:
//   statistics : per-channel mean and biased variance by sums shifted by row 0 (S1 = sum(y - y0), S2 = sum((y - y0)^2): the
//                shift is a sample of the channel, so S2 / n - (S1 / n)^2 cancels digits of the spread only, never of the
//                offset), per-block partial sums in fp32, second stage in fp64; writes (mean | rstd) and updates the
//                running statistics;
//   forward    : out = max(0, pre),  pre = fma((y - mean) * rstd, gamma, beta), written through (batch, y, x) strides so the
//                second layer lands in the reference's (B, X, Y, Z, C) order without a permute copy;
//   backward   : dz = grad_out * [pre > 0] (the SAME pre: bn3d_pre below is the only place it is written down),
//                dbeta = sum dz, dgamma = sum dz * xhat, dy = gamma * rstd * (dz - dbeta / n - xhat * dgamma / n); dy leaves as
//                the contiguous tensor of the data-gradient convolution and / or as the zero-haloed (B, Y+2, X+2, Z+2, 32) tensor
//                of the weight-gradient kernel, every element of which this kernel writes.
// A row is 128 bytes = 8 lanes x float4; a thread keeps the same 4 channels for all its rows.  Column sums: registers ->
// shuffle over the wave's 8 rows -> LDS over the 4 waves -> one record of 32 x 2 sums per block -> second stage in a fixed
// order (no float atomics: every result is the same bits run to run).  All kernels stream; offsets are 64-bit.
#include "common.h"

namespace occ {

constexpr int kBn3dMaxBlocks = 1024;     // first-stage blocks = records of 64 partial sums
constexpr int kBn3dApplyBlocks = 2048;   // grid cap of the element-wise passes (8 blocks of 256 per CU)

// The pre-activation of one element.  Forward output and backward mask both come from THIS expression on the same operands.
__device__ __forceinline__ float bn3d_pre(float y, float mean, float rstd, float g, float b, float& xhat) {
  xhat = (y - mean) * rstd;
  return fmaf(xhat, g, b);
}

// max(0, pre) that keeps a NaN (torch.relu does; fmaxf would return 0)
__device__ __forceinline__ float bn3d_relu(float pre) { return pre <= 0.f ? 0.f : pre; }

struct Bn3dGeom {   // unpadded grid and the (batch, y, x) element strides of the strided tensor (z stride 32, channel stride 1)
  int Z, Y, X;
  long sb, sy, sx;
};

// row r of the (B, Y, X, Z) grid -> element offset of its first channel in the strided tensor
__device__ __forceinline__ long bn3d_row_offset(unsigned r, const Bn3dGeom& g) {
  const unsigned z = r % (unsigned)g.Z, t = r / (unsigned)g.Z;
  const unsigned x = t % (unsigned)g.X, u = t / (unsigned)g.X;
  const unsigned y = u % (unsigned)g.Y, b = u / (unsigned)g.Y;
  return (long)b * g.sb + (long)y * g.sy + (long)x * g.sx + (long)z * 32;
}

// a / b: this thread's two sums over its rows for channels 4 * (tid & 7) ... + 3.  -> partial[block][channel][a | b]
__device__ __forceinline__ void bn3d_block_partial(const float4& a, const float4& b, float* __restrict__ partial) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v[8] = {a.x, b.x, a.y, b.y, a.z, b.z, a.w, b.w};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int d = 8; d <= 32; d <<= 1) v[k] += __shfl_xor(v[k], d);      // the wave's 8 rows
  }
  if (lane < 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[wave][lane * 8 + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int t = threadIdx.x;
    partial[(long)blockIdx.x * 64 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  }
}

// Second stage, block j of 4: channels 8 j .. 8 j + 7.  16 columns x 16 record groups, fp64, fixed order.  Threads 0 .. 7
// return the two sums of channel 8 j + tid.
__device__ __forceinline__ void bn3d_colsum(const float* __restrict__ partial, int blocks, double& a, double& b) {
  __shared__ double red[16][16];
  const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  double s = 0.0;
  for (int k = grp; k < blocks; k += 16) s += (double)partial[(long)k * 64 + col];
  red[grp][cl] = s;
  __syncthreads();
  a = b = 0.0;
  if (threadIdx.x < 8) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      a += red[g][2 * threadIdx.x];
      b += red[g][2 * threadIdx.x + 1];
    }
  }
}

__global__ __launch_bounds__(256) void bn3d_stats_kernel(const float* __restrict__ y, float* __restrict__ partial, long rows) {
  const int cq = threadIdx.x & 7, rs = threadIdx.x >> 3;
  const float4 s = *reinterpret_cast<const float4*>(y + cq * 4);       // the shift: row 0
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  for (long r = (long)blockIdx.x * 32 + rs; r < rows; r += (long)gridDim.x * 32) {
    const float4 v = *reinterpret_cast<const float4*>(y + r * 32 + cq * 4);
    const float dx = v.x - s.x, dy = v.y - s.y, dz = v.z - s.z, dw = v.w - s.w;
    s1.x += dx; s1.y += dy; s1.z += dz; s1.w += dw;
    s2.x = fmaf(dx, dx, s2.x); s2.y = fmaf(dy, dy, s2.y); s2.z = fmaf(dz, dz, s2.z); s2.w = fmaf(dw, dw, s2.w);
  }
  bn3d_block_partial(s1, s2, partial);
}

__global__ __launch_bounds__(256) void bn3d_stats_final_kernel(const float* __restrict__ partial, int blocks,
                                                               const float* __restrict__ y, float* __restrict__ mean_rstd,
                                                               float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, float eaf, float eps,
                                                               long rows) {
  double s1, s2;
  bn3d_colsum(partial, blocks, s1, s2);
  if (threadIdx.x < 8) {
    const int c = blockIdx.x * 8 + threadIdx.x;
    const double n = (double)rows, d = s1 / n;
    const double mean = (double)y[c] + d;
    double var = s2 / n - d * d;
    var = var > 0.0 ? var : 0.0;
    mean_rstd[c] = (float)mean;
    mean_rstd[32 + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
      const double f = (double)eaf;
      running_mean[c] = (float)((1.0 - f) * (double)running_mean[c] + f * mean);
      running_var[c] = (float)((1.0 - f) * (double)running_var[c] + f * (var * n / (n - 1.0)));
    }
  }
}

__global__ __launch_bounds__(256) void bn3d_relu_apply_kernel(const float* __restrict__ y, const float* __restrict__ mean_rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ out, long rows, Bn3dGeom geom) {
  const int cq = threadIdx.x & 7, rs = threadIdx.x >> 3;
  const float4 m4 = *reinterpret_cast<const float4*>(mean_rstd + cq * 4);
  const float4 r4 = *reinterpret_cast<const float4*>(mean_rstd + 32 + cq * 4);
  const float4 g4 = *reinterpret_cast<const float4*>(gamma + cq * 4), b4 = *reinterpret_cast<const float4*>(beta + cq * 4);
  for (long r = (long)blockIdx.x * 32 + rs; r < rows; r += (long)gridDim.x * 32) {
    const float4 v = *reinterpret_cast<const float4*>(y + r * 32 + cq * 4);
    float h;
    const float4 o = make_float4(bn3d_relu(bn3d_pre(v.x, m4.x, r4.x, g4.x, b4.x, h)),
                                 bn3d_relu(bn3d_pre(v.y, m4.y, r4.y, g4.y, b4.y, h)),
                                 bn3d_relu(bn3d_pre(v.z, m4.z, r4.z, g4.z, b4.z, h)),
                                 bn3d_relu(bn3d_pre(v.w, m4.w, r4.w, g4.w, b4.w, h)));
    *reinterpret_cast<float4*>(out + bn3d_row_offset((unsigned)r, geom) + cq * 4) = o;
  }
}

// dz and xhat of one element
__device__ __forceinline__ float bn3d_dz(float go, float y, float mean, float rstd, float g, float b, float& xhat) {
  return bn3d_pre(y, mean, rstd, g, b, xhat) > 0.f ? go : 0.f;
}

__global__ __launch_bounds__(256) void bn3d_relu_bwd_reduce_kernel(const float* __restrict__ grad_out,
                                                                   const float* __restrict__ y,
                                                                   const float* __restrict__ mean_rstd,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ partial,
                                                                   long rows, Bn3dGeom geom) {
  const int cq = threadIdx.x & 7, rs = threadIdx.x >> 3;
  const float4 m4 = *reinterpret_cast<const float4*>(mean_rstd + cq * 4);
  const float4 r4 = *reinterpret_cast<const float4*>(mean_rstd + 32 + cq * 4);
  const float4 g4 = *reinterpret_cast<const float4*>(gamma + cq * 4), b4 = *reinterpret_cast<const float4*>(beta + cq * 4);
  float4 sd = make_float4(0.f, 0.f, 0.f, 0.f), sx = sd;
  for (long r = (long)blockIdx.x * 32 + rs; r < rows; r += (long)gridDim.x * 32) {
    const float4 v = *reinterpret_cast<const float4*>(y + r * 32 + cq * 4);
    const float4 go = *reinterpret_cast<const float4*>(grad_out + bn3d_row_offset((unsigned)r, geom) + cq * 4);
    float h;
    float d = bn3d_dz(go.x, v.x, m4.x, r4.x, g4.x, b4.x, h); sd.x += d; sx.x = fmaf(d, h, sx.x);
    d = bn3d_dz(go.y, v.y, m4.y, r4.y, g4.y, b4.y, h); sd.y += d; sx.y = fmaf(d, h, sx.y);
    d = bn3d_dz(go.z, v.z, m4.z, r4.z, g4.z, b4.z, h); sd.z += d; sx.z = fmaf(d, h, sx.z);
    d = bn3d_dz(go.w, v.w, m4.w, r4.w, g4.w, b4.w, h); sd.w += d; sx.w = fmaf(d, h, sx.w);
  }
  bn3d_block_partial(sd, sx, partial);
}

// -> grad_gamma_beta (2, 32): dgamma = sum dz * xhat | dbeta = sum dz
__global__ __launch_bounds__(256) void bn3d_relu_bwd_final_kernel(const float* __restrict__ partial, int blocks,
                                                                  float* __restrict__ grad_gamma_beta) {
  double sd, sx;
  bn3d_colsum(partial, blocks, sd, sx);
  if (threadIdx.x < 8) {
    const int c = blockIdx.x * 8 + threadIdx.x;
    grad_gamma_beta[c] = (float)sx;
    grad_gamma_beta[32 + c] = (float)sd;
  }
}

// PAD: the rows walked are those of the padded (B, Y+2, X+2, Z+2) grid; halo rows get zeros, interior rows their dy (and the
// same dy goes to grad_y when it is wanted).  !PAD: the rows of the unpadded grid, grad_y only.
template <bool PAD>
__global__ __launch_bounds__(256) void bn3d_relu_bwd_apply_kernel(const float* __restrict__ grad_out, const float* __restrict__ y,
                                                                  const float* __restrict__ mean_rstd,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ grad_gamma_beta,
                                                                  float* __restrict__ grad_y, float* __restrict__ grad_y_pad,
                                                                  long rows, long walk_rows, Bn3dGeom geom) {
  const int cq = threadIdx.x & 7, rs = threadIdx.x >> 3;
  const float4 m4 = *reinterpret_cast<const float4*>(mean_rstd + cq * 4);
  const float4 r4 = *reinterpret_cast<const float4*>(mean_rstd + 32 + cq * 4);
  const float4 g4 = *reinterpret_cast<const float4*>(gamma + cq * 4), b4 = *reinterpret_cast<const float4*>(beta + cq * 4);
  const float inv = 1.f / (float)rows;
  float4 c1 = *reinterpret_cast<const float4*>(grad_gamma_beta + 32 + cq * 4);      // sum dz / n
  float4 c2 = *reinterpret_cast<const float4*>(grad_gamma_beta + cq * 4);           // sum dz xhat / n
  c1.x *= inv; c1.y *= inv; c1.z *= inv; c1.w *= inv;
  c2.x *= inv; c2.y *= inv; c2.z *= inv; c2.w *= inv;
  const float4 k4 = make_float4(g4.x * r4.x, g4.y * r4.y, g4.z * r4.z, g4.w * r4.w);
  for (long p = (long)blockIdx.x * 32 + rs; p < walk_rows; p += (long)gridDim.x * 32) {
    long r = p;
    bool inside = true;
    if (PAD) {
      const unsigned Zp = (unsigned)geom.Z + 2, Xp = (unsigned)geom.X + 2, Yp = (unsigned)geom.Y + 2;
      const unsigned q = (unsigned)p;
      const unsigned z = q % Zp, t = q / Zp;
      const unsigned x = t % Xp, u = t / Xp;
      const unsigned yy = u % Yp, b = u / Yp;
      inside = z >= 1 && z <= (unsigned)geom.Z && x >= 1 && x <= (unsigned)geom.X && yy >= 1 && yy <= (unsigned)geom.Y;
      r = inside ? (((long)b * geom.Y + (yy - 1)) * geom.X + (x - 1)) * geom.Z + (z - 1) : 0;
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) {
      const float4 v = *reinterpret_cast<const float4*>(y + r * 32 + cq * 4);
      const float4 go = *reinterpret_cast<const float4*>(grad_out + bn3d_row_offset((unsigned)r, geom) + cq * 4);
      float h;
      float d = bn3d_dz(go.x, v.x, m4.x, r4.x, g4.x, b4.x, h); o.x = k4.x * fmaf(-h, c2.x, d - c1.x);
      d = bn3d_dz(go.y, v.y, m4.y, r4.y, g4.y, b4.y, h); o.y = k4.y * fmaf(-h, c2.y, d - c1.y);
      d = bn3d_dz(go.z, v.z, m4.z, r4.z, g4.z, b4.z, h); o.z = k4.z * fmaf(-h, c2.z, d - c1.z);
      d = bn3d_dz(go.w, v.w, m4.w, r4.w, g4.w, b4.w, h); o.w = k4.w * fmaf(-h, c2.w, d - c1.w);
      if (!PAD || grad_y) *reinterpret_cast<float4*>(grad_y + r * 32 + cq * 4) = o;
    }
    if (PAD) *reinterpret_cast<float4*>(grad_y_pad + p * 32 + cq * 4) = o;
  }
}

static int bn3d_blocks(long rows, int cap) {
  const long b = (rows + 31) / 32;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// rows of the grid, or 0 when the kernels do not cover it (C != 32, fewer than 2 rows, 2^31 elements or more — counted on the
// padded grid, the largest tensor any of the calls touches)
static long bn3d_grid_rows(int B, int Z, int Y, int X, int C) {
  if (C != 32 || B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  const long rows = (long)B * Y * X * Z;
  const __int128 padded = (__int128)B * (Y + 2L) * (X + 2L) * (Z + 2L) * 32;
  if (rows < 2 || padded >= ((__int128)1 << 31)) return 0;
  return rows;
}

}  // namespace occ

extern "C" int64_t occ_bn3d_relu_train_partial_floats(int64_t rows, int C) {
  if (C != 32 || rows < 2 || rows >= (1L << 31) / 32) return 0;
  return (int64_t)occ::bn3d_blocks(rows, occ::kBn3dMaxBlocks) * 64;
}

extern "C" int occ_bn3d_relu_train_stats_f32(const float* y, float* partial, float* mean_rstd, float* running_mean,
                                             float* running_var, float eaf, float eps, int64_t rows, int C, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(y && partial && mean_rstd, "bn3d_relu_train_stats: null pointer argument");
  OCC_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr),
                "bn3d_relu_train_stats: running_mean and running_var come together or not at all");
  OCC_CHECK_ARG(rows > 0 && eps >= 0.f, "bn3d_relu_train_stats: bad argument (rows=%ld eps=%g)", (long)rows, (double)eps);
  if (occ_bn3d_relu_train_partial_floats(rows, C) == 0) {
    set_error("bn3d_relu_train_stats: C=%d rows=%ld: the kernels cover C = 32, at least 2 rows and fewer than 2^31 elements", C,
              (long)rows);
    return OCC_E_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int blocks = bn3d_blocks(rows, kBn3dMaxBlocks);
  hipLaunchKernelGGL(bn3d_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, partial, (long)rows);
  OCC_CHECK_LAUNCH("bn3d_relu_train_stats");
  hipLaunchKernelGGL(bn3d_stats_final_kernel, dim3(4), dim3(256), 0, st, partial, blocks, y, mean_rstd, running_mean,
                     running_var, eaf, eps, (long)rows);
  OCC_CHECK_LAUNCH("bn3d_relu_train_stats (finalise)");
  return OCC_OK;
}

extern "C" int occ_bn3d_relu_train_fwd_f32(const float* y, const float* mean_rstd, const float* gamma, const float* beta,
                                           float* out, int B, int Z, int Y, int X, int C, int64_t out_sb, int64_t out_sy,
                                           int64_t out_sx, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(y && mean_rstd && gamma && beta && out, "bn3d_relu_train_fwd: null pointer argument");
  OCC_CHECK_ARG(B > 0 && Z > 0 && Y > 0 && X > 0, "bn3d_relu_train_fwd: bad grid (B=%d Z=%d Y=%d X=%d)", B, Z, Y, X);
  const long rows = bn3d_grid_rows(B, Z, Y, X, C);
  if (rows == 0) {
    set_error("bn3d_relu_train_fwd: C=%d grid %dx%dx%dx%d: the kernels cover C = 32, at least 2 rows and fewer than 2^31 elements",
              C, B, Y, X, Z);
    return OCC_E_UNSUPPORTED;
  }
  const Bn3dGeom geom = {Z, Y, X, (long)out_sb, (long)out_sy, (long)out_sx};
  hipLaunchKernelGGL(bn3d_relu_apply_kernel, dim3((unsigned)bn3d_blocks(rows, kBn3dApplyBlocks)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), y, mean_rstd, gamma, beta, out, rows, geom);
  OCC_CHECK_LAUNCH("bn3d_relu_train_fwd");
  return OCC_OK;
}

extern "C" int occ_bn3d_relu_train_bwd_f32(const float* grad_out, int64_t go_sb, int64_t go_sy, int64_t go_sx, const float* y,
                                           const float* mean_rstd, const float* gamma, const float* beta, float* partial,
                                           float* grad_gamma_beta, float* grad_y, float* grad_y_pad, int B, int Z, int Y, int X,
                                           int C, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(grad_out && y && mean_rstd && gamma && beta && partial && grad_gamma_beta,
                "bn3d_relu_train_bwd: null pointer argument");
  OCC_CHECK_ARG(B > 0 && Z > 0 && Y > 0 && X > 0, "bn3d_relu_train_bwd: bad grid (B=%d Z=%d Y=%d X=%d)", B, Z, Y, X);
  const long rows = bn3d_grid_rows(B, Z, Y, X, C);
  if (rows == 0) {
    set_error("bn3d_relu_train_bwd: C=%d grid %dx%dx%dx%d: the kernels cover C = 32, at least 2 rows and fewer than 2^31 elements",
              C, B, Y, X, Z);
    return OCC_E_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Bn3dGeom geom = {Z, Y, X, (long)go_sb, (long)go_sy, (long)go_sx};
  const int blocks = bn3d_blocks(rows, kBn3dMaxBlocks);
  hipLaunchKernelGGL(bn3d_relu_bwd_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, grad_out, y, mean_rstd, gamma, beta,
                     partial, rows, geom);
  OCC_CHECK_LAUNCH("bn3d_relu_train_bwd (reduce)");
  hipLaunchKernelGGL(bn3d_relu_bwd_final_kernel, dim3(4), dim3(256), 0, st, partial, blocks, grad_gamma_beta);
  OCC_CHECK_LAUNCH("bn3d_relu_train_bwd (second stage)");
  if (grad_y_pad) {
    const long walk = (long)B * (Y + 2L) * (X + 2L) * (Z + 2L);
    hipLaunchKernelGGL(bn3d_relu_bwd_apply_kernel<true>, dim3((unsigned)bn3d_blocks(walk, kBn3dApplyBlocks)), dim3(256), 0, st,
                       grad_out, y, mean_rstd, gamma, beta, grad_gamma_beta, grad_y, grad_y_pad, rows, walk, geom);
    OCC_CHECK_LAUNCH("bn3d_relu_train_bwd (apply, padded)");
  } else if (grad_y) {
    hipLaunchKernelGGL(bn3d_relu_bwd_apply_kernel<false>, dim3((unsigned)bn3d_blocks(rows, kBn3dApplyBlocks)), dim3(256), 0, st,
                       grad_out, y, mean_rstd, gamma, beta, grad_gamma_beta, grad_y, grad_y_pad, rows, rows, geom);
    OCC_CHECK_LAUNCH("bn3d_relu_train_bwd (apply)");
  }
  return OCC_OK;
}
