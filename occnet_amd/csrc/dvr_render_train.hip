// Differentiable ray rendering through a density grid — gfx950 version of the reference's `dvr.render`
// (tools/ray_iou/lib/dvr/dvr.cu:391-703): per ray the expected depth, and the gradient of an L1 / L2 / abs-rel depth loss with
// respect to every voxel the ray crossed, summed over the rays.  C ABI and the mathematics: include/occnet_amd_dvr.h;
// derivation and measurements: DESIGN.md §11e.
//
// The reference records the path and five doubles per step in per-thread arrays (int3 path[1446] + 5 x double[1446], about
// 75 KB of scratch per lane) and then runs three backward loops over them.  Those loops reduce to
//     d exp_d / d sigma_k = -delta_k * sum_{j=k}^{n-2} v_j,      v_j = T_j (d_{j+1} - d_j)
// so this kernel marches each ray TWICE with running scalars only: march 1 gives exp_d (in the reference's summation order:
// with sigma == 0 every p_i is 1 - 1 and exp_d == d_{n-1} exactly, which decides the sign of the L1 gradient of every ray that
// crosses only empty space), d_{n-1}, dl_dd and the sums of v_j; march 2 repeats the identical traversal (one function,
// render_march, so the two cannot drift apart) and issues one float atomic per voxel.  The last voxel's term is exactly 0 and
// gets no add.
//
// The suffix sum of voxel k is "total minus prefix", which cancels once the ray has gone opaque: behind a surface v_j falls by
// orders of magnitude and total - prefix keeps an absolute error of 1e-16 * total, far above the true 1e-20.  The v_j are
// therefore summed in kBins bins by the binary exponent of the transmittance (a factor 2^10 per bin, made monotone along the
// ray, so a bin is a contiguous piece of the path): the suffix of voxel k is tail[bin] minus the prefix INSIDE that bin, where
// tail[b] is the sum of the bins >= b, added up from the small end.  The cancellation is then confined to terms within 2^10
// of each other.  The bins live in registers (compile-time indices, selects): no scratch.
//
// The loop is the reference's (:508-579) statement for statement; it is NOT dvr_render_forward_kernel's: before the ray has
// entered the grid it also stops when last_d > gt_d.  Set-up: rm_ray_setup (ray_cast.h), uncontracted doubles.  Lane predicates
// that choose an address are 0 / 1 integers (common.h: lane_flag), every sigma load uses a clamped, always-legal index, and a
// lane that is not cast runs zero steps.
#include <float.h>
#include "../../include/occnet_amd_dvr.h"
#include "ray_cast.h"

namespace occ {

constexpr int kBins = 16;     // 2^-10 of transmittance each; the last one takes everything below 2^-150 (beyond float32)

struct RenderSums {     // what march 1 hands to march 2
  double exp_d;         // sum_i p_i d_i, ascending (the caller adds p_out * max_d)
  double max_d, p_out;  // d_{n-1}, T_{n-1}
  double bin[kBins];    // march 1: sum of v_j per bin; for march 2 turned into tails (render_tails)
  int count;            // in-grid voxels visited
};

// bin of a transmittance: (exponent below 1) / 10, clamped (T > 1 from a negative sigma: bin 0; 0 or denormal: the last)
__device__ __forceinline__ int render_bin(double T) {
  const int e = (int)((__double_as_longlong(T) >> 52) & 0x7ff);
  const int b = (1023 - e) / 10;
  return b < 0 ? 0 : b > kBins - 1 ? kBins - 1 : b;
}

__device__ __forceinline__ void render_tails(RenderSums& s) {
  double acc = 0.0;
#pragma unroll
  for (int i = kBins - 1; i >= 0; --i) { acc += s.bin[i]; s.bin[i] = acc; }
}

// One march.  ADD == false: the sums.  ADD == true: the same traversal, adding -dl_dd * delta_k * (suffix sum of v from k) to
// gsig for the voxels k < count - 1 (sums.bin holds the tails, sums.count the first march's count).  live == 0: zero steps.
template <bool ADD>
__device__ __forceinline__ RenderSums render_march(const RmRay& r, const float* __restrict__ grid, float* __restrict__ gsig, int X,
                                                   int Y, int Z, int live, double dl_dd, const RenderSums& sums) {
#pragma clang fp contract(off)
  int vx = r.vx, vy = r.vy, vz = r.vz;
  double tMaxX = r.tMaxX, tMaxY = r.tMaxY, tMaxZ = r.tMaxZ;
  int was_inside = 0, count = 0;
  double last_d = 0.0;
  double csd = 0.0, Tcur = 1.0;               // csd_{i-1}, T_{i-1} = exp(-csd_{i-1}); T_{-1} = exp(-0) = 1
  double dprev = 0.0;                         // d_{i-1}
  double exp_d = 0.0;
  int bcur = 0;                               // bin of voxel i - 1 (monotone: max over the path so far)
  int bheld = -1;                             // ADD: the bin `base` and `inbin` belong to
  double base = 0.0, inbin = 0.0;             // ADD: tail[bheld], and the sum of v_j of that bin before the current voxel
  RenderSums out;
#pragma unroll
  for (int i = 0; i < kBins; ++i) out.bin[i] = 0.0;
  const int last_add = sums.count - 1;        // ADD: voxels 0 .. count - 2 get a term
  const int last_step = live ? 1000 : -1;     // MAX_STEP = 1000: the reference runs steps 0..1000
  for (int step = 0; step <= last_step; ++step) {
    const int inside = lane_flag(0 <= vx) & lane_flag(vx < X) & lane_flag(0 <= vy) & lane_flag(vy < Y) &
                       lane_flag(0 <= vz) & lane_flag(vz < Z);
    if (!inside) {
      if (was_inside) break;                  // left the grid: never comes back
      if (last_d > r.gt_d) break;             // passed the end point before entering
    }
    const int cx = vx, cy = vy, cz = vz;
    double d;
    if (tMaxX < tMaxY) {
      if (tMaxX < tMaxZ) { d = tMaxX; vx += r.stepX; tMaxX += r.tDeltaX; }
      else { d = tMaxZ; vz += r.stepZ; tMaxZ += r.tDeltaZ; }
    } else {
      if (tMaxY < tMaxZ) { d = tMaxY; vy += r.stepY; tMaxY += r.tDeltaY; }
      else { d = tMaxZ; vz += r.stepZ; tMaxZ += r.tDeltaZ; }
    }
    const long cell = inside ? ((long)cz * Y + cy) * X + cx : 0;      // always a legal element
    const double sg = (double)grid[cell];
    if (inside) {
      was_inside = 1;
      const double delta = fmax(0.0, d - last_d);
      const double sd = sg * delta;
      const double csd_i = csd + sd;
      const double Ti = exp(-csd_i);
      const double v = count > 0 ? Tcur * (d - dprev) : 0.0;       // v_{i-1} = T_{i-1} (d_i - d_{i-1}), of bin bcur
      const int bnow = max(bcur, render_bin(Ti));
      if (!ADD) {
        exp_d += (Tcur - Ti) * d;
#pragma unroll
        for (int i = 0; i < kBins; ++i) out.bin[i] += (i == bcur) ? v : 0.0;
      } else {
        inbin += v;
        if (bnow != bheld) {                  // a new bin starts at this voxel: v_{i-1} was the last of the one before
          bheld = bnow;
          inbin = 0.0;
#pragma unroll
          for (int i = 0; i < kBins; ++i) base = (i == bnow) ? sums.bin[i] : base;
        }
        const double term = -dl_dd * delta * (base - inbin);
        if (count < last_add && term != 0.0) atomicAdd(gsig + cell, (float)term);
      }
      csd = csd_i; Tcur = Ti; dprev = d; bcur = bnow;
      ++count;
    }
    last_d = d;
  }
  out.exp_d = exp_d; out.max_d = dprev; out.p_out = Tcur; out.count = count;
  return out;
}

__global__ __launch_bounds__(256) void dvr_render_train_kernel(
    const float* __restrict__ sigma, const float* __restrict__ origin, const float* __restrict__ points,
    const float* __restrict__ tindex, float* __restrict__ pred_dist, float* __restrict__ gt_dist, float* __restrict__ grad_sigma,
    int T, int Z, int Y, int X, int M, int pstride, int loss_type) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int c0 = blockIdx.x * blockDim.x + threadIdx.x;
  const int in_range = lane_flag(c0 < M);
  const int c = in_range ? c0 : 0;
  const long oi = (long)n * M + c;
  const float tf = tindex[oi];
  const int timed = in_range & lane_flag(tf >= 0.f) & lane_flag(tf < (float)T);      // NaN fails both
  const int t = timed ? (int)tf : 0;
  const int ts = (T == 1) ? 0 : t;
  const float* o = origin + ((long)n * T + t) * 3;
  const float* e = points + oi * pstride;
  const float xo = o[0], yo = o[1], zo = o[2], xe = e[0], ye = e[1], ze = e[2];
  const float inf = __builtin_huge_valf();
  const int finite = lane_flag(fabsf(xo) < inf) & lane_flag(fabsf(yo) < inf) & lane_flag(fabsf(zo) < inf) &
                     lane_flag(fabsf(xe) < inf) & lane_flag(fabsf(ye) < inf) & lane_flag(fabsf(ze) < inf);
  const RmRay r = rm_ray_setup(xo, yo, zo, xe, ye, ze);
  const int live = timed & finite & lane_flag(r.gt_d > 0.0);        // zero length: 0 / 0 directions
  const long slice = ((long)n * T + ts) * Z * Y * X;
  const float* grid = sigma + slice;
  float* gsig = grad_sigma + slice;

  RenderSums none;
  none.count = 0;
  RenderSums s = render_march<false>(r, grid, gsig, X, Y, Z, live, 0.0, none);
  if (s.count == 0) return;                   // never entered (or not cast): outputs keep -1, nothing is added
  const double exp_d = s.exp_d + s.p_out * s.max_d;
  const double gt_d = r.gt_d < s.max_d ? r.gt_d : s.max_d;
  pred_dist[oi] = (float)exp_d;
  gt_dist[oi] = (float)gt_d;
  double dl_dd;
  if (loss_type == 0) dl_dd = (exp_d >= gt_d) ? 1.0 : -1.0;
  else if (loss_type == 1) dl_dd = exp_d - gt_d;
  else dl_dd = (exp_d >= gt_d) ? (1.0 / gt_d) : -(1.0 / gt_d);
  const int add = lane_flag(s.count > 1) & lane_flag(dl_dd != 0.0);
  render_tails(s);
  render_march<true>(r, grid, gsig, X, Y, Z, add, dl_dd, s);
}

__global__ void dvr_render_fill_kernel(float* __restrict__ a, float* __restrict__ b, float v, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { a[i] = v; b[i] = v; }
}

}  // namespace occ

extern "C" int occ_dvr_render_f32(const float* sigma, const float* origin, const float* points, const float* tindex,
                                  float* pred_dist, float* gt_dist, float* grad_sigma, int N, int T, int Z, int Y, int X, int M,
                                  int point_stride, int loss_type, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(sigma && origin && points && tindex && pred_dist && gt_dist && grad_sigma, "dvr_render: null pointer argument");
  OCC_CHECK_ARG(N > 0 && T > 0 && Z > 0 && Y > 0 && X > 0 && M > 0, "dvr_render: bad dimension (N=%d T=%d Z=%d Y=%d X=%d M=%d)", N,
                T, Z, Y, X, M);
  OCC_CHECK_ARG(N <= 65535, "dvr_render: N = %d exceeds 65535 (one grid row per batch entry)", N);
  OCC_CHECK_ARG(point_stride >= 3, "dvr_render: points need at least 3 coordinates per ray");
  OCC_CHECK_ARG(loss_type >= 0 && loss_type <= 2, "dvr_render: loss_type must be 0 (l1), 1 (l2) or 2 (absrel), got %d", loss_type);
  // N * T * Z * Y * X elements, indexed in int64: each partial product of five ints < 2^31 is checked against 2^62
  int64_t cells = 1;
  for (int64_t f : {(int64_t)N, (int64_t)T, (int64_t)Z, (int64_t)Y, (int64_t)X}) {
    OCC_CHECK_ARG(cells <= ((int64_t)1 << 62) / f, "dvr_render: sigma %dx%dx%dx%dx%d too large", N, T, Z, Y, X);
    cells *= f;
  }
  OCC_CHECK_ARG((int64_t)N * M <= ((int64_t)1 << 62) / point_stride, "dvr_render: points %dx%dx%d too large", N, M, point_stride);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long nm = (long)N * M;
  // reference host wrapper: pred / gt = -ones, grad_sigma = zeros (dvr.cu:664-666)
  if (hipMemsetAsync(grad_sigma, 0, (size_t)cells * sizeof(float), st) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dvr_render: clearing grad_sigma failed");
    return OCC_E_LAUNCH;
  }
  hipLaunchKernelGGL(dvr_render_fill_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, pred_dist, gt_dist, -1.f, nm);
  hipLaunchKernelGGL(dvr_render_train_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)N), dim3(256), 0, st, sigma, origin,
                     points, tindex, pred_dist, gt_dist, grad_sigma, T, Z, Y, X, M, point_stride, loss_type);
  OCC_CHECK_LAUNCH("dvr_render");
  return OCC_OK;
}
