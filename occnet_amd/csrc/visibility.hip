// Camera visibility masks — the voxels seen by the cameras — and confusion counts over the voxels a mask admits.  The fourth
// client of ray_cast.h: a camera is the bundle of pixel rays occ_render.hip casts; here every voxel a ray passes through before
// it is stopped is marked, instead of the one voxel it stops in being reported.
//
// DEFINITION.
// For sample `b`, view `v` and pixel `(i, j)` of an `h × w` raster, the ray is the ray of `occ_render_views_kernel`:
// - the same float32 statements in the same order,
// - `px = j + 0.5f`, `py = i + 0.5f`,
// - `dir = (D·(px,py)) + D[:,2]`, `ray = dir * far`,
// - the float32 overload of `rm_ray_from_origin`,
// - `#pragma clang fp contract(off)`.
//
// The walk is `rm_cast`'s loop statement for statement:
// - the same `tMax` comparison order,
// - steps `0..1000`,
// - the same "left the grid" break.
//
// A voxel is **visited** by a ray if the loop body runs for it with `inside` true. This includes the first occupied voxel, where
// the loop ends. Occupied means `class != free_id`, exactly as the pillar masks define it. Ids beyond `int` count as occupied.
//
// `mask[b,x,y,z] = 1` iff at least one ray of at least one view of sample `b` visits the voxel, else 0.
//
// Consequences to keep:
// - A ray that never enters the grid marks nothing.
// - A camera inside an occupied voxel marks only that voxel.
// - `far` only scales the direction, as in the renderer. The walk is not cut at `far`.
//
// LAUNCHES, all on the caller's stream, no host synchronisation.  The workspace holds the pillar occupancy masks (uint16 words up
// to Z = 16, uint32 up to Z = 32: ray_cast.h) and behind them one uint32 VISIBILITY word per pillar, bit z = voxel (x, y, z) seen.
//   1  visibility_prepare_kernel   one thread per pillar: its occupancy bits, and its visibility word cleared — a caller's reused
//                                  workspace needs no clearing
//   2  visibility_views_kernel     one thread per pixel, a wave an 8 x 8 pixel tile, a block four tiles side by side, grid
//                                  (ceil(w / 32), ceil(h / 8), B * V) as occ_render_views_kernel; rm_visit (ray_cast.h) ORs the z
//                                  bits a ray collects while it stays in one pillar into that pillar's word with one atomicOr —
//                                  an ordinary vector global atomic; OR is order-independent, so the words are deterministic.
//                                  Lanes of a wave that leave the same pillar in the same step share the atomic, and it is
//                                  skipped where the word already shows the bits (rm_mark; measurements: DESIGN.md 11d)
//   3  visibility_expand_kernel    one thread per pillar: the word -> Z bytes of `mask`, every byte written
// A pixel outside the raster is a dead lane: zero steps, clamped legal load addresses, no store.  Predicates that select a load
// address are 0 / 1 integers (common.h: lane_flag).
//
// CONFUSION COUNTS — state of (ncls + 1) * ncls int64 words, ncls = free_id + 1: row g, column p counts the admitted voxels whose
// ground truth is class g and whose prediction is class p; the last row holds [skipped, admitted, unused ...] (the layout is
// written out in include/occnet_amd_visibility.h).  Grid-stride over the voxels, 256 per step with a block-uniform bound; each
// block keeps an int32 histogram of the ncls * ncls <= 1024 cells in LDS (a block sees at most 2^40 / 2048 + 256 < 2^31 voxels),
// the two counters of the last row in registers, and flushes its non-zero counters once with 64-bit global integer atomic adds.
// Integer sums: exact, and the same whatever the number of blocks, calls, batches or ranks.
#include <limits.h>
#include "ray_cast.h"
#include "../../include/occnet_amd_visibility.h"

namespace occ {

struct VisArgs {
  const void* sem; const float* cams; const void* masks; unsigned* vis; unsigned char* mask;
  float off_x, off_y, off_z, voxel_size, far;
  int sem_i64, free_id, B, V, X, Y, Z, h, w;
};

template <typename MaskT>
__global__ __launch_bounds__(256) void visibility_prepare_kernel(const void* __restrict__ sem, int sem_i64,
                                                                 MaskT* __restrict__ masks, unsigned* __restrict__ vis,
                                                                 long pillars, int Z, int free_id) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pillars) return;
  masks[p] = (MaskT)rm_pillar_bits(sem, sem_i64, p, Z, free_id);
  vis[p] = 0u;
}

template <typename MaskT>
__global__ __launch_bounds__(256) void visibility_views_kernel(const VisArgs a) {
#pragma clang fp contract(off)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 32 + wave * 8 + (lane & 7);
  const int i = blockIdx.y * 8 + (lane >> 3);
  const int bv = blockIdx.z, b = bv / a.V;
  const int live = lane_flag(j < a.w) & lane_flag(i < a.h);
  const int jj = live ? j : 0, ii = live ? i : 0;
  const float* cam = a.cams + (long)bv * 12;
  const float px = (float)jj + 0.5f, py = (float)ii + 0.5f;
  const float rx = ((cam[3] * px + cam[4] * py) + cam[5]) * a.far;
  const float ry = ((cam[6] * px + cam[7] * py) + cam[8]) * a.far;
  const float rz = ((cam[9] * px + cam[10] * py) + cam[11]) * a.far;
  const RmRay rs = rm_ray_from_origin(cam[0], cam[1], cam[2], rx, ry, rz, a.off_x, a.off_y, a.off_z, a.voxel_size);
  const long pillars = (long)a.X * a.Y;
  rm_visit<MaskT>(rs, static_cast<const MaskT*>(a.masks) + b * pillars, a.vis + b * pillars, a.X, a.Y, a.Z, live);
}

// WORDS: Z % 4 == 0 and a 4-byte aligned mask -> four bytes per store
template <int WORDS>
__global__ __launch_bounds__(256) void visibility_expand_kernel(const unsigned* __restrict__ vis, unsigned char* __restrict__ mask,
                                                                long pillars, int Z) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pillars) return;
  const unsigned v = vis[p];
  if (WORDS) {
    unsigned* o = reinterpret_cast<unsigned*>(mask + p * Z);
    for (int z = 0; z < Z; z += 4) {
      const unsigned n = v >> z;
      o[z >> 2] = (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
    }
  } else {
    for (int z = 0; z < Z; ++z) mask[p * Z + z] = (unsigned char)((v >> z) & 1u);
  }
}

constexpr int kCfMaxCls = 32;            // ncls = free_id + 1 <= 32
constexpr int kCfMaxBlocks = 2048;
constexpr int kCfPerBlock = 4096;        // a block per this many voxels, up to kCfMaxBlocks

__device__ __forceinline__ int cf_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__global__ __launch_bounds__(256) void confusion_accumulate_kernel(const void* __restrict__ sem_pred, int pred_i64,
                                                                   const void* __restrict__ sem_gt, int gt_i64,
                                                                   const unsigned char* __restrict__ mask,
                                                                   unsigned long long* __restrict__ state, long n, int free_id) {
  __shared__ int hist[kCfMaxCls * kCfMaxCls];
  const int ncls = free_id + 1, cells = ncls * ncls;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  int n_admitted = 0, n_skipped = 0;
  for (long i0 = (long)blockIdx.x * 256; i0 < n; i0 += (long)gridDim.x * 256) {          // block-uniform bound
    const long i = i0 + threadIdx.x;
    const int live = lane_flag(i < n);
    const long at = live ? i : 0;                                                         // voxel 0: legal
    const int g = rm_class_at(sem_gt, gt_i64, at), p = rm_class_at(sem_pred, pred_i64, at);
    const int open = mask ? lane_flag(mask[at] != 0) : 1;
    const int kept = live & open;
    const int classed = lane_flag(g >= 0) & lane_flag(g < ncls) & lane_flag(p >= 0) & lane_flag(p < ncls);
    n_admitted += kept;
    n_skipped += kept & (classed ^ 1);
    if (kept & classed) atomicAdd(&hist[g * ncls + p], 1);
  }
  n_admitted = cf_wave_sum(n_admitted);
  n_skipped = cf_wave_sum(n_skipped);
  if ((threadIdx.x & 63) == 0) {
    if (n_skipped) atomicAdd(state + cells, (unsigned long long)n_skipped);
    if (n_admitted) atomicAdd(state + cells + 1, (unsigned long long)n_admitted);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const int v = hist[i];
    if (v) atomicAdd(state + i, (unsigned long long)v);
  }
}

static int64_t visibility_word_bytes(int B, int X, int Y) { return ((int64_t)B * X * Y * 4 + 255) / 256 * 256; }

}  // namespace occ

extern "C" int64_t occ_visibility_workspace_bytes(int B, int X, int Y, int Z) {
  const int64_t masks = occ::pillar_mask_bytes(B, X, Y, Z, 1);
  return masks ? masks + occ::visibility_word_bytes(B, X, Y) : 0;
}

extern "C" int occ_visibility_views(const void* sem, int sem_dtype, const float* cams, float off_x, float off_y, float off_z,
                                    float voxel_size, int free_id, float far, uint8_t* mask, void* workspace,
                                    int64_t workspace_bytes, int B, int V, int X, int Y, int Z, int h, int w, void* stream) {
  using namespace occ;
  const char* what = "visibility_views";
  const int rc = check_grid_args(what, sem, sem_dtype, nullptr, 0, free_id, workspace, workspace_bytes, B, INT_MAX, X, Y, Z);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_ARG((int64_t)B * X * Y <= (int64_t)1 << 30, "%s: grid %dx%dx%dx%d too large", what, B, X, Y, Z);
  OCC_CHECK_ARG(cams && mask, "%s: null pointer argument (cams, mask)", what);
  OCC_CHECK_ARG(V > 0 && h > 0 && w > 0 && (int64_t)B * V <= 65535 && h <= 16384 && w <= 16384,
                "%s: bad dimension (B=%d V=%d h=%d w=%d; B * V <= 65535, h, w in 1..16384)", what, B, V, h, w);
  OCC_CHECK_ARG(voxel_size > 0.f, "%s: voxel_size must be positive", what);
  OCC_CHECK_ARG(far > 0.f && far <= 3.0e38f, "%s: far must be positive and finite", what);
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(cams) % 4 == 0, "%s: cams must be 4-byte aligned", what);
  const int64_t need = occ_visibility_workspace_bytes(B, X, Y, Z);
  OCC_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%lld < %lld bytes)", what, (long long)workspace_bytes,
                (long long)need);
  const long pillars = (long)B * X * Y;
  unsigned* vis = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + pillar_mask_bytes(B, X, Y, Z, 1));
  VisArgs a{sem, cams, workspace, vis, mask, off_x, off_y, off_z, voxel_size, far, sem_dtype, free_id, B, V, X, Y, Z, h, w};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_pillar((unsigned)((pillars + 255) / 256));
  with_mask_type(Z, [&](auto m) {
    using MaskT = decltype(m);
    hipLaunchKernelGGL(visibility_prepare_kernel<MaskT>, per_pillar, dim3(256), 0, st, sem, sem_dtype,
                       static_cast<MaskT*>(workspace), vis, pillars, Z, free_id);
    hipLaunchKernelGGL(visibility_views_kernel<MaskT>, dim3((unsigned)((w + 31) / 32), (unsigned)((h + 7) / 8), (unsigned)(B * V)),
                       dim3(256), 0, st, a);
  });
  if (Z % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0)
    hipLaunchKernelGGL(visibility_expand_kernel<1>, per_pillar, dim3(256), 0, st, vis, mask, pillars, Z);
  else
    hipLaunchKernelGGL(visibility_expand_kernel<0>, per_pillar, dim3(256), 0, st, vis, mask, pillars, Z);
  OCC_CHECK_LAUNCH(what);
  return OCC_OK;
}

extern "C" int64_t occ_confusion_state_words(int free_id) {
  if (free_id < 1 || free_id >= occ::kCfMaxCls) return 0;
  return (int64_t)(free_id + 2) * (free_id + 1);
}

extern "C" int occ_confusion_accumulate(const void* sem_pred, int sem_pred_dtype, const void* sem_gt, int sem_gt_dtype,
                                        const uint8_t* mask, int free_id, int64_t* state, int64_t n_voxels, void* stream) {
  using namespace occ;
  const char* what = "confusion_accumulate";
  OCC_CHECK_ARG(sem_pred && sem_gt && state, "%s: null pointer argument (sem_pred, sem_gt, state)", what);
  OCC_CHECK_ARG((sem_pred_dtype == 0 || sem_pred_dtype == 1) && (sem_gt_dtype == 0 || sem_gt_dtype == 1),
                "%s: class dtype code must be 0 (uint8) or 1 (int64), got %d / %d", what, sem_pred_dtype, sem_gt_dtype);
  OCC_CHECK_ARG(free_id >= 1 && free_id < kCfMaxCls, "%s: free_id must be 1..%d (got %d)", what, kCfMaxCls - 1, free_id);
  OCC_CHECK_ARG(n_voxels > 0 && n_voxels <= (int64_t)1 << 40, "%s: bad dimension (n_voxels=%lld; 1 .. 2^40)", what,
                (long long)n_voxels);
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(state) % 8 == 0 && (sem_pred_dtype == 0 || reinterpret_cast<uintptr_t>(sem_pred) % 8 == 0) &&
                    (sem_gt_dtype == 0 || reinterpret_cast<uintptr_t>(sem_gt) % 8 == 0),
                "%s: state and int64 class grids must be 8-byte aligned", what);
  int64_t blocks = (n_voxels + kCfPerBlock - 1) / kCfPerBlock;
  if (blocks > kCfMaxBlocks) blocks = kCfMaxBlocks;
  hipLaunchKernelGGL(confusion_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     sem_pred, sem_pred_dtype, sem_gt, sem_gt_dtype, mask, reinterpret_cast<unsigned long long*>(state),
                     (long)n_voxels, free_id);
  OCC_CHECK_LAUNCH(what);
  return OCC_OK;
}
