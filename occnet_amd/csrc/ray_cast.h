// The ray caster shared by the device-resident evaluation (ray_metrics_fused.hip), the submission writer (submission_rays.hip),
// the renderer (occ_render.hip) and the camera visibility masks (visibility.hip, which walks with rm_visit): class read,
// occupancy bit masks per pillar, the origin / end-point conversion of process_one_sample, the traversal set-up of
// csrc/dvr_render.hip and its "test"-phase walk over the masks.  One copy of the text: the files report the same voxel and the
// same distance for the same ray, bit for bit.  Below the kernels, the host side their entry points share: the workspace size,
// the grid-argument checks, the mask launch and the mask-type dispatch.
//
// Lane predicates that select a load address are kept as 0 / 1 integers (common.h: lane_flag) and every load inside the
// traversal is issued with a clamped, always-legal index; the traversal of a lane that is not cast runs zero steps.
#pragma once
#include <float.h>
#include "common.h"

namespace occ {

__device__ __forceinline__ int rm_class_at(const void* __restrict__ sem, int is_i64, long i) {
  if (!is_i64) return (int)static_cast<const unsigned char*>(sem)[i];
  const long long v = static_cast<const long long*>(sem)[i];
  return (v < -2147483647ll || v > 2147483647ll) ? -1 : (int)v;      // beyond int: occupied, counted in no class
}

// The occupancy bits of pillar p (cells p * Z .. p * Z + Z - 1): bit z set iff class(x, y, z) != free_id.
__device__ __forceinline__ unsigned rm_pillar_bits(const void* __restrict__ sem, int is_i64, long p, int Z, int free_id) {
  unsigned m = 0;
  for (int z = 0; z < Z; ++z) m |= (rm_class_at(sem, is_i64, p * Z + z) != free_id ? 1u : 0u) << z;
  return m;
}

// One thread per pillar of one grid: its occupancy bits.  grid 0 = prediction, 1 = ground truth
// (a launch with gridDim.y == 1 builds the prediction's masks only and never reads sem_gt).
template <typename MaskT>
__global__ __launch_bounds__(256) void ray_metrics_occupancy_kernel(
    const void* __restrict__ sem_pred, int pred_i64, const void* __restrict__ sem_gt, int gt_i64,
    MaskT* __restrict__ masks, long pillars, int Z, int free_id) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pillars) return;
  const int g = blockIdx.y;
  const void* sem = g ? sem_gt : sem_pred;
  const int is_i64 = g ? gt_i64 : pred_i64;
  masks[(long)g * pillars + p] = (MaskT)rm_pillar_bits(sem, is_i64, p, Z, free_id);
}

struct RmHit {
  float dist;       // ray parameter (voxel units) at which the ray leaves the reported voxel; -1: never entered the grid
  int x, y, z;
};

struct RmRay {      // per-ray constants of the traversal (dvr_render_forward_kernel's set-up)
  int vx, vy, vz, stepX, stepY, stepZ;
  double tMaxX, tMaxY, tMaxZ, tDeltaX, tDeltaY, tDeltaZ;
  double gt_d;      // |end - origin| (dvr_render_train.hip: the pre-entry stop, the depth target and the padded-ray rule)
};

#pragma clang fp contract(off)
__device__ __forceinline__ RmRay rm_ray_setup(float fxo, float fyo, float fzo, float fxe, float fye, float fze) {
#pragma clang fp contract(off)
  RmRay r;
  const double xo = fxo, yo = fyo, zo = fzo;
  const double xe = fxe, ye = fye, ze = fze;
  r.vx = (int)xo; r.vy = (int)yo; r.vz = (int)zo;
  const double rx = xe - xo, ry = ye - yo, rz = ze - zo;
  const double gt_d = sqrt(rx * rx + ry * ry + rz * rz);
  const double dx = rx / gt_d, dy = ry / gt_d, dz = rz / gt_d;
  r.stepX = (dx >= 0) ? 1 : -1; r.stepY = (dy >= 0) ? 1 : -1; r.stepZ = (dz >= 0) ? 1 : -1;
  const double bx = r.vx + (r.stepX < 0 ? 0 : 1), by = r.vy + (r.stepY < 0 ? 0 : 1), bz = r.vz + (r.stepZ < 0 ? 0 : 1);
  r.tMaxX = (dx != 0) ? (bx - xo) / dx : DBL_MAX;
  r.tMaxY = (dy != 0) ? (by - yo) / dy : DBL_MAX;
  r.tMaxZ = (dz != 0) ? (bz - zo) / dz : DBL_MAX;
  r.tDeltaX = (dx != 0) ? r.stepX / dx : DBL_MAX;
  r.tDeltaY = (dy != 0) ? r.stepY / dy : DBL_MAX;
  r.tDeltaZ = (dz != 0) ? r.stepZ / dz : DBL_MAX;
  r.gt_d = gt_d;
  return r;
}

// process_one_sample's conversion of a lidar origin o (ego metres) and a ray d to voxel units, then the set-up.  The arithmetic
// follows the origin's type as torch's promotion does there: float32 origins -> float32 end = ray + origin and
// (p - offset) / scaler in float32; float64 origins (what io.lidar_origins returns) -> the same statements in float64, rounded
// to float32 once.
__device__ __forceinline__ RmRay rm_ray_from_origin(float ox, float oy, float oz, float dx, float dy, float dz, float off_x,
                                                    float off_y, float off_z, float voxel_size) {
#pragma clang fp contract(off)
  const float ex = dx + ox, ey = dy + oy, ez = dz + oz;
  return rm_ray_setup((ox - off_x) / voxel_size, (oy - off_y) / voxel_size, (oz - off_z) / voxel_size,
                      (ex - off_x) / voxel_size, (ey - off_y) / voxel_size, (ez - off_z) / voxel_size);
}
__device__ __forceinline__ RmRay rm_ray_from_origin(double ox, double oy, double oz, float dx, float dy, float dz, float off_x,
                                                    float off_y, float off_z, float voxel_size) {
#pragma clang fp contract(off)
  const double ex = (double)dx + ox, ey = (double)dy + oy, ez = (double)dz + oz;
  const double fx = off_x, fy = off_y, fz = off_z, s = voxel_size;
  return rm_ray_setup((float)((ox - fx) / s), (float)((oy - fy) / s), (float)((oz - fz) / s),
                      (float)((ex - fx) / s), (float)((ey - fy) / s), (float)((ez - fz) / s));
}

// "test"-phase traversal over one grid's pillar masks (X * Y words, pillar (x, y) at x * Y + y).  live == 0: zero steps.
template <typename MaskT>
__device__ __forceinline__ RmHit rm_cast(const RmRay& r, const MaskT* __restrict__ masks, int X, int Y, int Z, int live) {
#pragma clang fp contract(off)
  int vx = r.vx, vy = r.vy, vz = r.vz;
  double tMaxX = r.tMaxX, tMaxY = r.tMaxY, tMaxZ = r.tMaxZ;
  int was_inside = 0;
  double last_d = 0.0;
  int lx = 0, ly = 0, lz = 0;
  const int last_step = live ? 1000 : -1;     // MAX_STEP = 1000: the reference runs steps 0..1000
  for (int step = 0; step <= last_step; ++step) {
    const int inside = lane_flag(0 <= vx) & lane_flag(vx < X) & lane_flag(0 <= vy) & lane_flag(vy < Y) &
                       lane_flag(0 <= vz) & lane_flag(vz < Z);
    if (!inside && was_inside) break;         // left the grid: never comes back
    const int cx = vx, cy = vy, cz = vz;
    double d;
    if (tMaxX < tMaxY) {
      if (tMaxX < tMaxZ) { d = tMaxX; vx += r.stepX; tMaxX += r.tDeltaX; }
      else { d = tMaxZ; vz += r.stepZ; tMaxZ += r.tDeltaZ; }
    } else {
      if (tMaxY < tMaxZ) { d = tMaxY; vy += r.stepY; tMaxY += r.tDeltaY; }
      else { d = tMaxZ; vz += r.stepZ; tMaxZ += r.tDeltaZ; }
    }
    const int pillar = inside ? cx * Y + cy : 0;                 // always a legal word
    const unsigned m = (unsigned)masks[pillar];
    if (inside) {
      was_inside = 1;
      last_d = d; lx = cx; ly = cy; lz = cz;
      if ((m >> cz) & 1u) break;              // first occupied voxel: nothing after it matters in the "test" phase
    }
  }
  RmHit h;
  h.dist = was_inside ? (float)last_d : -1.f;
  h.x = lx; h.y = ly; h.z = lz;
  return h;
}

// The visiting walk (visibility.hip): rm_cast's loop statement for statement — the same tMax comparison order, steps 0..1000, the
// same "left the grid" break — which MARKS every voxel the loop body runs for with `inside` true, the first occupied voxel (where
// the loop ends) included.  `vis` holds one uint32 word per pillar of this grid, bit z = voxel (x, y, z) visited.  A ray ORs the z
// bits it collects while it stays in one pillar into that word with one atomicOr when it leaves the pillar (rm_mark), and at the
// end of the walk.  OR is order-independent: the words do not depend on the order of the rays.  live == 0: zero steps, no store.
//
// rm_mark — the lanes of a wave that leave a pillar in the same step mostly leave the SAME pillar with the same bits (an 8 x 8
// pixel tile is a narrow bundle), so they are served in rounds: the first lane still waiting is the round's leader, it alone
// touches memory, and every lane of its pillar whose bits its own cover is done with it (the leader always retires itself, so the
// loop ends).  The leader skips the atomic when the word already shows its bits; that read may be served from the vector L1
// (wavefront scope).  `seen` may be stale only towards FEWER bits, which costs an atomic and never a mark: within the kernel bits
// are only ever set, and the acquire at the kernel's start keeps words of an earlier launch — set bits of a reused workspace, from
// before visibility_prepare_kernel cleared them — out of the L1.
// KEEP WAVE-UNIFORM: the `while` condition and the readlane index.  `todo` is a ballot and every marking lane stays in the loop to
// its end; a loop that lanes leave one by one (readfirstlane inside a divergent `while`) was compiled to a single pass and marked
// wrong voxels (EXPERIMENTS.md 8zc).
__device__ __forceinline__ void rm_mark(unsigned* vis, int held, unsigned bits) {
  if (!bits) return;
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __builtin_amdgcn_ballot_w64(true);              // the lanes that mark now
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lead = __builtin_amdgcn_readlane(held, leader);
    const unsigned lead_bits = (unsigned)__builtin_amdgcn_readlane((int)bits, leader);
    if (lane == leader) {
      const unsigned seen = __hip_atomic_load(vis + lead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      if ((seen & lead_bits) != lead_bits) atomicOr(vis + lead, lead_bits);
    }
    const int done = lane_flag(held == lead) & lane_flag((bits & ~lead_bits) == 0u);
    todo &= ~__builtin_amdgcn_ballot_w64(done != 0);
  }
}

template <typename MaskT>
__device__ __forceinline__ void rm_visit(const RmRay& r, const MaskT* __restrict__ masks, unsigned* vis, int X, int Y, int Z,
                                         int live) {
#pragma clang fp contract(off)
  int vx = r.vx, vy = r.vy, vz = r.vz;
  double tMaxX = r.tMaxX, tMaxY = r.tMaxY, tMaxZ = r.tMaxZ;
  int was_inside = 0;
  int held = 0;                               // the pillar whose bits are in `bits` (any legal word while bits == 0)
  unsigned bits = 0u;
  const int last_step = live ? 1000 : -1;
  for (int step = 0; step <= last_step; ++step) {
    const int inside = lane_flag(0 <= vx) & lane_flag(vx < X) & lane_flag(0 <= vy) & lane_flag(vy < Y) &
                       lane_flag(0 <= vz) & lane_flag(vz < Z);
    if (!inside && was_inside) break;
    const int cx = vx, cy = vy, cz = vz;
    if (tMaxX < tMaxY) {
      if (tMaxX < tMaxZ) { vx += r.stepX; tMaxX += r.tDeltaX; }
      else { vz += r.stepZ; tMaxZ += r.tDeltaZ; }
    } else {
      if (tMaxY < tMaxZ) { vy += r.stepY; tMaxY += r.tDeltaY; }
      else { vz += r.stepZ; tMaxZ += r.tDeltaZ; }
    }
    const int pillar = inside ? cx * Y + cy : 0;                 // always a legal word
    const unsigned m = (unsigned)masks[pillar];
    if (inside) {
      was_inside = 1;
      if (pillar != held) {
        rm_mark(vis, held, bits);
        held = pillar;
        bits = 0u;
      }
      bits |= 1u << cz;
      if ((m >> cz) & 1u) break;
    }
  }
  rm_mark(vis, held, bits);
}

// ---- host side: what every entry point over the pillar masks asks, checks and launches -----------------------------------------

// Bytes of the pillar masks of `grids` grids (1: prediction, 2: prediction + ground truth), rounded up to 256: uint16 words up to
// Z = 16, uint32 up to Z = 32.  0: no such masks (a non-positive dimension, or Z > 32).
inline int64_t pillar_mask_bytes(int B, int X, int Y, int Z, int grids) {
  if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || Z > 32) return 0;
  return ((int64_t)grids * B * X * Y * (Z <= 16 ? 2 : 4) + 255) / 256 * 256;
}

// The checks of the grid arguments; `what` names the entry point in the message.  sem_gt == nullptr: one grid.  Z > 32 answers
// OCC_E_UNSUPPORTED before any pointer is looked at: the workspace queries answer 0 bytes for it.
inline int check_grid_args(const char* what, const void* sem, int sem_dtype, const void* sem_gt, int sem_gt_dtype, int free_id,
                           const void* workspace, int64_t workspace_bytes, int B, int max_B, int X, int Y, int Z) {
  if (Z > 32) {
    set_error("%s: Z = %d has no pillar bit mask (Z <= 32)", what, Z);
    return OCC_E_UNSUPPORTED;
  }
  OCC_CHECK_ARG(sem, "%s: null pointer argument (sem)", what);
  OCC_CHECK_ARG(workspace, "%s: null pointer argument (workspace)", what);
  OCC_CHECK_ARG(B > 0 && B <= max_B && X > 0 && Y > 0 && Z > 0, "%s: bad dimension (B=%d X=%d Y=%d Z=%d)", what, B, X, Y, Z);
  OCC_CHECK_ARG((int64_t)X * Y * Z <= (int64_t)1 << 30, "%s: grid %dx%dx%d too large", what, X, Y, Z);
  OCC_CHECK_ARG(sem_dtype == 0 || sem_dtype == 1, "%s: class dtype code must be 0 (uint8) or 1 (int64), got sem_dtype = %d", what,
                sem_dtype);
  OCC_CHECK_ARG(!sem_gt || sem_gt_dtype == 0 || sem_gt_dtype == 1,
                "%s: class dtype code must be 0 (uint8) or 1 (int64), got sem_gt_dtype = %d", what, sem_gt_dtype);
  OCC_CHECK_ARG(free_id >= 1 && free_id <= 31, "%s: free_id must be 1..31 (got %d)", what, free_id);
  const int64_t need = pillar_mask_bytes(B, X, Y, Z, sem_gt ? 2 : 1);
  OCC_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%lld < %lld bytes)", what, (long long)workspace_bytes,
                (long long)need);
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "%s: workspace must be 4-byte aligned", what);
  return OCC_OK;
}

// f(MaskT{}) with the mask word that holds Z bits
template <typename F>
inline void with_mask_type(int Z, F&& f) {
  if (Z <= 16) f(uint16_t{}); else f(uint32_t{});
}

// The masks of the prediction, and with sem_gt of the ground truth behind them (gridDim.y == 1 never reads sem_gt).
template <typename MaskT>
inline void launch_pillar_masks(hipStream_t stream, const void* sem, int dt, const void* sem_gt, int gt_dt, MaskT* masks, int B,
                                int X, int Y, int Z, int free_id) {
  const long pillars = (long)B * X * Y;
  hipLaunchKernelGGL(ray_metrics_occupancy_kernel<MaskT>, dim3((unsigned)((pillars + 255) / 256), sem_gt ? 2 : 1), dim3(256), 0,
                     stream, sem, dt, sem_gt, gt_dt, masks, pillars, Z, free_id);
}

}  // namespace occ
