// Device-resident submission rows: the per-ray class / depth / flow of a batch of predictions, cast and packed into the
// types of submission.gz (pcd_cls int8, pcd_dist float16, pcd_flow float16 x 2) in one launch pair.  Replaces, for the
// submission, the per-sample / per-origin host loop of io.format_submission -> metrics.process_one_sample (the mirror of the
// reference's projects/mmdet3d_plugin/datasets/nuscenes_occ.py:189-257), whose arithmetic it restates bit for bit:
//   * occupancy bit masks of the PREDICTION only (ray_cast.h: bit z of pillar (x, y) set iff class != free_id),
//   * origin / end point in voxel units and the "test"-phase traversal exactly as ray_metrics_cast_kernel (ray_cast.h: one
//     copy of the text); a ray that never enters the grid reports voxel (0, 0, 0) and depth -1 * voxel_size,
//   * depth = float32 distance * float32 voxel_size; class / flow read at the reported voxel,
//   * class -> int8: the low 8 bits of the id (ids 0..127 are what the host's astype(np.int8) defines; above that the C cast
//     behind it is undefined, here it is two's-complement wrap); depth and flow -> float16, round to nearest even, overflow to
//     inf (v_cvt_f16_f32: what numpy's astype(np.float16) computes).
//
// PACKED OUTPUT: one buffer of three sections, each starting on a 256-byte boundary.  N = B * Tmax * R rows, row
// (b * Tmax + t) * R + r (process_one_sample's order):
//   cls  int8[N]     at 0
//   dist fp16[N]     at align256(N)
//   flow fp16[N][2]  at align256(N) + align256(2 N)
// occ_submission_rays_bytes = align256(N) + align256(2 N) + align256(4 N).  Rows of origins beyond origin_counts[b] are not
// written.
#include "ray_cast.h"

namespace occ {

__host__ __device__ __forceinline__ int64_t sub_align256(int64_t v) { return (v + 255) / 256 * 256; }

// float32 -> float16 of a value that is ROUNDED TO float32 FIRST, as numpy converts the host path's float32 rows.  Without the
// empty asm hipcc folds `(_Float16)(dist * voxel_size)` into v_fma_mixlo_f16, which rounds the exact product once: a depth whose
// float32 value lies halfway between two float16 values then rounds by the product's discarded bits instead of to even.
__device__ __forceinline__ _Float16 f16_of_f32(float v) {
  asm volatile("" : "+v"(v));
  return (_Float16)v;
}

// Thread (b = blockIdx.z, t = blockIdx.y, r): ray r of origin t of sample b on the predicted grid.
template <typename MaskT, typename OriginT>
__global__ __launch_bounds__(256) void submission_rays_kernel(
    const void* __restrict__ sem_pred, int pred_i64, const float* __restrict__ flow_pred,
    const OriginT* __restrict__ origins, const int* __restrict__ origin_counts, const float* __restrict__ rays,
    const MaskT* __restrict__ masks, signed char* __restrict__ out_cls, _Float16* __restrict__ out_dist,
    _Float16* __restrict__ out_flow, float off_x, float off_y, float off_z, float voxel_size,
    int Tmax, int X, int Y, int Z, int R) {
#pragma clang fp contract(off)
  const int b = blockIdx.z, t = blockIdx.y;
  if (origin_counts && t >= origin_counts[b]) return;          // block-uniform: sample b has fewer origins
  const int ray = blockIdx.x * blockDim.x + threadIdx.x;
  const int live = lane_flag(ray < R);
  const int rr = live ? ray : 0;
  const OriginT* o = origins + ((long)b * Tmax + t) * 3;
  const OriginT ox = o[0], oy = o[1], oz = o[2];
  const float dx = rays[rr * 3 + 0], dy = rays[rr * 3 + 1], dz = rays[rr * 3 + 2];
  const RmRay rs = rm_ray_from_origin(ox, oy, oz, dx, dy, dz, off_x, off_y, off_z, voxel_size);
  const RmHit h = rm_cast<MaskT>(rs, masks + (long)b * X * Y, X, Y, Z, live);
  const long i = (long)b * X * Y * Z + ((long)h.x * Y + h.y) * Z + h.z;   // (0, 0, 0) for a ray that never entered: legal
  // low 8 bits of the class id (little endian: the first byte of an int64)
  const signed char c = static_cast<const signed char*>(sem_pred)[pred_i64 ? i * 8 : i];
  const float2 f = *reinterpret_cast<const float2*>(flow_pred + i * 2);
  const float d = h.dist * voxel_size;
  if (live) {
    typedef _Float16 occ_f16x2 __attribute__((ext_vector_type(2)));
    const long row = ((long)b * Tmax + t) * R + ray;
    out_cls[row] = c;
    out_dist[row] = f16_of_f32(d);
    const occ_f16x2 fh = {f16_of_f32(f.x), f16_of_f32(f.y)};
    *reinterpret_cast<occ_f16x2*>(out_flow + row * 2) = fh;
  }
}

}  // namespace occ

extern "C" int64_t occ_submission_rays_bytes(int B, int Tmax, int R) {
  if (B <= 0 || Tmax <= 0 || R <= 0) return 0;
  const int64_t n = (int64_t)B * Tmax * R;
  return occ::sub_align256(n) + occ::sub_align256(2 * n) + occ::sub_align256(4 * n);
}

extern "C" int64_t occ_submission_rays_workspace_bytes(int B, int X, int Y, int Z) {
  return occ::pillar_mask_bytes(B, X, Y, Z, 1);
}

extern "C" int occ_submission_rays(const void* sem_pred, int sem_pred_dtype, const float* flow_pred, const void* origins,
                                   int origins_dtype, const int32_t* origin_counts, const float* rays, float off_x,
                                   float off_y, float off_z, float voxel_size, int free_id, void* out, int64_t out_bytes,
                                   void* workspace, int64_t workspace_bytes, int B, int Tmax, int X, int Y, int Z, int R,
                                   void* stream) {
  using namespace occ;
  const int rc = check_grid_args("submission_rays", sem_pred, sem_pred_dtype, nullptr, 0, free_id, workspace, workspace_bytes, B,
                                 65535, X, Y, Z);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_ARG(flow_pred && origins && rays && out, "submission_rays: null pointer argument");
  OCC_CHECK_ARG(R > 0 && R <= (1 << 24), "submission_rays: bad dimension (R=%d)", R);
  OCC_CHECK_ARG(Tmax >= 1 && Tmax <= 8, "submission_rays: origins per sample must be 1..8 (Tmax=%d)", Tmax);
  OCC_CHECK_ARG(origins_dtype == 0 || origins_dtype == 1,
                "submission_rays: origins dtype code must be 0 (float32) or 1 (float64), got %d", origins_dtype);
  OCC_CHECK_ARG(voxel_size > 0.f, "submission_rays: voxel_size must be positive");
  OCC_CHECK_ARG(out_bytes >= occ_submission_rays_bytes(B, Tmax, R), "submission_rays: output too small (%lld < %lld bytes)",
                (long long)out_bytes, (long long)occ_submission_rays_bytes(B, Tmax, R));
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 4 == 0, "submission_rays: out must be 4-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned char* o = static_cast<unsigned char*>(out);
  const int64_t n = (int64_t)B * Tmax * R;
  signed char* cls = reinterpret_cast<signed char*>(o);
  _Float16* dist = reinterpret_cast<_Float16*>(o + sub_align256(n));
  _Float16* flow = reinterpret_cast<_Float16*>(o + sub_align256(n) + sub_align256(2 * n));
  const dim3 grid((unsigned)((R + 255) / 256), (unsigned)Tmax, (unsigned)B);
  with_mask_type(Z, [&](auto m) {
    using MaskT = decltype(m);
    MaskT* masks = static_cast<MaskT*>(workspace);
    launch_pillar_masks(st, sem_pred, sem_pred_dtype, nullptr, 0, masks, B, X, Y, Z, free_id);
    auto cast = [&](auto origin) {
      using OriginT = decltype(origin);
      hipLaunchKernelGGL((submission_rays_kernel<MaskT, OriginT>), grid, dim3(256), 0, st, sem_pred, sem_pred_dtype, flow_pred,
                         static_cast<const OriginT*>(origins), origin_counts, rays, masks, cls, dist, flow, off_x, off_y, off_z,
                         voxel_size, Tmax, X, Y, Z, R);
    };
    if (origins_dtype) cast(double{}); else cast(float{});
  });
  OCC_CHECK_LAUNCH("submission_rays");
  return OCC_OK;
}
