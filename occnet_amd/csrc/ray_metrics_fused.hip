// Device-resident RayIoU / mAVE evaluation: occupancy bit masks, the ray cast on the ground-truth AND the predicted grid, the
// non-free filter and the per-class scoring in one pass, accumulated into 64-bit integer counters that never leave the device.
// Replaces, for scoring, the per-sample / per-origin host loop of occnet_amd/metrics/ray_metrics.py (process_one_sample + main
// + calc_metrics — the mirror of the reference's projects/mmdet3d_plugin/datasets/ray_metrics.py:89-257), whose arithmetic it
// restates bit for bit:
//   * origin / end point in voxel units: float32 (p - offset) / voxel_size with end = ray + origin in float32 (:110-113),
//   * the traversal of csrc/dvr_render.hip, "test" phase (doubles on float inputs, contraction off, MAX_STEP 1000; a ray that
//     never enters the grid reports distance -1 and voxel (0, 0, 0)),
//   * depth = float32 distance * float32 voxel_size; label / flow read at the reported voxel,
//   * a ray is scored iff its ground-truth label is not free_id (main(): `valid`); for a scored ray calc_metrics' terms.
//
// STATE: (8 + 3 + 3) * ncls int64 words, ncls = free_id + 1, in this order (c = class, j = depth threshold 1 / 2 / 4 m):
//   gt_cnt[c] | pred_cnt[c] | tp_cnt[j][c] | ave_cnt[j][c] | ave_sum[j][c] | ave_bad[j][c]
// ave_sum is FIXED POINT: the float32 flow error of a true positive of a flow class (c < 8), rounded to the nearest multiple of
// the quantum 2^-28 m/s (exact for errors >= 2^-4, within quantum / 2 below) and added as an integer, so the sum does not
// depend on the order of arrival: two runs — and any split over batches or ranks — give bit-identical state.  Range: an int64
// holds sums below 2^63 * 2^-28 = 2^35 = 3.4e10 m/s.  A full validation set is 6 019 samples x 8 origins x 14 040 rays =
// 6.76e8 < 2^29.34 rays: even if every one of them were a true positive of ONE class, the sum fits while the MEAN flow error
// stays below 2^(35 - 29.34) = 50 m/s; a single error >= 2^34 m/s is treated like a non-finite one.  A non-finite (or
// >= 2^34) flow error never reaches the float-to-integer conversion: it still counts in ave_cnt but adds 1 to ave_bad[j][c]
// instead of to ave_sum, and RayMetrics.compute() reports that class's AVE as NaN (the reference yields NaN or inf there).
//
// Inside a block the contributions go to an LDS histogram of 64-bit words; afterwards one global 64-bit integer atomic per
// non-zero word per block.  No float atomics.
//
// Lane predicates that select a load address are kept as 0 / 1 integers (common.h: lane_flag) and every load inside the
// traversal is issued with a clamped, always-legal index; the traversal of a lane that is not scored runs zero steps.
//
// The class read, the occupancy kernel, the origin / end-point conversion, the traversal set-up and the walk live in ray_cast.h,
// shared as text with the submission writer (submission_rays.hip).
#include "ray_cast.h"

namespace occ {

constexpr int kRmMaxCls = 32;           // ncls = free_id + 1 <= 32
constexpr int kRmFlowCls = 8;           // classes 0..7 carry a flow error (flow_class_names)
constexpr int kRmWordsPerCls = 14;      // gt, pred, 3 tp, 3 ave_cnt, 3 ave_sum, 3 ave_bad
constexpr float kRmQuantumInv = 268435456.f;         // 2^28
constexpr float kRmErrLimit = 17179869184.f;         // 2^34

// Thread (b = blockIdx.z, t = blockIdx.y, r): ray r of origin t of sample b, on the ground truth and then the prediction.
template <typename MaskT>
__global__ __launch_bounds__(256) void ray_metrics_cast_kernel(
    const void* __restrict__ sem_pred, int pred_i64, const float* __restrict__ flow_pred,
    const void* __restrict__ sem_gt, int gt_i64, const float* __restrict__ flow_gt,
    const float* __restrict__ origins, const int* __restrict__ origin_counts, const float* __restrict__ rays,
    const MaskT* __restrict__ masks, unsigned long long* __restrict__ state, float* __restrict__ rows_pred,
    float* __restrict__ rows_gt, float off_x, float off_y, float off_z, float voxel_size, int free_id,
    int B, int Tmax, int X, int Y, int Z, int R) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hist[kRmMaxCls * kRmWordsPerCls];
  const int b = blockIdx.z, t = blockIdx.y;
  if (origin_counts && t >= origin_counts[b]) return;          // block-uniform: sample b has fewer origins
  const int ncls = free_id + 1;
  const int words = ncls * kRmWordsPerCls;
  for (int i = threadIdx.x; i < words; i += blockDim.x) hist[i] = 0ull;
  __syncthreads();

  const int ray = blockIdx.x * blockDim.x + threadIdx.x;
  const int live = lane_flag(ray < R);
  const int rr = live ? ray : 0;
  const float* o = origins + ((long)b * Tmax + t) * 3;
  const float ox = o[0], oy = o[1], oz = o[2];
  const float dx = rays[rr * 3 + 0], dy = rays[rr * 3 + 1], dz = rays[rr * 3 + 2];
  // process_one_sample: float32 end = ray + origin; (p - offset) / scaler in float32
  const RmRay rs = rm_ray_from_origin(ox, oy, oz, dx, dy, dz, off_x, off_y, off_z, voxel_size);
  const long pillars = (long)B * X * Y;
  const long vox0 = (long)b * X * Y * Z;
  const MaskT* mp = masks + (long)b * X * Y;
  const MaskT* mg = masks + pillars + (long)b * X * Y;

  const RmHit hg = rm_cast<MaskT>(rs, mg, X, Y, Z, live);
  const long ig = vox0 + ((long)hg.x * Y + hg.y) * Z + hg.z;    // (0, 0, 0) for a ray that never entered: legal
  const int lg = rm_class_at(sem_gt, gt_i64, ig);
  const float2 fg = *reinterpret_cast<const float2*>(flow_gt + ig * 2);
  const float dg = hg.dist * voxel_size;
  const int kept = live & lane_flag(lg != free_id);
  const int want_rows = rows_pred != nullptr;
  const int cast_pred = want_rows ? live : kept;

  const RmHit hp = rm_cast<MaskT>(rs, mp, X, Y, Z, cast_pred);
  const long ip = vox0 + ((long)hp.x * Y + hp.y) * Z + hp.z;    // (0, 0, 0) when the cast was skipped: legal
  const int lp = rm_class_at(sem_pred, pred_i64, ip);
  const float2 fp = *reinterpret_cast<const float2*>(flow_pred + ip * 2);
  const float dp = hp.dist * voxel_size;

  if (want_rows && live) {
    const long row = (((long)b * Tmax + t) * R + ray) * 4;
    *reinterpret_cast<float4*>(rows_gt + row) = make_float4((float)lg, dg, fg.x, fg.y);
    *reinterpret_cast<float4*>(rows_pred + row) = make_float4((float)lp, dp, fp.x, fp.y);
  }

  if (kept) {
    const int in_g = lg >= 0 && lg < ncls, in_p = lp >= 0 && lp < ncls;
    if (in_g) atomicAdd(&hist[lg], 1ull);
    if (in_p) atomicAdd(&hist[ncls + lp], 1ull);
    if (in_g && lp == lg) {
      const float l1 = fabsf(dp - dg);
      const float ux = fg.x - fp.x, uy = fg.y - fp.y;
      const float err = sqrtf(ux * ux + uy * uy);               // np.linalg.norm(axis=1) on float32, uncontracted
      const int bad = !(err < kRmErrLimit);                     // NaN, inf or beyond the fixed-point range
      const unsigned long long q = bad ? 0ull : (unsigned long long)(long long)rint((double)err * (double)kRmQuantumInv);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float thr = (float)(1 << j);
        if (l1 < thr) {
          atomicAdd(&hist[(2 + j) * ncls + lg], 1ull);
          if (lg < kRmFlowCls) {
            atomicAdd(&hist[(5 + j) * ncls + lg], 1ull);
            if (bad) atomicAdd(&hist[(11 + j) * ncls + lg], 1ull);
            else atomicAdd(&hist[(8 + j) * ncls + lg], q);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += blockDim.x) {
    const unsigned long long v = hist[i];
    if (v) atomicAdd(state + i, v);
  }
}

}  // namespace occ

extern "C" int64_t occ_ray_metrics_state_words(int free_id) {
  if (free_id < 1 || free_id >= occ::kRmMaxCls) return 0;
  return (int64_t)(free_id + 1) * occ::kRmWordsPerCls;
}

extern "C" int64_t occ_ray_metrics_workspace_bytes(int B, int X, int Y, int Z) { return occ::pillar_mask_bytes(B, X, Y, Z, 2); }

extern "C" int occ_ray_metrics_accumulate(const void* sem_pred, int sem_pred_dtype, const float* flow_pred,
                                          const void* sem_gt, int sem_gt_dtype, const float* flow_gt,
                                          const float* origins, const int32_t* origin_counts, const float* rays,
                                          float off_x, float off_y, float off_z, float voxel_size, int free_id,
                                          int64_t* state, float* rows_pred, float* rows_gt, void* workspace,
                                          int64_t workspace_bytes, int B, int Tmax, int X, int Y, int Z, int R,
                                          void* stream) {
  using namespace occ;
  const int rc = check_grid_args("ray_metrics_accumulate", sem_pred, sem_pred_dtype, sem_gt, sem_gt_dtype, free_id, workspace,
                                 workspace_bytes, B, 65535, X, Y, Z);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_ARG(flow_pred && sem_gt && flow_gt && origins && rays && state, "ray_metrics_accumulate: null pointer argument");
  OCC_CHECK_ARG((rows_pred == nullptr) == (rows_gt == nullptr),
                "ray_metrics_accumulate: rows_pred and rows_gt must be given together");
  OCC_CHECK_ARG(R > 0, "ray_metrics_accumulate: bad dimension (R=%d)", R);
  OCC_CHECK_ARG(Tmax >= 1 && Tmax <= 8, "ray_metrics_accumulate: origins per sample must be 1..8 (Tmax=%d)", Tmax);
  OCC_CHECK_ARG(voxel_size > 0.f, "ray_metrics_accumulate: voxel_size must be positive");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 cg((unsigned)((R + 255) / 256), (unsigned)Tmax, (unsigned)B);
  unsigned long long* s = reinterpret_cast<unsigned long long*>(state);
  with_mask_type(Z, [&](auto m) {
    using MaskT = decltype(m);
    MaskT* masks = static_cast<MaskT*>(workspace);
    launch_pillar_masks(st, sem_pred, sem_pred_dtype, sem_gt, sem_gt_dtype, masks, B, X, Y, Z, free_id);
    hipLaunchKernelGGL(ray_metrics_cast_kernel<MaskT>, cg, dim3(256), 0, st, sem_pred, sem_pred_dtype, flow_pred, sem_gt,
                       sem_gt_dtype, flow_gt, origins, origin_counts, rays, masks, s, rows_pred, rows_gt, off_x, off_y, off_z,
                       voxel_size, free_id, B, Tmax, X, Y, Z, R);
  });
  OCC_CHECK_LAUNCH("ray_metrics_accumulate");
  return OCC_OK;
}
