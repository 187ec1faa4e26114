// Device-resident score of submission rows as the challenge server computes it: the stand-alone scorer of the reference
// (tools/ray_iou/metric.py:calc_metrics, :31-73), restated over B samples of per-ray rows and accumulated into 64-bit integer
// counters that never leave the device.  It is NOT the scorer that ray_metrics_fused.hip mirrors (projects/mmdet3d_plugin/
// datasets/ray_metrics.py): metric.py reads the rows of the file (pcd_cls int8, pcd_dist float16, pcd_flow float16) and its AVE
// rule is different — once a flow class has ANY true positive in a sample at a threshold, it adds the flow error of EVERY valid
// ray of that sample, and the count of all those rays (metric.py:70-73: `flow_error` is not masked by `tp_mask`).
//
// ROWS, per side (prediction, ground truth), by a format code:
//   0  the packed sections of occ_submission_rays: cls int8[N], dist fp16[N], flow fp16[N][2] (three section pointers);
//      int8 -> int32 and fp16 -> float32 are exact, which is all metric.py's astype(np.int32 / np.float32) does to them;
//   1  float32 rows (N, 4) = [class, dist, flow_x, flow_y] (process_one_sample / RayMetrics.update(return_rays=True)); the class
//      is converted as astype(np.int32) does, truncating toward zero.  A class value that is not finite or does not fit an int32
//      counts as an OUT-OF-RANGE class (numpy leaves that conversion to the C cast, which yields INT_MIN on x86: the same effect).
// Sample b owns rows [b * stride, b * stride + counts[b]); counts[b] is clamped to 0 .. stride and rows beyond it are never read
// into the score.
//
// PER RAY (float32, contraction off): valid iff gt_cls != free_id; gt_cnt[c] / pred_cnt[c] over valid rays (a class outside
// [0, ncls) matches no class, the ray stays valid); l1 = |pred_dist - gt_dist|; tp[j][c] counts gt_cls == pred_cls == c and
// l1 < thr_j (1, 2, 4 m; l1 == thr is no hit, a NaN l1 neither); err = sqrtf(ux * ux + uy * uy) on the float32 flow differences
// (np.linalg.norm(axis=1)), for EVERY valid ray.
// PER SAMPLE: for each threshold j and flow class c < 8 with at least one true positive IN THAT SAMPLE, ave_sum[j][c] += the sum
// of err over all valid rays of the sample and ave_cnt[j][c] += their number.
//
// STATE: 17 * ncls int64 words, ncls = free_id + 1 <= 32, in this order (c = class, j = depth threshold):
//   gt_cnt[c] | pred_cnt[c] | tp[j][c] | ave_cnt[j][c] | ave_sum[j][c] | ave_inf[j][c] | ave_nan[j][c]
// ave_sum is FIXED POINT with the quantum 2^-28 m/s of ray_metrics_fused.hip: each float32 error is rounded to the nearest
// multiple of the quantum (exact for errors >= 2^-4, within quantum / 2 below) and added as an integer, so no sum depends on the
// order of arrival: two runs — and any split of the samples over calls, batches, ranks or blocks — give bit-identical state.
// Range: an int64 holds sums below 2^63 * 2^-28 = 2^35 = 3.4e10 m/s.  The sums here run over every VALID ray, not over the true
// positives only: a full validation set is 6 019 samples x 8 origins x 14 040 rays = 6.76e8 < 2^29.34 rays, and even if every
// one of them were valid and every sample had a true positive of the class, the sum fits while the MEAN flow error stays below
// 2^(35 - 29.34) = 50 m/s.  A single error >= 2^34 m/s is treated like an infinite one.  An error that is NaN adds 1 to
// ave_nan[j][c], one that is infinite (or >= 2^34) adds 1 to ave_inf[j][c], neither reaches the float-to-integer conversion or
// ave_sum; both still count in ave_cnt.  numpy's sum is NaN with any NaN term and inf with an infinite one otherwise (errors are
// never negative), which is what SubmissionScore.compute() reports from the two words.
//
// KERNEL FORM: the per-sample "any true positive" decision needs the whole sample before the sums are added.  The rows of a sample
// are split over up to 128 blocks (grid-stride over the sample, 256 rows per step): each block keeps an LDS histogram of 64-bit
// words (gt, pred, tp) and the sample terms (valid count, error sum, inf / nan counts) and STORES its record of 5 * ncls + 4 words
// into an uninitialised caller-provided workspace; a fold kernel, one block per sample, adds the records of the sample, takes the
// decision and adds to the state with one global 64-bit integer atomic per non-zero word.  No float atomics; integer sums, so the
// number of blocks does not show in the state.  (One block per sample — max_chunks = 1 — serialises the LDS atomics of 112 320
// rows on one compute unit: DESIGN.md 11b has the measurement.)
//
// Lane predicates that select a load address are kept as 0 / 1 integers (common.h: lane_flag); every load uses a clamped, always
// legal row index (row 0 of the sample for a lane beyond counts[b]).
#include "common.h"

namespace occ {

constexpr int kScMaxCls = 32;           // ncls = free_id + 1 <= 32
constexpr int kScFlowCls = 8;           // classes 0..7 carry a flow error (flow_class_names)
constexpr int kScWordsPerCls = 17;      // gt, pred, 3 tp, 3 ave_cnt, 3 ave_sum, 3 ave_inf, 3 ave_nan
constexpr int kScMaxChunks = 128;       // blocks per sample
constexpr int kScRowsPerChunk = 1024;   // a sample gets one block per this many rows of `stride`, up to kScMaxChunks
constexpr int kScRecWords = 5 * kScMaxCls + 4;       // record stride in the workspace: gt, pred, 3 tp rows + V, S, I, N
constexpr float kScQuantumInv = 268435456.f;         // 2^28
constexpr float kScErrLimit = 17179869184.f;         // 2^34

struct ScSide {          // format 0: cls / dist / flow sections; format 1: rows in `cls`
  const void* cls;
  const void* dist;
  const void* flow;
};

struct ScRow {
  int cls;
  float dist, fx, fy;
};

template <int FMT>
__device__ __forceinline__ ScRow sc_load(const ScSide& s, long row) {
  ScRow r;
  if (FMT == 0) {
    typedef _Float16 occ_f16x2 __attribute__((ext_vector_type(2)));
    r.cls = static_cast<const signed char*>(s.cls)[row];
    r.dist = (float)static_cast<const _Float16*>(s.dist)[row];
    const occ_f16x2 f = *reinterpret_cast<const occ_f16x2*>(static_cast<const _Float16*>(s.flow) + row * 2);
    r.fx = (float)f[0];
    r.fy = (float)f[1];
  } else {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(s.cls) + row * 4);
    // astype(np.int32): truncation toward zero; NaN, inf and values beyond int32 are no class at all
    const bool fits = v.x >= -2147483648.f && v.x < 2147483648.f;
    r.cls = fits ? (int)v.x : -1;
    r.dist = v.y;
    r.fx = v.z;
    r.fy = v.w;
  }
  return r;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Block (k = blockIdx.x, b = blockIdx.y): rows k * 256 + tid, + gridDim.x * 256, ... of sample b -> record (b, k).
template <int FP, int FG>
__global__ __launch_bounds__(256) void submission_score_rows_kernel(ScSide pred, ScSide gt, const int* __restrict__ counts,
                                                                    unsigned long long* __restrict__ records, long stride,
                                                                    int free_id) {
#pragma clang fp contract(off)
  __shared__ unsigned long long hist[kScRecWords];
  const int b = blockIdx.y, k = blockIdx.x, chunks = gridDim.x;
  const int ncls = free_id + 1;
  const int words = 5 * ncls + 4;
  for (int i = threadIdx.x; i < words; i += blockDim.x) hist[i] = 0ull;
  __syncthreads();

  long n = counts[b];
  n = n < 0 ? 0 : n > stride ? stride : n;
  const long base = (long)b * stride;
  unsigned long long sum_q = 0ull;
  int n_valid = 0, n_inf = 0, n_nan = 0;
  for (long i0 = (long)k * 256; i0 < n; i0 += (long)chunks * 256) {        // block-uniform bound
    const long i = i0 + threadIdx.x;
    const int live = lane_flag(i < n);
    const long row = base + (live ? i : 0);                                // row 0 of the sample: legal
    const ScRow p = sc_load<FP>(pred, row);
    const ScRow g = sc_load<FG>(gt, row);
    const int kept = live & lane_flag(g.cls != free_id);
    if (kept) {
      const int lg = g.cls, lp = p.cls;
      const int in_g = lg >= 0 && lg < ncls, in_p = lp >= 0 && lp < ncls;
      if (in_g) atomicAdd(&hist[lg], 1ull);
      if (in_p) atomicAdd(&hist[ncls + lp], 1ull);
      if (in_g && lp == lg) {
        const float l1 = fabsf(p.dist - g.dist);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (l1 < (float)(1 << j)) atomicAdd(&hist[(2 + j) * ncls + lg], 1ull);
      }
      const float ux = g.fx - p.fx, uy = g.fy - p.fy;
      const float err = sqrtf(ux * ux + uy * uy);                          // np.linalg.norm(axis=1) on float32, uncontracted
      const int is_nan = err != err;
      const int is_inf = !is_nan && !(err < kScErrLimit);                  // inf or beyond the fixed-point range
      n_valid += 1;
      n_nan += is_nan;
      n_inf += is_inf;
      if (!is_nan && !is_inf) sum_q += (unsigned long long)(long long)rint((double)err * (double)kScQuantumInv);
    }
  }
  // every lane of every wave arrives here: the loop bound is block-uniform
  sum_q = wave_sum_u64(sum_q);
  n_valid = wave_sum_i32(n_valid);
  n_inf = wave_sum_i32(n_inf);
  n_nan = wave_sum_i32(n_nan);
  if ((threadIdx.x & 63) == 0) {
    if (n_valid) atomicAdd(&hist[5 * ncls + 0], (unsigned long long)n_valid);
    if (sum_q) atomicAdd(&hist[5 * ncls + 1], sum_q);
    if (n_inf) atomicAdd(&hist[5 * ncls + 2], (unsigned long long)n_inf);
    if (n_nan) atomicAdd(&hist[5 * ncls + 3], (unsigned long long)n_nan);
  }
  __syncthreads();
  unsigned long long* rec = records + ((long)b * chunks + k) * kScRecWords;
  for (int i = threadIdx.x; i < words; i += blockDim.x) rec[i] = hist[i];  // the whole record, zeros included
}

// Block b: the records of sample b -> the sample's totals -> the state.
__global__ __launch_bounds__(256) void submission_score_fold_kernel(const unsigned long long* __restrict__ records,
                                                                    unsigned long long* __restrict__ state, int chunks,
                                                                    int free_id) {
  __shared__ unsigned long long tot[kScRecWords];
  const int b = blockIdx.x;
  const int ncls = free_id + 1;
  const int words = 5 * ncls + 4;
  const unsigned long long* rec = records + (long)b * chunks * kScRecWords;
  for (int i = threadIdx.x; i < words; i += blockDim.x) {
    unsigned long long v = 0ull;
    for (int k = 0; k < chunks; ++k) v += rec[(long)k * kScRecWords + i];
    tot[i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 5 * ncls; i += blockDim.x) {               // gt_cnt | pred_cnt | tp[3]: the state's first rows
    const unsigned long long v = tot[i];
    if (v) atomicAdd(state + i, v);
  }
  const int nflow = ncls < kScFlowCls ? ncls : kScFlowCls;
  for (int i = threadIdx.x; i < 3 * nflow; i += blockDim.x) {
    const int j = i / nflow, c = i - j * nflow;
    if (tot[(2 + j) * ncls + c]) {                                         // a true positive of class c in THIS sample
#pragma unroll
      for (int q = 0; q < 4; ++q) {                                        // ave_cnt, ave_sum, ave_inf, ave_nan
        const unsigned long long v = tot[5 * ncls + q];
        if (v) atomicAdd(state + (5 + 3 * q + j) * ncls + c, v);
      }
    }
  }
}

template <int FP, int FG>
static void score_launch(hipStream_t st, const ScSide& pred, const ScSide& gt, const int32_t* counts,
                         unsigned long long* records, int64_t stride, int free_id, int B, int chunks) {
  hipLaunchKernelGGL((submission_score_rows_kernel<FP, FG>), dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, st, pred, gt,
                     counts, records, (long)stride, free_id);
}

static bool side_aligned(int fmt, const void* cls, const void* dist, const void* flow) {
  if (fmt == 1) return reinterpret_cast<uintptr_t>(cls) % 16 == 0;
  return reinterpret_cast<uintptr_t>(dist) % 2 == 0 && reinterpret_cast<uintptr_t>(flow) % 4 == 0;
}

}  // namespace occ

extern "C" int64_t occ_submission_score_state_words(int free_id) {
  if (free_id < 1 || free_id >= occ::kScMaxCls) return 0;
  return (int64_t)(free_id + 1) * occ::kScWordsPerCls;
}

extern "C" int64_t occ_submission_score_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return (int64_t)B * occ::kScMaxChunks * occ::kScRecWords * 8;
}

extern "C" int occ_submission_score_accumulate(int pred_format, const void* pred_cls, const void* pred_dist,
                                               const void* pred_flow, int gt_format, const void* gt_cls, const void* gt_dist,
                                               const void* gt_flow, const int32_t* counts, int free_id, int64_t* state,
                                               void* workspace, int64_t workspace_bytes, int B, int64_t stride, int max_chunks,
                                               void* stream) {
  using namespace occ;
  OCC_CHECK_ARG((pred_format == 0 || pred_format == 1) && (gt_format == 0 || gt_format == 1),
                "submission_score_accumulate: format code must be 0 (packed sections) or 1 (float32 rows), got %d / %d",
                pred_format, gt_format);
  OCC_CHECK_ARG(pred_cls && gt_cls && counts && state && workspace, "submission_score_accumulate: null pointer argument");
  OCC_CHECK_ARG((pred_format == 1 || (pred_dist && pred_flow)) && (gt_format == 1 || (gt_dist && gt_flow)),
                "submission_score_accumulate: null pointer argument (packed sections need cls, dist and flow)");
  OCC_CHECK_ARG(free_id >= 1 && free_id < kScMaxCls, "submission_score_accumulate: free_id must be 1..%d (got %d)",
                kScMaxCls - 1, free_id);
  OCC_CHECK_ARG(B > 0 && B <= 65535 && stride > 0 && stride <= ((int64_t)1 << 40) / B,
                "submission_score_accumulate: bad dimension (B=%d stride=%lld)", B, (long long)stride);
  OCC_CHECK_ARG(max_chunks >= 0, "submission_score_accumulate: max_chunks must be >= 0 (got %d)", max_chunks);
  OCC_CHECK_ARG(workspace_bytes >= occ_submission_score_workspace_bytes(B),
                "submission_score_accumulate: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
                (long long)occ_submission_score_workspace_bytes(B));
  OCC_CHECK_ARG(side_aligned(pred_format, pred_cls, pred_dist, pred_flow) && side_aligned(gt_format, gt_cls, gt_dist, gt_flow) &&
                    reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && reinterpret_cast<uintptr_t>(state) % 8 == 0,
                "submission_score_accumulate: float32 rows must be 16-byte, fp16 flow 4-byte, fp16 dist 2-byte, state and "
                "workspace 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t want = (stride + kScRowsPerChunk - 1) / kScRowsPerChunk;
  if (want > kScMaxChunks) want = kScMaxChunks;
  if (max_chunks > 0 && want > max_chunks) want = max_chunks;
  const int chunks = (int)want;
  const ScSide pred = {pred_cls, pred_dist, pred_flow}, gt = {gt_cls, gt_dist, gt_flow};
  unsigned long long* records = static_cast<unsigned long long*>(workspace);
  if (pred_format == 0) {
    if (gt_format == 0) score_launch<0, 0>(st, pred, gt, counts, records, stride, free_id, B, chunks);
    else score_launch<0, 1>(st, pred, gt, counts, records, stride, free_id, B, chunks);
  } else {
    if (gt_format == 0) score_launch<1, 0>(st, pred, gt, counts, records, stride, free_id, B, chunks);
    else score_launch<1, 1>(st, pred, gt, counts, records, stride, free_id, B, chunks);
  }
  hipLaunchKernelGGL(submission_score_fold_kernel, dim3((unsigned)B), dim3(256), 0, st, records,
                     reinterpret_cast<unsigned long long*>(state), chunks, free_id);
  OCC_CHECK_LAUNCH("submission_score_accumulate");
  return OCC_OK;
}
