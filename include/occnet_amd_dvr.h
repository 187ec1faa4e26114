/*
 * occnet_amd_dvr.h — C ABI of the differentiable ray renderer (csrc/dvr_render_train.hip).  An extension of occnet_amd.h in the
 * same conventions: plain device pointers + sizes, a hipStream_t passed as void*, work enqueued on `stream`, no call
 * synchronises the device, 0 on success and a negative OCC_E_* code with an occ_last_error() message on failure.  The entry
 * point lives in the same library and shares its ABI version.
 *
 * Reference interface replaced (path relative to the OccNet tree):
 *   occ_dvr_render_f32  <- dvr.render(sigma, origin, points, tindex, loss_name), tools/ray_iou/lib/dvr/dvr.cu:391-703
 */
#ifndef OCCNET_AMD_DVR_H_
#define OCCNET_AMD_DVR_H_

#include <stdint.h>

#include "occnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Expected depth of every ray through a density grid, and the gradient of a depth loss summed over the rays with respect to
 * every voxel a ray crossed.  All tensors float32, dense, voxel units:
 *   sigma       (N, T, Z, Y, X)  density, sigma[z][y][x]
 *   origin      (N, T, 3)        ray origins (x, y, z)
 *   points      (N, M, point_stride >= 3)  ray end points (x, y, z, ...)
 *   tindex      (N, M)           the origin / time slice of each ray (sigma slice 0 when T == 1)
 *   pred_dist   (N, M)  out      expected depth, -1 for a ray that is not rendered
 *   gt_dist     (N, M)  out      min(|end - origin|, exit distance of the last in-grid voxel), -1 likewise
 *   grad_sigma  (N, T, Z, Y, X)  out  d(sum of the per-ray losses) / d sigma
 *   loss_type   0: l1  |p - g|,  1: l2  (p - g)^2 / 2,  2: absrel  |p - g| / g
 * The call itself sets pred_dist = gt_dist = -1 and grad_sigma = 0 first.
 *
 * Per ray, in double on the float inputs, uncontracted: the voxel walk of occ_dvr_render_forward_f32 (the same set-up, the same
 * comparison order, steps 0..1000), which before it has entered the grid also stops once the distance walked exceeds
 * |end - origin|.  For the in-grid voxels 0..n-1 with exit distances d_i, delta_i = max(0, d_i - d of the step before),
 * T_i = exp(-sum_{j<=i} sigma_j delta_j):
 *     pred = sum_i (T_{i-1} - T_i) d_i + T_{n-1} d_{n-1}      (T_{-1} = 1; summed in this order)
 *     d pred / d sigma_k = -delta_k * sum_{j=k}^{n-2} T_j (d_{j+1} - d_j)
 *     d loss / d pred    = l1: pred >= gt ? 1 : -1;  l2: pred - gt;  absrel: (pred >= gt ? 1 : -1) / gt
 * The kernel walks each ray twice with a few scalars of state (no per-step array): the first walk gives pred, gt and the sum,
 * the second repeats the identical walk and adds each voxel's term.  A ray that never enters the grid keeps -1 and adds nothing.
 *
 * Two deliberate deviations from the reference:
 *   - PADDED RAYS.  The reference skips a ray with tindex < 0.  Here a ray is also skipped (outputs stay -1, nothing is added
 *     to grad_sigma) when it has zero length (end == origin: 0 / 0 in the reference), when one of its six coordinates is not
 *     finite, or when its tindex is NaN or >= T (the reference asserts; it would read past `origin`).  The reference would write
 *     NaN into the grid for the first two.
 *   - ACCUMULATION.  The terms are added with float atomics (the reference uses a plain racy +=), one atomic per voxel and ray:
 *     no term is lost, but the sums may differ in their last bits from run to run (the order of the adds is not fixed).
 *     A term that is exactly zero (delta_k = 0, the last voxel of a ray, l2 with pred == gt) issues no add.
 *
 * N, T, Z, Y, X, M > 0; N * T * Z * Y * X < 2^62 elements; N <= 65535 (one grid row per batch entry).
 * One memset and two launches (the -1 fill, the renderer). */
int occ_dvr_render_f32(const float* sigma, const float* origin, const float* points, const float* tindex, float* pred_dist,
                       float* gt_dist, float* grad_sigma, int N, int T, int Z, int Y, int X, int M, int point_stride,
                       int loss_type, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCCNET_AMD_DVR_H_ */
