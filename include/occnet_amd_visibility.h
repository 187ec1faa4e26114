/*
 * occnet_amd_visibility.h — C ABI of the camera visibility masks and the masked voxel confusion counts
 * (csrc/visibility.hip).  An extension of occnet_amd.h in the same conventions: plain device pointers + sizes, a hipStream_t
 * passed as void*, work enqueued on `stream`, no call synchronises the device, 0 on success and a negative OCC_E_* code with
 * an occ_last_error() message on failure.  The entry points live in the same library and share its ABI version.
 *
 * Reference interfaces replaced (paths relative to the OccNet tree, P/ = projects/mmdet3d_plugin/):
 *   occ_visibility_views      <- the `mask_camera` input of BEVFormerOccHead.loss (use_mask=True),
 *        P/bevformer/dense_heads/bevformer_occ_head.py:183-188, which the challenge's ground-truth files do not carry
 *   occ_confusion_accumulate  <- the per-class voxel IoU over the voxels a mask admits
 */
#ifndef OCCNET_AMD_VISIBILITY_H_
#define OCCNET_AMD_VISIBILITY_H_

#include <stdint.h>

#include "occnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The voxels seen by the cameras: mask u8 (B, X, Y, Z), 1 where at least one pixel ray of at least one of the V views of the
 * sample visits the voxel, else 0; every byte is written.
 *
 * For sample b, view v and pixel (i, j) of an h x w raster the ray is the ray of occ_render_views (occnet_amd.h), the same
 * float32 statements in the same order, uncontracted:
 *     px = (float)j + 0.5f;  py = (float)i + 0.5f
 *     dir_k = (D[k][0] * px + D[k][1] * py) + D[k][2]          k = 0, 1, 2
 *     ray_k = dir_k * far
 *     end = ray + o;  origin, end -> (p - off) / voxel_size      float32
 * and the walk is the first-hit walk of that renderer (steps 0..1000, the same comparison order, the same "left the grid"
 * stop).  A voxel is VISITED by a ray if the walk's body runs for it while it lies inside the grid, the first occupied voxel
 * (class != free_id; int64 ids beyond int count as occupied), where the walk ends, included.  A ray that never enters the grid
 * marks nothing; a camera inside an occupied voxel marks only that voxel; `far` only scales the direction, the walk is not cut
 * at `far`.
 *   sem              (B, X, Y, Z) class ids, sem_dtype 0: uint8, 1: int64
 *   cams             (B, V, 12) float32: per view the centre o[3] in ego metres and the row-major 3 x 3 D
 *   off_x .. off_z   pc_range[:3];  voxel_size > 0;  free_id 1..31;  far > 0, finite
 *   mask             B * X * Y * Z bytes
 *   workspace        occ_visibility_workspace_bytes(B, X, Y, Z) bytes, 4-byte aligned, uninitialised and reusable as it is: the
 *                    pillar occupancy masks, then one uint32 visibility word per pillar (cleared by the call itself)
 *   Z <= 32 (OCC_E_UNSUPPORTED beyond; the workspace query answers 0), B * V <= 65535, h, w in 1..16384
 * Three launches. */
int64_t occ_visibility_workspace_bytes(int B, int X, int Y, int Z);
int occ_visibility_views(const void* sem, int sem_dtype, const float* cams, float off_x, float off_y, float off_z,
                         float voxel_size, int free_id, float far, uint8_t* mask, void* workspace, int64_t workspace_bytes,
                         int B, int V, int X, int Y, int Z, int h, int w, void* stream);

/* Confusion counts of two class grids over the voxels a mask admits, added to `state`:
 * (ncls + 1) * ncls int64 words, ncls = free_id + 1.  For every voxel n in [0, n_voxels) with mask == NULL or mask[n] != 0:
 *     state[ncls * ncls + 1] += 1                               admitted voxels
 *     g = class(sem_gt[n]), p = class(sem_pred[n])              (int64 ids beyond int are no class)
 *     both in 0..free_id:  state[g * ncls + p] += 1             row = ground truth, column = prediction
 *     otherwise:           state[ncls * ncls + 0] += 1          skipped voxels
 * The other words of the last row stay untouched.  Counts are exact integers: calls, batches and ranks add up in any order.
 *   sem_pred, sem_gt  n_voxels class ids each, dtype code 0: uint8, 1: int64
 *   mask              NULL, or n_voxels bytes (bool or uint8)
 *   state             occ_confusion_state_words(free_id) words, 8-byte aligned (0 words: free_id outside 1..31)
 *   n_voxels          1 .. 2^40
 * One launch. */
int64_t occ_confusion_state_words(int free_id);
int occ_confusion_accumulate(const void* sem_pred, int sem_pred_dtype, const void* sem_gt, int sem_gt_dtype,
                             const uint8_t* mask, int free_id, int64_t* state, int64_t n_voxels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCCNET_AMD_VISIBILITY_H_ */
