/*
 * occnet_amd_input.h — C ABI of the camera input at an image scale (csrc/input_scale_u8.hip).  An extension of occnet_amd.h in
 * the same conventions: plain device pointers + sizes, a hipStream_t passed as void*, work enqueued on `stream`, no call
 * synchronises the device, 0 on success and a negative OCC_E_* code with an occ_last_error() message on failure.  The entry
 * point lives in the same library and shares its ABI version.
 *
 * Reference interface replaced (path relative to the OccNet tree, P/ = projects/mmdet3d_plugin/):
 *   occ_input_u8_scaled_f32  <- PhotoMetricDistortionMultiViewImage, NormalizeMultiviewImage, RandomScaleImageMultiViewImage,
 *        PadMultiViewImage of P/datasets/pipelines/transform_3d.py and GridMask, in the order of the "small" / "tiny" recipes
 */
#ifndef OCCNET_AMD_INPUT_H_
#define OCCNET_AMD_INPUT_H_

#include <stdint.h>

#include "occnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* uint8 frames -> photometric distortion -> normalise -> bilinear rescale to Hd x Wd -> pad to H x W -> GridMask, float32.
 *
 * x, records, mean, std, to_rgb and grid_mask are those of occ_train_input_u8_f32 (occnet_amd.h), and n(r, c) below is the value
 * that entry writes for source pixel (r, c) without a mask: (x'[perm][to_rgb ? 2 - ch : ch] - mean[ch]) * (float)(1.0 / std[ch]),
 * x' the photometrically distorted pixel.  The rescale is this library's definition of a float32 linear resize; every
 * statement is rounded to float32 unless it says double, and none is fused:
 *     scale_x = 1.0 / ((double)Wd / Ws);  scale_y = 1.0 / ((double)Hd / Hs)                          double
 *   column dx of the output, 0 <= dx < Wd:
 *     fx = (float)((dx + 0.5) * scale_x - 0.5)          product and difference in double
 *     sx = floor(fx);  fx = fx - (float)sx
 *     sx < 0:        sx = 0,      fx = 0
 *     sx >= Ws - 1:  sx = Ws - 1, fx = 0
 *     sx1 = min(sx + 1, Ws - 1);  a0 = 1.f - fx;  a1 = fx
 *   row dy, 0 <= dy < Hd:
 *     fy, sy formed alike from scale_y; fy is NOT reset at the borders
 *     r0 = clip(sy, 0, Hs - 1);  r1 = clip(sy + 1, 0, Hs - 1);  b0 = 1.f - fy;  b1 = fy
 *   per channel:
 *     h0 = n(r0, sx) * a0 + n(r0, sx1) * a1
 *     h1 = n(r1, sx) * a0 + n(r1, sx1) * a1
 *     out(dy, dx) = (h0 * b0 + h1 * b1) * mask(dy, dx)
 * out is 0 wherever dy >= Hd or dx >= Wd, and the GridMask is that of an H x W image.  Hd == Hs and Wd == Ws give what
 * occ_train_input_u8_f32 writes.  Hd and Wd are arguments: how a scale factor becomes a size is the caller's rule.
 *   x          (n_images, Hs, Ws, 3) uint8; nothing outside these bytes is read
 *   records    (n_images, 8) float32, 4-byte aligned
 *   out        (n_images, 3, H, W) float32, 16-byte aligned; every element is written
 *   mean, std  3 host floats each, std != 0
 *   grid_mask  NULL, or 8 host ints (on, d, l, st_h, st_w, use_h, use_w, mode)
 *   1 <= n_images <= 65535; 1 <= Hd <= H, 1 <= Wd <= W; Hs, Ws, H, W <= 32768; H * W < 2^30; W % 4 == 0 (OCC_E_UNSUPPORTED
 *   otherwise: one thread stores four pixels)
 * One launch. */
int occ_input_u8_scaled_f32(const uint8_t* x, const void* records, float* out, int n_images, int Hs, int Ws, int Hd, int Wd,
                            int H, int W, const float* mean, const float* std, int to_rgb, const int32_t* grid_mask,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCCNET_AMD_INPUT_H_ */
