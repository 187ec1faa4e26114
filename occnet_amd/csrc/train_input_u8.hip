// The reference's TRAINING input in one pass (bevformer_base_occ.py:153-164 + use_grid_mask):
//   PhotoMetricDistortionMultiViewImage -> NormalizeMultiviewImage -> PadMultiViewImage -> GridMask
// on raw uint8 frames: x (NI, Hs, Ws, 3) uint8 HWC, channel order as loaded (BGR)  ->  out (NI, 3, H, W) fp32 NCHW, every
// element written, the pad area 0.  The random draws stay on the host (occnet_amd/io.py: sample_photometric,
// plugin/grid_mask.py: GridMask.sample_params), a record of 8 floats per image and one grid record per call come in.
//
// Per pixel, float32, in the reference's order (transform_3d.py:141-188, :91, :31-43, grid_mask.py:84-124):
//   x = float(u8) ; x += delta ; x *= alpha_pre
//   BGR -> HSV as OpenCV's float path: v = max, diff = v - min, s = diff / (|v| + eps), k = 60 / (diff + eps),
//     h = (g-b)k | (b-r)k + 120 | (r-g)k + 240 on v == r | v == g | else ; h < 0: h += 360
//   s *= sat ; h += hue ; h > 360: h -= 360 ; h < 0: h += 360
//   HSV -> BGR as OpenCV's float path (sector table) ; x *= alpha_post ; x = x[perm]
//   to_rgb: reverse ; x = (x - mean) * (1 / std) ; x *= grid mask
// A stage that is off has the identity as its parameter (delta 0, alpha 1, sat 1, hue 0, perm 0 1 2): x + 0, x * 1 and
// h + 0 are exact, and h leaves BGR -> HSV inside [0, 360] (each branch gives [-60, 300] before the wrap), so the two
// wrap tests of the hue stage are no-ops when hue == 0.  The kernel therefore applies every stage unconditionally and
// still equals the reference, which skips the stages that are off.  The HSV round trip is always made, as there.
//
// One thread = four horizontally adjacent output pixels: 12 byte loads (a row of 3-byte pixels starts at any byte
// address; the loads of a wave cover 768 contiguous bytes), one float4 store per plane.  blockIdx.y = image, so the
// image's record arrives through uniform loads.  Source coordinates are clamped into the frame (the pad area reads
// the frame's last row / column and discards it): nothing outside the NI * Hs * Ws * 3 bytes is read.
#include "train_input.h"

namespace occ {

__global__ __launch_bounds__(256) void train_input_u8_kernel(const unsigned char* __restrict__ x,
                                                             const float* __restrict__ records, float* __restrict__ out,
                                                             TrainInputArgs a) {
#pragma clang fp contract(off)
  const int W4 = a.W >> 2;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.H * W4) return;
  const int img = blockIdx.y;
  const int y = item / W4, x0 = (item - y * W4) * 4;
  const float* rec = records + (long)img * 8;

  // 12 clamped byte loads first, then the arithmetic
  const int sy = min(y, a.Hs - 1);
  const unsigned char* row = x + ((long)img * a.Hs + sy) * a.Ws * 3;
  unsigned char raw[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sx = min(x0 + j, a.Ws - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) raw[j][c] = row[sx * 3 + c];
  }

  const int row_in = lane_flag(y < a.Hs);
  GridCursor gc = grid_cursor(a, y, x0);

  float o[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float n[3];
    normalised_pixel((float)raw[j][0], (float)raw[j][1], (float)raw[j][2], rec, a, n);
    const float m = grid_next(a, gc);
    const int in = row_in & lane_flag(x0 + j < a.Ws);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c][j] = in ? n[c] * m : 0.f;
  }
  const long plane = (long)a.H * a.W;
  float* dst = out + (long)img * 3 * plane + (long)y * a.W + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *reinterpret_cast<float4*>(dst + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
}

}  // namespace occ

extern "C" int occ_train_input_u8_f32(const uint8_t* x, const void* records, float* out, int n_images, int Hs, int Ws,
                                      int H, int W, const float* mean, const float* std, int to_rgb,
                                      const int32_t* grid_mask, void* stream) {
  using namespace occ;
  if (int rc = check_input_buffers("train_input_u8", x, records, out, mean, std, n_images, Hs, Ws)) return rc;
  OCC_CHECK_ARG(H >= Hs && W >= Ws, "train_input_u8: padded size (%d, %d) smaller than the frames (%d, %d)", H, W, Hs, Ws);
  if (int rc = check_input_output("train_input_u8", std, H, W)) return rc;
  TrainInputArgs a = {};
  set_norm(a, mean, std, to_rgb);
  a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
  if (int rc = set_grid_mask(a, grid_mask, H, W, "train_input_u8")) return rc;
  const int items = H * (W / 4);
  hipLaunchKernelGGL(train_input_u8_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)n_images), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, reinterpret_cast<const float*>(records), out, a);
  OCC_CHECK_LAUNCH("train_input_u8");
  return OCC_OK;
}
