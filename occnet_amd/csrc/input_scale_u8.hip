// The camera input at an image scale, in one pass (RandomScaleImageMultiViewImage between normalise and pad):
//   PhotoMetricDistortionMultiViewImage -> NormalizeMultiviewImage -> bilinear rescale to Hd x Wd -> PadMultiViewImage -> GridMask
// on raw uint8 frames: x (NI, Hs, Ws, 3) uint8 HWC, channel order as loaded (BGR)  ->  out (NI, 3, H, W) fp32 NCHW, every
// element written, everything outside Hd x Wd exactly 0.  The per-pixel chain up to the normalised value n(r, c) is
// train_input_u8.hip's (train_input.h); the rescale is the project's definition of a float32 linear resize (DESIGN.md,
// "Image scale on the device"; include/occnet_amd_input.h states it in full), float32, every operation rounded, none fused:
//   scale_x = 1.0 / ((double)Wd / Ws), scale_y alike (formed once on the host, in double)
//   column dx: fx = (float)((dx + 0.5) * scale_x - 0.5) in double; sx = floor(fx); fx -= sx;
//              sx < 0: sx = 0, fx = 0;  sx >= Ws - 1: sx = Ws - 1, fx = 0;  taps sx, min(sx + 1, Ws - 1), weights 1 - fx, fx
//   row dy:    fy, sy alike, fy NOT zeroed at the borders; rows clip(sy), clip(sy + 1) into [0, Hs - 1], weights 1 - fy, fy
//   out = (n(r0,sx) a0 + n(r0,sx1) a1) b0 + (n(r1,sx) a0 + n(r1,sx1) a1) b1 ; out *= grid mask (of the H x W output)
// Hd == Hs and Wd == Ws give fx = fy = 0 in every pixel and the result of train_input_u8 (n * 1 + n' * 0).
//
// One thread = four horizontally adjacent output pixels, one float4 store per plane; blockIdx.y = image, so the record
// arrives through uniform loads.  Tap indices and weights depend on dx or dy and the sizes alone: once per thread for the
// row, four times for the columns.  Tap coordinates are clamped into the frame for every thread, the pad area's included:
// nothing outside the NI * Hs * Ws * 3 bytes is read.  The four pixels are a ROLLED loop: per pixel the four taps' 12 byte
// loads, then the photometric chain on the four taps side by side.  Unrolled, the compiler interleaves all 16 chains
// (201 VGPRs, 2 waves per SIMD); rolled it needs 78 (6 waves), and a pixel's result goes to its slot by uniform selects.
#include "train_input.h"
#include "../../include/occnet_amd_input.h"

namespace occ {

struct ScaledInputArgs {
  TrainInputArgs t;              // Hs x Ws the frames, H x W the output
  int Hd, Wd;                    // the resized image inside the output
  double scale_x, scale_y;
};

// One axis of the resize: d = destination index, scale = the double ratio  ->  i = floor of the source coordinate
// (unclamped), f = its fraction
__device__ __forceinline__ void source_coord(int d, double scale, int& i, float& f) {
#pragma clang fp contract(off)
  const float s = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(s);
  i = (int)fl;
  f = s - fl;
}

__global__ __launch_bounds__(256) void input_scale_u8_kernel(const unsigned char* __restrict__ x,
                                                             const float* __restrict__ records, float* __restrict__ out,
                                                             ScaledInputArgs sa) {
#pragma clang fp contract(off)
  const TrainInputArgs& a = sa.t;
  const int W4 = a.W >> 2;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.H * W4) return;
  const int img = blockIdx.y;
  const int y = item / W4, x0 = (item - y * W4) * 4;
  const float* rec = records + (long)img * 8;

  // rows: the weight keeps its fraction at the borders, the indices are clipped
  int sy;
  float fy;
  source_coord(y, sa.scale_y, sy, fy);
  const int r0 = min(max(sy, 0), a.Hs - 1), r1 = min(max(sy + 1, 0), a.Hs - 1);
  const float b0 = 1.f - fy, b1 = fy;
  const unsigned char* img0 = x + (long)img * a.Hs * a.Ws * 3;
  const unsigned char* row0 = img0 + (long)r0 * a.Ws * 3;
  const unsigned char* row1 = img0 + (long)r1 * a.Ws * 3;

  const int row_in = lane_flag(y < sa.Hd);
  GridCursor gc = grid_cursor(a, y, x0);

  float o[3][4] = {};
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    int sx;
    float fx;
    source_coord(x0 + j, sa.scale_x, sx, fx);
    const int lo = lane_flag(sx < 0), hi = lane_flag(sx >= a.Ws - 1);
    const float a1 = (lo | hi) ? 0.f : fx, a0 = 1.f - a1;
    sx = min(max(sx, 0), a.Ws - 1);
    const int sx1 = min(sx + 1, a.Ws - 1);
    unsigned char raw[2][2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      raw[0][0][c] = row0[sx * 3 + c];
      raw[0][1][c] = row0[sx1 * 3 + c];
      raw[1][0][c] = row1[sx * 3 + c];
      raw[1][1][c] = row1[sx1 * 3 + c];
    }
    float n[2][2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        normalised_pixel((float)raw[r][t][0], (float)raw[r][t][1], (float)raw[r][t][2], rec, a, n[r][t]);
    const float m = grid_next(a, gc);
    const int in = row_in & lane_flag(x0 + j < sa.Wd);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float h0 = n[0][0][c] * a0 + n[0][1][c] * a1;
      const float h1 = n[1][0][c] * a0 + n[1][1][c] * a1;
      const float v = h0 * b0 + h1 * b1;
      const float w = in ? v * m : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[c][k] = j == k ? w : o[c][k];
    }
  }
  const long plane = (long)a.H * a.W;
  float* dst = out + (long)img * 3 * plane + (long)y * a.W + x0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    *reinterpret_cast<float4*>(dst + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
}

}  // namespace occ

extern "C" int occ_input_u8_scaled_f32(const uint8_t* x, const void* records, float* out, int n_images, int Hs, int Ws,
                                       int Hd, int Wd, int H, int W, const float* mean, const float* std, int to_rgb,
                                       const int32_t* grid_mask, void* stream) {
  using namespace occ;
  if (int rc = check_input_buffers("input_u8_scaled", x, records, out, mean, std, n_images, Hs, Ws)) return rc;
  OCC_CHECK_ARG(Hd >= 1 && Wd >= 1, "input_u8_scaled: resized size (%d, %d) has an empty dimension", Hd, Wd);
  OCC_CHECK_ARG(H >= Hd && W >= Wd, "input_u8_scaled: padded size (%d, %d) smaller than the resized image (%d, %d)", H, W, Hd,
                Wd);
  // (dx + 0.5) * scale_x <= (W + 0.5) * Ws < 2^31: the float source coordinate converts to int, and every index stays an int
  OCC_CHECK_ARG(Hs <= 32768 && Ws <= 32768 && H <= 32768 && W <= 32768,
                "input_u8_scaled: a dimension beyond 32768 (frames (%d, %d), output (%d, %d))", Hs, Ws, H, W);
  if (int rc = check_input_output("input_u8_scaled", std, H, W)) return rc;
  ScaledInputArgs sa = {};
  set_norm(sa.t, mean, std, to_rgb);
  sa.t.Hs = Hs; sa.t.Ws = Ws; sa.t.H = H; sa.t.W = W;
  sa.Hd = Hd; sa.Wd = Wd;
  sa.scale_x = 1.0 / ((double)Wd / Ws);
  sa.scale_y = 1.0 / ((double)Hd / Hs);
  if (int rc = set_grid_mask(sa.t, grid_mask, H, W, "input_u8_scaled")) return rc;
  const int items = H * (W / 4);
  hipLaunchKernelGGL(input_scale_u8_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)n_images), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, reinterpret_cast<const float*>(records), out, sa);
  OCC_CHECK_LAUNCH("input_u8_scaled");
  return OCC_OK;
}
