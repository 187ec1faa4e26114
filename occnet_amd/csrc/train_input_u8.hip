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
#include "common.h"
#include <float.h>

namespace occ {

struct TrainInputArgs {
  float mean[3], stdinv[3];
  int Hs, Ws, H, W, to_rgb;
  // GridMask (rotate = 1, offset = False): d, l, st_h, st_w as drawn; oy / ox = offset of the crop in the
  // (1.5 H, 1.5 W) plane; nh / nw = number of bands (hh / d, ww / d); use_h / use_w / inv as 0 / 1
  int gm, d, l, st_h, st_w, oy, ox, nh, nw, use_h, use_w, inv;
};

// band test of grid_mask.py:96-110 on coordinate t = Y - st + d (> 0 because st < d): quotient q = t / d - 1 is the band
// number, r = t % d the position inside the period; in a band iff 0 <= q < n and r < l
__device__ __forceinline__ int in_band(int q, int r, int n, int l) {
  return lane_flag(q >= 0) & lane_flag(q < n) & lane_flag(r < l);
}

__device__ __forceinline__ void photometric_pixel(float& b, float& g, float& r, float delta, float alpha_pre, float sat,
                                                  float hue, float alpha_post) {
#pragma clang fp contract(off)        // the reference rounds every operation: no fused multiply-add
  b = (b + delta) * alpha_pre;
  g = (g + delta) * alpha_pre;
  r = (r + delta) * alpha_pre;
  // BGR -> HSV
  const float v = fmaxf(fmaxf(b, g), r), vmin = fminf(fminf(b, g), r);
  const float diff = v - vmin;
  float s = fdiv(diff, fabsf(v) + FLT_EPSILON);
  const float k = fdiv(60.f, diff + FLT_EPSILON);
  const int is_r = lane_flag(v == r), is_g = lane_flag(v == g);
  const float hr = (g - b) * k, hg = (b - r) * k + 120.f, hb = (r - g) * k + 240.f;
  float h = hb;                                   // flat select chains: all three candidates are computed, no branch
  h = is_g ? hg : h;
  h = is_r ? hr : h;
  h = lane_flag(h < 0.f) ? h + 360.f : h;
  // saturation, hue
  s *= sat;
  h += hue;
  h = lane_flag(h > 360.f) ? h - 360.f : h;
  h = lane_flag(h < 0.f) ? h + 360.f : h;
  // HSV -> BGR.  h is in [0, 360] here, so one step of -6 brings h / 60 into [0, 6)
  const int grey = lane_flag(s == 0.f);
  h *= (float)(1.0 / 60.0);
  h = lane_flag(h < 0.f) ? h + 6.f : h;
  h = lane_flag(h >= 6.f) ? h - 6.f : h;
  const float fl = floorf(h);
  const int over = lane_flag(fl >= 6.f);          // (unsigned)sector >= 6: sector = 0, f = 0
  const float sec = over ? 0.f : fl;
  const float f = over ? 0.f : h - fl;
  const float p = v * (1.f - s), q = v * (1.f - s * f), t = v * (1.f - s * (1.f - f));
  const int e0 = lane_flag(sec == 0.f), e1 = lane_flag(sec == 1.f), e2 = lane_flag(sec == 2.f), e3 = lane_flag(sec == 3.f),
            e4 = lane_flag(sec == 4.f);
  // tab = {v, p, q, t}; (b, g, r) = tab[{{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}[sector]]
  float nb = q, ng = p, nr = v;                   // sector 5
  nb = (e3 | e4) ? v : nb; nb = e2 ? t : nb; nb = (e0 | e1) ? p : nb;
  ng = e3 ? q : ng; ng = (e1 | e2) ? v : ng; ng = e0 ? t : ng;
  nr = e4 ? t : nr; nr = (e2 | e3) ? p : nr; nr = e1 ? q : nr;
  b = (grey ? v : nb) * alpha_post;
  g = (grey ? v : ng) * alpha_post;
  r = (grey ? v : nr) * alpha_post;
}

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
  const float delta = rec[0], alpha_pre = rec[1], sat = rec[2], hue = rec[3], alpha_post = rec[4];
  const float pm0 = rec[5], pm1 = rec[6], pm2 = rec[7];

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
  int row_band = 0, cq = 0, cr = 0;
  if (a.gm) {
    const unsigned ty = (unsigned)(y + a.oy - a.st_h + a.d);
    row_band = a.use_h & in_band((int)(ty / (unsigned)a.d) - 1, (int)(ty % (unsigned)a.d), a.nh, a.l);
    const unsigned tx = (unsigned)(x0 + a.ox - a.st_w + a.d);
    cq = (int)(tx / (unsigned)a.d) - 1;
    cr = (int)(tx % (unsigned)a.d);
  }

  float o[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float b = (float)raw[j][0], g = (float)raw[j][1], r = (float)raw[j][2];
    photometric_pixel(b, g, r, delta, alpha_pre, sat, hue, alpha_post);
    // x = x[perm] (uniform per image), then the channel reversal of to_rgb
    float c0 = r, c1 = r, c2 = r;
    c0 = pm0 == 1.f ? g : c0; c0 = pm0 == 0.f ? b : c0;
    c1 = pm1 == 1.f ? g : c1; c1 = pm1 == 0.f ? b : c1;
    c2 = pm2 == 1.f ? g : c2; c2 = pm2 == 0.f ? b : c2;
    const float n0 = a.to_rgb ? c2 : c0, n2 = a.to_rgb ? c0 : c2;
    float m = 1.f;
    if (a.gm) {
      const int band = row_band | (a.use_w & in_band(cq, cr, a.nw, a.l));
      m = (band ^ a.inv) ? 0.f : 1.f;
      const int wrap = lane_flag(cr + 1 == a.d);         // next column
      cr = wrap ? 0 : cr + 1;
      cq += wrap;
    }
    const int in = row_in & lane_flag(x0 + j < a.Ws);
    o[0][j] = in ? (n0 - a.mean[0]) * a.stdinv[0] * m : 0.f;
    o[1][j] = in ? (c1 - a.mean[1]) * a.stdinv[1] * m : 0.f;
    o[2][j] = in ? (n2 - a.mean[2]) * a.stdinv[2] * m : 0.f;
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
  OCC_CHECK_ARG(x && records && out && mean && std, "train_input_u8: null pointer argument");
  OCC_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(records) & 3) == 0,
                "train_input_u8: out must be 16-byte aligned, records 4-byte aligned");
  OCC_CHECK_ARG(n_images > 0 && n_images <= 65535 && Hs > 0 && Ws > 0, "train_input_u8: bad dimension");
  OCC_CHECK_ARG(H >= Hs && W >= Ws, "train_input_u8: padded size (%d, %d) smaller than the frames (%d, %d)", H, W, Hs, Ws);
  OCC_CHECK_ARG((long)H * W < (1L << 30), "train_input_u8: image too large");
  OCC_CHECK_ARG(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "train_input_u8: zero std");
  if (W % 4 != 0) {
    set_error("train_input_u8: W = %d is not a multiple of 4 (one thread stores four pixels)", W);
    return OCC_E_UNSUPPORTED;
  }
  TrainInputArgs a = {};
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdinv[c] = (float)(1.0 / (double)std[c]); }   // stdinv in f64 (mmcv), used in f32
  a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W; a.to_rgb = to_rgb ? 1 : 0;
  if (grid_mask && grid_mask[0]) {
    const int d = grid_mask[1], l = grid_mask[2], st_h = grid_mask[3], st_w = grid_mask[4];
    OCC_CHECK_ARG(d >= 2, "train_input_u8: grid mask period d = %d < 2", d);
    OCC_CHECK_ARG(l >= 1 && l <= d - 1, "train_input_u8: grid mask band l = %d outside [1, d - 1]", l);
    OCC_CHECK_ARG(st_h >= 0 && st_h < d && st_w >= 0 && st_w < d, "train_input_u8: grid mask start outside [0, d)");
    const int hh = (int)(3L * H / 2), ww = (int)(3L * W / 2);           // int(1.5 * H)
    a.gm = 1; a.d = d; a.l = l; a.st_h = st_h; a.st_w = st_w;
    a.oy = (hh - H) / 2; a.ox = (ww - W) / 2; a.nh = hh / d; a.nw = ww / d;
    a.use_h = grid_mask[5] ? 1 : 0; a.use_w = grid_mask[6] ? 1 : 0; a.inv = grid_mask[7] == 1 ? 1 : 0;
  }
  const int items = H * (W / 4);
  hipLaunchKernelGGL(train_input_u8_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)n_images), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, reinterpret_cast<const float*>(records), out, a);
  OCC_CHECK_LAUNCH("train_input_u8");
  return OCC_OK;
}
