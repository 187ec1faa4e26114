// Shared by the two uint8 input kernels (train_input_u8.hip, input_scale_u8.hip): the launch record, the per-pixel
// photometric distortion + channel order + normalisation, the GridMask band test with its column cursor, and the host-side
// reading of a grid-mask record.  The arithmetic is stated in train_input_u8.hip's header comment.
#pragma once
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

// The mask along one output row: whether row y lies in a band, and (band number, position) of the current column.
struct GridCursor {
  int row_band, cq, cr;
};

__device__ __forceinline__ GridCursor grid_cursor(const TrainInputArgs& a, int y, int x0) {
  GridCursor g = {0, 0, 0};
  if (a.gm) {
    const unsigned ty = (unsigned)(y + a.oy - a.st_h + a.d);
    g.row_band = a.use_h & in_band((int)(ty / (unsigned)a.d) - 1, (int)(ty % (unsigned)a.d), a.nh, a.l);
    const unsigned tx = (unsigned)(x0 + a.ox - a.st_w + a.d);
    g.cq = (int)(tx / (unsigned)a.d) - 1;
    g.cr = (int)(tx % (unsigned)a.d);
  }
  return g;
}

// multiplier of the current column (1 without a mask), then one column to the right
__device__ __forceinline__ float grid_next(const TrainInputArgs& a, GridCursor& g) {
  float m = 1.f;
  if (a.gm) {
    const int band = g.row_band | (a.use_w & in_band(g.cq, g.cr, a.nw, a.l));
    m = (band ^ a.inv) ? 0.f : 1.f;
    const int wrap = lane_flag(g.cr + 1 == a.d);
    g.cr = wrap ? 0 : g.cr + 1;
    g.cq += wrap;
  }
  return m;
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

// One source pixel through the whole per-pixel chain: rec = the image's 8-float record (uniform), (b, g, r) the bytes as
// floats -> n[c] = (x[perm][to_rgb ? 2 - c : c] - mean[c]) * stdinv[c]
__device__ __forceinline__ void normalised_pixel(float b, float g, float r, const float* rec, const TrainInputArgs& a,
                                                 float n[3]) {
#pragma clang fp contract(off)
  photometric_pixel(b, g, r, rec[0], rec[1], rec[2], rec[3], rec[4]);
  // x = x[perm] (uniform per image), then the channel reversal of to_rgb
  const float pm0 = rec[5], pm1 = rec[6], pm2 = rec[7];
  float c0 = r, c1 = r, c2 = r;
  c0 = pm0 == 1.f ? g : c0; c0 = pm0 == 0.f ? b : c0;
  c1 = pm1 == 1.f ? g : c1; c1 = pm1 == 0.f ? b : c1;
  c2 = pm2 == 1.f ? g : c2; c2 = pm2 == 0.f ? b : c2;
  const float n0 = a.to_rgb ? c2 : c0, n2 = a.to_rgb ? c0 : c2;
  n[0] = (n0 - a.mean[0]) * a.stdinv[0];
  n[1] = (c1 - a.mean[1]) * a.stdinv[1];
  n[2] = (n2 - a.mean[2]) * a.stdinv[2];
}

// Host: the argument checks both entry points make, in two halves with the entry's own padded-size check between them, so
// that a call wrong in several ways gets the message it always got.
inline int check_input_buffers(const char* what, const void* x, const void* records, const float* out, const float* mean,
                               const float* std, int n_images, int Hs, int Ws) {
  OCC_CHECK_ARG(x && records && out && mean && std, "%s: null pointer argument", what);
  OCC_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(records) & 3) == 0,
                "%s: out must be 16-byte aligned, records 4-byte aligned", what);
  OCC_CHECK_ARG(n_images > 0 && n_images <= 65535 && Hs > 0 && Ws > 0, "%s: bad dimension", what);
  return OCC_OK;
}

inline int check_input_output(const char* what, const float* std, int H, int W) {
  OCC_CHECK_ARG((long)H * W < (1L << 30), "%s: image too large", what);
  OCC_CHECK_ARG(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "%s: zero std", what);
  if (W % 4 != 0) {
    set_error("%s: W = %d is not a multiple of 4 (one thread stores four pixels)", what, W);
    return OCC_E_UNSUPPORTED;
  }
  return OCC_OK;
}

// Host: mean, 1 / std and to_rgb into the record.  stdinv is formed in float64 (mmcv) and used in float32.
inline void set_norm(TrainInputArgs& a, const float* mean, const float* std, int to_rgb) {
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdinv[c] = (float)(1.0 / (double)std[c]); }
  a.to_rgb = to_rgb ? 1 : 0;
}

// Host: the 8-int grid-mask record (on, d, l, st_h, st_w, use_h, use_w, mode) of a call whose output is H x W.
// NULL or on == 0: no mask.  -> OCC_OK, or OCC_E_INVALID with the message set.
inline int set_grid_mask(TrainInputArgs& a, const int32_t* grid_mask, int H, int W, const char* what) {
  if (!grid_mask || !grid_mask[0]) return OCC_OK;
  const int d = grid_mask[1], l = grid_mask[2], st_h = grid_mask[3], st_w = grid_mask[4];
  OCC_CHECK_ARG(d >= 2, "%s: grid mask period d = %d < 2", what, d);
  OCC_CHECK_ARG(l >= 1 && l <= d - 1, "%s: grid mask band l = %d outside [1, d - 1]", what, l);
  OCC_CHECK_ARG(st_h >= 0 && st_h < d && st_w >= 0 && st_w < d, "%s: grid mask start outside [0, d)", what);
  const int hh = (int)(3L * H / 2), ww = (int)(3L * W / 2);           // int(1.5 * H)
  a.gm = 1; a.d = d; a.l = l; a.st_h = st_h; a.st_w = st_w;
  a.oy = (hh - H) / 2; a.ox = (ww - W) / 2; a.nh = hh / d; a.nw = ww / d;
  a.use_h = grid_mask[5] ? 1 : 0; a.use_w = grid_mask[6] ? 1 : 0; a.inv = grid_mask[7] == 1 ? 1 : 0;
  return OCC_OK;
}

}  // namespace occ
