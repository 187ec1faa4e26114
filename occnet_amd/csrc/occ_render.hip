// Occupancy rendered on the device: pin-hole camera views and a bird's-eye view of a batch of class grids, as label / depth /
// colour images.  The third client of ray_cast.h (after ray_metrics_fused.hip and submission_rays.hip): a camera is one more
// bundle of rays through the same occupancy bit masks and the same first-hit traversal, so a pixel reports the voxel and the
// distance that the evaluator and the submission writer report for that ray, bit for bit.
//
// PERSPECTIVE VIEWS — one thread per pixel (i, j) of view v of sample b; a wave is an 8 x 8 pixel tile, a block four tiles side
// by side (32 x 8 pixels), grid (ceil(w / 32), ceil(h / 8), B * V).  Per view the host gives 12 floats: the camera centre
// o[3] (ego metres) and a row-major 3 x 3 matrix D (vis.view_rays).  float32 throughout, uncontracted, in this order:
//   px = (float)j + 0.5f;  py = (float)i + 0.5f
//   dir_k = (D[k][0] * px + D[k][1] * py) + D[k][2]          k = 0, 1, 2
//   ray_k = dir_k * far                                      far in metres
//   rm_ray_from_origin(o, ray, off, voxel_size)              the float32 overload: end = ray + o, (p - off) / voxel_size
//   hit = rm_cast(...)                                       voxel (x, y, z) and ray parameter `dist` in voxel units
//   depth = hit.dist * voxel_size
// class = the grid's value at the reported voxel.  The pixel is a HIT iff hit.dist >= 0 and class != free_id; a ray that never
// enters the grid reports voxel (0, 0, 0) with dist -1 and is a miss whatever that voxel holds.
//   label  u8  (B, V, h, w)     hit: class & 0xff, miss: free_id
//   depth  f32 (B, V, h, w)     hit: depth in metres, miss: -1
//   rgb    u8  (B, V, h, w, 3)  per channel k, all in int:
//       bg[k]  = frames ? frames[b][v][si][sj][k] : (bg_rgb >> (16 - 8 * k)) & 0xff
//                si = ((2 * i + 1) * Hs) / (2 * h),  sj = ((2 * j + 1) * Ws) / (2 * w)       (nearest, integer division)
//       q      = (int)fminf((depth * 192.0f) / far, 192.0f)                                  (the one float -> int truncation)
//       shade  = 256 - q                                                                     (64 .. 256)
//       lit    = (palette[label][k] * shade) >> 8
//       hit:  (lit * alpha + bg[k] * (256 - alpha)) >> 8          miss: bg[k]
// DIFF MODE (sem_gt given) — the same launch casts the ray through the ground truth's masks too; `label` then holds a category:
//   0 both miss | 1 both hit, same class, fabsf(depth_pred - depth_gt) < tol | 2 same class, depth off | 3 both hit, class
//   differs | 4 prediction hits, ground truth misses | 5 ground truth hits, prediction misses.
// Classes are compared as read (int64 ids in full).  `depth` stays the prediction's.  rgb: category 0 is bg; otherwise the colour
// is palette[class_gt & 0xff] for category 1 and cat_palette[category] for 2..5, shaded by the prediction's depth where it hit
// (categories 1..4) and the ground truth's for category 5, then blended as above.
//
// BEV — one thread per pillar (b, x, y), in grid order (the display orientation is the caller's flip):
//   top = index of the highest set bit of the pillar's mask;  empty pillar: label = free_id, rgb = bg_rgb
//   label = class(x, y, top) & 0xff;  shade = 128 + (128 * (top + 1)) / Z;  rgb[k] = (palette[label][k] * shade) >> 8
// diff mode: category 0 both empty | 1 same class and same top | 2 same class, top differs | 3 class differs | 4 prediction only |
//   5 ground truth only; colour as for the views (category 1: palette[class_gt & 0xff]), shaded by the prediction's top where it
//   has one and the ground truth's for category 5; no blend.
//
// A pixel outside the image is a dead lane: zero traversal steps, clamped legal load addresses, no store.  Predicates that select
// a load address are 0 / 1 integers (common.h: lane_flag).  One mask launch + one render launch on the caller's stream.
#include <limits.h>
#include "ray_cast.h"

namespace occ {

struct RdArgs {
  const void* sem; const void* sem_gt; const float* cams; const unsigned char* frames; const unsigned char* palette;
  const unsigned char* cat_palette; const void* masks; unsigned char* label; float* depth; unsigned char* rgb;
  float off_x, off_y, off_z, voxel_size, far, tol;
  int sem_i64, gt_i64, free_id, alpha, bg_rgb, Hs, Ws, B, V, X, Y, Z, h, w;
};

__device__ __forceinline__ int rd_shade(float depth, float far) {
#pragma clang fp contract(off)
  return 256 - (int)fminf((depth * 192.0f) / far, 192.0f);
}

template <typename MaskT, int DIFF>
__global__ __launch_bounds__(256) void occ_render_views_kernel(const RdArgs a) {
#pragma clang fp contract(off)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 32 + wave * 8 + (lane & 7);
  const int i = blockIdx.y * 8 + (lane >> 3);
  const int bv = blockIdx.z, b = bv / a.V;
  const int live = lane_flag(j < a.w) & lane_flag(i < a.h);
  const int jj = live ? j : 0, ii = live ? i : 0;
  const float* cam = a.cams + (long)bv * 12;
  const float px = (float)jj + 0.5f, py = (float)ii + 0.5f;
  const float rx = ((cam[3] * px + cam[4] * py) + cam[5]) * a.far;
  const float ry = ((cam[6] * px + cam[7] * py) + cam[8]) * a.far;
  const float rz = ((cam[9] * px + cam[10] * py) + cam[11]) * a.far;
  const RmRay rs = rm_ray_from_origin(cam[0], cam[1], cam[2], rx, ry, rz, a.off_x, a.off_y, a.off_z, a.voxel_size);
  const long pillars = (long)a.X * a.Y, cells = pillars * a.Z;
  const MaskT* masks = static_cast<const MaskT*>(a.masks);

  const RmHit hp = rm_cast<MaskT>(rs, masks + b * pillars, a.X, a.Y, a.Z, live);
  const int cp = rm_class_at(a.sem, a.sem_i64, b * cells + ((long)hp.x * a.Y + hp.y) * a.Z + hp.z);   // (0, 0, 0): legal
  const int hit_p = lane_flag(hp.dist >= 0.f) & lane_flag(cp != a.free_id);
  const float dp = hit_p ? hp.dist * a.voxel_size : -1.f;
  int code, draw, colour_id, from_cat = 0;
  float shade_depth = dp;
  if (DIFF) {
    const RmHit hg = rm_cast<MaskT>(rs, masks + ((long)a.B + b) * pillars, a.X, a.Y, a.Z, live);
    const int cg = rm_class_at(a.sem_gt, a.gt_i64, b * cells + ((long)hg.x * a.Y + hg.y) * a.Z + hg.z);
    const int hit_g = lane_flag(hg.dist >= 0.f) & lane_flag(cg != a.free_id);
    const float dg = hit_g ? hg.dist * a.voxel_size : -1.f;
    code = hit_p ? (hit_g ? (cp == cg ? (fabsf(dp - dg) < a.tol ? 1 : 2) : 3) : 4) : (hit_g ? 5 : 0);
    draw = code != 0;
    from_cat = lane_flag(code != 1);
    colour_id = from_cat ? code : (cg & 0xff);
    shade_depth = hit_p ? dp : dg;
  } else {
    code = hit_p ? (cp & 0xff) : (a.free_id & 0xff);
    draw = hit_p;
    colour_id = code;
  }
  const long pix = ((long)bv * a.h + ii) * a.w + jj;
  if (a.rgb) {
    const unsigned char* table = from_cat ? a.cat_palette : a.palette;     // both tables are legal for every colour_id met
    const unsigned char* col = table + colour_id * 3;
    const int shade = rd_shade(shade_depth, a.far);
    int bg[3] = {(a.bg_rgb >> 16) & 0xff, (a.bg_rgb >> 8) & 0xff, a.bg_rgb & 0xff};
    if (a.frames) {
      const long si = ((2l * ii + 1) * a.Hs) / (2l * a.h), sj = ((2l * jj + 1) * a.Ws) / (2l * a.w);
      const unsigned char* f = a.frames + (((long)bv * a.Hs + si) * a.Ws + sj) * 3;
      bg[0] = f[0]; bg[1] = f[1]; bg[2] = f[2];
    }
    const int c0 = col[0], c1 = col[1], c2 = col[2];
    if (live) {
      unsigned char* o = a.rgb + pix * 3;
      o[0] = (unsigned char)(draw ? ((((c0 * shade) >> 8) * a.alpha + bg[0] * (256 - a.alpha)) >> 8) : bg[0]);
      o[1] = (unsigned char)(draw ? ((((c1 * shade) >> 8) * a.alpha + bg[1] * (256 - a.alpha)) >> 8) : bg[1]);
      o[2] = (unsigned char)(draw ? ((((c2 * shade) >> 8) * a.alpha + bg[2] * (256 - a.alpha)) >> 8) : bg[2]);
    }
  }
  if (live) {
    if (a.label) a.label[pix] = (unsigned char)code;
    if (a.depth) a.depth[pix] = dp;
  }
}

template <typename MaskT, int DIFF>
__global__ __launch_bounds__(256) void occ_render_bev_kernel(const RdArgs a) {
  const long pillars = (long)a.B * a.X * a.Y;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pillars) return;
  const MaskT* masks = static_cast<const MaskT*>(a.masks);
  const unsigned mp = (unsigned)masks[p];
  const int has_p = lane_flag(mp != 0u);
  const int top_p = has_p ? 31 - __clz((int)mp) : 0;
  const int cp = rm_class_at(a.sem, a.sem_i64, p * a.Z + top_p);
  int code, draw, colour_id, from_cat = 0, top = top_p;
  if (DIFF) {
    const unsigned mg = (unsigned)masks[pillars + p];
    const int has_g = lane_flag(mg != 0u);
    const int top_g = has_g ? 31 - __clz((int)mg) : 0;
    const int cg = rm_class_at(a.sem_gt, a.gt_i64, p * a.Z + top_g);
    code = has_p ? (has_g ? (cp == cg ? (top_p == top_g ? 1 : 2) : 3) : 4) : (has_g ? 5 : 0);
    draw = code != 0;
    from_cat = lane_flag(code != 1);
    colour_id = from_cat ? code : (cg & 0xff);
    top = has_p ? top_p : top_g;
  } else {
    code = has_p ? (cp & 0xff) : (a.free_id & 0xff);
    draw = has_p;
    colour_id = code;
  }
  if (a.label) a.label[p] = (unsigned char)code;
  if (a.rgb) {
    const unsigned char* col = (from_cat ? a.cat_palette : a.palette) + colour_id * 3;
    const int shade = 128 + (128 * (top + 1)) / a.Z;
    unsigned char* o = a.rgb + p * 3;
    o[0] = (unsigned char)(draw ? (col[0] * shade) >> 8 : (a.bg_rgb >> 16) & 0xff);
    o[1] = (unsigned char)(draw ? (col[1] * shade) >> 8 : (a.bg_rgb >> 8) & 0xff);
    o[2] = (unsigned char)(draw ? (col[2] * shade) >> 8 : a.bg_rgb & 0xff);
  }
}

// one mask launch + one render launch of Kernel<MaskT, DIFF>, from the entry point's `a` (RdArgs), `workspace` and stream `st`
#define OCC_RENDER_LAUNCH(Kernel, grid)                                                                                        \
  with_mask_type(a.Z, [&](auto m) {                                                                                            \
    using MaskT = decltype(m);                                                                                                 \
    launch_pillar_masks(st, a.sem, a.sem_i64, a.sem_gt, a.gt_i64, static_cast<MaskT*>(workspace), a.B, a.X, a.Y, a.Z,          \
                        a.free_id);                                                                                            \
    if (a.sem_gt) hipLaunchKernelGGL((Kernel<MaskT, 1>), grid, dim3(256), 0, st, a);                                           \
    else hipLaunchKernelGGL((Kernel<MaskT, 0>), grid, dim3(256), 0, st, a);                                                    \
  })

// the checks shared by the two entry points, the grid's first; `what` names the caller in the message
static int render_check_common(const char* what, const void* sem, int sem_dtype, const void* sem_gt, int sem_gt_dtype,
                               const uint8_t* palette, const uint8_t* cat_palette, int free_id, int bg_rgb, const void* rgb,
                               const void* workspace, int64_t workspace_bytes, int B, int X, int Y, int Z) {
  const int rc = check_grid_args(what, sem, sem_dtype, sem_gt, sem_gt_dtype, free_id, workspace, workspace_bytes, B, INT_MAX, X,
                                 Y, Z);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_ARG((int64_t)B * X * Y <= (int64_t)1 << 30, "%s: grid %dx%dx%dx%d too large", what, B, X, Y, Z);
  OCC_CHECK_ARG(!rgb || palette, "%s: null pointer argument (palette is needed with rgb)", what);
  OCC_CHECK_ARG(!rgb || !sem_gt || cat_palette, "%s: null pointer argument (cat_palette is needed with rgb and sem_gt)", what);
  OCC_CHECK_ARG(bg_rgb >= 0 && bg_rgb <= 0xffffff, "%s: bg_rgb must be 0x000000..0xffffff (got %d)", what, bg_rgb);
  return OCC_OK;
}

}  // namespace occ

extern "C" int64_t occ_render_workspace_bytes(int B, int X, int Y, int Z, int diff) {
  return occ::pillar_mask_bytes(B, X, Y, Z, diff ? 2 : 1);
}

extern "C" int occ_render_views(const void* sem, int sem_dtype, const void* sem_gt, int sem_gt_dtype, const float* cams,
                                const uint8_t* frames, int Hs, int Ws, const uint8_t* palette, const uint8_t* cat_palette,
                                float off_x, float off_y, float off_z, float voxel_size, int free_id, float far, float tol,
                                int alpha, int bg_rgb, uint8_t* label, float* depth, uint8_t* rgb, void* workspace,
                                int64_t workspace_bytes, int B, int V, int X, int Y, int Z, int h, int w, void* stream) {
  using namespace occ;
  const int rc = render_check_common("render_views", sem, sem_dtype, sem_gt, sem_gt_dtype, palette, cat_palette, free_id, bg_rgb,
                                     rgb, workspace, workspace_bytes, B, X, Y, Z);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_ARG(cams, "render_views: null pointer argument (cams)");
  OCC_CHECK_ARG(label || depth || rgb, "render_views: null pointer argument (give at least one of label, depth, rgb)");
  OCC_CHECK_ARG(V > 0 && h > 0 && w > 0 && (int64_t)B * V <= 65535 && h <= 16384 && w <= 16384,
                "render_views: bad dimension (B=%d V=%d h=%d w=%d; B * V <= 65535, h, w <= 16384)", B, V, h, w);
  OCC_CHECK_ARG(!frames || (Hs > 0 && Ws > 0 && Hs <= 16384 && Ws <= 16384),
                "render_views: frames need a source size Hs, Ws in 1..16384 (Hs=%d Ws=%d)", Hs, Ws);
  OCC_CHECK_ARG(voxel_size > 0.f, "render_views: voxel_size must be positive");
  OCC_CHECK_ARG(far > 0.f && far <= 3.0e38f, "render_views: far must be positive and finite");
  OCC_CHECK_ARG(tol >= 0.f, "render_views: tol must not be negative");
  OCC_CHECK_ARG(alpha >= 0 && alpha <= 256, "render_views: alpha must be 0..256 (got %d)", alpha);
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(depth) % 4 == 0 && reinterpret_cast<uintptr_t>(cams) % 4 == 0,
                "render_views: depth and cams must be 4-byte aligned");
  RdArgs a{sem, sem_gt, cams, frames, palette, cat_palette, workspace, label, depth, rgb, off_x, off_y, off_z, voxel_size, far,
           tol, sem_dtype, sem_gt ? sem_gt_dtype : 0, free_id, alpha, bg_rgb, frames ? Hs : 1, frames ? Ws : 1, B, V, X, Y, Z,
           h, w};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  OCC_RENDER_LAUNCH(occ_render_views_kernel, dim3((unsigned)((w + 31) / 32), (unsigned)((h + 7) / 8), (unsigned)(B * V)));
  OCC_CHECK_LAUNCH("render_views");
  return OCC_OK;
}

extern "C" int occ_render_bev(const void* sem, int sem_dtype, const void* sem_gt, int sem_gt_dtype, const uint8_t* palette,
                              const uint8_t* cat_palette, int free_id, int bg_rgb, uint8_t* label, uint8_t* rgb,
                              void* workspace, int64_t workspace_bytes, int B, int X, int Y, int Z, void* stream) {
  using namespace occ;
  const int rc = render_check_common("render_bev", sem, sem_dtype, sem_gt, sem_gt_dtype, palette, cat_palette, free_id, bg_rgb,
                                     rgb, workspace, workspace_bytes, B, X, Y, Z);
  if (rc != OCC_OK) return rc;
  OCC_CHECK_ARG(label || rgb, "render_bev: null pointer argument (give at least one of label, rgb)");
  RdArgs a{sem, sem_gt, nullptr, nullptr, palette, cat_palette, workspace, label, nullptr, rgb, 0.f, 0.f, 0.f, 1.f, 1.f, 0.f,
           sem_dtype, sem_gt ? sem_gt_dtype : 0, free_id, 256, bg_rgb, 1, 1, B, 1, X, Y, Z, 1, 1};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  OCC_RENDER_LAUNCH(occ_render_bev_kernel, dim3((unsigned)(((long)B * X * Y + 255) / 256)));
  OCC_CHECK_LAUNCH("render_bev");
  return OCC_OK;
}
#undef OCC_RENDER_LAUNCH
