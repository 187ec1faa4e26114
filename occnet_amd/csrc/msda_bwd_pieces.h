// The blocks of the binned grad_value pipeline (msda_backward.hip: count -> scan -> fill -> replay) that two kernels must keep
// the same, once.  The wave-aggregated and the block-aggregated binning kernels must emit the SAME row items (the second is the
// default, the first the fallback for a level whose histogram does not fit), and both replay kernels must resolve a work entry
// to the same 32 pixels and walk its items the same way.  Included by msda_backward.hip only.
// A piece is a __forceinline__ function where that leaves every kernel's device code the parent's (the two row addresses), and
// TEXT otherwise: a macro on the enclosing kernel's locals, for the reason given in conv3x3_kloop.h and gather_pieces.h (hipcc
// simplifies a callee before it inlines it; EXPERIMENTS.md section 8v lists what each piece did as a function).  The
// predicates keep the 0 / 1 lane_flag form (common.h); no piece has a `bool` predicate of its own.  What differs between two
// kernels stays written out in them: wave ballot aggregation against the LDS histogram with its two-phase slot, the SCA source
// of location and weight, the accumulate step and the epilogue of each replay.
#pragma once
#include "common.h"

namespace occ {

constexpr int kBinPix = 32;                            // pixels per bin

struct BwdItem { int qpl; float w0, w1; };            // (query << 5 | pixel in bin), left / right corner weight

// ---- the binning kernels ---------------------------------------------------------------------------------------------------
// level l of `shapes`: declares binoff = its first bin inside a (batch, head), H, W = its size.  shapes, l
#define OCC_BWD_LEVEL                                                                                                  \
  int binoff = 0, H = 0, W = 0;                                                                                        \
  for (int i = 0; i <= l; ++i) {                                                                                       \
    H = (int)shapes[2 * i]; W = (int)shapes[2 * i + 1];                                                                \
    if (i < l) binoff += (H * W + kBinPix - 1) / kBinPix;                                                              \
  }

// The row items of one sample: per bilinear row r (top, bottom) one item at the bin of its left pixel (of the right one when
// the left is outside the map) with the two corner weights i0, i1, already multiplied by the attention weight a; when the
// pair straddles a bin edge (`split`, 1 in 32) two single items instead: {in, i0, 0} in `bin` and {0, wr, 0} in bin + 1.
// The record of an item of query q is BwdItem{(q << 5) | in, i0, i1}.
// OCC_BWD_ROW_EDGES declares the sample's terms (ok, h_low, w_low, lh, lw, hh, hw) and column flags (l_ok, r_ok, both) from
// BilinearTerms t and W; OCC_BWD_ROW_ITEM(r, VALID, BIN, IN, SPLIT, I0, I1, WR) then assigns row r's item to the named
// lvalues (VALID and SPLIT: 0 / 1 lane flags, common.h lane_flag).  a, H, W
#define OCC_BWD_ROW_EDGES                                                                                              \
  const int ok = t.adm;                                                                                                \
  const int h_low = t.h_low, w_low = t.w_low;                                                                          \
  const float lh = t.lh, lw = t.lw, hh = t.hh, hw = t.hw;                                                              \
  const int l_ok = lane_flag(w_low >= 0), r_ok = lane_flag(w_low + 1 <= W - 1);                                        \
  const int both = l_ok & r_ok;
#define OCC_BWD_ROW_ITEM(r, VALID, BIN, IN, SPLIT, I0, I1, WR)                                                         \
  {                                                                                                                    \
    const int hy = h_low + r;                                                                                          \
    VALID = ok & lane_flag(hy >= 0) & lane_flag(hy <= H - 1);                                                          \
    const float wy = (r ? lh : hh) * a;                                                                                \
    const float w_l = l_ok ? wy * hw : 0.f, w_r = r_ok ? wy * lw : 0.f;                                                \
    const int pl = hy * W + (l_ok ? w_low : w_low + 1);                                                                \
    BIN = VALID ? pl / kBinPix : 0;                                                                                    \
    IN = pl - BIN * kBinPix;                                                                                           \
    SPLIT = VALID & both & lane_flag(IN == kBinPix - 1);                                                               \
    I0 = l_ok ? w_l : w_r;                                                                                             \
    I1 = (both & (SPLIT ^ 1)) ? w_r : 0.f;                                                                             \
    WR = w_r;                                                                                                          \
  }

// ---- the replay kernels ----------------------------------------------------------------------------------------------------
// declares wk = the block's work-list entry {bin, first item, last item + 1, tag} and bin_g, beg, end = its first three
// fields; the grid is an upper bound of the work list, so the blocks behind it leave.  work, work_count
#define OCC_BWD_WORK_ENTRY                                                                                             \
  if ((int)blockIdx.x >= work_count[0]) return;                                                                        \
  const int4 wk = work[blockIdx.x];                                                                                    \
  const long bin_g = wk.x;                                                                                             \
  const int beg = wk.y, end = wk.z;

// the inverse of OCC_BWD_LEVEL: global bin bin_g -> declares batch entry b, head m, level l, bin bl inside the level, HW = the
// level's pixels; l == L for the slack bins of the upper bound bins_per_bm (never filled).  bin_g, shapes, bins_per_bm, M, L
#define OCC_BWD_BIN_REF                                                                                                \
  const long bm = bin_g / bins_per_bm;                                                                                 \
  int bl = (int)(bin_g - bm * bins_per_bm);                                                                            \
  const int m = (int)(bm % M);                                                                                         \
  const long b = bm / M;                                                                                               \
  int l = 0, HW = 0;                                                                                                   \
  for (; l < L; ++l) {                                                                                                 \
    HW = (int)shapes[2 * l] * (int)shapes[2 * l + 1];                                                                  \
    const int nb = (HW + kBinPix - 1) / kBinPix;                                                                       \
    if (bl < nb) break;                                                                                                \
    bl -= nb;                                                                                                          \
  }

// channel ch of the output-gradient rows of batch entry b, head m: + q * M * 32 for query q (bdiv: msda_bwd_bins.h)
__device__ __forceinline__ const float* bwd_go_row(const float* grad_out, long b, int bdiv, int Lq, int M, int m, int ch) {
  return grad_out + ((b / bdiv) * Lq * (long)M + m) * 32 + ch;
}

// the 32 grad_value channels of head m in pixel row `row` = b * S + the pixel's index in the batch entry
__device__ __forceinline__ float* bwd_gv_row(float* grad_value, long row, int M, int m) {
  return grad_value + (row * M + m) * 32;
}

// The items [beg, end) of a work entry, dealt round-robin to the block's 8 half-waves (hw), 8 per half-wave and step,
// software-pipelined over three steps: the item records of step i+2 and the output-gradient rows of step i+1 are in flight
// while step i is accumulated (two dependent global loads per item made every step cost both latencies: ~1.5 us per 64 items
// and block).  The argument is the kernel's accumulate step for one item: pixel pl of the bin gets g * w0, pixel pl + 1 gets
// g * w1 (w1 == 0 for single items: pixel 32 is a dummy row); pl, g, w0, w1 name the item (g, w0, w1 as references, which keeps
// the parent's order of the register reads).  items, go, beg, end, hw, M, D
#define OCC_BWD_REPLAY_ITEMS(...)                                                                                      \
  int qA[8], qB[8], qC[8];                                                                                             \
  float w0A[8], w1A[8], w0B[8], w1B[8], w0C[8], w1C[8], gA[8], gB[8];                                                  \
  _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                                      \
    const int i0 = beg + hw + 8 * u, i1 = i0 + 64;                                                                     \
    const BwdItem a = items[i0 < end ? i0 : beg];                                                                      \
    const BwdItem c = items[i1 < end ? i1 : beg];                                                                      \
    qA[u] = i0 < end ? a.qpl : -1; w0A[u] = a.w0; w1A[u] = a.w1;                                                       \
    qB[u] = i1 < end ? c.qpl : -1; w0B[u] = c.w0; w1B[u] = c.w1;                                                       \
  }                                                                                                                    \
  _Pragma("unroll") for (int u = 0; u < 8; ++u) gA[u] = go[(long)(qA[u] < 0 ? 0 : qA[u] >> 5) * M * D];                \
  for (int base = beg; base < end; base += 64) {                                                                       \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) { /* item records two steps ahead */                                 \
      const int idx = base + 128 + hw + 8 * u;                                                                         \
      const BwdItem it = items[idx < end ? idx : beg];                                                                 \
      qC[u] = idx < end ? it.qpl : -1; w0C[u] = it.w0; w1C[u] = it.w1;                                                 \
    }                                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) /* rows one step ahead */                                            \
      gB[u] = go[(long)(qB[u] < 0 ? 0 : qB[u] >> 5) * M * D];                                                          \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                                    \
      if (qA[u] >= 0) {                                                                                                \
        const int pl = qA[u] & 31;                                                                                     \
        const float &g = gA[u], &w0 = w0A[u], &w1 = w1A[u];                                                            \
        __VA_ARGS__                                                                                                    \
      }                                                                                                                \
    }                                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                                    \
      qA[u] = qB[u]; w0A[u] = w0B[u]; w1A[u] = w1B[u]; gA[u] = gB[u];                                                  \
      qB[u] = qC[u]; w0B[u] = w0C[u]; w1B[u] = w1C[u];                                                                 \
    }                                                                                                                  \
  }

}  // namespace occ
