// The binned, atomic-free grad_value machinery of msda_backward.hip (count -> scan -> fill -> replay, see its file header),
// shared with the fused SCA backward (sca_fused_backward.hip).
#pragma once
#include <cstdlib>
#include "common.h"

namespace occ {

// OCC_MSDA_BWD_DETERMINISTIC=1: the order-independent fixed-point replay (bit-identical grad_value from run to run).  Read per
// call (tests switch it inside one process) by the msda, fused SCA and fused TSA backward.
inline bool bwd_deterministic() {
  const char* e = getenv("OCC_MSDA_BWD_DETERMINISTIC");
  return e != nullptr && e[0] == '1';
}

struct BwdWsLayout { size_t off_cnt, off_cur, off_work, off_items, off_meta, off_tiles, off_aux, bytes; long n_bins, n_samples, max_items, work_cap, max_split; int bins_per_bm; bool ok; };
// scratch of the binned path for B value batch entries of S pixels, M heads, L levels, Lq queries of P points each
BwdWsLayout bwd_ws_layout(int B, int S, int M, int L, int Lq, int P);
// true when the block-aggregated binning passes take these shapes (their LDS histogram holds the largest level's bins)
bool bwd_block_bins_fit(int B, int S, int M, int L, int Lq, int P);

// Where the binning passes of the fused SCA backward take a sample from (its items have no precomputed location):
// value batch entry bv = b * NC + c, query q, head m, level l, point p ->
//   location = ref_cam[c][b][q][p % Z] + oxy[b][q][m][l][p],  weight = aw[b][q][m][l][p] (softmax / camera count),
//   only where bit c of vis_bits[0][q] is set (batch 0's mask picks the cameras).
struct ScaBinSource {
  const float* ref_cam;
  const float* oxy;
  const float* aw;
  const uint32_t* vis_bits;
  int NC, B, Z;
};

// Count -> scan -> fill -> replay into grad_value (B value batch entries; accumulated: the caller zeroes it).  Items come from
// loc / attn / nzflag (ms_deform_attn layout) or, with `sca`, from the fused SCA gather's source; the output-gradient row of an
// item of batch entry bv and query q is grad_out[((bv / NC) * Lq + q) * M + m][0 .. 31]; without `sca`, NC is loc_batch_div
// (1: one grad row per value batch entry, the msda backward; 2: the fused TSA backward, whose two queue entries of a batch
// share the batch's grad row).  grad_out_n: floats in grad_out (the deterministic mode's range scan).  The flags / counts of
// the workspace must arrive zeroed.
int bwd_bins_replay(const BwdWsLayout& w, char* ws, bool deterministic, const int64_t* shapes, const int64_t* lstart,
                    const float* loc, const float* attn, const ScaBinSource* sca, const float* grad_out, long grad_out_n,
                    float* grad_value, int B, int S, int M, int L, int Lq, int P, hipStream_t st, int loc_batch_div = 1);

}  // namespace occ
