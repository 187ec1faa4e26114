// The pass loop of the activation-resident 1x1 convolution (conv1x1_resident_bf16.hip has the structure), as TEXT:
// conv1x1_resident_kernel and phase 2 of conv3x3_conv1x1_kernel both expand these macros, so the two sum the same products
// in the same order and round once at the same place by construction.  Macros on the kernel's locals and not __device__
// functions, for the reason given in conv3x3_kloop.h.
//
// A (32 RT) x K bf16 tile lies at `lds`, 16-byte pieces XOR-swizzled by row (slot s of row r holds piece s ^ (r & MASK)); the
// four waves' scratch and the f32 bias of the block's columns follow it (c1r_lds_bytes).  The kernel expands, in this order,
// OCC_C1R_RING and three OCC_C1R_LOADs of the first pass; OCC_C1R_RES_START (ring and residual requests travel under whatever
// the kernel still does in front of its barrier); and, behind the barrier after which tile and bias are in LDS,
// OCC_C1R_PASSES.  OCC_C1R_AFRAG_STATE goes anywhere in front of OCC_C1R_PASSES.  They expect in scope
//   K, RT, NTW, RD              constants: input channels, row tiles, 32-column tiles per wave and pass, residual tiles in flight
//   PITCH, KS, MASK, NTILES     constants: 2 K, K / 16, min(K / 8, 32) - 1, RT * NTW
//   N                           output channels
//   lds, scratch, sbias         char*: the tile; char*: this wave's kC1rScratch bytes; float*: the bias, first column of
//                               pass OCC_C1R_P_BEGIN first
//   residual, out               const unsigned short*, unsigned short*
//   wave, lane, vi, kb          tid >> 6, tid & 63, lane & 31, lane >> 5
// and the kernel's own macros, expanded where the statements stand:
//   OCC_C1R_P_BEGIN, OCC_C1R_P_END    the block's passes (128 NTW columns each)
//   OCC_C1R_RESIDUAL, OCC_C1R_RELU    whether a residual is added / the ReLU applied
//   OCC_C1R_RES_ROW(RTI, J)           declares what OCC_C1R_RES_PIXEL, a long expression, is made of: the residual's pixel for
//                                     tile row 32 RTI + 16 J + (rlane >> 2), clamped into the map.  (Two parts, and an
//                                     expression where OCC_C1R_OUT_ROW has a variable: the statement order of both parents.)
//   OCC_C1R_OUT_ROW(RTI, J)           declares `const long orow`, `const bool olive`: the output pixel of tile row
//                                     32 RTI + 16 J + erow and whether it exists
//   OCC_C1R_PASS_LOCALS               what the kernel wants computed once per pass for OCC_C1R_OUT_ROW, behind the opaque
//                                     erow (may be empty)
#pragma once
#include "common.h"

namespace occ {

constexpr int kC1rPitch = 80, kC1rScratch = 32 * kC1rPitch;     // per-wave epilogue scratch: 32 rows x 64 B, padded

// LDS: activation tile + the four waves' scratch + the bias of the block's columns
constexpr int c1r_lds_bytes(int K, int RT, int bias_cols) { return 32 * RT * K * 2 + 4 * kC1rScratch + bias_cols * 4; }

}  // namespace occ

// weight ring: slot (step & 3) = the wave's NTW column tiles of flat step = pass * KS + k-step (buffer loads: one
// lane-offset VGPR for all of them, the step's offset in an SGPR, the tile in the immediate) of the conv1x1_pack_weight
// buffer WP
#define OCC_C1R_RING(WP)                                                                          \
  occ_u32x4 w[4][NTW];                                                                            \
  const __amdgpu_buffer_rsrc_t wrs = uniform_rsrc(WP, (unsigned)K * (unsigned)N * 2u);            \
  const int wv = (wave * NTW * 64 + lane) * 16;                                                   \
  const int kstep_bytes = (N / 32) * 1024;
#define OCC_C1R_LOAD(SLOT, PASS, KSTEP)                                                           \
  {                                                                                               \
    const int so = (KSTEP) * kstep_bytes + (PASS) * (4 * NTW * 1024);                             \
    _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                               \
      w[SLOT][t] = __builtin_amdgcn_raw_buffer_load_b128(wrs, wv + t * 1024, so, 0);              \
  }
// activation fragments of k-step ks (the same for every pass): double buffered, read one step ahead.  Slot of piece
// 2 ks + kb in row vi = (2 ks) ^ ((kb ^ vi) & MASK): one XOR per step on an address the compiler cannot see through
#define OCC_C1R_AFRAG_STATE                                                                       \
  bf16x8 af[2][RT];                                                                               \
  unsigned abase = (unsigned)(vi * PITCH + ((kb ^ vi) & MASK) * 16);
#define OCC_C1R_AFRAG(BUF, KSTEP)                                                                 \
  {                                                                                               \
    asm volatile("" : "+v"(abase));                                                               \
    const char* ap = lds + (abase ^ (unsigned)((KSTEP) * 32));                                    \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                             \
      af[BUF][rt] = *reinterpret_cast<const bf16x8*>(ap + rt * (32 * PITCH));                     \
  }
// residual row segments of tile (rt, t) of the pass whose first column (for this wave) is NW: lane -> rows (lane >> 2)
// and + 16 of the tile, 16-byte piece lane & 3
#define OCC_C1R_RES(DST, NW, RTI, TI)                                                             \
  {                                                                                               \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                               \
      OCC_C1R_RES_ROW(RTI, j)                                                                     \
      DST[j] = *reinterpret_cast<const uint4*>(residual + (OCC_C1R_RES_PIXEL) * N + (NW) + (TI) * 32 + (rlane & 3) * 8); \
    }                                                                                             \
  }
// the residual runs RD tiles ahead of the epilogue, across passes: rq[0] is the tile the epilogue takes next
#define OCC_C1R_RES_START                                                                         \
  uint4 rq[RD][2];                                                                                \
  int rlane = lane;                                                                               \
  if (OCC_C1R_RESIDUAL) {                                                                         \
    const int nwf = (OCC_C1R_P_BEGIN) * (128 * NTW) + wave * (32 * NTW);                          \
    _Pragma("unroll") for (int i = 0; i < RD; ++i) OCC_C1R_RES(rq[i], nwf, i / NTW, i % NTW)      \
  }

// The passes.  Per pass:
//  * D[column][row]: lane (vi, kb) holds row rt * 32 + vi, register 4 q + i = column 8 q + 4 kb + i of tile t.  The
//    accumulators start at the bias;
//  * the k loop; the ring runs into the next pass (last pass: a harmless re-read).  The scheduling groups pin the software
//    pipeline (hipcc otherwise sinks every ring request down to its use: load, vmcnt(0), MFMA): MFMAs in four runs with the
//    ring request of step s + 3 (one per column tile) and the A fragments of step s + 1 between them;
//  * the epilogue, one 32 x 32 tile at a time through the wave's scratch (row pitch 80 B): residual segments in, every lane
//    adds its quads in f32, ReLU, ONE rounding, bf16 quad back in place, the rows leave as 16-byte segments.  elane is
//    opaque per pass: the epilogue's offsets are recomputed here instead of living across the k loop.
#define OCC_C1R_PASSES                                                                            \
  OCC_C1R_AFRAG(0, 0)                                                                             \
  _Pragma("unroll 1") for (int p = (OCC_C1R_P_BEGIN); p < (OCC_C1R_P_END); ++p) {                 \
    const int nw = p * (128 * NTW) + wave * (32 * NTW);         /* the wave's first column of this pass */ \
    int elane = lane;                                                                             \
    asm volatile("" : "+v"(elane));                                                               \
    f32x16 pacc[RT][NTW];                                                                         \
    _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                               \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                             \
        const float4 c0 = *reinterpret_cast<const float4*>(sbias + (nw - (OCC_C1R_P_BEGIN) * (128 * NTW)) + t * 32 + 8 * q + 4 * kb); \
        _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) {                                       \
          pacc[rt][t][4 * q + 0] = c0.x;                                                          \
          pacc[rt][t][4 * q + 1] = c0.y;                                                          \
          pacc[rt][t][4 * q + 2] = c0.z;                                                          \
          pacc[rt][t][4 * q + 3] = c0.w;                                                          \
        }                                                                                         \
      }                                                                                           \
    const int pn = p + 1 < (OCC_C1R_P_END) ? p + 1 : p;                                           \
    _Pragma("unroll") for (int ks = 0; ks < KS; ++ks) {                                           \
      if (ks + 3 < KS) OCC_C1R_LOAD((ks + 3) & 3, p, ks + 3)                                      \
      else OCC_C1R_LOAD((ks + 3) & 3, pn, ks + 3 - KS)                                            \
      OCC_C1R_AFRAG((ks + 1) & 1, (ks + 1) & (KS - 1))                                            \
      _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                           \
        _Pragma("unroll") for (int t = 0; t < NTW; ++t)                                           \
          pacc[rt][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w[ks & 3][t]), af[ks & 1][rt], \
                                                                pacc[rt][t], 0, 0, 0);            \
      if (NTILES >= 4) {                                                                          \
        constexpr int MQ = NTILES / 4, MR = NTILES - 3 * MQ;                                      \
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);                                       \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                        \
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);                                       \
        __builtin_amdgcn_sched_group_barrier(0x100, (RT + 1) / 2, 0);                             \
        __builtin_amdgcn_sched_group_barrier(0x008, MQ, 0);                                       \
        if (NTW > 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                           \
        __builtin_amdgcn_sched_group_barrier(0x008, MR, 0);                                       \
        __builtin_amdgcn_sched_group_barrier(0x100, RT / 2, 0);                                   \
      } else {                                                                                    \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                        \
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                        \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                        \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                        \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                        \
      }                                                                                           \
    }                                                                                             \
    const int erow = elane >> 2, epiece = elane & 3;                                              \
    OCC_C1R_PASS_LOCALS                                                                           \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) {                                           \
      _Pragma("unroll") for (int t = 0; t < NTW; ++t) {                                           \
        const int e = rt * NTW + t;                                                               \
        if (OCC_C1R_RESIDUAL) {                                                                   \
          const uint4 r0 = rq[0][0], r1 = rq[0][1];                                               \
          _Pragma("unroll") for (int i = 0; i + 1 < RD; ++i) { rq[i][0] = rq[i + 1][0]; rq[i][1] = rq[i + 1][1]; } \
          asm volatile("" : "+v"(rlane));                                                         \
          if (e + RD < NTILES) OCC_C1R_RES(rq[RD - 1], nw, (e + RD) / NTW, (e + RD) % NTW)        \
          else if (p + 1 < (OCC_C1R_P_END)) OCC_C1R_RES(rq[RD - 1], nw + 128 * NTW, (e + RD - NTILES) / NTW, (e + RD - NTILES) % NTW) \
          *reinterpret_cast<uint4*>(scratch + erow * kC1rPitch + epiece * 16) = r0;               \
          *reinterpret_cast<uint4*>(scratch + (erow + 16) * kC1rPitch + epiece * 16) = r1;        \
          wave_lds_sync();                                                                        \
        }                                                                                         \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                           \
          char* const sp = scratch + vi * kC1rPitch + 16 * q + 8 * kb;                            \
          float v0 = pacc[rt][t][4 * q + 0], v1 = pacc[rt][t][4 * q + 1], v2 = pacc[rt][t][4 * q + 2],  \
                v3 = pacc[rt][t][4 * q + 3];                                                      \
          if (OCC_C1R_RESIDUAL) {                                                                 \
            const uint2 r = *reinterpret_cast<const uint2*>(sp);                                  \
            v0 += bf16_lo_to_f32(r.x); v1 += bf16_hi_to_f32(r.x); v2 += bf16_lo_to_f32(r.y); v3 += bf16_hi_to_f32(r.y); \
          }                                                                                       \
          if (OCC_C1R_RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); } \
          *reinterpret_cast<uint2*>(sp) = make_uint2(pack_bf16x2_rne(v0, v1), pack_bf16x2_rne(v2, v3)); \
        }                                                                                         \
        wave_lds_sync();                                                                          \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                           \
          OCC_C1R_OUT_ROW(rt, j)                                                                  \
          const uint4 v = *reinterpret_cast<const uint4*>(scratch + (erow + 16 * j) * kC1rPitch + epiece * 16); \
          if (olive) *reinterpret_cast<uint4*>(out + orow * N + nw + t * 32 + epiece * 8) = v;    \
        }                                                                                         \
        wave_lds_sync();                                                                          \
      }                                                                                           \
    }                                                                                             \
  }
