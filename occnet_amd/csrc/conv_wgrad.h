// Shared by the bf16 weight-gradient kernels of the backbone's convolutions (conv1x1_wgrad_bf16.hip, conv3x3_wgrad_bf16.hip):
// the register-only fragment builder and the launcher of the fixed-order reduce over the split-range workspace.
#pragma once
#include "common.h"

namespace occ {

// 8 dwords (pixel j: channel 2c in the low half, 2c + 1 in the high half) -> the fragments of the even and the odd channel
__device__ __forceinline__ void cw_frag(const unsigned (&v)[8], bf16x8& even, bf16x8& odd) {
  occ_u32x4 e, o;
  e.x = __builtin_amdgcn_perm(v[1], v[0], 0x05040100u); o.x = __builtin_amdgcn_perm(v[1], v[0], 0x07060302u);
  e.y = __builtin_amdgcn_perm(v[3], v[2], 0x05040100u); o.y = __builtin_amdgcn_perm(v[3], v[2], 0x07060302u);
  e.z = __builtin_amdgcn_perm(v[5], v[4], 0x05040100u); o.z = __builtin_amdgcn_perm(v[5], v[4], 0x07060302u);
  e.w = __builtin_amdgcn_perm(v[7], v[6], 0x05040100u); o.w = __builtin_amdgcn_perm(v[7], v[6], 0x07060302u);
  even = __builtin_bit_cast(bf16x8, e);
  odd = __builtin_bit_cast(bf16x8, o);
}

// dw[i] = sum over c < chunks of part[c * OI + i] in a fixed order, rounded once to f32 or (dw_bf16) bf16: launches
// conv1x1_wgrad_reduce_kernel (conv1x1_wgrad_bf16.hip), which only sees OI flat outputs per range.  Returns the launch status.
hipError_t conv_wgrad_reduce_launch(const float* part, void* dw, long OI, int chunks, int dw_bf16, hipStream_t st);

}  // namespace occ
