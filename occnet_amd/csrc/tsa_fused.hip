// Fused temporal self-attention gather for gfx950 (single BEV level, 2-deep queue).
//
// Replaces (reference: projects/mmdet3d_plugin/bevformer/modules/temporal_self_attention.py):
//   :206-222  view/softmax of the offsets/weights Linear outputs and the (bs*2) permutes
//   :224-228  sampling_locations = ref_2d + offsets / (W, H)
//   :240-253  ms_deform_attn_forward on (bs*2, Nq) rows
//   :255-262  permute + mean over the two queue entries
// One 64-lane wave owns one BEV query: lane = m*8 + t*4 + p resolves exactly one sample
// (head m, queue entry t, point p); softmax is a 4-lane shuffle; every 8-lane group then gathers
// its head's 8 samples (32 x 16-byte loads per lane) from the two queue entries' value maps and
// writes the mean.  When there is no history BEV the reference stacks the current BEV twice:
// pass value_bt_stride = 0 and the two entries alias one projected buffer.
//
// tsa_fused_q16_kernel (occ_tsa_fused_forward_q16v; opt-in, OCC_TSA_VALUES=q16): the same gather over q16 value rows (block
// floating point, common.h fma8q) in the pixel-pair layout of the 16-bit SCA gather, [b*2+t][pix >> 1][head][pix & 1][32]
// int16: a head row is 64 bytes = 4 lanes x 16 bytes where the fp32 row is 128 bytes = 8 lanes.  The set-up is the fp32
// kernel's (tsa_lane_setup, one sample per lane, the slab in LDS).  The gathering lanes then are
//     lane = head * 8 + piece * 2 + t :   the 4 samples of (head, queue entry t), 8 channels (piece) of each corner row,
// 16 16-byte buffer loads per lane (gather_samples_buf_h<4, 4, true>: all 16 in flight) where the fp32 kernel has 32; the two
// queue halves of a piece sit in neighbouring lanes and are combined by ONE exchange step (lane t keeps channels 4 t .. 4 t + 3
// of the piece and sends the other four), after which lane l holds floats 4 l .. 4 l + 3 of the query's output row: the 1 KB
// row is written by one linear wave store.  t is a LANE index here, so the two queue entries cannot have a descriptor each (a
// per-lane descriptor makes hipcc serialise every load in a waterfall loop): ONE descriptor spans both padded maps of the batch
// entry, value_bt_stride elements apart (one map when they alias), and the set-up adds t * stride to the sample's offsets.  A
// corner outside the map still carries kOobOffset — the launcher keeps stride + map below it, so it stays out of the
// descriptor's range: the load returns 0 and requests nothing; in-map corners never leave their own map.  (Two queries per
// wave with both entries per lane would keep per-map descriptors but needs two set-up passes per wave and the 32-load
// register window again.)  The sums carry 2^15 * s / 2 (s = the range scale the rows were stored with): divided out together
// with the 0.5 of the queue mean, all powers of two.
// hipcc -O3 for gfx950 (-Rpass-analysis=kernel-resource-usage) on tsa_fused_q16_kernel: 96 VGPRs, 0 AGPRs, 29 SGPRs, scratch 0,
// LDS 9216 bytes per block (the fp32 kernel's slab), 5 waves per SIMD; 16 buffer_load_dwordx4, none inside a waterfall loop.
// Round 6 timed a 4-lanes-per-row variant on garbage data (53.4 -> 41.3 us per launch, profiles/r06_c12_tsa_16bit_rows_timing.txt);
// what the encoders in front of it cost, and the step times with real rows: EXPERIMENTS.md, DESIGN.md section on TSA q16 rows.
#include "gather_pieces.h"

namespace occ {

constexpr int kTsaWaves = 4;

__global__ __launch_bounds__(256) void tsa_fused_kernel(
    const float* __restrict__ value, long value_bt_stride, const float* __restrict__ offs,
    long offs_stride, const float* __restrict__ logits, long logits_stride,
    const float* __restrict__ ref_2d, const int32_t* __restrict__ order, float* __restrict__ out,
    int B, int Nq, int bev_h, int bev_w) {
  constexpr int M = 8, D = 32, P = 4, NS = 2 * P;  // samples per head
  constexpr int NSp = NS + 1;
  __shared__ __attribute__((aligned(16))) SampleParamB smem[kTsaWaves * M * NSp];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long wg = (long)blockIdx.x * kTsaWaves + wave;
  if (wg >= (long)B * Nq) return;
  const int b = (int)(wg / Nq);
  const int r = (int)(wg - (long)b * Nq);
  const int q = order ? order[r] : r;
  SampleParamB* sp = smem + wave * M * NSp;
  constexpr int row_stride = M * D;

  // lane = m*8 + t*4 + p : exactly the memory order of both Linear outputs (set-up shared with the backward: gather_pieces.h)
  const int m = lane >> 3, t = (lane >> 2) & 1;
  float aw, lx, ly;
  tsa_lane_setup(logits, logits_stride, offs, offs_stride, ref_2d, (long)b * Nq + q, lane, b, t, q, Nq, bev_h, bev_w, aw, lx, ly);
  // corners outside the BEV map carry an out-of-range byte offset: the buffer load returns 0 without a request (no
  // dummy load of row 0, no 0 * Inf)
  SampleParamB p;
  bilinear_setup_b(lx, ly, aw, bev_h, bev_w, 0, (unsigned)row_stride * 4u, kOobOffset, 1, p);
  sp[m * NSp + (lane & 7)] = p;
  wave_lds_sync();

  const int g = lane >> 3, c4 = lane & 7;
  const unsigned map_bytes = (unsigned)bev_h * (unsigned)bev_w * (unsigned)row_stride * 4u;
  const __amdgpu_buffer_rsrc_t r0 = uniform_rsrc(value + ((long)b * 2 + 0) * value_bt_stride, map_bytes);
  const __amdgpu_buffer_rsrc_t r1 = uniform_rsrc(value + ((long)b * 2 + 1) * value_bt_stride, map_bytes);
  const unsigned lane_off = (unsigned)(g * D + c4 * 4) * 4u;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  a0 = gather_samples_buf<4>(r0, lane_off, sp + g * NSp, P, a0);
  a1 = gather_samples_buf<4>(r1, lane_off, sp + g * NSp + P, P, a1);
  float4 o4 = make_float4((a0.x + a1.x) * 0.5f, (a0.y + a1.y) * 0.5f, (a0.z + a1.z) * 0.5f,
                          (a0.w + a1.w) * 0.5f);
  *reinterpret_cast<float4*>(out + ((long)b * Nq + q) * row_stride + g * D + c4 * 4) = o4;
}

// q16 value rows in the pixel-pair layout (header).  value_bt_stride in int16 elements; map_rows = the padded (even) row count.
__global__ __launch_bounds__(256) void tsa_fused_q16_kernel(
    const short* __restrict__ value, long value_bt_stride, const float* __restrict__ offs,
    long offs_stride, const float* __restrict__ logits, long logits_stride,
    const float* __restrict__ ref_2d, const int32_t* __restrict__ order, float* __restrict__ out,
    int B, int Nq, int bev_h, int bev_w, int map_rows, const float* __restrict__ value_scale) {
  constexpr int M = 8, D = 32, P = 4, NS = 2 * P;
  constexpr int NSp = NS + 1;
  __shared__ __attribute__((aligned(16))) SampleParamB smem[kTsaWaves * M * NSp];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long wg = (long)blockIdx.x * kTsaWaves + wave;
  if (wg >= (long)B * Nq) return;
  const int b = (int)(wg / Nq);
  const int r = (int)(wg - (long)b * Nq);
  const int q = order ? order[r] : r;
  SampleParamB* sp = smem + wave * M * NSp;
  constexpr int row_stride = M * D;

  // set-up: lane = m*8 + t*4 + p, as in tsa_fused_kernel
  const int m = lane >> 3, t = (lane >> 2) & 1;
  float aw, lx, ly;
  tsa_lane_setup(logits, logits_stride, offs, offs_stride, ref_2d, (long)b * Nq + q, lane, b, t, q, Nq, bev_h, bev_w, aw, lx, ly);
  SampleParamB p;
  bilinear_setup_b(lx, ly, aw, bev_h, bev_w, 0, (unsigned)row_stride * 2u, kOobOffset, 1, p);
  // pixel pairs (the transform of OCC_SCA16_RESOLVE: pix * 512 -> (pix >> 1) * 1024 + (pix & 1) * 64, the marker stays out
  // of range), then the lane's queue entry: t * stride bytes inside the one descriptor
  const unsigned t_off = (unsigned)t * (unsigned)value_bt_stride * 2u;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) p.o[kk] = ((p.o[kk] & ~1023u) | ((p.o[kk] >> 3) & 64u)) + t_off;
  sp[m * NSp + (lane & 7)] = p;
  wave_lds_sync();

  // gather: lane = head*8 + piece*2 + t
  const int g = lane >> 3, piece = (lane >> 1) & 3, tt = lane & 1;
  const unsigned map_bytes = (unsigned)map_rows * (unsigned)row_stride * 2u;
  const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(value + (long)b * 2 * value_bt_stride,
                                                 (unsigned)value_bt_stride * 2u + map_bytes);
  const unsigned lane_off = (unsigned)(g * 128 + piece * 16);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), acc2 = acc;
  gather_samples_buf_h<P, 4, true>(rs, lane_off, sp + g * NSp + tt * P, acc, acc2);
  // lane t keeps channels 4 t .. 4 t + 3 of the piece and receives the other queue entry's sum of them
  const int hi = lane_flag(tt != 0);
  const float4 keep = hi ? acc2 : acc, send = hi ? acc : acc2;
  // 1 / (2^15 * s / 2 * 2): exact, s is a power of two (|log2 s| <= 100)
  const float rinv = fdiv(1.f, (value_scale != nullptr ? *value_scale : 1.f) * 32768.f);
  const float4 o4 = make_float4((keep.x + __shfl_xor(send.x, 1)) * rinv, (keep.y + __shfl_xor(send.y, 1)) * rinv,
                                (keep.z + __shfl_xor(send.z, 1)) * rinv, (keep.w + __shfl_xor(send.w, 1)) * rinv);
  *reinterpret_cast<float4*>(out + ((long)b * Nq + q) * row_stride + lane * 4) = o4;
}


}  // namespace occ

extern "C" int occ_tsa_fused_forward_f32(const float* value, int64_t value_bt_stride,
                                         const float* offs, int64_t offs_stride,
                                         const float* logits, int64_t logits_stride,
                                         const float* ref_2d, const int32_t* order, float* out,
                                         int B, int Nq, int bev_h, int bev_w, int M, int D, int P,
                                         void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(value && offs && logits && ref_2d && out, "tsa_fused_forward: null pointer argument");
  OCC_CHECK_ARG(B > 0 && Nq > 0 && bev_h > 0 && bev_w > 0, "tsa_fused_forward: bad dimension");
  OCC_CHECK_ARG((long)bev_h * bev_w * M * D * 4 < (long)occ::kOobOffset, "tsa_fused_forward: BEV map too large");
  OCC_CHECK_ARG(value_bt_stride >= 0, "tsa_fused_forward: negative value stride");
  OCC_CHECK_ARG(offs_stride >= (int64_t)M * 2 * P * 2 && logits_stride >= (int64_t)M * 2 * P,
                "tsa_fused_forward: row strides smaller than a row");
  // the kernel reads an offsets row and a reference point as float2, a value row as float4 pieces, and writes float4
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(offs) % 8 == 0, "tsa_fused_forward: offs must be 8-byte aligned");
  OCC_CHECK_ARG(offs_stride % 2 == 0, "tsa_fused_forward: offs row stride must be even");
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(value) % 16 == 0 && value_bt_stride % 4 == 0,
                "tsa_fused_forward: value must be 16-byte aligned");
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(ref_2d) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
                "tsa_fused_forward: ref_2d must be 8-byte aligned, out 16-byte aligned");
  OCC_CHECK_ARG((long)bev_h * bev_w * M * D < (1L << 31), "tsa_fused_forward: value map too large");
  if (M != 8 || D != 32 || P != 4) {
    set_error("tsa_fused_forward: no fused kernel for M=%d D=%d P=%d", M, D, P);
    return OCC_E_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long waves = (long)B * Nq;
  const long blocks = (waves + kTsaWaves - 1) / kTsaWaves;
  hipLaunchKernelGGL(tsa_fused_kernel, dim3((unsigned)blocks), dim3(256), 0, st, value,
                     (long)value_bt_stride, offs, (long)offs_stride, logits, (long)logits_stride,
                     ref_2d, order, out, B, Nq, bev_h, bev_w);
  OCC_CHECK_LAUNCH("tsa_fused_forward");
  return OCC_OK;
}

extern "C" int occ_tsa_fused_forward_q16v(const void* value_q16, int64_t value_bt_stride, int value_rows,
                                          const float* offs, int64_t offs_stride, const float* logits,
                                          int64_t logits_stride, const float* ref_2d, const int32_t* order,
                                          float* out, int B, int Nq, int bev_h, int bev_w, int M, int D, int P,
                                          const float* value_scale, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(value_q16 && offs && logits && ref_2d && out, "tsa_fused_forward_q16v: null pointer argument");
  OCC_CHECK_ARG(B > 0 && Nq > 0 && bev_h > 0 && bev_w > 0 && M > 0 && D > 0, "tsa_fused_forward_q16v: bad dimension");
  const long pix = (long)bev_h * bev_w;
  // pixel pairs: the maps hold an even number of rows (the pad row of an odd map is never sampled)
  OCC_CHECK_ARG(value_rows % 2 == 0 && value_rows == pix + (pix & 1),
                "tsa_fused_forward_q16v: value_rows must be bev_h*bev_w rounded up to even");
  const long map_elems = (long)value_rows * M * D;
  OCC_CHECK_ARG(value_bt_stride == 0 || value_bt_stride >= map_elems,
                "tsa_fused_forward_q16v: value stride must be 0 (aliased queue entries) or at least one padded map");
  // one descriptor spans both maps of a batch entry; the out-of-range marker (+ the lane's piece) must stay beyond it
  OCC_CHECK_ARG((value_bt_stride + map_elems) * 2 < (long)occ::kOobOffset - 1024, "tsa_fused_forward_q16v: BEV map too large");
  OCC_CHECK_ARG(offs_stride >= (int64_t)M * 2 * P * 2 && logits_stride >= (int64_t)M * 2 * P,
                "tsa_fused_forward_q16v: row strides smaller than a row");
  // the kernel reads an offsets row and a reference point as float2, 16-byte pieces of value rows, and writes float4
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(offs) % 8 == 0, "tsa_fused_forward_q16v: offs must be 8-byte aligned");
  OCC_CHECK_ARG(offs_stride % 2 == 0, "tsa_fused_forward_q16v: offs row stride must be even");
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(value_q16) % 16 == 0 && value_bt_stride % 8 == 0,
                "tsa_fused_forward_q16v: value must be 16-byte aligned");
  OCC_CHECK_ARG(reinterpret_cast<uintptr_t>(ref_2d) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0,
                "tsa_fused_forward_q16v: ref_2d must be 8-byte aligned, out 16-byte aligned");
  if (M != 8 || D != 32 || P != 4) {
    set_error("tsa_fused_forward_q16v: no fused kernel for M=%d D=%d P=%d", M, D, P);
    return OCC_E_UNSUPPORTED;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long waves = (long)B * Nq;
  const long blocks = (waves + kTsaWaves - 1) / kTsaWaves;
  hipLaunchKernelGGL(tsa_fused_q16_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                     reinterpret_cast<const short*>(value_q16), (long)value_bt_stride, offs, (long)offs_stride, logits,
                     (long)logits_stride, ref_2d, order, out, B, Nq, bev_h, bev_w, value_rows, value_scale);
  OCC_CHECK_LAUNCH("tsa_fused_forward_q16v");
  return OCC_OK;
}
