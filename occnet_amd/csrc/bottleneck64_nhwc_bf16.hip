// One whole ResNet bottleneck with 64 mid channels (the three stride-4 blocks of the reference's ResNet-50
// `layer1`: mmdet Bottleneck, style='pytorch') as ONE kernel on NHWC bf16 activations:
//
//   c1  = relu(conv1x1(x,  W1) + b1)                      Cin -> 64          (on the tile's 10 x 18 halo)
//   c2  = relu(conv3x3(c1, W2) + b2)                      64  -> 64, pad 1
//   out = relu(conv1x1(c2, W3) + b3 + identity)           64  -> 256
//   identity = x (Cin = 256)  or  conv1x1(x, Wds) + bds (Cin = 64, first block: folded into the third GEMM
//   as 64 extra K columns, b3 := b3 + bds)
//
// NOT part of the hand-written hot path.  Why it exists: at stride 4 the 6 x 232 x 400
// pixel maps make every layer of the block HBM-bound (rocprofv3 PMC: the separate 1x1 kernels move 1.14 GB
// per block, 0.57 GB of it for 64-channel intermediates and the second read of the identity), so the only
// way down is to keep c1 / c2 in LDS: x is read as the tile's halo (+41 % overlap, mostly L2 hits) and, by this
// kernel, once more for the identity (EXPERIMENTS.md section 8q); out is written once.
//
// bottleneck64_phases.h has the block structure, the LDS layout and phases A and B, which this kernel shares as text with
// the second kernel (bottleneck64_v2_nhwc_bf16.hip; the launcher below routes to it by default).  This kernel's own:
// biases up front, a W1 ring of four slots that travels with the x prefetch, and phase C with the PIXELS as the row
// operand: wave = 4 row tiles x 2 column tiles, W3 in a ring of 4 k-steps, epilogue through the same f32 LDS transpose as
// conv1x1_nhwc_bf16.hip (bias, identity read from x a second time, ReLU, bf16).
#include "bottleneck64_phases.h"

namespace occ {

constexpr int kBnOLD = 256 + 4;              // epilogue transpose row stride (floats)

// f32 row-major weight (N, K) -> bf16 MFMA B-fragment order: packed[((ks * N/32 + nt) * 64 + lane) * 8 + j]
// = w[nt*32 + (lane & 31)][ks*16 + (lane >> 5)*8 + j]   (v_mfma_f32_32x32x16_bf16 operand of lane `lane`)
__global__ void mfma_pack_b_frag_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed,
                                        int N, int K) {
  const long n_el = (long)N * K;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_el) return;
  const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
  const long rest = idx >> 9;
  const int nts = N / 32;
  const int nt = (int)(rest % nts), ks = (int)(rest / nts);
  const int n = nt * 32 + (lane & 31), k = ks * 16 + (lane >> 5) * 8 + j;
  packed[idx] = bf16_rne(w[(long)n * K + k]);
}

template <int CIN, bool DS>
__global__ __launch_bounds__(256, 2) void bottleneck64_nhwc_bf16_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ w1p, const float* __restrict__ b1,
    const uint4* __restrict__ w2p, const float* __restrict__ b2, const uint4* __restrict__ w3p,
    const float* __restrict__ b3, unsigned short* __restrict__ out, int H, int W, int tiles_x, int tiles_y) {
  static_assert(CIN % 32 == 0 && (!DS || CIN == 64), "downsample variant keeps both x chunks in LDS");
  constexpr int NCH = CIN / 32, CQ = CIN / 8;
  __shared__ __attribute__((aligned(16))) char lds[kBnStageBytes];
  static_assert(32 * kBnOLD * 4 <= 2 * kBnXA + kBnH1, "epilogue transpose aliases the x chunks + c1 halo");
  char* const sH1 = lds + 2 * kBnXA;
  char* const sC2 = sH1 + kBnH1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  OCC_BN_TILE_DECODE(blockIdx.x)

  // ================= phase A: c1 = relu(x . W1^T + b1) on the 180 halo pixels ==========================
  OCC_BN_STAGING
  // chunk order rotated per block; the downsample variant keeps chunk c in buffer c for phase C
  const int rot = DS ? 0 : (int)((blockIdx.x * 5u) % (unsigned)NCH);

  OCC_BN_WAVE_TILES
  // Biases of this lane's channels, requested first (an in-order vmcnt wait on them later would otherwise
  // also wait for every weight prefetch issued in between)
  float4 bA[4], bB[4];
  OCC_BN_ISSUE_BIASES
  OCC_BN_ZERO_ACC(acc1, 3)
  // W1 fragments travel with the x chunk of the same index (four sets in flight): vmcnt retires in order,
  // a weight load younger than the x prefetches would drain them all
  uint4 wa[4][2];
#define OCC_BN_ISSUE_XW(S, CH) { OCC_BN_ISSUE_W1(S, CH) OCC_BN_ISSUE_X(S, CH) }
  OCC_BN_ISSUE_XW(0, OCC_BN_CH(0))
  OCC_BN_ISSUE_XW(1, OCC_BN_CH(NCH > 1 ? 1 : 0))
  if (NCH > 2) {
    OCC_BN_ISSUE_XW(2, OCC_BN_CH(NCH > 2 ? 2 : 0))
    OCC_BN_ISSUE_XW(3, OCC_BN_CH(NCH > 3 ? 3 : 0))
  }
#define OCC_BN_STEP_A(S, CI)                                                                      \
  {                                                                                               \
    char* sX = lds + ((CI) & 1) * kBnXA;                                                          \
    OCC_BN_STAGE_STORE(S, sX)                                                                     \
    OCC_BN_W1_FRAGS(S)                                                                            \
    __syncthreads();                                                                              \
    if ((CI) + 4 < NCH) OCC_BN_ISSUE_XW(S, OCC_BN_CH((CI) + 4 < NCH ? (CI) + 4 : NCH - 1))        \
    OCC_BN_STEP_MFMA(sX)                                                                          \
  }
#pragma unroll
  for (int ci = 0; ci < NCH; ci += 4) {
    OCC_BN_STEP_A(0, ci)
    if (ci + 1 < NCH) OCC_BN_STEP_A(1, ci + 1)
    if (ci + 2 < NCH) OCC_BN_STEP_A(2, ci + 2)
    if (ci + 3 < NCH) OCC_BN_STEP_A(3, ci + 3)
  }
#undef OCC_BN_STEP_A
#undef OCC_BN_ISSUE_XW

  OCC_BN_W2_PROLOGUE
  OCC_BN_WRITE_C1
  __syncthreads();

  OCC_BN_PHASE_B
  // W3 fragments (ring of 4 k-steps) in flight while c2 is written
  constexpr int KS3 = DS ? 8 : 4;
  uint4 w3r[4][2];
#define OCC_BN_ISSUE_W3(SLOT, KS)                                                                 \
  {                                                                                               \
    w3r[SLOT][0] = w3p[((long)(KS) * 8 + 2 * wave + 0) * 64 + lane];                              \
    w3r[SLOT][1] = w3p[((long)(KS) * 8 + 2 * wave + 1) * 64 + lane];                              \
  }
  OCC_BN_ISSUE_W3(0, 0)
  OCC_BN_ISSUE_W3(1, 1)
  OCC_BN_ISSUE_W3(2, 2)
  OCC_BN_ISSUE_W3(3, 3)
  OCC_BN_WRITE_C2
  __syncthreads();

  // ================= phase C: out = relu(c2 . W3^T (+ x . Wds^T) + b3 (+ x)) ==============================
  // (pixels as the row operand again: the epilogue wants D[pixel][channel])
  f32x16 acc3[4][2];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[rt][t][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS3; ++ks) {
    const bf16x8 wf0 = __builtin_bit_cast(bf16x8, w3r[ks & 3][0]);
    const bf16x8 wf1 = __builtin_bit_cast(bf16x8, w3r[ks & 3][1]);
    if (ks + 4 < KS3) OCC_BN_ISSUE_W3(ks & 3, ks + 4)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      bf16x8 af;
      OCC_BN_C_AFRAG(af, rt, ks)
      acc3[rt][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, wf0, acc3[rt][0], 0, 0, 0);
      acc3[rt][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, wf1, acc3[rt][1], 0, 0, 0);
    }
  }
#undef OCC_BN_ISSUE_W3

  // ---- epilogue, one 32-pixel row tile (two image rows) at a time through an LDS transpose -------------
  const int c = lane * 4;
  const float4 bv = *reinterpret_cast<const float4*>(b3 + c);
  float* sO = reinterpret_cast<float*>(lds);
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(x);
  // identity = x (Cin == 256): the 8 rows a wave adds in pass rt are requested one pass ahead
  uint2 rv[8], rn[8];
#define OCC_BN_ISSUE_RES(DST, RT)                                                                 \
  _Pragma("unroll") for (int rr = 0; rr < 8; ++rr) {                                              \
    DST[rr] = make_uint2(0u, 0u);                                                                 \
    if (!DS) {                                                                                    \
      const int row = wave * 8 + rr;                                                              \
      const int cy = min(y0 + 2 * (RT) + (row >> 4), H - 1), cx = min(x0 + (row & 15), W - 1);    \
      DST[rr] = *reinterpret_cast<const uint2*>(xs + (((long)img * H + cy) * W + cx) * CIN + c);  \
    }                                                                                             \
  }
  OCC_BN_ISSUE_RES(rn, 0)
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        sO[((r & 3) + 8 * (r >> 2) + 4 * kb) * kBnOLD + (wave * 2 + t) * 32 + vi] = acc3[rt][t][r];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) rv[rr] = rn[rr];
    if (rt + 1 < 4) OCC_BN_ISSUE_RES(rn, rt + 1)
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int row = wave * 8 + rr;
      const int oy = y0 + 2 * rt + (row >> 4), ox = x0 + (row & 15);
      if (oy < H && ox < W) {
        float4 v = *reinterpret_cast<const float4*>(sO + row * kBnOLD + c);
        v.x += bv.x + bf16_to_f32((unsigned short)(rv[rr].x & 0xffffu));
        v.y += bv.y + bf16_to_f32((unsigned short)(rv[rr].x >> 16));
        v.z += bv.z + bf16_to_f32((unsigned short)(rv[rr].y & 0xffffu));
        v.w += bv.w + bf16_to_f32((unsigned short)(rv[rr].y >> 16));
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        const uint2 o = make_uint2(pack_bf16x2_rne(v.x, v.y), pack_bf16x2_rne(v.z, v.w));
        *reinterpret_cast<uint2*>(out + (((long)img * H + oy) * W + ox) * 256 + c) = o;
      }
    }
  }
#undef OCC_BN_ISSUE_RES
}

}  // namespace occ

extern "C" int occ_mfma_pack_b_frag_bf16(const float* weight, void* packed, int N, int K, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(weight && packed, "mfma_pack_b_frag_bf16: null pointer argument");
  OCC_CHECK_ARG(N > 0 && K > 0, "mfma_pack_b_frag_bf16: bad dimension");
  if (N % 32 || K % 16) {
    set_error("mfma_pack_b_frag_bf16: N=%d K=%d (need N %% 32 == 0, K %% 16 == 0)", N, K);
    return OCC_E_UNSUPPORTED;
  }
  const long n = (long)N * K;
  hipLaunchKernelGGL(mfma_pack_b_frag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), weight, reinterpret_cast<unsigned short*>(packed),
                     N, K);
  OCC_CHECK_LAUNCH("mfma_pack_b_frag_bf16");
  return OCC_OK;
}

// variant: 0 = chosen here, 1 = the kernel above, 2 = the second kernel with its default tile order, 3 / 4 / 5 = the second
// kernel with tile order 0 (the first kernel's) / 1 (XCD-contiguous, row-major) / 2 (XCD-contiguous, banded).
static int bottleneck64_nhwc_bf16_launch(const void* x, const void* w1_frag, const float* b1, const void* w2_frag,
                                         const float* b2, const void* w3_frag, const float* b3, void* out, int batch,
                                         int H, int W, int Cin, int downsample, int variant, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(x && w1_frag && b1 && w2_frag && b2 && w3_frag && b3 && out,
                "bottleneck64_nhwc_bf16: null pointer argument");
  OCC_CHECK_ARG(batch > 0 && H > 0 && W > 0, "bottleneck64_nhwc_bf16: bad dimension");
  if (!((Cin == 256 && !downsample) || (Cin == 64 && downsample))) {
    set_error("bottleneck64_nhwc_bf16: no kernel for Cin=%d downsample=%d (256/identity or 64/projection)", Cin,
              downsample);
    return OCC_E_UNSUPPORTED;
  }
  if (variant < 0 || variant > 5) {
    set_error("bottleneck64_nhwc_bf16: no variant %d (1 = first kernel; 2 = second kernel; 3, 4, 5 = second kernel with "
              "tile order 0, 1, 2)", variant);
    return OCC_E_UNSUPPORTED;
  }
  // development switches, read once: OCC_BOTTLENECK64_V2=0 keeps every default launch on the first kernel;
  // OCC_BOTTLENECK64_ORDER=0 / 1 / 2 sets the tile order of variants 0 and 2 (EXPERIMENTS.md section 8q)
  static const bool v2_on = env_default_on("OCC_BOTTLENECK64_V2");
  static const int order_default = [] {
    const char* e = getenv("OCC_BOTTLENECK64_ORDER");
    return e && e[0] >= '0' && e[0] <= '2' && !e[1] ? e[0] - '0' : kBnOrderDefault;
  }();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (variant == 0) variant = v2_on ? 2 : 1;
  if (variant != 1) {
    bottleneck64_v2_launch(x, w1_frag, b1, w2_frag, b2, w3_frag, b3, out, batch, H, W, downsample,
                           variant == 2 ? order_default : variant - 3, st);
    OCC_CHECK_LAUNCH("bottleneck64_nhwc_bf16");
    return OCC_OK;
  }
  bn64_launch(bottleneck64_nhwc_bf16_kernel<64, true>, bottleneck64_nhwc_bf16_kernel<256, false>, x, w1_frag, b1, w2_frag,
              b2, w3_frag, b3, out, batch, H, W, downsample, st);
  OCC_CHECK_LAUNCH("bottleneck64_nhwc_bf16");
  return OCC_OK;
}

extern "C" int occ_bottleneck64_nhwc_bf16(const void* x, const void* w1_frag, const float* b1,
                                          const void* w2_frag, const float* b2, const void* w3_frag,
                                          const float* b3, void* out, int batch, int H, int W, int Cin,
                                          int downsample, void* stream) {
  return bottleneck64_nhwc_bf16_launch(x, w1_frag, b1, w2_frag, b2, w3_frag, b3, out, batch, H, W, Cin, downsample, 0,
                                       stream);
}

// The same bottleneck with the kernel forced (tests, probes): see bottleneck64_nhwc_bf16_launch.  An unknown variant
// returns OCC_E_UNSUPPORTED before any launch.  Every variant computes the same bits.
extern "C" int occ_bottleneck64_nhwc_bf16_variant(const void* x, const void* w1_frag, const float* b1,
                                                  const void* w2_frag, const float* b2, const void* w3_frag,
                                                  const float* b3, void* out, int batch, int H, int W, int Cin,
                                                  int downsample, int variant, void* stream) {
  return bottleneck64_nhwc_bf16_launch(x, w1_frag, b1, w2_frag, b2, w3_frag, b3, out, batch, H, W, Cin, downsample,
                                       variant, stream);
}
