// Backbone 3x3 / pad-1 convolutions, stride 1 or 2 (NHWC bf16) as an implicit GEMM on the gfx950 bf16 matrix
// cores with bias + ReLU fused: out = relu?( conv3x3(x, W) + bias ), bf16 in / f32 accumulate / bf16 out.
//
// NOT part of the hand-written hot path: it replaces MIOpen's igemm kernel plus its
// zero-fill / cast helpers plus the elementwise tail for the stride-1 3x3 convolutions of the reference's
// ResNet-50 (mmdet Bottleneck conv2, style='pytorch', incl. the stride-2 first blocks of layer2..4) and the
// FPN output / extra-level convolutions, when Cout % 128 == 0 and Cin % 32 == 0; the 7x7 stem stays on MIOpen
// (the 64-channel layer1 blocks have their own whole-bottleneck kernel).
//
// GEMM view: M = output pixels, N = Cout, K = 9 taps x Cin.  Block = 4 waves x (2*RT x 16 output pixels = RT
// 32-pixel MFMA row tiles of two image rows each) x 128*NT output channels; waves split N.  Per chunk of 32
// input channels the (2*RT+2) x (16+2) pixel halo (stride 2: (4*RT+1) x 33) is staged ONCE into LDS (zero-filled outside the image =
// the convolution's padding; double buffered; 80-byte pixel slots, 1536-byte halo rows: conflict-free
// ds_read_b128) and reused by the 9 taps with compile-time offsets; the weights are pre-packed in MFMA
// B-fragment order ([chunk][tap][k-step][Cout/32][lane][8]) and every wave streams the operands of its own
// 32*NT columns global -> registers through a ring of 6 k-steps — they never touch LDS;
// the chunk order is rotated per block (L2 channel hot-spotting, see conv1x1_nhwc_bf16.hip).
// v_mfma_f32_32x32x16_bf16, 2 k-steps per (chunk, tap).
//
// Variants (id 10 * NT + RT; the launcher picks one per shape, occ_conv3x3_nhwc_bf16_variant forces one): RT = 2..8 row
// tiles per wave, i.e. 64..256 output pixels per block, and NT = 1 or 2.  Every wave streams 1 KB of weights per k-step
// and column tile whatever RT is, so a taller tile feeds more MFMAs from the same weight bytes and stages less halo per
// pixel; a shorter one pads less on small maps and gives a larger grid; NT 2 stages each halo chunk once for 256
// channels and halves the A-fragment reads per MFMA.
#include "conv3x3_kloop.h"

namespace occ {

// torch weight (Cout, Cin, 3, 3) f32 -> bf16 in MFMA B-fragment order
// packed[chunk = ci/32][tap = ky*3+kx][ks = 0,1][Cout/32][lane][8]:  element j of lane `lane` is
// w[co = nt*32 + (lane & 31)][ci = chunk*32 + ks*16 + (lane >> 5)*8 + j][tap]
__global__ void conv3x3_pack_weight_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed,
                                           int Cout, int Cin) {
  const long n = (long)Cout * Cin * 9;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
  long r = idx >> 9;
  const int nt32 = Cout / 32;
  const int nt = (int)(r % nt32); r /= nt32;
  const int ks = (int)(r & 1); r >>= 1;
  const int tap = (int)(r % 9);
  const int chunk = (int)(r / 9);
  const int co = nt * 32 + (lane & 31), ci = chunk * 32 + ks * 16 + (lane >> 5) * 8 + j;
  packed[idx] = bf16_rne(w[((long)co * Cin + ci) * 9 + tap]);
}

// What the K loop (conv3x3_kloop.h) takes from this kernel: the wave's column tiles are clamped to the packed weight's last
// one, and the chunk rotation mixes in the column block
#define OCC_C3_NT32 (Cout / 32)
#define OCC_C3_WTILE(T) ((nw0 / 32 + (T)) < NT32 ? nw0 / 32 + (T) : NT32 - 1)
#define OCC_C3_ROT (blockIdx.x * 5u + blockIdx.y * 3u)

template <int NT, int S, int PF, int RT_, int MINW>
__global__ __launch_bounds__(256, MINW) void conv3x3_nhwc_bf16_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ wp, const float* __restrict__ bias,
    unsigned short* __restrict__ out, int H, int W, int Ho, int Wo, int Cin, int Cout, int tiles_x,
    int tiles_y, int relu, unsigned* __restrict__ amax8) {
  using G = C3Geom<S, RT_>;
  constexpr int RT = G::RT, BN = 128 * NT, WR = 32 * NT, OLD = BN + 4;
  constexpr int kC3ROW = G::ROW, kC3TH = G::TH;
  constexpr int HALO_BYTES = G::HH * kC3ROW;                 // RT 4: 15 360 (stride 1) / RT 2: 25 344 (stride 2)
  constexpr int STAGE_BYTES = 2 * HALO_BYTES, OUT_BYTES = 32 * OLD * 4;   // LDS carries only the halo
  __shared__ __attribute__((aligned(16))) char lds[STAGE_BYTES > OUT_BYTES ? STAGE_BYTES : OUT_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kb = lane >> 5;
  int bid = blockIdx.x;
  const int tx_i = bid % tiles_x; bid /= tiles_x;
  const int ty_i = bid % tiles_y;
  const int img = bid / tiles_y;
  const int y0 = ty_i * kC3TH, x0 = tx_i * kC3TW;
  const int n0 = blockIdx.y * BN, nw0 = n0 + wave * WR;
  const int CQ = Cin / 8, NCH = Cin / 32;

  f32x16 acc[RT][NT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rt][t][r] = 0.f;

  { OCC_C3_KLOOP }

  // ---- epilogue, one 32-pixel row tile (two image rows) at a time through an LDS transpose -------------
  const int c = lane * 4;
  const bool col_live = c < BN && n0 + c < Cout;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col_live) bv = *reinterpret_cast<const float4*>(bias + n0 + c);
  float* sO = reinterpret_cast<float*>(lds);
  unsigned amax2 = 0;                                        // two 16-bit maxima of the sign-stripped bf16 patterns stored
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        sO[((r & 3) + 8 * (r >> 2) + 4 * kb) * OLD + (wave * NT + t) * 32 + vi] = acc[rt][t][r];
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int row = wave * 8 + rr;                       // pixel inside the row tile
      const int oy = y0 + 2 * rt + (row >> 4), ox = x0 + (row & 15);
      if (oy < Ho && ox < Wo && col_live) {
        float4 v = *reinterpret_cast<const float4*>(sO + row * OLD + c);
        v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
        if (relu) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        const uint2 o = make_uint2(pack_bf16x2_rne(v.x, v.y), pack_bf16x2_rne(v.z, v.w));
        *reinterpret_cast<uint2*>(out + (((long)img * Ho + oy) * Wo + ox) * Cout + n0 + c) = o;
        amax2 = absmax_pk2(absmax_pk2(amax2, o.x), o.y);
      }
    }
  }
  // max|out| of what this launch stored, for the consumer's fp16 range scale (value_range.hip): one atomic per wave into
  // one of 8 words (Inf / NaN patterns order above every finite one and reach the consumer as such)
  if (amax8 != nullptr) {
    unsigned m16 = (amax2 & 0xffffu) > (amax2 >> 16) ? (amax2 & 0xffffu) : (amax2 >> 16);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)m16, d);
      m16 = o > m16 ? o : m16;
    }
    if (lane == 0 && m16 != 0u) atomicMax(amax8 + ((blockIdx.x + wave) & 7u), m16);
  }
}

}  // namespace occ

extern "C" int occ_conv3x3_pack_weight_bf16(const float* weight, void* packed, int Cout, int Cin,
                                            void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(weight && packed, "conv3x3_pack_weight_bf16: null pointer argument");
  if (Cin % 32 || Cout % 128) {
    set_error("conv3x3_pack_weight_bf16: no kernel for Cin=%d Cout=%d (need Cin %% 32 == 0, Cout %% 128 == 0)",
              Cin, Cout);
    return OCC_E_UNSUPPORTED;
  }
  const long n = (long)Cout * Cin * 9;
  hipLaunchKernelGGL(conv3x3_pack_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), weight,
                     reinterpret_cast<unsigned short*>(packed), Cout, Cin);
  OCC_CHECK_LAUNCH("conv3x3_pack_weight_bf16");
  return OCC_OK;
}

namespace occ {
// Default variant for a shape: the candidate with the least
//   cost = rounds * W * RT * (NT + 1),   rounds = ceil(blocks / (256 CUs * W)),   W = waves per SIMD of the variant.
// A block keeps its slot for time proportional to what each of its waves issues per k-step, in units of one MFMA:
// NT * RT MFMAs plus RT A-fragment reads out of the staged halo (the halo is staged once per block, so a 256-channel
// block pays it once for twice the MFMAs), times the W waves that share the SIMD.  The grid runs in `rounds` passes
// over the 256 CUs, so row padding (ceil(Ho / 2RT) tiles) and a partly filled last pass both count.  Ties go to the
// earlier (smaller) tile.  The two constants (weights 1 and 1) fit the per-shape sweep of every variant over the
// backbone's shapes (tools_dev/conv_probe.py c3v) without making any shape slower than the 8 x 16 tile it replaced.
int c3_pick(long batch, int Ho, int Wo, int Cout, int stride) {
  const long tiles_x = (Wo + kC3TW - 1) / kC3TW;
  int best = 12;
  long best_cost = -1;
  for (const C3Variant& v : kC3Variants) {
    const int nt = v.id / 10, rt = v.id % 10;
    if (v.stride != stride || Cout % (128 * nt)) continue;
    const long blocks = batch * tiles_x * ((Ho + 2 * rt - 1) / (2 * rt)) * (Cout / (128 * nt));
    const long rounds = (blocks + 256L * v.minw - 1) / (256L * v.minw);
    const long cost = rounds * v.minw * rt * (nt + 1);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = v.id; }
  }
  return best;
}
}  // namespace occ

static int conv3x3_nhwc_bf16_launch(const void* x, const void* weight_packed, const float* bias, void* out,
                                    int batch, int H, int W, int Cin, int Cout, int stride, int relu,
                                    uint32_t* amax8, int variant, void* stream) {
  using namespace occ;
  OCC_CHECK_ARG(x && weight_packed && bias && out, "conv3x3_nhwc_bf16: null pointer argument");
  OCC_CHECK_ARG(batch > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv3x3_nhwc_bf16: bad dimension");
  if (Cin % 32 || Cout % 128 || (stride != 1 && stride != 2)) {
    set_error("conv3x3_nhwc_bf16: no kernel for Cin=%d Cout=%d stride=%d (need Cin %% 32 == 0, Cout %% 128 == 0, "
              "stride 1 or 2)", Cin, Cout, stride);
    return OCC_E_UNSUPPORTED;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;     // floor((H + 2 - 3) / stride) + 1
  const int id = variant == 0 ? c3_pick(batch, Ho, Wo, Cout, stride) : variant;
  const int nt = id / 10, rt = id % 10;
  if (c3_minw(stride, id) == 0 || Cout % (128 * nt)) {
    set_error("conv3x3_nhwc_bf16: no variant %d at stride %d, Cout %d (stride 1: 12, 13, 14, 16, 18, 22, 23, 24; "
              "stride 2: 12, 13, 22; 2x: Cout %% 256 == 0)", variant, stride, Cout);
    return OCC_E_UNSUPPORTED;
  }
  const int tiles_x = (Wo + kC3TW - 1) / kC3TW, tiles_y = (Ho + 2 * rt - 1) / (2 * rt);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned gx = (unsigned)((long)batch * tiles_x * tiles_y);
#define OCC_C3_LAUNCH(SS, ID)                                                                       \
  case ID:                                                                                          \
    hipLaunchKernelGGL((conv3x3_nhwc_bf16_kernel<ID / 10, SS, 6, ID % 10, c3_minw(SS, ID)>),       \
                       dim3(gx, (unsigned)(Cout / (128 * (ID / 10)))), dim3(256), 0, st,            \
                       reinterpret_cast<const uint4*>(x), reinterpret_cast<const uint4*>(weight_packed), bias, \
                       reinterpret_cast<unsigned short*>(out), H, W, Ho, Wo, Cin, Cout, tiles_x, tiles_y, relu, amax8); \
    break;
  // ring of 6 k-steps + 3 waves per SIMD measured faster than 12 k-steps + 2 waves on every ResNet-50 shape (RT 4)
  if (stride == 2) {
    switch (id) { OCC_C3_LAUNCH(2, 12) OCC_C3_LAUNCH(2, 13) default: OCC_C3_LAUNCH(2, 22) }
  } else {
    switch (id) {
      OCC_C3_LAUNCH(1, 12) OCC_C3_LAUNCH(1, 13) OCC_C3_LAUNCH(1, 14) OCC_C3_LAUNCH(1, 16) OCC_C3_LAUNCH(1, 18)
      OCC_C3_LAUNCH(1, 22) OCC_C3_LAUNCH(1, 23) default: OCC_C3_LAUNCH(1, 24)
    }
  }
#undef OCC_C3_LAUNCH
  OCC_CHECK_LAUNCH("conv3x3_nhwc_bf16");
  return OCC_OK;
}

extern "C" int occ_conv3x3_nhwc_bf16(const void* x, const void* weight_packed, const float* bias, void* out,
                                     int batch, int H, int W, int Cin, int Cout, int stride, int relu,
                                     void* stream) {
  return conv3x3_nhwc_bf16_launch(x, weight_packed, bias, out, batch, H, W, Cin, Cout, stride, relu, nullptr, 0, stream);
}

// The same convolution; additionally folds max|out| (sign-stripped bf16 patterns of every element it stores) into amax8[0..8)
// with atomic maxima — the words ACCUMULATE across launches (the caller zeroes them once in front of the FPN's output
// convolutions) and feed occ_value_range_scale_from_amax: the consumer's range pass over the maps is not needed.
extern "C" int occ_conv3x3_nhwc_bf16_amax(const void* x, const void* weight_packed, const float* bias, void* out,
                                          int batch, int H, int W, int Cin, int Cout, int stride, int relu,
                                          uint32_t* amax8, void* stream) {
  OCC_CHECK_ARG(amax8, "conv3x3_nhwc_bf16_amax: null amax8");
  return conv3x3_nhwc_bf16_launch(x, weight_packed, bias, out, batch, H, W, Cin, Cout, stride, relu, amax8, 0, stream);
}

// Either of the above with the tile forced: variant = row tiles per wave (stride 1: 2, 3, 4, 6, 8; stride 2: 2, 3) or 0
// for the launcher's own choice; amax8 may be null.  Variants differ only in f32 summation order (the chunk rotation
// follows the block index); each one is deterministic.
extern "C" int occ_conv3x3_nhwc_bf16_variant(const void* x, const void* weight_packed, const float* bias, void* out,
                                             int batch, int H, int W, int Cin, int Cout, int stride, int relu,
                                             uint32_t* amax8, int variant, void* stream) {
  return conv3x3_nhwc_bf16_launch(x, weight_packed, bias, out, batch, H, W, Cin, Cout, stride, relu, amax8, variant,
                                  stream);
}
