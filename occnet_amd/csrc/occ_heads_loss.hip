// Training tail of the occupancy model as ONE node: both decoder MLP heads AND their losses, forward and backward.
//
// Replaces (reference: projects/mmdet3d_plugin/bevformer/):
//   modules/transformer_occ.py:132-141, 318-319       predicter / flow_predicter applied to every voxel feature
//   dense_heads/bevformer_occ_head.py:163-196         loss / loss_single: CrossEntropyLoss on the logits (optionally times
//                                                     mask_camera, averaged over mask.sum()), L1Loss on the flow
// and the autograd graph between them.  As separate modules the training step writes, saves and reads back two (N, 64)
// pre-activations, the Softplus / ReLU outputs, the logits, their log_softmax and the flow residual, and the same again as
// gradients.  Here nothing but the inputs is kept: the forward reduces every 32-voxel tile to three partial sums, the backward
// recomputes the tile and leaves with dfeat and the eight parameter gradients.
//
// FORWARD (heads_loss_fwd_kernel + heads_loss_finalize_kernel): heads_tile (heads_x3.h, bf16x3 — the arithmetic of the
// inference heads) leaves the tile's logits in sm[voxel][33]; lanes 0..31 turn one voxel each into its cross-entropy term
//   ce = (logsumexp(z[0:ncls]) - z[y]) * class_weight[y] * mask        (0 for y == ignore_index and for y outside [0, ncls))
// lanes 32..63 one voxel each into l1 = |f0 - g0| + |f1 - g1| (unmasked).  Per block: one (sum ce, sum l1, mask count) record;
// the finalise wave adds the records in a fixed order (double) and writes loss_occ, loss_flow and the occ denominator.
//
// BACKWARD (heads_loss_bwd_kernel + heads_loss_reduce_kernel), exact f32 on v_mfma_f32_32x32x2_f32 and TRANSPOSED like
// occ_heads_kernel (occ_heads.hip), so every product that contracts over hidden units or channels takes the previous product's
// D registers as its B operand:
//   H^T  (128 x vox) = W1cat . X^T + b1            O^T (32 x vox) = W2cat . act(H^T) + b2
//   dz^T (32 x vox)  : g_occ w (softmax - onehot) / denom on the class rows, g_flow sign(f - g) / denom on the two flow rows
//   dA^T (128 x vox) = W2cat^T . dz^T              dH^T = dA^T * act'(H^T)    (Softplus' = sigmoid, ReLU' = H > 0)
//   dX^T (32 x vox)  = W1cat^T . dH^T  -> dfeat
// The weight gradients contract over the VOXEL index, which sits on the lanes: act(H^T), dz^T, dH^T and X go through a
// per-wave LDS image [row][voxel] (stride 33) and come back as operands with the voxel in the k slot:
//   dW2cat (32 x 128) += dz^T . act(H)             dW1cat (128 x 32) += dH^T . X
// Each wave keeps dW1cat / dW2cat in MFMA accumulators and the bias gradients as per-lane sums across its tile loop and writes
// ONE partial record at the end; the reduce kernel adds the records in a fixed order.  No float atomics anywhere: losses and
// gradients are bit-identical run to run.  The grids depend on n_rows and max_blocks only.
//
// A label outside [0, ncls) that is not ignore_index contributes nothing (torch raises a device assert there); nothing is read
// through it.
#include "heads_x3.h"

namespace occ {

constexpr int kHLWaves = 4;
constexpr int kHLFwdBlocks = 1024;                       // launcher's choice, forward: 2 blocks per CU, persistent waves
constexpr int kHLBwdBlocks = 256;                        // backward: one 4-wave block per CU (accumulators: 1 wave per SIMD)
constexpr int kHLRecord = 4096 + 128 + 4096 + 32;        // floats per wave: dW1cat | db1cat | dW2cat | db2cat
constexpr int kHLOffB1 = 4096, kHLOffW2 = 4096 + 128, kHLOffB2 = 4096 + 128 + 4096;
// backward LDS (floats): W1cat [128][33], W2cat [32][129], b1cat, b2cat, then per wave T [4][32][33] and Tz [32][33]
constexpr int kHLW1 = 128 * 33, kHLW2 = 32 * 129, kHLT = 4 * 32 * 33, kHLTz = 32 * 33;
constexpr int kHLBwdLdsFloats = kHLW1 + kHLW2 + 128 + 32 + kHLWaves * (kHLT + kHLTz);

__device__ __forceinline__ long long load_label(const void* labels, int dtype, long row) {
  return dtype == 0 ? (long long)reinterpret_cast<const unsigned char*>(labels)[row]
                    : reinterpret_cast<const long long*>(labels)[row];
}

// row of a D register: accumulator register r of lane half kh holds row (r & 3) + 8 (r >> 2) + 4 kh of the 32 x 32 tile
__host__ __device__ constexpr int drow(int r) { return (r & 3) + 8 * (r >> 2); }

__global__ __launch_bounds__(256, 2) void heads_loss_fwd_kernel(
    const float* __restrict__ feat, const float* __restrict__ w1o, const float* __restrict__ b1o,
    const float* __restrict__ w2o, const float* __restrict__ b2o, const float* __restrict__ w1f,
    const float* __restrict__ b1f, const float* __restrict__ w2f, const float* __restrict__ b2f,
    const void* __restrict__ labels, int labels_dtype, const float* __restrict__ flow_gt,
    const unsigned char* __restrict__ mask, const float* __restrict__ class_weight, long long ignore_index,
    float* __restrict__ partial, long n_rows, int ncls) {
  constexpr int C = kHeadsC;
  __shared__ __attribute__((aligned(16))) unsigned short w1s[16 * 512];
  __shared__ __attribute__((aligned(16))) unsigned short w2s[16 * 512];
  __shared__ __attribute__((aligned(16))) float b1s[128];
  __shared__ __attribute__((aligned(16))) float b2s[32];
  __shared__ float osm[kHLWaves][32 * 33];
  __shared__ float red[kHLWaves][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, g = lane >> 5;

  for (int e = tid; e < 4096; e += 256) heads_pack_weights<false>(e, w1o, w2o, w1f, w2f, ncls, w1s, w2s);
  heads_pack_bias(tid, b1o, b2o, b1f, b2f, ncls, b1s, b2s);
  __syncthreads();
  float* sm = osm[wave];
  const bf16x8* W1 = reinterpret_cast<const bf16x8*>(w1s) + lane;
  const bf16x8* W2 = reinterpret_cast<const bf16x8*>(w2s) + lane;

  float ce_acc = 0.f, l1_acc = 0.f;
  int cnt_acc = 0;
  const long n_tiles = (n_rows + 31) / 32;
  for (long tile = (long)blockIdx.x * kHLWaves + wave; tile < n_tiles; tile += (long)gridDim.x * kHLWaves) {
    const long row0 = tile * 32;
    uint4 xh[2], xl[2];
    {
      long row = row0 + vi;
      if (row >= n_rows) row = n_rows - 1;
      const float* src = feat + row * C + 8 * g;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float4 p = *reinterpret_cast<const float4*>(src + 16 * s);
        const float4 q = *reinterpret_cast<const float4*>(src + 16 * s + 4);
        bf16_split2(p.x, p.y, xh[s].x, xl[s].x); bf16_split2(p.z, p.w, xh[s].y, xl[s].y);
        bf16_split2(q.x, q.y, xh[s].z, xl[s].z); bf16_split2(q.z, q.w, xh[s].w, xl[s].w);
      }
    }
    heads_tile(xh, xl, W1, W2, b1s, b2s, sm, vi, g);
    wave_lds_sync();
    const long row = row0 + vi;
    if (row < n_rows) {
      const float* z = sm + vi * 33;
      if (g == 0) {
        const long long y = load_label(labels, labels_dtype, row);
        const bool mk = mask == nullptr || mask[row] != 0;
        if (mask != nullptr && mk) ++cnt_acc;
        if (y != ignore_index && y >= 0 && y < ncls && mk) {
          float m = z[0];
          for (int c = 1; c < ncls; ++c) m = fmaxf(m, z[c]);
          float s = 0.f;
          for (int c = 0; c < ncls; ++c) s += expf(z[c] - m);
          const float ce = (logf(s) + m) - z[(int)y];
          ce_acc += class_weight != nullptr ? ce * class_weight[(int)y] : ce;
        }
      } else {
        const float2 gt = *reinterpret_cast<const float2*>(flow_gt + row * 2);
        l1_acc += fabsf(z[ncls] - gt.x) + fabsf(z[ncls + 1] - gt.y);
      }
    }
    wave_lds_sync();
  }
  ce_acc = wave_sum(ce_acc);
  l1_acc = wave_sum(l1_acc);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt_acc += __shfl_xor(cnt_acc, d);
  if (lane == 0) {
    red[wave][0] = ce_acc; red[wave][1] = l1_acc; red[wave][2] = __int_as_float(cnt_acc);
  }
  __syncthreads();
  if (tid == 0) {
    float ce = red[0][0], l1 = red[0][1];
    int cnt = __float_as_int(red[0][2]);
    for (int w = 1; w < kHLWaves; ++w) { ce += red[w][0]; l1 += red[w][1]; cnt += __float_as_int(red[w][2]); }
    float* dst = partial + 4 * (long)blockIdx.x;
    dst[0] = ce; dst[1] = l1; dst[2] = __int_as_float(cnt); dst[3] = 0.f;
  }
}

// one wave: lane l adds records l, l + 64, ... in order, then a fixed butterfly; out = loss_occ, loss_flow, occ denominator
__global__ __launch_bounds__(64) void heads_loss_finalize_kernel(const float* __restrict__ partial, int n_records,
                                                                 int has_mask, double n_rows, int reduction_mean,
                                                                 float* __restrict__ out) {
  const int lane = threadIdx.x;
  double ce = 0.0, l1 = 0.0;
  long long cnt = 0;
  for (int p = lane; p < n_records; p += 64) {
    ce += (double)partial[4 * p]; l1 += (double)partial[4 * p + 1]; cnt += __float_as_int(partial[4 * p + 2]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    ce += __shfl_xor(ce, d); l1 += __shfl_xor(l1, d); cnt += __shfl_xor(cnt, d);
  }
  if (lane == 0) {
    const double d_occ = has_mask ? (double)cnt : (reduction_mean ? n_rows : 1.0);
    const double d_flow = reduction_mean ? 2.0 * n_rows : 1.0;
    out[0] = (float)(ce / d_occ);          // 0 / 0 stays NaN, as the reference's sum() / mask.sum()
    out[1] = (float)(l1 / d_flow);
    out[2] = (float)d_occ;
  }
}

#define OCC_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0)

__global__ __launch_bounds__(256) void heads_loss_bwd_kernel(
    const float* __restrict__ feat, const float* __restrict__ w1o, const float* __restrict__ b1o,
    const float* __restrict__ w2o, const float* __restrict__ b2o, const float* __restrict__ w1f,
    const float* __restrict__ b1f, const float* __restrict__ w2f, const float* __restrict__ b2f,
    const void* __restrict__ labels, int labels_dtype, const float* __restrict__ flow_gt,
    const unsigned char* __restrict__ mask, const float* __restrict__ class_weight, long long ignore_index,
    const float* __restrict__ grad_losses, const float* __restrict__ occ_denom, float flow_denom,
    float* __restrict__ dfeat, float* __restrict__ records, long n_rows, int ncls) {
  constexpr int C = kHeadsC, HID = kHeadsHid;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* W1s = lds;                       // W1cat [128][33]
  float* W2s = W1s + kHLW1;               // W2cat [32][129], rows >= ncls + 2 zero
  float* b1s = W2s + kHLW2;               // [128]
  float* b2s = b1s + 128;                 // [32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vi = lane & 31, kh = lane >> 5;
  float* T = b2s + 32 + wave * (kHLT + kHLTz);   // [4][32][33]: act(H^T), then dH^T, as [hidden row][voxel]
  float* Tz = T + kHLT;                          // [32][33]: dz^T as [channel][voxel], then X as [voxel][channel]

  for (int e = tid; e < 128 * 32; e += 256) {
    const int u = e >> 5, c = e & 31;
    W1s[u * 33 + c] = u < HID ? w1o[u * C + c] : w1f[(u - HID) * C + c];
    const int o = e >> 7, uu = e & 127;
    float v = 0.f;
    if (o < ncls) { if (uu < HID) v = w2o[o * HID + uu]; }
    else if (o < ncls + 2) { if (uu >= HID) v = w2f[(o - ncls) * HID + (uu - HID)]; }
    W2s[o * 129 + uu] = v;
  }
  if (tid < 128) b1s[tid] = tid < HID ? b1o[tid] : b1f[tid - HID];
  if (tid < 32) b2s[tid] = tid < ncls ? b2o[tid] : (tid < ncls + 2 ? b2f[tid - ncls] : 0.f);
  __syncthreads();

  const float one = kh == 0 ? 1.f : 0.f;
  const float g_occ = grad_losses[0], g_flow = grad_losses[1];
  const float inv_occ = 1.f / occ_denom[0], inv_flow = 1.f / flow_denom;
  const bool want_w = records != nullptr;

  f32x16 dw1[4], dw2[4];                   // this wave's dW1cat (row tile a) / dW2cat (column tile a) across its tiles
  // bias gradients: lane (i, kh) sums the A operands of the two weight-gradient products it feeds — dH^T[hidden 32 a + i] and
  // dz^T[channel i] over the voxels of parity kh; the two parities meet at the end
  float db1[4] = {0.f, 0.f, 0.f, 0.f}, db2 = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dw1[a][r] = 0.f; dw2[a][r] = 0.f; }

  const long n_tiles = (n_rows + 31) / 32;
  for (long tile = (long)blockIdx.x * kHLWaves + wave; tile < n_tiles; tile += (long)gridDim.x * kHLWaves) {
    const long row = tile * 32 + vi;
    const bool live = row < n_rows;
    // X^T fragment: lane (voxel, kh) holds channels 16 kh .. 16 kh + 15 of its voxel (k pair s = channels s, 16 + s)
    float xr[16];
    if (live) {
      const float* src = feat + row * C + kh * 16;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const float4 x4 = *reinterpret_cast<const float4*>(src + s4 * 4);
        xr[s4 * 4 + 0] = x4.x; xr[s4 * 4 + 1] = x4.y; xr[s4 * 4 + 2] = x4.z; xr[s4 * 4 + 3] = x4.w;
      }
    } else {
#pragma unroll
      for (int s = 0; s < 16; ++s) xr[s] = 0.f;
    }
    // ---- H^T = W1cat . X^T + b1 (pre-activations, kept)
    f32x16 h[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) h[a][r] = 0.f;
      h[a] = OCC_MFMA_F32(kh == 0 ? b1s[32 * a + vi] : 0.f, one, h[a]);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int a = 0; a < 4; ++a) h[a] = OCC_MFMA_F32(W1s[(32 * a + vi) * 33 + kh * 16 + s], xr[s], h[a]);
    // ---- O^T = W2cat . act(H^T) + b2; act(H^T) -> T for the weight gradient
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    o = OCC_MFMA_F32(kh == 0 ? b2s[vi] : 0.f, one, o);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float av = a < 2 ? softplus(h[a][r]) : fmaxf(h[a][r], 0.f);
        if (want_w) T[(a * 32 + drow(r) + 4 * kh) * 33 + vi] = av;
        o = OCC_MFMA_F32(W2s[vi * 129 + 32 * a + drow(r) + 4 * kh], av, o);
      }
    // ---- dz^T in the D layout: this lane holds channels drow(r) + 4 kh of its voxel, the other half sits on lane ^ 32
    float dz[16];
    {
      long long y = -1;
      float wgt = 0.f, g0 = 0.f, g1 = 0.f, cf = 0.f;
      if (live) {
        y = load_label(labels, labels_dtype, row);
        const bool ok = y != ignore_index && y >= 0 && y < ncls && (mask == nullptr || mask[row] != 0);
        if (ok) wgt = class_weight != nullptr ? class_weight[(int)y] : 1.f;
        else y = -1;
        const float2 gt = *reinterpret_cast<const float2*>(flow_gt + row * 2);
        g0 = gt.x; g1 = gt.y;
        cf = g_flow * inv_flow;
      }
      float m = -__builtin_huge_valf();
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (drow(r) + 4 * kh < ncls) m = fmaxf(m, o[r]);
      m = fmaxf(m, __shfl_xor(m, 32));
      float e[16], ssum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        e[r] = drow(r) + 4 * kh < ncls ? expf(o[r] - m) : 0.f;
        ssum += e[r];
      }
      ssum += __shfl_xor(ssum, 32);
      const float co = y >= 0 ? g_occ * wgt * inv_occ : 0.f;
      const float inv_s = 1.f / ssum;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = drow(r) + 4 * kh;
        float v = 0.f;
        if (ch < ncls) {
          v = y >= 0 ? co * (e[r] * inv_s - (ch == (int)y ? 1.f : 0.f)) : 0.f;
        } else if (ch < ncls + 2) {
          const float d = o[r] - (ch == ncls ? g0 : g1);
          v = cf * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        }
        dz[r] = v;
        if (want_w) Tz[ch * 33 + vi] = v;
      }
    }
    if (want_w) {
      // ---- dW2cat (channel x hidden tile a) += dz^T . act(H): both operands from LDS with the voxel as k
      wave_lds_sync();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const float az = Tz[vi * 33 + 2 * s + kh];
        db2 += az;
#pragma unroll
        for (int a = 0; a < 4; ++a) dw2[a] = OCC_MFMA_F32(az, T[(a * 32 + vi) * 33 + 2 * s + kh], dw2[a]);
      }
      wave_lds_sync();
    }
    // ---- dA^T = W2cat^T . dz^T; dH^T = dA^T * act'(H^T), written over H^T
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      f32x16 da;
#pragma unroll
      for (int r = 0; r < 16; ++r) da[r] = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) da = OCC_MFMA_F32(W2s[(drow(r) + 4 * kh) * 129 + 32 * a + vi], dz[r], da);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float hv = h[a][r];
        // Softplus' = sigmoid (1 above the threshold of 20, where 1 / (1 + exp(-x)) rounds to 1 as well); ReLU' = H > 0
        const float dact = a < 2 ? 1.f / (1.f + expf(-hv)) : (hv > 0.f ? 1.f : 0.f);
        const float dh = da[r] * dact;
        h[a][r] = dh;
        if (want_w) T[(a * 32 + drow(r) + 4 * kh) * 33 + vi] = dh;
      }
    }
    if (want_w) {
      // ---- dW1cat (hidden tile a x channel) += dH^T . X: X as [voxel][channel] in Tz
#pragma unroll
      for (int s = 0; s < 16; ++s) Tz[vi * 33 + kh * 16 + s] = xr[s];
      wave_lds_sync();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const float bx = Tz[(2 * s + kh) * 33 + vi];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float ah = T[(a * 32 + vi) * 33 + 2 * s + kh];
          db1[a] += ah;
          dw1[a] = OCC_MFMA_F32(ah, bx, dw1[a]);
        }
      }
      wave_lds_sync();
    }
    if (dfeat != nullptr) {
      // ---- dX^T = W1cat^T . dH^T: lane (voxel, kh) ends with channels 8 q + 4 kh .. + 3 in registers 4 q .. 4 q + 3
      f32x16 dx;
#pragma unroll
      for (int r = 0; r < 16; ++r) dx[r] = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) dx = OCC_MFMA_F32(W1s[(32 * a + drow(r) + 4 * kh) * 33 + vi], h[a][r], dx);
      if (live) {
        float* dst = dfeat + row * C + 4 * kh;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(dst + 8 * q) = make_float4(dx[4 * q], dx[4 * q + 1], dx[4 * q + 2], dx[4 * q + 3]);
      }
    }
  }
  if (want_w) {
    // every wave of the grid writes one whole record (zeros if it had no tile): the reduce kernel reads all of them
    float* rec = records + (long)(blockIdx.x * kHLWaves + wave) * kHLRecord;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        rec[(32 * a + drow(r) + 4 * kh) * 32 + vi] = dw1[a][r];                    // dW1cat[hidden][channel vi]
        rec[kHLOffW2 + (drow(r) + 4 * kh) * 128 + 32 * a + vi] = dw2[a][r];        // dW2cat[channel][hidden 32 a + vi]
      }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float v = db1[a] + __shfl_xor(db1[a], 32);
      if (kh == 0) rec[kHLOffB1 + 32 * a + vi] = v;
    }
    const float v2 = db2 + __shfl_xor(db2, 32);
    if (kh == 0) rec[kHLOffB2 + vi] = v2;
  }
}

struct HeadsLossGrads {
  float *dw1o, *db1o, *dw2o, *db2o, *dw1f, *db1f, *dw2f, *db2f;
};

// Element e of the record -> its place in the eight gradients (nullptr: padding rows of W2cat / the zero blocks of the block
// diagonal / a gradient nobody asked for).
__device__ __forceinline__ float* heads_loss_dst(const HeadsLossGrads& g, int e, int ncls) {
  constexpr int C = kHeadsC, HID = kHeadsHid;
  if (e < kHLOffB1) {
    const int u = e >> 5, c = e & 31;
    return u < HID ? (g.dw1o ? g.dw1o + u * C + c : nullptr) : (g.dw1f ? g.dw1f + (u - HID) * C + c : nullptr);
  }
  if (e < kHLOffW2) {
    const int u = e - kHLOffB1;
    return u < HID ? (g.db1o ? g.db1o + u : nullptr) : (g.db1f ? g.db1f + (u - HID) : nullptr);
  }
  if (e < kHLOffB2) {
    const int o = (e - kHLOffW2) >> 7, u = (e - kHLOffW2) & 127;
    if (o < ncls) return u < HID && g.dw2o ? g.dw2o + o * HID + u : nullptr;
    if (o < ncls + 2) return u >= HID && g.dw2f ? g.dw2f + (o - ncls) * HID + (u - HID) : nullptr;
    return nullptr;
  }
  const int o = e - kHLOffB2;
  if (o < ncls) return g.db2o ? g.db2o + o : nullptr;
  if (o < ncls + 2) return g.db2f ? g.db2f + (o - ncls) : nullptr;
  return nullptr;
}

// 16 record elements per block; thread (element, group q) adds records q, q + 16, ... in order, then the 16 groups are added
// in order: a fixed summation tree for every element
__global__ __launch_bounds__(256) void heads_loss_reduce_kernel(const float* __restrict__ records, int n_records,
                                                                HeadsLossGrads g, int ncls) {
  __shared__ float part[16][17];
  const int el = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  float acc = 0.f;
  for (int p = q; p < n_records; p += 16) acc += records[(long)p * kHLRecord + e];
  part[q][el] = acc;
  __syncthreads();
  if (q == 0) {
    float s = part[0][el];
    for (int k = 1; k < 16; ++k) s += part[k][el];
    float* dst = heads_loss_dst(g, e, ncls);
    if (dst != nullptr) *dst = s;
  }
}

static long heads_loss_blocks(int64_t n_rows, int max_blocks, int own) {
  const long n_tiles = (long)((n_rows + 31) / 32);
  long blocks = (n_tiles + kHLWaves - 1) / kHLWaves;
  const long cap = max_blocks > 0 ? max_blocks : own;
  return blocks > cap ? cap : blocks;
}

static bool heads_loss_supported(int C, int hidden, int num_classes) {
  return C == kHeadsC && hidden == kHeadsHid && num_classes + 2 <= 32;
}

}  // namespace occ

extern "C" int64_t occ_heads_loss_workspace_bytes(int64_t n_rows, int num_classes, int max_blocks) {
  using namespace occ;
  if (n_rows <= 0 || num_classes <= 0 || max_blocks < 0 || !heads_loss_supported(kHeadsC, kHeadsHid, num_classes)) return 0;
  const int64_t fwd = heads_loss_blocks(n_rows, max_blocks, kHLFwdBlocks) * 4 * (int64_t)sizeof(float);
  const int64_t bwd = heads_loss_blocks(n_rows, max_blocks, kHLBwdBlocks) * kHLWaves * kHLRecord * (int64_t)sizeof(float);
  return fwd > bwd ? fwd : bwd;
}

#define OCC_HL_CHECK_COMMON(what)                                                                                        \
  OCC_CHECK_ARG(feat && w1_occ && b1_occ && w2_occ && b2_occ && w1_flow && b1_flow && w2_flow && b2_flow && labels &&    \
                    flow_gt && workspace,                                                                                \
                what ": null pointer argument");                                                                         \
  OCC_CHECK_ARG(n_rows > 0 && num_classes > 0 && C > 0 && hidden > 0, what ": bad dimension");                           \
  OCC_CHECK_ARG(labels_dtype == 0 || labels_dtype == 1, what ": labels_dtype must be 0 (uint8) or 1 (int64)");           \
  OCC_CHECK_ARG(reduction_mean == 0 || reduction_mean == 1, what ": reduction_mean must be 0 or 1");                     \
  OCC_CHECK_ARG(max_blocks >= 0, what ": max_blocks must be >= 0");                                                      \
  if (!heads_loss_supported(C, hidden, num_classes)) {                                                                   \
    set_error(what ": no fused kernel for C=%d hidden=%d num_classes=%d", C, hidden, num_classes);                       \
    return OCC_E_UNSUPPORTED;                                                                                            \
  }                                                                                                                      \
  OCC_CHECK_ARG(workspace_bytes >= occ_heads_loss_workspace_bytes(n_rows, num_classes, max_blocks),                      \
                what ": workspace too small");                                                                           \
  OCC_CHECK_ARG((reinterpret_cast<uintptr_t>(feat) & 15) == 0 && (reinterpret_cast<uintptr_t>(flow_gt) & 7) == 0 &&      \
                    (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,                                                  \
                what ": feat / workspace must be 16-byte aligned, flow_gt 8-byte aligned")

extern "C" int occ_heads_loss_fwd_f32(const float* feat, const float* w1_occ, const float* b1_occ, const float* w2_occ,
                                      const float* b2_occ, const float* w1_flow, const float* b1_flow,
                                      const float* w2_flow, const float* b2_flow, const void* labels, int labels_dtype,
                                      const float* flow_gt, const uint8_t* mask, const float* class_weight,
                                      int64_t ignore_index, int reduction_mean, float* losses, void* workspace,
                                      int64_t workspace_bytes, int64_t n_rows, int C, int hidden, int num_classes,
                                      int max_blocks, void* stream) {
  using namespace occ;
  OCC_HL_CHECK_COMMON("heads_loss_fwd");
  OCC_CHECK_ARG(losses != nullptr, "heads_loss_fwd: null pointer argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long blocks = heads_loss_blocks(n_rows, max_blocks, kHLFwdBlocks);
  float* partial = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(heads_loss_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, feat, w1_occ, b1_occ, w2_occ,
                     b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, labels, labels_dtype, flow_gt, mask, class_weight,
                     (long long)ignore_index, partial, (long)n_rows, num_classes);
  OCC_CHECK_LAUNCH("heads_loss_fwd");
  hipLaunchKernelGGL(heads_loss_finalize_kernel, dim3(1), dim3(64), 0, st, partial, (int)blocks, mask != nullptr ? 1 : 0,
                     (double)n_rows, reduction_mean, losses);
  OCC_CHECK_LAUNCH("heads_loss_fwd (finalize)");
  return OCC_OK;
}

extern "C" int occ_heads_loss_bwd_f32(const float* feat, const float* w1_occ, const float* b1_occ, const float* w2_occ,
                                      const float* b2_occ, const float* w1_flow, const float* b1_flow,
                                      const float* w2_flow, const float* b2_flow, const void* labels, int labels_dtype,
                                      const float* flow_gt, const uint8_t* mask, const float* class_weight,
                                      int64_t ignore_index, int reduction_mean, const float* grad_losses,
                                      const float* occ_denom, float* dfeat, float* dw1_occ, float* db1_occ,
                                      float* dw2_occ, float* db2_occ, float* dw1_flow, float* db1_flow, float* dw2_flow,
                                      float* db2_flow, void* workspace, int64_t workspace_bytes, int64_t n_rows, int C,
                                      int hidden, int num_classes, int max_blocks, void* stream) {
  using namespace occ;
  OCC_HL_CHECK_COMMON("heads_loss_bwd");
  OCC_CHECK_ARG(grad_losses && occ_denom, "heads_loss_bwd: null pointer argument");
  const HeadsLossGrads g = {dw1_occ, db1_occ, dw2_occ, db2_occ, dw1_flow, db1_flow, dw2_flow, db2_flow};
  const bool want_w = dw1_occ || db1_occ || dw2_occ || db2_occ || dw1_flow || db1_flow || dw2_flow || db2_flow;
  OCC_CHECK_ARG(dfeat || want_w, "heads_loss_bwd: no gradient requested");
  OCC_CHECK_ARG((reinterpret_cast<uintptr_t>(dfeat) & 15) == 0, "heads_loss_bwd: dfeat must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long blocks = heads_loss_blocks(n_rows, max_blocks, kHLBwdBlocks);
  const int lds = kHLBwdLdsFloats * (int)sizeof(float);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(heads_loss_bwd_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) {
    set_error("heads_loss_bwd: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    return OCC_E_LAUNCH;
  }
  float* records = want_w ? reinterpret_cast<float*>(workspace) : nullptr;
  const float flow_denom = reduction_mean ? 2.f * (float)n_rows : 1.f;
  hipLaunchKernelGGL(heads_loss_bwd_kernel, dim3((unsigned)blocks), dim3(256), lds, st, feat, w1_occ, b1_occ, w2_occ,
                     b2_occ, w1_flow, b1_flow, w2_flow, b2_flow, labels, labels_dtype, flow_gt, mask, class_weight,
                     (long long)ignore_index, grad_losses, occ_denom, flow_denom, dfeat, records, (long)n_rows,
                     num_classes);
  OCC_CHECK_LAUNCH("heads_loss_bwd");
  if (want_w) {
    hipLaunchKernelGGL(heads_loss_reduce_kernel, dim3(kHLRecord / 16), dim3(256), 0, st, records,
                       (int)(blocks * kHLWaves), g, num_classes);
    OCC_CHECK_LAUNCH("heads_loss_bwd (reduce)");
  }
  return OCC_OK;
}
