// REJECTED DESIGN (round 4), kept for the record — not built.  Persistent, wave-specialised form of the Linear chain
// programs (csrc/linear_chain_x3.hip): one 8-wave block per CU for the whole launch, waves 0-3 compute, waves 4-7
// bring the next tile's input rows and the residual rows in behind the block barriers.  Parity-green (14 chain tests),
// measured on MI355X (profiles/r04_chain_persistent.txt): program A 120-128 us and program B 235-248 us at 40 000
// rows against 95-102 / 167-179 us for the block-per-tile kernel: a tile costs ~38 us per CU whether its inputs are
// prefetched or not.  It was inserted before the `#undef OCC_CH_LOAD` line of linear_chain_x3.hip and launched with
// grid = min(#CUs, tiles), 512 threads, kPpLds bytes of dynamic LDS.

// ---- persistent, wave-specialised form of the two programs ------------------------------------------------------------
// What round 4's measurements said about the block-per-tile kernel above (profiles/r04_chain_*.txt): alone on a CU its k
// loops run at the MFMA rate (~320-380 clocks per 16-k step), but a block spends 3/4 of its life in the phases AROUND
// them — waiting for its 64 KB input tile, then for the residual rows, storing — and all resident blocks do so in
// lockstep, so load bursts, MFMA and store bursts add up chip-wide (with the k loops compiled out the launch still took
// 30 of its 40 us; coalescing the transfers, rotating the k order and staggering block starts changed nothing).  A
// wave's loads return in order, so a compute wave cannot prefetch from HBM without stalling its own weight ring.
// Here a block is 8 waves on one CU for the whole launch: waves 0-3 compute exactly as above; waves 4-7 only move
// data — while tile i is computed they bring tile i + 1's input rows in, split them into the OTHER 64 KB tile buffer,
// and stage tile i's residual rows (fp32, swizzled) in the buffer the previous tile left, all behind the block barriers
// the compute waves execute anyway:
//   BAR1  tile i's planes are in X (loaders wrote them during tile i-1), tile i-1 is completely done with Y
//         loaders: residual(i) registers -> Y            compute: stage-1 k loop over X
//   BAR2  residual(i) visible                              compute: acc += residual, LayerNorm sums
//   BAR3  (LayerNorm 1st) compute is done reading Y        loaders: request tile i+1's input rows
//   BAR4  (LayerNorm 2nd)
//   BAR5  LayerNorm'd planes of tile i visible in X        compute: remaining stages; loaders: split -> planes(i+1) into Y,
//                                                          request residual(i+1)
// (program B has seven more barriers per tile, which the loaders pass without work).  Tiles alternate between the two
// buffers; the weight ring wraps from a tile's last k loop into the next tile's first.  One block per CU (130 KB LDS).
constexpr int kPpBuf = 2 * kChPlane;              // one tile buffer: hi + lo planes, or 64 rows x 256 f32
constexpr int kPpRed = 2 * kPpBuf;
constexpr int kPpLds = kPpRed + 2 * 4 * kChRows * 4;

__device__ __forceinline__ void pp_load_rows(float4 (&v)[16], const float* src, long ld, long m0, int M, int lw, int lane) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    long m = m0 + j * 4 + lw;
    if (m >= M) m = (long)M - 1;
    v[j] = *reinterpret_cast<const float4*>(src + m * ld + lane * 4);
  }
}

// input rows -> hi / lo planes of tile buffer `x` (a wave instruction = one whole row)
__device__ __forceinline__ void pp_split_rows(const float4 (&v)[16], char* x, int lw, int lane) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = j * 4 + lw;
    unsigned h01, h23, l01, l23;
    bf16_split2(v[j].x, v[j].y, h01, l01);
    bf16_split2(v[j].z, v[j].w, h23, l23);
    char* q = x + row * 512 + (((lane >> 1) ^ row) & 31) * 16 + (lane & 1) * 8;
    *reinterpret_cast<uint2*>(q) = make_uint2(h01, h23);
    *reinterpret_cast<uint2*>(q + kChPlane) = make_uint2(l01, l23);
  }
}

// residual rows, fp32, into buffer `y`: 16-byte piece p of row r at slot p ^ r of the row's 1 KB (the compute waves read
// a column of pieces — 32 rows, one piece each — per instruction: conflict-free with the swizzle)
__device__ __forceinline__ void pp_stage_rows(const float4 (&v)[16], char* y, int lw, int lane) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = j * 4 + lw;
    *reinterpret_cast<float4*>(y + row * 1024 + ((lane ^ row) & 63) * 16) = v[j];
  }
}

__device__ __forceinline__ void pp_add_rows(f32x16 (&acc)[2][2], const char* y, int wave, int vi, int kb) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = rt * 32 + vi, piece = 16 * wave + 8 * t + 2 * q + kb;
        const float4 v = *reinterpret_cast<const float4*>(y + r * 1024 + ((piece ^ r) & 63) * 16);
        acc[rt][t][4 * q + 0] += v.x;
        acc[rt][t][4 * q + 1] += v.y;
        acc[rt][t][4 * q + 2] += v.z;
        acc[rt][t][4 * q + 3] += v.w;
      }
}

template <int PROG>
__global__ __launch_bounds__(512, 2) void linear_chain_pp_kernel(const ChainArgs p) {
  extern __shared__ __attribute__((aligned(16))) char tl[];
  float* red = reinterpret_cast<float*>(tl + kPpRed);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = p.M;
  const int ntiles = (M + kChRows - 1) / kChRows, G = (int)gridDim.x;

  if (wave >= 4) {
    // ---------------------------------------------------------------------------------------------- loader waves
    const int lw = wave - 4;
    float4 v[16], vr[16];
    int tile = (int)blockIdx.x;
    pp_load_rows(v, p.a, p.lda, (long)tile * kChRows, M, lw, lane);
    pp_load_rows(vr, p.res, p.ldres, (long)tile * kChRows, M, lw, lane);
    pp_split_rows(v, tl, lw, lane);
    int par = 0;
#pragma unroll 1
    for (; tile < ntiles; tile += G, par ^= 1) {
      char* y = tl + (par ^ 1) * kPpBuf;
      const bool more = tile + G < ntiles;          // block-uniform
      __syncthreads();                              // BAR1
      pp_stage_rows(vr, y, lw, lane);
      __syncthreads();                              // BAR2
      __syncthreads();                              // BAR3
      if (more) pp_load_rows(v, p.a, p.lda, (long)(tile + G) * kChRows, M, lw, lane);
      __syncthreads();                              // BAR4
      __syncthreads();                              // BAR5  (both passed at once: waiting for the rows HERE would hold the
      if (more) pp_split_rows(v, y, lw, lane);      //        compute waves at BAR5 for a whole HBM round trip)
      if (PROG == 1) {
        __syncthreads(); __syncthreads(); __syncthreads(); __syncthreads();     // BAR6 .. BAR9
        __syncthreads(); __syncthreads();                                       // BAR10, BAR11 (second LayerNorm)
        if (p.npass > 0) __syncthreads();                                       // BAR12
      }
      if (more) pp_load_rows(vr, p.res, p.ldres, (long)(tile + G) * kChRows, M, lw, lane);
    }
    return;
  }

  // ------------------------------------------------------------------------------------------------ compute waves
  const int vi = lane & 31, kb = lane >> 5;
  occ_u32x4 w[4][4];
  const __amdgpu_buffer_rsrc_t wr = uniform_rsrc(p.wp, p.wbytes);
  const int wv = (wave * 4096) + lane * 16;
  const int rot = (int)(blockIdx.x >> 3) & 15;
  OCC_CH_LOAD(0, rot)
  OCC_CH_LOAD(1, (rot + 1) & 15)
  OCC_CH_LOAD(2, (rot + 2) & 15)
  const unsigned abase = (unsigned)(vi * 512 + ((kb ^ vi) & 31) * 16);
  const int tail0 = PROG == 1 ? 80 : 16;           // first ring step / bias offset of the tail stage
  const int bias_off = PROG == 1 ? 1024 : 256;
  const int after1 = PROG == 1 ? 16 : (p.npass > 0 ? 16 : 0);

  int par = 0;
#pragma unroll 1
  for (int tile = (int)blockIdx.x; tile < ntiles; tile += G, par ^= 1) {
    char* x = tl + par * kPpBuf;
    const char* y = tl + (par ^ 1) * kPpBuf;
    const long m0 = (long)tile * kChRows;
    long rows[2];
    bool live[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const long r = m0 + rt * 32 + vi;
      live[rt] = r < M;
      rows[rt] = live[rt] ? r : (long)M - 1;
    }
    f32x16 acc[2][2];
    ch_init(acc, p.bias, nullptr, 0, rows, wave * 64, kb);
    __syncthreads();                                // BAR1
    ch_kloop<0>(acc, w, wr, wv, 0, after1, x, abase, rot);
    __syncthreads();                                // BAR2
    pp_add_rows(acc, y, wave, vi, kb);
    ch_layernorm(acc, red, p.ln1_g, p.ln1_b, p.eps1, wave, vi, kb);              // BAR3, BAR4
    ch_store(acc, p.y, p.ldy, rows, live, wave * 64, kb, true, true, false, p.dbg);     // A: x1.  B: x2 parked in its own rows of y
    ch_to_tile(acc, x, wave, vi, kb);
    __syncthreads();                                // BAR5

    if constexpr (PROG == 1) {
      f32x16 ha[2][2], hb[2][2];
      ch_init(ha, p.bias + 256, nullptr, 0, rows, wave * 64, kb);
      ch_kloop<0>(ha, w, wr, wv, 16, 32, x, abase, rot);
      ch_relu(ha);
      ch_init(hb, p.bias + 512, nullptr, 0, rows, wave * 64, kb);
      ch_kloop<0>(hb, w, wr, wv, 32, 48, x, abase, rot);
      ch_relu(hb);
      __syncthreads();                              // BAR6: every wave has read the x2 tile for the last time
      ch_to_tile(ha, x, wave, vi, kb);
      __syncthreads();                              // BAR7
      ch_init(acc, p.bias + 768, p.y, p.ldy, rows, wave * 64, kb);               // b2 + x2 (this lane's own stores)
      ch_kloop<0>(acc, w, wr, wv, 48, 64, x, abase, rot);
      __syncthreads();                              // BAR8
      ch_to_tile(hb, x, wave, vi, kb);
      __syncthreads();                              // BAR9
      ch_kloop<0>(acc, w, wr, wv, 64, p.npass > 0 ? 80 : 0, x, abase, rot);
      ch_layernorm(acc, red, p.ln2_g, p.ln2_b, p.eps2, wave, vi, kb);            // BAR10, BAR11
      ch_store(acc, p.y, p.ldy, rows, live, wave * 64, kb, true, true, false, p.dbg);   // x3
      if (p.npass > 0) {
        ch_to_tile(acc, x, wave, vi, kb);
        __syncthreads();                            // BAR12
      }
    }

#pragma unroll 1
    for (int ps = 0; ps < p.npass; ++ps) {
      const int c0 = ps * 256 + wave * 64;
      const bool tm = p.term != nullptr && c0 < p.term_cols;
      ch_init(acc, p.bias + bias_off, tm ? p.term : nullptr, p.ldterm, rows, c0, kb);
      ch_kloop<0>(acc, w, wr, wv, tail0 + ps * 16, ps + 1 < p.npass ? tail0 + (ps + 1) * 16 : 0, x, abase, rot);
      const int ca = c0, cb = c0 + 32;
      const bool a1 = ca < p.n1, b1 = cb < p.n1;
      const bool a2 = ca >= p.off2 && ca < p.off2 + p.n2, b2 = cb >= p.off2 && cb < p.off2 + p.n2;
      if (a1 || b1) ch_store(acc, p.z1, p.ldz1, rows, live, c0, kb, a1, b1, p.act != 0, p.dbg);
      if (a2 || b2) ch_store(acc, p.z2, p.ldz2, rows, live, c0 - p.off2, kb, a2, b2, p.act != 0, p.dbg);
    }
  }
}

