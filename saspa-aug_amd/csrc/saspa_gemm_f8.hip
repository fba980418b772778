// fp8 (OCP e4m3) W8A8 linear layers for the SDXL transformer blocks (BASELINE.json configs[4]: "fp8 MFMA"):
//   saspa_layernorm_quant_fp8   LayerNorm over the last dim -> fp8 row + one fp32 scale per row (amax / 448), one wave per row
//   saspa_gemm_fp8              out[m][n] = act(sa[m] * sw[n] * sum_k A8[m][k] * W8[n][k] + bias[n]) (+ residual), bf16 out
// on `v_mfma_f32_16x16x128_f8f6f4` (the K = 128 form that reaches the fp8 peak; the K = 32 `_fp8_fp8` form runs at the bf16
// rate).  Per-token x per-channel scales are applied in the epilogue, so the K loop is byte movement + MFMA only.
// Tile 128 x 128 x 128 bytes of K, 4 waves (2 x 2, 64 x 64 per wave), operands global -> LDS by LDS-DMA with the XOR
// swizzle on the source side (the same 128-byte-row LDS image as the bf16 kernel: one row = ONE K = 128 MFMA step; lane
// (row, g = lane >> 4) reads chunks 2g, 2g + 1 = its 32 k values -- both operands use the same assignment, so it is a valid
// permutation of the sum whatever the hardware's k order inside the instruction is), 2-stage ring, one barrier per K-tile.
// Bound: L2 -> LDS fill (32 KB per 4.2 MFLOP K-tile: 1.85x the flops per filled byte of the bf16 128x160 tile).
// MX feed-forward (calibration-free ff.net.0 -> ff.net.2, the same kernel with MX = true):
//   saspa_gemm_fp8_geglu_mx     the GEGLU launch whose epilogue emits e4m3 bytes + one E8M0 exponent per row and 32 gated columns
//                               (mx_block_exponent, the rule of saspa_groupnorm_quant_mxfp8): 8 threads walk a row of the tile, so a
//                               block is four adjacent lanes and its maximum two lane exchanges; no tensor-wide scale, no atomics
//   saspa_gemm_mxfp8            the plain launch with those exponents applied INSIDE v_mfma_scale_f32_16x16x128_f8f6f4 as the
//                               activation-side scale operand, staged the way saspa_conv_mx.hip stages them (per-lane byte loads
//                               issued with the DMA of the same K-tile, retired by the same vmcnt(0)); fragments as saspa_conv_mx.hip
//                               reads them (chunks g, g + 4), because the instruction scales k = 32 b .. 32 b + 31 by lane group b
#include "common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
constexpr unsigned kInvalidOff = 0x80000000u;   // beyond num_records of make_rsrc: the DMA lands zeros

template <int SEL>
__device__ __forceinline__ f32x4 mma_mx(const i32x8& w, const i32x8& x, const f32x4& c, int sx) {
  // as saspa_conv_mx.hip: weight scale 127 = 1.0, activation scale = byte SEL of sx (the lane's block exponent of row fragment SEL)
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, 127, SEL, sx);
}

// MX = false: qs / ldqs unused.  MX && GEGLU: qs receives the block exponents.  MX && !GEGLU: qs holds those of the activations.
template <bool GEGLU, bool MX>
__global__ __launch_bounds__(256, 2) void gemm_f8_kernel(const SaspaGemmF8Params p, uint8_t* qs, int ldqs) {
  constexpr bool MXIN = MX && !GEGLU, MXOUT = MX && GEGLU;
  constexpr int BM = 128, BN = 128, STAGE = (BM + BN) * 8;   // u32x4 per stage
  __shared__ u32x4 lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int frow = lane & 15, fg = lane >> 4;
  const int nbn = p.N / BN;
  // XCD-aware order: blocks congruent mod 8 (one XCD) walk neighbouring tiles (same activation rows -> same L2)
  int tile;
  {
    const int G = gridDim.x, L = blockIdx.x;
    const int qd = G >> 3, rr = G & 7, xcd = L & 7, idx = L >> 3;
    tile = (xcd < rr ? xcd * (qd + 1) : rr * (qd + 1) + (xcd - rr) * qd) + idx;
  }
  const int bm = tile / nbn, bn = tile - bm * nbn;
  const rsrc_t rsa = make_rsrc(p.a), rsw = make_rsrc(p.w);
  // MXIN: the exponent bytes of the lane's MFMA rows wm * 64 + 16 i + frow, block fg of each K-tile; rows >= M are never read
  // (their data is zero: any finite scale would do, an E8M0 255 from stray memory would not)
  const rsrc_t rss = make_rsrc(qs);
  unsigned bases[4], sb[4];
  if constexpr (MXIN) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = bm * BM + wm * 64 + 16 * i + frow;
      bases[i] = m < p.M ? (unsigned)m * (unsigned)ldqs + (unsigned)fg : kInvalidOff;
    }
  }
  const int r0 = tid >> 3;
  const int kcs = (tid & 7) ^ (r0 & 7);
  unsigned offa[4], offb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = bm * BM + r0 + 32 * i;
    offa[i] = m < p.M ? (unsigned)((long long)m * p.lda + kcs * 16) : kInvalidOff;
    const int n = bn * BN + r0 + 32 * i;
    offb[i] = (unsigned)((long long)n * p.ldw + kcs * 16);
  }
  auto dma = [&](int kt, int stage) __attribute__((always_inline)) {
    u32x4* la = lds + stage * STAGE;
    u32x4* lb = la + BM * 8;
    const int soff = kt * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lds_void_t*)(la + (32 * i + 8 * wave) * 8), 16, (int)offa[i], soff, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void_t*)(lb + (32 * i + 8 * wave) * 8), 16, (int)offb[i], soff, 0, 0);
    if constexpr (MXIN) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        sb[i] = __builtin_amdgcn_raw_buffer_load_b8(rss, (int)(bases[i] + 4u * (unsigned)kt), 0, 0);   // kInvalidOff + 4 kt stays out of range
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto frag = [&](const u32x4* base, int row) __attribute__((always_inline)) {
    // MXIN: chunks g and g + 4 (saspa_conv_mx.hip), so that the block the instruction scales with lane group b's byte is the
    // 32 consecutive k of block b; otherwise chunks 2 g, 2 g + 1 (any assignment both operands share sums the same products)
    const u32x4 c0 = base[row * 8 + ((MXIN ? fg : 2 * fg) ^ (row & 7))];
    const u32x4 c1 = base[row * 8 + ((MXIN ? fg + 4 : 2 * fg + 1) ^ (row & 7))];
    return i32x8{(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], (int)c1[2], (int)c1[3]};
  };
  const int nk = p.K / 128;
  dma(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                     // K-tile kt has landed for everyone; the other stage is free
    asm volatile("" ::: "memory");
    int sx = 0;
    if constexpr (MXIN) sx = (int)(sb[0] | (sb[1] << 8) | (sb[2] << 16) | (sb[3] << 24));
    if (kt + 1 < nk) dma(kt + 1, (kt + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);                // issue the DMA before the MFMA block so that it flies under it
    const u32x4* la = lds + (kt & 1) * STAGE;
    const u32x4* lb = la + BM * 8;
    i32x8 xa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xa[i] = frag(la, wm * 64 + i * 16 + frow);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x8 wb = frag(lb, wn * 64 + j * 16 + frow);
      if constexpr (MXIN) {
        acc[0][j] = mma_mx<0>(wb, xa[0], acc[0][j], sx);
        acc[1][j] = mma_mx<1>(wb, xa[1], acc[1][j], sx);
        acc[2][j] = mma_mx<2>(wb, xa[2], acc[2][j], sx);
        acc[3][j] = mma_mx<3>(wb, xa[3], acc[3][j], sx);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          // D^T: weights as the A operand, so a lane owns 4 consecutive output channels of one row; formats 0 / 0 = e4m3,
          // scale exponents 127 = 1.0 (E8M0) in byte 0 of both scale operands
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wb, xa[i], acc[i][j], 0, 0, 0, 127, 0, 127);
      }
    }
  }
  __syncthreads();
  // ---- epilogue: scales + bias, tile through LDS, whole-row 16-byte stores (GEGLU pairs values / gates there) ----
  constexpr int CP = BN + 8;
  bf16_t* ct = reinterpret_cast<bf16_t*>(lds);
  float4 sw4[4], b4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = bn * BN + wn * 64 + j * 16 + fg * 4;
    sw4[j] = *reinterpret_cast<const float4*>(p.sw + n);
    b4[j] = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mrow = wm * 64 + i * 16 + frow;
    const int m = bm * BM + mrow;
    float sa = 1.0f;                                  // MXIN: the activation scales went into the MFMA
    if constexpr (!MXIN) sa = m < p.M ? p.sa[p.sa_broadcast ? 0 : m] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ncol = wn * 64 + j * 16 + fg * 4;
      const float v[4] = {acc[i][j][0] * (sa * sw4[j].x) + b4[j].x, acc[i][j][1] * (sa * sw4[j].y) + b4[j].y,
                          acc[i][j][2] * (sa * sw4[j].z) + b4[j].z, acc[i][j][3] * (sa * sw4[j].w) + b4[j].w};
      Elem<bf16_t>::store4(ct + mrow * CP + ncol, v);
    }
  }
  __syncthreads();
  bf16_t* out = reinterpret_cast<bf16_t*>(p.out);
  if constexpr (MXOUT) {
    // ABI 20 + saspa_gemm_fp8_geglu_mx: the hidden state leaves as e4m3 under one exponent per row and 32 gated columns.  Thread
    // (row, ch) holds 8 of them, lanes ch & ~3 .. ch | 3 one block.  The trip count is uniform (BM * 8 = 4 * 256) and pad rows take
    // part in the exchanges (whole 8-lane rows are live or not): only their stores are masked.
    uint8_t* out8 = reinterpret_cast<uint8_t*>(p.out);
    for (int q = tid; q < BM * 8; q += 256) {
      const int row = q >> 3, ch = q & 7;
      const int m = bm * BM + row;
      float a[8], g[8];
      unpack8(*reinterpret_cast<const uint4*>(ct + row * CP + ch * 8), a);
      unpack8(*reinterpret_cast<const uint4*>(ct + row * CP + 64 + ch * 8), g);
      float amax = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e] = fast_gelu_mul(a[e], g[e]);
        amax = fmaxf(amax, fabsf(a[e]));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
      const int ex = mx_block_exponent(amax);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = ldexpf(a[e], -ex);    // exact; |a| <= 448 by the choice of ex
      int w0 = 0, w1 = 0;
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], w0, false);
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], w0, true);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(a[4], a[5], w1, false);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(a[6], a[7], w1, true);
      if (m < p.M) {
        *reinterpret_cast<int2*>(out8 + (long long)m * p.ldo + bn * 64 + ch * 8) = make_int2(w0, w1);
        if ((ch & 3) == 0) qs[(long long)m * ldqs + bn * 2 + (ch >> 2)] = (uint8_t)(ex + 127);
      }
    }
  } else if constexpr (GEGLU) {
    // tile columns [0, 64) are values, [64, 128) their gates (weights.pack_geglu with a 128-column tile)
    float amax = 0.f;
    const float inv_os = p.out_fp8 ? 1.0f / *p.out_scale : 1.0f;
    for (int q = tid; q < BM * 8; q += 256) {
      const int row = q >> 3, ch = q & 7;
      const int m = bm * BM + row;
      if (m >= p.M) continue;
      float a[8], g[8];
      unpack8(*reinterpret_cast<const uint4*>(ct + row * CP + ch * 8), a);
      unpack8(*reinterpret_cast<const uint4*>(ct + row * CP + 64 + ch * 8), g);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = fast_gelu_mul(a[e], g[e]);
      if (p.amax) {
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(a[e]));
      }
      if (p.out_fp8) {
        // ABI 20: the feed-forward hidden state leaves as e4m3 under ONE tensor-wide scale (a power of two from a calibration
        // pass, see SaspaGemmF8Params.out_scale): the output projection reads bytes, no quantisation pass exists.  Saturating.
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = fminf(fmaxf(a[e] * inv_os, -448.f), 448.f);
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(a[4], a[5], w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(a[6], a[7], w1, true);
        *reinterpret_cast<int2*>(reinterpret_cast<uint8_t*>(p.out) + (long long)m * p.ldo + bn * 64 + ch * 8) = make_int2(w0, w1);
      } else {
        *reinterpret_cast<uint4*>(out + (long long)m * p.ldo + bn * 64 + ch * 8) = pack8(a);
      }
    }
    if (p.amax) {
      amax = wave_max(amax);
      // non-negative floats order like their bit patterns: one integer atomic per wave
      if (lane == 0) atomicMax(reinterpret_cast<unsigned*>(p.amax), __float_as_uint(amax));
    }
  } else {
    const bf16_t* res = reinterpret_cast<const bf16_t*>(p.residual);
    for (int q = tid; q < BM * 16; q += 256) {
      const int row = q >> 4, ch = q & 15;
      const int m = bm * BM + row, n = bn * BN + ch * 8;
      if (m >= p.M) continue;
      uint4 c4 = *reinterpret_cast<const uint4*>(ct + row * CP + ch * 8);
      if (res) {
        float a[8], b[8];
        unpack8(c4, a);
        Elem<bf16_t>::load_chunk(res + (long long)m * p.ldr + n, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b[e];
        c4 = pack8(a);
      }
      *reinterpret_cast<uint4*>(out + (long long)m * p.ldo + n) = c4;
    }
  }
}

// LayerNorm + per-row fp8 quantisation: one wave per row, the row stays in registers (C <= 2048).
__global__ __launch_bounds__(256) void layernorm_quant_fp8_kernel(const bf16_t* x, int ldx, uint8_t* q, int ldq, float* scale, long long rows,
                                                                  int C, const float* gamma, const float* beta, float eps) {
  constexpr int MAXCH = 4;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int C8 = C >> 3;
  const bf16_t* xr = x + row * ldx;
  float v[MAXCH][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int chunk = lane + 64 * i;
    if (chunk < C8) {
      Elem<bf16_t>::load_chunk(xr + chunk * 8, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int chunk = lane + 64 * i;
    if (chunk < C8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; sq += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int chunk = lane + 64 * i;
    if (chunk < C8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[i][j] = (v[i][j] - mean) * rstd * gamma[chunk * 8 + j] + beta[chunk * 8 + j];
        amax = fmaxf(amax, fabsf(v[i][j]));
      }
    }
  }
  amax = wave_max(amax);
  const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;     // e4m3 maximum 448
  const float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  uint8_t* qr = q + row * ldq;
#pragma unroll
  for (int i = 0; i < MAXCH; ++i) {
    const int chunk = lane + 64 * i;
    if (chunk < C8) {
      int w0 = 0, w1 = 0;
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i][0] * inv, v[i][1] * inv, w0, false);
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i][2] * inv, v[i][3] * inv, w0, true);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i][4] * inv, v[i][5] * inv, w1, false);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[i][6] * inv, v[i][7] * inv, w1, true);
      *reinterpret_cast<int2*>(qr + chunk * 8) = make_int2(w0, w1);
    }
  }
}

}  // namespace

extern "C" int saspa_layernorm_quant_fp8(const void* x, int ldx, void* q, int ldq, float* scale, long long rows, int C,
                                         const float* gamma, const float* beta, float eps, void* stream) {
  if (!x || !q || !scale || !gamma || !beta || rows <= 0 || C <= 0) return SASPA_EINVAL;
  if (C % 8 || ldx % 8 || ldq % 8 || !aligned16(x) || (reinterpret_cast<uintptr_t>(q) & 7u)) return SASPA_EALIGN;
  if (C > 2048 || ldq < C || ldx < C) return SASPA_ERANGE;
  hipLaunchKernelGGL(layernorm_quant_fp8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const bf16_t*)x, ldx, (uint8_t*)q, ldq, scale, rows, C, gamma, beta, eps);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_gemm_fp8(const SaspaGemmF8Params* pp, void* stream) {
  if (!pp) return SASPA_EINVAL;
  const SaspaGemmF8Params& p = *pp;
  if (!p.a || !p.w || !p.sa || !p.sw || !p.out || p.M <= 0 || p.N <= 0 || p.K <= 0) return SASPA_EINVAL;
  if (p.act != SASPA_ACT_NONE && p.act != SASPA_ACT_GEGLU) return SASPA_EINVAL;
  if (p.K % 128 || p.N % 128) return SASPA_ERANGE;                 // whole K-tiles and output tiles
  if (p.lda < p.K || p.ldw < p.K || p.lda % 16 || p.ldw % 16) return SASPA_EALIGN;
  if (!aligned16(p.a) || !aligned16(p.w) || !aligned16(p.out) || !aligned16(p.sw) || (p.bias && !aligned16(p.bias))) return SASPA_EALIGN;
  if (p.ldo % 8 || p.ldo < (p.act == SASPA_ACT_GEGLU ? p.N / 2 : p.N)) return SASPA_EALIGN;
  if (p.out_fp8 && (p.act != SASPA_ACT_GEGLU || !p.out_scale)) return SASPA_EINVAL;       // fp8 emission exists in the GEGLU epilogue only
  if (p.amax && p.act != SASPA_ACT_GEGLU) return SASPA_EINVAL;
  if (p.out_fp8 && (p.ldo % 16)) return SASPA_EALIGN;                                      // the consumer's DMA reads 16-byte pieces
  if (p.act == SASPA_ACT_GEGLU && p.residual) return SASPA_ERANGE;
  if (p.residual && (p.ldr % 8 || !aligned16(p.residual))) return SASPA_EALIGN;
  if ((long long)p.M * p.lda >= (1ll << 31) || (long long)p.N * p.ldw >= (1ll << 31)) return SASPA_ERANGE;   // 32-bit DMA offsets
  const int tiles = ((p.M + 127) / 128) * (p.N / 128);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (p.act == SASPA_ACT_GEGLU) hipLaunchKernelGGL((gemm_f8_kernel<true, false>), dim3(tiles), dim3(256), 0, s, p, (uint8_t*)nullptr, 0);
  else hipLaunchKernelGGL((gemm_f8_kernel<false, false>), dim3(tiles), dim3(256), 0, s, p, (uint8_t*)nullptr, 0);
  SASPA_CHECK_LAUNCH();
  return 0;
}

namespace {

// what saspa_gemm_fp8 asks of the operands both MX entry points share with it (same codes); nout = columns of `out`
int gemm_f8_mx_checks(const SaspaGemmF8Params& p, int nout) {
  if (!p.a || !p.w || !p.sw || !p.out || p.M <= 0 || p.N <= 0 || p.K <= 0) return SASPA_EINVAL;
  if (p.K % 128 || p.N % 128) return SASPA_ERANGE;                 // whole K-tiles and output tiles
  if (p.lda < p.K || p.ldw < p.K || p.lda % 16 || p.ldw % 16) return SASPA_EALIGN;
  if (!aligned16(p.a) || !aligned16(p.w) || !aligned16(p.out) || !aligned16(p.sw) || (p.bias && !aligned16(p.bias))) return SASPA_EALIGN;
  if (p.ldo < nout) return SASPA_EALIGN;
  if ((long long)p.M * p.lda >= (1ll << 31) || (long long)p.N * p.ldw >= (1ll << 31)) return SASPA_ERANGE;   // 32-bit DMA offsets
  return 0;
}

}  // namespace

extern "C" int saspa_gemm_fp8_geglu_mx(const SaspaGemmF8Params* pp, void* qs, int ldqs, void* stream) {
  if (!pp || !qs) return SASPA_EINVAL;
  const SaspaGemmF8Params& p = *pp;
  if (p.act != SASPA_ACT_GEGLU || !p.sa || p.out_fp8 || p.out_scale || p.amax) return SASPA_EINVAL;   // no tensor-wide scale here
  if (const int rc = gemm_f8_mx_checks(p, p.N / 2)) return rc;
  if (p.ldo % 16) return SASPA_EALIGN;                             // the consumer's DMA reads 16-byte pieces
  if (ldqs % 4 || (reinterpret_cast<uintptr_t>(qs) & 3u)) return SASPA_EALIGN;     // a row's K-tile of exponents is one aligned dword
  if (ldqs < p.N / 64 || p.residual) return SASPA_ERANGE;
  const int tiles = ((p.M + 127) / 128) * (p.N / 128);
  hipLaunchKernelGGL((gemm_f8_kernel<true, true>), dim3(tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, (uint8_t*)qs, ldqs);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_gemm_mxfp8(const SaspaGemmF8Params* pp, const void* qs, int ldqs, void* stream) {
  if (!pp || !qs) return SASPA_EINVAL;
  const SaspaGemmF8Params& p = *pp;
  if (p.act != SASPA_ACT_NONE || p.sa || p.out_fp8 || p.out_scale || p.amax) return SASPA_EINVAL;     // the exponents ARE the scales
  if (const int rc = gemm_f8_mx_checks(p, p.N)) return rc;
  if (p.ldo % 8) return SASPA_EALIGN;
  if (ldqs % 4 || (reinterpret_cast<uintptr_t>(qs) & 3u)) return SASPA_EALIGN;
  if (ldqs < p.K / 32 || (long long)p.M * ldqs >= (1ll << 31)) return SASPA_ERANGE;
  if (p.residual && (p.ldr % 8 || !aligned16(p.residual))) return SASPA_EALIGN;
  const int tiles = ((p.M + 127) / 128) * (p.N / 128);
  hipLaunchKernelGGL((gemm_f8_kernel<false, true>), dim3(tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p,
                     const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(qs)), ldqs);
  SASPA_CHECK_LAUNCH();
  return 0;
}
