// MX-fp8 implicit-GEMM 3x3 convolution (stride 1, pad 1): ResnetBlock2D conv1 / conv2 on the opt-in fp8 conv path
// (pipeline.enable_fp8(convs=True) / SASPA_FP8_CONV=1; SURVEY 8a a7.5 / a7.6, BASELINE.json configs[4] "fp8 MFMA"):
//   out[m][n] = bf16(sw[n] * sum_k 2^(qs[m, k] - 127) q[m][k] w8[n][k] + bias[n] + rowvec[b(m)][n]) (+ residual[m][n])
// where q / qs are the e4m3 bytes and E8M0 block exponents saspa_groupnorm_quant_mxfp8 writes (one exponent per pixel and
// 32-channel block), applied INSIDE v_mfma_scale_f32_16x16x128_f8f6f4: a per-pixel scale does not factor out of the sum over taps,
// a per-lane block scale does.  The weight-side scale operand stays 127 (= 1.0); sw[n] is the per-output-channel weight scale.
// Structure: gemm_f8_kernel's (saspa_gemm_f8.hip) LDS-DMA ring with the XOR swizzle on the source side, widened to 128 x 160 tiles
// (4 waves 2 x 2, 64 x 80 per wave, 20 accumulators; 36 KB per stage, 2 stages, two workgroups per CU), with the per-16-byte-chunk
// im2col addressing of the bf16 gemm_dma_kernel.  K = tap * C + c (weights.pack_conv order, zero padded to Kp): a K-tile of 128
// channels straddles taps when C % 128 != 0 (C = 320 / 960), so each lane derives the tap of its OWN chunk; a 32-channel block never
// straddles a tap (C % 32 == 0), so the 32 k values of an MFMA lane share one exponent.
// Scale bytes: lane (frow, g) of row fragment i needs the exponent of (its row, the tap and block of k = 128 kt + 32 g).  Its four
// bytes (four row fragments) are per-lane byte loads issued together with the DMA of the same K-tile, one K-step ahead: the
// vmcnt(0) that retires the tile retires them too, so the K loop never waits on them separately.  Packed into one VGPR, op_sel
// picks byte i for row fragment i.  Taps outside the image, the K padding and rows >= M read zero data and a zero byte.
#include "common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

template <int SEL>
__device__ __forceinline__ f32x4 mma_mx(const i32x8& w, const i32x8& x, const f32x4& c, int sx) {
  // weights as the A operand (a lane ends up with 4 consecutive output channels of one pixel); formats 0 / 0 = e4m3; A scale 127
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, 0, 0, 0, 127, SEL, sx);
}

// source-pixel offset of tap t (0..8) of a 3x3 / pad 1 window, in pixels
__device__ __forceinline__ int tap_pixoff(int t, int W) {
  const int dy = (t * 11) >> 5;                      // t / 3 for t < 12
  return (dy - 1) * W + (t - 3 * dy - 1);
}

__device__ __forceinline__ int window_mask(int m, int M, int hw, int H, int W) {
  int mask = 0;
  if (m < M) {
    const int rem = m % hw;
    const int oy = rem / W, ox = rem - oy * W;
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)
        if ((unsigned)(oy + ty - 1) < (unsigned)H && (unsigned)(ox + tx - 1) < (unsigned)W) mask |= 1 << (ty * 3 + tx);
  }
  return mask;
}

__global__ __launch_bounds__(256, 2) void conv3x3_mx_kernel(const SaspaConvMxParams p) {
  constexpr int BM = 128, BN = 160, STAGE = (BM + BN) * 8;   // u32x4 per stage
  __shared__ u32x4 lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int frow = lane & 15, fg = lane >> 4;
  const int nbn = p.N / BN;
  const int hw = p.h * p.w, M = p.batch * hw, C = p.C;
  // XCD-aware order: blocks congruent mod 8 (one XCD) walk neighbouring tiles (same activation rows -> same L2)
  int tile;
  {
    const int G = gridDim.x, L = blockIdx.x;
    const int qd = G >> 3, rr = G & 7, xcd = L & 7, idx = L >> 3;
    tile = (xcd < rr ? xcd * (qd + 1) : rr * (qd + 1) + (xcd - rr) * qd) + idx;
  }
  const int bm = tile / nbn, bn = tile - bm * nbn;
  const rsrc_t rsa = make_rsrc(p.q), rsw = make_rsrc(p.w8), rss = make_rsrc(p.qs);
  // DMA pieces: tile row r0 + 32 i, logical 16-byte chunk kcs of the K-tile
  const int r0 = tid >> 3;
  const int kcs = (tid & 7) ^ (r0 & 7);
  unsigned basea[4], offb[5];
  int maska[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = bm * BM + r0 + 32 * i;
    basea[i] = (unsigned)m * (unsigned)p.ldq;          // rows >= M: never used (mask 0)
    maska[i] = window_mask(m, M, hw, p.h, p.w);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) offb[i] = (unsigned)((bn * BN + r0 + 32 * i) * p.ldw + kcs * 16);
  // scale bytes: the lane's MFMA rows wm * 64 + 16 i + frow
  unsigned bases[4];
  int masks[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = bm * BM + wm * 64 + 16 * i + frow;
    bases[i] = (unsigned)m * (unsigned)p.ldqs;
    masks[i] = window_mask(m, M, hw, p.h, p.w);
  }
  // (tap, channel) of the lane's DMA chunk and of its MFMA block in the NEXT K-tile to load, advanced by 128 channels per tile
  int ta = (kcs * 16) / C, ca = kcs * 16 - ta * C;
  int ts = (32 * fg) / C, cs = 32 * fg - ts * C;
  unsigned sb[4];
  auto load_tile = [&](int kt, int stage) __attribute__((always_inline)) {
    u32x4* la = lds + stage * STAGE;
    u32x4* lb = la + BM * 8;
    const unsigned tapa = (unsigned)(tap_pixoff(ta, p.w) * p.ldq + ca);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = ((maska[i] >> ta) & 1) != 0;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (lds_void_t*)(la + (32 * i + 8 * wave) * 8), 16, (int)(ok ? basea[i] + tapa : kInvalid),
                                               0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void_t*)(lb + (32 * i + 8 * wave) * 8), 16, (int)offb[i], kt * 128, 0, 0);
    const unsigned taps = (unsigned)(tap_pixoff(ts, p.w) * p.ldqs + (cs >> 5));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = ((masks[i] >> ts) & 1) != 0;
      sb[i] = __builtin_amdgcn_raw_buffer_load_b8(rss, (int)(ok ? bases[i] + taps : kInvalid), 0, 0);
    }
    ca += 128;
    while (ca >= C) { ca -= C; ++ta; }
    cs += 128;
    while (cs >= C) { cs -= C; ++ts; }
  };
  f32x4 acc[4][5];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // operand bytes of lane group g: 16-byte chunks g and g + 4 of the K-tile's row.  The instruction reads VGPRs 0-3 of group g as
  // k = 16 g .. 16 g + 15 and VGPRs 4-7 as k = 64 + 16 g .. + 15, and applies the scale of group b to k = 32 b .. 32 b + 31: chunks
  // (g, g + 4) put the two halves of ONE 32-channel block (2 b, 2 b + 1) under the scale lane group b supplies for block b
  auto frag = [&](const u32x4* base, int row) __attribute__((always_inline)) {
    const u32x4 c0 = base[row * 8 + (fg ^ (row & 7))];
    const u32x4 c1 = base[row * 8 + ((fg + 4) ^ (row & 7))];
    return i32x8{(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], (int)c1[2], (int)c1[3]};
  };
  const int nk = p.Kp / 128;
  load_tile(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                     // K-tile kt (and its scale bytes) landed for everyone; the other stage is free
    asm volatile("" ::: "memory");
    const int sx = (int)(sb[0] | (sb[1] << 8) | (sb[2] << 16) | (sb[3] << 24));
    if (kt + 1 < nk) load_tile(kt + 1, (kt + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);                // issue the loads before the MFMA block so that they fly under it
    const u32x4* la = lds + (kt & 1) * STAGE;
    const u32x4* lb = la + BM * 8;
    i32x8 xa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xa[i] = frag(la, wm * 64 + i * 16 + frow);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const i32x8 wb = frag(lb, wn * 80 + j * 16 + frow);
      acc[0][j] = mma_mx<0>(wb, xa[0], acc[0][j], sx);
      acc[1][j] = mma_mx<1>(wb, xa[1], acc[1][j], sx);
      acc[2][j] = mma_mx<2>(wb, xa[2], acc[2][j], sx);
      acc[3][j] = mma_mx<3>(wb, xa[3], acc[3][j], sx);
    }
  }
  __syncthreads();
  // ---- epilogue: weight scale + bias + time-embedding row, rounded to bf16 in an LDS tile; whole-row 16-byte stores with the
  // residual added there (the rounding points of the bf16 conv's epilogue); GroupNorm statistics of the stored values ----
  constexpr int CP = BN + 8;
  bf16_t* ct = reinterpret_cast<bf16_t*>(lds);
  float4 sw4[5], b4[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int n = bn * BN + wn * 80 + j * 16 + fg * 4;
    sw4[j] = *reinterpret_cast<const float4*>(p.sw + n);
    b4[j] = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mrow = wm * 64 + i * 16 + frow;
    const int m = bm * BM + mrow;
    const float* rv = (p.rowvec && m < M) ? p.rowvec + (long long)(m / hw) * p.ldrv : nullptr;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int ncol = wn * 80 + j * 16 + fg * 4;
      float4 a = b4[j];
      if (rv) {
        const float4 r4 = *reinterpret_cast<const float4*>(rv + bn * BN + ncol);
        a.x += r4.x; a.y += r4.y; a.z += r4.z; a.w += r4.w;
      }
      const float v[4] = {acc[i][j][0] * sw4[j].x + a.x, acc[i][j][1] * sw4[j].y + a.y, acc[i][j][2] * sw4[j].z + a.z,
                          acc[i][j][3] * sw4[j].w + a.w};
      Elem<bf16_t>::store4(ct + mrow * CP + ncol, v);
    }
  }
  __syncthreads();
  bf16_t* out = reinterpret_cast<bf16_t*>(p.out);
  const bf16_t* res = reinterpret_cast<const bf16_t*>(p.residual);
  constexpr int CPR = BN / 8;
  for (int q = tid; q < BM * CPR; q += 256) {
    const int row = q / CPR, ch = q - row * CPR;
    const int m = bm * BM + row, n = bn * BN + ch * 8;
    if (m >= M) continue;
    u32x4 c4 = *reinterpret_cast<const u32x4*>(ct + row * CP + ch * 8);
    if (res) {
      float a[8], r[8];
      unpack8(__builtin_bit_cast(uint4, c4), a);
      Elem<bf16_t>::load_chunk(res + (long long)m * p.ldr + n, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += r[e];
      c4 = __builtin_bit_cast(u32x4, pack8(a));
      if (p.gn_stats) *reinterpret_cast<u32x4*>(ct + row * CP + ch * 8) = c4;   // the statistics read the STORED values
    }
    *reinterpret_cast<u32x4*>(out + (long long)m * p.ldo + n) = c4;
  }
  if (p.gn_stats) {
    // SaspaGemmParams.gn_stats layout: BM = 128 rows = one statistics block, 160 % gn_unit == 0 (host check)
    __syncthreads();
    gn_tile_stats<256>(ct, CP, min(BM, M - bm * BM), BN / p.gn_unit, p.gn_unit, reinterpret_cast<float*>(ct + BM * CP),
                       p.gn_stats + ((long long)bm * (p.N / p.gn_unit) + (bn * BN) / p.gn_unit) * 2);
  }
}

// shape and pitch rules (pointers only where given: _eligible is asked before the operands exist)
int check_conv_mx(const SaspaConvMxParams& p) {
  if (p.batch <= 0 || p.h <= 0 || p.w <= 0 || p.C <= 0 || p.N <= 0 || p.Kp <= 0) return SASPA_EINVAL;
  if (p.kh != 3 || p.kw != 3 || p.stride != 1 || p.pad != 1 || p.upsample) return SASPA_ERANGE;
  // Kp: the 9 C taps padded to the NEXT whole K-tile only -- a longer padding would walk the lanes' tap index past the 9 bits of
  // their window masks
  if (p.C % 32 || p.N % 160 || p.Kp % 128 || p.Kp < 9 * p.C || p.Kp >= 9 * p.C + 128) return SASPA_ERANGE;
  if (p.gn_stats && (p.gn_unit <= 0 || p.gn_unit % 2 || p.gn_unit > 16 || 80 % p.gn_unit)) return SASPA_ERANGE;
  const long long M = (long long)p.batch * p.h * p.w;
  if (M >= (1ll << 30) || M * p.ldq >= (1ll << 31) || M * p.ldqs >= (1ll << 31) || (long long)p.N * p.ldw >= (1ll << 31))
    return SASPA_ERANGE;                                                                          // 32-bit buffer offsets
  if (p.ldq % 16 || p.ldq < p.C || p.ldqs < p.C / 32 || p.ldw % 16 || p.ldw < p.Kp) return SASPA_EALIGN;
  if (p.ldo % 8 || p.ldo < p.N || (p.residual && (p.ldr % 8 || p.ldr < p.N)) || (p.rowvec && p.ldrv % 4)) return SASPA_EALIGN;
  if ((p.q && !aligned16(p.q)) || (p.w8 && !aligned16(p.w8)) || (p.out && !aligned16(p.out)) || (p.sw && !aligned16(p.sw)) ||
      (p.bias && !aligned16(p.bias)) || (p.rowvec && !aligned16(p.rowvec)) || (p.residual && !aligned16(p.residual)) ||
      (reinterpret_cast<uintptr_t>(p.gn_stats) & 7u))
    return SASPA_EALIGN;
  return 0;
}

}  // namespace

extern "C" int saspa_conv3x3_mxfp8_eligible(const SaspaConvMxParams* p) { return p && check_conv_mx(*p) == 0 ? 1 : 0; }

extern "C" int saspa_conv3x3_mxfp8(const SaspaConvMxParams* pp, void* stream) {
  if (!pp) return SASPA_EINVAL;
  const SaspaConvMxParams& p = *pp;
  if (!p.q || !p.qs || !p.w8 || !p.sw || !p.out) return SASPA_EINVAL;
  if (int e = check_conv_mx(p)) return e;
  const int M = p.batch * p.h * p.w;
  const int tiles = ((M + 127) / 128) * (p.N / 160);
  hipLaunchKernelGGL(conv3x3_mx_kernel, dim3(tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  SASPA_CHECK_LAUNCH();
  return 0;
}
