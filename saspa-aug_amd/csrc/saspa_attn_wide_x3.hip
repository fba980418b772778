// Fused single-head attention for WIDE heads (192 <= d <= 512, d % 64 == 0) on fp32 STORAGE with x3 products: the cross of
// saspa_attn_wide (the layout) and saspa_flash_attn_f32x3 (the arithmetic).  The 512-channel mid-block attention of the fp32 VAE in one
// launch, no n x n score matrix in memory.  See include/saspa_hip.h (saspa_attn_wide_f32x3).
//
// Layout, as saspa_attn_wide.hip (read its header for the lane maps; they are the same, operand for operand): a workgroup of four
// waves takes 32 queries and 32-key tiles and splits the HEAD DIMENSION four ways, twice:
//   S^T = K Q^T      wave w sums over the 32-channel steps s with s % 4 == w and leaves a partial 32 x 32 fp32 tile in LDS; behind a
//                    barrier every wave adds the four partials in wave order, so all four hold bit-identical logits and run the same
//                    fp32 online softmax redundantly
//   O^T += V^T P^T   wave w owns output channels w d/4 .. (w + 1) d/4: its slice of V (read transposed from the row-major LDS tile with
//                    ds_read_b64_tr_b16) and of the fp32 accumulator
// Arithmetic, as saspa_attn_x3.hip: K and V of a tile are split ONCE, between the staging registers and LDS, into a bf16 "hi" and a bf16
// "lo" plane (split2: hi = bf16(x), lo = bf16(x - hi), round to nearest); Q is split once into resident registers; P is split from its
// fp32 value and never rounded to one bf16.  Every product sum is lo hi + hi lo + hi hi (run3) on v_mfma_f32_16x16x32_bf16 with one fp32
// accumulator; t = S c (c = scale log2 e) is an fp32 product, the running maximum, p = exp2(t - m), the row sum and the rescale are fp32;
// O is divided by the fp32 row sum.  Every sum has a fixed order (MFMA chains over a wave's channel steps / the key tiles, the four
// partials in wave order, a lane's 8 weights in register order, the four lane groups last); nothing is atomic; a workgroup reads one
// batch entry only.
// LDS: the K and V images of saspa_attn_wide (K rows unpadded with 16-byte chunk c of key k at c ^ (k & 7); V rows swizzled in 32-byte
// units where d % 128 == 0, padded otherwise), two planes each, and the four partial S tiles: 2 x 32 + 2 x 32 + 16 = 144 KiB at d = 512
// (one workgroup per CU), 64 KiB at d = 192.  Key rows >= nk are never read from memory: their K and V rows are zeros in LDS and their
// logits are -inf.
#include "common.h"

#ifdef SASPA_HALF_F16
#error "saspa_attn_wide_x3.hip splits fp32 into bf16 pairs: it belongs to the default library only"
#endif

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x2 lds_read_tr16(const unsigned char* ptr) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ptr)));
}

constexpr int kBQ = 32;   // queries per workgroup
constexpr int kKT = 32;   // keys per tile
constexpr int kNW = 4;    // waves per workgroup: the head dimension is split over them

constexpr int v_pitch(int d) {               // bytes per key row of ONE bf16 plane, as saspa_attn_wide.hip
  if (d % 128 == 0) return d * 2;            // swizzled, no pad
  int b = d * 2;
  while ((b / 4) % 64 != 8) b += 16;         // rows 8 banks apart: 8 key rows x 8 banks = the 64 banks once
  return b;
}

// two fp32 values -> their packed bf16 hi pair and lo pair (round to nearest), as Mma<f32x3_t>::split does
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack2(a, b);
  lo = pack2(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}
// eight consecutive fp32 values -> one 16-byte bf16 chunk of the hi plane and one of the lo plane
__device__ __forceinline__ void split8(const float4& a, const float4& b, u32x4& hi, u32x4& lo) {
  uint32_t h0, h1, h2, h3, l0, l1, l2, l3;
  split2(a.x, a.y, h0, l0);
  split2(a.z, a.w, h1, l1);
  split2(b.x, b.y, h2, l2);
  split2(b.z, b.w, h3, l3);
  hi = u32x4{h0, h1, h2, h3};
  lo = u32x4{l0, l1, l2, l3};
}
// Mma<f32x3_t>::run3 on the 16x16x32 tile: lo hi, hi lo, hi hi
__device__ __forceinline__ void run3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl, f32x4& acc) {
  acc = MFMA_16X16X32(al, bh, acc);
  acc = MFMA_16X16X32(ah, bl, acc);
  acc = MFMA_16X16X32(ah, bh, acc);
}

template <int D>
__global__ __launch_bounds__(64 * kNW) void attn_wide_x3_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, float* __restrict__ o, const int nq,
                                                                const int nk, const int ldq, const int ldk, const int ldv,
                                                                const int ldo, const long long sqb, const long long skb,
                                                                const long long svb, const long long sob, const float c) {
  constexpr int NSTEP = D / 32;                 // 32-channel steps of the QK^T sum
  constexpr int MAXS = (NSTEP + kNW - 1) / kNW; // ... per wave
  constexpr int NCB = D / 64;                   // 16-channel output blocks per wave
  constexpr int DW = D / kNW;                   // output channels per wave
  constexpr int CH = D / 8;                     // 8-element chunks per K / V row (a multiple of 8): 16 bytes per bf16 plane
  constexpr int NCH = kKT * CH / (64 * kNW);    // chunks per thread and operand = D / 64
  constexpr bool VSW = D % 128 == 0;
  constexpr int KP = D * 2, VP = v_pitch(D);    // bytes per key row of one plane
  constexpr int K_PLANE = kKT * KP, V_PLANE = kKT * VP;
  constexpr int S_BYTES = kNW * kBQ * kKT * 4;
  static_assert(2 * K_PLANE + 2 * V_PLANE + S_BYTES <= 160 * 1024, "gfx950: 160 KiB of LDS per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * K_PLANE + 2 * V_PLANE + S_BYTES];
  unsigned char* ksm = smem;                              // hi plane, lo plane at + K_PLANE
  unsigned char* vsm = smem + 2 * K_PLANE;                // hi plane, lo plane at + V_PLANE
  unsigned char* ssm = smem + 2 * K_PLANE + 2 * V_PLANE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * kBQ;
  const float* Q = q + b * sqb;
  const float* K = k + b * skb;
  const float* V = v + b * svb;
  float* O = o + b * sob;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // ---- Q fragments of this wave's channel steps (B operand), split once, resident: channels 32 s + 8 g + 0..7 of query 16 qb + r ----
  u32x4 qh[MAXS][2], ql[MAXS][2];
#pragma unroll
  for (int i = 0; i < MAXS; ++i)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int s = w + kNW * i, qi = q0 + 16 * qb + r;
      float4 a = zero4, bb = zero4;
      if (s < NSTEP && qi < nq) {
        const float* src = Q + (long long)qi * ldq + 32 * s + 8 * g;
        a = *reinterpret_cast<const float4*>(src);
        bb = *reinterpret_cast<const float4*>(src + 4);
      }
      split8(a, bb, qh[i][qb], ql[i][qb]);
    }

  // ---- staging: thread (key row tid >> 3, chunk lane tid & 7) moves the 8-element chunks (tid & 7) + 8 i, i < NCH, of its key row:
  //      two float4 loads each, split on the way into the two LDS planes.  Key rows >= nk are zeros and are not read.  ONE register
  //      set: K of tile t+1 travels during the QK^T of tile t, V of tile t+1 during its softmax and PV (see the loop) ----
  static_assert(CH == 8 * NCH && 64 * kNW == 8 * kKT, "eight threads per key row");
  const int skey = tid >> 3, scl = tid & 7, sk7 = skey & 7;
  const int st_k = skey * KP + ((scl ^ sk7) << 4);                       // + 128 i: the XOR touches chunk bits 0..2 only
  // swizzled V: byte (ch << 4) ^ (k7 << 5) with ch = scl + 8 i  ==  [((scl >> 1) ^ (k7 & 3)) << 5 | (scl & 1) << 4] + 128 (i ^ (k7 >> 2))
  const int st_vb = skey * VP + (VSW ? (((((scl >> 1) ^ (sk7 & 3)) << 5) | ((scl & 1) << 4))) : (scl << 4));
  const int st_v0 = st_vb + (VSW ? 128 * (sk7 >> 2) : 0);                // chunk group i even (VSW) / every i
  const int st_v1 = st_vb + 128 * (1 - (sk7 >> 2)) - 128;                // VSW, i odd: + 128 (i - 1) + this
  const int go_k = skey * ldk + scl * 8, go_v = skey * ldv + scl * 8;    // elements inside a tile; the tile's base is wave-uniform
  float4 sreg[NCH][2];
  auto load_rows = [&](const float* base, int go, int key0) __attribute__((always_inline)) {
    const bool ok = key0 + skey < nk;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      sreg[i][0] = ok ? *reinterpret_cast<const float4*>(base + go + 64 * i) : zero4;
      sreg[i][1] = ok ? *reinterpret_cast<const float4*>(base + go + 64 * i + 4) : zero4;
    }
  };
  auto store_k = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      u32x4 hi, lo;
      split8(sreg[i][0], sreg[i][1], hi, lo);
      *reinterpret_cast<u32x4*>(ksm + st_k + 128 * i) = hi;
      *reinterpret_cast<u32x4*>(ksm + K_PLANE + st_k + 128 * i) = lo;
    }
  };
  auto store_v = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      u32x4 hi, lo;
      split8(sreg[i][0], sreg[i][1], hi, lo);
      const int at = ((VSW && (i & 1)) ? st_v1 : st_v0) + 128 * i;
      *reinterpret_cast<u32x4*>(vsm + at) = hi;
      *reinterpret_cast<u32x4*>(vsm + V_PLANE + at) = lo;
    }
  };

  // per-lane LDS addresses
  // K fragment of step s, key block kb: row 16 kb + r, chunk 4 s + g  (row & 7 == r & 7)
  const int ka_row = r * KP, ka_x = r & 7;
  // S partial tile: [wave][query 0..31][32 keys] fp32, 16-byte chunk cc of a query row at cc ^ (query & 7)
  const int sw_base = (w * kBQ + r) * (kKT * 4);            // + 16 qb rows; chunk 4 kb + g
  // V^T fragment: key rows 4 g + (r >> 2) (+ 16), channels c0 + 4 (r & 3) ..; (row & 7) = 4 (g & 1) + (r >> 2) for both reads
  const int vt_row = (4 * g + (r >> 2)) * VP;
  const int vt_x = VSW ? ((4 * (g & 1) + (r >> 2)) << 5) : 0;
  const int vt_lo = 8 * (r & 3);

  f32x4 acc[NCB][2];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) acc[cb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-1e30f, -1e30f};     // running maximum of this lane's query (log2 domain), per query block
  float l_run[2] = {0.f, 0.f};           // this lane's share (its 8 keys of every tile) of the running sum

  const int ntiles = (nk + kKT - 1) / kKT;
  // Two barriers per tile.  Behind barrier A(t) every wave has finished PV(t-1): the V region is free and K(t) (stored behind
  // barrier B(t-1)) is visible.  Behind barrier B(t) every wave has finished reading K(t) and has written its partial logits:
  // the K region is free, V(t) (stored behind A(t)) and the partials are visible.  The partials are rewritten behind A(t+1).
  load_rows(K, go_k, 0);
  store_k();
  load_rows(V, go_v, 0);
  for (int t = 0; t < ntiles; ++t) {
    const int key0 = t * kKT;
    __syncthreads();                      // A(t)
    store_v();
    if (t + 1 < ntiles) load_rows(K + (long long)(key0 + kKT) * ldk, go_k, key0 + kKT);   // in flight during QK^T

    // ---- this wave's partial S^T = K Q^T over its channel steps ----
    f32x4 sp[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) sp[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
      const int s = w + kNW * i;
      if (NSTEP % kNW == 0 || s < NSTEP) {        // wave-uniform
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const unsigned char* src = ksm + ka_row + 16 * kb * KP + (((4 * s + g) ^ ka_x) << 4);
          const u32x4 kh = *reinterpret_cast<const u32x4*>(src);
          const u32x4 kl = *reinterpret_cast<const u32x4*>(src + K_PLANE);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) run3(kh, kl, qh[i][qb], ql[i][qb], sp[kb][qb]);
        }
      }
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
        *reinterpret_cast<f32x4*>(ssm + sw_base + 16 * qb * (kKT * 4) + (((4 * kb + g) ^ (r & 7)) << 4)) = sp[kb][qb];
    __syncthreads();                      // B(t)
    if (t + 1 < ntiles) {
      store_k();
      load_rows(V + (long long)(key0 + kKT) * ldv, go_v, key0 + kKT);                     // in flight during softmax and PV
    }

    // ---- the full logits of query 16 qb + r, keys 4 g .. 4 g + 3 and 16 + 4 g ..: the four partials in wave order ----
    u32x4 ph[2], pl[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float sv[8];
#pragma unroll
      for (int hlf = 0; hlf < 2; ++hlf) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ww = 0; ww < kNW; ++ww)
          a += *reinterpret_cast<const f32x4*>(ssm + ((ww * kBQ + 16 * qb + r) * (kKT * 4)) + (((4 * hlf + g) ^ (r & 7)) << 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[4 * hlf + e] = a[e] * c;             // the fp32 logit, log2 domain
      }
      if (key0 + kKT > nk) {              // wave-uniform: only the last tile holds keys >= nk
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (key0 + 16 * (j >> 2) + 4 * g + (j & 3) >= nk) sv[j] = -INFINITY;
      }
      float mx = sv[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) mx = fmaxf(mx, sv[j]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[qb], mx);
      if (__any(m_new > m_run[qb])) {     // some query's maximum moved: rescale what was accumulated at the old one
        const float alpha = __builtin_amdgcn_exp2f(m_run[qb] - m_new);
        m_run[qb] = m_new;
        l_run[qb] *= alpha;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb][qb] *= alpha;
      }
      float pv[8], psum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pv[j] = __builtin_amdgcn_exp2f(sv[j] - m_run[qb]);
        psum += pv[j];
      }
      l_run[qb] += psum;
      uint32_t h[4], l[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split2(pv[2 * j], pv[2 * j + 1], h[j], l[j]);   // P split from its fp32 value
      ph[qb] = u32x4{h[0], h[1], h[2], h[3]};
      pl[qb] = u32x4{l[0], l[1], l[2], l[3]};
    }

    // ---- O^T += V^T P^T on this wave's channels ----
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int cbyte = (w * DW + 16 * cb) * 2;            // a multiple of 32
      const unsigned char* blk = vsm + vt_row + ((cbyte ^ vt_x) + vt_lo);
      const u32x2 h0 = lds_read_tr16(blk);
      const u32x2 h1 = lds_read_tr16(blk + 16 * VP);
      const u32x2 l0 = lds_read_tr16(blk + V_PLANE);
      const u32x2 l1 = lds_read_tr16(blk + V_PLANE + 16 * VP);
      const u32x4 vh = {h0.x, h0.y, h1.x, h1.y};
      const u32x4 vl = {l0.x, l0.y, l1.x, l1.y};
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) run3(vh, vl, ph[qb], pl[qb], acc[cb][qb]);
    }
  }

  // ---- divide by the row sum and store: lane holds O[query 16 qb + r][w DW + 16 cb + 4 g + 0..3] ----
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float l = l_run[qb];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int qi = q0 + 16 * qb + r;
    if (qi < nq) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        *reinterpret_cast<float4*>(O + (long long)qi * ldo + w * DW + 16 * cb + 4 * g) =
            make_float4(acc[cb][qb][0] / l, acc[cb][qb][1] / l, acc[cb][qb][2] / l, acc[cb][qb][3] / l);
    }
  }
}

template <int D>
int launch_wide_x3(const float* q, const float* k, const float* v, float* o, int batch, int nq, int nk, int ldq, int ldk, int ldv,
                   int ldo, long long sqb, long long skb, long long svb, long long sob, float scale, hipStream_t s) {
  const dim3 grid((unsigned)((nq + kBQ - 1) / kBQ), (unsigned)batch);
  hipLaunchKernelGGL(attn_wide_x3_kernel<D>, grid, dim3(64 * kNW), 0, s, q, k, v, o, nq, nk, ldq, ldk, ldv, ldo, sqb, skb, svb, sob,
                     scale * 1.4426950408889634f);
  SASPA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int saspa_attn_wide_f32x3(const void* q, int ldq, long long sqb, const void* k, int ldk, long long skb, const void* v, int ldv,
                                     long long svb, void* out, int ldo, long long sob, int batch, int nq, int nk, int d, float scale,
                                     void* stream) {
  if (!q || !k || !v || !out) return SASPA_EINVAL;
  if (batch <= 0 || batch > 65535 || nq <= 0 || nk <= 0) return SASPA_EINVAL;
  if (d < 192 || d > 512 || d % 64) return SASPA_EINVAL;      // narrower heads: saspa_flash_attn_f32x3
  if (ldq < d || ldk < d || ldv < d || ldo < d) return SASPA_EINVAL;
  if (ldq % 4 || ldk % 4 || ldv % 4 || ldo % 4 || sqb % 4 || skb % 4 || svb % 4 || sob % 4) return SASPA_EALIGN;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define SASPA_WIDE_X3(D_)                                                                                                          \
  case D_:                                                                                                                         \
    return launch_wide_x3<D_>(reinterpret_cast<const float*>(q), reinterpret_cast<const float*>(k), reinterpret_cast<const float*>(v), \
                              reinterpret_cast<float*>(out), batch, nq, nk, ldq, ldk, ldv, ldo, sqb, skb, svb, sob, scale, s)
  switch (d) {
    SASPA_WIDE_X3(192);
    SASPA_WIDE_X3(256);
    SASPA_WIDE_X3(320);
    SASPA_WIDE_X3(384);
    SASPA_WIDE_X3(448);
    SASPA_WIDE_X3(512);
    default: break;
  }
#undef SASPA_WIDE_X3
  return SASPA_EINVAL;
}
