// Fused single-head attention for WIDE heads (192 <= d <= 512, d % 64 == 0): the 512-channel mid-block attention of the VAE in one
// launch, no score matrix in memory, no logit ever rounded to 16 bits.  See include/saspa_hip.h (saspa_attn_wide).
//
// 32 query rows x 512 fp32 output columns is 256 accumulator registers per lane before any operand, so one wave cannot own a row
// block's output.  A workgroup of four waves takes 32 queries and splits the HEAD DIMENSION four ways, twice:
//   S^T = K Q^T      each wave sums over ITS 32-channel steps (step s belongs to wave s % 4) and leaves a partial 32 x 32 fp32 tile in
//                    LDS; after a barrier every wave adds the four partials in the same fixed order, so all four hold bit-identical
//                    logits and run the same online softmax (fp32 logits, maximum, sum and rescale; scale * log2 e applied to the
//                    fp32 logit) redundantly -- 8 exponentials per lane and tile -- instead of exchanging m / l / P.
//   O^T += V^T P^T   each wave owns d / 4 output channels: its slice of V (read transposed from the row-major LDS tile with
//                    ds_read_b64_tr_b16, as saspa_attn's row-major-V kernels do) and of the fp32 accumulator.
// Both products are v_mfma_f32_16x16x32 (MFMA_16X16X32): operand lane maps A[row l & 15][k 8 (l >> 4) + j], B[k 8 (l >> 4) + j][col l & 15],
// C[row 4 (l >> 4) + reg][col l & 15].  With r = l & 15 and g = l >> 4:
//   S^T tile   A = K[key 16 kb + r][32 s + 8 g + j], B = Q[query 16 qb + r][32 s + 8 g + j]   ->  C = S[query r][keys 16 kb + 4 g + 0..3]
//   reduced    lane (r, g) reads S[query r][4 g + 0..3] and S[query r][16 + 4 g + 0..3]: k index 8 g + j of the PV step stands for
//              key 16 (j >> 2) + 4 g + (j & 3) in BOTH operands (any fixed permutation of a k-step's keys is a valid product)
//   O^T tile   A = V^T[channel c0 + r][those keys] (two transposed reads: key rows 4 g .. and 16 + 4 g ..), B = P packed
//              ->  C = O[query r][channels c0 + 4 g + 0..3]: the query is on the lane in S, P and O alike, so m, l and the rescale
//              factor are per-lane scalars and the store is one 8-byte piece per accumulator.
// LDS images (32 keys per tile): K rows unpadded, 16-byte chunk c of key row k at chunk c ^ (k & 7) (the b128 fragment reads of 16
// rows spread over 8 chunk columns); V rows likewise with 32-byte units u ^ (k & 7) where d % 128 == 0 (a 32-lane half of the transposed
// read takes 8 key rows of one unit: 8 distinct units = all 64 banks), padded to 8 banks past a multiple of 64 otherwise; the four
// partial S tiles with chunk c ^ (query & 7).  At d = 512 that is 32 + 32 + 16 KiB: two workgroups per CU.
#include "common.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x2 lds_read_tr16(const unsigned char* ptr) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ptr)));
}

constexpr int kBQ = 32;   // queries per workgroup
constexpr int kKT = 32;   // keys per tile
constexpr int kNW = 4;    // waves per workgroup: the head dimension is split over them

constexpr int v_pitch(int d) {
  if (d % 128 == 0) return d * 2;           // swizzled, no pad
  int b = d * 2;
  while ((b / 4) % 64 != 8) b += 16;        // rows 8 banks apart: 8 key rows x 8 banks = the 64 banks once
  return b;
}

template <int D>
__global__ __launch_bounds__(64 * kNW, 2) void attn_wide_kernel(const h16_t* __restrict__ q, const h16_t* __restrict__ k,
                                                                const h16_t* __restrict__ v, h16_t* __restrict__ o, const int nq,
                                                                const int nk, const int ldq, const int ldk, const int ldv,
                                                                const int ldo, const long long sqb, const long long skb,
                                                                const long long svb, const long long sob, const float c) {
  constexpr int NSTEP = D / 32;                 // 32-channel steps of the QK^T sum
  constexpr int MAXS = (NSTEP + kNW - 1) / kNW; // ... per wave
  constexpr int NCB = D / 64;                   // 16-channel output blocks per wave
  constexpr int DW = D / kNW;                   // output channels per wave
  constexpr int CH = D / 8;                     // 16-byte chunks per K / V row (a multiple of 8)
  constexpr int NCH = kKT * CH / (64 * kNW);    // chunks per thread and operand = D / 64
  constexpr bool VSW = D % 128 == 0;
  constexpr int KP = D * 2, VP = v_pitch(D);    // bytes per key row
  constexpr int K_BYTES = kKT * KP, V_BYTES = kKT * VP;
  constexpr int S_BYTES = kNW * kBQ * kKT * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[K_BYTES + V_BYTES + S_BYTES];
  unsigned char* ksm = smem;
  unsigned char* vsm = smem + K_BYTES;
  unsigned char* ssm = smem + K_BYTES + V_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * kBQ;
  const h16_t* Q = q + b * sqb;
  const h16_t* K = k + b * skb;
  const h16_t* V = v + b * svb;
  h16_t* O = o + b * sob;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // ---- Q fragments of this wave's channel steps (B operand), resident ----
  u32x4 qf[MAXS][2];
#pragma unroll
  for (int i = 0; i < MAXS; ++i)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int s = w + kNW * i, qi = q0 + 16 * qb + r;
      qf[i][qb] = (s < NSTEP && qi < nq) ? *reinterpret_cast<const u32x4*>(Q + (long long)qi * ldq + 32 * s + 8 * g) : zero4;
    }

  // ---- staging: thread (key row tid >> 3, chunk lane tid & 7) moves chunks (tid & 7) + 8 i, i < NCH, of its key row: one global
  //      and one LDS base per operand, everything else is an immediate offset.  Key rows >= nk are zeros.  ONE register set: K of
  //      tile t+1 travels during the QK^T of tile t, V of tile t+1 during its softmax and PV (see the loop) ----
  static_assert(CH == 8 * NCH && 64 * kNW == 8 * kKT, "eight threads per key row");
  const int skey = tid >> 3, scl = tid & 7, sk7 = skey & 7;
  const int st_k = skey * KP + ((scl ^ sk7) << 4);                       // + 128 i: the XOR touches chunk bits 0..2 only
  // swizzled V: byte (ch << 4) ^ (k7 << 5) with ch = scl + 8 i  ==  [((scl >> 1) ^ (k7 & 3)) << 5 | (scl & 1) << 4] + 128 (i ^ (k7 >> 2))
  const int st_vb = skey * VP + (VSW ? (((((scl >> 1) ^ (sk7 & 3)) << 5) | ((scl & 1) << 4))) : (scl << 4));
  const int st_v0 = st_vb + (VSW ? 128 * (sk7 >> 2) : 0);                // chunk group i even (VSW) / every i
  const int st_v1 = st_vb + 128 * (1 - (sk7 >> 2)) - 128;                // VSW, i odd: + 128 (i - 1) + this
  const int go_k = skey * ldk + scl * 8, go_v = skey * ldv + scl * 8;    // elements inside a tile; the tile's base is wave-uniform
  u32x4 sreg[NCH];
  auto load_rows = [&](const h16_t* base, int go, int key0) __attribute__((always_inline)) {
    const bool ok = key0 + skey < nk;
#pragma unroll
    for (int i = 0; i < NCH; ++i) sreg[i] = ok ? *reinterpret_cast<const u32x4*>(base + go + 64 * i) : zero4;
  };
  auto store_k = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) *reinterpret_cast<u32x4*>(ksm + st_k + 128 * i) = sreg[i];
  };
  auto store_v = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      *reinterpret_cast<u32x4*>(vsm + ((VSW && (i & 1)) ? st_v1 : st_v0) + 128 * i) = sreg[i];
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
  float m_run[2] = {-1e30f, -1e30f};     // running maximum of this lane's query (x c), per query block
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
          const u32x4 kf = *reinterpret_cast<const u32x4*>(ksm + ka_row + 16 * kb * KP + (((4 * s + g) ^ ka_x) << 4));
#pragma unroll
          for (int qb = 0; qb < 2; ++qb) sp[kb][qb] = MFMA_16X16X32(kf, qf[i][qb], sp[kb][qb]);
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
    u32x4 pf[2];
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
        for (int e = 0; e < 4; ++e) sv[4 * hlf + e] = a[e];
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
      const float m_new = fmaxf(m_run[qb], mx * c);
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
        pv[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[j], c, -m_run[qb]));
        psum += pv[j];
      }
      l_run[qb] += psum;
      pf[qb] = u32x4{pack2(pv[0], pv[1]), pack2(pv[2], pv[3]), pack2(pv[4], pv[5]), pack2(pv[6], pv[7])};
    }

    // ---- O^T += V^T P^T on this wave's channels ----
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int cbyte = (w * DW + 16 * cb) * 2;            // a multiple of 32
      const unsigned char* blk = vsm + vt_row + ((cbyte ^ vt_x) + vt_lo);
      const u32x2 lo = lds_read_tr16(blk);
      const u32x2 hi = lds_read_tr16(blk + 16 * VP);
      const u32x4 vf = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) acc[cb][qb] = MFMA_16X16X32(vf, pf[qb], acc[cb][qb]);
    }
  }

  // ---- normalise and store: lane holds O[query 16 qb + r][w DW + 16 cb + 4 g + 0..3] ----
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    float l = l_run[qb];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    const int qi = q0 + 16 * qb + r;
    if (qi < nq) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const float vals[4] = {acc[cb][qb][0] * inv, acc[cb][qb][1] * inv, acc[cb][qb][2] * inv, acc[cb][qb][3] * inv};
        Elem<h16_t>::store4(O + (long long)qi * ldo + w * DW + 16 * cb + 4 * g, vals);
      }
    }
  }
}

template <int D>
int launch_wide(const void* q, const void* k, const void* v, void* o, int batch, int nq, int nk, int ldq, int ldk, int ldv, int ldo,
                long long sqb, long long skb, long long svb, long long sob, float scale, hipStream_t s) {
  const dim3 grid((unsigned)((nq + kBQ - 1) / kBQ), (unsigned)batch);
  hipLaunchKernelGGL(attn_wide_kernel<D>, grid, dim3(64 * kNW), 0, s, reinterpret_cast<const h16_t*>(q),
                     reinterpret_cast<const h16_t*>(k), reinterpret_cast<const h16_t*>(v), reinterpret_cast<h16_t*>(o), nq, nk, ldq,
                     ldk, ldv, ldo, sqb, skb, svb, sob, scale * 1.4426950408889634f);
  SASPA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int saspa_attn_wide(int dtype, const void* q, int ldq, long long sqb, const void* k, int ldk, long long skb, const void* v,
                               int ldv, long long svb, void* out, int ldo, long long sob, int batch, int nq, int nk, int d, float scale,
                               void* stream) {
  if (!q || !k || !v || !out) return SASPA_EINVAL;
  if (dtype != SASPA_HALF) return SASPA_EINVAL;
  if (batch <= 0 || batch > 65535 || nq <= 0 || nk <= 0) return SASPA_EINVAL;
  if (d < 192 || d > 512 || d % 64) return SASPA_EINVAL;      // narrower heads: saspa_flash_attn_bf16
  if (ldq < d || ldk < d || ldv < d || ldo < d) return SASPA_EINVAL;
  if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8 || sqb % 8 || skb % 8 || svb % 8 || sob % 8) return SASPA_EALIGN;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define SASPA_WIDE(D_) \
  case D_: return launch_wide<D_>(q, k, v, out, batch, nq, nk, ldq, ldk, ldv, ldo, sqb, skb, svb, sob, scale, s)
  switch (d) {
    SASPA_WIDE(192);
    SASPA_WIDE(256);
    SASPA_WIDE(320);
    SASPA_WIDE(384);
    SASPA_WIDE(448);
    SASPA_WIDE(512);
    default: break;
  }
#undef SASPA_WIDE
  return SASPA_EINVAL;
}
