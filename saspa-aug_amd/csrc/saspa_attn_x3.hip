// Flash attention on fp32 STORAGE with x3 products (three bf16 MFMAs per product, SASPA_F32X3's arithmetic): the fused form of the fp32
// parity path's scores GEMM -> row softmax -> PV GEMM, no score matrix in memory.  See include/saspa_hip.h (saspa_flash_attn_f32x3).
//
// A workgroup of four waves takes 128 queries of one (batch entry, head), 32 per wave, and walks the keys in tiles of 64.  K and V^T of
// a tile are split ONCE, on the way into LDS, into a bf16 "hi" and a bf16 "lo" plane (hi = bf16(x), lo = bf16(x - hi): split2, the
// arithmetic of Mma<f32x3_t>::split in saspa_gemm.hip), so every fragment read is a plain 16-byte bf16 read; the head dimension pads to
// the MFMA's 16-channel step with zeros in LDS.  Q is split once per wave into resident registers.  Both products are
// v_mfma_f32_32x32x16_bf16 (MFMA_32X32X16), lane l = (r = l & 31, h = l >> 5): A[row r][k 8 h + j], B[k 8 h + j][col r],
// C[row 8 (i >> 2) + 4 h + (i & 3)][col r] in register i of 16.  Each product sum takes Mma<f32x3_t>::run3's order, lo hi + hi lo + hi hi,
// on one fp32 accumulator:
//   S^T = K Q^T      A = K[key 32 kb + r][16 s + 8 h + j], B = Q[query r][16 s + 8 h + j]  ->  C = S[query r][key 32 kb + 8 (i >> 2) + 4 h + (i & 3)]
//   softmax          the query is on the lane: fp32 logit t = S c (c = scale log2 e), running maximum m, p = exp2(t - m), row sum and
//                    the rescale factor are per-lane scalars; lanes l and l ^ 32 hold the two halves of a query's keys
//   O^T += V^T P^T   P is split from its fp32 value (never rounded to ONE bf16); registers 8 s' .. 8 s' + 7 of a key block are the B
//                    fragment of a 16-key step as they stand: element j of lane half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3), so the
//                    V^T image in LDS holds a step's keys in that order (bits 2 and 3 of the key index swapped) and A = V^T[channel
//                    32 cb + r] is one 16-byte read  ->  C = O[query r][channel 32 cb + 8 (i >> 2) + 4 h + (i & 3)]
// Every sum has a fixed order (MFMA chains over the channel / key steps, the lane's 32 weights in register order, the two lane halves
// last); nothing is atomic; a workgroup reads one batch entry only.
// LDS: K rows of 2 DP + 16 bytes, V^T rows of 144 bytes (pitch / 4 = 4 x odd: the 16 rows of a b128 read phase fall on distinct banks),
// two planes each: 32 KiB at d = 40, 87 KiB at d = 160.
#include "common.h"

#ifdef SASPA_HALF_F16
#error "saspa_attn_x3.hip splits fp32 into bf16 pairs: it belongs to the default library only"
#endif

namespace {

constexpr int kNW = 4;     // waves per workgroup
constexpr int kBQ = 32;    // queries per wave
constexpr int kKT = 64;    // keys per tile
constexpr int kVP = kKT * 2 + 16;   // bytes per V^T row (one plane)

// two fp32 values -> their packed bf16 hi pair and lo pair (round to nearest), as Mma<f32x3_t>::split does
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack2(a, b);
  lo = pack2(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}
// Mma<f32x3_t>::run3 on the 32x32x16 tile: lo hi, hi lo, hi hi
__device__ __forceinline__ void run3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl, f32x16& acc) {
  acc = MFMA_32X32X16(al, bh, acc);
  acc = MFMA_32X32X16(ah, bl, acc);
  acc = MFMA_32X32X16(ah, bh, acc);
}

template <int DP>   // the head dimension padded to a multiple of 16
__global__ __launch_bounds__(64 * kNW) void attn_x3_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ vt, float* __restrict__ o, const int heads,
                                                           const int D, const int nq, const int nk, const int ldq, const int ldk,
                                                           const int ldvt, const int ldo, const long long sqb, const long long skb,
                                                           const long long svb, const long long sob, const float c, const int causal,
                                                           const int nqb) {
  constexpr int NS = DP / 16;              // 16-channel steps of the QK^T sum
  constexpr int NCB = (DP + 31) / 32;      // 32-channel output blocks
  constexpr int KP = 2 * DP + 16;          // bytes per K row (one plane)
  constexpr int K_PLANE = kKT * KP;
  constexpr int V_ROWS = NCB * 32;
  constexpr int V_PLANE = V_ROWS * kVP;
  constexpr int KCH = DP / 4;              // float4 chunks per K row
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * K_PLANE + 2 * V_PLANE];
  unsigned char* ksm = smem;
  unsigned char* vsm = smem + 2 * K_PLANE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int bid = blockIdx.x;
  const int qb = bid % nqb, bh = bid / nqb;
  const int head = bh % heads, b = bh / heads;
  const int q0 = qb * (kBQ * kNW);         // first query of the workgroup
  const int q0w = q0 + w * kBQ;            // ... of this wave
  const int qi = q0w + r;                  // this lane's query
  const float* Q = q + b * sqb + (long long)head * D;
  const float* K = k + b * skb + (long long)head * D;
  const float* VT = vt + b * svb + (long long)head * D * ldvt;
  float* O = o + b * sob + (long long)head * D;

  // ---- Q fragments (B operand of S^T), split once, resident: channels 16 s + 8 hh + 0..7 of query qi ----
  u32x4 qh[NS], ql[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int ch = 16 * s + 8 * hh;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
    if (qi < nq && ch < D) {               // D % 8 == 0: the 8 channels are inside D together
      const float* src = Q + (long long)qi * ldq + ch;
      a = *reinterpret_cast<const float4*>(src);
      bb = *reinterpret_cast<const float4*>(src + 4);
    }
    uint32_t h0, h1, h2, h3, l0, l1, l2, l3;
    split2(a.x, a.y, h0, l0);
    split2(a.z, a.w, h1, l1);
    split2(bb.x, bb.y, h2, l2);
    split2(bb.z, bb.w, h3, l3);
    qh[s] = u32x4{h0, h1, h2, h3};
    ql[s] = u32x4{l0, l1, l2, l3};
  }

  f32x16 oacc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[cb][i] = 0.f;
  float m_run = -1e30f;                    // running maximum of this lane's query (log2 domain)
  float l_run = 0.f;                       // this lane's share (its 32 keys of every tile) of the running sum

  // causal: keys beyond the workgroup's last query are masked for every one of its queries
  const int nk_eff = causal ? min(nk, q0 + kBQ * kNW) : nk;
  const int ntiles = (nk_eff + kKT - 1) / kKT;
  for (int t = 0; t < ntiles; ++t) {
    const int key0 = t * kKT;
    __syncthreads();                       // every wave has finished reading the previous tile

    // ---- stage K: float4 chunk cc of key row kk -> 4 hi + 4 lo bf16; keys >= nk and channels >= D are zeros ----
#pragma unroll
    for (int it = 0; it < DP / 16; ++it) {
      const int ci = tid + 64 * kNW * it;
      const int kk = ci / KCH, cc = ci - kk * KCH;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (key0 + kk < nk && 4 * cc < D) v = *reinterpret_cast<const float4*>(K + (long long)(key0 + kk) * ldk + 4 * cc);
      uint32_t h0, h1, l0, l1;
      split2(v.x, v.y, h0, l0);
      split2(v.z, v.w, h1, l1);
      *reinterpret_cast<u32x2*>(ksm + kk * KP + 8 * cc) = u32x2{h0, h1};
      *reinterpret_cast<u32x2*>(ksm + K_PLANE + kk * KP + 8 * cc) = u32x2{l0, l1};
    }
    // ---- stage V^T: 4 consecutive keys of channel row ch; the 4-key groups of a 16-key step go to slots (0, 2, 1, 3): key
    //      8 a + 4 h + e -> slot 8 h + 4 a + e.  Keys >= nk are zeros (their weight is 0, and 0 x garbage must stay 0) ----
#pragma unroll
    for (int it = 0; it < NCB * 2; ++it) {
      const int ci = tid + 64 * kNW * it;
      const int ch = ci >> 4, kc = ci & 15;
      const int key = key0 + 4 * kc;
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      if (ch < D && key < nk) {
        const float* src = VT + (long long)ch * ldvt + key;
        if (key + 3 < nk) {
          const float4 v = *reinterpret_cast<const float4*>(src);
          x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (key + e < nk) x[e] = src[e];
        }
      }
      uint32_t h0, h1, l0, l1;
      split2(x[0], x[1], h0, l0);
      split2(x[2], x[3], h1, l1);
      const int slot = (kc & 12) | ((kc & 1) << 1) | ((kc >> 1) & 1);
      *reinterpret_cast<u32x2*>(vsm + ch * kVP + 8 * slot) = u32x2{h0, h1};
      *reinterpret_cast<u32x2*>(vsm + V_PLANE + ch * kVP + 8 * slot) = u32x2{l0, l1};
    }
    __syncthreads();

    if (causal && key0 > q0w + kBQ - 1) continue;    // wave-uniform: every key of the tile is masked for this wave's queries

    // ---- S^T = K Q^T: two 32-key blocks, one fp32 accumulator chain each over the channel steps ----
    f32x16 sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const unsigned char* src = ksm + (32 * kb + r) * KP + 32 * s + 16 * hh;
        const u32x4 kh = *reinterpret_cast<const u32x4*>(src);
        const u32x4 kl = *reinterpret_cast<const u32x4*>(src + K_PLANE);
        run3(kh, kl, qh[s], ql[s], sacc[kb]);
      }

    // ---- online softmax in fp32; register i of block kb is key key0 + 32 kb + 8 (i >> 2) + 4 hh + (i & 3) ----
    const bool tail = key0 + kKT > nk;                        // only the last tile holds keys >= nk
    const bool diag = causal && key0 + kKT - 1 > q0w;         // some key of the tile is beyond some query of the wave
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = key0 + 32 * kb + 8 * (i >> 2) + 4 * hh + (i & 3);
        float v = sacc[kb][i] * c;
        if ((tail && key >= nk) || (diag && key > qi)) v = -INFINITY;
        sacc[kb][i] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    if (__any(m_new > m_run)) {            // some query's maximum moved: rescale what was accumulated at the old one
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) oacc[cb] *= alpha;
    }
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(sacc[kb][i] - m_run);
        sacc[kb][i] = p;
        psum += p;
      }
    l_run += psum;

    // ---- O^T += V^T P^T: four 16-key steps, P split from its fp32 value ----
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int kb = s >> 1, i0 = 8 * (s & 1);
      uint32_t ph[4], pl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split2(sacc[kb][i0 + 2 * j], sacc[kb][i0 + 2 * j + 1], ph[j], pl[j]);
      const u32x4 pH = {ph[0], ph[1], ph[2], ph[3]}, pL = {pl[0], pl[1], pl[2], pl[3]};
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const unsigned char* src = vsm + (32 * cb + r) * kVP + 32 * s + 16 * hh;
        const u32x4 vh = *reinterpret_cast<const u32x4*>(src);
        const u32x4 vl = *reinterpret_cast<const u32x4*>(src + V_PLANE);
        run3(vh, vl, pH, pL, oacc[cb]);
      }
    }
  }

  // ---- divide by the row sum and store: lane holds O[query qi][32 cb + 8 g + 4 hh + 0..3] ----
  const float l = l_run + __shfl_xor(l_run, 32, 64);
  if (qi < nq) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = 32 * cb + 8 * g + 4 * hh;
        if (ch < D)
          *reinterpret_cast<float4*>(O + (long long)qi * ldo + ch) =
              make_float4(oacc[cb][4 * g] / l, oacc[cb][4 * g + 1] / l, oacc[cb][4 * g + 2] / l, oacc[cb][4 * g + 3] / l);
      }
  }
}

template <int DP>
int launch_x3(const SaspaAttnParams& p, hipStream_t s) {
  const long long nqb = (p.nq + kBQ * kNW - 1) / (kBQ * kNW);
  const long long blocks = nqb * p.heads * p.batch;
  if (blocks > 0x7fffffffLL) return SASPA_EINVAL;
  hipLaunchKernelGGL(attn_x3_kernel<DP>, dim3((unsigned)blocks), dim3(64 * kNW), 0, s, reinterpret_cast<const float*>(p.q),
                     reinterpret_cast<const float*>(p.k), reinterpret_cast<const float*>(p.vt), reinterpret_cast<float*>(p.o), p.heads,
                     p.D, p.nq, p.nk, p.ldq, p.ldk, p.ldvt, p.ldo, p.sqb, p.skb, p.svb, p.sob, p.scale * 1.4426950408889634f,
                     p.causal ? 1 : 0, (int)nqb);
  SASPA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int saspa_flash_attn_f32x3(const SaspaAttnParams* pp, void* stream) {
  if (!pp) return SASPA_EINVAL;
  const SaspaAttnParams& p = *pp;
  if (!p.q || !p.k || !p.vt || !p.o) return SASPA_EINVAL;
  if (p.batch < 1 || p.heads < 1 || p.nq < 1 || p.nk < 1) return SASPA_EINVAL;
  if (p.D < 8 || p.D > 160 || p.D % 8) return SASPA_EINVAL;
  const long long c = (long long)p.heads * p.D;
  if (p.ldq < c || p.ldk < c || p.ldo < c || p.ldvt < p.nk) return SASPA_EINVAL;
  if (p.flags) return SASPA_EINVAL;        // prescaled queries and row-major V belong to the 16-bit loops
  if (!aligned16(p.q) || !aligned16(p.k) || !aligned16(p.vt) || !aligned16(p.o)) return SASPA_EALIGN;
  if (p.ldq % 4 || p.ldk % 4 || p.ldvt % 4 || p.ldo % 4 || p.sqb % 4 || p.skb % 4 || p.svb % 4 || p.sob % 4) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch ((p.D + 15) / 16) {
    case 1: return launch_x3<16>(p, s);
    case 2: return launch_x3<32>(p, s);
    case 3: return launch_x3<48>(p, s);
    case 4: return launch_x3<64>(p, s);
    case 5: return launch_x3<80>(p, s);
    case 6: return launch_x3<96>(p, s);
    case 7: return launch_x3<112>(p, s);
    case 8: return launch_x3<128>(p, s);
    case 9: return launch_x3<144>(p, s);
    case 10: return launch_x3<160>(p, s);
    default: break;
  }
  return SASPA_EINVAL;
}
