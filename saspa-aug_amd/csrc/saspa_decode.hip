// Caption decoder kernels (include/saspa_hip.h, "caption decoder"): one-query attention against a key/value cache and one
// beam-search step's log-softmax + top-k.  Both are latency / bandwidth bound (a cross-attention launch reads 577 x 64 x 2 operands per
// (image, head) for three query rows): plain VALU dot products on 16-byte loads, no MFMA.  Both are deterministic: every sum has a
// fixed order, nothing is atomic, and a row's (an image's) result does not depend on what else is in the launch.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kDecThreads = 256;                    // 4 waves per (cache entry, head)
constexpr int kMaxD = SASPA_DECODE_MAX_D;
constexpr int kMaxNk = SASPA_DECODE_MAX_NK;
constexpr int kMaxG = SASPA_DECODE_MAX_GROUP;
constexpr int kPartFloats = kDecThreads * 8;        // P V partials of one row: (key slices) x d <= 256 / (d / EPC) * d <= 256 * 8

// grid (entries in use, heads).  Phase 1: a thread per key, the logits of the group's rows to LDS.  Phase 2: a wave per row, maximum,
// exp and sum.  Phase 3: thread (channel chunk, key slice) accumulates P V over its keys for every row, the slices are summed in order.
template <typename T>
__global__ __launch_bounds__(kDecThreads) void decode_attn_kernel(const T* __restrict__ q, const int ldq, const T* __restrict__ k,
                                                                  const int ldk, const long long ske, const T* __restrict__ v,
                                                                  const int ldv, const long long sve, const int* __restrict__ len,
                                                                  T* __restrict__ out, const int ldo, const int rows, const int d,
                                                                  const int nk, const int group, const float scale) {
  constexpr int EPC = Elem<T>::EPC;
  __shared__ __attribute__((aligned(16))) float sq[kMaxG * kMaxD];       // the group's queries, later its outputs
  __shared__ __attribute__((aligned(16))) float sp[kMaxG * kMaxNk];      // logits, then exp(logit - max)
  __shared__ __attribute__((aligned(16))) float part[kPartFloats];
  __shared__ float ssum[kMaxG];
  __shared__ int slen[kMaxG];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.x, h = blockIdx.y;
  const int r0 = e * group;
  const int ng = min(group, rows - r0);                                  // >= 1: the grid covers ceil(rows / group) entries
  const T* kb = k + e * ske + h * d;
  const T* vb = v + e * sve + h * d;

  if (tid < kMaxG) slen[tid] = tid < ng ? (len ? max(0, min(len[r0 + tid], nk)) : nk) : 0;
  for (int i = tid; i < ng * d; i += kDecThreads) {
    const int g = i / d, c = i - g * d;
    sq[g * kMaxD + c] = Elem<T>::load1(q + (long long)(r0 + g) * ldq + h * d + c);
  }
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int g = 0; g < kMaxG; ++g) maxlen = max(maxlen, slen[g]);

  // ---- 1. logits: key j of this thread against every row that still sees it ----
  for (int j = tid; j < maxlen; j += kDecThreads) {
    float acc[kMaxG];
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) acc[g] = 0.f;
    const T* kr = kb + (long long)j * ldk;
    for (int c = 0; c < d; c += EPC) {
      float f[EPC];
      Elem<T>::load_chunk(kr + c, f);
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) {
        if (g < ng) {
#pragma unroll
          for (int t = 0; t < EPC; ++t) acc[g] = fmaf(sq[g * kMaxD + c + t], f[t], acc[g]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < kMaxG; ++g)
      if (g < ng) sp[g * kMaxNk + j] = acc[g] * scale;
  }
  __syncthreads();

  // ---- 2. per row: maximum, p = exp(logit - max) (0 beyond the row's length), 1 / sum ----
  for (int g = wave; g < ng; g += kDecThreads / 64) {
    const int n = slen[g];
    float* row = sp + g * kMaxNk;
    float m = -INFINITY;
    for (int j = lane; j < n; j += 64) m = fmaxf(m, row[j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < maxlen; j += 64) {
      const float pj = j < n ? expf(row[j] - m) : 0.f;
      row[j] = pj;
      s += pj;
    }
    s = wave_sum(s);
    if (lane == 0) ssum[g] = s;
  }
  __syncthreads();

  // ---- 3. P V ----
  const int nch = d / EPC;                              // 16-byte channel chunks of a head: <= 32
  const int nsl = kDecThreads / nch;                    // key slices
  const int cc = tid % nch, ks = tid / nch;
  float acc[kMaxG][EPC];
#pragma unroll
  for (int g = 0; g < kMaxG; ++g)
#pragma unroll
    for (int t = 0; t < EPC; ++t) acc[g][t] = 0.f;
  if (ks < nsl) {
    for (int j = ks; j < maxlen; j += nsl) {
      float f[EPC];
      Elem<T>::load_chunk(vb + (long long)j * ldv + cc * EPC, f);
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) {
        if (g < ng && j < slen[g]) {                    // a key beyond a row's length may hold anything: never multiplied
          const float pj = sp[g * kMaxNk + j];
#pragma unroll
          for (int t = 0; t < EPC; ++t) acc[g][t] = fmaf(pj, f[t], acc[g][t]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kMaxG; ++g) {
    if (g < ng) {                                       // uniform over the workgroup
      if (ks < nsl) {
#pragma unroll
        for (int t = 0; t < EPC; ++t) part[ks * d + cc * EPC + t] = acc[g][t];
      }
      __syncthreads();
      if (tid < d) {
        float o = 0.f;
        for (int s = 0; s < nsl; ++s) o += part[s * d + tid];
        const float l = ssum[g];
        sq[g * kMaxD + tid] = l > 0.f ? o / l : 0.f;
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < ng * nch; i += kDecThreads) {
    const int g = i / nch, c = (i - g * nch) * EPC;
    Elem<T>::store_chunk(out + (long long)(r0 + g) * ldo + h * d + c, sq + g * kMaxD + c);
  }
}

// ---- log-softmax + beam top-k ----------------------------------------------------------------------------------------------------
constexpr int kTopThreads = 1024;
constexpr int kTopWaves = kTopThreads / 64;

// candidate order: higher score first, ties to the lower flat index; (-inf, INT_MAX) = none
__device__ __forceinline__ bool cand_before(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

__global__ __launch_bounds__(kTopThreads) void logprob_topk_kernel(const float* __restrict__ logits, const int ld, const int vocab,
                                                                   const int group, const float* __restrict__ scores,
                                                                   const int ban_token, const int ban_on,
                                                                   float* __restrict__ out_score, int* __restrict__ out_idx) {
  __shared__ float red[kTopWaves];
  __shared__ int redi[kTopWaves];
  __shared__ float smax[kMaxG], slse[kMaxG], sscore[kMaxG];
  __shared__ float bestv;
  __shared__ int besti;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x;
  const float* base = logits + (long long)img * group * ld;

  // ---- per row: maximum and log-sum-exp over the live columns (thread stride order, wave butterfly, waves ascending) ----
  for (int g = 0; g < group; ++g) {
    const float* row = base + (long long)g * ld;
    float m = -INFINITY;
    for (int c = tid * 4; c < vocab; c += kTopThreads * 4) {
      const float4 x = *reinterpret_cast<const float4*>(row + c);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (c + t < vocab) m = fmaxf(m, xs[t]);
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < kTopWaves; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    float s = 0.f;
    for (int c = tid * 4; c < vocab; c += kTopThreads * 4) {
      const float4 x = *reinterpret_cast<const float4*>(row + c);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (c + t < vocab) s += expf(xs[t] - m);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) {
      float a = 0.f;
      for (int w = 0; w < kTopWaves; ++w) a += red[w];
      smax[g] = m;
      slse[g] = logf(a);
      sscore[g] = scores[img * group + g];
    }
    __syncthreads();
  }

  // ---- k rounds: the best candidate that comes after the previous round's ----
  const int k = 2 * group;
  float pv = INFINITY;
  int pi = -1;
  for (int round = 0; round < k; ++round) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int g = 0; g < group; ++g) {
      const float* row = base + (long long)g * ld;
      const float m = smax[g], lse = slse[g], sc = sscore[g];
      for (int c = tid * 4; c < vocab; c += kTopThreads * 4) {
        const float4 x = *reinterpret_cast<const float4*>(row + c);
        const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int col = c + t;
          if (col < vocab) {
            const float lp = (ban_on && col == ban_token) ? -INFINITY : (xs[t] - m) - lse;
            const float val = lp + sc;
            const int idx = g * vocab + col;
            if (cand_before(pv, pi, val, idx) && cand_before(val, idx, bv, bi)) {
              bv = val;
              bi = idx;
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (cand_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      red[wave] = bv;
      redi[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      float v0 = red[0];
      int i0 = redi[0];
      for (int w = 1; w < kTopWaves; ++w)
        if (cand_before(red[w], redi[w], v0, i0)) {
          v0 = red[w];
          i0 = redi[w];
        }
      bestv = v0;
      besti = i0;
      const bool none = i0 == INT_MAX;
      out_score[img * k + round] = none ? -INFINITY : v0;
      out_idx[(img * k + round) * 2] = none ? -1 : i0 / vocab;
      out_idx[(img * k + round) * 2 + 1] = none ? -1 : i0 % vocab;
    }
    __syncthreads();
    pv = bestv;
    pi = besti;
    __syncthreads();
  }
}

}  // namespace

extern "C" int saspa_decode_attn(const SaspaDecodeAttnParams* p, void* stream) {
  if (!p || !p->q || !p->k || !p->v || !p->out) return SASPA_EINVAL;
  if (p->dtype != SASPA_BF16 && p->dtype != SASPA_F32) return SASPA_EINVAL;
  if (p->rows < 1 || p->heads < 1 || p->d < 1 || p->nk < 1 || p->entries < 1 || p->group < 1) return SASPA_EINVAL;
  if (p->d % 8 || p->d > kMaxD || p->nk > kMaxNk || p->group > kMaxG) return SASPA_ERANGE;
  if ((long long)p->entries * p->group < p->rows) return SASPA_EINVAL;
  const long long c = (long long)p->heads * p->d;
  if (p->ldq < c || p->ldk < c || p->ldv < c || p->ldo < c || p->heads > 65535) return SASPA_EINVAL;
  const int ea = p->dtype == SASPA_F32 ? 4 : 8;           // elements per 16 bytes
  if (p->ldq % ea || p->ldk % ea || p->ldv % ea || p->ldo % ea || p->ske % ea || p->sve % ea) return SASPA_EALIGN;
  if (!aligned16(p->q) || !aligned16(p->k) || !aligned16(p->v) || !aligned16(p->out)) return SASPA_EALIGN;
  if (p->len && (reinterpret_cast<uintptr_t>(p->len) & 3u)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p->rows + p->group - 1) / p->group), (unsigned)p->heads);
  if (p->dtype == SASPA_F32)
    hipLaunchKernelGGL(decode_attn_kernel<float>, grid, dim3(kDecThreads), 0, s, reinterpret_cast<const float*>(p->q), p->ldq,
                       reinterpret_cast<const float*>(p->k), p->ldk, p->ske, reinterpret_cast<const float*>(p->v), p->ldv, p->sve,
                       p->len, reinterpret_cast<float*>(p->out), p->ldo, p->rows, p->d, p->nk, p->group, p->scale);
  else
    hipLaunchKernelGGL(decode_attn_kernel<h16_t>, grid, dim3(kDecThreads), 0, s, reinterpret_cast<const h16_t*>(p->q), p->ldq,
                       reinterpret_cast<const h16_t*>(p->k), p->ldk, p->ske, reinterpret_cast<const h16_t*>(p->v), p->ldv, p->sve,
                       p->len, reinterpret_cast<h16_t*>(p->out), p->ldo, p->rows, p->d, p->nk, p->group, p->scale);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_logprob_topk(const float* logits, int ld, int vocab, int images, int group, const float* scores, int ban_token,
                                  int ban_on, float* out_score, int* out_idx, void* stream) {
  if (!logits || !scores || !out_score || !out_idx) return SASPA_EINVAL;
  if (images < 1 || vocab < 1 || ld < vocab || group < 1) return SASPA_EINVAL;
  if (group > kMaxG || (long long)group * vocab > INT_MAX) return SASPA_ERANGE;
  if (!aligned16(logits) || ld % 4) return SASPA_EALIGN;
  if ((reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(out_score) | reinterpret_cast<uintptr_t>(out_idx)) & 3u)
    return SASPA_EALIGN;
  hipLaunchKernelGGL(logprob_topk_kernel, dim3((unsigned)images), dim3(kTopThreads), 0, reinterpret_cast<hipStream_t>(stream), logits,
                     ld, vocab, group, scores, ban_token, ban_on, out_score, out_idx);
  SASPA_CHECK_LAUNCH();
  return 0;
}
