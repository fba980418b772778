// T5 kernels (include/saspa_hip.h, "T5 key-to-text"): an RMS norm, attention against a key/value cache with an additive
// relative-position bias, and one sampling step (temperature -> top-k -> top-p -> inverse-CDF draw).  All three are latency bound (a
// decoder step of T5-base works on rows x 768 values): plain VALU work on 16-byte loads, wave butterflies and LDS, no MFMA.  All three
// are deterministic: every sum has a fixed order, nothing is atomic, and a row's result does not depend on what else is in the launch.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

// ---- RMS norm: a wave per row ---------------------------------------------------------------------------------------------------
constexpr int kRmsThreads = 256;
constexpr int kRmsRows = kRmsThreads / 64;

// Lane l owns the 16-byte chunks l, l + 64, ... of its row: squares added chunk by chunk, element by element (one fma chain per lane),
// then the 64-lane butterfly.  The second pass reads the row again (it is in L1 / L2) and rounds once.
template <typename T>
__global__ __launch_bounds__(kRmsThreads) void rmsnorm_kernel(const T* __restrict__ x, const int ldx, T* __restrict__ out, const int ldo,
                                                              const int rows, const int c, const float* __restrict__ gamma,
                                                              const float eps) {
  constexpr int EPC = Elem<T>::EPC;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kRmsRows + (threadIdx.x >> 6);
  if (r >= rows) return;                                  // whole waves leave; there is no barrier below
  const T* xr = x + (long long)r * ldx;
  T* orow = out + (long long)r * ldo;
  float ss = 0.f;
  for (int i = lane * EPC; i < c; i += 64 * EPC) {
    float f[EPC];
    Elem<T>::load_chunk(xr + i, f);
#pragma unroll
    for (int t = 0; t < EPC; ++t) ss = fmaf(f[t], f[t], ss);
  }
  ss = wave_sum(ss);
  const float rs = 1.0f / sqrtf(ss / (float)c + eps);
  for (int i = lane * EPC; i < c; i += 64 * EPC) {
    float f[EPC];
    Elem<T>::load_chunk(xr + i, f);
#pragma unroll
    for (int t = 0; t < EPC; ++t) f[t] = (f[t] * rs) * gamma[i + t];
    Elem<T>::store_chunk(orow + i, f);
  }
}

// ---- attention with a relative-position bias -------------------------------------------------------------------------------------
constexpr int kAttThreads = 256;                    // 4 waves per (entry, head, block of kRowBlock rows)
constexpr int kMaxD = SASPA_RELBIAS_MAX_D;
constexpr int kMaxNk = SASPA_RELBIAS_MAX_NK;
constexpr int kRowBlock = 8;                        // rows of one entry that share a workgroup (and its K / V loads)
constexpr int kPartFloats = kAttThreads * 8;        // P V partials of one row: (key slices) x d <= 256 / (d / EPC) * d <= 256 * 8

// grid (entries in use, heads, ceil(rows_per_entry / kRowBlock)).  The phases of saspa_decode.hip's decode_attn_kernel: 1. a thread per
// key, the logits of the block's rows to LDS (scale, then the bias column of (row position, key)); 2. a wave per row, maximum, exp and
// sum; 3. thread (channel chunk, key slice) accumulates P V over its keys for every row, the slices are summed in order.  Every row's
// order of operations depends on its own length only, not on its block mates'.
template <typename T>
__global__ __launch_bounds__(kAttThreads) void attn_relbias_kernel(const T* __restrict__ q, const int ldq, const T* __restrict__ k,
                                                                   const int ldk, const long long ske, const T* __restrict__ v,
                                                                   const int ldv, const long long sve, const int* __restrict__ len,
                                                                   const int* __restrict__ pos, const float* __restrict__ bias,
                                                                   const int ldb, const int ncol, const int center,
                                                                   T* __restrict__ out, const int ldo, const int rows, const int d,
                                                                   const int nk, const int rpe, const float scale) {
  constexpr int EPC = Elem<T>::EPC;
  __shared__ __attribute__((aligned(16))) float sq[kRowBlock * kMaxD];       // the block's queries, later its outputs
  __shared__ __attribute__((aligned(16))) float sp[kRowBlock * kMaxNk];      // logits, then exp(logit - max)
  __shared__ __attribute__((aligned(16))) float part[kPartFloats];
  __shared__ float ssum[kRowBlock];
  __shared__ int slen[kRowBlock];
  __shared__ int spos[kRowBlock];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.x, h = blockIdx.y;
  const int r0 = e * rpe + blockIdx.z * kRowBlock;
  const int rend = min(rows, (e + 1) * rpe);
  const int ng = min(kRowBlock, rend - r0);
  if (ng <= 0) return;                                                       // uniform: the last entry may hold fewer blocks
  const T* kb = k + e * ske + h * d;
  const T* vb = v + e * sve + h * d;
  const float* bh = bias + (long long)h * ldb;

  if (tid < kRowBlock) {
    slen[tid] = tid < ng ? (len ? max(0, min(len[r0 + tid], nk)) : nk) : 0;
    spos[tid] = tid < ng ? pos[r0 + tid] : 0;
  }
  for (int i = tid; i < ng * d; i += kAttThreads) {
    const int g = i / d, c = i - g * d;
    sq[g * kMaxD + c] = Elem<T>::load1(q + (long long)(r0 + g) * ldq + h * d + c);
  }
  __syncthreads();
  int maxlen = 0;
#pragma unroll
  for (int g = 0; g < kRowBlock; ++g) maxlen = max(maxlen, slen[g]);

  // ---- 1. logits: key j of this thread against every row that still sees it ----
  for (int j = tid; j < maxlen; j += kAttThreads) {
    float acc[kRowBlock];
#pragma unroll
    for (int g = 0; g < kRowBlock; ++g) acc[g] = 0.f;
    const T* kr = kb + (long long)j * ldk;
    for (int c = 0; c < d; c += EPC) {
      float f[EPC];
      Elem<T>::load_chunk(kr + c, f);
#pragma unroll
      for (int g = 0; g < kRowBlock; ++g) {
        if (g < ng) {
#pragma unroll
          for (int t = 0; t < EPC; ++t) acc[g] = fmaf(sq[g * kMaxD + c + t], f[t], acc[g]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < kRowBlock; ++g) {
      if (g < ng && j < slen[g]) {
        // the column saturates at both ends of the table: 64-bit, so that no position can wrap
        const long long col = (long long)spos[g] - j + center;
        const int cc = (int)max(0LL, min(col, (long long)ncol - 1));
        sp[g * kMaxNk + j] = acc[g] * scale + bh[cc];
      }
    }
  }
  __syncthreads();

  // ---- 2. per row: maximum, p = exp(logit - max) (0 beyond the row's length), sum ----
  for (int g = wave; g < ng; g += kAttThreads / 64) {
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
  const int nsl = kAttThreads / nch;                    // key slices
  const int cc = tid % nch, ks = tid / nch;
  float acc[kRowBlock][EPC];
#pragma unroll
  for (int g = 0; g < kRowBlock; ++g)
#pragma unroll
    for (int t = 0; t < EPC; ++t) acc[g][t] = 0.f;
  if (ks < nsl) {
    for (int j = ks; j < maxlen; j += nsl) {
      float f[EPC];
      Elem<T>::load_chunk(vb + (long long)j * ldv + cc * EPC, f);
#pragma unroll
      for (int g = 0; g < kRowBlock; ++g) {
        if (g < ng && j < slen[g]) {                    // a key beyond a row's length may hold anything: never multiplied
          const float pj = sp[g * kMaxNk + j];
#pragma unroll
          for (int t = 0; t < EPC; ++t) acc[g][t] = fmaf(pj, f[t], acc[g][t]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kRowBlock; ++g) {
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
  for (int i = tid; i < ng * nch; i += kAttThreads) {
    const int g = i / nch, c = (i - g * nch) * EPC;
    Elem<T>::store_chunk(out + (long long)(r0 + g) * ldo + h * d + c, sq + g * kMaxD + c);
  }
}

// ---- one sampling step -----------------------------------------------------------------------------------------------------------
constexpr int kSmpThreads = 1024;
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kMaxTopK = SASPA_SAMPLE_MAX_TOPK;

// candidate order: higher value first, ties to the lower index; (-inf, INT_MAX) = none
__device__ __forceinline__ bool cand_before(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

// One workgroup per row.  k rounds of "the best candidate after the previous round's" over y = x / temperature (thread scan, wave
// butterfly, 16 values in LDS) leave the kept tokens in their final order; thread 0 then walks the <= 64 of them in that order:
// exp(y - y0), the top-p prefix, the kept sum, the inverse-CDF draw.
__global__ __launch_bounds__(kSmpThreads) void sample_topk_kernel(const float* __restrict__ logits, const int ld, const int vocab,
                                                                  const float temperature, const int k, const float top_p,
                                                                  const float* __restrict__ u, int* __restrict__ out_tok,
                                                                  float* __restrict__ out_logp) {
  __shared__ float red[kSmpWaves];
  __shared__ int redi[kSmpWaves];
  __shared__ float topv[kMaxTopK];
  __shared__ int topi[kMaxTopK];
  __shared__ float bestv;
  __shared__ int besti;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  const float* row = logits + (long long)r * ld;

  float pv = INFINITY;
  int pi = -1;
  for (int round = 0; round < k; ++round) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int c = tid * 4; c < vocab; c += kSmpThreads * 4) {
      const float4 x = *reinterpret_cast<const float4*>(row + c);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int col = c + t;
        if (col < vocab) {
          const float val = xs[t] / temperature;
          if (cand_before(pv, pi, val, col) && cand_before(val, col, bv, bi)) {
            bv = val;
            bi = col;
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
      for (int w = 1; w < kSmpWaves; ++w)
        if (cand_before(red[w], redi[w], v0, i0)) {
          v0 = red[w];
          i0 = redi[w];
        }
      bestv = v0;
      besti = i0;
      topv[round] = v0;
      topi[round] = i0;
    }
    __syncthreads();
    pv = bestv;
    pi = besti;
    __syncthreads();
  }

  if (tid == 0) {
    // a row of NaN or -inf has fewer than k candidates: keep what there is (at least token 0, so that the id is always in range)
    int n = 0;
    while (n < k && topi[n] != INT_MAX) ++n;
    if (n == 0) {
      out_tok[r] = 0;
      out_logp[r] = -INFINITY;
      return;
    }
    const float m = topv[0];
    float z = 0.f;
    for (int i = 0; i < n; ++i) {
      topv[i] = expf(topv[i] - m);
      z += topv[i];
    }
    int keep = n;
    if (top_p < 1.0f) {
      float cum = 0.f;
      for (int i = 0; i < n; ++i) {
        cum += topv[i] / z;
        if (cum >= top_p) {
          keep = i + 1;
          break;
        }
      }
    }
    float s = 0.f;
    for (int i = 0; i < keep; ++i) s += topv[i];
    const float ur = u[r];
    int pick = keep - 1;
    float cum = 0.f;
    for (int i = 0; i < keep; ++i) {
      cum += topv[i] / s;
      if (cum > ur) {
        pick = i;
        break;
      }
    }
    out_tok[r] = topi[pick];
    out_logp[r] = logf(topv[pick] / s);
  }
}

}  // namespace

extern "C" int saspa_rmsnorm(int dtype, const void* x, int ldx, void* out, int ldo, int rows, int c, const float* gamma, float eps,
                             void* stream) {
  if (!x || !out || !gamma) return SASPA_EINVAL;
  if (dtype != SASPA_BF16 && dtype != SASPA_F32) return SASPA_EINVAL;
  if (rows < 1 || c < 1 || ldx < c || ldo < c || !(eps >= 0.f)) return SASPA_EINVAL;
  if (c > SASPA_RMSNORM_MAX_C) return SASPA_ERANGE;
  const int ea = dtype == SASPA_F32 ? 4 : 8;
  if (c % 8 || ldx % ea || ldo % ea || !aligned16(x) || !aligned16(out)) return SASPA_EALIGN;
  if (reinterpret_cast<uintptr_t>(gamma) & 3u) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((rows + kRmsRows - 1) / kRmsRows));
  if (dtype == SASPA_F32)
    hipLaunchKernelGGL(rmsnorm_kernel<float>, grid, dim3(kRmsThreads), 0, s, reinterpret_cast<const float*>(x), ldx,
                       reinterpret_cast<float*>(out), ldo, rows, c, gamma, eps);
  else
    hipLaunchKernelGGL(rmsnorm_kernel<h16_t>, grid, dim3(kRmsThreads), 0, s, reinterpret_cast<const h16_t*>(x), ldx,
                       reinterpret_cast<h16_t*>(out), ldo, rows, c, gamma, eps);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_attn_relbias(const SaspaAttnRelbiasParams* p, void* stream) {
  if (!p || !p->q || !p->k || !p->v || !p->out || !p->pos || !p->bias) return SASPA_EINVAL;
  if (p->dtype != SASPA_BF16 && p->dtype != SASPA_F32) return SASPA_EINVAL;
  if (p->rows < 1 || p->heads < 1 || p->d < 1 || p->nk < 1 || p->entries < 1 || p->rows_per_entry < 1 || p->ncol < 1) return SASPA_EINVAL;
  if (p->d % 8 || p->d > kMaxD || p->nk > kMaxNk || p->rows_per_entry > SASPA_RELBIAS_MAX_ROWS) return SASPA_ERANGE;
  if ((long long)p->entries * p->rows_per_entry < p->rows) return SASPA_EINVAL;
  const long long c = (long long)p->heads * p->d;
  if (p->ldq < c || p->ldk < c || p->ldv < c || p->ldo < c || p->ldb < p->ncol || p->heads > 65535) return SASPA_EINVAL;
  const int ea = p->dtype == SASPA_F32 ? 4 : 8;           // elements per 16 bytes
  if (p->ldq % ea || p->ldk % ea || p->ldv % ea || p->ldo % ea || p->ske % ea || p->sve % ea) return SASPA_EALIGN;
  if (!aligned16(p->q) || !aligned16(p->k) || !aligned16(p->v) || !aligned16(p->out)) return SASPA_EALIGN;
  if ((reinterpret_cast<uintptr_t>(p->pos) | reinterpret_cast<uintptr_t>(p->bias) | reinterpret_cast<uintptr_t>(p->len)) & 3u)
    return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p->rows + p->rows_per_entry - 1) / p->rows_per_entry), (unsigned)p->heads,
                  (unsigned)((p->rows_per_entry + kRowBlock - 1) / kRowBlock));
  if (p->dtype == SASPA_F32)
    hipLaunchKernelGGL(attn_relbias_kernel<float>, grid, dim3(kAttThreads), 0, s, reinterpret_cast<const float*>(p->q), p->ldq,
                       reinterpret_cast<const float*>(p->k), p->ldk, p->ske, reinterpret_cast<const float*>(p->v), p->ldv, p->sve,
                       p->len, p->pos, p->bias, p->ldb, p->ncol, p->center, reinterpret_cast<float*>(p->out), p->ldo, p->rows, p->d,
                       p->nk, p->rows_per_entry, p->scale);
  else
    hipLaunchKernelGGL(attn_relbias_kernel<h16_t>, grid, dim3(kAttThreads), 0, s, reinterpret_cast<const h16_t*>(p->q), p->ldq,
                       reinterpret_cast<const h16_t*>(p->k), p->ldk, p->ske, reinterpret_cast<const h16_t*>(p->v), p->ldv, p->sve,
                       p->len, p->pos, p->bias, p->ldb, p->ncol, p->center, reinterpret_cast<h16_t*>(p->out), p->ldo, p->rows, p->d,
                       p->nk, p->rows_per_entry, p->scale);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_sample_topk(const float* logits, int ld, int vocab, int rows, float temperature, int top_k, float top_p,
                                 const float* u, int* out_tok, float* out_logp, void* stream) {
  if (!logits || !u || !out_tok || !out_logp) return SASPA_EINVAL;
  if (rows < 1 || vocab < 1 || ld < vocab) return SASPA_EINVAL;
  if (!(temperature > 0.f) || isinf(temperature) || !(top_p > 0.f) || !(top_p <= 1.f)) return SASPA_EINVAL;
  if (top_k < 1 || top_k > kMaxTopK) return SASPA_ERANGE;
  if (!aligned16(logits) || ld % 4) return SASPA_EALIGN;
  if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(out_tok) | reinterpret_cast<uintptr_t>(out_logp)) & 3u)
    return SASPA_EALIGN;
  hipLaunchKernelGGL(sample_topk_kernel, dim3((unsigned)rows), dim3(kSmpThreads), 0, reinterpret_cast<hipStream_t>(stream), logits, ld,
                     vocab, temperature, top_k < vocab ? top_k : vocab, top_p, u, out_tok, out_logp);
  SASPA_CHECK_LAUNCH();
  return 0;
}
