// Kernels of the filter stage that follows generation (all_utils/utils.py:306-323, :357-375): pooling of the
// CLIP-RN50 / ResNet feature extractors and the sign-sqrt + L2-normalise tail of WSDAN_CAL's bilinear attention pooling.
// saspa_lpips_layer is one feature level of the LPIPS distance (lpips_min / lpips_max filter, all_utils/utils.py:377-381).
// All are HBM-bound streaming kernels (16-byte vectors of 8 channels per lane); the convolutions and linears of the two
// models are saspa_gemm launches (BatchNorm folded into weights + bias, ReLU in the epilogue).
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ void ld8(const T* p, float* v) {
  if constexpr (sizeof(T) == 2) {
    Elem<T>::load_chunk(p, v);
  } else {
    Elem<T>::load_chunk(p, v);
    Elem<T>::load_chunk(p + 4, v + 4);
  }
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const float* v) {
  if constexpr (sizeof(T) == 2) {
    Elem<T>::store_chunk(p, v);
  } else {
    Elem<T>::store_chunk(p, v);
    Elem<T>::store_chunk(p + 4, v + 4);
  }
}

// one lane = 8 channels of one output pixel; window taps outside the image are skipped (max) -- the average form has pad 0
template <typename T, int MODE>
__global__ __launch_bounds__(256) void pool2d_kernel(const T* x, int ldx, T* y, int ldy, int batch, int hin, int win, int C, int k,
                                                     int stride, int pad, int hout, int wout) {
  const int C8 = C >> 3;
  const long long total = (long long)batch * hout * wout * C8;
  const float inv = 1.0f / (float)(k * k);
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const int c = (int)(it % C8) * 8;
    long long pix = it / C8;
    const int ox = (int)(pix % wout);
    pix /= wout;
    const int oy = (int)(pix % hout);
    const int b = (int)(pix / hout);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = MODE == 0 ? -3.0e38f : 0.0f;
    for (int ty = 0; ty < k; ++ty) {
      const int iy = oy * stride - pad + ty;
      if ((unsigned)iy >= (unsigned)hin) continue;
      for (int tx = 0; tx < k; ++tx) {
        const int ix = ox * stride - pad + tx;
        if ((unsigned)ix >= (unsigned)win) continue;
        float v[8];
        ld8(x + ((long long)(b * hin + iy) * win + ix) * ldx + c, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = MODE == 0 ? fmaxf(acc[j], v[j]) : acc[j] + v[j];
      }
    }
    if (MODE == 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= inv;
    }
    st8(y + ((long long)(b * hout + oy) * wout + ox) * ldy + c, acc);
  }
}

// one workgroup per row: y = sign(x) sqrt(|x| + eps) kept in registers / re-derived, sum of squares in fp32 per lane then
// fp64 across the workgroup (65 536 elements per row for ResNet-101 x 32 attention maps), out = scale * y / max(|y|, 1e-12).
// sign(0) = 0: an exact zero (ordinary under ReLU features and ReLU attention maps) has y = 0 and adds NOTHING to the norm -- not
// its eps (with 60 % zeros, eps per zero scaled a row by 2.2e-5, 370 units of 2^-24)
__global__ __launch_bounds__(256) void signsqrt_l2norm_kernel(const float* x, long long ldx, float* y, long long ldy, long long C,
                                                              float eps, float scale) {
  __shared__ double part[4];
  const float* xr = x + (long long)blockIdx.x * ldx;
  float* yr = y + (long long)blockIdx.x * ldy;
  float ss = 0.0f;
  for (long long i = threadIdx.x; i < C; i += 256) {
    const float v = xr[i];
    if (v != 0.0f) ss += fabsf(v) + eps;                  // y^2 = |x| + eps exactly (before rounding of the sqrt)
  }
  double d = (double)wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = d;
  __syncthreads();
  const double tot = part[0] + part[1] + part[2] + part[3];
  const float inv = scale / fmaxf((float)sqrt(tot), 1e-12f);
  for (long long i = threadIdx.x; i < C; i += 256) {
    const float v = xr[i];
    const float r = sqrtf(fabsf(v) + eps);
    yr[i] = (v > 0.0f ? r : (v < 0.0f ? -r : 0.0f)) * inv;
  }
}

// ---- LPIPS level -----------------------------------------------------------------------------------------------------------
// A pixel's channel vector lives in the registers of LPP lanes (LPP = the power of two >= C / 8, at most 64: one wave), 8 channels per
// lane, from the 16-byte loads until the weighted squared difference is summed: each feature row is read once.  256 / LPP pixel slots
// per workgroup; workgroup b of pair j owns the pixels [b * ppb, (b + 1) * ppb), slot s the pixels s, s + slots, ... of that range.
// Every sum has a fixed shape: 8 values per lane as a tree, xor-butterflies inside the slot / wave, the four waves in order through
// LDS, the workgroups of a pair by one wave of the finishing launch.  nblk and ppb are functions of (hw, C) alone.
// (no FMA contraction anywhere in this kernel: both operands of a pair must see the very same operation sequence)
__device__ __forceinline__ float tree8(const float* t) {
#pragma clang fp contract(off)
  return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

// x / (|x|_2 + 1e-10) over the slot's lanes (lpips.normalize_tensor: the eps sits outside the root); a zero vector stays zero
__device__ __forceinline__ void lpips_unit(float* v, int lpp) {
#pragma clang fp contract(off)
  float sq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) sq[i] = v[i] * v[i];
  float s = tree8(sq);
  for (int o = lpp >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float d = sqrtf(s) + 1e-10f;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = v[i] / d;
}

template <typename T>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const T* __restrict__ a, int lda, const T* __restrict__ r, int ldr,
                                                          const int* __restrict__ ref_index, const float* __restrict__ w,
                                                          float* __restrict__ partial, int hw, int C, int lpp, int ppb) {
#pragma clang fp contract(off)
  __shared__ float part[4];
  const int j = blockIdx.y, tid = threadIdx.x;
  const int slots = 256 / lpp, slot = tid / lpp, q = tid % lpp;
  const bool live = q * 8 < C;                              // lanes beyond C / 8 of a slot carry zeros through the butterflies
  const T* ap = a + (long long)j * hw * lda + q * 8;
  const T* rp = r + (long long)ref_index[j] * hw * ldr + q * 8;
  float wt[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wt[i] = live ? w[q * 8 + i] : 0.0f;
  const int p0 = blockIdx.x * ppb, p1 = min(hw, p0 + ppb);
  float acc = 0.0f;
  // the trip count is uniform over the wave (the shuffles need every lane); a slot past the range works on zeros
  for (int pb = p0; pb < p1; pb += slots) {
    const int p = pb + slot;
    float va[8], vr[8];
    if (live && p < p1) {
      ld8(ap + (long long)p * lda, va);
      ld8(rp + (long long)p * ldr, vr);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) va[i] = vr[i] = 0.0f;
    }
    lpips_unit(va, lpp);
    lpips_unit(vr, lpp);
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = va[i] - vr[i];
      t[i] = wt[i] * (d * d);
    }
    acc += tree8(t);
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[(long long)j * SASPA_LPIPS_MAX_BLOCKS + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(64) void lpips_finish_kernel(const float* __restrict__ partial, float* __restrict__ dist, int nblk, int hw,
                                                          int accumulate) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const float s = wave_sum(lane < nblk ? partial[(long long)j * SASPA_LPIPS_MAX_BLOCKS + lane] : 0.0f);
  if (lane == 0) {
    const float d = s / (float)hw;
    dist[j] = accumulate ? dist[j] + d : d;
  }
}

// ---- class head ------------------------------------------------------------------------------------------------------------
// One workgroup (4 waves) per row.  Embedding mode: the row's embedding is staged once in LDS (and scaled to unit length there), then
// wave w takes the classes w, w + 4, ...: 64 lanes x 16 bytes of the class row per load, an xor-butterfly, lane 0 writes z_c to LDS.
// The row statistics read z from LDS only.  Every reduction: lanes stride the row, butterfly inside the wave, the four waves in
// order through LDS -- the same shape for every row whatever else is in the launch.
struct MaxIdx {
  float m;
  int i;
};
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) {          // the larger value; of equal values the lower index
  return (b.m > a.m || (b.m == a.m && b.i < a.i)) ? b : a;
}

template <bool EMB>
__global__ __launch_bounds__(256) void class_head_kernel(const float* __restrict__ feat, int ldf, const float* __restrict__ cls, int ldc,
                                                         const int* __restrict__ labels, float scale, int normalize,
                                                         float* __restrict__ stats, int* __restrict__ idx, float* __restrict__ logits,
                                                         int ldl, int D, int C) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float redf[4];
  __shared__ int redi[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* fr = feat + (long long)row * ldf;
  float* z = smem;
  if constexpr (EMB) {
    float* u = smem;
    z = smem + ((D + 3) & ~3);
    float ss = 0.0f;
    for (int i = tid; i < D; i += 256) {
      const float v = fr[i];
      u[i] = v;
      ss += v * v;
    }
    ss = wave_sum(ss);
    if (lane == 0) redf[wave] = ss;
    __syncthreads();
    const float inv = normalize ? 1.0f / sqrtf((redf[0] + redf[1]) + (redf[2] + redf[3])) : 1.0f;
    for (int i = tid; i < D; i += 256) u[i] *= inv;       // a thread rescales the elements it staged itself
    __syncthreads();
    const int D4 = D >> 2;
    const float4* u4 = reinterpret_cast<const float4*>(u);
    for (int c = wave; c < C; c += 4) {
      const float* cr = cls + (long long)c * ldc;
      const float4* c4 = reinterpret_cast<const float4*>(cr);
      float acc = 0.0f;
      for (int j = lane; j < D4; j += 64) {
        const float4 t = c4[j], v = u4[j];
        acc += (t.x * v.x + t.y * v.y) + (t.z * v.z + t.w * v.w);
      }
      for (int i = (D4 << 2) + lane; i < D; i += 64) acc += cr[i] * u[i];
      acc = wave_sum(acc);
      if (lane == 0) z[c] = scale * acc;
    }
  } else {
    for (int c = tid; c < C; c += 256) z[c] = scale * fr[c];
  }
  __syncthreads();
  if (logits) {
    float* lr = logits + (long long)row * ldl;
    for (int c = tid; c < C; c += 256) lr[c] = z[c];
  }
  // m = max_c z_c and the lowest c that reaches it
  MaxIdx best{-INFINITY, 0x7fffffff};
  for (int c = tid; c < C; c += 256) best = better(best, MaxIdx{z[c], c});
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = better(best, MaxIdx{__shfl_xor(best.m, o, 64), __shfl_xor(best.i, o, 64)});
  if (lane == 0) {
    redf[wave] = best.m;
    redi[wave] = best.i;
  }
  __syncthreads();
  best = better(better(MaxIdx{redf[0], redi[0]}, MaxIdx{redf[1], redi[1]}), better(MaxIdx{redf[2], redi[2]}, MaxIdx{redf[3], redi[3]}));
  __syncthreads();
  const int label = labels[row];
  const bool valid = (unsigned)label < (unsigned)C;
  const float zl = valid ? z[label] : 0.0f;
  float s = 0.0f;
  int ng = 0;
  for (int c = tid; c < C; c += 256) {
    const float v = z[c];
    s += expf(v - best.m);
    ng += v > zl ? 1 : 0;
  }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ng += __shfl_xor(ng, o, 64);
  if (lane == 0) {
    redf[wave] = s;
    redi[wave] = ng;
  }
  __syncthreads();
  if (tid == 0) {
    const float tot = (redf[0] + redf[1]) + (redf[2] + redf[3]);
    float* st = stats + 4ll * row;
    int* ix = idx + 2ll * row;
    if (valid) {
      st[0] = zl;
      st[1] = expf(zl - best.m) / tot;
      st[2] = best.m;
      st[3] = best.m + logf(tot);
      ix[0] = best.i;
      ix[1] = (redi[0] + redi[1]) + (redi[2] + redi[3]);
    } else {
      const float nan = __builtin_nanf("");
      st[0] = st[1] = st[2] = st[3] = nan;
      ix[0] = ix[1] = -1;
    }
  }
}

}  // namespace

extern "C" int saspa_class_head(const float* feat, int ldf, const float* cls, int ldc, const int* labels, float scale, int normalize,
                                float* stats, int* idx, float* logits, int ldl, int rows, int D, int C, void* stream) {
  if (!feat || !labels || !stats || !idx || rows <= 0) return SASPA_EINVAL;
  if (C < 1 || D < 1 || D > SASPA_CLASS_HEAD_MAX_D || C > SASPA_CLASS_HEAD_MAX_C || (!cls && D != C)) return SASPA_ERANGE;
  if (!aligned16(feat) || ldf % 4 || ldf < D) return SASPA_EALIGN;
  if (cls && (!aligned16(cls) || ldc % 4 || ldc < D)) return SASPA_EALIGN;
  if (logits && (!aligned16(logits) || ldl % 4 || ldl < C)) return SASPA_EALIGN;
  if ((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(labels)) & 3u) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 g((unsigned)rows), t(256);
  if (cls) {
    const size_t lds = sizeof(float) * (size_t)(((D + 3) & ~3) + C);
    hipLaunchKernelGGL(class_head_kernel<true>, g, t, lds, s, feat, ldf, cls, ldc, labels, scale, normalize, stats, idx, logits, ldl, D, C);
  } else {
    hipLaunchKernelGGL(class_head_kernel<false>, g, t, sizeof(float) * (size_t)C, s, feat, ldf, cls, ldc, labels, scale, normalize, stats,
                       idx, logits, ldl, D, C);
  }
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_pool2d(int dtype, int mode, const void* x, int ldx, void* y, int ldy, int batch, int hin, int win, int C, int k,
                            int stride, int pad, void* stream) {
  if (!x || !y || batch <= 0 || hin <= 0 || win <= 0 || C <= 0 || k <= 0 || stride <= 0 || pad < 0) return SASPA_EINVAL;
  if (mode != 0 && mode != 1) return SASPA_EINVAL;
  if (C % 8 || ldx % 8 || ldy % 8 || ldx < C || ldy < C || !aligned16(x) || !aligned16(y)) return SASPA_EALIGN;
  if (mode == 1 && pad != 0) return SASPA_ERANGE;         // AvgPool2d(k) only: every window lies inside the image
  const int hout = (hin + 2 * pad - k) / stride + 1, wout = (win + 2 * pad - k) / stride + 1;
  if (hout <= 0 || wout <= 0) return SASPA_ERANGE;
  if (pad >= k) return SASPA_ERANGE;                      // a window must hold at least one real pixel
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  long long blocks = ((long long)batch * hout * wout * (C / 8) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const dim3 g((unsigned)blocks), t(256);
  if (dtype == SASPA_BF16) {
    if (mode == 0) hipLaunchKernelGGL((pool2d_kernel<bf16_t, 0>), g, t, 0, s, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, batch, hin, win, C, k, stride, pad, hout, wout);
    else hipLaunchKernelGGL((pool2d_kernel<bf16_t, 1>), g, t, 0, s, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, batch, hin, win, C, k, stride, pad, hout, wout);
  } else if (dtype == SASPA_F32) {
    if (mode == 0) hipLaunchKernelGGL((pool2d_kernel<float, 0>), g, t, 0, s, (const float*)x, ldx, (float*)y, ldy, batch, hin, win, C, k, stride, pad, hout, wout);
    else hipLaunchKernelGGL((pool2d_kernel<float, 1>), g, t, 0, s, (const float*)x, ldx, (float*)y, ldy, batch, hin, win, C, k, stride, pad, hout, wout);
  } else {
    return SASPA_EINVAL;
  }
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_signsqrt_l2norm(const float* x, long long ldx, float* y, long long ldy, int rows, long long C, float eps,
                                     float scale, void* stream) {
  if (!x || !y || rows <= 0 || C <= 0 || ldx < C || ldy < C) return SASPA_EINVAL;
  hipLaunchKernelGGL(signsqrt_l2norm_kernel, dim3((unsigned)rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, ldx, y, ldy,
                     C, eps, scale);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_lpips_layer(int dtype, const void* a, int lda, const void* r, int ldr, const int* ref_index, const float* w,
                                 float* dist, float* workspace, int n, int hw, int C, int accumulate, void* stream) {
  if (!a || !r || !ref_index || !w || !dist || !workspace || n <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (dtype != SASPA_BF16 && dtype != SASPA_F32) return SASPA_EINVAL;
  if (C % 8 || lda % 8 || ldr % 8 || lda < C || ldr < C || !aligned16(a) || !aligned16(r) || !aligned16(w)) return SASPA_EALIGN;
  if ((reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(ref_index)) & 3u) return SASPA_EALIGN;
  if (C > SASPA_LPIPS_MAX_C || n > 65535) return SASPA_ERANGE;          // 8 channels per lane, one wave per pixel; grid.y
  int lpp = 1;
  while (lpp * 8 < C) lpp <<= 1;
  const int slots = 256 / lpp;
  // at least four pixels per slot and workgroup, at most SASPA_LPIPS_MAX_BLOCKS workgroups per pair: (hw, C) decide, never n
  int nblk = (hw + 4 * slots - 1) / (4 * slots);
  if (nblk > SASPA_LPIPS_MAX_BLOCKS) nblk = SASPA_LPIPS_MAX_BLOCKS;
  const int ppb = (hw + nblk - 1) / nblk;
  nblk = (hw + ppb - 1) / ppb;                                           // no empty workgroup
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 g((unsigned)nblk, (unsigned)n), t(256);
  if (dtype == SASPA_BF16)
    hipLaunchKernelGGL(lpips_layer_kernel<bf16_t>, g, t, 0, s, (const bf16_t*)a, lda, (const bf16_t*)r, ldr, ref_index, w, workspace, hw, C, lpp, ppb);
  else
    hipLaunchKernelGGL(lpips_layer_kernel<float>, g, t, 0, s, (const float*)a, lda, (const float*)r, ldr, ref_index, w, workspace, hw, C, lpp, ppb);
  SASPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)n), dim3(64), 0, s, (const float*)workspace, dist, nblk, hw, accumulate);
  SASPA_CHECK_LAUNCH();
  return 0;
}
