// Elementwise / data-movement kernels of the sampling loop (all HBM-bound, 16-byte vectors
// per lane, grid-stride with a capped grid).  See include/saspa_hip.h.
#include "common.h"

namespace {

constexpr int kMaxBlocks = 8192;
inline unsigned grid_for(long long items) {
  long long b = (items + 255) / 256;
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}

template <typename T>
__device__ __forceinline__ void load8(const T* p, float* v) {
  if constexpr (sizeof(T) == 2) {
    Elem<T>::load_chunk(p, v);
  } else {
    Elem<T>::load_chunk(p, v);
    Elem<T>::load_chunk(p + 4, v + 4);
  }
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float* v) {
  if constexpr (sizeof(T) == 2) {
    Elem<T>::store_chunk(p, v);
  } else {
    Elem<T>::store_chunk(p, v);
    Elem<T>::store_chunk(p + 4, v + 4);
  }
}

// GEGLU: y[m][f] = x[m][f] * gelu_erf(x[m][F + f])
template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* x, int ldx, T* y, int ldy, long long rows, int F) {
  const int F8 = F >> 3;
  const long long total = rows * F8;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const long long row = it / F8;
    const int f = (int)(it - row * F8) * 8;
    float a[8], g[8];
    load8(x + row * ldx + f, a);
    load8(x + row * ldx + F + f, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = a[j] * (0.5f * g[j] * (1.0f + erff(g[j] * 0.70710678118654752440f)));
    store8(y + row * ldy + f, a);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void activation_kernel(int act, const T* x, int ldx, T* y, int ldy, long long rows, int C) {
  const int C8 = C >> 3;
  const long long total = rows * C8;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const long long row = it / C8;
    const int c = (int)(it - row * C8) * 8;
    float a[8];
    load8(x + row * ldx + c, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (act == 1) a[j] = silu_f(a[j]);
      else if (act == 5) a[j] = fmaxf(a[j], 0.0f);
      else if (act == 4) a[j] = 0.5f * a[j] * (1.0f + erff(a[j] * 0.70710678118654752440f));   // exact (erf) GELU: BERT / Q-Former FFN
      else a[j] = a[j] / (1.0f + expf(-1.702f * a[j]));
    }
    store8(y + row * ldy + c, a);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int* ids, int n, int npos, const T* tok, const T* pos, int C,
                                                           T* out) {
  const int C8 = C >> 3;
  const long long total = (long long)n * C8;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const int i = (int)(it / C8);
    const int c = (int)(it - (long long)i * C8) * 8;
    float a[8], b[8];
    load8(tok + (long long)ids[i] * C + c, a);
    load8(pos + (long long)(i % npos) * C + c, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += b[j];
    store8(out + (long long)i * C + c, a);
  }
}

// ContextCLIPTextEmbeddings (BLIP-Diffusion): row p of sequence b is the token embedding of the prompt with
// `nctx` subject-token embeddings spliced in at position `cbeg`, plus the position embedding of p.
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_ctx_kernel(const int* ids, int nseq, int ntok, const T* ctx, int nctx, int cbeg,
                                                               const T* tok, const T* pos, int C, T* out) {
  const int C8 = C >> 3;
  const int len = ntok + nctx;
  const long long total = (long long)nseq * len * C8;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const int row = (int)(it / C8);
    const int c = (int)(it - (long long)row * C8) * 8;
    const int b = row / len, p = row - b * len;
    float a[8], q[8];
    if (p >= cbeg && p < cbeg + nctx) load8(ctx + ((long long)b * nctx + (p - cbeg)) * C + c, a);
    else load8(tok + (long long)ids[b * ntok + (p < cbeg ? p : p - nctx)] * C + c, a);
    load8(pos + (long long)p * C + c, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += q[j];
    store8(out + (long long)row * C + c, a);
  }
}

// CFG + one linear multistep (PNDM / PLMS) update.  e = eu + g (ec - eu) is optionally stored in the history
// ring; m = w_cur e + sum_k w[k] hist[k]; x' = cx * s + cm * m with s = the saved sample or x itself.
// table != nullptr (hipGraph replays): the step's parameters are row *index of a device table [evaluations][10] =
// (store_slot, w_cur, w_hist[4], coef_sample, coef_model, save_sample, use_saved); `saved` is then a real buffer: the
// step with save_sample copies x into it before the update, the step with use_saved reads it instead of x.
template <typename T>
__global__ __launch_bounds__(256) void cfg_plms_kernel(const T* eps, T* x, T* hist, const T* sample, int nimg, long long hw, int C,
                                                       float g, int store_slot, float w_cur, float w0, float w1, float w2, float w3,
                                                       float cx, float cm, const float* table = nullptr, const int* index = nullptr,
                                                       T* saved = nullptr) {
  const long long total = (long long)nimg * hw;
  const long long half = total * 8;
  bool save = false;
  if (table) {
    const float* r = table + 10ll * (*index);
    store_slot = (int)r[0]; w_cur = r[1]; w0 = r[2]; w1 = r[3]; w2 = r[4]; w3 = r[5]; cx = r[6]; cm = r[7];
    save = r[8] != 0.f;
    sample = (r[9] != 0.f) ? saved : nullptr;
  }
  const float w[4] = {w0, w1, w2, w3};
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    float eu[8], ec[8], sv[8], e[8], m[8], o[8];
    load8(eps + it * 8, eu);
    load8(eps + half + it * 8, ec);
    load8((sample ? sample : x) + it * 8, sv);
    if (save) store8(saved + it * 8, sv);           // sv is x here (a saving step never reads the saved sample)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      e[j] = eu[j] + g * (ec[j] - eu[j]);
      m[j] = w_cur * e[j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (w[k] != 0.f) {   // uniform
        float h[8];
        load8(hist + k * half + it * 8, h);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] += w[k] * h[j];
      }
    }
    if (store_slot >= 0) store8(hist + store_slot * half + it * 8, e);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (j < C) ? (cx * sv[j] + cm * m[j]) : 0.f;
    store8(x + it * 8, o);
    store8(x + half + it * 8, o);
  }
}

// CFG + one UniPC step (UniPCMultistepScheduler, solver_order <= 2, predict_x0; saspa_aug_amd/scheduler.py derives the row):
//   x0 = (x - r[1] * e) * r[0];  if r[2]: x = r[3] * last + r[4] * m0 + r[5] * m1 + r[6] * x0   (corrector)
//   m1, m0, last = m0, x0, x;    x = r[7] * x + r[8] * m0 + r[9] * m1                          (predictor)
// state = [last | m0 | m1], each [nimg][hw][8] in the activation dtype.  row = 12 floats, from the launch arguments or
// from row *index of a device table (hipGraph replays).
struct UniPcRow { float v[12]; };
// CFG = false (sd_xl-turbo, guidance_scale 0): eps holds ONE evaluation per image and x is not duplicated
template <typename T, bool CFG = true>
__global__ __launch_bounds__(256) void cfg_unipc_kernel(const T* eps, T* x, T* state, int nimg, long long hw, int C, float g, UniPcRow row,
                                                        const float* table, const int* index) {
  const long long total = (long long)nimg * hw;
  const long long half = total * 8;
  float r[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) r[j] = table ? table[12ll * (*index) + j] : row.v[j];
  T* last = state;
  T* m0p = state + half;
  T* m1p = state + 2 * half;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    float eu[8], ec[8], xv[8], lv[8], m0[8], m1[8], x0[8], o[8];
    load8(eps + it * 8, eu);
    if (CFG) load8(eps + half + it * 8, ec);
    load8(x + it * 8, xv);
    load8(m0p + it * 8, m0);
    load8(m1p + it * 8, m1);
    if (r[2] != 0.f) load8(last + it * 8, lv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float e = CFG ? eu[j] + g * (ec[j] - eu[j]) : eu[j];
      x0[j] = (xv[j] - r[1] * e) * r[0];
      float xc = xv[j];
      if (r[2] != 0.f) xc = r[3] * lv[j] + r[4] * m0[j] + r[5] * m1[j] + r[6] * x0[j];
      lv[j] = (j < C) ? xc : 0.f;
      o[j] = (j < C) ? (r[7] * xc + r[8] * x0[j] + r[9] * m0[j]) : 0.f;        // new m0 = x0, new m1 = old m0
      if (j >= C) x0[j] = 0.f;
    }
    store8(last + it * 8, lv);
    store8(m1p + it * 8, m0);
    store8(m0p + it * 8, x0);
    store8(x + it * 8, o);
    if (CFG) store8(x + half + it * 8, o);
  }
}

// the CFG-free form of saspa_cfg_unipc_step (sd_xl-turbo runs at guidance_scale 0: run_aug/run_aug.py:567-571, sampler
// "unipcmultistep" :223-226): eps / x are [nimg][hw][8], state as below
extern "C" int saspa_unipc_step(int dtype, const void* eps, void* x, void* state, int nimg, long long hw, int C, int ldc,
                                const float* row, const float* table, const int* index, void* stream) {
  if (!eps || !x || !state || nimg <= 0 || hw <= 0 || C <= 0 || (!row && !(table && index))) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x) || !aligned16(state)) return SASPA_EALIGN;
  UniPcRow rr{};
  if (row && !table)
    for (int j = 0; j < 12; ++j) rr.v[j] = row[j];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_unipc_kernel<h16_t, false>), dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, (h16_t*)state, nimg, hw, C, 0.f, rr, table, index);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_unipc_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, (float*)state, nimg, hw, C, 0.f, rr, table, index);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_cfg_unipc_step(int dtype, const void* eps, void* x, void* state, int nimg, long long hw, int C, int ldc,
                                    float guidance, const float* row, const float* table, const int* index, void* stream) {
  if (!eps || !x || !state || nimg <= 0 || hw <= 0 || C <= 0 || (!row && !(table && index))) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x) || !aligned16(state)) return SASPA_EALIGN;
  UniPcRow rr{};
  if (row && !table)
    for (int j = 0; j < 12; ++j) rr.v[j] = row[j];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(cfg_unipc_kernel<h16_t>, dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, (h16_t*)state, nimg, hw, C, guidance, rr, table, index);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(cfg_unipc_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, (float*)state, nimg, hw, C, guidance, rr, table, index);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

// CFG + DDIM (eta = 0).  One item = one pixel (ldc == 8 channels, C live).
// CFG == false: plain DDIM step on nimg samples (guidance off: SDXL-Turbo, run_aug/run_aug.py:568).
// coefs != nullptr: the four coefficients come from row *index of a device table [steps][4] (hipGraph replays: one
// captured step serves every timestep, the host only bumps the device-side step counter).
template <typename T, bool CFG>
__global__ __launch_bounds__(256) void cfg_ddim_kernel(const T* eps, T* x, int nimg, long long hw, int C, float g, float sa_t,
                                                       float s1m_t, float sa_p, float s1m_p, const float* coefs = nullptr,
                                                       const int* index = nullptr) {
  if (coefs) {
    const float* c4 = coefs + 4ll * (*index);
    sa_t = c4[0]; s1m_t = c4[1]; sa_p = c4[2]; s1m_p = c4[3];
  }
  const long long total = (long long)nimg * hw;
  const long long half = total * 8;  // elements in one CFG half
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    float eu[8], ec[8], xv[8], o[8];
    load8(eps + it * 8, eu);
    if (CFG) load8(eps + half + it * 8, ec);
    load8(x + it * 8, xv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float e = CFG ? eu[j] + g * (ec[j] - eu[j]) : eu[j];
      const float x0 = (xv[j] - s1m_t * e) / sa_t;
      o[j] = (j < C) ? (sa_p * x0 + s1m_p * e) : 0.f;
    }
    store8(x + it * 8, o);
    if (CFG) store8(x + half + it * 8, o);
  }
}

// v-prediction forms (prediction_type "v_prediction": the 768-pixel stable-diffusion-2-1 checkpoint).  The network output is
// v = sqrt(a_t) eps - sqrt(1 - a_t) x0; everything else (layouts, CFG flag, coefs / index) is as in cfg_ddim_kernel.
//   v = vu + g (vc - vu);  x0 = sa_t x - s1m_t v;  e = sa_t v + s1m_t x;  x' = sa_p x0 + s1m_p e
// fp32 throughout, one rounding at the store; no division, so the result is finite for every a_t.
template <typename T, bool CFG>
__global__ __launch_bounds__(256) void cfg_ddim_v_kernel(const T* vout, T* x, int nimg, long long hw, int C, float g, float sa_t,
                                                         float s1m_t, float sa_p, float s1m_p, const float* coefs = nullptr,
                                                         const int* index = nullptr) {
  if (coefs) {
    const float* c4 = coefs + 4ll * (*index);
    sa_t = c4[0]; s1m_t = c4[1]; sa_p = c4[2]; s1m_p = c4[3];
  }
  const long long total = (long long)nimg * hw;
  const long long half = total * 8;  // elements in one CFG half
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    float vu[8], vc[8], xv[8], o[8];
    load8(vout + it * 8, vu);
    if (CFG) load8(vout + half + it * 8, vc);
    load8(x + it * 8, xv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = CFG ? vu[j] + g * (vc[j] - vu[j]) : vu[j];
      const float x0 = sa_t * xv[j] - s1m_t * v;
      const float e = sa_t * v + s1m_t * xv[j];
      o[j] = (j < C) ? (sa_p * x0 + s1m_p * e) : 0.f;
    }
    store8(x + it * 8, o);
    if (CFG) store8(x + half + it * 8, o);
  }
}

// cfg_unipc_kernel with a v-prediction network: x0 = r[10] * x - r[1] * v (r[10] = alpha_t, r[1] = sigma_t; r[0] is not read),
// then the unchanged corrector / predictor update on x0.
template <typename T, bool CFG>
__global__ __launch_bounds__(256) void cfg_unipc_v_kernel(const T* vout, T* x, T* state, int nimg, long long hw, int C, float g,
                                                          UniPcRow row, const float* table, const int* index) {
  const long long total = (long long)nimg * hw;
  const long long half = total * 8;
  float r[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) r[j] = table ? table[12ll * (*index) + j] : row.v[j];
  T* last = state;
  T* m0p = state + half;
  T* m1p = state + 2 * half;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    float vu[8], vc[8], xv[8], lv[8], m0[8], m1[8], x0[8], o[8];
    load8(vout + it * 8, vu);
    if (CFG) load8(vout + half + it * 8, vc);
    load8(x + it * 8, xv);
    load8(m0p + it * 8, m0);
    load8(m1p + it * 8, m1);
    if (r[2] != 0.f) load8(last + it * 8, lv);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = CFG ? vu[j] + g * (vc[j] - vu[j]) : vu[j];
      x0[j] = r[10] * xv[j] - r[1] * v;
      float xc = xv[j];
      if (r[2] != 0.f) xc = r[3] * lv[j] + r[4] * m0[j] + r[5] * m1[j] + r[6] * x0[j];
      lv[j] = (j < C) ? xc : 0.f;
      o[j] = (j < C) ? (r[7] * xc + r[8] * x0[j] + r[9] * m0[j]) : 0.f;        // new m0 = x0, new m1 = old m0
      if (j >= C) x0[j] = 0.f;
    }
    store8(last + it * 8, lv);
    store8(m1p + it * 8, m0);
    store8(m0p + it * 8, x0);
    store8(x + it * 8, o);
    if (CFG) store8(x + half + it * 8, o);
  }
}

// Three-branch guidance + DDIM (eta = 0): the InstructPix2Pix update.  eps / x: [3 * nimg][hw][8] in the groups (uncond | image |
// text); the UNet input carries the noisy latents in channels < C and the image latents (zeros in group 0) in channels C..7.
//   e = e0 + g (e2 - e1) + ig (e1 - e0), then the DDIM step of cfg_ddim_kernel on e and the x of group 0.
// One thread owns one pixel's word of each group: channels < C of all three groups get the new sample (fp32 arithmetic, one
// rounding), channels C..7 are stored back as the bits that were loaded.  coefs / index: as cfg_ddim_kernel.
template <typename T> struct alignas(16) Pixel8 { T v[8]; };
template <typename T>
__global__ __launch_bounds__(256) void cfg3_ddim_kernel(const T* eps, T* x, int nimg, long long hw, int C, float g, float ig,
                                                        float sa_t, float s1m_t, float sa_p, float s1m_p,
                                                        const float* coefs = nullptr, const int* index = nullptr) {
  if (coefs) {
    const float* c4 = coefs + 4ll * (*index);
    sa_t = c4[0]; s1m_t = c4[1]; sa_p = c4[2]; s1m_p = c4[3];
  }
  const long long total = (long long)nimg * hw;
  const long long group = total * 8;  // elements in one of the three groups
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    float e0[8], e1[8], e2[8];
    load8(eps + it * 8, e0);
    load8(eps + group + it * 8, e1);
    load8(eps + 2 * group + it * 8, e2);
    Pixel8<T> w0 = *reinterpret_cast<const Pixel8<T>*>(x + it * 8);
    Pixel8<T> w1 = *reinterpret_cast<const Pixel8<T>*>(x + group + it * 8);
    Pixel8<T> w2 = *reinterpret_cast<const Pixel8<T>*>(x + 2 * group + it * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < C) {
        const float e = e0[j] + g * (e2[j] - e1[j]) + ig * (e1[j] - e0[j]);
        const float x0 = ((float)w0.v[j] - s1m_t * e) / sa_t;
        const T o = (T)(sa_p * x0 + s1m_p * e);
        w0.v[j] = o;
        w1.v[j] = o;
        w2.v[j] = o;
      }
    }
    *reinterpret_cast<Pixel8<T>*>(x + it * 8) = w0;
    *reinterpret_cast<Pixel8<T>*>(x + group + it * 8) = w1;
    *reinterpret_cast<Pixel8<T>*>(x + 2 * group + it * 8) = w2;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void scale_kernel(const T* x, T* y, long long n8, float s) {
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < n8; it += (long long)gridDim.x * 256) {
    float a[8];
    load8(x + it * 8, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= s;
    store8(y + it * 8, a);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void u8_to_act_kernel(const uint8_t* src, T* dst, long long npix) {
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < npix; it += (long long)gridDim.x * 256) {
    const uint8_t* s = src + it * 3;
    float a[8] = {s[0] / 255.0f, s[1] / 255.0f, s[2] / 255.0f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store8(dst + it * 8, a);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void act_to_u8_kernel(const T* x, int ldx, uint8_t* dst, long long npix) {
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < npix; it += (long long)gridDim.x * 256) {
    float a[4];
    Elem<T>::load4(x + it * ldx, a);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float v = a[j] / 2.0f + 0.5f;
      v = fminf(fmaxf(v, 0.0f), 1.0f);
      dst[it * 3 + j] = (uint8_t)rintf(v * 255.0f);
    }
  }
}

}  // namespace


extern "C" int saspa_geglu(int dtype, const void* x, int ldx, void* y, int ldy, long long rows, int F, void* stream) {
  if (!x || !y || rows <= 0 || F <= 0) return SASPA_EINVAL;
  if (F % 8 || ldx % 8 || ldy % 8 || !aligned16(x) || !aligned16(y)) return SASPA_EALIGN;
  if (ldx < 2 * F || ldy < F) return SASPA_ERANGE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(geglu_kernel<h16_t>, dim3(grid_for(rows * (F / 8))), dim3(256), 0, s, (const h16_t*)x, ldx, (h16_t*)y, ldy, rows, F);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(geglu_kernel<float>, dim3(grid_for(rows * (F / 8))), dim3(256), 0, s, (const float*)x, ldx, (float*)y, ldy, rows, F);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_activation(int dtype, int act, const void* x, int ldx, void* y, int ldy, long long rows, int C,
                                void* stream) {
  if (!x || !y || rows <= 0 || C <= 0 || (act != 1 && act != 2 && act != 4 && act != 5)) return SASPA_EINVAL;
  if (C % 8 || ldx % 8 || ldy % 8 || !aligned16(x) || !aligned16(y)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(activation_kernel<h16_t>, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, act, (const h16_t*)x, ldx, (h16_t*)y, ldy, rows, C);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(activation_kernel<float>, dim3(grid_for(rows * (C / 8))), dim3(256), 0, s, act, (const float*)x, ldx, (float*)y, ldy, rows, C);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_embed_tokens(int dtype, const int* ids, int n, int npos, const void* tok, const void* pos, int C,
                                  void* out, void* stream) {
  if (!ids || !tok || !pos || !out || n <= 0 || npos <= 0 || C <= 0) return SASPA_EINVAL;
  if (C % 8 || !aligned16(tok) || !aligned16(pos) || !aligned16(out)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(embed_tokens_kernel<h16_t>, dim3(grid_for((long long)n * (C / 8))), dim3(256), 0, s, ids, n, npos, (const h16_t*)tok, (const h16_t*)pos, C, (h16_t*)out);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(embed_tokens_kernel<float>, dim3(grid_for((long long)n * (C / 8))), dim3(256), 0, s, ids, n, npos, (const float*)tok, (const float*)pos, C, (float*)out);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_embed_tokens_ctx(int dtype, const int* ids, int nseq, int ntok, const void* ctx, int nctx, int ctx_begin,
                                      const void* tok, const void* pos, int C, void* out, void* stream) {
  if (!ids || !tok || !pos || !out || nseq <= 0 || ntok <= 0 || C <= 0 || nctx < 0) return SASPA_EINVAL;
  if (nctx > 0 && !ctx) return SASPA_EINVAL;
  if (ctx_begin < 0 || ctx_begin > ntok) return SASPA_ERANGE;
  if (C % 8 || !aligned16(tok) || !aligned16(pos) || !aligned16(out) || (ctx && !aligned16(ctx))) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nseq * (ntok + nctx) * (C / 8));
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(embed_tokens_ctx_kernel<h16_t>, dim3(grid), dim3(256), 0, s, ids, nseq, ntok, (const h16_t*)ctx, nctx, ctx_begin, (const h16_t*)tok, (const h16_t*)pos, C, (h16_t*)out);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(embed_tokens_ctx_kernel<float>, dim3(grid), dim3(256), 0, s, ids, nseq, ntok, (const float*)ctx, nctx, ctx_begin, (const float*)tok, (const float*)pos, C, (float*)out);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_cfg_plms_step(int dtype, const void* eps, void* x, void* hist, const void* sample, int nimg, long long hw,
                                   int C, int ldc, float guidance, int store_slot, float w_cur, const float* w_hist,
                                   float coef_sample, float coef_model, void* stream) {
  if (!eps || !x || !hist || !w_hist || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8 || store_slot < -1 || store_slot > 3) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x) || !aligned16(hist) || (sample && !aligned16(sample))) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(cfg_plms_kernel<h16_t>, dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, (h16_t*)hist, (const h16_t*)sample, nimg, hw, C, guidance, store_slot, w_cur, w_hist[0], w_hist[1], w_hist[2], w_hist[3], coef_sample, coef_model);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(cfg_plms_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, (float*)hist, (const float*)sample, nimg, hw, C, guidance, store_slot, w_cur, w_hist[0], w_hist[1], w_hist[2], w_hist[3], coef_sample, coef_model);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_cfg_plms_step_dev(int dtype, const void* eps, void* x, void* hist, void* saved, int nimg, long long hw, int C,
                                       int ldc, float guidance, const float* table, const int* index, void* stream) {
  if (!eps || !x || !hist || !saved || !table || !index || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x) || !aligned16(hist) || !aligned16(saved)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(cfg_plms_kernel<h16_t>, dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, (h16_t*)hist, (const h16_t*)nullptr, nimg, hw, C, guidance, -1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, table, index, (h16_t*)saved);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(cfg_plms_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, (float*)hist, (const float*)nullptr, nimg, hw, C, guidance, -1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, table, index, (float*)saved);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_cfg_ddim_step(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc,
                                   float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                   float sqrt_1m_a_prev, void* stream) {
  if (!eps || !x || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x)) return SASPA_EALIGN;
  if (!(sqrt_a_t > 0.f)) return SASPA_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_ddim_kernel<h16_t, true>), dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, nimg, hw, C, guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_ddim_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, nimg, hw, C, guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_ddim_step(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, float sqrt_a_t,
                               float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, void* stream) {
  if (!eps || !x || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x)) return SASPA_EALIGN;
  if (!(sqrt_a_t > 0.f)) return SASPA_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_ddim_kernel<h16_t, false>), dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, nimg, hw, C, 0.f, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_ddim_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, nimg, hw, C, 0.f, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

// ---- device-side step state for hipGraph replays of the sampling loop ----
namespace {
__global__ __launch_bounds__(256) void gather_row_kernel(const float* __restrict__ table, long long row_elems,
                                                         const int* __restrict__ index, float* __restrict__ dst, long long n) {
  const float* src = table + (long long)(*index) * row_elems;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < n; it += (long long)gridDim.x * 256) dst[it] = src[it];
}
__global__ void index_add_kernel(int* index, int delta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *index += delta;
}
// One sleeping wave: shader-clock cycles (s_memtime) against the constant 100 MHz counter (s_memrealtime) over a window of
// `iters` x s_sleep 127 (64 x 127 shader clocks each).  Launched on a side stream WHILE the hot path runs, it reads the
// clock the power management grants the loaded chip; a sleeping wave issues nothing and holds 1 wave slot of one SIMD.
__global__ void clock_probe_kernel(unsigned long long* out, int iters) {
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < iters; ++i) __builtin_amdgcn_s_sleep(127);
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = r1 - r0;
  }
}
}  // namespace

extern "C" int saspa_clock_probe(unsigned long long* out2, int iters, void* stream) {
  if (!out2) return SASPA_EINVAL;
  if (iters <= 0 || iters > 100000) return SASPA_ERANGE;          // <= ~0.4 s at 2 GHz: a probe always terminates
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), out2, iters);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_gather_row_f32(const float* table, long long row_elems, const int* index, float* dst, long long n,
                                    void* stream) {
  if (!table || !index || !dst || row_elems <= 0 || n <= 0 || n > row_elems) return SASPA_EINVAL;
  hipLaunchKernelGGL(gather_row_kernel, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), table, row_elems,
                     index, dst, n);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_index_add(int* index, int delta, void* stream) {
  if (!index) return SASPA_EINVAL;
  hipLaunchKernelGGL(index_add_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), index, delta);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_ddim_step_dev(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, int cfg,
                                   float guidance, const float* coefs, const int* index, void* stream) {
  if (!eps || !x || !coefs || !index || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(eps) || !aligned16(x)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF) {
    if (cfg) hipLaunchKernelGGL((cfg_ddim_kernel<h16_t, true>), dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, nimg, hw, C, guidance, 1.f, 0.f, 1.f, 0.f, coefs, index);
    else hipLaunchKernelGGL((cfg_ddim_kernel<h16_t, false>), dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, nimg, hw, C, 0.f, 1.f, 0.f, 1.f, 0.f, coefs, index);
  } else if (dtype == SASPA_F32 && kServesF32) {
    if (cfg) hipLaunchKernelGGL((cfg_ddim_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, nimg, hw, C, guidance, 1.f, 0.f, 1.f, 0.f, coefs, index);
    else hipLaunchKernelGGL((cfg_ddim_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, nimg, hw, C, 0.f, 1.f, 0.f, 1.f, 0.f, coefs, index);
  } else {
    return SASPA_EINVAL;
  }
  SASPA_CHECK_LAUNCH();
  return 0;
}

// ---- v-prediction sampler steps: the entry points above with cfg_ddim_v_kernel / cfg_unipc_v_kernel; the host-side checks and
// their order are those of the epsilon entry points ----
extern "C" int saspa_cfg_ddim_step_v(int dtype, const void* v, void* x, int nimg, long long hw, int C, int ldc, float guidance,
                                     float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, void* stream) {
  if (!v || !x || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(v) || !aligned16(x)) return SASPA_EALIGN;
  if (!(sqrt_a_t > 0.f)) return SASPA_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_ddim_v_kernel<h16_t, true>), dim3(grid), dim3(256), 0, s, (const h16_t*)v, (h16_t*)x, nimg, hw, C, guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_ddim_v_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)v, (float*)x, nimg, hw, C, guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_ddim_step_v(int dtype, const void* v, void* x, int nimg, long long hw, int C, int ldc, float sqrt_a_t,
                                 float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, void* stream) {
  if (!v || !x || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(v) || !aligned16(x)) return SASPA_EALIGN;
  if (!(sqrt_a_t > 0.f)) return SASPA_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_ddim_v_kernel<h16_t, false>), dim3(grid), dim3(256), 0, s, (const h16_t*)v, (h16_t*)x, nimg, hw, C, 0.f, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_ddim_v_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)v, (float*)x, nimg, hw, C, 0.f, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_ddim_step_v_dev(int dtype, const void* v, void* x, int nimg, long long hw, int C, int ldc, int cfg,
                                     float guidance, const float* coefs, const int* index, void* stream) {
  if (!v || !x || !coefs || !index || nimg <= 0 || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(v) || !aligned16(x)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF) {
    if (cfg) hipLaunchKernelGGL((cfg_ddim_v_kernel<h16_t, true>), dim3(grid), dim3(256), 0, s, (const h16_t*)v, (h16_t*)x, nimg, hw, C, guidance, 1.f, 0.f, 1.f, 0.f, coefs, index);
    else hipLaunchKernelGGL((cfg_ddim_v_kernel<h16_t, false>), dim3(grid), dim3(256), 0, s, (const h16_t*)v, (h16_t*)x, nimg, hw, C, 0.f, 1.f, 0.f, 1.f, 0.f, coefs, index);
  } else if (dtype == SASPA_F32 && kServesF32) {
    if (cfg) hipLaunchKernelGGL((cfg_ddim_v_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)v, (float*)x, nimg, hw, C, guidance, 1.f, 0.f, 1.f, 0.f, coefs, index);
    else hipLaunchKernelGGL((cfg_ddim_v_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)v, (float*)x, nimg, hw, C, 0.f, 1.f, 0.f, 1.f, 0.f, coefs, index);
  } else {
    return SASPA_EINVAL;
  }
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_unipc_step_v(int dtype, const void* v, void* x, void* state, int nimg, long long hw, int C, int ldc,
                                  const float* row, const float* table, const int* index, void* stream) {
  if (!v || !x || !state || nimg <= 0 || hw <= 0 || C <= 0 || (!row && !(table && index))) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(v) || !aligned16(x) || !aligned16(state)) return SASPA_EALIGN;
  UniPcRow rr{};
  if (row && !table)
    for (int j = 0; j < 12; ++j) rr.v[j] = row[j];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_unipc_v_kernel<h16_t, false>), dim3(grid), dim3(256), 0, s, (const h16_t*)v, (h16_t*)x, (h16_t*)state, nimg, hw, C, 0.f, rr, table, index);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_unipc_v_kernel<float, false>), dim3(grid), dim3(256), 0, s, (const float*)v, (float*)x, (float*)state, nimg, hw, C, 0.f, rr, table, index);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_cfg_unipc_step_v(int dtype, const void* v, void* x, void* state, int nimg, long long hw, int C, int ldc,
                                      float guidance, const float* row, const float* table, const int* index, void* stream) {
  if (!v || !x || !state || nimg <= 0 || hw <= 0 || C <= 0 || (!row && !(table && index))) return SASPA_EINVAL;
  if (ldc != 8 || C > 8) return SASPA_ERANGE;
  if (!aligned16(v) || !aligned16(x) || !aligned16(state)) return SASPA_EALIGN;
  UniPcRow rr{};
  if (row && !table)
    for (int j = 0; j < 12; ++j) rr.v[j] = row[j];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL((cfg_unipc_v_kernel<h16_t, true>), dim3(grid), dim3(256), 0, s, (const h16_t*)v, (h16_t*)x, (h16_t*)state, nimg, hw, C, guidance, rr, table, index);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL((cfg_unipc_v_kernel<float, true>), dim3(grid), dim3(256), 0, s, (const float*)v, (float*)x, (float*)state, nimg, hw, C, guidance, rr, table, index);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

// host-side checks shared by the two entry points of cfg3_ddim_kernel (nothing is launched on a refusal)
static int cfg3_ddim_check(int dtype, const void* eps, const void* x, int nimg, long long hw, int C, int ldc) {
  if (!eps || !x || hw <= 0 || C <= 0) return SASPA_EINVAL;
  if (!aligned16(eps) || !aligned16(x)) return SASPA_EALIGN;
  if (ldc != 8 || C > 4 || nimg < 1) return SASPA_ERANGE;
  if (!(dtype == SASPA_HALF || (dtype == SASPA_F32 && kServesF32))) return SASPA_EINVAL;
  return 0;
}

extern "C" int saspa_cfg3_ddim_step(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, float guidance,
                                    float image_guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                    float sqrt_1m_a_prev, void* stream) {
  const int rc = cfg3_ddim_check(dtype, eps, x, nimg, hw, C, ldc);
  if (rc) return rc;
  if (!(sqrt_a_t > 0.f)) return SASPA_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(cfg3_ddim_kernel<h16_t>, dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, nimg, hw, C, guidance, image_guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  else
    hipLaunchKernelGGL(cfg3_ddim_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, nimg, hw, C, guidance, image_guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev);
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_cfg3_ddim_step_dev(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, float guidance,
                                        float image_guidance, const float* coefs, const int* index, void* stream) {
  if (!coefs || !index) return SASPA_EINVAL;
  const int rc = cfg3_ddim_check(dtype, eps, x, nimg, hw, C, ldc);
  if (rc) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = grid_for((long long)nimg * hw);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(cfg3_ddim_kernel<h16_t>, dim3(grid), dim3(256), 0, s, (const h16_t*)eps, (h16_t*)x, nimg, hw, C, guidance, image_guidance, 1.f, 0.f, 1.f, 0.f, coefs, index);
  else
    hipLaunchKernelGGL(cfg3_ddim_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)eps, (float*)x, nimg, hw, C, guidance, image_guidance, 1.f, 0.f, 1.f, 0.f, coefs, index);
  SASPA_CHECK_LAUNCH();
  return 0;
}

// img2img start latents (SDEdit): one 8-channel pixel per lane.  moments = quant_conv output (mean in channels 0..3, logvar
// in 4..7); x0 = (mean + exp(0.5 * clamp(logvar, -30, 20)) * e1) * scaling; out = sa * x0 + s1m * e2 (scheduler.add_noise)
template <typename T>
__global__ __launch_bounds__(256) void vae_sample_noise_kernel(const T* mom, const T* e1, const T* e2, T* out, long long npix,
                                                               float scaling, float sa, float s1m) {
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < npix; it += (long long)gridDim.x * 256) {
    float m[8], a[8], b[8], o[8];
    load8(mom + it * 8, m);
    load8(e1 + it * 8, a);
    load8(e2 + it * 8, b);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float lv = fminf(fmaxf(m[4 + c], -30.0f), 20.0f);
      const float x0 = (m[c] + expf(0.5f * lv) * a[c]) * scaling;
      o[c] = sa * x0 + s1m * b[c];
      o[4 + c] = 0.0f;
    }
    store8(out + it * 8, o);
  }
}

extern "C" int saspa_vae_sample_noise(int dtype, const void* moments, const void* e1, const void* e2, void* out, long long npix,
                                      float scaling, float sa, float s1m, void* stream) {
  if (!moments || !e1 || !e2 || !out || npix <= 0) return SASPA_EINVAL;
  if (!aligned16(moments) || !aligned16(e1) || !aligned16(e2) || !aligned16(out)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(vae_sample_noise_kernel<h16_t>, dim3(grid_for(npix)), dim3(256), 0, s, (const h16_t*)moments, (const h16_t*)e1,
                       (const h16_t*)e2, (h16_t*)out, npix, scaling, sa, s1m);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(vae_sample_noise_kernel<float>, dim3(grid_for(npix)), dim3(256), 0, s, (const float*)moments, (const float*)e1,
                       (const float*)e2, (float*)out, npix, scaling, sa, s1m);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_scale(int dtype, const void* x, void* y, long long n, float sc, void* stream) {
  if (!x || !y || n <= 0) return SASPA_EINVAL;
  if (n % 8 || !aligned16(x) || !aligned16(y)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(scale_kernel<h16_t>, dim3(grid_for(n / 8)), dim3(256), 0, s, (const h16_t*)x, (h16_t*)y, n / 8, sc);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(scale_kernel<float>, dim3(grid_for(n / 8)), dim3(256), 0, s, (const float*)x, (float*)y, n / 8, sc);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_u8_to_act(int dtype, const uint8_t* src, void* dst, long long npix, void* stream) {
  if (!src || !dst || npix <= 0) return SASPA_EINVAL;
  if (!aligned16(dst)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(u8_to_act_kernel<h16_t>, dim3(grid_for(npix)), dim3(256), 0, s, src, (h16_t*)dst, npix);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(u8_to_act_kernel<float>, dim3(grid_for(npix)), dim3(256), 0, s, src, (float*)dst, npix);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_act_to_u8(int dtype, const void* x, int ldx, uint8_t* dst, long long npix, void* stream) {
  if (!x || !dst || npix <= 0) return SASPA_EINVAL;
  if (ldx % 4 || ldx < 4 || !aligned16(x)) return SASPA_EALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == SASPA_HALF)
    hipLaunchKernelGGL(act_to_u8_kernel<h16_t>, dim3(grid_for(npix)), dim3(256), 0, s, (const h16_t*)x, ldx, dst, npix);
  else if (dtype == SASPA_F32 && kServesF32)
    hipLaunchKernelGGL(act_to_u8_kernel<float>, dim3(grid_for(npix)), dim3(256), 0, s, (const float*)x, ldx, dst, npix);
  else
    return SASPA_EINVAL;
  SASPA_CHECK_LAUNCH();
  return 0;
}

extern "C" int saspa_abi_version(void) { return 20; }
extern "C" int saspa_half_type(void) { return SASPA_HALF; }
extern "C" const char* saspa_build_arch(void) { return "gfx950"; }
