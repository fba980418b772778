// The in-line filter stage (Settings.FILTER_INLINE): one threshold-free score record per augmented image, written on the device while
// the image is still there.  The towers, the linears and saspa_class_head carry the arithmetic; this launch turns their per-batch
// outputs into the 8 fp32 of include/saspa_hip.h (`saspa_filter_record`) and files them in the run's table, so that no score of a batch
// crosses to the host during generation.  One wave per image: the semantic head (argmax and margin over <= 64 prompts) is one lane per
// prompt and a fixed-order (value, index) butterfly; everything else is a copy.  Plain stores, no atomics, nothing but row slot[b].
#include "common.h"

namespace {

// numpy's argmax order: a NaN counts as the maximum and the first one wins; equal values give the lowest index.  `i < 0` = no entry.
struct Cand {
  float v;
  int i;
};

__device__ __forceinline__ Cand pick(Cand a, Cand b) {
  if (b.i < 0) return a;
  if (a.i < 0) return b;
  const bool an = a.v != a.v, bn = b.v != b.v;
  if (an || bn) {
    if (an && bn) return a.i < b.i ? a : b;
    return an ? a : b;
  }
  if (b.v > a.v) return b;
  if (b.v == a.v && b.i < a.i) return b;
  return a;
}

// `pick` is commutative and associative (a total order on (is NaN, value, -index)), so the xor butterfly leaves the same winner in
// every lane whatever the order of the five exchanges.
__device__ __forceinline__ Cand wave_pick(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c = pick(c, Cand{__shfl_xor(c.v, o, 64), __shfl_xor(c.i, o, 64)});
  return c;
}

__global__ __launch_bounds__(64) void filter_record_kernel(const float* __restrict__ sem, int ld, int P, const float* __restrict__ conf_stats,
                                                           const int* __restrict__ conf_idx, const float* __restrict__ pc_stats,
                                                           const int* __restrict__ pc_idx, const unsigned char* __restrict__ bad,
                                                           const int* __restrict__ slot, float* __restrict__ table, int n_rows) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int row = slot[b];
  if ((unsigned)row >= (unsigned)n_rows) return;       // the host wrapper refuses such a slot; a raw caller's is dropped, never written
  const float nan = __builtin_nanf("");
  float arg = nan, margin = nan;
  if (sem) {
    const float v = lane < P ? sem[(long long)b * ld + lane] : 0.0f;
    const Cand all = wave_pick(Cand{v, lane < P ? lane : -1});
    const Cand neg = wave_pick(Cand{v, (lane >= 1 && lane < P) ? lane : -1});
    const float first = __shfl(v, 0, 64);
    arg = (float)all.i;
    margin = neg.i < 0 ? INFINITY : first - neg.v;     // one prompt: nothing to lose against
    if (margin != margin) margin = nan;                // one NaN: the canonical quiet one, whatever the operands carried
  }
  if (lane != 0) return;
  const bool skip = bad && bad[b];
  float4 lo, hi;
  lo.x = skip ? 0.0f : (float)((sem ? 1 : 0) | (conf_stats ? 2 : 0) | (pc_stats ? 4 : 0));
  lo.y = skip ? nan : arg;
  lo.z = skip ? nan : margin;
  lo.w = (skip || !conf_stats) ? nan : (float)conf_idx[2ll * b + 1];
  hi.x = (skip || !conf_stats) ? nan : conf_stats[4ll * b + 1];
  hi.y = (skip || !pc_stats) ? nan : pc_stats[4ll * b + 1];
  hi.z = (skip || !pc_stats) ? nan : (float)pc_idx[2ll * b + 1];
  hi.w = 0.0f;
  float4* out = reinterpret_cast<float4*>(table + 8ll * row);
  out[0] = lo;
  out[1] = hi;
}

}  // namespace

extern "C" int saspa_filter_record(const float* sem, int ld, int P, const float* conf_stats, const int* conf_idx, const float* pc_stats,
                                   const int* pc_idx, const unsigned char* bad, const int* slot, float* table, int n_rows, int rows,
                                   void* stream) {
  if (!slot || !table || rows <= 0 || n_rows <= 0) return SASPA_EINVAL;
  if ((conf_stats == nullptr) != (conf_idx == nullptr) || (pc_stats == nullptr) != (pc_idx == nullptr)) return SASPA_EINVAL;
  if (sem && (P < 1 || P > SASPA_FILTER_RECORD_MAX_P || ld < P)) return SASPA_ERANGE;
  if (rows > n_rows) return SASPA_ERANGE;               // distinct slots inside the table cannot number more than its rows
  if (!aligned16(table)) return SASPA_EALIGN;
  if ((reinterpret_cast<uintptr_t>(sem) | reinterpret_cast<uintptr_t>(conf_stats) | reinterpret_cast<uintptr_t>(conf_idx) |
       reinterpret_cast<uintptr_t>(pc_stats) | reinterpret_cast<uintptr_t>(pc_idx) | reinterpret_cast<uintptr_t>(slot)) & 3u)
    return SASPA_EALIGN;
  hipLaunchKernelGGL(filter_record_kernel, dim3((unsigned)rows), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sem, ld, P, conf_stats,
                     conf_idx, pc_stats, pc_idx, bad, slot, table, n_rows);
  SASPA_CHECK_LAUNCH();
  return 0;
}
