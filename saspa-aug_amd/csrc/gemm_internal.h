// Internal (not exported) entry points shared between the GEMM translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "saspa_hip.h"

// The kernel families of saspa_gemm (saspa_gemm.hip: plan_gemm decides which one runs a problem, with the *_eligible / *_ok
// predicates below; the launchers assume the plan's checks and only decide how to launch).
// 8-wave 256 x (64*fn) ping-pong kernel (saspa_gemm_pp.hip).  bf16, "fast" operand layout only (see saspa_gemm.hip); fn in {4, 5}
// (or a SASPA_GEMM_PP loop flavour).
__attribute__((visibility("hidden"))) int saspa_gemm_pp_launch(const SaspaGemmParams& p, hipStream_t s, int ksplit, int fn);
__attribute__((visibility("hidden"))) bool saspa_gemm_pp_eligible(const SaspaGemmParams& p);
// split-K reduce + epilogue launch shared by both variants (saspa_gemm.hip)
__attribute__((visibility("hidden"))) int saspa_gemm_splitk_reduce(const SaspaGemmParams& p, hipStream_t s, int ksplit);
// N-partitioned tile order (weight-heavy problems): nbn / 8 if the launch should use it, else 0 (saspa_gemm.hip)
__attribute__((visibility("hidden"))) int saspa_gemm_npart8(const SaspaGemmParams& p, int BM, int BN, int G, int tiles);
// Persistent grid of a one-workgroup-per-CU kernel (round 5): `tiles` work items over at most `cap` workgroups.  With tiles just above
// a whole number of rounds (352 row tiles of the 64x88 level at 512x704: 1.375 rounds) a grid of `cap` workgroups makes a few of
// them run one tile more than the rest while the others idle -- and every tile pays the contention of a full chip.  A grid of
// ceil(tiles / rounds) workgroups gives every workgroup the SAME number of tiles on fewer CUs: 176 workgroups x 2 tiles run the
// level-0 conv of that bucket in 149 us against 174 (tools/msplit_704.py: fewer CUs store at once and the power limit leaves them
// a higher clock).
static inline int saspa_balanced_grid(int tiles, int cap) {
  if (cap < 1) cap = 1;
  if (tiles <= cap) return tiles;
  const int rounds = (tiles + cap - 1) / cap;
  return (tiles + rounds - 1) / rounds;
}

// wave-specialised 8-wave kernel for short-K bf16 layers (saspa_gemm_ws.hip)
__attribute__((visibility("hidden"))) int saspa_gemm_ws_launch(const SaspaGemmParams& p, hipStream_t s);
__attribute__((visibility("hidden"))) bool saspa_gemm_ws_eligible(const SaspaGemmParams& p);
// A-stationary kernel for K = 320 pointwise layers (saspa_gemm_as.hip): fused LayerNorm, transposed second output
__attribute__((visibility("hidden"))) int saspa_gemm_as_launch(const SaspaGemmParams& p, hipStream_t s);
__attribute__((visibility("hidden"))) bool saspa_gemm_as_ok(const SaspaGemmParams& p);
// channel slabs of the GroupNorm statistics pass for C / 8 chunks (saspa_norm.hip: layout of SaspaGroupNormParams.partial)
__attribute__((visibility("hidden"))) int saspa_gn_slabs(int c8);
