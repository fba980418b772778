// Implicit-GEMM convolution / linear on gfx950 MFMA (bf16: v_mfma_f32_16x16x32_bf16,
// fp32 parity mode: v_mfma_f32_16x16x4_f32).  See include/saspa_hip.h (SaspaGemmParams).
//
// Structure (one workgroup = 4 waves in a 2x2 grid, each wave WM x WN tiles of 16x16):
//   * A operand = im2col view of up to two channel-concatenated NHWC tensors (optionally
//     nearest-x2 upsampled), B operand = weights [N][K]; both K-contiguous, so one
//     16-byte chunk per lane is exactly one MFMA fragment (8 bf16 / 4 fp32 along K).
//   * K-tile = 128 bytes per row for both dtypes (64 bf16 / 32 fp32): the LDS image, its
//     XOR swizzle (chunk ^ (row & 7): conflict-free for ds_read_b128 row reads) and the
//     staging code are shared between the two precisions.
//   * operands are fetched with raw buffer loads (hardware bounds check -> zeros) whose
//     per-lane offsets are fixed per output tile; the K advance lives in scalar registers.
//   * register-staged pipeline, two staging register sets: while tile t is multiplied out of
//     LDS (2 stages), the global loads of tiles t+1 and t+2 are in flight; VGPR -> LDS after
//     the MFMA block, one barrier per K-tile.
//   * the MFMA computes D^T (weights as the A operand) so every lane ends up with 4
//     consecutive output channels of one pixel: 8/16-byte epilogue accesses for bias,
//     time-embedding row vector, residual and the store.
//   * tile shapes: 128x160 when N is a multiple of 160 (the SD-1.5 widths 320/640/1280 and
//     their multiples tile exactly), else 128x128; 128x32 for skinny N; 64x64 when there
//     are too few tiles to fill 256 CUs.
//   * tiles are enumerated so that the 8 XCDs each own a contiguous range (blocks b and
//     b+8 share an XCD): neighbouring tiles (same activation rows) hit the same L2.
//   * split-K (gridDim.y slices of the K range, fp32 partial slabs in a caller workspace +
//     one reduce/epilogue launch) for the deep levels where M is 1-4 K rows but K is 6-23 K.
#include <cstdlib>

#include "common.h"
#include "gemm_internal.h"

namespace {

template <typename T> struct Mma;
template <> struct Mma<h16_t> {
  __device__ static __forceinline__ void run(const u32x4& wf, const u32x4& xf, f32x4& acc) {
    acc = MFMA_16X16X32(wf, xf, acc);
  }
};
template <> struct Mma<float> {
  // one 16-byte chunk = 4 consecutive k per lane; lane group g = lane>>4 owns chunk
  // (4*kk + g), so MFMA step j pairs element j of every group: the k order is a fixed
  // permutation shared by both operands (exact fp32 fma chain per output).
  __device__ static __forceinline__ void run(const u32x4& wf, const u32x4& xf, f32x4& acc) {
    // NOTE: bit-cast the WHOLE vector; __builtin_bit_cast(float, vec.x) on an ext-vector
    // element lvalue silently reads element 0 (hipcc / ROCm 7.2).
    const f32x4 a = __builtin_bit_cast(f32x4, wf);
    const f32x4 b = __builtin_bit_cast(f32x4, xf);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc, 0, 0, 0);
  }
};

template <> struct Mma<f32x3_t> {
  // (bf16 by construction -- hi / lo halves of an fp32 value; the fp16 build refuses SASPA_F32X3 and never instantiates a launch of it)
  // per-chunk form (generic loader kernel, fp32 parity of odd shapes): the exact fp32 chain
  __device__ static __forceinline__ void run(const u32x4& wf, const u32x4& xf, f32x4& acc) { Mma<float>::run(wf, xf, acc); }
  // 8 fp32 values of one lane (its two 16-byte chunks of the K-tile) -> 8 bf16 "hi" + 8 bf16 "lo" (round to nearest)
  __device__ static __forceinline__ void split(const u32x4& f0, const u32x4& f1, u32x4& hi, u32x4& lo) {
    const f32x4 a = __builtin_bit_cast(f32x4, f0), b = __builtin_bit_cast(f32x4, f1);
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    uint32_t h[4], l[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t hp = pack2(x[2 * q], x[2 * q + 1]);
      h[q] = hp;
      l[q] = pack2(x[2 * q] - __builtin_bit_cast(float, hp << 16), x[2 * q + 1] - __builtin_bit_cast(float, hp & 0xffff0000u));
    }
    hi = u32x4{h[0], h[1], h[2], h[3]};
    lo = u32x4{l[0], l[1], l[2], l[3]};
  }
  __device__ static __forceinline__ void run3(const u32x4& wh, const u32x4& wl, const u32x4& xh, const u32x4& xl, f32x4& acc) {
    acc = MFMA_16X16X32(wl, xh, acc);
    acc = MFMA_16X16X32(wh, xl, acc);
    acc = MFMA_16X16X32(wh, xh, acc);
  }
};
template <typename T> struct is_x3 { static constexpr bool value = false; };
template <> struct is_x3<f32x3_t> { static constexpr bool value = true; };

// ---- shared epilogue of both kernel variants ------------------------------------------
// split-K: raw fp32 slab.  bf16: the tile goes through LDS so that global stores (and the
// residual read) are whole 16-byte chunks of contiguous output rows; GEGLU pairs the value /
// gate halves there.  fp32 parity mode / odd N: direct per-lane path.
// The caller guarantees every wave has finished reading the K-loop's LDS stages.
// PH: phase mode of the nearest-x2 conv (SaspaGemmParams.upsample = 2) -- a template parameter here and in the kernels, so that the
// instantiations every other launch runs are the code they were.
template <typename T, int WM, int WN, int NWM = 2, int NWN = 2, bool PH = false>
__device__ __forceinline__ void gemm_epilogue(const SaspaGemmParams& p, f32x4 (&acc)[WM][WN], u32x4* lds, const int cbm,
                                              const int cbn, const long long ooff) {
  constexpr int BM = 16 * WM * NWM, BN = 16 * WN * NWN, NT = 64 * NWM * NWN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / NWN, wn = wave % NWN;
  const int frow = lane & 15, fg = lane >> 4;
  const int hw = p.hout * p.wout;
  T* out = reinterpret_cast<T*>(p.out) + ooff;
  const T* res = p.residual ? reinterpret_cast<const T*>(p.residual) + ooff : nullptr;
  const bool geglu = p.act == SASPA_ACT_GEGLU;
  const bool staged = sizeof(T) == 2 && (p.N % 8) == 0 && (p.ldo % 8) == 0 && (!res || (p.ldr % 8) == 0) &&
                      (!geglu || (p.N % BN) == 0);
  // phase mode (lowered by saspa_gemm: blockIdx.z = phase (py, px), rows = low-res pixels): row (b, i, j) is pixel
  // (b, 2i + py, 2j + px) of the output
  const int phz = PH ? (int)blockIdx.z : 0;
  auto orow = [&](const int m) __attribute__((always_inline)) -> long long {
    if (!PH) return m;
    const int b = m / hw, rem = m - b * hw;
    const int i = rem / p.wout, j = rem - i * p.wout;
    return (long long)(b * 2 * p.hout + 2 * i + (phz >> 1)) * (2 * p.wout) + 2 * j + (phz & 1);
  };
    if (gridDim.y > 1) {
      // ---- split-K: raw fp32 partial slab, epilogue happens in the reduce launch ----
      // (phase mode: slabs are [slice][phase][row of the phase][N]; the reduce launch gathers them per output pixel)
      float* ws = p.workspace + (long long)(PH ? blockIdx.y * 4 + phz : blockIdx.y) * p.M * p.N;
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int m = cbm * BM + wm * (16 * WM) + i * 16 + frow;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          const int n = cbn * BN + wn * (16 * WN) + j * 16 + fg * 4;
          if (n >= p.N) continue;   // N % 4 == 0 is required with split-K
          *reinterpret_cast<float4*>(ws + (long long)m * p.N + n) =
              make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
      }
    } else if (staged) {
    constexpr int CP = BN + 8;                       // LDS row pitch in elements (16-byte pad)
    T* ct = reinterpret_cast<T*>(lds);
    // bias + time-embedding row of the wave's FIRST image, loaded once per column fragment (WN loads in
    // flight together instead of one dependent L2 round trip per accumulator fragment); rows of a later
    // image (tiles that straddle images) take the reload path
    const int m0 = cbm * BM + wm * (16 * WM);
    const int img0 = min(m0, p.M - 1) / hw;
    const int mnext = (img0 + 1) * hw;
    float4 add[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = cbn * BN + wn * (16 * WN) + j * 16 + fg * 4;
      add[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < p.N) {   // N % 8 == 0: a 4-vector never straddles N
        if (p.bias) add[j] = *reinterpret_cast<const float4*>(p.bias + n);
        if (p.rowvec) {
          const float4 r4 = *reinterpret_cast<const float4*>(p.rowvec + (long long)img0 * p.ldrv + n);
          add[j].x += r4.x; add[j].y += r4.y; add[j].z += r4.z; add[j].w += r4.w;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int mrow = wm * (16 * WM) + i * 16 + frow;
      const int m = cbm * BM + mrow;
      const bool other = p.rowvec && m >= mnext && m < p.M;
      const float* rvd = other ? p.rowvec + (long long)(m / hw) * p.ldrv : nullptr;
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const int ncol = wn * (16 * WN) + j * 16 + fg * 4;
        const int n = cbn * BN + ncol;
        float v[4] = {acc[i][j][0] + add[j].x, acc[i][j][1] + add[j].y, acc[i][j][2] + add[j].z, acc[i][j][3] + add[j].w};
        if (other && n < p.N) {
          const float4 a4 = *reinterpret_cast<const float4*>(rvd + n);
          const float4 c4 = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
          v[0] = acc[i][j][0] + (c4.x + a4.x); v[1] = acc[i][j][1] + (c4.y + a4.y);
          v[2] = acc[i][j][2] + (c4.z + a4.z); v[3] = acc[i][j][3] + (c4.w + a4.w);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= p.alpha;   // SiLU (if any) is applied in the read phase
        Elem<T>::store4(ct + mrow * CP + ncol, v);
      }
    }
    __syncthreads();
    if (!geglu) {
      constexpr int CPR = BN / 8;                    // 16-byte chunks per tile row
      for (int q = tid; q < BM * CPR; q += NT) {
        const int row = q / CPR, ch = q - row * CPR;
        const int m = cbm * BM + row, n = cbn * BN + ch * 8;
        if (m >= p.M || n >= p.N) continue;
        u32x4 c4 = *reinterpret_cast<const u32x4*>(ct + row * CP + ch * 8);
        if (res || p.act != SASPA_ACT_NONE) {
          float a[8];
          unpack8(__builtin_bit_cast(uint4, c4), a);
          if (p.act == SASPA_ACT_SILU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = a[e] * __builtin_amdgcn_rcpf(1.0f + __expf(-a[e]));
          } else if (p.act == SASPA_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = fmaxf(a[e], 0.0f);
          }
          if (res) {
            float b[8];
            Elem<h16_t>::load_chunk(reinterpret_cast<const h16_t*>(res) + (long long)m * p.ldr + n, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += b[e];
          }
          if (p.act == SASPA_ACT_ADD_RELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = fmaxf(a[e], 0.0f);
          }
          c4 = __builtin_bit_cast(u32x4, pack8(a));
          if (p.gn_stats) *reinterpret_cast<u32x4*>(ct + row * CP + ch * 8) = c4;   // the statistics read the STORED values
        }
        *reinterpret_cast<u32x4*>(out + orow(m) * p.ldo + n) = c4;
      }
      if constexpr (sizeof(T) == 2) if (p.gn_stats) {
        // GroupNorm statistics of this tile's row block (SaspaGemmParams.gn_stats): BM = 128 rows = one block
        static_assert(BM == 128 || BM == 256 || BM <= 64, "row blocks of the statistics are 128 rows");
        __syncthreads();
        const int nunits = BN / p.gn_unit;
        float* scratch = reinterpret_cast<float*>(ct + BM * CP);
#pragma unroll
        for (int hb = 0; hb < (BM + 127) / 128; ++hb) {
          const int r0 = hb * 128;
          const int nrows = min(128, min(BM, p.M - cbm * BM) - r0);
          if (nrows > 0) {
            // phase mode (whole 128-row blocks per low-res image, plan_gemm): image b's 4 * hw / 128 slots, phase-major
            const int r128 = (cbm * BM + r0) / 128, nlo = hw >> 7;
            const int rb = PH ? (r128 / nlo * 4 + phz) * nlo + r128 % nlo : r128;
            gn_tile_stats<NT>(reinterpret_cast<const h16_t*>(ct) + r0 * CP, CP, nrows, nunits, p.gn_unit, scratch,
                              p.gn_stats + ((long long)rb * (p.N / p.gn_unit) + (cbn * BN) / p.gn_unit) * 2);
          }
          if (hb + 1 < (BM + 127) / 128) __syncthreads();
        }
      }
    } else {
      // tile columns [0, BN/2) are values, [BN/2, BN) the matching gates (weights packed so)
      constexpr int HB = BN / 2, CPR = HB / 8;
      for (int q = tid; q < BM * CPR; q += NT) {
        const int row = q / CPR, ch = q - row * CPR;
        const int m = cbm * BM + row, f = cbn * HB + ch * 8;
        if (m >= p.M) continue;
        float a[8], g[8];
        unpack8(*reinterpret_cast<const uint4*>(ct + row * CP + ch * 8), a);
        unpack8(*reinterpret_cast<const uint4*>(ct + row * CP + HB + ch * 8), g);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = fast_gelu_mul(a[e], g[e]);
        *reinterpret_cast<uint4*>(out + (long long)m * p.ldo + f) = pack8(a);
      }
    }
    } else {
  // generic path (fp32 parity mode, odd N): lane holds out[m][n..n+3], m = tile row (lane&15), n = 4*(lane>>4)
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int m = cbm * BM + wm * (16 * WM) + i * 16 + frow;
    if (m >= p.M) continue;
    const float* rv = nullptr;
    if (p.rowvec) rv = p.rowvec + (long long)(m / hw) * p.ldrv;
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = cbn * BN + wn * (16 * WN) + j * 16 + fg * 4;
      if (n >= p.N) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (n + 3 < p.N) {
        if (p.bias) {
          const float4 b4 = *reinterpret_cast<const float4*>(p.bias + n);
          v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
        }
        if (rv) {
          const float4 r4 = *reinterpret_cast<const float4*>(rv + n);
          v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = act_pre(p.act, v[r] * p.alpha);
        if (res) {
          float rr[4];
          Elem<T>::load4(res + (long long)m * p.ldr + n, rr);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += rr[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = act_post(p.act, v[r]);
        Elem<T>::store4(out + orow(m) * p.ldo + n, v);
      } else {
        for (int r = 0; r < 4 && n + r < p.N; ++r) {
          float x = v[r];
          if (p.bias) x += p.bias[n + r];
          if (rv) x += rv[n + r];
          x = act_pre(p.act, x * p.alpha);
          if (res) x += Elem<T>::load1(res + (long long)m * p.ldr + n + r);
          Elem<T>::store1(out + orow(m) * p.ldo + n + r, act_post(p.act, x));
        }
      }
    }
  }
    }
}

// PW: pointwise (1x1, stride 1, no pad, no upsample): the A row of output pixel m is input
// pixel m -- no window arithmetic at all.
// Persistent over tiles: workgroup b walks tiles s(b), s(b)+G, s(b)+2G ... (s = XCD-aware
// remap of the block id, G = gridDim.x).  The global loads of the NEXT tile's first two
// K-tiles are issued before the current tile's epilogue, so workgroups stream continuously
// instead of loading / storing in lock-step bursts (short-K layers are memory-bound).
template <typename T, int WM, int WN, bool PW, bool PH = false>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const SaspaGemmParams p, const int ntiles, const int npart8) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int EPC = Elem<T>::EPC;
  constexpr int BK = 8 * EPC;
  constexpr int A_CH = BM * 8 / 256, B_CH = BN * 8 / 256;
  static_assert(A_CH >= 1 && B_CH >= 1, "tile too small for 256 threads");
  constexpr int STAGE = (BM + BN) * 8;  // u32x4 per stage
  __shared__ u32x4 lds[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // ---- XCD-aware order (bijective for any grid size): blocks b and b+8 share an XCD and
  //      get neighbouring tiles (same activation rows -> same L2) ----
  const int nbn = (p.N + BN - 1) / BN;
  const int G = gridDim.x;
  int tile;
  {
    const int L = blockIdx.x;
    const int qd = G >> 3, rr = G & 7, xcd = L & 7, idx = L >> 3;
    tile = (xcd < rr ? xcd * (qd + 1) : rr * (qd + 1) + (xcd - rr) * qd) + idx;
  }
  const int z = blockIdx.z;
  const int i1 = z / p.nb2, i2 = z - i1 * p.nb2;

  const T* a0 = reinterpret_cast<const T*>(p.a0) + (i1 * p.sa1 + i2 * p.sa2);
  const T* a1 = reinterpret_cast<const T*>(p.a1);
  const T* w = reinterpret_cast<const T*>(p.w) + (i1 * p.sw1 + i2 * p.sw2);
  const long long ooff = i1 * p.so1 + i2 * p.so2;

  // ---- K range of this block (split-K over gridDim.y) ----
  const int nk_all = (p.K + BK - 1) / BK;
  const int kt_per = (nk_all + gridDim.y - 1) / gridDim.y;
  const int kt0 = blockIdx.y * kt_per;
  const int nk = max(0, min(nk_all, kt0 + kt_per) - kt0);

  // ---- loader state (re-initialised per tile by setup_tile) ----
  // FAST mode (every SD-1.5 layer): a K-tile lies inside ONE tap of ONE source, so the tap,
  // the source and the channel offset are wave-uniform scalars; each lane keeps, per A row,
  // the pixel index of the window centre and a bitmask of the taps that fall inside the
  // image, and per B row a constant byte offset.  A K-tile of loads then costs ~3 VALU
  // instructions per A row and none per B row.  GENERIC mode (channel counts below one
  // K-tile, nearest-x2 upsample, ragged concat) derives tap / source per lane.
  constexpr int SZ = (int)sizeof(T);
  const int kc = tid & 7;
  const int r0 = tid >> 3;  // rows r0 + 32*i
  const int hw = p.hout * p.wout;
  const int ctot = p.c0 + p.c1;
  const int up = PH ? 0 : p.upsample;              // nearest-x2 input (phase mode reads the stored low-res input)
  const int hv = up ? 2 * p.hin : p.hin;
  const int wv = up ? 2 * p.win : p.win;
  const bool fast = (ctot % BK) == 0 && (p.c1 == 0 || (p.c0 % BK) == 0) && !up;
  // phase mode (PH: upsample = 2, blockIdx.z = phase (py, px)): a 2x2 window with pad (1 - py, 1 - px) over the low-res grid
  const int pady = PH ? p.pad - (z >> 1) : p.pad, padx = PH ? p.pad - (z & 1) : p.pad;
  const rsrc_t rs0 = make_rsrc(a0);
  const rsrc_t rs1 = make_rsrc(p.c1 > 0 ? (const void*)a1 : (const void*)a0);
  const rsrc_t rsw = make_rsrc(w);
  int bm = 0, bn = 0;
  int row_a[A_CH], row_b[A_CH], row_c[A_CH];  // FAST: (centre pixel, tap mask, -); GENERIC: (iy0, ix0, pix0) / PW (m,-,-)
  unsigned offb[B_CH];                        // byte offset of (weight row, chunk kc) or kInvalid
  int k = 0, c = 0, dy = 0, dx = 0;           // GENERIC: per-lane k-state
  int ku = 0, cu = 0, dyu = 0, dxu = 0;       // FAST: wave-uniform k-state (tile start)

  auto setup_tile = [&](int t) __attribute__((always_inline)) {
    if (npart8 > 0) {
      // N-partitioned order (weight-heavy problems, host decides): the XCD of this block (L & 7 -> the x-th eighth of every
      // round of G tiles) owns the x-th eighth of the N tiles for ALL row blocks, so its slice of the weights stays in
      // its L2 while the activations stream through once per XCD
      const int G8 = G >> 3;
      const int k = t / G, r = t - k * G;
      const int x = r / G8;
      const int q = k * G8 + (r - x * G8);
      bm = q / npart8;
      bn = x * npart8 + (q - bm * npart8);
    } else {
      bm = t / nbn;
      bn = t - bm * nbn;
    }
    if (PW) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int m = bm * BM + r0 + 32 * i;
        row_a[i] = (m < p.M) ? m : -1;
        row_b[i] = (m < p.M) ? 1 : 0;
        row_c[i] = 0;
      }
    } else {
      // first row by division, the following rows (+32 each) by carry propagation
      int m = bm * BM + r0;
      int b = m / hw;
      int rem = m - b * hw;
      int oy = rem / p.wout;
      int ox = rem - oy * p.wout;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int iy0 = oy * p.stride - pady, ix0 = ox * p.stride - padx;
        if (fast) {
          // centre pixel of the window and the validity bit of every tap
          row_a[i] = b * p.hin * p.win + (oy * p.stride) * p.win + ox * p.stride;
          int mask = 0;
          if (m < p.M) {
            for (int ty = 0; ty < p.kh; ++ty)
              for (int tx = 0; tx < p.kw; ++tx)
                if ((unsigned)(iy0 + ty) < (unsigned)hv && (unsigned)(ix0 + tx) < (unsigned)wv) mask |= 1 << (ty * p.kw + tx);
          }
          row_b[i] = mask;
          row_c[i] = 0;
        } else if (m < p.M) {
          row_a[i] = iy0;
          row_b[i] = ix0;
          row_c[i] = b * p.hin * p.win;
        } else {
          row_a[i] = row_b[i] = -(1 << 28);
          row_c[i] = 0;
        }
        m += 32;
        ox += 32;
        while (ox >= p.wout) { ox -= p.wout; ++oy; }
        while (oy >= p.hout) { oy -= p.hout; ++b; }
      }
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int n = bn * BN + r0 + 32 * i;
      offb[i] = (n < p.N) ? (unsigned)(n * p.ldw * SZ + kc * 16) : kInvalid;
    }
    k = kt0 * BK + kc * EPC;
    const int tap = k / ctot;
    c = k - tap * ctot;
    dy = tap / p.kw;
    dx = tap - dy * p.kw;
    ku = kt0 * BK;
    const int tapu = ku / ctot;
    cu = ku - tapu * ctot;
    dyu = tapu / p.kw;
    dxu = tapu - dyu * p.kw;
  };

  // two register staging sets: while tile t is being multiplied out of LDS, tiles t+1 and
  // t+2 are in flight from global memory (two K-tiles of loads outstanding per workgroup)
  u32x4 ra0[A_CH], rb0[B_CH], ra1[A_CH], rb1[B_CH];

  auto load_tile = [&](u32x4 (&ra)[A_CH], u32x4 (&rb)[B_CH]) __attribute__((always_inline)) {
    if (fast) {
      // ---- wave-uniform tap / source / channel offset ----
      const bool s0 = cu < p.c0;
      const rsrc_t rs = s0 ? rs0 : rs1;
      const int ldsz = (s0 ? p.lda0 : p.lda1) * SZ;
      const unsigned soff = (unsigned)((s0 ? cu : cu - p.c0) * SZ);
      const int tapbit = dyu * p.kw + dxu;
      const int pixoff = PW ? 0 : (dyu - pady) * p.win + (dxu - padx);
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const unsigned off = (unsigned)((row_a[i] + pixoff) * ldsz + kc * 16);
        const bool ok = PW ? (row_b[i] != 0) : (((row_b[i] >> tapbit) & 1) != 0);
        ra[i] = buf_load(rs, ok ? off : kInvalid, soff);
      }
      const unsigned soffw = (unsigned)(ku * SZ);
#pragma unroll
      for (int i = 0; i < B_CH; ++i) rb[i] = buf_load(rsw, offb[i], soffw);
      ku += BK;
      cu += BK;
      if (cu >= ctot) {
        cu -= ctot;
        if (++dxu == p.kw) { dxu = 0; ++dyu; }
      }
    } else {
      // ---- per-lane tap / source (small channel counts, upsample, ragged concat) ----
      const bool kvalid = k < p.K;
      const bool s0 = c < p.c0;
      const int ld = s0 ? p.lda0 : p.lda1;
      const int cc = s0 ? c : c - p.c0;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        unsigned off;
        bool inb;
        if (PW) {
          inb = kvalid && row_a[i] >= 0;
          off = (unsigned)((row_a[i] * ld + cc) * SZ);
        } else {
          int iy = row_a[i] + dy, ix = row_b[i] + dx;
          inb = kvalid && (unsigned)iy < (unsigned)hv && (unsigned)ix < (unsigned)wv;
          if (up) { iy >>= 1; ix >>= 1; }
          off = (unsigned)(((row_c[i] + iy * p.win + ix) * ld + cc) * SZ);
        }
        u32x4 v = buf_load(rs0, (inb && s0) ? off : kInvalid, 0u);
        if (p.c1 > 0) v |= buf_load(rs1, (inb && !s0) ? off : kInvalid, 0u);
        ra[i] = v;
      }
#pragma unroll
      for (int i = 0; i < B_CH; ++i) rb[i] = buf_load(rsw, kvalid ? offb[i] + (unsigned)((k - kc * EPC) * SZ) : kInvalid, 0u);
      k += BK;
      c += BK;
      while (c >= ctot) {
        c -= ctot;
        if (++dx == p.kw) { dx = 0; ++dy; }
      }
    }
  };
  auto store_tile = [&](int stage, const u32x4 (&ra)[A_CH], const u32x4 (&rb)[B_CH]) __attribute__((always_inline)) {
    u32x4* la = lds + stage * STAGE;
    u32x4* lb = la + BM * 8;
    const int sw = kc ^ (r0 & 7);
#pragma unroll
    for (int i = 0; i < A_CH; ++i) la[(r0 + 32 * i) * 8 + sw] = ra[i];
#pragma unroll
    for (int i = 0; i < B_CH; ++i) lb[(r0 + 32 * i) * 8 + sw] = rb[i];
  };

  f32x4 acc[WM][WN];
  const int frow = lane & 15, fg = lane >> 4;
  auto compute = [&](int stage) __attribute__((always_inline)) {
    const u32x4* la = lds + stage * STAGE;
    const u32x4* lb = la + BM * 8;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + fg;
      u32x4 xa[WM], wb[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int row = wm * (16 * WM) + i * 16 + frow;
        xa[i] = la[row * 8 + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const int row = wn * (16 * WN) + j * 16 + frow;
        wb[j] = lb[row * 8 + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) Mma<T>::run(wb[j], xa[i], acc[i][j]);
    }
  };

  setup_tile(tile);
  if (nk > 0) load_tile(ra0, rb0);
  if (nk > 1) load_tile(ra1, rb1);
  for (;;) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nk > 0) store_tile(0, ra0, rb0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
      // even tile kt: LDS stage 0; set 0 is free -> prefetch tile kt+2; set 1 (tile kt+1) -> stage 1
      if (kt + 2 < nk) load_tile(ra0, rb0);
      compute(0);
      if (kt + 1 < nk) store_tile(1, ra1, rb1);
      __syncthreads();
      if (kt + 1 >= nk) break;
      // odd tile kt+1: LDS stage 1; set 1 is free -> prefetch tile kt+3; set 0 (tile kt+2) -> stage 0
      if (kt + 3 < nk) load_tile(ra1, rb1);
      compute(1);
      if (kt + 2 < nk) store_tile(0, ra0, rb0);
      __syncthreads();
    }

    // ---- next tile: its first two K-tiles go in flight now, under this tile's epilogue ----
    const int cbm = bm, cbn = bn;
    const int next = tile + G;
    const bool has_next = next < ntiles;
    if (has_next) {
      setup_tile(next);
      if (nk > 0) load_tile(ra0, rb0);
      if (nk > 1) load_tile(ra1, rb1);
    }

    gemm_epilogue<T, WM, WN, 2, 2, PH>(p, acc, lds, cbm, cbn, ooff);
    if (!has_next) break;
    tile = next;
    __syncthreads();   // LDS reads of the staged epilogue are done before the next tile's first store
  }
}

// ---- LDS-DMA variant (FAST layers: a K-tile lies inside one tap of one source) -------------
// Operand tiles go global -> LDS directly (buffer_load ... lds): no staging VGPRs and no
// ds_write pass (register staging costs ~9 KB of ds_write_b128 per wave per K-tile at only
// ~79 B/clk/CU, which alone exceeds the MFMA time of the tile).  The LDS image is lane-linear
// per wave instruction (64 lanes x 16 B = 8 rows x 128 B), so the XOR swizzle is applied on
// the SOURCE side: the lane that lands in slot s of row r fetches logical chunk s ^ (r & 7);
// the fragment reads apply the same XOR.  Out-of-range lanes (M / N edge, halo) use an offset
// beyond num_records and land as zeros.  Two LDS stages: the DMA of tile t+1 is in flight
// during the MFMAs of tile t; one barrier per K-tile.

// UP (nearest-x2 input) is a template parameter: as a run-time flag it put one scalar branch in front of every A-piece
// DMA of every 3x3 conv's K-tile (4 per K-tile on the 128-row tile), and this issue path does not forgive branches.
template <typename T, int WM, int WN, int NWM, int NWN, bool PW, int NSTAGE, bool UP = false, bool PH = false>
__global__ __launch_bounds__(64 * NWM * NWN, (NWM * NWN == 4 && NSTAGE > 2) ? 1 : 2) void gemm_dma_kernel(const SaspaGemmParams p,
                                                                                                      const int ntiles_abl, const int npart8) {
  // diagnostic ablation (tools/gemm_ablate.py only; 0 in production): bits 28..30 of the tile count
  const int ntiles = ntiles_abl & 0x0fffffff;
#ifdef SASPA_GEMM_ABLATION
  const int abl = (ntiles_abl >> 28) & 15;     // 1: no MFMA  2: no LDS reads / MFMA  4: no DMA  8: MFMA on stale registers (no LDS reads)
#else
  constexpr int abl = 0;                       // production build: the ablation branches fold away
#endif
  constexpr int BM = 16 * WM * NWM, BN = 16 * WN * NWN, NT = 64 * NWM * NWN;
  constexpr int RPI = NT / 8;                         // tile rows covered by one DMA instruction of the whole workgroup
  constexpr int EPC = Elem<T>::EPC;
  constexpr int BK = 8 * EPC;
  constexpr int A_CH = (BM + RPI - 1) / RPI, B_CH = (BN + RPI - 1) / RPI;
  static_assert(BM % RPI == 0 || NSTAGE == 2, "counted vmcnt: A rows must fill whole DMA instructions");
  // B rows may end inside the last DMA instruction: waves whose 8-row slice lies beyond BN skip it,
  // so the number of DMA instructions per K-tile is wave-dependent (G_LO for the low waves)
  constexpr int B_FULL = BN / RPI;                    // B instructions every wave issues
  constexpr bool B_RAGGED = (BN % RPI) != 0;
  constexpr int STAGE = (BM + BN) * 8;  // u32x4 per stage
  constexpr int SZ = (int)sizeof(T);
  __shared__ u32x4 lds[NSTAGE * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;

  const int nbn = (p.N + BN - 1) / BN;
  const int G = gridDim.x;
  int tile;
  {
    const int L = blockIdx.x;
    const int qd = G >> 3, rr = G & 7, xcd = L & 7, idx = L >> 3;
    tile = (xcd < rr ? xcd * (qd + 1) : rr * (qd + 1) + (xcd - rr) * qd) + idx;
  }
  const int z = blockIdx.z;
  const int i1 = z / p.nb2, i2 = z - i1 * p.nb2;
  const T* a0 = reinterpret_cast<const T*>(p.a0) + (i1 * p.sa1 + i2 * p.sa2);
  const T* a1 = reinterpret_cast<const T*>(p.a1);
  const T* w = reinterpret_cast<const T*>(p.w) + (i1 * p.sw1 + i2 * p.sw2);
  const long long ooff = i1 * p.so1 + i2 * p.so2;

  const int nk_all = (p.K + BK - 1) / BK;
  const int kt_per = (nk_all + gridDim.y - 1) / gridDim.y;
  const int kt0 = blockIdx.y * kt_per;
  const int nk = max(0, min(nk_all, kt0 + kt_per) - kt0);

  const int r0 = tid >> 3;                        // tile row r0 + RPI*i lands in LDS row r0 + RPI*i
  const int kcs = (tid & 7) ^ (r0 & 7);           // logical 16-byte chunk fetched by this lane
  const int hw = p.hout * p.wout;
  const int ctot = p.c0 + p.c1;
  const int chunk_major = p.korder == SASPA_KORDER_CHUNK ? 1 : 0;   // wave-uniform
  const rsrc_t rs0 = make_rsrc(a0);
  const rsrc_t rs1 = make_rsrc(p.c1 > 0 ? (const void*)a1 : (const void*)a0);
  const rsrc_t rsw = make_rsrc(w);
  int bm = 0, bn = 0;
  int pix[A_CH], msk[A_CH], upc[A_CH];
  // !UP: byte offset of (pixel of row i, chunk kcs) in each source, fixed per tile -- the per-K-tile address of an A piece
  // is then one add of the (wave-uniform) tap offset instead of a 64-bit multiply-add per piece and K-tile
  unsigned offa0[A_CH], offa1[A_CH];
  const int hv = UP ? 2 * p.hin : p.hin, wv = UP ? 2 * p.win : p.win;
  // phase mode (PH: upsample = 2, blockIdx.z = phase (py, px)): a 2x2 window with pad (1 - py, 1 - px) over the low-res grid
  const int pady = PH ? p.pad - (z >> 1) : p.pad, padx = PH ? p.pad - (z & 1) : p.pad;
  unsigned offb[B_CH];
  int ku = 0, cu = 0, dyu = 0, dxu = 0;

  auto setup_tile = [&](int t) __attribute__((always_inline)) {
    if (npart8 > 0) {
      // N-partitioned order (weight-heavy problems, host decides): the XCD of this block (L & 7 -> the x-th eighth of every
      // round of G tiles) owns the x-th eighth of the N tiles for ALL row blocks, so its slice of the weights stays in
      // its L2 while the activations stream through once per XCD
      const int G8 = G >> 3;
      const int k = t / G, r = t - k * G;
      const int x = r / G8;
      const int q = k * G8 + (r - x * G8);
      bm = q / npart8;
      bn = x * npart8 + (q - bm * npart8);
    } else {
      bm = t / nbn;
      bn = t - bm * nbn;
    }
    if (PW) {
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int m = bm * BM + r0 + RPI * i;
        pix[i] = m;
        msk[i] = (m < p.M) ? 1 : 0;
        upc[i] = 0;
        offa0[i] = (unsigned)(m * (p.lda0 * SZ) + kcs * 16);
        offa1[i] = (unsigned)(m * (p.lda1 * SZ) + kcs * 16);
      }
    } else {
      int m = bm * BM + r0;
      int b = m / hw;
      int rem = m - b * hw;
      int oy = rem / p.wout;
      int ox = rem - oy * p.wout;
#pragma unroll
      for (int i = 0; i < A_CH; ++i) {
        const int iy0 = oy * p.stride - pady, ix0 = ox * p.stride - padx;
        if (UP) {
          // nearest x2: the window walks the virtual 2H x 2W grid; keep its top-left corner
          // (packed y | x) and resolve the source pixel ((iy0+dy)>>1, (ix0+dx)>>1) per tap
          pix[i] = b * p.hin * p.win;
          upc[i] = ((iy0 + 1) << 16) | (ix0 + 1);     // +1 keeps both halves non-negative (pad <= 1)
        } else {
          pix[i] = b * p.hin * p.win + (oy * p.stride) * p.win + ox * p.stride;
          offa0[i] = (unsigned)(pix[i] * (p.lda0 * SZ) + kcs * 16);
          offa1[i] = (unsigned)(pix[i] * (p.lda1 * SZ) + kcs * 16);
        }
        int mask = 0;
        if (m < p.M) {
          for (int ty = 0; ty < p.kh; ++ty)
            for (int tx = 0; tx < p.kw; ++tx)
              if ((unsigned)(iy0 + ty) < (unsigned)hv && (unsigned)(ix0 + tx) < (unsigned)wv) mask |= 1 << (ty * p.kw + tx);
        }
        msk[i] = mask;
        m += RPI;
        ox += RPI;
        while (ox >= p.wout) { ox -= p.wout; ++oy; }
        while (oy >= p.hout) { oy -= p.hout; ++b; }
      }
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int n = bn * BN + r0 + RPI * i;
      offb[i] = (n < p.N && r0 + RPI * i < BN) ? (unsigned)(n * p.ldw * SZ + kcs * 16) : kInvalid;
    }
    ku = kt0 * BK;
    if (chunk_major) {
      // chunk-major K: K-tile kt = (channel chunk kt / T, tap kt % T)
      const int ntap = p.kh * p.kw;
      const int chunk = kt0 / ntap, tap = kt0 - chunk * ntap;
      cu = chunk * BK;
      dyu = tap / p.kw;
      dxu = tap - dyu * p.kw;
    } else {
      const int tapu = ku / ctot;
      cu = ku - tapu * ctot;
      dyu = tapu / p.kw;
      dxu = tapu - dyu * p.kw;
    }
  };

  auto dma_tile = [&](int stage) __attribute__((always_inline)) {
    if (abl & 4) return;
    const bool s0 = cu < p.c0;
    const rsrc_t rs = s0 ? rs0 : rs1;
    const int ldsz = (s0 ? p.lda0 : p.lda1) * SZ;
    const int soff = (s0 ? cu : cu - p.c0) * SZ;
    const int tapbit = dyu * p.kw + dxu;
    const int pixoff = PW ? 0 : (dyu - pady) * p.win + (dxu - padx);
    const unsigned tapoff = (unsigned)(pixoff * ldsz);
    u32x4* la = lds + stage * STAGE;
    u32x4* lb = la + BM * 8;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      unsigned off;
      if (!PW && UP) {
        const int iy = ((upc[i] >> 16) - 1 + dyu) >> 1, ix = ((upc[i] & 0xffff) - 1 + dxu) >> 1;
        off = (unsigned)((pix[i] + iy * p.win + ix) * ldsz + kcs * 16);
      } else {
        off = (s0 ? offa0[i] : offa1[i]) + tapoff;      // == (pix + pixoff) * ldsz + kcs * 16 mod 2^32
      }
      const bool ok = PW ? (msk[i] != 0) : (((msk[i] >> tapbit) & 1) != 0);
      if (BM % RPI == 0 || RPI * i + 8 * wave < BM)   // compile-time true for whole groups: no branch around the DMA
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(la + (RPI * i + 8 * wave) * 8), 16, (int)(ok ? off : kInvalid),
                                                 soff, 0, 0);
    }
    const int soffw = ku * SZ;
#pragma unroll
    for (int i = 0; i < B_CH; ++i)
      if (RPI * (i + 1) <= BN || RPI * i + 8 * wave < BN)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void_t*)(lb + (RPI * i + 8 * wave) * 8), 16, (int)offb[i], soffw, 0, 0);
    ku += BK;
    // branch-free mixed-radix step (a scalar branch in this path costs the DMA kernels ~25 %, measured): tap-major
    // counts (c, x, y) with the channel offset fastest, chunk-major (x, y, c) with the tap fastest
    const int cu_t = cu + BK;
    const int wc = (cu_t >= ctot) ? 1 : 0;                        // tap-major: channel wrap carries into x
    const int dx1 = dxu + (chunk_major ? 1 : wc);
    const int wx = (dx1 == p.kw) ? 1 : 0;
    const int dy1 = dyu + wx;
    const int wy = (chunk_major && dy1 == p.kh) ? 1 : 0;          // chunk-major: tap wrap carries into the chunk
    cu = chunk_major ? cu + (wy ? BK : 0) : (wc ? cu_t - ctot : cu_t);
    dxu = wx ? 0 : dx1;
    dyu = wy ? 0 : dy1;
  };

  f32x4 acc[WM][WN];
  const int frow = lane & 15, fg = lane >> 4;
  auto compute = [&](int stage) __attribute__((always_inline)) {
    if (abl & 2) return;
    const u32x4* la = lds + stage * STAGE;
    const u32x4* lb = la + BM * 8;
    if constexpr (is_x3<T>::value) {
      // SASPA_F32X3: the lane's two chunks (fg, 4 + fg) are its 8 k values of ONE 16x16x32 bf16 MFMA step -- the same
      // k assignment for both operands, so any fixed assignment is a valid permutation of the sum
      u32x4 xh[WM], xl[WM];
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int row = wm * (16 * WM) + i * 16 + frow;
        Mma<T>::split(la[row * 8 + (fg ^ (row & 7))], la[row * 8 + ((4 + fg) ^ (row & 7))], xh[i], xl[i]);
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const int row = wn * (16 * WN) + j * 16 + frow;
        u32x4 wh, wl;
        if (p.w_split) {       // ABI 20: the weights arrive as [hi | lo] per K-tile, chunk fg of either half = this lane's 8 k values
          wh = lb[row * 8 + (fg ^ (row & 7))];
          wl = lb[row * 8 + ((4 + fg) ^ (row & 7))];
        } else {
          Mma<T>::split(lb[row * 8 + (fg ^ (row & 7))], lb[row * 8 + ((4 + fg) ^ (row & 7))], wh, wl);
        }
#pragma unroll
        for (int i = 0; i < WM; ++i) Mma<T>::run3(wh, wl, xh[i], xl[i], acc[i][j]);
      }
      return;
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chunk = kk * 4 + fg;
      u32x4 xa[WM], wb[WN];
      if (abl & 8) {
#pragma unroll
        for (int i = 0; i < WM; ++i) xa[i] = u32x4{(unsigned)chunk, (unsigned)i, kHalfOnes2, kHalfOnes2};
#pragma unroll
        for (int j = 0; j < WN; ++j) wb[j] = u32x4{(unsigned)j, (unsigned)stage, kHalfOnes2, kHalfOnes2};
      } else {
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int row = wm * (16 * WM) + i * 16 + frow;
        xa[i] = la[row * 8 + (chunk ^ (row & 7))];
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const int row = wn * (16 * WN) + j * 16 + frow;
        wb[j] = lb[row * 8 + (chunk ^ (row & 7))];
      }
      }
      if (abl & 1) {
        // keep the fragment reads alive without issuing MFMAs
#pragma unroll
        for (int i = 0; i < WM; ++i) asm volatile("" ::"v"(xa[i]));
#pragma unroll
        for (int j = 0; j < WN; ++j) asm volatile("" ::"v"(wb[j]));
        continue;
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) Mma<T>::run(wb[j], xa[i], acc[i][j]);
    }
  };

  setup_tile(tile);
  for (;;) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // NSTAGE-deep ring: tiles kt+1 .. kt+NSTAGE-1 are in flight while tile kt is multiplied.
    // Counted vmcnt + raw s_barrier (a __syncthreads() would drain every DMA).
#pragma unroll
    for (int st = 0; st < NSTAGE - 1; ++st)
      if (st < nk) dma_tile(st);
    for (int kt = 0; kt < nk; ++kt) {
      // tile kt has landed once at most (NSTAGE-2) younger groups are outstanding
      if (NSTAGE > 2 && kt + NSTAGE - 2 < nk) {
        if (B_RAGGED && RPI * B_FULL + 8 * wave < BN) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * (A_CH + B_FULL + 1)) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * (A_CH + B_FULL)) : "memory");
        }
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();                    // everyone's share landed; stage of tile kt-1 is free
      asm volatile("" ::: "memory");
      // (issuing the tail's pieces unconditionally with out-of-range offsets instead of this branch: measured 1.2 % slower)
      if (kt + NSTAGE - 1 < nk) dma_tile((kt + NSTAGE - 1) % NSTAGE);
      // the DMA must be ISSUED before the MFMA block so that it flies under it: without this fence
      // hipcc's scheduler sinks all but one buffer_load..lds below the MFMAs (measured: DMA time
      // and compute time then add up instead of overlapping)
      __builtin_amdgcn_sched_barrier(0);
      compute(kt % NSTAGE);
    }
    __syncthreads();   // every wave is done with the K-loop's LDS stages before the epilogue reuses them
    const int cbm = bm, cbn = bn;
    const int next = tile + G;
    const bool has_next = next < ntiles;
    if (has_next) setup_tile(next);
    gemm_epilogue<T, WM, WN, NWM, NWN, PH>(p, acc, lds, cbm, cbn, ooff);
    if (!has_next) break;
    tile = next;
    __syncthreads();   // staged epilogue reads are done before the next tile's first DMA
  }
}

// Phase mode (upsample = 2; p is the caller's view: M = batch * hout * wout output pixels): the slab row that holds output pixel m
// = (b, y, x) -- phase (y & 1, x & 1), low-res pixel (b, y >> 1, x >> 1); slabs are [slice][phase][M / 4][N].  Both reduce kernels
// walk the OUTPUT rows, so the GroupNorm statistics keep their blocks of 128 consecutive output rows whatever the image size.
template <bool PH> __device__ __forceinline__ long long reduce_src_row(const SaspaGemmParams& p, const int m) {
  if (!PH) return m;
  const int hw = p.hout * p.wout;
  const int b = m / hw, rem = m - b * hw;
  const int y = rem / p.wout, x = rem - y * p.wout;
  return (long long)((y & 1) * 2 + (x & 1)) * (p.M >> 2) + (long long)(b * p.hin + (y >> 1)) * p.win + (x >> 1);
}

// split-K reduce + epilogue: out = act(alpha*(sum_s ws[s] + bias + rowvec)) + residual
template <typename T, bool PH = false>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const SaspaGemmParams p, int ksplit) {
  const int n4 = p.N >> 2;
  const long long total = (long long)p.M * n4;
  const long long slab = (long long)p.M * p.N;
  const int hw = p.hout * p.wout;
  T* out = reinterpret_cast<T*>(p.out);
  const T* res = reinterpret_cast<const T*>(p.residual);
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const int m = (int)(it / n4);
    const int n = (int)(it - (long long)m * n4) * 4;
    const long long ms = reduce_src_row<PH>(p, m);
    float4 a = *reinterpret_cast<const float4*>(p.workspace + ms * p.N + n);
    for (int s = 1; s < ksplit; ++s) {
      const float4 b = *reinterpret_cast<const float4*>(p.workspace + s * slab + ms * p.N + n);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float v[4] = {a.x, a.y, a.z, a.w};
    if (p.bias) {
      const float4 b4 = *reinterpret_cast<const float4*>(p.bias + n);
      v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
    }
    if (p.rowvec) {
      const float4 r4 = *reinterpret_cast<const float4*>(p.rowvec + (long long)(m / hw) * p.ldrv + n);
      v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act_pre(p.act, v[r] * p.alpha);
    if (res) {
      float rr[4];
      Elem<T>::load4(res + (long long)m * p.ldr + n, rr);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += rr[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act_post(p.act, v[r]);
    Elem<T>::store4(out + (long long)m * p.ldo + n, v);
  }
}

// split-K reduce + epilogue + GroupNorm statistics (SaspaGemmParams.gn_stats): one workgroup per (128-row block, 80-column
// slab) -- 512 - 1024 workgroups on the 16x16 / 32x32 levels, two per CU; four rows per trip (4 x ksplit 16-byte loads in
// flight per lane: the pass is bandwidth bound, the first version with one row per trip ran at half the plain reduce's rate);
// the finished bf16 slab is staged in LDS like a GEMM tile and gn_tile_stats reads it.  bf16 only.
template <bool PH = false> __global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const SaspaGemmParams p, int ksplit) {
  constexpr int BR = 128, BC = 80, CP = BC + 8, C4 = BC / 4, U = 4;
  __shared__ __attribute__((aligned(16))) h16_t ct[BR * CP + 4 * 256];
  const int tid = threadIdx.x;
  const int rb = blockIdx.x, cs = blockIdx.y;
  const long long slab = (long long)p.M * p.N;
  const int hw = p.hout * p.wout;
  h16_t* out = reinterpret_cast<h16_t*>(p.out);
  const h16_t* res = reinterpret_cast<const h16_t*>(p.residual);
  const int nrows = min(BR, p.M - rb * BR);
  const int total = nrows * C4;
  for (int q0 = tid; q0 < total; q0 += U * 256) {
    float4 a[U];
    int row[U], c4[U];
    long long ms[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = min(q0 + u * 256, total - 1);           // clamped duplicates are recomputed, never stored twice (below)
      row[u] = q / C4;
      c4[u] = q - row[u] * C4;
      ms[u] = reduce_src_row<PH>(p, rb * BR + row[u]);
      a[u] = *reinterpret_cast<const float4*>(p.workspace + ms[u] * p.N + cs * BC + c4[u] * 4);
    }
    for (int s = 1; s < ksplit; ++s) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 b = *reinterpret_cast<const float4*>(p.workspace + s * slab + ms[u] * p.N + cs * BC + c4[u] * 4);
        a[u].x += b.x; a[u].y += b.y; a[u].z += b.z; a[u].w += b.w;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q0 + u * 256 >= total) continue;
      const int m = rb * BR + row[u], n = cs * BC + c4[u] * 4;
      float v[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
      if (p.bias) {
        const float4 b4 = *reinterpret_cast<const float4*>(p.bias + n);
        v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
      }
      if (p.rowvec) {
        const float4 r4 = *reinterpret_cast<const float4*>(p.rowvec + (long long)(m / hw) * p.ldrv + n);
        v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = act_pre(p.act, v[r] * p.alpha);
      if (res) {
        float rr[4];
        Elem<h16_t>::load4(res + (long long)m * p.ldr + n, rr);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += rr[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = act_post(p.act, v[r]);
      Elem<h16_t>::store4(out + (long long)m * p.ldo + n, v);
      Elem<h16_t>::store4(ct + row[u] * CP + c4[u] * 4, v);
    }
  }
  __syncthreads();
  gn_tile_stats<256>(ct, CP, nrows, BC / p.gn_unit, p.gn_unit, reinterpret_cast<float*>(ct + BR * CP),
                     p.gn_stats + ((long long)rb * (p.N / p.gn_unit) + (cs * BC) / p.gn_unit) * 2);
}

// The DMA loaders (LDS-DMA kernels of both tile widths) need a K-tile inside one tap of one source; a nearest-x2 input also needs
// pad <= 1 and the packed 16-bit window corner of gemm_dma_kernel
bool dma_loader_ok(const SaspaGemmParams& p) {
  const int bk = p.dtype == SASPA_HALF ? 64 : 32;
  const int ctot = p.c0 + p.c1;
  return (ctot % bk) == 0 && (p.c1 == 0 || (p.c0 % bk) == 0) && (!p.upsample || (p.pad <= 1 && p.hin < 16000 && p.win < 16000));
}

template <typename T, int WM, int WN, int NWM = 2, int NWN = 2>
int launch(const SaspaGemmParams& p, hipStream_t s, int ksplit) {
  constexpr int BM = 16 * WM * NWM, BN = 16 * WN * NWN, NT = 64 * NWM * NWN;
  const int tiles = ((p.N + BN - 1) / BN) * ((p.M + BM - 1) / BM);
  // persistent grid: as many workgroups as the chip keeps resident (256 CUs x blocks/CU by LDS / VGPR budget)
  constexpr int kResident = 256 * (NT > 256 ? 1 : ((BM + BN) * 256 > 48 * 1024 ? 2 : 4));
  const int zy = ksplit * p.nb1 * p.nb2;
  int gx = tiles;
  if ((long long)tiles * zy > kResident) gx = max(1, min(tiles, kResident / zy));
  dim3 grid(gx, ksplit, p.nb1 * p.nb2);
  const bool pw = p.kh == 1 && p.kw == 1 && p.stride == 1 && p.pad == 0 && !p.upsample;
  static const int abl = getenv("SASPA_GEMM_ABLATE") ? (atoi(getenv("SASPA_GEMM_ABLATE")) & 15) : 0;       // diagnostics only
  const int tiles_abl = tiles | (abl << 28);
  const int npart8 = saspa_gemm_npart8(p, BM, BN, gx, tiles);
  if (p.upsample == 2) {
    // phase mode (check_gemm: 16-bit types only), the same choices as below on instantiations of its own
    if constexpr (sizeof(T) == 2) {
      if constexpr (NT != 256) {
        hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, NWM, NWN, false, 3, false, true>), grid, dim3(NT), 0, s, p, tiles_abl, npart8);
      } else if (dma_loader_ok(p)) {
        constexpr bool can4 = (BM + BN) * 128 * 4 <= 160 * 1024;
        if (can4 && (long long)tiles * zy <= 320)
          hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, false, can4 ? 4 : 2, false, true>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
        else
          hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, false, 2, false, true>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
      } else {
        hipLaunchKernelGGL((gemm_kernel<T, WM, WN, false, true>), grid, dim3(256), 0, s, p, tiles, npart8);
      }
      SASPA_CHECK_LAUNCH();
      if (ksplit > 1) return saspa_gemm_splitk_reduce(p, s, ksplit);
      return 0;
    } else {
      return SASPA_ERANGE;
    }
  }
  if constexpr (NT != 256) {
    // 8-wave tiles exist only as DMA kernels (the plan checked dma_loader_ok)
    if (pw) hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, NWM, NWN, true, 3>), grid, dim3(NT), 0, s, p, tiles_abl, npart8);
    else if (p.upsample) hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, NWM, NWN, false, 3, true>), grid, dim3(NT), 0, s, p, tiles_abl, npart8);
    else hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, NWM, NWN, false, 3>), grid, dim3(NT), 0, s, p, tiles_abl, npart8);
  } else if (dma_loader_ok(p)) {
    // few tiles (<= ~1 workgroup per CU): spend the idle LDS on a 4-deep DMA ring (latency-bound
    // K loops); otherwise 2 stages and 2 workgroups per CU
    constexpr bool can4 = (BM + BN) * 128 * 4 <= 160 * 1024;
    const bool deep = can4 && (long long)tiles * zy <= 320;
    if (deep) {
      if (pw) hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, true, can4 ? 4 : 2>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
      else if (p.upsample) hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, false, can4 ? 4 : 2, true>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
      else hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, false, can4 ? 4 : 2>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
    } else {
      if (pw) hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, true, 2>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
      else if (p.upsample) hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, false, 2, true>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
      else hipLaunchKernelGGL((gemm_dma_kernel<T, WM, WN, 2, 2, false, 2>), grid, dim3(256), 0, s, p, tiles_abl, npart8);
    }
  } else {
    if (pw) hipLaunchKernelGGL((gemm_kernel<T, WM, WN, true>), grid, dim3(256), 0, s, p, tiles, npart8);
    else hipLaunchKernelGGL((gemm_kernel<T, WM, WN, false>), grid, dim3(256), 0, s, p, tiles, npart8);
  }
  SASPA_CHECK_LAUNCH();
  if (ksplit > 1) return saspa_gemm_splitk_reduce(p, s, ksplit);
  return 0;
}

// ---- the dispatch policy of the GEMM family ---------------------------------------------------------------------------------
// plan_gemm() decides, for a validated problem, the kernel family, its tile and the K split -- or refuses the problem; saspa_gemm
// runs the plan, saspa_gemm_which reports it, saspa_gemm_suggest_ksplit and saspa_gemm_as_auto answer from the same rules.  Every
// threshold is written once, here; the measurements behind them are in DESIGN.md (kernel table, K-split and round rules).
constexpr int kCUs = 256;
// a round of one-workgroup-per-CU launches counts as full from 85 % of its slots; a wide launch just over a whole number of rounds
// with its last round below 65 % (264 / 288 tiles of the fused Q|K|V projection of the 16x22 / 16x24 level: 99 us against 81 on
// the 4-wave tiles) takes the finer tiles
constexpr int kRoundFull = 85, kRoundRagged = 65;
// 8-wave wide kernel (256 x 320 / 256 tiles):
constexpr int kWideKMin = 640;                // K below this never goes wide
constexpr int kWideKFull = 960;               // 640 <= K < 960 (the level-1 pointwise layers) only un-split, from kWideAlone tiles
                                              // (a twin beside it: kTwinWholeRound)
constexpr int kLongK = 4096;                  // from here on one slice at half the chip, or K slices on the wide kernel
constexpr long long kTwinWholeRound = 96;     // with a twin launch beside it (sharing): un-split, whatever K
constexpr long long kWideAlone = 144;         // alone: un-split from 144 tiles (the 32x44 / 32x48 levels: 176 / 192 workgroups in one
                                              // round against 704 / 768 4-wave tiles in two, 74 vs 124 us; 128, the 512x512 case, ties)
constexpr long long kWideSplitMinTiles = 24;  // fewer tiles than CUs but long K: the wide kernel on K slices (1.17 - 1.45x the 4-wave
                                              // tiles on the 3x3 convs of the 32x32 / 16x16 levels)
constexpr long long kWideGegluTiles = 384;    // fused GEGLU projection: at least 1.5 rounds of wide tiles
// wave-specialised kernel: short-K GEGLU projections (level 0: 199 vs 214 us) and one full round of 128-row tiles
constexpr int kWsGegluKMax = 384;
// A-stationary kernel on a ragged last round of row blocks: the layers with a residual or at least this many columns
constexpr int kAsRaggedMinN = 640;

// t work items in rounds of kCUs: is the last round at least pct % full?
bool fills_rounds(long long t, int pct) { return t * 100 >= (t + kCUs - 1) / kCUs * kCUs * pct; }

// exactly one round of 128-row tiles, full: the wave-specialised kernel without K slices (19 vs 24 us at (4096, 1280, 1280), 52 vs
// 72 at (4096, 1280, 5120)); with more tiles it only ties the 4-wave kernel and, owning the CU's whole LDS, keeps the other graph
// branch's kernels off the CU.  352 tiles (the 16x22 level of a 512x704 image) would be two rounds at 69 %.
bool ws_one_round(long long t128) { return t128 >= kCUs && t128 < 2 * kCUs && fills_rounds(t128, kRoundFull); }

long long tiles128(const SaspaGemmParams& p) {
  const int bn = (p.N % 160 == 0) ? 160 : 128;
  return (long long)((p.M + 127) / 128) * ((p.N + bn - 1) / bn);
}
// the wide kernel's tile width in 64-column units (5: 320, 4: 256), 0 if N fits neither
int wide_fn(const SaspaGemmParams& p) { return (p.N % 320 == 0) ? 5 : (p.N % 256 == 0) ? 4 : 0; }
long long wide_tiles(const SaspaGemmParams& p, int fn) { return (long long)((p.M + 255) / 256) * (p.N / (64 * fn)); }

// The wide kernel under AUTO for t tiles and the caller's K split: the split it runs on, or 0 = not taken.  With GroupNorm statistics
// (gn) neither the short-K admission nor the ragged-round exception applies.
int wide_auto(const SaspaGemmParams& p, long long t, int ksplit, bool must_split, bool gn) {
  if (p.K < kWideKMin) return 0;
  if (p.K < kWideKFull && (gn || ksplit != 1 || must_split || t < (p.sharing ? kTwinWholeRound : kWideAlone))) return 0;
  if (ksplit == 1 && p.sharing && t >= kTwinWholeRound) return 1;
  if (ksplit == 1 && p.K >= kLongK && t >= kCUs / 2) return 1;        // one slice chosen by the cost model, half the CUs busy
  const bool ragged = !gn && t > kCUs && !fills_rounds(t, kRoundRagged);
  if (ksplit == 1 && !must_split && !ragged && t >= kWideAlone) return 1;
  if (ksplit > 1 && p.K >= kLongK && t >= kWideSplitMinTiles && t * ksplit >= kCUs / 2) return ksplit;
  return 0;
}

// A-stationary kernel under AUTO: whole rounds of 256-row blocks, or -- with a ragged last round (352 blocks at 512x704) -- the
// layers with a residual or >= kAsRaggedMinN columns, not the GEGLU projection (tools/as_bench.py); the only kernel with a fused
// LayerNorm / transposed tail
bool as_auto(const SaspaGemmParams& p) {
  if (p.variant != SASPA_GEMM_AUTO || p.defer_reduce || !saspa_gemm_as_ok(p)) return false;
  const long long blocks = (p.M + 255) / 256;
  return p.ln_gamma || p.out_t || fills_rounds(blocks, kRoundFull) || (p.act != SASPA_ACT_GEGLU && (p.residual || p.N >= kAsRaggedMinN));
}

// K-split of the wide kernel from a cost model (round 3): with t tiles and ks slices the launch takes ceil(t * ks / ncu) ROUNDS
// of workgroups, each c0 + (K-tiles per slice) * c1 long, plus a reduce pass over ks fp32 slabs.  Constants fitted on
// tools/conv_variant_sweep.py (profiles/r3_conv_sweep_704.txt): c0 = 20 us per workgroup (prologue, epilogue, launch), c1 = 1.34 us
// per 64-deep K-tile of a 256 x 320 tile (x 0.8 for 256 x 256), reduce at 4 TB/s.  ncu: 256, or 128 beside a twin launch.
int pp_choose_ksplit(long long t, int ktiles, long long mn, int fn, int ncu) {
  const double c0 = 20.0, c1 = fn == 5 ? 1.34 : 1.07;
  int best = 1;
  double best_cost = 1e30;
  for (int ks = 1; ks <= 8; ++ks) {
    if (ks > 1 && ktiles / ks < 8) break;
    const long long rounds = (t * ks + ncu - 1) / ncu;
    double cost = (double)rounds * (c0 + (double)((ktiles + ks - 1) / ks) * c1);
    if (ks > 1) cost += 5.0 + (4.0 * ks + 4.0) * (double)mn / 4.0e6;
    if (cost < best_cost - 1e-9) { best_cost = cost; best = ks; }
  }
  return best;
}

int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
// Measurement pins (tools/tile_sweep.py, tools/pp_check.py ...), read once.  SASPA_GEMM_TILE = WM WN of a 4-wave tile (45 44 25 24
// 22 41) or 845 = the 8-wave 256x160 tile; SASPA_GEMM_PP = 0: never the wide kernel, 4 / 5 / 14 / 15 / 24 / 25: force its tile and
// loop flavour, 1: AUTO
struct Pins { int tile, pp; };
const Pins& pins() {
  static const Pins v = [] {
    const int t = env_int("SASPA_GEMM_TILE", 0);
    const bool tile = t == 845 || t == 45 || t == 44 || t == 25 || t == 24 || t == 22 || t == 41;
    return Pins{tile ? t : 0, env_int("SASPA_GEMM_PP", 1)};
  }();
  return v;
}

struct GemmPlan {
  int family;   // SASPA_GEMM_TILED / WIDE / WS / AS
  int tile;     // TILED: WM * 10 + WN of the 4-wave tile, or 845; WIDE: fn (4, 5, or a SASPA_GEMM_PP flavour)
  int ksplit;
};

// the 4-wave tiles (and the 8-wave 256x160 one): chunk-major K, pre-split weights and the 8-wave tile need the DMA loaders
int plan_tiled(const SaspaGemmParams& p, int tile, int ksplit, GemmPlan& g) {
  const bool dma = dma_loader_ok(p);
  if ((p.korder == SASPA_KORDER_CHUNK || p.w_split || tile == 845) && !dma) return SASPA_ERANGE;
  g = {SASPA_GEMM_TILED, tile, ksplit};
  return 0;
}

// p: validated by check_gemm
int plan_gemm(const SaspaGemmParams& p, GemmPlan& g) {
  const bool bf16 = p.dtype == SASPA_HALF;
  const long long nb = (long long)p.nb1 * p.nb2;
  const bool pp_ok = nb == 1 && saspa_gemm_pp_eligible(p);     // bf16 only
  const bool ws_ok = saspa_gemm_ws_eligible(p);                // bf16, unbatched only
  const bool n160 = (p.N % 160) == 0;
  auto pick = [&](int family, int tile, int ksplit) { g = {family, tile, ksplit}; return 0; };
  // the A-stationary kernel writes no K slices
  if (bf16 && p.variant == SASPA_GEMM_AS) return !p.defer_reduce && saspa_gemm_as_ok(p) ? pick(SASPA_GEMM_AS, 0, 1) : SASPA_ERANGE;
  if (bf16 && as_auto(p)) return pick(SASPA_GEMM_AS, 0, 1);
  if (p.ln_gamma || p.out_t || p.variant == SASPA_GEMM_AS) return SASPA_ERANGE;
  const int ksplit = (p.workspace && p.ksplit > 1 && nb == 1 && p.N % 4 == 0) ? p.ksplit : 1;
  // ABI 18 deferred reduce: the caller's saspa_splitk_groupnorm sums exactly p.ksplit slabs.  A launch that ended on ONE slice (or
  // on a kernel that writes no slabs) would leave the workspace uninitialised: every rule below that drops the K split is closed
  // to such a call, and a call that cannot be split at all is refused here.
  const bool must_split = p.defer_reduce != 0;
  // phase mode: un-split launches key the statistics by 128-row blocks of a phase's low-res image; smaller images need the reduce
  // launch, which walks the output rows (saspa_gemm_suggest_ksplit answers >= 2 for them)
  if (p.upsample == 2 && p.gn_stats && (p.hin * p.win) % 128 != 0 && ksplit <= 1) return SASPA_ERANGE;
  if (must_split && (ksplit <= 1 || p.act == SASPA_ACT_GEGLU || p.N <= 32 || p.variant == SASPA_GEMM_WS)) return SASPA_ERANGE;
  if (p.gn_stats) {
    // statistics need the LDS-staged bf16 epilogue on 160 / 320-column tiles of 128 / 256 rows (check_gemm checked the shape):
    // the wide kernel where AUTO would take it, the 4-wave 128x160 tiles otherwise -- never the wave-specialised kernel (its
    // epilogue waves have no statistics pass) or the 64x64 tiles
    if (p.variant == SASPA_GEMM_WS) return SASPA_ERANGE;
    const bool can = pp_ok && (p.N % 320) == 0;
    if (p.variant == SASPA_GEMM_WIDE) return can ? pick(SASPA_GEMM_WIDE, 5, ksplit) : SASPA_ERANGE;
    if (can && pins().pp != 0 && p.variant == SASPA_GEMM_AUTO)
      if (const int ks = wide_auto(p, wide_tiles(p, 5), ksplit, must_split, true)) return pick(SASPA_GEMM_WIDE, 5, ks);
    return plan_tiled(p, 45, ksplit, g);
  }
  if (p.variant == SASPA_GEMM_WS) return ws_ok ? pick(SASPA_GEMM_WS, 0, 1) : SASPA_ERANGE;
  if (p.act == SASPA_ACT_GEGLU) {
    // (check_gemm: bf16, whole tiles)
    if (p.variant == SASPA_GEMM_AUTO && nb == 1 && tiles128(p) >= kCUs && p.K <= kWsGegluKMax && ws_ok) return pick(SASPA_GEMM_WS, 0, 1);
    // long K and enough wide tiles (116 vs 142 us at (4096, 10240, 1280); the level-1 projection (16384, 5120, 640) 117 vs 137-139)
    const bool wide = p.variant == SASPA_GEMM_WIDE ||
                      (p.variant == SASPA_GEMM_AUTO && p.K >= kWideKMin && (long long)((p.M + 255) / 256) * (p.N / 320) >= kWideGegluTiles);
    if (wide && pp_ok) return pick(SASPA_GEMM_WIDE, 5, 1);
    if (p.variant == SASPA_GEMM_WIDE) return SASPA_ERANGE;
    return plan_tiled(p, n160 ? 45 : 44, 1, g);
  }
  if (pins().tile) return plan_tiled(p, pins().tile, ksplit, g);
  if (p.N <= 32) return plan_tiled(p, 41, 1, g);
  if (p.variant == SASPA_GEMM_WIDE) {
    if (!pp_ok) return SASPA_ERANGE;
    return pick(SASPA_GEMM_WIDE, (p.N % 320 == 0 || p.N % 256 != 0) ? 5 : 4, ksplit);
  }
  if (pp_ok && pins().pp >= 4) return pick(SASPA_GEMM_WIDE, pins().pp, ksplit);
  const int fn = wide_fn(p);
  if (pp_ok && fn && pins().pp == 1 && p.variant == SASPA_GEMM_AUTO)
    if (const int ks = wide_auto(p, wide_tiles(p, fn), ksplit, must_split, false)) return pick(SASPA_GEMM_WIDE, fn, ks);
  if (p.variant == SASPA_GEMM_AUTO && ksplit == 1 && ws_ok && ws_one_round(tiles128(p))) return pick(SASPA_GEMM_WS, 0, 1);
  if (tiles128(p) * nb * ksplit >= 160 && p.N > 64) return plan_tiled(p, n160 ? 45 : 44, ksplit, g);
  return plan_tiled(p, 22, ksplit, g);
}

template <typename T>
int launch_tiled(const SaspaGemmParams& p, hipStream_t s, const GemmPlan& g) {
  switch (g.tile) {
    case 845: return launch<T, 4, 5, 4, 2>(p, s, g.ksplit);   // 256x160, 8 waves
    case 45: return launch<T, 4, 5>(p, s, g.ksplit);
    case 44: return launch<T, 4, 4>(p, s, g.ksplit);
    case 25: return launch<T, 2, 5>(p, s, g.ksplit);
    case 24: return launch<T, 2, 4>(p, s, g.ksplit);
    case 22: return launch<T, 2, 2>(p, s, g.ksplit);
    case 41: return launch<T, 4, 1>(p, s, g.ksplit);
  }
  return SASPA_ERANGE;
}

// Argument validation shared by saspa_gemm and saspa_gemm_which: p = *pp with the defaults filled in (nb1 / nb2, ksplit of GEGLU)
int check_gemm(const SaspaGemmParams* pp, SaspaGemmParams& p) {
  if (!pp) return SASPA_EINVAL;
  p = *pp;
  if (p.nb1 <= 0) p.nb1 = 1;
  if (p.nb2 <= 0) p.nb2 = 1;
  if (!p.a0 || !p.w || !p.out) return SASPA_EINVAL;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.batch <= 0) return SASPA_EINVAL;
  if (!dtype_served(p.dtype)) return SASPA_EINVAL;
  if (p.kh <= 0 || p.kw <= 0 || p.stride <= 0 || p.pad < 0) return SASPA_EINVAL;
  if (p.c1 > 0 && !p.a1) return SASPA_EINVAL;
  if (p.c1 < 0 || p.c0 <= 0) return SASPA_EINVAL;
  const int epc = p.dtype == SASPA_HALF ? 8 : 4;
  if (p.c0 % epc || p.c1 % epc || p.lda0 % epc || (p.c1 > 0 && p.lda1 % epc) || p.ldw % epc) return SASPA_EALIGN;
  if (p.ldo % 4 || (p.residual && p.ldr % 4)) return SASPA_EALIGN;
  if (!aligned16(p.a0) || !aligned16(p.w) || !aligned16(p.out) || (p.a1 && !aligned16(p.a1)) ||
      (p.residual && !aligned16(p.residual)) || (p.bias && !aligned16(p.bias)) || (p.rowvec && !aligned16(p.rowvec)))
    return SASPA_EALIGN;
  if (p.sa1 % epc || p.sa2 % epc || p.sw1 % epc || p.sw2 % epc || p.so1 % 4 || p.so2 % 4) return SASPA_EALIGN;
  if (p.rowvec && (p.ldrv % 4)) return SASPA_EALIGN;
  if (p.K != p.kh * p.kw * (p.c0 + p.c1)) return SASPA_ERANGE;
  if ((long long)p.batch * p.hout * p.wout != p.M) return SASPA_ERANGE;
  if (p.lda0 < p.c0 || (p.c1 > 0 && p.lda1 < p.c1) || p.ldw < p.K) return SASPA_ERANGE;
  if (p.act != SASPA_ACT_GEGLU && p.ldo < (p.out_t ? p.n_split : p.N)) return SASPA_ERANGE;
  if (p.ln_gamma && !p.ln_beta) return SASPA_EINVAL;
  if (p.out_t) {      // transposed tail columns (ABI 13): geometry is checked here, eligibility of the kernel in plan_gemm()
    if (p.n_split < 0 || p.n_split > p.N || p.rows_per_batch <= 0 || p.M % p.rows_per_batch || p.ldt < p.rows_per_batch) return SASPA_ERANGE;
    if (p.M / p.rows_per_batch > 1 && p.st < (long long)(p.N - p.n_split) * p.ldt) return SASPA_ERANGE;
    if ((reinterpret_cast<uintptr_t>(p.out_t) & 1u)) return SASPA_EALIGN;
  }
  // the window of every output pixel must come from the declared input extent
  {
    const int hv = p.upsample ? 2 * p.hin : p.hin, wv = p.upsample ? 2 * p.win : p.win;
    if ((p.hout - 1) * p.stride - p.pad >= hv || (p.wout - 1) * p.stride - p.pad >= wv) return SASPA_ERANGE;
  }
  if ((long long)p.batch * p.hin * p.win >= (1ll << 31)) return SASPA_ERANGE;
  const int bk = p.dtype == SASPA_HALF ? 64 : 32;
  {
    // buffer loads address every operand with 32-bit byte offsets below 2 GiB
    const long long esz = p.dtype == SASPA_HALF ? 2 : 4;
    const long long a0b = (long long)p.batch * p.hin * p.win * p.lda0 * esz;
    const long long a1b = p.c1 > 0 ? (long long)p.batch * p.hin * p.win * p.lda1 * esz : 0;
    const long long wb = (long long)p.N * p.ldw * esz;
    if (a0b >= (1ll << 31) || a1b >= (1ll << 31) || wb >= (1ll << 31)) return SASPA_ERANGE;
    // the tap-validity bitmask of the fast loaders (a K-tile inside one tap) holds 31 taps; larger windows (the 7x7 stem of
    // the filter stage's ResNet, 3 -> 8 padded channels) run on the generic per-lane loader, which has no mask
    const bool fastpath = ((p.c0 + p.c1) % bk) == 0 && (p.c1 == 0 || (p.c0 % bk) == 0);
    if (p.kh * p.kw > 31 && fastpath) return SASPA_ERANGE;
  }
  if (p.ksplit < 0 || p.ksplit > 64) return SASPA_ERANGE;
  if (p.korder != SASPA_KORDER_TAP && p.korder != SASPA_KORDER_CHUNK) return SASPA_EINVAL;
  if (p.korder == SASPA_KORDER_CHUNK && (p.c0 % bk || p.c1 % bk)) return SASPA_ERANGE;
  if (p.variant < SASPA_GEMM_AUTO || p.variant > SASPA_GEMM_AS) return SASPA_EINVAL;
  if (p.act == SASPA_ACT_GEGLU) {
    // fused GEGLU: bf16 only, whole tiles, weights pre-interleaved per tile (see header)
    const int bn = (p.N % 160) == 0 ? 160 : 128;
    if (p.dtype != SASPA_HALF || p.N % bn || p.residual || p.ldo % 8 || p.ldo < p.N / 2) return SASPA_ERANGE;
    p.ksplit = 1;
  } else if (p.act != SASPA_ACT_NONE && p.act != SASPA_ACT_SILU && p.act != SASPA_ACT_RELU && p.act != SASPA_ACT_ADD_RELU) {
    return SASPA_EINVAL;
  }
  if (p.ksplit > 1 && p.workspace && !aligned16(p.workspace)) return SASPA_EALIGN;
  if (p.gn_stats) {
    // epilogue GroupNorm statistics (ABI 12): bf16, whole 160-column tiles whose first column is a multiple of the unit
    if (p.dtype != SASPA_HALF || p.act == SASPA_ACT_GEGLU || (long long)p.nb1 * p.nb2 != 1) return SASPA_ERANGE;
    if (p.gn_unit < 2 || p.gn_unit > 16 || (p.gn_unit & 1) || (80 % p.gn_unit) != 0 || (p.N % 160) != 0) return SASPA_ERANGE;
    if ((p.ldo % 8) != 0 || (p.residual && (p.ldr % 8) != 0)) return SASPA_ERANGE;
  }
  // pre-split weights (ABI 20): only the SASPA_F32X3 DMA loop reads them
  if (p.w_split && p.dtype != SASPA_F32X3) return SASPA_ERANGE;
  if (p.upsample == 2) {
    // phase mode of the nearest-x2 3x3 / pad 1 conv (see SaspaGemmParams.upsample): 16-bit types, one source, plain epilogue
    if (p.dtype != SASPA_HALF || p.kh != 2 || p.kw != 2 || p.stride != 1 || p.pad != 1) return SASPA_ERANGE;
    if (p.hout != 2 * p.hin || p.wout != 2 * p.win) return SASPA_ERANGE;
    if (p.c1 > 0 || p.residual || p.rowvec || p.act == SASPA_ACT_GEGLU || p.ln_gamma || p.out_t || p.defer_reduce) return SASPA_ERANGE;
    if ((long long)p.nb1 * p.nb2 != 1) return SASPA_ERANGE;
    if (4ll * p.N * p.ldw * 2 >= (1ll << 31)) return SASPA_ERANGE;          // the four phase matrices, [4][N][ldw]
  }
  return 0;
}

// Phase mode: the launchers' view of the problem -- ONE phase's 2x2 conv over the low-res grid, the four phases as the batched
// dimension (blockIdx.z: its weight matrix, the same input, the same output buffer -- the epilogue scatters the rows)
SaspaGemmParams lower_phase(const SaspaGemmParams& p) {
  SaspaGemmParams q = p;
  q.M = p.M / 4;
  q.hout = p.hin;
  q.wout = p.win;
  q.nb1 = 4;
  q.nb2 = 1;
  q.sa1 = 0;
  q.sw1 = (long long)p.N * p.ldw;
  q.so1 = 0;
  return q;
}

}  // namespace

// Recommended K-split of a problem (1 = none): the caller sizes the fp32 workspace (ksplit*M*N floats) from it.
static int suggest_ksplit(const SaspaGemmParams& p);
extern "C" int saspa_gemm_suggest_ksplit(const SaspaGemmParams* pp) {
  if (!pp) return 1;
  const int ks = suggest_ksplit(*pp);
  // phase mode with epilogue statistics on images of less than whole 128-row blocks per phase: only the reduce launch can key them
  const bool need2 = pp->upsample == 2 && pp->gn_stats && (pp->hin * pp->win) % 128 != 0 && pp->N % 4 == 0;
  return need2 && ks < 2 ? 2 : ks;
}
static int suggest_ksplit(const SaspaGemmParams& p) {
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || (long long)p.nb1 * p.nb2 > 1 || p.N % 4 || p.act == SASPA_ACT_GEGLU) return 1;
  const int bk = p.dtype == SASPA_HALF ? 64 : 32;
  const int ktiles = (p.K + bk - 1) / bk;
  // one round of 128-row tiles on a pointwise layer: the wave-specialised kernel without K slices beats the wide kernel on K slices
  // ((4096, 1280, 5120): 52 vs 76 us, and no slabs) -- not beside a twin launch with long K, where two slices on the wide kernel
  // win (pair times 124 vs 146 us at (4096, 1280, 5120) + residual, tools/twin_sweep.py)
  if (!(p.sharing && p.K >= kLongK) && !p.gn_stats && p.dtype == SASPA_HALF && p.variant == SASPA_GEMM_AUTO && p.kh == 1 && p.kw == 1 &&
      ws_one_round(tiles128(p)) && saspa_gemm_ws_eligible(p))
    return 1;
  const int fn = wide_fn(p);
  if (p.dtype == SASPA_HALF && p.K >= kLongK && fn && saspa_gemm_pp_eligible(p)) {
    const long long t = wide_tiles(p, fn);
    if (t >= kWideSplitMinTiles) {
      // a twin launch beside it (sharing) counts on half the chip; one slice only where plan_gemm really takes the wide kernel
      // un-split -- below that a one-slice answer would land on the 4-wave tiles un-split: fall through
      const int ks = pp_choose_ksplit(t, ktiles, (long long)p.M * p.N, fn, p.sharing ? kCUs / 2 : kCUs);
      if (ks > 1 || wide_auto(p, t, 1, false, false)) return ks;
    }
  }
  // 4-wave tiles: enough K slices to give the CUs about two workgroups each, for the deep levels only
  const long long tiles = tiles128(p);
  if (p.N <= 64 || tiles >= 2 * kCUs || ktiles < 32) return 1;
  long long ks = (2 * kCUs + tiles - 1) / tiles;
  if (ks > 8) ks = 8;
  if (ks > ktiles / 8) ks = ktiles / 8;
  return ks < 1 ? 1 : (int)ks;
}

extern "C" int saspa_gemm_as_auto(const SaspaGemmParams* pp) { return pp && as_auto(*pp) ? 1 : 0; }

// Tile order of a launch: 0 = M-partitioned (an XCD walks whole rows of N tiles: its activations stay in L2, the weights
// stream through once per row block) or n = nbn / 8 > 0 = N-partitioned (an XCD owns an eighth of the N tiles for every row
// block: its weight slice stays in L2, the activations stream through once per XCD).  Estimated beyond-L2 bytes decide;
// profiles/r2_pmc_per_shape.txt has the measured ones (GEGLU projection at M = 16 384: 684 MB fetched for 28 MB of operands
// with the M-partitioned order).
int saspa_gemm_npart8(const SaspaGemmParams& p, int BM, int BN, int G, int tiles) {
  const int nbn = (p.N + BN - 1) / BN, nbm = (p.M + BM - 1) / BM;
  if ((long long)p.nb1 * p.nb2 != 1 || (nbn & 7) || (G & 7) || G <= 0 || tiles % G || p.N % BN) return 0;
  const double esz = p.dtype == SASPA_HALF ? 2.0 : 4.0;
  const double a = (double)p.batch * p.hin * p.win * (p.c0 + p.c1) * esz;     // the input tensor (taps re-read from L2)
  const double w = (double)p.N * p.K * esz;
  const double l2 = 3.8 * (1 << 20);                                            // of the 4 MiB per XCD
  const double g8 = G / 8.0;
  const double mpart = a * (nbn > g8 ? nbn / g8 : 1.0) + w * (w <= l2 ? 8.0 : (double)nbm);
  const double npart = 8.0 * a + w * (w / 8.0 <= l2 ? 1.0 : (double)nbm);
  return npart < 0.75 * mpart ? nbn / 8 : 0;
}

int saspa_gemm_splitk_reduce(const SaspaGemmParams& pl, hipStream_t s, int ksplit) {
  if (pl.defer_reduce) return 0;      // ABI 18: the slabs go to saspa_splitk_groupnorm
  SaspaGemmParams p = pl;
  if (p.upsample == 2 && p.nb1 == 4) {   // phase mode: back from the launchers' per-phase view (lower_phase) to the output's
    p.M *= 4;
    p.hout *= 2;
    p.wout *= 2;
    p.nb1 = 1;
  }
  if (p.gn_stats) {        // saspa_gemm checked: bf16, N % 160 == 0, 160 % gn_unit == 0
    if (p.upsample == 2) hipLaunchKernelGGL(splitk_reduce_stats_kernel<true>, dim3((p.M + 127) / 128, p.N / 80), dim3(256), 0, s, p, ksplit);
    else hipLaunchKernelGGL(splitk_reduce_stats_kernel<false>, dim3((p.M + 127) / 128, p.N / 80), dim3(256), 0, s, p, ksplit);
    SASPA_CHECK_LAUNCH();
    return 0;
  }
  long long blocks = ((long long)p.M * (p.N / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (p.upsample == 2) hipLaunchKernelGGL((splitk_reduce_kernel<h16_t, true>), dim3((unsigned)blocks), dim3(256), 0, s, p, ksplit);   // 16-bit only
  else if (p.dtype == SASPA_HALF) hipLaunchKernelGGL((splitk_reduce_kernel<h16_t>), dim3((unsigned)blocks), dim3(256), 0, s, p, ksplit);
#ifndef SASPA_HALF_F16
  else hipLaunchKernelGGL((splitk_reduce_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, s, p, ksplit);
#endif
  SASPA_CHECK_LAUNCH();
  return 0;
}

/* ABI 20: which kernel family saspa_gemm would run `p` on, and on how many K slices: the validation and the plan, nothing launched.
 * Returns family | (ksplit << 8) with family = SASPA_GEMM_TILED / WIDE / WS / AS, or the SASPA_E* code saspa_gemm would return.
 * bench.py attributes every recorded launch to its kernel with this (roofline.by_kernel / roofline.dominant). */
extern "C" int saspa_gemm_which(const SaspaGemmParams* pp) {
  SaspaGemmParams p;
  GemmPlan g{};
  int rc = check_gemm(pp, p);
  if (rc == 0) rc = plan_gemm(p, g);
  return rc != 0 ? rc : g.family | (g.ksplit << 8);
}

extern "C" int saspa_gemm(const SaspaGemmParams* pp, void* stream) {
  SaspaGemmParams p;
  GemmPlan g{};
  int rc = check_gemm(pp, p);
  if (rc == 0) rc = plan_gemm(p, g);
  if (rc != 0) return rc;
  if (p.upsample == 2) p = lower_phase(p);       // planned on the caller's view (M output rows, K = 4 C), launched per phase
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (g.family) {
    case SASPA_GEMM_AS: return saspa_gemm_as_launch(p, s);
    case SASPA_GEMM_WS: return saspa_gemm_ws_launch(p, s);
    case SASPA_GEMM_WIDE: return saspa_gemm_pp_launch(p, s, g.ksplit, g.tile);
  }
  if (p.dtype == SASPA_HALF) return launch_tiled<h16_t>(p, s, g);
#ifndef SASPA_HALF_F16       // the fp16 library holds no fp32 tiles: check_gemm refused those dtype codes
  if (p.dtype == SASPA_F32X3) return launch_tiled<f32x3_t>(p, s, g);
  return launch_tiled<float>(p, s, g);
#else
  return SASPA_EINVAL;
#endif
}
