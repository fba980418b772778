// PNG encode on the device (include/saspa_hip.h, DESIGN.md "PNG encode on the device"): per image the zlib stream of its PNG-filtered
// rows, Huffman-only.  png_segment_kernel: one workgroup per segment of <= 16 rows (<= 32767 filtered bytes, resident in LDS) --
// row filters, histogram, code lengths, canonical codes, header and bit packing into LDS, then one coalesced copy to the segment's
// workspace slot.  png_join_kernel: moves the segments to the front of the image's slot and appends the Adler-32.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kHeaderBits = 1222;   // 3 + 5 + 5 + 4 + 19 * 3 + 286 * 4 + 4
constexpr int kLenBit0 = 74;        // bit offset of the first literal/length code length
constexpr uint32_t kAdlerMod = 65521;

struct SegMeta {
  uint32_t size;   // bytes of the segment in the stream
  uint32_t a, b;   // Adler partial sums of its filtered bytes, mod 65521: sum d, sum (len - i) * d
  uint32_t len;    // filtered bytes
};

__host__ __device__ inline long long align16ll(long long v) { return (v + 15) & ~15ll; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup, returned to every thread; `scratch`: kThreads / 64 words.  Two barriers.
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* scratch) {
  v = (uint32_t)wave_sum_i((int)v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// or `n` (<= 32) bits of `val` into the LSB-first bit stream at bit `bit`
__device__ __forceinline__ void put_bits(uint32_t* out, uint32_t bit, uint32_t val, int n) {
  const uint32_t w = bit >> 5, s = bit & 31;
  const uint64_t v = (uint64_t)val << s;
  atomicOr(&out[w], (uint32_t)v);
  if (s + n > 32) atomicOr(&out[w + 1], (uint32_t)(v >> 32));
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int predict(int f, int a, int b, int c) {
  return f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : paeth(a, b, c);
}
__device__ __forceinline__ int cost8(int r) { r &= 255; return r < 128 ? r : 256 - r; }

// filt: filt_cap bytes of dynamic LDS, then the output words.  wdata + block * seg_stride: the segment's workspace slot.
__global__ __launch_bounds__(kThreads) void png_segment_kernel(const uint8_t* __restrict__ px, int H, int W, int C, int R, int nseg,
                                                               int filt_cap, uint8_t* __restrict__ wdata, long long seg_stride,
                                                               SegMeta* __restrict__ meta) {
  extern __shared__ __align__(16) uint8_t smem[];
  uint8_t* filt = smem;
  uint32_t* outw = reinterpret_cast<uint32_t*>(smem + filt_cap);
  __shared__ uint32_t hist[257];
  __shared__ uint8_t lens[288];
  __shared__ uint16_t codes[288];
  __shared__ uint16_t order[257];
  __shared__ uint8_t sorted_len[257];
  __shared__ uint8_t ftype[16];
  __shared__ uint32_t bl_count[16], next_code[16];
  __shared__ uint32_t scratch[4];
  __shared__ uint32_t kraft, nused;
  __shared__ unsigned long long adler_b;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = blockIdx.x % nseg, img = blockIdx.x / nseg;
  const int wc = W * C, rowbytes = wc + 1;
  const int r0 = seg * R, rows = min(R, H - r0);
  const int segbytes = rows * rowbytes;
  const bool final_seg = seg == nseg - 1;
  const uint8_t* base = px + (size_t)img * H * wc;
  uint8_t* dst = wdata + (long long)blockIdx.x * seg_stride;

  for (int s = tid; s < 288; s += kThreads) lens[s] = 0;
  for (int s = tid; s < 257; s += kThreads) hist[s] = s == 256 ? 1u : 0u;
  if (tid < 16) bl_count[tid] = 0;
  if (tid == 0) { kraft = 0; nused = 0; adler_b = 0; }

  // ---- 1. the filter of every row: one wave per row, lanes stride the row ----
  for (int r = wave; r < rows; r += kThreads / 64) {
    const int y = r0 + r;
    const uint8_t* cur = base + (size_t)y * wc;
    const uint8_t* up = cur - wc;                    // read only when y > 0
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int x = lane; x < wc; x += 64) {
      const int v = cur[x];
      const int a = x >= C ? cur[x - C] : 0;
      const int b = y > 0 ? up[x] : 0;
      const int c = (y > 0 && x >= C) ? up[x - C] : 0;
      c0 += cost8(v);
      c1 += cost8(v - a);
      c2 += cost8(v - b);
      c3 += cost8(v - ((a + b) >> 1));
      c4 += cost8(v - paeth(a, b, c));
    }
    c0 = wave_sum_i(c0); c1 = wave_sum_i(c1); c2 = wave_sum_i(c2); c3 = wave_sum_i(c3); c4 = wave_sum_i(c4);
    if (lane == 0) {
      int best = 0, bc = c0;
      if (c1 < bc) { best = 1; bc = c1; }
      if (c2 < bc) { best = 2; bc = c2; }
      if (c3 < bc) { best = 3; bc = c3; }
      if (c4 < bc) { best = 4; bc = c4; }
      ftype[r] = (uint8_t)best;
    }
  }
  __syncthreads();

  // ---- 2. filtered bytes into LDS, histogram, Adler partial sums ----
  uint32_t sum_a = 0;
  unsigned long long sum_b = 0;
  for (int r = 0; r < rows; ++r) {
    const int y = r0 + r, f = ftype[r];
    const uint8_t* cur = base + (size_t)y * wc;
    const uint8_t* up = cur - wc;
    for (int i = tid; i < rowbytes; i += kThreads) {
      int d;
      if (i == 0) {
        d = f;
      } else {
        const int x = i - 1;
        const int v = cur[x];
        const int a = x >= C ? cur[x - C] : 0;
        const int b = y > 0 ? up[x] : 0;
        const int c = (y > 0 && x >= C) ? up[x - C] : 0;
        d = (v - predict(f, a, b, c)) & 255;
      }
      const int idx = r * rowbytes + i;
      filt[idx] = (uint8_t)d;
      atomicAdd(&hist[d], 1u);
      sum_a += (uint32_t)d;
      sum_b += (unsigned long long)(uint32_t)(segbytes - idx) * (uint32_t)d;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum_b += __shfl_xor(sum_b, o, 64);
  if (lane == 0) atomicAdd(&adler_b, sum_b);
  sum_a = block_sum_u32(sum_a, scratch);             // (its barriers also publish hist, filt and adler_b)

  // ---- 3. code lengths: l = the smallest l >= 1 with (count << l) >= T, then the greedy shortening in (count desc, symbol asc) order ----
  const uint32_t T = (uint32_t)segbytes + 1u;
  for (int s = tid; s < 257; s += kThreads) {
    const uint32_t c = hist[s];
    int rank = 0;
    for (int j = 0; j < 257; ++j) {
      const uint32_t cj = hist[j];
      rank += (cj > c || (cj == c && j < s)) ? 1 : 0;
    }
    order[rank] = (uint16_t)s;
    int l = 0;
    if (c) {
      l = 1;
      while ((c << l) < T) ++l;                      // <= 15: T <= 32768
      atomicAdd(&kraft, 1u << (15 - l));
      atomicAdd(&nused, 1u);
    }
    sorted_len[rank] = (uint8_t)l;
  }
  __syncthreads();
  if (tid == 0) {
    // the slack is a multiple of the smallest weight in use, so the walk always ends on slack 0: the code is complete
    uint32_t slack = 32768u - kraft;
    const int n = (int)nused;
    while (slack > 0) {
      bool changed = false;
      for (int i = 0; i < n; ++i) {
        const int l = sorted_len[i];
        const uint32_t w = 1u << (15 - l);
        if (l > 1 && w <= slack) {
          sorted_len[i] = (uint8_t)(l - 1);
          slack -= w;
          changed = true;
          if (slack == 0) break;
        }
      }
      if (!changed) break;
    }
  }
  __syncthreads();
  uint32_t body = 0;
  for (int i = tid; i < 257; i += kThreads) {
    const int s = order[i], l = sorted_len[i];
    lens[s] = (uint8_t)l;
    if (l) atomicAdd(&bl_count[l], 1u);
    body += hist[s] * (uint32_t)l;
  }
  body = block_sum_u32(body, scratch);

  // ---- the stored fallback, decided before anything is written ----
  const uint32_t hb = kHeaderBits + body;
  const uint32_t hbytes = final_seg ? (hb + 7) / 8 : (hb + 3 + 7) / 8 + 4;
  if (tid == 0) {
    SegMeta m;
    m.size = hbytes >= (uint32_t)segbytes + 5u ? (uint32_t)segbytes + 5u : hbytes;
    m.a = sum_a % kAdlerMod;
    m.b = (uint32_t)(adler_b % kAdlerMod);
    m.len = (uint32_t)segbytes;
    meta[blockIdx.x] = m;
  }
  if (hbytes >= (uint32_t)segbytes + 5u) {
    if (tid == 0) {
      dst[0] = final_seg ? 1 : 0;
      dst[1] = (uint8_t)(segbytes & 255);
      dst[2] = (uint8_t)(segbytes >> 8);
      dst[3] = (uint8_t)(~segbytes & 255);
      dst[4] = (uint8_t)((~segbytes >> 8) & 255);
    }
    for (int i = tid; i < segbytes; i += kThreads) dst[5 + i] = filt[i];
    return;
  }

  // ---- 4. canonical codes (RFC 1951 3.2.2), bit-reversed ----
  const int nwords = (int)((hbytes + 3) / 4);        // <= (segbytes + 7) / 4: inside the LDS plan and the workspace slot
  for (int w = tid; w < nwords; w += kThreads) outw[w] = 0;
  if (tid == 0) {
    uint32_t code = 0;
    next_code[0] = 0;
    for (int bits = 1; bits < 16; ++bits) {
      code = (code + (bits > 1 ? bl_count[bits - 1] : 0u)) << 1;
      next_code[bits] = code;
    }
  }
  __syncthreads();
  for (int s = tid; s < 257; s += kThreads) {
    const int l = lens[s];
    if (l) {
      uint32_t k = 0;
      for (int j = 0; j < s; ++j) k += lens[j] == l ? 1u : 0u;
      codes[s] = (uint16_t)(__brev(next_code[l] + k) >> (32 - l));
    }
  }
  // ---- 5. the block header ----
  if (tid == 0) {
    put_bits(outw, 0, (final_seg ? 1u : 0u) | 4u, 3);       // BFINAL, BTYPE = 10
    put_bits(outw, 3, 29u, 5);                               // HLIT: 286 lengths
    put_bits(outw, 8, 0u, 5);                                // HDIST: 1 distance code
    put_bits(outw, 13, 15u, 4);                              // HCLEN: 19 code-length code lengths
    for (int i = 3; i < 19; ++i) put_bits(outw, 17 + 3 * i, 4u, 3);   // 16, 17, 18 -> 0 (already); symbols 0..15 -> 4 bits each
    put_bits(outw, kLenBit0 + 4 * 286, 8u, 4);               // the distance code: length 1 (0001 reversed)
  }
  for (int s = tid; s < 286; s += kThreads) {
    const uint32_t l = lens[s];
    put_bits(outw, kLenBit0 + 4 * s, __brev(l) >> 28, 4);
  }
  __syncthreads();

  // ---- 6. bit packing: a contiguous run of symbols per lane, offsets from a workgroup scan ----
  const int nsym = segbytes + 1;
  const int per = (nsym + kThreads - 1) / kThreads;
  const int i0 = min(tid * per, nsym), i1 = min(i0 + per, nsym);
  uint32_t mybits = 0;
  for (int i = i0; i < i1; ++i) mybits += lens[i < segbytes ? filt[i] : 256];
  uint32_t incl = mybits;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  uint32_t start = kHeaderBits + incl - mybits;
  for (int w = 0; w < wave; ++w) start += scratch[w];
  {
    uint64_t acc = 0;
    int nacc = (int)(start & 31);
    uint32_t word = start >> 5;
    for (int i = i0; i < i1; ++i) {
      const int s = i < segbytes ? filt[i] : 256;
      acc |= (uint64_t)codes[s] << nacc;
      nacc += lens[s];
      if (nacc >= 32) {
        atomicOr(&outw[word], (uint32_t)acc);
        acc >>= 32;
        nacc -= 32;
        ++word;
      }
    }
    if (nacc > 0 && acc != 0) atomicOr(&outw[word], (uint32_t)acc);
  }
  // ---- 7. a segment that is not the last: empty stored block (000, pad to a byte, 00 00 FF FF) ----
  if (tid == 0 && !final_seg) put_bits(outw, 8 * (hbytes - 4) + 16, 0xFFFFu, 16);
  __syncthreads();
  uint32_t* dw = reinterpret_cast<uint32_t*>(dst);
  for (int w = tid; w < nwords; w += kThreads) dw[w] = outw[w];
}

// One workgroup per segment: its offset in the stream is the sum of the sizes before it.
__global__ __launch_bounds__(kThreads) void png_join_kernel(const uint8_t* __restrict__ wdata, long long seg_stride,
                                                            const SegMeta* __restrict__ meta, int nseg, uint8_t* __restrict__ streams,
                                                            long long capacity, int* __restrict__ sizes) {
  __shared__ uint32_t scratch[4];
  const int tid = threadIdx.x;
  const int seg = blockIdx.x % nseg, img = blockIdx.x / nseg;
  const SegMeta* m = meta + (long long)img * nseg;
  uint32_t before = 0;
  for (int k = tid; k < seg; k += kThreads) before += m[k].size;
  before = block_sum_u32(before, scratch);
  const uint32_t size = m[seg].size;
  uint8_t* slot = streams + (long long)img * capacity;
  const uint8_t* src = wdata + (long long)blockIdx.x * seg_stride;
  uint8_t* dst = slot + 2 + before;
  for (uint32_t i = tid; i < size; i += kThreads) dst[i] = src[i];
  if (tid != 0) return;
  if (seg == 0) { slot[0] = 0x78; slot[1] = 0x01; }
  if (seg == nseg - 1) {
    uint64_t a = 1, b = 0;
    for (int k = 0; k < nseg; ++k) {
      b = (b + (uint64_t)(m[k].len % kAdlerMod) * a + m[k].b) % kAdlerMod;
      a = (a + m[k].a) % kAdlerMod;
    }
    uint8_t* tail = dst + size;
    tail[0] = (uint8_t)(b >> 8); tail[1] = (uint8_t)b; tail[2] = (uint8_t)(a >> 8); tail[3] = (uint8_t)a;
    sizes[img] = (int)(2 + before + size + 4);
  }
}

struct PngGeom { int rowbytes, R, nseg, segmax; long long capacity, seg_stride; };

// SASPA_E* or 0
int png_geom(int H, int W, int C, PngGeom* g) {
  if (H <= 0 || W <= 0) return SASPA_EINVAL;
  if (C != 1 && C != 3) return SASPA_ERANGE;
  const long long rb = 1 + (long long)W * C;
  if (rb > 32767) return SASPA_ERANGE;
  g->rowbytes = (int)rb;
  g->R = SASPA_PNG_SEG_ROWS(g->rowbytes);
  g->nseg = (int)(((long long)H + g->R - 1) / g->R);
  g->segmax = (H < g->R ? H : g->R) * g->rowbytes;
  g->capacity = 2 + (long long)H * rb + 5ll * g->nseg + 4;
  g->seg_stride = align16ll(g->segmax + 8);      // a Huffman segment is copied out in whole words: <= segbytes + 7 bytes
  if (g->capacity > 0x7fffffffll) return SASPA_ERANGE;
  return 0;
}

}  // namespace

extern "C" long long saspa_png_capacity(int H, int W, int C) {
  PngGeom g;
  const int rc = png_geom(H, W, C, &g);
  return rc ? rc : g.capacity;
}

extern "C" long long saspa_png_workspace(int n, int H, int W, int C) {
  PngGeom g;
  if (n <= 0) return SASPA_EINVAL;
  const int rc = png_geom(H, W, C, &g);
  if (rc) return rc;
  const long long segs = (long long)n * g.nseg;
  if (segs > 0x7fffffffll) return SASPA_ERANGE;
  return align16ll(segs * (long long)sizeof(SegMeta)) + segs * g.seg_stride;
}

extern "C" int saspa_png_deflate(const uint8_t* px, int n, int H, int W, int C, uint8_t* streams, long long capacity, int* sizes,
                                 void* workspace, long long workspace_bytes, void* stream) {
  if (!px || !streams || !sizes || !workspace || n <= 0) return SASPA_EINVAL;
  PngGeom g;
  const int rc = png_geom(H, W, C, &g);
  if (rc) return rc;
  const long long need = saspa_png_workspace(n, H, W, C);
  if (need < 0) return (int)need;
  if (capacity < g.capacity || workspace_bytes < need) return SASPA_ERANGE;
  if (!aligned16(workspace) || (reinterpret_cast<uintptr_t>(sizes) & 3u)) return SASPA_EALIGN;
  const long long segs = (long long)n * g.nseg;
  SegMeta* meta = reinterpret_cast<SegMeta*>(workspace);
  uint8_t* wdata = reinterpret_cast<uint8_t*>(workspace) + align16ll(segs * (long long)sizeof(SegMeta));
  const int filt_cap = (int)align16ll(g.segmax);
  const size_t lds = (size_t)filt_cap + (size_t)g.seg_stride;      // <= 32768 + 32784: above the 64 KiB a launch gets by default
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(png_segment_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       32768 + 32784);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)segs), dim3(kThreads), lds, s, px, H, W, C, g.R, g.nseg, filt_cap, wdata,
                     g.seg_stride, meta);
  SASPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(png_join_kernel, dim3((unsigned)segs), dim3(kThreads), 0, s, wdata, g.seg_stride, meta, g.nseg, streams, capacity,
                     sizes);
  SASPA_CHECK_LAUNCH();
  return 0;
}
