/*
 * saspa_hip.h -- C ABI of libsaspa_hip.so: the MI355X (gfx950) kernels behind the
 * SaSPA augmentation-generation hot path.
 *
 * The reference (EyalMichaeli/SaSPA-Aug) has NO FFI / native layer: the path sits
 * behind one Python call, `pipe(**pipe_args)` (run_aug/run_aug.py:278), whose
 * arithmetic runs inside diffusers/torch CUDA kernels, and behind
 * `cv2.Canny` (all_utils/utils.py:83).  This header is therefore the boundary a
 * maintainer binds *instead of* those library calls; each entry point names the
 * upstream module whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; no allocation, no
 *     host sync, no hidden stream: work is enqueued on `stream` (a hipStream_t
 *     passed as void*), so calls are graph-capturable;
 *   - activations are channels-last: [batch][H*W][C], pixel pitch given in
 *     elements; dtype selects bf16 (SASPA_BF16) or fp32 (SASPA_F32) storage,
 *     accumulation is always fp32;
 *   - weights are [N][K] with K contiguous (conv: K = (ky*kw+kx)*Cin + c);
 *   - bias / norm parameters / per-batch vectors are always fp32;
 *   - return value 0 on success, negative SASPA_E* on a rejected argument
 *     (checked on the host BEFORE any launch), positive = hipError_t of the launch.
 */
#ifndef SASPA_HIP_H
#define SASPA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SASPA_BF16 0
#define SASPA_F32 1
/* saspa_gemm only: fp32 storage (every pointer as for SASPA_F32), products formed as three bf16 MFMAs (x = hi + lo with
 * hi = bf16(x), lo = bf16(x - hi); a b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32 accumulation): ~2^-17 relative per
 * product instead of 2^-24, at several times the rate of the fp32 MFMA.  For the fp32-upcast SDXL VAE
 * (run_aug/run_aug.py:224 `pipe.upcast_vae()`), whose range -- not its last 7 bits -- is why the reference leaves fp16. */
#define SASPA_F32X3 2
/* IEEE fp16 storage and MFMA operands (fp32 accumulation): the compute type of libsaspa_hip_f16.so, a second build of the 16-bit kernels
 * (GEMM / conv, attention, norms, elementwise, the fused transformer-block launches) with the element type swapped -- same entry points,
 * layouts and schedules; wherever this header says "bf16" of those, read "the library's 16-bit type" (saspa_half_type).  The reference
 * runs its pipelines in fp16 (run_aug/run_aug.py:323).  That library accepts ONLY this code (SASPA_BF16 / SASPA_F32 / SASPA_F32X3 ->
 * SASPA_EINVAL); libsaspa_hip.so refuses it the same way.  Stores do not clamp: beyond 65504 the result is inf, as in the reference. */
#define SASPA_F16 3

#define SASPA_EINVAL (-1) /* null pointer / non-positive size */
#define SASPA_EALIGN (-2) /* channel count, pitch or pointer not 16-byte compatible */
#define SASPA_ERANGE (-3) /* shape outside what the kernel supports */

#define SASPA_ACT_NONE 0
#define SASPA_ACT_SILU 1
/* saspa_gemm only, bf16 only: fused GEGLU epilogue.  N = 2F columns are computed, F are
 * stored: out[m][f] = val * gelu_erf(gate).  The weight rows (and bias) must be packed per
 * output tile of BN columns (BN = 160 if N % 160 == 0 else 128; N % BN == 0 required):
 * tile t holds features [t*BN/2, (t+1)*BN/2) -- their value rows first, then their gate rows. */
#define SASPA_ACT_GEGLU 3
/* filter stage (CLIP-RN50 / WSDAN_CAL ResNet convs with the BatchNorm folded into weights + bias): */
#define SASPA_ACT_RELU 5     /* out = relu(alpha*(acc + bias + rowvec)) + residual */
#define SASPA_ACT_ADD_RELU 6 /* out = relu(alpha*(acc + bias + rowvec) + residual): Bottleneck "out += identity; relu" */

#define SASPA_GEMM_AUTO 0
#define SASPA_GEMM_TILED 1 /* 4-wave 128x160 / 128x128 / 64x64 tiles, two workgroups per CU */
#define SASPA_GEMM_WIDE 2  /* 8-wave 256x320 / 256x256 tile, one workgroup per CU */
#define SASPA_GEMM_WS 3    /* wave-specialised 128x160 tile (12 waves: 4 MMA + 4 loader + 4 epilogue): short-K bf16 layers */
#define SASPA_GEMM_AS 4    /* A-stationary: 256 rows x K = 320 held in registers, W streamed through LDS (level-0 pointwise layers) */

#define SASPA_KORDER_TAP 0
#define SASPA_KORDER_CHUNK 1
#define SASPA_KORDER_CHUNK32 2   /* saspa_conv3x3_halo only (ABI 19): K = ((chunk32 * 9 + ky*3+kx) * 32 + c_in_chunk), chunks of 32 channels */

/* ---- implicit-GEMM convolution / linear ----------------------------------
 * out[m][n] = act( alpha * (sum_k A[m][k] * W[n][k] + bias[n] + rowvec[b(m)][n]) ) + residual[m][n]
 * where m = (b, oy, ox) and A is the im2col view of up to two channel-concatenated
 * NHWC sources (skip-concat of the UNet up blocks), optionally nearest-x2 upsampled.
 * Replaces: ResnetBlock2D.conv1/conv2/conv_shortcut, Downsample2D.conv, Upsample2D
 * (interpolate+conv), Transformer2DModel.proj_in/proj_out, Attention.to_q/k/v/to_out,
 * GEGLU.proj, FeedForward.net.2, time_emb_proj, ControlNet zero convs and
 * cond-embedding, VAE decoder convs, CLIP linears (a7.1, a7.5, a7.6, a7.8).
 * A linear layer is the kh=kw=1 case with batch=1, hin=hout=M, win=wout=1.
 * Batched use (nb1*nb2 independent problems, element strides per operand) serves
 * the unfused attention path (scores = Q K^T, out = P V) and the V^T projection. */
typedef struct SaspaGemmParams {
  int dtype;                 /* SASPA_BF16 | SASPA_F32 (A, W, residual, out) */
  const void* a0;            /* source 0, NHWC */
  const void* a1;            /* source 1 (channels appended after source 0) or NULL */
  int c0, c1;                /* channels taken from each source (multiples of 8) */
  int lda0, lda1;            /* pixel pitch of each source, elements */
  int batch, hin, win;       /* stored input extent */
  int hout, wout;            /* output extent */
  int kh, kw, stride, pad;   /* kernel window */
  int upsample;              /* 1: conv sees the input nearest-upsampled x2.
                              * 2: PHASE MODE of the same layer (nearest x2 + 3x3 / pad 1), 4/9 of the multiply-accumulates: output
                              * pixel (2i+py, 2j+px) is a 2x2 correlation over the low-res input whose window starts at
                              * (i+py-1, j+px-1) (zero padding carries over) and whose weights are sums of the 3x3 taps -- rows
                              * {0}, {1, 2} for py = 0 and {0, 1}, {2} for py = 1, columns alike.  The caller passes kh = kw = 2,
                              * stride = 1, pad = 1, hout = 2 hin, wout = 2 win, M = batch*hout*wout, K = 4 c0 and `w` = the four
                              * phase matrices [py*2+px][N][ldw], each a 2x2 conv packed in `korder`; ONE launch (the phase is the
                              * kernels' batched dimension, every row tile lies in one phase, the epilogue and the split-K reduce
                              * scatter the rows to their pixels).  16-bit types, one source, no residual / rowvec / GEGLU /
                              * defer_reduce: SASPA_ERANGE otherwise.  gn_stats: as usual; where hin*win % 128 != 0 only a launch
                              * on K slices can key them (saspa_gemm_suggest_ksplit answers >= 2, SASPA_ERANGE without slabs). */
  const void* w;             /* [N][K] */
  int ldw;                   /* row pitch of w, elements */
  int M, N, K;               /* M = batch*hout*wout, K = kh*kw*(c0+c1) */
  const float* bias;         /* [N] or NULL */
  const float* rowvec;       /* [batch or 1][N] or NULL (time-embedding projection) */
  int ldrv;                  /* batch pitch of rowvec (0: same vector for every batch) */
  const void* residual;      /* [M][N] or NULL */
  int ldr;
  float alpha;
  int act;                   /* SASPA_ACT_* */
  void* out;                 /* [M][N] */
  int ldo;
  /* batching: problem index z = i1*nb2 + i2 */
  int nb1, nb2;
  long long sa1, sa2;        /* element strides of a0 */
  long long sw1, sw2;        /* element strides of w */
  long long so1, so2;        /* element strides of out (and residual) */
  /* split-K (optional): ksplit > 1 with a workspace of ksplit*M*N floats makes the library
   * slice the K range over ksplit workgroups per tile (fp32 partial slabs + one reduce /
   * epilogue launch).  Ignored when workspace is NULL, for batched problems or N % 4 != 0. */
  int ksplit;
  float* workspace;
  /* kernel variant: SASPA_GEMM_AUTO lets the library choose per shape; the other values pin one
   * (tests, tuning).  SASPA_GEMM_WIDE = one 8-wave workgroup per CU on a 256 x 256/320 tile
   * (long-K bf16 layers); it returns SASPA_ERANGE for a problem it cannot run (fp32, fused GEGLU
   * unless N % 320 == 0, channel counts that are not multiples of 64, windows other than 1x1 or 3x3/pad 1). */
  int variant;
  /* K order of the packed weights (and of the K walk), ABI v4.  SASPA_KORDER_TAP: K = (ky*kw+kx)*C + c (tap-major, the
   * default).  SASPA_KORDER_CHUNK: the C = c0+c1 channels are cut into chunks of one K-tile (64 bf16 / 32 fp32 elements)
   * and K = ((chunk*kh*kw) + ky*kw+kx)*tile + c_in_chunk: the kh*kw taps of one channel chunk are consecutive K-tiles,
   * so a workgroup re-reads the same input rows back to back (L2 hits) instead of once per pass over all channels.
   * Requires c0 (and c1, if used) to be multiples of the K-tile; SASPA_ERANGE otherwise. */
  int korder;
  /* GroupNorm statistics out of the epilogue (ABI 12; removes the consumer's statistics pass, saspa_groupnorm_stats).
   * gn_stats != NULL: besides `out`, the launch leaves, for every block rb of 128 consecutive output rows and every unit u of
   * gn_unit consecutive output channels, gn_stats[(rb * (N / gn_unit) + u) * 2 + {0, 1}] = (sum, sum of squares) of the
   * STORED values (after bias / row vector / activation / residual, as rounded to the output dtype) over the block's rows < M.
   * A unit is the finest channel granule every consuming GroupNorm's groups are made of (block_out[0] / groups = 10 for
   * SD-1.5 / SDXL), so one buffer serves a plain consumer, a consumer over a channel concat and both consumers of a skip
   * tensor (SaspaGroupNormParams.stats0 / stats1).  bf16 only, N % 160 == 0, 80 % gn_unit == 0, gn_unit even and <= 16, every
   * tile's first column a multiple of gn_unit (the library picks 160 / 320-column tiles), no fused GEGLU, unbatched;
   * SASPA_ERANGE otherwise.  Deterministic (fixed summation order; no atomics). */
  float* gn_stats;
  int gn_unit;
  /* LayerNorm fused into the operand load, and a transposed second output (ABI 13): the A-stationary kernel for pointwise
   * layers with K = 320 (the level-0 transformer blocks: each workgroup keeps 256 rows of A in REGISTERS across every column
   * tile, so the rows can be normalised once, in place, before the first product).
   * ln_gamma != NULL: A is replaced by LayerNorm(A) over its K channels (two-pass mean / variance in fp32, eps = ln_eps,
   * affine ln_gamma / ln_beta [K], rounded to bf16 -- the arithmetic of saspa_layernorm) before the product; removes the
   * LayerNorm launch and its 2 x M x K bytes.  Only problems saspa_gemm_as_eligible() accepts; SASPA_ERANGE otherwise.
   * out_t != NULL: output columns n >= n_split are written TRANSPOSED to out_t instead of out: element (row, n) goes to
   * out_t[(row / rows_per_batch) * st + (n - n_split) * ldt + row % rows_per_batch] -- the V^T operand of saspa_flash_attn
   * out of the same launch as Q | K (BasicTransformerBlock.attn1: one read of the normalised tokens instead of two
   * launches).  n_split % 64 == 0, rows_per_batch % 32 == 0, same eligibility. */
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  void* out_t;
  int ldt;
  long long st;
  int n_split;
  int rows_per_batch;
  /* Concurrency hint (ABI 15).  0: the launch has the chip to itself (the default).  1: a TWIN launch of the same shape
   * runs beside it on another stream -- the two encoder branches of a sampling step (UNet encoder || ControlNet encoder walk
   * identical layer shapes side by side) -- so AUTO sizes tile choice and split-K for HALF the CUs: the convs / projections
   * of the 32x32 level (128 tiles of 256 x 320) run un-split on the 8-wave kernel next to their twin instead of on two K
   * slices with fp32 slabs and a reduce launch, the 16x16 level takes two slices instead of four.  Only saspa_gemm_suggest_ksplit
   * and the AUTO dispatch read it; the result differs from sharing = 0 by the summation order of K only. */
  int sharing;
  /* ABI 18.  1: when the launch runs on K slices (ksplit > 1 with a workspace), saspa_gemm leaves the fp32 partial slabs in
   * `workspace` and does NOT run its reduce / epilogue launch -- the caller hands them to saspa_splitk_groupnorm, which sums
   * them, adds bias / row vector and applies the consuming GroupNorm in the same launch (`out` is then not written).
   * ABI 19: a contract, not a hint -- a launch that would end on ONE K slice or on a kernel without slabs (fused GEGLU, N <= 32,
   * the weight-stationary and A-stationary kernels) returns SASPA_ERANGE instead of writing `out` behind the caller's back. */
  int defer_reduce;
  /* ABI 20, SASPA_F32X3 only.  1: `w` holds the weights PRE-SPLIT: every K-tile of 32 packed-K values of a row (128 bytes, where the fp32
   * values would sit) is [32 bf16 hi | 32 bf16 lo], hi = bf16(w), lo = bf16(w - hi), in the order the kernel's lanes consume a tile:
   * 16-byte chunk c (0..3) of either half carries tile positions 4c..4c+3 and 16+4c..16+4c+3 (weights.presplit_x3).  The launch then
   * splits only the activation operand in registers (half the VALU work of the K loop, which is what bounds the SASPA_F32X3 GEMMs);
   * same products, same order: bit-identical to the in-kernel split.  Needs the LDS-DMA loader ((c0 + c1) % 32 == 0, c0 % 32 == 0 with a
   * second source); SASPA_ERANGE otherwise. */
  int w_split;
} SaspaGemmParams;
/* Non-zero if the A-stationary kernel can run the problem (bf16 pointwise layer, K = c0 = 320, N % 64 == 0, at least 192
 * blocks of 256 rows, no row vector / split-K / GroupNorm statistics / batching, alpha = 1, activation none or fused GEGLU,
 * 16-byte aligned operands, ldo % 8 == 0): the only kernel that takes ln_gamma / out_t.  Returns 2 or 0 (the kernel deals its
 * work evenly over the CUs at every eligible size; 1, "ragged last round", is no longer returned). */
int saspa_gemm_as_eligible(const SaspaGemmParams* p);
/* ABI 20: 1 if saspa_gemm with variant AUTO will run THIS problem on the A-stationary kernel (the predicate dispatch itself uses):
 * what a caller must ask before it plans around that choice -- e.g. dropping SaspaGemmParams.gn_stats, which that kernel's
 * epilogue does not produce.  (saspa_gemm_as_eligible says whether the kernel CAN run it.) */
int saspa_gemm_as_auto(const SaspaGemmParams* p);
/* ABI 20: which kernel family saspa_gemm would run `p` on and on how many K slices: saspa_gemm's validation and dispatch plan, nothing
 * launched, `stream` not needed.  Returns family | (ksplit << 8), family = SASPA_GEMM_TILED / WIDE / WS / AS, or the SASPA_E* code
 * saspa_gemm would return.  Measurement aid: bench.py attributes every recorded launch to its kernel (roofline.dominant). */
int saspa_gemm_which(const SaspaGemmParams* p);
int saspa_gemm(const SaspaGemmParams* p, void* stream);
/* The library's recommended K-split factor for a problem (1 = none; every field but ksplit / workspace filled in):
 * the caller allocates ksplit*M*N floats, sets p->ksplit / p->workspace and calls saspa_gemm.  Long-K layers with
 * too few tiles to fill the chip get K slices (the 8-wave kernel on the 32x32 / 16x16 levels' 3x3 convs, the 4-wave
 * tiles on the 8x8 level). */
int saspa_gemm_suggest_ksplit(const SaspaGemmParams* p);

/* ---- fused flash attention (bf16) -----------------------------------------
 * O[b][i][h*D+d] = sum_j softmax_j(scale * Q[b][i][h,:] . K[b][j][h,:]) * V[b][j][h,d]
 * V is consumed TRANSPOSED: vt[b][(h*D+d)][j] (produced by saspa_gemm with the
 * operands swapped), keys j >= nk are masked; causal=1 additionally masks j > i
 * (CLIP text tower).  Replaces AttnProcessor2_0 / F.scaled_dot_product_attention in
 * BasicTransformerBlock.attn1/attn2 and CLIPAttention (a7.1, a7.5, a7.6). */
typedef struct SaspaAttnParams {
  const void* q; int ldq; long long sqb;   /* [B][nq][heads*D], row pitch, batch stride (elements) */
  const void* k; int ldk; long long skb;   /* [B][nk][heads*D] */
  const void* vt; int ldvt; long long svb; /* [B][heads*D][ldvt >= nk] */
  void* o; int ldo; long long sob;
  int batch, heads, D;                     /* D multiple of 8, <= 160 */
  int nq, nk;
  float scale;
  int causal;
  int flags;                               /* SASPA_ATTN_* bits (ABI 11) */
} SaspaAttnParams;
/* The queries already carry scale * log2(e) (folded into the to_q weights when they are packed): K Q^T is the
 * log2-domain logit, `scale` is ignored, and the kernel runs the loop with no per-score multiply / subtract / max
 * (saspa_attn.hip, "v2").  Same result up to the rounding point of the scale. */
#define SASPA_ATTN_QPRESCALED 1
/* ABI 14: `vt` holds V ROW-MAJOR -- V[b][key][heads * D], row pitch ldvt >= heads * D, batch stride svb -- i.e. the columns of
 * a fused Q | K | V projection as they are; the kernel transposes on the way from LDS to the MFMA (ds_read_b64_tr_b16), so
 * no transposed value projection is launched (BasicTransformerBlock.attn1 at the 32x32 / 16x16 levels). */
#define SASPA_ATTN_V_ROWMAJOR 2
/* Which loop saspa_flash_attn_bf16 would run `p` on and in which form: its validation, its knobs (SASPA_ATTN_MODE / _V4 / _RING, read
 * per call as the launch reads them) and its launch plan (saspa_attn.hip: plan_attn), nothing launched, `stream` not needed.  Returns
 * SASPA_ATTN_LOOP_* in bits 0-3, ORed with the SASPA_ATTN_PLAN_* bits and (ablation id << SASPA_ATTN_PLAN_ABL_SHIFT; 0 in the shipped
 * library) -- one value per kernel instantiation -- or the SASPA_E* code saspa_flash_attn_bf16 would return.  Measurement and test aid:
 * a test that means one loop asserts it before it runs, tests/golden/attn_dispatch.json records the rule decision for decision. */
#define SASPA_ATTN_LOOP_V1 1          /* running-maximum loop, 4 waves x 32 queries (flash_attn_kernel) */
#define SASPA_ATTN_LOOP_V2 2          /* prescaled queries, reference level, 4 waves (flash_attn_v2_kernel) */
#define SASPA_ATTN_LOOP_V3 3          /* v2's arithmetic software-pipelined, 8 waves x 32 queries (flash_attn_v3_kernel) */
#define SASPA_ATTN_LOOP_V4 4          /* 8 waves x 64 queries, 32-key half steps, d = 40 (flash_attn_v4_kernel) */
#define SASPA_ATTN_LOOP_MASK 15
#define SASPA_ATTN_PLAN_KEYS128 16    /* 128-key K / V tiles (64 otherwise) */
#define SASPA_ATTN_PLAN_DB 32         /* v2: two LDS buffers, one barrier per tile */
#define SASPA_ATTN_PLAN_RING6 64      /* v3: six ring slots, one barrier per two steps (four otherwise) */
#define SASPA_ATTN_PLAN_VROW 128      /* the kernel reads V row-major (SASPA_ATTN_V_ROWMAJOR) */
#define SASPA_ATTN_PLAN_ONES 256      /* the softmax denominator accumulates in the spare ones row of V^T (D < padded head dim) */
#define SASPA_ATTN_PLAN_ABL_SHIFT 12
int saspa_flash_attn_which(const SaspaAttnParams* p);
int saspa_flash_attn_bf16(const SaspaAttnParams* p, void* stream);

/* Fused attention for ONE WIDE head per batch entry (the 512-channel mid-block attention of the VAE):
 *   out[b][i][:] = sum_j softmax_j(scale * q[b][i][:] . k[b][j][:]) * v[b][j][:]
 * d is a multiple of 64 with 192 <= d <= 512 (narrower heads: saspa_flash_attn_bf16).  q, k, v and out are row-major [batch][n][ld]
 * in the library's 16-bit type (`dtype` must be saspa_half_type()), each with its own row pitch (ld*) and batch stride (s*b), in
 * elements -- so q, k and v may be column slices of one fused Q | K | V buffer.  V is read row-major: no transposed copy, no
 * workspace.  nq, nk >= 1, otherwise arbitrary; keys >= nk of the last key tile are masked inside the kernel.
 * Arithmetic: logits, running maximum, running sum and the online-softmax rescale in fp32; scale * log2(e) is applied to the fp32
 * logit; P is rounded once to the 16-bit type for the PV MFMA; O accumulates in fp32 and is rounded once on store -- the rounding
 * points of saspa_flash_attn_bf16.  No logit is ever stored in 16 bits, so unscaled dot products beyond 65504 are harmless in fp16.
 * A batch entry's result does not depend on the batch size or its position in the batch.
 * Host-side validation, before any launch: null pointer, dtype other than the library's 16-bit type, batch / nq / nk < 1,
 * batch > 65535, d outside the range above, a pitch shorter than d -> SASPA_EINVAL; pointers not 16-byte aligned, pitches or batch
 * strides not multiples of 8 -> SASPA_EALIGN. */
int saspa_attn_wide(int dtype, const void* q, int ldq, long long sqb, const void* k, int ldk, long long skb, const void* v, int ldv,
                    long long svb, void* out, int ldo, long long sob, int batch, int nq, int nk, int d, float scale, void* stream);

/* saspa_attn_wide on fp32 STORAGE with x3 products (default library only): ONE WIDE head per batch entry,
 *   out[b][i][:] = sum_j softmax_j(scale * q[b][i][:] . k[b][j][:]) * v[b][j][:]
 * the mid-block attention of the fp32 VAE without its n x n score matrix.  The call shape of saspa_attn_wide minus `dtype`: q, k, v and
 * out point to float, row-major [batch][n][ld], each with its own row pitch (ld*) and batch stride (s*b) in elements -- so q, k and v
 * may be column slices of one fused Q | K | V buffer.  V is read row-major.  d is a multiple of 64 with 192 <= d <= 512 (narrower
 * heads: saspa_flash_attn_f32x3).  nq, nk >= 1, otherwise arbitrary; keys >= nk of the last key tile are masked inside the kernel and
 * their rows are never read.  No workspace, no allocation, no host synchronisation; capturable.
 * Arithmetic: the contract of saspa_flash_attn_f32x3 below.  Every fp32 operand is split as hi = bf16(x), lo = bf16(x - hi) (round to
 * nearest) and every product sum -- Q K^T and P V alike -- is lo hi + hi lo + hi hi accumulated in fp32 on bf16 MFMAs; scale * log2(e)
 * is applied to the fp32 logit; running maximum, exp2, row sum and the online rescale are fp32; P is split from its fp32 value and
 * NEVER rounded to one bf16; O accumulates in fp32 and is divided by the fp32 row sum.  Every reduction has a fixed order, nothing is
 * atomic: a batch entry's bytes depend neither on the batch size nor on its position in the batch.
 * Host-side validation, before any launch: null pointer, batch / nq / nk < 1, batch > 65535, d outside the range above, a pitch shorter
 * than d -> SASPA_EINVAL; pointers not 16-byte aligned, pitches or batch strides not multiples of 4 -> SASPA_EALIGN. */
int saspa_attn_wide_f32x3(const void* q, int ldq, long long sqb, const void* k, int ldk, long long skb, const void* v, int ldv,
                          long long svb, void* out, int ldo, long long sob, int batch, int nq, int nk, int d, float scale, void* stream);

/* Flash attention on fp32 STORAGE with x3 products (the fused form of the fp32 parity path; default library only):
 *   o[b][i][h*D+d] = sum_j softmax_j(scale * q[b][i][h,:] . k[b][j][h,:]) * v[b][j][h,d]
 * Takes SaspaAttnParams as saspa_flash_attn_bf16 does, with q, k, vt and o pointing to float; pitches and batch strides in elements.
 * V arrives TRANSPOSED, vt[b][h*D+d][ldvt >= nk].  D is a multiple of 8, at most 160; nq, nk >= 1, otherwise arbitrary: keys >= nk are
 * masked inside the kernel, causal = 1 masks j > i, `scale` is honoured.  No score matrix, no workspace, no allocation, no host
 * synchronisation; capturable.
 * Arithmetic: every fp32 operand is split as hi = bf16(x), lo = bf16(x - hi) (round to nearest) and every product sum -- the logits
 * Q K^T and the weighted values P V alike -- is lo hi + hi lo + hi hi accumulated in fp32 on bf16 MFMAs (SASPA_F32X3's split and order:
 * at most 2^-17 of |a b| per product).  scale * log2(e) is applied to the fp32 logit; running maximum, exp2, row sum and the online
 * rescale are fp32; P is split from its fp32 value and NEVER rounded to one bf16 (what separates this kernel from the 16-bit loops); O
 * accumulates in fp32 and is divided by the fp32 row sum.  Every reduction has a fixed order, nothing is atomic: a batch entry's result
 * depends neither on the batch size nor on its position in the batch.
 * Host-side validation, before any launch: null pointer, batch / heads / nq / nk < 1, D outside the range above, ldq / ldk / ldo <
 * heads * D, ldvt < nk, any SASPA_ATTN_* flag set (prescaled queries and row-major V belong to the 16-bit loops) -> SASPA_EINVAL;
 * pointers not 16-byte aligned, pitches or batch strides not multiples of 4 -> SASPA_EALIGN. */
int saspa_flash_attn_f32x3(const SaspaAttnParams* p, void* stream);

/* row softmax in place over a [rows][ld] matrix (unfused attention path: fp32
 * parity mode and the 512-wide single-head VAE attention): x = softmax(scale*x) over
 * the first n columns; causal: row r of each `rows_per_mat` block only sees cols <= r. */
int saspa_softmax_rows(int dtype, void* x, long long rows, int n, int ld, float scale,
                       int causal, int rows_per_mat, void* stream);

/* ---- GroupNorm (+SiLU): NHWC, two launches -------------------------------
 * stats: per (image, pixel split, channel slab, group) sums of x and x^2 into `partial`;
 * apply: every workgroup first combines the sums of ITS image in fp64 into mean / rstd per group (no
 * finalize launch in between, ABI 10), then streams y = act((x - mean) * rstd * gamma + beta).
 * Replaces ResnetBlock2D.norm1/norm2 (+SiLU), Transformer2DModel.norm, conv_norm_out,
 * VAE GroupNorms (a7.5, a7.6, a7.8).
 * x may be the channel concat of two sources (x1 != NULL). */
typedef struct SaspaGroupNormParams {
  int dtype;
  const void* x0; const void* x1;
  int c0, c1, ldx0, ldx1;
  int batch, hw, groups;
  float eps;
  const float* gamma; const float* beta;  /* [C] */
  float* partial;        /* workspace: batch * nsplit * C * 2 floats (holds the per-(image, split, slab, group) sums that
                            saspa_groupnorm_stats leaves for saspa_groupnorm_apply; same p for both calls) */
  int nsplit;            /* pixel splits of the statistics pass, 1 .. hw */
  float* scale_shift;    /* unused since ABI 10 (the apply pass derives scale / shift itself); may be NULL */
  int act;
  void* y; int ldy;      /* apply output [batch*hw][C] */
  /* ABI 12: statistics left by the producers' epilogues (SaspaGemmParams.gn_stats) instead of a saspa_groupnorm_stats
   * launch: stats0 belongs to x0, stats1 to x1 (NULL without x1); each is [batch * hw / 128][c_i / unit][2] floats.
   * Needs hw % 128 == 0, c0 % unit == 0 and (C / groups) % unit == 0; `partial` / `nsplit` are then unused. */
  const float* stats0; const float* stats1;
  int unit;
} SaspaGroupNormParams;
int saspa_groupnorm_stats(const SaspaGroupNormParams* p, void* stream);
int saspa_groupnorm_apply(const SaspaGroupNormParams* p, void* stream);
/* ABI 17: statistics + apply in ONE launch for small images (one workgroup per (image, group): the group's hw * C / groups
 * values are read once into registers, reduced, normalised and written) -- the 8x8 level of the UNet / ControlNet, where a
 * GroupNorm was two launches of launch latency.  `partial` / `nsplit` / `stats*` are not read.  _eligible: non-zero when every
 * group lies inside one source, has whole 8-channel chunks and hw * (C / groups) <= 8 192. */
int saspa_groupnorm_onepass_eligible(const SaspaGroupNormParams* p);
int saspa_groupnorm_onepass(const SaspaGroupNormParams* p, void* stream);
/* ABI 18: split-K reduce + epilogue + GroupNorm(+SiLU) in ONE launch for small images: ResnetBlock2D.conv1 -> norm2 -> SiLU at
 * the 8x8 / 16x16 levels, where conv1 runs on K slices and its reduce launch, the GroupNorm statistics and the apply pass were
 * three launches of launch latency around a tensor nobody else reads.  g: the conv's parameters as given to saspa_gemm with
 * defer_reduce = 1 (M, N, hout * wout rows per image, workspace, ksplit, bias, rowvec / ldrv, alpha; no activation, no residual);
 * n: the GroupNorm (batch, hw, groups, eps, gamma, beta, act, y / ldy; one source of N channels).  One workgroup per (image,
 * group) sums the slabs of its hw x N / groups values, rounds them to the storage dtype (the rounding point of the unfused path),
 * takes the statistics, normalises from registers and writes y.  _eligible: non-zero if (N / groups) % 4 == 0 and
 * hw * N / groups <= 12 288. */
int saspa_splitk_groupnorm_eligible(const SaspaGemmParams* g, const SaspaGroupNormParams* n);
int saspa_splitk_groupnorm(const SaspaGemmParams* g, const SaspaGroupNormParams* n, void* stream);

/* ---- halo-tiled 3x3 conv with the CONSUMING GroupNorm (+SiLU) applied to its input tile in LDS (ABI 19) -----------------
 * out = conv3x3(act(GroupNorm(cat(a0, a1)))) (+ bias + rowvec, * alpha, + residual, epilogue statistics: as saspa_gemm) in ONE
 * launch: ResnetBlock2D's  norm1 -> SiLU -> conv1  and  norm2 -> SiLU -> conv2  (diffusers ResnetBlock2D.forward; SURVEY 8a
 * a7.5 / a7.6).  Replaces saspa_groupnorm_apply + saspa_gemm for these layers: the normalised tensor is never written.
 * p: the conv exactly as for saspa_gemm (bf16, 3x3 / stride 1 / pad 1, no upsampling, c0 / c1 multiples of 32 with c0 + c1 a
 * multiple of 64, N % 320 == 0 or N % 256 == 0, hout * wout % 256 == 0, weights packed SASPA_KORDER_CHUNK32; ksplit /
 * workspace / defer_reduce / gn_stats as for saspa_gemm).  g: the GroupNorm over the conv's INPUT channels, NULL for a plain
 * conv of an already normalised tensor; its statistics come from the producers' epilogues (stats0 / stats1 / unit, see
 * SaspaGroupNormParams) or from saspa_groupnorm_stats (partial / nsplit).  Same arithmetic and rounding points as the two
 * launches it replaces (scale / shift in fp32, SiLU by v_exp + v_rcp, rounding to bf16 before the product).
 * _eligible: non-zero if the launch can run; _ksplit: the K slices a requested factor really uses (slices are whole pairs of
 * 32-channel chunks) -- size the workspace and set p->ksplit from it. */
typedef struct SaspaConvGnParams {
  const float* gamma_beta32;   /* [(c0 + c1) / 32][64]: per 32-channel chunk gamma[32] | beta[32] */
  int groups;
  float eps;
  int act;                     /* SASPA_ACT_NONE | SASPA_ACT_SILU, applied after the affine */
  const float* stats0; const float* stats1; int unit;
  const float* partial; int nsplit;
} SaspaConvGnParams;
int saspa_conv3x3_halo_eligible(const SaspaGemmParams* p, const SaspaConvGnParams* g);
int saspa_conv3x3_halo_ksplit(const SaspaGemmParams* p, int want);
int saspa_conv3x3_halo(const SaspaGemmParams* p, const SaspaConvGnParams* g, void* stream);

/* LayerNorm over the last dim (BasicTransformerBlock.norm1/2/3, CLIP LNs). */
int saspa_layernorm(int dtype, const void* x, int ldx, void* y, int ldy, long long rows, int C,
                    const float* gamma, const float* beta, float eps, void* stream);

/* ---- elementwise ----------------------------------------------------------*/
/* GEGLU: y[m][f] = x[m][f] * gelu_erf(x[m][F+f])   (diffusers GEGLU) */
int saspa_geglu(int dtype, const void* x, int ldx, void* y, int ldy, long long rows, int F, void* stream);
/* act: 1 SiLU, 2 quick-GELU x*sigmoid(1.702x) (CLIP MLP), 4 erf-GELU (BERT / Q-Former FFN), 5 ReLU; in/out [rows][C] */
int saspa_activation(int dtype, int act, const void* x, int ldx, void* y, int ldy, long long rows, int C,
                     void* stream);
/* CLIP embeddings: out[i][:] = tok[ids[i]][:] + pos[i % npos][:] */
int saspa_embed_tokens(int dtype, const int* ids, int n, int npos, const void* tok, const void* pos, int C,
                       void* out, void* stream);
/* ContextCLIPTextEmbeddings of BLIP-Diffusion (a8): ids [nseq][ntok] prompt tokens, ctx
 * [nseq][nctx][C] subject tokens spliced in at position ctx_begin (reference: ctx_begin_pos = 2, 16 tokens,
 * ntok = 77 - 16); out [nseq][ntok+nctx][C] = spliced token embeddings + pos[0 .. ntok+nctx). */
int saspa_embed_tokens_ctx(int dtype, const int* ids, int nseq, int ntok, const void* ctx, int nctx, int ctx_begin,
                           const void* tok, const void* pos, int C, void* out, void* stream);
/* classifier-free guidance + one linear-multistep update (PNDMScheduler.step_plms with skip_prk_steps, the
 * scheduler BlipDiffusionControlNetPipeline keeps, run_aug/run_aug.py:217), fused:
 *   e = eu + g (ec - eu);  if store_slot >= 0: hist[store_slot] = e
 *   m = w_cur e + sum_k w_hist[k] hist[k]   (hist slots as they were BEFORE this call's store)
 *   x' = coef_sample * s + coef_model * m,  s = sample if non-NULL else x;  x' goes to both CFG halves of x.
 * hist: 4 slots of nimg*hw*ldc elements; the host owns which slot holds which past output. */
int saspa_cfg_plms_step(int dtype, const void* eps, void* x, void* hist, const void* sample, int nimg, long long hw,
                        int C, int ldc, float guidance, int store_slot, float w_cur, const float* w_hist,
                        float coef_sample, float coef_model, void* stream);
/* classifier-free guidance + DDIM step (eta=0), fused; writes x_prev into both
 * CFG halves of the model-input buffer.  eps: [2*nimg][hw][ldc] (uncond first),
 * x: [2*nimg][hw][ldc]; channels c < C are live.
 *   e = eu + g*(ec-eu); x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); x' = sqrt(a_p) x0 + sqrt(1-a_p) e
 * Replaces the CFG lines + DDIMScheduler.step (a7.4, a7.7). */
int saspa_cfg_ddim_step(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc,
                        float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                        float sqrt_1m_a_prev, void* stream);
/* DDIM step (eta=0) without classifier-free guidance: eps, x [nimg][hw][ldc], x updated in place.  The
 * SDXL-Turbo operating point of the reference (guidance_scale 0 -> one conditional evaluation per step,
 * run_aug/run_aug.py:564-571; SURVEY 8a: a9). */
int saspa_ddim_step(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, float sqrt_a_t,
                    float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, void* stream);
/* ---- device-side step state: ONE captured hipGraph of a sampling step serves every timestep -------------
 * The per-step values a captured launch sequence cannot take as kernel arguments live in device tables indexed by a
 * device-resident step counter: saspa_gather_row_f32 copies row *index of a [rows][row_elems] fp32 table into the
 * buffer the time-embedding row vectors point into (dst[0..n)), saspa_ddim_step_dev is the (CFG +) DDIM update with
 * its four coefficients read from row *index of coefs[steps][4] (cfg = 1: classifier-free guidance pair as
 * saspa_cfg_ddim_step, 0: plain as saspa_ddim_step), saspa_index_add bumps the counter at the end of the step. */
int saspa_gather_row_f32(const float* table, long long row_elems, const int* index, float* dst, long long n, void* stream);
int saspa_ddim_step_dev(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, int cfg, float guidance,
                        const float* coefs, const int* index, void* stream);
int saspa_index_add(int* index, int delta, void* stream);
/* three-branch guidance + DDIM step (eta=0), fused: the InstructPix2Pix update.  eps, x: [3*nimg][hw][ldc] in the groups
 * (uncond | image | text); x carries the noisy latents in channels c < C (C <= 4) and the image latents (zeros in group 0) above.
 *   e = e0 + g (e2 - e1) + ig (e1 - e0); x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); x' = sqrt(a_p) x0 + sqrt(1-a_p) e
 * x is read from group 0; x' is written to channels c < C of all three groups, channels C..ldc-1 keep their bits.
 * Errors before any launch: null pointer SASPA_EINVAL, alignment SASPA_EALIGN, ldc != 8 / C > 4 / nimg < 1 SASPA_ERANGE.
 * _dev: the four coefficients come from row *index of coefs[steps][4], as saspa_ddim_step_dev. */
int saspa_cfg3_ddim_step(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, float guidance,
                         float image_guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev,
                         void* stream);
int saspa_cfg3_ddim_step_dev(int dtype, const void* eps, void* x, int nimg, long long hw, int C, int ldc, float guidance,
                             float image_guidance, const float* coefs, const int* index, void* stream);
/* saspa_cfg_plms_step with its per-evaluation parameters read from row *index of table[evaluations][10] =
 * (store_slot, w_cur, w_hist[4], coef_sample, coef_model, save_sample, use_saved): the evaluation with save_sample copies
 * x into `saved` ([nimg][hw][ldc]) before the update, the one with use_saved reads it instead of x. */
int saspa_cfg_plms_step_dev(int dtype, const void* eps, void* x, void* hist, void* saved, int nimg, long long hw, int C, int ldc,
                            float guidance, const float* table, const int* index, void* stream);
/* y = x * s  (latents / scaling_factor before the VAE) */
int saspa_scale(int dtype, const void* x, void* y, long long n, float s, void* stream);
/* u8 RGB [n][H*W][3] -> [n][H*W][8] activations in [0,1], pad channels zero
 * (VaeImageProcessor.preprocess with do_normalize=False; SURVEY 8a: a7.2) */
int saspa_u8_to_act(int dtype, const uint8_t* src, void* dst, long long npix, void* stream);
/* VAE output [npix][ldx] (3 live channels) -> u8 RGB: round(255*clamp(x/2+0.5,0,1))
 * (VaeImageProcessor.postprocess; SURVEY 8a: a7.10) */
int saspa_act_to_u8(int dtype, const void* x, int ldx, uint8_t* dst, long long npix, void* stream);

/* ---- Canny edge extractor (integer exact vs cv2.Canny, aperture 3, L1) ------
 * src: u8 [n][H][W][3]; dst: u8 [n][H][W][3] in {0,255} (HWC3 replicated);
 * work: 8*n*H*W bytes of scratch.  The hysteresis bitmaps of one image (2*H*ceil(W/32)*4 bytes)
 * live in one CU's LDS when they fit 160 KiB (up to e.g. 512x1280); larger images (1024x1024)
 * keep them in the tail of `work` (W >= 64 required there, else SASPA_ERANGE).
 * Replaces all_utils/utils.py:81-99 CannyDetector/preprocess_canny (a6). */
int saspa_canny(const uint8_t* src, uint8_t* dst, uint8_t* work, int n, int H, int W, int low, int high,
                void* stream);

/* ---- image pre-processing of the CLIP image front-ends (integer exact) ----------
 * One separable pass of Pillow's antialiased resampling for 8-bit channels (ImagingResample, the arithmetic behind
 * PIL.Image.resize that transformers' CLIPImageProcessor -- the feature_extractor of StableDiffusionSafetyChecker --
 * and BlipImageProcessor call; SURVEY 8a: a7.9, a8):
 *   dst[(o*out_len + t)*inner + i] = clip8(((1 << 21) + sum_{k < bounds[t][1]} src[(o*in_len + bounds[t][0] + k)*inner + i]
 *                                           * coeffs[t][k]) >> 22)
 * bounds [out_len][2] = (first input sample, sample count <= ksize), coeffs [out_len][ksize] = the filter weights in
 * 22-bit fixed point -- both DEVICE int32 tables prepared by the host (they depend only on the sizes).  A horizontal
 * pass over [n][H][W][3] is outer = n*H, inner = 3; a vertical pass is outer = n, inner = W*3.  A crop is folded in by
 * passing only the table rows of the wanted outputs. */
int saspa_resample_u8(const uint8_t* src, uint8_t* dst, long long outer, int in_len, int out_len, int inner,
                      const int* bounds, const int* coeffs, int ksize, void* stream);
/* u8 RGB [npix][3] -> [npix][8] activations ((x/255) - mean[c]) / std[c], pad channels zero
 * (CLIPImageProcessor rescale + normalize; SURVEY 8a: a7.9) */
int saspa_u8_to_act_norm(int dtype, const uint8_t* src, void* dst, long long npix, float mean0, float mean1, float mean2,
                         float std0, float std1, float std2, void* stream);
/* Pillow's convert("L").convert("RGB") (the grey conversion in front of the LPIPS filter, all_utils/utils.py:577-578): u8 RGB
 * [npix][3] -> u8 [npix][3] with all three channels = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  Integer exact; src == dst allowed. */
int saspa_u8_luma(const uint8_t* src, uint8_t* dst, long long npix, void* stream);

/* StableDiffusionSafetyChecker decision + black-out on the device (no host round trip; SURVEY 8a: a7.9):
 * dots [nimg][ldd] = image embedding . unit(special-care | concept embeddings) (special-care columns first),
 * gram [nimg][ldg] = e e^T (diagonal = |e|^2), both fp32 GEMM outputs; special_w / concept_w = the fp64 thresholds.
 * Per image, in fp64 and upstream's order: cos = dot/|e|; a special-care score cos - w >= threshold sets the 0.01
 * adjustment; the image is flagged when any concept score cos - w + adjustment >= threshold, where `threshold` is
 * the smallest double t with Python's round(t, 3) > 0 (the host computes it once).  flags[i] = 0/1; the bytes of a
 * flagged image (bytes_per_image, multiple of 16) are zeroed -- upstream's black image. */
int saspa_safety_decide(const float* dots, int ldd, const float* gram, int ldg, int nimg, const double* special_w,
                        int n_special, const double* concept_w, int n_concepts, double threshold, uint8_t* images,
                        long long bytes_per_image, int* flags, void* stream);

/* CFG + one UniPCMultistepScheduler step (run_aug/run_aug.py:218-219 `sampler="unipcmultistep"`): eps, x:
 * [2*nimg][hw][8]; state: [3][nimg][hw][8] = last sample | newest x0-prediction | the one before (zero-initialised by the
 * caller).  The 12-float row (saspa_aug_amd/scheduler.py UniPCMultistepScheduler.plan) comes from `row` (host pointer) or,
 * when `table` is non-NULL, from row *index of a device table (hipGraph replays):
 *   x0 = (x - r1 * e) * r0;  if r2: x = r3*last + r4*m0 + r5*m1 + r6*x0;  m1, m0, last = m0, x0, x;  x = r7*x + r8*m0 + r9*m1 */
int saspa_cfg_unipc_step(int dtype, const void* eps, void* x, void* state, int nimg, long long hw, int C, int ldc, float guidance,
                         const float* row, const float* table, const int* index, void* stream);
/* the same update without classifier-free guidance (sd_xl-turbo at guidance_scale 0 with sampler = "unipcmultistep",
 * run_aug/run_aug.py:223-226, :567-571): eps / x are [nimg][hw][ldc], nothing is duplicated.  ABI 11. */
int saspa_unipc_step(int dtype, const void* eps, void* x, void* state, int nimg, long long hw, int C, int ldc,
                     const float* row, const float* table, const int* index, void* stream);

/* ---- v-prediction forms of the DDIM / UniPC steps (scheduler prediction_type "v_prediction": the 768-pixel
 * stabilityai/stable-diffusion-2-1 checkpoint).  `v` is the network output in the layout `eps` has above; all other
 * arguments, the host-side checks and their error codes are those of the epsilon entry point of the same name.
 *   v = vu + g (vc - vu)                                  (guidance on v, the order of the epsilon kernels' guidance line)
 *   DDIM:  x0 = sqrt(a_t) x - sqrt(1-a_t) v;  e = sqrt(a_t) v + sqrt(1-a_t) x;  x' = sqrt(a_p) x0 + sqrt(1-a_p) e
 *   UniPC: x0 = r10 * x - r1 * v  (r10 = alpha_t, r1 = sigma_t; r0 is not read), then the update of saspa_cfg_unipc_step
 * fp32 arithmetic in this order, one rounding to the storage type; an element's result does not depend on the launch.
 * saspa_ddim_step_v_dev serves both the CFG (cfg = 1) and the plain (cfg = 0) form, as saspa_ddim_step_dev.  ABI 20. */
int saspa_cfg_ddim_step_v(int dtype, const void* v, void* x, int nimg, long long hw, int C, int ldc, float guidance,
                          float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, void* stream);
int saspa_ddim_step_v(int dtype, const void* v, void* x, int nimg, long long hw, int C, int ldc, float sqrt_a_t,
                      float sqrt_1m_a_t, float sqrt_a_prev, float sqrt_1m_a_prev, void* stream);
int saspa_ddim_step_v_dev(int dtype, const void* v, void* x, int nimg, long long hw, int C, int ldc, int cfg, float guidance,
                          const float* coefs, const int* index, void* stream);
int saspa_cfg_unipc_step_v(int dtype, const void* v, void* x, void* state, int nimg, long long hw, int C, int ldc, float guidance,
                           const float* row, const float* table, const int* index, void* stream);
int saspa_unipc_step_v(int dtype, const void* v, void* x, void* state, int nimg, long long hw, int C, int ldc,
                       const float* row, const float* table, const int* index, void* stream);

/* SDEdit / img2img start latents (StableDiffusionControlNetImg2ImgPipeline.prepare_latents): per 8-channel
 * latent pixel, moments = AutoencoderKL.encode's quant_conv output (mean | logvar), e1 / e2 = the two generator draws:
 * out = sa * ((mean + exp(0.5 * clamp(logvar, -30, 20)) * e1) * scaling) + s1m * e2, pad channels zero. */
int saspa_vae_sample_noise(int dtype, const void* moments, const void* e1, const void* e2, void* out, long long npix,
                           float scaling, float sa, float s1m, void* stream);

/* ---- filter stage (all_utils/utils.py:306-323, :357-375) ----------------------------------------------
 * 2-D pooling over channels-last activations [batch][hin][win][C] -> [batch][hout][wout][C], hout = (hin + 2*pad - k) /
 * stride + 1: mode 0 = max (nn.MaxPool2d(3, 2, 1) of the ResNet stem: padding never wins), mode 1 = average over the k*k
 * window (nn.AvgPool2d(k): CLIP's anti-aliased strides, the attention pool's mean token; pad must be 0).  C % 8 == 0. */
int saspa_pool2d(int dtype, int mode, const void* x, int ldx, void* y, int ldy, int batch, int hin, int win, int C, int k,
                 int stride, int pad, void* stream);
/* Bilinear-attention-pooling tail of WSDAN_CAL (fgvc/models/cal.py:73-77): per row of [rows][C],
 * y = sign(x) * sqrt(|x| + eps); out = scale * y / max(||y||_2, 1e-12).  fp32 in / out. */
int saspa_signsqrt_l2norm(const float* x, long long ldx, float* y, long long ldy, int rows, long long C, float eps,
                          float scale, void* stream);
/* One feature level of LPIPS (Zhang et al. 2018; lpips v0.1 `normalize_tensor` + `lin` + spatial average) for a batch of pairs, the
 * distance behind the reference's lpips_min / lpips_max filter (all_utils/utils.py:377-381, :576-590):
 *   dist[j] (+)= 1/hw * sum_p sum_c w[c] * (a[j][p][c] / (|a[j][p]|_2 + 1e-10) - r[i][p][c] / (|r[i][p]|_2 + 1e-10))^2,  i = ref_index[j]
 * a: [n][hw][lda], r: [m][hw][ldr] channels-last features as saspa_gemm leaves them (SASPA_BF16 or SASPA_F32 storage; fp32 arithmetic),
 * w: C non-negative fp32 weights, ref_index: n DEVICE int32 (NOT validated here: the caller guarantees 0 <= ref_index[j] < m),
 * dist: n fp32, overwritten (accumulate == 0) or added to (accumulate != 0: the five levels sum into one vector).
 * workspace: n * SASPA_LPIPS_MAX_BLOCKS fp32 of scratch (per-workgroup partial sums; reduced in a fixed order by a second launch).
 * C % 8 == 0, C <= SASPA_LPIPS_MAX_C, pitches % 8 == 0 and >= C, 16-byte aligned bases, n <= 65535.  The difference form is
 * evaluated as written (no expanded products): d(x, x) == 0.0 exactly and an all-zero pixel vector contributes 0.  No atomics; how a
 * pair's pixels are cut over workgroups depends on (hw, C) only, so dist[j] is bit-identical from run to run, for every batch size
 * and every position of the pair in the batch. */
#define SASPA_LPIPS_MAX_C 512
#define SASPA_LPIPS_MAX_BLOCKS 64
int saspa_lpips_layer(int dtype, const void* a, int lda, const void* r, int ldr, const int* ref_index, const float* w, float* dist,
                      float* workspace, int n, int hw, int C, int accumulate, void* stream);
/* The class head of a filter decision: one row of class logits, its softmax and the entries a decision looks at, on the device --
 * the per-class CLIP filter of the Real-Guidance baseline (all_utils/utils.py:180-191, :383-393: softmax over ALL class prompts, the
 * source image's class >= 1 / n_classes / discount) and the too-high-confidence test on the baseline classifier's logits (:368-373).
 * One launch per batch, one workgroup of 256 threads per row, fp32 throughout.
 *   embedding mode (cls != NULL): feat [rows][ldf] = UNNORMALISED image embeddings of width D, cls [C][ldc] = unit text rows;
 *       u = feat / sqrt(sum feat^2) (normalize != 0; feat as it is otherwise),  z_c = scale * sum_d u_d cls[c][d]
 *   logits mode (cls == NULL, D == C): feat [rows][ldf] holds the logits,  z_c = scale * feat[c]
 * labels: rows DEVICE int32.  Per row:
 *   stats[4 * row + 0..3] = z_label,  p_label = exp(z_label - m) / sum_c exp(z_c - m) with m = max_c z_c,  m,  log-sum-exp of the row
 *   idx[2 * row + 0..1]   = argmax (the LOWEST c with z_c == m),  the number of c with z_c strictly greater than z_label
 *   logits [rows][ldl] (optional, may be NULL) = z
 * A label outside [0, C) cannot be seen from the host: that row gets four NaN statistics and two -1 indices (its logits are still
 * written).  Every sum has a fixed shape (lanes stride the row, xor-butterflies inside a wave, the four waves in order through
 * LDS); no atomics; a row never looks at another row, so its results are bit-identical from run to run, for every batch size and
 * every position in the batch.
 * Host-side validation: null feat / labels / stats / idx or rows < 1 -> SASPA_EINVAL; feat / cls / logits not 16-byte aligned,
 * ldf / ldc / ldl not multiples of 4 or shorter than the row, stats / idx / labels not 4-byte aligned -> SASPA_EALIGN;
 * C < 1, D < 1, D > SASPA_CLASS_HEAD_MAX_D, C > SASPA_CLASS_HEAD_MAX_C (the LDS plan: the embedding and the row of logits are
 * resident, 4 * (D + C) bytes), or D != C in logits mode -> SASPA_ERANGE.  (CLIP RN50: D = 1024; the largest class list of the
 * reference's datasets: C = 431.) */
#define SASPA_CLASS_HEAD_MAX_D 2048
#define SASPA_CLASS_HEAD_MAX_C 4096
int saspa_class_head(const float* feat, int ldf, const float* cls, int ldc, const int* labels, float scale, int normalize,
                     float* stats, int* idx, float* logits, int ldl, int rows, int D, int C, void* stream);
/* The in-line filter stage (Settings.FILTER_INLINE): one threshold-free score record per augmented image, written while the batch is
 * still on the device; `filters.decide` makes every decision of the post-hoc stage from the records, on the host, for any top_k /
 * too_high / discount / semantic setting.  One launch per batch, one wave per image.  Row slot[b] of table [n_rows][8] fp32 becomes
 *   0 valid          bit 0 semantic, bit 1 confidence, bit 2 per-class: which of the fields below were recorded (an exact float)
 *   1 sem_argmax     numpy's argmax of sem[b][0..P): equal logits give the lowest index, a NaN counts as the maximum, the first one wins
 *   2 sem_margin     sem[b][0] - max(sem[b][1..P)) as one fp32 subtraction; +inf when P == 1; every NaN result is the canonical quiet NaN
 *   3 conf_n_greater (float)conf_idx[2 b + 1]   4 conf_p_label  conf_stats[4 b + 1]     (saspa_class_head in logits mode)
 *   5 pc_p_label     pc_stats[4 b + 1]           6 pc_n_greater  (float)pc_idx[2 b + 1]  (saspa_class_head in embedding mode)
 *   7 reserved, 0
 * sem (fp32 [rows][ld], P <= SASPA_FILTER_RECORD_MAX_P prompts, one lane each), the (conf_stats, conf_idx) pair and the (pc_stats,
 * pc_idx) pair are each optional: NULL = that filter is off, its fields are NaN and its valid bit is clear.  bad (optional, rows
 * bytes): a non-zero bad[b] gives valid = 0 and NaN fields.  slot: rows DEVICE int32, distinct, each in [0, n_rows) -- the CALLER
 * checks them (ops.filter_record does, on the host, before anything is uploaded); a slot outside the table is dropped, not written.
 * The (value, index) reduction is an xor butterfly over a total order, so the record does not depend on the batch size or on the
 * image's place in the batch.  Plain stores, no atomics, no row but slot[b] is touched, the host is not read.
 * Host-side validation: null slot / table, rows < 1, n_rows < 1 or half a (stats, idx) pair -> SASPA_EINVAL; P < 1, P >
 * SASPA_FILTER_RECORD_MAX_P, ld < P or rows > n_rows -> SASPA_ERANGE; table not 16-byte, another pointer not 4-byte aligned ->
 * SASPA_EALIGN. */
#define SASPA_FILTER_RECORD_MAX_P 64
int saspa_filter_record(const float* sem, int ld, int P, const float* conf_stats, const int* conf_idx, const float* pc_stats,
                        const int* pc_idx, const unsigned char* bad, const int* slot, float* table, int n_rows, int rows, void* stream);

/* ---- cv2.resize, 8-bit RGB [n][h][w][3] -> [n][dh][dw][3] (all_utils/utils.py:58-79 `resize_image`) -------
 * saspa_resize_taps_u8: OpenCV's separable fixed-point filters; xofs / yofs = first tap index per destination sample,
 * xw / yw = ntaps 11-bit weights per destination sample.  mode 0 = INTER_LANCZOS4 (ntaps 8), mode 1 = the 8-bit bilinear
 * code INTER_AREA falls back to when a side is up-scaled (ntaps 2).  Out-of-image taps are clamped (replicate).
 * saspa_resize_area_u8: INTER_AREA down-scaling.  isx, isy > 0: integer scale factors (resizeAreaFast_), tables unused;
 * otherwise CSR-style tables from computeResizeAreaTab: destination sample d owns entries [start[d], start[d+1]) of
 * (source index, float weight); accumulation order and float roundings follow resizeArea_<uchar, float>. */
int saspa_resize_taps_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int dh, int dw, const int* xofs,
                         const short* xw, const int* yofs, const short* yw, int ntaps, int mode, void* stream);
int saspa_resize_area_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int dh, int dw, const int* xstart,
                         const int* xsi, const float* xalpha, const int* ystart, const int* ysi, const float* ybeta,
                         int isx, int isy, void* stream);

/* library self-description */
/* ---- fp8 (OCP e4m3) W8A8 linears (BASELINE.json configs[4] "fp8 MFMA") ------------------------------------
 * saspa_layernorm_quant_fp8: LayerNorm over the last dim of bf16 x [rows][C] (C <= 2048), then per-row quantisation:
 *   scale[r] = max|y[r][:]| / 448, q[r][c] = e4m3(y[r][c] / scale[r])      (BasicTransformerBlock.norm2 / norm3 feeding
 *   attn2.to_q / ff.net.0.proj on the fp8 path; the normalised bf16 tensor is never written).
 * saspa_gemm_fp8: out[m][n] = act(sa[m] * sw[n] * sum_k a[m][k] * w[n][k] + bias[n]) (+ residual[m][n]), a / w e4m3 bytes
 *   (row pitches lda / ldw in bytes = elements, multiples of 16), K and N multiples of 128, sa per row (the quantiser's
 *   scales), sw per output channel (weights.quantize_fp8), out / residual bf16; act = SASPA_ACT_NONE or SASPA_ACT_GEGLU
 *   (rows of w regrouped per 128-column tile: 64 values then their 64 gates; out has N / 2 columns).  128x128 tiles on
 *   v_mfma_f32_16x16x128_f8f6f4, fp32 accumulation. */
typedef struct SaspaGemmF8Params {
  const void* a; int lda;
  const void* w; int ldw;
  int M, N, K;
  const float* sa; const float* sw; const float* bias;
  const void* residual; int ldr;
  int act;
  void* out; int ldo;
  /* ABI 20 (configs[4] breadth: self-attention Q|K|V and the feed-forward OUTPUT projection on fp8 tiles too) */
  int sa_broadcast;        /* 1: `sa` is ONE fp32 scale for every row (an activation tensor quantised under a tensor-wide scale) */
  int out_fp8;             /* GEGLU only. 1: `out` receives e4m3 BYTES, out[m][n] = sat(gelu-gated value / *out_scale), ldo in bytes
                            * (% 16): BasicTransformerBlock.ff.net.0 -> ff.net.2 without a bf16 round trip or a quantisation pass */
  const float* out_scale;  /* device scalar read by the launch (required with out_fp8); a power of two keeps e4m3 rounding scale-free */
  float* amax;             /* GEGLU only, optional device scalar: atomic max of |gated value| over the launch (calibration of out_scale) */
} SaspaGemmF8Params;
int saspa_gemm_fp8(const SaspaGemmF8Params* p, void* stream);
/* Calibration-free feed-forward (ff.net.0.proj -> ff.net.2 with no tensor-wide scale): the hidden state as MX e4m3, one E8M0
 * exponent per row and 32 columns.  Both take SaspaGemmF8Params as saspa_gemm_fp8 reads it, plus the exponent array; default
 * library only.
 * saspa_gemm_fp8_geglu_mx (producer): the GEGLU launch of saspa_gemm_fp8 up to and including the gated value y (same K loop, same
 *   acc * (sa * sw) + bias, same bf16 rounding of the tile); then for every row m < M and block b of 32 consecutive gated columns
 *   (N / 64 blocks per row): e = the smallest integer with max|y| <= 448 * 2^e, clamped to [-127, 127], 0 for an all-zero block (the
 *   rule of saspa_groupnorm_quant_mxfp8); qs[m][b] = e + 127 (uint8 at pitch ldqs), out[m][n] = e4m3fn(y * 2^-e) rounded to nearest
 *   even, bytes at pitch ldo.  Cannot saturate; no atomics; a row's bytes depend on that row alone; rows >= M write nothing.
 *   act must be SASPA_ACT_GEGLU and out_fp8 / out_scale / amax 0 / NULL (SASPA_EINVAL); ldo % 16, ldqs % 4, qs 4-byte aligned
 *   (SASPA_EALIGN); ldqs >= N / 64, no residual (SASPA_ERANGE).
 * saspa_gemm_mxfp8 (consumer): out[m][n] = bf16(sw[n] * sum_k 2^(qs[m][k / 32] - 127) a[m][k] w[n][k] + bias[n]) (+ residual[m][n]),
 *   the exponent applied inside v_mfma_scale_f32_16x16x128_f8f6f4 as the activation-side scale operand (weight side 127).  sa must
 *   be NULL, act SASPA_ACT_NONE, out_fp8 / out_scale / amax 0 / NULL (SASPA_EINVAL); K and N multiples of 128 (SASPA_ERANGE);
 *   ldqs % 4, qs 4-byte aligned (SASPA_EALIGN: the four exponents of a row's K-tile are one aligned dword); ldqs >= K / 32
 *   (SASPA_ERANGE).  Rows >= M of qs are never read.  Tile shape, ring, XCD order and epilogue of saspa_gemm_fp8. */
int saspa_gemm_fp8_geglu_mx(const SaspaGemmF8Params* p, void* qs, int ldqs, void* stream);
int saspa_gemm_mxfp8(const SaspaGemmF8Params* p, const void* qs, int ldqs, void* stream);
int saspa_layernorm_quant_fp8(const void* x, int ldx, void* q, int ldq, float* scale, long long rows, int C,
                              const float* gamma, const float* beta, float eps, void* stream);

/* ---- MX-fp8 3x3 convolutions (block-scaled e4m3; opt-in fp8 conv path of ResnetBlock2D conv1 / conv2) --
 * saspa_groupnorm_quant_mxfp8: GroupNorm(+SiLU) exactly as saspa_groupnorm_apply takes it (one or two bf16 sources, statistics from
 *   the producers' epilogues or from saspa_groupnorm_stats, act NONE / SILU; p->y is not read), quantised instead of stored:
 *   y = act((x - mean) * rstd * gamma + beta) in fp32 (the apply pass's arithmetic); for every pixel and block of 32 consecutive
 *   channels, e = the smallest integer with max|y| <= 448 * 2^e, clamped to [-127, 127] (0 for an all-zero block);
 *   qs[pixel][block] = e + 127 (E8M0), q[pixel][c] = e4m3fn(y * 2^-e) rounded to nearest even (cannot saturate).
 *   q: uint8 [batch * hw][C] at pitch ldq bytes (% 16), qs: uint8 [batch * hw][C / 32] at pitch ldqs.  bf16, C = c0 + c1,
 *   C % 32 == 0, C <= 4096; SASPA_ERANGE / SASPA_EALIGN otherwise.  Deterministic, no atomics; an image's bytes depend on it alone.
 * saspa_conv3x3_mxfp8: 3x3 / stride 1 / pad 1 conv of ONE such (q, qs) source with e4m3 weights w8 [N][ldw] (K = tap * C + c as
 *   weights.pack_conv orders it, zero padded to Kp = 9 C rounded up to a multiple of 128) and per-output-channel fp32 scales sw [N]:
 *   out[m][n] = bf16(sw[n] * sum_k 2^(qs - 127) q[m][k] w8[n][k] + bias[n] + rowvec[b(m)][n]) + residual[m][n]   (bf16 out /
 *   residual, the exponent of the (pixel, tap, block) a k belongs to applied inside v_mfma_scale_f32_16x16x128_f8f6f4; taps
 *   outside the image contribute zero).  gn_stats / gn_unit: exactly SaspaGemmParams.gn_stats (160-column tiles).
 *   C % 32 == 0, N % 160 == 0, any M (row tail masked), kh = kw = 3, stride 1, pad 1, no upsampling -- SASPA_ERANGE otherwise;
 *   16-byte aligned operands, ldq / ldw % 16, ldo / ldr % 8 -- SASPA_EALIGN otherwise.  No split-K.
 * saspa_conv3x3_mxfp8_eligible: non-zero if the shapes, pitches and the alignment of the pointers given are accepted. */
typedef struct SaspaConvMxParams {
  const void* q; int ldq;        /* e4m3 activations [batch * h * w][C], pitch in bytes */
  const void* qs; int ldqs;      /* E8M0 block exponents [batch * h * w][C / 32], pitch in bytes */
  int batch, h, w, C;            /* input extent = output extent */
  int kh, kw, stride, pad;       /* must be 3, 3, 1, 1 */
  int upsample;                  /* must be 0 */
  const void* w8; int ldw;       /* e4m3 weights [N][ldw] */
  int N, Kp;
  const float* sw;               /* [N] */
  const float* bias;             /* [N] or NULL */
  const float* rowvec; int ldrv; /* [batch or 1][N] or NULL (time-embedding projection) */
  const void* residual; int ldr; /* bf16 [M][ldr] or NULL */
  void* out; int ldo;            /* bf16 [M][ldo] */
  float* gn_stats; int gn_unit;
} SaspaConvMxParams;
int saspa_groupnorm_quant_mxfp8(const SaspaGroupNormParams* p, void* q, int ldq, void* qs, int ldqs, void* stream);
int saspa_conv3x3_mxfp8_eligible(const SaspaConvMxParams* p);
int saspa_conv3x3_mxfp8(const SaspaConvMxParams* p, void* stream);

/* ---- HED annotator head (run_aug/run_aug.py:311-312, :438-439 -> controlnet_aux HEDdetector.__call__) -------
 * The network's conv stack runs as saspa_gemm / saspa_pool2d launches; this is what follows it: side output k
 * ([n][mh][mw] fp32 samples at element pitch ld -- channel 0 of a channel-padded NHWC tensor) is resized to H x W like
 * cv2.resize(INTER_LINEAR) on float32 (xofs [W] first source column, xw [W][2] weights; yofs [H][2] the two clamped source
 * rows, yw [H][2] weights: host tables), the nmaps results are averaged in float32 in order, then
 * u8 = trunc(clip(255 / (1 + exp(-mean)), 0, 255)) in fp64, written to all three channels of dst [n][H][W][3]. */
typedef struct SaspaHedFuseParams {
  int nmaps, n, H, W;
  const float* map[5]; int mh[5], mw[5], ld[5];
  const int* xofs[5]; const float* xw[5];
  const int* yofs[5]; const float* yw[5];
  uint8_t* dst;
} SaspaHedFuseParams;
int saspa_hed_fuse(const SaspaHedFuseParams* p, void* stream);

/* ---- cross-attention half of a level-0 transformer block in one launch (ABI 16) --------------------------------------
 * out = residual + to_out( softmax( to_q(LayerNorm(x)) K^T ) V ) + bias for C = 320 channels, 8 heads of 40 and nk <= 96 keys:
 * BasicTransformerBlock.norm2 -> attn2.to_q -> scaled_dot_product_attention over the text tokens -> attn2.to_out.0 -> residual
 * (diffusers attention.py / attention_processor.py; the reference reaches it through pipe(), run_aug/run_aug.py:278).
 * Replaces three launches (LayerNorm + to_q, flash attention, to_out + residual) that each stream the [M, 320] token matrix.
 * Operands in the layouts the kernel's MFMA chain consumes (saspa_aug_amd/weights.py: pack_xattn_*; built once):
 *   w    [640][ldw >= 320] bf16: rows 0..319 = to_q rows (softmax scale * log2 e folded in) ordered [heads 0-7: channels 0-31 |
 *        heads 0-7: channels 32-39]; rows 320..639 = to_out with its K columns in the order the attention stage emits them.
 *   bias [640] fp32: 320 zeros, then the to_out bias.
 *   kf / vf: per sample (byte strides kf_stride >= 73 728, vf_stride >= 98 304) the text K and V^T of this block cut into
 *        MFMA A-operand fragments [head][key block 3][K-step 3][lane 64][8 bf16] and [head][channel block 2][K-step 6][lane 64][8 bf16]
 *        (zero-padded; V^T row 40 of every head = 1.0: the softmax denominator rides the same MFMAs).  Time-invariant.
 * M % 256 == 0, rows_per_sample % 256 == 0 (a workgroup's 256 rows share one sample's keys), all pitches % 8 == 0,
 * 16-byte aligned operands, 32-bit byte offsets (M * pitch * 2 < 2 GiB); SASPA_ERANGE / SASPA_EALIGN otherwise. */
typedef struct SaspaXattnBlockParams {
  const void* x;             /* [M][ldx] bf16: the block's hidden states (LayerNorm input) */
  int ldx;
  const void* residual;      /* [M][ldr] bf16: added to the result (the reference adds x itself) */
  int ldr;
  long long M;
  int rows_per_sample;       /* tokens per sample (H/8 * W/8) */
  const float* ln_gamma;     /* [320] */
  const float* ln_beta;
  float ln_eps;
  const void* w;             /* [640][ldw] bf16, see above */
  int ldw;
  const float* bias;         /* [640] */
  const void* kf;
  long long kf_stride;       /* bytes per sample */
  const void* vf;
  long long vf_stride;
  int nk;                    /* valid keys (77) */
  void* out;                 /* [M][ldo] bf16 */
  int ldo;
} SaspaXattnBlockParams;
int saspa_xattn_block(const SaspaXattnBlockParams* p, void* stream);
/* The same launch reading a SHARED x / residual of x_rows rows (the parameter struct is unchanged): output row r reads x / residual
 * row r % x_rows, its keys are those of sample r / rows_per_sample as above; out, kf and vf cover M rows.  Under classifier-free
 * guidance the unconditional and the conditional half of a batch share the hidden states up to the first cross-attention and differ
 * in the text keys only: x_rows = M / 2 lets that prefix run once per image (models._Net.encode(cfg_pair=True)).
 * x_rows > 0 (SASPA_EINVAL), x_rows % rows_per_sample == 0 and M % x_rows == 0 (SASPA_ERANGE); the 32-bit offset limit holds for
 * x / residual over x_rows rows and for out over M rows.  x_rows == M is saspa_xattn_block, which is a call of this function. */
int saspa_xattn_block_bcast(const SaspaXattnBlockParams* p, long long x_rows, void* stream);

/* ---- measurement aid (ABI 20): effective shader clock under load ------------------------------------------------------
 * One sleeping wave measures s_memtime (shader clocks) against s_memrealtime (constant 100 MHz) over iters x s_sleep 127
 * (about 4 us each at 2 GHz; 1 <= iters <= 100000) and writes out2[0] = shader clocks, out2[1] = 100 MHz ticks:
 * clock [MHz] = 100 * out2[0] / out2[1].  bench.py launches it on a side stream while the timed region runs, so that the
 * record of a run carries the clock the box's power management granted it (MI355X_MICROARCH.md: MFMA-dense loops are
 * power-limited and boxes differ by up to 12 %).  No counterpart in the reference (it reports no clocks). */
int saspa_clock_probe(unsigned long long* out2, int iters, void* stream);

/* ---- feed-forward half of a level-0 transformer block in one launch (ABI 20) ---------------------------------------------
 * out = residual + W2 ( v * gelu(g) ) + b2 with [v ; g] = W1 LayerNorm(x) + b1, for C = 320 channels and an inner width F (1 280):
 * BasicTransformerBlock.norm3 -> ff.net.0 (GEGLU) -> ff.net.2 -> residual add (diffusers attention.py; the reference reaches it
 * through pipe(), run_aug/run_aug.py:278).  Replaces two launches (LayerNorm + GEGLU projection, output projection + residual)
 * whose [M, F] hidden state made an HBM round trip.  Operands in the layouts the kernel's MFMA chain consumes (weights.pack_ff_block):
 *   w1  [2 F][ldw1 >= 320] bf16: per slice t of 32 hidden features rows 64 t .. 64 t + 31 = the VALUE rows of features 32 t .. 32 t + 31
 *       (ff.net.0.proj.weight rows f), rows 64 t + 32 .. 64 t + 63 = their GATE rows (rows F + f);  b1 [2 F] fp32 in the same order.
 *   w2f [F / 32][10][2][64][8] bf16: ff.net.2.weight as MFMA A-operand fragments -- fragment (t, nb, s), lane (m, h = lane >> 5),
 *       element e = W2[32 nb + m][32 t + 16 s + (e & 3) + 8 (e >> 2) + 4 h];  b2 [320] fp32.
 * M % 128 == 0, F % 32 == 0, pitches % 8 == 0, 16-byte aligned operands, 32-bit byte offsets; ln_gamma / ln_beta NULL = no LayerNorm.
 * Two forms of the same arithmetic (bit-identical results): the wave-specialised one (8 waves: 4 keep the token rows and run LayerNorm /
 * the first projection / the gate, 4 keep the output accumulators and run the second projection / the epilogue) is the default;
 * SASPA_FF_WS=0 in the environment (read per launch) selects the four-wave form (slower; kept as a cross-check).
 * saspa_ff_block_eligible: host-side check of the geometry (1 = can run). */
typedef struct SaspaFfBlockParams {
  const void* x;             /* [M][ldx] bf16: the block's hidden states (LayerNorm input) */
  int ldx;
  const void* residual;      /* [M][ldr] bf16: added to the result (the reference adds x itself) */
  int ldr;
  long long M;
  int F;                     /* inner width (hidden features after the gate): 4 x 320 */
  const float* ln_gamma;     /* [320] or NULL */
  const float* ln_beta;
  float ln_eps;
  const void* w1;
  int ldw1;
  const float* b1;
  const void* w2f;
  const float* b2;
  void* out;                 /* [M][ldo] bf16 */
  int ldo;
} SaspaFfBlockParams;
int saspa_ff_block(const SaspaFfBlockParams* p, void* stream);
int saspa_ff_block_eligible(const SaspaFfBlockParams* p);

/* ---- PNG encode on the device: row filters + Huffman-only deflate (opt-in, DESIGN "PNG encode on the device") ----
 * px: contiguous u8 [n][H][W][C], C = 3 (RGB) or 1 (grey).  Per image a complete ZLIB STREAM of the PNG-filtered rows is written to
 * streams + i * capacity and its length to sizes[i]: 78 01, deflate blocks, big-endian Adler-32 of the filtered bytes.  The host only
 * frames it (IHDR, one IDAT with its CRC-32, IEND).
 *   rowbytes = 1 + W * C (filter type byte + residuals); an image is cut into segments of R = SASPA_PNG_SEG_ROWS(rowbytes) rows (the last
 *   one may be shorter), one workgroup each, <= 32767 bytes.  Per row the filter (None, Sub, Up, Average, Paeth; bpp = C, zeros above row
 *   0) with the smallest sum |int8(residual)| is kept, ties to the lowest type; the row above a segment comes from the raw image.
 *   Per segment ONE dynamic-Huffman block of literals only (no match search): 286 literal/length code lengths sent as 4-bit codes of a
 *   flat code-length alphabet (header of 1222 bits), lengths from the integer construction of DESIGN.md, canonical codes.  A segment that
 *   is not the last ends with an empty stored block (000, pad, 00 00 FF FF) so that every segment starts on a byte; a segment whose
 *   Huffman form would take >= segbytes + 5 bytes is one stored block of exactly segbytes + 5.  Hence
 *       capacity(H, W, C) = 2 + H * rowbytes + 5 * ceil(H / R) + 4            (saspa_png_capacity; never exceeded)
 *   A second launch moves the segments to the front of the slot, folds the segments' Adler partial sums and writes sizes[i].
 * Deterministic: an image's bytes depend on its pixels alone (integer arithmetic; the atomics are integer adds / ors whose result does
 * not depend on their order), for every batch size and position in the batch.  Nothing outside [i * capacity, i * capacity + the slot's
 * capacity) is written.
 * saspa_png_capacity / saspa_png_workspace launch nothing: bytes per slot / of `workspace`, or a SASPA_E* code.
 * Host-side validation, before any launch: null px / streams / sizes / workspace, n, H, W < 1 -> SASPA_EINVAL; workspace not 16-byte or
 * sizes not 4-byte aligned -> SASPA_EALIGN; C not 1 or 3, rowbytes > 32767, capacity / workspace_bytes smaller than the two functions
 * say, a slot of 2 GiB or more -> SASPA_ERANGE. */
#define SASPA_PNG_SEG_ROWS(rowbytes) (32767 / (rowbytes) < 1 ? 1 : (32767 / (rowbytes) > 16 ? 16 : 32767 / (rowbytes)))
long long saspa_png_capacity(int H, int W, int C);
long long saspa_png_workspace(int n, int H, int W, int C);
int saspa_png_deflate(const uint8_t* px, int n, int H, int W, int C, uint8_t* streams, long long capacity, int* sizes,
                      void* workspace, long long workspace_bytes, void* stream);

/* ---- caption decoder (csrc/saspa_decode.hip; default library only) ----
 * One new token per row against a key/value cache: out[r] = softmax(scale * q[r] K^T) V per head, one query row each.
 *   q / out: [rows, heads * d] (pitches ldq / ldo).  k / v: caches [entries, nk_max, heads * d], row-major (V is NOT transposed),
 *   key pitch ldk / ldv, entry stride ske / sve (elements).  Row r reads entry r / group: group = 1 is self-attention (an entry per
 *   beam row), group = beams is cross-attention (the beams of an image share its K / V, loaded once per workgroup).
 *   len: int32 per row on the device, keys < len[r] are live (clamped to [0, nk]; 0 gives a zero row); NULL = all nk keys.  Keys at or
 *   beyond a row's length are never read for it.
 * Arithmetic: products and sums in fp32 in a fixed order (a logit over d ascending; the maximum and the sum over a fixed lane / stride
 * pattern; P V over key slices, then the slices ascending), scale multiplies the fp32 logit, expf, one division by the sum, ONE
 * rounding to the storage type.  No atomics; a row's result does not depend on the other rows of the launch.
 * dtype SASPA_BF16 or SASPA_F32.  Before any launch: null q / k / v / out, rows / heads / nk / entries < 1, entries * group < rows, a
 * pitch shorter than heads * d -> SASPA_EINVAL; d % 8 != 0, d > 128, nk > 1024, group outside 1 .. 8 -> SASPA_ERANGE; pointers not
 * 16-byte aligned, pitches / entry strides not multiples of 16 bytes, len not 4-byte aligned -> SASPA_EALIGN. */
#define SASPA_DECODE_MAX_D 128
#define SASPA_DECODE_MAX_NK 1024
#define SASPA_DECODE_MAX_GROUP 8
typedef struct {
  int dtype;
  const void* q; int ldq;
  const void* k; int ldk; long long ske;
  const void* v; int ldv; long long sve;
  const int* len;
  void* out; int ldo;
  int rows, entries, heads, d, nk, group;
  float scale;
} SaspaDecodeAttnParams;
int saspa_decode_attn(const SaspaDecodeAttnParams* p, void* stream);

/* One beam-search step's selection, one workgroup per image.  logits: fp32 [images * group, ld], columns < vocab are live (columns
 * vocab .. ld - 1 are padding: loaded with their 16-byte chunk, never part of a maximum, a sum or a candidate).  Per row
 *   lp[t] = (x[t] - max) - log(sum_t exp(x[t] - max))      fp32, fixed order;
 * the candidate (row g of the image, token t) scores (ban_on && t == ban_token ? -inf : lp[t]) + scores[row], fp32.  Per image the
 * k = 2 * group best of the group * vocab candidates go to out_score[image][k] (descending) and out_idx[image][k][2] = (row in group,
 * token); ties go to the lowest flat index row * vocab + token.  -inf candidates (a row whose score is -inf, a banned token) are taken
 * last and never make a NaN; with fewer than k candidates the tail is (-inf, -1, -1).  No atomics; an image's result does not depend on
 * the rest of the batch.
 * Before any launch: null pointers, images / vocab < 1, ld < vocab -> SASPA_EINVAL; group outside 1 .. 8, group * vocab >= 2^31 ->
 * SASPA_ERANGE; logits not 16-byte aligned, ld % 4 != 0, scores / out_score / out_idx not 4-byte aligned -> SASPA_EALIGN. */
int saspa_logprob_topk(const float* logits, int ld, int vocab, int images, int group, const float* scores, int ban_token, int ban_on,
                       float* out_score, int* out_idx, void* stream);

/* ---- T5 key-to-text (csrc/saspa_t5.hip; default library only) ----
 * RMS norm (T5LayerNorm): out[r][c] = (x[r][c] * rs[r]) * gamma[c], rs[r] = 1 / sqrt(sum_c x[r][c]^2 / C + eps): no mean is
 * subtracted and there is no bias.  x / out: [rows, C] with pitches ldx / ldo (elements), gamma fp32 [C].
 * Arithmetic: fp32; a wave per row, lane l adds the squares of the 16-byte chunks l, l + 64, ... element by element in one fma chain,
 * then the 64-lane butterfly; IEEE division and square root; the two products in the order written; ONE rounding to the storage
 * type.  No atomics; a row's result does not depend on the other rows of the launch.
 * dtype SASPA_BF16 or SASPA_F32.  Before any launch: null x / out / gamma, another dtype, rows / C < 1, a pitch shorter than C, eps < 0
 * or NaN -> SASPA_EINVAL; C > 8192 -> SASPA_ERANGE; C % 8 != 0, x / out not 16-byte aligned, pitches not multiples of 16 bytes, gamma
 * not 4-byte aligned -> SASPA_EALIGN. */
#define SASPA_RMSNORM_MAX_C 8192
int saspa_rmsnorm(int dtype, const void* x, int ldx, void* out, int ldo, int rows, int C, const float* gamma, float eps, void* stream);

/* Attention of one query per row against a key/value cache with an additive relative-position bias: saspa_decode_attn's contract
 * (same cache layout [entries, nk_max, heads * d], row-major V, per-row len clamped to [0, nk] with 0 giving a zero row, keys at or
 * beyond a row's length never read for it) with three additions:
 *   rows_per_entry replaces group: row r reads entry r / rows_per_entry, 1 .. 1024 (the tokens of an encoder sequence are the rows of
 *     its entry; 1 is the cached decoder self-attention);
 *   pos: int32 per row on the device, the query's position;
 *   bias: fp32 [heads, ncol] with pitch ldb, and center.  The logit of key j for row r, head h is
 *       (q . k_j) * scale + bias[h][clamp(pos[r] - j + center, 0, ncol - 1)]
 *     the bias added in fp32 AFTER the scale; the column is formed in 64 bits and saturates at both ends (T5's buckets saturate beyond
 *     max_distance, so a table of 2 * max_distance + 1 columns (bidirectional, center = max_distance) or max_distance + 1 (causal,
 *     center = 0) is exact at any length).  The host builds the table; the kernel never evaluates the bucket function.
 * Arithmetic: as saspa_decode_attn (a logit over d ascending in one fma chain; the maximum and the sum over a fixed lane / stride
 * pattern; expf; P V over key slices, then the slices ascending; one division by the sum; ONE rounding to the storage type).  Rows of
 * an entry share a workgroup in blocks of 8, but each row's order of operations depends on its own len only.  No atomics; a row's
 * result does not depend on the other rows of the launch.
 * dtype SASPA_BF16 or SASPA_F32.  Before any launch: null q / k / v / out / pos / bias, rows / heads / d / nk / entries /
 * rows_per_entry / ncol < 1, entries * rows_per_entry < rows, a pitch shorter than heads * d, ldb < ncol -> SASPA_EINVAL; d % 8 != 0,
 * d > 128, nk > 1024, rows_per_entry > 1024 -> SASPA_ERANGE; pointers not 16-byte aligned, pitches / entry strides not multiples of
 * 16 bytes, len / pos / bias not 4-byte aligned -> SASPA_EALIGN. */
#define SASPA_RELBIAS_MAX_D 128
#define SASPA_RELBIAS_MAX_NK 1024
#define SASPA_RELBIAS_MAX_ROWS 1024
typedef struct {
  int dtype;
  const void* q; int ldq;
  const void* k; int ldk; long long ske;
  const void* v; int ldv; long long sve;
  const int* len;
  const int* pos;
  const float* bias; int ldb, ncol, center;
  void* out; int ldo;
  int rows, entries, heads, d, nk, rows_per_entry;
  float scale;
} SaspaAttnRelbiasParams;
int saspa_attn_relbias(const SaspaAttnRelbiasParams* p, void* stream);

/* One sampling step, one workgroup per row of fp32 logits [rows, ld] (columns vocab .. ld - 1 are padding: loaded with their 16-byte
 * chunk, never a candidate).  In the order of transformers' warpers (temperature, top-k, top-p), all fp32:
 *   y[t] = x[t] / temperature (IEEE division);
 *   the min(top_k, vocab) largest y are kept, ordered by y descending, ties to the lowest token id;
 *   e[i] = expf(y[i] - y[0]) in that order, z = their sum ascending;
 *   top_p < 1: the shortest prefix whose running sum of e[i] / z reaches top_p (>=) is kept, at least one token;
 *   s = the sum of the kept e[i] ascending; the result is the first kept token whose running sum of e[i] / s exceeds u[r] (>), the
 *   last kept token if rounding leaves none; out_logp[r] = logf(e[i] / s), its log-probability under the kept distribution.
 * u: one fp32 uniform in [0, 1) per row, on the device.  This does NOT reproduce torch.multinomial's random stream: what it
 * reproduces is the kept set, the kept probabilities and an inverse-CDF draw on the supplied uniform.  top_k = 1 is the argmax
 * (greedy) whatever u is.  No atomics; a row's result does not depend on the other rows of the launch.
 * Before any launch: null pointers, rows / vocab < 1, ld < vocab, temperature not in (0, inf), top_p not in (0, 1] -> SASPA_EINVAL;
 * top_k outside 1 .. 64 -> SASPA_ERANGE; logits not 16-byte aligned, ld % 4 != 0, u / out_tok / out_logp not 4-byte aligned ->
 * SASPA_EALIGN. */
#define SASPA_SAMPLE_MAX_TOPK 64
int saspa_sample_topk(const float* logits, int ld, int vocab, int rows, float temperature, int top_k, float top_p, const float* u,
                      int* out_tok, float* out_logp, void* stream);

int saspa_abi_version(void);
/* the dtype code of the library's 16-bit element type: SASPA_BF16 (libsaspa_hip.so) or SASPA_F16 (libsaspa_hip_f16.so) */
int saspa_half_type(void);
const char* saspa_build_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* SASPA_HIP_H */
