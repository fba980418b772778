"""TEST INFRASTRUCTURE ONLY -- float64 references, fp32 emulations and mutants of the calibration-free fp8 feed-forward of
csrc/saspa_gemm_f8.hip: `saspa_gemm_fp8_geglu_mx` (producer: GEGLU epilogue -> e4m3 bytes + one E8M0 exponent per row and 32
columns) and `saspa_gemm_mxfp8` (consumer: the exponents applied inside the scaled MFMA).  CPU only; tests/test_mxfp8_ff_host.py
(the proof of the limits) and tests/test_mxfp8_ff_gpu.py both import it.

Rounding points (gemm_f8_kernel<GEGLU, MX>), on top of those tests/fp8_ref.py lists for the K loop and the bf16 tile:
- producer: y = fast_gelu_mul(value, gate) in fp32 on the bf16 tile; the block maximum of |y| over 32 consecutive gated columns;
  e = mx_block_exponent (common.h): exact integer arithmetic on the fp32 bits; y * 2^-e exact (ldexpf); ONE e4m3 conversion, round
  to nearest even; nothing can exceed 448.
- consumer: the products 2^(qs - 127) a w are exact in fp32; fp32 accumulation per 128-wide K-tile; v = acc * sw + bias in fp32 (one
  fma); the tile rounded to bf16; + residual in fp32 and a second bf16 rounding.
"""
import math

import torch
import torch.nn.functional as F

from tests import fp8_ref as R
from tests.errbudget import geglu_gemm_scale, gemm_scale

BLOCK = 32
E4M3_MAX = R.E4M3_MAX


# ------------------------------------------------------------------ the block rule
def block_exponent(amax):
    """mx_block_exponent of common.h on fp32 values, bit for bit: the smallest e with amax <= 448 * 2^e off the fp32 fields,
    clamped to [-127, 127]; 0 for a zero."""
    bits = amax.float().contiguous().view(torch.int32)
    e = (bits >> 23) - 135 + ((bits & 0x7fffff) > 0x600000).to(torch.int32)
    return torch.where(bits == 0, torch.zeros_like(e), e.clamp(-127, 127))


def block_exponent_def(amax):
    """The rule from its definition in float64 (no bit tricks): the smallest integer e with amax <= 448 * 2^e, clamped; 0 for 0."""
    a = amax.double()
    m, x = torch.frexp(a / E4M3_MAX)                   # a / 448 = m 2^x, m in [0.5, 1): a <= 448 * 2^x always; 2^(x - 1) iff m == 0.5
    e = torch.where(m == 0.5, x - 1, x).to(torch.int32)
    return torch.where(a == 0, torch.zeros_like(e), e.clamp(-127, 127))


def block_exponent_floor(amax):
    """The mutant: the LARGEST e with 448 * 2^e <= amax (floor for ceiling): whatever lies above 448 * 2^e saturates."""
    a = amax.double()
    m, x = torch.frexp(a / E4M3_MAX)
    e = (x - 1).to(torch.int32)
    return torch.where(a == 0, torch.zeros_like(e), e.clamp(-127, 127))


def quantize_blocks(y, *, rule=block_exponent, shift=0, to_bytes=R.e4m3_bytes):
    """fp32 y [M, F] (F % 32 == 0) -> (q uint8 [M, F], qs uint8 [M, F / 32]) as the producer's epilogue does it.  shift: the mutant
    whose block maxima are taken over columns [32 b + shift, 32 b + shift + 32) (wrapping) while exponent b still scales columns
    [32 b, 32 b + 32); to_bytes: R.e4m3_bytes (saturating, as the device conversion) or R.e4m3_bytes_rtz."""
    y = y.float()
    m, f = y.shape
    amax = y.roll(-shift, 1).abs().reshape(m, f // BLOCK, BLOCK).amax(-1)
    e = rule(amax)
    t = torch.ldexp(y.reshape(m, f // BLOCK, BLOCK), -e[:, :, None])
    return to_bytes(t.reshape(m, f)).reshape(m, f), (e + 127).to(torch.uint8)


def decode_blocks(q, qs):
    """(q, qs) -> float64 values q * 2^(qs - 127)."""
    m, f = q.shape
    e = qs.to(torch.int32)[:, :f // BLOCK] - 127
    return torch.ldexp(R.e4m3_decode(q).reshape(m, f // BLOCK, BLOCK), e[:, :, None]).reshape(m, f)


# ------------------------------------------------------------------ producer
def producer_gated32(op, **kw):
    """The fp32 gated values of the kernel's GEGLU epilogue [M, N / 2] (R.gemm_f8_emul up to fast_gelu_mul)."""
    return R.gemm_f8_emul(op, geglu=True, out_scale=1.0, to_bytes=lambda g: g.float(), **kw)


def producer_emul(op, *, rule=block_exponent, shift=0, to_bytes=R.e4m3_bytes, **kw):
    return quantize_blocks(producer_gated32(op, **kw), rule=rule, shift=shift, to_bytes=to_bytes)


def producer_ref(op):
    """float64: the gated value hv * gelu_erf(hg) of the exact projection, and the magnitude its e4m3 image is held against.  Two
    terms, from the formats alone: the e4m3 conversion errs by at most 2^-4 (16 units of 2^-8) of |y|, floored at the e4m3 normal
    minimum of its block, 2^(e - 6) (below it the format's absolute step takes over); what enters the conversion is the bf16 path's
    gated value, which errbudget holds to 2^-8 of geglu_gemm_scale (value and gate are sums of the projection's magnitude, rounded
    to bf16; a gate near zero carries the error of its whole sum).  Hence max(|y|, 2^(e - 6)) + 2^-4 geglu_gemm_scale: a right
    result stays near 16 units."""
    x, w = op["a"] * op["sa"][:, None], op["w"] * op["sw"][:, None]
    hv, hg = R.untile(x @ w.t() + op["bias"])
    mv, mg = R.untile(gemm_scale(x, w, op["bias"]))
    y = hv * F.gelu(hg)
    m, f = y.shape
    e = block_exponent_def(y.abs().reshape(m, f // BLOCK, BLOCK).amax(-1)).double()
    floor = torch.exp2(e - 6)[:, :, None].expand(m, f // BLOCK, BLOCK).reshape(m, f)
    return y, torch.maximum(y.abs(), floor) + 2.0 ** -4 * geglu_gemm_scale(hv, hg, mv, mg)


# ------------------------------------------------------------------ consumer
def consumer_emul(q, qs, op2, *, residual=True, bias=True, ignore_exponents=False, block_roll=0, **kw):
    """saspa_gemm_mxfp8 in fp32 (R.gemm_f8_emul on the decoded activations: 2^(qs - 127) a is exact).  Mutants: ignore_exponents
    (every scale 1.0), block_roll (block b takes the exponent of block b + block_roll of its row)."""
    qs_used = torch.full_like(qs, 127) if ignore_exponents else qs.roll(-block_roll, 1)
    a = decode_blocks(q, qs_used)
    b = op2["bias"] if bias else torch.zeros_like(op2["bias"])
    op = dict(a=a, w=op2["w"], sa=torch.ones(a.shape[0], dtype=torch.float64), sw=op2["sw"], bias=b, res=op2["res"])
    return R.gemm_f8_emul(op, residual=residual, **kw)


def consumer_ref(y, op2, *, residual=True):
    """float64 y (sw W)^T + bias (+ residual) from float64 activations y, and its magnitude."""
    w = op2["w"] * op2["sw"][:, None]
    v = y @ w.t() + op2["bias"]
    if residual:
        return v + op2["res"], gemm_scale(y, w, op2["bias"], residual=op2["res"])
    return v, gemm_scale(y, w, op2["bias"])


# ------------------------------------------------------------------ operands
def pair_operands(rand, m, c, seed):
    """The feed-forward pair of a width-c block on random operands: the GEGLU projection c -> 8 c as R.random_operands(geglu=True)
    draws it, the output projection 4 c -> c with Gaussian weights quantised per output channel, an fp32 bias and a bf16 residual at
    half the rms of the product (fp8_ref.random_operands explains why not at 1)."""
    from saspa_aug_amd import weights as W
    op1 = R.random_operands(rand, m, c, 8 * c, seed, geglu=True)
    wq, sw = W.quantize_fp8(rand(c, 4 * c, seed=seed + 11, scale=1 / math.sqrt(4 * c)))
    op2 = dict(w=R.e4m3_decode(wq), sw=sw.double())
    y, _ = producer_ref(op1)
    size = 0.5 * (y @ (op2["w"] * op2["sw"][:, None]).t()).pow(2).mean().sqrt().item()
    op2["bias"] = (rand(c, seed=seed + 12) * size).float().double()
    op2["res"] = R.rne(rand(m, c, seed=seed + 13) * size)
    return op1, op2


def exact_consumer_operands(rand, m, k, n, seed):
    """Operands whose result is known exactly whatever the summation order: activations in {-2 .. 2}, weights in {-1, 0, 1}
    (|sum of products| <= 2 K < 2^10 for K <= 384), block exponents that cover 120 .. 134 over (row, block) while the blocks of ONE
    row stay within +-3 of the row's base (every partial sum is a multiple of 2^(base - 130) below 2^(base - 114): 17 bits), power-of
    -two weight scales, bias on the scales' grid, a bf16 residual of the size of the element it joins."""
    a = (rand(m, k, seed=seed) * 1.2).round().clamp(-2, 2).double()
    w = rand(n, k, seed=seed + 1).round().clamp(-1, 1).double()
    base = 123 + torch.arange(m) % 9                                   # 123 .. 131
    d = (rand(m, k // BLOCK, seed=seed + 2) * 2).round().clamp(-3, 3).to(torch.int64)
    qs = (base[:, None] + d).to(torch.uint8)
    sw = R._pow2(rand, n, -3, 3, seed + 3)
    bias = (rand(n, seed=seed + 4) * 8).round().double() * 2.0 ** -4 * sw
    res = R.rne(rand(m, n, seed=seed + 5).double() * 32 * torch.exp2(base.double() - 127)[:, None] * sw[None, :])
    return dict(a=a, w=w, qs=qs, sw=sw, bias=bias, res=res)


# ------------------------------------------------------------------ the limits' catalogue (tests/test_mxfp8_ff_host.py)
PAIR_SHAPE = (515, 640)           # rows, block width c: (515, 640, 5120) -> (515, 2560) -> (515, 640), SDXL level 1
PAIR_SEED = 701


def pair_cases(rand, m=PAIR_SHAPE[0], c=PAIR_SHAPE[1], seed=PAIR_SEED):
    """[(name, family, got, ref64, scale, legit?)] for the two checks of the pair: 'emit' (the producer's decoded bytes against the
    float64 gated values) and 'pair' (the output projection's result against the float64 pair)."""
    op1, op2 = pair_operands(rand, m, c, seed)
    y, ys = producer_ref(op1)
    ref, s = consumer_ref(y, op2)
    out = []

    def add(name, legit, q, qs, **ckw):
        out.append((name, "emit", decode_blocks(q, qs), y, ys, legit))
        out.append((name, "pair", consumer_emul(q, qs, op2, **ckw), ref, s, legit))

    q, qs = producer_emul(op1)
    add("legit forward K-tiles", True, q, qs)
    add("legit reversed K-tiles", True, *producer_emul(op1, rev=True), rev=True)
    add("legit libm exp in the erf", True, *producer_emul(op1, libm_exp=True))
    add("mutant exponent rule floor for ceiling (saturates)", False, *producer_emul(op1, rule=block_exponent_floor))
    add("mutant conversion rounding toward zero", False, *producer_emul(op1, to_bytes=R.e4m3_bytes_rtz))
    add("mutant block boundaries shifted by 8 columns", False, *producer_emul(op1, shift=8))
    # consumer-side mutants: the emission itself is right, only the 'pair' check can see them
    out.append(("mutant consumer takes the neighbouring block's exponent", "pair", consumer_emul(q, qs, op2, block_roll=1), ref, s, False))
    out.append(("mutant consumer ignores the exponents", "pair", consumer_emul(q, qs, op2, ignore_exponents=True), ref, s, False))
    return out
