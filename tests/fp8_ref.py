"""TEST INFRASTRUCTURE ONLY -- float64 references, magnitudes, fp32 emulations and mutants of the fp8 (OCP e4m3) W8A8 kernels of
csrc/saspa_gemm_f8.hip: `gemm_f8_kernel` and `layernorm_quant_fp8_kernel`.  CPU only; the CPU proof (tests/test_errbudget.py)
and the GPU tests (tests/test_fp8_gpu.py) both import it.

Rounding points of gemm_f8_kernel (saspa_gemm_f8.hip):
- :87       fp32 accumulation of the products of one 128-wide K-tile per MFMA; the products of two e4m3 values are exact in fp32;
- :109-110  v = acc * (sa * sw) + bias in fp32 (pad rows of the last row-tile see sa = 0, :105);
- :111      the tile is rounded to bf16 on its way through LDS (Elem<bf16_t>::store4);
then one of
- :159-168  plain: the bf16 tile IS the output; with a residual: unpack, + residual in fp32 (:165), a SECOND bf16 rounding (:166);
- :125-128  GEGLU: fast_gelu_mul (common.h:192, the polynomial erf) on the bf16 value and its bf16 gate in fp32, then
  - :145      a bf16 rounding (pack8), or
  - :137-142  * 1 / out_scale, a clamp to +-448 and the e4m3 conversion (round to nearest even);
- :131, :149-151 amax: the maximum of the fp32 gated values of the rows < M (:123 skips the pad rows).
Rounding points of layernorm_quant_fp8_kernel:
- :190, :196  mean = fp32 sum / C;  :203, :206  rstd = 1 / sqrt(fp32 sum of (x - mean)^2 / C + eps);
- :214        y = (x - mean) * rstd * gamma + beta in fp32;  :220  scale = max|y| * (1 / 448) (1.0 for an all-zero row);
- :221, :229  y * (1 / scale) converted to e4m3 (round to nearest even).
"""
import math

import torch
import torch.nn.functional as F

from tests.errbudget import elem_scale, gemm_scale

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
E4M3_MAX = 448.0
UNIT_E4M3 = 2.0 ** -4                  # half an e4m3 ulp (3 mantissa bits) relative to the bottom of the binade
KT = 128                               # K-tile of the kernel


def rne(x):
    return x.float().to(BF).double()


def trunc(x):
    i = x.float().contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).double()


def f32r(x):
    """ONE fp32 rounding of a float64 value."""
    return x.float().double()


# ------------------------------------------------------------------ e4m3
def e4m3_decode(u8):
    return u8.contiguous().view(F8).double()


def e4m3_bytes(x):
    """fp32 values -> e4m3 codes, round to nearest even, saturating at +-448 (the kernel clamps before it converts)."""
    return x.float().clamp(-E4M3_MAX, E4M3_MAX).to(F8).view(torch.uint8)


def e4m3_step(v):
    """The e4m3 ulp at |v|'s binade (the subnormal step 2^-9 below 2^-6)."""
    e = torch.floor(torch.log2(v.double().abs().clamp_min(2.0 ** -6))).clamp(-6, 8)
    return torch.exp2(e - 3)


def e4m3_bytes_rtz(x):
    """The mutant: conversion rounding toward zero."""
    x = x.double().clamp(-E4M3_MAX, E4M3_MAX)
    st = e4m3_step(x)
    return (torch.sign(x) * torch.floor(x.abs() / st) * st).float().to(F8).view(torch.uint8)


def code_distance(a_u8, b_u8):
    """|difference| of two e4m3 codes in steps along the number line (sign-magnitude bytes; +0 and -0 coincide)."""
    def line(u):
        i = u.to(torch.int32)
        return torch.where(i >= 128, -(i - 128), i)
    return (line(a_u8) - line(b_u8)).abs()


# ------------------------------------------------------------------ operands
def _uniform(rand, *shape, seed):
    return 0.5 * (1 + torch.erf(rand(*shape, seed=seed).double() / math.sqrt(2)))


def _pow2(rand, n, lo, hi, seed):
    return torch.exp2(torch.floor(_uniform(rand, n, seed=seed) * (hi - lo + 1)).clamp(0, hi - lo) + lo)


def _int_codes(rand, *shape, seed):
    return (rand(*shape, seed=seed) * 8).round().clamp(-16, 16).double()


def exact_operands(rand, m, k, n, seed, *, geglu=False):
    """Operands whose result is known exactly whatever the summation order: e4m3 codes that decode to integers in [-16, 16]
    (|sum| <= 256 K < 2^24 for K <= 384), power-of-two scales per row and per column (2^-6 .. 2^6: a scale read from the
    neighbouring row, column or 4-column group is off by binades), bias = a small multiple of 2^-4 times the column's scale, and a
    bf16 residual of the size of the element it joins.  geglu: scales 2^-6 .. 2^-5 and 2^-6 .. 2^-4, so that the gates (a sum of
    standard deviation 64 sqrt(K)) cover roughly [-4, 4]."""
    a, w = _int_codes(rand, m, k, seed=seed), _int_codes(rand, n, k, seed=seed + 1)
    sa = _pow2(rand, m, -6, -5 if geglu else 6, seed + 2)
    sw = _pow2(rand, n, -6, -4 if geglu else 6, seed + 3)
    bias = (rand(n, seed=seed + 4) * 8).round().double() * 2.0 ** -4 * sw
    res = rne(rand(m, n, seed=seed + 5).double() * 512 * sa[:, None] * sw[None, :])
    return dict(a=a, w=w, sa=sa, sw=sw, bias=bias, res=res)


def random_operands(rand, m, k, n, seed, *, geglu=False):
    """Operands as tests/test_fp8_gpu.py::test_gemm_fp8 draws them: arbitrary e4m3 activations, sa in [0.5, 1.5], Gaussian weights
    quantised per output channel, an fp32 bias, a bf16 residual.  One difference: bias and residual are drawn at HALF THE RMS OF THE
    PRODUCT instead of at 1.  With 100 x N(0, 1) activations a product is several hundred, a unit bias less than half a bf16 ulp of it
    -- a missing bias or a misread residual would be inside the rounding of a right result, whatever the check.  (GEGLU keeps the
    unit bias: its gates must stay where the GELU bends.)"""
    from saspa_aug_amd import weights as W
    a = (rand(m, k, seed=seed).clamp(-3, 3) * 100).to(F8).double()
    sa = (0.5 + _uniform(rand, m, seed=seed + 2)).float().double()
    w = rand(n, k, seed=seed + 1, scale=1 / math.sqrt(k))
    b = rand(n, seed=seed + 4)
    if geglu:
        w, b = W.pack_geglu_tile(w, b, 128)
    wq, sw = W.quantize_fp8(w)
    wd, sw = e4m3_decode(wq), sw.double()
    size = 1.0 if geglu else 0.5 * ((a * sa[:, None]) @ (wd * sw[:, None]).t()).pow(2).mean().sqrt().item()
    return dict(a=a, w=wd, sa=sa, sw=sw, bias=(b * size).float().double(), res=rne(rand(m, n, seed=seed + 5) * size))


def to_codes(v):
    """Exactly representable values -> e4m3 bytes."""
    u = v.float().to(F8)
    assert torch.equal(u.double(), v.double()), "not e4m3 values"
    return u.view(torch.uint8).contiguous()


def untile(t):
    """[M, N] in the kernel's GEGLU packing (per 128-column tile: 64 values, then their 64 gates) -> (values, gates) [M, N / 2]."""
    m, n = t.shape
    r = t.reshape(m, n // 128, 2, 64)
    return r[:, :, 0].reshape(m, n // 2), r[:, :, 1].reshape(m, n // 2)


# ------------------------------------------------------------------ float64 references and magnitudes
def gemm_f8_ref(op, *, residual=False, bias=True):
    """float64 (sa A)(sw W)^T + bias (+ residual after the tile's bf16 rounding, :111 then :165) and its magnitude."""
    x, w = op["a"] * op["sa"][:, None], op["w"] * op["sw"][:, None]
    b = op["bias"] if bias else None
    v = x @ w.t() + (0 if b is None else b)
    if residual:
        return rne(v) + op["res"], gemm_scale(x, w, b, residual=op["res"])
    return v, gemm_scale(x, w, b)


def geglu_exact_ref(tile):
    """The GEGLU epilogue from the EXACT bf16 tile [M, N] (what exact_operands make known): float64 hv * gelu_erf(hg) and the elem
    magnitude."""
    hv, hg = untile(tile)
    gl = F.gelu(hg)
    return hv * gl, elem_scale(hv, gl)


def e4m3_scale(ref, out_scale):
    """Magnitude of the fp8 emission: |ref| floored at the e4m3 normal minimum 2^-6 * out_scale (below it the format's absolute
    step takes over)."""
    return ref.abs().clamp_min(2.0 ** -6 * out_scale)


# ------------------------------------------------------------------ fp32 emulation of gemm_f8_kernel, one slip at a time by option
def _erf_as32(x, libm_exp=False):
    """common.h fast_erf in fp32 (tests/test_errbudget._erf_as is its float64-capable twin); libm_exp: exp() for exp2()."""
    x = x.float()
    ax = x.abs()
    t = 1.0 / (0.3275911 * ax + 1.0)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    e = torch.exp(-ax * ax) if libm_exp else torch.exp2(-ax * ax * 1.4426950408889634)
    return torch.copysign(1.0 - poly * e, x)


def fast_gelu_mul32(val, gate, libm_exp=False):
    val, gate = val.float(), gate.float()
    return val * (0.5 * gate * (1.0 + _erf_as32(gate * 0.70710678118654752440, libm_exp)))


def gemm_f8_emul(op, *, residual=False, geglu=False, out_scale=None, rev=False, rnd_tile=rne, rnd_out=rne, kdrop_tiles=0,
                 sa_roll=0, sw_roll=0, bias_cols=None, res_before=False, gelu="as", swap_tile=None, to_bytes=e4m3_bytes,
                 scale_twice=False, libm_exp=False, want_amax=False):
    """The kernel in fp32.  Options: rev (K-tiles in descending order), res_before (residual added BEFORE the tile rounding: one
    rounding), and the mutants: rnd_tile / rnd_out = trunc, kdrop_tiles (last K-tiles left out), sa_roll / sw_roll (the scale of
    a neighbouring row / 4-column group), bias_cols (bias only on columns < bias_cols), gelu = 'tanh', swap_tile (value and gate
    halves of that 128-column tile swapped), to_bytes = e4m3_bytes_rtz, scale_twice.  Returns float64 values, or uint8 codes
    with out_scale; (out, amax) with want_amax."""
    a, w = op["a"].float(), op["w"].float()
    nk = a.shape[1] // KT - kdrop_tiles
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for kt in (range(nk - 1, -1, -1) if rev else range(nk)):
        acc = acc + a[:, kt * KT:(kt + 1) * KT] @ w[:, kt * KT:(kt + 1) * KT].t()
    sa, sw = op["sa"].float().roll(sa_roll), op["sw"].float().roll(sw_roll)
    b = op["bias"].float().clone()
    if bias_cols is not None:
        b[bias_cols:] = 0
    # (acc * (sa * sw) + b contracts to one fma on the device: one fp32 rounding of the exact value)
    v = f32r(acc.double() * (sa[:, None] * sw[None, :]).double() + b.double())
    if residual and res_before:
        return rnd_out(v + op["res"])
    t = rnd_tile(v)
    if not geglu:
        return rnd_out(f32r(t + op["res"])) if residual else t
    hv, hg = untile(t)
    if swap_tile is not None:
        sl = slice(64 * swap_tile, 64 * swap_tile + 64)
        hv, hg = hv.clone(), hg.clone()
        hv[:, sl], hg[:, sl] = untile(t)[1][:, sl], untile(t)[0][:, sl]
    if gelu == "tanh":
        g = hv.float() * F.gelu(hg.float(), approximate="tanh")
    elif gelu == "erf":
        g = hv.float() * F.gelu(hg.float())
    else:
        g = fast_gelu_mul32(hv, hg, libm_exp)
    amax = g.abs().max().item()
    if out_scale is None:
        out = rnd_out(g)
    else:
        inv = torch.tensor(1.0 / out_scale, dtype=torch.float32)
        out = to_bytes(g * inv * (inv if scale_twice else 1.0))
    return (out, amax) if want_amax else out


# ------------------------------------------------------------------ quantising LayerNorm
def ln_quant_ref(x, gamma, beta, eps=1e-5):
    """float64 LayerNorm of bf16 x [rows, C] -> (y, max|y| / 448 per row (1.0 for an all-zero row), |gamma xhat| + |beta|)."""
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(-1, keepdim=True)
    xhat = (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    y = xhat * g + b
    amax = y.abs().amax(-1)
    return y, torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax)), (xhat * g).abs() + b.abs()


def ln_quant_emul(x, gamma, beta, eps=1e-5, to_bytes=e4m3_bytes):
    """The kernel in fp32 -> (codes uint8 [rows, C], scale fp32 [rows])."""
    xf, g, b = x.float(), gamma.float(), beta.float()
    c = xf.shape[-1]
    mean = xf.sum(-1, keepdim=True) / c
    d = xf - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / c + eps)
    y = d * rstd * g + b
    amax = y.abs().amax(-1)
    sc = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
    inv = 1.0 / sc
    return to_bytes(y * inv[:, None]), sc


def ln_quant_violations(q_u8, scale_got, y64, mag64):
    """Elements whose decoded byte is NOT within half an e4m3 ulp of y64 / scale_got -- the ulp at the value's own binade (of the
    target, or of the decoded byte where rounding carried it up into the next binade), the subnormal step below 2^-6 --, plus
    2^-20 (|gamma xhat| + |beta|) / scale for the fp32 arithmetic.  No excluded share."""
    sc = scale_got.double()[:, None]
    t = y64 / sc
    d = e4m3_decode(q_u8)
    half = 0.5 * e4m3_step(torch.maximum(t.abs().clamp_max(E4M3_MAX), d.abs()))
    return (d - t).abs() > half + 2.0 ** -20 * mag64 / sc


# Worst relative difference of the fp32 emulation's row scale from max|y64| / 448, measured over every case and edge row of
# tests/test_fp8_gpu.py's LayerNorm tests on four seed shifts: 2.82e-7 (4.7 x 2^-24) with the random gamma, 6.73e-7 where ONE channel's
# gamma decides the maximum (ln_one_channel_affine: x - mean of a single element, not the largest of 640).  The GPU test grants 4x that.
LN_SCALE_MEASURED = 6.73e-7
LN_SCALE_RTOL = 4 * LN_SCALE_MEASURED
# Share of emitted bytes two legitimate emulations disagree on (byte_disagreement below): measured 0 on four seed shifts; the GPU test
# grants 4x the measurement and no less than 1e-4, and every differing byte differs by ONE code.
BYTE_SHARE_CAP = 1e-4
LN_CASES = [(5, 8), (77, 640), (4, 2048), (1, 1280), (300, 640), (77, 1280), (1000, 128), (5, 2048)]


def ln_case(rand, rows, c, seed=1):
    """ln_rows plus the edge rows (where the case has rows for them): row 1 constant (variance 0: y = beta), row 2 = 0.01 z with one
    1000 x outlier (the rest lands C times below it, in the lowest binades the row's scale leaves)."""
    x, g, b = ln_rows(rand, rows, c, seed)
    if rows >= 4:
        x[1] = 0.7
        x[2] = (rand(c, seed=seed + 8) * 0.01).to(BF)
        x[2, c // 3] = 10.0
    return x, g, b


def ln_one_channel_affine(c):
    """gamma = 2^-7 except 1 on channel c // 3, beta = 0: with ln_case's outlier row everything but the outlier lands in e4m3
    subnormals or zero."""
    g = torch.full((c,), 2.0 ** -7)
    g[c // 3] = 1.0
    return g, torch.zeros(c)


def ln_rows(rand, rows, c, seed):
    """bf16 rows and fp32 gamma / beta as test_layernorm_quant_fp8 draws them."""
    x = (rand(rows, c, seed=seed) * 2 + 0.5).to(BF)
    return x, (1 + 0.1 * rand(c, seed=seed + 1)).float(), (0.1 * rand(c, seed=seed + 2)).float()


# ------------------------------------------------------------------ the catalogue (tests/test_errbudget.py registers these)
CPU_SHAPES = [(70, 128, 128, 401), (130, 384, 256, 411), (130, 1280, 256, 421)]


def gemm_cases(rand):
    """'gemm' family: (name, got, ref64, scale, legit?) on random operands, plain and residual forms."""
    out = []
    for (m, k, n, seed) in CPU_SHAPES:
        op = random_operands(rand, m, k, n, seed)
        for residual in (False, True):
            ref, s = gemm_f8_ref(op, residual=residual)
            tag = f"fp8 gemm {'residual' if residual else 'plain'} {m}x{k}x{n}"
            emu = lambda **kw: gemm_f8_emul(op, residual=residual, **kw)          # noqa: E731
            out.append((f"legit forward K-tiles {tag}", emu(), ref, s, True))
            out.append((f"legit reversed K-tiles {tag}", emu(rev=True), ref, s, True))
            out.append((f"mutant truncating tile pack {tag}", emu(rnd_tile=trunc), ref, s, False))
            if residual:
                # the kernel rounds the tile first (:111) and adds the residual to the rounded value (:165); adding it before
                # the rounding (ONE rounding) is within half the budget of that reference as well
                out.append((f"legit residual added before the tile rounding {tag}", emu(res_before=True), ref, s, True))
                out.append((f"mutant truncating final pack {tag}", emu(rnd_out=trunc), ref, s, False))
            if k <= 384:
                out.append((f"mutant last K-tile dropped {tag}", emu(kdrop_tiles=1), ref, s, False))
            out.append((f"mutant sa of the neighbouring row {tag}", emu(sa_roll=1), ref, s, False))
            out.append((f"mutant sw of the neighbouring 4-column group {tag}", emu(sw_roll=4), ref, s, False))
            out.append((f"mutant fp8 bias missing on last 8 columns {tag}", emu(bias_cols=n - 8), ref, s, False))
    return out


GEGLU_SHAPES = [(130, 384, 256, 431), (127, 256, 128, 441)]


def geglu_cases(rand):
    """'elem' family: the fp8 GEGLU epilogue on exact operands (value and gate entering the GELU are known exactly)."""
    out = []
    for (m, k, n, seed) in GEGLU_SHAPES:
        op = exact_operands(rand, m, k, n, seed, geglu=True)
        ref, s = geglu_exact_ref(gemm_f8_emul(op))
        tag = f"fp8 geglu {m}x{k}x{n}"
        out.append((f"legit polynomial erf {tag}", gemm_f8_emul(op, geglu=True), ref, s, True))
        out.append((f"legit libm erf {tag}", gemm_f8_emul(op, geglu=True, gelu="erf"), ref, s, True))
        out.append((f"mutant tanh-gelu in the {tag}", gemm_f8_emul(op, geglu=True, gelu="tanh"), ref, s, False))
        out.append((f"mutant truncation {tag}", gemm_f8_emul(op, geglu=True, rnd_out=trunc), ref, s, False))
        out.append((f"mutant value and gate halves of one 128-column tile swapped {tag}",
                    gemm_f8_emul(op, geglu=True, swap_tile=n // 128 - 1), ref, s, False))
    return out


def pow2_scale(amax, margin=16.0):
    """ops.fp8_pow2_scale on the host."""
    return 2.0 ** math.ceil(math.log2(amax * margin / 448.0))


def e4m3_cases(rand):
    """'e4m3' family (unit 2^-4): the fp8 emission of the GEGLU epilogue, decoded bytes x scale against float64."""
    out = []
    for (m, k, n, seed) in GEGLU_SHAPES:
        op = exact_operands(rand, m, k, n, seed, geglu=True)
        ref, _ = geglu_exact_ref(gemm_f8_emul(op))
        tag = f"fp8 emission {m}x{k}x{n}"
        for margin in (16.0, 1.0):
            osc = pow2_scale(ref.abs().max().item(), margin)
            s = e4m3_scale(ref, osc)
            dec = lambda **kw: e4m3_decode(gemm_f8_emul(op, geglu=True, out_scale=osc, **kw)) * osc       # noqa: E731
            t2 = f"{tag} margin {margin:g}"
            out.append((f"legit polynomial erf {t2}", dec(), ref, s, True))
            out.append((f"legit libm exp {t2}", dec(libm_exp=True), ref, s, True))
            out.append((f"mutant emission rounding toward zero {t2}", dec(to_bytes=e4m3_bytes_rtz), ref, s, False))
            if osc != 1.0:                       # (a scale of 1 applied twice is a scale of 1)
                out.append((f"mutant out_scale applied twice {t2}", dec(scale_twice=True), ref, s, False))
    return out


def byte_disagreement(rand):
    """The share of emitted bytes on which two legitimate emulations disagree (forward against reversed K-tiles, exp2-based
    fast_erf against libm exp), worst over GEGLU_SHAPES and both operand kinds.  The GPU test grants 4x this, at least 1e-4."""
    worst = 0.0
    for (m, k, n, seed) in GEGLU_SHAPES:
        for make in (exact_operands, random_operands):
            op = make(rand, m, k, n, seed, geglu=True)
            base, amax = gemm_f8_emul(op, geglu=True, want_amax=True)
            osc = pow2_scale(amax)
            b0 = gemm_f8_emul(op, geglu=True, out_scale=osc)
            for kw in (dict(rev=True), dict(libm_exp=True)):
                b1 = gemm_f8_emul(op, geglu=True, out_scale=osc, **kw)
                assert code_distance(b0, b1).max().item() <= 1
                worst = max(worst, (b0 != b1).double().mean().item())
    return worst
