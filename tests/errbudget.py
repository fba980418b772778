"""Rounding-error budgets for kernel parity (tests only).

A bf16 kernel that is right differs from a float64 reference of the same operation (computed from the bf16-rounded operands, with
the kernel's documented intermediate rounding points applied) by rounding only: the RNE output rounding (at most 2^-8 of |out|),
bf16 intermediates (at most 2^-8 of the magnitude that was rounded) and fp32 accumulation in some order (far smaller).  All of
these are bounded by 2^-8 times the per-output magnitude s_i of the terms that formed output i, so the error in units of
`unit * s_i` stays O(1) and has no sign preference.  check_budget measures four statistics of that error:

- max    max_i |e_i|,  e_i = (got_i - ref_i) / (unit * s_i)
- rms    sqrt(mean e_i^2)
- bias   mean(e_i * sign(ref_i)): negative = pulled toward zero (truncation instead of RNE, a denominator too large)
- slope  sum (got_i - ref_i) ref_i / (unit * sum ref_i^2): a relative scale error of the whole output in units (a wrong eps, an
         unmasked pad key, a wrong softmax scale)

and asserts each against a per-family limit table.  bias and slope are means over the outputs, so even the correctly rounded
result carries sampling noise in them (a few 1e-3 units at a few thousand outputs): their allowance is the table's systematic limit
PLUS Z_NOISE standard errors of the statistic measured on the same outputs (se_bias = std(e sign(ref)) / sqrt(N), se_slope =
sqrt(sum (err ref)^2) / (unit sum ref^2)).  A systematic slip grows with N; the noise allowance shrinks with it.  tests/test_errbudget.py proves on the CPU that every limit sits at least 2x
above what legitimate emulations of the kernels produce and at least 2x below what a catalogue of subtly wrong results produces.
"""
import math

import torch
import torch.nn.functional as F

UNIT_BF16 = 2.0 ** -8
# SASPA_F32X3: a = hi + lo with hi = bf16(a), lo = bf16(a - hi), products hi*hi + hi*lo + lo*hi in fp32.  |a - hi - lo| <=
# 2^-9 |a - hi| <= 2^-18 |a| and the dropped lo*lo <= 2^-18 |a b|: 2^-17 |a b| per product at most, fp32 accumulation below that.
UNIT_F32X3 = 2.0 ** -17
# the exact-fp32 kernels (SASPA_F32: fp32 operands on the fp32 MFMA, fp32 epilogue and storage): half an fp32 ulp at the bottom of a
# binade.  A right kernel rounds every product and every partial sum to that, in whatever order it adds (tests/f32_ref.py).
UNIT_F32 = 2.0 ** -24

# Per family: max / rms / |bias| / |slope| in units.  Each value is checked against both margins in tests/test_errbudget.py.
LIMITS = {
    "gemm": dict(max=2.2, rms=0.3, bias=0.002, slope=0.032),
    "attn": dict(max=3.2, rms=0.62, bias=0.024, slope=0.1),
    "norm": dict(max=2.2, rms=0.9, bias=0.0145, slope=0.0095),
    "elem": dict(max=2.2, rms=1.0, bias=0.025, slope=0.09),
    "f32x3": dict(max=0.9, rms=0.2, bias=0.006, slope=0.036),
    # the fused transformer-block chains (chain_*_scale).  "xattn" / "ff": launches with a zero residual, where the reference's last
    # rounding point is the output itself and a right result differs from it by rare one-ulp flips; "as": the A-stationary GEMM's
    # fused LayerNorm / GEGLU / V^T forms; "chain_res": the chains with the residual kept, where the output rounding dominates.
    # max of "xattn" / "ff" is set by ONE legitimate flip at the element where a bf16 ulp is largest against the (worst-case, hence
    # generous) chain magnitude; the subtle slips there (a truncating pack, tanh-GELU, a wrong scale) are caught by the slope
    "xattn": dict(max=0.8, rms=0.002, bias=0.00015, slope=0.01),
    "ff": dict(max=0.3, rms=0.0011, bias=0.0005, slope=0.006),
    "as": dict(max=0.7, rms=0.1, bias=0.003, slope=0.03),
    "chain_res": dict(max=0.4, rms=0.014, bias=0.0002, slope=0.02),
    # the fp8 emission of the fp8 GEMM's GEGLU epilogue (tests/fp8_ref.py), in units of 2^-4 (half an e4m3 ulp at the bottom of a
    # binade) of |ref| floored at the e4m3 normal minimum.  Round to nearest even: max 1.000, rms 0.41 .. 0.48 (1 / sqrt(3) = 0.58
    # with every value at the bottom of its binade), |bias| <= 0.021, |slope| <= 0.051 (inside its noise allowance).  Rounding toward
    # zero: max 2.0, rms 0.82 .. 0.93 and bias -0.70 .. -0.78 (mean of -binade bottom / |ref| = -ln 2 on log-uniform values): max
    # and rms cannot hold both margins, the bias does (ratio >= 8).  The scale applied twice: every statistic above 6.
    "e4m3": dict(max=2.2, rms=1.2, bias=0.05, slope=0.05),
    # the ResnetBlock2D path (tests/resnet_ref.py), measured over test_errbudget.SEEDS.
    # "gnstat": the (sum, sum of squares) a producer's epilogue leaves per (128-row block, unit), in units of 2^-24 of sum |v| /
    # sum v^2.  The kernels' orders (fdot2 pairs, 8 / 16 / 32 row groups): max 2.6 .. 5.8, rms 0.90 .. 1.65, |bias| <= 1.06, |slope|
    # <= 2.2; ONE fp32 accumulator walking all 1280 values in order, the coarsest order a right kernel could take: max 64 .. 80, rms
    # 27.6 .. 37.9, bias 19 .. 26.4, slope 36 .. 52 -- it sets the limits.  Weakest mutant, the sums of the unrounded fp32
    # accumulators: max 6.6e3 .. 1.1e4, rms 1.9e3 .. 2.4e3 (bias and slope inside their noise: max and rms carry it, ratio >= 23);
    # a row left out, a unit's columns shifted, sums taken before the residual: every statistic above 1e4.
    "gnstat": dict(max=180.0, rms=80.0, bias=56.0, slope=110.0),
    # "gn_chain": conv -> bf16 -> GroupNorm -> SiLU with every rounding point in the reference, the output's included (as
    # "xattn" / "ff": a right result differs by rare one-ulp flips).  Legit: max <= 0.21 (0.34 .. 0.59 for ONE output flip, worst
    # placed: it sets max), rms <= 7.8e-4 (1.7e-3 for the one flip), |bias| <= 5e-6, |slope| <= 9e-4.  The intermediate kept in fp32 /
    # alpha after the rounding: max 0.26 .. 0.62 and bias / slope inside their noise -- the rms carries them, 0.021 .. 0.042 (ratio
    # >= 3.4); n-1 variance (n = 1280 / 1760): rms 0.015 .. 0.019, slope 0.075 .. 0.115; tail items left out: rms 0.26 .. 4.4; eps x 10
    # (low variance): rms 4.5; the row vector of image b - 1: rms 3.5 .. 10.
    "gn_chain": dict(max=1.2, rms=0.006, bias=0.0005, slope=0.02),
    # "conv_gn": GroupNorm -> SiLU -> bf16 -> 3x3 conv, the output rounding measured.  Legit: max 0.05 .. 0.21, rms 0.006 .. 0.0202,
    # |bias| <= 1.4e-4, |slope| <= 0.0069 (both inside 4 standard errors).  n-1 variance (n = 512): max 0.33 .. 0.44, rms 0.028 -- the
    # bias carries it, 1.4e-3 .. 1.6e-3 at a standard error of 5e-5 (ratio >= 2.5), the slope (0.044 .. 0.050) holds 2.0; the
    # normalised input truncated: max 0.07 .. 0.44, carried by bias 4e-3 .. 1.1e-2 and slope 0.21 .. 0.49; padding before the
    # normalisation, the previous chunk's affine, un-SiLU'd halo rows, the first group's statistics, eps x 10: max 2.1 .. 11.9.
    "conv_gn": dict(max=0.45, rms=0.045, bias=0.00015, slope=0.007),
    # the exact-fp32 kernels (tests/f32_ref.py), in units of 2^-24 (UNIT_F32), measured over test_errbudget.SEEDS.  Where the weakest
    # mutant is far away the limits sit 2.2 .. 2.6x above the legit envelope, not 2.0x: torch's own sums are among the emulations, and
    # their order is the host's.
    # "f32_gemm": linear / conv / split-K with every epilogue form, N(0, 1) and post-ReLU operands against zero-mean weights, K = 40
    # .. 4608.  Legit (torch's matmul, K reversed, one fma chain, one exactly-summed 4-product step per rounding, K in 2 / 5 / 8
    # slices): max 0.41 .. 4.14 (SiLU epilogue at K = 64), rms 0.070 .. 0.432 (bias only, K = 64), |bias| <= 0.027 and |slope| <=
    # 0.36, both inside 3 of their standard errors.  Weakest mutant, the bf16x3 split operands (SASPA_F32X3 where exact was asked),
    # K <= 576 only: max 16.5 .. 110, rms 2.92 (K = 576) .. 19 (K = 40), bias and slope inside their noise -- the rms carries it (ratio >= 2.9), max
    # does not hold 2x at K = 576; beyond K = 576 it sinks into the accumulation error and is not asserted.  Operands truncated to
    # tf32: rms 194 .. 2.6e3; bias / residual / output through bf16: rms 294 .. 9e3; K columns dropped, bias missing on 4 columns,
    # alpha before the bias, a copied tail row, ReLU on the wrong side of the residual, column 0's bias in the scalar tail: rms >=
    # 9.4e3.
    "f32_gemm": dict(max=10.0, rms=1.0, bias=0.01, slope=0.05),
    # "f32_gemm_pos": non-negative against non-negative operands (the bilinear attention pooling product, K = 52 / 196 + 4 zero
    # columns, alpha = 1 / HW): nothing cancels, every partial sum is as large as the result and one accumulator errs by ~0.13
    # sqrt(K) units.  Legit: max 3.0 .. 7.99, rms 0.91 .. 2.07, |bias| <= 0.105, |slope| <= 0.099 (inside 3 standard errors).
    # bf16x3 split operands: max 51.9 .. 131, rms 14.5 .. 28.8 (ratio >= 2.6 on max, 2.9 on rms); tf32 operands, output through bf16, a K
    # tile dropped, a copied tail row: rms >= 1e4.
    "f32_gemm_pos": dict(max=20.0, rms=5.0, bias=0.05, slope=0.05),
    # "f32_pool": average pooling, fp32 storage, 4 .. 361 taps added in tap order.  Legit: max 0.74 .. 6.97, rms 0.28 .. 2.78 (196
    # non-negative taps), |bias| <= 0.58, |slope| <= 3.1, inside 2.1 standard errors (48 .. 2376 outputs).  Weakest mutant, 1 / (k*k
    # - 1) at 361 taps: max 5.5e3, rms 2.5e3; the last tap row left out: rms >= 1.8e5.
    "f32_pool": dict(max=18.0, rms=7.0, bias=1.5, slope=1.0),
    # "f32_pool_bf16": the same with bf16 storage, in units of 2^-8: the output rounding dominates.  Legit: max 0.064 .. 0.996, rms
    # 0.022 .. 0.422, |bias| <= 0.05, |slope| <= 0.19 (inside 1.1 standard errors).  1 / (k*k - 1) where it is named (f32_ref.pool_
    # cases): rms 5.3 .. 83, and at 196 non-negative taps (48 outputs) max 1.93, rms 1.26 -- there the bias carries it, 1.21 .. 1.44
    # at a standard error of 0.056 (ratio >= 2.4).  The last tap row left out: rms 2.78 .. 155.  A bf16 accumulator at 196
    # non-negative taps: max 5.7 .. 7.4, rms 2.3 .. 2.8 (ratio >= 2.5); at 49 taps (rms 1.3 against a limit that has to grant 0.84)
    # and on zero-mean inputs (rms 0.3 .. 0.5) it CANNOT hold the 2x margin under any statistic and is not asserted there.
    "f32_pool_bf16": dict(max=2.1, rms=0.9, bias=0.05, slope=0.1),
    # "f32_tail": signsqrt_l2norm on rows of 1000 / 4096 post-ReLU features (and N(0, 1) rows of both signs), s = |ref|.  Legit (the
    # kernel's per-lane sums with the fp64 combine, the reference's own expression in fp32, one wave's 64 lanes combined in fp32):
    # max 1.96 .. 4.62, rms 0.39 .. 1.62, |bias| <= 1.07, |slope| <= 1.17 (the rounding of a row's 1 / norm is common to the row:
    # systematic over 4 or 5 rows).  Weakest mutant, eps counted for exact zeros on the rows with 1 / 32 zeros: max 8.2 .. 10.3, rms
    # 6.2 .. 6.8 -- the bias carries it, 6.0 .. 6.7 (ratio >= 2.2); with 60 % zeros every
    # statistic is above 110.  eps = 1e-12, the norm taken before the sign-sqrt: rms >= 210.
    "f32_tail": dict(max=10.5, rms=3.6, bias=2.5, slope=2.7),
    # the fp32 forms of kernels with bf16 budgets (operands and cases of the bf16 families, nothing rounded on the way out).
    # "f32_norm": layernorm and groupnorm (statistics + apply), s = norm_scale(..., cancel=1.0).  Legit (two-pass LayerNorm with
    # torch's sums and with the kernel's lanes; GroupNorm from the kernels' own statistics, scale / shift form and (x - mean) rstd
    # gamma + beta): max 0.09 .. 4.61, rms 0.011 .. 0.784, |bias| <= 0.037, |slope| <= 0.77 (mean-offset groups: the rounding of
    # a group's mean x scale is common to its elements, so the slope's standard error, ~0.13, understates it).
    # Weakest mutant, ONE-pass fp32 statistics for the LayerNorm of mean-offset rows (mu / sigma = 64): max 339 .. 415, rms 36 ..
    # 39; output or gamma through bf16: rms >= 428; n-1 variance, eps 1e-3, eps swapped / x 10: rms >= 1.4e3.
    "f32_norm": dict(max=11.0, rms=1.8, bias=0.1, slope=1.0),
    # "f32_softmax": softmax_rows, s = p (1 + |l| + |l - m|) (f32_ref.softmax_ref).  Legit (the kernel's lane order, torch's own
    # fp32 softmax): max 1.48 .. 1.84, rms 0.28 .. 0.40, |bias| <= 0.021, |slope| <= 0.068 (inside 2.5 standard errors).  Weakest
    # mutant, the scale x (1 + 2^-12): max 2.1e3, rms 767; logits or output through bf16: rms >= 4.9e3; the causal mask shifted by
    # one: rms 5e9 (an output where the reference has an exact zero).
    "f32_softmax": dict(max=4.5, rms=0.9, bias=0.05, slope=0.1),
    # "f32_elem": geglu (erf), SiLU, quick-GELU; s carries the cancelling terms of 0.5 g (1 + erf) and the rounding of 1.702 x
    # (f32_ref.elem_refs).  Legit: the kernel's expressions max 2.1 .. 2.5, rms 0.52 .. 0.67; torch's own fp32 GELU max 7.9 .. 8.9,
    # rms 1.38 .. 1.41, slope 0.24 .. 0.29 -- it sets the limits.  Weakest mutant, tanh-GELU: max 3.4e3, rms 2.0e3; output through
    # bf16: rms >= 2e4; SiLU and quick-GELU swapped: rms >= 7e6.
    "f32_elem": dict(max=21.0, rms=3.3, bias=0.05, slope=0.5),
}
STATS = ("max", "rms", "bias", "slope")
Z_NOISE = 8.0           # standard errors of bias / slope granted on top of the systematic limit (8 sigma: never by chance)


def budget_stats(got, ref64, scale, unit):
    """The four statistics (a dict, plus 'worst': the flat index of the largest |e|) of got against ref64."""
    got = got.detach().to("cpu", torch.float64).reshape(-1)
    ref = ref64.detach().to("cpu", torch.float64).reshape(-1)
    s = scale.detach().to("cpu", torch.float64).expand_as(ref64).reshape(-1) if torch.is_tensor(scale) else \
        torch.full_like(ref, float(scale))
    if got.shape != ref.shape:
        raise ValueError(f"shape mismatch: got {tuple(got.shape)} vs reference {tuple(ref.shape)}")
    if not torch.isfinite(ref).all() or not (s > 0).all():
        raise ValueError("reference must be finite and scale strictly positive (floor it)")
    if not torch.isfinite(got).all():
        bad = int((~torch.isfinite(got)).nonzero()[0])
        return dict(max=math.inf, rms=math.inf, bias=math.inf, slope=math.inf, se_bias=0.0, se_slope=0.0, worst=bad)
    err = got - ref
    e = err / (unit * s)
    worst = int(e.abs().argmax())
    den = (ref * ref).sum().item()
    n = e.numel()
    es = e * torch.sign(ref)
    return dict(max=e.abs().max().item(), rms=e.pow(2).mean().sqrt().item(), bias=es.mean().item(),
                slope=(err * ref).sum().item() / (unit * den) if den > 0 else 0.0,
                se_bias=es.std().item() / math.sqrt(n) if n > 1 else 0.0,
                se_slope=(err * ref).pow(2).sum().sqrt().item() / (unit * den) if den > 0 else 0.0, worst=worst)


def allowance(st, limits):
    """The allowance of each statistic: the table's limit, plus Z_NOISE standard errors for bias and slope."""
    return dict(max=limits["max"], rms=limits["rms"], bias=limits["bias"] + Z_NOISE * st["se_bias"],
                slope=limits["slope"] + Z_NOISE * st["se_slope"])


def ratio(st, limits):
    """max over the four statistics of |stat| / allowance (<= 1: within budget)."""
    a = allowance(st, limits)
    return max(abs(st[k]) / a[k] for k in STATS)


def fmt(st):
    return " ".join(f"{k} {st[k]:+.3e}" for k in STATS)


def check_budget(got, ref64, scale, unit, *, limits, what=""):
    """Assert that got (kernel output, any dtype / device) is within the rounding budget of ref64 (float64 reference); scale is the
    per-output magnitude s_i (broadcastable to ref64, floored > 0).  Returns the statistics (for printing)."""
    st = budget_stats(got, ref64, scale, unit)
    if ratio(st, limits) > 1.0:
        w = st["worst"]
        shape = tuple(ref64.shape)
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(w), shape))
        g = got.detach().to("cpu", torch.float64).reshape(-1)[w].item()
        r = ref64.detach().to("cpu", torch.float64).reshape(-1)[w].item()
        a = allowance(st, limits)
        raise AssertionError(f"{what}: error budget exceeded: {fmt(st)}; allowance " + " ".join(f"{k} {a[k]:.3e}" for k in STATS)
                             + f" (limits {limits}, se_bias {st['se_bias']:.2e}, se_slope {st['se_slope']:.2e}); worst element "
                             f"{idx}: got {g:.6g} ref {r:.6g}")
    return st


def rejects(got, ref64, scale, unit, *, limits):
    """True when check_budget would fail (negative controls)."""
    return ratio(budget_stats(got, ref64, scale, unit), limits) > 1.0


# ------------------------------------------------------------------ magnitudes s_i (float64)
def _abs64(t):
    return t.detach().to("cpu", torch.float64).abs()


def _floor(s, rel=2.0 ** -10, absolute=1e-30):
    """Zero magnitudes (all-zero rows, a constant group) must not divide by zero: floor at rel * mean(s)."""
    return s.clamp_min(max(rel * s.mean().item(), absolute))


def gemm_scale(a, b, bias=None, *, alpha=1.0, residual=None, rowvec=None):
    """|alpha| (|A| @ |B|^T + |bias| + |rowvec|) + |residual| for out = alpha (A B^T + bias + rowvec) + residual (act after the
    sum: SiLU / GELU have |f'| <= 1.13, inside the factor-of-2 margin)."""
    s = _abs64(a) @ _abs64(b).t()
    if bias is not None:
        s = s + _abs64(bias)
    if rowvec is not None:
        s = s + _abs64(rowvec)
    s = abs(alpha) * s
    if residual is not None:
        s = s + _abs64(residual)
    return _floor(s)


def conv_scale(x, w, bias=None, *, stride=1, pad=1, residual=None, alpha=1.0):
    """The GEMM magnitude of an NCHW convolution: conv2d(|x|, |w|) + |bias| (+ |residual|)."""
    s = F.conv2d(_abs64(x), _abs64(w), None if bias is None else _abs64(bias), stride=stride, padding=pad)
    s = abs(alpha) * s
    if residual is not None:
        s = s + _abs64(residual)
    return _floor(s)


def geglu_gemm_scale(hv, hg, mv, mg):
    """out = hv * gelu(hg) with hv, hg GEMM outputs of magnitudes mv, mg: the error of each factor propagated through the product
    (|gelu(hg)| mv + |hv gelu'(hg)| mg) plus |out| for the output rounding."""
    hv, hg = hv.double(), hg.double()
    phi = torch.exp(-0.5 * hg * hg) / math.sqrt(2 * math.pi)
    gel = F.gelu(hg)
    dgel = 0.5 * (1 + torch.erf(hg / math.sqrt(2))) + hg * phi
    return _floor(gel.abs() * mv + (hv * dgel).abs() * mg + (hv * gel).abs())


def attn_scale(p, v):
    """sum_j p_ij |v_j| / l_i with p the float64 softmax weights [..., nq, nk] (already divided by l) and v [..., nk, d]."""
    return _floor(p.double() @ _abs64(v))


def norm_scale(xhat, gamma, beta, mu_rstd=None, cancel=2.0 ** -15):
    """|gamma * xhat| + |beta| for a normalised xhat [..., C] (channels last) and per-channel gamma, beta.  mu_rstd (mean * rstd,
    broadcastable): the kernels apply y = x sc + (beta - mean sc) with sc = gamma rstd in fp32 (saspa_norm.hip, gn_apply_kernel and
    the one-pass / fused forms that restate it), two fp32 terms of magnitude |mean sc| that cancel: 2^-24 of each, i.e. 2^-15 |mean sc|
    in bf16 units, joins the budget (it dominates for a constant group, where rstd = eps^-1/2).  cancel: that 2^-24 in the caller's
    unit (the default: bf16 units; 1.0 for the fp32 families, whose unit it is)."""
    s = (xhat.double() * gamma.double()).abs() + beta.double().abs()
    if mu_rstd is not None:
        s = s + cancel * (mu_rstd.double() * gamma.double()).abs()
    return _floor(s)


# ------------------------------------------------------------------ magnitudes through a chain of fused stages
# A fused kernel hands stage k's result to stage k + 1 as bf16 in registers.  A flipped rounding of that intermediate moves it by
# at most one unit of ITS scale s^(k), and every product it enters by that times the other factor: stage k + 1's scale is the
# magnitude of its own terms (the single-stage helpers above) plus s^(k) pushed through |W| (through p and |V| for attention).
# The helpers only compose magnitudes; the limits they are checked against live in LIMITS.
def chain_gemm_scale(a, b, bias=None, *, prev=None, residual=None):
    """out = A B^T + bias (+ residual) with A an intermediate of per-element scale `prev` ([M, K], or None: A is an exact input):
    gemm_scale's own terms + prev @ |B|^T."""
    s = _abs64(a) @ _abs64(b).t()
    if bias is not None:
        s = s + _abs64(bias)
    if prev is not None:
        s = s + prev.double() @ _abs64(b).t()
    if residual is not None:
        s = s + _abs64(residual)
    return _floor(s)


def chain_norm_scale(xhat, gamma, beta, prev, rstd, mu_rstd=None):
    """out = act(gamma xhat + beta) with xhat = (y - mean) rstd and y an intermediate of per-element scale `prev` (a conv output
    rounded to the storage type: conv_scale): norm_scale's own terms + prev pushed through |gamma rstd| (rstd broadcastable to
    xhat).  A flipped y also moves its group's mean and variance, by 1 / n of that: inside the margin.  SiLU after the affine has a
    slope of at most 1.1 and is absorbed as gemm_scale documents."""
    return _floor(norm_scale(xhat, gamma, beta, mu_rstd) + prev.double() * (gamma.double() * rstd.double()).abs())


def chain_attn_scale(p, v, o, k, prev_q, *, logit_unit=math.log(2.0)):
    """O = p V with p [..., nq, nk] the normalised softmax weights of logits q k^T taken in the log2 domain (logit_unit = ln 2 per
    logit unit; 1.0 for natural-log logits), q an intermediate of scale prev_q [..., nq, d]: attn_scale's own terms (sum_j p_ij
    |v_j|) plus the query's scale pushed through the softmax: a logit moves by prev_q |k_j|, its weight by p_ij logit_unit times
    that, the output by that times |v_j - o_i| (the first-order sensitivity of a normalised weighted mean)."""
    p, v, o = p.double(), v.double(), o.double()
    t = logit_unit * (prev_q.double() @ _abs64(k).transpose(-1, -2)) * p                 # [..., nq, nk]: |dp_ij| per unit
    # sum_j t_ij |v_jc - o_ic| <= sum_j t_ij |v_jc| + (sum_j t_ij) |o_ic| would lose the cancellation a dominant key has (v_j = o_i)
    push = torch.einsum("...qk,...qkc->...qc", t, (v.unsqueeze(-3) - o.unsqueeze(-2)).abs())
    return _floor(p @ v.abs() + push)


def elem_scale(*factors, floor=2.0 ** -8):
    """|product of the factors| with an absolute floor near zero (GEGLU: hv * gelu(hg); SiLU: x * sigmoid(x))."""
    s = torch.ones_like(factors[0], dtype=torch.float64)
    for f in factors:
        s = s * f.double().abs()
    return s.clamp_min(floor)
