"""CPU proof that tests/errbudget.py has power (no GPU): per kernel family, legitimate emulations of the kernel (fp32 accumulation
in another order, split-K slabs, bf16-rounded P and softmax level, bf16 intermediates where the kernels round, RNE output) stay
within HALF the family's limits, and a catalogue of subtly wrong results ("mutants": truncating output rounding, a missing tail
mask, a dropped key or K slice, a wrong eps / scale / variance, ...) exceeds TWICE the limits.  A later loosening or tightening of
a limit that breaks either margin turns this file red.

The fused transformer-block kernels (saspa_xattn_block, saspa_ff_block, the A-stationary GEMM's fused forms) have their float64
references here as well (xattn_ref / ff_ref / as_ref: the chain with RNE-to-bf16 at exactly the hand-offs the kernels pack at, each
citing its source line), their magnitudes composed stage by stage (errbudget.chain_*_scale), and families of their own.

The exact-fp32 kernels (fp32 MFMA GEMM / conv / split-K, pooling, the sign-sqrt L2 tail and the fp32 forms of the softmax / norm /
elementwise kernels) have theirs in tests/f32_ref.py: families f32_*, in units of 2^-24."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import f32_ref, fp8_ref, resnet_ref, sampler_ref
from tests.errbudget import (LIMITS, UNIT_BF16, UNIT_F32, UNIT_F32X3, attn_scale, budget_stats, check_budget, conv_scale, elem_scale,
                             fmt, gemm_scale, geglu_gemm_scale, norm_scale, ratio, rejects)

BF = torch.bfloat16
LEGIT_MAX, MUTANT_MIN = 0.5, 2.0       # |stat| / limit: legit at most half the budget, every mutant at least twice it


SEEDS = (0, 1, 2, 3)                   # the CPU proof runs every case on these seed shifts; the GPU file runs shift 0
_SEED_SHIFT = [0]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * _SEED_SHIFT[0])
    return torch.randn(*shape, generator=g) * scale


def q(x):
    return x.to(BF).double()


def rne(x):
    """Round to bf16 (round to nearest even) and back to float64."""
    return x.float().to(BF).double()


def trunc(x):
    """Round to bf16 by truncation (toward zero): the mutant of rne."""
    i = x.float().contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).double()


def f32(x):
    return x.float()


# ------------------------------------------------------------------ GEMM / conv
def _gemm_operands(m, k, n, seed, mean_a=0.0):
    x = q(_rand(m, k, seed=seed) + mean_a)
    w = q(_rand(n, k, seed=seed + 1, scale=1 / math.sqrt(k)))
    if mean_a:
        w = q(w - w.mean(1, keepdim=True))             # zero-mean rows: |ref| << s (cancellation)
    b = _rand(n, seed=seed + 2).double()
    res = q(_rand(m, n, seed=seed + 3))
    return x, w, b, res


def _gemm_acc32(x, w, ks=1, kdrop=0):
    """fp32 accumulation, K split into ks slices each summed in fp32 and the slabs added in fp32 (the split-K reduce)."""
    k = x.shape[1] - kdrop
    bounds = [round(i * k / ks) for i in range(ks + 1)]
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for a, b in zip(bounds[:-1], bounds[1:]):
        acc = acc + f32(x[:, a:b]) @ f32(w[:, a:b]).t()
    return acc


def _gemm_cases():
    """(name, got, ref64, scale, legit?) for out = silu(alpha (x w^T + b)) + res."""
    out = []
    alpha = 0.75
    for (m, k, n, seed) in [(300, 320, 960, 1), (129, 64, 40, 5), (77, 768, 320, 9), (1, 320, 1280, 13), (4096, 1280, 320, 17),
                            (1024, 2560, 192, 21), (260, 320, 4, 25), (260, 320, 3, 29)]:
        x, w, b, res = _gemm_operands(m, k, n, seed)
        ref = F.silu(alpha * (x @ w.t() + b)) + res
        s = gemm_scale(x, w, b, alpha=alpha, residual=res)
        tag = f"{m}x{k}x{n}"

        def epi(acc, alpha_first=False, bias_cols=n, rnd=rne):
            bb = f32(b).clone()
            bb[bias_cols:] = 0
            z = alpha * acc + bb if alpha_first else alpha * (acc + bb)
            return rnd(F.silu(z) + f32(res))
        acc = _gemm_acc32(x, w)
        out.append((f"legit fp32 {tag}", epi(acc), ref, s, True))
        for ks in (2, 5, 8):
            if k >= 64 * ks:
                out.append((f"legit split-K {ks} {tag}", epi(_gemm_acc32(x, w, ks)), ref, s, True))
        # reversed K order, fp32
        out.append((f"legit reversed-K {tag}", epi(f32(x.flip(1)) @ f32(w.flip(1)).t()), ref, s, True))
        if m * n >= 4096:
            out.append((f"mutant truncation {tag}", epi(acc, rnd=trunc), ref, s, False))
        if k <= 1280:
            out.append((f"mutant last 32 of K dropped {tag}", epi(_gemm_acc32(x, w, kdrop=32)), ref, s, False))
        if k <= 768:
            out.append((f"mutant last 8 of K dropped {tag}", epi(_gemm_acc32(x, w, kdrop=8)), ref, s, False))
        if n % 8 == 0 and n >= 16:
            out.append((f"mutant bias missing on last 8 columns {tag}", epi(acc, bias_cols=n - 8), ref, s, False))
        out.append((f"mutant alpha before bias {tag}", epi(acc, alpha_first=True), ref, s, False))
        if m > 1:
            g = epi(acc)
            g[-1] = g[-2]
            out.append((f"mutant ragged tail row copies neighbour {tag}", g, ref, s, False))
        if m * n >= 20000:               # (a 2^-7 scale error is inside the sampling noise of ~1k outputs)
            out.append((f"mutant alpha x (1 + 2^-7) {tag}", rne(F.silu(alpha * (1 + 2 ** -7) * (acc + f32(b))) + f32(res)), ref,
                        s, False))
    # convolution, cancellation-heavy: nonzero-mean activations, zero-mean weights (|ref| << s); Cin = 4 padded; upsample
    for (bsz, h, w_, cin, cout, up, mean, seed) in [(2, 16, 16, 64, 96, False, 2.0, 41), (2, 16, 16, 4, 320, False, 0.0, 45),
                                                     (1, 8, 12, 32, 48, True, 0.0, 49)]:
        x = q(_rand(bsz, cin, h, w_, seed=seed) + mean)
        wt = q(_rand(cout, cin, 3, 3, seed=seed + 1, scale=1 / math.sqrt(cin * 9)))
        if mean:
            wt = q(wt - wt.mean((1, 2, 3), keepdim=True))
        bias = _rand(cout, seed=seed + 2).double()
        xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
        ref = F.conv2d(xin, wt, bias, padding=1)
        s = conv_scale(xin, wt, bias)
        tag = f"conv {bsz}x{h}x{w_}x{cin}->{cout}{' up' if up else ''}{' mean' if mean else ''}"
        acc = F.conv2d(f32(xin), f32(wt), None, padding=1)
        out.append((f"legit fp32 {tag}", rne(acc + f32(bias)[:, None, None]), ref, s, True))
        out.append((f"mutant truncation {tag}", trunc(acc + f32(bias)[:, None, None]), ref, s, False))
        out.append((f"mutant alpha x (1 + 2^-7) {tag}", rne((1 + 2 ** -7) * (acc + f32(bias)[:, None, None])), ref, s, False))
        wd = wt.clone()
        wd[:, -1] = 0                                                    # the last input channel (a K slice of 9) dropped
        out.append((f"mutant last channel of K dropped {tag}", rne(F.conv2d(f32(xin), f32(wd), f32(bias), padding=1)), ref, s,
                    False))
    # fused GEGLU epilogue: value / gate GEMMs in fp32, fp32 gelu, RNE
    m, k, f = 512, 320, 256
    x, w, b, _ = _gemm_operands(m, k, 2 * f, 61)
    h = x @ w.t() + b
    ref = h[:, :f] * F.gelu(h[:, f:])
    mv = gemm_scale(x, w[:f], b[:f])
    mg = gemm_scale(x, w[f:], b[f:])
    s = geglu_gemm_scale(h[:, :f], h[:, f:], mv, mg)
    h32 = _gemm_acc32(x, w) + f32(b)
    out.append(("legit fused geglu", rne(h32[:, :f] * F.gelu(h32[:, f:])), ref, s, True))
    out.append(("mutant fused geglu tanh-gelu", rne(h32[:, :f] * F.gelu(h32[:, f:], approximate="tanh")), ref, s, False))
    out.append(("mutant fused geglu truncation", trunc(h32[:, :f] * F.gelu(h32[:, f:])), ref, s, False))
    return out


# ------------------------------------------------------------------ flash attention
LOG2E = 1.4426950408889634


def _attn_ref(qq, kk, vv, scale, causal=False):
    """float64 softmax(q k^T scale) v and the softmax weights (heads folded into the leading dim)."""
    sc = (qq @ kk.transpose(-1, -2)) * scale
    if causal:
        sc = sc + torch.full(sc.shape[-2:], float("-inf"), dtype=torch.float64).triu_(1)
    p = torch.softmax(sc, -1)
    return p @ vv, p


def _attn_emul(qq, kk, vv, scale, *, causal=False, causal_shift=0, kt=64, level_bf16=False, l_from_bf16=False, rnd=rne,
               pad_keys=0, rnd_p=rne):
    """The kernels' online softmax: 64-key tiles, fp32 logits in the log2 domain, running level m (rounded to bf16 like v4 when
    level_bf16), p = exp2(s - m) rounded to bf16 for the P V MFMA, l summed from fp32 p (or from the bf16 p: the ones row),
    O rescaled when the level moves, RNE output.  pad_keys appends zero keys with zero values that are NOT masked (mutant)."""
    if pad_keys:
        kk = torch.cat([kk, torch.zeros(*kk.shape[:-2], pad_keys, kk.shape[-1], dtype=kk.dtype)], -2)
        vv = torch.cat([vv, torch.zeros(*vv.shape[:-2], pad_keys, vv.shape[-1], dtype=vv.dtype)], -2)
    nq, nk = qq.shape[-2], kk.shape[-2]
    s_all = (f32(qq) @ f32(kk).transpose(-1, -2)) * torch.tensor(scale * LOG2E, dtype=torch.float32)
    if causal:
        s_all = s_all + torch.full((nq, nk), float("-inf")).triu_(1 + causal_shift)
    m = torch.full((*qq.shape[:-1], 1), float("-inf"))
    l = torch.zeros(*qq.shape[:-1], 1)
    o = torch.zeros(*qq.shape[:-1], vv.shape[-1])
    for k0 in range(0, nk, kt):
        st = s_all[..., k0:k0 + kt]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        if level_bf16:
            m_new = torch.where(torch.isfinite(m_new), m_new.to(BF).float(), m_new)
            m_new = torch.maximum(m_new, m)
        alpha = torch.where(torch.isfinite(m), torch.exp2(m - m_new), torch.zeros_like(m))
        p = torch.exp2(st - m_new)
        p = torch.where(torch.isfinite(m_new), p, torch.zeros_like(p))
        pb = rnd_p(p).float()
        l = l * alpha + (pb if l_from_bf16 else p).sum(-1, keepdim=True)
        o = o * alpha + pb @ f32(vv[..., k0:k0 + kt, :])
        m = m_new
    return rnd(o / l)


def attn_operands(heads, nq, nk, d, seed, shift=4.0):
    """bf16 q, k, v [heads, n, d] with two features that make tail slips visible: every logit is shifted by -shift (q[..., 0] = 1,
    k[..., 0] = -shift sqrt(d): softmax-invariant, but an unmasked zero key gets e^shift times its fair weight) and the LAST key is
    planted on query nq // 2 (4 x its direction: that query's output is dominated by the last key)."""
    qq = _rand(heads, nq, d, seed=seed)
    kk = _rand(heads, nk, d, seed=seed + 1)
    vv = q(_rand(heads, nk, d, seed=seed + 2))
    qq[..., 0] = 1.0
    kk[..., 0] = -shift * math.sqrt(d)
    if nk > 1:
        kk[:, -1] = 4.0 * qq[:, nq // 2]
    return q(qq), q(kk), vv


def _attn_cases():
    out = []
    for (d, heads, nq, nk, causal, seed) in [(40, 2, 130, 77, False, 1), (64, 3, 77, 77, True, 5), (48, 1, 100, 513, False, 9),
                                             (80, 2, 300, 1090, False, 13), (40, 1, 257, 2048 + 31, False, 17),
                                             (40, 2, 64, 1, False, 21), (40, 4, 200, 1024, False, 25)]:
        qq, kk, vv = attn_operands(heads, nq, nk, d, seed)
        sc = d ** -0.5
        ref, p = _attn_ref(qq, kk, vv, sc, causal)
        s = attn_scale(p, vv)
        tag = f"d={d} nq={nq} nk={nk}{' causal' if causal else ''}"
        emu = functools.partial(_attn_emul, qq, kk, vv, sc, causal=causal)
        out.append((f"legit v1 (64-key tiles, fp32 l) {tag}", emu(), ref, s, True))
        out.append((f"legit 128-key tiles, bf16 l (ones row) {tag}", emu(kt=128, l_from_bf16=True), ref, s, True))
        out.append((f"legit v4 (bf16 level, 32-key steps) {tag}", emu(kt=32, level_bf16=True, l_from_bf16=True), ref, s, True))
        if nk > 1:                           # (one key: the output IS a bf16 row of V, nothing to round)
            out.append((f"mutant truncation {tag}", emu(rnd=trunc), ref, s, False))
        if not causal:                       # (with nq = nk a key past nk is causally masked anyway)
            out.append((f"mutant one unmasked zero key past nk {tag}", emu(pad_keys=1), ref, s, False))
        if nk > 1:
            out.append((f"mutant last key dropped {tag}", _attn_emul(qq, kk[:, :-1], vv[:, :-1], sc, causal=causal), ref, s, False))
            out.append((f"mutant scale (d+8)^-0.5 {tag}", _attn_emul(qq, kk, vv, (d + 8) ** -0.5, causal=causal), ref, s, False))
            out.append((f"mutant scale x (1 + 2^-5) {tag}", _attn_emul(qq, kk, vv, sc * (1 + 2 ** -5), causal=causal), ref, s,
                        False))
        if causal:
            out.append((f"mutant causal mask shifted by one {tag}", emu(causal_shift=1), ref, s, False))
    return out


# ------------------------------------------------------------------ norms
def _ln_emul(x, g, b, eps, onepass=False, rnd=rne, eps_used=None, unbiased=False):
    """fp32 LayerNorm over the last dim; onepass: fp32 sum / sum of squares over contiguous 64-element pieces, combined in fp64 (a
    legitimate summation order; the GroupNorm kernels' own layout is restated by gn_kernel_stats)."""
    eps = eps if eps_used is None else eps_used
    xf = f32(x)
    n = x.shape[-1]
    if onepass:
        xs = xf.reshape(*xf.shape[:-1], -1, 64) if n % 64 == 0 else xf.unsqueeze(-2)
        s1 = xs.sum(-1).double().sum(-1, keepdim=True)
        s2 = (xs * xs).sum(-1).double().sum(-1, keepdim=True)
        mu = s1 / n
        var = (s2 / n - mu * mu).clamp_min(0)
        if unbiased:
            var = var * n / (n - 1)
        rstd = (1 / torch.sqrt(var + eps)).float()
        xhat = (xf - mu.float()) * rstd
    else:
        mu = xf.mean(-1, keepdim=True)
        var = (xf - mu).pow(2).sum(-1, keepdim=True) / (n - 1 if unbiased else n)
        xhat = (xf - mu) * torch.rsqrt(var + eps)
    return rnd(xhat * f32(g) + f32(b))


def _ln_ref(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    xhat = (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    return xhat * g.double() + b.double(), xhat


def mu_rstd(x, eps):
    """mean / sqrt(var + eps) over the last dim (keepdim): the size of the kernels' cancelling scale / shift terms."""
    return x.mean(-1, keepdim=True) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)


def _gn_to_rows(x, groups):
    """NHWC [B, HW, C] -> [B, G, HW * C/G] (a group's elements on the last dim) and back."""
    bsz, hw, c = x.shape
    return x.reshape(bsz, hw, groups, c // groups).permute(0, 2, 1, 3).reshape(bsz, groups, -1)


def _gn_from_rows(y, hw, c, groups):
    bsz = y.shape[0]
    return y.reshape(bsz, groups, hw, c // groups).permute(0, 2, 1, 3).reshape(bsz, hw, c)


def _gn_geometry(c8):
    """saspa_norm.hip gn_geometry: cxw chunk columns (8 channels each) per block, slabs of cxw chunks."""
    if c8 <= 16:
        return c8, 1
    for d in range(128, 15, -1):
        if c8 % d == 0 and (256 // d) * d >= 230:
            return d, c8 // d
    return 32, (c8 + 31) // 32


def gn_kernel_stats(x, groups, eps, onepass=False, nsplit=None, combine32=False):
    """The GroupNorm statistics exactly as the kernels form them (their documented rounding points), x [B, HW, C] bf16 values:
    - two-pass (saspa_norm.hip gn_partial_kernel, 24-105): block (split, slab); thread (pixel row py, chunk) sums its pixels
      pbeg + py, + rows, ... in fp32 (v * v exact for bf16 v); the rows of a chunk column are summed in fp32 in row order, the
      channels of a group inside the slab in fp32 in channel order, and those fp32 partials are combined in fp64 (160-185);
    - one-pass (gn_onepass_kernel, 381-425; hw * cpg <= 8192, cpg % 8 == 0): thread tid sums items tid + 256 i (i = 0..3, 8
      channels each) in fp32, combined in fp64.
    Returns (mean, rstd) as the fp32 values the apply pass uses, [B, groups].  The E[x^2] - mean^2 of fp32 partials is where a
    mean offset cancels (mu / sigma = 64: 12 bits); restating it here keeps the reference honest about that design, and the
    CPU proof pins how far it may drift from the exact statistics.  combine32: the partials summed in fp32."""
    from saspa_aug_amd.ops import _gn_nsplit
    bsz, hw, c = x.shape
    cpg = c // groups
    xf = x.float()
    if onepass:
        cp8 = cpg // 8
        v = xf.reshape(bsz, hw, groups, cp8, 8).permute(0, 2, 1, 3, 4).reshape(bsz, groups, hw * cp8, 8)
        v = F.pad(v, (0, 0, 0, 1024 - hw * cp8)).reshape(bsz, groups, 4, 256, 8)
        sm = torch.zeros(bsz, groups, 256)
        sq = torch.zeros(bsz, groups, 256)
        for i in range(4):
            for j in range(8):
                t = v[:, :, i, :, j]
                sm = sm + t
                sq = sq + t * t
        if combine32:
            sm, sq = sm.sum(-1).double(), sq.sum(-1).double()
        else:
            sm, sq = sm.double().sum(-1), sq.double().sum(-1)
    else:
        c8 = c // 8
        cxw, slabs = _gn_geometry(c8)
        rows = 256 // cxw
        ns = nsplit or _gn_nsplit(bsz, hw, c8)
        pps = (hw + ns - 1) // ns
        trips = (pps + rows - 1) // rows
        v = F.pad(xf, (0, 0, 0, ns * pps - hw)).reshape(bsz, ns, pps, c)            # zero pixels add exactly nothing
        v = F.pad(v, (0, 0, 0, trips * rows - pps)).reshape(bsz, ns, trips, rows, c)
        s1 = torch.zeros(bsz, ns, rows, c)
        s2 = torch.zeros(bsz, ns, rows, c)
        for t in range(trips):
            s1 = s1 + v[:, :, t]
            s2 = s2 + v[:, :, t] * v[:, :, t]
        a1 = torch.zeros(bsz, ns, c)
        a2 = torch.zeros(bsz, ns, c)
        for r in range(rows):
            a1 = a1 + s1[:, :, r]
            a2 = a2 + s2[:, :, r]
        gidx = torch.arange(groups) * cpg
        p1 = torch.zeros(bsz, ns, slabs, groups)
        p2 = torch.zeros(bsz, ns, slabs, groups)
        for z in range(slabs):
            ch0, ch1 = z * cxw * 8, min(c, (z + 1) * cxw * 8)
            for j in range(cpg):
                ch = gidx + j
                inside = (ch >= ch0) & (ch < ch1)
                p1[:, :, z] = p1[:, :, z] + torch.where(inside, a1[:, :, ch], torch.zeros(()))
                p2[:, :, z] = p2[:, :, z] + torch.where(inside, a2[:, :, ch], torch.zeros(()))
        if combine32:
            sm, sq = p1.sum((1, 2)).double(), p2.sum((1, 2)).double()
        else:
            sm, sq = p1.double().sum((1, 2)), p2.double().sum((1, 2))
    n = float(cpg * hw)
    mean = sm / n
    var = (sq / n - mean * mean).clamp_min(0)
    return mean.float().double(), (1.0 / torch.sqrt(var + eps)).float().double()


def gn_kernel_ref(x, g, b, groups, eps, **kw):
    """float64 GroupNorm of x [B, HW, C] with the kernels' fp32 statistics: (ref, xhat, mean * rstd per element)."""
    bsz, hw, c = x.shape
    mean, rstd = gn_kernel_stats(x, groups, eps, **kw)
    cpg = c // groups
    mc = mean.repeat_interleave(cpg, 1)[:, None, :]
    rc = rstd.repeat_interleave(cpg, 1)[:, None, :]
    xhat = (x.double() - mc) * rc
    return xhat * g.double() + b.double(), xhat, (mc * rc).expand_as(xhat)


def gn_kernel_apply(x, g, b, mean, rstd, groups, rnd=rne):
    """The apply pass: y = x sc + (beta - mean sc), sc = gamma rstd, all fp32 (saspa_norm.hip 106, 436, 543), then the store."""
    cpg = x.shape[-1] // groups
    sc = f32(g)[None, None, :] * rstd.float().repeat_interleave(cpg, 1)[:, None, :]
    sh = f32(b)[None, None, :] - mean.float().repeat_interleave(cpg, 1)[:, None, :] * sc
    return rnd(f32(x) * sc + sh)


def _norm_inputs(kind, shape, seed):
    z = _rand(*shape, seed=seed)
    if kind == "normal":
        return q(z * 2 + 0.5)
    if kind == "lowvar":
        return q(z * 1e-3 + 0.01)
    if kind == "offset":
        return q(z + 64.0)
    raise ValueError(kind)


def _norm_cases():
    out = []
    # LayerNorm rows x C
    for (rows, c, kind, eps, seed) in [(4096, 320, "normal", 1e-5, 1), (77, 768, "lowvar", 1e-5, 5), (77, 768, "lowvar", 1e-6, 7),
                                        (300, 320, "offset", 1e-5, 9)]:
        x = _norm_inputs(kind, (rows, c), seed)
        g, b = 1 + 0.1 * _rand(c, seed=seed + 1), 0.1 * _rand(c, seed=seed + 2)
        ref, xhat = _ln_ref(x, g, b, eps)
        s = norm_scale(xhat, g, b, mu_rstd(x, eps))
        tag = f"layernorm {rows}x{c} {kind} eps={eps:g}"
        out.append((f"legit two-pass fp32 {tag}", _ln_emul(x, g, b, eps), ref, s, True))
        out.append((f"legit one-pass 64-element pieces {tag}", _ln_emul(x, g, b, eps, onepass=True), ref, s, True))
        out.append((f"mutant truncation {tag}", _ln_emul(x, g, b, eps, rnd=trunc), ref, s, False))
        if kind == "normal":
            out.append((f"mutant eps 1e-3 {tag}", _ln_emul(x, g, b, eps, eps_used=1e-3), ref, s, False))
        if kind == "lowvar":
            out.append((f"mutant eps swapped {tag}", _ln_emul(x, g, b, eps, eps_used=1e-6 if eps == 1e-5 else 1e-5), ref, s, False))
            out.append((f"mutant eps x 10 {tag}", _ln_emul(x, g, b, eps, eps_used=eps * 10), ref, s, False))
    # GroupNorm NHWC [B, HW, C]: the reference carries the kernels' fp32 statistics (gn_kernel_stats); two-pass and one-pass layouts
    for (bsz, hw, c, groups, kind, eps, seed) in [(8, 256, 320, 32, "normal", 1e-5, 11), (2, 64, 1280, 32, "lowvar", 1e-5, 13),
                                                  (2, 64, 1280, 32, "lowvar", 1e-6, 15),
                                                  # the GPU file's mean-offset operands (seed 11 + c + hw): few distinct bf16 values
                                                  (2, 256, 320, 32, "offset", 1e-5, 587), (2, 1024, 640, 32, "offset", 1e-5, 1675),
                                                  (2, 64, 1280, 32, "offset", 1e-5, 1355)]:
        x = _norm_inputs(kind, (bsz, hw, c), seed)
        g, b = 1 + 0.1 * _rand(c, seed=12 + c), 0.1 * _rand(c, seed=13 + c)     # (as the GPU file draws them)
        layouts = [False] + ([True] if (c // groups) % 8 == 0 and hw * (c // groups) <= 8192 else [])
        for op in layouts:
            ref, xhat, mr = gn_kernel_ref(x, g, b, groups, eps, onepass=op)
            s = norm_scale(xhat, g, b, mr)
            mean, rstd = gn_kernel_stats(x, groups, eps, onepass=op)
            tag = f"groupnorm {bsz}x{hw}x{c}/{groups} {kind} eps={eps:g} {'one-pass' if op else 'two-pass'}"
            rows = _gn_to_rows(x, groups)
            y = _gn_from_rows(_ln_emul(rows, torch.ones(1), torch.zeros(1), eps, rnd=f32).float(), hw, c, groups)
            out.append((f"legit kernel statistics, fp32 scale / shift {tag}", gn_kernel_apply(x, g, b, mean, rstd, groups), ref, s,
                        True))
            out.append((f"legit kernel statistics, fp32 (x - mean) rstd gamma + beta {tag}",
                        rne((f32(x) - mean.float().repeat_interleave(c // groups, 1)[:, None])
                            * rstd.float().repeat_interleave(c // groups, 1)[:, None] * f32(g) + f32(b)), ref, s, True))
            out.append((f"mutant truncation {tag}", gn_kernel_apply(x, g, b, mean, rstd, groups, rnd=trunc), ref, s, False))
            if kind == "normal":
                n = hw * c // groups
                out.append((f"mutant n-1 variance {tag}",
                            gn_kernel_apply(x, g, b, mean, (rstd ** -2 * n / (n - 1)) ** -0.5, groups), ref, s, False))
                if not op:
                    out.append((f"legit exact statistics, fp32 apply {tag}", rne(y * f32(g) + f32(b)), ref, s, True))
            if kind == "lowvar":
                for e2, nm in [(1e-6 if eps == 1e-5 else 1e-5, "eps swapped"), (eps * 10, "eps x 10")]:
                    r2 = (rstd ** -2 - eps + e2) ** -0.5
                    out.append((f"mutant {nm} {tag}", gn_kernel_apply(x, g, b, mean, r2, groups), ref, s, False))
    return out


# ------------------------------------------------------------------ elementwise
def _elem_cases():
    out = []
    x = q(_rand(123, 2 * 96, seed=38) * 2)
    a, gt = x[:, :96], x[:, 96:]
    ref = a * F.gelu(gt)
    s = elem_scale(a, F.gelu(gt))
    out.append(("legit geglu fp32", rne(f32(a) * F.gelu(f32(gt))), ref, s, True))
    out.append(("mutant geglu tanh-gelu", rne(f32(a) * F.gelu(f32(gt), approximate="tanh")), ref, s, False))
    out.append(("mutant geglu truncation", trunc(f32(a) * F.gelu(f32(gt))), ref, s, False))
    for name, fn, mut in [("silu", F.silu, lambda t: t * torch.sigmoid(1.702 * t)),
                          ("quick-gelu", lambda t: t * torch.sigmoid(1.702 * t), F.silu)]:
        ref = fn(x)
        s = elem_scale(x, torch.sigmoid(1.702 * x if name == "quick-gelu" else x))
        out.append((f"legit {name} fp32", rne(fn(f32(x))), ref, s, True))
        out.append((f"mutant {name} truncation", trunc(fn(f32(x))), ref, s, False))
        out.append((f"mutant {name} swapped for the other", rne(mut(f32(x))), ref, s, False))
    # softmax rows (scale 0.3, causal)
    for causal in (False, True):
        xs = q(_rand(6, 77, 77, seed=27, scale=3.0))
        mask = torch.full((77, 77), float("-inf"), dtype=torch.float64).triu_(1) if causal else 0
        ref = torch.softmax(xs * 0.3 + mask, -1)
        s = elem_scale(ref)
        tag = "causal" if causal else "plain"
        out.append((f"legit softmax fp32 {tag}", rne(torch.softmax(f32(xs) * 0.3 + (mask.float() if causal else 0), -1)), ref, s,
                    True))
        out.append((f"mutant softmax truncation {tag}", trunc(torch.softmax(f32(xs) * 0.3 + (mask.float() if causal else 0), -1)),
                    ref, s, False))
        if causal:
            m2 = torch.full((77, 77), float("-inf")).triu_(2)
            out.append(("mutant softmax causal mask shifted by one", rne(torch.softmax(f32(xs) * 0.3 + m2, -1)), ref, s, False))
    # CFG + DDIM update
    ref, s, emu = cfg_ddim_case()
    out.append(("legit cfg+ddim fp32", emu(), ref, s, True))
    out.append(("mutant cfg+ddim truncation", emu(rnd=trunc), ref, s, False))
    out.append(("mutant cfg+ddim guidance 7.5 -> 7.0", emu(gs=7.0), ref, s, False))
    return out


CFG_COEF = dict(a_t=0.3, a_p=0.45, gs=7.5)


def cfg_ddim_ref(eps, xx, a_t, a_p, gs):
    """float64 CFG + DDIM update and its magnitude: out = A x + B e with e = (1 - gs) eps_u + gs eps_c."""
    n = xx.shape[0]
    eu, ec = eps[:n].double(), eps[n:].double()
    e = eu + gs * (ec - eu)
    sa_t, s1m_t, sa_p, s1m_p = a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5
    ref = sa_p * (xx.double() - s1m_t * e) / sa_t + s1m_p * e
    A, B = sa_p / sa_t, s1m_p - sa_p * s1m_t / sa_t
    s = (A * xx.double()).abs() + abs(B) * (abs(1 - gs) * eu.abs() + gs * ec.abs())
    return ref, s.clamp_min(2.0 ** -10 * s.mean().item())


def cfg_ddim_case():
    eps = q(_rand(4, 300, 4, seed=42))
    xx = q(_rand(2, 300, 4, seed=43))
    ref, s = cfg_ddim_ref(eps, xx, **CFG_COEF)

    def emu(rnd=rne, gs=CFG_COEF["gs"]):
        eu, ec = f32(eps[:2]), f32(eps[2:])
        e = eu + gs * (ec - eu)
        a_t, a_p = CFG_COEF["a_t"], CFG_COEF["a_p"]
        x0 = (f32(xx) - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
        return rnd(a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e)
    return ref, s, emu


# ------------------------------------------------------------------ f32x3 (fp32 storage, three bf16 MFMAs per product)
def split_hi_lo(a):
    hi = a.float().to(BF).float()
    return hi, (a.float() - hi).to(BF).float()


def f32x3_emul(x, w, b, drop_hilo=False):
    xh, xl = split_hi_lo(x)
    wh, wl = split_hi_lo(w)
    acc = xh @ wh.t() + (0 if drop_hilo else xh @ wl.t()) + xl @ wh.t()
    return (acc + b.float()).double()


def _f32x3_cases():
    out = []
    for (m, k, n, seed) in [(1000, 512, 320, 80), (256, 1280, 640, 84), (300, 96, 40, 88)]:
        x = (_rand(m, k, seed=seed) * 3 + 0.3).double()
        w = _rand(n, k, seed=seed + 1, scale=1 / math.sqrt(k)).double()
        b = _rand(n, seed=seed + 2).double()
        ref = x @ w.t() + b
        s = gemm_scale(x, w, b)
        tag = f"{m}x{k}x{n}"
        out.append((f"legit x3 {tag}", f32x3_emul(x, w, b), ref, s, True))
        out.append((f"legit exact fp32 {tag}", (f32(x) @ f32(w).t() + f32(b)).double(), ref, s, True))
        out.append((f"mutant hi*lo term dropped {tag}", f32x3_emul(x, w, b, drop_hilo=True), ref, s, False))
        out.append((f"mutant alpha x (1 + 2^-12) {tag}", f32x3_emul(x * (1 + 2 ** -12), w, b), ref, s, False))
        out.append((f"mutant plain bf16 product {tag}", (split_hi_lo(x)[0] @ split_hi_lo(w)[0].t() + f32(b)).double(), ref, s,
                    False))
    return out


# ------------------------------------------------------------------ fused transformer-block chains
# saspa_xattn_block, saspa_ff_block and the A-stationary GEMM's fused forms hand bf16 intermediates from stage to stage in
# registers.  Each *_ref below is the float64 chain on the bf16 operands with RNE-to-bf16 applied exactly where the kernel packs
# (every rounding point cites its source line in csrc/), and the chain magnitude of tests/errbudget.py; each *_emul is the same
# chain in fp32 with the summation orders the kernels are free to choose -- and, by option, one slip at a time (the mutants).
XA_C, XA_HEADS, XA_D = 320, 8, 40
XA_QS = XA_D ** -0.5 * LOG2E           # the softmax scale and log2 e, folded into to_q (weights.pack_xattn_w's contract)
LOWVAR_EVERY = 8                       # rows 3 mod 8 of the chain operands have variance 1e-6: there eps decides the result


def f32v(t):
    """A float64 tensor of fp32-representable values (gamma / beta / biases reach the kernels as fp32)."""
    return t.float().double()


def _chain_rows(m, seed, mean, std):
    """bf16 token rows [m, 320]; every LOWVAR_EVERY-th row (from row 3) is 0.01 + 1e-3 z: its variance is a tenth of eps = 1e-5."""
    x = _rand(m, XA_C, seed=seed) * std + mean
    x[3::LOWVAR_EVERY] = _rand(m, XA_C, seed=seed + 50)[3::LOWVAR_EVERY] * 1e-3 + 0.01
    return q(x)


def _mm32(a, w, rev=False):
    """a w^T accumulated in fp32, K ascending or descending."""
    a, w = f32(a), f32(w)
    return a.flip(1) @ w.flip(1).t() if rev else a @ w.t()


def _xa_heads(t, nsamp):
    """[nsamp * n, 320] -> [nsamp, heads, n, 40]."""
    return t.reshape(nsamp, -1, XA_HEADS, XA_D).permute(0, 2, 1, 3)


def _xa_flat(t):
    return t.permute(0, 2, 1, 3).reshape(-1, XA_C)


def xattn_operands(nsamp, ntok, nk, seed, shift=4.0):
    """Operands of saspa_xattn_block that make tail slips visible (attn_operands' two features, through the fused chain):
    - LayerNorm channel 0 is ~1 (beta 1, gamma 1/16) and channel 0 of every head's query reads it alone, channel 0 of every key is
      -shift sqrt(d): every real logit carries a common offset of about -shift (natural log), which the softmax ignores but an
      unmasked zero key at logit 0 does not -- it takes e^shift times its fair weight;
    - the LAST key of sample s is 4 x the reference query of that sample's token ntok // 2: that token's output is the last value;
    - keys and values differ per sample; every LOWVAR_EVERY-th row has variance 1e-6 (eps decides its LayerNorm)."""
    m = nsamp * ntok
    x = _chain_rows(m, seed, 0.3, 1.5)
    gamma, beta = f32v(1 + 0.2 * _rand(XA_C, seed=seed + 1)), f32v(0.1 * _rand(XA_C, seed=seed + 2))
    gamma[0], beta[0] = 1.0 / 16, 1.0
    wq = _rand(XA_C, XA_C, seed=seed + 3, scale=1 / math.sqrt(XA_C))
    wq[::XA_D] = 0.0
    wq[::XA_D, 0] = 1.0
    wq = q(wq * XA_QS)
    wo = q(_rand(XA_C, XA_C, seed=seed + 4, scale=1 / math.sqrt(XA_C)))
    bo = f32v(0.2 * _rand(XA_C, seed=seed + 5))
    k = _rand(nsamp, nk, XA_C, seed=seed + 6)
    v = q(_rand(nsamp, nk, XA_C, seed=seed + 7))
    k[..., ::XA_D] = -shift * math.sqrt(XA_D)
    op = dict(x=x, gamma=gamma, beta=beta, eps=1e-5, wq=wq, wo=wo, bo=bo, v=v, nsamp=nsamp, ntok=ntok, nk=nk)
    if nk > 1:
        qref = rne(rne(_ln_ref(x, gamma, beta, 1e-5)[0]) @ wq.t()) / XA_QS
        k[:, -1] = 4.0 * qref.reshape(nsamp, ntok, XA_C)[:, ntok // 2]
    op["k"] = q(k)
    return op


def xattn_ref(op, res=None):
    """float64 saspa_xattn_block (csrc/saspa_xattn.hip) -> (out [M, 320], chain magnitude).  res: the residual (None: x)."""
    from tests.errbudget import chain_attn_scale, chain_gemm_scale
    x, g, b, eps, ns = op["x"], op["gamma"], op["beta"], op["eps"], op["nsamp"]
    res = x if res is None else res
    ln, xhat = _ln_ref(x, g, b, eps)
    n = rne(ln)                                        # LayerNorm output packed to bf16: saspa_xattn.hip:154-155 (pack8)
    qf = rne(n @ op["wq"].t())                         # Q^T accumulators (bias rows 0..319 are zero) packed: :219-221, :232-233
    qh, kh, vh = _xa_heads(qf, ns), _xa_heads(op["k"], ns), _xa_heads(op["v"], ns)
    s = qh @ kh.transpose(-1, -2)                      # log2-domain logits, fp32; keys >= nk are -inf (:303), here absent
    p = rne(torch.exp2(s - s.amax(-1, keepdim=True)))  # P^T packed to bf16 for the P V MFMA: :312-314
    den = p.sum(-1, keepdim=True)                      # row 40 of V^T is ones: the denominator is the sum of the bf16 P: :324-325
    o = rne((p @ vh) / den)                            # O^T / denominator packed to bf16: :326-334
    of = _xa_flat(o)
    y = rne(of @ op["wo"].t() + op["bo"])              # to_out accumulators (bias = initial value) packed to bf16: finish(), :370-374
    out = y + res                                      # staging tile unpacked, + residual in fp32 (:391-394); the pack that
                                                       # follows (:395) is the output rounding the budget measures
    s_n = norm_scale(xhat, g, b, mu_rstd(x, eps))
    s_q = _xa_heads(chain_gemm_scale(n, op["wq"], prev=s_n), ns)
    s_o = torch.stack([chain_attn_scale(p[i] / den[i], vh[i], o[i], kh[i], s_q[i]) for i in range(ns)])
    return out, chain_gemm_scale(of, op["wo"], op["bo"], prev=_xa_flat(s_o), residual=res)


def xattn_emul(op, res=None, *, rev=False, onepass=False, rnd_p=rne, rnd_o=rne, drop_last=False, pad_keys=0, qscale=1.0, eps_mul=1.0,
               bo_cols=XA_C, res_neighbour=False, prev_sample_keys=False, drop_tail_head=None):
    """The fused chain in fp32: LayerNorm (_ln_emul), to_q, ONE 96-key tile of the online softmax with the denominator summed from
    the bf16 P (_attn_emul, kt = 96, l_from_bf16), to_out with the two-rounding epilogue.  The options are the mutants."""
    x, ns, nk = op["x"], op["nsamp"], op["nk"]
    res = (x if res is None else res).clone()
    if res_neighbour:                                  # the last row of every sample adds its neighbour's residual
        last = torch.arange(1, ns + 1) * op["ntok"] - 1
        res[last] = res[last - 1]
    n = _ln_emul(x, op["gamma"], op["beta"], op["eps"], onepass=onepass, eps_used=op["eps"] * eps_mul)
    qh = _xa_heads(rne(_mm32(n, op["wq"], rev) * qscale), ns).clone()
    if drop_tail_head is not None:                     # the tail block (channels 32..39) of one head left out of Q K^T
        qh[:, drop_tail_head, :, 32:] = 0.0
    kh, vh = _xa_heads(op["k"], ns), _xa_heads(op["v"], ns)
    if prev_sample_keys:
        kh, vh = kh.roll(1, 0), vh.roll(1, 0)
    if drop_last:
        kh, vh = kh[..., :-1, :], vh[..., :-1, :]
    # (_attn_emul multiplies by scale * log2 e: the queries are already in the log2 domain)
    o = _attn_emul(qh, kh, vh, 1.0 / LOG2E, kt=96, l_from_bf16=True, rnd=rnd_o, rnd_p=rnd_p, pad_keys=pad_keys)
    bo = f32(op["bo"]).clone()
    bo[bo_cols:] = 0.0
    return rne(f32(rne(_mm32(_xa_flat(o), op["wo"], rev) + bo)) + f32(res))


def _one_flip(ref, s):
    """The reference with ONE output a bf16 ulp off, at the element where an ulp is largest against the scale.  With a zero residual
    the reference's last rounding point is the output, so a right kernel differs from it by such flips only -- anywhere: the max
    limit has to grant the worst-placed one."""
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
    i = int((ulp / s).argmax())
    got = ref.clone()
    got.view(-1)[i] += ulp.reshape(-1)[i]
    return got


def _xattn_cases(zero_res=True):
    """Zero residual ('xattn': the branch alone sets the scale; the reference's last rounding point is then the output itself, so
    a right result differs from it by rare one-ulp flips only) or the residual x ('chain_res': the output rounding dominates)."""
    out = []
    shapes = [(2, 256, 77, 101), (2, 256, 33, 111), (3, 128, 1, 121)] if zero_res else [(2, 256, 77, 101)]
    for (nsamp, ntok, nk, seed) in shapes:                                  # (one key: the output is to_out of a row of V)
        op = xattn_operands(nsamp, ntok, nk, seed)
        res = torch.zeros_like(op["x"]) if zero_res else None
        ref, s = xattn_ref(op, res)
        tag = f"xattn {nsamp}x{ntok} nk={nk} {'zero residual' if zero_res else 'residual x'}"
        emu = functools.partial(xattn_emul, op, res)
        out.append((f"legit fp32 {tag}", emu(), ref, s, True))
        out.append((f"legit reversed-K, one-pass LayerNorm statistics {tag}", emu(rev=True, onepass=True), ref, s, True))
        if not zero_res:
            out.append((f"mutant residual of the neighbouring row in a sample's last row {tag}", emu(res_neighbour=True), ref, s,
                        False))
            continue
        out.append((f"legit one output flipped by an ulp, worst placed {tag}", _one_flip(ref, s), ref, s, True))
        out.append((f"mutant to_out bias missing on last 8 columns {tag}", emu(bo_cols=XA_C - 8), ref, s, False))
        if nk == 1:
            continue
        out.append((f"mutant LayerNorm eps x 10 {tag}", emu(eps_mul=10.0), ref, s, False))
        out.append((f"mutant truncating pack of P {tag}", emu(rnd_p=trunc), ref, s, False))
        out.append((f"mutant truncating pack of O {tag}", emu(rnd_o=trunc), ref, s, False))
        out.append((f"mutant last key dropped {tag}", emu(drop_last=True), ref, s, False))
        # (the denominator counts the pad keys, as a ones row over all 96 slots would: with the ones row zero past nk an unmasked
        # zero key changes nothing but the level, which is why the GPU file poisons the pad KEYS and asks for bit-equality)
        out.append((f"mutant keys nk..95 left unmasked (zero logit) {tag}", emu(pad_keys=96 - nk), ref, s, False))
        out.append((f"mutant softmax scale (d+8)^-0.5 {tag}", emu(qscale=math.sqrt(XA_D / (XA_D + 8.0))), ref, s, False))
        out.append((f"mutant sample s reads sample s-1's keys {tag}", emu(prev_sample_keys=True), ref, s, False))
        out.append((f"mutant channels 32..39 of one head dropped from Q K^T {tag}", emu(drop_tail_head=5), ref, s, False))
    return out


def ff_operands(m, f, seed):
    x = _chain_rows(m, seed, 0.2, 1.5)
    return dict(x=x, gamma=f32v(1 + 0.1 * _rand(XA_C, seed=seed + 1)), beta=f32v(0.1 * _rand(XA_C, seed=seed + 2)), eps=1e-5,
                w1=q(_rand(2 * f, XA_C, seed=seed + 3, scale=1 / math.sqrt(XA_C))),
                b1=f32v(_rand(2 * f, seed=seed + 4, scale=0.2) + torch.cat([torch.ones(f), torch.zeros(f)])),
                w2=q((_rand(XA_C, f, seed=seed + 5) + 0.5) / math.sqrt(f)), b2=f32v(_rand(XA_C, seed=seed + 6, scale=0.2)), f=f)


def ff_ref(op, res=None, ln=True):
    """float64 saspa_ff_block (csrc/saspa_ff.hip; the four-wave and the wave-specialised kernel round at the same points) ->
    (out [M, 320], chain magnitude).  res: the residual (None: x)."""
    from tests.errbudget import chain_gemm_scale
    x, g, b, eps, f = op["x"], op["gamma"], op["beta"], op["eps"], op["f"]
    res = x if res is None else res
    s_n = None
    n = x
    if ln:
        lnv, xhat = _ln_ref(x, g, b, eps)
        n = rne(lnv)                                   # LayerNorm output packed to bf16: saspa_ff.hip:151-152 (ws: :411-412)
        s_n = norm_scale(xhat, g, b, mu_rstd(x, eps))
    a = n @ op["w1"].t() + op["b1"]                    # [v ; g], fp32 accumulators with b1 as the initial value: :176-179
    hv, hg = a[:, :f], a[:, f:]
    h = rne(hv * F.gelu(hg))                           # the gated hidden state packed to bf16: :265-266 (ws: :490-491)
    y = rne(h @ op["w2"].t())                          # Y^T accumulators packed into the staging tile BEFORE b2: :281 (ws: :547)
    y = rne(y + op["b2"])                              # + b2 in fp32, packed: :302-303 (ws: :566-567)
    out = y + res                                      # + residual in fp32: :306 (ws: :570); the pack that follows is the
                                                       # output rounding the budget measures
    mv = chain_gemm_scale(n, op["w1"][:f], op["b1"][:f], prev=s_n)
    mg = chain_gemm_scale(n, op["w1"][f:], op["b1"][f:], prev=s_n)
    s_h = geglu_gemm_scale(hv, hg, mv, mg)
    return out, chain_gemm_scale(h, op["w2"], op["b2"], prev=s_h, residual=res)


def _erf_as(x):
    """common.h fast_erf: Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7) in fp32."""
    ax = x.abs()
    t = 1.0 / (0.3275911 * ax + 1.0)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    return torch.copysign(1.0 - poly * torch.exp2(-ax * ax * 1.4426950408889634), x)


def ff_emul(op, res=None, ln=True, *, rev=False, onepass=False, gelu="erf", rnd_h=rne, swap_slice=None, b1_missing_slice=None,
            drop_last32=False, b2_cols=XA_C, skip_ln=False):
    """The fused chain in fp32; value and gate stay fp32 until their product is rounded.  The options are the mutants."""
    x, f = op["x"], op["f"]
    res = x if res is None else res
    n = _ln_emul(x, op["gamma"], op["beta"], op["eps"], onepass=onepass) if ln and not skip_ln else x
    b1 = f32(op["b1"]).clone()
    if b1_missing_slice is not None:
        sl = slice(32 * b1_missing_slice, 32 * b1_missing_slice + 32)
        b1[sl] = 0.0
        b1[f:][sl] = 0.0
    a = _mm32(n, op["w1"], rev) + b1
    hv, hg = a[:, :f].clone(), a[:, f:].clone()
    if swap_slice is not None:                         # one 32-feature slice packed gates first
        sl = slice(32 * swap_slice, 32 * swap_slice + 32)
        hv[:, sl], hg[:, sl] = a[:, f:][:, sl], a[:, :f][:, sl]
    if gelu == "erf":
        gl = F.gelu(hg)
    elif gelu == "tanh":
        gl = F.gelu(hg, approximate="tanh")
    else:
        gl = 0.5 * hg * (1.0 + _erf_as(hg * 0.70710678118654752440))
    h = rnd_h(hv * gl)
    if drop_last32:
        h = h.clone()
        h[:, -32:] = 0.0
    b2 = f32(op["b2"]).clone()
    b2[b2_cols:] = 0.0
    return rne(f32(rne(f32(rne(_mm32(h, op["w2"], rev))) + b2)) + f32(res))


def _ff_cases(zero_res=True):
    out = []
    shapes = [(128, 32, True, 201), (128, 64, True, 211), (256, 1280, True, 221), (256, 1280, False, 231)] if zero_res else \
        [(128, 64, True, 241)]
    for (m, f, ln, seed) in shapes:
        op = ff_operands(m, f, seed)
        res = torch.zeros_like(op["x"]) if zero_res else None
        ref, s = ff_ref(op, res, ln)
        tag = f"ff {m}x{f}{'' if ln else ' no LayerNorm'} {'zero residual' if zero_res else 'residual x'}"
        emu = functools.partial(ff_emul, op, res, ln)
        out.append((f"legit fp32, value and gate fp32 until the product {tag}", emu(), ref, s, True))
        out.append((f"legit reversed-K, one-pass LayerNorm statistics {tag}", emu(rev=True, onepass=True), ref, s, True))
        out.append((f"legit polynomial erf {tag}", emu(gelu="as"), ref, s, True))
        if not zero_res:
            continue
        out.append((f"legit one output flipped by an ulp, worst placed {tag}", _one_flip(ref, s), ref, s, True))
        # tanh-GELU differs from erf-GELU by at most 5e-4, the size of the hidden state's own bf16 rounding; behind 1280 random
        # columns of W2 with a LayerNorm in front it is inside the sampling noise of 256 rows.  It shows where few features are mixed
        # (the GPU file's F = 32 and F = 64 cases) and without the LayerNorm, where the gates are wider.
        if f <= 64 or not ln:
            out.append((f"mutant tanh-gelu {tag}", emu(gelu="tanh"), ref, s, False))
        out.append((f"mutant truncated hidden state {tag}", emu(rnd_h=trunc), ref, s, False))
        out.append((f"mutant value and gate rows of one 32-feature slice swapped {tag}", emu(swap_slice=f // 32 - 1), ref, s, False))
        out.append((f"mutant b1 missing on one slice {tag}", emu(b1_missing_slice=f // 64), ref, s, False))
        out.append((f"mutant last 32 hidden features dropped {tag}", emu(drop_last32=True), ref, s, False))
        out.append((f"mutant b2 missing on last 8 columns {tag}", emu(b2_cols=XA_C - 8), ref, s, False))
        if ln:
            out.append((f"mutant LayerNorm skipped {tag}", emu(skip_ln=True), ref, s, False))
    return out


def as_operands(m, n, seed, kind="normal", geglu=False):
    """A-stationary GEMM operands (K = 320): x of `kind` (_norm_inputs, plus 'const': every third row constant), w, bias,
    LayerNorm gamma / beta, a residual."""
    x = _norm_inputs("normal" if kind == "const" else kind, (m, XA_C), seed)
    if kind == "const":
        x[::3] = q(torch.full((XA_C,), 0.7, dtype=torch.float64))
    return dict(x=x, w=q(_rand(n, XA_C, seed=seed + 1, scale=1 / math.sqrt(XA_C))), b=f32v(_rand(n, seed=seed + 2)),
                gamma=f32v(1 + 0.3 * _rand(XA_C, seed=seed + 3)), beta=f32v(0.2 * _rand(XA_C, seed=seed + 4)),
                res=q(_rand(m, n // 2 if geglu else n, seed=seed + 5)))


def as_ref(op, *, bias=True, residual=False, ln=None, geglu=False):
    """float64 A-stationary GEMM (csrc/saspa_gemm_as.hip) -> (out, chain magnitude).  ln: eps of the fused LayerNorm or None;
    geglu: out = v * gelu(g) with rows 0..N/2-1 of w the values, N/2.. the gates (the UNPACKED order)."""
    from tests.errbudget import chain_gemm_scale
    x, w = op["x"], op["w"]
    b = op["b"] if bias else None
    s_n, n = None, x
    if ln is not None:
        lnv, xhat = _ln_ref(x, op["gamma"], op["beta"], ln)
        n = rne(lnv)                                   # fused LayerNorm output packed to bf16: saspa_gemm_as.hip:211-212
        s_n = norm_scale(xhat, op["gamma"], op["beta"], mu_rstd(x, ln))
    y = n @ w.t() + (0 if b is None else b)
    if geglu:
        f = w.shape[0] // 2
        mv = chain_gemm_scale(n, w[:f], None if b is None else b[:f], prev=s_n)
        mg = chain_gemm_scale(n, w[f:], None if b is None else b[f:], prev=s_n)
        # value and gate stay fp32 accumulators (Done.sv); ONE rounding, of the product (:329-330): the output rounding
        return y[:, :f] * F.gelu(y[:, f:]), geglu_gemm_scale(y[:, :f], y[:, f:], mv, mg)
    if residual:
        # accumulators (bias = initial value) packed to bf16 by finish() (:316), the staging tile unpacked and the residual added
        # in fp32 (:355-359); the pack that follows (:360) is the output rounding.  Without a residual :316 IS the output rounding.
        y = rne(y) + op["res"]
    return y, chain_gemm_scale(n, w, b, prev=s_n, residual=op["res"] if residual else None)


def as_emul(op, *, bias=True, residual=False, ln=None, geglu=False, rev=False, onepass=False, eps_used=None, unbiased=False,
            gate_shift=0):
    x, w = op["x"], op["w"]
    n = x if ln is None else _ln_emul(x, op["gamma"], op["beta"], ln, onepass=onepass, eps_used=eps_used, unbiased=unbiased)
    y = _mm32(n, w, rev) + (f32(op["b"]) if bias else 0.0)
    if geglu:
        f = w.shape[0] // 2
        return rne(y[:, :f] * F.gelu(y[:, f:].roll(gate_shift, 1)))
    y = rne(y)
    return rne(f32(y) + f32(op["res"])) if residual else y


def vt_tail(y, n_split, rows_per_batch):
    """The transposed tail of the Q | K | V^T launch: columns >= n_split of y [M, N] as [batch, N - n_split, rows_per_batch]."""
    return y[:, n_split:].reshape(-1, rows_per_batch, y.shape[1] - n_split).transpose(1, 2)


def _as_plain_cases():
    """The unfused A-stationary forms: they join the 'gemm' family under its limits (the two-rounding residual epilogue is a
    documented rounding point of the reference)."""
    out = []
    for (m, n, seed) in [(257, 64, 301), (449, 320, 305)]:
        op = as_operands(m, n, seed)
        for name, kw in [("plain", dict(bias=False)), ("bias", dict()), ("residual", dict(residual=True))]:
            ref, s = as_ref(op, **kw)
            tag = f"A-stationary {name} {m}x320x{n}"
            out.append((f"legit fp32 {tag}", as_emul(op, **kw), ref, s, True))
            out.append((f"legit reversed-K {tag}", as_emul(op, rev=True, **kw), ref, s, True))
            g = as_emul(op, **kw)
            g[-1] = g[-2]
            out.append((f"mutant ragged last block: its last row copies its neighbour {tag}", g, ref, s, False))
    return out


def _as_cases():
    out = []
    # fused LayerNorm (+ bias); x std 0.5 for the eps 1e-3 mutant (the variance has to be small enough for 1e-3 to matter)
    for (m, n, kind, seed) in [(512, 320, "normal", 311), (384, 320, "lowvar", 315), (384, 64, "offset", 319), (257, 320, "const", 323)]:
        op = as_operands(m, n, seed, kind)
        if kind == "normal":
            op["x"] = q(op["x"] * 0.25)
        ref, s = as_ref(op, ln=1e-5)
        tag = f"A-stationary LayerNorm {m}x320x{n} {kind}"
        out.append((f"legit fp32 {tag}", as_emul(op, ln=1e-5), ref, s, True))
        out.append((f"legit reversed-K, one-pass statistics {tag}", as_emul(op, ln=1e-5, rev=True, onepass=True), ref, s, True))
        if kind == "normal":
            out.append((f"mutant fused LayerNorm n-1 variance {tag}", as_emul(op, ln=1e-5, unbiased=True), ref, s, False))
            out.append((f"mutant fused LayerNorm eps 1e-3 {tag}", as_emul(op, ln=1e-5, eps_used=1e-3), ref, s, False))
        if kind == "lowvar":
            out.append((f"mutant fused LayerNorm eps x 10 {tag}", as_emul(op, ln=1e-5, eps_used=1e-4), ref, s, False))
        g = as_emul(op, ln=1e-5)
        g[-1] = g[-2]
        out.append((f"mutant ragged last block: its last row copies its neighbour {tag}", g, ref, s, False))
    # fused LayerNorm + GEGLU: 160-column packing (N = 320) and 128-column packing (N = 1024)
    for (m, n, seed) in [(256, 320, 331), (256, 1024, 335)]:
        op = as_operands(m, n, seed, geglu=True)
        ref, s = as_ref(op, ln=1e-5, geglu=True)
        tag = f"A-stationary LayerNorm + GEGLU {m}x320x{n}"
        out.append((f"legit fp32, value and gate fp32 until the product {tag}", as_emul(op, ln=1e-5, geglu=True), ref, s, True))
        out.append((f"legit reversed-K, one-pass statistics {tag}", as_emul(op, ln=1e-5, geglu=True, rev=True, onepass=True), ref, s,
                    True))
        pack = (160 if n % 160 == 0 else 128) // 2
        out.append((f"mutant fused-GEGLU gate and value from different 128-column packs {tag}",
                    as_emul(op, ln=1e-5, geglu=True, gate_shift=pack), ref, s, False))
    # Q | K | V^T: 4 samples of 128 rows, the row-major part and the transposed tail budgeted separately
    op = as_operands(512, 960, 341)
    ref, s = as_ref(op, bias=False, ln=1e-5)
    for rev in (False, True):
        g = as_emul(op, bias=False, ln=1e-5, rev=rev, onepass=rev)
        nm = "reversed-K, one-pass statistics" if rev else "fp32"
        out.append((f"legit {nm} Q | K row-major part", g[:, :640], ref[:, :640], s[:, :640], True))
        out.append((f"legit {nm} V^T tail", vt_tail(g, 640, 128), vt_tail(ref, 640, 128), vt_tail(s, 640, 128), True))
    gt = vt_tail(as_emul(op, bias=False, ln=1e-5), 640, 128).clone()
    gt[:-1, :, -1] = gt[1:, :, 0]
    out.append(("mutant V^T tail: first row of sample s+1 where the last row of sample s belongs", gt, vt_tail(ref, 640, 128),
                vt_tail(s, 640, 128), False))
    return out


def _bf16_only(cases):
    """The fp8 W8A8 path and the sampler-step references exist for the default bf16 library only (fp8 and the fp16 compute mode
    exclude each other; tests/fp8_ref.py and tests/sampler_ref.py round to bf16 themselves): when tests/fp16_budget.py re-runs a family
    with this module's rounding switched to fp16, they stay out."""
    return cases() if BF is torch.bfloat16 else []


def _gemm_family_cases():
    """... the fp8 W8A8 GEMM (tests/fp8_ref.py: random operands, plain and residual forms) and the conv epilogue forms that
    models.resnet() launches (tests/resnet_ref.py: time-embedding row, residual + alpha, stride 2, concat, the 1x1 shortcut, K
    slices; they round through this module's q / rne and follow the fp16 re-run -- but for the residual forms: two fp16 roundings
    of a sum whose K is only 576 measure 0.327 in tests/fp16_budget.py's typical-magnitude rms, a hair above half its limit of 0.65,
    and that table belongs to the fp16 tests)."""
    return _gemm_cases() + _as_plain_cases() + _bf16_only(lambda: fp8_ref.gemm_cases(_rand)) + \
        resnet_ref.conv_cases(_rand, residual_forms=BF is torch.bfloat16)


def _elem_family_cases():
    """... the fp8 GEMM's GEGLU epilogue on exact operands (tests/fp8_ref.py) and ONE update of the multistep sampler kernels
    (tests/sampler_ref.py)."""
    return _elem_cases() + _bf16_only(lambda: fp8_ref.geglu_cases(_rand) + sampler_ref.elem_cases(_rand))


def _e4m3_cases():
    """The fp8 emission of the fp8 GEMM's GEGLU epilogue: decoded bytes x scale against float64, in units of 2^-4."""
    return fp8_ref.e4m3_cases(_rand)


def _gnstat_cases():
    """The GroupNorm statistics a producer's epilogue leaves (SaspaGemmParams.gn_stats; bf16 only), in units of 2^-24."""
    return _bf16_only(lambda: resnet_ref.gnstat_cases(_rand))


def _gn_chain_cases():
    """conv -> bf16 -> GroupNorm -> SiLU (saspa_splitk_groupnorm)."""
    return _bf16_only(lambda: resnet_ref.gn_chain_cases(_rand))


def _conv_gn_cases():
    """GroupNorm -> SiLU -> bf16 -> 3x3 conv (saspa_conv3x3_halo and the two launches it replaces; bf16 only)."""
    return _bf16_only(lambda: resnet_ref.conv_gn_cases(_rand))


def _f32_gemm_cases():
    """The exact-fp32 GEMM / conv / split-K path (SASPA_F32 on the fp32 MFMA) with every epilogue form, in units of 2^-24
    (tests/f32_ref.py; fp32 families do not follow the fp16 re-run)."""
    return f32_ref.gemm_cases(_rand)


def _f32_gemm_pos_cases():
    """... on non-negative operands (the bilinear attention pooling product): no cancellation, a budget of its own."""
    return f32_ref.gemm_cases(_rand, f32_ref.GEMM_POS_CASES)


def _f32_pool_cases():
    """saspa_pool2d's average form, fp32 storage."""
    return f32_ref.pool_cases(_rand, torch.float32)


def _f32_pool_bf16_cases():
    """saspa_pool2d's average form, bf16 storage (units of 2^-8)."""
    return f32_ref.pool_cases(_rand, torch.bfloat16)


def _f32_tail_cases():
    """saspa_signsqrt_l2norm."""
    return f32_ref.tail_cases(_rand)


def _f32_norm_cases():
    """layernorm / groupnorm on fp32 storage (the bf16 cases with the output rounding removed)."""
    return f32_ref.norm_cases(_rand)


def _f32_softmax_cases():
    return f32_ref.softmax_cases(_rand)


def _f32_elem_cases():
    """geglu / SiLU / quick-GELU on fp32 storage."""
    return f32_ref.elem_cases(_rand)


def _chain_res_cases():
    """The chains with the residual kept (x itself): the output rounding of branch + residual dominates the error."""
    return _xattn_cases(zero_res=False) + _ff_cases(zero_res=False)


FAMILIES = {"gemm": (_gemm_family_cases, UNIT_BF16), "attn": (_attn_cases, UNIT_BF16), "norm": (_norm_cases, UNIT_BF16),
            "elem": (_elem_family_cases, UNIT_BF16), "e4m3": (_e4m3_cases, fp8_ref.UNIT_E4M3), "f32x3": (_f32x3_cases, UNIT_F32X3), "xattn": (_xattn_cases, UNIT_BF16),
            "ff": (_ff_cases, UNIT_BF16), "as": (_as_cases, UNIT_BF16), "chain_res": (_chain_res_cases, UNIT_BF16),
            "gnstat": (_gnstat_cases, resnet_ref.UNIT_GNSTAT), "gn_chain": (_gn_chain_cases, UNIT_BF16),
            "conv_gn": (_conv_gn_cases, UNIT_BF16),
            "f32_gemm": (_f32_gemm_cases, UNIT_F32), "f32_gemm_pos": (_f32_gemm_pos_cases, UNIT_F32),
            "f32_pool": (_f32_pool_cases, UNIT_F32), "f32_pool_bf16": (_f32_pool_bf16_cases, UNIT_BF16),
            "f32_tail": (_f32_tail_cases, UNIT_F32), "f32_norm": (_f32_norm_cases, UNIT_F32),
            "f32_softmax": (_f32_softmax_cases, UNIT_F32), "f32_elem": (_f32_elem_cases, UNIT_F32)}


@functools.lru_cache(maxsize=None)
def _measured(family):
    """Every case of the family on every seed shift in SEEDS (the margins must hold for the operands, not for one draw)."""
    make, unit = FAMILIES[family]
    res = []
    for shift in SEEDS:
        _SEED_SHIFT[0] = shift
        try:
            cases = make()
        finally:
            _SEED_SHIFT[0] = 0
        for name, got, ref, s, legit in cases:
            st = budget_stats(got, ref, s, unit)
            res.append((f"{name} [seeds +{1000 * shift}]", legit, st, ratio(st, LIMITS[family]), (got, ref, s, unit)))
    return res


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_legit_emulations_within_half_the_budget(family):
    rows = [r for r in _measured(family) if r[1]]
    assert rows
    for name, _, st, r, (got, ref, s, unit) in rows:
        print(f"{family:5s} {r:6.3f}  {name}: {fmt(st)}")
        check_budget(got, ref, s, unit, limits=LIMITS[family], what=name)
    worst = max(rows, key=lambda t: t[3])
    assert worst[3] <= LEGIT_MAX, f"{family}: limit less than 2x above legit '{worst[0]}': {fmt(worst[2])} vs {LIMITS[family]}"


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_mutants_rejected_at_twice_the_budget(family):
    rows = [r for r in _measured(family) if not r[1]]
    assert rows
    for name, _, st, r, (got, ref, s, unit) in rows:
        print(f"{family:5s} {r:8.2f}  {name}: {fmt(st)}")
        assert rejects(got, ref, s, unit, limits=LIMITS[family]), name
        with pytest.raises(AssertionError, match="error budget exceeded"):
            check_budget(got, ref, s, unit, limits=LIMITS[family], what=name)
    weakest = min(rows, key=lambda t: t[3])
    assert weakest[3] >= MUTANT_MIN, f"{family}: limit less than 2x below mutant '{weakest[0]}': {fmt(weakest[2])} vs {LIMITS[family]}"


@pytest.mark.parametrize("onepass,shape", [(False, (2, 1024, 640)), (False, (2, 256, 320)), (False, (16, 64, 1280)),
                                           (True, (2, 64, 1280))])
def test_gn_kernel_statistics_cancellation_is_bounded(onepass, shape):
    """The kernels' documented statistics (fp32 partial sums, E[x^2] - mean^2 in fp64: gn_kernel_stats) against the exact ones on
    mu / sigma = 64 inputs, where 12 bits cancel: the variance error per group stays within 4 units of 2^-24 (1 + mu^2 / sigma^2),
    i.e. the cancellation of ONE fp32 rounding of the sum of squares, not of a sum accumulated in a coarser way.  (On the MI355X
    the kernel reproduces these statistics: the GroupNorm offset cases of test_errbudget_gpu.py use them as the reference.)"""
    x = _norm_inputs("offset", shape, 7)
    mean, rstd = gn_kernel_stats(x, 32, 0.0, onepass=onepass)
    rows = _gn_to_rows(x, 32)
    mu, var = rows.mean(-1), rows.var(-1, unbiased=False)
    rel = (rstd.pow(-2) / var - 1).abs() / (2.0 ** -24 * (1 + mu * mu / var))
    print(f"{shape} one-pass={onepass}: worst variance error {rel.max().item():.3f} x 2^-24 (1 + mu^2 / sigma^2)")
    assert rel.max().item() <= 4.0
    assert ((mean - mu).abs() <= 2.0 ** -23 * mu.abs()).all()


@pytest.mark.parametrize("rgs", [8, 16, 32])
@pytest.mark.parametrize("c", [320, 960])
def test_epilogue_form_statistics_cancellation_is_bounded(c, rgs):
    """The same bound for the statistics a producer's epilogue leaves (fp32 sums per 128-row block and unit of 10 channels in the
    order of gn_tile_stats, combined in fp64: resnet_ref.epilogue_form_stats) on mu / sigma = 64 inputs; the GroupNorm cases of
    test_resnet_errbudget_gpu.py that are fed by epilogue statistics take them as their reference there."""
    x = _norm_inputs("offset", (2, 16, 24, c), 7)
    st = resnet_ref.gnstat_emul(x, 10, rgs).reshape(2, -1, 32, c // 320, 2).sum((1, 3))
    n = 16 * 24 * c // 32
    mean = st[..., 0] / n
    var_k = st[..., 1] / n - mean * mean
    rows = _gn_to_rows(x.reshape(2, -1, c), 32)
    mu, var = rows.mean(-1), rows.var(-1, unbiased=False)
    rel = (var_k / var - 1).abs() / (2.0 ** -24 * (1 + mu * mu / var))
    print(f"C = {c}, {rgs} row groups: worst variance error {rel.max().item():.3f} x 2^-24 (1 + mu^2 / sigma^2)")
    assert rel.max().item() <= 4.0
    assert ((mean - mu).abs() <= 2.0 ** -23 * mu.abs()).all()


def test_catalogue_is_complete():
    """Every mutant the issue lists is in the catalogue (a rename that drops one shows up here)."""
    names = " | ".join(r[0] for fam in FAMILIES for r in _measured(fam) if not r[1])
    for want in ["truncation", "unmasked zero key", "last key dropped", "last 8 of K", "last 32 of K", "bias missing on last 8",
                 "alpha before bias", "tail row copies", "causal mask shifted", "(d+8)^-0.5", "eps swapped", "eps 1e-3",
                 "n-1 variance", "tanh-gelu", "hi*lo term dropped", "layernorm", "groupnorm",
                 # the fused transformer-block chains
                 "truncating pack of P", "truncating pack of O", "last key dropped xattn", "keys nk..95 left unmasked",
                 "softmax scale (d+8)^-0.5 xattn", "LayerNorm eps x 10 xattn", "to_out bias missing on last 8 columns",
                 "residual of the neighbouring row in a sample's last row", "sample s reads sample s-1's keys",
                 "channels 32..39 of one head dropped from Q K^T",
                 "tanh-gelu ff", "truncated hidden state", "value and gate rows of one 32-feature slice swapped",
                 "b1 missing on one slice", "last 32 hidden features dropped", "b2 missing on last 8 columns", "LayerNorm skipped",
                 "fused LayerNorm n-1 variance", "fused LayerNorm eps 1e-3",
                 "fused-GEGLU gate and value from different 128-column packs",
                 "V^T tail: first row of sample s+1 where the last row of sample s belongs",
                 "ragged last block: its last row copies its neighbour A-stationary",
                 # the fp8 W8A8 GEMM (tests/fp8_ref.py)
                 "truncating tile pack fp8 gemm", "truncating final pack fp8 gemm", "last K-tile dropped fp8 gemm",
                 "sa of the neighbouring row fp8 gemm", "sw of the neighbouring 4-column group fp8 gemm",
                 "fp8 bias missing on last 8 columns", "tanh-gelu in the fp8 geglu",
                 "value and gate halves of one 128-column tile swapped fp8 geglu", "emission rounding toward zero",
                 "out_scale applied twice",
                 # ONE update of the sampler steps (tests/sampler_ref.py)
                 "truncating stores cfg_unipc", "truncating stores unipc", "truncating stores cfg_plms",
                 "truncating stores ddim without cfg", "truncating stores vae_sample_noise", "guidance 7.0 cfg_unipc",
                 "guidance 7.0 cfg_plms", "UniPC predictor reads m1 for the old m0", "UniPC corrector skipped",
                 "PLMS history weights rotated by one slot", "exp(logvar) for exp(0.5 logvar)",
                 # the ResnetBlock2D path (tests/resnet_ref.py): conv epilogue forms, epilogue statistics, the two fused chains
                 "time-embedding row of the neighbouring image in a tile that spans two images",
                 "bottom-row taps read the next image's top row instead of zero padding", "rowvec missing on columns 256..319",
                 "second concat source's last 32 channels dropped from one tap", "residual added before alpha",
                 "bias added once per K slice", "truncating store conv",
                 "statistics of the unrounded fp32 accumulators", "statistics taken before the residual add",
                 "row 127 of a block left out", "unit u reads the columns of unit u+1 at a tile's last unit",
                 "intermediate kept in fp32 (rounding point skipped)", "alpha applied after the rounding",
                 "rowvec of image b-1 splitk_gn", "eps x 10 splitk_gn", "n-1 variance splitk_gn",
                 "tail items beyond a multiple of 256 left out of the statistics",
                 "zero padding applied before the normalisation", "normalised input truncated to bf16", "eps x 10 conv_gn",
                 "n-1 variance conv_gn", "scale / shift of the previous 32-channel chunk for a chunk's first tap",
                 "SiLU skipped on the halo rows", "a chunk that straddles groups takes the first group's statistics",
                 # the exact-fp32 kernels (tests/f32_ref.py)
                 "bf16x3 split operands f32", "operands truncated to tf32", "bias rounded to bf16 f32",
                 "residual rounded to bf16 f32", "output through bf16 f32", "last 4 of K dropped f32", "last 32 of K dropped f32",
                 "bias missing on the last 4 columns f32", "alpha applied before the bias f32",
                 "ragged tail row copies its neighbour f32", "ReLU before the residual where ADD_RELU was asked",
                 "ReLU after the residual where RELU was asked", "scalar-tail columns take column 0's bias",
                 "bf16x3 split operands f32 bap", "1 / (k*k - 1) avgpool", "last tap row left out avgpool",
                 "accumulation in bf16 avgpool", "eps counted for exact zeros signsqrt_l2norm", "eps = 1e-12 signsqrt_l2norm",
                 "norm taken before the sign-sqrt signsqrt_l2norm",
                 "output through bf16 f32 layernorm", "gamma rounded to bf16 f32 layernorm", "eps 1e-3 f32 layernorm",
                 "n-1 variance f32 layernorm", "eps swapped f32 layernorm", "one-pass fp32 statistics f32 layernorm",
                 "output through bf16 f32 groupnorm", "n-1 variance f32 groupnorm", "eps x 10 f32 groupnorm",
                 "output through bf16 f32 softmax_rows", "logits through bf16 f32 softmax_rows",
                 "scale x (1 + 2^-12) f32 softmax_rows", "causal mask shifted by one f32 softmax_rows",
                 "f32 geglu tanh-gelu", "f32 silu swapped for quick-gelu", "f32 quick-gelu swapped for silu",
                 "f32 geglu output through bf16"]:
        assert want in names, want


def test_checker_message_and_nonfinite():
    ref = _rand(64, 64, seed=3).double()
    got = rne(ref)
    st = check_budget(got, ref, ref.abs() + 0.1, UNIT_BF16, limits=LIMITS["elem"], what="ok")
    assert st["max"] <= 1.0
    bad = got.clone()
    bad[3, 5] += 0.25
    with pytest.raises(AssertionError) as ei:
        check_budget(bad, ref, ref.abs() + 0.1, UNIT_BF16, limits=LIMITS["elem"], what="one bad element")
    msg = str(ei.value)
    for k in ("max", "rms", "bias", "slope", "limits", "(3, 5)"):
        assert k in msg, (k, msg)
    nan = got.clone()
    nan[0, 0] = float("nan")
    assert rejects(nan, ref, ref.abs() + 0.1, UNIT_BF16, limits=LIMITS["elem"])
