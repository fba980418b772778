"""References for saspa_flash_attn_f32x3 (tests only): the float64 attention of the fp32 operands, an fp32 emulation with the kernel's
split, product order, tile size and rescale rule, seven mutants, the operands, the per-output magnitude and the limit table that the
host and the GPU file share.

The kernel (csrc/saspa_attn_x3.hip): every fp32 operand x is split as hi = bf16(x), lo = bf16(x - hi), round to nearest; a product
sum is lo hi + hi lo + hi hi accumulated in fp32 (A operand first: K for the logits, V for the weighted values), chained over
16-channel steps (logits; the head dimension zero-padded to a multiple of 16) and 16-key steps (weighted values); 64-key tiles; the
fp32 logit times the fp32 constant scale * log2(e); running maximum m, p = exp2(t - m), row sum and rescale factor exp2(m_old -
m_new) in fp32; p split from its fp32 value; O accumulated in fp32 and divided by the row sum.

Magnitude.  Write the result as o_ic = sum_j p_ij v_jc with p the normalised weights of the natural-log logits t_ij = scale sum_c
q_ic k_jc.  One x3 product a b is wrong by at most 2^-17 |a b| (errbudget.UNIT_F32X3), so
  (1) the weighted values are wrong by at most 2^-17 sum_j p_ij |v_jc|                            (errbudget.attn_scale's term), and
  (2) a logit is wrong by at most dt_ij = 2^-17 scale sum_c |q_ic| |k_jc|.  A normalised weighted mean answers a change of its logits
      with do_ic = sum_j p_ij dt_ij (v_jc - o_ic) to first order (the derivative of softmax, the -o_ic from the denominator), hence by
      at most 2^-17 scale sum_j p_ij (|q_i| . |k_j|) |v_jc - o_ic|.
s_ic = sum_j p_ij |v_jc| + scale sum_j p_ij (|q_i| . |k_j|) |v_jc - o_ic| is errbudget.chain_attn_scale with the query's per-element
scale |q| and logit_unit = scale (natural-log logits, one unit of error per product).  Term (2) is not small: with logits of standard
deviation 2 and |q| . |k| ~ (2 / pi) d amp^2 it is several times term (1), and it is what keeps a dominant key (v_j = o_i) from being
charged for its own logit.  The fp32 steps (exp2, the sums, the division) add 2^-24 each, 2^-7 of a unit: inside the margin.

Limits.  Measured, not fixed in advance: tests/test_attn_x3_host.py runs the emulation and every mutant over CASES x
test_errbudget.SEEDS and asserts the project's rule -- every limit at least 2 x above what the legitimate emulation produces, and
every mutant at least 2 x above the table on at least one statistic, in every case it applies to.  profiles/attn_x3_errbudget.txt has
every row.  Legitimate emulation, worst over the 24 rows: max 0.980 (0.74 .. 0.98 in every case: the bound of 2^-17 per product is
nearly met at the outputs one key dominates), rms 0.0746, |bias| 0.00267, |slope| 0.155.  Weakest row of each mutant (ratio = max over
the statistics of |stat| / allowance against LIMITS; the statistics that carry it):
  Q K^T on hi hi only      ratio 52                        (max and rms)
  P rounded to one bf16    ratio 12                        (rms 1.8 .. 7.3, max 7 .. 94)
  V on hi only             ratio 196                       (max and rms)
  truncating split         ratio 3.3                       (bias -0.096 .. -0.21 at a standard error of 1e-3 .. 4e-3, slope -3.1 .. -6.5;
                                                            max 2.5 .. 3.9 and rms 0.17 .. 0.35 alone would not hold both margins)
  one pad key unmasked     ratio 9.7                       (bias -0.21 and slope -11 at 1000 keys, everything at 77; cases with a key tail)
  causal mask j >= i       inf                             (query 0 loses its only key; the causal case)
  scale without log2(e)    ratio 6.3e3
Every mutant is rejected at twice the table in every case it applies to; none has to be named as missed."""
import functools
import math

import numpy as np
import torch

from tests import errbudget as E

LOG2E = 1.4426950408889634
KT = 64                                   # keys per tile of the kernel
UNIT = E.UNIT_F32X3

# (B, heads, nq, nk, d, causal)
CASES = (
    (1, 1, 64, 64, 64, False),            # one tile, no padding
    (2, 3, 100, 77, 40, False),           # query and key tails, d padded to the MFMA step, batch and head strides, slices of wider buffers
    (1, 2, 130, 1000, 80, False),         # many key tiles plus a tail: the online rescale
    (1, 2, 77, 77, 64, True),             # the CLIP text tower
    (1, 2, 257, 257, 88, False),          # the BLIP-2 ViT head
    (1, 1, 33, 300, 160, False),          # widest head
)
MUTANTS = ("qk_hihi", "p_bf16", "v_hi", "trunc_split", "pad_unmasked", "causal_ge", "no_log2e")

# 2 x the worst legitimate value of each statistic over CASES x SEEDS (see the docstring), rounded up to two digits
MEASURED_WORST = dict(max=0.9796, rms=0.07461, bias=0.002668, slope=0.1548)
LIMITS = dict(max=2.0, rms=0.15, bias=0.0054, slope=0.31)


def case_id(c):
    return f"B{c[0]}-h{c[1]}-nq{c[2]}-nk{c[3]}-d{c[4]}" + ("-causal" if c[5] else "")


def applies(mutant, case):
    """pad_unmasked needs a pad key (nk not a multiple of the tile), causal_ge a causal case; the others apply everywhere."""
    if mutant == "pad_unmasked":
        return case[3] % KT != 0
    if mutant == "causal_ge":
        return case[5]
    return True


def operands(b, heads, nq, nk, d, seed, amp=math.sqrt(2.0)):
    """q [b, nq, heads * d], k, v [b, nk, heads * d] in fp32:
    - plain fp32 normal draws: 24-bit mantissas, NOT bf16-representable, so a dropped lo term shows;
    - q, k ~ amp N(0, 1) with amp^2 = 2: scaled logits of standard deviation about 2, a peaked softmax (few keys carry a row, an
      error of one weight is not averaged away);
    - the LAST key of every head is planted on query nq // 2 (that query's output is dominated by it: a dropped or unmasked tail
      key shows)."""
    g = torch.Generator().manual_seed(3000 + seed)
    q = amp * torch.randn(b, nq, heads * d, generator=g)
    k = amp * torch.randn(b, nk, heads * d, generator=g)
    v = torch.randn(b, nk, heads * d, generator=g)
    if nk > 1:
        k[:, -1, :] = 2.0 * q[:, nq // 2, :] / amp
    return q, k, v


def _heads(t, heads):
    """[b, n, heads * d] -> [b, heads, n, d]"""
    b, n, c = t.shape
    return t.reshape(b, n, heads, c // heads).permute(0, 2, 1, 3)


def _flat(t):
    """[b, heads, n, d] -> [b, n, heads * d]"""
    b, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, n, h * d)


def _mask(nq, nk, causal, ge=False):
    """True where key j is masked for query i."""
    i = torch.arange(nq)[:, None]
    j = torch.arange(nk)[None, :]
    return (j >= i) if ge else (j > i) if causal else torch.zeros(nq, nk, dtype=torch.bool)


def ref64(q, k, v, heads, scale, causal=False):
    """float64 attention from the fp32 operands -> (out [b, nq, heads * d], magnitude s of the docstring, same shape)."""
    qh, kh, vh = (_heads(t.double(), heads) for t in (q, k, v))
    t = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        t = t.masked_fill(_mask(q.shape[1], k.shape[1], True), -math.inf)
    p = torch.softmax(t, -1)
    o = p @ vh
    s = E.chain_attn_scale(p, vh, o, kh, qh.abs(), logit_unit=scale)
    return _flat(o), _flat(s)


def rne_bf16(x):
    return x.to(torch.bfloat16).float()


def trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def split(x, rnd=rne_bf16):
    hi = rnd(x)
    return hi, rnd(x - hi)


def emul(q, k, v, heads, scale, causal=False, mutant=None):
    """The kernel in fp32 (see the docstring) -> [b, nq, heads * d].  mutant: one of MUTANTS or None."""
    assert mutant is None or mutant in MUTANTS
    rnd = trunc_bf16 if mutant == "trunc_split" else rne_bf16
    qf, kf, vf = (_heads(t.float(), heads) for t in (q, k, v))
    nq, nk, d = qf.shape[-2], kf.shape[-2], qf.shape[-1]
    pad = 1 if mutant == "pad_unmasked" else 0            # one zero key behind the last one takes part
    if pad:
        kf = torch.cat([kf, torch.zeros_like(kf[..., :1, :])], -2)
        vf = torch.cat([vf, torch.zeros_like(vf[..., :1, :])], -2)
    qh, ql = split(qf, rnd)
    kh, kl = split(kf, rnd)
    vh, vl = split(vf, rnd)
    if mutant == "v_hi":
        vl = torch.zeros_like(vl)
    # logits: one fp32 chain over 16-channel steps, lo hi + hi lo + hi hi with K first
    s_all = torch.zeros(*qf.shape[:-1], nk + pad)
    for c0 in range(0, d, 16):
        sl = slice(c0, c0 + 16)
        if mutant != "qk_hihi":
            s_all = s_all + qh[..., sl] @ kl[..., sl].transpose(-1, -2)
            s_all = s_all + ql[..., sl] @ kh[..., sl].transpose(-1, -2)
        s_all = s_all + qh[..., sl] @ kh[..., sl].transpose(-1, -2)
    c = np.float32(scale) * (np.float32(1.0) if mutant == "no_log2e" else np.float32(LOG2E))
    t_all = s_all * torch.tensor(c, dtype=torch.float32)
    if causal:
        mask = _mask(nq, nk + pad, True, ge=mutant == "causal_ge")
        if pad:
            mask[:, nk:] = False
        t_all = t_all.masked_fill(mask, -math.inf)
    m = torch.full((*qf.shape[:-1], 1), -1e30)
    l = torch.zeros(*qf.shape[:-1], 1)
    o = torch.zeros(*qf.shape[:-1], d)
    for k0 in range(0, nk + pad, KT):
        t = t_all[..., k0:k0 + KT]
        m_new = torch.maximum(m, t.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(t - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha
        ph, pl = split(p, rnd)
        if mutant == "p_bf16":
            pl = torch.zeros_like(pl)
        for j0 in range(0, t.shape[-1], 16):               # 16-key steps, lo hi + hi lo + hi hi with V first
            js, ks = slice(j0, j0 + 16), slice(k0 + j0, k0 + j0 + 16)
            o = o + ph[..., js] @ vl[..., ks, :]
            o = o + pl[..., js] @ vh[..., ks, :]
            o = o + ph[..., js] @ vh[..., ks, :]
        m = m_new
    return _flat(o / l)


@functools.lru_cache(maxsize=None)
def case_data(case, seed=0):
    """(q, k, v, scale, ref64, magnitude) of one case; computed once, shared, never modified."""
    b, heads, nq, nk, d, causal = case
    q, k, v = operands(b, heads, nq, nk, d, seed=seed + 7 * CASES.index(case))
    scale = d ** -0.5
    ref, s = ref64(q, k, v, heads, scale, causal)
    return q, k, v, scale, ref, s


def stats(got, case, seed=0):
    *_, ref, s = case_data(case, seed)
    return E.budget_stats(got, ref, s, UNIT)


def check(got, case, seed=0, what=""):
    *_, ref, s = case_data(case, seed)
    return E.check_budget(got, ref, s, UNIT, limits=LIMITS, what=what or f"flash_attn_f32x3 {case_id(case)}")
