"""References for saspa_attn_wide_f32x3 (tests only): the float64 attention of one wide head per batch entry, an fp32 emulation with
the kernel's split, product order, wave split of the head dimension, tile size and rescale rule, five mutants, the operands and the
limit table that the host and the GPU file share.

The kernel (csrc/saspa_attn_wide_x3.hip): the arithmetic contract of saspa_flash_attn_f32x3 (tests/attn_x3_ref.py has the derivation
of the magnitude s, used here unchanged through ref64 with one head) on saspa_attn_wide's layout.  Every fp32 operand x is split as
hi = bf16(x), lo = bf16(x - hi), round to nearest; a product sum is lo hi + hi lo + hi hi accumulated in fp32 (A operand first: K for
the logits, V for the weighted values).  The logits are four partial sums -- wave w chains the 32-channel steps s with s % 4 == w --
added in wave order; 32-key tiles; the fp32 logit times the fp32 constant scale * log2(e); running maximum m, p = exp2(t - m), row sum
and rescale factor exp2(m_old - m_new) in fp32; p split from its fp32 value; one 32-key product step per tile into the fp32 O, which
is divided by the row sum.

Limits.  Measured, not fixed in advance: tests/test_attn_wide_x3_host.py runs the emulation and every mutant over CASES x
test_errbudget.SEEDS and asserts the project's rule -- every limit at least 2 x above what the legitimate emulation produces, and
every mutant at least 2 x above the table on at least one statistic, in every case it applies to.
profiles/attn_wide_x3_errbudget.txt has every row; MEASURED_WORST below is its summary line.

Mutants and where they apply (applies()):
  p_bf16         P rounded to one bf16 (its lo plane dropped)
  qk_cross       one cross term of Q K^T dropped (K lo . Q hi)
  pv_cross       one cross term of P V dropped (V lo . P hi; the other cross term IS p_bf16)
  logit_bf16     the scaled logit rounded to bf16 before the softmax
  pad_unmasked   the zero key behind the last one takes part (every case: no nk here is a multiple of the 32-key tile)
NOT SEPARABLE at nk = 1 (the case B1-nq1-nk1-d256), and therefore not applied there: p_bf16, qk_cross and logit_bf16.  With a single
key the softmax weight is exactly 1 whatever the logit is and 1 has no lo part, so these three mutants compute the same bytes as the
kernel.  pv_cross and pad_unmasked do show at nk = 1 and are applied."""
import functools
import math

import numpy as np
import torch

from tests import attn_x3_ref as X
from tests import errbudget as E

LOG2E = X.LOG2E
KT = 32                                   # keys per tile of the kernel
NW = 4                                    # waves the head dimension is split over
UNIT = E.UNIT_F32X3

# (B, nq, nk, d): the smallest shapes at which each failure mode shows -- a single query and key; query and key tails at the narrowest
# head (d / 32 = 6 steps: waves 2 and 3 take one step, waves 0 and 1 two; padded V rows); the widest head (144 KiB of LDS) with several
# key tiles and a tail; a three-entry batch at a width that is no multiple of 128, 9 key tiles: the online rescale
CASES = (
    (1, 1, 1, 256),
    (2, 33, 65, 192),
    (1, 64, 130, 512),
    (3, 40, 257, 320),
)
MUTANTS = ("p_bf16", "qk_cross", "pv_cross", "logit_bf16", "pad_unmasked")

# 2 x the worst legitimate value of each statistic over CASES x SEEDS (profiles/attn_wide_x3_errbudget.txt), rounded up to two digits
MEASURED_WORST = dict(max=0.9735, rms=0.3366, bias=0.03333, slope=0.09315)
LIMITS = dict(max=2.0, rms=0.68, bias=0.067, slope=0.19)


def case_id(c):
    return f"B{c[0]}-nq{c[1]}-nk{c[2]}-d{c[3]}"


def applies(mutant, case):
    """See the docstring: three mutants are the kernel itself where there is one key."""
    if mutant in ("p_bf16", "qk_cross", "logit_bf16"):
        return case[2] > 1
    return True


def operands(b, nq, nk, d, seed):
    """q [b, nq, d], k, v [b, nk, d] in fp32: attn_x3_ref.operands with one head (plain fp32 draws, logits of standard deviation 2,
    the last key planted on query nq // 2)."""
    return X.operands(b, 1, nq, nk, d, seed)


def ref64(q, k, v, scale):
    """float64 attention from the fp32 operands -> (out [b, nq, d], magnitude s, same shape)."""
    return X.ref64(q, k, v, 1, scale)


def emul(q, k, v, scale, mutant=None):
    """The kernel in fp32 (see the docstring) -> [b, nq, d].  mutant: one of MUTANTS or None."""
    assert mutant is None or mutant in MUTANTS
    qf, kf, vf = q.float(), k.float(), v.float()
    nq, nk, d = qf.shape[-2], kf.shape[-2], qf.shape[-1]
    pad = 1 if mutant == "pad_unmasked" else 0            # one zero key behind the last one takes part
    if pad:
        kf = torch.cat([kf, torch.zeros_like(kf[..., :1, :])], -2)
        vf = torch.cat([vf, torch.zeros_like(vf[..., :1, :])], -2)
    qh, ql = X.split(qf)
    kh, kl = X.split(kf)
    vh, vl = X.split(vf)
    # logits: wave w chains its 32-channel steps, lo hi + hi lo + hi hi with K first; the four partials in wave order
    s_all = torch.zeros(*qf.shape[:-1], nk + pad)
    for w in range(NW):
        part = torch.zeros_like(s_all)
        for c0 in range(32 * w, d, 32 * NW):
            sl = slice(c0, c0 + 32)
            if mutant != "qk_cross":
                part = part + qh[..., sl] @ kl[..., sl].transpose(-1, -2)
            part = part + ql[..., sl] @ kh[..., sl].transpose(-1, -2)
            part = part + qh[..., sl] @ kh[..., sl].transpose(-1, -2)
        s_all = s_all + part
    c = np.float32(scale) * np.float32(LOG2E)
    t_all = s_all * torch.tensor(c, dtype=torch.float32)
    if mutant == "logit_bf16":
        t_all = X.rne_bf16(t_all)
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
        ph, pl = X.split(p)
        if mutant == "p_bf16":
            pl = torch.zeros_like(pl)
        ks = slice(k0, k0 + KT)                            # one 32-key step, lo hi + hi lo + hi hi with V first
        if mutant != "pv_cross":
            o = o + ph @ vl[..., ks, :]
        o = o + pl @ vh[..., ks, :]
        o = o + ph @ vh[..., ks, :]
        m = m_new
    return o / l


@functools.lru_cache(maxsize=None)
def case_data(case, seed=0):
    """(q, k, v, scale, ref64, magnitude) of one case; computed once, shared, never modified."""
    b, nq, nk, d = case
    q, k, v = operands(b, nq, nk, d, seed=seed + 7 * CASES.index(case))
    scale = d ** -0.5
    ref, s = ref64(q, k, v, scale)
    return q, k, v, scale, ref, s


def large_operands(nq=40, nk=100, d=512, seed=5):
    """Activations near 30: q . k is about 30 x 30 x 512 = 4.6 x 10^5 before the scale, while the scaled logits of one query differ
    by about one standard deviation only (q = 30 + x, k = 30 + y with every y row of mean zero: 900 d and 30 sum(x) are common to the
    keys of a query, 30 sum(y) is zero, x . y / sqrt(d) remains)."""
    g = torch.Generator().manual_seed(seed)
    x, y, v = torch.randn(1, nq, d, generator=g), torch.randn(1, nk, d, generator=g), torch.randn(1, nk, d, generator=g)
    y = y - y.mean(-1, keepdim=True)
    return 30.0 + x, 30.0 + y, 30.0 + v


def stats(got, case, seed=0):
    *_, ref, s = case_data(case, seed)
    return E.budget_stats(got, ref, s, UNIT)


def check(got, case, seed=0, what=""):
    *_, ref, s = case_data(case, seed)
    return E.check_budget(got, ref, s, UNIT, limits=LIMITS, what=what or f"attn_wide_x3 {case_id(case)}")
