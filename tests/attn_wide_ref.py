"""References for saspa_attn_wide (tests only): the float64 attention of one wide head per batch entry, an fp32 emulation with the
kernel's rounding points, two mutants, the operands and the budget the host and GPU files share.

The kernel (csrc/saspa_attn_wide.hip): 32-key tiles; logits q . k accumulated in fp32 and multiplied by scale * log2(e) in fp32;
running maximum m, p = exp2(s - m) in fp32; the row sum l from the fp32 p; p rounded ONCE to the 16-bit type for the P V MFMA; O
accumulated in fp32, rescaled when m moves, divided by l and rounded ONCE on store.  Nothing else is rounded to 16 bits -- in
particular no logit, which is what separates it from the unfused path (scores GEMM stored in the 16-bit type, row softmax, PV GEMM).

Budget: tests/errbudget.py's statistics in units of 2^-8 (bf16) / 2^-11 (fp16) of s_i = sum_j p_ij |v_j| (errbudget.attn_scale; fp16
with fp16_budget's absolute floor).  tests/test_attn_wide_host.py decides between the flash-attention family's table
(errbudget.LIMITS["attn"]) and a table measured here, by the rule written at LIMITS below."""
import functools
import math

import torch

from tests import errbudget as E
from tests import fp16_budget as FB

LOG2E = 1.4426950408889634
KT = 32                                   # keys per tile of the kernel
UNIT = {torch.bfloat16: E.UNIT_BF16, torch.float16: FB.UNIT_F16}
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}

# (B, nq, nk, d, rows): rows = how many query rows (evenly spread) the references cover, None = all.  The last case is the 1024^2
# decode shape: K / V have 16384 rows, the kernel runs every query, the references are computed for 64 sampled rows.
CASES = (
    (1, 64, 64, 512, None),               # one tile
    (2, 100, 77, 512, None),              # query and key tails, batch stride
    (1, 320, 1000, 512, None),            # many key tiles + tail: the online rescale
    (1, 33, 4096, 256, None),             # other width, long key loop
    (1, 64, 200, 192, None),              # smallest width
    (1, 16384, 16384, 512, 64),           # the 1024^2 shape, 64 sampled rows
)


def case_id(c):
    return f"B{c[0]}-nq{c[1]}-nk{c[2]}-d{c[3]}"


def rne(x, dt):
    """Round to the 16-bit type (nearest even) and back to float32."""
    return x.float().to(dt).float()


def trunc(x, dt):
    """Round to the 16-bit type toward zero (the mutant of rne), as float32."""
    if dt == torch.bfloat16:
        return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)
    return FB.trunc16(x).float()


def operands(b, nq, nk, d, dt, seed, amp=1.5, shift=128.0):
    """q [b, nq, d], k, v [b, nk, d] in the 16-bit type, built so that the slips this kernel exists to avoid are visible:
    - q, k ~ amp N(0, 1): scaled logits of standard deviation amp^2 = 2.25, a peaked softmax (few keys carry a row, so an error of
      one weight is not averaged away);
    - channel 0 shifts every UNSCALED logit by -shift sqrt(d) (q0 = sqrt(d), k0 = -shift): the softmax ignores it, a logit stored
      in 16 bits pays for it (|q . k| ~ 2900 at d = 512: spacing 16 in bf16, 2 in fp16, against a logit unit of sqrt(d) = 22.6;
      in fp32 it costs 2^-12 of a logit unit);
    - the LAST key is planted on query nq // 2 (that query's output is dominated by it: a dropped or unmasked tail key shows)."""
    g = torch.Generator().manual_seed(1000 + seed)
    q = amp * torch.randn(b, nq, d, generator=g)
    k = amp * torch.randn(b, nk, d, generator=g)
    v = torch.randn(b, nk, d, generator=g)
    q[..., 0] = math.sqrt(d)
    k[..., 0] = -shift
    if nk > 1:
        k[:, -1, 1:] = 2.0 * q[:, nq // 2, 1:] / amp
    return q.to(dt), k.to(dt), v.to(dt)


def sample_rows(nq, rows):
    if rows is None or rows >= nq:
        return torch.arange(nq)
    return torch.linspace(0, nq - 1, rows).round().long().unique()


def ref64(q, k, v, scale):
    """float64 softmax(scale q k^T) v from the 16-bit operands -> (out, magnitude s = sum_j p_ij |v_j|)."""
    q, k, v = q.double(), k.double(), v.double()
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
    return p @ v, E.attn_scale(p, v)


def scale_for(s, dt):
    return FB.floor16(s) if dt == torch.float16 else s


def emul(q, k, v, scale, dt, *, kt=KT, logits16=False, rnd_p=rne):
    """The kernel in fp32 with its rounding points.  Mutants: logits16 -- the unscaled q . k rounded to the 16-bit type before the
    softmax (what the unfused path stores); rnd_p=trunc -- P rounded toward zero for the PV product."""
    qf, kf, vf = q.float(), k.float(), v.float()
    raw = qf @ kf.transpose(-1, -2)
    if logits16:
        raw = rne(raw, dt)
    s_all = raw * torch.tensor(scale * LOG2E, dtype=torch.float32)
    nk = k.shape[-2]
    m = torch.full((*q.shape[:-1], 1), -1e30)
    l = torch.zeros(*q.shape[:-1], 1)
    o = torch.zeros(*q.shape[:-1], v.shape[-1])
    for k0 in range(0, nk, kt):
        st = s_all[..., k0:k0 + kt]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(st - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + rnd_p(p, dt) @ vf[..., k0:k0 + kt, :]
        m = m_new
    return rne(o / l, dt)


@functools.lru_cache(maxsize=None)
def case_data(case, dt, seed=0):
    """(q, k, v, scale, rows, ref64 on the sampled rows, magnitude) of one case; computed once, shared, never modified."""
    b, nq, nk, d, rows = case
    q, k, v = operands(b, nq, nk, d, dt, seed=seed + 7 * CASES.index(case))
    idx = sample_rows(nq, rows)
    scale = d ** -0.5
    ref, s = ref64(q[:, idx], k, v, scale)
    return q, k, v, scale, idx, ref, scale_for(s, dt)


# ---- the budget ------------------------------------------------------------------------------------------------------------
# Rule (tests/test_attn_wide_host.py asserts it): the flash-attention family's table errbudget.LIMITS["attn"] is used for a 16-bit
# type if, over CASES, the legitimate emulation stays within HALF of it at d = 512 and both mutants are rejected at TWICE it.
# Otherwise the table is 2 x the emulation's worst value of each statistic over CASES (rounded up to two digits).  Measured
# (profiles/attn_wide_errbudget.txt has every row): see MEASURED below; the host test recomputes the figures and fails if they moved.
FLASH = E.LIMITS["attn"]
# Worst |statistic| of the legitimate emulation over CASES, both 16-bit types (seed 0): max 1.265 (bf16, 2 x 100 x 77), rms 0.2277,
# bias 0.00798, slope 0.01325 (fp16, 64 x 64).  That is within half of FLASH (worst ratio 0.395) -- but FLASH does not reject the
# truncated-P mutant at twice in every case (ratios 0.92 .. 2.67: max and rms of FLASH are sized for d <= 160 heads, and the slip is a
# relative scale error of -0.08 .. -0.18 units that only the slope sees).  So the rule gives the measured table:
MEASURED_WORST = dict(max=1.265, rms=0.2277, bias=0.00798, slope=0.01325)
LIMITS = dict(max=2.6, rms=0.46, bias=0.016, slope=0.027)


def limits_for(dt):
    return LIMITS


def stats(got, case, dt):
    """errbudget statistics of `got` ([B, sampled rows, d], any device / dtype) against the case's float64 reference."""
    *_, ref, s = case_data(case, dt)
    return E.budget_stats(got, ref, s, UNIT[dt])


def check(got, case, dt, what=""):
    *_, ref, s = case_data(case, dt)
    return E.check_budget(got, ref, s, UNIT[dt], limits=limits_for(dt), what=what or f"attn_wide {NAME[dt]} {case_id(case)}")
