"""fp16 forms of the rounding-error budgets (tests only; tests/errbudget.py and tests/test_errbudget.py are the bf16 originals).

The references, magnitudes, emulations and mutants of tests/test_errbudget.py round through three module-level names (BF, trunc,
_one_flip).  `fp16_rounding()` swaps them for their IEEE-fp16 forms for the duration of a `with` block, so the SAME float64 chains --
with the kernels' documented rounding points -- are taken from fp16-rounded operands with RNE-to-fp16 at every hand-off.  The GPU
file does the same to tests/test_errbudget_gpu.py (`gpu_fp16`) and runs its test bodies on fp16 tensors.

What differs from bf16 besides the element type:
- unit = 2^-11 (UNIT_F16);
- the magnitude s_i has an absolute floor of 2^-13 (`floor16`): fp16 underflows gradually, its subnormal spacing 2^-24 is one unit at
  that magnitude (bf16 never gets there);
- errors that are absolute in fp32 terms -- accumulation order, the A&S erf, 1-ulp exp / rcp -- are 8x larger in these units, so a
  family whose limit was set by rare one-ulp flips of a bf16 hand-off needs a table of its own: LIMITS_F16, measured by
  tests/test_fp16_host.py (2x the worst legitimate emulation) and recorded in profiles/fp16_errbudget.txt.
Every table in use must still reject, at twice the limit, the catalogue's mutants AND the same operation carried out with bf16
rounding (the bf16 emulation of tests/test_errbudget.py on the same draws, held against the fp16 reference): the mutant that tells an
f16 launch from one that was routed to the bf16 kernels."""
import contextlib
import functools

import torch

from tests import errbudget as E
from tests import test_errbudget as T

F16 = torch.float16
UNIT_F16 = 2.0 ** -11
S_FLOOR = 2.0 ** -13

# Families whose bf16 limits (errbudget.LIMITS) do not leave legitimate fp16 emulations within half the limit; entries are 2x the
# worst legitimate emulation over tests/test_errbudget.SEEDS (profiles/fp16_errbudget.txt has the measurements), rounded up to two
# digits.  Everything else uses errbudget.LIMITS as it is.
LIMITS_F16 = {
    # torch's fp32 erf-GELU loses its 1 + erf(x) to cancellation in the negative tail: 1.94 units at the 2^-8 floor of elem_scale
    "elem": dict(E.LIMITS["elem"], max=3.9),
    # zero-residual chains: a right result differs from the reference by one-ulp flips of a hand-off, and an fp32 summation-order
    # difference flips an fp16 hand-off 8x as often as a bf16 one (rms 1.11e-3 / 1.42e-3 measured)
    "ff": dict(E.LIMITS["ff"], rms=0.0023),
    "xattn": dict(E.LIMITS["xattn"], rms=0.0029),
}


# The magnitude s_i of the gemm family is a worst-case sum over K (|A| |B|^T), about 0.8 sqrt(K) times the typical |out|: a bf16
# rounding of the output, 2^-9 |out|, is 4 / (0.8 sqrt(K)) units of 2^-11 s -- inside the family's limits for K >= 320, whatever the
# element type of the launch.  What separates f16 from bf16 arithmetic at every K is the error against the TYPICAL magnitude of the
# output: t_i = max(|ref_i|, rms(ref)) (from the reference alone).  RNE to fp16 errs by at most 2^-11 |out|, uniformly: at most
# 1 / sqrt(3) = 0.58 rms in units of 2^-11 t, 0.19 .. 0.33 measured over the gemm catalogue (two roundings in the A-stationary
# residual epilogue); fp32 accumulation adds ~2^-24 sqrt(K) t.  bf16 rounding of operands and output gives 3.2 .. 39.  The limit is
# 2x the worst legitimate emulation; tests/test_fp16_host.py holds every legit row to half of it and every bf16-arithmetic row to
# twice it, and the GPU file asserts it on every GEMM launch and on a bf16 counter-launch of every GEMM kernel.
TYPICAL_RMS_LIMIT = {"gemm": 0.65}


def typical_rms(got, ref64):
    """rms of (got - ref) / (2^-11 t), t_i = max(|ref_i|, rms(ref)): the error in units of the output's typical magnitude."""
    ref = ref64.detach().to("cpu", torch.float64)
    got = got.detach().to("cpu", torch.float64)
    if not torch.isfinite(got).all():
        return float("inf")
    t = ref.abs().clamp_min(max(ref.pow(2).mean().sqrt().item(), S_FLOOR))
    return ((got - ref) / (UNIT_F16 * t)).pow(2).mean().sqrt().item()


# The catalogue's LayerNorm emulations with ONE-PASS statistics (fp32 sum and sum of squares over 64-element pieces) on the
# mean-offset operands (mu / sigma = 64) are no emulation of a kernel: every LayerNorm in csrc/ is two-pass in registers
# (saspa_norm.hip layernorm_kernel, and the fused forms of saspa_gemm_as / saspa_xattn / saspa_ff, which restate it).  The 12 bits
# that E[x^2] - mean^2 cancels there are an fp32 error, 8x larger in fp16 units; against bf16 rounding it hid in the noise
# allowance.  The GroupNorm kernels' one-pass statistics are the kernels' own (gn_kernel_stats) and stay.  The excluded cases by
# name (tests/test_fp16_host.py asserts that each exists in the catalogue, so a rename cannot change the set silently):
NOT_A_KERNEL = {
    "norm": ("legit one-pass 64-element pieces layernorm 300x320 offset eps=1e-05",),
    "as": ("legit reversed-K, one-pass statistics A-stationary LayerNorm 384x320x64 offset",),
}


def emulates_a_kernel(family, name):
    return name not in NOT_A_KERNEL.get(family, ())


def limits_for(family):
    return LIMITS_F16.get(family, E.LIMITS[family])


def floor16(s):
    return s.clamp_min(S_FLOOR) if torch.is_tensor(s) else max(float(s), S_FLOOR)


def trunc16(x):
    """Round to fp16 toward zero (normal and subnormal range alike): the mutant of RNE."""
    x = x.double()
    r = x.float().to(F16).double()
    over = r.abs() > x.abs()                      # RNE went away from zero: step back one fp16 value (sign-magnitude bits - 1)
    bits = r.to(F16).contiguous().view(torch.int16)
    step = torch.where(over, bits - 1, bits).view(F16).double()
    return step


def norm_scale16(xhat, gamma, beta, mu_rstd=None):
    """errbudget.norm_scale with its fp32-cancellation term restated in fp16 units: the kernels' y = x sc + (beta - mean sc) has two
    fp32 terms of magnitude |mean sc| that cancel, 2^-24 of each; that is 2^-15 |mean sc| in units of 2^-8 and 2^-12 |mean sc| in
    units of 2^-11."""
    s = E.norm_scale(xhat, gamma, beta, None)
    if mu_rstd is not None:
        s = s + 2.0 ** -12 * (mu_rstd.double() * gamma.double()).abs()
    return s


def _one_flip16(ref, s):
    """tests/test_errbudget._one_flip with an fp16 ulp (2^-10 of the binade, 2^-24 in the subnormal range)."""
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - 10)
    i = int((ulp / s).argmax())
    got = ref.clone()
    got.view(-1)[i] += ulp.reshape(-1)[i]
    return got


@contextlib.contextmanager
def fp16_rounding():
    """Inside: tests.test_errbudget rounds to fp16 wherever it rounded to bf16 (operands q, hand-offs rne, the truncation mutant,
    the one-ulp flip) and takes the norm magnitude in fp16 units (norm_scale16).  Restores the bf16 forms on exit; nothing built inside may be cached across the boundary."""
    saved = (T.BF, T.trunc, T._one_flip, T.norm_scale)
    T.BF, T.trunc, T._one_flip, T.norm_scale = F16, trunc16, _one_flip16, norm_scale16
    try:
        probe = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -12], dtype=torch.float64)
        assert T.q(probe).tolist() == [1.0 + 2.0 ** -9, 1.0] and T.rne(probe).tolist() == [1.0 + 2.0 ** -9, 1.0], \
            "tests.test_errbudget no longer rounds through its module-level BF: the fp16 references would be bf16 ones"
        yield
    finally:
        T.BF, T.trunc, T._one_flip, T.norm_scale = saved


def fresh_cache(fn):
    """A new lru_cache over the function a cached helper wraps (fp16 operands must not share a cache with the bf16 ones)."""
    return functools.lru_cache(maxsize=None)(getattr(fn, "__wrapped__", fn))
