"""Host side of saspa_attn_wide_f32x3 (no GPU):
- the limit table of tests/attn_wide_x3_ref.py holds both margins for every case and seed, and profiles/attn_wide_x3_errbudget.txt
  is its report;
- every validation code of the entry point comes back before any launch; export lists; the ops wrapper's own refusals."""
import os
import re

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops
from tests import attn_wide_x3_ref as A
from tests import errbudget as E
from tests.test_errbudget import SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    """(case, seed, variant, statistics) of the emulation and the mutants over every case and seed; computed once."""
    if not _rows.cache:
        for case in A.CASES:
            for seed in SEEDS:
                q, k, v, scale, ref, s = A.case_data(case, seed)
                for name in (None,) + A.MUTANTS:
                    if name is not None and not A.applies(name, case):
                        continue
                    got = A.emul(q, k, v, scale, mutant=name)
                    _rows.cache.append((case, seed, name or "legit", E.budget_stats(got, ref, s, A.UNIT)))
    return _rows.cache


_rows.cache = []


def report():
    """The text of profiles/attn_wide_x3_errbudget.txt."""
    out = ["saspa_attn_wide_f32x3: error statistics of the fp32 emulation and its mutants against the float64 reference",
           "(tests/attn_wide_x3_ref.py), in units of 2^-17 of the magnitude derived in tests/attn_x3_ref.py; ratio = max |stat| / allowance",
           f"against the table.  table (2 x worst legitimate value): {A.LIMITS}",
           "not separable, not applied (one key: the weight is exactly 1): p_bf16, qk_cross, logit_bf16 at " + A.case_id(A.CASES[0]), ""]
    for case, seed, name, st in _rows():
        out.append(f"{A.case_id(case):24s} seed {seed} {name:12s} {E.fmt(st)}  ratio {E.ratio(st, A.LIMITS):10.3f}")
    worst = {k: max(abs(st[k]) for _, _, n, st in _rows() if n == "legit") for k in E.STATS}
    out += ["", "worst legitimate value per statistic: " + " ".join(f"{k} {v:.4g}" for k, v in worst.items())]
    for m in A.MUTANTS:
        out.append(f"weakest row of {m:12s}: ratio {min(E.ratio(st, A.LIMITS) for _, _, n, st in _rows() if n == m):.4g}")
    return "\n".join(out) + "\n"


# ---- budget -----------------------------------------------------------------------------------------------------------------
def test_table_is_twice_the_worst_legitimate_value():
    worst = {k: max(abs(st[k]) for _, _, n, st in _rows() if n == "legit") for k in E.STATS}
    print("worst legitimate:", worst)
    for k in E.STATS:
        # (the host BLAS' fp32 summation order moves the last digits of max / rms; bias and slope are means of signed errors, mostly
        # sampling noise, which the allowance covers with its standard-error term)
        assert worst[k] <= A.MEASURED_WORST[k] * (1.05 if k in ("max", "rms") else 1.5), (k, worst[k])
        assert 2.0 * A.MEASURED_WORST[k] <= A.LIMITS[k] <= 2.0 * A.MEASURED_WORST[k] * 1.25, k


def test_emulation_within_half_the_table_in_every_case_and_seed():
    for case, seed, name, st in _rows():
        if name == "legit":
            r = E.ratio(st, A.LIMITS)
            print(f"{A.case_id(case)} seed {seed}: {E.fmt(st)} ratio {r:.3f}")
            assert r <= 0.5 * 1.05, (A.case_id(case), seed, r)


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutant_rejected_at_twice_the_table_wherever_it_applies(mutant):
    rows = [(c, s, st) for c, s, n, st in _rows() if n == mutant]
    assert len(rows) >= len(SEEDS) * (len(A.CASES) - 1)
    for case, seed, st in rows:
        r = E.ratio(st, A.LIMITS)
        print(f"{mutant} {A.case_id(case)} seed {seed}: {E.fmt(st)} ratio {r:.3f}")
        assert r >= 2.0, (mutant, A.case_id(case), seed, r)


def test_single_key_mutants_are_the_kernel_itself():
    """Why three mutants are not applied at nk = 1: they compute the legitimate bytes there."""
    case = A.CASES[0]
    q, k, v, scale, *_ = A.case_data(case)
    legit = A.emul(q, k, v, scale)
    for m in A.MUTANTS:
        assert A.applies(m, case) == (not torch.equal(A.emul(q, k, v, scale, mutant=m), legit)), m


def test_large_activation_operands_have_logits_near_1e5():
    q, k, v = A.large_operands()
    raw = q.double() @ k.double().transpose(-1, -2)
    assert raw.min().item() > 4e5 and (raw.amax(-1) - raw.amin(-1)).max().item() * q.shape[-1] ** -0.5 < 30.0   # per query
    ref, s = A.ref64(q, k, v, q.shape[-1] ** -0.5)
    got = A.emul(q, k, v, q.shape[-1] ** -0.5)
    assert bool(torch.isfinite(got).all())
    print("large activations, emulation:", E.fmt(E.check_budget(got, ref, s, A.UNIT, limits=A.LIMITS, what="large activations")))


def test_profile_file_is_the_report_of_this_table():
    text = open(os.path.join(ROOT, "profiles", "attn_wide_x3_errbudget.txt")).read()
    assert str(A.LIMITS) in text
    assert all(A.case_id(c) in text for c in A.CASES) and all(m in text for m in A.MUTANTS)


# ---- the entry point --------------------------------------------------------------------------------------------------------
_Q, _K, _V, _O = (1 << 20) * 1, (1 << 20) * 2, (1 << 20) * 3, (1 << 20) * 4      # never dereferenced: every call below is refused
_VALID = dict(q=_Q, ldq=960, sqb=40 * 960, k=_K, ldk=960, skb=257 * 960, v=_V, ldv=960, svb=257 * 960, out=_O, ldo=320, sob=40 * 320,
              batch=3, nq=40, nk=257, d=320, scale=320 ** -0.5)
_ORDER = ("q", "ldq", "sqb", "k", "ldk", "skb", "v", "ldv", "svb", "out", "ldo", "sob", "batch", "nq", "nk", "d", "scale")


def _call(**over):
    a = dict(_VALID, **over)
    return _lib.load().saspa_attn_wide_f32x3(*(a[n] for n in _ORDER), None)


EINVAL_ROWS = [dict(q=None), dict(k=None), dict(v=None), dict(out=None),
               dict(batch=0), dict(batch=-1), dict(batch=65536), dict(nq=0), dict(nk=0), dict(nq=-3),
               dict(d=128), dict(d=160), dict(d=200), dict(d=576), dict(d=0),
               dict(ldq=316), dict(ldk=316), dict(ldv=316), dict(ldo=316)]
EALIGN_ROWS = [dict(q=_Q + 4), dict(k=_K + 8), dict(v=_V + 4), dict(out=_O + 12),
               dict(ldq=962), dict(ldk=961), dict(ldv=963), dict(ldo=322),
               dict(sqb=40 * 960 + 2), dict(skb=257 * 960 + 1), dict(svb=257 * 960 + 3), dict(sob=40 * 320 + 2)]


@pytest.mark.parametrize("over", EINVAL_ROWS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_invalid_arguments_are_refused_before_any_launch(over):
    assert _call(**over) == _lib.SASPA_EINVAL


@pytest.mark.parametrize("over", EALIGN_ROWS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_misaligned_arguments_are_refused_before_any_launch(over):
    assert _call(**over) == _lib.SASPA_EALIGN


def test_export_lists():
    lib, f16 = _lib.load(), _lib.load_f16()
    assert "saspa_attn_wide_f32x3" in _lib.SYMBOLS and "saspa_attn_wide_f32x3" not in _lib.F16_SYMBOL_NAMES
    assert hasattr(lib, "saspa_attn_wide_f32x3") and not hasattr(f16, "saspa_attn_wide_f32x3")
    header = open(os.path.join(ROOT, "include", "saspa_hip.h")).read()
    assert re.search(r"\bint saspa_attn_wide_f32x3\(const void\* q, int ldq,", header)
    mk = open(os.path.join(ROOT, "saspa-aug_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    f16_srcs = re.search(r"^F16_SRCS := (.*)$", mk, re.M).group(1).split()
    assert "saspa_attn_wide_x3.hip" in srcs and "saspa_attn_wide_x3.hip" not in f16_srcs


def test_wrapper_refuses_16_bit_tensors_and_strided_last_dims(monkeypatch):
    monkeypatch.setattr(ops, "_check_dev", lambda *ts: None)
    t = torch.zeros(1, 8, 192, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="fp32 path"):
        ops.attn_wide_x3(t, t, t, t, 8, 8, 1.0)
    f = torch.zeros(1, 8, 384)
    with pytest.raises(ValueError, match="contiguous last dim"):
        ops.attn_wide_x3(f[:, :, ::2], f[:, :, ::2], f[:, :, ::2], f[:, :, ::2], 8, 8, 1.0)


if __name__ == "__main__":
    # regenerate the profile:  python -m tests.test_attn_wide_x3_host > profiles/attn_wide_x3_errbudget.txt
    print(report(), end="")
