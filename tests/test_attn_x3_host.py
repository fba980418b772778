"""Host side of the fused fp32 attention with x3 products and of the fp32 mode switch (no GPU):
- the limit table of saspa_flash_attn_f32x3 (tests/attn_x3_ref.py) holds both margins for every case and seed;
- every validation code of the entry point comes back before any launch; ABI and export lists;
- ops.f32_attn_mode and pipe.set_f32_mode on the host."""
import ctypes as C
import os
import re

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops
from saspa_aug_amd import config as CFG
from saspa_aug_amd import pipeline as P
from tests import attn_x3_ref as A
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
                    got = A.emul(q, k, v, case[1], scale, case[5], mutant=name)
                    _rows.cache.append((case, seed, name or "legit", E.budget_stats(got, ref, s, A.UNIT)))
    return _rows.cache


_rows.cache = []


def report():
    """The text of profiles/attn_x3_errbudget.txt."""
    out = ["saspa_flash_attn_f32x3: error statistics of the fp32 emulation and its mutants against the float64 reference",
           "(tests/attn_x3_ref.py), in units of 2^-17 of the magnitude derived there; ratio = max |stat| / allowance against the table.",
           f"table (2 x worst legitimate value): {A.LIMITS}", ""]
    for case, seed, name, st in _rows():
        out.append(f"{A.case_id(case):30s} seed {seed} {name:12s} {E.fmt(st)}  ratio {E.ratio(st, A.LIMITS):10.3f}")
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
    assert len(rows) >= len(SEEDS)
    for case, seed, st in rows:
        r = E.ratio(st, A.LIMITS)
        print(f"{mutant} {A.case_id(case)} seed {seed}: {E.fmt(st)} ratio {r:.3f}")
        assert r >= 2.0, (mutant, A.case_id(case), seed, r)


def test_profile_file_is_the_report_of_this_table():
    text = open(os.path.join(ROOT, "profiles", "attn_x3_errbudget.txt")).read()
    assert str(A.LIMITS) in text
    assert all(A.case_id(c) in text for c in A.CASES) and all(m in text for m in A.MUTANTS)


# ---- the entry point --------------------------------------------------------------------------------------------------------
_Q, _K, _VT, _O = (1 << 20) * 1, (1 << 20) * 2, (1 << 20) * 3, (1 << 20) * 4      # never dereferenced: every call below is refused


def _params(**over):
    """A valid launch (2 x 3 heads of 40, 100 queries, 77 keys) over operands that are never dereferenced; `over` overwrites fields."""
    p = _lib.AttnParams()
    p.q, p.ldq, p.sqb = _Q, 240, 100 * 240
    p.k, p.ldk, p.skb = _K, 240, 77 * 240
    p.vt, p.ldvt, p.svb = _VT, 80, 120 * 80
    p.o, p.ldo, p.sob = _O, 120, 100 * 120
    p.batch, p.heads, p.D, p.nq, p.nk = 2, 3, 40, 100, 77
    p.scale, p.causal, p.flags = 40 ** -0.5, 0, 0
    for name, v in over.items():
        setattr(p, name, v)
    return p


EINVAL_ROWS = [dict(q=None), dict(k=None), dict(vt=None), dict(o=None),
               dict(batch=0), dict(heads=0), dict(nq=0), dict(nk=0), dict(batch=-1),
               dict(D=0), dict(D=44), dict(D=168), dict(D=-8),
               dict(ldq=116), dict(ldk=116), dict(ldo=116), dict(ldvt=76),
               dict(flags=1), dict(flags=2), dict(flags=3)]
EALIGN_ROWS = [dict(q=_Q + 4), dict(k=_K + 8), dict(vt=_VT + 4), dict(o=_O + 12),
               dict(ldq=242), dict(ldk=241), dict(ldvt=78), dict(ldo=122),
               dict(sqb=100 * 240 + 2), dict(skb=77 * 240 + 1), dict(svb=120 * 80 + 3), dict(sob=100 * 120 + 2)]


@pytest.mark.parametrize("over", EINVAL_ROWS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_invalid_arguments_are_refused_before_any_launch(over):
    assert _lib.load().saspa_flash_attn_f32x3(C.byref(_params(**over)), None) == _lib.SASPA_EINVAL


@pytest.mark.parametrize("over", EALIGN_ROWS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_misaligned_arguments_are_refused_before_any_launch(over):
    assert _lib.load().saspa_flash_attn_f32x3(C.byref(_params(**over)), None) == _lib.SASPA_EALIGN


def test_null_parameter_block_is_refused():
    assert _lib.load().saspa_flash_attn_f32x3(None, None) == _lib.SASPA_EINVAL


def test_abi_and_export_lists():
    lib, f16 = _lib.load(), _lib.load_f16()
    assert lib.saspa_abi_version() == 20 and f16.saspa_abi_version() == 20
    assert "saspa_flash_attn_f32x3" in _lib.SYMBOLS and "saspa_flash_attn_f32x3" not in _lib.F16_SYMBOL_NAMES
    assert hasattr(lib, "saspa_flash_attn_f32x3") and not hasattr(f16, "saspa_flash_attn_f32x3")
    header = open(os.path.join(ROOT, "include", "saspa_hip.h")).read()
    assert re.search(r"\bint saspa_flash_attn_f32x3\(const SaspaAttnParams\* p, void\* stream\);", header)
    mk = open(os.path.join(ROOT, "saspa-aug_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    f16_srcs = re.search(r"^F16_SRCS := (.*)$", mk, re.M).group(1).split()
    assert "saspa_attn_x3.hip" in srcs and "saspa_attn_x3.hip" not in f16_srcs


# ---- the switches -----------------------------------------------------------------------------------------------------------
def test_f32_attn_mode_context_nests_and_restores():
    assert not ops.f32_attn_fused()
    with ops.f32_attn_mode("fused"):
        assert ops.f32_attn_fused()
        with ops.f32_attn_mode("unfused"):
            assert not ops.f32_attn_fused()
        assert ops.f32_attn_fused()
    assert not ops.f32_attn_fused()
    with pytest.raises(ValueError):
        ops.f32_attn_mode("flash")


def test_flash_attn_f32x3_refuses_16_bit_tensors(monkeypatch):
    monkeypatch.setattr(ops, "_check_dev", lambda *ts: None)
    t = torch.zeros(1, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="fp32 path"):
        ops.flash_attn_f32x3(t, t, t, t, 1, 8, 8, 8, 1.0)


def test_set_f32_mode_records_validates_and_refuses_after_to():
    pipe = P.StableDiffusionControlNetPipeline({}, CFG.tiny())
    assert pipe._f32_mode is None and (pipe.f32_gemm, pipe.f32_attn) == ("exact", "unfused")
    assert pipe.set_f32_mode("x3", "fused") is pipe and pipe._f32_mode == ("x3", "fused")
    assert pipe.set_f32_mode(attn="fused")._f32_mode == ("exact", "fused")
    assert pipe.set_f32_mode()._f32_mode == ("exact", "unfused")
    for bad in (dict(gemm="bf16"), dict(attn="flash"), dict(gemm="X3"), dict(gemm=None), dict(attn=1)):
        with pytest.raises(ValueError, match="fp32 (GEMM|attention) mode"):
            pipe.set_f32_mode(**bad)
    assert pipe._f32_mode == ("exact", "unfused")                # a refused call changes nothing
    pipe.unet = object()                                          # what .to() leaves behind
    with pytest.raises(RuntimeError, match="before .to"):
        pipe.set_f32_mode("x3", "fused")


def test_f32_scope_is_empty_by_default_and_in_16_bit():
    pipe = P.StableDiffusionControlNetPipeline({}, CFG.tiny())
    for dt, modes, entered in ((torch.float32, ("exact", "unfused"), False), (torch.bfloat16, ("x3", "fused"), False),
                               (torch.float32, ("x3", "fused"), True), (torch.float32, ("exact", "fused"), True)):
        pipe.dtype, (pipe.f32_gemm, pipe.f32_attn) = dt, modes
        with pipe._f32_scope():
            assert ops.f32_attn_fused() == (entered and modes[1] == "fused")
            assert (ops._F32_GEMM_MODE[0] == "x3") == (entered and modes[0] == "x3")
        assert not ops.f32_attn_fused() and ops._F32_GEMM_MODE[0] == "exact"


if __name__ == "__main__":
    # regenerate the profile:  python -m tests.test_attn_x3_host > profiles/attn_x3_errbudget.txt
    print(report(), end="")
