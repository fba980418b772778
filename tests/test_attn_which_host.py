"""The loop every attention GPU test expects, checked on the host: the dry plan (ops.flash_attn_which -> saspa_flash_attn_which) needs
no GPU, so the parameter lists of tests/test_kernels_gpu.py, tests/test_attn_v4_gpu.py and the attention cases of
tests/test_errbudget_gpu.py are walked here with the knobs each test sets and the assertion each test makes before it launches.  The
operands are uninitialised host tensors of the tests' shapes (the plan reads shapes, flags and knobs, never memory)."""
import os

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops
from tests import test_attn_v4_gpu as V4
from tests import test_errbudget_gpu as E
from tests import test_kernels_gpu as K

DTYPES = [torch.bfloat16] + ([torch.float16] if os.path.exists(_lib.F16_LIB_PATH) else [])


def _which(bsz, heads, d, nq, nk, causal=False, prescaled=False, rowmajor=False, dtype=torch.bfloat16):
    c = heads * d
    q, k, out = (torch.empty(bsz, n, c, dtype=dtype) for n in (nq, nk, nq))
    v = torch.empty(bsz, nk, c, dtype=dtype) if rowmajor else torch.empty(bsz, c, ops.round8(nk) + 8, dtype=dtype)
    return ops.flash_attn_which(q, k, v, out, heads, d, nq, nk, causal, prescaled, rowmajor) & 15


def _pin(monkeypatch, mode=None, v4=None):
    for name, v in (("SASPA_ATTN_MODE", mode), ("SASPA_ATTN_V4", v4)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    monkeypatch.delenv("SASPA_ATTN_RING", raising=False)


def test_kernel_tests_name_their_loop(monkeypatch):
    for mode in K.PRESCALED_MODES:
        _pin(monkeypatch, mode)
        for d, heads, nq, nk, causal in K.PRESCALED_CASES:
            assert _which(2, heads, d, nq, nk, causal, prescaled=True) == K.prescaled_loop(mode, nk), (mode, d, heads, nq, nk)
    for prescaled in (False, True):
        _pin(monkeypatch, "4" if prescaled else "0")
        for d, heads, nq, nk, causal in K.VROW_CASES:
            got = tuple(_which(K.VROW_BATCH, heads, d, nq, nk, causal, prescaled, rowmajor=rm) for rm in (False, True))
            assert got == K.vrow_loops(prescaled, nk, d), (prescaled, d, heads, nq, nk)
    bsz, heads, d, n = K.LEVEL_MOVE_SHAPE
    for mode in K.LEVEL_MOVE_MODES:
        _pin(monkeypatch, mode)
        assert _which(bsz, heads, d, n, n, prescaled=True) == K.prescaled_loop(mode, n), mode
    assert {K.prescaled_loop(m, n) for m in K.LEVEL_MOVE_MODES} == {2, 3}


def test_v4_tests_name_their_loop(monkeypatch):
    for v4, loop in (("2", 4), ("0", 3)):
        _pin(monkeypatch, "4", v4)
        for bsz, heads, nq, nk in V4.V4_CASES:
            assert _which(bsz, heads, 40, nq, nk, prescaled=True) == loop, (v4, bsz, heads, nq, nk)
    _pin(monkeypatch, "4", "2")
    bsz, heads, d, n = V4.LEVEL_MOVE_SHAPE
    assert _which(bsz, heads, d, n, n, prescaled=True) == 4
    # v4 is the default at the level-0 shape, v3 with SASPA_ATTN_V4=0
    bsz, heads, d, n = V4.LEVEL0_SHAPE
    _pin(monkeypatch)
    assert _which(bsz, heads, d, n, n, prescaled=True) == 4
    _pin(monkeypatch, None, "0")
    assert _which(bsz, heads, d, n, n, prescaled=True) == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t).split(".")[-1])
def test_errbudget_cases_name_their_loop(monkeypatch, dtype):
    ran = set()
    for loop in E.LOOPS:
        mode, v4, prescaled, rowmajor = loop
        _pin(monkeypatch, mode, v4)
        for case in E.ATTN_CASES:
            if E.attn_skip(case, loop):
                continue
            d, heads, nq, nk, causal, _ = case
            want = E.attn_loop(case, loop)
            assert _which(1, heads, d, nq, nk, causal, prescaled, rowmajor, dtype) == want, (case, loop)
            if nk > 1:                                                              # the negative control with one key less
                assert _which(1, heads, d, nq, nk - 1, causal, prescaled, rowmajor, dtype) == want, (case, loop)
            ran.add(want)
    assert ran == {1, 2, 3, 4}                                                      # the budget cases reach every loop
