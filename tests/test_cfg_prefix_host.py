"""saspa_xattn_block_bcast (the fused cross-attention launch reading a CFG-shared x / residual): exported by both libraries, and
its argument validation happens on the host before any launch (no GPU: every call below is refused)."""
import ctypes as C
import os

import pytest

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib

EINVAL, EALIGN, ERANGE = -1, -2, -3


def _params(base, m=512, rps=256):
    p = _lib.XattnBlockParams()
    p.x = p.residual = p.out = p.w = p.bias = p.kf = p.vf = p.ln_gamma = p.ln_beta = base
    p.ldx = p.ldr = p.ldo = p.ldw = 320
    p.M, p.rows_per_sample, p.nk = m, rps, 77
    p.kf_stride, p.vf_stride = 8 * 9 * 1024, 8 * 12 * 1024
    return p


@pytest.fixture()
def base():
    buf = (C.c_char * 64)()
    yield (C.addressof(buf) + 15) // 16 * 16
    del buf


def test_exported_by_both_libraries():
    lib = _lib.load()
    assert hasattr(lib, "saspa_xattn_block_bcast") and "saspa_xattn_block_bcast" in _lib.SYMBOLS
    assert "saspa_xattn_block_bcast" in _lib.F16_SYMBOL_NAMES
    if not os.path.exists(_lib.F16_LIB_PATH):
        pytest.fail(f"{_lib.F16_LIB_PATH} missing: run __graft_entry__.build()")
    f16 = C.CDLL(_lib.F16_LIB_PATH)
    assert hasattr(f16, "saspa_xattn_block_bcast") and hasattr(f16, "saspa_xattn_block")
    assert lib.saspa_abi_version() == 20                    # the parameter struct did not change


def test_x_rows_is_validated_on_the_host(base):
    lib = _lib.load()
    assert lib.saspa_xattn_block_bcast(None, 256, None) == EINVAL
    p = _params(base, m=1024, rps=512)
    assert lib.saspa_xattn_block_bcast(C.byref(p), 0, None) == EINVAL          # no rows
    assert lib.saspa_xattn_block_bcast(C.byref(p), -512, None) == EINVAL
    assert lib.saspa_xattn_block_bcast(C.byref(p), 256, None) == ERANGE        # not whole samples
    assert lib.saspa_xattn_block_bcast(C.byref(p), 768, None) == ERANGE
    p = _params(base, m=768, rps=256)
    assert lib.saspa_xattn_block_bcast(C.byref(p), 512, None) == ERANGE        # whole samples that do not divide M
    assert lib.saspa_xattn_block_bcast(C.byref(p), 1536, None) == ERANGE       # more rows than the output has
    # 32-bit byte offsets: x / residual against x_rows, out against M (first refusal below: out alone is too large)
    p = _params(base, m=4 * 1024 * 1024, rps=256)
    assert lib.saspa_xattn_block_bcast(C.byref(p), 1024 * 1024, None) == ERANGE
    p = _params(base, m=2 * 1024 * 1024, rps=256)
    p.ldx = 1288                                                                 # 1 Mi rows x 2576 B: x alone is too large
    assert lib.saspa_xattn_block_bcast(C.byref(p), 1024 * 1024, None) == ERANGE


def test_x_rows_equal_m_validates_as_xattn_block(base):
    """The null-operand, geometry and alignment cases of test_lib_abi.test_ff_block_host_side_validation, through both entry
    points: the same code from each."""
    lib = _lib.load()

    def both(p, want):
        assert lib.saspa_xattn_block(C.byref(p), None) == want
        assert lib.saspa_xattn_block_bcast(C.byref(p), p.M, None) == want

    assert lib.saspa_xattn_block(None, None) == EINVAL
    p = _lib.XattnBlockParams()
    both(p, EINVAL)                                         # null operands (and M = 0)
    p = _params(base)
    p.ln_beta = None
    both(p, EINVAL)                                         # gamma without beta
    p = _params(base)
    p.nk = 0
    both(p, EINVAL)
    p = _params(base, m=100, rps=100)
    both(p, ERANGE)                                         # rows % 256
    p = _params(base, m=512, rps=128)
    both(p, ERANGE)                                         # a workgroup's 256 rows share one sample
    p = _params(base)
    p.nk = 97
    both(p, ERANGE)
    p = _params(base)
    p.ldo = 300
    both(p, ERANGE)                                         # pitch < 320
    p = _params(base)
    p.ldx = 324
    both(p, EALIGN)                                         # pitch % 8
    p = _params(base)
    p.w = base + 8
    both(p, EALIGN)                                         # alignment
    p = _params(base)
    p.kf_stride = 1024
    both(p, ERANGE)                                         # fragments of fewer than 8 heads
    p = _params(base, m=4 * 1024 * 1024)
    both(p, ERANGE)                                         # 32-bit byte offsets
