"""Upsample2D as four 2x2 phase convs over the low-res input (weights.pack_conv_up2x, SaspaGemmParams.upsample = 2): the algebra,
the rounding of the pre-summed weights, and the library's host-side refusals.  No GPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib
from saspa_aug_amd import weights as W

BF = torch.bfloat16
CASES = [(1, 3, 5, 16, 8), (2, 8, 8, 64, 96), (1, 8, 12, 32, 48)]          # (B, H, W, Cin, Cout)


def phase_conv(x, wph, bias=None):
    """The four 2x2 convs of the phase form, in x's dtype: x [B, C, H, W], wph [4, Cout, 4*Cp] (tap-major, as pack_conv_up2x
    returns it; Cp >= C) -> [B, Cout, 2H, 2W].  Phase (py, px) pads (1 - py) rows on top / py below, columns alike."""
    b, c, h, w = x.shape
    co = wph.shape[1]
    cp = wph.shape[2] // 4
    out = torch.zeros((b, co, 2 * h, 2 * w), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            k = wph[py * 2 + px].reshape(co, 2, 2, cp)[..., :c].permute(0, 3, 1, 2).to(x.dtype)
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            out[:, :, py::2, px::2] = F.conv2d(xp, k)
    return out if bias is None else out + bias.to(x.dtype).view(1, -1, 1, 1)


def _operands(case, seed):
    b, h, w, cin, cout = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5)       # the fp32 master weights
    return x, wt


def _direct(x, wt):
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt.double(), padding=1)


@pytest.mark.parametrize("case", CASES)
def test_phase_convs_reproduce_upsample_conv(case):
    x, wt = _operands(case, 7)
    wph = W.pack_conv_up2x(wt)
    assert wph.dtype == torch.float64 and tuple(wph.shape) == (4, case[4], 4 * W.round8(case[3]))
    d = (phase_conv(x, wph) - _direct(x, wt)).abs().max().item()
    print(f"phase convs vs interpolate + conv2d, {case}: max |d| = {d:.3e}")
    assert d <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_presummed_rounding_is_no_worse_than_tapwise(case):
    """One rounding of a sum of up to four taps against four roundings of the taps: both errors are bounded by 2^-9 sum |w_i|
    per phase tap, so the pre-summed error may not exceed the tap-wise one by more than the slack between bound and typical
    case: 1.5x (measured 1.00 - 1.14)."""
    x, wt = _operands(case, 11)
    ref = _direct(x, wt)
    e_sum = (phase_conv(x, W.pack_conv_up2x(wt).to(BF).double()) - ref).pow(2).mean().sqrt().item()
    e_tap = (_direct(x, wt.to(BF)) - ref).pow(2).mean().sqrt().item()
    print(f"bf16 weights, {case}: rms error pre-summed {e_sum:.3e}, tap-wise {e_tap:.3e}, ratio {e_sum / e_tap:.3f} "
          f"(output rms {ref.pow(2).mean().sqrt().item():.3f})")
    assert e_sum <= 1.5 * e_tap


def _phase_params(base, b=2, h=16, w=16, cin=256, n=640):
    p = _lib.GemmParams()
    p.a0 = p.w = p.out = base
    p.dtype, p.batch, p.hin, p.win, p.hout, p.wout = _lib.SASPA_BF16, b, h, w, 2 * h, 2 * w
    p.kh, p.kw, p.stride, p.pad, p.upsample = 2, 2, 1, 1, 2
    p.c0 = p.lda0 = cin
    p.K = p.ldw = 4 * cin
    p.N = p.ldo = n
    p.M, p.nb1, p.nb2, p.alpha = b * 4 * h * w, 1, 1, 1.0
    return p


def test_library_answers_and_refuses_on_the_host():
    lib = _lib.load()
    a = (C.c_char * 64)()
    base = (C.addressof(a) + 15) // 16 * 16
    ok = lib.saspa_gemm_which(C.byref(_phase_params(base)))
    assert ok > 0 and (ok & 0xff) in (1, 2), ok
    assert lib.saspa_gemm_suggest_ksplit(C.byref(_phase_params(base))) >= 1
    # the production levels go to the 8-wave kernel un-split
    for shape in ((16, 32, 32, 640, 640), (16, 16, 16, 1280, 1280)):
        wch = lib.saspa_gemm_which(C.byref(_phase_params(base, *shape)))
        assert (wch & 0xff, wch >> 8) == (2, 1), (shape, wch)
    bad = _phase_params(base)                # a concat source
    bad.a1, bad.c1, bad.lda1, bad.K, bad.ldw = base, 64, 64, 4 * (256 + 64), 4 * (256 + 64)
    assert lib.saspa_gemm_which(C.byref(bad)) == _lib.SASPA_ERANGE
    bad = _phase_params(base)                # a residual
    bad.residual, bad.ldr = base, 640
    assert lib.saspa_gemm_which(C.byref(bad)) == _lib.SASPA_ERANGE
    bad = _phase_params(base)                # a row vector
    bad.rowvec = base
    assert lib.saspa_gemm_which(C.byref(bad)) == _lib.SASPA_ERANGE
    bad = _phase_params(base)                # kh != 2
    bad.kh, bad.kw, bad.K, bad.ldw = 3, 3, 9 * 256, 9 * 256
    assert lib.saspa_gemm_which(C.byref(bad)) == _lib.SASPA_ERANGE
    bad = _phase_params(base)                # fp32: the parity paths keep the 3x3 launch
    bad.dtype = _lib.SASPA_F32
    assert lib.saspa_gemm_which(C.byref(bad)) == _lib.SASPA_ERANGE
    # statistics on images of less than whole 128-row blocks per phase: only a launch on K slices keys them
    st = (C.c_float * 4096)()
    ws = (C.c_float * 64)()
    small = _phase_params(base, 3, 8, 8, 64, 320)
    small.gn_stats, small.gn_unit = C.cast(st, C.c_void_p), 10
    assert lib.saspa_gemm_which(C.byref(small)) == _lib.SASPA_ERANGE
    ks = lib.saspa_gemm_suggest_ksplit(C.byref(small))
    assert ks >= 2
    small.ksplit, small.workspace = ks, C.cast((C.addressof(ws) + 15) // 16 * 16, C.c_void_p)
    got = lib.saspa_gemm_which(C.byref(small))
    assert got > 0 and got >> 8 == ks, got
