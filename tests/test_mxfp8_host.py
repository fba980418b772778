"""MX-fp8 3x3 convs (opt-in fp8 conv path of the resnets): what runs without a GPU -- the exported entry points, their host-side
argument checks, the weight packer, and the block-exponent rule restated in Python (the GPU tests hold the kernels to it)."""
import ctypes as C
import math

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, models, ops
from saspa_aug_amd import weights as W

E4M3_MAX = 448.0


def mx_exponent(amax):
    """The smallest integer e with amax <= 448 * 2^e, clamped to [-127, 127]; 0 for an all-zero block (saspa_hip.h)."""
    if amax == 0.0:
        return 0
    e = math.ceil(math.log2(amax / E4M3_MAX))
    # log2 of a float can land a hair off an exact power of two: settle on the defining inequality
    while amax > E4M3_MAX * 2.0 ** e:
        e += 1
    while e > -200 and amax <= E4M3_MAX * 2.0 ** (e - 1):
        e -= 1
    return max(-127, min(127, e))


def test_exponent_rule_edges():
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))                     # noqa: E731
    for k in (-30, -1, 0, 1, 7, 60):
        exact = E4M3_MAX * 2.0 ** k
        assert mx_exponent(exact) == k                                               # amax == 448 * 2^k fits at k
        above = float(torch.nextafter(torch.tensor(exact, dtype=torch.float32), torch.tensor(math.inf)))
        assert mx_exponent(above) == k + 1                                           # one ulp above needs one binade more
        below = float(torch.nextafter(torch.tensor(exact, dtype=torch.float32), torch.tensor(0.0)))
        assert mx_exponent(below) == k
    assert mx_exponent(0.0) == 0
    assert mx_exponent(f32(2.0 ** -140)) == -127                                     # fp32 subnormal y: clamped
    assert mx_exponent(f32(1e-38)) == -127
    assert mx_exponent(f32(3.0e38)) == 120
    # y * 2^-e never exceeds the e4m3 range, and the largest block value uses its top binade (above 224) unless clamped
    g = torch.Generator().manual_seed(0)
    for a in (torch.rand(200, generator=g) * 2.0 ** torch.randint(-60, 60, (200,), generator=g)).tolist():
        a = f32(a)
        e = mx_exponent(a)
        assert a * 2.0 ** -e <= E4M3_MAX and (a * 2.0 ** -e > E4M3_MAX / 2 or e == -127)


def test_symbols_exported():
    lib = _lib.load()
    for name in ("saspa_groupnorm_quant_mxfp8", "saspa_conv3x3_mxfp8", "saspa_conv3x3_mxfp8_eligible"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.saspa_abi_version() == 20
    assert ops.GEMM_FAMILY_NAMES[ops.GEMM_FAMILY_MXFP8_CONV] == "mxfp8_conv"


def _aligned(buf):
    return (C.addressof(buf) + 15) // 16 * 16


def _conv_params(base, c=320, n=320):
    p = _lib.ConvMxParams()
    p.q = p.qs = p.w8 = p.sw = p.out = base
    p.batch, p.h, p.w, p.C = 2, 8, 8, c
    p.kh, p.kw, p.stride, p.pad, p.upsample = 3, 3, 1, 1, 0
    p.N, p.Kp = n, (9 * c + 127) // 128 * 128
    p.ldq, p.ldqs, p.ldw, p.ldo = c, c // 32, p.Kp, n
    return p


def test_conv_host_validation():
    lib = _lib.load()
    buf = (C.c_char * 64)()
    base = _aligned(buf)
    assert lib.saspa_conv3x3_mxfp8(None, None) == _lib.SASPA_EINVAL
    p = _conv_params(base)
    assert lib.saspa_conv3x3_mxfp8_eligible(C.byref(p)) == 1
    for field in ("q", "qs", "w8", "sw", "out"):
        p = _conv_params(base)
        setattr(p, field, None)
        assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_EINVAL, field
    for field, value in (("ldq", 328), ("ldw", 2952), ("ldo", 324), ("ldqs", 9)):
        p = _conv_params(base)
        setattr(p, field, value)
        assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_EALIGN, field
        assert lib.saspa_conv3x3_mxfp8_eligible(C.byref(p)) == 0
    p = _conv_params(base)
    p.out = base + 8                                                                 # misaligned output
    assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_EALIGN
    p = _conv_params(base)
    p.residual, p.ldr = base, 321
    assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_EALIGN
    for field, value in (("C", 336), ("N", 128), ("stride", 2), ("upsample", 1), ("kh", 1), ("Kp", 2816)):
        p = _conv_params(base)
        setattr(p, field, value)
        if field == "C":
            p.ldq, p.ldqs, p.Kp, p.ldw = 336, 10, 3072, 3072
        assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_ERANGE, field
        assert lib.saspa_conv3x3_mxfp8_eligible(C.byref(p)) == 0, field
    p = _conv_params(base)
    p.Kp = p.ldw = p.Kp + 128                                                        # padding beyond the next whole K-tile
    assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_ERANGE
    assert lib.saspa_conv3x3_mxfp8_eligible(C.byref(p)) == 0
    p = _conv_params(base)
    p.gn_stats, p.gn_unit = base, 12                                                 # 80 % 12 != 0: no 160-column unit tiling
    assert lib.saspa_conv3x3_mxfp8(C.byref(p), None) == _lib.SASPA_ERANGE


def test_eligible_answers():
    for c in (320, 640, 960, 1280, 1920, 2560):
        for n in (320, 640, 1280):
            assert ops.conv3x3_mxfp8_eligible(c, n)
    assert ops.conv3x3_mxfp8_eligible(32, 160)
    assert not ops.conv3x3_mxfp8_eligible(336, 320)                                  # C % 32
    assert not ops.conv3x3_mxfp8_eligible(320, 128)                                  # N % 160
    assert not ops.conv3x3_mxfp8_eligible(4, 320)
    # the routing rule (measured, models.py): two tiles per CU, or one with a short K; never fewer
    assert models.mxfp8_conv_takes(2 * 128 * 128, 320, 320) and models.mxfp8_conv_takes(8 * 32 * 32, 1280, 2560)
    assert models.mxfp8_conv_takes(8 * 32 * 32, 640, 640) and not models.mxfp8_conv_takes(8 * 32 * 32, 640, 1920)
    assert not models.mxfp8_conv_takes(2 * 32 * 32, 1280, 1280) and not models.mxfp8_conv_takes(8 * 16 * 16, 1280, 640)


def test_quantiser_host_validation():
    lib = _lib.load()
    buf = (C.c_char * 64)()
    base = _aligned(buf)
    p = _lib.GroupNormParams()
    p.dtype, p.x0, p.c0, p.ldx0, p.batch, p.hw, p.groups, p.eps = 0, base, 320, 320, 1, 256, 32, 1e-5
    p.gamma = p.beta = p.partial = base
    p.nsplit, p.act = 4, 1
    assert lib.saspa_groupnorm_quant_mxfp8(C.byref(p), None, 320, base, 10, None) == _lib.SASPA_EINVAL
    assert lib.saspa_groupnorm_quant_mxfp8(C.byref(p), base, 320, None, 10, None) == _lib.SASPA_EINVAL
    assert lib.saspa_groupnorm_quant_mxfp8(C.byref(p), base, 328, base, 10, None) == _lib.SASPA_EALIGN     # ldq % 16
    assert lib.saspa_groupnorm_quant_mxfp8(C.byref(p), base, 320, base, 9, None) == _lib.SASPA_EALIGN      # ldqs < C / 32
    p.c0 = p.ldx0 = 328
    p.groups = 41
    assert lib.saspa_groupnorm_quant_mxfp8(C.byref(p), base, 336, base, 11, None) == _lib.SASPA_ERANGE     # C % 32
    p.c0, p.ldx0, p.groups, p.dtype = 320, 320, 32, 1
    assert lib.saspa_groupnorm_quant_mxfp8(C.byref(p), base, 320, base, 10, None) == _lib.SASPA_ERANGE     # fp32 source


@pytest.mark.parametrize("cin,cout", [(320, 320), (960, 640), (64, 160)])
def test_pack_conv_mxfp8(cin, cout):
    w = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(cin)) / math.sqrt(9 * cin)
    w8, sw = W.pack_conv_mxfp8(w)
    k = 9 * cin
    kp = (k + 127) // 128 * 128
    assert w8.dtype == torch.uint8 and tuple(w8.shape) == (cout, kp) and tuple(sw.shape) == (cout,)
    assert (w8[:, k:] == 0).all()                                                    # zero padding to whole 128-byte K-tiles
    deq = W.dequantize_fp8(w8, sw)[:, :k]
    ref = w.permute(0, 2, 3, 1).reshape(cout, k)                                     # K = (ky * 3 + kx) * Cin + c
    # e4m3: half an ulp = 2^-4 relative, plus the subnormal floor of the row scale
    assert ((deq - ref).abs() <= 2.0 ** -4 * ref.abs() + sw[:, None] * 2.0 ** -9 + 1e-12).all()
    # the tap order is checked on one element: tap (ky, kx) = (2, 1), channel 5 of output 3
    assert abs(deq[3, (2 * 3 + 1) * cin + 5] - w[3, 5, 2, 1]) <= 2.0 ** -4 * abs(w[3, 5, 2, 1]) + sw[3] * 2.0 ** -9
