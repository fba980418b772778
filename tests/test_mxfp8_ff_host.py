"""Calibration-free fp8 feed-forward (saspa_gemm_fp8_geglu_mx -> saspa_gemm_mxfp8, enable_fp8(ff="mx")): what runs without a GPU
-- the exported entry points and their host-side refusals, the public switch, the block rule on hand-made blocks, and the proof of
the error limits the GPU test (tests/test_mxfp8_ff_gpu.py) reuses unchanged.

THE LIMITS.  Units of tests/errbudget.py (2^-8 x the magnitude of the terms; max, rms, toward-zero bias, scale slope), random
operands (M.pair_operands at M.PAIR_SHAPE: 515 rows of the SDXL level-1 block, 640 -> 5120 -> GEGLU 2560 -> 640), no element
excluded.  Two checks:
- 'emit': the producer's bytes decoded, q * 2^(qs - 127), against the float64 gated values hv * gelu_erf(hg) of the exact
  projection; magnitude max(|y|, 2^(e - 6)) + 2^-4 geglu_gemm_scale (M.producer_ref: the e4m3 conversion at 16 units of the first
  term, the bf16 path's gated value that enters it at 1 unit of geglu_gemm_scale): a right result is bounded near 16 units; where
  both terms are of one size it reaches half of that.
- 'pair': the output projection's result against the float64 pair; magnitude errbudget.gemm_scale (sum |y w| + |bias| +
  |residual|).  2560 independent e4m3 roundings of 16 units average down to 0.35 units rms.
Measured on the CPU with the fp32 emulation of M (three seeds 701 / 711 / 721, forward and reversed K-tiles, libm exp in the erf;
the variants agree to 3 digits):
    emit  max 7.97 .. 8.43   rms 1.140 .. 1.145 bias -0.0195 .. -0.0205 slope -0.16 .. -0.21
    pair  max 1.64 .. 1.69   rms 0.352 .. 0.356 bias -0.0038 .. -0.0062 slope -0.095 .. -0.145
and the mutants (seed 701):
    floor for ceiling    emit max 73  bias -1.4 slope -43      pair max 15  slope -29
    round toward zero    emit bias -1.16 slope -11             pair bias -0.33 slope -7.5
    blocks shifted by 8  emit max 132 slope -6.7               pair max 12.8 slope -4.6
    neighbour's exponent                                       pair max 65  rms 9.2
    exponents ignored                                          pair max 63  slope -171
Each limit below is at least 2x what the legitimate emulations give, and every mutant exceeds the allowance of at least one
statistic of at least one check by 2x or more (test_limits_hold_both_margins asserts exactly that)."""
import ctypes as C
import re
import os

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops
from saspa_aug_amd import config as CFG
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline
from tests import fp8_ref as R
from tests import mxfp8_ff_ref as M
from tests.errbudget import UNIT_BF16, budget_stats, fmt, ratio

MX_LIMITS = {
    "emit": dict(max=18.0, rms=2.4, bias=0.045, slope=0.5),
    "pair": dict(max=3.5, rms=0.75, bias=0.0125, slope=0.3),
}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("saspa_gemm_fp8_geglu_mx", "saspa_gemm_mxfp8")


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------ ABI
def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "saspa_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*const SaspaGemmF8Params\s*\*" % name, src), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert name not in _lib.F16_SYMBOL_NAMES                  # the fp16 build has no fp8 translation unit
    assert lib.saspa_abi_version() == 20                          # the struct did not change


def _params(base, m=130, n=256, k=256, geglu=False):
    p = _lib.GemmF8Params()
    p.a = p.w = p.sw = p.out = base
    p.sa = base if geglu else None
    p.M, p.N, p.K, p.lda, p.ldw = m, n, k, k, k
    p.act = int(ops.ACT_GEGLU if geglu else ops.ACT_NONE)
    p.ldo = n // 2 if geglu else n
    return p


def test_host_refusals():
    """Every refusal happens before a launch: this runs where there is no GPU."""
    lib = _lib.load()
    buf = C.create_string_buffer(64)
    base = (C.addressof(buf) + 15) // 16 * 16
    codes = {}

    def prod(p, qs=base, ldqs=4):
        return lib.saspa_gemm_fp8_geglu_mx(C.byref(p), qs, ldqs, None)

    def cons(p, qs=base, ldqs=8):
        return lib.saspa_gemm_mxfp8(C.byref(p), qs, ldqs, None)

    # the codes the neighbouring entry point uses for the same faults
    g = _params(base, geglu=True)
    g.sa = None
    codes["inval"] = lib.saspa_gemm_fp8(C.byref(g), None)                      # a NULL operand
    g = _params(base, geglu=True)
    g.K = g.lda = g.ldw = 192
    codes["range"] = lib.saspa_gemm_fp8(C.byref(g), None)                      # K = 192
    g = _params(base, geglu=True)
    g.lda = 264
    codes["align"] = lib.saspa_gemm_fp8(C.byref(g), None)                      # lda % 16
    assert len(set(codes.values())) == 3 and 0 not in codes.values()
    # producer
    for mut, want in ((dict(out_fp8=1), "inval"), (dict(out_scale=base), "inval"), (dict(amax=base), "inval"), (dict(act=int(ops.ACT_NONE)), "inval"),
                      (dict(ldo=136), "align"), (dict(K=192, lda=192, ldw=192), "range"), (dict(residual=base), "range")):
        p = _params(base, geglu=True)
        for k, v in mut.items():
            setattr(p, k, v)
        assert prod(p) == codes[want], (mut, want)
    p = _params(base, geglu=True)
    assert prod(p, ldqs=6) == codes["align"] and prod(p, qs=base + 2) == codes["align"]      # ldqs % 4, qs not on a dword
    assert prod(p, ldqs=0) == codes["range"]                                                 # ldqs < N / 64 = 4
    assert prod(p, qs=None) == codes["inval"]
    # consumer
    for mut, want in ((dict(sa=base), "inval"), (dict(act=int(ops.ACT_GEGLU)), "inval"), (dict(out_fp8=1), "inval"), (dict(amax=base), "inval"),
                      (dict(K=192, lda=192, ldw=192), "range"), (dict(N=192), "range"), (dict(ldo=260), "align"),
                      (dict(residual=base, ldr=260), "align")):
        p = _params(base)
        for k, v in mut.items():
            setattr(p, k, v)
        assert cons(p) == codes[want], (mut, want)
    p = _params(base)
    assert cons(p, ldqs=10) == codes["align"] and cons(p, qs=base + 1) == codes["align"]
    assert cons(p, ldqs=4) == codes["range"]                                                 # ldqs < K / 32 = 8
    assert cons(p, qs=None) == codes["inval"]


# ------------------------------------------------------------------ the public switch
def _pipe():
    cfgs = CFG.tiny()
    return StableDiffusionControlNetPipeline(W.synth_family(cfgs, seed=5), cfgs)


def test_enable_fp8_ff_argument():
    pipe = _pipe()
    with pytest.raises(ValueError):
        pipe.enable_fp8(ff="x")
    with pytest.raises(ValueError):
        pipe.enable_fp8(False, ff="mx")                           # as enable_fp8(False, convs=True): needs fp8 on
    with pytest.raises(ValueError):
        pipe.enable_fp8(False, convs=True)
    assert pipe.enable_fp8(True, ff="mx") is pipe and pipe._fp8_ff == "mx" and pipe._fp8
    assert pipe.enable_fp8(True)._fp8_ff == "calibrated"          # the default stays the calibrated tensor scale
    from saspa_aug_amd import models
    with pytest.raises(ValueError):
        models._Net({}, {}, "cpu", torch.bfloat16, fp8=True, fp8_ff="block")


def test_ip2p_keeps_refusing_fp8():
    from saspa_aug_amd.pipeline import StableDiffusionInstructPix2PixPipeline
    with pytest.raises(NotImplementedError):
        StableDiffusionInstructPix2PixPipeline.enable_fp8(object.__new__(StableDiffusionInstructPix2PixPipeline), True, ff="mx")


# ------------------------------------------------------------------ the block rule on hand-made blocks
def test_block_rule_on_hand_made_blocks():
    f32 = torch.float32
    up = lambda v: torch.nextafter(torch.tensor(v, dtype=f32), torch.tensor(float("inf")))         # noqa: E731
    rows, want_e = [], []
    rows.append(torch.zeros(32)); want_e.append(0)                                  # all zero -> byte 127, zero codes
    for e in (-20, -6, -1, 0, 3, 40):
        b = torch.linspace(-1, 1, 32) * 100 * 2.0 ** e
        b[7] = -448.0 * 2.0 ** e                                                    # a maximum of exactly 448 * 2^e keeps e
        rows.append(b); want_e.append(e)
        b = b.clone()
        b[7] = up(448.0 * 2.0 ** e)                                                 # the next fp32 above it takes e + 1
        rows.append(b); want_e.append(e + 1)
    rows.append(torch.full((32,), 2.0 ** -140)); want_e.append(-127)                # clamped below
    rows.append(torch.full((32,), 3.0e38)); want_e.append(120)
    y = torch.stack(rows).to(f32)
    q, qs = M.quantize_blocks(y)
    assert qs[:, 0].tolist() == [e + 127 for e in want_e]
    assert torch.equal(M.block_exponent(y.abs().amax(-1)), M.block_exponent_def(y.abs().amax(-1)))
    assert qs[0, 0].item() == 127 and (q[0] == 0).all()
    dec = R.e4m3_decode(q)
    assert dec.abs().max().item() <= 448.0 and torch.isfinite(dec).all()            # decoded values never exceed 448
    assert dec[1, 7].item() == -448.0 and dec[2, 7].item() == 224.0                 # exactly 448 stays; one ulp above: next binade
    # the bit rule and the definition agree on random magnitudes over the whole fp32 range, and nothing leaves the e4m3 range
    g = torch.Generator().manual_seed(0)
    a = (torch.rand(4096, generator=g) * torch.exp2(torch.randint(-140, 127, (4096,), generator=g).float())).to(f32)
    e = M.block_exponent(a)
    assert torch.equal(e, M.block_exponent_def(a))
    scaled = torch.ldexp(a.double(), -e)
    assert (scaled <= 448.0).all() and ((scaled > 224.0) | (e == -127) | (a == 0)).all()
    # the floor mutant differs from the rule everywhere but on exact maxima
    inner = (e > -127) & (e < 127)
    assert (M.block_exponent_floor(a) == e - 1)[inner].all()


# ------------------------------------------------------------------ the limits
@pytest.fixture(scope="module")
def cases():
    return M.pair_cases(_rand)


def test_limits_hold_both_margins(cases):
    """Legitimate emulations use at most half of every allowance; every mutant exceeds at least one allowance of at least one of
    its checks by 2x."""
    worst_mutant = {}
    for (name, fam, got, ref, s, legit) in cases:
        st = budget_stats(got, ref, s, UNIT_BF16)
        r = ratio(st, MX_LIMITS[fam])
        print(f"\n[{fam}] {name}: {fmt(st)} -> {r:.2f} of the allowance")
        if legit:
            assert r <= 0.5, (name, fam, fmt(st), r)
        else:
            worst_mutant[name] = max(worst_mutant.get(name, 0.0), r)
    assert len(worst_mutant) == 5
    for name, r in worst_mutant.items():
        assert r >= 2.0, (name, r)


def test_emulation_never_saturates_and_blocks_are_independent(cases):
    op1, _ = M.pair_operands(_rand, *M.PAIR_SHAPE, M.PAIR_SEED)
    y = M.producer_gated32(op1)
    q, qs = M.quantize_blocks(y)
    assert R.e4m3_decode(q).abs().max().item() <= 448.0
    top = R.e4m3_decode(q).abs().reshape(y.shape[0], -1, 32).amax(-1)
    assert ((top >= 224.0) | (top == 0)).all()                     # every block uses its top binade (a value just above 224 rounds to it)
    q1, qs1 = M.quantize_blocks(y[7:8])
    assert torch.equal(q1, q[7:8]) and torch.equal(qs1, qs[7:8])   # a row's bytes depend on that row alone
