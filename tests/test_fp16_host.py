"""The opt-in fp16 compute mode, host side (no GPU): the second library, its ABI and dtype contract, the public switch, and the CPU
proof that the fp16 rounding-error budgets (tests/fp16_budget.py) have power -- legitimate fp16 emulations of the kernels within
half the limits; the catalogue's mutants AND the same operations carried out with bf16 rounding beyond twice the limits."""
import ctypes as C
import functools
import os

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import pipeline as P
from tests import errbudget as E
from tests import fp16_budget as H
from tests import test_errbudget as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the two libraries
def test_both_libraries_exist_and_name_their_half_type():
    assert os.path.exists(_lib.LIB_PATH), "libsaspa_hip.so missing: run __graft_entry__.build()"
    assert os.path.exists(_lib.F16_LIB_PATH), "libsaspa_hip_f16.so missing: run __graft_entry__.build()"
    lib, f16 = _lib.load(), _lib.load_f16()
    assert lib.saspa_half_type() == _lib.SASPA_BF16 == 0
    assert f16.saspa_half_type() == _lib.SASPA_F16 == 3
    assert lib.saspa_abi_version() == 20 and f16.saspa_abi_version() == 20
    assert f16.saspa_build_arch() == b"gfx950"
    for name in _lib.F16_SYMBOL_NAMES:                      # its own symbol subset, all declared in the header's table
        assert name in _lib.SYMBOLS and hasattr(f16, name), name
    for name in ("saspa_canny", "saspa_gemm_fp8", "saspa_conv3x3_mxfp8", "saspa_conv3x3_halo", "saspa_png_deflate", "saspa_hed_fuse"):
        assert not hasattr(f16, name), f"{name} belongs to the default library only"


def test_header_and_binding_agree_on_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "saspa_hip.h")).read()
    assert "#define SASPA_F16 3" in hdr and "int saspa_half_type(void);" in hdr


def _linear_params(dtype, buf, m=128, n=160, k=64):
    """A valid small linear layer over one aligned host buffer (never dereferenced: saspa_gemm_which launches nothing)."""
    p = _lib.GemmParams()
    ptr = C.c_void_p(buf.data_ptr())
    p.dtype, p.a0, p.c0, p.lda0 = dtype, ptr, k, k
    p.batch, p.hin, p.win, p.hout, p.wout = 1, m, 1, m, 1
    p.kh = p.kw = p.stride = 1
    p.w, p.ldw, p.M, p.N, p.K = ptr, k, m, n, k
    p.alpha, p.out, p.ldo, p.nb1, p.nb2 = 1.0, ptr, n, 1, 1
    return p


def test_each_library_refuses_the_other_ones_dtype_codes():
    """Host-side validation only: saspa_gemm_which is saspa_gemm's validation and plan with nothing launched; the elementwise / norm
    entry points are called with a REFUSED code only (they return before their launch)."""
    buf = torch.zeros(1 << 16, dtype=torch.float32)
    ptr = C.c_void_p(buf.data_ptr())
    lib, f16 = _lib.load(), _lib.load_f16()
    served = {0: lib, 1: lib, 2: lib, 3: f16}
    for code in (0, 1, 2, 3):
        for which, L in (("default", lib), ("f16", f16)):
            rc = L.saspa_gemm_which(C.byref(_linear_params(code, buf)))
            if L is served[code]:
                assert rc > 0, f"{which} library must plan dtype code {code}, got {rc}"
            else:
                assert rc == _lib.SASPA_EINVAL, f"{which} library must refuse dtype code {code}, got {rc}"
    gn = _lib.GroupNormParams()
    gn.x0, gn.c0, gn.ldx0, gn.batch, gn.hw, gn.groups, gn.eps = ptr, 64, 64, 1, 16, 8, 1e-5
    gn.gamma = gn.beta = gn.partial = gn.y = ptr
    gn.nsplit, gn.ldy = 1, 64
    for L, refused in ((f16, (0, 1, 2)), (lib, (3,))):
        for code in refused:
            gn.dtype = code
            calls = {
                "saspa_layernorm": lambda: L.saspa_layernorm(code, ptr, 64, ptr, 64, 4, 64, ptr, ptr, 1e-5, None),
                "saspa_geglu": lambda: L.saspa_geglu(code, ptr, 64, ptr, 32, 4, 32, None),
                "saspa_activation": lambda: L.saspa_activation(code, 1, ptr, 64, ptr, 64, 4, 64, None),
                "saspa_softmax_rows": lambda: L.saspa_softmax_rows(code, ptr, 4, 64, 64, 1.0, 0, 4, None),
                "saspa_scale": lambda: L.saspa_scale(code, ptr, ptr, 64, 0.5, None),
                "saspa_cfg_ddim_step": lambda: L.saspa_cfg_ddim_step(code, ptr, ptr, 1, 16, 4, 8, 7.5, 0.5, 0.5, 0.5, 0.5, None),
                "saspa_groupnorm_stats": lambda: L.saspa_groupnorm_stats(C.byref(gn), None),
                "saspa_groupnorm_apply": lambda: L.saspa_groupnorm_apply(C.byref(gn), None),
            }
            for name, call in calls.items():
                assert call() == _lib.SASPA_EINVAL, f"{name} must refuse dtype code {code}"


def test_ops_names_the_fp16_code_and_library():
    from saspa_aug_amd import ops
    assert ops._dt(torch.zeros(1, dtype=torch.float16)) == _lib.SASPA_F16
    assert ops._dt(torch.zeros(1, dtype=torch.bfloat16)) == _lib.SASPA_BF16
    assert ops.is_half(torch.zeros(1, dtype=torch.float16)) and not ops.is_half(torch.zeros(1))
    lib, f16 = _lib.load(), _lib.load_f16()
    assert ops._L(torch.zeros(1, dtype=torch.float16)) is f16
    assert ops._L(torch.zeros(1, dtype=torch.bfloat16)) is lib and ops._L(torch.zeros(1)) is lib and ops._L() is lib
    assert ops._L(_lib.SASPA_F16) is f16 and ops._L(_lib.SASPA_F32X3) is lib
    rec = []
    ops.set_recorder(lambda kind, flops, call, meta: rec.append(kind) or call())
    try:
        wrapped = ops._L(torch.zeros(1, dtype=torch.float16))
        assert isinstance(wrapped, ops._RecordingLib) and wrapped._lib is f16      # the recorder wraps whichever library is handed out
    finally:
        ops.set_recorder(None)


# ------------------------------------------------------------------ the public switch
SD_PIPES = (P.StableDiffusionControlNetPipeline, P.StableDiffusionControlNetImg2ImgPipeline, P.StableDiffusionImg2ImgPipeline)


@pytest.mark.parametrize("cls", SD_PIPES)
def test_enable_fp16_before_to_only(cls):
    pipe = cls({}, CFG.tiny())
    assert pipe._fp16 is False                              # off by default
    assert pipe.enable_fp16(True, vae="x3") is pipe and pipe._fp16 and pipe._fp16_vae == "x3"
    assert pipe.enable_fp16(False) is pipe and not pipe._fp16
    with pytest.raises(ValueError):
        pipe.enable_fp16(True, vae="fp16")
    pipe.unet = object()                                    # what .to() leaves behind
    with pytest.raises(RuntimeError, match="before .to"):
        pipe.enable_fp16()


def test_enable_fp16_refused_by_blip_and_sdxl():
    for cls, cfgs in ((P.BlipDiffusionControlNetPipeline, CFG.BLIP_DIFFUSION), (P.StableDiffusionXLControlNetPipeline, CFG.tiny_xl())):
        with pytest.raises(NotImplementedError, match="SD-1.5"):
            cls({}, cfgs).enable_fp16()


def test_fp16_and_fp8_exclude_each_other():
    with pytest.raises(ValueError, match="fp8"):
        P.StableDiffusionControlNetPipeline({}, CFG.tiny()).enable_fp8(True).enable_fp16()
    with pytest.raises(ValueError, match="fp8"):
        P.StableDiffusionControlNetPipeline({}, CFG.tiny()).enable_fp16().enable_fp8(True)
    from saspa_aug_amd import models
    with pytest.raises(ValueError, match="fp8"):
        models._Net({}, CFG.tiny()["unet"], torch.device("cpu"), torch.float16, fp8=True)


def test_run_aug_settings_carry_the_switch():
    from saspa_aug_amd.run_aug import Settings
    s = Settings()
    assert s.FP16 is False and s.FP16_VAE == "bf16"
    for entry in ("run_aug.py", "run_aug_real_guidance.py"):
        src = open(os.path.join(ROOT, "run_aug", entry)).read()
        assert "SASPA_FP16" in src and "SASPA_FP16_VAE" in src, entry


def test_weights_granularity_rule_knows_fp16():
    from saspa_aug_amd import weights as W
    assert W.ktile(torch.float16) == W.ktile(torch.bfloat16) == 64 and W.ktile(torch.float32) == 32
    assert W.chunk_major_ok(3, 3, 64, 0, torch.float16) and not W.chunk_major_ok(3, 3, 32, 0, torch.float16)


# ------------------------------------------------------------------ the budget proof for fp16
FAMILIES = ("gemm", "attn", "norm", "elem", "xattn", "ff", "as", "chain_res")


def test_fp16_rounding_helpers():
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 + 2.0 ** -11 + 2.0 ** -20), 2.0 ** -24 * 1.75, 3.0e-8, 65519.0],
                     dtype=torch.float64)
    with H.fp16_rounding():
        assert T.BF is torch.float16
        assert torch.equal(T.rne(x), torch.tensor([1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 2.0 ** -23, 2.0 ** -24, 65504.0], dtype=torch.float64))
        assert torch.equal(T.trunc(x), torch.tensor([1.0, -1.0, 2.0 ** -24, 0.0, 65504.0], dtype=torch.float64))
    assert T.BF is torch.bfloat16 and T.trunc is not H.trunc16
    assert H.floor16(torch.tensor([1e-9, 1.0])).tolist() == [2.0 ** -13, 1.0]


@functools.lru_cache(maxsize=None)
def _measured16(family):
    """tests/test_errbudget._measured under fp16 rounding: every case of the family on every seed shift, against the fp16 unit,
    the floored magnitude and the table in use; next to every legitimate row the catalogue's bf16 emulation of the same case on the
    same draws (the routing mutant), and for the gemm family the typical-magnitude rms of both."""
    make, _ = T.FAMILIES[family]
    lim = H.limits_for(family)
    bf16 = {name: payload[0] for name, legit, _, _, payload in T._measured(family) if legit}
    rows, excluded = [], set()
    for shift in T.SEEDS:
        T._SEED_SHIFT[0] = shift
        try:
            with H.fp16_rounding():
                cases = make()
        finally:
            T._SEED_SHIFT[0] = 0
        for name, got, ref, s, legit in cases:
            if legit and not H.emulates_a_kernel(family, name):
                excluded.add(name)
                continue
            s = H.floor16(s)
            st = E.budget_stats(got, ref, s, H.UNIT_F16)
            if legit and family in H.TYPICAL_RMS_LIMIT:
                st["typical_rms"] = H.typical_rms(got, ref)
            rows.append((f"{name} [seeds +{1000 * shift}]", "legit" if legit else "mutant", st, E.ratio(st, lim)))
            if legit and "flipped by an ulp" not in name:
                # the same operation carried out with bf16 rounding: the catalogue's own bf16 emulation on the same draws
                gb = bf16[f"{name} [seeds +{1000 * shift}]"]
                sb = E.budget_stats(gb, ref, s, H.UNIT_F16)
                if family in H.TYPICAL_RMS_LIMIT:
                    sb["typical_rms"] = H.typical_rms(gb, ref)
                rows.append((f"bf16 arithmetic: {name} [seeds +{1000 * shift}]", "bf16", sb, E.ratio(sb, lim)))
    assert excluded == set(H.NOT_A_KERNEL.get(family, ())), (family, excluded)      # every listed exclusion exists, nothing else left out
    return rows


@pytest.mark.parametrize("family", FAMILIES)
def test_fp16_legit_emulations_within_half_the_budget(family):
    rows = [r for r in _measured16(family) if r[1] == "legit"]
    assert rows
    worst = max(rows, key=lambda t: t[3])
    print(f"{family}: worst legit {worst[3]:.3f} {worst[0]}: {E.fmt(worst[2])}")
    assert worst[3] <= T.LEGIT_MAX, f"{family}: fp16 limit less than 2x above legit '{worst[0]}': {E.fmt(worst[2])} vs {H.limits_for(family)}"


@pytest.mark.parametrize("family", FAMILIES)
def test_fp16_mutants_rejected_at_twice_the_budget(family):
    rows = [r for r in _measured16(family) if r[1] == "mutant"]
    assert rows
    weakest = min(rows, key=lambda t: t[3])
    print(f"{family}: weakest mutant {weakest[3]:.2f} {weakest[0]}: {E.fmt(weakest[2])}")
    assert weakest[3] >= T.MUTANT_MIN, f"{family}: fp16 limit less than 2x below mutant '{weakest[0]}': {E.fmt(weakest[2])} vs {H.limits_for(family)}"


@pytest.mark.parametrize("family", FAMILIES)
def test_fp16_budget_rejects_bf16_rounding(family):
    """The same operation carried out with bf16 rounding (operands, hand-offs and output: tests/test_errbudget.py's emulation on the
    same draws) against the fp16 reference is rejected at twice the limits: a GPU result inside the fp16 checks ran f16 arithmetic.
    gemm family: by the typical-magnitude rms (fp16_budget.TYPICAL_RMS_LIMIT) on EVERY row -- the magnitude budget cannot see an
    output rounding behind a long K -- with every legit row within half of that limit."""
    rows = [r for r in _measured16(family) if r[1] == "bf16"]
    assert rows
    if family in H.TYPICAL_RMS_LIMIT:
        lim = H.TYPICAL_RMS_LIMIT[family]
        legit = [r for r in _measured16(family) if r[1] == "legit"]
        worst, weakest = max(legit, key=lambda t: t[2]["typical_rms"]), min(rows, key=lambda t: t[2]["typical_rms"])
        print(f"{family}: typical rms limit {lim}: worst legit {worst[2]['typical_rms']:.3f} {worst[0]}; weakest bf16 arithmetic "
              f"{weakest[2]['typical_rms']:.2f} {weakest[0]}; magnitude budget on the same bf16 rows x{min(r[3] for r in rows):.2f} .. "
              f"x{max(r[3] for r in rows):.2f}")
        assert worst[2]["typical_rms"] <= T.LEGIT_MAX * lim, worst
        assert weakest[2]["typical_rms"] >= T.MUTANT_MIN * lim, weakest
        return
    weakest = min(rows, key=lambda t: t[3])
    print(f"{family}: weakest bf16 arithmetic {weakest[3]:.2f} {weakest[0]}: {E.fmt(weakest[2])}")
    assert weakest[3] >= T.MUTANT_MIN, f"{family}: bf16 arithmetic passes the fp16 budget: '{weakest[0]}': {E.fmt(weakest[2])}"


def test_fp16_tables_are_recorded():
    """profiles/fp16_errbudget.txt carries every entry of the fp16 table (a table edited without re-measuring shows up here)."""
    txt = open(os.path.join(ROOT, "profiles", "fp16_errbudget.txt")).read()
    for fam, lim in H.LIMITS_F16.items():
        assert set(lim) == set(E.STATS)
        line = f"LIMITS_F16[{fam}] = " + " ".join(f"{k} {lim[k]:g}" for k in E.STATS)
        assert line in txt, line
    for fam, lim in H.TYPICAL_RMS_LIMIT.items():
        assert f"TYPICAL_RMS_LIMIT[{fam}] = {lim:g}" in txt
    for fam, names in H.NOT_A_KERNEL.items():
        for name in names:
            assert f"excluded from the legit set [{fam}]: {name}" in txt, name
