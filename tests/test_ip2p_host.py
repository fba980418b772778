"""InstructPix2Pix (BASE_MODEL = "ip2p"), host side (no GPU): the two entry points of the three-branch guidance + DDIM kernel and
their host-side validation, the float64 reference of that update and the CPU proof that the "elem" rounding budget has power on
it, init_pipeline / pass_thorugh_pipe / the output folder, and the oracle helper tests/ip2p_ref.py on a case with a closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionInstructPix2PixPipeline
from saspa_aug_amd.scheduler import DDIMScheduler
from tests import errbudget as E
from tests import ip2p_ref as IR
from tests import test_errbudget as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("saspa_cfg3_ddim_step", "saspa_cfg3_ddim_step_dev")
COEF = dict(a_t=0.3, a_p=0.45, gs=7.5, igs=1.3)


# ------------------------------------------------------------------ symbols and host-side validation
def test_symbols_declared_bound_and_exported_by_both_libraries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "saspa_hip.h")).read(), flags=re.S)
    lib, f16 = _lib.load(), _lib.load_f16()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), f"{name} is not declared in include/saspa_hip.h"
        assert name in _lib.SYMBOLS and name in _lib.F16_SYMBOL_NAMES
        for L in (lib, f16):
            fn = getattr(L, name)
            assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype is C.c_int
    assert lib.saspa_abi_version() == 20 and f16.saspa_abi_version() == 20
    from saspa_aug_amd import ops
    assert callable(ops.cfg3_ddim_step) and callable(ops.cfg3_ddim_step_dev)


def _refused(L, what, value):
    """Both entry points on host buffers with exactly ONE argument wrong -> their two return codes.  `what` names that argument, so no
    call made here can pass the host checks: a refusal launches nothing, and a valid call on host memory must never be made."""
    buf = torch.zeros(1 << 12, dtype=torch.float32)
    base = buf.data_ptr()
    assert base % 16 == 0
    ok, bad = C.c_void_p(base), {"null": None, "odd": C.c_void_p(base + 2)}
    a = dict(dtype=L.saspa_half_type(), eps=ok, x=ok, nimg=2, c=4, ldc=8, coefs=ok, index=ok)
    assert what in a and a[what] != value
    a[what] = bad[value] if what in ("eps", "x", "coefs", "index") else value
    # the header's contract, restated: whatever this helper is asked, it refuses to make a call the library would accept
    served = (L.saspa_half_type(),) + ((_lib.SASPA_F32,) if L.saspa_half_type() == _lib.SASPA_BF16 else ())
    assert what in ("eps", "x", "coefs", "index") or a["dtype"] not in served or a["ldc"] != 8 or not 1 <= a["c"] <= 4 or a["nimg"] < 1
    dev = L.saspa_cfg3_ddim_step_dev(a["dtype"], a["eps"], a["x"], a["nimg"], 16, a["c"], a["ldc"], 7.5, 1.3, a["coefs"], a["index"], None)
    if what in ("coefs", "index"):          # the immediate form does not take them: it would be a VALID call
        return None, dev
    imm = L.saspa_cfg3_ddim_step(a["dtype"], a["eps"], a["x"], a["nimg"], 16, a["c"], a["ldc"], 7.5, 1.3, 0.5, 0.5, 0.5, 0.5, None)
    return imm, dev


def test_host_side_validation_codes():
    for L in (_lib.load(), _lib.load_f16()):
        assert _refused(L, "eps", "null") == (-1, -1) and _refused(L, "x", "null") == (-1, -1)
        assert _refused(L, "coefs", "null") == (None, -1) and _refused(L, "index", "null") == (None, -1)
        assert _refused(L, "eps", "odd") == (-2, -2) and _refused(L, "x", "odd") == (-2, -2)
        assert _refused(L, "ldc", 4) == (-3, -3) and _refused(L, "ldc", 16) == (-3, -3)
        assert _refused(L, "c", 5) == (-3, -3) and _refused(L, "c", 8) == (-3, -3)
        assert _refused(L, "nimg", 0) == (-3, -3) and _refused(L, "nimg", -1) == (-3, -3)
    assert (_lib.SASPA_EINVAL, _lib.SASPA_EALIGN, _lib.SASPA_ERANGE) == (-1, -2, -3)


def test_each_library_refuses_the_other_ones_dtype_codes():
    lib, f16 = _lib.load(), _lib.load_f16()
    assert _refused(lib, "dtype", _lib.SASPA_F16) == (_lib.SASPA_EINVAL,) * 2
    assert _refused(lib, "dtype", _lib.SASPA_F32X3) == (_lib.SASPA_EINVAL,) * 2          # a GEMM mode, not a storage type
    for code in (_lib.SASPA_BF16, _lib.SASPA_F32, _lib.SASPA_F32X3):
        assert _refused(f16, "dtype", code) == (_lib.SASPA_EINVAL,) * 2, code


# ------------------------------------------------------------------ the float64 reference
def _operands():
    return T.q(T._rand(6, 300, 4, seed=42)), T.q(T._rand(2, 300, 4, seed=43))


def test_reference_reduces_to_the_two_branch_form_at_image_guidance_one():
    eps, xx = _operands()
    ref3, s3 = IR.cfg3_ddim_ref(eps, xx, 0.3, 0.45, 7.5, 1.0)
    ref2, s2 = T.cfg_ddim_ref(eps[2:], xx, 0.3, 0.45, 7.5)          # (e1, e2): the image and the text group
    assert (ref3 - ref2).abs().max().item() < 1e-12 and (s3 - s2).abs().max().item() < 1e-12


def test_reference_reduces_to_plain_ddim_for_equal_groups():
    eps, xx = _operands()
    e = eps[:2]
    ref3, _ = IR.cfg3_ddim_ref(torch.cat([e, e, e]), xx, 0.3, 0.45, 7.5, 1.3)
    plain = 0.45 ** 0.5 * (xx - 0.7 ** 0.5 * e) / 0.3 ** 0.5 + 0.55 ** 0.5 * e
    assert (ref3 - plain).abs().max().item() < 1e-12


# ------------------------------------------------------------------ power of the budget (the pattern of tests/test_fp16_host.py)
def _emul(eps, xx, *, igs=COEF["igs"], swap01=False):
    """The kernel's arithmetic: fp32 throughout, one bf16 rounding on the store."""
    e0, e1, e2 = T.f32(eps[:2]), T.f32(eps[2:4]), T.f32(eps[4:])
    if swap01:
        e0, e1 = e1, e0
    e = e0 + torch.tensor(COEF["gs"], dtype=torch.float32) * (e2 - e1) + torch.tensor(igs, dtype=torch.float32) * (e1 - e0)
    sa_t, s1m_t, sa_p, s1m_p = (torch.tensor(v, dtype=torch.float32) for v in
                                (COEF["a_t"] ** 0.5, (1 - COEF["a_t"]) ** 0.5, COEF["a_p"] ** 0.5, (1 - COEF["a_p"]) ** 0.5))
    x0 = (T.f32(xx) - s1m_t * e) / sa_t
    return T.rne(sa_p * x0 + s1m_p * e)


def _rows():
    rows = []
    for shift in T.SEEDS:
        T._SEED_SHIFT[0] = shift
        try:
            eps, xx = _operands()
        finally:
            T._SEED_SHIFT[0] = 0
        ref, s = IR.cfg3_ddim_ref(eps, xx, **COEF)
        for name, got, legit in (("fp32 emulation", _emul(eps, xx), True),
                                 ("groups 0 and 1 swapped", _emul(eps, xx, swap01=True), False),
                                 ("image guidance 1.3 -> 1.5", _emul(eps, xx, igs=1.5), False)):
            st = E.budget_stats(got, ref, s, E.UNIT_BF16)
            rows.append((f"{name} [seeds +{1000 * shift}]", legit, st, E.ratio(st, E.LIMITS["elem"])))
    return rows


def test_budget_has_power_on_the_three_branch_update():
    rows = _rows()
    for name, legit, st, r in rows:
        print(f"{'legit ' if legit else 'mutant'} {r:8.3f}  {name}: {E.fmt(st)}")
    worst = max((r for r in rows if r[1]), key=lambda t: t[3])
    weakest = min((r for r in rows if not r[1]), key=lambda t: t[3])
    assert len(rows) == 3 * len(T.SEEDS)
    assert worst[3] <= T.LEGIT_MAX, f"limit less than 2x above the legit emulation '{worst[0]}': {E.fmt(worst[2])}"
    assert weakest[3] >= T.MUTANT_MIN, f"limit less than 2x below the mutant '{weakest[0]}': {E.fmt(weakest[2])}"


# ------------------------------------------------------------------ run_aug
@pytest.fixture(scope="module")
def tiny_family():
    cfgs = {k: v for k, v in CFG.tiny_ip2p().items() if k != "safety"}
    return cfgs, W.synth_family(cfgs, seed=3)


def test_configs():
    assert CFG.IP2P["unet"] == dict(CFG.SD15_UNET, in_channels=8) and "controlnet" not in CFG.IP2P
    assert {k: v for k, v in CFG.IP2P.items() if k != "unet"} == {k: v for k, v in CFG.SD15.items() if k not in ("unet", "controlnet")}
    t, base = CFG.tiny_ip2p(), CFG.tiny()
    assert t["unet"] == dict(base["unet"], in_channels=8) and "controlnet" not in t and t["vae"] == base["vae"]
    assert CFG.SD15_UNET["in_channels"] == 4 and base["unet"]["in_channels"] == 4          # the families they derive from are untouched


def test_synthetic_family_follows_the_channel_count(tiny_family):
    cfgs, fam = tiny_family
    assert "controlnet" not in fam and fam["unet"]["conv_in.weight"].shape[1] == 8
    same = W.synth_family({k: v for k, v in CFG.tiny().items() if k != "safety"}, seed=3)
    assert torch.equal(fam["vae"]["decoder.conv_in.weight"], same["vae"]["decoder.conv_in.weight"])     # the other networks' seeds stay
    assert torch.equal(fam["text"]["text_model.final_layer_norm.weight"], same["text"]["text_model.final_layer_norm.weight"])


def test_init_pipeline_builds_ip2p_with_ddim(tiny_family):
    cfgs, fam = tiny_family
    pipe = R.init_pipeline("ip2p", None, 0, cfgs=cfgs, state_dicts=fam)
    assert type(pipe) is StableDiffusionInstructPix2PixPipeline and type(pipe.scheduler) is DDIMScheduler
    assert pipe.controlnet is None and not pipe.HAS_CONTROLNET and not pipe.CFG_PREFIX and not pipe.SUPPORTS_FP16
    for args, kw in ((("ip2p", "canny", 0), {}), (("ip2p", "hed", 0), {}), (("ip2p", None, 1), {}),
                     (("ip2p", None, 0), dict(sampler="unipcmultistep"))):
        with pytest.raises(NotImplementedError):
            R.init_pipeline(*args, cfgs=cfgs, state_dicts=fam, **kw)
    with pytest.raises(NotImplementedError):
        pipe.enable_fp8()
    with pytest.raises(NotImplementedError):
        pipe.enable_fp16()


def test_ip2p_call_kwargs_follow_the_reference():
    from PIL import Image
    seen = {}

    class FakePipe:
        def __call__(self, **kw):
            seen.update(kw)
            return type("O", (), {"images": ["img"]})()
    src, gen = Image.new("RGB", (96, 64)), torch.Generator()
    out = R.pass_thorugh_pipe("ip2p", FakePipe(), "make it snowy", src, 0, 0.85, 30, gen, 7.5, 0.75, control_image=None)
    assert out == "img"
    assert (R.IP2P_IMAGE_GUIDANCE_SCALE, R.IP2P_NUM_INFERENCE_STEPS) == (1.3, 100)
    assert seen == {"prompt": "make it snowy", "num_inference_steps": 100, "generator": gen, "guidance_scale": 7.5,
                    "negative_prompt": R.NEGATIVE_PROMPT, "image_guidance_scale": 1.3, "image": src}       # run_aug/run_aug.py:235-255
    assert seen["image"] is src and seen["generator"] is gen


def test_output_folder():
    s = R.Settings(BASE_MODEL="ip2p", CONTROLNET=None, SDEDIT=0, SEED=1)
    assert R.output_folder_for(s, "/data/root").startswith("/data/root/aug_data/regular/ip2p/None/")


# ------------------------------------------------------------------ the oracle helper
def test_oracle_with_a_silent_unet_is_ddim_of_pure_noise(tiny_family):
    """conv_out = 0 -> every noise prediction is 0 -> x_{t-1} = sqrt(a_prev / a_t) x_t for every group and any guidance."""
    from oracle import pipeline as OP
    from saspa_aug_amd.synthetic import synthetic_image
    cfgs, fam = tiny_family
    fam = dict(fam, unet=dict(fam["unet"]))
    fam["unet"]["conv_out.weight"] = torch.zeros_like(fam["unet"]["conv_out.weight"])
    fam["unet"]["conv_out.bias"] = torch.zeros_like(fam["unet"]["conv_out.bias"])
    ids = torch.from_numpy(np.random.RandomState(1).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    neg = torch.from_numpy(np.random.RandomState(2).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    lat = torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(5))
    out, x, img = IR.ip2p_pipeline(fam, cfgs, ids, neg, synthetic_image(64, 64, 7), lat, 3, 7.5, 1.3, return_latents=True)
    sch = OP.DDIM()
    want = lat.double()
    for t in sch.set_timesteps(3):
        a_t, a_p = sch.coefficients(t)
        want = want * (a_p.double() / a_t.double()) ** 0.5
    assert out.shape == (1, 64, 64, 3) and out.dtype == np.uint8 and img.shape == (1, 3, 64, 64)
    assert (x.double() - want).abs().max().item() < 1e-5 * want.abs().max().item()
