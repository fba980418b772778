"""Host side of the fp16 SDXL VAE and its fused wide-head attention (no GPU):
- the budget of saspa_attn_wide (tests/attn_wide_ref.py): the rule that chose the table, the legitimate emulation within half of
  it, both mutants rejected;
- the declarations: header, ctypes tables, Makefile lists;
- the switches: run_aug.Settings.XL_VAE, SASPA_XL_VAE, set_vae_mode and who refuses it;
- run_aug's per-item status for an image whose decoder output was not finite."""
import json
import os
import re

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models
from saspa_aug_amd import pipeline as P
from saspa_aug_amd import run_aug as R
from tests import attn_wide_ref as A
from tests import errbudget as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.bfloat16, torch.float16)
VARIANTS = (("legit", {}), ("logits16", dict(logits16=True)), ("p_trunc", dict(rnd_p=A.trunc)))


def _rows():
    """(dtype, case, variant, statistics) of the emulation and the two mutants over every case; computed once."""
    if not _rows.cache:
        for dt in DTYPES:
            for case in A.CASES:
                q, k, v, scale, idx, ref, s = A.case_data(case, dt)
                for name, kw in VARIANTS:
                    got = A.emul(q[:, idx], k, v, scale, dt, **kw)
                    _rows.cache.append((dt, case, name, E.budget_stats(got, ref, s, A.UNIT[dt])))
    return _rows.cache


_rows.cache = []


def report():
    """The text of profiles/attn_wide_errbudget.txt."""
    out = ["saspa_attn_wide: error statistics of the fp32 emulation and its mutants against the float64 reference (tests/attn_wide_ref.py),",
           "in units of 2^-8 (bf16) / 2^-11 (fp16) of sum_j p_ij |v_j|; ratio = max |stat| / allowance against the named table.",
           f"flash table (errbudget.LIMITS['attn']): {A.FLASH}", f"chosen table (2 x worst legitimate value): {A.LIMITS}", ""]
    for dt, case, name, st in _rows():
        out.append(f"{A.NAME[dt]} {A.case_id(case):28s} {name:9s} {E.fmt(st)}  vs flash {E.ratio(st, A.FLASH):7.3f}  "
                   f"vs chosen {E.ratio(st, A.LIMITS):7.3f}")
    worst = {k: max(abs(st[k]) for _, _, n, st in _rows() if n == "legit") for k in E.STATS}
    out.append("")
    out.append("worst legitimate value per statistic: " + " ".join(f"{k} {v:.4g}" for k, v in worst.items()))
    return "\n".join(out) + "\n"


# ---- budget -----------------------------------------------------------------------------------------------------------------
def test_flash_table_does_not_qualify_and_the_measured_one_is_twice_the_worst_emulation():
    legit = [(dt, c, st) for dt, c, n, st in _rows() if n == "legit"]
    # first half of the rule holds: at d = 512 the emulation is within half of the flash-attention family's table ...
    assert all(E.ratio(st, A.FLASH) <= 0.5 for dt, c, st in legit if c[3] == 512)
    # ... the second does not: the truncated-P mutant is not rejected at twice that table in every case
    assert any(E.ratio(st, A.FLASH) < 2.0 for dt, c, n, st in _rows() if n == "p_trunc")
    # so the table is 2 x the worst legitimate value of each statistic, rounded up to two digits
    worst = {k: max(abs(st[k]) for _, _, st in legit) for k in E.STATS}
    print("worst legitimate:", worst)
    for k in E.STATS:
        # (the host BLAS' fp32 summation order moves the last digits of max / rms; bias and slope are means of signed errors,
        # i.e. mostly sampling noise, which the allowance covers with its standard-error term)
        assert worst[k] <= A.MEASURED_WORST[k] * (1.02 if k in ("max", "rms") else 1.5), (k, worst[k])
        assert 2.0 * A.MEASURED_WORST[k] <= A.LIMITS[k] <= 2.0 * A.MEASURED_WORST[k] * 1.25, k
    assert A.limits_for(torch.float16) is A.LIMITS and A.limits_for(torch.bfloat16) is A.LIMITS


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: A.NAME[d])
def test_emulation_within_half_the_budget_and_mutants_rejected(dt):
    for d, case, name, st in _rows():
        if d != dt:
            continue
        r = E.ratio(st, A.LIMITS)
        print(f"{A.NAME[dt]} {A.case_id(case)} {name}: {E.fmt(st)} ratio {r:.3f}")
        if name == "legit":
            assert r <= 0.5 * 1.02, (A.case_id(case), r)
        elif name == "logits16":
            assert r >= 2.0, (A.case_id(case), r)          # a logit stored in 16 bits: far outside, in every case
        else:
            assert r > 1.0, (A.case_id(case), r)           # P truncated: rejected in every case
    # ... and at twice the budget wherever the outputs are enough for the slope's noise allowance not to swallow it
    assert sum(E.ratio(st, A.LIMITS) >= 2.0 for d, c, n, st in _rows() if d == dt and n == "p_trunc") >= 3


def test_profile_file_is_the_report_of_this_table():
    text = open(os.path.join(ROOT, "profiles", "attn_wide_errbudget.txt")).read()
    assert str(A.LIMITS) in text and str(A.FLASH) in text
    assert all(A.case_id(c) in text for c in A.CASES)


# ---- declarations -----------------------------------------------------------------------------------------------------------
def test_declarations_name_the_entry_point_everywhere():
    header = open(os.path.join(ROOT, "include", "saspa_hip.h")).read()
    assert re.search(r"\bint saspa_attn_wide\(int dtype, const void\* q,", header)
    assert "saspa_attn_wide" in _lib.SYMBOLS and "saspa_attn_wide" in _lib.F16_SYMBOL_NAMES
    res, args = _lib.SYMBOLS["saspa_attn_wide"]
    assert len(args) == 19                                     # dtype, 4 x (pointer, pitch, batch stride), batch, nq, nk, d, scale, stream
    mk = open(os.path.join(ROOT, "saspa-aug_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    f16 = re.search(r"^F16_SRCS := (.*)$", mk, re.M).group(1).split()
    assert "saspa_attn_wide.hip" in srcs and "saspa_attn_wide.hip" in f16
    assert os.path.exists(os.path.join(ROOT, "saspa-aug_amd", "csrc", "saspa_attn_wide.hip"))
    assert re.search(r"saspa_abi_version\(\) == 20", open(os.path.join(ROOT, "__graft_entry__.py")).read())


def test_wide_head_widths_and_the_attention_knob(monkeypatch):
    assert [d for d in range(0, 1024, 8) if models.wide_head(d)] == [192, 256, 320, 384, 448, 512]
    monkeypatch.delenv("SASPA_VAE_ATTN", raising=False)
    assert models.vae_attn_fused(torch.float16) and not models.vae_attn_fused(torch.bfloat16) and not models.vae_attn_fused(torch.float32)
    monkeypatch.setenv("SASPA_VAE_ATTN", "fused")
    assert models.vae_attn_fused(torch.bfloat16) and models.vae_attn_fused(torch.float16) and not models.vae_attn_fused(torch.float32)
    monkeypatch.setenv("SASPA_VAE_ATTN", "flash")
    with pytest.raises(ValueError, match="SASPA_VAE_ATTN"):
        models.vae_attn_fused(torch.bfloat16)


# ---- switches ---------------------------------------------------------------------------------------------------------------
def test_settings_default_and_mode_parsing():
    assert R.Settings().XL_VAE is None
    assert P.XL_VAE_MODES == (None, "x3", "exact", "bf16", "f16")
    for v in ("x3", "exact", "bf16", "f16"):
        assert P.xl_vae_mode(v) == v
    for v in (None, "", "default"):
        assert P.xl_vae_mode(v) is None
    for v in ("fp16", "f32", "F16", 16):
        with pytest.raises(ValueError, match="VAE mode"):
            P.xl_vae_mode(v)


def test_sdxl_pipeline_records_the_mode_before_to():
    pipe = P.StableDiffusionXLControlNetPipeline({}, CFG.tiny_xl())
    assert pipe._vae_mode is None and not pipe._vae_mode_set and pipe.last_nonfinite is None
    assert pipe.set_vae_mode("f16") is pipe and pipe._vae_mode == "f16" and pipe._vae_mode_set
    assert pipe.upcast_vae() is pipe and not pipe._vae_fp32              # a no-op in the 16-bit modes
    assert pipe.set_vae_mode("bf16").upcast_vae()._vae_fp32 is False
    pipe.set_vae_mode("exact").upcast_vae()
    assert pipe._vae_fp32 and pipe._vae_gemm == "exact"
    pipe.set_vae_mode(None)
    assert pipe._vae_mode is None and pipe._vae_mode_set                # explicit None: the environment is not consulted
    with pytest.raises(ValueError, match="VAE mode"):
        pipe.set_vae_mode("fp16")


@pytest.mark.parametrize("cls,cfgs", [(P.StableDiffusionControlNetPipeline, CFG.tiny), (P.StableDiffusionControlNetImg2ImgPipeline, CFG.tiny),
                                      (P.StableDiffusionImg2ImgPipeline, CFG.tiny), (P.StableDiffusionInstructPix2PixPipeline, CFG.tiny),
                                      (P.BlipDiffusionControlNetPipeline, lambda: CFG.BLIP_DIFFUSION)],
                         ids=lambda v: getattr(v, "__name__", ""))
def test_sd15_family_refuses_the_vae_modes(cls, cfgs):
    pipe = cls({}, cfgs())
    with pytest.raises(NotImplementedError, match="not the fp16-fix one"):
        pipe.set_vae_mode("f16")
    with pytest.raises(ValueError, match="VAE mode"):                  # an unknown mode is a ValueError before it is a refusal
        pipe.set_vae_mode("fp16")


def test_init_pipeline_applies_the_setting_for_sdxl():
    pipe = R.init_pipeline("sd_xl-turbo", "canny", 0, state_dicts={}, cfgs=CFG.tiny_xl(), xl_vae="f16")
    assert pipe._vae_mode == "f16" and not pipe._vae_fp32
    pipe = R.init_pipeline("sd_xl-turbo", "canny", 0, state_dicts={}, cfgs=CFG.tiny_xl())
    assert pipe._vae_mode is None and pipe._vae_fp32                    # today's behaviour: upcast_vae()


# ---- run_aug: an item whose decoder output was not finite -------------------------------------------------------------------
def _generator(bad_order):
    def gen(batch, noises, sources):
        imgs = np.stack([np.full(src.shape, 10 + it.order, np.uint8) for it, src in zip(batch, sources)])
        return imgs, sources.copy(), np.array([it.order == bad_order for it in batch])
    return gen


def test_run_aug_fails_the_flagged_item_only(tmp_path):
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("An airplane.\nAnother airplane.\n")
    s = R.Settings(DATASET="synthetic", NUM_PER_IMAGE=2, SEED=1, RESOLUTION=64, BATCH_SIZE=4, PROMPTS_FILE=str(prompts),
                   DATASET_KWARGS=dict(root_path=str(tmp_path / "d" / "data"), n_images=3, sizes=((64, 64),), seed=2),
                   SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, XL_VAE="f16")
    r = R.main(s, batch_generator=_generator(bad_order=2))
    st = r["status"].tolist()
    assert len(st) == 6 and st[2] == -1 and [v for i, v in enumerate(st) if i != 2] == [1] * 5
    bad = next(it for it in r["items"] if it.order == 2)
    assert not os.path.exists(bad.output_path)
    for it in r["items"]:
        if it.order != 2:
            assert os.path.exists(it.output_path), it.output_path
    body = json.load(open(r["json_path"]))
    assert sum(len(v) for v in body.values()) == 5
    # the source image of the failed item's index is still written (it belongs to the index, not to the variant)
    assert any(f.endswith("_source.png") and f.startswith(bad.image_stem[:R.MAX_FILENAME_LENGTH]) for f in os.listdir(r["output_folder"]))


if __name__ == "__main__":
    # regenerate the profile:  python -m tests.test_attn_wide_host > profiles/attn_wide_errbudget.txt
    print(report(), end="")
