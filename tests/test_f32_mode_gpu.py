"""The fp32 mode switch (pipe.set_f32_mode / SASPA_F32_GEMM / SASPA_F32_ATTN) on the GPU: module and pipeline parity against the CPU
oracle at the project's own fp32 bars, and what the launch recorder sees with the switch set, unset and in a 16-bit dtype."""
import contextlib

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from oracle import sd_models as OM
from oracle.canny import generate_canny_array
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline
from saspa_aug_amd.synthetic import synthetic_image
from tests.test_fp16_models_gpu import _evaluation
from tests.test_models_gpu import _relerr, _unet_cn_case
from tests.util import from_nhwc

pytestmark = pytest.mark.gpu
F32_BAR = 2e-4                                    # test_models_gpu._limits(torch.float32): the fp32 module bar
TODAY = ("exact", "unfused")
MODES = (("exact", "fused"), ("x3", "fused"))


@contextlib.contextmanager
def _modes(gemm, attn):
    with ops.f32_gemm_mode(gemm), ops.f32_attn_mode(attn):
        yield


@pytest.fixture(scope="module")
def tiny():
    cfgs = CFG.tiny()
    return cfgs, W.synth_family(cfgs, seed=3)


# ---- modules ----------------------------------------------------------------------------------------------------------------
def test_clip_text_tiny_in_every_mode(dev, tiny):
    cfgs, fam = tiny
    ids = torch.from_numpy(np.random.RandomState(0).randint(0, cfgs["text"]["vocab"], (3, 77)))
    ref = OM.clip_text_forward(fam["text"], cfgs["text"], ids)
    net = models.CLIPText(fam["text"], cfgs["text"], dev, torch.float32)
    e = {}
    for mode in (TODAY,) + MODES:
        with _modes(*mode):
            e[mode] = _relerr(net.forward(ids.to(dev)).float().cpu(), ref)
    for mode in MODES:
        print(f"\n[f32 mode] CLIP text tiny {mode}: relerr {e[mode]:.3e} (today {TODAY}: {e[TODAY]:.3e}; bar {F32_BAR})")
    assert all(e[mode] < F32_BAR for mode in (TODAY,) + MODES), e


@pytest.mark.parametrize("b,h,w", [(2, 8, 8), (1, 8, 24)])
def test_unet_controlnet_tiny_in_every_mode(dev, tiny, b, h, w):
    cfgs, fam = tiny
    cache, e = {}, {}
    for mode in (TODAY,) + MODES:
        with _modes(*mode):
            e[mode] = _unet_cn_case(cfgs, fam, dev, torch.float32, b, h, w, cache=cache)
    for mode in MODES:
        print(f"\n[f32 mode] tiny UNet + ControlNet {b}x{h}x{w} {mode}: ControlNet / UNet / plain UNet relerr "
              + " / ".join(f"{v:.3e}" for v in e[mode]) + f" (today {TODAY}: " + " / ".join(f"{v:.3e}" for v in e[TODAY]) + f"; bar {F32_BAR})")
    assert all(max(e[mode]) < F32_BAR for mode in (TODAY,) + MODES), e


# ---- the tiny pipeline at the north-star bar --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipeline_case(tiny):
    """Inputs and oracle images of test_models_gpu.test_pipeline_fp32_parity_tiny's case (64 x 64, 10 DDIM steps, 2 images); once."""
    cfgs, fam = tiny
    hh = ww = 64
    steps, nimg = 10, 2
    ids = torch.from_numpy(np.random.RandomState(1).randint(0, cfgs["text"]["vocab"] - 2, (nimg, 77)))
    neg = torch.from_numpy(np.random.RandomState(2).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    ctrls = np.stack([generate_canny_array(synthetic_image(hh, ww, 10 + i), 120, 200) for i in range(nimg)])
    g = torch.manual_seed(1)
    lat = torch.cat([torch.randn((1, 4, hh // 8, ww // 8), generator=g, dtype=torch.float32) for _ in range(nimg)])
    refs = [OP.sd_controlnet_pipeline(fam, cfgs, ids[i:i + 1], neg, ctrls[i], lat[i:i + 1], steps, return_latents=True)
            for i in range(nimg)]
    return dict(ids=ids, neg=neg, ctrls=ctrls, lat=lat, steps=steps, ref_u8=np.concatenate([r[0] for r in refs]),
                ref_img=torch.cat([r[2] for r in refs]))


def _run_pipeline(pipe, c, steps=None):
    return pipe.generate_batch(c["ids"].numpy(), c["neg"].numpy(), c["ctrls"], c["lat"], steps or c["steps"], return_latents=True)


def _distance(out, img, c):
    d01 = ((from_nhwc(img, 3) / 2 + 0.5).clamp(0, 1) - (c["ref_img"] / 2 + 0.5).clamp(0, 1)).abs().max().item()
    return d01, int(np.abs(out.cpu().numpy().astype(int) - c["ref_u8"].astype(int)).max())


@pytest.mark.parametrize("how", ["set_f32_mode", "environment"])
def test_pipeline_fp32_parity_tiny_x3_fused(dev, tiny, pipeline_case, monkeypatch, how):
    cfgs, fam = tiny
    monkeypatch.delenv("SASPA_F32_GEMM", raising=False)
    monkeypatch.delenv("SASPA_F32_ATTN", raising=False)
    today = StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.float32)
    assert (today.f32_gemm, today.f32_attn) == TODAY
    out, _, img = _run_pipeline(today, pipeline_case)
    d_today = _distance(out, img, pipeline_case)
    pipe = StableDiffusionControlNetPipeline(fam, cfgs)
    if how == "set_f32_mode":
        assert pipe.set_f32_mode("x3", "fused") is pipe
    else:
        monkeypatch.setenv("SASPA_F32_GEMM", "x3")
        monkeypatch.setenv("SASPA_F32_ATTN", "fused")
    pipe.to(dev, torch.float32)
    assert (pipe.f32_gemm, pipe.f32_attn) == ("x3", "fused")
    with pytest.raises(RuntimeError, match="before .to"):
        pipe.set_f32_mode("exact", "unfused")
    out, _, img = _run_pipeline(pipe, pipeline_case)
    d01, du8 = _distance(out, img, pipeline_case)
    print(f"\n[f32 mode] tiny pipeline (x3, fused) via {how}: max|d| {d01:.3e} u8 {du8} (today {TODAY}: {d_today[0]:.3e} u8 {d_today[1]})")
    assert d01 < 1e-3 and du8 <= 1, (d01, du8)


def test_unknown_environment_values_raise(dev, tiny, monkeypatch):
    cfgs, fam = tiny
    monkeypatch.setenv("SASPA_F32_ATTN", "flash")
    with pytest.raises(ValueError, match="fp32 attention mode"):
        StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.float32)
    StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.bfloat16)        # read for the fp32 dtype only


# ---- what the recorder sees -------------------------------------------------------------------------------------------------
def _launches(pipe, c):
    """(kind, meta) of every launch of a 2-step run of the pipeline, in order (under a recorder the step runs from Python)."""
    got = []
    ops.set_recorder(lambda kind, flops, call, meta: got.append((kind, meta)) or call())
    try:
        _run_pipeline(pipe, c, steps=2)
    finally:
        ops.set_recorder(None)
    return got


def test_fused_mode_launches_the_new_kernel_and_no_row_softmax(dev, tiny, pipeline_case, monkeypatch):
    cfgs, fam = tiny
    monkeypatch.delenv("SASPA_F32_GEMM", raising=False)
    monkeypatch.delenv("SASPA_F32_ATTN", raising=False)
    # one UNet + ControlNet evaluation (the launches of test_fp16_models_gpu._evaluation): every attention is the new launch
    cache, plain, default, fused = {}, [], [], []
    _evaluation(cfgs, fam, dev, torch.float32, 2, 8, 8, cache, launches=plain)               # the contexts never entered
    with _modes(*TODAY):
        _evaluation(cfgs, fam, dev, torch.float32, 2, 8, 8, cache, launches=default)
    with _modes("exact", "fused"):
        _evaluation(cfgs, fam, dev, torch.float32, 2, 8, 8, cache, launches=fused)
    assert default == plain and len(plain) > 100
    n_attn = sum(k == "softmax_rows" for k, _ in plain)
    assert n_attn > 0 and all(k != "flash_attn_f32x3" for k, _ in plain)
    assert sum(k == "flash_attn_f32x3" for k, _ in fused) == n_attn and all(k != "softmax_rows" for k, _ in fused)
    assert all(m is not None and len(m) == 5 for k, m in fused if k == "flash_attn_f32x3")   # (batch, heads, nq, nk, d) with the FLOPs
    assert len(fused) == len(plain) - 2 * n_attn                                            # two GEMMs and a softmax became one launch
    # the pipeline: text tower and networks run fused, the VAE and the safety checker keep their own rule
    pipe = StableDiffusionControlNetPipeline(fam, cfgs).set_f32_mode("exact", "fused").to(dev, torch.float32)
    kinds = [k for k, _ in _launches(pipe, pipeline_case)]
    text_at = kinds.index("u8_to_act")                    # the control image is converted after the prompts are encoded
    assert kinds[:text_at].count("flash_attn_f32x3") == 2 * cfgs["text"]["layers"] and "softmax_rows" not in kinds[:text_at]
    assert kinds[text_at:].count("flash_attn_f32x3") > 0 and "softmax_rows" in kinds[text_at:]


def test_unset_mode_launches_what_a_run_without_the_contexts_launches(dev, tiny, pipeline_case, monkeypatch):
    cfgs, fam = tiny
    monkeypatch.delenv("SASPA_F32_GEMM", raising=False)
    monkeypatch.delenv("SASPA_F32_ATTN", raising=False)
    pipe = StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.float32)
    _launches(pipe, pipeline_case)                       # (the first run also encodes the negative prompt, cached afterwards)
    with_switch = _launches(pipe, pipeline_case)
    monkeypatch.setattr(pipe, "_f32_scope", contextlib.nullcontext)          # the contexts never entered
    without = _launches(pipe, pipeline_case)
    assert with_switch == without and len(without) > 100
    kinds = {k for k, _ in without}
    assert "flash_attn_f32x3" not in kinds and "softmax_rows" in kinds


def test_bf16_pipeline_ignores_the_switch(dev, tiny, pipeline_case, monkeypatch):
    cfgs, fam = tiny
    monkeypatch.delenv("SASPA_F32_GEMM", raising=False)
    monkeypatch.delenv("SASPA_F32_ATTN", raising=False)
    plain = _launches(StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.bfloat16), pipeline_case)
    switched = _launches(StableDiffusionControlNetPipeline(fam, cfgs).set_f32_mode("x3", "fused").to(dev, torch.bfloat16), pipeline_case)
    assert switched == plain and len(plain) > 100
    assert "flash_attn_f32x3" not in {k for k, _ in plain}
