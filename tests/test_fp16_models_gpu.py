"""The opt-in fp16 compute mode against the CPU oracle, next to bf16 on the same cases: model graphs (tiny and full width) and the tiny
pipeline.  fp16 has 3 more mantissa bits than bf16 (unit round-off 2^-11 against 2^-8), so its distance to the fp32 oracle should be
1/8 of bf16's; the tests assert rms-rel(fp16) <= 0.25 x rms-rel(bf16) (2x margin: the compounding of rounding through a network is
not linear) and print every measured value (profiles/fp16_parity.txt records a run)."""
import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from oracle import sd_models as OM
from oracle.canny import generate_canny_array
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import (StableDiffusionControlNetImg2ImgPipeline, StableDiffusionControlNetPipeline,
                                    StableDiffusionImg2ImgPipeline)
from saspa_aug_amd.scheduler import UniPCMultistepScheduler
from saspa_aug_amd.synthetic import synthetic_image
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
RATIO = 0.25                    # rms-rel(fp16) / rms-rel(bf16): expected 1/8, asserted with a 2x margin
VERDICT_EPS = 3e-3              # the absolute figure VERDICT.md asks of one evaluation (reported, not asserted)


def _rms_rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)).item()


def _report(what, e_bf, e_16, extra=""):
    print(f"\n[fp16 parity] {what}: rms-rel bf16 {e_bf:.3e} fp16 {e_16:.3e} ratio {e_16 / e_bf:.3f} (<= {RATIO}; expected 0.125)"
          f"{' ; fp16 eps <= 3e-3: ' + str(e_16 <= VERDICT_EPS) if what.endswith(': eps') else ''}{extra}")


@pytest.fixture(scope="module")
def tiny():
    cfgs = CFG.tiny()
    return cfgs, W.synth_family(cfgs, seed=3)


@pytest.fixture(scope="module")
def full_sd15():
    cfgs = CFG.SD15
    fam = dict(unet=W.synth_state_dict("unet", cfgs["unet"], 0), controlnet=W.synth_state_dict("controlnet", cfgs["controlnet"], 1))
    cache = {}
    yield cfgs, fam, cache
    fam.clear()
    cache.clear()


def test_text_tower_tiny(dev, tiny):
    cfgs, fam = tiny
    ids = torch.from_numpy(np.random.RandomState(0).randint(0, cfgs["text"]["vocab"], (3, 77)))
    ref = OM.clip_text_forward(fam["text"], cfgs["text"], ids)
    e = {dt: _rms_rel(models.CLIPText(fam["text"], cfgs["text"], dev, dt).forward(ids.to(dev)).float(), ref) for dt in (BF, F16)}
    _report("text tower, tiny", e[BF], e[F16])
    assert e[F16] <= RATIO * e[BF], e


def _evaluation(cfgs, fam, dev, dtype, b, h, w, cache, finite=None, launches=None):
    """One UNet + ControlNet evaluation in the pipeline's order against the oracle (computed once per case): rms-rel of the noise
    prediction, of the ControlNet residuals and of the ControlNet-free UNet.  finite: a list that receives a device flag per tensor
    handed from one module to the next.  launches: a list that receives (kind, shape / kernel family / K slices) of every launch of
    the evaluation, in order (ops' launch recorder: the GEMM launches carry the library's own dispatch, saspa_gemm_which)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, 4, h, w, generator=g)
    ctx = torch.randn(b, 77, cfgs["unet"]["ctx_dim"], generator=g)
    cond = torch.rand(b, 3, 8 * h, 8 * w, generator=g)
    ts = OP.DDIM().set_timesteps(4)
    step = 1
    if "ref" not in cache:
        down, mid = OM.controlnet_forward(fam["controlnet"], cfgs["controlnet"], x, int(ts[step]), ctx, cond, 0.75)
        cache.update(down=down, mid=mid, ref=OM.unet_forward(fam["unet"], cfgs["unet"], x, int(ts[step]), ctx, down, mid))
    unet = models.UNet(fam["unet"], cfgs["unet"], dev, dtype)
    cn = models.ControlNet(fam["controlnet"], cfgs["controlnet"], dev, dtype)
    for net in (unet, cn):
        net.prepare_context(ctx.to(dev, dtype))
        net.prepare_timesteps(ts)
    xd = to_nhwc(x, dtype, dev, cpad=8)
    cemb = cn.cond_embedding(to_nhwc(cond, dtype, dev, cpad=8))
    if launches is not None:
        ops.set_recorder(lambda kind, flops, call, meta: launches.append((kind, meta)) or call())
    try:
        outs, m, umid, uskips, s2, m2, eps = _run(unet, cn, xd, step, cemb)
    finally:
        ops.set_recorder(None)
    res = torch.cat([from_nhwc(o).reshape(-1) for o in outs] + [from_nhwc(m).reshape(-1)])
    ref_res = torch.cat([r.reshape(-1) for r in cache["down"]] + [cache["mid"].reshape(-1)])
    if finite is not None:
        for t in (cemb, *outs, m, umid, *uskips, *s2, m2, eps):
            assert t.dtype == dtype
            finite.append(torch.isfinite(t).all())
    return _rms_rel(from_nhwc(eps, 4), cache["ref"]), _rms_rel(res, ref_res)


def _run(unet, cn, xd, step, cemb):
    outs, m = cn.forward(xd, step, cemb, 0.75)
    umid, uskips = unet.encode(xd, step)
    s2, m2 = cn.forward(xd, step, cemb, 0.75, uskips, umid)
    return outs, m, umid, uskips, s2, m2, unet.decode(m2, s2, step)


@pytest.mark.parametrize("b,h,w", [(2, 8, 8), (1, 8, 24)])
def test_unet_controlnet_tiny(dev, tiny, b, h, w):
    cfgs, fam = tiny
    cache = {}
    e = {dt: _evaluation(cfgs, fam, dev, dt, b, h, w, cache) for dt in (BF, F16)}
    _report(f"tiny UNet + ControlNet {b}x{h}x{w}: eps", e[BF][0], e[F16][0])
    _report(f"tiny UNet + ControlNet {b}x{h}x{w}: ControlNet residuals", e[BF][1], e[F16][1])
    assert e[F16][0] <= RATIO * e[BF][0] and e[F16][1] <= RATIO * e[BF][1], e


def test_unet_controlnet_full_width(dev, full_sd15):
    """One SD-v1.5 + ControlNet evaluation at full width, 16x16 latents, CFG batch 2 (the case of
    test_models_gpu.test_unet_controlnet_full_width_step); every activation handed between modules is finite in fp16, and the fp16
    evaluation is the bf16 one launch for launch (kind, shape, kernel family, K slices)."""
    cfgs, fam, cache = full_sd15
    finite, l_bf, l_16 = [], [], []
    e_bf = _evaluation(cfgs, fam, dev, BF, 2, 16, 16, cache, launches=l_bf)
    e_16 = _evaluation(cfgs, fam, dev, F16, 2, 16, 16, cache, finite=finite, launches=l_16)
    # fp16 takes every fused path the bf16 dispatch takes: the same launches, kernel families and K slices, in the same order
    kinds = {k for k, _ in l_16}
    assert l_16 == l_bf and len(l_16) > 300, (len(l_bf), len(l_16), [(a, b) for a, b in zip(l_bf, l_16) if a != b][:5])
    assert {"gemm", "flash_attn"} <= kinds, sorted(kinds)
    fams = sorted({m[-2] for k, m in l_16 if k == "gemm" and m})
    print(f"\n[fp16 launches] {len(l_16)} launches, kinds {sorted(kinds)}, GEMM kernel families {fams}: identical to bf16")
    _report("full-width UNet + ControlNet 2x16x16: eps", e_bf[0], e_16[0])
    _report("full-width UNet + ControlNet 2x16x16: ControlNet residuals", e_bf[1], e_16[1])
    assert len(finite) > 30 and bool(torch.stack(finite).all()), "a non-finite activation between modules in fp16"
    assert e_16[0] <= RATIO * e_bf[0] and e_16[1] <= RATIO * e_bf[1], (e_bf, e_16)


# ------------------------------------------------------------------ tiny pipeline
def _pipe_inputs(cfgs, hh, ww, nimg):
    ids = torch.from_numpy(np.random.RandomState(1).randint(0, cfgs["text"]["vocab"] - 2, (nimg, 77)))
    neg = torch.from_numpy(np.random.RandomState(2).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    srcs = np.stack([synthetic_image(hh, ww, 10 + i) for i in range(nimg)])
    ctrls = np.stack([generate_canny_array(s, 120, 200) for s in srcs])
    g = torch.manual_seed(1)
    lat = [torch.randn((1, 4, hh // 8, ww // 8), generator=g, dtype=torch.float32) for _ in range(2 * nimg)]
    return ids, neg, srcs, ctrls, torch.cat(lat[:nimg]), torch.cat(lat[nimg:])


def _psnr01(img, ref_img):
    mse = float(((from_nhwc(img, 3) / 2 + 0.5).clamp(0, 1) - (ref_img / 2 + 0.5).clamp(0, 1)).pow(2).mean())
    return 10 * np.log10(1.0 / max(mse, 1e-20))


def _build(cls, fam, cfgs, dev, mode):
    pipe = cls(fam, cfgs)
    if mode != "bf16":
        pipe.enable_fp16(True, vae=mode)
    return pipe.to(dev, torch.float16)


def test_pipeline_tiny_latents_and_image(dev, tiny):
    """64 x 64, 10 DDIM steps, 2 images: the final latents obey the ratio rule; with vae="x3" the decoded image gains >= 12 dB over
    the bf16 pipeline (expected 18 dB); with vae="bf16" the image PSNR is reported only (the VAE's own bf16 rounding bounds it)."""
    cfgs, fam = tiny
    ids, neg, _, ctrls, lat, _ = _pipe_inputs(cfgs, 64, 64, 2)
    refs = [OP.sd_controlnet_pipeline(fam, cfgs, ids[i:i + 1], neg, ctrls[i], lat[i:i + 1], 10, return_latents=True) for i in range(2)]
    ref_x, ref_img = torch.cat([r[1] for r in refs]), torch.cat([r[2] for r in refs])
    e, psnr = {}, {}
    for mode in ("bf16", "x3"):                                   # "bf16" here = the flag off
        pipe = _build(StableDiffusionControlNetPipeline, fam, cfgs, dev, mode)
        assert pipe.dtype is (BF if mode == "bf16" else F16) and pipe.vae.dtype is (BF if mode == "bf16" else torch.float32)
        out, x, img = pipe.generate_batch(ids.numpy(), neg.numpy(), ctrls, lat, 10, return_latents=True)
        assert x.dtype is pipe.dtype and out.dtype is torch.uint8
        e[mode], psnr[mode] = _rms_rel(from_nhwc(x, 4), ref_x), _psnr01(img, ref_img)
    p16 = StableDiffusionControlNetPipeline(fam, cfgs).enable_fp16().to(dev, torch.float16)       # vae="bf16" (the default)
    assert p16.dtype is F16 and p16.vae.dtype is BF and p16.text_encoder.dtype is F16 and p16.unet.dtype is F16
    _, x16, img16 = p16.generate_batch(ids.numpy(), neg.numpy(), ctrls, lat, 10, return_latents=True)
    _report("tiny pipeline 64x64, 10 DDIM steps, 2 images: final latents", e["bf16"], e["x3"],
            f"; image PSNR bf16 {psnr['bf16']:.2f} dB, fp16 + vae x3 {psnr['x3']:.2f} dB (gain {psnr['x3'] - psnr['bf16']:.2f} dB, >= 12 "
            f"asserted, 18 expected), fp16 + vae bf16 {_psnr01(img16, ref_img):.2f} dB (reported only)")
    assert torch.equal(x16, x)                                    # the VAE choice does not touch the sampling loop
    assert e["x3"] <= RATIO * e["bf16"], e
    assert psnr["x3"] - psnr["bf16"] >= 12.0, psnr


def test_graph_replay_equals_python_loop_fp16(dev, tiny, monkeypatch):
    cfgs, fam = tiny
    ids, neg, _, ctrls, lat, _ = _pipe_inputs(cfgs, 64, 64, 2)
    outs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("SASPA_GRAPH", flag)
        pipe = _build(StableDiffusionControlNetPipeline, fam, cfgs, dev, "x3")
        outs[flag] = pipe.generate_batch(ids.numpy(), neg.numpy(), ctrls, lat, 6, return_latents=True)[1].clone()
        assert outs[flag].dtype is F16
    assert torch.equal(outs["0"], outs["1"])


def _watch_steps(monkeypatch, flags):
    """Every scheduler-step launch of the Python loop also leaves a device flag: eps and the updated latents are finite."""
    for name in ("cfg_ddim_step", "cfg_unipc_step"):
        real = getattr(ops, name)

        def watched(eps, x, *a, _real=real, **k):
            r = _real(eps, x, *a, **k)
            assert x.dtype is F16 and eps.dtype is F16
            flags.append(torch.isfinite(eps).all() & torch.isfinite(x).all())
            return r
        monkeypatch.setattr(ops, name, watched)


@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
def test_latents_finite_at_every_step_50_steps(dev, tiny, monkeypatch, sampler):
    cfgs, fam = tiny
    ids, neg, _, ctrls, lat, _ = _pipe_inputs(cfgs, 64, 64, 2)
    monkeypatch.setenv("SASPA_GRAPH", "0")
    flags = []
    _watch_steps(monkeypatch, flags)
    pipe = StableDiffusionControlNetPipeline(fam, cfgs, scheduler=UniPCMultistepScheduler() if sampler == "unipc" else None)
    pipe.enable_fp16().to(dev, torch.float16)
    out = pipe.generate_batch(ids.numpy(), neg.numpy(), ctrls, lat, 50)
    assert len(flags) == 50 and bool(torch.stack(flags).all()), f"non-finite latents in fp16 ({sampler})"
    assert out.shape == (2, 64, 64, 3)


@pytest.mark.parametrize("vae", ["bf16", "x3"])
@pytest.mark.parametrize("cls", [StableDiffusionControlNetImg2ImgPipeline, StableDiffusionImg2ImgPipeline])
def test_img2img_fp16_strength_half(dev, tiny, monkeypatch, cls, vae):
    """vae="x3": the fp32 VAE encoder under SASPA_F32X3 GEMMs hands its moments to the fp16 latents by an explicit cast."""
    cfgs, fam = tiny
    ids, neg, srcs, ctrls, e1, e2 = _pipe_inputs(cfgs, 64, 64, 2)
    monkeypatch.setenv("SASPA_GRAPH", "0")
    flags = []
    _watch_steps(monkeypatch, flags)
    pipe = cls(fam, cfgs).enable_fp16(True, vae=vae).to(dev, torch.float16)
    vdt = BF if vae == "bf16" else torch.float32
    assert pipe.vae_encoder.dtype is vdt and pipe.vae.dtype is vdt and pipe.dtype is F16
    assert pipe.vae.f32_gemm == ("x3" if vae == "x3" else "exact")
    args = (srcs, ctrls) if cls is StableDiffusionControlNetImg2ImgPipeline else (srcs,)
    out, x, _ = pipe.generate_batch_img2img(ids.numpy(), neg.numpy(), *args, e1, e2, 50, 0.5, return_latents=True)
    assert len(flags) == 25 and bool(torch.stack(flags).all()) and x.dtype is F16 and out.shape == (2, 64, 64, 3)


def test_flag_off_selects_bf16_and_opens_nothing(dev, tiny):
    """Without enable_fp16() / SASPA_FP16 nothing changes: torch.float16 still selects bf16, and a process that only does that never
    opens the fp16 library (checked in a fresh interpreter: this session's other tests have loaded it)."""
    import os
    import subprocess
    import sys
    cfgs, fam = tiny
    pipe = StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.float16)
    assert pipe.dtype is BF and pipe.vae.dtype is BF and pipe.unet.dtype is BF and pipe.noise_dtype is F16
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, numpy as np, saspa_aug_amd\n"
            "from saspa_aug_amd import _lib, config as CFG, weights as W\n"
            "from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline as P\n"
            "cfgs = CFG.tiny(); pipe = P(W.synth_family(cfgs, seed=3), cfgs).to('cuda:0', torch.float16)\n"
            "ids = np.zeros((1, 77), dtype=np.int64); ctrl = np.zeros((1, 64, 64, 3), dtype=np.uint8)\n"
            "pipe.generate_batch(ids, ids, ctrl, torch.randn(1, 4, 8, 8), 2)\n"
            "assert pipe.dtype is torch.bfloat16 and not _lib.f16_loaded()\n"
            "assert 'libsaspa_hip_f16' not in open('/proc/self/maps').read()\n"
            "print('flag off: bf16, fp16 library not opened')\n")
    env = {k: v for k, v in os.environ.items() if k not in ("SASPA_FP16", "SASPA_FP16_VAE")}
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fp16 library not opened" in r.stdout, r.stdout + r.stderr


def test_env_switch(dev, tiny, monkeypatch):
    cfgs, fam = tiny
    monkeypatch.setenv("SASPA_FP16", "1")
    monkeypatch.setenv("SASPA_FP16_VAE", "x3")
    pipe = StableDiffusionControlNetPipeline(fam, cfgs).to(dev)
    assert pipe.dtype is F16 and pipe.vae.dtype is torch.float32 and pipe.vae.f32_gemm == "x3" and _lib.f16_loaded()
    assert StableDiffusionControlNetPipeline(fam, cfgs).to(dev, torch.float32).dtype is torch.float32     # fp32 stays fp32
