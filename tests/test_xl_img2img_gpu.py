"""StableDiffusionXLControlNetImg2ImgPipeline on the MI355X against its CPU restatement (tests/xl_img2img_ref.py) on identical seeded
weights / token ids / source and control images / noise draws: fp32 parity at the bar of the XL text-to-image parity test (atol 1e-3 on
the decoded image in [0,1], <= 1 u8 level), graph replay against the Python launch loop, the bf16 denoiser with the x3 and the fp16
VAE, the reference's call form and the batched run_aug loop."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from oracle.canny import generate_canny_array
from saspa_aug_amd import run_aug as R
from saspa_aug_amd.pipeline import StableDiffusionXLControlNetImg2ImgPipeline
from saspa_aug_amd.synthetic import synthetic_image
from tests import xl_img2img_ref as X
from tests.util import from_nhwc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe32(dev):
    cfgs, fam = X.tiny_xl()
    return StableDiffusionXLControlNetImg2ImgPipeline(fam, cfgs).upcast_vae().to(dev, torch.float32)


def _run(pipe, hh, ww, steps, strength, guidance=0.0, negative=False, **kw):
    ids1, ids2, n1, n2, srcs, ctrls, e1, e2 = X.inputs(hh, ww)
    return pipe.generate_batch_img2img(ids1, n1 if negative else None, srcs, ctrls, e1, e2, steps, strength, guidance, 0.75,
                                       prompt_ids_2=ids2, negative_ids_2=n2 if negative else None, **kw)


def _distances(pipe, hh, ww, steps, strength, guidance=0.0, negative=False):
    ref_u8, ref_x, ref_img = X.reference(hh, ww, steps, strength, guidance, negative)
    out, x, img = _run(pipe, hh, ww, steps, strength, guidance, negative, return_latents=True)
    d01 = ((from_nhwc(img, 3) / 2 + 0.5).clamp(0, 1) - (ref_img / 2 + 0.5).clamp(0, 1)).abs().max().item()
    du8 = int(np.abs(out.cpu().numpy().astype(int) - ref_u8.astype(int)).max())
    ex = ((from_nhwc(x, 4) - ref_x).abs().max() / ref_x.abs().max()).item()
    return d01, du8, ex


@pytest.mark.parametrize("hh,ww,steps,strength,guidance,negative", [
    (64, 64, 4, 0.5, 0.0, False),           # two of four steps
    (64, 96, 2, 0.85, 0.0, False),          # the reference's sd_xl-turbo point: one of two steps, a non-square image
    (64, 96, 4, 0.5, 5.0, True),            # guidance with a negative prompt
], ids=["64x64-4-0.5", "64x96-2-0.85", "64x96-4-0.5-cfg-neg"])
def test_fp32_parity(pipe32, hh, ww, steps, strength, guidance, negative):
    assert pipe32.vae.dtype == pipe32.vae_encoder.dtype == torch.float32 and pipe32.vae_encoder.f32_gemm == pipe32.vae.f32_gemm == "x3"
    d01, du8, ex = _distances(pipe32, hh, ww, steps, strength, guidance, negative)
    print(f"xl img2img fp32 {hh}x{ww} steps {steps} strength {strength} guidance {guidance}: d01 {d01:.3e} du8 {du8} latents {ex:.3e}")
    assert d01 < 1e-3 and du8 <= 1, (d01, du8, ex)


def test_graph_replay_equals_the_launch_loop(pipe32, monkeypatch):
    outs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SASPA_GRAPH", graph)
        outs.append(_run(pipe32, 64, 64, 4, 0.5).clone())
    assert torch.equal(*outs)


def test_zero_steps_raise_before_anything_is_launched(pipe32):
    from saspa_aug_amd import ops
    log = []
    ops.set_recorder(lambda kind, flops, call, meta: log.append(kind) or call())
    try:
        with pytest.raises(ValueError, match="number of pipeline steps is 0"):
            _run(pipe32, 64, 64, 2, 0.4)
    finally:
        ops.set_recorder(None)
    assert not log


def _psnr(a, b):
    mse = ((a.float() - b.float()) ** 2).mean().item()
    return math.inf if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("vae_mode", [None, "f16"])
def test_bf16_denoiser(dev, pipe32, vae_mode):
    """bf16 denoiser with the default (x3 after upcast_vae) VAE and with the fp16 VAE: finite, deterministic; PSNR against the fp32
    run reported."""
    cfgs, fam = X.tiny_xl()
    pipe = StableDiffusionXLControlNetImg2ImgPipeline(fam, cfgs)
    if vae_mode is not None:
        pipe.set_vae_mode(vae_mode)
    pipe = pipe.upcast_vae().to(dev, torch.bfloat16)
    want = torch.float16 if vae_mode == "f16" else torch.float32
    assert pipe.vae.dtype == pipe.vae_encoder.dtype == want and pipe.unet.dtype == torch.bfloat16
    a, x, img = _run(pipe, 64, 96, 4, 0.5, return_latents=True)
    b = _run(pipe, 64, 96, 4, 0.5)
    assert torch.equal(a, b) and bool(torch.isfinite(img[..., :3].float()).all())
    if vae_mode == "f16":
        assert pipe.last_nonfinite is not None and not bool(pipe.last_nonfinite.any())
    else:
        assert pipe.last_nonfinite is None
    print(f"xl img2img bf16 denoiser, VAE {vae_mode or 'x3'}: PSNR vs fp32 {_psnr(a, _run(pipe32, 64, 96, 4, 0.5)):.1f} dB")
    # the encoder follows the VAE mode after .to() as well
    pipe.set_vae_mode("exact")
    assert (pipe.vae_encoder.dtype, pipe.vae_encoder.f32_gemm) == (torch.float32, "exact") == (pipe.vae.dtype, pipe.vae.f32_gemm)


def test_call_form_equals_generate_batch(dev):
    cfgs, fam = X.tiny_xl()
    pipe = R.init_pipeline("sd_xl-turbo", "canny", 1, cfgs=cfgs, state_dicts=fam)
    assert isinstance(pipe, StableDiffusionXLControlNetImg2ImgPipeline)
    pipe = pipe.to(dev, torch.bfloat16)
    src_u8 = synthetic_image(64, 96, 4)
    ctrl_u8 = generate_canny_array(src_u8, 120, 200)
    src, ctrl = Image.fromarray(src_u8), Image.fromarray(ctrl_u8)
    a = R.pass_thorugh_pipe("sd_xl-turbo", pipe, "a bird on a branch", src, 1, 0.5, 4, torch.manual_seed(1), 0, 0.75,
                            negative_prompt=None, control_image=ctrl)
    g = torch.manual_seed(1)
    e1 = torch.randn((1, 4, 8, 12), generator=g, dtype=pipe.noise_dtype)
    e2 = torch.randn((1, 4, 8, 12), generator=g, dtype=pipe.noise_dtype)
    ids1 = pipe.tokenizer("a bird on a branch")
    ids2 = pipe.pad_ids_2(pipe.tokenizer_2("a bird on a branch"))
    b = pipe.generate_batch_img2img(ids1, None, src_u8[None], ctrl_u8[None], e1, e2, 4, 0.5, 0, 0.75, prompt_ids_2=ids2)
    assert a.size == (96, 64) and np.array_equal(np.asarray(a), b[0].cpu().numpy())
    with pytest.raises(ValueError):
        pipe(prompt="x", image=src, control_image=ctrl, strength=0.4, num_inference_steps=2, generator=torch.manual_seed(1))


def test_run_aug_end_to_end(dev, tmp_path):
    cfgs, fam = X.tiny_xl()
    pipe = R.init_pipeline("sd_xl-turbo", "canny", 1, cfgs=cfgs, state_dicts=fam).to(dev, torch.float16)
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("".join(f"a bird in scene {k}.\n" for k in range(6)))
    s = R.Settings(DATASET="synthetic", BASE_MODEL="sd_xl-turbo", SDEDIT=1, SDEDIT_STRENGTH=0.5, RESOLUTION=64, NUM_INFERENCE_STEPS=4,
                   GUIDANCE_SCALE=0, NUM_PER_IMAGE=2, SEED=1, USE_ARTISTIC_PROMPTS=False, SEMANTIC_FILTERING=0,
                   MODEL_CONFIDENCE_BASED_FILTERING=0, PROMPTS_FILE=str(prompts), BATCH_SIZE=4,
                   DATASET_KWARGS=dict(root_path=str(tmp_path / "ds" / "data"), n_images=3, sizes=((64, 64), (64, 128))))
    res = R.main(s, pipe=pipe)
    out = Path(res["output_folder"])
    assert "aug_data/controlnet/sd_xl-turbo-SDEdit_strength_0.5/canny/" in str(out)
    assert (res["status"] == 1).all() and len(res["items"]) == 6
    pngs = sorted(p.name for p in out.glob("*.png"))
    assert len([n for n in pngs if "_prompt_" in n]) == 6
    assert len([n for n in pngs if n.endswith("_source.png")]) == 3 and len([n for n in pngs if n.endswith("_control.png")]) == 3
    body = json.load(open(res["json_path"]))
    assert len(body) == 3 and all(len(v) == 2 for v in body.values())
    assert all("_source" not in p and "_control" not in p for v in body.values() for p in v)
    # item 0 of the batched run == the single call with the same two draws from the seed-1 stream and both tokenizers
    it = res["items"][0]
    src = Image.open(it.source_path).convert("RGB")
    single = pipe(prompt=it.prompt, image=src, control_image=Image.fromarray(generate_canny_array(np.array(src), 120, 200)),
                  strength=0.5, num_inference_steps=4, generator=torch.manual_seed(1), guidance_scale=0, negative_prompt=None,
                  controlnet_conditioning_scale=s.CONTROLNET_CONDITIONING_SCALE).images[0]
    assert np.array_equal(np.asarray(single), np.array(Image.open(it.output_path)))
    res2 = R.main(s, pipe=pipe)
    assert all(it.skip for it in res2["items"]) and (res2["status"] == 0).all()
