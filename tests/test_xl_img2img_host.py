"""Host side of the SDXL-Turbo ControlNet img2img (SDEdit) form (no GPU): init_pipeline's branch, the step-count helper, the kwargs
pass_thorugh_pipe hands a pipeline, the refusals and predicates that must still hold, and the VAE classes' new keywords."""
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, models
from saspa_aug_amd import config as CFG
from saspa_aug_amd import pipeline as P
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import scheduler as S


def _init(base, controlnet, sdedit, **kw):
    return R.init_pipeline(base, controlnet, sdedit, cfgs=CFG.tiny_xl(), state_dicts={}, **kw)


def test_init_pipeline_builds_the_img2img_form():
    pipe = _init("sd_xl-turbo", "canny", 1)
    assert type(pipe) is P.StableDiffusionXLControlNetImg2ImgPipeline and type(pipe.scheduler) is S.DDIMScheduler
    assert pipe.scheduler.config["timestep_spacing"] == "trailing" and pipe._vae_fp32 and pipe._vae_mode is None
    assert not pipe.SUPPORTS_FP16 and pipe.vae_encoder is None
    with pytest.raises(NotImplementedError):
        pipe.enable_fp16()
    assert _init("sd_xl-turbo", "canny", 1, xl_vae="f16")._vae_mode == "f16"
    assert type(_init("sd_xl-turbo", "canny", 0)) is P.StableDiffusionXLControlNetPipeline        # the text-to-image form is unchanged


def test_refusals_that_stay():
    for combo in (("sd_xl-turbo", None, 1), ("sd_xl", "canny", 1), ("sd_xl-turbo", None, 0), ("sd_xl", "canny", 0)):
        with pytest.raises(NotImplementedError):
            _init(*combo)
    with pytest.raises(NotImplementedError, match="unipcmultistep"):
        _init("sd_xl-turbo", "canny", 1, sampler="unipcmultistep")


@pytest.mark.parametrize("steps,strength,want", [(2, 0.85, (1, 1)), (4, 0.5, (2, 2)), (50, 0.15, (43, 7))])
def test_step_count_helper(steps, strength, want):
    assert P.img2img_steps(steps, strength) == want


def test_step_count_helper_refuses_zero_steps_and_bad_strengths():
    with pytest.raises(ValueError, match="number of pipeline steps is 0"):
        P.img2img_steps(2, 0.4)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="strength"):
            P.img2img_steps(4, bad)


def test_generate_refuses_zero_steps_before_it_needs_a_device(monkeypatch):
    pipe = _init("sd_xl-turbo", "canny", 1)
    monkeypatch.setattr(pipe, "_need_device", lambda: None)
    with pytest.raises(ValueError, match="number of pipeline steps is 0"):       # nothing was converted, encoded or launched
        pipe.generate_batch_img2img(None, None, None, None, None, None, 2, 0.4)


def test_pass_thorugh_pipe_kwargs():
    seen = {}

    class FakePipe:
        def __call__(self, **kw):
            seen.update(kw)
            return type("O", (), {"images": ["img"]})()
    gen = torch.Generator()
    out = R.pass_thorugh_pipe("sd_xl-turbo", FakePipe(), "a bird", "src", 1, 0.5, 4, gen, 0, 0.75, negative_prompt=None, control_image="ctrl")
    assert out == "img"
    assert seen == {"prompt": "a bird", "num_inference_steps": 4, "generator": gen, "guidance_scale": 0, "negative_prompt": None,
                    "control_image": "ctrl", "controlnet_conditioning_scale": 0.75, "image": "src", "strength": 0.5}


def test_output_folder_carries_the_strength():
    s = R.Settings(BASE_MODEL="sd_xl-turbo", SDEDIT=1, SDEDIT_STRENGTH=0.5)
    assert "/aug_data/controlnet/sd_xl-turbo-SDEdit_strength_0.5/canny/" in R.output_folder_for(s, "/root")


def test_vae_attention_predicates(monkeypatch):
    monkeypatch.delenv("SASPA_VAE_ATTN", raising=False)
    monkeypatch.delenv("SASPA_VAE_ATTN_F32", raising=False)
    pinned = lambda: (models.vae_attn_fused(torch.float16), models.vae_attn_fused(torch.bfloat16), models.vae_attn_fused(torch.float32))  # noqa: E731
    assert pinned() == (True, False, False) and not models.vae_attn_f32_fused()
    monkeypatch.setenv("SASPA_VAE_ATTN_F32", "fused")
    assert pinned() == (True, False, False) and models.vae_attn_f32_fused()
    monkeypatch.setenv("SASPA_VAE_ATTN_F32", "unfused")
    assert not models.vae_attn_f32_fused()
    monkeypatch.setenv("SASPA_VAE_ATTN_F32", "flash")
    with pytest.raises(ValueError, match="SASPA_VAE_ATTN_F32"):
        models.vae_attn_f32_fused()


def test_vae_keywords_are_validated_before_anything_is_packed():
    for cls in (models.VAEDecoder, models.VAEEncoder):
        with pytest.raises(ValueError, match="f32_gemm"):
            cls({}, {}, "cpu", torch.float32, f32_gemm="bf16")
        with pytest.raises(ValueError, match="attn_f32"):
            cls({}, {}, "cpu", torch.float32, attn_f32="flash")


def test_the_new_symbol_is_exported_by_the_default_library_only():
    lib, f16 = _lib.load(), _lib.load_f16()
    assert hasattr(lib, "saspa_attn_wide_f32x3") and not hasattr(f16, "saspa_attn_wide_f32x3")
    assert "saspa_attn_wide_f32x3" in _lib.SYMBOLS and "saspa_attn_wide_f32x3" not in _lib.F16_SYMBOL_NAMES
    # (its validation codes: tests/test_attn_wide_x3_host.py)
    assert lib.saspa_attn_wide_f32x3(None, 192, 0, None, 192, 0, None, 192, 0, None, 192, 0, 1, 1, 1, 192, 1.0, None) == _lib.SASPA_EINVAL
