"""CPU proof of the ControlNet-free text-to-image / SD-2.1 pipelines and the v-prediction sampler steps: the `init_pipeline`
switchboard, the call form, the entrypoints' switches, the SD-2.1 weight layout, the GELU text tower against transformers, the dry
GEMM / attention plans of the full-width SD-2.1 UNet, the step references with their mutants (tests/sd21_ref.py) and the exported
symbols.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import sd_models as OM
from saspa_aug_amd import _lib, ops, pipeline as P, run_aug as R, scheduler as S
from saspa_aug_amd import config as CFG
from saspa_aug_amd import weights as W
from tests import sd21_ref as REF
from tests import test_errbudget as TE
from tests.errbudget import budget_stats, check_budget, fmt, ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_SYMBOLS = ("saspa_cfg_ddim_step_v", "saspa_ddim_step_v", "saspa_ddim_step_v_dev", "saspa_cfg_unipc_step_v", "saspa_unipc_step_v")


# ------------------------------------------------------------------ init_pipeline
def _init(base, controlnet, sdedit, cfgs, **kw):
    return R.init_pipeline(base, controlnet, sdedit, cfgs=cfgs, state_dicts=W.synth_family(cfgs, 0), **kw)


def test_init_pipeline_builds_the_controlnet_free_forms():
    t15, t21 = CFG.tiny(), CFG.tiny_sd21()
    for base, cfgs in (("sd_v1.5", t15), ("sd_v2.1", t21)):
        p = _init(base, None, 0, cfgs)
        assert type(p) is P.StableDiffusionPipeline and not p.HAS_CONTROLNET and type(p.scheduler) is S.DDIMScheduler
        assert type(_init(base, None, 0, cfgs, sampler="unipcmultistep").scheduler) is S.UniPCMultistepScheduler
    p = _init("sd_v2.1", None, 1, t21)
    assert type(p) is P.StableDiffusionImg2ImgPipeline and p.cfgs is t21
    assert p.tokenizer.pad == 0 and _init("sd_v1.5", None, 0, t15).tokenizer.pad == t15["text"]["vocab"] - 1      # pad id 0 / EOS
    # the defaults are the full-width families
    assert R.init_pipeline.__defaults__ is not None and CFG.SD21["unet"]["ctx_dim"] == CFG.SD21["text"]["width"] == 1024
    assert "controlnet" not in CFG.SD21 and "safety" not in CFG.SD21 and CFG.SD21["vae"] is CFG.SD15_VAE
    for cn in ("canny", "hed"):
        for sdedit in (0, 1):
            with pytest.raises(NotImplementedError, match=r"768.*1024|1024.*768"):
                R.init_pipeline("sd_v2.1", cn, sdedit)


def test_existing_combinations_return_what_they_did():
    t = CFG.tiny()
    assert type(_init("sd_v1.5", "canny", 0, t)) is P.StableDiffusionControlNetPipeline
    assert type(_init("sd_v1.5", "hed", 1, t)) is P.StableDiffusionControlNetImg2ImgPipeline
    assert type(_init("sd_v1.5", None, 1, t)) is P.StableDiffusionImg2ImgPipeline
    assert type(_init("ip2p", None, 0, CFG.tiny_ip2p())) is P.StableDiffusionInstructPix2PixPipeline
    assert type(_init("blip_diffusion", "canny", 0, t)) is P.BlipDiffusionControlNetPipeline
    assert type(_init("sd_xl-turbo", "canny", 0, CFG.tiny_xl())) is P.StableDiffusionXLControlNetPipeline
    for combo in (("sd_xl", None, 0), ("sd_xl-turbo", None, 0), ("blip_diffusion", None, 0), ("ip2p", "canny", 0)):
        with pytest.raises(NotImplementedError):
            R.init_pipeline(*combo)


def test_v_prediction_travels_from_the_checkpoint_to_the_sampler(tmp_path):
    """A checkpoint directory whose scheduler_config.json says v_prediction gives a v-prediction DDIM / UniPC scheduler."""
    import json
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(prediction_type="v_prediction", beta_schedule="scaled_linear")))
    sch = P._checkpoint_scheduler(str(tmp_path))
    assert sch.config["prediction_type"] == "v_prediction"
    p = P.StableDiffusionPipeline(W.synth_family(CFG.tiny_sd21(), 0), CFG.tiny_sd21(), scheduler=sch)
    for cls in (S.DDIMScheduler, S.UniPCMultistepScheduler):
        assert cls.from_config(p.scheduler.config).config["prediction_type"] == "v_prediction"
    assert P._checkpoint_scheduler(str(tmp_path / "scheduler")) is None                      # no file: the SD default (epsilon)
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(prediction_type="sample")))
    with pytest.raises(NotImplementedError):
        P._checkpoint_scheduler(str(tmp_path))


def test_schedulers_accept_v_prediction_and_keep_their_refusals():
    d = S.DDIMScheduler(prediction_type="v_prediction")
    e = S.DDIMScheduler()
    d.set_timesteps(4), e.set_timesteps(4)
    assert d.step_coefficients(501) == e.step_coefficients(501)                               # the same four constants
    u = S.UniPCMultistepScheduler(prediction_type="v_prediction").plan(5)
    ue = S.UniPCMultistepScheduler().plan(5)
    for (t, row), (te, rowe) in zip(u, ue):
        assert t == te and row[:10] == rowe[:10] and rowe[10] == 0.0 and row[11] == 0.0
        assert row[10] == pytest.approx(1.0 / row[0], rel=1e-15) and row[10] ** 2 + row[1] ** 2 == pytest.approx(1.0, rel=1e-12)
    with pytest.raises(NotImplementedError):
        S.PNDMScheduler(prediction_type="v_prediction")
    for cls in (S.DDIMScheduler, S.UniPCMultistepScheduler):
        for bad in (dict(prediction_type="sample"), dict(thresholding=True), dict(prediction_type="v_prediction", thresholding=True)):
            with pytest.raises(NotImplementedError):
                cls(**bad)
    with pytest.raises(NotImplementedError):
        S.DDIMScheduler(prediction_type="v_prediction", clip_sample=True)


# ------------------------------------------------------------------ call form, settings, entrypoints
class _FakePipe:
    def __call__(self, **kw):
        self.kw = kw

        class _Out:
            images = ["image"]
        return _Out()


@pytest.mark.parametrize("base", ["sd_v1.5", "sd_v2.1"])
def test_pass_thorugh_pipe_text_to_image_kwargs(base):
    pipe, gen = _FakePipe(), torch.Generator()
    out = R.pass_thorugh_pipe(base, pipe, "a prompt", object(), 0, 0.85, 30, gen, 7.5, 0.75)
    assert out == "image"
    assert pipe.kw == {"prompt": "a prompt", "num_inference_steps": 30, "generator": gen, "guidance_scale": 7.5,
                       "negative_prompt": R.NEGATIVE_PROMPT}
    assert not {"image", "strength", "controlnet_conditioning_scale", "control_image"} & set(pipe.kw)
    R.pass_thorugh_pipe(base, pipe, "p", "src", 1, 0.5, 30, gen, 7.5, 0.75)                   # SDEdit without a control image
    assert pipe.kw["image"] == "src" and pipe.kw["strength"] == 0.5 and "control_image" not in pipe.kw


def test_other_call_forms_keep_their_rules():
    pipe, gen = _FakePipe(), torch.Generator()
    for base in ("blip_diffusion", "sd_xl-turbo", "blip_diffusion-edit"):
        with pytest.raises(NotImplementedError):
            R.pass_thorugh_pipe(base, pipe, "p", "src", 0, 0.85, 30, gen, 7.5, 0.75)
    with pytest.raises(NotImplementedError):
        R.pass_thorugh_pipe("ip2p", pipe, "p", "src", 1, 0.85, 30, gen, 7.5, 0.75)


def test_settings_and_entrypoints_carry_the_switch():
    s = R.Settings(BASE_MODEL="sd_v2.1", CONTROLNET=None, SDEDIT=0)
    assert "/aug_data/regular/sd_v2.1/None/" in R.output_folder_for(s, "/data")
    s.SDEDIT = 1
    assert f"/aug_data/regular/sd_v2.1-SDEdit_strength_{s.SDEDIT_STRENGTH}/None/" in R.output_folder_for(s, "/data")
    assert "sd_v2.1" in R.BASE_MODEL_DICT
    src = open(os.path.join(ROOT, "run_aug", "run_aug.py")).read()
    assert "SASPA_BASE_MODEL" in src and "SASPA_CONTROLNET" in src and "SASPA_SDEDIT" in src and "sd_v2.1" in src
    import importlib.util
    spec = importlib.util.spec_from_file_location("_rg_entry", os.path.join(ROOT, "run_aug", "run_aug_real_guidance.py"))
    rg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rg)
    s = rg.real_guidance_settings({"SASPA_BASE_MODEL": "sd_v2.1"})
    assert (s.BASE_MODEL, s.CONTROLNET, s.SDEDIT) == ("sd_v2.1", None, 1)


# ------------------------------------------------------------------ weights
def test_sd21_weight_spec_follows_the_diffusers_layout():
    unet = {n: s for n, s, _ in W.unet_spec(CFG.SD21_UNET)}
    t = "down_blocks.0.attentions.0"
    assert unet[t + ".proj_in.weight"] == (320, 320) and unet[t + ".proj_out.weight"] == (320, 320)           # use_linear_projection
    assert unet[t + ".transformer_blocks.0.attn2.to_k.weight"] == (320, 1024)
    assert unet["mid_block.attentions.0.transformer_blocks.0.attn2.to_v.weight"] == (1280, 1024)
    assert unet["up_blocks.3.attentions.2.transformer_blocks.0.ff.net.0.proj.weight"] == (2560, 320)
    assert not any(".transformer_blocks.1." in k for k in unet) and not any(k.startswith("down_blocks.3.attentions") for k in unet)
    assert "add_embedding.linear_1.weight" not in unet and unet["conv_in.weight"] == (320, 4, 3, 3)
    text = {n: s for n, s, _ in W.clip_text_spec(CFG.OPENCLIP_H)}
    assert text["text_model.encoder.layers.22.mlp.fc1.weight"] == (4096, 1024) and "text_model.encoder.layers.23.mlp.fc1.weight" not in text
    assert "text_projection.weight" not in text and text["text_model.embeddings.position_embedding.weight"] == (77, 1024)
    n_unet = sum(math.prod(s) for s in unet.values())
    n_text = sum(math.prod(s) for s in text.values())
    n_vae = sum(math.prod(s) for _, s, _ in W.vae_decoder_spec(CFG.SD21["vae"])) + sum(math.prod(s) for _, s, _ in W.vae_encoder_spec(CFG.SD21["vae"]))
    print(f"SD-2.1 parameters: unet {n_unet:,}  text encoder {n_text:,}  vae {n_vae:,}")
    # RECALLED public figures (the parameter counts diffusers reports for stabilityai/stable-diffusion-2-1-base): the UNet's 865.9 M
    # and the 23-layer OpenCLIP-H text encoder's 340.4 M.  The VAE is SD-1.5's; its count is unpinned here.
    assert n_unet == 865_910_724
    assert n_text == 340_387_840
    # heads: the count per level, 64 channels each
    assert [c // h for c, h in zip(CFG.SD21_UNET["block_out"], CFG.SD21_UNET["heads"])] == [64, 64, 64, 64]
    tiny = CFG.tiny_sd21()["unet"]
    assert [c // h for c, h in zip(tiny["block_out"], tiny["heads"])] == [16, 16, 16, 16] and tiny["linear_proj"]
    assert tiny["ctx_dim"] not in tiny["block_out"] and CFG.tiny_sd21()["text"]["pad_id"] == 0 and CFG.tiny_sd21()["text"]["act"] == "gelu"


def test_gelu_text_tower_matches_transformers():
    """The check tests/test_oracle.py makes for CLIP-L, for the SD-2.1 tower: GELU, pad id 0, last hidden state after the final LN."""
    tr = pytest.importorskip("transformers")
    cfg = CFG.tiny_sd21()["text"]
    hf_cfg = tr.CLIPTextConfig(vocab_size=cfg["vocab"], hidden_size=cfg["width"], intermediate_size=cfg["mlp"],
                               num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], max_position_embeddings=77,
                               hidden_act="gelu", layer_norm_eps=1e-5, bos_token_id=cfg["vocab"] - 2, eos_token_id=cfg["vocab"] - 1,
                               pad_token_id=0)
    model = tr.CLIPTextModel(hf_cfg).eval()
    sd = W.synth_state_dict("text", cfg, seed=4)
    hf_sd = sd
    if not any(k.startswith("text_model.") for k in model.state_dict()):      # transformers >= 5 dropped the prefix
        hf_sd = {k[len("text_model."):]: v for k, v in sd.items()}
    missing = model.load_state_dict(hf_sd, strict=False)
    assert not [k for k in missing.missing_keys if "position_ids" not in k], missing
    assert not missing.unexpected_keys
    ids = torch.from_numpy(np.random.RandomState(0).randint(1, cfg["vocab"] - 2, (2, 77)))
    ids[:, 0], ids[:, 20], ids[:, 21:] = cfg["vocab"] - 2, cfg["vocab"] - 1, 0                  # BOS ... EOS, then pad id 0
    with torch.no_grad():
        ref = model(input_ids=ids).last_hidden_state
        got = OM.clip_text_forward(sd, cfg, ids)
    assert (ref - got).abs().max().item() < 1e-4


# ------------------------------------------------------------------ dry plans at full width
_BUF = (C.c_char * 64)()
_BASE = (C.addressof(_BUF) + 15) // 16 * 16          # never dereferenced: the dry plans read shapes and flags only


def _conv_plan(lib, b, hin, win, cin, n, k, stride=1, upsample=0):
    p = _lib.GemmParams()
    p.a0 = p.w = p.out = _BASE
    ho, wo = (hin * 2, win * 2) if upsample else (hin // stride, win // stride)
    p.dtype, p.batch, p.hin, p.win, p.hout, p.wout = _lib.SASPA_BF16, b, hin, win, ho, wo
    p.kh = p.kw = k
    p.stride, p.pad, p.upsample = stride, k // 2, upsample
    p.c0 = p.lda0 = ops.round8(cin)
    p.K = p.ldw = k * k * ops.round8(cin)
    p.N, p.ldo = n, ops.round8(n)
    p.M, p.nb1, p.nb2, p.alpha = b * ho * wo, 1, 1, 1.0
    return lib.saspa_gemm_which(C.byref(p))


def _linear_plan(lib, m, k, n):
    p = _lib.GemmParams()
    p.a0 = p.w = p.out = _BASE
    p.dtype, p.M, p.N, p.K, p.batch = _lib.SASPA_BF16, m, n, k, 1
    p.kh = p.kw = p.stride = 1
    p.c0 = p.lda0 = p.ldw = k
    p.ldo, p.hin, p.hout, p.win, p.wout, p.nb1, p.nb2, p.alpha = n, m, m, 1, 1, 1, 1, 1.0
    return lib.saspa_gemm_which(C.byref(p))


def _level_of(name, n_lvl):
    """(level the layer's INPUT lives at, stride, upsample) from its diffusers key."""
    m = re.match(r"(down|up)_blocks\.(\d+)\.(\w+)", name)
    if m is None:
        return (n_lvl - 1, 1, 0) if name.startswith("mid_block") else (0, 1, 0)                 # conv_in / conv_out: level 0
    i = int(m.group(2))
    lvl = i if m.group(1) == "down" else n_lvl - 1 - i
    return lvl, 2 if m.group(3) == "downsamplers" else 1, 1 if m.group(3) == "upsamplers" else 0


@pytest.mark.parametrize("latent", [64, 96])
@pytest.mark.parametrize("batch", [8, 16])
def test_every_gemm_of_the_full_width_unet_has_a_plan(latent, batch):
    """saspa_gemm_which (saspa_gemm's own validation and dispatch, nothing launched) on every conv and linear layer of SD21_UNET at
    64 x 64 and 96 x 96 latents, batch 8 and 16 (the CFG pair included in the batch), bf16.  A skip concat is described as ONE source
    of the summed channel count; linear layers over tokens have M = batch x pixels, those over the text context M = batch x 77, the
    time-embedding ones M = batch."""
    lib = _lib.load()
    cfg = CFG.SD21_UNET
    n_lvl = len(cfg["block_out"])
    seen = set()
    for name, shape, kind in W.unet_spec(cfg):
        if kind != "w":
            continue
        lvl, stride, up = _level_of(name, n_lvl)
        side = latent >> lvl
        if len(shape) == 4:
            w = _conv_plan(lib, batch, side, side, shape[1], shape[0], shape[2], stride, up)
        elif ".attn2.to_k" in name or ".attn2.to_v" in name:
            w = _linear_plan(lib, batch * 77, shape[1], shape[0])
        elif "time_emb" in name:
            w = _linear_plan(lib, batch, shape[1], shape[0])
        else:
            w = _linear_plan(lib, batch * side * side, shape[1], shape[0])
        assert w > 0, (name, shape, side, w)
        seen.add(w & 0xff)
    assert seen <= {1, 2, 3, 4} and len(seen) > 1, seen                                       # real kernel families, more than one


def _attn_which(bsz, heads, d, nq, nk, rowmajor):
    c = heads * d
    q, k, out = (torch.empty(bsz, n, c, dtype=torch.bfloat16) for n in (nq, nk, nq))
    v = torch.empty(bsz, nk, c, dtype=torch.bfloat16) if rowmajor else torch.empty(bsz, c, ops.round8(nk) + 8, dtype=torch.bfloat16)
    return ops.flash_attn_which(q, k, v, out, heads, d, nq, nk, False, True, rowmajor)


def test_level0_attention_of_sd21_has_a_plan(monkeypatch):
    for name in ("SASPA_ATTN_MODE", "SASPA_ATTN_V4", "SASPA_ATTN_RING"):
        monkeypatch.delenv(name, raising=False)
    heads, d = CFG.SD21_UNET["heads"][0], CFG.SD21_UNET["block_out"][0] // CFG.SD21_UNET["heads"][0]
    assert (heads, d) == (5, 64)
    for n in (64 * 64, 96 * 96):
        assert _attn_which(2, heads, d, n, n, True) > 0, n             # self-attention: V row-major, as the fused Q|K|V launch leaves it
        assert _attn_which(2, heads, d, n, 77, False) > 0, n           # cross-attention over the 77 text keys: V^T
    for lvl in (1, 2):                                                 # the deeper levels: 10 / 20 heads of 64
        heads = CFG.SD21_UNET["heads"][lvl]
        n = (64 >> lvl) ** 2
        assert _attn_which(2, heads, 64, n, n, True) > 0 and _attn_which(2, heads, 64, n, 77, False) > 0


# ------------------------------------------------------------------ step references
def test_v_step_reference_equals_the_published_formulas():
    g = torch.Generator().manual_seed(7)
    for a_t, a_p, gs in ((0.3, 0.45, 7.5), (0.0047, 0.0120, 7.5), (0.9, 0.9991, 1.0), (0.5, 0.6, 0.0)):
        inp = dict(eps=torch.randn(4, 50, 4, generator=g, dtype=torch.float64), x=torch.randn(2, 50, 4, generator=g, dtype=torch.float64),
                   state=torch.randn(3, 2, 50, 4, generator=g, dtype=torch.float64), nimg=2, hw=50)
        ref, _ = REF.vddim_ref(inp, a_t, a_p, gs)
        sa_t, s1m_t, sa_p, s1m_p = (float(v) for v in REF._coef(a_t, a_p, torch.float32))      # the constants as the kernels get them
        want = REF.transcription_ddim(inp["eps"][:2], inp["eps"][2:], inp["x"], sa_t ** 2, sa_p ** 2, gs)
        # (1 - sa^2) ** 0.5 against the fp32-rounded sqrt(1 - a): the two differ by the rounding of the constants, ~1e-7 relative
        assert torch.allclose(ref, want, rtol=0, atol=4e-6 * (1 + gs)), (ref - want).abs().max()
        exact = dict(inp)
        want2 = sa_p * (sa_t * inp["x"] - s1m_t * (inp["eps"][:2] + gs * (inp["eps"][2:] - inp["eps"][:2]))) + \
            s1m_p * (sa_t * (inp["eps"][:2] + gs * (inp["eps"][2:] - inp["eps"][:2])) + s1m_t * inp["x"])
        assert torch.equal(ref, want2)
        row = REF.vunipc_row()
        u = REF.vunipc_ref(exact, row, gs)
        r = [float(torch.tensor(v, dtype=torch.float32)) for v in row]
        assert torch.equal(u["m0"][0], REF.transcription_unipc_x0(inp["eps"][:2], inp["eps"][2:], inp["x"], r[10], r[1], gs))
        # the unchanged multistep update: sampler_ref's epsilon reference on the eps this v is equivalent to gives the same step
        a, s = r[10], r[1]
        v = inp["eps"][:2] + gs * (inp["eps"][2:] - inp["eps"][:2])
        as_eps = dict(inp, eps=a * v + s * inp["x"])
        e = REF.SR.unipc_ref(as_eps, [1.0 / a] + row[1:], None)
        slack = abs(a * a + s * s - 1.0) + 1e-12                                          # the fp32 rounding of alpha_t and sigma_t
        for nm in ("x", "last", "m0"):
            assert torch.allclose(u[nm][0], e[nm][0], rtol=0, atol=100 * slack * (1 + gs) + 1e-9), nm


def _vpred_measured(storage):
    res = []
    for shift in TE.SEEDS:
        TE._SEED_SHIFT[0] = shift
        try:
            cases = REF.vpred_cases(TE._rand, storage)
        finally:
            TE._SEED_SHIFT[0] = 0
        for name, got, ref, s, legit, key in cases:
            st = budget_stats(got, ref, s, REF.UNITS[storage])
            res.append((f"{name} [seeds +{1000 * shift}]", legit, key, st, ratio(st, REF.VPRED_LIMITS[storage]), (got, ref, s)))
    return res


def vpred_table():
    """The measured table (profiles/vpred_errbudget.txt): per storage type the worst legitimate ratio and every mutant's weakest."""
    lines = ["v-prediction sampler steps: error statistics against the float64 reference, in units of half an ulp of the storage type",
             "(tests/sd21_ref.py; |stat| / allowance over the seed shifts of tests/test_errbudget.SEEDS; legit <= 0.5, mutants >= 2.0)", ""]
    for storage in REF.DTYPES:
        rows = _vpred_measured(storage)
        lines.append(f"== {storage}: limits {REF.VPRED_LIMITS[storage]}")
        worst = {}
        for name, legit, key, st, r, _ in rows:
            base = name.split(" [seeds")[0]
            if base not in worst or (r > worst[base][0]) == legit:
                worst[base] = (r, st, legit, key)
        for base, (r, st, legit, key) in sorted(worst.items(), key=lambda t: (not t[1][2], t[0])):
            note = "  NOT SEPARABLE (not asserted)" if (storage, key) in REF.NOT_SEPARABLE else ""
            lines.append(f"{'legit ' if legit else 'mutant'} ratio {r:10.3f}  {base}: {fmt(st)}{note}")
        lines.append("")
    lines += ["NOT SEPARABLE under 16-bit storage: a second rounding of x0 to the storage type.  The stored output is rounded to the same",
              "width, which costs up to one unit by itself; the rounded x0 adds at most sa_p (or |r6|, |r8|) of a unit of x0's magnitude",
              "to it, an rms of 0.2 .. 0.4 units against 0.07 .. 0.35 of the right kernel -- inside every limit that grants the right kernel",
              "its 2x margin.  Under fp32 storage the same slip (x0 through 16 bits) stands 1e4 units out and is asserted."]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("storage", list(REF.DTYPES))
def test_v_step_limits_hold_both_margins(storage):
    rows = _vpred_measured(storage)
    legit = [r for r in rows if r[1]]
    mutants = [r for r in rows if not r[1] and (storage, r[2]) not in REF.NOT_SEPARABLE]
    assert legit and mutants and {r[2] for r in mutants} >= set(REF.DDIM_MUTANTS) - {"x0_rounded"}
    for name, _, _, st, r, (got, ref, s) in legit:
        print(f"{storage} {r:8.3f}  {name}: {fmt(st)}")
        check_budget(got, ref, s, REF.UNITS[storage], limits=REF.VPRED_LIMITS[storage], what=name)
    for name, _, _, st, r, (got, ref, s) in mutants:
        print(f"{storage} {r:8.2f}  {name}: {fmt(st)}")
        with pytest.raises(AssertionError, match="error budget exceeded"):
            check_budget(got, ref, s, REF.UNITS[storage], limits=REF.VPRED_LIMITS[storage], what=name)
    worst, weakest = max(legit, key=lambda t: t[4]), min(mutants, key=lambda t: t[4])
    assert worst[4] <= TE.LEGIT_MAX, f"{storage}: limit less than 2x above legit '{worst[0]}': {fmt(worst[3])}"
    assert weakest[4] >= TE.MUTANT_MIN, f"{storage}: limit less than 2x below mutant '{weakest[0]}': {fmt(weakest[3])}"
    if storage == "fp32":
        assert any(r[2] == "x0_rounded" for r in mutants)                                  # asserted where it is separable


def test_committed_table_lists_the_measured_cases():
    """The table is printed here and committed as profiles/vpred_errbudget.txt (PYTHONPATH=. python tests/test_sd21_host.py
    --write-table).  The last digits of the statistics follow the host's summation order, so the committed copy is compared by its
    rows (case names, limits, what is not separable), not by its digits."""
    table = vpred_table()
    print(table)

    def rows(text):
        return [re.sub(r"ratio\s+\S+", "ratio", ln.split(": max")[0]) for ln in text.splitlines()]
    with open(os.path.join(ROOT, "profiles", "vpred_errbudget.txt")) as f:
        assert rows(f.read()) == rows(table), "profiles/vpred_errbudget.txt is stale"


# ------------------------------------------------------------------ symbols
def test_both_libraries_export_the_v_steps():
    lib, f16 = _lib.load(), _lib.load_f16()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "saspa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(saspa_[a-z0-9_]+)\s*\(", src))
    for name in V_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and name in _lib.F16_SYMBOL_NAMES, name
        assert hasattr(lib, name) and hasattr(f16, name), name
        eps_name = name.replace("_v_dev", "_dev") if name.endswith("_v_dev") else name[:-2]
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[eps_name], name                           # the epsilon entry point's signature
    assert declared == set(_lib.SYMBOLS)
    assert lib.saspa_abi_version() == f16.saspa_abi_version() == 20


def test_v_steps_validate_like_the_epsilon_steps():
    """Host-side refusals, nothing launched: the v entry points answer every bad argument with the code of the epsilon entry point."""
    buf = (C.c_char * 4096)()
    ptr = (C.addressof(buf) + 15) // 16 * 16
    row = (C.c_float * 12)(*([1.0] * 12))
    for L, ok, bad in ((_lib.load(), (_lib.SASPA_BF16, _lib.SASPA_F32), (_lib.SASPA_F16, _lib.SASPA_F32X3, 7)),
                       (_lib.load_f16(), (_lib.SASPA_F16,), (_lib.SASPA_BF16, _lib.SASPA_F32, 7))):
        def ddim(fn, dt, v=ptr, x=ptr, nimg=1, hw=4, c=4, ldc=8, sa=0.5):
            return fn(dt, v, x, nimg, hw, c, ldc, 7.5, sa, 0.5, 0.5, 0.5, None)

        def ddim_nocfg(fn, dt, v=ptr, x=ptr, nimg=1, hw=4, c=4, ldc=8, sa=0.5):
            return fn(dt, v, x, nimg, hw, c, ldc, sa, 0.5, 0.5, 0.5, None)

        def dev(fn, dt, v=ptr, x=ptr, nimg=1, hw=4, c=4, ldc=8, coefs=ptr, index=ptr):
            return fn(dt, v, x, nimg, hw, c, ldc, 1, 7.5, coefs, index, None)

        def unipc(fn, dt, v=ptr, x=ptr, state=ptr, nimg=1, hw=4, c=4, ldc=8, r=row):
            return fn(dt, v, x, state, nimg, hw, c, ldc, 7.5, r, None, None, None)

        def unipc_nocfg(fn, dt, v=ptr, x=ptr, state=ptr, nimg=1, hw=4, c=4, ldc=8, r=row):
            return fn(dt, v, x, state, nimg, hw, c, ldc, r, None, None, None)
        pairs = [(ddim, L.saspa_cfg_ddim_step, L.saspa_cfg_ddim_step_v), (ddim_nocfg, L.saspa_ddim_step, L.saspa_ddim_step_v),
                 (dev, L.saspa_ddim_step_dev, L.saspa_ddim_step_v_dev), (unipc, L.saspa_cfg_unipc_step, L.saspa_cfg_unipc_step_v),
                 (unipc_nocfg, L.saspa_unipc_step, L.saspa_unipc_step_v)]
        for call, eps_fn, v_fn in pairs:
            refusals = [dict(v=None), dict(x=None), dict(nimg=0), dict(hw=0), dict(c=0), dict(c=9), dict(ldc=4), dict(v=ptr + 2),
                        dict(x=ptr + 8)]
            if call in (ddim, ddim_nocfg):
                refusals += [dict(sa=0.0), dict(sa=-1.0)]
            if call is dev:
                refusals += [dict(coefs=None), dict(index=None)]
            if call in (unipc, unipc_nocfg):
                refusals += [dict(state=None), dict(state=ptr + 4), dict(r=None)]
            for kw in refusals:
                want = call(eps_fn, ok[0], **kw)
                assert want < 0 and call(v_fn, ok[0], **kw) == want, (v_fn.__name__, kw, want)
            assert call(v_fn, ok[0], ldc=4) == _lib.SASPA_ERANGE                              # a pixel of half a vector: refused
            for dt in bad:                                                                    # a dtype code this library does not serve
                assert call(v_fn, dt) == call(eps_fn, dt) == _lib.SASPA_EINVAL, (v_fn.__name__, dt)


def test_ops_refuse_mixed_element_types():
    """ops' own checks run before the library is asked (CPU tensors are refused first, so the dtype check is called directly)."""
    x, v = torch.zeros(2, 16, 8, dtype=torch.bfloat16), torch.zeros(2, 16, 8, dtype=torch.float16)
    with pytest.raises(ValueError, match="v is torch.float16"):
        ops._vstep_shapes("cfg_ddim_step_v", v, x, 1, 16, 2)
    with pytest.raises(ValueError, match=r"contiguous \[2 \* nimg, hw, 8\]"):
        ops._vstep_shapes("cfg_ddim_step_v", x[:1], x, 1, 16, 2)
    with pytest.raises(ValueError, match="state"):
        ops._vstep_shapes("cfg_unipc_step_v", x, x, 1, 16, 2, torch.zeros(2, 1, 16, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cfg_ddim_step_v(x, x, 1, 16, 4, 7.5, 0.5, 0.5, 0.5, 0.5)


if __name__ == "__main__":
    import sys
    if "--write-table" in sys.argv:
        with open(os.path.join(ROOT, "profiles", "vpred_errbudget.txt"), "w") as f:
            f.write(vpred_table())
