"""The ControlNet-free text-to-image pipeline (sd_v1.5, sd_v2.1) and the SD-2.1 family on the device: fp32 parity with the oracle
composition of tests/sd21_ref.py (DDIM, UniPC, a v-prediction scheduler; img2img on SD21), the 16-bit compute types against the
existing ControlNet-free img2img pipeline as the yardstick, the captured step against the Python loop, the shared CFG prefix, one
full-width evaluation of the SD-2.1 UNet, and `run_aug.main` with BASE_MODEL = "sd_v2.1", CONTROLNET = None.

Images are 64 x 128: the four-level UNets halve the latent three times, so the sides are multiples of 64, and 64 x 128 is the smallest
size that is not square."""
import json
import logging
import os
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from oracle import sd_models as OM
from saspa_aug_amd import config as CFG
from saspa_aug_amd import filters, models
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import scheduler as S
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionImg2ImgPipeline, StableDiffusionPipeline
from saspa_aug_amd.synthetic import synthetic_image
from saspa_aug_amd.tokenizer import HashTokenizer
from tests import sd21_ref as REF
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
HH, WW, STEPS = 64, 128, 4
_PARITY = []                            # lines of profiles/sd21_parity.txt (written where SD21_PARITY_OUT names a file)


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    path = os.environ.get("SD21_PARITY_OUT")
    if path and _PARITY:
        with open(path, "w") as f:
            f.write("tests/test_sd21_gpu.py on an MI355X: distance of the decoded image to the fp32 oracle (per pixel, [0, 1] scale), reduced-width\n"
                    "families, 64 x 128, 4 evaluations, 2 images; then the full-width UNet evaluation\n" + "\n".join(_PARITY) + "\n")


@pytest.fixture(scope="module")
def fams():
    t15 = CFG.tiny()
    t21 = CFG.tiny_sd21()
    return {"tiny": (t15, W.synth_family(t15, seed=3)), "tiny_sd21": (t21, W.synth_family(t21, seed=3))}


def _inputs(cfgs, nimg, seed=1):
    v = cfgs["text"]["vocab"]
    ids = torch.from_numpy(np.random.RandomState(seed).randint(1, v - 2, (nimg, 77)))
    neg = torch.from_numpy(np.random.RandomState(seed + 1).randint(1, v - 2, (1, 77)))
    g = torch.manual_seed(seed)
    lat = torch.cat([torch.randn((1, 4, HH // 8, WW // 8), generator=g) for _ in range(nimg)])
    return ids, neg, lat


def _sched(sampler, prediction_type):
    cls = S.DDIMScheduler if sampler == "ddim" else S.UniPCMultistepScheduler
    return cls(prediction_type=prediction_type)


_REFS = {}


def _txt2img_ref(name, fams, nimg, sampler, prediction_type):
    """The oracle run of a case, computed once and shared by the tests (and dtypes) that need it."""
    key = (name, nimg, sampler, prediction_type)
    if key not in _REFS:
        cfgs, fam = fams[name]
        ids, neg, lat = _inputs(cfgs, nimg)
        _REFS[key] = REF.txt2img(fam, cfgs, ids, neg, lat, STEPS, sampler=sampler, prediction_type=prediction_type)
    return _REFS[key]


def _dist(img, ref_img):
    """(max, rms) per-pixel distance of two decoded images on the [0, 1] scale."""
    d = (from_nhwc(img, 3) / 2 + 0.5).clamp(0, 1) - (ref_img / 2 + 0.5).clamp(0, 1)
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _place(pipe, dev, compute):
    """compute: "fp32" | "bf16" | "fp16" (enable_fp16, x3 VAE: the decoded image's parity is the point)."""
    if compute == "fp16":
        pipe.enable_fp16(True, vae="x3")
    return pipe.to(dev, torch.float32 if compute == "fp32" else torch.float16)


def _txt2img(fams, name, dev, compute, nimg, sampler="ddim", prediction_type="epsilon"):
    cfgs, fam = fams[name]
    ids, neg, lat = _inputs(cfgs, nimg)
    pipe = _place(StableDiffusionPipeline(fam, cfgs, scheduler=_sched(sampler, prediction_type)), dev, compute)
    assert pipe.controlnet is None and (pipe.safety_checker is not None) == ("safety" in cfgs)
    out, x, img = pipe.generate_batch(ids.numpy(), neg.numpy(), lat, STEPS, return_latents=True)
    ref_u8, _, ref_img = _txt2img_ref(name, fams, nimg, sampler, prediction_type)
    du8 = int(np.abs(out.cpu().numpy().astype(int) - ref_u8.astype(int)).max())
    return _dist(img, ref_img) + (du8,)


# ------------------------------------------------------------------ fp32 parity
@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
@pytest.mark.parametrize("name", ["tiny", "tiny_sd21"])
def test_text_to_image_fp32_parity(dev, fams, name, sampler, nimg):
    dmax, drms, du8 = _txt2img(fams, name, dev, "fp32", nimg, sampler)
    print(f"\ntext-to-image {name} {sampler} x{nimg} fp32: max |d| {dmax:.2e} rms {drms:.2e} u8 {du8}")
    assert dmax < 1e-3 and du8 <= 1, (dmax, du8)


@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
def test_text_to_image_v_prediction_fp32_parity(dev, fams, sampler, nimg):
    dmax, drms, du8 = _txt2img(fams, "tiny_sd21", dev, "fp32", nimg, sampler, "v_prediction")
    print(f"\ntext-to-image tiny_sd21 {sampler} v_prediction x{nimg} fp32: max |d| {dmax:.2e} rms {drms:.2e} u8 {du8}")
    assert dmax < 1e-3 and du8 <= 1, (dmax, du8)
    # and the v-prediction run is not the epsilon run: the same weights read as epsilon give another image
    ref_v, ref_e = (_txt2img_ref("tiny_sd21", fams, nimg, sampler, p)[2] for p in ("v_prediction", "epsilon"))
    assert (ref_v - ref_e).abs().max() > 1e-2


def _img2img_inputs(cfgs, nimg, seed=1):
    ids, neg, _ = _inputs(cfgs, nimg, seed)
    srcs = np.stack([synthetic_image(HH, WW, 30 + i) for i in range(nimg)])
    g = torch.manual_seed(seed)
    e = [torch.randn((1, 4, HH // 8, WW // 8), generator=g) for _ in range(2 * nimg)]
    return ids, neg, srcs, torch.cat(e[0::2]), torch.cat(e[1::2])


def _img2img(fams, name, dev, compute, nimg=2, prediction_type="epsilon"):
    """strength 0.5 of 2 * STEPS steps: STEPS evaluations, as the text-to-image cases."""
    cfgs, fam = fams[name]
    cfgs = {k: v for k, v in cfgs.items() if k != "safety"}
    ids, neg, srcs, e1, e2 = _img2img_inputs(cfgs, nimg)
    key = ("img2img", name, nimg, prediction_type)
    if key not in _REFS:
        _REFS[key] = REF.img2img(fam, cfgs, ids, neg, srcs, e1, e2, 2 * STEPS, 0.5, prediction_type=prediction_type)
    ref_u8, _, ref_img = _REFS[key]
    pipe = _place(StableDiffusionImg2ImgPipeline(fam, cfgs, scheduler=_sched("ddim", prediction_type)), dev, compute)
    out, x, img = pipe.generate_batch_img2img(ids.numpy(), neg.numpy(), srcs, e1, e2, 2 * STEPS, 0.5, return_latents=True)
    du8 = int(np.abs(out.cpu().numpy().astype(int) - ref_u8.astype(int)).max())
    return _dist(img, ref_img) + (du8,)


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
def test_img2img_on_sd21_fp32_parity(dev, fams, prediction_type):
    cfgs, fam = fams["tiny_sd21"]
    pipe = R.init_pipeline("sd_v2.1", None, 1, cfgs=cfgs, state_dicts=fam)
    assert type(pipe) is StableDiffusionImg2ImgPipeline and pipe.safety_checker is None
    dmax, drms, du8 = _img2img(fams, "tiny_sd21", dev, "fp32", 2, prediction_type)
    print(f"\nimg2img tiny_sd21 {prediction_type} fp32: max |d| {dmax:.2e} rms {drms:.2e} u8 {du8}")
    assert dmax < 1e-3 and du8 <= 1, (dmax, du8)


# ------------------------------------------------------------------ bf16 / fp16 against the existing img2img pipeline
def test_16bit_compute_against_the_img2img_yardstick(dev, fams):
    """The distance (rms per pixel of the decoded image on [0, 1]; the maximum is printed beside it) of each new form to its oracle, in
    bf16 and in fp16 compute, may be at most 2x the distance the existing StableDiffusionImg2ImgPipeline on tiny() keeps to ITS oracle
    at the same size and number of evaluations -- measured here, in the same process.  The factor allows for the other text tower and
    head geometry on draws this small.  fp16 must be closer to the oracle than bf16."""
    res = {}
    for compute in ("bf16", "fp16"):
        yard = _img2img(fams, "tiny", dev, compute)
        new = {"text-to-image tiny": _txt2img(fams, "tiny", dev, compute, 2),
               "text-to-image tiny_sd21": _txt2img(fams, "tiny_sd21", dev, compute, 2),
               "text-to-image tiny_sd21 v_prediction": _txt2img(fams, "tiny_sd21", dev, compute, 2, "ddim", "v_prediction"),
               "img2img tiny_sd21": _img2img(fams, "tiny_sd21", dev, compute)}
        res[compute] = (yard, new)
        line = f"{compute}: yardstick img2img tiny() rms {yard[1]:.3e} max {yard[0]:.3e}"
        print("\n" + line)
        _PARITY.append(line)
        for k, (dmax, drms, du8) in new.items():
            line = f"{compute}: {k} rms {drms:.3e} max {dmax:.3e} ({drms / yard[1]:.2f}x the yardstick's rms)"
            print(line)
            _PARITY.append(line)
    for compute, (yard, new) in res.items():
        for k, (dmax, drms, du8) in new.items():
            assert drms <= 2.0 * yard[1], (compute, k, drms, yard[1])
    for k in res["bf16"][1]:
        assert res["fp16"][1][k][1] < res["bf16"][1][k][1], (k, res["fp16"][1][k], res["bf16"][1][k])


# ------------------------------------------------------------------ the captured step, the shared CFG prefix
@pytest.mark.parametrize("name,prediction_type", [("tiny", "epsilon"), ("tiny_sd21", "epsilon"), ("tiny_sd21", "v_prediction")])
def test_graph_replay_equals_the_python_loop(dev, fams, monkeypatch, name, prediction_type):
    cfgs, fam = fams[name]
    ids, neg, lat = _inputs(cfgs, 2)
    for sampler in ("ddim", "unipc"):
        pipe = StableDiffusionPipeline(fam, cfgs, scheduler=_sched(sampler, prediction_type)).to(dev, torch.float16)
        out = {}
        for graph in ("0", None):
            monkeypatch.setenv("SASPA_GRAPH", graph) if graph else monkeypatch.delenv("SASPA_GRAPH", raising=False)
            img, x, _ = pipe.generate_batch(ids.numpy(), neg.numpy(), lat, STEPS, return_latents=True)
            out[graph] = (img.clone(), x.clone())
        assert len(pipe._graphs) == 1 and all(len(g.nets) == 1 for g in pipe._graphs.values())     # ONE branch: the UNet alone
        assert torch.equal(out["0"][1], out[None][1]) and torch.equal(out["0"][0], out[None][0]), (name, sampler)


@pytest.mark.parametrize("name", ["tiny", "tiny_sd21"])
def test_cfg_prefix_on_vs_off(dev, fams, monkeypatch, name):
    """SASPA_CFG_PREFIX=0 against the default, the tolerance of tests/test_cfg_prefix_gpu.py: u8 images within one level."""
    cfgs, fam = fams[name]
    ids, neg, lat = _inputs(cfgs, 2)
    for dtype in (torch.bfloat16, torch.float32):
        pipe = StableDiffusionPipeline(fam, cfgs).to(dev, dtype)
        out = {}
        for knob in ("0", None):
            monkeypatch.setenv("SASPA_CFG_PREFIX", knob) if knob else monkeypatch.delenv("SASPA_CFG_PREFIX", raising=False)
            out[knob] = pipe.generate_batch(ids.numpy(), neg.numpy(), lat, 2).cpu().numpy().astype(int)
        assert sorted(g.cfg_pair for g in pipe._graphs.values()) == [False, True]
        du8 = np.abs(out["0"] - out[None]).max()
        print(f"\nSASPA_CFG_PREFIX off vs default, {name} {dtype}: u8 images differ by {du8}")
        assert du8 <= 1, du8


# ------------------------------------------------------------------ one full-width evaluation
def _rms_rel(got, ref):
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def test_full_width_sd21_unet_evaluation(dev):
    """SD21_UNET in bf16 at 32 x 32 latents, batch 2, a 77 x 1024 context, against oracle.sd_models.unet_forward: 64-wide heads through
    the 320-channel level's fused Q|K|V, feed-forward and LayerNorm launches at real width.  Yardstick, in the same test: SD15_UNET at
    the same size without residuals.  SD-2.1's rms-relative error may be at most 1.5x SD-1.5's."""
    errs = {}
    for tag, cfg in (("sd_v1.5", CFG.SD15_UNET), ("sd_v2.1", CFG.SD21_UNET)):
        sd = W.synth_state_dict("unet", cfg, seed=5)
        g = torch.Generator().manual_seed(11)
        x = torch.randn(2, 4, 32, 32, generator=g)
        ctx = torch.randn(2, 77, cfg["ctx_dim"], generator=g)
        ts = OP.DDIM().set_timesteps(4)
        ref = OM.unet_forward(sd, cfg, x, int(ts[1]), ctx)
        net = models.UNet(sd, cfg, dev, torch.bfloat16)
        del sd
        net.prepare_context(ctx.to(dev, torch.bfloat16))
        net.prepare_timesteps(ts)
        got = from_nhwc(net.forward(to_nhwc(x, torch.bfloat16, dev, cpad=8), 1), 4)
        assert torch.isfinite(got).all()
        errs[tag] = _rms_rel(got, ref)
        if tag == "sd_v2.1":
            assert net.tr_info["down_blocks.0.attentions.0"] == (5, 1) and net.tr_info["mid_block.attentions.0"] == (20, 1)
        del net
        torch.cuda.empty_cache()
    line = (f"full-width UNet, bf16, 32x32 latents, batch 2: rms-relative error sd_v1.5 {errs['sd_v1.5']:.3e}, sd_v2.1 {errs['sd_v2.1']:.3e} "
            f"({errs['sd_v2.1'] / errs['sd_v1.5']:.2f}x)")
    print("\n" + line)
    _PARITY.append(line)
    assert errs["sd_v2.1"] <= 1.5 * errs["sd_v1.5"], errs


# ------------------------------------------------------------------ the call form and run_aug.main
def test_call_form(dev, fams):
    cfgs, fam = fams["tiny_sd21"]
    pipe = R.init_pipeline("sd_v2.1", None, 0, cfgs=cfgs, state_dicts=fam).to("cuda:0", torch.float16)
    a = R.pass_thorugh_pipe("sd_v2.1", pipe, "an airplane", None, 0, 0.85, 3, torch.manual_seed(1), 7.5, 0.75)
    side = 8 * cfgs["unet"].get("sample_size", 64)
    assert a.size == (side, side)                                            # the UNet's sample size, as diffusers defaults it
    b = pipe(prompt="an airplane", height=HH, width=WW, num_inference_steps=3, generator=torch.manual_seed(1)).images[0]
    c = pipe(prompt="an airplane", height=HH, width=WW, num_inference_steps=3, generator=torch.manual_seed(1),
             negative_prompt="").images[0]
    assert b.size == (WW, HH) and np.array_equal(np.asarray(b), np.asarray(c))
    with pytest.raises(ValueError):
        pipe(prompt="x", height=72, width=64)
    with pytest.raises(ValueError):
        pipe(num_inference_steps=3)


def _settings(root, **kw):
    prompts = Path(root) / "prompts.txt"
    prompts.parent.mkdir(parents=True, exist_ok=True)
    prompts.write_text("".join(f"an airplane in scene {k}.\n" for k in range(6)))
    base = dict(DATASET="synthetic", BASE_MODEL="sd_v2.1", CONTROLNET=None, SDEDIT=0, RESOLUTION=64, NUM_INFERENCE_STEPS=3, NUM_PER_IMAGE=2,
                SEED=1, USE_ARTISTIC_PROMPTS=False, SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, PROMPTS_FILE=str(prompts),
                BATCH_SIZE=4, SDEDIT_STRENGTH=0.5,
                DATASET_KWARGS=dict(root_path=str(Path(root) / "ds" / "data"), n_images=4, sizes=((64, 64), (64, 128))))
    base.update(kw)
    return R.Settings(**base)


@pytest.mark.parametrize("sdedit", [0, 1])
def test_run_aug_main_sd21(dev, fams, tmp_path, sdedit):
    cfgs, fam = fams["tiny_sd21"]
    pipe = R.init_pipeline("sd_v2.1", None, sdedit, cfgs=cfgs, state_dicts=fam).to("cuda:0", torch.float16)
    s = _settings(tmp_path, SDEDIT=sdedit)
    res = R.main(s, pipe=pipe)
    out = Path(res["output_folder"])
    want = "/aug_data/regular/sd_v2.1-SDEdit_strength_0.5/None/" if sdedit else "/aug_data/regular/sd_v2.1/None/"
    assert want in str(out) and (res["status"] == 1).all() and len(res["items"]) == 8
    names = sorted(p.name for p in out.glob("*.png"))
    assert len([n for n in names if "_prompt_" in n]) == 8 and len([n for n in names if n.endswith("_source.png")]) == 4
    assert not any(n.endswith("_control.png") for n in names)
    body = json.load(open(res["json_path"]))
    assert len(body) == 4 and all(len(v) == 2 for v in body.values())
    assert set(body) == {Path(it.source_path).name for it in res["items"]}                               # keyed by the source image
    assert all(Path(p).exists() and "_source" not in p for v in body.values() for p in v)
    # item 0 of the batched run == the single call with the draws of the seed-1 stream, at the source's planned size
    it = res["items"][0]
    if sdedit:
        single = pipe(prompt=it.prompt, image=Image.open(it.source_path).convert("RGB"), strength=0.5, num_inference_steps=3,
                      generator=torch.manual_seed(1), guidance_scale=7.5, negative_prompt=R.NEGATIVE_PROMPT).images[0]
    else:
        single = pipe(prompt=it.prompt, height=it.height, width=it.width, num_inference_steps=3, generator=torch.manual_seed(1),
                      guidance_scale=7.5, negative_prompt=R.NEGATIVE_PROMPT).images[0]
    assert np.array_equal(np.asarray(single), np.array(Image.open(it.output_path)))
    # a second run finds every output on disk and generates nothing
    res2 = R.main(s, pipe=pipe)
    assert all(i.skip for i in res2["items"]) and (res2["status"] == 0).all()


def test_run_aug_main_sd21_filters(dev, fams, tmp_path, caplog):
    """The semantic + confidence filters on synthetic filter weights behind the text-to-image loop: the post-hoc stage, FILTER_INLINE and
    PNG_DEVICE give the same JSON body (the labels and the JSON keys come from the source image)."""
    cfgs, fam = fams["tiny_sd21"]
    pipe = R.init_pipeline("sd_v2.1", None, 0, cfgs=cfgs, state_dicts=fam).to("cuda:0", torch.float16)
    cf = CFG.tiny_filters(num_classes=6)
    tok = HashTokenizer(cf["clip_rn50"]["vocab"], pad_id=0)
    clip_sd, cal_sd = W.synth_state_dict("clip_rn50", cf["clip_rn50"], 31), W.synth_state_dict("cal", cf["cal"], 32)
    bodies = {}
    for tag, kw in (("posthoc", {}), ("inline", dict(FILTER_INLINE=True)), ("png_device", dict(PNG_DEVICE=True)),
                    ("inline_png_device", dict(FILTER_INLINE=True, PNG_DEVICE=True))):
        s = _settings(tmp_path / tag, SEMANTIC_FILTERING=1, MODEL_CONFIDENCE_BASED_FILTERING=1, **kw)
        s.DATASET_KWARGS = dict(root_path=str(tmp_path / tag / "ds" / "data"), n_images=4, sizes=((64, 64),))
        ds = R.dataset_utils.DS_UTILS_DICT[s.DATASET](**s.DATASET_KWARGS)
        sem = filters.SemanticFilter(clip_sd, cf["clip_rn50"], dev, ds.get_basic_prompt(), tok)
        conf = filters.ConfidenceFilter(cal_sd, cf["cal"], dev, top_k=3)
        with caplog.at_level(logging.INFO):
            res = R.main(s, ds_utils=ds, pipe=pipe, filter_models=(sem, conf))
        assert (res["status"] == 1).all() and "/aug_data/regular/sd_v2.1/None/" in res["output_folder"]
        name = Path(res["json_path"]).name
        assert "semantic_filtering" in name and "model_confidence_based_filtering_top_10_classes" in name
        body = json.load(open(res["json_path"]))
        assert len(body) == 4 and all(len(v) <= 2 for v in body.values())
        assert all(Path(p).exists() for v in body.values() for p in v)
        bodies[tag] = {Path(k).name: sorted(Path(p).name for p in v) for k, v in body.items()}
        assert not list(Path(res["output_folder"]).glob("*_control.png"))
    assert bodies["inline"] == bodies["posthoc"] and bodies["png_device"] == bodies["posthoc"]
    assert bodies["inline_png_device"] == bodies["posthoc"]
