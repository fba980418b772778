"""InstructPix2Pix (BASE_MODEL = "ip2p"; run_aug/run_aug.py:174-176, :252-255) on the GPU: the three-branch guidance + DDIM kernel
against its float64 reference (rounding-error budget, pass-through of the image-latent channels, the device-table form), the UNet
with 8 input channels, the whole pipeline against the oracle restatement tests/ip2p_ref.py (fp32 path, north-star bar; bf16 PSNR),
the captured step graph against the Python-launched loop, the reference's call form, the batched run_aug path, and one run at
production width."""
import pathlib

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from oracle import sd_models as OM
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionInstructPix2PixPipeline
from saspa_aug_amd.synthetic import synthetic_image
from tests import ip2p_ref as IR
from tests.errbudget import LIMITS, UNIT_BF16, check_budget, fmt, rejects
from tests.test_errbudget import _rand, q
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
COEF = dict(a_t=0.3, a_p=0.45, gs=7.5, igs=1.3)
GS, IGS = 7.5, 1.3


# ------------------------------------------------------------------ the kernel
def _coefs(a_t, a_p):
    return a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5


def _kernel_inputs(eps, xx, dtype):
    """[3n, hw, 4] / [n, hw, 4] operands -> the kernel's [3n, hw, 8] buffers: channels 4..7 carry a pattern (what the pipeline keeps
    there are the image latents), different in every group and in eps."""
    n3, hw = eps.shape[0], eps.shape[1]
    g = torch.Generator().manual_seed(77)
    e8 = torch.cat([eps.float(), torch.randn(n3, hw, 4, generator=g)], -1).to(dtype)
    x8 = torch.cat([torch.cat([xx, xx, xx]).float(), torch.randn(n3, hw, 4, generator=g) * 3 + 0.25], -1).to(dtype)
    return e8.contiguous(), x8.contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run(dev, eps, xx, dtype, igs=IGS, table=False):
    n, hw = xx.shape[0], xx.shape[1]
    e8, x8 = _kernel_inputs(eps, xx, dtype)
    xd, ed = x8.to(dev), e8.to(dev)
    c = _coefs(COEF["a_t"], COEF["a_p"])
    if table:           # row 2 of a three-row table; rows 0 and 1 would give another result
        tab = torch.tensor([_coefs(0.9, 0.95), _coefs(0.6, 0.7), c], dtype=torch.float32, device=dev)
        ops.cfg3_ddim_step_dev(ed, xd, n, hw, 4, GS, igs, tab, torch.tensor([2], dtype=torch.int32, device=dev))
    else:
        ops.cfg3_ddim_step(ed, xd, n, hw, 4, GS, igs, *c)
    got = xd.cpu()
    assert torch.equal(_bits(got[..., 4:]), _bits(x8[..., 4:])), "channels 4..7 must keep their bits in all three groups"
    assert torch.equal(ed.cpu(), e8), "eps is read only"
    assert torch.equal(got[:n, :, :4], got[n:2 * n, :, :4]) and torch.equal(got[:n, :, :4], got[2 * n:, :, :4])
    return got


# (nimg, hw): 2 x 300 pixels = three blocks with a tail; one image; one pixel per image; one pixel in all
SHAPES = [(2, 300), (1, 300), (2, 1), (1, 1)]


def _slice(eps, xx, n, hw):
    return torch.cat([eps[g * 2:g * 2 + n, :hw] for g in range(3)]), xx[:n, :hw]


@pytest.mark.parametrize("n,hw", SHAPES)
def test_cfg3_ddim_budget(dev, n, hw):
    eps, xx = _slice(q(_rand(6, 300, 4, seed=42)), q(_rand(2, 300, 4, seed=43)), n, hw)
    ref, s = IR.cfg3_ddim_ref(eps, xx, **COEF)
    got = _run(dev, eps, xx, BF)
    st = check_budget(got[:n, :, :4], ref, s, UNIT_BF16, limits=LIMITS["elem"], what=f"cfg3 + ddim {n}x{hw}")
    print(f"\n[budget] elem  cfg3 + ddim nimg {n} hw {hw}: {fmt(st)}")
    wrong = _run(dev, eps, xx, BF, igs=1.5)
    assert rejects(wrong[:n, :, :4], ref, s, UNIT_BF16, limits=LIMITS["elem"]), "image guidance 1.5 against 1.3 must fail the budget"
    assert torch.equal(_run(dev, eps, xx, BF, table=True), got), "the device-table form must be bit-equal to the immediate form"


@pytest.mark.parametrize("n,hw", SHAPES)
def test_cfg3_ddim_fp32_storage(dev, n, hw):
    """fp32 storage: fp32 arithmetic on fp32 operands, so the float64 reference is met to 1e-6 of the magnitude s of the terms that
    formed each output (a handful of fp32 roundings, 2^-24 each, of terms no larger than s)."""
    eps, xx = _slice(_rand(6, 300, 4, seed=42).double(), _rand(2, 300, 4, seed=43).double(), n, hw)
    ref, s = IR.cfg3_ddim_ref(eps, xx, **COEF)
    got = _run(dev, eps, xx, torch.float32)
    rel = ((got[:n, :, :4].double() - ref).abs() / s).max().item()
    print(f"\ncfg3 + ddim fp32 nimg {n} hw {hw}: max |err| / s = {rel:.2e}")
    assert rel < 1e-6, rel
    assert torch.equal(_run(dev, eps, xx, torch.float32, table=True), got)


def test_cfg3_ddim_wrapper_refuses_wrong_shapes(dev):
    x = torch.zeros(6, 16, 8, device=dev, dtype=BF)
    with pytest.raises(ValueError):
        ops.cfg3_ddim_step(x.clone(), x, 3, 16, 4, GS, IGS, 0.5, 0.5, 0.5, 0.5)            # 3 images need 9 rows
    with pytest.raises(ValueError):
        ops.cfg3_ddim_step(x.float(), x, 2, 16, 4, GS, IGS, 0.5, 0.5, 0.5, 0.5)            # mixed element types
    with pytest.raises(RuntimeError, match="SASPA_ERANGE"):
        ops.cfg3_ddim_step(x.clone(), x, 2, 16, 8, GS, IGS, 0.5, 0.5, 0.5, 0.5)            # C > 4: no room for the image latents


# ------------------------------------------------------------------ the networks
@pytest.fixture(scope="module")
def tiny():
    cfgs = {k: v for k, v in CFG.tiny_ip2p().items() if k != "safety"}
    return cfgs, W.synth_family(cfgs, seed=3)


def test_unet_eight_input_channels(dev, tiny):
    """conv_in over 8 live channels, batch 3 (one image's three groups), 8 x 16 latent, fp32: the tolerance of the tiny-UNet case of
    tests/test_models_gpu.py."""
    cfgs, fam = tiny
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 8, 8, 16, generator=g)
    ctx = torch.randn(3, 77, cfgs["unet"]["ctx_dim"], generator=g)
    ts = OP.DDIM().set_timesteps(4)
    ref = OM.unet_forward(fam["unet"], cfgs["unet"], x, int(ts[1]), ctx)
    unet = models.UNet(fam["unet"], cfgs["unet"], dev, torch.float32)
    unet.prepare_context(ctx.to(dev))
    unet.prepare_timesteps(ts)
    got = from_nhwc(unet.forward(to_nhwc(x, torch.float32, dev, cpad=8), 1), 4)
    err = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    assert got.shape == ref.shape and err < 2e-4, err


# ------------------------------------------------------------------ the pipeline against the oracle
NIMG, HH, WW = 2, 64, 128


def _inputs(cfgs):
    ids = torch.from_numpy(np.random.RandomState(1).randint(0, cfgs["text"]["vocab"] - 2, (NIMG, 77)))
    neg = torch.from_numpy(np.random.RandomState(2).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    srcs = np.stack([synthetic_image(HH, WW, 30 + i) for i in range(NIMG)])
    g = torch.manual_seed(1)
    lat = torch.cat([torch.randn((1, 4, HH // 8, WW // 8), generator=g) for _ in range(NIMG)])
    return ids, neg, srcs, lat


@pytest.fixture(scope="module")
def oracle_runs(tiny):
    """The oracle's results, computed once per step count and shared (never written to)."""
    cfgs, fam = tiny
    ids, neg, srcs, lat = _inputs(cfgs)
    cache = {}

    def get(steps):
        if steps not in cache:
            refs = [IR.ip2p_pipeline(fam, cfgs, ids[i:i + 1], neg, srcs[i], lat[i:i + 1], steps, GS, IGS, return_latents=True)
                    for i in range(NIMG)]
            cache[steps] = (np.concatenate([r[0] for r in refs]), torch.cat([r[2] for r in refs]))
        return cache[steps]
    return get


def _against_oracle(pipe, cfgs, oracle_runs, steps):
    ids, neg, srcs, lat = _inputs(cfgs)
    ref_u8, ref_img = oracle_runs(steps)
    out, x, img = pipe.generate_batch_ip2p(ids.numpy(), neg.numpy(), srcs, lat, steps, GS, IGS, return_latents=True)
    a, b = (from_nhwc(img, 3) / 2 + 0.5).clamp(0, 1), (ref_img / 2 + 0.5).clamp(0, 1)
    d01 = (a - b).abs().max().item()
    du8 = int(np.abs(out.cpu().numpy().astype(int) - ref_u8.astype(int)).max())
    psnr = 10 * np.log10(1.0 / max(float((a - b).pow(2).mean()), 1e-20))
    return d01, du8, psnr


@pytest.fixture(scope="module")
def pipe32(dev, tiny):
    cfgs, fam = tiny
    return StableDiffusionInstructPix2PixPipeline(fam, cfgs).to(dev, torch.float32)


@pytest.mark.parametrize("graph,steps", [("1", 10), ("0", 10), ("1", 100)])
def test_ip2p_pipeline_fp32_parity(tiny, pipe32, oracle_runs, graph, steps, monkeypatch):
    """The project's bar for the fp32 path: per-pixel atol 1e-3 in [0,1] and <= 1 u8 level; 100 steps is the reference's count."""
    monkeypatch.setenv("SASPA_GRAPH", graph)
    d01, du8, psnr = _against_oracle(pipe32, tiny[0], oracle_runs, steps)
    print(f"\nfp32 ip2p tiny {steps} steps graph={graph}: max|d|={d01:.2e} u8 {du8} PSNR {psnr:.1f} dB")
    assert d01 < 1e-3 and du8 <= 1, (steps, graph, d01, du8)


def test_ip2p_refusals(tiny, pipe32):
    ids, neg, srcs, lat = _inputs(tiny[0])
    for gs, igs in ((1.0, 1.3), (7.5, 0.9), (0.0, 1.0)):
        with pytest.raises(NotImplementedError):
            pipe32.generate_batch_ip2p(ids.numpy(), neg.numpy(), srcs, lat, 4, gs, igs)
    with pytest.raises(ValueError):           # the noise has the VAE's 4 latent channels, not the UNet's 8 input channels
        pipe32.generate_batch_ip2p(ids.numpy(), neg.numpy(), srcs, torch.cat([lat, lat], 1), 4, GS, IGS)
    with pytest.raises(NotImplementedError):
        pipe32.generate_batch_img2img(ids.numpy(), neg.numpy(), srcs, lat, lat, 4, 0.5)
    from saspa_aug_amd.scheduler import PNDMScheduler, UniPCMultistepScheduler
    keep = pipe32.scheduler
    try:
        for sch in (PNDMScheduler(), UniPCMultistepScheduler.from_config(keep.config)):
            pipe32.scheduler = sch
            with pytest.raises(NotImplementedError, match="DDIM"):
                pipe32.generate_batch_ip2p(ids.numpy(), neg.numpy(), srcs, lat, 4, GS, IGS)
    finally:
        pipe32.scheduler = keep


@pytest.fixture(scope="module")
def pipe16(dev, tiny):
    cfgs, fam = tiny
    return StableDiffusionInstructPix2PixPipeline(fam, cfgs).to(dev, torch.bfloat16)


def test_ip2p_graph_equals_python_loop_bf16(tiny, pipe16, monkeypatch):
    ids, neg, srcs, lat = _inputs(tiny[0])
    res = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("SASPA_GRAPH", graph)
        out, x, _ = pipe16.generate_batch_ip2p(ids.numpy(), neg.numpy(), srcs, lat, 6, GS, IGS, return_latents=True)
        res[graph] = (out.cpu(), x.cpu().clone())
    assert torch.equal(res["1"][1], res["0"][1]) and torch.equal(res["1"][0], res["0"][0])
    assert (res["1"][1][..., 4:] == 0).all()          # group 0 carries zeros next to the latents


BF16_PSNR_MEASURED = 42.67         # dB at 10 steps against the fp32 oracle (profiles/ip2p_parity.txt)


def test_ip2p_pipeline_bf16_psnr(tiny, pipe16, oracle_runs):
    """bf16 against the fp32 oracle, 10 steps.  The run is deterministic; the 6 dB (2x the error) are for other weight seeds."""
    d01, du8, psnr = _against_oracle(pipe16, tiny[0], oracle_runs, 10)
    print(f"\nbf16 ip2p tiny 10 steps: max|d|={d01:.4f} (u8 {du8}) PSNR={psnr:.2f} dB")
    assert psnr > BF16_PSNR_MEASURED - 6.0, (d01, du8, psnr)


# ------------------------------------------------------------------ the reference's call form and the batched loop
def test_ip2p_call_form_and_run_aug(dev, tiny, tmp_path, monkeypatch):
    """init_pipeline("ip2p", None, 0) -> StableDiffusionInstructPix2PixPipeline; pass_thorugh_pipe's kwargs (:235-241, :252-255);
    the batched loop writes under regular/ip2p/None/ (:668-692), one noise draw per item, and no *_control.png (:435-442)."""
    monkeypatch.setattr(R, "IP2P_NUM_INFERENCE_STEPS", 4)
    cfgs, fam = tiny
    pipe = R.init_pipeline("ip2p", None, 0, cfgs=cfgs, state_dicts=fam)
    assert isinstance(pipe, StableDiffusionInstructPix2PixPipeline)
    pipe = pipe.to("cuda:0", torch.float16)
    src = Image.fromarray(synthetic_image(64, 128, 4))
    a = R.pass_thorugh_pipe("ip2p", pipe, "make it a seaplane", src, 0, 0.85, 30, torch.manual_seed(1), 7.5, 0.75, control_image=None)
    b = pipe(prompt="make it a seaplane", image=src, num_inference_steps=4, generator=torch.manual_seed(1), guidance_scale=7.5,
             image_guidance_scale=R.IP2P_IMAGE_GUIDANCE_SCALE, negative_prompt=R.NEGATIVE_PROMPT).images[0]
    assert a.size == (128, 64) and np.array_equal(np.asarray(a), np.asarray(b))
    prompts = tmp_path / "p.txt"
    prompts.write_text("A white airplane on a runway.\nAn airplane above the clouds.\n")
    s = R.Settings(DATASET="synthetic", NUM_PER_IMAGE=2, SEED=1, RESOLUTION=64, BATCH_SIZE=3, PROMPTS_FILE=str(prompts), SDEDIT=0,
                   BASE_MODEL="ip2p", CONTROLNET=None, NUM_INFERENCE_STEPS=30, SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0,
                   DATASET_KWARGS=dict(root_path=str(tmp_path / "ds/data"), n_images=3, sizes=((64, 64),), seed=3))
    res = R.main(s, pipe=pipe)
    assert (res["status"] == 1).all()
    assert "/aug_data/regular/ip2p/None/" in res["output_folder"]
    names = [p.name for p in pathlib.Path(res["output_folder"]).glob("*.png")]
    assert not any(n.endswith("_control.png") for n in names) and sum(n.endswith("_source.png") for n in names) == 3
    it = res["items"][0]
    single = pipe(prompt=it.prompt, image=Image.open(it.source_path).convert("RGB"), num_inference_steps=4,
                  generator=torch.manual_seed(1), guidance_scale=7.5, image_guidance_scale=R.IP2P_IMAGE_GUIDANCE_SCALE,
                  negative_prompt=R.NEGATIVE_PROMPT).images[0]
    assert np.array_equal(np.asarray(single), np.array(Image.open(it.output_path)))


# ------------------------------------------------------------------ production width
def test_ip2p_full_width(dev, monkeypatch):
    """config.IP2P (859.5 M-parameter UNet with the 8-channel conv_in, the full VAE and text tower; no safety checker): batch 1 =
    three UNet samples, 512 x 512, 2 steps, bf16.  The captured step graph and the Python-launched loop agree bit for bit."""
    cfgs = {k: v for k, v in CFG.IP2P.items() if k != "safety"}
    pipe = StableDiffusionInstructPix2PixPipeline(W.synth_family(cfgs, seed=0), cfgs).to(dev, torch.bfloat16)
    from saspa_aug_amd.synthetic import synthetic_prompt_ids
    ids, neg = synthetic_prompt_ids(1, seed=2), synthetic_prompt_ids(1, seed=3)
    src = synthetic_image(512, 512, 5)[None]
    lat = torch.randn((1, 4, 64, 64), generator=torch.manual_seed(1))
    res = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("SASPA_GRAPH", graph)
        out, x, img = pipe.generate_batch_ip2p(ids, neg, src, lat, 2, GS, IGS, return_latents=True)
        res[graph] = (out.cpu(), x.float().cpu(), img.float().cpu())
    out, x, img = res["1"]
    assert out.shape == (1, 512, 512, 3) and torch.isfinite(x).all() and torch.isfinite(img).all()
    assert x[..., :4].abs().max() > 0 and out.float().std() > 0
    assert torch.equal(x, res["0"][1]) and torch.equal(out, res["0"][0])
