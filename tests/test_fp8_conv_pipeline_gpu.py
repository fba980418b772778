"""The opt-in MX-fp8 resnet convs in the pipelines (enable_fp8(convs=True)): which convs are routed (every branch of
_Net.resnet), determinism and closeness to the fp8 path without them on tiny SD-1.5 / SDXL families whose widths are multiples of
160; then at production size under the production routing rule against the CPU oracle (image 0, short trajectories: SD-1.5 at
512x512 and SDXL-Turbo at 1024x1024) and the fp8 FLOP share at 1024x1024 as tools/sdxl_bench.py records it.  PSNR bounds =
measured - 6 dB (printed)."""
import re

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from oracle.canny import generate_canny_array
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline, StableDiffusionXLControlNetPipeline, graphs_enabled
from saspa_aug_amd.synthetic import negative_prompt_ids, synthetic_image, synthetic_prompt_ids
from tests.util import from_nhwc

pytestmark = pytest.mark.gpu


# (latents rms-rel, image PSNR dB) of test_sd15_512_production_vs_oracle as measured on the MI355X (current synthetic weights)
SD15_MEASURED = (5.69e-2, 34.9)


def _resnet_convs(sd):
    return {k[:-len(".weight")] for k in sd if re.search(r"resnets\.\d+\.conv[12]\.weight$", k)}


def _eligible(sd):
    out = set()
    for name in _resnet_convs(sd):
        n, c = sd[name + ".weight"].shape[:2]
        if c % 32 == 0 and n % 160 == 0:
            out.add(name)
    return out


def _ids(vocab, n, seed):
    rs = np.random.RandomState(seed)
    ids = np.full((n, 77), vocab - 1, np.int64)
    ids[:, 0] = vocab - 2
    for r in range(n):
        k = rs.randint(5, 30)
        ids[r, 1:1 + k] = rs.randint(0, vocab - 2, k)
    return ids


@pytest.mark.parametrize("family", ["sd15", "sdxl"])
def test_routed_set_and_determinism(dev, family, monkeypatch):
    # tiny images have few output tiles: admit every eligible conv so that the routing itself is under test
    monkeypatch.setattr(models, "MXFP8_CONV_MIN_TILES", 0)
    monkeypatch.setattr(models, "MXFP8_CONV_FULL_TILES", 0)
    if family == "sd15":
        cfgs = CFG.tiny(width=160, groups=16, heads=4)
        cls = StableDiffusionControlNetPipeline
    else:
        cfgs = CFG.tiny_xl(width=160, groups=16)
        cls = StableDiffusionXLControlNetPipeline
    fam = W.synth_family(cfgs, seed=5)
    b = 2
    ids = _ids(cfgs["text"]["vocab"], b, 1)
    neg = _ids(cfgs["text"]["vocab"], b, 2) if family == "sd15" else None        # SD-1.5 with CFG, SDXL-Turbo without
    ctrl = np.zeros((b, 128, 128, 3), np.uint8)
    ctrl[:, 40:90, 30:100] = 255
    lat = torch.randn((b, 4, 16, 16), generator=torch.manual_seed(2), dtype=torch.float16)
    outs = {}
    for convs in (False, True):
        pipe = cls(dict(fam), cfgs)
        pipe.enable_fp8(True, convs=convs)
        pipe = pipe.to(dev, torch.bfloat16)
        a = pipe.generate_batch(ids, neg, ctrl, lat, 2)
        for net, sd in ((pipe.unet, fam["unet"]), (pipe.controlnet, fam["controlnet"])):
            if convs:
                want = _eligible(sd)
                assert want and net.fp8_convs == want, sorted(net.fp8_convs ^ want)
            else:
                assert net.fp8_convs == set()                    # enable_fp8() alone routes no conv
        b2 = pipe.generate_batch(ids, neg, ctrl, lat, 2)
        assert torch.equal(a, b2)                                # bit-identical runs (the second one replays the step graph)
        outs[convs] = a.float()
        del pipe
    d = (outs[True] - outs[False]).abs()
    print(f"[{family}] MX-fp8 convs vs fp8 projections only: image max|d| {d.max().item():.1f}, mean {d.mean().item():.2f} (u8)")
    assert d.mean().item() < 8.0


def test_convs_need_fp8():
    cfgs = CFG.tiny(width=160, groups=16, heads=4)
    pipe = StableDiffusionControlNetPipeline(W.synth_family(cfgs, seed=5), cfgs)
    with pytest.raises(ValueError):
        pipe.enable_fp8(False, convs=True)


def test_mixed_branches(dev, monkeypatch):
    """A rule that admits conv1 but not conv2 of some resnets (MX conv1 -> GroupNorm -> bf16 conv2) and conv2 but not conv1 of others
    (bf16 conv1 leaving epilogue statistics -> quantiser -> MX conv2): here by input channels, C <= 320."""
    monkeypatch.setattr(models, "MXFP8_CONV_FULL_TILES", 1 << 30)
    monkeypatch.setattr(models, "MXFP8_CONV_MIN_TILES", 0)
    monkeypatch.setattr(models, "MXFP8_CONV_SHORT_C", 320)
    cfgs = CFG.tiny(width=160, groups=16, heads=4)
    fam = W.synth_family(cfgs, seed=5)
    b = 2
    ids, neg = _ids(cfgs["text"]["vocab"], b, 1), _ids(cfgs["text"]["vocab"], b, 2)
    ctrl = np.zeros((b, 128, 128, 3), np.uint8)
    ctrl[:, 30:100, 40:80] = 255
    lat = torch.randn((b, 4, 16, 16), generator=torch.manual_seed(3), dtype=torch.float16)
    outs = {}
    for convs in (False, True):
        pipe = StableDiffusionControlNetPipeline(dict(fam), cfgs)
        pipe.enable_fp8(True, convs=convs)
        pipe = pipe.to(dev, torch.bfloat16)
        a = pipe.generate_batch(ids, neg, ctrl, lat, 2)
        if convs:
            for net, sd in ((pipe.unet, fam["unet"]), (pipe.controlnet, fam["controlnet"])):
                want = {n for n in _eligible(sd) if sd[n + ".weight"].shape[1] <= 320}
                assert net.fp8_convs == want, sorted(net.fp8_convs ^ want)
            routed = pipe.unet.fp8_convs
            res = {n.rsplit(".", 1)[0] for n in _resnet_convs(fam["unet"])}
            only1 = [r for r in res if r + ".conv1" in routed and r + ".conv2" not in routed]
            only2 = [r for r in res if r + ".conv2" in routed and r + ".conv1" not in routed]
            assert only1 and only2, (only1, only2)
        assert torch.equal(pipe.generate_batch(ids, neg, ctrl, lat, 2), a)
        outs[convs] = a.float()
        del pipe
    d = (outs[True] - outs[False]).abs()
    print(f"[mixed] MX-fp8 convs (C <= 320) vs fp8 projections only: image max|d| {d.max().item():.1f}, mean {d.mean().item():.2f} (u8)")
    assert d.mean().item() < 8.0


def _metrics(img, x, ref_img, ref_x):
    got01, ref01 = (from_nhwc(img, 3) / 2 + 0.5).clamp(0, 1), (ref_img / 2 + 0.5).clamp(0, 1)
    mse = float((got01.double() - ref01.double()).pow(2).mean())
    gx = from_nhwc(x, 4)
    rms = ((gx - ref_x).pow(2).mean().sqrt() / ref_x.pow(2).mean().sqrt()).item()
    return 10 * np.log10(1.0 / max(mse, 1e-20)), (got01 - ref01).abs().max().item(), rms


def test_sd15_512_production_vs_oracle(dev):
    """SD-1.5 + ControlNet at the bench's configs[1] size (batch 8, 512x512, CFG 7.5) with fp8 projections and MX-fp8 convs under the
    production routing rule, 5 DDIM steps, image 0 against the CPU oracle."""
    cfgs = {k: v for k, v in CFG.SD15.items() if k != "safety"}
    fam = W.synth_family(cfgs, seed=0)
    b, res, steps = 8, 512, 5
    vocab = cfgs["text"]["vocab"]
    ids, neg = synthetic_prompt_ids(b, seed=1, vocab=vocab), negative_prompt_ids(vocab)
    ctrls = np.stack([generate_canny_array(synthetic_image(res, res, 40 + i), 120, 200) for i in range(b)])
    lat = torch.randn((b, 4, res // 8, res // 8), generator=torch.Generator().manual_seed(1), dtype=torch.float16)
    ref_u8, ref_x, ref_img = OP.sd_controlnet_pipeline(fam, cfgs, torch.from_numpy(ids[:1]), torch.from_numpy(neg), ctrls[0],
                                                       lat[:1].float(), steps, return_latents=True)
    # the fp8 projections alone on the same run, for scale (printed, not asserted: test_production_gpu.py holds the bf16 path)
    pipe = StableDiffusionControlNetPipeline(dict(fam), cfgs)
    pipe.enable_fp8(True)
    pipe = pipe.to(dev, torch.bfloat16)
    out, x, img = pipe.generate_batch(ids, neg, ctrls, lat, steps, return_latents=True)
    psnr8, _, rms8 = _metrics(img[:1], x[:1], ref_img, ref_x)
    del pipe
    pipe = StableDiffusionControlNetPipeline(dict(fam), cfgs)
    pipe.enable_fp8(True, convs=True)
    pipe = pipe.to(dev, torch.bfloat16)
    assert graphs_enabled()
    out, x, img = pipe.generate_batch(ids, neg, ctrls, lat, steps, return_latents=True)
    # the production rule routes the 64x64 / 32x32 levels (>= 256 tiles at 2 x 8 images) and leaves 16x16 / 8x8 on bf16
    for net, sd in ((pipe.unet, fam["unet"]), (pipe.controlnet, fam["controlnet"])):
        assert net.fp8_convs and net.fp8_convs < _eligible(sd), sorted(net.fp8_convs)
    psnr, d01, rms = _metrics(img[:1], x[:1], ref_img, ref_x)
    print(f"\n[production SD-1.5 fp8 + MX-fp8 convs] batch {b} 512x512 vs oracle, {steps} steps, image 0: latents rms-rel {rms:.3e}; "
          f"image max|d| {d01:.4f} PSNR {psnr:.1f} dB ({len(pipe.unet.fp8_convs)} + {len(pipe.controlnet.fp8_convs)} convs routed); "
          f"fp8 projections alone: latents rms-rel {rms8:.3e}, PSNR {psnr8:.1f} dB")
    # measured: SD15_MEASURED (the CFG combine amplifies uncorrelated eps error by ~7.5 sqrt(2)); the bf16 path measures PSNR 41.4 dB,
    # latents rms-rel 2.66e-2 (test_production_gpu.py).  Bounds = 2x rms, PSNR - 6 dB.
    assert rms < 2 * SD15_MEASURED[0] and psnr > SD15_MEASURED[1] - 6.0, (rms, d01, psnr)
    del pipe
    torch.cuda.empty_cache()


def test_sdxl_1024_production_vs_oracle_and_fp8_share(dev):
    """configs[4]: SDXL-Turbo + ControlNet at full width, 1024x1024, 4 DDIM steps, no CFG, conditioning scale 0.75 (the configuration of
    test_production_families_gpu.py's SDXL test: batch 2, fp32-upcast VAE), fp8 projections + MX-fp8 convs under the production rule.
    Image 0 against the oracle must meet the fp8 path's bar (latents rms-rel < 3e-2, PSNR > 42.7 dB).  Then the fp8 FLOP share of one
    UNet + ControlNet evaluation at the batch tools/sdxl_bench.py times (8), recorded as it records it (2 x steps minus steps)."""
    cfgs = CFG.SDXL_TURBO
    fam = W.synth_family(cfgs, seed=0)
    b, res, steps = 2, 1024, 4
    v = cfgs["text"]["vocab"]
    rs = np.random.RandomState(3)
    ids1 = np.full((b, 77), v - 1, np.int64)
    ids1[:, 0] = v - 2
    for r in range(b):
        k = rs.randint(8, 30)
        ids1[r, 1:1 + k] = rs.randint(0, v - 2, k)
    ctrls = np.stack([generate_canny_array(synthetic_image(res, res, 90 + i), 120, 200) for i in range(b)])
    lat = torch.randn((b, 4, res // 8, res // 8), generator=torch.manual_seed(1), dtype=torch.float16)
    pipe = StableDiffusionXLControlNetPipeline(dict(fam), cfgs)
    pipe.enable_fp8(True, convs=True)
    pipe.upcast_vae()
    pipe = pipe.to(dev, torch.bfloat16)
    ids2 = pipe.pad_ids_2(ids1)
    out, x, img = pipe.generate_batch(ids1, None, ctrls, lat, steps, 0.0, 0.75, return_latents=True, prompt_ids_2=ids2)
    assert pipe.unet.fp8_convs and pipe.controlnet.fp8_convs
    img, x = img.clone(), x.clone()
    ref_u8, ref_x, ref_img = OP.sdxl_controlnet_pipeline(fam, cfgs, torch.from_numpy(ids1[:1]), torch.from_numpy(ids2[:1]), ctrls[0],
                                                         lat[:1].float(), steps, return_latents=True)
    psnr, d01, rms = _metrics(img[:1], x[:1], ref_img, ref_x)
    print(f"\n[production SDXL fp8 + MX-fp8 convs] bf16+graph batch {b} 1024x1024 vs oracle, {steps} steps, image 0: latents rms-rel "
          f"{rms:.3e}; image max|d| {d01:.4f} PSNR {psnr:.1f} dB")
    assert rms < 3e-2 and psnr > 42.7, (rms, d01, psnr)
    # fp8 share (tools/sdxl_bench.py: batch 8, its prompts / control images / noise; families 8 = saspa_gemm_fp8, 32 = MX-fp8 conv)
    from bench import Recorder
    nb = 8
    ids8 = synthetic_prompt_ids(nb)
    imgs = torch.from_numpy(np.stack([synthetic_image(res, res, i) for i in range(nb)])).to(dev)
    lat8 = torch.randn((nb, 4, res // 8, res // 8), generator=torch.manual_seed(1), dtype=torch.float16)

    def recorded(nsteps):
        rec = Recorder()
        ops.set_recorder(rec)
        try:
            pipe.generate_batch(ids8, None, ops.canny(imgs, 120, 200), lat8, nsteps, 0.0, 0.75)
        finally:
            ops.set_recorder(None)
        torch.cuda.synchronize()
        fams = (ops.GEMM_FAMILY_FP8, ops.GEMM_FAMILY_MXFP8_CONV)
        f8 = sum(fl for k, fl, _, _, m in rec.items if k == "gemm" and Recorder.kernel_family(k, m) in fams)
        mx = sum(fl for k, fl, _, _, m in rec.items if k == "gemm" and Recorder.kernel_family(k, m) == ops.GEMM_FAMILY_MXFP8_CONV)
        return f8, mx, sum(fl for k, fl, _, _, m in rec.items if k in ("gemm", "flash_attn"))
    (f8a, mxa, alla), (f8b, mxb, allb) = recorded(steps), recorded(2 * steps)
    share, mx_share = (f8b - f8a) / (allb - alla), (mxb - mxa) / (allb - alla)
    print(f"[production SDXL fp8 + MX-fp8 convs] batch {nb} 1024x1024: fp8 FLOP share of an evaluation {share:.4f} "
          f"(MX-fp8 convs {mx_share:.4f})")
    assert share >= 0.74 and mx_share > 0.15, (share, mx_share)
    del pipe
    torch.cuda.empty_cache()
