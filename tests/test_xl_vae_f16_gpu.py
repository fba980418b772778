"""The SDXL VAE in IEEE fp16 (and bf16 with the fused mid-block attention) on the MI355X: decoder and encoder against the CPU oracle on
a VAE with the real 512-channel mid block, the tiny SDXL pipeline in every VAE mode, run_aug's construction under SASPA_XL_VAE, and the
launches of the mid block.  Parity is shown on synthetic weights: the fp16-fix checkpoint is not available offline."""
import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import sd_models as OM
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionXLControlNetPipeline
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
BF, F16 = torch.bfloat16, torch.float16
RATIO = 0.25                    # rms-rel(fp16) / rms-rel(bf16): expected 2^-11 / 2^-8 = 1/8 (tests/test_fp16_models_gpu.py's margin)
BF16_MAXREL = 6e-2              # the bound tests/test_models_gpu.py / test_sdedit_gpu.py hold the bf16 VAE to (max-abs relative)
# the real mid width and little else
VAE = dict(latent_channels=4, out_channels=3, block_out=(16, 32, 512, 512), layers=1, groups=8, scaling_factor=0.13025)
LATENTS = ((2, 4, 8, 8), (1, 4, 8, 24))


def _rms_rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)).item()


def _max_rel(got, ref):
    return ((got.float().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


@pytest.fixture(scope="module")
def wide_vae():
    sd = W.synth_state_dict("vae", VAE, 4)
    sd.update(W.synth_state_dict("vae_enc", VAE, 104))
    return sd


@pytest.fixture(scope="module")
def decoder_refs(wide_vae):
    """Latents and the oracle's decode of them: computed once, shared, never modified."""
    out = []
    for i, shape in enumerate(LATENTS):
        z = torch.randn(shape, generator=torch.Generator().manual_seed(12 + i))
        out.append((z, OM.vae_decode(wide_vae, VAE, z)))
    return out


def _fused(monkeypatch, on):
    if on:
        monkeypatch.setenv("SASPA_VAE_ATTN", "fused")
    else:
        monkeypatch.delenv("SASPA_VAE_ATTN", raising=False)


def test_decoder_fp16_and_fused_bf16_against_the_oracle(dev, wide_vae, decoder_refs, monkeypatch):
    nets = {}
    for name, dt, fused in (("bf16", BF, False), ("bf16 fused", BF, True), ("fp16", F16, False)):
        _fused(monkeypatch, fused)
        nets[name] = models.VAEDecoder(wide_vae, VAE, dev, dt)
    _fused(monkeypatch, False)
    a = "decoder.mid_block.attentions.0"
    assert a + ".qkv.w" in nets["fp16"].p and a + ".qkv.w" in nets["bf16 fused"].p and a + ".qkv.w" not in nets["bf16"].p
    assert nets["fp16"].p[a + ".qkv.w"].dtype == F16 and nets["fp16"].p["decoder.conv_in.w"].dtype == F16
    for z, ref in decoder_refs:
        e, m = {}, {}
        for name, net in nets.items():
            raw = net.decode(to_nhwc(z, net.dtype, dev, cpad=8))
            got = from_nhwc(raw, 3)
            assert raw.dtype == net.dtype and bool(torch.isfinite(got).all()), name
            e[name], m[name] = _rms_rel(got, ref), _max_rel(got, ref)
        print(f"\n[xl vae] decode {tuple(z.shape)}: rms-rel " + ", ".join(f"{k} {v:.3e}" for k, v in e.items())
              + f"; ratio fp16 / bf16 {e['fp16'] / e['bf16']:.3f} (<= {RATIO}; expected 0.125); max-rel "
              + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
        assert e["fp16"] <= RATIO * e["bf16"], (e, tuple(z.shape))
        assert m["bf16"] < BF16_MAXREL and m["bf16 fused"] < BF16_MAXREL, m


def test_encoder_fp16_and_fused_bf16_against_the_oracle(dev, wide_vae, monkeypatch):
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)) * 2 - 1
    mean, logvar = OM.vae_encode(wide_vae, VAE, x)
    ref = torch.cat([mean, logvar], 1)
    e, m = {}, {}
    for name, dt, fused in (("bf16", BF, False), ("bf16 fused", BF, True), ("fp16", F16, False)):
        _fused(monkeypatch, fused)
        net = models.VAEEncoder(wide_vae, VAE, dev, dt)
        assert ("encoder.mid_block.attentions.0.qkv.w" in net.p) == (name != "bf16")
        got = from_nhwc(net.encode(to_nhwc(x, dt, dev, cpad=8)))
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
        e[name], m[name] = _rms_rel(got, ref), _max_rel(got, ref)
    print(f"\n[xl vae] encode moments: rms-rel " + ", ".join(f"{k} {v:.3e}" for k, v in e.items())
          + f"; ratio fp16 / bf16 {e['fp16'] / e['bf16']:.3f} (<= {RATIO}); max-rel " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()))
    assert e["fp16"] <= RATIO * e["bf16"], e
    assert m["bf16"] < BF16_MAXREL and m["bf16 fused"] < BF16_MAXREL, m


def test_mid_block_is_one_attention_launch_without_a_score_matrix(dev, wide_vae, monkeypatch):
    z, b, n = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3)), 2, 64

    def mid_launches(net):
        x = ops.conv(ops.conv(to_nhwc(z, net.dtype, dev, cpad=8), net.p["post_quant_conv.w"], net.p["post_quant_conv.b"]),
                     net.p["decoder.conv_in.w"], net.p["decoder.conv_in.b"], kh=3, kw=3, pad=1)
        kinds, shapes, real_empty = [], [], torch.empty

        def empty(*a, **k):
            shapes.append(tuple(a[0]) if a and isinstance(a[0], (tuple, list, torch.Size)) else tuple(a))
            return real_empty(*a, **k)
        monkeypatch.setattr(torch, "empty", empty)
        ops.set_recorder(lambda kind, flops, call, meta: kinds.append(kind) or call())
        try:
            net.mid_attention(x)
        finally:
            ops.set_recorder(None)
            monkeypatch.setattr(torch, "empty", real_empty)
        torch.cuda.synchronize()
        return kinds, shapes

    for dt, fused in ((F16, False), (BF, True)):
        _fused(monkeypatch, fused)
        kinds, shapes = mid_launches(models.VAEDecoder(wide_vae, VAE, dev, dt))
        assert kinds.count("attn_wide") == 1 and "softmax_rows" not in kinds and "flash_attn" not in kinds, kinds
        assert kinds.count("gemm") == 2, kinds           # the Q | K | V projection and the out projection (+ the GroupNorm launches)
        assert (b, 1, n, n) not in shapes, shapes
    _fused(monkeypatch, False)                           # the default bf16 VAE: today's launches, the score matrix included
    kinds, shapes = mid_launches(models.VAEDecoder(wide_vae, VAE, dev, BF))
    assert "attn_wide" not in kinds and kinds.count("softmax_rows") == 1 and (b, 1, n, n) in shapes, (kinds, shapes)


# ---- the tiny SDXL pipeline ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_xl():
    cfgs = CFG.tiny_xl()
    return cfgs, W.synth_family(cfgs, seed=3)


def _inputs(cfgs, n=2):
    v = cfgs["text"]["vocab"]
    rs = np.random.RandomState(1)
    ids = np.full((n, 77), v - 1, np.int64)
    ids[:, 0] = v - 2
    ids[:, 1:20] = rs.randint(0, v - 2, (n, 19))
    ctrl = (rs.rand(n, 64, 64, 3) > 0.9).astype(np.uint8) * 255
    lat = torch.randn((n, 4, 8, 8), generator=torch.manual_seed(5))
    return ids, ctrl, lat


def test_pipeline_f16_mode_decodes_its_own_latents_in_fp16(dev, tiny_xl):
    cfgs, fam = tiny_xl
    ids, ctrl, lat = _inputs(cfgs)
    pipe = StableDiffusionXLControlNetPipeline(fam, cfgs)
    pipe.set_vae_mode("f16").upcast_vae()                           # the reference's upcast_vae() call is a no-op in this mode
    pipe = pipe.to(dev, torch.float16)
    assert pipe.vae.dtype == F16 and pipe.unet.dtype == BF and pipe.dtype == BF
    out, x, img = pipe.generate_batch(ids, None, ctrl, lat, 2, return_latents=True)
    assert img.dtype == F16 and out.dtype == torch.uint8
    vae = models.VAEDecoder(fam["vae"], cfgs["vae"], dev, F16)
    z = ops.scale(x, 1.0 / cfgs["vae"]["scaling_factor"]).to(F16)
    assert torch.equal(ops.act_to_u8(vae.decode(z)), out)
    assert pipe.last_nonfinite is not None and pipe.last_nonfinite.dtype == torch.bool
    assert pipe.last_nonfinite.cpu().tolist() == [False, False]
    # the guard is per image, and only this mode raises it
    bad = img.clone()
    bad[1, 3, 4, 1] = float("inf")
    assert pipe._nonfinite_guard(bad).cpu().tolist() == [False, True]
    pipe.set_vae_mode("bf16")                                       # after .to(): re-packed from the retained state dict
    assert pipe.vae.dtype == BF
    pipe.generate_batch(ids, None, ctrl, lat, 2)
    assert pipe.last_nonfinite is None


def test_pipeline_default_mode_is_todays_upcast(dev, tiny_xl, monkeypatch):
    monkeypatch.delenv("SASPA_XL_VAE", raising=False)
    cfgs, fam = tiny_xl
    ids, ctrl, lat = _inputs(cfgs)
    ref = StableDiffusionXLControlNetPipeline(fam, cfgs)
    ref.upcast_vae()
    ref = ref.to(dev, torch.float16)
    assert ref.vae.dtype == torch.float32 and ref.vae.f32_gemm == "x3" and ref._vae_mode is None
    want = ref.generate_batch(ids, None, ctrl, lat, 2)
    assert ref.last_nonfinite is None
    for mode in (None, "x3"):
        p = StableDiffusionXLControlNetPipeline(fam, cfgs).set_vae_mode(mode)
        p.upcast_vae()
        p = p.to(dev, torch.float16)
        assert p.vae.dtype == torch.float32 and p.vae.f32_gemm == "x3"
        assert torch.equal(p.generate_batch(ids, None, ctrl, lat, 2), want), mode
    p = StableDiffusionXLControlNetPipeline(fam, cfgs).set_vae_mode(None).to(dev, torch.float16)
    assert p.vae.dtype == BF                                        # no upcast_vae(): the pipeline's dtype, as today


def test_init_pipeline_under_the_environment_builds_the_fp16_vae(dev, tiny_xl, monkeypatch):
    cfgs, fam = tiny_xl
    monkeypatch.setenv("SASPA_XL_VAE", "f16")
    pipe = R.init_pipeline("sd_xl-turbo", "canny", 0, cfgs=cfgs, state_dicts=fam).to(dev, torch.float16)
    assert pipe.vae.dtype == F16 and pipe._vae_mode == "f16"
    monkeypatch.setenv("SASPA_XL_VAE", "f32")
    with pytest.raises(ValueError, match="VAE mode"):
        R.init_pipeline("sd_xl-turbo", "canny", 0, cfgs=cfgs, state_dicts=dict(fam)).to(dev, torch.float16)
