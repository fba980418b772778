"""The fp32-storage VAE with its mid-block attention as one fused x3 launch (SASPA_VAE_ATTN_F32=fused, ops.attn_wide_x3) on the
MI355X: encoder moments and decoder output against the CPU oracle at the fp32 bars the unfused path is held to, under both fp32 GEMM
forms; the launches with the knob unset against those recorded on the commit before the knob existed
(tests/golden/xl_vae_x3attn_launches.json); the encoder's x3 GEMM form and its chunking for the 32-bit byte-offset limit.

The VAE is a reduced one whose mid block is 192 channels wide -- the narrowest head models.wide_head admits."""
import json
import os
from collections import Counter

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import sd_models as OM
from saspa_aug_amd import models, ops
from saspa_aug_amd import weights as W
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
F32 = torch.float32
VAE = dict(latent_channels=4, out_channels=3, block_out=(32, 64, 192, 192), layers=1, groups=8, scaling_factor=0.13025)
SIZES = ((64, 64), (64, 96))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xl_vae_x3attn_launches.json")
# the bars of tests/test_sdedit_gpu.py::test_vae_encoder (fp32: max-abs relative to the largest moment) and of
# tests/test_models_gpu.py's XL decoder parity test (max |d| of the image on [0,1]: exact, x3)
ENC_BAR = 2e-4
DEC_BAR = dict(exact=2e-5, x3=2e-4)
A_DEC, A_ENC = "decoder.mid_block.attentions.0", "encoder.mid_block.attentions.0"


@pytest.fixture(scope="module")
def vae_sd():
    assert models.wide_head(VAE["block_out"][-1])
    sd = W.synth_state_dict("vae", VAE, 4)
    sd.update(W.synth_state_dict("vae_enc", VAE, 104))
    return sd


@pytest.fixture(scope="module")
def refs(vae_sd):
    """Per size: (pixels, oracle moments, latents, oracle decode); computed once, shared, never modified."""
    out = []
    for i, (hh, ww) in enumerate(SIZES):
        x = torch.rand(2, 3, hh, ww, generator=torch.Generator().manual_seed(1 + i)) * 2 - 1
        z = torch.randn(2, 4, hh // 8, ww // 8, generator=torch.Generator().manual_seed(12 + i))
        out.append((x, torch.cat(OM.vae_encode(vae_sd, VAE, x), 1), z, OM.vae_decode(vae_sd, VAE, z)))
    return out


def _knob(monkeypatch, on):
    if on:
        monkeypatch.setenv("SASPA_VAE_ATTN_F32", "fused")
    else:
        monkeypatch.delenv("SASPA_VAE_ATTN_F32", raising=False)


def _nets(monkeypatch, vae_sd, dev, cls, gemm):
    nets = {}
    for name, on in (("unfused", False), ("fused", True)):
        _knob(monkeypatch, on)
        nets[name] = cls(vae_sd, VAE, dev, F32, f32_gemm=gemm)
    _knob(monkeypatch, False)
    return nets


@pytest.mark.parametrize("gemm", ["x3", "exact"])
def test_encoder_moments_against_the_oracle(dev, vae_sd, refs, monkeypatch, gemm):
    nets = _nets(monkeypatch, vae_sd, dev, models.VAEEncoder, gemm)
    assert (A_ENC + ".qkv.w") in nets["fused"].p and (A_ENC + ".qkv.w") not in nets["unfused"].p
    assert models.vae_attn_fused(F32) is False
    for x, ref, _, _ in refs:
        e = {}
        for name, net in nets.items():
            got = from_nhwc(net.encode(to_nhwc(x, F32, dev, cpad=8)))
            assert got.shape == ref.shape
            e[name] = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"\n[xl vae x3attn] encode {tuple(x.shape)} f32_gemm={gemm}: max-rel unfused {e['unfused']:.3e}, fused {e['fused']:.3e} (bar {ENC_BAR})")
        assert e["unfused"] < ENC_BAR and e["fused"] < ENC_BAR, e


@pytest.mark.parametrize("gemm", ["x3", "exact"])
def test_decoder_output_against_the_oracle(dev, vae_sd, refs, monkeypatch, gemm):
    nets = _nets(monkeypatch, vae_sd, dev, models.VAEDecoder, gemm)
    assert (A_DEC + ".qkv.w") in nets["fused"].p and (A_DEC + ".qkv.w") not in nets["unfused"].p
    for _, _, z, ref in refs:
        e = {}
        for name, net in nets.items():
            got = from_nhwc(net.decode(to_nhwc(z, F32, dev, cpad=8)), 3)
            e[name] = ((got / 2 + 0.5).clamp(0, 1) - (ref / 2 + 0.5).clamp(0, 1)).abs().max().item()
        print(f"\n[xl vae x3attn] decode {tuple(z.shape)} f32_gemm={gemm}: max |d| on [0,1] unfused {e['unfused']:.3e}, fused {e['fused']:.3e} "
              f"(bar {DEC_BAR[gemm]})")
        assert e["unfused"] < DEC_BAR[gemm] and e["fused"] < DEC_BAR[gemm], e


def _kinds(run):
    kinds = []
    ops.set_recorder(lambda kind, flops, call, meta: kinds.append(kind) or call())
    try:
        run()
    finally:
        ops.set_recorder(None)
    torch.cuda.synchronize()
    return kinds


def launches(dev, vae_sd, **kw):
    """Kernel kinds, in launch order, of one fp32 decode of a [1,8,8,*] latent and one fp32 encode of a [1,64,64,*] image per GEMM form:
    what tests/golden/xl_vae_x3attn_launches.json holds for the commit before SASPA_VAE_ATTN_F32 (recorded by this function there)."""
    z = torch.zeros(1, 8, 8, 8, device=dev)
    x = torch.zeros(1, 64, 64, 8, device=dev)
    out = {}
    for gemm in ("exact", "x3"):
        dec = models.VAEDecoder(vae_sd, VAE, dev, F32, f32_gemm=gemm, **kw)
        out[f"decoder {gemm}"] = _kinds(lambda: dec.decode(z))
    enc = models.VAEEncoder(vae_sd, VAE, dev, F32, **kw)
    out["encoder exact"] = _kinds(lambda: enc.encode(x))
    return out


def test_knob_unset_launches_what_the_parent_launched(dev, vae_sd, monkeypatch):
    _knob(monkeypatch, False)
    golden = json.load(open(GOLDEN))
    got = launches(dev, vae_sd)
    assert set(got) == set(golden)
    for name in golden:
        assert got[name] == golden[name], (name, Counter(got[name]), Counter(golden[name]))
        assert "attn_wide_x3" not in got[name] and got[name].count("softmax_rows") == 1
    # with the knob on: one fused launch instead of scores GEMM, softmax, PV GEMM and the transposed value projection
    _knob(monkeypatch, True)
    fused = launches(dev, vae_sd)
    for name in golden:
        assert fused[name].count("attn_wide_x3") == 1 and "softmax_rows" not in fused[name], name
        assert Counter(fused[name]) - Counter(golden[name]) == Counter({"attn_wide_x3": 1}), name
        assert len(golden[name]) - len(fused[name]) == 3, name


def test_encoder_x3_against_exact(dev, vae_sd, refs):
    """The x3 GEMM form of the encoder against the exact one, inside the bound the decoder's x3 test uses (2e-4)."""
    nets = {g: models.VAEEncoder(vae_sd, VAE, dev, F32, f32_gemm=g) for g in ("exact", "x3")}
    assert any(getattr(t, "saspa_wsplit", 0) for t in nets["x3"].p.values())
    assert not any(getattr(t, "saspa_wsplit", 0) for t in nets["exact"].p.values())
    for x, *_ in refs:
        xd = to_nhwc(x, F32, dev, cpad=8)
        a, b = nets["exact"].encode(xd), nets["x3"].encode(xd)
        d = ((a - b).abs().max() / a.abs().max()).item()
        print(f"\n[xl vae x3attn] encoder x3 vs exact {tuple(x.shape)}: max-rel {d:.3e}")
        assert 0.0 < d < 2e-4, d
    assert ops._F32_GEMM_MODE[0] == "exact"                 # encode leaves the mode as it found it


@pytest.mark.parametrize("gemm", ["exact", "x3"])
def test_chunked_encode_equals_the_unchunked_one(dev, vae_sd, refs, gemm):
    """Three images with the offset limit forced down to one image per launch sequence (and to two: a last chunk of one)."""
    x = refs[1][0]
    xd = to_nhwc(torch.cat([x, x[:1].flip(-1)]), F32, dev, cpad=8)
    net = models.VAEEncoder(vae_sd, VAE, dev, F32, f32_gemm=gemm)
    whole = net.encode(xd)
    per_img = xd.shape[1] * xd.shape[2] * VAE["block_out"][0] * 4
    assert per_img * 3 < net.OFFSET_LIMIT
    for imgs in (1, 2):
        net.OFFSET_LIMIT = per_img * imgs + 1                # the test hook: an instance attribute over the class constant
        sizes = []
        real = net._encode
        net._encode = lambda t: sizes.append(t.shape[0]) or real(t)
        try:
            got = net.encode(xd)
        finally:
            del net._encode, net.OFFSET_LIMIT
        assert sizes == ([1, 1, 1] if imgs == 1 else [2, 1]) and torch.equal(got, whole), (imgs, sizes)
