"""The CFG-shared encoder prefix (SASPA_CFG_PREFIX): under classifier-free guidance the two halves of the batch differ in the
text context only, so conv_in, down_blocks.0.resnets.0 and the first transformer up to its self-attention run once per image,
in the UNet and in the ControlNet.  Three layers: the fused cross-attention launch reading a shared x / residual
(saspa_xattn_block_bcast) against the same launch on duplicated rows, the networks' encode(cfg_pair=True) against
encode(cat([x, x])), and the pipeline with the knob on and off."""
import math

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.models import ATTN_LOG2E
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline, StableDiffusionXLControlNetPipeline, cfg_prefix_enabled
from saspa_aug_amd.synthetic import synthetic_image
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
C, D = 320, 40


def _relerr(got, ref):
    return ((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-6)).item()


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_operands():
    """Four samples of 256 rows (the most any case reads) and their contexts, made once."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(512, C, generator=g) * 1.5 + 0.3
    res = torch.randn(512, C, generator=g)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wq = torch.randn(C, C, generator=g) / math.sqrt(C) * (D ** -0.5 * ATTN_LOG2E)
    wo, bo = torch.randn(C, C, generator=g) / math.sqrt(C), 0.2 * torch.randn(C, generator=g)
    k, v = torch.randn(4, 77, C, generator=g) * 2.0, torch.randn(4, 77, C, generator=g)
    w, bias = W.pack_xattn_w(wq, wo, bo)
    return dict(x=x, res=res, gamma=gamma, beta=beta, w=w, bias=bias, k=k, v=v)


def _kernel_case(dev, op, dtype, x_rows, m, separate_residual, pitched):
    rep = m // x_rows
    ln = (op["gamma"].to(dev), op["beta"].to(dev), 1e-5)
    w, bias = op["w"].to(dev, dtype), op["bias"].to(dev)
    kf, vf = W.xattn_kv_fragments(op["k"][:m // 256].to(dev, dtype), op["v"][:m // 256].to(dev, dtype))

    def rows(t, n):
        t = t[:n].to(dev, dtype)
        if not pitched:
            return t.contiguous()
        buf = torch.zeros((n, 328), device=dev, dtype=dtype)          # ldx = 328
        buf[:, :C] = t
        return buf[:, :C]
    x = rows(op["x"], x_rows)
    res = op["res"][:x_rows].to(dev, dtype).contiguous() if separate_residual else None
    got = ops.xattn_block(x, ln, w, bias, kf, vf, 77, 256, residual=res, x_rows=x_rows)
    xd = rows(op["x"][:x_rows].repeat(rep, 1), m)
    resd = res.repeat(rep, 1) if separate_residual else None
    ref = ops.xattn_block(xd, ln, w, bias, kf, vf, 77, 256, residual=resd)
    assert got.shape == ref.shape == (m, C)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got, ref), f"max |d| = {(got.float() - ref.float()).abs().max().item()}"
    # the halves really saw different keys (a wrong sample index would make them equal or swap them)
    assert not torch.equal(got[:x_rows], got[x_rows:2 * x_rows])


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("separate_residual", [False, True])
@pytest.mark.parametrize("x_rows,m", [(256, 512), (512, 1024)])
def test_xattn_block_bcast_is_bit_identical(dev, kernel_operands, x_rows, m, separate_residual, pitched):
    _kernel_case(dev, kernel_operands, torch.bfloat16, x_rows, m, separate_residual, pitched)


def test_xattn_block_bcast_fp16_library(dev, kernel_operands):
    _kernel_case(dev, kernel_operands, torch.float16, 512, 1024, True, True)


def test_xattn_block_bcast_refuses_bad_rows(dev, kernel_operands):
    op = kernel_operands
    kf, vf = W.xattn_kv_fragments(op["k"][:3].to(dev, torch.bfloat16), op["v"][:3].to(dev, torch.bfloat16))
    x = op["x"].to(dev, torch.bfloat16)
    with pytest.raises(RuntimeError):        # 768 output rows are no whole number of copies of 512
        ops.xattn_block(x, (op["gamma"].to(dev), op["beta"].to(dev), 1e-5), op["w"].to(dev, torch.bfloat16), op["bias"].to(dev), kf, vf,
                        77, 256, x_rows=512)
    with pytest.raises(ValueError):          # x_rows is the number of rows x holds
        ops.xattn_block(x, (op["gamma"].to(dev), op["beta"].to(dev), 1e-5), op["w"].to(dev, torch.bfloat16), op["bias"].to(dev), kf, vf,
                        77, 256, x_rows=256)


# ---- 2. the networks, full SD-1.5 width -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_nets(dev):
    cfgs = CFG.SD15
    fam = dict(unet=W.synth_state_dict("unet", cfgs["unet"], 0), controlnet=W.synth_state_dict("controlnet", cfgs["controlnet"], 1))
    nets = {}

    def get(dtype):
        if dtype not in nets:
            nets.clear()                    # one dtype's pair resident at a time
            nets[dtype] = (models.UNet(fam["unet"], cfgs["unet"], dev, dtype), models.ControlNet(fam["controlnet"], cfgs["controlnet"], dev, dtype))
        return nets[dtype]
    yield cfgs, get
    nets.clear()
    fam.clear()


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_networks_shared_prefix_vs_duplicated_batch(dev, full_nets, monkeypatch, dtype, b):
    """256x256 image (1024 level-0 tokens): encode(x, cfg_pair=True) against encode(cat([x, x])) for both networks, and the whole
    evaluation.  bf16 takes the fused cross-attention launch on the shared rows (a different kernel from the three launches the
    duplicated batch of 2048 / 4096 rows takes): the project's limit for 'the same evaluation through a different kernel',
    2e-2 (test_unet_controlnet_ff_block_knob).  fp32 takes the generic fallback (one copy, then the same code): 1e-5.
    Measured (MI355X) -- see profiles/EXPERIMENTS.md, "CFG-shared encoder prefix"."""
    cfgs, get = full_nets
    unet, cn = get(dtype)
    h = w = 32
    g = torch.Generator().manual_seed(23 + b)
    x = torch.randn(b, 4, h, w, generator=g)
    ctx = torch.randn(2 * b, 77, cfgs["unet"]["ctx_dim"], generator=g)       # uncond rows first, every row different
    cond = torch.rand(b, 3, 8 * h, 8 * w, generator=g)
    ts = OP.DDIM().set_timesteps(4)
    for net in (unet, cn):
        net.prepare_context(ctx.to(dev, dtype))
        net.prepare_timesteps(ts)
    xd = to_nhwc(x, dtype, dev, cpad=8)
    cemb = cn.cond_embedding(to_nhwc(cond, dtype, dev, cpad=8))
    x2, cemb2 = torch.cat([xd, xd]), torch.cat([cemb, cemb])

    shared_calls, self_attn = [], []
    real_x, real_a = ops.xattn_block, models.attention_core

    def counted_x(*a, **k):
        if k.get("x_rows") is not None:
            shared_calls.append(k["x_rows"])
        return real_x(*a, **k)

    def counted_a(q, k, vt, heads, nq, nk, **kw):
        if nq == nk == h * w:
            self_attn.append(q.shape[0])
        return real_a(q, k, vt, heads, nq, nk, **kw)
    monkeypatch.setattr(ops, "xattn_block", counted_x)
    monkeypatch.setattr(models, "attention_core", counted_a)

    errs = {}
    outs = {}
    for name, net, res in (("unet", unet, None), ("controlnet", cn, cemb)):
        del shared_calls[:], self_attn[:]
        mid_s, skips_s = net.encode(xd, 1, conv_in_residual=res, cfg_pair=True)
        # one fused cross-attention launch on the shared rows (bf16) / none (fp32: the fallback); of the two level-0 blocks'
        # self-attentions one ran at B rows and one at 2B
        assert shared_calls == ([b * h * w] if dtype == torch.bfloat16 else []), shared_calls
        assert sorted(self_attn) == [b, 2 * b], self_attn
        del self_attn[:]
        mid_u, skips_u = net.encode(x2, 1, conv_in_residual=None if res is None else cemb2)
        assert sorted(self_attn) == [2 * b, 2 * b], self_attn
        assert skips_s[0].shape[0] == b and all(s.shape[0] == 2 * b for s in skips_s[1:]) and mid_s.shape == mid_u.shape
        assert len(skips_s) == len(skips_u)
        e = [_relerr(mid_s, mid_u), _relerr(skips_s[0], skips_u[0][:b])] + [_relerr(s, u) for s, u in zip(skips_s[1:], skips_u[1:])]
        errs[name] = max(e)
        outs[name] = (mid_s, skips_s, mid_u, skips_u)
    umid_s, uskips_s, umid_u, uskips_u = outs["unet"]
    cmid_s, cfeats_s, cmid_u, cfeats_u = outs["controlnet"]
    s2, m2 = cn.zero_convs(cmid_s, cfeats_s, 0.75, uskips_s, umid_s, cfg_pair=True)
    assert all(s.shape[0] == 2 * b for s in s2)
    got = from_nhwc(unet.decode(m2, s2, 1), 4).float().cpu()
    s2, m2 = cn.zero_convs(cmid_u, cfeats_u, 0.75, uskips_u, umid_u)
    ref = from_nhwc(unet.decode(m2, s2, 1), 4).float().cpu()
    errs["evaluation"] = _relerr(got, ref)
    print(f"CFG-shared prefix vs duplicated batch, {dtype}, B = {b}: max-rel differences {errs}")
    assert not torch.equal(got[:b], got[b:])                 # the halves saw their own contexts
    lim = 2e-2 if dtype == torch.bfloat16 else 1e-5
    assert max(errs.values()) < lim, errs


def test_sdxl_networks_refuse_the_shared_form(dev):
    """The added conditioning gives the two halves different time embeddings: encode(cfg_pair=True) raises before any launch."""
    cfgs = CFG.tiny_xl()
    fam = W.synth_family(cfgs, seed=3)
    unet = models.UNet(fam["unet"], cfgs["unet"], dev, torch.bfloat16)
    x = torch.zeros((1, 8, 8, 8), device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="cfg_pair"):
        unet.encode(x, 0, cfg_pair=True)


# ---- 3. the pipeline --------------------------------------------------------------------------------------------------------
def _inputs(cfgs, n, hh, ww, seed):
    rs = np.random.RandomState(seed)
    ids = rs.randint(0, cfgs["text"]["vocab"] - 2, (n, 77))
    neg = rs.randint(0, cfgs["text"]["vocab"] - 2, (1, 77))
    ctrl = np.stack([(synthetic_image(hh, ww, seed + i) > 128).astype(np.uint8) * 255 for i in range(n)])
    lat = torch.randn((n, 4, hh // 8, ww // 8), generator=torch.manual_seed(seed))
    return ids, neg, ctrl, lat


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pipeline_knob_on_vs_off(dev, monkeypatch, dtype):
    """Tiny config, 2 steps, two images: SASPA_CFG_PREFIX=1 against 0 through generate_batch on the graph path and on the eager
    path (u8 images within 1 level), and the graph path against the eager path under the knob (bit for bit, as without it:
    test_graph_gpu.test_graph_replay_equals_eager_sd15)."""
    cfgs = CFG.tiny()
    pipe = StableDiffusionControlNetPipeline(W.synth_family(cfgs, seed=3), cfgs).to(dev, dtype)
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SASPA_CFG_PREFIX", knob)
        assert cfg_prefix_enabled() == (knob == "1")
        for graph in ("0", "1"):
            monkeypatch.setenv("SASPA_GRAPH", graph)
            img, lat, _ = pipe.generate_batch(*_inputs(cfgs, 2, 64, 64, 31), 2, return_latents=True)
            out[knob, graph] = (img.cpu().numpy().astype(int), lat.clone())
    assert sorted(g.cfg_pair for g in pipe._graphs.values()) == [False, True]
    for graph in ("0", "1"):
        du8 = np.abs(out["1", graph][0] - out["0", graph][0]).max()
        dl = _relerr(out["1", graph][1], out["0", graph][1])
        print(f"SASPA_CFG_PREFIX on vs off, {dtype}, SASPA_GRAPH={graph}: u8 images differ by {du8}, latents max-rel {dl:.3e}")
        assert du8 <= 1, du8
    for knob in ("0", "1"):
        assert torch.equal(out[knob, "1"][1], out[knob, "0"][1]), f"graph replay differs from the eager loop, SASPA_CFG_PREFIX={knob}"
        assert np.array_equal(out[knob, "1"][0], out[knob, "0"][0])


def test_pipeline_without_cfg_is_untouched(dev, monkeypatch):
    """No classifier-free guidance (the SDXL-Turbo operating point, guidance_scale 0): nothing is shared, bit-identical with the knob
    on and off; with guidance the SDXL pipeline does not ask for the shared form either."""
    cfgs = CFG.tiny_xl()
    pipe = StableDiffusionXLControlNetPipeline(W.synth_family(cfgs, seed=3), cfgs).to(dev, torch.bfloat16)
    v = cfgs["text"]["vocab"]
    rs = np.random.RandomState(41)
    ids = np.full((2, 77), v - 1, np.int64)
    ids[:, 0] = v - 2
    ids[:, 1:20] = rs.randint(0, v - 2, (2, 19))
    ctrl = np.stack([(synthetic_image(64, 64, 41 + i) > 128).astype(np.uint8) * 255 for i in range(2)])
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SASPA_CFG_PREFIX", knob)
        for gs in (0.0, 2.0):
            lat = torch.randn((2, 4, 8, 8), generator=torch.manual_seed(41))
            img, x, _ = pipe.generate_batch(ids, None, ctrl, lat, 2, guidance_scale=gs, return_latents=True)
            out[knob, gs] = (img.clone(), x.clone())
    for gs in (0.0, 2.0):
        assert torch.equal(out["1", gs][0], out["0", gs][0]) and torch.equal(out["1", gs][1], out["0", gs][1]), gs
