"""Upsample2D as four 2x2 phase convs in one launch (SaspaGemmParams.upsample = 2): ops.conv with the phase weights of
weights.pack_conv_up2x against a float64 reference built from exactly the bf16 phase weights the kernel reads (the `gemm` budget of
tests/errbudget.py with the magnitude of the phase operands), on every kernel family that takes the mode; the GroupNorm statistics
of the epilogue and of the split-K reduce; the networks and the pipeline with SASPA_UPCONV_PHASE on against off."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from oracle import pipeline as OP
from saspa_aug_amd import config as CFG
from saspa_aug_amd import models, ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline
from saspa_aug_amd.synthetic import synthetic_image
from tests.errbudget import LIMITS, UNIT_BF16, budget_stats, check_budget, conv_scale, fmt, ratio
from tests.test_upconv_phase_host import phase_conv
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
UNIT_F16 = 2.0 ** -11

# (B, H, W, Cin, Cout)
ODD = (1, 3, 5, 16, 48)            # odd extents, every border tap, N below a tile; Cin below a K-tile: the generic loader
RAGGED = (1, 8, 12, 32, 48)        # 96 rows per phase: a ragged tail in every phase
SPLITK = (2, 16, 16, 256, 640)     # K slices + reduce, an image boundary inside a 256-row tile
STATS = (3, 8, 8, 64, 320)         # 64 rows per phase and image: statistics through the reduce launch
STATS_UNSPLIT = (2, 16, 16, 64, 320)   # whole 128-row blocks per phase and image: statistics out of the epilogues


def _case(case, seed, dtype=BF):
    """Operands of a case (made on the CPU): x and the fp32 master weights; the phase weights as stored (rounded once), the fp64
    reference of the four 2x2 convs with exactly those, and its magnitude."""
    b, h, w, cin, cout = case
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(b, cin, h, w, generator=g) + 0.25).to(dtype).double()
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    bias = torch.randn(cout, generator=g).double()
    wph = W.pack_conv_up2x(wt).to(dtype)                       # [4, Cout, 4 * Cin_pad], tap-major
    ref = phase_conv(x, wph.double(), bias)
    s = (phase_conv(x.abs(), wph.double().abs(), bias.abs())).clamp_min(2.0 ** -10 * ref.abs().mean().item())
    return dict(case=case, x=x, wt=wt, bias=bias, wph=wph, ref=ref, s=s, dtype=dtype)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(case, dtype=BF):
        if (case, dtype) not in made:
            made[case, dtype] = _case(case, 101 + len(made), dtype)
        return made[case, dtype]
    return get


def _phase_weights(op, dev, chunk=False):
    cp = W.round8(op["case"][3])
    wph = op["wph"]
    if chunk:
        wph = torch.stack([W.to_chunk_major(wph[i], 4, op["dtype"]) for i in range(4)])
    t = wph.to(dev).contiguous()
    t.saspa_korder = 1 if chunk else 0
    t.saspa_cin = cp
    return t


def _run(op, dev, *, variant=0, ksplit=None, chunk=False, gn_unit=None):
    b, h, w, cin, cout = op["case"]
    xd = to_nhwc(op["x"].float(), op["dtype"], dev, cpad=W.round8(cin))
    out = ops.conv(xd, _phase_weights(op, dev, chunk), op["bias"].float().to(dev), kh=3, kw=3, pad=1, upsample=True, variant=variant,
                   ksplit=ksplit, gn_unit=gn_unit)
    assert tuple(out.shape[:3]) == (b, 2 * h, 2 * w)
    return out


def _check(out, op, what):
    unit = UNIT_BF16 if op["dtype"] == BF else UNIT_F16
    st = check_budget(from_nhwc(out, op["case"][4]), op["ref"], op["s"], unit, limits=LIMITS["gemm"], what=what)
    print(f"\n[budget] gemm  {what}: {fmt(st)}")
    return st


# ---- kernel level ------------------------------------------------------------------------------------------------------------
# variant: SASPA_GEMM_AUTO / TILED (4-wave LDS-DMA tiles; the generic loader where Cin is no whole K-tile) / WIDE (8-wave)
@pytest.mark.parametrize("case,variant,ksplit,chunk", [
    (ODD, 0, None, False), (ODD, 1, None, False),                    # generic loader (Cin = 16), odd extents
    (RAGGED, 0, None, False), (RAGGED, 1, None, False),              # generic loader (Cin = 32), ragged phase tail
    (SPLITK, 0, None, False), (SPLITK, 0, None, True),               # the dispatch's own choice, both K orders
    (SPLITK, 1, 1, True), (SPLITK, 1, 4, True), (SPLITK, 1, 3, False),   # 4-wave DMA tiles: epilogue store / slabs + reduce
    (SPLITK, 2, 1, True), (SPLITK, 2, 4, True), (SPLITK, 2, 2, False),   # 8-wave kernel: epilogue store / slabs + reduce
    (STATS, 2, 1, True), (STATS_UNSPLIT, 1, 1, False),               # more images, 64 / 256 rows per phase and image
])
def test_phase_conv_budget(dev, cases, case, variant, ksplit, chunk):
    op = cases(case)
    _check(_run(op, dev, variant=variant, ksplit=ksplit, chunk=chunk), op, f"phase conv {case} variant {variant} ksplit {ksplit} chunk {chunk}")


def test_phase_conv_fp16_library(dev, cases):
    op = cases(SPLITK, torch.float16)
    _check(_run(op, dev, chunk=True), op, f"phase conv {SPLITK} fp16")
    _check(_run(op, dev, variant=1, ksplit=1), op, f"phase conv {SPLITK} fp16, 4-wave tiles")


def test_phase_conv_against_the_nine_tap_launch(dev, cases):
    """Today's upsample=True launch with tap-wise bf16 weights from the same master: both lie within the budget of the fp64 result of
    their own weights, which differ by the weights' rounding (one unit of the same magnitude): twice the limit between them."""
    for case in (RAGGED, SPLITK):
        op = cases(case)
        b, h, w, cin, cout = case
        xd = to_nhwc(op["x"].float(), BF, dev, cpad=W.round8(cin))
        old = ops.conv(xd, W.pack_conv(op["wt"]).to(dev, BF), op["bias"].float().to(dev), kh=3, kw=3, pad=1, upsample=True)
        new = _run(op, dev)
        xin = F.interpolate(op["x"], scale_factor=2.0, mode="nearest")
        s = conv_scale(xin, op["wt"].to(BF).double(), op["bias"])
        twice = {k: 2 * v for k, v in LIMITS["gemm"].items()}
        st = budget_stats(from_nhwc(new, cout), from_nhwc(old, cout).double(), s, UNIT_BF16)
        print(f"\n[budget x2] phase vs nine-tap launch {case}: {fmt(st)}")
        assert ratio(st, twice) <= 1.0, (case, fmt(st))


@pytest.mark.parametrize("case,variant,ksplit", [(STATS, 0, None), (STATS, 1, 2), (STATS_UNSPLIT, 1, 1), (STATS_UNSPLIT, 2, 1),
                                                 (STATS_UNSPLIT, 2, 2), (STATS_UNSPLIT, 0, None)])
def test_phase_conv_groupnorm_statistics(dev, cases, case, variant, ksplit):
    """gn_unit: the statistics the launch leaves against sums formed from the stored output, per image and unit (the consumer sums
    an image's hw / 128 slots: which rows a slot holds is the producer's business)."""
    op = cases(case)
    b, h, w, cin, cout = case
    out = _run(op, dev, variant=variant, ksplit=ksplit, gn_unit=10)
    _check(out, op, f"phase conv + statistics {case} variant {variant} ksplit {ksplit}")
    assert hasattr(out, "saspa_gn"), "no statistics were left"
    stats, unit = out.saspa_gn[0], out.saspa_gn[1]
    nblk = 4 * h * w // 128
    assert tuple(stats.shape) == (b * nblk, cout // unit, 2) and unit == 10
    got = stats.double().cpu().view(b, nblk, cout // unit, 2).sum(1)
    o = out.double().cpu()[..., :cout].reshape(b, 4 * h * w, cout // unit, unit)
    want = torch.stack([o.sum((1, 3)), (o * o).sum((1, 3))], -1)
    # a slot is an fp32 sum of at most 128 rows * unit exact terms (bf16 values, their exact squares) added one after the other:
    # at most 1280 roundings of 2^-24 of the running magnitude each < 2^-13 of the sum of magnitudes; the slots are added in fp64
    mag = torch.stack([o.abs().sum((1, 3)), (o * o).sum((1, 3))], -1)
    err = ((got - want).abs() / mag).max().item()
    print(f"\nstatistics {case} variant {variant} ksplit {ksplit}: max error / sum of magnitudes {err:.3e}")
    assert err <= 2.0 ** -13
    # and the consumer reads them: GroupNorm with the epilogue statistics against GroupNorm with its own pass
    gamma, beta = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    y1 = ops.groupnorm(out, gamma, beta, 32, 1e-5)
    del out.saspa_gn
    y0 = ops.groupnorm(out, gamma, beta, 32, 1e-5)
    # (the two sets of statistics differ in fp32 rounding only: at most one bf16 step of a normalised value below 8)
    assert (y1.float() - y0.float()).abs().max().item() <= 2.0 ** -5


def test_phase_conv_refuses_what_it_does_not_serve(dev, cases):
    op = cases(RAGGED)
    b, h, w, cin, cout = RAGGED
    xd = to_nhwc(op["x"].float(), BF, dev, cpad=W.round8(cin))
    wph = _phase_weights(op, dev)
    res = torch.zeros((b, 2 * h, 2 * w, cout), device=dev, dtype=BF)
    with pytest.raises(ValueError):
        ops.conv(xd, wph, None, kh=3, kw=3, pad=1, upsample=True, residual=res)
    with pytest.raises(ValueError):
        ops.conv(xd, wph, None, kh=3, kw=3, pad=1, upsample=False)


# ---- network level -----------------------------------------------------------------------------------------------------------
def _relerr(got, ref):
    return ((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-6)).item()


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_networks_knob_on_vs_off(dev, monkeypatch, dtype):
    """Tiny config: UNet.decode and the VAE decoder packed with SASPA_UPCONV_PHASE=1 against =0.  bf16: a different kernel and
    differently rounded weights, the project's 2e-2 max-rel limit for that; fp32: the same launches, bit-identical."""
    cfgs = CFG.tiny()
    fam = W.synth_family(cfgs, seed=3)
    nets = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SASPA_UPCONV_PHASE", knob)
        nets[knob] = (models.UNet(fam["unet"], cfgs["unet"], dev, dtype), models.VAEDecoder(fam["vae"], cfgs["vae"], dev, dtype))
    phase = [k for k, t in nets["1"][0].p.items() if k.endswith("upsamplers.0.conv.w") and t.dim() == 3]
    assert bool(phase) == (dtype == BF) and not any(torch.is_tensor(t) and t.dim() == 3 for t in nets["0"][0].p.values())
    g = torch.Generator().manual_seed(5)
    x = to_nhwc(torch.randn(2, 4, 16, 16, generator=g), dtype, dev, cpad=8)
    ctx = torch.randn(2, 77, cfgs["unet"]["ctx_dim"], generator=g).to(dev, dtype)
    outs = {}
    for knob in ("0", "1"):
        unet, vae = nets[knob]
        unet.prepare_context(ctx)
        unet.prepare_timesteps(OP.DDIM().set_timesteps(4))
        mid, skips = unet.encode(x, 1)
        eps = unet.decode(mid, skips, 1)
        outs[knob] = (eps.clone(), vae.decode(x).clone())
    for i, name in enumerate(("UNet", "VAE decoder")):
        a, b = outs["1"][i], outs["0"][i]
        if dtype == BF:
            e = _relerr(a, b)
            print(f"\nSASPA_UPCONV_PHASE on vs off, {name}, bf16: max-rel {e:.3e}")
            assert e < 2e-2, (name, e)
        else:
            assert torch.equal(a, b), name


def test_pipeline_graph_equals_eager_with_phase_convs(dev, monkeypatch):
    monkeypatch.setenv("SASPA_UPCONV_PHASE", "1")
    cfgs = CFG.tiny()
    pipe = StableDiffusionControlNetPipeline(W.synth_family(cfgs, seed=3), cfgs).to(dev, BF)
    assert any(torch.is_tensor(t) and t.dim() == 3 for t in pipe.unet.p.values())
    rs = np.random.RandomState(31)
    ids = rs.randint(0, cfgs["text"]["vocab"] - 2, (2, 77))
    neg = rs.randint(0, cfgs["text"]["vocab"] - 2, (1, 77))
    ctrl = np.stack([(synthetic_image(64, 64, 31 + i) > 128).astype(np.uint8) * 255 for i in range(2)])
    out = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("SASPA_GRAPH", graph)
        lat = torch.randn((2, 4, 8, 8), generator=torch.manual_seed(31))
        img, x, _ = pipe.generate_batch(ids, neg, ctrl, lat, 2, return_latents=True)
        out[graph] = (img.clone(), x.clone())
    assert torch.equal(out["1"][1], out["0"][1]) and torch.equal(out["1"][0], out["0"][0])
