"""Calibration-free fp8 feed-forward on the GPU: `saspa_gemm_fp8_geglu_mx` (GEGLU epilogue -> e4m3 bytes + one E8M0 exponent per row
and 32 columns) and `saspa_gemm_mxfp8` (the exponents applied inside the scaled MFMA) against tests/mxfp8_ff_ref.py -- bit equality
on exact operands, the limits proven in tests/test_mxfp8_ff_host.py on random ones -- and `enable_fp8(ff="mx")` in the SDXL pipeline:
the oracle distance the calibrated path is held to, and the properties the mode exists for (no state from an earlier batch, capture
without an eager run)."""
import ctypes as C

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, models, ops
from saspa_aug_amd import config as CFG
from saspa_aug_amd import weights as W
from tests import fp8_ref as R
from tests import mxfp8_ff_ref as M
from tests.errbudget import UNIT_BF16, check_budget, fmt, rejects
from tests.test_mxfp8_ff_host import MX_LIMITS

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _f32(t, dev):
    return t.float().to(dev)


def _producer(dev, op, **kw):
    return ops.linear_fp8(R.to_codes(op["a"]).to(dev), _f32(op["sa"], dev), R.to_codes(op["w"]).to(dev), _f32(op["sw"], dev),
                          _f32(op["bias"], dev), act=ops.ACT_GEGLU, out_mx=True, **kw)


def _consumer(dev, q, qs, op2, *, residual=True, bias=True):
    return ops.linear_mxfp8(q, qs, R.to_codes(op2["w"]).to(dev), _f32(op2["sw"], dev), _f32(op2["bias"], dev) if bias else None,
                            residual=op2["res"].to(dev, torch.bfloat16) if residual else None)


def _same_bytes(got, want, what):
    got = got.cpu()
    bad = (got != want).nonzero()
    print(f"\n[bytes] {what}: {len(bad)} of {want.numel()} differ")
    assert len(bad) == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def _raw_params(a, w, sw, out, *, sa=None, bias=None, act=ops.ACT_NONE, m=None):
    p = _lib.GemmF8Params()
    p.a, p.lda, p.w, p.ldw = a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0)
    p.M, p.N, p.K = a.shape[0] if m is None else m, w.shape[0], a.shape[1]
    p.sa, p.sw, p.bias = None if sa is None else sa.data_ptr(), sw.data_ptr(), None if bias is None else bias.data_ptr()
    p.act, p.out, p.ldo = int(act), out.data_ptr(), out.stride(0)
    return p


# ------------------------------------------------------------------ producer
@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("k", [128, 256])
@pytest.mark.parametrize("m", [1, 127, 129, 515])
def test_producer_exact_operands_bit_equal(dev, m, k, n):
    """Integer e4m3 codes and power-of-two scales (R.exact_operands): the bf16 tile entering the GELU is known to the bit, so the
    bytes and the exponents must be the emulation's.  M: one row | a ragged first row tile | one row in the second | five tiles;
    K: one K-tile | both ring stages; N = 256: the second column tile writes blocks 2, 3 (bn * 2 + half)."""
    op = R.exact_operands(_rand, m, k, n, 811, geglu=True)
    want_q, want_qs = M.producer_emul(op)
    q, qs = _producer(dev, op)
    assert q.dtype == torch.uint8 and q.shape == (m, n // 2) and qs.dtype == torch.uint8 and qs.shape == (m, n // 64)
    _same_bytes(qs, want_qs, f"exponents {m}x{k}x{n}")
    _same_bytes(q, want_q, f"codes {m}x{k}x{n}")
    assert R.e4m3_decode(q.cpu()).abs().max().item() <= 448.0


def test_producer_isolation(dev):
    """A row's bytes depend on that row alone (row r of M = 515 == the M = 1 launch of that row), and nothing is written outside the
    M rows and the N / 2 (N / 64) columns: `out` and `qs` are views of larger buffers filled with 0xFF."""
    m, k, n = 515, 256, 256
    op = R.exact_operands(_rand, m, k, n, 821, geglu=True)
    q, qs = _producer(dev, op)
    for r in (0, 127, 128, 514):
        op1 = {key: (v[r:r + 1] if v.shape[0] == m else v) for key, v in op.items()}
        q1, qs1 = _producer(dev, op1)
        assert torch.equal(q1, q[r:r + 1]) and torch.equal(qs1, qs[r:r + 1]), r
    a8, w8 = R.to_codes(op["a"]).to(dev), R.to_codes(op["w"]).to(dev)
    sa, sw, b = _f32(op["sa"], dev), _f32(op["sw"], dev), _f32(op["bias"], dev)
    obuf = torch.full((640, n // 2 + 16), 0xFF, dtype=torch.uint8, device=dev)
    sbuf = torch.full((640, 8), 0xFF, dtype=torch.uint8, device=dev)
    p = _raw_params(a8, w8, sw, obuf, sa=sa, bias=b, act=ops.ACT_GEGLU)
    _lib.check(_lib.load().saspa_gemm_fp8_geglu_mx(C.byref(p), sbuf.data_ptr(), sbuf.stride(0), ops._stream()), "saspa_gemm_fp8_geglu_mx")
    assert torch.equal(obuf[:m, :n // 2], q) and torch.equal(sbuf[:m, :n // 64], qs)
    assert (obuf[m:] == 0xFF).all() and (obuf[:, n // 2:] == 0xFF).all()
    assert (sbuf[m:] == 0xFF).all() and (sbuf[:, n // 64:] == 0xFF).all()


# ------------------------------------------------------------------ consumer
@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("m", [1, 129])
@pytest.mark.parametrize("k", [128, 384])
def test_consumer_exact_operands_bit_equal(dev, k, m, n):
    """M.exact_consumer_operands: exponents 120 .. 134 varying per (row, block), sums exact whatever their order.  K = 128: one tile,
    all four op-sel bytes; K = 384: an odd tile count that wraps the ring.  With and without bias / residual; ldqs > K / 32."""
    op = M.exact_consumer_operands(_rand, m, k, n, 831)
    assert m == 1 or (op["qs"].min().item() == 120 and op["qs"].max().item() == 134)
    q = R.to_codes(op["a"]).to(dev)
    sbuf = torch.full((m, k // 32 + 4), 0xFF, dtype=torch.uint8, device=dev)
    sbuf[:, :k // 32] = op["qs"].to(dev)
    for qs in (op["qs"].to(dev), sbuf[:, :k // 32]):                          # dense, then inside a wider buffer
        for residual, bias in ((True, True), (False, True), (False, False), (True, False)):
            got = _consumer(dev, q, qs, op, residual=residual, bias=bias).cpu().double()
            want = M.consumer_emul(q.cpu(), op["qs"], op, residual=residual, bias=bias)
            assert torch.equal(got, want), (k, m, n, residual, bias, int((got != want).sum()))


def test_consumer_never_reads_pad_rows(dev):
    """E8M0 255 is NaN and NaN * 0 is NaN: the scale bytes of the rows >= M of the last row tile must not come from memory."""
    m, k, n = 129, 256, 128
    op = M.exact_consumer_operands(_rand, m, k, n, 841)
    q = R.to_codes(op["a"]).to(dev)
    buf = torch.full((256, 16), 0xFF, dtype=torch.uint8, device=dev)
    buf[:m, :k // 32] = op["qs"].to(dev)
    got = _consumer(dev, q, buf[:m, :k // 32], op)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, _consumer(dev, q, op["qs"].to(dev), op))


def test_consumer_equals_the_tensor_scale_kernel_on_uniform_exponents(dev):
    """Every exponent 127 + log2 s: saspa_gemm_mxfp8 == saspa_gemm_fp8 with ONE activation scale s on the same bytes."""
    m, k, n = 129, 384, 256
    op = M.exact_consumer_operands(_rand, m, k, n, 851)
    q, w8 = R.to_codes(op["a"]).to(dev), R.to_codes(op["w"]).to(dev)
    res = op["res"].to(dev, torch.bfloat16)
    for l in (-5, 0, 4):
        qs = torch.full((m, k // 32), 127 + l, dtype=torch.uint8, device=dev)
        mx = ops.linear_mxfp8(q, qs, w8, _f32(op["sw"], dev), _f32(op["bias"], dev), residual=res)
        one = ops.linear_fp8(q, torch.tensor([2.0 ** l], device=dev), w8, _f32(op["sw"], dev), _f32(op["bias"], dev), residual=res)
        assert torch.equal(mx, one), l


# ------------------------------------------------------------------ the pair on random operands
def test_pair_random_operands_within_the_host_limits(dev):
    """(515, 640, 5120) -> (515, 2560) -> (515, 640) on M.pair_operands: both checks of tests/test_mxfp8_ff_host.py, its limits
    unchanged; handing the consumer the neighbouring block's exponents must fall outside them."""
    m, c = M.PAIR_SHAPE
    op1, op2 = M.pair_operands(_rand, m, c, M.PAIR_SEED)
    y, ys = M.producer_ref(op1)
    ref, s = M.consumer_ref(y, op2)
    q, qs = _producer(dev, op1)
    st = check_budget(M.decode_blocks(q.cpu(), qs.cpu()), y, ys, UNIT_BF16, limits=MX_LIMITS["emit"], what="emit")
    print(f"\n[budget] emit {m}x{c}x{8 * c}: {fmt(st)}")
    assert R.e4m3_decode(q.cpu()).abs().max().item() <= 448.0
    out = _consumer(dev, q, qs, op2)
    st = check_budget(out.cpu(), ref, s, UNIT_BF16, limits=MX_LIMITS["pair"], what="pair")
    print(f"\n[budget] pair {m}x{4 * c}x{c}: {fmt(st)}")
    want_q, want_qs = M.producer_emul(op1)
    print(f"\n[bytes] against the emulation: {(qs.cpu() != want_qs).double().mean().item():.2e} of the exponents, "
          f"{(q.cpu() != want_q).double().mean().item():.2e} of the codes differ")
    wrong = _consumer(dev, q, qs.roll(-1, 1).contiguous(), op2)
    assert rejects(wrong.cpu(), ref, s, UNIT_BF16, limits=MX_LIMITS["pair"]), "the neighbouring block's exponents were not rejected"


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    lib = _lib.load()
    x8 = torch.zeros(128, 128, dtype=torch.uint8, device=dev)
    one = torch.ones(128, device=dev)
    s1 = torch.ones(1, device=dev)
    for kw in (dict(out_fp8_scale=s1), dict(amax=s1)):
        with pytest.raises(ValueError):
            ops.linear_fp8(x8, one, x8, one, act=ops.ACT_GEGLU, out_mx=True, **kw)
    with pytest.raises(ValueError):
        ops.linear_fp8(x8, one, x8, one, out_mx=True)                                          # not the GEGLU epilogue
    out = torch.full((128, 128), 7.0, dtype=torch.bfloat16, device=dev)
    qs = torch.full((128, 8), 127, dtype=torch.uint8, device=dev)
    ok = _raw_params(x8, x8, one, out)
    codes = set()
    for mut in (dict(sa=one.data_ptr()), dict(act=int(ops.ACT_GEGLU)), dict(out_fp8=1), dict(amax=s1.data_ptr())):
        p = _raw_params(x8, x8, one, out)
        for key, v in mut.items():
            setattr(p, key, v)
        rc = lib.saspa_gemm_mxfp8(C.byref(p), qs.data_ptr(), 8, ops._stream())
        assert rc != 0, mut
        codes.add(rc)
    assert len(codes) == 1                                                                     # SASPA_EINVAL, all of them
    assert lib.saspa_gemm_mxfp8(C.byref(ok), qs.data_ptr(), 6, ops._stream()) not in (0, *codes)        # ldqs % 4
    pg = _raw_params(x8, x8, one, out.view(torch.uint8), sa=one, act=ops.ACT_GEGLU)
    for mut in (dict(out_fp8=1, out_scale=s1.data_ptr()), dict(amax=s1.data_ptr())):
        p = _raw_params(x8, x8, one, out.view(torch.uint8), sa=one, act=ops.ACT_GEGLU)
        for key, v in mut.items():
            setattr(p, key, v)
        assert lib.saspa_gemm_fp8_geglu_mx(C.byref(p), qs.data_ptr(), 8, ops._stream()) in codes, mut
    assert lib.saspa_gemm_fp8_geglu_mx(C.byref(pg), qs.data_ptr(), 6, ops._stream()) not in (0, *codes)
    x192 = torch.zeros(128, 192, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="saspa_gemm_mxfp8"):
        ops.linear_mxfp8(x192, qs, x192, one)                                                  # K = 192
    with pytest.raises(RuntimeError, match="saspa_gemm_fp8_geglu_mx"):
        ops.linear_fp8(x192, one, x192, one, act=ops.ACT_GEGLU, out_mx=True)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (qs == 127).all()                                            # refused before any launch


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def sdxl():
    """The reduced-width SDXL case of tests/test_fp8_gpu.py::test_sdxl_pipeline_fp8_vs_oracle_and_bf16 (tiny_xl(width=64), batch 2,
    64 x 64, 2 steps) plus a second batch X of other prompts, edges and noise."""
    from oracle.canny import generate_canny_array
    from saspa_aug_amd.synthetic import synthetic_image
    cfgs = CFG.tiny_xl(width=64)
    fam = W.synth_family(cfgs, seed=2)
    b, res = 2, 64
    v = cfgs["text"]["vocab"]

    def batch(seed, img0, lat_seed):
        rs = np.random.RandomState(seed)
        ids1 = np.full((b, 77), v - 1, np.int64)
        ids1[:, 0] = v - 2
        ids1[:, 1:9] = rs.randint(0, v - 2, (b, 8))
        ctrls = np.stack([generate_canny_array(synthetic_image(res, res, img0 + i), 120, 200) for i in range(b)])
        lat = torch.randn((b, 4, res // 8, res // 8), generator=torch.manual_seed(lat_seed), dtype=torch.float16)
        return ids1, ctrls, lat
    y = batch(3, 30, 1)
    x = batch(13, 50, 7)
    x = (x[0], x[1], x[2] * 4.0)                     # a louder batch: a scale calibrated on it would differ
    return dict(cfgs=cfgs, fam=fam, Y=y, X=x, steps=2, cache={})


def _run(sdxl, dev, batches, *, ff="mx", graph=None, monkeypatch=None):
    from saspa_aug_amd.pipeline import StableDiffusionXLControlNetPipeline
    from tests.util import from_nhwc
    if graph is not None:
        monkeypatch.setenv("SASPA_GRAPH", graph)
    pipe = StableDiffusionXLControlNetPipeline(dict(sdxl["fam"]), sdxl["cfgs"])
    pipe.enable_fp8(True, ff=ff)
    pipe = pipe.to(dev, torch.bfloat16)
    outs = []
    for name in batches:
        ids1, ctrls, lat = sdxl[name]
        _, x, _ = pipe.generate_batch(ids1, None, ctrls, lat, sdxl["steps"], 0.0, 0.75, return_latents=True, prompt_ids_2=pipe.pad_ids_2(ids1))
        outs.append(x.clone())
    return pipe, [from_nhwc(o, 4) for o in outs], outs


def _mx_default(sdxl, dev):
    """ONE fresh ff="mx" pipeline whose first call is batch Y under the default (graph) mode, shared by the tests below."""
    if "mx" not in sdxl["cache"]:
        sdxl["cache"]["mx"] = _run(sdxl, dev, ["Y"])
    return sdxl["cache"]["mx"]


def test_model_mx_mode_vs_oracle(sdxl, dev):
    from oracle import pipeline as OP
    pipe, (lat_mx,), _ = _mx_default(sdxl, dev)
    for net in (pipe.unet, pipe.controlnet):
        assert len(net.fp8_blocks) > 0 and net.fp8_ff_mx == net.fp8_blocks       # every fp8 block runs the MX pair
        assert net.fp8_ffout == {}
        assert not any(k.endswith(".ff.scale") or k.endswith(".ff.amax") for k in net.p)
    pc, (lat_cal,), _ = _run(sdxl, dev, ["Y"], ff="calibrated")
    assert pc.unet.fp8_ff_mx == set() and len(pc.unet.fp8_ffout) == len(pc.unet.fp8_blocks)
    ids1, ctrls, lat = sdxl["Y"]
    ids2 = pipe.pad_ids_2(ids1)
    ref = torch.cat([OP.sdxl_controlnet_pipeline(sdxl["fam"], sdxl["cfgs"], torch.from_numpy(ids1[i:i + 1]), torch.from_numpy(ids2[i:i + 1]),
                                                 ctrls[i], lat[i:i + 1].float(), sdxl["steps"], return_latents=True)[1] for i in range(len(ids1))])
    rel = lambda t: ((t - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()     # noqa: E731
    e_mx, e_cal = rel(lat_mx), rel(lat_cal)
    print(f"\nSDXL (reduced width) final latents vs oracle, rms-rel: fp8 ff='mx' {e_mx:.3e}, ff='calibrated' {e_cal:.3e}")
    assert e_mx < 8e-2, (e_mx, e_cal)


def test_mode_from_the_environment(sdxl, dev, monkeypatch):
    from saspa_aug_amd.pipeline import StableDiffusionXLControlNetPipeline
    monkeypatch.setenv("SASPA_FP8", "1")
    monkeypatch.setenv("SASPA_FP8_FF", "mx")
    pipe = StableDiffusionXLControlNetPipeline(dict(sdxl["fam"]), sdxl["cfgs"]).to(dev, torch.bfloat16)
    assert len(pipe.unet.fp8_ff_mx) > 0 and pipe.unet.fp8_ff_mx == pipe.unet.fp8_blocks and pipe.controlnet.fp8_ffout == {}
    monkeypatch.setenv("SASPA_FP8_FF", "block")
    with pytest.raises(ValueError):
        StableDiffusionXLControlNetPipeline(dict(sdxl["fam"]), sdxl["cfgs"]).to(dev, torch.bfloat16)


def test_first_call_under_graph_equals_eager(sdxl, dev, monkeypatch):
    """Property 1: a fresh pipeline whose first call replays a captured step == a fresh pipeline that launches every kernel from
    Python, bit for bit."""
    from saspa_aug_amd.pipeline import graphs_enabled
    assert graphs_enabled()
    _, _, (g,) = _mx_default(sdxl, dev)
    _, _, (e,) = _run(sdxl, dev, ["Y"], graph="0", monkeypatch=monkeypatch)
    assert not graphs_enabled()
    assert torch.equal(g, e)


def test_no_state_from_an_earlier_batch(sdxl, dev):
    """Property 2: Y after X on one fresh pipeline == Y alone on another, bit for bit (nothing is measured on the first batch)."""
    _, _, (alone,) = _mx_default(sdxl, dev)
    _, _, (_, after) = _run(sdxl, dev, ["X", "Y"])
    assert torch.equal(alone, after)


def test_transformer_captured_cold(sdxl, dev):
    """A transformer of a fresh UNet captured into a graph WITHOUT ever having run (the calibrated mode raises there: its scale is
    measured by an eager launch; the pipelines always run one eager step first, so only a direct capture shows it): the MX mode
    captures, and the replay equals an eager run of another fresh UNet bit for bit."""
    cfgs, fam = sdxl["cfgs"], sdxl["fam"]
    ctx = _rand(2, 77, cfgs["unet"]["ctx_dim"], seed=5).to(dev, torch.bfloat16)

    def fresh(ff):
        net = models.UNet(dict(fam["unet"]), cfgs["unet"], dev, torch.bfloat16, fp8=True, fp8_ff=ff)
        net.prepare_context(ctx)
        pfx = next(p for p in net.tr_info if any(t.startswith(p) for t in net.fp8_blocks))
        c = net.p[pfx + ".norm.g"].numel()
        return net, pfx, (_rand(2, 8, 8, c, seed=6) * 0.5).to(dev, torch.bfloat16)

    net, pfx, x = fresh("mx")
    assert any(t.startswith(pfx) for t in net.fp8_ff_mx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = net.transformer(pfx, x)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    net2, pfx2, x2 = fresh("mx")
    assert pfx2 == pfx and torch.equal(x, x2)
    assert torch.equal(out, net2.transformer(pfx, x2))
