"""MX-fp8 3x3 convs (opt-in fp8 conv path of the resnets): the quantising GroupNorm against the block-exponent rule restated in
Python, and the block-scaled conv against a float64 reference on the dequantised operands (tests/errbudget.py), with negative
controls that the same check must reject."""
import math

import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from tests.errbudget import LIMITS, UNIT_BF16, check_budget, fmt, rejects
from tests.test_mxfp8_host import mx_exponent

pytestmark = pytest.mark.gpu
SILU, NONE = ops.ACT_SILU, ops.ACT_NONE


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- quantiser
def _gn_reference_y(x, gamma, beta, groups, eps, act):
    """y of the apply pass in fp32 (scale / shift per channel from fp64 statistics of the stored bf16 values)."""
    b, h, w, c = x.shape
    xd = x.double().reshape(b, h * w, groups, c // groups)
    mean = xd.mean(dim=(1, 3))
    var = (xd * xd).mean(dim=(1, 3)) - mean * mean
    rstd = (1.0 / torch.sqrt(var.clamp_min(0) + eps)).float()
    mean = mean.float()
    cpg = c // groups
    sc = gamma.float()[None] * rstd.repeat_interleave(cpg, dim=1)
    sh = beta.float()[None] - mean.repeat_interleave(cpg, dim=1) * sc
    y = x.float().reshape(b, h * w, c) * sc[:, None] + sh[:, None]
    if act == SILU:
        y = y * torch.sigmoid(y)
    return y.reshape(b, h, w, c)


def _check_quant(q, qs, y):
    b, h, w, c = y.shape
    blocks = y.reshape(b, h, w, c // 32, 32)
    amax = blocks.abs().amax(-1)
    e_ref = torch.tensor([mx_exponent(a) for a in amax.reshape(-1).tolist()], dtype=torch.int32).reshape(amax.shape)
    e_got = qs.cpu().to(torch.int32) - 127
    assert torch.equal(e_got, e_ref), f"{(e_got != e_ref).sum().item()} block exponents differ"
    want = (blocks * torch.exp2(-e_ref.float())[..., None]).reshape(b, h, w, c).to(torch.float8_e4m3fn).view(torch.uint8)
    got = q.cpu()
    diff = got != want
    assert diff.float().mean().item() < 1e-3, diff.float().mean().item()           # last-bit fp32 differences only
    if diff.any():
        assert ((got[diff].to(torch.int32) - want[diff].to(torch.int32)).abs() <= 1).all()
    return e_ref


@pytest.mark.parametrize("c0,c1,act,hw", [(320, 0, SILU, (16, 16)), (640, 0, NONE, (9, 13)), (320, 640, SILU, (8, 24)),
                                          (1280, 1280, SILU, (4, 4))])
def test_quantiser_statistics_pass(dev, c0, c1, act, hw):
    h, w = hw
    x = (torch.randn(2, h, w, c0, generator=_g(1)) * 3 + 1).bfloat16()
    x2 = (torch.randn(2, h, w, c1, generator=_g(2)) * 0.5 - 2).bfloat16() if c1 else None
    c = c0 + c1
    gamma = 1 + 0.5 * torch.randn(c, generator=_g(3))
    beta = 0.3 * torch.randn(c, generator=_g(4))
    gamma[32:64] = 0                                                                  # an all-zero block: exponent 0, bytes 0
    beta[32:64] = 0
    q, qs = ops.groupnorm_quant_mxfp8(x.to(dev), gamma.to(dev), beta.to(dev), 32, 1e-5, act,
                                      x2=None if x2 is None else x2.to(dev))
    xc = x if x2 is None else torch.cat([x, x2], -1)
    e = _check_quant(q, qs, _gn_reference_y(xc, gamma, beta, 32, 1e-5, act))
    assert (e[..., 1] == 0).all() and (q.cpu()[..., 32:64] == 0).all()
    # an image quantised alone: the same bytes as its slice of the batch
    q1, qs1 = ops.groupnorm_quant_mxfp8(x[1:].to(dev), gamma.to(dev), beta.to(dev), 32, 1e-5, act,
                                        x2=None if x2 is None else x2[1:].to(dev))
    assert torch.equal(q1, q[1:]) and torch.equal(qs1, qs[1:])


def test_quantiser_epilogue_statistics(dev):
    """Statistics left by the producing conv's epilogue (gn_unit): the quantiser reads them as groupnorm does."""
    src = torch.randn(2, 16, 16, 320, generator=_g(5)).bfloat16().to(dev)
    wc = W.pack_conv(torch.randn(320, 320, 3, 3, generator=_g(6)) / math.sqrt(2880)).to(dev, torch.bfloat16)
    x = ops.conv(src, wc, kh=3, kw=3, pad=1, gn_unit=10)
    assert hasattr(x, "saspa_gn")
    gamma = (1 + 0.2 * torch.randn(320, generator=_g(7))).to(dev)
    beta = (0.1 * torch.randn(320, generator=_g(8))).to(dev)
    q, qs = ops.groupnorm_quant_mxfp8(x, gamma, beta, 32, 1e-5, SILU)
    _check_quant(q, qs, _gn_reference_y(x.cpu(), gamma.cpu(), beta.cpu(), 32, 1e-5, SILU))
    # the same values through the statistics pass
    q2, qs2 = ops.groupnorm_quant_mxfp8(x.clone(), gamma, beta, 32, 1e-5, SILU)
    assert (q2 != q).float().mean().item() < 1e-3 and torch.equal(qs2, qs)


def test_quantiser_exponent_edges(dev):
    """Blocks whose maximum sits exactly on the rule's edges.  gamma = 0 makes y = beta, so each block's values are exact: 448 * 2^k
    (fits at k), its fp32 neighbours above (k + 1) and below (k), fp32 subnormals and the bottom of the E8M0 range (clamped at -127),
    zero, and the top of the fp32 range."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)                            # noqa: E731
    up = lambda v: torch.nextafter(f32(v), f32(math.inf)).item()                     # noqa: E731
    down = lambda v: torch.nextafter(f32(v), f32(0.0)).item()                        # noqa: E731
    edges = [448.0, up(448.0), down(448.0), 448.0 * 2 ** -3, up(448.0 * 2 ** -3), 448.0 * 2 ** 5, down(448.0 * 2 ** 5),
             448.0 * 2 ** -127, up(448.0 * 2 ** -127), 2.0 ** -130, 2.0 ** -149, 0.0, 3.0e38, 1.0]
    nb = len(edges)
    beta = torch.zeros(nb, 32)
    for j, v in enumerate(edges):
        beta[j, 0] = -v if j % 2 and v else v                                        # the maximum of |y|, either sign
        beta[j, 1:] = f32(v) * torch.linspace(0.05, 0.9, 31)                         # the rest below it (no signed zeros)
    beta = beta.reshape(-1)
    c = 32 * nb
    x = torch.randn(2, 8, 16, c, generator=_g(22)).bfloat16()
    gamma = torch.zeros(c)
    q, qs = ops.groupnorm_quant_mxfp8(x.to(dev), gamma.to(dev), beta.to(dev), nb, 1e-5, NONE)
    y = _gn_reference_y(x, gamma, beta, nb, 1e-5, NONE)
    assert torch.equal(y, beta.expand_as(y))                                        # the reference forms y = beta exactly too
    e = _check_quant(q, qs, y)
    want_e = torch.tensor([mx_exponent(abs(v)) for v in edges], dtype=torch.int32)
    assert torch.equal(e[0, 0, 0], want_e) and want_e.tolist()[:9] == [0, 1, 0, -3, -2, 5, 5, -127, -126]
    want = (y.reshape(2, 8, 16, nb, 32) * torch.exp2(-want_e.float())[:, None]).reshape(y.shape).to(torch.float8_e4m3fn)
    assert torch.equal(q.cpu(), want.view(torch.uint8))                              # exact values: every byte, no slack


# ------------------------------------------------------------------------------------------------------------------ conv
def _operands(b, h, w, c, n, seed, spread=20):
    """Random e4m3 activations with an exponent per (pixel, block) drawn from [-spread, spread] (a wrong scale-to-lane association
    moves an output by up to 2^40), e4m3 weights with per-channel scales, fp32 bias / row vector, bf16 residual."""
    g = _g(seed)
    qv = (torch.randn(b, h, w, c, generator=g) * 100).clamp(-448, 448).to(torch.float8_e4m3fn)
    qs = (127 + torch.randint(-spread, spread + 1, (b, h, w, c // 32), generator=g)).to(torch.uint8)
    wt = torch.randn(n, c, 3, 3, generator=g) / math.sqrt(9 * c)
    w8, sw = W.pack_conv_mxfp8(wt)
    return qv.view(torch.uint8), qs, w8, sw


def _deq_act(q, qs):
    b, h, w, c = q.shape
    v = q.view(torch.float8_e4m3fn).double().reshape(b, h, w, c // 32, 32)
    return (v * torch.exp2(qs.double() - 127)[..., None]).reshape(b, h, w, c)


def _reference(xd, wd, bias=None, rowvec=None, residual=None):
    """float64 conv (NHWC in / out) and the GEMM magnitude of every output."""
    c = xd.shape[-1]
    n = wd.shape[0]
    w4 = wd[:, :9 * c].reshape(n, 3, 3, c).permute(0, 3, 1, 2)
    x4 = xd.permute(0, 3, 1, 2)
    ref = F.conv2d(x4, w4, padding=1).permute(0, 2, 3, 1)
    s = F.conv2d(x4.abs(), w4.abs(), padding=1).permute(0, 2, 3, 1)
    if bias is not None:
        ref, s = ref + bias.double(), s + bias.double().abs()
    if rowvec is not None:
        ref, s = ref + rowvec.double()[:, None, None], s + rowvec.double().abs()[:, None, None]
    if residual is not None:
        ref, s = ref + residual.double(), s + residual.double().abs()
    return ref, s.clamp_min(1e-30)


def _run(dev, q, qs, w8, sw, bias=None, rowvec=None, residual=None, gn_unit=None):
    t = lambda v: None if v is None else v.to(dev)                                   # noqa: E731
    return ops.conv3x3_mxfp8(t(q), t(qs), t(w8), t(sw), t(bias), rowvec=t(rowvec), residual=t(residual), gn_unit=gn_unit)


@pytest.mark.parametrize("b,h,w,c,n", [(1, 64, 88, 320, 320), (2, 16, 16, 640, 640), (1, 24, 20, 960, 640), (1, 16, 16, 1280, 1280),
                                       (1, 12, 12, 1920, 640), (1, 12, 12, 2560, 1280), (3, 7, 9, 320, 1280), (1, 8, 16, 640, 320)])
def test_conv_vs_float64(dev, b, h, w, c, n):
    q, qs, w8, sw = _operands(b, h, w, c, n, seed=c + n + h)
    g = _g(9)
    bias = torch.randn(n, generator=g)
    rowvec = torch.randn(b, n, generator=g)
    residual = torch.randn(b, h, w, n, generator=g).bfloat16()
    out = _run(dev, q, qs, w8, sw, bias, rowvec, residual, gn_unit=10)
    xd = _deq_act(q, qs)
    wd = W.dequantize_fp8(w8, sw).double()
    ref, s = _reference(xd, wd, bias, rowvec, residual)
    st = check_budget(out, ref, s, UNIT_BF16, limits=LIMITS["gemm"], what=f"mxfp8 conv {b}x{h}x{w} {c}->{n}")
    print(f"mxfp8 conv {b}x{h}x{w} {c}->{n}: {fmt(st)}")
    # epilogue GroupNorm statistics: the sums of the STORED values per 128-row block and unit of 10 channels
    if (h * w) % 128 == 0:
        stats = out.saspa_gn[0].cpu().double()
        o = out.cpu().double().reshape(-1, 128, n // 10, 10)
        want = torch.stack([o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], -1)
        assert torch.allclose(stats, want, rtol=1e-4, atol=1e-3 * want[..., 1].abs().max().item() ** 0.5)


def test_conv_plain_and_negative_controls(dev):
    b, h, w, c, n = 1, 20, 28, 320, 320
    q, qs, w8, sw = _operands(b, h, w, c, n, seed=11)
    # one block dominant: its exponent is the largest of the tensor, so an off-by-one there is far outside the budget
    qs[0, 5, 7, 3] = 127 + 24
    out = _run(dev, q, qs, w8, sw)
    xd = _deq_act(q, qs)
    wd = W.dequantize_fp8(w8, sw).double()
    ref, s = _reference(xd, wd)
    check_budget(out, ref, s, UNIT_BF16, limits=LIMITS["gemm"], what="mxfp8 conv, no epilogue terms")
    lim = LIMITS["gemm"]
    qs_bad = qs.clone()
    qs_bad[0, 5, 7, 3] += 1
    ref_b, s_b = _reference(_deq_act(q, qs_bad), wd)
    assert rejects(out, ref_b, s_b, UNIT_BF16, limits=lim), "one block's exponent off by one"
    ref_b, s_b = _reference(xd, torch.roll(wd[:, :9 * c], c, dims=1))
    assert rejects(out, ref_b, s_b, UNIT_BF16, limits=lim), "weights shifted by one tap"
    wd_cut = wd.clone()
    wd_cut[:, (wd.shape[1] - 128):] = 0
    ref_b, s_b = _reference(xd, wd_cut)
    assert rejects(out, ref_b, s_b, UNIT_BF16, limits=lim), "last K-tile dropped"


def test_end_to_end_against_bf16_layer(dev):
    """Quantiser + MX conv against the unquantised bf16 layer (GroupNorm + SiLU + conv): the quantisation error only."""
    x = torch.randn(2, 16, 16, 640, generator=_g(12)).bfloat16().to(dev)
    gamma = (1 + 0.2 * torch.randn(640, generator=_g(13))).to(dev)
    beta = (0.1 * torch.randn(640, generator=_g(14))).to(dev)
    wt = torch.randn(320, 640, 3, 3, generator=_g(15)) / math.sqrt(9 * 640)
    bias = (0.1 * torch.randn(320, generator=_g(16))).to(dev)
    w8, sw = W.pack_conv_mxfp8(wt)
    q, qs = ops.groupnorm_quant_mxfp8(x, gamma, beta, 32, 1e-5, SILU)
    got = ops.conv3x3_mxfp8(q, qs, w8.to(dev), sw.to(dev), bias).float()
    hn = ops.groupnorm(x, gamma, beta, 32, 1e-5, SILU)
    want = ops.conv(hn, W.pack_conv(wt).to(dev, torch.bfloat16), bias, kh=3, kw=3, pad=1).float()
    rel = ((got - want).norm() / want.norm()).item()
    print(f"MX-fp8 vs bf16 layer: rms-rel {rel:.4f}")
    assert rel < 0.05                                                                # e4m3 on both operands: ~2-3 % rms


def test_conv_argument_checks(dev):
    q, qs, w8, sw = (t.to(dev) for t in _operands(2, 8, 8, 320, 320, seed=3))
    with pytest.raises(ValueError):
        ops.conv3x3_mxfp8(q, qs, w8, sw, torch.zeros(320, device=dev, dtype=torch.bfloat16))         # bias read as fp32 bits
    with pytest.raises(ValueError):
        ops.conv3x3_mxfp8(q, qs, w8, sw.double())
    with pytest.raises(ValueError):
        ops.conv3x3_mxfp8(q, qs, w8, sw, rowvec=torch.zeros(3, 320, device=dev))                     # neither 1 nor batch rows
    with pytest.raises(ValueError):
        ops.conv3x3_mxfp8(q, qs, torch.cat([w8, torch.zeros_like(w8[:, :128])], 1).contiguous(), sw)  # K padded too far
    assert ops.conv3x3_mxfp8(q, qs, w8, sw, rowvec=torch.zeros(1, 320, device=dev)).shape == (2, 8, 8, 320)


def test_graph_replay_bit_identical(dev):
    x = torch.randn(2, 16, 16, 320, generator=_g(17)).bfloat16().to(dev)
    gamma = (1 + 0.2 * torch.randn(320, generator=_g(18))).to(dev)
    beta = (0.1 * torch.randn(320, generator=_g(19))).to(dev)
    w8, sw = W.pack_conv_mxfp8(torch.randn(640, 320, 3, 3, generator=_g(20)) / math.sqrt(2880))
    w8, sw = w8.to(dev), sw.to(dev)
    rv = torch.randn(2, 640, generator=_g(21)).to(dev)

    def step():
        q, qs = ops.groupnorm_quant_mxfp8(x, gamma, beta, 32, 1e-5, SILU)
        return ops.conv3x3_mxfp8(q, qs, w8, sw, rowvec=rv, gn_unit=10)
    eager = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
