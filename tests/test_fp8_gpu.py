"""fp8 (OCP e4m3) W8A8 linears of the SDXL transformer blocks (BASELINE.json configs[4]): the quantising
LayerNorm and the 128x128x128 fp8 GEMM against the float64 references of tests/fp8_ref.py (bit equality on exact operands, the
rounding-error budgets of tests/errbudget.py on random ones, an exact byte rule for the quantisation), and the quantisation error
itself against the unquantised layer."""
import math

import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from tests import fp8_ref as R
from tests.errbudget import LIMITS, UNIT_BF16, check_budget, fmt, geglu_gemm_scale, gemm_scale, rejects

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _check(got, ref, s, family, what, unit=UNIT_BF16):
    st = check_budget(got, ref, s, unit, limits=LIMITS[family], what=what)
    print(f"\n[budget] {family:5s} {what}: {fmt(st)}")
    return st


def _control(got, ref, s, family, what, unit=UNIT_BF16):
    assert rejects(got, ref, s, unit, limits=LIMITS[family]), f"negative control not rejected: {what}"
    print(f"\n[control rejected] {family:5s} {what}")


# ------------------------------------------------------------------ quantising LayerNorm
def _ln_check(x, g, b, q, sc, what):
    """Row scale to R.LN_SCALE_RTOL (4x the fp32 emulation's worst case against float64, 6.73e-7: tests/test_fp8_ref_host.py), every
    byte within half an e4m3 ulp at its own binade of y64 / scale (R.ln_quant_violations: no excluded share; rejects round-toward-
    zero on half the elements)."""
    y, want_sc, mag = R.ln_quant_ref(x, g, b)
    rel = ((sc.cpu().double() - want_sc) / want_sc).abs().max().item()
    print(f"\n[ln-quant] {what}: row scale off by {rel:.2e} relative (granted {R.LN_SCALE_RTOL:.2e})")
    assert rel <= R.LN_SCALE_RTOL, rel
    bad = R.ln_quant_violations(q.cpu(), sc.cpu(), y, mag)
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[0].tolist())
    return y


@pytest.mark.parametrize("rows,c", R.LN_CASES)
def test_layernorm_quant_fp8(dev, rows, c):
    """(5, 8): one chunk, 63 idle lanes, a ragged block of waves; (77, 640): rows no multiple of 4; (4, 2048): the register limit;
    (1, 1280): a single row; the production-sized cases.  Row 1 is constant (variance 0: y = beta), row 2 carries one 1000 x outlier
    (R.ln_case)."""
    x, g, b = R.ln_case(_rand, rows, c)
    q, sc = ops.layernorm_quant_fp8(x.to(dev), g.to(dev), b.to(dev))
    assert q.dtype == torch.uint8 and q.shape == (rows, c) and sc.shape == (rows,)
    _ln_check(x, g, b, q, sc, f"{rows}x{c}")


def test_layernorm_quant_fp8_zero_affine_and_row_pitch(dev):
    x, g, b = R.ln_case(_rand, 77, 640, seed=3)
    q, sc = ops.layernorm_quant_fp8(x.to(dev), torch.zeros_like(g).to(dev), torch.zeros_like(b).to(dev))
    assert (sc == 1.0).all() and (q & 0x7f == 0).all()                      # gamma = beta = 0: scale 1.0, all bytes 0
    # the outlier row with beta = 0 and gamma 2^-7 off the outlier's channel: everything but the outlier lands in e4m3 subnormals or zero
    g2, b2 = R.ln_one_channel_affine(640)
    q2, sc2 = ops.layernorm_quant_fp8(x.to(dev), g2.to(dev), b2.to(dev))
    _ln_check(x, g2, b2, q2, sc2, "77x640, gamma 2^-7 off one channel")
    d2 = R.e4m3_decode(q2[2].cpu()).abs()
    assert d2.max().item() == 448.0 and (d2 < 2.0 ** -6).sum().item() >= 600 and (d2 > 0).sum().item() > 320
    # x as a view of a wider buffer (ldx > C); the filler would move every mean
    buf = torch.full((77, 648), 1000.0, device=dev, dtype=torch.bfloat16)
    buf[:, :640] = x.to(dev)
    xv = buf[:, :640]
    assert xv.stride(0) == 648
    q1, sc1 = ops.layernorm_quant_fp8(xv, g.to(dev), b.to(dev))
    q0, sc0 = ops.layernorm_quant_fp8(x.to(dev), g.to(dev), b.to(dev))
    assert torch.equal(q1, q0) and torch.equal(sc1, sc0)
    _ln_check(x, g, b, q1, sc1, "77x640 in a 648-wide buffer")


@pytest.mark.parametrize("c", [2056, 12])
def test_layernorm_quant_fp8_refuses_unsupported_widths(dev, c):
    x = torch.zeros(4, c, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="saspa_layernorm_quant_fp8"):
        ops.layernorm_quant_fp8(x, torch.ones(c, device=dev), torch.zeros(c, device=dev))


# ------------------------------------------------------------------ the fp8 GEMM
# (M, K, N): one row, one K-tile and no prefetch | both ring stages | the ring wraps, 2 ragged rows in the second row-tile | 9 tiles:
# the XCD remap has a remainder, nbn = 3 in the tile decode
EXACT_SHAPES = [(1, 128, 128), (127, 256, 128), (130, 384, 256), (257, 128, 384)]
BUDGET_SHAPES = EXACT_SHAPES + [(515, 640, 256)]
CODE_448 = 0x7e


def _launch(dev, op, *, residual=False, geglu=False, bias=True, sa=None, a=None, w=None, res=None, **kw):
    a8 = R.to_codes(op["a"]).to(dev) if a is None else a
    w8 = R.to_codes(op["w"]).to(dev) if w is None else w
    r = (op["res"].to(dev, torch.bfloat16) if res is None else res) if residual else None
    return ops.linear_fp8(a8, (op["sa"] if sa is None else sa).float().to(dev), w8, op["sw"].float().to(dev),
                          op["bias"].float().to(dev) if bias else None, residual=r, act=ops.ACT_GEGLU if geglu else ops.ACT_NONE, **kw)


def _assert_exact(got, want, what):
    """Bit equality with the emulation (both are bf16 values)."""
    got = got.cpu().double()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements differ, first {i}: got {got[i].item()!r} want {want[i].item()!r}")
    print(f"\n[bit-equal] fp8 gemm {what}")


@pytest.mark.parametrize("m,k,n", EXACT_SHAPES)
def test_gemm_fp8_exact_operands_bit_equal(dev, m, k, n):
    """Integer e4m3 codes, power-of-two scales, bias on the scales' grid (R.exact_operands): every sum is exact in fp32 whatever its
    order, so the plain output and the residual output rne(rne(v) + r) are known to the bit."""
    op = R.exact_operands(_rand, m, k, n, 601)
    _assert_exact(_launch(dev, op), R.gemm_f8_emul(op), f"plain {m}x{k}x{n}")
    _assert_exact(_launch(dev, op, residual=True), R.gemm_f8_emul(op, residual=True), f"residual {m}x{k}x{n}")
    _assert_exact(_launch(dev, op, bias=False), R.gemm_f8_emul(dict(op, bias=torch.zeros(n, dtype=torch.float64))), f"no bias {m}x{k}x{n}")


def test_gemm_fp8_exact_operands_pitches_and_single_scale(dev):
    """lda, ldw and ldr come from strides: A inside a [M, K + 16] byte buffer and W inside [N, K + 128], both filled with the code of
    448, the residual inside [M, N + 8] filled with 2^100 -- one over-read shows.  Then ONE activation scale for all rows."""
    m, k, n = 130, 384, 256
    op = R.exact_operands(_rand, m, k, n, 601)
    abuf = torch.full((m, k + 16), CODE_448, dtype=torch.uint8, device=dev)
    wbuf = torch.full((n, k + 128), CODE_448, dtype=torch.uint8, device=dev)
    rbuf = torch.full((m, n + 8), 2.0 ** 100, dtype=torch.bfloat16, device=dev)
    abuf[:, :k], wbuf[:, :k], rbuf[:, :n] = R.to_codes(op["a"]).to(dev), R.to_codes(op["w"]).to(dev), op["res"].to(dev, torch.bfloat16)
    av, wv, rv = abuf[:, :k], wbuf[:, :k], rbuf[:, :n]
    assert av.stride(0) == k + 16 and wv.stride(0) == k + 128 and rv.stride(0) == n + 8
    _assert_exact(_launch(dev, op, a=av, w=wv), R.gemm_f8_emul(op), "plain, A and W inside wider buffers")
    _assert_exact(_launch(dev, op, residual=True, a=av, w=wv, res=rv), R.gemm_f8_emul(op, residual=True),
                  "residual, A, W and the residual inside wider buffers")
    one = torch.tensor([2.0 ** -3], dtype=torch.float64)
    op1 = dict(op, sa=one.expand(m).clone())
    got1 = _launch(dev, op, residual=True, sa=one)
    assert torch.equal(got1, _launch(dev, op1, residual=True))
    _assert_exact(got1, R.gemm_f8_emul(op1, residual=True), "ONE activation scale for all rows")
    # M = 1 with a 1-element scale is the per-row form
    opm = R.exact_operands(_rand, 1, 128, 128, 601)
    _assert_exact(_launch(dev, opm, sa=opm["sa"][:1]), R.gemm_f8_emul(opm), "M = 1, 1-element scale")


@pytest.mark.parametrize("m,k,n", EXACT_SHAPES)
def test_gemm_fp8_geglu_exact_operands(dev, m, k, n):
    """GEGLU on exact operands: value and gate entering the GELU are known exactly (the bf16 tile), so the output is held to float64
    hv * gelu_erf(hg) under the elem budget (which separates tanh-GELU and truncation: tests/test_errbudget.py); amax to 2^-20 of the
    emulation's (about ten fp32 operations of the polynomial at 2^-24 each); the fp8 emission under the e4m3 budget, its bytes equal
    to the emulation's except for R.BYTE_SHARE_CAP of them, by one code."""
    op = R.exact_operands(_rand, m, k, n, 611, geglu=True)
    tile = R.gemm_f8_emul(op)
    ref, s = R.geglu_exact_ref(tile)
    hg = R.untile(tile)[1]
    assert m == 1 or (hg.min().item() < -3 and hg.max().item() > 3)            # the gates cover the bend of the GELU
    amax = torch.zeros(1, device=dev)
    got = _launch(dev, op, geglu=True, amax=amax)
    assert got.shape == (m, n // 2)
    _check(got.cpu(), ref, s, "elem", f"fp8 geglu exact operands {m}x{k}x{n}")
    assert torch.equal(got, _launch(dev, op, geglu=True))                      # measuring does not change the result
    emu, want_amax = R.gemm_f8_emul(op, geglu=True, want_amax=True)
    rel = abs(amax.item() - want_amax) / want_amax
    print(f"\n[amax] fp8 geglu {m}x{k}x{n}: {amax.item():.9g} against {want_amax:.9g}, {rel:.2e} relative")
    assert rel <= 2.0 ** -20
    big = torch.full((1,), 2.0 * want_amax + 1.0, device=dev)
    _launch(dev, op, geglu=True, amax=big)
    assert big.item() == float(torch.tensor(2.0 * want_amax + 1.0, dtype=torch.float32))     # a larger value is left alone
    # fp8 emission under the calibrated power-of-two scale
    scale = ops.fp8_pow2_scale(amax)
    osc = scale.item()
    assert osc == R.pow2_scale(want_amax)
    q = _launch(dev, op, geglu=True, out_fp8_scale=scale)
    assert q.dtype == torch.uint8 and q.shape == (m, n // 2)
    _check(R.e4m3_decode(q.cpu()) * osc, ref, R.e4m3_scale(ref, osc), "e4m3", f"fp8 emission {m}x{k}x{n} scale {osc:g}", unit=R.UNIT_E4M3)
    want_q = R.gemm_f8_emul(op, geglu=True, out_scale=osc)
    dist = R.code_distance(q.cpu(), want_q)
    share = (dist > 0).double().mean().item()
    print(f"\n[bytes] fp8 emission {m}x{k}x{n}: {share:.2e} of the bytes differ from the emulation's (cap {R.BYTE_SHARE_CAP:.0e})")
    assert dist.max().item() <= 1 and share <= R.BYTE_SHARE_CAP
    # negative controls on the same outputs
    _control(R.e4m3_decode(q.cpu()) * osc * 2, ref, R.e4m3_scale(ref, osc), "e4m3", "decoded under twice the scale", unit=R.UNIT_E4M3)
    if m > 1:
        _control(R.e4m3_decode(R.gemm_f8_emul(op, geglu=True, out_scale=osc, to_bytes=R.e4m3_bytes_rtz)) * osc, ref, R.e4m3_scale(ref, osc),
                 "e4m3", "emulation rounding toward zero", unit=R.UNIT_E4M3)
        _control(R.gemm_f8_emul(op, geglu=True, gelu="tanh"), ref, s, "elem", "emulation with tanh-GELU")


def test_gemm_fp8_amax_ignores_the_pad_rows(dev):
    """M = 130: the 126 pad rows of the second row-tile see sa = 0, hence v = bias.  Column 0 gets a bias whose gated value exceeds
    every real row's (non-negative activations against a row of -1 codes pull every real value BELOW the bias; the gate's weights are
    zero): were the pad rows to enter amax, it would be that value."""
    m, k, n = 130, 384, 256
    op = R.exact_operands(_rand, m, k, n, 621, geglu=True)
    op["a"] = op["a"].abs()
    op["a"][:, 0] = 1.0
    op["w"][0], op["w"][64] = -1.0, 0.0
    op["bias"][0], op["bias"][64] = 64.0, 6.0
    pad_value = 64.0 * F.gelu(torch.tensor(6.0, dtype=torch.float64)).item()
    emu, want_amax = R.gemm_f8_emul(op, geglu=True, want_amax=True)
    assert want_amax < 0.999 * pad_value, (want_amax, pad_value)
    amax = torch.zeros(1, device=dev)
    got = _launch(dev, op, geglu=True, amax=amax)
    assert abs(amax.item() - want_amax) <= 2.0 ** -20 * want_amax, (amax.item(), want_amax, pad_value)
    ref, s = R.geglu_exact_ref(R.gemm_f8_emul(op))
    _check(got.cpu(), ref, s, "elem", "fp8 geglu 130x384x256, a dominant bias in column 0")


def _random_controls(op, residual):
    """References a right result must be rejected against: the last K-tile zeroed, sa rolled by one row, sw rolled by 4 columns,
    the bias dropped on the last 8 columns."""
    n = op["w"].shape[0]
    a0 = op["a"].clone()
    a0[:, -R.KT:] = 0
    b0 = op["bias"].clone()
    b0[n - 8:] = 0
    out = [("last K-tile zeroed", dict(op, a=a0)), ("sw rolled by 4 columns", dict(op, sw=op["sw"].roll(4))),
           ("bias dropped on the last 8 columns", dict(op, bias=b0))]
    if op["a"].shape[0] > 1:                         # (one row: rolling sa changes nothing)
        out.append(("sa rolled by one row", dict(op, sa=op["sa"].roll(1))))
    return [(nm, R.gemm_f8_ref(o, residual=residual)[0]) for nm, o in out]


@pytest.mark.parametrize("m,k,n", BUDGET_SHAPES)
def test_gemm_fp8_budget(dev, m, k, n):
    """Random operands (R.random_operands: test_gemm_fp8's, with bias and residual at the size of the product) under the gemm
    budget, plain and residual forms, each with its negative controls."""
    op = R.random_operands(_rand, m, k, n, 631)
    for residual in (False, True):
        ref, s = R.gemm_f8_ref(op, residual=residual)
        tag = f"fp8 gemm {'residual' if residual else 'plain'} {m}x{k}x{n}"
        got = _launch(dev, op, residual=residual).cpu()
        _check(got, ref, s, "gemm", tag)
        for nm, wrong in _random_controls(op, residual):
            _control(got, wrong, s, "gemm", f"{tag} against the reference with {nm}")


@pytest.mark.parametrize("m,k,n,geglu,res", [(1000, 640, 640, False, True), (4096, 1280, 1280, False, False),
                                             (515, 640, 5120, True, False), (2048, 1280, 10240, True, False),
                                             (130, 128, 128, False, True)])
def test_gemm_fp8(dev, m, k, n, geglu, res):
    """The production sizes under the gemm budget (float64 reference on the quantised operands, with the kernel's rounding points:
    the bf16 tile before the residual / before the GELU)."""
    xq = torch.randn(m, k, generator=torch.Generator().manual_seed(4)).clamp(-3, 3)
    sa = 0.5 + torch.rand(m, generator=torch.Generator().manual_seed(5))
    xq8 = (xq * 100).to(torch.float8_e4m3fn)                          # arbitrary representable e4m3 values
    w = _rand(n, k, seed=6, scale=1 / math.sqrt(k))
    b = _rand(n, seed=7)
    if geglu:
        w, b = W.pack_geglu_tile(w, b, 128)
    wq, sw = W.quantize_fp8(w)
    r = _rand(m, n, seed=8).bfloat16() if res else None
    x64, w64 = xq8.double() * sa.double()[:, None], W.dequantize_fp8(wq, sw).double()
    ref = x64 @ w64.t() + b.double()
    s = gemm_scale(x64, w64, b, residual=r)
    if geglu:
        # un-pack: tile t = [values of features 64t .. 64t+63 | their gates]; value and gate are rounded to bf16 before the GELU
        hv, hg = R.untile(R.rne(ref))
        mv, mg = R.untile(s)
        ref, s = hv * F.gelu(hg), geglu_gemm_scale(hv, hg, mv, mg)
    if res:
        ref = R.rne(ref) + r.double()
    out = ops.linear_fp8(xq8.view(torch.uint8).to(dev), sa.to(dev), wq.to(dev), sw.to(dev), b.to(dev),
                         residual=None if r is None else r.to(dev), act=ops.ACT_GEGLU if geglu else ops.ACT_NONE)
    _check(out.cpu(), ref, s, "gemm", f"fp8 gemm {m}x{k}x{n}{' geglu' if geglu else ''}{' residual' if res else ''}")


@pytest.mark.parametrize("m,k,n", [(515, 640, 5120), (2048, 1280, 10240)])
def test_gemm_fp8_geglu_emits_fp8_under_a_tensor_scale(dev, m, k, n):
    """ABI 20: the GEGLU epilogue of saspa_gemm_fp8 with `amax` (calibration) and `out_fp8` (e4m3 bytes under ONE power-of-two
    scale).  The bf16-output launch of the same operands is the reference: amax = its largest magnitude (up to the bf16 rounding the
    reference carries), the dequantised bytes are within half an e4m3 ulp of it, a power-of-two change of the scale leaves the
    decoded values unchanged (the format is floating: the exponent shifts), a far-too-small scale saturates at +-448 instead of
    producing NaN bytes."""
    xq8 = (torch.randn(m, k, generator=torch.Generator().manual_seed(4)).clamp(-3, 3) * 100).to(torch.float8_e4m3fn).view(torch.uint8).to(dev)
    sa = (0.5 + torch.rand(m, generator=torch.Generator().manual_seed(5))).to(dev)
    w, b = W.pack_geglu_tile(_rand(n, k, seed=6, scale=1 / math.sqrt(k)), _rand(n, seed=7), 128)
    wq, sw = W.quantize_fp8(w)
    wq, sw, b = wq.to(dev), sw.to(dev), b.to(dev)
    ref = ops.linear_fp8(xq8, sa, wq, sw, b, act=ops.ACT_GEGLU).float()
    amax = torch.zeros(1, device=dev)
    again = ops.linear_fp8(xq8, sa, wq, sw, b, act=ops.ACT_GEGLU, amax=amax).float()
    assert torch.equal(ref, again)                                         # measuring does not change the bf16 result
    a = amax.item()
    assert abs(a - ref.abs().max().item()) <= 2 ** -8 * a
    scale = ops.fp8_pow2_scale(amax)
    sv = scale.item()
    assert math.log2(sv) == round(math.log2(sv)) and 16 * a / 448 <= sv < 32 * a / 448
    q = ops.linear_fp8(xq8, sa, wq, sw, b, act=ops.ACT_GEGLU, out_fp8_scale=scale)
    assert q.dtype == torch.uint8 and q.shape == (m, n // 2)
    deq = q.view(torch.float8_e4m3fn).float() * sv
    err = (deq - ref).abs()
    assert (err <= (0.0625 + 2 ** -8) * ref.abs() + sv * 2 ** -9 + 1e-6).all(), err.max().item()
    q4 = ops.linear_fp8(xq8, sa, wq, sw, b, act=ops.ACT_GEGLU, out_fp8_scale=scale / 4)
    d4 = q4.view(torch.float8_e4m3fn).float() * (sv / 4)
    big = ref.abs() > sv * 2 ** -4                                           # away from either scale's subnormal range
    assert torch.equal(d4[big], deq[big])
    qs = ops.linear_fp8(xq8, sa, wq, sw, b, act=ops.ACT_GEGLU, out_fp8_scale=scale / 4096)
    ds = qs.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(ds).all() and ds.abs().max().item() == 448.0
    # the output projection that reads the bytes: ONE scale for every row == the same scale spelled out per row
    w2q, sw2 = W.quantize_fp8(_rand(640, n // 2, seed=9, scale=1 / math.sqrt(n // 2)))
    r = _rand(m, 640, seed=10).bfloat16().to(dev)
    o1 = ops.linear_fp8(q, scale, w2q.to(dev), sw2.to(dev), residual=r)
    o2 = ops.linear_fp8(q, scale.expand(m).contiguous(), w2q.to(dev), sw2.to(dev), residual=r)
    assert torch.equal(o1, o2)


def test_fp8_gemm_refuses_fp8_output_outside_the_geglu_epilogue(dev):
    x8 = torch.zeros(128, 128, dtype=torch.uint8, device=dev)
    one = torch.ones(1, device=dev)
    with pytest.raises(ValueError):
        ops.linear_fp8(x8, one.expand(128).contiguous(), x8, one.expand(128).contiguous(), out_fp8_scale=one)


def test_fp8_linear_quantisation_error_vs_bf16_layer(dev):
    """LayerNorm -> Linear: W8A8 (per-token x per-channel scales) against the fp64 layer, next to the bf16 path's error."""
    m, c, n = 2048, 1280, 1280
    x = (_rand(m, c, seed=9) * 1.5 + 0.3).bfloat16()
    g, be = 1 + 0.1 * _rand(c, seed=10), 0.1 * _rand(c, seed=11)
    w = _rand(n, c, seed=12, scale=1 / math.sqrt(c))
    ref = F.layer_norm(x.double(), (c,), g.double(), be.double(), 1e-5) @ w.double().t()
    wq, sw = W.quantize_fp8(w)
    q, sc = ops.layernorm_quant_fp8(x.to(dev), g.to(dev), be.to(dev))
    o8 = ops.linear_fp8(q, sc, wq.to(dev), sw.to(dev)).float().cpu().double()
    o16 = ops.linear(ops.layernorm(x.to(dev), g.to(dev), be.to(dev)), w.bfloat16().to(dev)).float().cpu().double()[:, :n]
    rel = lambda y: ((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()     # noqa: E731
    print(f"LN -> linear {m}x{c}x{n}: rms-rel error fp8 {rel(o8):.3e}, bf16 {rel(o16):.3e}")
    assert rel(o8) < 4e-2 and rel(o16) < 6e-3


def test_sdxl_pipeline_fp8_vs_oracle_and_bf16(dev):
    """`enable_fp8()` on a reduced-width SDXL whose transformer widths are multiples of 128 (so the fp8 kernels really run):
    the W8A8 projections keep the 2-step trajectory within the bf16 path's distance class of the oracle, deterministically."""
    import numpy as np
    from oracle import pipeline as OP
    from oracle.canny import generate_canny_array
    from saspa_aug_amd import config as CFG
    from saspa_aug_amd.pipeline import StableDiffusionXLControlNetPipeline
    from saspa_aug_amd.synthetic import synthetic_image
    from tests.util import from_nhwc
    cfgs = CFG.tiny_xl(width=64)                                     # levels 1 / 2 carry the transformers: 128- and 256-wide
    fam = W.synth_family(cfgs, seed=2)
    b, res, steps = 2, 64, 2
    v = cfgs["text"]["vocab"]
    rs = np.random.RandomState(3)
    ids1 = np.full((b, 77), v - 1, np.int64)
    ids1[:, 0] = v - 2
    ids1[:, 1:9] = rs.randint(0, v - 2, (b, 8))
    ctrls = np.stack([generate_canny_array(synthetic_image(res, res, 30 + i), 120, 200) for i in range(b)])
    lat = torch.randn((b, 4, res // 8, res // 8), generator=torch.manual_seed(1), dtype=torch.float16)
    outs = {}
    for mode in ("bf16", "fp8"):
        pipe = StableDiffusionXLControlNetPipeline(dict(fam), cfgs)
        if mode == "fp8":
            pipe.enable_fp8()
        pipe = pipe.to(dev, torch.bfloat16)
        if mode == "fp8":
            assert len(pipe.unet.fp8_blocks) > 0 and len(pipe.controlnet.fp8_blocks) > 0
            # round 6 breadth: the fused self-attention projection and the feed-forward output projection too
            assert len(pipe.unet.fp8_qkv) == len(pipe.unet.fp8_blocks) and len(pipe.unet.fp8_ffout) == len(pipe.unet.fp8_blocks)
            assert not any(pipe.unet.fp8_ffout.values())                       # scales not calibrated before the first evaluation
        ids2 = pipe.pad_ids_2(ids1)
        out, x, img = pipe.generate_batch(ids1, None, ctrls, lat, steps, 0.0, 0.75, return_latents=True, prompt_ids_2=ids2)
        out2, _, _ = pipe.generate_batch(ids1, None, ctrls, lat, steps, 0.0, 0.75, return_latents=True, prompt_ids_2=ids2)
        assert torch.equal(out, out2)
        if mode == "fp8":
            assert all(pipe.unet.fp8_ffout.values()) and all(pipe.controlnet.fp8_ffout.values())
            sc = [pipe.unet.p[t + ".ff.scale"].item() for t in pipe.unet.fp8_ffout]
            assert all(v > 0 and math.log2(v) == round(math.log2(v)) for v in sc)    # calibrated powers of two
        outs[mode] = from_nhwc(x, 4)
    refs = [OP.sdxl_controlnet_pipeline(fam, cfgs, torch.from_numpy(ids1[i:i + 1]), torch.from_numpy(ids2[i:i + 1]), ctrls[i],
                                        lat[i:i + 1].float(), steps, return_latents=True)[1] for i in range(b)]
    ref = torch.cat(refs)
    rel = lambda y: ((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()     # noqa: E731
    e16, e8 = rel(outs["bf16"]), rel(outs["fp8"])
    print(f"SDXL (reduced width) final latents vs oracle, rms-rel: bf16 {e16:.3e}, fp8 projections {e8:.3e}")
    assert e16 < 3e-2 and e8 < 8e-2, (e16, e8)
