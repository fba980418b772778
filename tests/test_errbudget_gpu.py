"""The HIP kernels under the rounding-error budget (tests/errbudget.py) on the operands whose margins tests/test_errbudget.py proves
on the CPU: every case builds a float64 reference from the bf16 operands and its magnitude s_i, and check_budget asserts max / rms /
toward-zero bias / slope against the family's limits.  Each family also launches its kernel once with one argument perturbed (a
negative control: an ordinary valid launch) and asserts that the budget REJECTS that result against the unperturbed reference, so
every test here is shown to be able to fail on the hardware."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from tests.errbudget import (LIMITS, UNIT_BF16, UNIT_F32X3, attn_scale, check_budget, conv_scale, elem_scale, fmt, gemm_scale,
                             geglu_gemm_scale, norm_scale, rejects)
from tests.test_errbudget import (CFG_COEF, XA_C, XA_D, _attn_ref, _gemm_operands, _ln_ref, _norm_inputs, _rand, as_operands,
                                  as_ref, attn_operands, cfg_ddim_ref, ff_operands, ff_ref, gn_kernel_ref, mu_rstd, q, vt_tail,
                                  xattn_operands, xattn_ref)
from tests.util import from_nhwc, to_nhwc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LOG2E = 1.4426950408889634


def _check(got, ref, s, family, what, unit=UNIT_BF16):
    st = check_budget(got, ref, s, unit, limits=LIMITS[family], what=what)
    print(f"\n[budget] {family:5s} {what}: {fmt(st)}")
    return st


def _control(got, ref, s, family, what, unit=UNIT_BF16):
    assert rejects(got, ref, s, unit, limits=LIMITS[family]), f"negative control not rejected: {what}"
    print(f"\n[control rejected] {family:5s} {what}")


# ------------------------------------------------------------------ GEMM / conv
GEMM_SHAPES = [(300, 320, 960, 1), (129, 64, 40, 5), (77, 768, 320, 9), (1, 320, 1280, 13), (4096, 1280, 320, 17),
               (1024, 2560, 192, 21), (260, 320, 4, 25)]          # (N = 3 is a convolution-only shape: linear needs N % 4 == 0)


def _linear(dev, x, w, b, res, alpha, **kw):
    n = w.shape[0]
    out = ops.linear(x.to(dev, BF), w.to(dev, BF), b.float().to(dev), residual=res.to(dev, BF), alpha=alpha, act=ops.ACT_SILU, **kw)
    return out.cpu()[:, :n]


# SASPA_GEMM_AUTO / TILED / WIDE / WS (include/saspa_hip.h); WIDE needs channel counts that are multiples of 64, WS is pinned on the
# level-0 pointwise shape it serves
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("m,k,n,seed", GEMM_SHAPES)
def test_linear_budget(dev, m, k, n, seed, variant):
    if variant == 2 and (n % 64 or k % 64):
        pytest.skip("the wide kernel needs channel counts that are multiples of 64")
    if variant == 3 and (m, k, n) != (300, 320, 960):
        pytest.skip("WS is pinned on the level-0 pointwise shape")
    x, w, b, res = _gemm_operands(m, k, n, seed)
    alpha = 0.75
    ref = F.silu(alpha * (x @ w.t() + b)) + res
    s = gemm_scale(x, w, b, alpha=alpha, residual=res)
    _check(_linear(dev, x, w, b, res, alpha, variant=variant), ref, s, "gemm", f"linear {m}x{k}x{n} variant {variant}")
    if (m, k, n) == (300, 320, 960) and variant == 0:
        _control(_linear(dev, x, w, b, res, alpha * (1 + 2 ** -7)), ref, s, "gemm", "linear alpha x (1 + 2^-7)")


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("ks", [2, 5, 8])
def test_linear_splitk_budget(dev, ks, variant):
    m, k, n, seed = 1024, 2560, 192, 21
    x, w, b, res = _gemm_operands(m, k, n, seed)
    ref = F.silu(0.75 * (x @ w.t() + b)) + res
    s = gemm_scale(x, w, b, alpha=0.75, residual=res)
    _check(_linear(dev, x, w, b, res, 0.75, variant=variant, ksplit=ks), ref, s, "gemm", f"split-K {ks} variant {variant}")


CONV_CASES = [(2, 16, 16, 64, 96, False, 2.0, 41), (2, 16, 16, 4, 320, False, 0.0, 45), (1, 8, 12, 32, 48, True, 0.0, 49)]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_budget(dev, case):
    bsz, h, w_, cin, cout, up, mean, seed = case
    x = q(_rand(bsz, cin, h, w_, seed=seed) + mean)
    wt = q(_rand(cout, cin, 3, 3, seed=seed + 1, scale=1 / math.sqrt(cin * 9)))
    if mean:
        wt = q(wt - wt.mean((1, 2, 3), keepdim=True))
    bias = _rand(cout, seed=seed + 2).double()
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    ref = F.conv2d(xin, wt, bias, padding=1)
    s = conv_scale(xin, wt, bias)
    xd = to_nhwc(x.float(), BF, dev, cpad=W.round8(cin))
    wd = W.pack_conv(wt.float()).to(dev, BF)
    run = lambda a: from_nhwc(ops.conv(xd, wd, bias.float().to(dev), kh=3, kw=3, pad=1, upsample=up, alpha=a), cout)  # noqa: E731
    _check(run(1.0), ref, s, "gemm", f"conv {case}")
    _control(run(1 + 2 ** -7), ref, s, "gemm", f"conv {case} with alpha x (1 + 2^-7)")


def test_linear_fused_geglu_budget(dev):
    m, k, f = 512, 320, 256
    x, w, b, _ = _gemm_operands(m, k, 2 * f, 61)
    h = x @ w.t() + b
    ref = h[:, :f] * F.gelu(h[:, f:])
    s = geglu_gemm_scale(h[:, :f], h[:, f:], gemm_scale(x, w[:f], b[:f]), gemm_scale(x, w[f:], b[f:]))
    wp, bp = W.pack_geglu(w.float(), b.float())
    got = ops.linear(x.to(dev, BF), wp.to(dev, BF), bp.to(dev), act=ops.ACT_GEGLU).cpu()
    _check(got, ref, s, "gemm", "fused geglu 512x320x256")


@pytest.mark.parametrize("m,k,n,seed", [(1000, 512, 320, 80), (256, 1280, 640, 84)])
def test_f32x3_budget(dev, m, k, n, seed):
    x = (_rand(m, k, seed=seed) * 3 + 0.3).double()
    w = _rand(n, k, seed=seed + 1, scale=1 / math.sqrt(k)).double()
    b = _rand(n, seed=seed + 2).double()
    ref = x @ w.t() + b
    s = gemm_scale(x, w, b)
    with ops.f32_gemm_mode("x3"):
        got = ops.linear(x.float().to(dev), w.float().to(dev), b.float().to(dev)).cpu()[:, :n]
        # negative control: A x (1 + 2^-12), the smallest perturbation the CPU proof shows caught at this unit
        bad = ops.linear((x * (1 + 2 ** -12)).float().to(dev), w.float().to(dev), b.float().to(dev)).cpu()[:, :n]
    _check(got, ref, s, "f32x3", f"f32x3 linear {m}x{k}x{n}", unit=UNIT_F32X3)
    _control(bad, ref, s, "f32x3", f"f32x3 linear {m}x{k}x{n} with A x (1 + 2^-12)", unit=UNIT_F32X3)


# ------------------------------------------------------------------ flash attention
ATTN_CASES = [(40, 2, 130, 77, False, 1), (64, 3, 77, 77, True, 5), (48, 1, 100, 513, False, 9), (80, 2, 300, 1090, False, 13),
              (40, 1, 257, 2048 + 31, False, 17), (40, 2, 64, 1, False, 21), (40, 4, 200, 1024, False, 25)]


def _flash(dev, qq, kk, vv, heads, d, nq, nk, scale, causal, prescaled, rowmajor, loop):
    """Heads-folded [h, n, d] operands -> the kernel's [1, n, h d] layout.  The buffers hold max(nq, nk) + 8 rows: K rows past nk
    are POISONED with a large key along the queries' common direction (an unmasked tail key would dominate its rows) and V rows /
    V^T columns past nk are NaN.  `loop`: the loop (1 .. 4) the knobs as they stand must put the launch on, asserted before it runs."""
    c = heads * d
    nr = max(nq, nk) + 8
    flat = lambda t: t.permute(1, 0, 2).reshape(1, t.shape[1], c).float()  # noqa: E731
    poison = torch.zeros(1, nr - nk, c)
    poison.view(1, nr - nk, heads, d)[..., 0] = 8.0 * math.sqrt(d)
    qkv = torch.full((1, nr, 3 * c), float("nan"))
    qkv[:, :, :c] = 0.0
    qkv[:, :nq, :c] = flat(qq)
    qkv[:, :nk, c:2 * c] = flat(kk)
    qkv[:, nk:, c:2 * c] = poison
    qkv = qkv.to(dev, BF)
    vt = torch.full((1, c, ops.round8(nk) + 8), float("nan"), device=dev, dtype=BF)
    vt[:, :, :nk] = flat(vv).transpose(1, 2).to(dev, BF)
    qkv[:, :nk, 2 * c:] = flat(vv).to(dev, BF)
    out = torch.zeros(1, nq, c, device=dev, dtype=BF)
    v = qkv[:, :nk, 2 * c:] if rowmajor else vt
    assert ops.flash_attn_which(qkv[:, :nq, :c], qkv[:, :nk, c:2 * c], v, out, heads, d, nq, nk, causal, prescaled, rowmajor) & 15 == loop
    ops.flash_attn(qkv[:, :nq, :c], qkv[:, :nk, c:2 * c], v, out, heads, d, nq, nk, scale, causal, prescaled=prescaled,
                   v_rowmajor=rowmajor)
    return out.cpu().reshape(nq, heads, d).permute(1, 0, 2)


# (SASPA_ATTN_MODE, SASPA_ATTN_V4, prescaled queries, row-major V): v1 plain; v1/v2/v3 prescaled (modes 1 / 2 / 4: short sequences
# take v1 whatever the mode); v4 (d = 40, prescaled); row-major V on v1 and on the 8-wave v3 loop
LOOPS = [("0", "0", False, False), ("1", "0", True, False), ("2", "0", True, False), ("4", "0", True, False), ("4", "2", True, False),
         ("0", "0", False, True), ("4", "0", True, True)]


def attn_skip(case, loop):
    """Why test_flash_attn_budget does not run this (case, loop), or None."""
    d, nk = case[0], case[3]
    mode, v4, _, rowmajor = loop
    if rowmajor and d not in (40, 64, 80):
        return "row-major V is pinned at the production head dimensions"
    if v4 == "2" and d != 40:
        return "v4 serves d = 40 only"
    if mode in ("1", "2") and nk < 512:
        return "short sequences take the v1 loop whatever the mode (covered by mode 4)"
    return None


def attn_loop(case, loop):
    """The loop (1 .. 4) a LOOPS entry puts an ATTN_CASES launch on (d <= 80, no causal mask from 512 keys on): v1 for plain
    queries and below 512 keys whatever the mode; modes 1 / 2 v2; mode 4 v3, or v4 where SASPA_ATTN_V4=2 and d = 40 with V^T."""
    d, nk = case[0], case[3]
    mode, v4, prescaled, rowmajor = loop
    if not prescaled or nk < 512:
        return 1
    if mode in ("1", "2"):
        return 2
    return 4 if v4 == "2" and d == 40 and not rowmajor else 3


@pytest.mark.parametrize("loop", LOOPS, ids=lambda t: f"mode{t[0]}-v4_{t[1]}-{'pre' if t[2] else 'plain'}-{'vrow' if t[3] else 'vt'}")
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda t: f"d{t[0]}h{t[1]}q{t[2]}k{t[3]}{'c' if t[4] else ''}")
def test_flash_attn_budget(dev, monkeypatch, case, loop):
    d, heads, nq, nk, causal, seed = case
    mode, v4, prescaled, rowmajor = loop
    if attn_skip(case, loop):
        pytest.skip(attn_skip(case, loop))
    want = attn_loop(case, loop)
    monkeypatch.setenv("SASPA_ATTN_MODE", mode)
    monkeypatch.setenv("SASPA_ATTN_V4", v4)
    qq, kk, vv = attn_operands(heads, nq, nk, d, seed)
    sc = d ** -0.5
    if prescaled:
        qs = q(qq * (sc * LOG2E))                 # what the folded to_q weights produce; the reference uses the same rounded queries
        qeff, kscale = qs / (sc * LOG2E), 1.0
    else:
        qs, qeff, kscale = qq, qq, sc
    ref, p = _attn_ref(qeff, kk, vv, sc, causal)
    s = attn_scale(p, vv)
    tag = f"flash d={d} h={heads} nq={nq} nk={nk}{' causal' if causal else ''} loop {loop}"
    got = _flash(dev, qs, kk, vv, heads, d, nq, nk, kscale, causal, prescaled, rowmajor, want)
    _check(got, ref, s, "attn", tag)
    if nk > 1 and loop in (LOOPS[0], LOOPS[3]):
        # negative controls: the same launch with nk - 1 keys, and (plain queries) with the scale x (1 + 2^-5)
        _control(_flash(dev, qs, kk[:, :-1], vv[:, :-1], heads, d, nq, nk - 1, kscale, causal, prescaled, rowmajor, want), ref, s, "attn",
                 f"{tag} with nk - 1")
        if not prescaled:
            _control(_flash(dev, qs, kk, vv, heads, d, nq, nk, kscale * (1 + 2 ** -5), causal, prescaled, rowmajor, want), ref, s, "attn",
                     f"{tag} with scale x (1 + 2^-5)")


# ------------------------------------------------------------------ norms
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
@pytest.mark.parametrize("rows,c", [(300, 320), (77, 768)])
def test_layernorm_budget(dev, rows, c, kind, eps):
    x = _norm_inputs("normal" if kind == "const" else kind, (rows, c), 1 + c)
    if kind == "const":
        x[::3] = q(torch.full((c,), 0.7, dtype=torch.float64))      # every third row constant: var = 0
    g, b = 1 + 0.1 * _rand(c, seed=2 + c), 0.1 * _rand(c, seed=3 + c)
    ref, xhat = _ln_ref(x, g, b, eps)
    s = norm_scale(xhat, g, b, mu_rstd(x, eps))
    run = lambda e: ops.layernorm(x.to(dev, BF), g.to(dev), b.to(dev), e).cpu()  # noqa: E731
    _check(run(eps), ref, s, "norm", f"layernorm {rows}x{c} {kind} eps={eps:g}")
    if kind == "lowvar":
        _control(run(eps * 10), ref, s, "norm", f"layernorm {rows}x{c} {kind} with eps x 10")


@pytest.mark.parametrize("onepass", ["1", "0"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
@pytest.mark.parametrize("bsz,h,w_,c,groups", [(2, 16, 16, 320, 32), (2, 8, 8, 1280, 32), (2, 32, 32, 640, 32)])
def test_groupnorm_budget(dev, monkeypatch, bsz, h, w_, c, groups, kind, eps, onepass):
    """saspa_groupnorm (two-pass) and saspa_groupnorm_onepass (SASPA_GN_ONEPASS; eligible at 8x8 x 1280), NHWC.  The reference
    carries the statistics the launched kernel forms (fp32 partial sums, test_errbudget.gn_kernel_stats): at mu / sigma = 64 they
    differ from the exact ones by up to ~1e-2 units of bias, which the CPU proof bounds at the design level."""
    import ctypes
    monkeypatch.setenv("SASPA_GN_ONEPASS", onepass)
    hw = h * w_
    x = _norm_inputs("normal" if kind == "const" else kind, (bsz, hw, c), 11 + c + hw)
    if kind == "const":
        x[:, :, : c // groups] = q(torch.tensor(0.7, dtype=torch.float64))   # group 0 constant: var = 0
    g, b = 1 + 0.1 * _rand(c, seed=12 + c), 0.1 * _rand(c, seed=13 + c)
    prm = ops._lib.GroupNormParams()
    prm.c0, prm.c1, prm.batch, prm.hw, prm.groups = c, 0, bsz, hw, groups
    one = onepass == "1" and ops._lib.load().saspa_groupnorm_onepass_eligible(ctypes.byref(prm)) == 1
    ref, xhat, mr = gn_kernel_ref(x, g, b, groups, eps, onepass=one)
    s = norm_scale(xhat, g, b, mr)
    xd = x.reshape(bsz, h, w_, c).to(dev, BF)
    run = lambda e: ops.groupnorm(xd, g.to(dev), b.to(dev), groups, e, 0).cpu().reshape(bsz, hw, c)  # noqa: E731
    _check(run(eps), ref, s, "norm", f"groupnorm {bsz}x{h}x{w_}x{c}/{groups} {kind} eps={eps:g} {'one-pass' if one else 'two-pass'}")
    if kind == "lowvar":
        _control(run(eps * 10), ref, s, "norm", f"groupnorm {bsz}x{h}x{w_}x{c} {kind} with eps x 10")


# ------------------------------------------------------------------ elementwise
def test_geglu_silu_quick_gelu_budget(dev):
    x = q(_rand(123, 2 * 96, seed=38) * 2)
    a, gt = x[:, :96], x[:, 96:]
    xd = x.to(dev, BF)
    _check(ops.geglu(xd).cpu(), a * F.gelu(gt), elem_scale(a, F.gelu(gt)), "elem", "geglu (erf)")
    _check(ops.activation(xd, ops.ACT_SILU).cpu(), F.silu(x), elem_scale(x, torch.sigmoid(x)), "elem", "silu")
    sq = torch.sigmoid(1.702 * x)
    _check(ops.activation(xd, ops.ACT_QUICK_GELU).cpu(), x * sq, elem_scale(x, sq), "elem", "quick gelu")
    # negative control: the SiLU kernel checked against the quick-GELU reference
    _control(ops.activation(xd, ops.ACT_SILU).cpu(), x * sq, elem_scale(x, sq), "elem", "silu vs quick-gelu reference")


@pytest.mark.parametrize("causal", [False, True])
def test_softmax_rows_budget(dev, causal):
    xs = q(_rand(6, 77, 77, seed=27, scale=3.0))
    mask = torch.full((77, 77), float("-inf"), dtype=torch.float64).triu_(1) if causal else 0
    ref = torch.softmax(xs * 0.3 + mask, -1)
    s = elem_scale(ref)
    x80 = torch.zeros(6, 77, 80)
    x80[..., :77] = xs.float()

    def run(scale):
        xd = x80.to(dev, BF)
        ops.softmax_rows(xd, 77, scale, causal, 77)
        return xd.cpu()[..., :77]
    _check(run(0.3), ref, s, "elem", f"softmax_rows {'causal' if causal else 'plain'}")
    _control(run(0.3 * (1 + 2 ** -5)), ref, s, "elem", f"softmax_rows scale x (1 + 2^-5) {'causal' if causal else ''}")


def test_cfg_ddim_budget(dev):
    eps = q(_rand(4, 300, 4, seed=42))
    xx = q(_rand(2, 300, 4, seed=43))
    ref, s = cfg_ddim_ref(eps, xx, **CFG_COEF)
    a_t, a_p = CFG_COEF["a_t"], CFG_COEF["a_p"]

    def run(gs):
        e8 = F.pad(eps.float(), (0, 4)).to(dev, BF)
        x8 = F.pad(torch.cat([xx, xx]).float(), (0, 4)).to(dev, BF)
        ops.cfg_ddim_step(e8, x8, 2, 300, 4, gs, a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5)
        got = x8.cpu()
        assert torch.equal(got[:2], got[2:])
        return got[:2, :, :4]
    _check(run(CFG_COEF["gs"]), ref, s, "elem", "cfg + ddim")
    _control(run(7.0), ref, s, "elem", "cfg + ddim guidance 7.0 against 7.5")


# ------------------------------------------------------------------ fused transformer-block chains
# saspa_xattn_block, saspa_ff_block and the A-stationary GEMM's fused forms against the float64 chains of tests/test_errbudget.py
# (every bf16 hand-off of the kernels restated there with its source line).  Families: "xattn" / "ff" with a zero residual (the
# branch alone sets the scale), "chain_res" with the residual kept, "as" for the fused LayerNorm / GEGLU / V^T forms; the unfused
# A-stationary launches stay in "gemm".  References and magnitudes are built once per case (float64 on the CPU).
def _wide(t, dev, cols, fill):
    """t [M, C] as a view of a wider [M, cols] buffer filled with `fill`."""
    buf = torch.full((t.shape[0], cols), fill, device=dev, dtype=BF)
    buf[:, : t.shape[1]] = t.to(dev, BF)
    return buf, buf[:, : t.shape[1]]


XATTN_CASES = [(2, 256, 77), (3, 256, 1), (2, 512, 31), (2, 256, 32), (2, 256, 33), (2, 256, 64), (2, 256, 65), (1, 512, 96)]


@functools.lru_cache(maxsize=None)
def _xattn_case(nsamp, ntok, nk):
    op = xattn_operands(nsamp, ntok, nk, 400 + nk)
    return op, xattn_ref(op, torch.zeros_like(op["x"]))


def _xattn_launch(dev, op, *, nk=None, eps_mul=1.0, residual="zero", kf_edit=None, x=None, out=None):
    nk = op["nk"] if nk is None else nk
    w, bias = W.pack_xattn_w(op["wq"].float(), op["wo"].float(), op["bo"].float())
    kf, vf = W.xattn_kv_fragments(op["k"][:, :nk].to(dev, BF), op["v"][:, :nk].to(dev, BF))
    if kf_edit is not None:
        kf = kf_edit(kf)
    xd = op["x"].to(dev, BF) if x is None else x
    res = torch.zeros_like(op["x"]).to(dev, BF) if residual == "zero" else None
    got = ops.xattn_block(xd, (op["gamma"].float().to(dev), op["beta"].float().to(dev), op["eps"] * eps_mul), w.to(dev, BF),
                          bias.to(dev), kf, vf, nk, op["ntok"], residual=res, out=out)
    return got.float().cpu()


@pytest.mark.parametrize("nsamp,ntok,nk", XATTN_CASES)
def test_xattn_block_budget(dev, nsamp, ntok, nk):
    op, (ref, s) = _xattn_case(nsamp, ntok, nk)
    tag = f"xattn_block {nsamp}x{ntok} tokens, {nk} keys"
    got = _xattn_launch(dev, op)
    _check(got, ref, s, "xattn", tag)
    if nk in (33, 77):
        # the pad slots of kf (keys nk..95; found by packing an indicator through the same function) overwritten with a large key
        # along the queries' common direction (channel 0 of every head), vf's pad left zero as the header's contract says: only
        # the kernel's own mask stands between those keys and the softmax level, and the result must not change by a bit
        ind = torch.zeros(nsamp, 96, XA_C, device=dev, dtype=BF)
        ind[:, nk:, ::XA_D] = 1.0
        pad = W.xattn_kv_fragments(ind, torch.zeros_like(ind))[0] == 1.0
        assert int(pad.sum()) == nsamp * 8 * (96 - nk)
        poisoned = _xattn_launch(dev, op, kf_edit=lambda kf: torch.where(pad, torch.full_like(kf, 8.0 * math.sqrt(XA_D)), kf))
        assert torch.equal(poisoned, got), f"{tag}: a poisoned pad key changed the result: the tail mask does not decide alone"
        print(f"\n[bit-equal] xattn {tag}: pad keys poisoned")
    if nk > 1:
        _control(_xattn_launch(dev, op, nk=nk - 1), ref, s, "xattn", f"{tag} with nk - 1")
        _control(_xattn_launch(dev, op, eps_mul=10.0), ref, s, "xattn", f"{tag} with ln_eps x 10 (low-variance rows)")


def test_xattn_block_residual_and_pitches(dev):
    """residual=None (the kernel re-reads x), and x / out as views of wider buffers: bit-equal to the dense launch, nothing written
    outside the view."""
    nsamp, ntok, nk = 2, 256, 77
    op, (ref0, s0) = _xattn_case(nsamp, ntok, nk)
    ref, s = xattn_ref(op, None)
    got = _xattn_launch(dev, op, residual=None)
    _check(got, ref, s, "chain_res", f"xattn_block {nsamp}x{ntok} tokens, {nk} keys, residual = x")
    bad = got.clone()
    last = torch.arange(1, nsamp + 1) * ntok - 1
    bad[last] += (op["x"][last - 1] - op["x"][last]).float()             # (what reading the neighbour's residual would give)
    _control(bad, ref, s, "chain_res", "xattn_block residual of the neighbouring row in a sample's last row (host-side)")
    dense = _xattn_launch(dev, op)
    xbuf, xv = _wide(op["x"], dev, 384, float("nan"))
    obuf, ov = _wide(torch.zeros_like(op["x"]), dev, 448, float("nan"))
    pitched = _xattn_launch(dev, op, x=xv, out=ov)
    assert torch.equal(pitched, dense)
    assert torch.isnan(obuf[:, XA_C:]).all() and torch.isnan(xbuf[:, XA_C:]).all()
    _check(pitched, ref0, s0, "xattn", "xattn_block x pitch 384, out pitch 448")


FF_CASES = [(128, 32, True), (128, 64, True), (384, 1280, True), (256, 1280, False)]


@functools.lru_cache(maxsize=None)
def _ff_case(m, f, ln):
    op = ff_operands(m, f, 500 + f + m)
    return op, ff_ref(op, torch.zeros_like(op["x"]), ln)


def _ff_launch(dev, op, ln, *, eps_mul=1.0, residual="zero", x=None, out=None):
    w1p, b1p, w2f, b2p = W.pack_ff_block(op["w1"].float(), op["b1"].float(), op["w2"].float(), op["b2"].float())
    xd = op["x"].to(dev, BF) if x is None else x
    res = torch.zeros_like(op["x"]).to(dev, BF) if residual == "zero" else None
    lnp = (op["gamma"].float().to(dev), op["beta"].float().to(dev), op["eps"] * eps_mul) if ln else None
    got = ops.ff_block(xd, lnp, w1p.to(dev, BF), b1p.to(dev), w2f.to(dev, BF), b2p.to(dev), residual=res, out=out)
    return got.float().cpu()


@pytest.mark.parametrize("ws", ["1", "0"])
@pytest.mark.parametrize("m,f,ln", FF_CASES)
def test_ff_block_budget(dev, monkeypatch, m, f, ln, ws):
    monkeypatch.setenv("SASPA_FF_WS", ws)
    op, (ref, s) = _ff_case(m, f, ln)
    tag = f"ff_block {m}x{f}{'' if ln else ' no LayerNorm'} SASPA_FF_WS={ws}"
    got = _ff_launch(dev, op, ln)
    _check(got, ref, s, "ff", tag)
    if ln:
        _control(_ff_launch(dev, op, ln, eps_mul=10.0), ref, s, "ff", f"{tag} with ln_eps x 10 (low-variance rows)")
    if ws == "1":
        monkeypatch.setenv("SASPA_FF_WS", "0")
        assert torch.equal(_ff_launch(dev, op, ln), got), "the wave-specialised and the four-wave form differ"


@pytest.mark.parametrize("ws", ["1", "0"])
def test_ff_block_residual_and_pitches(dev, monkeypatch, ws):
    monkeypatch.setenv("SASPA_FF_WS", ws)
    m, f = 128, 64
    op, (ref0, s0) = _ff_case(m, f, True)
    ref, s = ff_ref(op, None, True)
    _check(_ff_launch(dev, op, True, residual=None), ref, s, "chain_res", f"ff_block {m}x{f} residual = x SASPA_FF_WS={ws}")
    dense = _ff_launch(dev, op, True)
    xbuf, xv = _wide(op["x"], dev, 384, float("nan"))
    obuf, ov = _wide(torch.zeros_like(op["x"]), dev, 448, float("nan"))
    pitched = _ff_launch(dev, op, True, x=xv, out=ov)
    assert torch.equal(pitched, dense)
    assert torch.isnan(obuf[:, XA_C:]).all() and torch.isnan(xbuf[:, XA_C:]).all()
    _check(pitched, ref0, s0, "ff", f"ff_block x pitch 384, out pitch 448 SASPA_FF_WS={ws}")


AS_M = 48897                    # 191 blocks of 256 rows + one row: the smallest size the A-stationary kernel takes, ragged


@functools.lru_cache(maxsize=None)
def _as_ops(m, n, kind="normal", geglu=False):
    return as_operands(m, n, 600 + n + (m % 7) + len(kind), kind, geglu=geglu)


@functools.lru_cache(maxsize=None)
def _as_case(m, n, kind="normal", **kw):
    return as_ref(_as_ops(m, n, kind, kw.get("geglu", False)), **kw)


def _as_launch(dev, op, *, bias=True, residual=False, ln=None, geglu=False, **kw):
    w, b = op["w"].float(), op["b"].float()
    if geglu:
        w, b = W.pack_geglu(w, b)
    lnp = None if ln is None else (op["gamma"].float().to(dev), op["beta"].float().to(dev), ln)
    return ops.linear(op["x"].to(dev, BF), w.to(dev, BF), b.to(dev) if bias else None,
                      residual=op["res"].to(dev, BF) if residual else None, act=ops.ACT_GEGLU if geglu else ops.ACT_NONE, ln=lnp,
                      variant=ops.GEMM_AS, **kw)


@pytest.mark.parametrize("form", ["plain", "bias", "residual"])
@pytest.mark.parametrize("n", [64, 320])
def test_gemm_as_budget(dev, n, form):
    kw = dict(bias=form != "plain", residual=form == "residual")
    ref, s = _as_case(AS_M, n, **kw)
    _check(_as_launch(dev, _as_ops(AS_M, n), **kw).cpu(), ref, s, "gemm", f"A-stationary {form} {AS_M}x320x{n}")


@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
def test_gemm_as_fused_layernorm_budget(dev, kind):
    m, n = 49152, 320
    op = _as_ops(m, n, kind)
    ref, s = _as_case(m, n, kind, ln=1e-5)
    _check(_as_launch(dev, op, ln=1e-5).cpu(), ref, s, "as", f"A-stationary LayerNorm {m}x320x{n} {kind}")
    if kind == "lowvar":
        _control(_as_launch(dev, op, ln=1e-4).cpu(), ref, s, "as", f"A-stationary LayerNorm {m}x320x{n} {kind} with ln_eps x 10")


@pytest.mark.parametrize("n", [320, 1024])                  # 160-column and 128-column GEGLU packing
def test_gemm_as_fused_layernorm_geglu_budget(dev, n):
    m = 49152
    op = _as_ops(m, n, "normal", True)
    ref, s = _as_case(m, n, "normal", ln=1e-5, geglu=True)
    got = _as_launch(dev, op, ln=1e-5, geglu=True).cpu()
    assert got.shape == (m, n // 2)
    _check(got, ref, s, "as", f"A-stationary LayerNorm + GEGLU {m}x320x{n}")


def test_gemm_as_qkv_vt_budget(dev):
    """Q | K row-major and V^T per sample out of one launch (n_split = 640, 12 samples of 4096 rows), budgeted separately."""
    m, n, n_split, rpb = 49152, 960, 640, 4096
    op = _as_ops(m, n)
    ref, s = _as_case(m, n, "normal", bias=False, ln=1e-5)
    out_t = torch.full((m // rpb, n - n_split, rpb), float("nan"), device=dev, dtype=BF)
    qk = _as_launch(dev, op, bias=False, ln=1e-5, out_t=out_t, n_split=n_split, rows_per_batch=rpb)
    assert qk.shape == (m, n_split)
    _check(qk.cpu(), ref[:, :n_split], s[:, :n_split], "as", "Q | K | V^T: the row-major part")
    _check(out_t.cpu(), vt_tail(ref, n_split, rpb), vt_tail(s, n_split, rpb), "as", "Q | K | V^T: the transposed tail")
    bad = out_t.cpu().clone()
    bad[:-1, :, -1] = bad[1:, :, 0]
    _control(bad, vt_tail(ref, n_split, rpb), vt_tail(s, n_split, rpb), "as", "V^T tail with a sample boundary off by one (host-side)")
