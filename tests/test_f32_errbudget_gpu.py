"""The exact-fp32 kernels under the rounding-error budget (tests/errbudget.py, units of 2^-24) on the operands whose margins
tests/test_errbudget.py proves on the CPU (tests/f32_ref.py; seed shift 0): saspa_gemm with SASPA_F32 operands -- every fp32
instantiation of the tiled kernels, every epilogue form, K slices, the batched form --, saspa_pool2d and saspa_signsqrt_l2norm, and
the fp32 forms of the softmax / norm / elementwise kernels.  Every case builds a float64 reference from the fp32 operands and its
magnitude s_i; check_budget asserts max / rms / bias / slope against the family's limits, and one negative control per case (the
kernel's own output with one documented slip applied on the host, or the same launch with one argument perturbed) shows that the
budget would have rejected a wrong result."""
import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from tests import f32_ref as R
from tests.errbudget import LIMITS, UNIT_F32, check_budget, fmt, norm_scale, rejects
from tests.test_errbudget import _ln_ref, _norm_inputs, _rand, gn_kernel_ref, mu_rstd

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
ACT = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "add_relu": ops.ACT_ADD_RELU, "silu": ops.ACT_SILU}
TILED = 1                               # SASPA_GEMM_TILED: the family saspa_gemm_which reports for every fp32 launch


def _check(got, ref, s, family, what, unit=UNIT_F32):
    st = check_budget(got, ref, s, unit, limits=LIMITS[family], what=what)
    print(f"\n[budget] {family:13s} {what}: {fmt(st)}")
    return st


def _control(got, ref, s, family, what, unit=UNIT_F32):
    assert rejects(got, ref, s, unit, limits=LIMITS[family]), f"negative control not rejected: {what}"
    print(f"\n[control rejected] {family:13s} {what}")


def _which(fn):
    """fn() under ops' launch recorder: (its result, kernel family, K slices) of the ONE saspa_gemm launch inside -- the library's
    own dispatch executed dry (saspa_gemm_which, appended to the launch's meta by ops._meta_kernel)."""
    seen = []

    def rec(kind, flops, call, meta):
        seen.append((kind, meta))
        return call()
    ops.set_recorder(rec)
    try:
        out = fn()
    finally:
        ops.set_recorder(None)
    gm = [m for k, m in seen if k == "gemm"]
    assert len(gm) == 1 and len(gm[0]) == 11, seen
    return out, gm[0][9], gm[0][10]


def _pitched(t, dev, pitch, fill=float("nan")):
    """t [..., C] (CPU, any float dtype) as an fp32 device view of a buffer whose last dim is `pitch` >= C, the padding `fill`."""
    buf = torch.full((*t.shape[:-1], pitch), fill, device=dev, dtype=F32)
    buf[..., : t.shape[-1]] = t.to(dev, F32)
    return buf, buf[..., : t.shape[-1]]


def _epilogue_args(dev, op, f, n, pitched=False):
    """bias / rowvec / residual [M, N] of a form as device tensors; the residual's row pitch is a multiple of 4 elements (the C
    ABI's alignment rule), wider than N with junk in the padding when N % 4 != 0 or `pitched`."""
    bias = op["b"].to(dev, F32) if f["bias"] else None
    rv = op["rv"].to(dev, F32) if f["rowvec"] else None
    res = None
    if f["res"]:
        ld = ops.round8(n) + (8 if pitched else 0)
        res = _pitched(op["res"], dev, ld)[1] if ld != n else op["res"].to(dev, F32)
    return bias, rv, res


# ------------------------------------------------------------------ linear
# (M, K, N, operand kind, epilogue form, forced K slices or None, K slices expected, seed)  # the path plan_gemm / launch take
LINEAR_CASES = [
    # 64x64 tile (<= 160 tiles), K % 32 == 0: gemm_dma_kernel<float, 2, 2, 2, 2, PW, 4 stages>; ragged M (300 = 4 * 64 + 44) and N
    (300, 64, 96, "plain", "bias", None, 1, 1),
    (300, 64, 96, "relu", "relu_res", None, 1, 2),
    (300, 64, 96, "plain", "add_relu_res", None, 1, 3),
    (300, 64, 96, "plain", "silu_full", None, 1, 4),
    # K = 40 is no multiple of 32: the generic loader, gemm_kernel<float, 2, 2, PW>; K tail of 8
    (129, 40, 40, "relu", "bias", None, 1, 5),
    (129, 40, 40, "plain", "relu_res", None, 1, 6),
    (129, 40, 40, "relu", "add_relu_res", None, 1, 7),
    (129, 40, 40, "plain", "silu_full", None, 1, 8),
    # N <= 32: the 128x32 tile, gemm_dma_kernel<float, 4, 1, ...>; N = 3 reaches the epilogue's scalar tail
    (260, 320, 4, "plain", "relu_res", None, 1, 9),
    (260, 320, 3, "relu", "add_relu_res", None, 1, 13),
    # 20 x 8 = 160 tiles of 128 rows, N % 160 != 0: 128x128, gemm_dma_kernel<float, 4, 4, 2, 2, PW, 4 stages>
    (2560, 96, 1024, "relu", "relu_res", None, 1, 31),
    # N % 160 == 0 but 21 x 6 = 126 tiles < 160: plan_gemm keeps the 64x64 tile (41 x 15 = 615 tiles > 320: its 2-stage ring), ragged M
    (2600, 64, 960, "plain", "silu_full", None, 1, 35),
    # 27 x 6 = 162 tiles, N % 160 == 0: 128x160, gemm_dma_kernel<float, 4, 5, 2, 2, PW, 4 stages>; ragged M (3400 = 26 * 128 + 72)
    (3400, 64, 960, "plain", "silu_full", None, 1, 37),
    # 41 x 8 = 328 tiles > 320: 128x128 on the 2-stage ring, gemm_dma_kernel<float, 4, 4, 2, 2, PW, 2>
    (5248, 64, 1024, "relu", "bias", None, 1, 39),
    # long K on few tiles: the library's own split (2 tiles, 64 K-tiles: 8 slices) and forced ones; slabs summed by
    # splitk_reduce_kernel<float>, which also carries the epilogue
    (192, 2048, 96, "plain", "add_relu_res", None, 8, 21),
    (192, 2048, 96, "plain", "add_relu_res", 2, 2, 21),
    (192, 2048, 96, "relu", "silu_full", 5, 5, 23),
    (192, 2048, 96, "relu", "relu_res", 8, 8, 25),
]


def _linear(dev, op, f, n, ksplit=None, pitched=False):
    k = op["x"].shape[1]
    xbuf, x = _pitched(op["x"], dev, k + 8) if pitched else (None, op["x"].to(dev, F32))
    bias, rv, res = _epilogue_args(dev, op, f, n, pitched)
    obuf, out = (None, None)
    if pitched:
        obuf = torch.full((x.shape[0], ops.round8(n) + 16), float("nan"), device=dev, dtype=F32)
        out = obuf[:, : ops.round8(n)]
    got, fam, ks = _which(lambda: ops.linear(x, op["w"].to(dev, F32), bias, residual=res, alpha=f["alpha"], act=ACT[f["act"]],
                                             rowvec=rv, ksplit=ksplit, out=out))
    if pitched:
        assert torch.isnan(obuf[:, n:]).all(), "the launch wrote outside the N output columns"
        assert torch.isnan(xbuf[:, k:]).all()
    return got.cpu()[:, :n], fam, ks


@pytest.mark.parametrize("m,k,n,kind,form,force,want_ks,seed", LINEAR_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}-{c[4]}-ks{c[5] or 'auto'}" for c in LINEAR_CASES])
def test_linear_f32_budget(dev, m, k, n, kind, form, force, want_ks, seed):
    op = R.gemm_operands(_rand, m, k, n, seed, kind)
    f = R.FORMS[form]
    ref, s = R.gemm_ref(op, f)
    tag = f"linear f32 {m}x{k}x{n} {kind} {form}{'' if force is None else f' ksplit {force}'}"
    got, fam, ks = _linear(dev, op, f, n, force)
    assert (fam, ks) == (TILED, want_ks), f"{tag}: saspa_gemm_which reports family {fam} on {ks} K slices"
    _check(got, ref, s, "f32_gemm", tag)
    _control(R.through_bf16(got), ref, s, "f32_gemm", f"{tag}, output passed through bf16 (host-side)")


def test_linear_f32_pitches(dev):
    """Input, residual and output rows wider than K / N with NaN in the padding: bit-equal to the dense launch, nothing written
    outside the N columns."""
    m, k, n, seed = 300, 64, 96, 4
    op = R.gemm_operands(_rand, m, k, n, seed, "plain")
    f = R.FORMS["silu_full"]
    ref, s = R.gemm_ref(op, f)
    dense, _, _ = _linear(dev, op, f, n)
    got, fam, ks = _linear(dev, op, f, n, pitched=True)
    assert (fam, ks) == (TILED, 1)
    assert torch.equal(got, dense)
    _check(got, ref, s, "f32_gemm", "linear f32 300x64x96 silu_full, x pitch 72, residual pitch 104, out pitch 112")
    o2 = dict(op, b=op["b"].roll(1))
    _control(_linear(dev, o2, f, n)[0], ref, s, "f32_gemm", "linear f32 300x64x96 with the bias shifted by one column")


# ------------------------------------------------------------------ batched (bilinear attention pooling)
def test_gemm_batched_f32_bap_budget(dev):
    """feature_matrix[b] = att_t[b] @ feat_t[b]^T / HW as WSDANCAL.forward launches it (filters.py:352-356): 32 x 200 x 64, two
    batches, alpha = 1 / 196, K padded past the 196 real columns with zeros.  K = 200 is no multiple of 32: the generic loader,
    gemm_kernel<float, 2, 2, PW>, batch on blockIdx.z."""
    m, k, n, nb, hw = 32, 200, 64, 2, 196
    opb = [R.gemm_operands(_rand, m, k, n, 29 + 100 * z, "bap") for z in range(nb)]
    f = R.bap_form(hw)
    refs = [R.gemm_ref(o, f) for o in opb]
    ref, s = torch.stack([r[0] for r in refs]), torch.stack([r[1] for r in refs])
    a = torch.stack([o["x"] for o in opb]).to(dev, F32)
    w = torch.stack([o["w"] for o in opb]).to(dev, F32)

    def run(alpha):
        out = torch.full((nb, m, n), float("nan"), device=dev, dtype=F32)
        _, fam, ks = _which(lambda: ops.gemm_batched(a, k, (m * k, 0), w, k, (n * k, 0), out, n, (m * n, 0), m, n, k, nb, 1, alpha=alpha))
        assert (fam, ks) == (TILED, 1)
        return out.cpu()
    _check(run(1.0 / hw), ref, s, "f32_gemm_pos", "gemm_batched f32 2 x 32x200x64 alpha = 1 / 196")
    _control(run(1.0 / (hw + 4)), ref, s, "f32_gemm_pos", "gemm_batched f32 with alpha = 1 / 200 (the padded width)")
    _control(R.through_bf16(run(1.0 / hw)), ref, s, "f32_gemm_pos", "gemm_batched f32, output passed through bf16 (host-side)")


# ------------------------------------------------------------------ conv
# (B, H, W, cin, creal, cout, k, stride, pad, operand kind, form, K slices expected, seed)  # the path
CONV_CASES = [
    # the HED stem in small: 8 channels (K = 72, no multiple of 32): the generic loader, gemm_kernel<float, 2, 2, conv>
    (2, 16, 16, 8, 8, 64, 3, 1, 1, "plain", "bias", 1, 41),
    (2, 16, 16, 8, 8, 64, 3, 1, 1, "plain", "silu_full", 1, 42),
    # 64 channels: gemm_dma_kernel<float, 2, 2, 2, 2, conv, 4 stages>, tap masks on a non-square border
    (2, 12, 20, 64, 64, 64, 3, 1, 1, "relu", "relu_res", 1, 43),
    (2, 12, 20, 64, 64, 64, 3, 1, 1, "relu", "add_relu_res", 1, 44),
    # 49 taps (beyond the fast loaders' 31-tap mask) on 3 -> 8 padded channels: the generic per-lane loader
    (2, 40, 56, 8, 3, 16, 7, 2, 3, "plain", "relu_res", 1, 45),
    # 1x1 stride 2 (not pointwise: the window arithmetic of the DMA conv loader), 64 -> 128
    (2, 14, 14, 64, 64, 128, 1, 2, 0, "relu", "bias", 1, 47),
    # 3x3 stride 2 on an odd, non-square image, 32 -> 64
    (2, 15, 17, 32, 32, 64, 3, 2, 1, "relu", "add_relu_res", 1, 49),
    # the deep HED level in small: K = 4608 on the library's own 8 K slices (4 tiles, 144 K-tiles), splitk_reduce_kernel<float>
    (1, 8, 8, 512, 512, 512, 3, 1, 1, "relu", "relu_res", 8, 51),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[5]}-k{c[6]}s{c[7]}-{c[10]}" for c in CONV_CASES])
def test_conv_f32_budget(dev, case):
    b, h, w_, cin, creal, cout, kh, stride, pad, kind, form, want_ks, seed = case
    op = R.conv_operands(_rand, b, h, w_, cin, cout, kh, stride, pad, seed, kind, creal)
    f = R.FORMS[form]
    ref, s = R.gemm_ref(op, f)
    ho, wo = op["out_hw"]
    bias, rv, res = _epilogue_args(dev, op, f, cout)
    if res is not None:
        res = res.reshape(b, ho, wo, cout)
    xd = op["x_nhwc"].to(dev, F32)
    wd = W.pack_conv(op["w_nchw"].float()).to(dev, F32)
    out, fam, ks = _which(lambda: ops.conv(xd, wd, bias, kh=kh, kw=kh, stride=stride, pad=pad, rowvec=rv, residual=res,
                                           alpha=f["alpha"], act=ACT[f["act"]]))
    tag = f"conv f32 {b}x{h}x{w_} {cin}({creal})->{cout} {kh}x{kh} stride {stride} pad {pad} {kind} {form}"
    assert tuple(out.shape) == (b, ho, wo, ops.round8(cout))
    assert (fam, ks) == (TILED, want_ks), f"{tag}: saspa_gemm_which reports family {fam} on {ks} K slices"
    got = out.cpu()[..., :cout].reshape(-1, cout)
    _check(got, ref, s, "f32_gemm", tag)
    _control(R.through_bf16(got), ref, s, "f32_gemm", f"{tag}, output passed through bf16 (host-side)")


# ------------------------------------------------------------------ pool2d
POOL_INPUTS = [(3, 23, 19, 8, "randn", 51), (2, 14, 14, 24, "relu", 55)]


def _pool_dev(x, dev, storage):
    """x [B, H, W, C] values of the storage type -> a device view with pixel pitch C + 8 and NaN in the padding."""
    buf = torch.full((*x.shape[:-1], x.shape[-1] + 8), float("nan"), device=dev, dtype=storage)
    buf[..., : x.shape[-1]] = x.to(dev, storage)
    return buf[..., : x.shape[-1]]


@pytest.mark.parametrize("storage", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("b,h,w_,c,kind,seed", POOL_INPUTS)
def test_maxpool_moves_values_only(dev, b, h, w_, c, kind, seed, storage):
    """Max pooling selects: bit-equal to F.max_pool2d of the stored values -- also on an all-negative input, where a padding tap
    that acted as a zero would win every border window."""
    x = R.pool_input(_rand, b, h, w_, c, seed, kind, storage)
    for name, xx in (("as drawn", x), ("all negative", (-x.abs() - 0.125).to(storage).double())):
        xd = _pool_dev(xx, dev, storage)
        for k, stride, pad in ((3, 2, 1), (3, 2, 0), (2, 1, 0)):
            got = ops.pool2d(xd, k, stride, pad, mode="max").float().cpu()
            ref = F.max_pool2d(xx.float().permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1)
            assert got.shape == ref.shape and torch.equal(got, ref), (name, k, stride, pad)


@pytest.mark.parametrize("storage", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("b,h,w_,c,kind,seed", POOL_INPUTS)
def test_avgpool_budget(dev, b, h, w_, c, kind, seed, storage):
    family = "f32_pool" if storage == F32 else "f32_pool_bf16"
    unit = R.pool_unit(storage)
    x = R.pool_input(_rand, b, h, w_, c, seed, kind, storage)
    xd = _pool_dev(x, dev, storage)
    for k in (2, 7, min(h, w_)):                       # (the last: the whole image where it is square)
        ref, s = R.avgpool_ref(x, k, k)
        got = ops.pool2d(xd, k).float().cpu()
        tag = f"avgpool {b}x{h}x{w_}x{c} k={k} {kind} {'fp32' if storage == F32 else 'bf16'} storage, pixel pitch {c + 8}"
        assert got.shape == ref.shape
        _check(got, ref, s, family, tag, unit)
        if storage == F32 or kind == "relu" or k == 2:          # (where f32_ref.pool_cases names the slip)
            bad = (got.double() * (k * k) / (k * k - 1)).to(storage)
            _control(bad, ref, s, family, f"{tag}, scaled by k*k / (k*k - 1) (host-side)", unit)


# ------------------------------------------------------------------ signsqrt_l2norm
@pytest.mark.parametrize("rows,c,kind,seed", R.TAIL_CASES, ids=[f"{t[0]}x{t[1]}-{t[2]}" for t in R.TAIL_CASES])
def test_signsqrt_l2norm_budget(dev, rows, c, kind, seed):
    """eps = 1e-6, scale = 100 against float64 of the reference's formula (sign(x) sqrt(|x| + eps), then F.normalize): rows without
    zeros, with one zero block of C / 32, with 60 % zeros and an all-zero row.  An exact zero in is an exact zero out and adds
    nothing to its row's norm."""
    x = R.tail_rows(_rand, rows, c, kind, seed)
    ref, s = R.tail_ref(x)
    xd = x.to(dev, F32)
    got = ops.signsqrt_l2norm(xd, R.TAIL_EPS, R.TAIL_SCALE).cpu()
    tag = f"signsqrt_l2norm {rows}x{c} {kind}"
    assert (got[x == 0] == 0).all(), f"{tag}: an exact zero did not stay an exact zero"
    _check(got, ref, s, "f32_tail", tag)
    if kind in ("block", "heavy"):
        # the slip this kernel had: eps counted into the squared norm for the exact zeros too (applied to the output on the host)
        t = x.abs() + R.TAIL_EPS
        wrong = torch.sqrt(torch.where(x != 0, t, torch.zeros(())).sum(-1, keepdim=True) / t.sum(-1, keepdim=True))
        _control(got.double() * wrong, ref, s, "f32_tail", f"{tag}, eps counted for the exact zeros (host-side)")
    else:
        _control(ops.signsqrt_l2norm(xd, 1e-12, R.TAIL_SCALE).cpu(), ref, s, "f32_tail", f"{tag} launched with eps = 1e-12")


# ------------------------------------------------------------------ second tier: fp32 forms of kernels with bf16 budgets
# Operands and case lists of tests/test_errbudget_gpu.py (bf16-representable values stored as fp32, so that the GroupNorm reference
# can restate the kernels' fp32 partial sums exactly); the output is NOT rounded, the unit is 2^-24.
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
@pytest.mark.parametrize("rows,c", [(300, 320), (77, 768)])
def test_layernorm_f32_budget(dev, rows, c, kind, eps):
    x = _norm_inputs("normal" if kind == "const" else kind, (rows, c), 1 + c)
    if kind == "const":
        x[::3] = x[0, 0]                               # every third row constant: var = 0
    g, b = R.f32v(1 + 0.1 * _rand(c, seed=2 + c)), R.f32v(0.1 * _rand(c, seed=3 + c))
    ref, xhat = _ln_ref(x, g, b, eps)
    s = norm_scale(xhat, g, b, mu_rstd(x, eps), cancel=1.0)
    run = lambda e: ops.layernorm(x.to(dev, F32), g.to(dev, F32), b.to(dev, F32), e).cpu()  # noqa: E731
    tag = f"layernorm f32 {rows}x{c} {kind} eps={eps:g}"
    got = run(eps)
    _check(got, ref, s, "f32_norm", tag)
    _control(run(eps * 10) if kind == "lowvar" else R.through_bf16(got), ref, s, "f32_norm",
             f"{tag} with eps x 10" if kind == "lowvar" else f"{tag}, output passed through bf16 (host-side)")


GN_SHAPES = [((2, 16, 16, 320, 32), "0"), ((2, 8, 8, 1280, 32), "1"), ((2, 8, 8, 1280, 32), "0"), ((2, 32, 32, 640, 32), "0")]


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
@pytest.mark.parametrize("shape,onepass", GN_SHAPES, ids=[f"{'x'.join(map(str, s))}-onepass{o}" for s, o in GN_SHAPES])
def test_groupnorm_f32_budget(dev, monkeypatch, shape, onepass, kind, eps):
    """saspa_groupnorm (statistics + apply) and saspa_groupnorm_onepass (8x8 x 1280) on fp32 storage; the reference carries the
    statistics the launched kernel forms (test_errbudget.gn_kernel_stats), as the bf16 tests' does."""
    import ctypes
    bsz, h, w_, c, groups = shape
    monkeypatch.setenv("SASPA_GN_ONEPASS", onepass)
    hw = h * w_
    x = _norm_inputs("normal" if kind == "const" else kind, (bsz, hw, c), 11 + c + hw)
    if kind == "const":
        x[:, :, : c // groups] = x[0, 0, 0]            # group 0 constant: var = 0
    g, b = R.f32v(1 + 0.1 * _rand(c, seed=12 + c)), R.f32v(0.1 * _rand(c, seed=13 + c))
    prm = ops._lib.GroupNormParams()
    prm.c0, prm.c1, prm.batch, prm.hw, prm.groups = c, 0, bsz, hw, groups
    one = onepass == "1" and ops._lib.load().saspa_groupnorm_onepass_eligible(ctypes.byref(prm)) == 1
    assert one == (onepass == "1")
    ref, xhat, mr = gn_kernel_ref(x, g, b, groups, eps, onepass=one)
    s = norm_scale(xhat, g, b, mr, cancel=1.0)
    xd = x.reshape(bsz, h, w_, c).to(dev, F32)
    run = lambda e: ops.groupnorm(xd, g.to(dev, F32), b.to(dev, F32), groups, e, 0).cpu().reshape(bsz, hw, c)  # noqa: E731
    tag = f"groupnorm f32 {bsz}x{h}x{w_}x{c}/{groups} {kind} eps={eps:g} {'one-pass' if one else 'two-pass'}"
    got = run(eps)
    _check(got, ref, s, "f32_norm", tag)
    _control(run(eps * 10) if kind == "lowvar" else R.through_bf16(got), ref, s, "f32_norm",
             f"{tag} with eps x 10" if kind == "lowvar" else f"{tag}, output passed through bf16 (host-side)")


def test_geglu_silu_quick_gelu_f32_budget(dev):
    x = R.f32v(_rand(123, 2 * 96, seed=38) * 2)
    refs = R.elem_refs(x)
    xd = x.to(dev, F32)
    got = {"geglu": ops.geglu(xd).cpu(), "silu": ops.activation(xd, ops.ACT_SILU).cpu(),
           "quick-gelu": ops.activation(xd, ops.ACT_QUICK_GELU).cpu()}
    for name, (ref, s) in refs.items():
        _check(got[name], ref, s, "f32_elem", f"{name} f32")
        _control(R.through_bf16(got[name]), ref, s, "f32_elem", f"{name} f32, output passed through bf16 (host-side)")
    _control(got["silu"], *refs["quick-gelu"], "f32_elem", "silu f32 against the quick-gelu reference")


@pytest.mark.parametrize("causal", [False, True])
def test_softmax_rows_f32_budget(dev, causal):
    x = R.f32v(_rand(6, 77, 77, seed=27, scale=3.0))
    ref, s = R.softmax_ref(x, R.f32_scalar(R.SOFTMAX_SCALE), causal)
    x80 = torch.zeros(6, 77, 80)
    x80[..., :77] = x.float()

    def run(scale):
        xd = x80.to(dev, F32)
        ops.softmax_rows(xd, 77, scale, causal, 77)
        out = xd.cpu()
        assert (out[..., 77:] == 0).all()
        return out[..., :77]
    tag = f"softmax_rows f32 {'causal' if causal else 'plain'}"
    got = run(R.SOFTMAX_SCALE)
    if causal:
        assert (got[ref == 0] == 0).all(), "a masked column is not an exact zero"
    _check(got, ref, s, "f32_softmax", tag)
    _control(run(R.SOFTMAX_SCALE * (1 + 2 ** -12)), ref, s, "f32_softmax", f"{tag} with scale x (1 + 2^-12)")
