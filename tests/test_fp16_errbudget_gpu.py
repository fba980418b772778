"""The fp16 build of the kernels (libsaspa_hip_f16.so) under the rounding-error budget: the cases of tests/test_errbudget_gpu.py --
its shapes, operands, negative controls and bit-equality checks -- run on fp16 tensors against float64 references taken from
fp16-rounded operands with RNE-to-fp16 at the kernels' rounding points (tests/fp16_budget.py; unit 2^-11, magnitudes floored at
2^-13, errbudget.LIMITS except where fp16_budget.LIMITS_F16 overrides a family).

Every family also launches the SAME operation in bf16 (the default library) and asserts that the fp16 checks reject that result
against the fp16 reference: a launch that had been routed to the bf16 kernels could not pass these tests.  For the gemm family the
check that does this at every K is the typical-magnitude rms (fp16_budget.TYPICAL_RMS_LIMIT), asserted on every GEMM launch here and
on a bf16 counter-launch of every GEMM kernel (tiled, wide, wave-specialised, split-K, fused GEGLU, A-stationary, the convs)."""
import contextlib

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib
from tests import errbudget as E
from tests import fp16_budget as H
from tests import test_errbudget_gpu as G

pytestmark = pytest.mark.gpu

# fp16 operands and references must not share the bf16 module's caches
_CACHES = {name: H.fresh_cache(getattr(G, name)) for name in ("_xattn_case", "_ff_case", "_as_ops", "_as_case")}


def _check16(got, ref, s, family, what, unit=None):
    s = H.floor16(s)
    st = E.check_budget(got, ref, s, H.UNIT_F16, limits=H.limits_for(family), what=f"fp16 {what}")
    print(f"\n[budget fp16] {family:5s} {what}: {E.fmt(st)}")
    if family in H.TYPICAL_RMS_LIMIT:
        # the error against the output's TYPICAL magnitude: what tells f16 from bf16 arithmetic behind a long K (fp16_budget.py)
        tr = H.typical_rms(got, ref)
        print(f"[typical rms fp16] {what}: {tr:.3f} (<= {H.TYPICAL_RMS_LIMIT[family]})")
        assert tr <= H.TYPICAL_RMS_LIMIT[family], f"fp16 {what}: typical-magnitude rms {tr:.3f} > {H.TYPICAL_RMS_LIMIT[family]}"
    return st


def _control16(got, ref, s, family, what, unit=None):
    assert E.rejects(got, ref, H.floor16(s), H.UNIT_F16, limits=H.limits_for(family)), f"negative control not rejected: fp16 {what}"
    print(f"\n[control rejected fp16] {family:5s} {what}")


def _bf16_must_fail(got, ref, s, family, what, unit=None):
    """The launch ran in bf16 (default library) on the bf16-rounded operands; the reference is the fp16 one."""
    st = E.budget_stats(got, ref, H.floor16(s), H.UNIT_F16)
    r = E.ratio(st, H.limits_for(family))
    print(f"\n[bf16 launch vs fp16 budget] {family:5s} {what}: x{r:.2f} of the allowance; {E.fmt(st)}")
    if family in H.TYPICAL_RMS_LIMIT:
        tr = H.typical_rms(got, ref)
        print(f"[bf16 launch, typical rms] {what}: {tr:.2f} (must exceed {H.TYPICAL_RMS_LIMIT[family]})")
        assert tr > H.TYPICAL_RMS_LIMIT[family], f"a bf16 launch passes the fp16 typical-magnitude check: {what}: {tr:.3f}"
    else:
        assert r > 1.0, f"a bf16 launch passes the fp16 budget: {what}: {E.fmt(st)}"
    return st


@contextlib.contextmanager
def _mode(dtype, check, control):
    """tests/test_errbudget_gpu with its device dtype, checkers, norm magnitude and caches swapped; references round to fp16."""
    names = ("BF", "_check", "_control", "norm_scale") + tuple(_CACHES)
    saved = {n: getattr(G, n) for n in names}
    with H.fp16_rounding():
        G.BF, G._check, G._control, G.norm_scale = dtype, check, control, H.norm_scale16
        for n, fn in _CACHES.items():
            setattr(G, n, fn)
        try:
            x = torch.tensor([1.0 + 2.0 ** -9], dtype=torch.float64)
            assert G.q is H.T.q and G.q(x).item() == x.item() and G._rand is H.T._rand, \
                "tests.test_errbudget_gpu no longer builds its operands through tests.test_errbudget: they would be bf16 ones"
            yield
        finally:
            for n, v in saved.items():
                setattr(G, n, v)


def fp16():
    return _mode(torch.float16, _check16, _control16)


def routed_to_bf16():
    """The same test body with bf16 device tensors: every budget check must FAIL (the body's own negative controls are moot)."""
    return _mode(torch.bfloat16, _bf16_must_fail, lambda *a, **k: None)


def test_fp16_launches_use_the_fp16_library(dev):
    x = torch.randn(64, 64, device=dev).to(torch.float16)
    w = torch.randn(32, 64, device=dev).to(torch.float16)
    from saspa_aug_amd import ops
    y = ops.linear(x, w)
    assert y.dtype == torch.float16 and _lib.f16_loaded()
    assert torch.allclose(y.float()[:, :32], x.float() @ w.float().t(), rtol=2e-3, atol=2e-2)
    with pytest.raises(ValueError):
        ops.linear(x, w.to(torch.bfloat16))                # mixed 16-bit types are a caller error, not a routing question


# ------------------------------------------------------------------ GEMM / conv
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("m,k,n,seed", G.GEMM_SHAPES)
def test_linear_budget_fp16(dev, m, k, n, seed, variant):
    with fp16():
        G.test_linear_budget(dev, m, k, n, seed, variant)
    # the bf16 counter-launch of every GEMM kernel: AUTO / TILED / WIDE / WS on the level-0 shape, the short-K and the two long-K
    # shapes on AUTO, the wide kernel behind K = 1280
    if (m, k, n) == (300, 320, 960) or (variant == 0 and (m, k, n) in ((129, 64, 40), (1024, 2560, 192))) or \
            (variant == 2 and (m, k, n) == (4096, 1280, 320)):
        with routed_to_bf16():
            G.test_linear_budget(dev, m, k, n, seed, variant)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("ks", [2, 5, 8])
def test_linear_splitk_budget_fp16(dev, ks, variant):
    with fp16():
        G.test_linear_splitk_budget(dev, ks, variant)
    if ks == 5:
        with routed_to_bf16():
            G.test_linear_splitk_budget(dev, ks, variant)


@pytest.mark.parametrize("case", G.CONV_CASES)
def test_conv_budget_fp16(dev, case):
    with fp16():
        G.test_conv_budget(dev, case)
    with routed_to_bf16():
        G.test_conv_budget(dev, case)


def test_linear_fused_geglu_budget_fp16(dev):
    with fp16():
        G.test_linear_fused_geglu_budget(dev)
    with routed_to_bf16():
        G.test_linear_fused_geglu_budget(dev)


# ------------------------------------------------------------------ flash attention
@pytest.mark.parametrize("loop", G.LOOPS, ids=lambda t: f"mode{t[0]}-v4_{t[1]}-{'pre' if t[2] else 'plain'}-{'vrow' if t[3] else 'vt'}")
@pytest.mark.parametrize("case", G.ATTN_CASES, ids=lambda t: f"d{t[0]}h{t[1]}q{t[2]}k{t[3]}{'c' if t[4] else ''}")
def test_flash_attn_budget_fp16(dev, monkeypatch, case, loop):
    with fp16():
        G.test_flash_attn_budget(dev, monkeypatch, case, loop)
    if case[3] == 1024 and loop in (G.LOOPS[0], G.LOOPS[3], G.LOOPS[4]):
        with routed_to_bf16():
            G.test_flash_attn_budget(dev, monkeypatch, case, loop)


# ------------------------------------------------------------------ norms
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
@pytest.mark.parametrize("rows,c", [(300, 320), (77, 768)])
def test_layernorm_budget_fp16(dev, rows, c, kind, eps):
    with fp16():
        G.test_layernorm_budget(dev, rows, c, kind, eps)
    if kind == "normal" and eps == 1e-5:
        with routed_to_bf16():
            G.test_layernorm_budget(dev, rows, c, kind, eps)


@pytest.mark.parametrize("onepass", ["1", "0"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
@pytest.mark.parametrize("bsz,h,w_,c,groups", [(2, 16, 16, 320, 32), (2, 8, 8, 1280, 32), (2, 32, 32, 640, 32)])
def test_groupnorm_budget_fp16(dev, monkeypatch, bsz, h, w_, c, groups, kind, eps, onepass):
    with fp16():
        G.test_groupnorm_budget(dev, monkeypatch, bsz, h, w_, c, groups, kind, eps, onepass)
    if kind == "normal" and eps == 1e-5:
        with routed_to_bf16():
            G.test_groupnorm_budget(dev, monkeypatch, bsz, h, w_, c, groups, kind, eps, onepass)


# ------------------------------------------------------------------ elementwise
def test_geglu_silu_quick_gelu_budget_fp16(dev):
    with fp16():
        G.test_geglu_silu_quick_gelu_budget(dev)
    with routed_to_bf16():
        G.test_geglu_silu_quick_gelu_budget(dev)


@pytest.mark.parametrize("causal", [False, True])
def test_softmax_rows_budget_fp16(dev, causal):
    with fp16():
        G.test_softmax_rows_budget(dev, causal)
    with routed_to_bf16():
        G.test_softmax_rows_budget(dev, causal)


def test_cfg_ddim_budget_fp16(dev):
    with fp16():
        G.test_cfg_ddim_budget(dev)
    with routed_to_bf16():
        G.test_cfg_ddim_budget(dev)


# ------------------------------------------------------------------ fused transformer-block chains
@pytest.mark.parametrize("nsamp,ntok,nk", G.XATTN_CASES)
def test_xattn_block_budget_fp16(dev, nsamp, ntok, nk):
    with fp16():
        G.test_xattn_block_budget(dev, nsamp, ntok, nk)
    if nk == 77:
        with routed_to_bf16():
            G.test_xattn_block_budget(dev, nsamp, ntok, nk)


def test_xattn_block_residual_and_pitches_fp16(dev):
    with fp16():
        G.test_xattn_block_residual_and_pitches(dev)


@pytest.mark.parametrize("ws", ["1", "0"])
@pytest.mark.parametrize("m,f,ln", G.FF_CASES)
def test_ff_block_budget_fp16(dev, monkeypatch, m, f, ln, ws):
    with fp16():
        G.test_ff_block_budget(dev, monkeypatch, m, f, ln, ws)
    if (m, f) == (384, 1280) and ws == "1":
        with routed_to_bf16():
            G.test_ff_block_budget(dev, monkeypatch, m, f, ln, ws)


@pytest.mark.parametrize("ws", ["1", "0"])
def test_ff_block_residual_and_pitches_fp16(dev, monkeypatch, ws):
    with fp16():
        G.test_ff_block_residual_and_pitches(dev, monkeypatch, ws)


@pytest.mark.parametrize("form", ["plain", "bias", "residual"])
@pytest.mark.parametrize("n", [64, 320])
def test_gemm_as_budget_fp16(dev, n, form):
    with fp16():
        G.test_gemm_as_budget(dev, n, form)
    if n == 320:
        with routed_to_bf16():
            G.test_gemm_as_budget(dev, n, form)


@pytest.mark.parametrize("kind", ["normal", "lowvar", "offset", "const"])
def test_gemm_as_fused_layernorm_budget_fp16(dev, kind):
    with fp16():
        G.test_gemm_as_fused_layernorm_budget(dev, kind)
    if kind == "normal":
        with routed_to_bf16():
            G.test_gemm_as_fused_layernorm_budget(dev, kind)


@pytest.mark.parametrize("n", [320, 1024])
def test_gemm_as_fused_layernorm_geglu_budget_fp16(dev, n):
    with fp16():
        G.test_gemm_as_fused_layernorm_geglu_budget(dev, n)


def test_gemm_as_qkv_vt_budget_fp16(dev):
    with fp16():
        G.test_gemm_as_qkv_vt_budget(dev)
