"""saspa_flash_attn_f32x3 on the GPU against the float64 reference, within the table of tests/attn_x3_ref.py (proven on the CPU by
tests/test_attn_x3_host.py): every case, then against the unfused fp32 path, batch independence, no score matrix, graph capture."""
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import models, ops
from tests import attn_x3_ref as A
from tests import errbudget as E

pytestmark = pytest.mark.gpu
MIB = 1 << 20


def _slice_of_wider(t, dev, right):
    """t [b, n, c] -> the same values as a column slice of a [b, n, 2 c] device buffer (pitch 2 c > c) whose other half is huge."""
    b, n, c = t.shape
    wide = torch.full((b, n, 2 * c), 1e30, dtype=torch.float32, device=dev)
    view = wide[:, :, c:] if right else wide[:, :, :c]
    view.copy_(t)
    return view


def _vt(v, dev, fill):
    """v [b, nk, c] -> V^T [b, c, round8(nk)] on the device, the pad columns holding `fill`."""
    b, nk, c = v.shape
    vt = torch.full((b, c, ops.round8(nk)), fill, dtype=torch.float32, device=dev)
    vt[:, :, :nk] = v.transpose(1, 2)
    return vt


def _device_operands(case, dev, seed=0, pad=float("nan")):
    q, k, v, scale, _, _ = A.case_data(case, seed)
    return _slice_of_wider(q, dev, False), _slice_of_wider(k, dev, True), _vt(v, dev, pad), scale


def _fused(case, dev):
    b, heads, nq, nk, d, causal = case
    q, k, vt, scale = _device_operands(case, dev)                # pad keys of V^T are NaN: the kernel must not let them in
    out = torch.full((b, nq, heads * d), float("nan"), dtype=torch.float32, device=dev)
    return ops.flash_attn_f32x3(q, k, vt, out, heads, d, nq, nk, scale, causal)


@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_kernel_within_the_table(dev, case):
    got = _fused(case, dev)
    st = A.check(got, case)
    print(f"\n[attn x3] {A.case_id(case)}: {E.fmt(st)} ratio {E.ratio(st, A.LIMITS):.3f}")


@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
def test_fused_against_the_unfused_fp32_path(dev, case):
    """attention_core with the mode off (exact fp32 GEMMs, row softmax) and on: the difference stays within the sum of the two
    paths' allowances -- the unfused path is granted the same table, which exact fp32 arithmetic uses a hundredth of."""
    b, heads, nq, nk, d, causal = case
    q, k, vt, _ = _device_operands(case, dev, pad=0.0)           # (the unfused PV GEMM sums over the pad columns: zeros there)
    unfused = models.attention_core(q, k, vt, heads, nq, nk, causal=causal)
    with ops.f32_attn_mode("fused"):
        fused = models.attention_core(q, k, vt, heads, nq, nk, causal=causal)
    *_, ref, s = A.case_data(case)
    both = {key: 2.0 * val for key, val in A.LIMITS.items()}
    st_u = E.check_budget(unfused, ref, s, A.UNIT, limits=A.LIMITS, what=f"unfused {A.case_id(case)}")
    st = E.check_budget(fused, unfused.double().cpu(), s, A.UNIT, limits=both, what=f"fused vs unfused {A.case_id(case)}")
    print(f"\n[attn x3] {A.case_id(case)}: unfused vs float64 {E.fmt(st_u)}; fused vs unfused {E.fmt(st)}")


def test_mode_off_is_the_unfused_path_and_wide_heads_stay_there(dev):
    kinds = []
    ops.set_recorder(lambda kind, flops, call, meta: kinds.append(kind) or call())
    try:
        q = torch.randn(1, 16, 384, device=dev)
        vt = torch.randn(1, 384, 16, device=dev)
        models.attention_core(q[:, :, :64], q[:, :, 64:128], vt[:, :64], 1, 16, 16)
        assert "flash_attn_f32x3" not in kinds and "softmax_rows" in kinds, kinds
        del kinds[:]
        with ops.f32_attn_mode("fused"):
            models.attention_core(q[:, :, :64], q[:, :, 64:128], vt[:, :64], 1, 16, 16)
            assert kinds == ["flash_attn_f32x3"], kinds
            del kinds[:]
            models.attention_core(q[:, :, :192], q[:, :, 192:], vt[:, :192], 1, 16, 16)     # d = 192 > 160
            assert "flash_attn_f32x3" not in kinds and "softmax_rows" in kinds, kinds
    finally:
        ops.set_recorder(None)


def test_batch_entry_alone_equals_the_entry_in_a_batch_of_three(dev):
    heads, nq, nk, d = 3, 100, 77, 40
    q, k, v = A.operands(3, heads, nq, nk, d, seed=5)
    scale = d ** -0.5
    qd, kd, vtd = _slice_of_wider(q, dev, False), _slice_of_wider(k, dev, True), _vt(v, dev, float("nan"))
    full = ops.flash_attn_f32x3(qd, kd, vtd, torch.empty(3, nq, heads * d, device=dev), heads, d, nq, nk, scale)
    for e in range(3):
        alone = ops.flash_attn_f32x3(qd[e:e + 1], kd[e:e + 1], vtd[e:e + 1].contiguous(), torch.empty(1, nq, heads * d, device=dev),
                                     heads, d, nq, nk, scale)
        assert torch.equal(alone[0], full[e]), e
    assert torch.isfinite(full).all()


def test_no_score_matrix(dev):
    """B = 2, 8 heads, 2048 x 2048, d = 40: the unfused path's scores are 256 MiB; the fused launch allocates the output only."""
    b, heads, n, d = 2, 8, 2048, 40
    c = heads * d
    g = torch.Generator(device=dev).manual_seed(3)
    q = torch.randn(b, n, c, device=dev, generator=g)
    k = torch.randn(b, n, c, device=dev, generator=g)
    vt = torch.randn(b, c, n, device=dev, generator=g)

    def peak_growth():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = models.attention_core(q, k, vt, heads, n, n)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    grown_unfused, ref = peak_growth()
    with ops.f32_attn_mode("fused"):
        grown_fused, out = peak_growth()
    out_bytes = b * n * c * 4
    print(f"\n[attn x3] peak growth: unfused {grown_unfused / MIB:.1f} MiB, fused {grown_fused / MIB:.1f} MiB (output {out_bytes / MIB:.1f} MiB)")
    assert grown_unfused >= 256 * MIB
    assert grown_fused <= out_bytes + 16 * MIB
    # the same attention: |o| <= max |v| ~ 5 and a product is off by 2^-17, the logits' share a few times that -- 1e-3 is a plumbing
    # check (a wrong head stride or mask is O(1)); the budget tests carry the precision
    assert (out - ref).abs().max().item() < 1e-3


def test_graph_capture_replays_the_eager_bits(dev):
    case = A.CASES[1]
    b, heads, nq, nk, d, causal = case
    q, k, vt, scale = _device_operands(case, dev)
    out = torch.zeros(b, nq, heads * d, device=dev)

    def step():
        return ops.flash_attn_f32x3(q, k, vt, out, heads, d, nq, nk, scale, causal)
    eager = step().clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    A.check(out, case)
