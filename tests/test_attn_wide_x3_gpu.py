"""saspa_attn_wide_f32x3 on the MI355X against the float64 reference, within the table of tests/attn_wide_x3_ref.py (proven on the CPU
by tests/test_attn_wide_x3_host.py): every case, operands as slices of one Q | K | V buffer and as three tensors of different pitches,
activations near 30, NaNs behind the last key, batch independence bit for bit, graph capture, and the refusals."""
import pytest
import torch

from saspa_aug_amd import ops
from tests import attn_wide_x3_ref as R
from tests import errbudget as E

pytestmark = pytest.mark.gpu


def _run(q, k, v, dev, out=None, nq=None, nk=None):
    q, k, v = (t.to(dev) for t in (q, k, v))
    if out is None:
        out = torch.empty(q.shape, device=dev, dtype=q.dtype)
    ops.attn_wide_x3(q, k, v, out, nq or q.shape[1], nk or k.shape[1], q.shape[2] ** -0.5)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_cases_within_budget(dev, case):
    q, k, v, scale, ref, s = R.case_data(case)
    got = _run(q, k, v, dev).cpu()
    st = R.stats(got, case)
    print(f"attn_wide_x3 {R.case_id(case)}: {E.fmt(st)}  ratio {E.ratio(st, R.LIMITS):.3f}")
    R.check(got, case)


def test_slices_of_one_qkv_buffer_and_separate_pitches(dev):
    """B3-nq40-nk257-d320: q, k, v as column slices of one [n][3 d] buffer (out a slice of a wider one), then as three tensors of
    three different pitches: both equal the contiguous launch bit for bit and nothing outside out's columns is written."""
    case = R.CASES[3]
    q, k, v, scale, ref, s = R.case_data(case)
    b, nq, nk, d = case
    plain = _run(q, k, v, dev)
    R.check(plain.cpu(), case)
    buf = torch.zeros(b, nk, 3 * d, device=dev)
    buf[:, :nq, :d], buf[:, :, d:2 * d], buf[:, :, 2 * d:] = q.to(dev), k.to(dev), v.to(dev)
    wide = torch.full((b, nq, d + 40), 7.0, device=dev)
    ops.attn_wide_x3(buf[:, :nq, :d], buf[:, :, d:2 * d], buf[:, :, 2 * d:], wide[:, :, :d], nq, nk, scale)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :, :d], plain) and bool((wide[:, :, d:] == 7.0).all())
    hold = [torch.zeros(b, t.shape[1] + extra, d + pad, device=dev) for t, extra, pad in ((q, 0, 4), (k, 2, 64), (v, 1, 12))]
    for h, t in zip(hold, (q, k, v)):
        h[:, :t.shape[1], :d] = t.to(dev)
    views = [h[:, :t.shape[1], :d] for h, t in zip(hold, (q, k, v))]
    assert len({x.stride(1) for x in views}) == 3 and len({x.stride(0) for x in views}) == 3
    assert torch.equal(_run(*views, dev), plain)


def test_activations_near_30(dev):
    q, k, v = R.large_operands()
    d = q.shape[2]
    ref, s = R.ref64(q, k, v, d ** -0.5)
    got = _run(q, k, v, dev).cpu()
    assert bool(torch.isfinite(got).all())
    st = E.check_budget(got, ref, s, R.UNIT, limits=R.LIMITS, what="activations near 30")
    print(f"attn_wide_x3 activations near 30: {E.fmt(st)}  ratio {E.ratio(st, R.LIMITS):.3f}")


def test_nans_behind_the_last_key_change_no_bit(dev):
    """The rows behind nk of K and V (the rest of the last 32-key tile and beyond) are never read."""
    case = R.CASES[1]                                       # nk = 65: 31 pad keys in the last tile
    q, k, v, *_ = R.case_data(case)
    nk = k.shape[1]
    clean = _run(q, k, v, dev)
    kn = torch.full((k.shape[0], nk + 40, k.shape[2]), float("nan"), device=dev)
    vn = kn.clone()
    kn[:, :nk], vn[:, :nk] = k.to(dev), v.to(dev)
    assert torch.equal(_run(q, kn, vn, dev, nk=nk), clean)


def test_batch_entry_is_independent_of_batch_and_slot(dev):
    q, k, v, *_ = R.case_data(R.CASES[1])                   # two entries of 33 x 65 x 192
    x = [t[:1] for t in (q, k, v)]
    y = [t[1:] for t in (q, k, v)]
    alone = _run(*x, dev)
    for slot in range(3):
        parts = [y, y, y]
        parts[slot] = x
        got = _run(*(torch.cat([p[i] for p in parts]) for i in range(3)), dev)
        assert torch.equal(got[slot:slot + 1], alone), f"slot {slot}"


def test_capturable(dev):
    case = R.CASES[2]
    q, k, v, scale, *_ = R.case_data(case)
    eager = _run(q, k, v, dev)
    qd, kd, vd = (t.to(dev) for t in (q, k, v))
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_wide_x3(qd, kd, vd, out, q.shape[1], k.shape[1], scale)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attn_wide_x3(qd, kd, vd, out, q.shape[1], k.shape[1], scale)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def _refused(dev, code, q, k, v, out, nq, nk):
    before = out.clone() if out.is_contiguous() else out.contiguous()
    with pytest.raises(RuntimeError, match=code):
        ops.attn_wide_x3(q, k, v, out, nq, nk, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(out.contiguous(), before), "a refused call must not write"


def test_refusals_write_nothing(dev):
    mk = lambda n, d: torch.full((1, n, d), 3.0, device=dev)      # noqa: E731
    for d in (128, 160, 200, 576):                                 # narrower, not a multiple of 64, wider than 512
        _refused(dev, "SASPA_EINVAL", mk(64, d), mk(64, d), mk(64, d), mk(64, d), 64, 64)
    t = mk(64, 256)
    _refused(dev, "SASPA_EINVAL", t, t, t, mk(64, 256), 64, 0)     # no keys
    _refused(dev, "SASPA_EINVAL", t, t, t, mk(64, 256), 0, 64)     # no queries
    _refused(dev, "SASPA_EINVAL", t[:0], t[:0], t[:0], mk(64, 256), 64, 64)                 # empty batch
    big = torch.zeros(65536, 1, 192, device=dev)
    _refused(dev, "SASPA_EINVAL", big, big, big, torch.full((65536, 1, 192), 3.0, device=dev), 1, 1)   # batch > 65535
    short = torch.full((4096,), 3.0, device=dev).as_strided((1, 8, 256), (2048, 192, 1))    # rows overlap: a pitch shorter than d
    _refused(dev, "SASPA_EINVAL", short, t, t, mk(8, 256), 8, 8)
    # misaligned: a pointer 4 bytes off, a pitch that is no multiple of 4, a batch stride that is no multiple of 4
    w = mk(64, 260)
    _refused(dev, "SASPA_EALIGN", w[:, :, 1:257], t, t, mk(64, 256), 64, 64)
    _refused(dev, "SASPA_EALIGN", t, w[:, :, 2:258], t, mk(64, 256), 64, 64)
    _refused(dev, "SASPA_EALIGN", t, t, t, w[:, :, 3:259], 64, 64)
    odd = torch.full((1, 64, 258), 3.0, device=dev)
    _refused(dev, "SASPA_EALIGN", t, t, odd[:, :, :256], mk(64, 256), 64, 64)
    two = torch.full((2, 1, 258), 3.0, device=dev)                 # pitch and batch stride 258
    _refused(dev, "SASPA_EALIGN", two[:, :, :256], two[:, :, :256], two[:, :, :256], torch.full((2, 1, 256), 3.0, device=dev), 1, 1)
    with pytest.raises(TypeError, match="fp32 path"):
        h = torch.ones(1, 64, 256, device=dev, dtype=torch.bfloat16)
        ops.attn_wide_x3(h, h, h, h, 64, 64, 1.0)
