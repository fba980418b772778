"""saspa_attn_wide on the MI355X, in both libraries (bf16: libsaspa_hip.so, fp16: libsaspa_hip_f16.so): every case of
tests/attn_wide_ref.CASES against the float64 reference within the budget of that file, strided operands out of one Q | K | V
buffer, batch independence bit for bit, unscaled logits far beyond the fp16 range, and the host-side refusals."""
import pytest
import torch

from saspa_aug_amd import models, ops
from tests import attn_wide_ref as R
from tests import errbudget as E

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)


def _run(q, k, v, dev, out=None):
    q, k, v = (t.to(dev) for t in (q, k, v))
    if out is None:
        out = torch.empty(q.shape, device=dev, dtype=q.dtype)
    ops.attn_wide(q, k, v, out, q.shape[1], k.shape[1], q.shape[2] ** -0.5)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: R.NAME[d])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_cases_within_budget(dev, case, dt):
    q, k, v, scale, idx, ref, s = R.case_data(case, dt)
    got = _run(q, k, v, dev)[:, idx.to(dev)].cpu()
    st = E.budget_stats(got, ref, s, R.UNIT[dt])
    print(f"attn_wide {R.NAME[dt]} {R.case_id(case)}: {E.fmt(st)}  ratio {E.ratio(st, R.limits_for(dt)):.3f}")
    R.check(got, case, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: R.NAME[d])
def test_strided_operands_of_one_qkv_buffer(dev, dt):
    """q, k, v are column slices of one [B, n, 3 * 512] buffer and out is a slice of a wider one: pitches and batch strides differ
    from the width, the result equals the contiguous launch bit for bit and nothing outside out's columns is written."""
    q, k, v, *_ = R.case_data(R.CASES[1], dt)                 # B = 2, nq = 100, nk = 77
    n, d = k.shape[1], k.shape[2]
    q = q[:, :n]
    buf = torch.cat([q, k, v], -1).to(dev).contiguous()        # [2, 77, 1536]
    wide = torch.full((2, n, d + 40), 7.0, device=dev, dtype=dt)
    out = wide[:, :, :d]
    ops.attn_wide(buf[:, :, :d], buf[:, :, d:2 * d], buf[:, :, 2 * d:], out, n, n, d ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(out, _run(q, k, v, dev))
    assert bool((wide[:, :, d:] == 7.0).all())
    ref, s = R.ref64(q, k, v, d ** -0.5)
    E.check_budget(out, ref, R.scale_for(s, dt), R.UNIT[dt], limits=R.limits_for(dt), what=f"strided {R.NAME[dt]}")


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: R.NAME[d])
def test_batch_entry_is_independent_of_batch_and_slot(dev, dt):
    q, k, v, *_ = R.case_data(R.CASES[1], dt)                 # two entries of 100 x 77 x 512
    x = [t[:1] for t in (q, k, v)]
    y = [t[1:] for t in (q, k, v)]
    alone = _run(*x, dev)
    for slot in range(3):
        parts = [y, y, y]
        parts[slot] = x
        got = _run(*(torch.cat([p[i] for p in parts]) for i in range(3)), dev)
        assert torch.equal(got[slot:slot + 1], alone), f"slot {slot}"


def _large_logit_operands(dt, nq=64, nk=200, d=512, seed=5):
    """q . k is about 2 x 10^5 (channel 0: 448 x 448 = 200 704, exact in both 16-bit types) while the scaled logits differ by the
    other 511 channels only: standard deviation 1, a span of about 7 over 200 keys."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.randn(1, nq, d, generator=g), torch.randn(1, nk, d, generator=g), torch.randn(1, nk, d, generator=g)
    q[..., 0] = 448.0
    k[..., 0] = 448.0
    return q.to(dt), k.to(dt), v.to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: R.NAME[d])
def test_large_unscaled_logits(dev, dt):
    q, k, v = _large_logit_operands(dt)
    d = q.shape[2]
    raw = q.double() @ k.double().transpose(-1, -2)
    assert raw.min().item() > 1.9e5 and (raw.max() - raw.min()).item() * d ** -0.5 < 30.0
    ref, s = R.ref64(q, k, v, d ** -0.5)
    got = _run(q, k, v, dev)
    assert bool(torch.isfinite(got).all())
    st = E.check_budget(got, ref, R.scale_for(s, dt), R.UNIT[dt], limits=R.limits_for(dt), what=f"large logits {R.NAME[dt]}")
    print(f"attn_wide {R.NAME[dt]} large logits: {E.fmt(st)}")
    if dt == torch.float16:
        # the reason for the kernel: the unfused path stores the unscaled q . k in fp16.  It computes infinities (NaN after the
        # softmax), it does not fault.
        qd, kd, vd = (t.to(dev) for t in (q, k, v))
        unfused = models.attention_core(qd, kd, vd.transpose(1, 2).contiguous(), 1, q.shape[1], k.shape[1])
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(unfused).all())


def _refused(dev, q, k, v, nq, nk):
    out = torch.full(q.shape, 3.0, device=dev, dtype=q.dtype)
    with pytest.raises(RuntimeError, match="SASPA_EINVAL"):
        ops.attn_wide(q, k, v, out, nq, nk, 1.0)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), "a refused call must not launch"


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: R.NAME[d])
def test_refusals(dev, dt):
    mk = lambda n, d, t=dt: torch.ones(1, n, d, device=dev, dtype=t)      # noqa: E731
    _refused(dev, mk(64, 40), mk(64, 40), mk(64, 40), 64, 64)              # narrower heads belong to the flash kernels
    _refused(dev, mk(64, 576), mk(64, 576), mk(64, 576), 64, 64)           # wider than 512
    _refused(dev, mk(64, 512), mk(64, 512), mk(64, 512), 64, 0)            # no keys
    if dt == torch.bfloat16:                                               # fp32 tensors reach the default library, which refuses
        f = torch.float32
        _refused(dev, mk(64, 512, f), mk(64, 512, f), mk(64, 512, f), 64, 64)
