"""saspa_class_head on the MI355X (ops.class_head): the row of class logits, its softmax and the entries the filter decisions read,
against a float64 restatement ON THE SAME fp32 INPUTS, with rounding bounds derived here instead of tolerances.

u = 2^-24 is the unit roundoff of fp32.  For one row, in exact arithmetic: v = feat / |feat|_2,  z_c = scale * sum_d v_d t_cd,
p = exp(z_l - m) / sum_c exp(z_c - m),  m = max_c z_c.

Logits.  The kernel rounds: the sum of squares (a tree: 4 + 6 + 2 levels), the root, the reciprocal and the scaling of v (3
roundings), the D products and their sum (a tree again), the multiplication by `scale`.  A SEQUENTIAL evaluation of all of it is
covered by            |dz_c| <= (D + 4) u scale sum_d |v_d t_cd|            (Higham, Accuracy and Stability, 3.1: gamma_n <= n u
to first order; D - 1 additions + 1 product per term, + 4 for normalisation and scale), and a tree sum sits far inside it.

Softmax.  Replace every z_c by z_c + d_c, |d_c| <= ez = max_c of the bound above.  p is invariant under a common shift, so the
perturbed value lies in [p exp(-2 ez), p exp(2 ez)]: that is the "2 max|dz|" term.  On top of it the kernel rounds
  * x_c = z_c - m: one subtraction, |error| <= u |x_c| <= u X with X = max_c (m - z_c); exp turns an absolute error of its argument
    into a relative error of its value, so each term carries u X from here,
  * expf itself: the device library documents 1 ulp for expf; 2 ulp = 4 u are allowed here,
  * the sum of C positive terms: <= (C - 1) u relative, whatever the order,
  * the division: u.
Numerator and denominator each have the (u X + 4 u) term.  A factor (1 + a) is <= exp(a) and 1 / (1 - a) <= exp(2 a) (a < 1/2), so
   |dp| / p <= expm1( 2 ez + (u X + 4 u) + 2 (u X + 4 u + (C - 1) u) + 2 u ).
One more term: p below the smallest normal fp32 number (2^-126; z spreads over tens of units at scale = 100) carries no relative
precision -- the hardware may flush it -- so 2^-126 is added as an absolute floor.  log-sum-exp = m + log(s): the relative error of
s becomes an absolute one, plus 2 ulp for logf and one rounding of the sum:  |d lse| <= ez + expm1(2 (u X + 4 u + (C - 1) u)) +
4 u |log s| + u |lse|.

Argmax and n_greater are exact functions of the logits the kernel itself produced (returned with want_logits): they are compared
with numpy on THOSE logits, bit for bit; the logits against float64 by the bound."""
import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from oracle import filter_models as FM
from saspa_aug_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SCALE = 100.0


def _inputs(rows, D, C, seed, ldf_pad=8, ldc_pad=4):
    g = torch.Generator().manual_seed(seed)
    feat = torch.zeros(rows, D + ldf_pad)
    feat[:, :D] = 3.0 * torch.randn(rows, D, generator=g)
    feat[:, D:] = 1e6                                             # the pitch is not part of the row
    cls = torch.full((C, D + ldc_pad), 1e6)
    t = torch.randn(C, D, generator=g).double()
    cls[:, :D] = (t / t.norm(dim=-1, keepdim=True)).float()
    labels = torch.tensor([0 if i % 2 == 0 else C - 1 for i in range(rows)], dtype=torch.int32)
    return feat, cls, labels


def _exact(feat, cls, labels, D, scale=SCALE):
    """float64 on the fp32 inputs -> z [rows, C], p_label, lse, and the factor sum_d |v_d t_cd| of the logit bound."""
    f, t = feat[:, :D].double().numpy(), cls[:, :D].double().numpy()
    v = f / np.sqrt((f * f).sum(-1, keepdims=True))
    z = scale * v @ t.T
    absdot = np.abs(v)[:, None, :] * np.abs(t)[None]
    m = z.max(-1, keepdims=True)
    s = np.exp(z - m).sum(-1)
    lb = labels.numpy().astype(np.int64)
    zl = z[np.arange(len(lb)), lb]
    return z, np.exp(zl - m[:, 0]) / s, m[:, 0] + np.log(s), absdot.sum(-1), s


def _bounds(z, absdot, s, D, C, scale=SCALE, exact_logits=False):
    ez_c = np.zeros_like(z) if exact_logits else (D + 4) * U * scale * absdot                   # per logit
    ez = ez_c.max(-1)
    X = (z.max(-1, keepdims=True) - z).max(-1)
    term = U * X + 4 * U
    rel_p = np.expm1(2 * ez + term + 2 * (term + (C - 1) * U) + 2 * U)
    lse = z.max(-1) + np.log(s)
    abs_lse = ez + np.expm1(2 * (term + (C - 1) * U)) + 4 * U * np.abs(np.log(s)) + U * np.abs(lse)
    return ez_c, rel_p, abs_lse


def _check_rows(stats, idx, logits, labels, z, p, lse, ez_c, rel_p, abs_lse, what):
    stats, idx, lg, lb = stats.cpu().double().numpy(), idx.cpu().numpy(), logits.cpu().numpy(), labels.numpy().astype(np.int64)
    n = len(lb)
    dz = np.abs(lg.astype(np.float64) - z)
    frac_z = float((dz / np.maximum(ez_c, 1e-300)).max()) if ez_c.max() > 0 else float(dz.max())
    dp = np.abs(stats[:, 1] - p)
    bound_p = p * rel_p + 2.0 ** -126
    frac_p = float((dp / bound_p).max())
    frac_l = float((np.abs(stats[:, 3] - lse) / abs_lse).max())
    print(f"{what}: max |dz| / bound = {frac_z:.3g}, max |dp| / bound = {frac_p:.3g} (bound: {rel_p.max():.3g} relative), "
          f"max |d lse| / bound = {frac_l:.3g}")
    assert (dz <= ez_c).all(), f"{what}: logits off by {frac_z} of the bound"
    assert (dp <= bound_p).all(), f"{what}: p_label off by {frac_p} of the bound"
    assert (np.abs(stats[:, 3] - lse) <= abs_lse).all(), f"{what}: log-sum-exp off by {frac_l} of the bound"
    # the rest is exact on the kernel's own logits
    assert np.array_equal(stats[:, 0].astype(np.float32), lg[np.arange(n), lb]), what
    assert np.array_equal(stats[:, 2].astype(np.float32), lg.max(-1)), what
    assert np.array_equal(idx[:, 0], lg.argmax(-1)), what                                       # numpy: the first of equal maxima
    assert np.array_equal(idx[:, 1], (lg > lg[np.arange(n), lb][:, None]).sum(-1)), what
    assert np.isfinite(stats).all() and (stats[:, 1] >= 0).all() and (stats[:, 1] <= 1).all(), what


@pytest.mark.parametrize("rows", [1, 3, 33])
@pytest.mark.parametrize("C", [1, 6, 7, 200, 257])
@pytest.mark.parametrize("D", [32, 1000, 1024])
def test_embedding_mode_within_the_rounding_bounds(dev, D, C, rows):
    feat, cls, labels = _inputs(rows, D, C, seed=1000 * D + 10 * C + rows)
    z, p, lse, absdot, s = _exact(feat, cls, labels, D)
    stats, idx, logits = ops.class_head(feat.to(dev), labels.to(dev), cls.to(dev), SCALE, True, width=D, want_logits=True)
    assert stats.shape == (rows, 4) and idx.shape == (rows, 2) and logits.shape == (rows, C)
    _check_rows(stats, idx, logits, labels, z, p, lse, *_bounds(z, absdot, s, D, C), what=f"D={D} C={C} rows={rows}")
    if C == 1:
        assert (stats[:, 1] == 1.0).all() and (idx == 0).all()


def test_normalize_off_takes_the_rows_as_they_are(dev):
    D, C, rows = 64, 9, 5
    feat, cls, labels = _inputs(rows, D, C, seed=5)
    unit = torch.zeros_like(feat)
    unit[:, :D] = (feat[:, :D].double() / feat[:, :D].double().norm(dim=-1, keepdim=True)).float()
    z = SCALE * unit[:, :D].double().numpy() @ cls[:, :D].double().numpy().T
    _, _, logits = ops.class_head(unit.to(dev), labels.to(dev), cls.to(dev), SCALE, False, width=D, want_logits=True)
    absdot = (np.abs(unit[:, :D].double().numpy())[:, None] * np.abs(cls[:, :D].double().numpy())[None]).sum(-1)
    assert (np.abs(logits.cpu().double().numpy() - z) <= (D + 4) * U * SCALE * absdot).all()


def test_stability_when_the_embedding_is_a_class_row(dev):
    """z_label is about 100: exp(z) without the subtraction of the maximum overflows fp32 (exp(88.7) is the largest finite)."""
    D, C = 1024, 200
    _, cls, _ = _inputs(1, D, C, seed=11)
    picks = [0, 57, C - 1]
    feat = torch.zeros(len(picks), D)
    for i, c in enumerate(picks):
        feat[i] = 7.25 * cls[c, :D]
    labels = torch.tensor(picks, dtype=torch.int32)
    z, p, lse, absdot, s = _exact(feat, cls, labels, D)
    assert (z.max(-1) > 99).all()
    stats, idx, logits = ops.class_head(feat.to(dev), labels.to(dev), cls.to(dev), SCALE, True, width=D, want_logits=True)
    st = stats.cpu().numpy()
    assert np.isfinite(st).all() and (st[:, 1] > 0).all() and (st[:, 1] <= 1).all()
    assert (idx.cpu().numpy()[:, 0] == np.array(picks)).all() and (idx.cpu().numpy()[:, 1] == 0).all()
    _check_rows(stats, idx, logits, labels, z, p, lse, *_bounds(z, absdot, s, D, C), what="embedding == class row")
    # a label far from the embedding: p underflows towards 0 but stays finite and non-negative
    far = torch.tensor([(c + 1) % C for c in picks], dtype=torch.int32)
    st = ops.class_head(feat.to(dev), far.to(dev), cls.to(dev), SCALE, True, width=D)[0].cpu().numpy()
    assert np.isfinite(st).all() and (st[:, 1] >= 0).all() and (st[:, 1] < 1e-6).all()


def test_ties_lowest_index_wins_and_equal_logits_are_not_greater(dev):
    D, C = 32, 7
    _, cls, _ = _inputs(1, D, C, seed=12)
    cls[5] = cls[2]                                             # two identical class rows
    feat = (4.0 * cls[2, :D]).repeat(3, 1).contiguous()         # the embedding is that row: both reach the maximum
    labels = torch.tensor([5, 2, 0], dtype=torch.int32)
    stats, idx, logits = ops.class_head(feat.to(dev), labels.to(dev), cls.to(dev), SCALE, True, width=D, want_logits=True)
    lg, ix, st = logits.cpu().numpy(), idx.cpu().numpy(), stats.cpu().numpy()
    assert (lg[:, 2] == lg[:, 5]).all() and (lg.max(-1) == lg[:, 2]).all()
    assert ix[:, 0].tolist() == [2, 2, 2]                       # the lower index
    assert ix[:, 1].tolist() == [0, 0, 2]                       # an equal logit is not "greater"; for label 0 both maxima are
    assert st[0, 1] == st[1, 1] and 0.49 < st[0, 1] <= 0.5


def test_rows_do_not_depend_on_their_batch_and_launches_repeat(dev):
    D, C, rows = 1000, 257, 33
    feat, cls, labels = _inputs(rows, D, C, seed=13)
    f, t, lb = feat.to(dev), cls.to(dev), labels.to(dev)
    a = ops.class_head(f, lb, t, SCALE, True, width=D, want_logits=True)
    b = ops.class_head(f, lb, t, SCALE, True, width=D, want_logits=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "repeat launches are bit-identical"
    for i in (0, 1, 16, 32):
        one = ops.class_head(f[i:i + 1].contiguous(), lb[i:i + 1].contiguous(), t, SCALE, True, width=D, want_logits=True)
        for x, y in zip(a, one):
            assert torch.equal(x[i:i + 1], y), f"row {i} alone == row {i} of the batch of {rows}"


def test_label_out_of_range_marks_the_row_only(dev):
    D, C, rows = 32, 6, 4
    feat, cls, labels = _inputs(rows, D, C, seed=14)
    good = ops.class_head(feat.to(dev), labels.to(dev), cls.to(dev), SCALE, True, width=D, want_logits=True)
    bad = labels.clone()
    bad[1], bad[2] = C, -1
    stats, idx, logits = ops.class_head(feat.to(dev), bad.to(dev), cls.to(dev), SCALE, True, width=D, want_logits=True)
    assert torch.isnan(stats[1:3]).all() and (idx[1:3] == -1).all()
    assert torch.equal(stats[[0, 3]], good[0][[0, 3]]) and torch.equal(idx[[0, 3]], good[1][[0, 3]]) and torch.equal(logits, good[2])


@pytest.mark.parametrize("C", [2, 6, 100, 196])
def test_logits_mode_top_k_and_softmax(dev, C):
    rows = 33
    g = torch.Generator().manual_seed(20 + C)
    ld = (C + 7) // 8 * 8 + 8
    buf = torch.full((rows, ld), 1e6)
    buf[:, :C] = 5.0 * torch.randn(rows, C, generator=g)
    labels = torch.randint(0, C, (rows,), generator=g, dtype=torch.int32)
    labels[0], labels[1] = 0, C - 1
    stats, idx, logits = ops.class_head(buf.to(dev), labels.to(dev), width=C, want_logits=True)
    lg = buf[:, :C]
    assert torch.equal(logits.cpu(), lg), "scale = 1: the logits pass through"
    ng = idx.cpu().numpy()[:, 1]
    for k in (1, 3, 10):
        want = [FM.confidence_pass(lg[i:i + 1], int(labels[i]), k) for i in range(rows)]
        assert (ng < min(k, C)).tolist() == want, k
    z = lg.double().numpy()
    m = z.max(-1)
    s = np.exp(z - m[:, None]).sum(-1)
    p = np.exp(z[np.arange(rows), labels.numpy().astype(np.int64)] - m) / s
    ez_c, rel_p, abs_lse = _bounds(z, None, s, C, C, scale=1.0, exact_logits=True)
    _check_rows(stats, idx, logits, labels, z, p, m + np.log(s), ez_c, rel_p, abs_lse, what=f"logits mode C={C}")


def test_wrapper_refuses_what_the_kernel_cannot_take(dev):
    feat, cls, labels = _inputs(2, 32, 6, seed=30)
    with pytest.raises(ValueError):
        ops.class_head(feat.to(dev), labels.to(dev).long(), cls.to(dev), width=32)
    with pytest.raises(ValueError):
        ops.class_head(feat.to(dev), labels.to(dev), cls.to(dev)[:, :16], width=32)
    with pytest.raises(ValueError):
        ops.class_head(torch.zeros(2, 4104, device=dev), labels.to(dev))                        # more classes than LDS holds
    with pytest.raises(RuntimeError):
        ops.class_head(feat, labels, cls)                                                      # host tensors
