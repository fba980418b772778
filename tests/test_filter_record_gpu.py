"""saspa_filter_record on the MI355X (ops.filter_record) against the numpy restatement of tests/filter_record_ref.py: every field of
every record bit for bit -- the fp32 margin included --, rows filed at permuted, non-contiguous slots of a table whose other rows stay
bitwise what they were, each optional input left out, invalidated images, batch invariance, and what the host wrapper refuses."""
import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops

from filter_record_ref import NAN, bits, record

pytestmark = pytest.mark.gpu

N_ROWS = 70
INF = np.float32("inf")


def _inputs(b, p, seed=0):
    rng = np.random.RandomState(100 * b + p + seed)
    sem = rng.randn(b, p).astype(np.float32)
    # constructed rows (as far as the batch and the prompt count have room for them)
    rows = []
    if p >= 7:
        t = rng.randn(p).astype(np.float32)
        t[4] = t[0] = np.float32(9.5)                                # an exact tie between index 0 and another index -> argmax 0, margin 0
        rows.append(t)
        t = rng.randn(p).astype(np.float32)
        t[0], t[2], t[5] = np.float32(-3.0), np.float32(7.25), np.float32(7.25)     # a tie among the negatives -> argmax 2
        rows.append(t)
        t = rng.randn(p).astype(np.float32)
        t[3] = NAN                                                   # a NaN at index 3 -> argmax 3, margin NaN
        rows.append(t)
        rows.append(np.full(p, np.float32(0.125)))                   # all equal -> argmax 0, margin 0
        t = rng.randn(p).astype(np.float32)
        t[1:] = -INF                                                 # every negative -inf -> margin +inf
        rows.append(t)
        rows.append(np.full(p, -INF))                                # -inf - -inf: a NaN margin the arithmetic makes itself
        t = rng.randn(p).astype(np.float32)
        t[0] = -INF
        rows.append(t)
        t = rng.randn(p).astype(np.float32)
        t[3], t[p - 1] = NAN, NAN                                    # two NaNs: the first wins
        rows.append(t)
    for k, t in enumerate(rows[:b]):
        sem[k] = t
    stats_c, stats_p = rng.rand(b, 4).astype(np.float32), rng.rand(b, 4).astype(np.float32)
    idx_c, idx_p = rng.randint(0, 200, (b, 2)).astype(np.int32), rng.randint(0, 431, (b, 2)).astype(np.int32)
    if b > 2:
        stats_c[2, 1], idx_c[2, 1] = NAN, -1                         # what class_head leaves for a label out of range
    slots = rng.permutation(N_ROWS)[:b]                              # permuted and non-contiguous
    return sem, (stats_c, idx_c), (stats_p, idx_p), slots


def _run(dev, sem, conf, pc, slots, bad=None, ld=None, table=None):
    b = len(slots)
    table = torch.full((N_ROWS, 8), float("nan"), device=dev) if table is None else table
    sem_d = None
    if sem is not None:
        p = sem.shape[1]
        buf = torch.zeros((b, ld or p), device=dev)                  # the pitch of a linear's padded output
        buf[:, :p] = torch.from_numpy(sem).to(dev)
        sem_d = buf[:, :p]
    pair = lambda q: None if q is None else (torch.from_numpy(q[0]).to(dev), torch.from_numpy(q[1]).to(dev))     # noqa: E731
    ops.filter_record(table, slots, sem_d, pair(conf), pair(pc), None if bad is None else torch.from_numpy(bad).to(dev))
    return table.cpu().numpy()


def _want(sem, conf, pc, slots, bad=None, before=None):
    out = np.full((N_ROWS, 8), NAN, np.float32) if before is None else before.copy()
    for k, s in enumerate(slots):
        out[s] = record(None if sem is None else sem[k], None if conf is None else (conf[0][k, 1], conf[1][k, 1]),
                        None if pc is None else (pc[0][k, 1], pc[1][k, 1]), bad is not None and bool(bad[k]))
    return out


@pytest.mark.parametrize("b", [1, 5, 33])
@pytest.mark.parametrize("p", [1, 7, 64])
def test_records_are_bit_equal_to_the_restatement(dev, b, p):
    sem, conf, pc, slots = _inputs(b, p)
    got = _run(dev, sem, conf, pc, slots, ld=(p + 7) // 8 * 8)
    want = _want(sem, conf, pc, slots)
    assert np.array_equal(bits(got), bits(want)), (got[slots], want[slots])
    assert (got[slots, 0] == 7).all() and (got[slots, 7] == 0).all()
    if p == 1:
        assert (got[slots, 1] == 0).all() and (got[slots, 2] == INF).all()
    if p >= 7 and b >= 5:
        assert got[slots[:4], 1].tolist() == [0, 2, 3, 0] and got[slots[0], 2] == 0 and np.isnan(got[slots[2], 2])
        assert got[slots[4], 2] == INF
    if p >= 7 and b == 33:
        assert np.isnan(got[slots[5], 2]) and got[slots[5], 1] == 0 and got[slots[6], 2] == -INF and got[slots[7], 1] == 3


def test_rows_that_are_not_addressed_stay_bitwise(dev):
    sem, conf, pc, slots = _inputs(5, 7)
    before = np.random.RandomState(3).randn(N_ROWS, 8).astype(np.float32)
    before[::3] = NAN
    before[1].view(np.uint32)[:] = 0xFFC12345                        # a NaN with a payload: a copy would keep it, arithmetic might not
    got = _run(dev, sem, conf, pc, slots, table=torch.from_numpy(before).to(dev))
    assert np.array_equal(bits(got), bits(_want(sem, conf, pc, slots, before=before)))
    rest = np.setdiff1d(np.arange(N_ROWS), slots)
    assert np.array_equal(bits(got[rest]), bits(before[rest]))


def test_bad_items_and_null_inputs(dev):
    sem, conf, pc, slots = _inputs(5, 7)
    bad = np.array([False, True, False, False, True])
    got = _run(dev, sem, conf, pc, slots, bad=bad)
    assert np.array_equal(bits(got), bits(_want(sem, conf, pc, slots, bad=bad)))
    assert got[slots[1], 0] == 0 and got[slots[4], 0] == 0 and np.isnan(got[slots[1], 1:7]).all() and got[slots[0], 0] == 7
    for use, valid, nan_cols in (((None, conf, pc), 6, [1, 2]), ((sem, None, pc), 5, [3, 4]), ((sem, conf, None), 3, [5, 6]),
                                 ((sem, None, None), 1, [3, 4, 5, 6]), ((None, None, None), 0, [1, 2, 3, 4, 5, 6])):
        got = _run(dev, *use, slots)
        assert np.array_equal(bits(got), bits(_want(*use, slots)))
        assert (got[slots, 0] == valid).all() and (bits(got[slots][:, nan_cols]) == 0x7FC00000).all()


def test_a_row_alone_equals_the_row_in_a_batch_of_33(dev):
    sem, conf, pc, slots = _inputs(33, 7)
    full = _run(dev, sem, conf, pc, slots)
    for k in (0, 2, 5, 17, 32):
        one = _run(dev, sem[k:k + 1], (conf[0][k:k + 1], conf[1][k:k + 1]), (pc[0][k:k + 1], pc[1][k:k + 1]), slots[k:k + 1])
        assert np.array_equal(bits(one[slots[k]]), bits(full[slots[k]]))


def test_the_wrapper_refuses(dev):
    sem, conf, pc, slots = _inputs(5, 7)
    table = torch.full((N_ROWS, 8), float("nan"), device=dev)
    sem_d = torch.from_numpy(sem).to(dev)
    before = table.clone()
    with pytest.raises(ValueError, match="share a slot"):
        ops.filter_record(table, [3, 9, 3, 1, 0], sem_d)
    for bad_slots in ([0, 1, 2, 3, N_ROWS], [-1, 1, 2, 3, 4]):
        with pytest.raises(ValueError, match="must lie in"):
            ops.filter_record(table, bad_slots, sem_d)
    with pytest.raises(ValueError, match="host integers"):
        ops.filter_record(table, [0.0, 1.0, 2.0, 3.0, 4.0], sem_d)
    with pytest.raises(ValueError, match="fp32"):
        ops.filter_record(table, slots, sem_d.double())
    with pytest.raises(ValueError, match="fp32"):
        ops.filter_record(table.double(), slots, sem_d)
    with pytest.raises(ValueError, match="int32"):
        ops.filter_record(table, slots, sem_d, (torch.from_numpy(conf[0]).to(dev), torch.from_numpy(conf[1]).to(dev).long()))
    with pytest.raises(ValueError, match="bool"):
        ops.filter_record(table, slots, sem_d, bad=torch.zeros(5, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="one lane per prompt"):
        ops.filter_record(table, slots, torch.zeros((5, 65), device=dev))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.filter_record(table, slots, torch.from_numpy(sem))
    torch.cuda.synchronize()
    assert torch.equal(table.view(torch.int32), before.view(torch.int32)), "a refused call wrote the table"
