"""numpy restatement of saspa_filter_record (include/saspa_hip.h): the 8 fp32 of one score record from what the kernel is handed.
CPU only; shared by tests/test_filter_record_gpu.py (bit equality with the kernel) and tests/test_filter_scores_host.py (records built
from CPU logits for `filters.decide`)."""
import numpy as np

NAN = np.float32("nan")            # the canonical quiet NaN, 0x7fc00000: what "no score" and every NaN margin are stored as


def semantic_head(logits):
    """fp32 [P] -> (argmax as numpy defines it, logit[0] - max(logit[1:]) as ONE fp32 subtraction; +inf for one prompt; a NaN
    result is the canonical NaN)."""
    lg = np.asarray(logits, np.float32)
    arg = int(np.argmax(lg))                                   # ties: the lowest index; a NaN is the maximum, the first one wins
    if lg.size == 1:
        return arg, np.float32("inf")
    with np.errstate(invalid="ignore"):
        m = np.float32(lg[0]) - np.float32(np.max(lg[1:]))      # np.max propagates a NaN
    return arg, (NAN if np.isnan(m) else np.float32(m))


def class_head_pair(logits, label):
    """What `ops.class_head` leaves for one row of fp32 logits z: (softmax(z)[label], number of z strictly greater than z[label]), the
    softmax in float64 -- the HOST form of the two entries; the device's fp32 value of the first is taken from the launch itself."""
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max())
    return np.float32(e[label] / e.sum()), int((np.asarray(logits, np.float32) > np.float32(logits[label])).sum())


def record(sem=None, conf=None, pc=None, bad=False):
    """One record.  sem: fp32 [P] logits or None; conf / pc: (p_label fp32, n_greater int) or None; bad: the image is invalidated."""
    r = np.array([0, NAN, NAN, NAN, NAN, NAN, NAN, 0], np.float32)
    if bad:
        return r
    r[0] = (1 if sem is not None else 0) | (2 if conf is not None else 0) | (4 if pc is not None else 0)
    if sem is not None:
        r[1], r[2] = semantic_head(sem)
    if conf is not None:
        r[4], r[3] = np.float32(conf[0]), np.float32(conf[1])
    if pc is not None:
        r[5], r[6] = np.float32(pc[0]), np.float32(pc[1])
    return r


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
