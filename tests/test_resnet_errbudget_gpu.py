"""The ResnetBlock2D path under the rounding-error budget (tests/errbudget.py) on the MI355X: every conv epilogue form that
models.resnet() launches, the GroupNorm statistics the epilogues leave, GroupNorm fed by them, conv -> GroupNorm -> SiLU in one launch
(saspa_splitk_groupnorm) and GroupNorm -> SiLU -> conv in one launch (saspa_conv3x3_halo) next to the two launches it replaces.  The
float64 references, their rounding points (each cited to its source line) and the magnitudes are tests/resnet_ref.py's; the limits are
proven on the CPU by tests/test_errbudget.py.  Which kernel ran is read from the library's own plan (saspa_gemm_which, through the ops
launch recorder) and eligibility from its own *_eligible calls (ops.conv_gn returns None otherwise).  Every family launches once with
one argument perturbed -- an ordinary valid launch -- and the budget must REJECT that result against the unperturbed reference."""
import contextlib

import pytest
import torch

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from tests import resnet_ref as R
from tests.errbudget import LIMITS, UNIT_BF16, check_budget, fmt, norm_scale, ratio, rejects
from tests.test_errbudget import _norm_inputs, _rand

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SILU = ops.ACT_SILU
FAMILY_NAME = {ops.GEMM_TILED: "tiled", ops.GEMM_WIDE: "wide"}


def _check(got, ref, s, family, what, unit=UNIT_BF16):
    st = check_budget(got, ref, s, unit, limits=LIMITS[family], what=what)
    print(f"\n[budget] {family:8s} x{ratio(st, LIMITS[family]):.3f} {what}: {fmt(st)}")
    return st


def _control(got, ref, s, family, what, unit=UNIT_BF16):
    assert rejects(got, ref, s, unit, limits=LIMITS[family]), f"negative control not rejected: {what}"
    print(f"\n[control rejected] {family:8s} {what}")


class _Recorder:
    """The ops launch recorder: (kind, meta) of every launch; a GEMM's meta ends in (kernel family, K slices) of the library's plan."""

    def __init__(self):
        self.log = []

    def __call__(self, kind, flops, call, meta):
        self.log.append((kind, meta))
        return call()

    def conditional(self, kind, flops, run, meta, ran):
        rc = run()
        if ran(rc):
            self.log.append((kind, meta))
        return rc

    def kinds(self):
        return [k for k, _ in self.log]

    def gemm_plan(self):
        """(kernel family, K slices) of the ONE GEMM launch recorded."""
        plans = [m[-2:] for k, m in self.log if k == "gemm"]
        assert len(plans) == 1, self.log
        return plans[0]


@contextlib.contextmanager
def _recording():
    rec = _Recorder()
    ops.set_recorder(rec)
    try:
        yield rec
    finally:
        ops.set_recorder(None)


def _dev_weights(op, dev, order):
    """[N, C, kh, kw] -> the packed device weights in tap-major ("tap"), chunk-major ("chunk") or chunk32-major order."""
    pk = W.pack_conv(op["w"].float())
    taps = op["kh"] * op["kh"]
    if order == "chunk":
        wt = W.to_chunk_major(pk, taps, BF).to(dev, BF)
        wt.saspa_korder = 1
        return wt
    return (W.to_chunk32_major(pk) if order == "chunk32" else pk).to(dev, BF)


def _d(t, dev, dtype=BF):
    return None if t is None else t.to(dev, dtype).contiguous()


def _conv(op, dev, *, variant=0, ksplit=None, gn_unit=None, x=None, alpha=None, rowvec=None, residual=None, bias=None, fuse_gn=None):
    """ops.conv of the operands (chunk-major weights where every source has whole 64-channel K-tiles) -> (device output, recorder)."""
    kh = op["kh"]
    c0, c1 = (op["x"].shape[-1], 0 if op["x2"] is None else op["x2"].shape[-1]) if x is None else (x.shape[-1], 0)
    chunk = kh == 3 and c0 % 64 == 0 and c1 % 64 == 0
    wt = _dev_weights(op, dev, "chunk" if chunk else "tap")
    rv = op["rowvec"] if rowvec is None else rowvec
    res = op["res"] if residual is None else residual
    b = op["bias"] if bias is None else bias
    with _recording() as rec:
        out = ops.conv(_d(op["x"], dev) if x is None else x, wt, _d(b, dev, torch.float32), kh=kh, kw=kh, stride=op["stride"],
                       pad=kh // 2, x2=_d(op["x2"], dev) if x is None else None, rowvec=_d(rv, dev, torch.float32),
                       residual=_d(res, dev), alpha=op["alpha"] if alpha is None else alpha, variant=variant, ksplit=ksplit,
                       gn_unit=gn_unit, fuse_gn=fuse_gn)
    return out, rec


# ------------------------------------------------------------------ conv epilogue forms (family gemm)
CONV_FORMS = [(i, f) for i, f in enumerate(R.CONV_FORMS)] + [(len(R.CONV_FORMS) + i, f) for i, f in enumerate(R.CONV_FORMS_GPU_ONLY)]


@pytest.mark.parametrize("variant", [ops.GEMM_AUTO, ops.GEMM_WIDE], ids=["auto", "wide"])
@pytest.mark.parametrize("i,form", CONV_FORMS, ids=[f"{f[0].replace(' ', '_')}-{f[1]}x{f[2]}x{f[3]}" for _, f in CONV_FORMS])
def test_conv_epilogue_budget(dev, i, form, variant):
    name, b, h, w_, c0, c1, n, kh, stride, flags = form
    op = R.conv_operands(_rand, form, 400 + 10 * i)
    for ks in ((2, 3) if "ks" in flags else (None,)):
        # K slices end in the reduce launch: one rounding (no residual in that form: the same reference either way)
        ref, s = R.conv_ref(op, two_roundings=ks is None)
        out, rec = _conv(op, dev, variant=variant, ksplit=ks)
        fam, got_ks = rec.gemm_plan()
        if variant == ops.GEMM_WIDE and n > 32:                  # (N <= 32 runs on the small 4-wave tile whatever the pin)
            assert fam == ops.GEMM_WIDE, f"pinned WIDE, the library planned family {fam}"
        if ks:
            assert got_ks == ks, f"asked for {ks} K slices, the library planned {got_ks}"
        tag = f"conv {name} {b}x{h}x{w_}x{c0}+{c1}->{n} {kh}x{kh} {FAMILY_NAME.get(fam, fam)} ks {got_ks}"
        _check(out.cpu()[..., :n], ref, s, "gemm", tag)
    if name == "multi-image tile" and b == 5:
        # negative controls: alpha x (1 + 2^-7), residual x (1 + 2^-6), the row vectors of images 1 and 2 swapped
        ref, s = R.conv_ref(op)
        _control(_conv(op, dev, variant=variant, alpha=op["alpha"] * (1 + 2 ** -7))[0].cpu()[..., :n], ref, s, "gemm",
                 f"conv {name} with alpha x (1 + 2^-7)")
        _control(_conv(op, dev, variant=variant, residual=op["res"] * (1 + 2 ** -6))[0].cpu()[..., :n], ref, s, "gemm",
                 f"conv {name} with residual x (1 + 2^-6)")
        rv = op["rowvec"].clone()
        rv[[1, 2]] = rv[[2, 1]]
        _control(_conv(op, dev, variant=variant, rowvec=rv)[0].cpu()[..., :n], ref, s, "gemm",
                 f"conv {name} with the row vectors of two images swapped")


# ------------------------------------------------------------------ epilogue statistics (family gnstat)
STAT_FORMS = [(500 + 10 * i, f, None) for i, f in enumerate(R.GNSTAT_FORMS)] + \
    [(440, R.CONV_FORMS[4], None), (450, R.CONV_FORMS[5], None), (460, R.CONV_FORMS[6], 2), (460, R.CONV_FORMS[6], 3),
     (530, ("wide_splitk", 1, 16, 16, 256, 0, 320, 3, 1, ""), 2)]


@pytest.mark.parametrize("variant", [ops.GEMM_TILED, ops.GEMM_WIDE], ids=["tiled", "wide"])
@pytest.mark.parametrize("seed,form,ks", STAT_FORMS, ids=[f"{f[0].replace(' ', '_')}-{f[1]}x{f[2]}x{f[3]}x{f[4]}-ks{k}" for _, f, k in STAT_FORMS])
def test_epilogue_statistics_budget(dev, seed, form, ks, variant):
    """gn_stats against float64 sums of the STORED output, per (128-row block, unit of 10 channels), in units of 2^-24."""
    op = R.conv_operands(_rand, form, seed)
    out, rec = _conv(op, dev, variant=variant, ksplit=ks, gn_unit=10)
    assert hasattr(out, "saspa_gn"), "the producer did not leave statistics"
    stats, unit = out.saspa_gn[:2]
    fam, got_ks = rec.gemm_plan()
    assert fam == variant and unit == 10 and (ks is None or got_ks == ks), (fam, unit, got_ks)
    ref, s = R.gnstat_ref(out.cpu(), unit)
    tag = f"gn_stats {form[0]} {form[1]}x{form[2]}x{form[3]}x{form[4]}+{form[5]}->{form[6]} {FAMILY_NAME[fam]} ks {got_ks}"
    _check(stats.cpu(), ref, s, "gnstat", tag, unit=R.UNIT_GNSTAT)
    if form[0] == "plain":
        # negative control: the statistics of THIS launch against the stored output of a launch with another bias
        other, _ = _conv(op, dev, variant=variant, ksplit=ks, bias=op["bias"] + 2.0 ** -6)
        ref2, s2 = R.gnstat_ref(other.cpu(), unit)
        _control(stats.cpu(), ref2, s2, "gnstat", f"{tag} against the output of a launch with bias + 2^-6", unit=R.UNIT_GNSTAT)


# ------------------------------------------------------------------ GroupNorm fed by epilogue statistics (family norm)
def _identity_producer(dev, x):
    """x [B, H, W, C] (bf16 values) through a pointwise conv with identity weights: the output IS x (every product exact, one
    non-zero term per sum), with the epilogue statistics of x hung on it -> (device tensor, row groups of the kernel that summed)."""
    c = x.shape[-1]
    with _recording() as rec:
        out = ops.conv(x.to(dev, BF), torch.eye(c).to(dev, BF), gn_unit=10)
    assert hasattr(out, "saspa_gn"), "the producer did not leave statistics"
    assert torch.equal(out.cpu().double(), x), "the identity producer changed its input"
    fam, ks = rec.gemm_plan()
    return out, (32 if ks > 1 else 8 if fam == ops.GEMM_WIDE else 16)


@pytest.mark.parametrize("act", [ops.ACT_NONE, SILU], ids=["none", "silu"])
@pytest.mark.parametrize("kind", ["lowvar", "offset"])
@pytest.mark.parametrize("c0,c1", [(320, 0), (640, 320), (1280, 640)])
def test_groupnorm_from_epilogue_statistics_budget(dev, c0, c1, kind, act):
    """(640 + 320) / 32 = 30 and (1280 + 640) / 32 = 60 channels per group: groups straddle the two sources.  The reference takes
    its statistics from the stored tensors: exact float64 ones for "lowvar"; for "offset" (mu / sigma = 64, where E[x^2] - mean^2
    cancels 12 bits) the fp32 block sums in the order of the kernel that left them (resnet_ref.gnstat_emul), as test_errbudget_gpu's
    GroupNorm cases take the statistics pass's: the epilogue sums themselves are held to 2^-24 by the gnstat family."""
    b, h, w_, eps = 2, 16, 24, 1e-5
    c = c0 + c1
    x = _norm_inputs(kind, (b, h, w_, c), 21 + c)
    gamma, beta = R.f32v(1 + 0.1 * _rand(c, seed=22 + c)), R.f32v(0.1 * _rand(c, seed=23 + c))
    xd, rgs = _identity_producer(dev, x[..., :c0].contiguous())
    x2d, rgs2 = _identity_producer(dev, x[..., c0:].contiguous()) if c1 else (None, rgs)
    if kind == "offset":
        st = torch.cat([R.gnstat_emul(t, 10, r) for t, r in ((x[..., :c0], rgs), (x[..., c0:], rgs2)) if t.shape[-1]], 1)
        st = st.reshape(b, -1, R.GROUPS, c // R.GROUPS // 10, 2).sum((1, 3))
        cnt = float(h * w_ * c // R.GROUPS)
        mean = st[..., 0] / cnt
        mean, rstd = R.f32v(mean), R.f32v(1.0 / torch.sqrt((st[..., 1] / cnt - mean * mean).clamp_min(0) + eps))
    else:
        mean, rstd = R.exact_stats(x, R.GROUPS, eps)
    mc, rc = R._per_channel(mean, c), R._per_channel(rstd, c)
    xhat = (x - mc) * rc
    ref = xhat * gamma + beta
    if act == SILU:
        ref = ref * torch.sigmoid(ref)
    s = norm_scale(xhat, gamma, beta, (mc * rc).expand_as(xhat))
    with _recording() as rec:
        run = lambda e: ops.groupnorm(xd, gamma.float().to(dev), beta.float().to(dev), R.GROUPS, e, act, x2=x2d).cpu()  # noqa: E731
        got = run(eps)
    assert "groupnorm_stats" not in rec.kinds(), f"a statistics pass ran beside the epilogue statistics: {rec.kinds()}"
    tag = f"groupnorm from epilogue statistics {c0}+{c1} {kind} act {act}"
    _check(got, ref, s, "norm", tag)
    if kind == "lowvar":
        _control(run(eps * 10), ref, s, "norm", f"{tag} with eps x 10")


# ------------------------------------------------------------------ conv -> GroupNorm -> SiLU in one launch (family gn_chain)
GN_CHAIN_GPU = [(600, R.GN_CHAIN_FORMS[0], 2), (600, R.GN_CHAIN_FORMS[0], 3), (610, R.GN_CHAIN_FORMS[1], 2),
                (620, R.GN_CHAIN_FORMS[2], 2), (630, (2, 16, 16, 128, 1280, True, "normal"), 2),
                (640, (3, 8, 8, 128, 640, False, "normal"), 2)]


def _fused_gn(op, dev, ks, *, eps=R.EPS, alpha=None, rowvec=None):
    fg = (op["gamma"].float().to(dev), op["beta"].float().to(dev), R.GROUPS, eps, SILU)
    out, rec = _conv(op, dev, ksplit=ks, fuse_gn=fg, alpha=alpha, rowvec=rowvec)
    assert "splitk_gn" in rec.kinds(), f"saspa_splitk_groupnorm was not launched: {rec.kinds()}"
    return out.cpu()


@pytest.mark.parametrize("seed,form,ks", GN_CHAIN_GPU, ids=[f"{f[0]}x{f[1]}x{f[2]}x{f[3]}-{f[4]}-{'rv' if f[5] else 'shared'}-{f[6]}-ks{k}"
                                                            for _, f, k in GN_CHAIN_GPU])
def test_conv_fused_groupnorm_budget(dev, seed, form, ks):
    b, h, w_, cin, n, per_image, kind = form
    op = R.gn_chain_operands(_rand, form, seed)
    ref, s = R.gn_chain_ref(op)
    tag = f"conv(fuse_gn) {b}x{h}x{w_}x{cin}->{n} {kind} {'per-image' if per_image else 'shared'} rowvec ks {ks}"
    _check(_fused_gn(op, dev, ks), ref, s, "gn_chain", tag)
    if kind == "lowvar":
        _control(_fused_gn(op, dev, ks, eps=R.EPS * 10), ref, s, "gn_chain", f"{tag} with eps x 10")
    elif per_image and ks == 2 and n == 640:
        _control(_fused_gn(op, dev, ks, alpha=op["alpha"] * (1 + 2 ** -7)), ref, s, "gn_chain", f"{tag} with alpha x (1 + 2^-7)")
        rv = op["rowvec"].clone()
        rv[[0, 1]] = rv[[1, 0]]
        _control(_fused_gn(op, dev, ks, rowvec=rv), ref, s, "gn_chain", f"{tag} with the row vectors of two images swapped")


# ------------------------------------------------------------------ GroupNorm -> SiLU -> conv in one launch (family conv_gn)
# (seed, (b, h, w, c0, c1, n, kind, flags), K slices); "border": the first row + 4, the last column - 3 (a pad pixel that was
# normalised instead of left zero would stand out)
CONV_GN_GPU = [(700, (2, 16, 16, 64, 0, 320, "offset", "rv res"), None), (710, (2, 16, 16, 64, 0, 320, "lowvar", ""), None),
               (720, (1, 16, 16, 128, 0, 256, "offset", ""), None), (730, (1, 32, 32, 96, 32, 320, "offset", ""), None),
               (740, (1, 32, 24, 64, 0, 320, "offset", ""), None), (750, (1, 16, 16, 256, 0, 320, "offset", "rv"), 2),
               (760, (2, 16, 16, 320, 0, 640, "offset", ""), 3), (770, (2, 16, 16, 64, 0, 320, "offset", "border"), None)]


def _conv_gn_op(seed, form):
    op = R.conv_gn_operands(_rand, form, seed)
    if "border" in form[7]:
        x = op["x"].clone()
        x[:, 0] += 4.0
        x[:, :, -1] -= 3.0
        op["x"] = R.q(x)
    return op


def _halo(op, dev, ks, *, gn=True, eps=R.EPS, x=None, x2=None, residual=None):
    """ops.conv_gn: the fused launch (gn) or the plain halo conv of an already normalised x."""
    g = (W.pack_gamma_beta32(op["gamma"].float(), op["beta"].float()).to(dev), R.GROUPS, eps, SILU) if gn else None
    res = op["res"] if residual is None else residual
    with _recording() as rec:
        out = ops.conv_gn(_d(op["x"], dev) if x is None else x, g, _dev_weights(op, dev, "chunk32"), _d(op["bias"], dev, torch.float32),
                          x2=(_d(op["x2"], dev) if x is None else x2), rowvec=_d(op["rowvec"], dev, torch.float32), residual=_d(res, dev),
                          alpha=op["alpha"], ksplit=ks)
    assert out is not None, "saspa_conv3x3_halo_eligible refused the launch"
    return out.cpu(), rec


@pytest.mark.parametrize("seed,form,ks", CONV_GN_GPU, ids=[f"{f[0]}x{f[1]}x{f[2]}x{f[3]}+{f[4]}-{f[5]}-{f[6]}-{f[7].replace(' ', '_')}-ks{k}"
                                                           for _, f, k in CONV_GN_GPU])
def test_halo_conv_groupnorm_budget(dev, seed, form, ks):
    b, h, w_, c0, c1, n, kind, flags = form
    op = _conv_gn_op(seed, form)
    ref, s, xn = R.conv_gn_ref(op, two_roundings=ks is None)
    tag = f"{b}x{h}x{w_}x{c0}+{c1}->{n} {kind} {flags} ks {ks}"
    # the fused launch, statistics from the pass form (a fresh tensor carries none)
    got, rec = _halo(op, dev, ks)
    assert "gn_stats" in rec.kinds(), rec.kinds()
    _check(got[..., :n], ref, s, "conv_gn", f"conv_gn {tag}")
    # the plain halo conv of the (reference's) normalised tensor: a conv epilogue form
    cref, cs = R.conv_ref(op, xn, two_roundings=ks is None)
    plain, _ = _halo(op, dev, ks, gn=False, x=_d(xn, dev), x2=None)
    _check(plain[..., :n], cref, cs, "gemm", f"halo conv without gn {tag}")
    # the two launches it replaces: same family, same reference
    gam, bet = op["gamma"].float().to(dev), op["beta"].float().to(dev)
    hn = ops.groupnorm(_d(op["x"], dev), gam, bet, R.GROUPS, R.EPS, SILU, x2=_d(op["x2"], dev))
    two, _ = _conv(op, dev, ksplit=ks, x=hn)
    _check(two.cpu()[..., :n], ref, s, "conv_gn", f"groupnorm + conv {tag}")
    if c0 % 160 == 0 and c1 == 0:
        # statistics from a producer's epilogue (the identity producer leaves them on x)
        xd, _ = _identity_producer(dev, op["x"])
        got2, rec2 = _halo(op, dev, ks, x=xd, x2=None)
        assert "gn_stats" not in rec2.kinds(), rec2.kinds()
        _check(got2[..., :n], ref, s, "conv_gn", f"conv_gn, epilogue statistics {tag}")
    if kind == "lowvar":
        _control(_halo(op, dev, ks, eps=R.EPS * 10)[0][..., :n], ref, s, "conv_gn", f"conv_gn {tag} with eps x 10")
    if "res" in flags:
        _control(_halo(op, dev, ks, residual=op["res"] * (1 + 2 ** -6))[0][..., :n], ref, s, "conv_gn",
                 f"conv_gn {tag} with residual x (1 + 2^-6)")
