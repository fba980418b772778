"""What `ops.py` puts into the parameter structs, launch for launch, against a recorded trace (no GPU: tests/ops_trace.py runs the
wrappers on CPU tensors and snapshots every library call instead of launching it).  The kernels trust the geometry they are handed,
so a pitch or a pointer that changes here is an out-of-bounds access there: the fixture pins all of it for the smallest shapes that
take each branch.  `python tests/test_ops_trace_host.py --write-golden` records tests/golden/ops_launch_trace.json."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import _lib, ops  # noqa: E402
from ops_trace import run_case  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_launch_trace.json")
BF, F16, F32, U8, I32 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int32
ERANGE = _lib.SASPA_ERANGE
CASES = []


def E(*shape, dt=BF):
    return torch.empty(shape, dtype=dt)


def case(name, **opts):
    def reg(fn):
        CASES.append((name, fn, opts))
        return fn
    return reg


def conv_case(name, shape, n, k=1, *, c1=0, dt=BF, setup=None, ctx=None, opts=None, **kw):
    """ops.conv of E(shape) (| x2 of c1 channels) with [n, k*k*C] weights; `setup(t)` adds operands to kw, `ctx()` wraps the call."""
    def fn(t):
        t.x, t.w = E(*shape, dt=dt), E(n, k * k * (shape[3] + c1), dt=dt)
        a = dict(kw)
        if c1:
            t.x2 = a["x2"] = E(*shape[:3], c1, dt=dt)
        if k > 1:
            a.update(kh=k, kw=k, pad=a.get("pad", 1))
        if setup:
            a.update(setup(t))
        if ctx is None:
            return ops.conv(t.x, t.w, **a)
        with ctx():
            return ops.conv(t.x, t.w, **a)
    CASES.append((name, fn, opts or {}))


def named(**mk):
    """setup helper: register the tensors `mk` builds (name -> thunk) and pass them to the op under their own names."""
    def setup(t):
        out = {}
        for k, f in mk.items():
            setattr(t, k, f())
            out[k] = getattr(t, k)
        return out
    return setup


L1 = (2, 32, 32, 640)

# ---- conv: shapes ----------------------------------------------------------------------------------------------------------
conv_case("conv 1x1", L1, 640)
conv_case("conv 3x3 bias", L1, 640, 3, setup=named(bias=lambda: E(640)))
conv_case("conv 3x3 concat", L1, 640, 3, c1=320)
conv_case("conv rowvec [N]", L1, 640, setup=named(rowvec=lambda: E(640)))
conv_case("conv rowvec [1,N]", L1, 640, setup=named(rowvec=lambda: E(1, 640)))
conv_case("conv rowvec [B,N] pitched", L1, 640, setup=named(rowvec=lambda: E(2, 1280)[:, :640]))
conv_case("conv residual wide view, out= wide", L1, 640,
          setup=named(residual=lambda: E(2, 32, 32, 1280)[..., 640:], out=lambda: E(2, 32, 32, 960)[..., :640]))
conv_case("conv N=4 (zeros)", L1, 4, 3)
conv_case("conv n_out", L1, 640, n_out=320)
conv_case("conv stride 2", L1, 640, 3, stride=2)
conv_case("conv out_hw asymmetric fp32", (1, 16, 16, 128), 128, 3, dt=F32, stride=2, pad=0, out_hw=(8, 8))
# ---- conv: upsampling and dtypes -----------------------------------------------------------------------------------------
conv_case("conv upsample 9 taps", (2, 16, 16, 640), 640, 3, upsample=True)


@case("conv upsample phase weights")
def _(t):
    t.x, t.w = E(2, 16, 16, 640), E(4, 640, 4 * 640)
    return ops.conv(t.x, t.w, kh=3, kw=3, pad=1, upsample=True)


@case("conv phase weights refused")
def _(t):
    t.x, t.w = E(2, 16, 16, 640), E(4, 640, 4 * 640)
    return ops.conv(t.x, t.w, kh=3, kw=3, pad=1, upsample=True, act=ops.ACT_SILU)


conv_case("conv fp32 exact", (2, 16, 16, 320), 320, 3, dt=F32, ctx=lambda: ops.f32_gemm_mode("exact"))
conv_case("conv fp32 x3", (2, 16, 16, 320), 320, 3, dt=F32, ctx=lambda: ops.f32_gemm_mode("x3"))


def _wsplit(t):
    t.w.saspa_wsplit = 1
    return {}


conv_case("conv wsplit in x3", (2, 16, 16, 320), 320, 3, dt=F32, setup=_wsplit, ctx=lambda: ops.f32_gemm_mode("x3"))
conv_case("conv wsplit outside x3", (2, 16, 16, 320), 320, 3, dt=F32, setup=_wsplit)
conv_case("conv fp16", L1, 640, 3, dt=F16)


def _korder(t):
    t.w.saspa_korder = 1
    return {}


conv_case("conv saspa_korder on w", L1, 640, 3, setup=_korder)
conv_case("conv korder= given", L1, 640, 3, setup=_korder, korder=2)
# ---- conv: split-K and statistics ----------------------------------------------------------------------------------------
conv_case("conv ksplit forced", L1, 640, 3, ksplit=4)
conv_case("conv twin_branch", L1, 640, 3, ctx=ops.twin_branch)
conv_case("conv 16x16 twin_branch", (2, 16, 16, 1280), 1280, 3, ctx=ops.twin_branch)
conv_case("conv 16x16 suggested slices", (2, 16, 16, 1280), 1280, 3)
conv_case("conv variant pin", L1, 640, 3, variant=ops.GEMM_TILED)
conv_case("conv SiLU", L1, 640, 3, act=ops.ACT_SILU)
conv_case("conv gn_unit stats", L1, 640, 3, gn_unit=10)
conv_case("conv gn_unit stats + residual", L1, 640, 3, gn_unit=10, setup=named(residual=lambda: E(*L1)))
conv_case("conv gn_unit no stats (hw % 128)", (2, 8, 8, 1280), 1280, 3, gn_unit=10)
conv_case("conv gn_unit no stats (N % 160)", L1, 200, 3, gn_unit=10)
conv_case("conv gn_unit no stats (fp32)", (2, 16, 16, 320), 320, 3, dt=F32, gn_unit=10)
conv_case("conv gn_unit SASPA_GN_FUSE=0", L1, 640, 3, gn_unit=10, opts={"env": {"SASPA_GN_FUSE": "0"}})


def _stale(t):
    t.out, t.old = E(*L1), E(16, 64, 2, dt=F32)
    t.out.saspa_gn = (t.old, 10, t.out.data_ptr(), t.out._version)
    return {"out": t.out}


conv_case("conv reused out= stale saspa_gn dropped", L1, 640, 3, setup=_stale)
conv_case("conv reused out= stale saspa_gn replaced", L1, 640, 3, setup=_stale, gn_unit=10)
L0 = (16, 64, 64, 320)
conv_case("conv level-0 pointwise: A-stationary over stats", L0, 320, gn_unit=10, setup=named(residual=lambda: E(*L0)))
conv_case("conv level-0 pointwise: SASPA_GEMM_AS_OVER_STATS=0", L0, 320, gn_unit=10, setup=named(residual=lambda: E(*L0)),
          opts={"env": {"SASPA_GEMM_AS_OVER_STATS": "0"}})

# ---- conv(fuse_gn=...) ----------------------------------------------------------------------------------------------------
L2 = (2, 16, 16, 1280)


def _fuse(c):
    def setup(t):
        t.bias, t.rowvec, t.gamma, t.beta = E(c), E(2, c), E(c, dt=F32), E(c, dt=F32)
        return {"bias": t.bias, "rowvec": t.rowvec, "gn_unit": 10, "fuse_gn": (t.gamma, t.beta, 32, 1e-5, ops.ACT_SILU)}
    return setup


for _rec in (False, True):
    _r = " (recorder)" if _rec else ""
    conv_case("conv fuse_gn deferred reduce" + _r, L2, 1280, 3, setup=_fuse(1280), opts={"recorder": _rec})
    conv_case("conv fuse_gn probe ERANGE" + _r, L2, 1280, 3, setup=_fuse(1280), opts={"rc": {"saspa_gemm": [ERANGE]}, "recorder": _rec})
conv_case("conv fuse_gn probe EINVAL", L2, 1280, 3, setup=_fuse(1280), opts={"rc": {"saspa_gemm": [-1]}})
conv_case("conv fuse_gn SASPA_SPLITK_GN=0", L2, 1280, 3, setup=_fuse(1280), opts={"env": {"SASPA_SPLITK_GN": "0"}})
conv_case("conv fuse_gn not eligible", (2, 64, 64, 320), 320, 3, setup=_fuse(320))
conv_case("conv fuse_gn forced ksplit", L2, 1280, 3, setup=_fuse(1280), ksplit=2)
conv_case("conv fuse_gn with residual", L2, 1280, 3, setup=lambda t: dict(_fuse(1280)(t), **named(residual=lambda: E(*L2))(t)))

# ---- conv_gn ---------------------------------------------------------------------------------------------------------------


def conv_gn_case(name, shape, n, *, c1=0, gn=True, stats=(), defer=False, dt=BF, setup=None, ctx=None, opts=None, **kw):
    """ops.conv_gn; `stats`: which of ("x", "x2") come out of a traced producer conv(..., gn_unit=10) first."""
    def fn(t):
        c0 = shape[3]
        srcs = {}
        for nm, c in (("x", c0), ("x2", c1)):
            if not c:
                continue
            if nm in stats:
                setattr(t, "p" + nm, E(*shape[:3], c))
                setattr(t, "pw" + nm, E(c, c))
                srcs[nm] = ops.conv(getattr(t, "p" + nm), getattr(t, "pw" + nm), gn_unit=10)
            else:
                setattr(t, nm, E(*shape[:3], c, dt=dt))
                srcs[nm] = getattr(t, nm)
        t.w32 = E(n, 9 * (c0 + c1), dt=dt)
        a = dict(kw, x2=srcs.get("x2"))
        g = None
        if gn:
            t.gb32 = E((c0 + c1) // 32, 64, dt=F32)
            g = (t.gb32, 32, 1e-5, ops.ACT_SILU)
        if defer:
            t.gamma, t.beta = E(n, dt=F32), E(n, dt=F32)
            a["defer_to"] = (t.gamma, t.beta, 32, 1e-6, ops.ACT_SILU)
        if setup:
            a.update(setup(t))
        if ctx is None:
            return ops.conv_gn(srcs["x"], g, t.w32, **a)
        with ctx():
            return ops.conv_gn(srcs["x"], g, t.w32, **a)
    CASES.append((name, fn, opts or {}))


conv_gn_case("conv_gn gn=None", L1, 640, gn=False)
conv_gn_case("conv_gn producer stats on x", L1, 640, stats=("x",), setup=named(bias=lambda: E(640), rowvec=lambda: E(2, 640)))
conv_gn_case("conv_gn producer stats on x | x2", L1, 640, c1=320, stats=("x", "x2"))
conv_gn_case("conv_gn producer stats on x only of x | x2", L1, 640, c1=320, stats=("x",))
conv_gn_case("conv_gn own statistics launch", L1, 640, c1=320, setup=named(residual=lambda: E(2, 32, 32, 1280)[..., :640]))
conv_gn_case("conv_gn out=, gn_unit", L1, 640, gn_unit=10, setup=named(out=lambda: E(*L1)))
conv_gn_case("conv_gn not eligible (N=4)", L1, 4)
conv_gn_case("conv_gn N=36 (zeros)", L1, 36)
conv_gn_case("conv_gn not eligible (channels)", (2, 32, 32, 48), 640)
conv_gn_case("conv_gn not bf16", L1, 640, dt=F16)
conv_gn_case("conv_gn defer_to deferred reduce", L2, 1280, defer=True)
conv_gn_case("conv_gn defer_to probe ERANGE", L2, 1280, defer=True, gn_unit=10, opts={"rc": {"saspa_conv3x3_halo": [ERANGE]}})
conv_gn_case("conv_gn defer_to probe EINVAL", L2, 1280, defer=True, opts={"rc": {"saspa_conv3x3_halo": [-1]}})
conv_gn_case("conv_gn defer_to SASPA_SPLITK_GN=0", L2, 1280, defer=True, opts={"env": {"SASPA_SPLITK_GN": "0"}})
conv_gn_case("conv_gn defer_to not eligible", L1, 640, defer=True)
conv_gn_case("conv_gn defer_to with residual", L2, 1280, defer=True, setup=named(residual=lambda: E(*L2)))
conv_gn_case("conv_gn defer_to (recorder)", L2, 1280, defer=True, opts={"recorder": True})
conv_gn_case("conv_gn ksplit forced", L2, 1280, ksplit=3)
conv_gn_case("conv_gn one slice", L2, 1280, ksplit=1)
conv_gn_case("conv_gn suggested slices", L2, 1280)
conv_gn_case("conv_gn twin_branch", L2, 1280, ctx=ops.twin_branch)

# ---- groupnorm / groupnorm_quant_mxfp8 --------------------------------------------------------------------------------------


def gn_case(name, shape, *, c1=0, stats=(), touch=False, quant=False, dt=BF, out=None, opts=None):
    def fn(t):
        srcs = {}
        for nm, c in (("x", shape[3]), ("x2", c1)):
            if not c:
                continue
            if nm in stats:
                setattr(t, "p" + nm, E(*shape[:3], c))
                setattr(t, "pw" + nm, E(c, c))
                srcs[nm] = ops.conv(getattr(t, "p" + nm), getattr(t, "pw" + nm), gn_unit=10)
            else:
                setattr(t, nm, E(*shape[:3], c, dt=dt))
                srcs[nm] = getattr(t, nm)
        if touch:
            srcs["x"].zero_()                   # an in-place write through torch: the version the statistics describe is gone
        ctot = shape[3] + c1
        t.gamma, t.beta = E(ctot, dt=F32), E(ctot, dt=F32)
        if quant:
            return ops.groupnorm_quant_mxfp8(srcs["x"], t.gamma, t.beta, 32, 1e-5, ops.ACT_SILU, x2=srcs.get("x2"))
        if out is not None:
            t.out = out()
        return ops.groupnorm(srcs["x"], t.gamma, t.beta, 32, 1e-5, ops.ACT_SILU, x2=srcs.get("x2"), out=getattr(t, "out", None))
    CASES.append((name, fn, opts or {}))


for _q in (False, True):
    _n = "groupnorm_quant_mxfp8" if _q else "groupnorm"
    gn_case(_n + " behind conv(gn_unit)", L1, stats=("x",), quant=_q)
    gn_case(_n + " behind conv(gn_unit), written in place since", L1, stats=("x",), touch=True, quant=_q)
    gn_case(_n + " x | x2, both with statistics", L1, c1=320, stats=("x", "x2"), quant=_q)
    gn_case(_n + " x | x2, one with statistics", L1, c1=320, stats=("x2",), quant=_q)
    gn_case(_n + " SASPA_GN_FUSE=0", L1, stats=("x",), quant=_q, opts={"env": {"SASPA_GN_FUSE": "0"}})
    gn_case(_n + " 8x8 x 1280", (2, 8, 8, 1280), quant=_q)
    gn_case(_n + " two-pass", L1, quant=_q)
gn_case("groupnorm 8x8 x 1280 SASPA_GN_ONEPASS=0", (2, 8, 8, 1280), opts={"env": {"SASPA_GN_ONEPASS": "0"}})
gn_case("groupnorm out= wide", L1, c1=320, out=lambda: E(2, 32, 32, 1280))
gn_case("groupnorm fp32", (2, 16, 16, 320), dt=F32)
gn_case("groupnorm fp16", (2, 16, 16, 320), dt=F16)
gn_case("groupnorm_quant_mxfp8 per-image nsplit (batch 32)", (32, 32, 32, 320), quant=True)
gn_case("groupnorm two-pass nsplit (batch 32)", (32, 32, 32, 320))


@case("groupnorm x2 mismatch")
def _(t):
    t.x, t.x2, t.g = E(*L1), E(2, 16, 16, 320), E(960, dt=F32)
    return ops.groupnorm(t.x, t.g, t.g, 32, 1e-5, x2=t.x2)


@case("groupnorm groups mismatch")
def _(t):
    t.x, t.g = E(*L1), E(640, dt=F32)
    return ops.groupnorm(t.x, t.g, t.g, 48, 1e-5)


@case("groupnorm out mismatch")
def _(t):
    t.x, t.g, t.out = E(*L1), E(640, dt=F32), E(2, 32, 32, 320)
    return ops.groupnorm(t.x, t.g, t.g, 32, 1e-5, out=t.out)


@case("groupnorm_quant_mxfp8 not bf16")
def _(t):
    t.x, t.g = E(*L1, dt=F16), E(640, dt=F32)
    return ops.groupnorm_quant_mxfp8(t.x, t.g, t.g, 32, 1e-5)


@case("groupnorm_quant_mxfp8 x2 mismatch")
def _(t):
    t.x, t.x2, t.g = E(*L1), E(2, 16, 16, 320), E(960, dt=F32)
    return ops.groupnorm_quant_mxfp8(t.x, t.g, t.g, 32, 1e-5, x2=t.x2)


@case("groupnorm_quant_mxfp8 groups mismatch")
def _(t):
    t.x, t.g = E(*L1), E(320, dt=F32)
    return ops.groupnorm_quant_mxfp8(t.x, t.g, t.g, 32, 1e-5)


# ---- conv / conv_gn: the operand checks, each once -------------------------------------------------------------------------
def _bad(name, fn):
    CASES.append((name, fn, {}))


def _conv_errors(which):
    def call(t, **kw):
        t.x = E(*L1)
        if which == "conv":
            t.w = kw.pop("w", None) if "w" in kw else E(640, 9 * 640)
            return ops.conv(t.x, t.w, kh=3, kw=3, pad=kw.pop("pad", 1), **kw)
        t.w32 = kw.pop("w", None) if "w" in kw else E(640, 9 * 640)
        kw.pop("pad", None)
        return ops.conv_gn(t.x, None, t.w32, **kw)
    mk = {"concat source": lambda t: call(t, x2=E(2, 16, 16, 320)),
          "weights too narrow": lambda t: call(t, w=E(640, 640)),
          "weights dtype": lambda t: call(t, w=E(640, 9 * 640, dt=F32)),
          "residual shape": lambda t: call(t, residual=E(2, 32, 32, 320)),
          "out dtype": lambda t: call(t, out=E(*L1, dt=F32)),
          "bias short": lambda t: call(t, bias=E(320)),
          "rowvec batch": lambda t: call(t, rowvec=E(3, 640)),
          "rowvec short": lambda t: call(t, rowvec=E(320))}
    if which == "conv":
        mk["empty output"] = lambda t: call(t, pad=-20)
        mk["residual not contiguous"] = lambda t: call(t, residual=E(2, 32, 32, 1280)[..., ::2])
        mk["out pitch irregular"] = lambda t: call(t, out=E(2, 32, 40, 640)[:, :, :32])
    for k, f in mk.items():
        _bad(f"{which} error: {k}", f)


_conv_errors("conv")
_conv_errors("conv_gn")

# ---- conv3x3_mxfp8 ---------------------------------------------------------------------------------------------------------


def mx_case(name, *, rowvec=None, residual=False, gn_unit=None, opts=None, bad=None):
    def fn(t):
        b, h, w, c, n = 2, 32, 32, 320, 640
        t.q, t.qs, t.w8, t.sw, t.bias = E(b, h, w, c, dt=U8), E(b, h, w, c // 32, dt=U8), E(n, 2944, dt=U8), E(n, dt=F32), E(n, dt=F32)
        a = {}
        if rowvec is not None:
            t.rowvec = a["rowvec"] = rowvec()
        if residual:
            t.residual = a["residual"] = E(b, h, w, n)
        if bad:
            a.update(bad(t))
        return ops.conv3x3_mxfp8(a.pop("q", t.q), a.pop("qs", t.qs), a.pop("w8", t.w8), a.pop("sw", t.sw), t.bias, gn_unit=gn_unit, **a)
    CASES.append((name, fn, opts or {}))


mx_case("conv3x3_mxfp8 plain")
mx_case("conv3x3_mxfp8 rowvec [N]", rowvec=lambda: E(640, dt=F32))
mx_case("conv3x3_mxfp8 rowvec [1,N]", rowvec=lambda: E(1, 640, dt=F32))
mx_case("conv3x3_mxfp8 rowvec [B,N] pitched", rowvec=lambda: E(2, 1280, dt=F32)[:, :640])
mx_case("conv3x3_mxfp8 residual, gn_unit", residual=True, gn_unit=10)
mx_case("conv3x3_mxfp8 (recorder)", residual=True, gn_unit=10, opts={"recorder": True})
mx_case("conv3x3_mxfp8 error: weights", bad=lambda t: {"w8": E(640, 2880, dt=U8)})
mx_case("conv3x3_mxfp8 error: dtype", bad=lambda t: {"q": E(2, 32, 32, 320)})
mx_case("conv3x3_mxfp8 error: dense", bad=lambda t: {"q": E(2, 32, 32, 640, dt=U8)[..., :320]})
mx_case("conv3x3_mxfp8 error: residual", bad=lambda t: {"residual": E(2, 32, 32, 320)})
mx_case("conv3x3_mxfp8 error: sw", bad=lambda t: {"sw": E(640)})
mx_case("conv3x3_mxfp8 error: rowvec", bad=lambda t: {"rowvec": E(2, 640)})

# ---- linear / gemm_batched -------------------------------------------------------------------------------------------------


def lin_case(name, xshape, n, *, dt=BF, setup=None, ctx=None, opts=None, **kw):
    def fn(t):
        t.x, t.w = E(*xshape, dt=dt), E(n, xshape[-1], dt=dt)
        a = dict(kw)
        if setup:
            a.update(setup(t))
        if ctx is None:
            return ops.linear(t.x, t.w, **a)
        with ctx():
            return ops.linear(t.x, t.w, **a)
    CASES.append((name, fn, opts or {}))


lin_case("linear plain", (2048, 640), 640, setup=named(bias=lambda: E(640)))
lin_case("linear (recorder)", (2048, 640), 640, setup=named(bias=lambda: E(640)), opts={"recorder": True})
lin_case("linear residual, 3-D", (2, 1024, 640), 640, setup=named(residual=lambda: E(2, 1024, 640)))
lin_case("linear one row", (1, 1280), 1000, setup=named(residual=lambda: E(1, 1000), rowvec=lambda: E(1000)))
lin_case("linear N=77 (zeros)", (2048, 640), 77)
lin_case("linear out= wide, pitched x", (2048, 640), 640, setup=lambda t: {"out": named(out=lambda: E(2048, 1920)[:, 640:1280])(t)["out"]})
lin_case("linear GEGLU", (2048, 640), 5120, act=ops.ACT_GEGLU)
L0T = (16 * 4096, 320)
lin_case("linear ln=", L0T, 320, setup=lambda t: {"ln": tuple(named(g=lambda: E(320, dt=F32), b=lambda: E(320, dt=F32))(t).values()) + (1e-5,)})
lin_case("linear out_t= with n_split", L0T, 960, n_split=640, rows_per_batch=4096, setup=named(out_t=lambda: E(16, 320, 4096)))
lin_case("linear suggested K slices", (128, 5120), 1280)
lin_case("linear ksplit forced, variant", (2048, 640), 640, ksplit=2, variant=ops.GEMM_TILED)
lin_case("linear twin_branch", (512, 1280), 1280, ctx=ops.twin_branch)
lin_case("linear fp32 x3", (512, 320), 320, dt=F32, ctx=lambda: ops.f32_gemm_mode("x3"))
lin_case("linear fp16", (2048, 640), 640, dt=F16)
lin_case("linear error: dtype", (2048, 640), 640, setup=named(residual=lambda: E(2048, 640, dt=F32)))
lin_case("linear error: ln", (2048, 640), 640, setup=lambda t: {"ln": (E(640), E(640), 1e-5)})
lin_case("linear error: out_t form", (2048, 640), 640, setup=named(out_t=lambda: E(2, 320, 1024), out=lambda: E(2048, 320)))
lin_case("linear error: out_t shape", (2048, 640), 960, n_split=640, rows_per_batch=1024, setup=named(out_t=lambda: E(3, 320, 1024)))


@case("gemm_batched")
def _(t):
    t.a, t.w, t.out, t.r = E(2, 8, 64, 80), E(2, 8, 77, 80), E(2, 8, 64, 80), E(2, 8, 64, 80)
    return ops.gemm_batched(t.a, 80, (8 * 64 * 80, 64 * 80), t.w, 80, (8 * 77 * 80, 77 * 80), t.out, 80, (8 * 64 * 80, 64 * 80),
                            64, 77, 80, 2, 8, alpha=0.125, residual=t.r, ldr=80, act=ops.ACT_SILU)


# ---- linear_fp8 / linear_mxfp8 ---------------------------------------------------------------------------------------------


def f8_case(name, m=256, *, scale_n=None, opts=None, setup=None, **kw):
    def fn(t):
        t.xq, t.xs, t.wq, t.ws, t.bias = E(m, 320, dt=U8), E(m if scale_n is None else scale_n, dt=F32), E(2560, 320, dt=U8), \
            E(2560, dt=F32), E(2560, dt=F32)
        a = dict(kw)
        if setup:
            a.update(setup(t))
        return ops.linear_fp8(t.xq, t.xs, t.wq, t.ws, t.bias, **a)
    CASES.append((name, fn, opts or {}))


f8_case("linear_fp8 per-row scale, residual", setup=named(residual=lambda: E(256, 2560)))
f8_case("linear_fp8 one row", m=1)
f8_case("linear_fp8 one-element scale", scale_n=1)
f8_case("linear_fp8 GEGLU out_fp8_scale + amax", act=ops.ACT_GEGLU, setup=named(out_fp8_scale=lambda: E(1, dt=F32), amax=lambda: E(1, dt=F32)))
f8_case("linear_fp8 GEGLU out_mx", act=ops.ACT_GEGLU, out_mx=True)
f8_case("linear_fp8 (recorder)", act=ops.ACT_GEGLU, out_mx=True, opts={"recorder": True})
f8_case("linear_fp8 error: out_fp8 without GEGLU", setup=named(amax=lambda: E(1, dt=F32)))
f8_case("linear_fp8 error: out_mx without GEGLU", out_mx=True)
f8_case("linear_fp8 error: scales", scale_n=7)
f8_case("linear_fp8 error: out_fp8_scale", act=ops.ACT_GEGLU, setup=named(out_fp8_scale=lambda: E(2, dt=F32)))
f8_case("linear_fp8 error: amax", act=ops.ACT_GEGLU, setup=named(amax=lambda: E(1)))


def mxl_case(name, m, *, residual=False, bad=None):
    def fn(t):
        t.q, t.qs, t.wq, t.ws, t.bias = E(m, 1280, dt=U8), E(m, 44, dt=U8)[:, :40], E(320, 1280, dt=U8), E(320, dt=F32), E(320, dt=F32)
        if residual:
            t.residual = E(m, 320)
        a = bad(t) if bad else {}
        return ops.linear_mxfp8(a.get("q", t.q), a.get("qs", t.qs), t.wq, t.ws, t.bias, residual=getattr(t, "residual", None))
    CASES.append((name, fn, {}))


mxl_case("linear_mxfp8 m > 1, residual", 256, residual=True)
mxl_case("linear_mxfp8 m == 1", 1)
mxl_case("linear_mxfp8 error: dtype", 256, bad=lambda t: {"q": E(256, 1280)})
mxl_case("linear_mxfp8 error: exponents", 256, bad=lambda t: {"qs": E(256, 20, dt=U8)})

# ---- sampler steps with a device table -------------------------------------------------------------------------------------


def step_case(name, call, groups=2, bad=None):
    def fn(t):
        nimg, hw = 2, 64
        t.eps, t.x, t.state = E(groups * nimg, hw, 8), E(groups * nimg, hw, 8), E(4, nimg, hw, 8)
        t.saved, t.index = E(nimg, hw, 8), E(1, dt=I32)
        t.t4, t.t10, t.t12 = E(5, 4, dt=F32), E(5, 10, dt=F32), E(5, 12, dt=F32)
        if bad:
            bad(t)
        return call(t, nimg, hw)
    CASES.append((name, fn, {}))


_ROW = [0.5 + i for i in range(12)]
_STEPS = {
    "ddim_step_dev": (2, lambda t, n, hw: ops.ddim_step_dev(t.eps, t.x, n, hw, 4, 7.5, t.t4, t.index)),
    "ddim_step_dev cfg=False": (1, lambda t, n, hw: ops.ddim_step_dev(t.eps, t.x, n, hw, 4, 7.5, t.t4, t.index, cfg=False)),
    "cfg3_ddim_step_dev": (3, lambda t, n, hw: ops.cfg3_ddim_step_dev(t.eps, t.x, n, hw, 4, 7.5, 1.5, t.t4, t.index)),
    "cfg_plms_step_dev": (2, lambda t, n, hw: ops.cfg_plms_step_dev(t.eps, t.x, t.state, t.saved, n, hw, 4, 7.5, t.t10, t.index)),
    "cfg_unipc_step device table": (2, lambda t, n, hw: ops.cfg_unipc_step(t.eps, t.x, t.state, n, hw, 4, 7.5, table=t.t12, index=t.index)),
    "cfg_unipc_step host row": (2, lambda t, n, hw: ops.cfg_unipc_step(t.eps, t.x, t.state, n, hw, 4, 7.5, row=_ROW)),
    "unipc_step device table": (1, lambda t, n, hw: ops.unipc_step(t.eps, t.x, t.state, n, hw, 4, table=t.t12, index=t.index)),
    "unipc_step host row": (1, lambda t, n, hw: ops.unipc_step(t.eps, t.x, t.state, n, hw, 4, row=_ROW)),
}
for _k, (_g, _f) in _STEPS.items():
    step_case(_k, _f, _g)


def _swap(**kw):
    def bad(t):
        for k, v in kw.items():
            setattr(t, k, v())
    return bad


step_case("ddim_step_dev error: table width", _STEPS["ddim_step_dev"][1], bad=_swap(t4=lambda: E(5, 10, dt=F32)))
step_case("cfg3_ddim_step_dev error: index dtype", _STEPS["cfg3_ddim_step_dev"][1], 3, bad=_swap(index=lambda: E(1, dt=torch.int64)))
step_case("cfg_plms_step_dev error: table dtype", _STEPS["cfg_plms_step_dev"][1], bad=_swap(t10=lambda: E(5, 10)))
step_case("cfg_unipc_step error: table not dense", _STEPS["cfg_unipc_step device table"][1], bad=_swap(t12=lambda: E(5, 24, dt=F32)[:, :12]))
step_case("unipc_step error: no index", lambda t, n, hw: ops.unipc_step(t.eps, t.x, t.state, n, hw, 4, table=t.t12), 1)

# ---- recorder: the remaining launch forms again with a recorder that has `conditional` --------------------------------------
conv_case("conv 3x3 (recorder)", L1, 640, 3, c1=320, gn_unit=10, setup=named(residual=lambda: E(*L1)), opts={"recorder": True})


@case("conv upsample phase weights (recorder)", recorder=True)
def _(t):
    t.x, t.w = E(2, 16, 16, 640), E(4, 640, 4 * 640)
    return ops.conv(t.x, t.w, kh=3, kw=3, pad=1, upsample=True)


gn_case("groupnorm two-pass (recorder)", L1, opts={"recorder": True})


RAISES = {"conv phase weights refused", "conv wsplit outside x3", "conv fuse_gn probe EINVAL", "conv_gn defer_to probe EINVAL",
          "groupnorm x2 mismatch", "groupnorm groups mismatch", "groupnorm out mismatch", "groupnorm_quant_mxfp8 not bf16",
          "groupnorm_quant_mxfp8 x2 mismatch", "groupnorm_quant_mxfp8 groups mismatch"}


def traces():
    """[(name, record)] of the whole corpus, normalised through JSON (tuples -> lists, as the fixture reads back)."""
    names = [n for n, _, _ in CASES]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return [(name, json.loads(json.dumps(run_case(fn, **opts)))) for name, fn, opts in CASES]


def _delta(rows, decode):
    """The fixture's one compression: a struct is stored as its difference from the previous struct of the same type in the file
    (near-identical cases follow each other), a field that went back to zero as 0.  Lossless; `decode` restores the full structs."""
    prev = {}
    for r in rows:
        for call in r["calls"]:
            for a in call[1:]:
                if not (isinstance(a, list) and len(a) == 2 and isinstance(a[1], dict)):
                    continue
                base = prev.get(a[0], {})
                if decode:
                    a[1] = full = {k: v for k, v in dict(base, **a[1]).items() if v}
                else:
                    full = a[1]
                    a[1] = dict({k: 0 for k in base if k not in full}, **{k: v for k, v in full.items() if base.get(k) != v})
                prev[a[0]] = full
    return rows


def _first_difference(got, want):
    """The first thing that differs between two records, field by field for a struct."""
    for key in ("exc", "allocs", "ret", "recorded"):
        if got.get(key) != want.get(key):
            return f"{key}:\n    got  {got.get(key)}\n    want {want.get(key)}"
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if g == w:
            continue
        lines = [f"call {i}: got {g[0]}, want {w[0]}"]
        for j, (ga, wa) in enumerate(zip(g[1:], w[1:])):
            if ga == wa:
                continue
            if isinstance(ga, list) and isinstance(wa, list) and len(ga) == 2 and isinstance(ga[1], dict) and isinstance(wa[1], dict):
                for f in sorted(set(ga[1]) | set(wa[1])):
                    if ga[1].get(f, 0) != wa[1].get(f, 0):
                        lines.append(f"    argument {j} {wa[0]}.{f}: got {ga[1].get(f, 0)}, want {wa[1].get(f, 0)}")
            else:
                lines.append(f"    argument {j}: got {ga}, want {wa}")
        if len(g) != len(w):
            lines.append(f"    {len(g) - 1} arguments, want {len(w) - 1}")
        return "\n".join(lines)
    return f"{len(got['calls'])} calls {[c[0] for c in got['calls']]}, want {len(want['calls'])} {[c[0] for c in want['calls']]}"


def test_ops_launch_trace():
    """Every library call ops.py makes for the corpus -- structs, pointers, allocations, returned tensors, recorder entries,
    exceptions -- is the recorded one."""
    assert os.path.getsize(GOLDEN) <= 73848, "the fixture outgrew tests/golden/gemm_dispatch.json, the largest the project carries"
    with open(GOLDEN) as f:
        want = _delta([json.loads(line) for line in f if line.strip()], decode=True)
    got = traces()
    assert [n for n, _ in got] == [w["case"] for w in want], "the corpus and the fixture list different cases"
    bad = [(n, g, w) for (n, g), w in zip(got, want) if dict(g, case=n) != w]
    msg = "\n".join(f"case {n!r}: {_first_difference(g, w)}" for n, g, w in bad[:8])
    assert not bad, f"{len(bad)} of {len(want)} launch traces changed:\n{msg}"


def test_corpus_takes_its_branches():
    """The corpus is not vacuous: the cases that are meant to launch do, the ones meant to raise raise, and the branches named in
    the case titles show in the records."""
    got = dict(traces())
    for name, r in got.items():
        assert ("exc" in r) == ("error:" in name or name in RAISES), (name, r.get("exc"))
    calls = lambda n: [c[0] for c in got[n]["calls"]]  # noqa: E731
    assert calls("conv fuse_gn deferred reduce") == ["saspa_gemm", "saspa_splitk_groupnorm"]
    assert calls("conv fuse_gn probe ERANGE") == ["saspa_gemm", "saspa_gemm", "saspa_groupnorm_apply"]
    assert calls("conv_gn defer_to deferred reduce") == ["saspa_groupnorm_stats", "saspa_conv3x3_halo", "saspa_splitk_groupnorm"]
    assert got["conv_gn not eligible (channels)"] == {"ret": None, "allocs": {}, "calls": []}
    assert calls("conv fp16") == ["f16:saspa_gemm"]
    assert calls("groupnorm behind conv(gn_unit)") == ["saspa_gemm", "saspa_groupnorm_apply"]
    assert calls("groupnorm behind conv(gn_unit), written in place since") == ["saspa_gemm", "saspa_groupnorm_stats", "saspa_groupnorm_apply"]
    assert calls("groupnorm 8x8 x 1280") == ["saspa_groupnorm_onepass"]
    assert "gn_stats" not in got["conv level-0 pointwise: A-stationary over stats"]["calls"][0][1][1]
    assert "gn_stats" in got["conv level-0 pointwise: SASPA_GEMM_AS_OVER_STATS=0"]["calls"][0][1][1]
    assert got["linear suggested K slices"]["calls"][0][1][1].get("ksplit", 1) > 1
    # a refused probe reaches the recorder not at all, the fallback's launches once
    assert [r[0] for r in got["conv fuse_gn probe ERANGE (recorder)"]["recorded"]] == ["gemm", "groupnorm_apply"]
    assert [r[0] for r in got["conv fuse_gn deferred reduce (recorder)"]["recorded"]] == ["gemm", "splitk_gn"]


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-golden"]:
        rows = _delta([dict({"case": name}, **r) for name, r in traces()], decode=False)
        with open(GOLDEN, "w") as f:
            for r in rows:
                f.write(json.dumps(r, separators=(",", ":")) + "\n")
        print(f"{GOLDEN}: {len(rows)} cases, {os.path.getsize(GOLDEN)} bytes")
    elif sys.argv[1:] == ["--list"]:
        for name, r in traces():
            print(name, "->", r.get("exc") or [c[0] for c in r["calls"]], r["allocs"])
