"""The v-prediction sampler steps of csrc/saspa_elem.hip (cfg_ddim_step_v, ddim_step_v, ddim_step_v_dev, cfg_unipc_step_v,
unipc_step_v) on the device, in fp32, bf16 and fp16 (the f16 library), against the float64 references of tests/sd21_ref.py inside the
limits tests/test_sd21_host.py proves on the CPU (2x above the legitimate fp32 emulations, 2x below every separable mutant:
profiles/vpred_errbudget.txt).  Shapes: 1 and 3 images of 4x8x8 and 4x8x24 latents, and 37 pixels (a count that fills neither a wave
nor a block; a pixel is always one whole 16-byte vector of eight channels -- anything else is refused like the epsilon steps refuse it,
tests/test_sd21_host.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops
from saspa_aug_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
from tests import sd21_ref as R
from tests.errbudget import check_budget, fmt, rejects
from tests.test_errbudget import _rand

pytestmark = pytest.mark.gpu
NC = R.C
JUNK = 3.0                             # channels 4..7 of the x that goes in: the step must write zeros there
STORAGE = list(R.DTYPES)
SHAPES = [(1, 64), (3, 64), (1, 192), (3, 192), (3, 37)]      # (images, latent pixels)
COEF = R.DDIM_COEF


def _c4(a_t, a_p):
    return a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5


def _check(storage, got, ref, s, what):
    st = check_budget(got, ref, s, R.UNITS[storage], limits=R.VPRED_LIMITS[storage], what=what)
    print(f"\n[budget] vpred {storage}  {what}: {fmt(st)}")


def _control(storage, got, ref, s, what):
    assert rejects(got, ref, s, R.UNITS[storage], limits=R.VPRED_LIMITS[storage]), f"negative control not rejected: {what}"


def _pad8(t, dev, dt, fill=0.0):
    return F.pad(t.float(), (0, R.LDC - NC), value=fill).to(dev, dt).contiguous()


def _live(t):
    t = t.cpu()
    assert (t[..., NC:] == 0).all(), "channels 4..7 of a written tensor are not zero"
    return t[..., :NC].double()


def _dev_inputs(dev, inp, cfg, dt):
    x = torch.cat([inp["x"], inp["x"]]) if cfg else inp["x"]
    return _pad8(inp["eps"], dev, dt), _pad8(x, dev, dt, JUNK), _pad8(inp["state"], dev, dt)


def _ddim(dev, inp, cfg, dt, coef, *, g=R.GUIDANCE, table=None, index=0):
    v8, x8, _ = _dev_inputs(dev, inp, cfg, dt)
    v0 = v8.clone()
    n, hw = inp["nimg"], inp["hw"]
    if table is not None:
        ops.ddim_step_v_dev(v8, x8, n, hw, NC, g, table, torch.tensor([index], dtype=torch.int32, device=dev), cfg=cfg)
    elif cfg:
        ops.cfg_ddim_step_v(v8, x8, n, hw, NC, g, *coef)
    else:
        ops.ddim_step_v(v8, x8, n, hw, NC, *coef)
    assert torch.equal(v8, v0)                                                # the network output is read only
    if cfg:
        assert torch.equal(x8[:n], x8[n:])                                    # the two CFG halves
    return x8


def _unipc(dev, inp, cfg, dt, rows, k, *, g=R.GUIDANCE, table=False):
    v8, x8, st8 = _dev_inputs(dev, inp, cfg, dt)
    v0, m0_old = v8.clone(), st8[1].clone()
    n, hw = inp["nimg"], inp["hw"]
    kw = dict(row=rows[k])
    if table:
        kw = dict(table=torch.tensor(rows, dtype=torch.float32, device=dev), index=torch.tensor([k], dtype=torch.int32, device=dev))
    if cfg:
        ops.cfg_unipc_step_v(v8, x8, st8, n, hw, NC, g, **kw)
        assert torch.equal(x8[:n], x8[n:])
    else:
        ops.unipc_step_v(v8, x8, st8, n, hw, NC, **kw)
    assert torch.equal(v8, v0) and torch.equal(st8[2], m0_old)                # m1 = the old m0, bits unchanged
    return dict(x=x8[:n], last=st8[0], m0=st8[1]), (x8, st8)


# ------------------------------------------------------------------ against the float64 reference
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "plain"])
@pytest.mark.parametrize("nimg,hw", SHAPES)
@pytest.mark.parametrize("storage", STORAGE)
def test_ddim_v_budget(dev, storage, nimg, hw, cfg):
    dt = R.DTYPES[storage]
    g = R.GUIDANCE if cfg else None
    inp = R.inputs(_rand, nimg, hw, 701, dt, cfg=cfg)
    ref, s = R.vddim_ref(inp, **COEF, g=g)
    tag = f"{'cfg_ddim_step_v' if cfg else 'ddim_step_v'} {storage} {nimg}x{hw}"
    x8 = _ddim(dev, inp, cfg, dt, _c4(**COEF))
    _check(storage, _live(x8[:nimg]), ref, s, tag)
    # the _dev form: the same constants from row 2 of a device table, bit for bit
    rows = [_c4(0.9, 0.95), _c4(0.6, 0.7), _c4(**COEF), _c4(0.1, 0.2)]
    table = torch.tensor(rows, dtype=torch.float32, device=dev)
    assert torch.equal(_ddim(dev, inp, cfg, dt, None, table=table, index=2), x8), f"{tag}: the _dev form differs"
    if nimg * hw >= 256:
        # negative controls on the device: the neighbouring table row, and the epsilon kernel fed with v
        _control(storage, _live(_ddim(dev, inp, cfg, dt, None, table=table, index=1)[:nimg]), ref, s, f"{tag} with the neighbouring row")
        v8, xe, _ = _dev_inputs(dev, inp, cfg, dt)
        (ops.cfg_ddim_step(v8, xe, nimg, hw, NC, g, *_c4(**COEF)) if cfg else ops.ddim_step(v8, xe, nimg, hw, NC, *_c4(**COEF)))
        _control(storage, _live(xe[:nimg]), ref, s, f"{tag} through the epsilon step")


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "plain"])
@pytest.mark.parametrize("nimg,hw", SHAPES)
@pytest.mark.parametrize("storage", STORAGE)
def test_unipc_v_budget(dev, storage, nimg, hw, cfg):
    """Rows 0 (no corrector), 2 (corrector, r[9] != 0) and 5 (the last) of the v-prediction plan of 6 steps."""
    dt = R.DTYPES[storage]
    g = R.GUIDANCE if cfg else None
    rows = [[float(v) for v in r] for _, r in UniPCMultistepScheduler(prediction_type="v_prediction").plan(6)]
    inp = R.inputs(_rand, nimg, hw, 711, dt, cfg=cfg)
    for k in (0, 2, 5):
        ref = R.vunipc_ref(inp, rows[k], g)
        got, raw = _unipc(dev, inp, cfg, dt, rows, k)
        tag = f"{'cfg_unipc_step_v' if cfg else 'unipc_step_v'} {storage} {nimg}x{hw} row {k}"
        for nm in ("x", "last", "m0"):
            if nm == "last" and rows[k][2] == 0:
                assert torch.equal(_live(got[nm]), inp["x"])                  # no corrector: last = x, exactly
                continue
            _check(storage, _live(got[nm]), *ref[nm], f"{tag} {nm}")
        _, raw_t = _unipc(dev, inp, cfg, dt, rows, k, table=True)
        assert all(torch.equal(a, b) for a, b in zip(raw, raw_t)), f"{tag}: table + index form differs from the immediate row"
        if nimg * hw >= 256:
            eps_row = list(rows[k])
            eps_row[10] = 0.0                                                 # the epsilon plan's row: x0 = -sigma_t v
            wrong, _ = _unipc(dev, inp, cfg, dt, [eps_row] * 6, k)
            _control(storage, _live(wrong["m0"]), *ref["m0"], f"{tag} m0 with alpha_t missing from the row")


# ------------------------------------------------------------------ exact operands
@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("g", [1.0, 0.0])
def test_exact_operands_give_exact_bits(dev, storage, g):
    """Small integers in v and x, integer constants, guidance 1 and 0: every product and sum is exact in fp32 and in the storage type, so
    the result equals the integer formula bit for bit (guidance 1 -> the conditional v, guidance 0 -> the unconditional one)."""
    dt = R.DTYPES[storage]
    inp = R.inputs(_rand, 3, 37, 721, dt, exact=True)
    n = inp["nimg"]
    v = inp["eps"][n:] if g == 1.0 else inp["eps"][:n]
    sa_t, s1m_t, sa_p, s1m_p = 2.0, 1.0, 3.0, 2.0
    want = sa_p * (sa_t * inp["x"] - s1m_t * v) + s1m_p * (sa_t * v + s1m_t * inp["x"])
    assert want.abs().max() < 256                                             # integers every storage type holds exactly
    x8 = _ddim(dev, inp, True, dt, (sa_t, s1m_t, sa_p, s1m_p), g=g)
    assert torch.equal(_live(x8[:n]), want)
    row = [0.5, 1.0, 1.0, 2.0, -1.0, 1.0, 3.0, 2.0, -2.0, 1.0, 2.0, 0.0]    # x0 = 2 x - v; corrector and predictor with integer weights
    last, m0, m1 = inp["state"]
    x0 = 2.0 * inp["x"] - v
    xc = 2.0 * last - m0 + m1 + 3.0 * x0
    got, _ = _unipc(dev, inp, True, dt, [row], 0, g=g)
    assert torch.equal(_live(got["m0"]), x0) and torch.equal(_live(got["last"]), xc)
    assert torch.equal(_live(got["x"]), 2.0 * xc - 2.0 * x0 + m0)


# ------------------------------------------------------------------ an image alone = the same image in a batch
@pytest.mark.parametrize("storage", STORAGE)
def test_an_image_alone_equals_the_image_in_a_batch(dev, storage):
    dt = R.DTYPES[storage]
    rows = [[float(v) for v in r] for _, r in UniPCMultistepScheduler(prediction_type="v_prediction").plan(6)]
    for hw in (64, 192, 37):
        inp = R.inputs(_rand, 3, hw, 731, dt)
        x3 = _ddim(dev, inp, True, dt, _c4(**COEF))
        u3, _ = _unipc(dev, inp, True, dt, rows, 2)
        for i in range(3):
            one = dict(eps=torch.cat([inp["eps"][i:i + 1], inp["eps"][3 + i:4 + i]]), x=inp["x"][i:i + 1], state=inp["state"][:, i:i + 1],
                       nimg=1, hw=hw)
            assert torch.equal(_ddim(dev, one, True, dt, _c4(**COEF))[0], x3[i]), (hw, i)
            u1, _ = _unipc(dev, one, True, dt, rows, 2)
            for nm in ("x", "last", "m0"):
                assert torch.equal(u1[nm][0], u3[nm][i]), (hw, i, nm)


# ------------------------------------------------------------------ the _dev forms over a schedule
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "plain"])
@pytest.mark.parametrize("storage", STORAGE)
def test_dev_forms_equal_the_host_constant_forms_over_a_schedule(dev, storage, cfg):
    """Four steps with the step counter on the device (ops.index_add between the steps, as the captured step graph does) against the
    same four steps with the constants as launch arguments: bit for bit, DDIM and UniPC."""
    dt = R.DTYPES[storage]
    nimg, hw, steps = 3, 64, 4
    sch = DDIMScheduler(prediction_type="v_prediction")
    ts = sch.set_timesteps(steps)
    coefs = [sch.step_coefficients(t) for t in ts]
    plan = [[float(v) for v in r] for _, r in UniPCMultistepScheduler(prediction_type="v_prediction").plan(steps)]
    g = R.GUIDANCE
    outs = [R.inputs(_rand, nimg, hw, 741 + 10 * k, dt, cfg=cfg)["eps"] for k in range(steps)]      # a "network output" per step
    inp = R.inputs(_rand, nimg, hw, 741, dt, cfg=cfg)
    for kind in ("ddim", "unipc"):
        res = []
        for on_device in (False, True):
            _, x8, st8 = _dev_inputs(dev, inp, cfg, dt)
            st8.zero_()
            idx = torch.zeros(1, dtype=torch.int32, device=dev)
            table = torch.tensor(coefs if kind == "ddim" else plan, dtype=torch.float32, device=dev)
            for k in range(steps):
                v8 = _pad8(outs[k], dev, dt)
                if kind == "ddim" and on_device:
                    ops.ddim_step_v_dev(v8, x8, nimg, hw, NC, g, table, idx, cfg=cfg)
                elif kind == "ddim":
                    (ops.cfg_ddim_step_v(v8, x8, nimg, hw, NC, g, *coefs[k]) if cfg else ops.ddim_step_v(v8, x8, nimg, hw, NC, *coefs[k]))
                else:
                    kw = dict(table=table, index=idx) if on_device else dict(row=plan[k])
                    (ops.cfg_unipc_step_v(v8, x8, st8, nimg, hw, NC, g, **kw) if cfg else ops.unipc_step_v(v8, x8, st8, nimg, hw, NC, **kw))
                ops.index_add(idx, 1)
            res.append((x8.clone(), st8.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (kind, storage, cfg)
        assert torch.isfinite(res[0][0].float()).all()


# ------------------------------------------------------------------ v kernels on v = epsilon kernels on the equivalent eps
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "plain"])
def test_v_steps_agree_with_the_epsilon_steps_on_the_equivalent_eps(dev, cfg):
    """fp32 storage: eps = sqrt(a_t) v + sqrt(1 - a_t) x (float64, rounded to fp32) through the epsilon kernels gives the step the v
    kernels give on v, within the fp32 budget of BOTH kernels plus the rounding of the eps that was handed over -- a cross-check of
    the constants (which coefficient multiplies what), not a bit test."""
    dt, storage = torch.float32, "fp32"
    nimg, hw = 3, 192
    inp = R.inputs(_rand, nimg, hw, 751, dt, cfg=cfg)
    a_t, a_p = COEF["a_t"], COEF["a_p"]
    sa_t, s1m_t = float(torch.tensor(a_t ** 0.5)), float(torch.tensor((1 - a_t) ** 0.5))       # as the kernels receive them
    xx = torch.cat([inp["x"], inp["x"]]) if cfg else inp["x"]
    as_eps = dict(inp, eps=(sa_t * inp["eps"] + s1m_t * xx).float().double())
    g = R.GUIDANCE if cfg else None
    ref, s = R.vddim_ref(inp, a_t, a_p, g)
    xv = _live(_ddim(dev, inp, cfg, dt, _c4(a_t, a_p))[:nimg])
    e8, xe, _ = _dev_inputs(dev, as_eps, cfg, dt)
    (ops.cfg_ddim_step(e8, xe, nimg, hw, NC, g, *_c4(a_t, a_p)) if cfg else ops.ddim_step(e8, xe, nimg, hw, NC, *_c4(a_t, a_p)))
    xe = _live(xe[:nimg])
    # the epsilon path divides by sqrt(a_t) what the v path never multiplied: its terms are 1 / a_t times larger, and
    # sa_t^2 + s1m_t^2 = 1 holds to fp32 rounding only -- both enter through the magnitude below
    slack = abs(sa_t * sa_t + s1m_t * s1m_t - 1.0) / R.UNITS[storage]
    lim = R.VPRED_LIMITS[storage]["max"] * (1.0 + 1.0 / a_t) + slack + 2.0
    err = ((xv - xe).abs() / (R.UNITS[storage] * s)).max().item()
    print(f"\n[cross-check] ddim {'cfg' if cfg else 'plain'}: max |v path - eps path| = {err:.2f} units (limit {lim:.1f})")
    assert err <= lim
    _check(storage, xv, ref, s, "the v path itself")
    # UniPC: row k of the v plan against the epsilon kernel on the equivalent eps with the epsilon plan's row
    rows_v = [[float(v) for v in r] for _, r in UniPCMultistepScheduler(prediction_type="v_prediction").plan(6)]
    rows_e = [[float(v) for v in r] for _, r in UniPCMultistepScheduler().plan(6)]
    k = 2
    al, sg = float(torch.tensor(rows_v[k][10])), float(torch.tensor(rows_v[k][1]))
    as_eps = dict(inp, eps=(al * inp["eps"] + sg * xx).float().double())
    gv, _ = _unipc(dev, inp, cfg, dt, rows_v, k)
    e8, xe8, st8 = _dev_inputs(dev, as_eps, cfg, dt)
    (ops.cfg_unipc_step(e8, xe8, st8, nimg, hw, NC, g, row=rows_e[k]) if cfg else ops.unipc_step(e8, xe8, st8, nimg, hw, NC, row=rows_e[k]))
    uref = R.vunipc_ref(inp, rows_v[k], g)
    for nm, got_e in (("x", xe8[:nimg]), ("last", st8[0]), ("m0", st8[1])):
        s = uref[nm][1]
        err = ((_live(gv[nm]) - _live(got_e)).abs() / (R.UNITS[storage] * s)).max().item()
        lim = R.VPRED_LIMITS[storage]["max"] * (1.0 + 1.0 / (al * al)) + abs(al * al + sg * sg - 1.0) / R.UNITS[storage] + 2.0
        print(f"[cross-check] unipc {nm}: {err:.2f} units (limit {lim:.1f})")
        assert err <= lim, nm


# ------------------------------------------------------------------ refusals (nothing is launched)
def test_refusals_on_the_device(dev):
    x = torch.zeros(2, 16, 8, device=dev, dtype=torch.bfloat16)
    st = torch.zeros(3, 1, 16, 8, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="v is torch.float16"):
        ops.cfg_ddim_step_v(x.to(torch.float16), x, 1, 16, 4, 7.5, 0.5, 0.5, 0.5, 0.5)
    with pytest.raises(ValueError, match="state is torch.float32"):
        ops.cfg_unipc_step_v(x, x, st.float(), 1, 16, 4, 7.5, row=[1.0] * 12)
    with pytest.raises(ValueError):
        ops.ddim_step_v(x, x, 1, 16, 4, 0.5, 0.5, 0.5, 0.5)                    # two images' worth of rows for nimg = 1 without CFG
    with pytest.raises(RuntimeError, match="SASPA_EINVAL"):
        ops.cfg_ddim_step_v(x, x, 1, 16, 4, 7.5, 0.0, 0.5, 0.5, 0.5)           # sqrt(a_t) = 0: refused like the epsilon step
    with pytest.raises(RuntimeError, match="SASPA_ERANGE"):
        ops.cfg_ddim_step_v(x, x, 1, 16, 9, 7.5, 0.5, 0.5, 0.5, 0.5)           # more live channels than a pixel has
    lib = _lib.load()
    ptr = C.c_void_p(x.data_ptr())
    for fn in (lib.saspa_cfg_ddim_step_v, lib.saspa_cfg_ddim_step):
        assert fn(_lib.SASPA_BF16, None, ptr, 1, 16, 4, 8, 7.5, 0.5, 0.5, 0.5, 0.5, None) == _lib.SASPA_EINVAL        # null pointer
        assert fn(_lib.SASPA_F16, ptr, ptr, 1, 16, 4, 8, 7.5, 0.5, 0.5, 0.5, 0.5, None) == _lib.SASPA_EINVAL          # not this library's
        assert fn(_lib.SASPA_BF16, ptr, ptr, 1, 16, 4, 4, 7.5, 0.5, 0.5, 0.5, 0.5, None) == _lib.SASPA_ERANGE         # half-vector pixels
    assert torch.equal(x, torch.zeros_like(x))
