"""TEST INFRASTRUCTURE ONLY -- float64 references, magnitudes, fp32 emulations and mutants of ONE update of the sampler-step
kernels of csrc/saspa_elem.hip, from exact bf16 inputs with every state buffer filled.  CPU only; the CPU proof
(tests/test_errbudget.py) and the GPU tests (tests/test_sampler_errbudget_gpu.py) both import it.

The kernels keep the guided eps, x0 and the corrected sample in fp32 inside one step; the only rounding points are the stores.
- cfg_unipc_kernel (saspa_elem.hip:166-200; CFG = false: unipc_step, eps is one evaluation per image and x is not duplicated):
    e = eu + g (ec - eu) (:186);  x0 = (x - r[1] e) r[0] (:187);
    xc = r[2] != 0 ? r[3] last + r[4] m0 + r[5] m1 + r[6] x0 : x (:188-189);
    stores: last = xc (:194), m1 = the OLD m0, bits unchanged (:195), m0 = x0 (:196), x = r[7] xc + r[8] x0 + r[9] m0_old (:191, :197).
- cfg_plms_kernel (:116-156): e as above (:138);  m = w_cur e + sum_k w[k] hist[k] over the slots with w[k] != 0 (:139-148);
    stores: hist[store_slot] = e (:150), x = cx s + cm m with s = the saved sample or x (:152-154), saved = x before the update when
    the table row says save_sample (:135).
- cfg_ddim_kernel<CFG = false> (:249-272): x = sa_p (x - s1m_t e) / sa_t + s1m_p e.
- vae_sample_noise_kernel (:598-614): out = sa (mean + exp(0.5 clamp(logvar, -30, 20)) e1) scaling + s1m e2.
Channels >= C of every written tensor are zero.

Magnitudes: the sum of |coefficient * term| expanded down to the inputs (the guided eps counts as |1 - g| |eu| + g |ec|), floored at
2^-10 of their mean as tests/test_errbudget.cfg_ddim_ref does.
"""
import torch

BF = torch.bfloat16
C, LDC = 4, 8
SHAPES = [(2, 300), (1, 1), (2, 1)]    # (nimg, hw): three 256-thread blocks and a tail; one pixel; one pixel per image
GUIDANCE = 7.5


def rne(x):
    return x.float().to(BF).double()


def trunc(x):
    i = x.float().contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).double()


def _floor(s):
    return s.clamp_min(max(2.0 ** -10 * s.mean().item(), 1e-30))


def _q(t):
    return t.to(BF).double()


def inputs(rand, nimg, hw, seed, *, cfg=True, nstate=3):
    """bf16 values in float64: eps [2 nimg | nimg, hw, 4], x [nimg, hw, 4], state [nstate, nimg, hw, 4] (all filled)."""
    return dict(eps=_q(rand((2 if cfg else 1) * nimg, hw, C, seed=seed)), x=_q(rand(nimg, hw, C, seed=seed + 1)),
                state=_q(rand(nstate, nimg, hw, C, seed=seed + 2)), nimg=nimg, hw=hw)


def _guided(eps, nimg, g, dt=torch.float64):
    """(e, its magnitude); g None: no CFG."""
    eps = eps.to(dt)
    if g is None:
        return eps, eps.abs()
    eu, ec = eps[:nimg], eps[nimg:]
    return eu + g * (ec - eu), abs(1 - g) * eu.abs() + abs(g) * ec.abs()


# ------------------------------------------------------------------ UniPC
def unipc_ref(inp, r, g=GUIDANCE):
    """-> dict name -> (float64 reference, magnitude) for x, last, m0; 'm1' -> the old m0 (bit-equal)."""
    r = [float(v) for v in r]
    x = inp["x"]
    last, m0, m1 = inp["state"]
    e, se = _guided(inp["eps"], inp["nimg"], g)
    x0 = (x - r[1] * e) * r[0]
    s0 = abs(r[0]) * (x.abs() + abs(r[1]) * se)
    if r[2] != 0:
        xc = r[3] * last + r[4] * m0 + r[5] * m1 + r[6] * x0
        sc = (r[3] * last).abs() + (r[4] * m0).abs() + (r[5] * m1).abs() + abs(r[6]) * s0
    else:
        xc, sc = x, x.abs()
    out = r[7] * xc + r[8] * x0 + r[9] * m0
    so = abs(r[7]) * sc + abs(r[8]) * s0 + (r[9] * m0).abs()
    return dict(x=(out, _floor(so)), last=(xc, _floor(sc)), m0=(x0, _floor(s0)), m1=m0)


def unipc_emul(inp, r, g=GUIDANCE, *, rnd=rne, m1_for_m0=False, skip_corrector=False):
    """The kernel in fp32 -> dict x, last, m0.  Mutants: rnd = trunc, g = 7.0, m1_for_m0 (the predictor reads m1 where the old m0
    belongs), skip_corrector (the corrector left out although r[2] != 0)."""
    f = torch.float32
    r = [torch.tensor(float(v), dtype=f) for v in r]
    x = inp["x"].to(f)
    last, m0, m1 = inp["state"].to(f)
    e, _ = _guided(inp["eps"], inp["nimg"], None if g is None else torch.tensor(g, dtype=f), f)
    x0 = (x - r[1] * e) * r[0]
    xc = x
    if r[2] != 0 and not skip_corrector:
        xc = r[3] * last + r[4] * m0 + r[5] * m1 + r[6] * x0
    out = r[7] * xc + r[8] * x0 + r[9] * (m1 if m1_for_m0 else m0)
    return dict(x=rnd(out), last=rnd(xc), m0=rnd(x0))


# ------------------------------------------------------------------ PLMS
def plms_ref(inp, d, g=GUIDANCE, saved=None):
    """inp['state']: the four history slots.  d: a row of PNDMScheduler().plan().  -> dict x, hist (None without a store)."""
    x, hist = inp["x"], inp["state"]
    e, se = _guided(inp["eps"], inp["nimg"], g)
    m, sm = d["w_cur"] * e, abs(d["w_cur"]) * se
    for k, w in enumerate(d["w_hist"]):
        m, sm = m + w * hist[k], sm + (w * hist[k]).abs()
    sv = saved if d["use_saved"] else x
    out = d["coef_sample"] * sv + d["coef_model"] * m
    so = (d["coef_sample"] * sv).abs() + abs(d["coef_model"]) * sm
    return dict(x=(out, _floor(so)), hist=(e, _floor(se)) if d["store_slot"] >= 0 else None)


def plms_emul(inp, d, g=GUIDANCE, saved=None, *, rnd=rne, rotate=0):
    """The kernel in fp32.  Mutants: rnd = trunc, g = 7.0, rotate = 1 (the history weights rotated by one slot)."""
    f = torch.float32
    x, hist = inp["x"].to(f), inp["state"].to(f)
    e, _ = _guided(inp["eps"], inp["nimg"], torch.tensor(g, dtype=f), f)
    m = torch.tensor(d["w_cur"], dtype=f) * e
    wh = list(d["w_hist"])
    wh = wh[-rotate:] + wh[:-rotate] if rotate else wh
    for k, w in enumerate(wh):
        if w != 0:
            m = m + torch.tensor(w, dtype=f) * hist[k]
    sv = saved.to(f) if d["use_saved"] else x
    out = torch.tensor(d["coef_sample"], dtype=f) * sv + torch.tensor(d["coef_model"], dtype=f) * m
    return dict(x=rnd(out), hist=rnd(e))


def plms_row(d):
    """The device-table row of cfg_plms_step_dev (pipeline.py builds the same)."""
    return [d["store_slot"], d["w_cur"], *d["w_hist"], d["coef_sample"], d["coef_model"], float(d["save_sample"]),
            float(d["use_saved"])]


# ------------------------------------------------------------------ DDIM without CFG, VAE sample + noise
DDIM_COEF = dict(a_t=0.3, a_p=0.45)


def ddim_ref(inp, a_t, a_p):
    """tests/test_errbudget.cfg_ddim_ref's formula without guidance: out = A x + B e."""
    x, e = inp["x"], inp["eps"]
    sa_t, s1m_t, sa_p, s1m_p = a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5
    ref = sa_p * (x - s1m_t * e) / sa_t + s1m_p * e
    a, b = sa_p / sa_t, s1m_p - sa_p * s1m_t / sa_t
    return ref, _floor((a * x).abs() + abs(b) * e.abs())


def ddim_emul(inp, a_t, a_p, rnd=rne):
    f = torch.float32
    x, e = inp["x"].to(f), inp["eps"].to(f)
    x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    return rnd(a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e)


VAE_COEF = dict(scaling=0.18215, sa=0.6, s1m=0.8)


def vae_inputs(rand, npix, seed):
    """bf16 moments [npix, 8] (mean | logvar) with the two log-variance clamps of tests/test_sdedit_gpu.py, e1, e2 [npix, 8]."""
    mom = rand(npix, LDC, seed=seed)
    mom[0, 4] = 50.0                   # clamp(logvar, -30, 20)
    mom[min(1, npix - 1), 5] = -60.0
    return dict(mom=_q(mom), e1=_q(rand(npix, LDC, seed=seed + 1)), e2=_q(rand(npix, LDC, seed=seed + 2)))


def vae_ref(v, scaling, sa, s1m):
    mean, lv = v["mom"][:, :4], v["mom"][:, 4:].clamp(-30, 20)
    sd = torch.exp(0.5 * lv)
    ref = sa * (mean + sd * v["e1"][:, :4]) * scaling + s1m * v["e2"][:, :4]
    return ref, _floor(abs(sa * scaling) * (mean.abs() + sd * v["e1"][:, :4].abs()) + (s1m * v["e2"][:, :4]).abs())


def vae_emul(v, scaling, sa, s1m, *, rnd=rne, half=0.5):
    """Mutant: half = 1.0 (exp(logvar) for exp(0.5 logvar))."""
    f = torch.float32
    mean, lv = v["mom"][:, :4].to(f), v["mom"][:, 4:].to(f).clamp(-30, 20)
    x0 = (mean + torch.exp(half * lv) * v["e1"][:, :4].to(f)) * scaling
    return rnd(sa * x0 + s1m * v["e2"][:, :4].to(f))


# ------------------------------------------------------------------ the catalogue ('elem' family)
def unipc_rows():
    """Three real rows of UniPCMultistepScheduler().plan(6): the first (no corrector), a middle one with r[9] != 0, the last."""
    from saspa_aug_amd.scheduler import UniPCMultistepScheduler
    plan = [[float(v) for v in r] for _, r in UniPCMultistepScheduler().plan(6)]
    assert plan[0][2] == 0 and plan[2][2] != 0 and plan[2][9] != 0 and plan[5][2] != 0
    return plan, (0, 2, 5)


def plms_rows():
    """Rows of PNDMScheduler().plan(5): 0 stores into slot 0 with no history weight and saves the sample, 1 reads the saved sample and
    stores nothing, 4 / 5 carry w_cur and three history weights (four weights: the full PLMS order)."""
    from saspa_aug_amd.scheduler import PNDMScheduler
    plan = [d for _, d in PNDMScheduler().plan(5)]
    assert plan[0]["save_sample"] and not any(plan[0]["w_hist"]) and plan[1]["use_saved"] and plan[1]["store_slot"] < 0
    assert sum(w != 0 for w in plan[5]["w_hist"]) == 3
    return plan, (0, 1, 4, 5)


def elem_cases(rand):
    out = []
    nimg, hw = SHAPES[0]
    plan, rows = unipc_rows()
    for cfg in (True, False):
        g = GUIDANCE if cfg else None
        inp = inputs(rand, nimg, hw, 501, cfg=cfg)
        for k in rows:
            ref = unipc_ref(inp, plan[k], g)
            tag = f"{'cfg_unipc' if cfg else 'unipc'} row {k}"
            emu = lambda **kw: unipc_emul(inp, plan[k], g, **kw)              # noqa: E731
            names = ("x", "last", "m0") if plan[k][2] != 0 else ("x", "m0")    # (without a corrector `last` is x itself: exact)
            for nm in names:
                out.append((f"legit fp32 {tag} {nm}", emu()[nm], *ref[nm], True))
                out.append((f"mutant truncating stores {tag} {nm}", emu(rnd=trunc)[nm], *ref[nm], False))
                if cfg:
                    out.append((f"mutant guidance 7.0 {tag} {nm}", unipc_emul(inp, plan[k], 7.0)[nm], *ref[nm], False))
            if plan[k][9] != 0:
                out.append((f"mutant UniPC predictor reads m1 for the old m0 {tag} x", emu(m1_for_m0=True)["x"], *ref["x"], False))
            if plan[k][2] != 0:
                for nm in ("x", "last") if plan[k][7] != 0 else ("last",):       # (the last row's x is its x0-prediction alone)
                    out.append((f"mutant UniPC corrector skipped {tag} {nm}", emu(skip_corrector=True)[nm], *ref[nm], False))
    plan, rows = plms_rows()
    inp = inputs(rand, nimg, hw, 511, nstate=4)
    saved = _q(rand(nimg, hw, C, seed=515))
    for k in rows:
        d = plan[k]
        ref = plms_ref(inp, d, saved=saved)
        tag = f"cfg_plms row {k}"
        for nm in ("x", "hist"):
            if ref[nm] is None:
                continue
            out.append((f"legit fp32 {tag} {nm}", plms_emul(inp, d, saved=saved)[nm], *ref[nm], True))
            out.append((f"mutant truncating stores {tag} {nm}", plms_emul(inp, d, saved=saved, rnd=trunc)[nm], *ref[nm], False))
            out.append((f"mutant guidance 7.0 {tag} {nm}", plms_emul(inp, d, 7.0, saved=saved)[nm], *ref[nm], False))
        if any(d["w_hist"]):
            out.append((f"mutant PLMS history weights rotated by one slot {tag} x", plms_emul(inp, d, saved=saved, rotate=1)["x"],
                        *ref["x"], False))
    inp = inputs(rand, nimg, hw, 521, cfg=False)
    ref, s = ddim_ref(inp, **DDIM_COEF)
    out.append(("legit fp32 ddim without cfg", ddim_emul(inp, **DDIM_COEF), ref, s, True))
    out.append(("mutant truncating stores ddim without cfg", ddim_emul(inp, **DDIM_COEF, rnd=trunc), ref, s, False))
    v = vae_inputs(rand, 600, 531)
    ref, s = vae_ref(v, **VAE_COEF)
    out.append(("legit fp32 vae_sample_noise", vae_emul(v, **VAE_COEF), ref, s, True))
    out.append(("mutant truncating stores vae_sample_noise", vae_emul(v, **VAE_COEF, rnd=trunc), ref, s, False))
    out.append(("mutant exp(logvar) for exp(0.5 logvar) vae_sample_noise", vae_emul(v, **VAE_COEF, half=1.0), ref, s, False))
    return out
