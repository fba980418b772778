"""TEST INFRASTRUCTURE ONLY -- references for the ControlNet-free text-to-image / SD-2.1 pipelines and for the v-prediction sampler
steps of csrc/saspa_elem.hip.  CPU only; tests/test_sd21_host.py (the CPU proof) and the GPU tests import it.

1. Pipelines: the existing oracle functions composed into text tower -> unet_forward without residuals -> CFG -> oracle DDIM / UniPC ->
   vae_decode (and the same behind a VAE-encoded source image).  The oracle's schedulers take eps; a v-prediction network output is
   handed to them as eps = sqrt(a_t) v + sqrt(1 - a_t) x, from which their own x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t) is the
   published sqrt(a_t) x - sqrt(1 - a_t) v.

2. ONE v-prediction update, in the manner of tests/sampler_ref.py: float64 references with magnitudes, fp32 emulations of the kernels
   (cfg_ddim_v_kernel, cfg_unipc_v_kernel) and named mutants, for the three storage types.
     v = vu + g (vc - vu);  DDIM: x0 = sa_t x - s1m_t v;  e = sa_t v + s1m_t x;  x' = sa_p x0 + s1m_p e
     UniPC: x0 = r[10] x - r[1] v, then the corrector / predictor of cfg_unipc_kernel (sampler_ref.unipc_ref) on that x0.
   Magnitudes: the sum of |coefficient * term| of the four products the DDIM kernel forms (they partly cancel: sa_p sa_t + s1m_p s1m_t
   and s1m_p sa_t - sa_p s1m_t are the net coefficients), the guided v counted as |1 - g| |vu| + g |vc|, floored as sampler_ref does.
"""
import math

import torch

from oracle import pipeline as OP
from oracle import sd_models as M
from tests import sampler_ref as SR

C, LDC = SR.C, SR.LDC
GUIDANCE = SR.GUIDANCE
DDIM_COEF = dict(a_t=0.3, a_p=0.45)            # the operating point of tests/test_errbudget.CFG_COEF
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
UNITS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}     # half an ulp at the bottom of a binade


# ------------------------------------------------------------------ pipelines
class _VAsEps:
    """An oracle scheduler (DDIM / UniPC: `step(eps, t, x)`) fed with a v-prediction output."""

    def __init__(self, sch):
        self.sch = sch
        self.init_noise_sigma = sch.init_noise_sigma

    def set_timesteps(self, n):
        self.k = 0
        return self.sch.set_timesteps(n)

    def step(self, v, t, x):
        if isinstance(self.sch, OP.UniPC):
            a, s = self.sch._as(self.sch.sigmas[self.k])           # alpha_t, sigma_t of this evaluation (float64)
            a, s = float(a), float(s)
        else:
            a_t = float(self.sch.alphas_cumprod[int(t)])
            a, s = a_t ** 0.5, (1 - a_t) ** 0.5
        self.k += 1
        return self.sch.step((a * v.double() + s * x.double()).to(v.dtype if isinstance(self.sch, OP.DDIM) else torch.float64), t, x)


def scheduler(sampler="ddim", prediction_type="epsilon"):
    sch = OP.DDIM() if sampler == "ddim" else OP.UniPC()
    return _VAsEps(sch) if prediction_type == "v_prediction" else sch


def _denoise(weights, cfgs, ctx, x, sch, ts, guidance_scale):
    for t in ts:
        out2 = M.unet_forward(weights["unet"], cfgs["unet"], torch.cat([x, x], 0), int(t), ctx)
        n = x.shape[0]
        out_u, out_c = out2[:n], out2[n:]
        x = sch.step(out_u + guidance_scale * (out_c - out_u), t, x).float()
    return x


def _context(weights, cfgs, ids_pos, ids_neg):
    b = ids_pos.shape[0]
    neg = ids_neg.expand(b, -1) if ids_neg.shape[0] == 1 else ids_neg
    return M.clip_text_forward(weights["text"], cfgs["text"], torch.cat([neg, ids_pos], 0))


def _finish(weights, cfgs, x):
    img = M.vae_decode(weights["vae"], cfgs["vae"], x / cfgs["vae"]["scaling_factor"])
    out = OP.postprocess(img)
    if "safety" in weights and "safety" in cfgs:
        out = OP.run_safety_checker(weights["safety"], cfgs["safety"], out)[0]
    return out, x, img


@torch.no_grad()
def txt2img(weights, cfgs, ids_pos, ids_neg, latents, steps, guidance_scale=7.5, sampler="ddim", prediction_type="epsilon"):
    """StableDiffusionPipeline.__call__ as the reference invokes it (run_aug/run_aug.py:235-241): ids_pos [B,77], ids_neg [1,77],
    latents fp32 [B,4,h,w].  -> (u8 [B,8h,8w,3], final latents, decoded float image)."""
    sch = scheduler(sampler, prediction_type)
    ctx = _context(weights, cfgs, ids_pos, ids_neg)
    x = latents.clone().float() * sch.init_noise_sigma
    return _finish(weights, cfgs, _denoise(weights, cfgs, ctx, x, sch, sch.set_timesteps(steps), guidance_scale))


@torch.no_grad()
def img2img(weights, cfgs, ids_pos, ids_neg, source_u8, sample_noise, noise, steps, strength, guidance_scale=7.5,
            prediction_type="epsilon"):
    """oracle.pipeline.sd_img2img_pipeline for a batch and either prediction type: source_u8 [B,H,W,3]."""
    import numpy as np
    sch = scheduler("ddim", prediction_type)
    ctx = _context(weights, cfgs, ids_pos, ids_neg)
    src = torch.from_numpy(np.ascontiguousarray(source_u8)).float().permute(0, 3, 1, 2) / 127.5 - 1.0
    mean, logvar = M.vae_encode(weights["vae"], cfgs["vae"], src)
    x0 = (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * sample_noise.float()) * cfgs["vae"]["scaling_factor"]
    ts_all = sch.set_timesteps(steps)
    ts = ts_all[max(steps - min(int(steps * strength), steps), 0):]
    a_t = OP.DDIM().alphas_cumprod[int(ts[0])]
    x = a_t ** 0.5 * x0 + (1 - a_t) ** 0.5 * noise.float()
    return _finish(weights, cfgs, _denoise(weights, cfgs, ctx, x, sch, ts, guidance_scale))


# ------------------------------------------------------------------ one v-prediction update
def rnd_to(dtype):
    """Round to the storage type (nearest even) and back to float64."""
    return lambda x: x.float().to(dtype).double()


def inputs(rand, nimg, hw, seed, dtype, *, cfg=True, exact=False):
    """Values of the storage type in float64: v [2 nimg | nimg, hw, 4], x [nimg, hw, 4], state [3, nimg, hw, 4] (all filled).
    exact: integers in [-4, 4] (with small integer coefficients every product and sum of the update is then exact in fp32, and the
    results are integers below 256, which bf16 holds exactly)."""
    def q(t):
        return (t * 2).round().clamp(-4, 4).double() if exact else t.to(dtype).double()
    return dict(eps=q(rand((2 if cfg else 1) * nimg, hw, C, seed=seed)), x=q(rand(nimg, hw, C, seed=seed + 1)),
                state=q(rand(3, nimg, hw, C, seed=seed + 2)), nimg=nimg, hw=hw)


def _coef(a_t, a_p, dt=None):
    c = (a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5)
    return c if dt is None else tuple(torch.tensor(v, dtype=dt) for v in c)          # (the kernels receive them as fp32)


def vddim_ref(inp, a_t, a_p, g=GUIDANCE):
    """-> (float64 reference, magnitude).  g None: no CFG."""
    sa_t, s1m_t, sa_p, s1m_p = (float(v) for v in _coef(a_t, a_p, torch.float32))
    x = inp["x"]
    v, sv = SR._guided(inp["eps"], inp["nimg"], g)
    x0 = sa_t * x - s1m_t * v
    e = sa_t * v + s1m_t * x
    s = sa_p * (sa_t * x.abs() + s1m_t * sv) + s1m_p * (sa_t * sv + s1m_t * x.abs())
    return sa_p * x0 + s1m_p * e, SR._floor(s)


def _fma(a, b, c):
    """a * b + c with one rounding to fp32 (the product of two fp32 values is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def vddim_emul(inp, a_t, a_p, g=GUIDANCE, *, rnd, form="plain", mutant=None, x0_rnd=None):
    """The kernel in fp32 -> the stored x'.  Legitimate forms: "plain" (every product and sum rounded to fp32), "fma" (the contractions
    the compiler may form), "guide_both" (guidance applied to x0 AND to e: the same affine map as guidance on v, other roundings).
    Mutants: "sign" (x0 = sa_t x + s1m_t v), "swap" (x0 and e exchanged in the last line),
    "guide_x0" (guidance on x0 only: e is taken from the conditional v), "eps_line" (v used as eps: x0 = (x - s1m_t v) / sa_t,
    x' = sa_p x0 + s1m_p v), "x0_rounded" (x0 rounded to the storage type before the last line; x0_rnd = that rounding)."""
    f = torch.float32
    sa_t, s1m_t, sa_p, s1m_p = _coef(a_t, a_p, f)
    x = inp["x"].to(f)
    n = inp["nimg"]
    gt = None if g is None else torch.tensor(g, dtype=f)
    v, _ = SR._guided(inp["eps"], n, gt, f)
    if form == "fma" and g is not None:
        vu, vc = inp["eps"][:n].to(f), inp["eps"][n:].to(f)
        v = _fma(gt, vc - vu, vu)
    if mutant == "eps_line":
        x0 = (x - s1m_t * v) / sa_t
        return rnd(sa_p * x0 + s1m_p * v)
    if mutant == "guide_x0" or form == "guide_both":
        vu, vc = inp["eps"][:n].to(f), inp["eps"][n:].to(f)
        x0u, x0c = sa_t * x - s1m_t * vu, sa_t * x - s1m_t * vc
        x0 = x0u + gt * (x0c - x0u)
        eu, ec = sa_t * vu + s1m_t * x, sa_t * vc + s1m_t * x
        e = ec if mutant == "guide_x0" else eu + gt * (ec - eu)
        return rnd(sa_p * x0 + s1m_p * e)
    if form == "fma":
        x0 = _fma(sa_t, x, -(s1m_t * v))
        e = _fma(sa_t, v, s1m_t * x)
        return rnd(_fma(sa_p, x0, s1m_p * e))
    x0 = sa_t * x + s1m_t * v if mutant == "sign" else sa_t * x - s1m_t * v
    e = sa_t * v + s1m_t * x
    if mutant == "x0_rounded":
        x0 = x0_rnd(x0).to(f)
    if mutant == "swap":
        x0, e = e, x0
    return rnd(sa_p * x0 + s1m_p * e)


def vunipc_row(k=2, steps=6):
    """Row k of the v-prediction UniPC plan (slot 10 = alpha_t); row 2 of 6 has a corrector and r[9] != 0."""
    from saspa_aug_amd.scheduler import UniPCMultistepScheduler
    return [float(v) for v in UniPCMultistepScheduler(prediction_type="v_prediction").plan(steps)[k][1]]


def vunipc_ref(inp, r, g=GUIDANCE):
    """-> dict name -> (float64 reference, magnitude) for x, last, m0; 'm1' -> the old m0 (bit-equal), as sampler_ref.unipc_ref."""
    r = [float(torch.tensor(v, dtype=torch.float32)) for v in r]
    x = inp["x"]
    last, m0, m1 = inp["state"]
    v, sv = SR._guided(inp["eps"], inp["nimg"], g)
    x0 = r[10] * x - r[1] * v
    s0 = abs(r[10]) * x.abs() + abs(r[1]) * sv
    if r[2] != 0:
        xc = r[3] * last + r[4] * m0 + r[5] * m1 + r[6] * x0
        sc = (r[3] * last).abs() + (r[4] * m0).abs() + (r[5] * m1).abs() + abs(r[6]) * s0
    else:
        xc, sc = x, x.abs()
    out = r[7] * xc + r[8] * x0 + r[9] * m0
    so = abs(r[7]) * sc + abs(r[8]) * s0 + (r[9] * m0).abs()
    return dict(x=(out, SR._floor(so)), last=(xc, SR._floor(sc)), m0=(x0, SR._floor(s0)), m1=m0)


def vunipc_emul(inp, r, g=GUIDANCE, *, rnd, form="plain", mutant=None, x0_rnd=None):
    """The kernel in fp32 -> dict x, last, m0.  Forms "plain" / "fma"; mutants "sign" (x0 = r10 x + r1 v), "eps_line" (x0 = (x - r1 v)
    r0, the epsilon kernel's line), "guide_x0" (x0 from the conditional v alone: what guidance on an x0 that is never formed per half
    degenerates to), "x0_rounded" (the predictor / corrector read the x0 that was stored)."""
    f = torch.float32
    r = [torch.tensor(float(v), dtype=f) for v in r]
    x = inp["x"].to(f)
    n = inp["nimg"]
    last, m0, m1 = inp["state"].to(f)
    gt = None if g is None else torch.tensor(g, dtype=f)
    v, _ = SR._guided(inp["eps"], n, gt, f)
    if mutant == "guide_x0":
        v = inp["eps"][n:].to(f)
    if form == "fma":
        if g is not None:
            v = _fma(gt, inp["eps"][n:].to(f) - inp["eps"][:n].to(f), inp["eps"][:n].to(f))
        x0 = _fma(r[10], x, -(r[1] * v))
    elif mutant == "sign":
        x0 = r[10] * x + r[1] * v
    elif mutant == "eps_line":
        x0 = (x - r[1] * v) * r[0]
    else:
        x0 = r[10] * x - r[1] * v
    x0u = x0_rnd(x0).to(f) if mutant == "x0_rounded" else x0
    xc = x
    if r[2] != 0:
        xc = _fma(r[6], x0u, _fma(r[5], m1, _fma(r[4], m0, r[3] * last))) if form == "fma" else \
            r[3] * last + r[4] * m0 + r[5] * m1 + r[6] * x0u
    out = _fma(r[9], m0, _fma(r[8], x0u, r[7] * xc)) if form == "fma" else r[7] * xc + r[8] * x0u + r[9] * m0
    return dict(x=rnd(out), last=rnd(xc), m0=rnd(x0))


DDIM_MUTANTS = ("sign", "swap", "guide_x0", "eps_line", "x0_rounded")
UNIPC_MUTANTS = ("sign", "guide_x0", "eps_line", "x0_rounded")
MUTANT_NAMES = dict(sign="the sign of the sqrt(1-a_t) v term", swap="x0 and eps swapped", guide_x0="guidance applied to x0 instead of v",
                    eps_line="the v line replaced by the epsilon line", x0_rounded="a second rounding of x0 to the storage type")
SHAPE = SR.SHAPES[0]                   # (2, 300): three 256-thread blocks and a tail


def vpred_cases(rand, storage):
    """[(name, got, ref, magnitude, legit, mutant key | None)] for one storage type ("bf16" | "fp16" | "fp32")."""
    dt = DTYPES[storage]
    rnd = rnd_to(dt)
    # the second rounding happens at the 16-bit width also under fp32 storage (a kernel that parks x0 in a 16-bit register)
    x0_rnd = rnd_to(torch.bfloat16) if storage == "fp32" else rnd
    nimg, hw = SHAPE
    out = []
    for cfg in (True, False):
        g = GUIDANCE if cfg else None
        inp = inputs(rand, nimg, hw, 601, dt, cfg=cfg)
        tag = "cfg_ddim_v" if cfg else "ddim_v"
        ref, s = vddim_ref(inp, **DDIM_COEF, g=g)
        for form in ("plain", "fma") + (("guide_both",) if cfg else ()):
            out.append((f"legit {form} {tag}", vddim_emul(inp, **DDIM_COEF, g=g, rnd=rnd, form=form), ref, s, True, None))
        for m in DDIM_MUTANTS:
            if m == "guide_x0" and not cfg:
                continue
            out.append((f"mutant {MUTANT_NAMES[m]} {tag}", vddim_emul(inp, **DDIM_COEF, g=g, rnd=rnd, mutant=m, x0_rnd=x0_rnd), ref, s,
                        False, m))
        row = vunipc_row()
        tag = "cfg_unipc_v" if cfg else "unipc_v"
        uref = vunipc_ref(inp, row, g)
        for nm in ("x", "last", "m0"):
            for form in ("plain", "fma"):
                out.append((f"legit {form} {tag} {nm}", vunipc_emul(inp, row, g, rnd=rnd, form=form)[nm], *uref[nm], True, None))
            for m in UNIPC_MUTANTS:
                if (m == "guide_x0" and not cfg) or (m == "x0_rounded" and nm == "m0"):      # (the stored m0 IS the rounded x0)
                    continue
                out.append((f"mutant {MUTANT_NAMES[m]} {tag} {nm}", vunipc_emul(inp, row, g, rnd=rnd, mutant=m, x0_rnd=x0_rnd)[nm],
                            *uref[nm], False, m))
    return out


# Limits of the v-prediction steps per storage type, in units of UNITS[storage]: max / rms / |bias| / |slope| as tests/errbudget.py
# defines them, placed as tests/test_errbudget.py places its own: at least 2x above the worst legitimate emulation and at least 2x
# below every separable mutant, over the seed shifts of test_errbudget.SEEDS (tests/test_sd21_host.py proves it; the measured table
# is profiles/vpred_errbudget.txt).  NOT SEPARABLE and therefore not asserted (see that file): "a second rounding of x0" under 16-bit
# storage -- the rounding of the output itself is as large as what the rounded x0 contributes.
VPRED_LIMITS = {
    "bf16": dict(max=2.2, rms=1.0, bias=0.025, slope=0.09),
    "fp16": dict(max=2.2, rms=1.0, bias=0.025, slope=0.09),
    "fp32": dict(max=10.0, rms=1.7, bias=0.05, slope=0.2),
}
NOT_SEPARABLE = {("bf16", "x0_rounded"), ("fp16", "x0_rounded")}


def quantum(storage):
    return UNITS[storage]


def transcription_ddim(v_u, v_c, x, alpha_prod_t, alpha_prod_t_prev, guidance_scale):
    """The published formulas, as printed (float64): classifier-free guidance of the pipelines and DDIMScheduler.step with
    prediction_type "v_prediction", eta = 0 ([upstream] diffusers scheduling_ddim.py, recalled)."""
    model_output = v_u + guidance_scale * (v_c - v_u)
    beta_prod_t = 1 - alpha_prod_t
    pred_original_sample = (alpha_prod_t ** 0.5) * x - (beta_prod_t ** 0.5) * model_output
    pred_epsilon = (alpha_prod_t ** 0.5) * model_output + (beta_prod_t ** 0.5) * x
    pred_sample_direction = (1 - alpha_prod_t_prev) ** 0.5 * pred_epsilon
    return alpha_prod_t_prev ** 0.5 * pred_original_sample + pred_sample_direction


def transcription_unipc_x0(v_u, v_c, x, alpha_t, sigma_t, guidance_scale):
    """UniPCMultistepScheduler.convert_model_output with predict_x0 and "v_prediction": x0_pred = alpha_t * sample - sigma_t * v."""
    model_output = v_u + guidance_scale * (v_c - v_u)
    return alpha_t * x - sigma_t * model_output


def eps_of_v(v, x, a_t):
    """The epsilon a v-prediction output is equivalent to (float64): the cross-check of the v kernels against the epsilon kernels."""
    return math.sqrt(a_t) * v + math.sqrt(1 - a_t) * x
