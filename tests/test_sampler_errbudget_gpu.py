"""ONE update of the multistep sampler kernels of csrc/saspa_elem.hip (cfg_unipc_step, unipc_step, cfg_plms_step, ddim_step,
vae_sample_noise) in bf16, from exact bf16 inputs with every state buffer filled, against the float64 references of
tests/sampler_ref.py under the elem budget of tests/errbudget.py -- every tensor the step writes, on three blocks and a tail, on one
pixel and on one pixel per image.  (The multi-step drift tests of tests/test_unipc.py and tests/test_blip_gpu.py test the host plans.)
tests/test_errbudget.py proves on the CPU that the budget accepts the fp32 emulations of these steps at half its limits and rejects
truncating stores, guidance 7.0, a predictor reading m1 for m0, a skipped corrector, rotated history weights and exp(logvar)."""
import pytest
import torch
import torch.nn.functional as F

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import ops
from tests import sampler_ref as S
from tests.errbudget import LIMITS, UNIT_BF16, check_budget, fmt, rejects
from tests.test_errbudget import _rand

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C = S.C
JUNK = 3.0                             # channels 4..7 of the x that goes in: the step must write zeros there


def _check(got, ref, s, what):
    st = check_budget(got, ref, s, UNIT_BF16, limits=LIMITS["elem"], what=what)
    print(f"\n[budget] elem  {what}: {fmt(st)}")


def _control(got, ref, s, what):
    assert rejects(got, ref, s, UNIT_BF16, limits=LIMITS["elem"]), f"negative control not rejected: {what}"
    print(f"\n[control rejected] elem  {what}")


def _pad8(t, dev, fill=0.0):
    return F.pad(t.float(), (0, S.LDC - C), value=fill).to(dev, BF).contiguous()


def _live(t):
    """Channels < C as float64 on the host; channels C..7 must be zero."""
    t = t.cpu()
    assert (t[..., C:] == 0).all(), "channels 4..7 of a written tensor are not zero"
    return t[..., :C].double()


def _dev_inputs(dev, inp, cfg):
    x = torch.cat([inp["x"], inp["x"]]) if cfg else inp["x"]
    return _pad8(inp["eps"], dev), _pad8(x, dev, JUNK), _pad8(inp["state"], dev)


# ------------------------------------------------------------------ UniPC, with and without CFG
def _unipc_run(dev, inp, cfg, plan, k, *, g=S.GUIDANCE, table=False):
    eps8, x8, st8 = _dev_inputs(dev, inp, cfg)
    e0, m0_old = eps8.clone(), st8[1].clone()
    n, hw = inp["nimg"], inp["hw"]
    kw = dict(row=plan[k])
    if table:
        kw = dict(table=torch.tensor(plan, dtype=torch.float32, device=dev), index=torch.tensor([k], dtype=torch.int32, device=dev))
    if cfg:
        ops.cfg_unipc_step(eps8, x8, st8, n, hw, C, g, **kw)
        assert torch.equal(x8[:n], x8[n:])                                    # the two CFG halves
    else:
        ops.unipc_step(eps8, x8, st8, n, hw, C, **kw)
    assert torch.equal(eps8, e0)                                              # eps is read only
    assert torch.equal(st8[2], m0_old)                                        # m1 = the old m0, bits unchanged
    return dict(x=x8[:n], last=st8[0], m0=st8[1]), (x8, st8)


@pytest.mark.parametrize("cfg", [True, False], ids=["cfg_unipc_step", "unipc_step"])
@pytest.mark.parametrize("nimg,hw", S.SHAPES)
def test_unipc_step_budget(dev, nimg, hw, cfg):
    """Rows 0 (no corrector), 2 (corrector, r[9] != 0) and 5 (the last) of UniPCMultistepScheduler().plan(6): x, last, m0 under the
    budget, m1 bit-equal to the old m0, the table + index form bit-equal to the immediate row."""
    plan, rows = S.unipc_rows()
    g = S.GUIDANCE if cfg else None
    inp = S.inputs(_rand, nimg, hw, 501, cfg=cfg)
    for k in rows:
        ref = S.unipc_ref(inp, plan[k], g)
        got, raw = _unipc_run(dev, inp, cfg, plan, k)
        tag = f"{'cfg_unipc_step' if cfg else 'unipc_step'} {nimg}x{hw} row {k}"
        for nm in ("x", "last", "m0"):
            if nm == "last" and plan[k][2] == 0:
                assert torch.equal(_live(got[nm]), inp["x"])                  # no corrector: last = x, exactly
                continue
            _check(_live(got[nm]), *ref[nm], f"{tag} {nm}")
        _, raw_t = _unipc_run(dev, inp, cfg, plan, k, table=True)
        assert all(torch.equal(a, b) for a, b in zip(raw, raw_t)), f"{tag}: table + index form differs from the immediate row"
        if hw < 256:
            continue
        # negative controls: the changed step against the unchanged reference
        if cfg:
            wrong, _ = _unipc_run(dev, inp, cfg, plan, k, g=7.0)
            for nm in ("x", "m0"):
                _control(_live(wrong[nm]), *ref[nm], f"{tag} {nm} with guidance 7.0")
        wrong, _ = _unipc_run(dev, inp, cfg, plan, k + 1 if k == 0 else k - 1, table=True)
        for nm in ("x", "m0"):
            _control(_live(wrong[nm]), *ref[nm], f"{tag} {nm} with the neighbouring table row")


# ------------------------------------------------------------------ PLMS
def _plms_run(dev, inp, saved, plan, k, *, g=S.GUIDANCE, table=False, slot_shift=0):
    d = plan[k]
    eps8, x8, h8 = _dev_inputs(dev, inp, True)
    sv8 = _pad8(saved, dev)
    e0, x_old, h_old, sv_old = eps8.clone(), x8.clone(), h8.clone(), sv8.clone()
    n, hw = inp["nimg"], inp["hw"]
    store = d["store_slot"] + slot_shift if d["store_slot"] >= 0 else -1
    if table:
        rows = [S.plms_row(dict(p, store_slot=store if i == k else p["store_slot"])) for i, p in enumerate(plan)]
        ops.cfg_plms_step_dev(eps8, x8, h8, sv8, n, hw, C, g, torch.tensor(rows, dtype=torch.float32, device=dev),
                              torch.tensor([k], dtype=torch.int32, device=dev))
        if d["save_sample"]:
            assert torch.equal(sv8, x_old[:n])                                # the sample as it was before the update
        else:
            assert torch.equal(sv8, sv_old)
    else:
        ops.cfg_plms_step(eps8, x8, h8, sv8 if d["use_saved"] else None, n, hw, C, g, store, d["w_cur"], d["w_hist"], d["coef_sample"],
                          d["coef_model"])
        assert torch.equal(sv8, sv_old)
    assert torch.equal(eps8, e0) and torch.equal(x8[:n], x8[n:])
    for slot in range(4):
        if slot != store:
            assert torch.equal(h8[slot], h_old[slot]), f"history slot {slot} changed"
    return dict(x=x8[:n], hist=h8[d["store_slot"]] if d["store_slot"] >= 0 else None), (x8, h8)


@pytest.mark.parametrize("nimg,hw", S.SHAPES)
def test_cfg_plms_step_budget(dev, nimg, hw):
    """Rows of PNDMScheduler().plan(5): 0 (a store into a slot, no history weight, save_sample), 1 (use_saved, no store), 4 and 5
    (four weights): x and the written slot under the budget; the other slots and the saved sample keep their bits."""
    plan, rows = S.plms_rows()
    inp = S.inputs(_rand, nimg, hw, 511, nstate=4)
    saved = S._q(_rand(nimg, hw, C, seed=515))
    for k in rows:
        d = plan[k]
        ref = S.plms_ref(inp, d, saved=saved)
        tag = f"cfg_plms_step {nimg}x{hw} row {k}"
        got, raw = _plms_run(dev, inp, saved, plan, k)
        _check(_live(got["x"]), *ref["x"], f"{tag} x")
        if d["store_slot"] >= 0:
            _check(_live(got["hist"]), *ref["hist"], f"{tag} hist[{d['store_slot']}]")
        _, raw_t = _plms_run(dev, inp, saved, plan, k, table=True)
        assert all(torch.equal(a, b) for a, b in zip(raw, raw_t)), f"{tag}: table + index form differs from the immediate arguments"
        if hw < 256:
            continue
        wrong, _ = _plms_run(dev, inp, saved, plan, k, g=7.0)
        _control(_live(wrong["x"]), *ref["x"], f"{tag} x with guidance 7.0")
        wrong, _ = _plms_run(dev, inp, saved, plan, k + 1 if k == 0 else k - 1, table=True)
        _control(_live(wrong["x"]), *ref["x"], f"{tag} x with the neighbouring table row")
        if d["store_slot"] >= 0:
            wrong, _ = _plms_run(dev, inp, saved, plan, k, slot_shift=1 if d["store_slot"] < 3 else -1)
            _control(_live(wrong["hist"]), *ref["hist"], f"{tag} hist[{d['store_slot']}] with the store one slot off")


# ------------------------------------------------------------------ DDIM without CFG, VAE sample + noise
@pytest.mark.parametrize("nimg,hw", S.SHAPES)
def test_ddim_step_budget(dev, nimg, hw):
    inp = S.inputs(_rand, nimg, hw, 521, cfg=False)
    ref, s = S.ddim_ref(inp, **S.DDIM_COEF)

    def run(a_t, a_p):
        eps8, x8, _ = _dev_inputs(dev, inp, False)
        e0 = eps8.clone()
        ops.ddim_step(eps8, x8, nimg, hw, C, a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5)
        assert torch.equal(eps8, e0)
        return _live(x8)
    _check(run(**S.DDIM_COEF), ref, s, f"ddim_step {nimg}x{hw}")
    if hw >= 256:
        _control(run(S.DDIM_COEF["a_t"], 0.5), ref, s, f"ddim_step {nimg}x{hw} with the next step's alpha")


@pytest.mark.parametrize("npix", [600, 1, 2])
def test_vae_sample_noise_bf16_budget(dev, npix):
    """bf16 (tests/test_sdedit_gpu.py runs it in fp32), with that test's two log-variance clamps."""
    v = S.vae_inputs(_rand, npix, 531)
    ref, s = S.vae_ref(v, **S.VAE_COEF)

    def run(scaling, sa, s1m):
        args = [v[k].to(dev, BF).reshape(1, npix, 1, S.LDC) for k in ("mom", "e1", "e2")]
        keep = [a.clone() for a in args]
        out = ops.vae_sample_noise(*args, scaling, sa, s1m)
        assert all(torch.equal(a, b) for a, b in zip(args, keep))
        return _live(out.reshape(npix, S.LDC))
    _check(run(**S.VAE_COEF), ref, s, f"vae_sample_noise {npix} pixels")
    if npix >= 256:
        _control(run(S.VAE_COEF["scaling"], S.VAE_COEF["s1m"], S.VAE_COEF["sa"]), ref, s, "vae_sample_noise with sa and s1m swapped")
