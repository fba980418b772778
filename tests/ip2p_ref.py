"""TEST INFRASTRUCTURE ONLY -- torch-CPU restatement of ``StableDiffusionInstructPix2PixPipeline.__call__`` as the reference
invokes it for BASE_MODEL = "ip2p" (run_aug/run_aug.py:174-176, :235-241, :252-255), composed from the oracle's networks
(oracle.sd_models) and scheduler (oracle.pipeline.DDIM), and the float64 reference of the fused three-branch guidance + DDIM update.

PARITY UNPINNED, like the rest of the denoiser oracle (oracle/__init__.py): diffusers is not installed, so what is restated here is
the specification this repository builds to:

- image latents = vae.encode(2 * image / 255 - 1).latent_dist.mode(): the posterior mean, NOT multiplied by the scaling factor;
- one randn((1, 4, H/8, W/8)) per image, times init_noise_sigma;
- three evaluations per step, unconditional first: (negative prompt, x | 0), (negative prompt, x | image latents),
  (prompt, x | image latents);
- e = e0 + gs (e2 - e1) + igs (e1 - e0), then DDIM (eta 0; the SD-1.5 scheduler values) on e.
"""
import numpy as np
import torch

from oracle import pipeline as OP
from oracle import sd_models as OM


def cfg3_ddim_ref(eps, xx, a_t, a_p, gs, igs):
    """float64 three-branch guidance + DDIM update and its magnitude.  eps: [3n, ...] in the groups (uncond | image | text), xx: [n, ...].
    out = A x + B e with e = (1 - igs) e0 + (igs - gs) e1 + gs e2 (tests/test_errbudget.cfg_ddim_ref with a third term)."""
    n = xx.shape[0]
    e0, e1, e2 = eps[:n].double(), eps[n:2 * n].double(), eps[2 * n:].double()
    e = e0 + gs * (e2 - e1) + igs * (e1 - e0)
    sa_t, s1m_t, sa_p, s1m_p = a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5
    ref = sa_p * (xx.double() - s1m_t * e) / sa_t + s1m_p * e
    A, B = sa_p / sa_t, s1m_p - sa_p * s1m_t / sa_t
    s = (A * xx.double()).abs() + abs(B) * (abs(1 - igs) * e0.abs() + abs(igs - gs) * e1.abs() + abs(gs) * e2.abs())
    return ref, s.clamp_min(2.0 ** -10 * s.mean().item())


def image_latents(weights, cfgs, source_u8):
    """u8 [H,W,3] -> [1,4,H/8,W/8]: the mode of the VAE posterior, unscaled."""
    src = torch.from_numpy(np.ascontiguousarray(source_u8)).float().permute(2, 0, 1)[None] / 127.5 - 1.0
    mean, _ = OM.vae_encode(weights["vae"], cfgs["vae"], src)
    return mean


def ip2p_step(weights, cfgs, sch, x, t, ctx3, img_lat, guidance_scale, image_guidance_scale):
    """One sampling step: three UNet evaluations (as one batch of 3), guidance, DDIM."""
    xin = torch.cat([torch.cat([x, torch.zeros_like(img_lat)], 1), torch.cat([x, img_lat], 1), torch.cat([x, img_lat], 1)], 0)
    e0, e1, e2 = OM.unet_forward(weights["unet"], cfgs["unet"], xin, int(t), ctx3).chunk(3)
    return sch.step(e0 + guidance_scale * (e2 - e1) + image_guidance_scale * (e1 - e0), t, x)


@torch.no_grad()
def ip2p_pipeline(weights, cfgs, ids_pos, ids_neg, source_u8, latents, steps, guidance_scale=7.5, image_guidance_scale=1.5,
                  return_latents=False):
    """ids_*: int64 [1,77]; source_u8: u8 [H,W,3]; latents: fp32 [1,4,H/8,W/8] noise.  Returns u8 [1,H,W,3] (and the final
    latents / the decoded float image if asked)."""
    neg = OM.clip_text_forward(weights["text"], cfgs["text"], ids_neg)
    pos = OM.clip_text_forward(weights["text"], cfgs["text"], ids_pos)
    ctx3 = torch.cat([neg, neg, pos], 0)
    img_lat = image_latents(weights, cfgs, source_u8)
    sch = OP.DDIM()
    x = latents.clone().float() * sch.init_noise_sigma
    for t in sch.set_timesteps(steps):
        x = ip2p_step(weights, cfgs, sch, x, t, ctx3, img_lat, guidance_scale, image_guidance_scale)
    img = OM.vae_decode(weights["vae"], cfgs["vae"], x / cfgs["vae"]["scaling_factor"])
    out = OP.postprocess(img)
    if "safety" in weights and "safety" in cfgs:
        out = OP.run_safety_checker(weights["safety"], cfgs["safety"], out)[0]
    if return_latents:
        return out, x, img
    return out
