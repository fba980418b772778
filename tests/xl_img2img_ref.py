"""CPU reference of StableDiffusionXLControlNetImg2ImgPipeline (tests only): the loop of oracle.pipeline.sdxl_controlnet_pipeline
restated with the img2img start of oracle.pipeline.sd_controlnet_img2img_pipeline -- oracle VAE encode, posterior sample, scale,
DDIM ("trailing") add-noise at the first kept timestep, then the UNet / ControlNet / text-tower calls from that timestep on, decode.
One image per call; the inputs the GPU tests share are built here once."""
import functools

import numpy as np
import torch

from oracle import pipeline as OP
from oracle import sd_models as M
from oracle.canny import generate_canny_array
from saspa_aug_amd import config as CFG
from saspa_aug_amd import weights as W
from saspa_aug_amd.synthetic import synthetic_image


@functools.lru_cache(maxsize=None)
def tiny_xl():
    cfgs = CFG.tiny_xl()
    return cfgs, W.synth_family(cfgs, seed=3)


def token_ids(cfgs, n, seed=1):
    """Token rows as the two tokenizers produce them: BOS, words, EOS then EOS padding (tower 1) / 0 padding (tower 2)."""
    v = cfgs["text"]["vocab"]
    rs = np.random.RandomState(seed)
    ids1 = np.full((n, 77), v - 1, np.int64)
    ids1[:, 0] = v - 2
    for r in range(n):
        k = rs.randint(5, 40)
        ids1[r, 1:1 + k] = rs.randint(0, v - 2, k)
    ids2 = ids1.copy()
    for r in range(n):
        ids2[r, int((ids1[r] == v - 1).argmax()) + 1:] = 0
    return ids1, ids2


@torch.no_grad()
def sdxl_controlnet_img2img(weights, cfgs, ids1, ids2, source_u8, control_u8, sample_noise, noise, steps, strength,
                            conditioning_scale=0.75, guidance_scale=0.0, neg_ids1=None, neg_ids2=None):
    """-> (u8 [1,H,W,3], final latents [1,4,h,w], decoded float image [1,3,H,W])."""
    h1, _ = M.clip_text_forward(weights["text"], cfgs["text"], ids1, penultimate=True)
    h2, pooled = M.clip_text_forward(weights["text2"], cfgs["text2"], ids2, penultimate=True)
    ctx = torch.cat([h1, h2], dim=-1)
    hh, ww = control_u8.shape[:2]
    cfg = guidance_scale > 1.0
    cond = OP.prepare_control(control_u8)
    if cfg:
        if neg_ids1 is None:
            nctx, npooled = torch.zeros_like(ctx), torch.zeros_like(pooled)
        else:
            n1, _ = M.clip_text_forward(weights["text"], cfgs["text"], neg_ids1, penultimate=True)
            n2, npooled = M.clip_text_forward(weights["text2"], cfgs["text2"], neg_ids2, penultimate=True)
            nctx = torch.cat([n1, n2], dim=-1)
        ctx = torch.cat([nctx, ctx], 0)
        pooled = torch.cat([npooled, pooled], 0)
        cond = torch.cat([cond, cond], 0)
    added = dict(text_embeds=pooled, time_ids=torch.tensor([[hh, ww, 0, 0, hh, ww]] * ctx.shape[0], dtype=torch.float32))
    src = torch.from_numpy(np.ascontiguousarray(source_u8)).float().permute(2, 0, 1)[None] / 127.5 - 1.0
    mean, logvar = M.vae_encode(weights["vae"], cfgs["vae"], src)
    x0 = (mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * sample_noise.float()) * cfgs["vae"]["scaling_factor"]
    sch = OP.DDIM(spacing="trailing")
    ts_all = sch.set_timesteps(steps)
    init = min(int(steps * strength), steps)
    ts = ts_all[max(steps - init, 0):]
    a_t = sch.alphas_cumprod[int(ts[0])]
    x = a_t ** 0.5 * x0 + (1 - a_t) ** 0.5 * noise.float()
    for t in ts:
        xin = torch.cat([x, x], 0) if cfg else x
        down, mid = M.controlnet_forward(weights["controlnet"], cfgs["controlnet"], xin, int(t), ctx, cond, conditioning_scale, added)
        eps = M.unet_forward(weights["unet"], cfgs["unet"], xin, int(t), ctx, down, mid, added)
        if cfg:
            eps_u, eps_c = eps.chunk(2)
            eps = eps_u + guidance_scale * (eps_c - eps_u)
        x = sch.step(eps, t, x)
    img = M.vae_decode(weights["vae"], cfgs["vae"], x / cfgs["vae"]["scaling_factor"])
    return OP.postprocess(img), x, img


@functools.lru_cache(maxsize=None)
def inputs(hh, ww, nimg=2):
    """(ids1, ids2, neg1, neg2, sources u8, controls u8, sample_noise, noise) of one image size; shared, never modified."""
    cfgs, _ = tiny_xl()
    ids1, ids2 = token_ids(cfgs, nimg)
    n1, n2 = token_ids(cfgs, 1, seed=9)
    srcs = np.stack([synthetic_image(hh, ww, 10 + i) for i in range(nimg)])
    ctrls = np.stack([generate_canny_array(s, 120, 200) for s in srcs])
    g = torch.manual_seed(1)
    draws = [torch.randn((1, 4, hh // 8, ww // 8), generator=g, dtype=torch.float32) for _ in range(2 * nimg)]
    return ids1, ids2, n1, n2, srcs, ctrls, torch.cat(draws[0::2]), torch.cat(draws[1::2])


@functools.lru_cache(maxsize=None)
def reference(hh, ww, steps, strength, guidance, negative):
    """(u8 [n,H,W,3], latents [n,4,h,w], float images [n,3,H,W]) of the oracle loop over inputs(hh, ww); computed once."""
    cfgs, fam = tiny_xl()
    ids1, ids2, n1, n2, srcs, ctrls, e1, e2 = inputs(hh, ww)
    tn = (lambda a: torch.from_numpy(a) if negative else None)
    rs = [sdxl_controlnet_img2img(fam, cfgs, torch.from_numpy(ids1[i:i + 1]), torch.from_numpy(ids2[i:i + 1]), srcs[i], ctrls[i],
                                  e1[i:i + 1], e2[i:i + 1], steps, strength, guidance_scale=guidance, neg_ids1=tn(n1), neg_ids2=tn(n2))
          for i in range(len(srcs))]
    return np.concatenate([r[0] for r in rs]), torch.cat([r[1] for r in rs]), torch.cat([r[2] for r in rs])
