"""Drop-in for the diffusers pipeline object the reference builds in `init_pipeline`
(run_aug/run_aug.py:128-230) and calls at run_aug/run_aug.py:278:

    pipe = StableDiffusionControlNetPipeline.from_pretrained(...).to(DEVICE, torch.float16)
    pipe.scheduler = DDIMScheduler.from_config(pipe.scheduler.config)
    image = pipe(prompt=..., image=<canny PIL>, num_inference_steps=..., generator=...,
                 guidance_scale=7.5, negative_prompt=..., controlnet_conditioning_scale=0.75).images[0]

Same names, argument meaning and error behaviour (Python exceptions; device problems are
RuntimeError, which is what the reference's loop catches, run_aug/run_aug.py:493).  The whole
sampling loop runs in the gfx950 kernels; `generate_batch` is the batched form (B images per
launch sequence, CFG doubles it) that run_aug and bench.py drive.

Precision: `.to(device, torch.float16)` / `torch.bfloat16` selects the bf16 MFMA path (the
MI355X counterpart of the reference's fp16 CUDA path; bf16 also avoids the SD-VAE fp16
overflow); `.to(device, torch.float32)` selects the exact-fp32 MFMA path used for the
end-to-end parity gate against the CPU oracle.  `pipe.enable_fp16()` before `.to()` (or
SASPA_FP16=1) makes `torch.float16` mean IEEE fp16 for the text tower, UNet, ControlNet and
scheduler steps (the f16-MFMA build of the kernels); the VAE and the safety checker stay out
of fp16 (`enable_fp16` docstring).  Off by default."""
import contextlib
import json
import os

import numpy as np
import torch
from PIL import Image

from . import imageproc, models, ops
from . import weights as W
from .config import BLIP_DIFFUSION, BLIP_IMAGE_MEAN, BLIP_IMAGE_STD, IP2P, SD15, SDXL_TURBO
from .scheduler import SDXL_TURBO_SCHEDULER_CONFIG, DDIMScheduler, PNDMScheduler, UniPCMultistepScheduler
from .tokenizer import make_bert_tokenizer, make_tokenizer


class PipelineOutput:
    def __init__(self, images, nsfw_content_detected=None):
        self.images = images
        self.nsfw_content_detected = nsfw_content_detected


_WEIGHTS = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors")
_TEXT_WEIGHTS = ("model.safetensors", "model.fp16.safetensors")


def _first_safetensors(d, names):
    """The state dict of the first of `names` that exists in the directory d."""
    for n in names:
        p = os.path.join(d, n)
        if os.path.exists(p):
            return W.load_safetensors(p)
    raise FileNotFoundError(f"no safetensors weights in {d}")


def _checkpoint_scheduler(base_dir):
    """The scheduler a ControlNet-free checkpoint directory asks for: {base}/scheduler/scheduler_config.json's `prediction_type` on top
    of the SD defaults (the SD-1.5 and SD-2.1-base repositories say "epsilon", which is the default; the 768-pixel
    stabilityai/stable-diffusion-2-1 says "v_prediction").  None without the file.  An unserved type raises here, before any weight
    is packed (scheduler.PREDICTION_TYPES)."""
    path = os.path.join(base_dir, "scheduler", "scheduler_config.json")
    if not os.path.exists(path):
        return None
    with open(path, encoding="utf-8") as f:
        cfg = json.load(f)
    return DDIMScheduler(prediction_type=cfg.get("prediction_type", "epsilon"))


def _rgb_u8(image):
    """PIL image or array -> u8 [H,W,3] array."""
    return np.asarray(image.convert("RGB") if isinstance(image, Image.Image) else image, dtype=np.uint8)


def graphs_enabled():
    """hipGraph replay of the DDIM sampling step (default on; SASPA_GRAPH=0 launches every kernel from Python).  Off while
    a launch recorder is installed (bench.py times individual launches with HIP events)."""
    return os.environ.get("SASPA_GRAPH", "1") != "0" and ops._RECORDER is None


def fork_enabled():
    """Two-branch sampling step (UNet encoder || ControlNet encoder inside the captured graph).  SASPA_FORK=0 captures
    the single-stream order."""
    return os.environ.get("SASPA_FORK", "1") != "0"


def cfg_prefix_enabled():
    """Classifier-free guidance evaluates the rows the two halves of the batch share -- conv_in, the first resnet, the first
    transformer up to its self-attention, in the UNet and in the ControlNet -- once per image (models._Net.encode(cfg_pair=True)).
    SASPA_CFG_PREFIX=0 evaluates them for both halves, as cat([x, x])."""
    return os.environ.get("SASPA_CFG_PREFIX", "1") != "0"


def replay_queue_depth():
    """Replays of the step graph the host keeps outstanding before it sleeps until the oldest has finished (see _StepGraph.run;
    0 = unthrottled)."""
    try:
        return int(os.environ.get("SASPA_REPLAY_DEPTH", "3"))
    except ValueError:
        return 3


side_stream = ops.side_stream          # one capture side stream per process and device (ops.side_stream)
_GATES = {}                            # device -> the int64 pair a twin recorder's ops.clock_probe writes (nothing reads it)


def _evaluate(unet, controlnet, x, cemb, step, cscale, cfg_pair, out, side=None):
    """ONE network evaluation, eps(x) into `out`: UNet encoder, ControlNet, UNet decoder -- the captured step (step = None: the step
    state is bound, _StepGraph._bind) and the eager loop (step = i) make the same launches with the same dispatch decisions.
    cfg_pair: the encoders take the B rows the two CFG halves share (the halves of x are equal, the update keeps them so).
    The UNet encoder and the ControlNet encoder are independent until the zero convs add the two.  The ControlNet
    encoder runs
      * on `side`, the capturing caller's second stream (fork_enabled): two branches of the captured graph.  Same kernels on the
        same inputs as on one stream; one branch's launch gaps / tile tails / small deep-level kernels are filled by the other's work;
      * under a launch recorder that wants the TIMED path's dispatch (bench.Recorder(twin=True)): on the shared side stream, between
        begin_twin / end_twin.  Both streams are held behind one sleeping wave (ops.clock_probe, ~40 ms) until the host has enqueued
        both launch sequences, so that they really run side by side;
      * on the current stream otherwise.
    The paired encoders walk the same shapes side by side, so their split-K is sized for half the chip each (ops.twin_branch) --
    except under any other launch recorder, which times every launch ALONE and therefore gets the full-chip dispatch."""
    xe = x[:x.shape[0] // 2] if cfg_pair else x
    if controlnet is None:                                 # img2img baseline, InstructPix2Pix
        mid, skips = unet.encode(xe, step, cfg_pair=cfg_pair)
        if cfg_pair:
            skips[0] = ops.dup_rows(skips[0])
        return unet.decode(mid, skips, step, out=out)
    ce = cemb[:cemb.shape[0] // 2] if cfg_pair else cemb
    rec = ops._RECORDER
    twin_rec = side is None and getattr(rec, "twin", False) and fork_enabled()
    if twin_rec:
        side = side_stream(x.device)
        if x.device not in _GATES:
            _GATES[x.device] = torch.zeros(2, dtype=torch.int64, device=x.device)
        ops.clock_probe(_GATES[x.device], 10000)
    if side is not None:
        main = torch.cuda.current_stream()
        side.wait_stream(main)
    if twin_rec:
        rec.begin_twin()
    with ops.twin_branch(twin_rec or (fork_enabled() and rec is None)):
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            cmid, cfeats = controlnet.encode(xe, step, conv_in_residual=ce, cfg_pair=cfg_pair)
        mid, skips = unet.encode(xe, step, cfg_pair=cfg_pair)
    if twin_rec:
        rec.end_twin()
    if side is not None:
        main.wait_stream(side)
    if twin_rec:
        for t in (cmid, *cfeats):
            t.record_stream(main)
    skips, mid = controlnet.zero_convs(cmid, cfeats, cscale, skips, mid, cfg_pair=cfg_pair)
    return unet.decode(mid, skips, step, out=out)


def _schedule(sch, steps, t_start=0, branches=2):
    """(timesteps of the network evaluations, plan rows | None) of a `steps`-step run.  PLMS: N + 1 evaluations, the second timestep
    twice, a dict per evaluation; UniPC: a coefficient row per evaluation; DDIM: no plan, and t_start > 0 (img2img / SDEdit) keeps
    the timesteps from that index on."""
    if branches == 3 and isinstance(sch, (PNDMScheduler, UniPCMultistepScheduler)):
        raise NotImplementedError("three guidance branches (InstructPix2Pix) run on DDIM only")
    if t_start and isinstance(sch, PNDMScheduler):
        raise NotImplementedError("img2img runs on DDIM / UniPC (the reference switches non-BLIP pipelines away from PNDM)")
    if t_start and isinstance(sch, UniPCMultistepScheduler):
        raise NotImplementedError("img2img with UniPC: the multistep history would have to start mid-schedule")
    if isinstance(sch, (PNDMScheduler, UniPCMultistepScheduler)):
        plan = sch.plan(steps)
        return [t for t, _ in plan], [r for _, r in plan]
    return list(sch.set_timesteps(steps))[t_start:], None


def _multistep_state(sch, x, nimg, static=False):
    """What a multistep update keeps between evaluations, zeroed: UniPC's last sample + two x0-predictions in one buffer; PLMS's
    4-slot history ring and, for the captured step (static), the buffer of the saved sample (the eager update clones it)."""
    def z(*lead):
        return torch.zeros(lead + (nimg,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
    if isinstance(sch, UniPCMultistepScheduler):
        return dict(state=z(3))
    if isinstance(sch, PNDMScheduler):
        return dict(hist=z(4), saved=z()) if static else dict(hist=z(4))
    return {}


def _update(sch, eps, x, mem, nimg, hw, nc, cfg, guidance, branches=2, image_guidance=1.0, row=None, table=None, index=None):
    """The scheduler update that closes an evaluation, (guided) eps -> x in place, in one of two forms: `table` + `index` (the
    captured step: the evaluation's coefficients are read on the device) or `row` (the eager loop: the plan's entry of the
    evaluation; for DDIM, which has no plan, its timestep).  branches = 3: x holds the groups (uncond | image | text)."""
    if sch.config["prediction_type"] == "v_prediction":     # DDIM / UniPC only (PNDM refuses it at construction)
        if branches == 3:
            raise NotImplementedError("three guidance branches (InstructPix2Pix) with a v-prediction scheduler")
        if isinstance(sch, UniPCMultistepScheduler):
            if cfg:
                ops.cfg_unipc_step_v(eps, x, mem["state"], nimg, hw, nc, guidance, row=row, table=table, index=index)
            else:
                ops.unipc_step_v(eps, x, mem["state"], nimg, hw, nc, row=row, table=table, index=index)
        elif table is not None:
            ops.ddim_step_v_dev(eps, x, nimg, hw, nc, guidance, table, index, cfg=cfg)
        elif cfg:
            ops.cfg_ddim_step_v(eps, x, nimg, hw, nc, guidance, *sch.step_coefficients(row))
        else:
            ops.ddim_step_v(eps, x, nimg, hw, nc, *sch.step_coefficients(row))
    elif isinstance(sch, UniPCMultistepScheduler):
        if cfg:
            ops.cfg_unipc_step(eps, x, mem["state"], nimg, hw, nc, guidance, row=row, table=table, index=index)
        else:
            ops.unipc_step(eps, x, mem["state"], nimg, hw, nc, row=row, table=table, index=index)
    elif isinstance(sch, PNDMScheduler):
        if table is not None:
            ops.cfg_plms_step_dev(eps, x, mem["hist"], mem["saved"], nimg, hw, nc, guidance, table, index)
        else:
            if row["save_sample"]:
                mem["saved"] = x[:nimg].clone()
            ops.cfg_plms_step(eps, x, mem["hist"], mem["saved"] if row["use_saved"] else None, nimg, hw, nc, guidance,
                              row["store_slot"], row["w_cur"], row["w_hist"], row["coef_sample"], row["coef_model"])
    elif table is not None:
        if branches == 3:
            ops.cfg3_ddim_step_dev(eps, x, nimg, hw, nc, guidance, image_guidance, table, index)
        else:
            ops.ddim_step_dev(eps, x, nimg, hw, nc, guidance, table, index, cfg=cfg)
    elif branches == 3:
        ops.cfg3_ddim_step(eps, x, nimg, hw, nc, guidance, image_guidance, *sch.step_coefficients(row))
    elif cfg:
        ops.cfg_ddim_step(eps, x, nimg, hw, nc, guidance, *sch.step_coefficients(row))
    else:
        ops.ddim_step(eps, x, nimg, hw, nc, *sch.step_coefficients(row))


class _StepGraph:
    """ONE captured hipGraph of a sampling step -- UNet encoder, ControlNet, UNet decoder, (CFG +) DDIM or PLMS update,
    ~1 500 kernel nodes -- replayed once per network evaluation.  Launching those kernels from Python costs 1.28 s per batch-8 / 50-step
    generation against 1.38 s of GPU time (tools/host_launch_time.py): the host was 7 % away from being the bottleneck.
    Everything a step reads lives in static buffers owned by this object; what changes from step to step is read on the
    device through a step counter (time-embedding rows: ops.gather_row; DDIM coefficients: ops.ddim_step_dev)."""

    def __init__(self, pipe, x_shape, cemb_shape, steps, cfg, guidance, cscale, cfg_pair=False, branches=2, image_guidance=1.0):
        dev, dt = pipe.device, pipe.dtype
        self.pipe, self.steps, self.cfg, self.guidance, self.cscale = pipe, steps, cfg, guidance, cscale
        # branches = 3 (InstructPix2Pix): x holds the groups (uncond | image | text) and the update is ops.cfg3_ddim_step_dev; DDIM
        # only, which _sample -- the one caller that passes 3 -- has checked
        self.branches, self.image_guidance = int(branches), image_guidance
        self.cfg_pair = bool(cfg and cfg_pair and self.branches == 2)   # the encoders' shared prefix once per image (cfg_prefix_enabled)
        self.x = torch.zeros(x_shape, device=dev, dtype=dt)
        self.eps = torch.zeros(x_shape, device=dev, dtype=dt)
        self.cemb = torch.zeros(cemb_shape, device=dev, dtype=dt)
        self.idx = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.nimg = x_shape[0] // self.branches if cfg else x_shape[0]
        self.sch = sch = pipe.scheduler
        # per-evaluation coefficient rows (PLMS: N + 1 evaluations) and the multistep history, in static buffers
        self.evals = steps + 1 if isinstance(sch, PNDMScheduler) else steps
        width = UniPCMultistepScheduler.ROW if isinstance(sch, UniPCMultistepScheduler) else 10 if isinstance(sch, PNDMScheduler) else 4
        self.coefs = torch.zeros((self.evals, width), device=dev, dtype=torch.float32)
        self.mem = _multistep_state(sch, self.x, self.nimg, static=True)
        self.nets = (pipe.unet,) if pipe.controlnet is None else (pipe.unet, pipe.controlnet)   # ControlNet-free: img2img baseline
        self.tables, self.curs, self.ctx_kv = [], [], []
        self.graph = None
        self.side = None                  # second capture stream of the forked step (fork_enabled)
        self._replay_events = []          # events of the replays still in the queue (run())

    def _bind(self):
        """Point the networks at this graph's static state."""
        for net, cur, kv in zip(self.nets, self.curs, self.ctx_kv):
            net.bind_step_state(cur)
            net.ctx_kv = kv

    def load(self, x, cemb, ctx, ts, added=None):
        """Refresh the static buffers for one generation (device-side copies; shapes are fixed by the cache key)."""
        sch = self.pipe.scheduler
        first = not self.tables
        refresh_t = first or added is not None          # without SDXL's added conditioning the time tables depend on ts only
        for i, net in enumerate(self.nets):
            net.prepare_context(ctx)
            if refresh_t:
                net.prepare_timesteps(ts, added)
            if first:
                self.tables.append(net.temb_all.clone())
                self.curs.append(torch.zeros_like(net.temb_all[0]))
                # (K, V^T, key count[, K / V^T fragments of the fused cross-attention launch]): tensors are cloned into static buffers
                self.ctx_kv.append({t: tuple(e.clone() if torch.is_tensor(e) else e for e in kv) for t, kv in net.ctx_kv.items()})
            else:
                if refresh_t:
                    self.tables[i].copy_(net.temb_all)
                for t, kv in net.ctx_kv.items():
                    for dst, src in zip(self.ctx_kv[i][t], kv):
                        if torch.is_tensor(src):
                            dst.copy_(src)
        self.x.copy_(x)
        self.cemb.copy_(cemb)
        if first:
            if isinstance(self.sch, PNDMScheduler):
                rows = [[d["store_slot"], d["w_cur"], *d["w_hist"], d["coef_sample"], d["coef_model"], float(d["save_sample"]),
                         float(d["use_saved"])] for d in self.plan]
            else:
                rows = self.plan if self.plan is not None else [sch.step_coefficients(t) for t in ts]
            self.coefs.copy_(torch.tensor(rows, dtype=torch.float32))
        self._rewind()
        self._bind()

    def _rewind(self):
        """Back to the first evaluation: the step counter and the multistep history."""
        self.idx.zero_()
        for buf in self.mem.values():
            buf.zero_()

    def _step(self):
        pipe, x = self.pipe, self.x
        for net, tab, cur in zip(self.nets, self.tables, self.curs):
            ops.gather_row(tab, self.idx, cur)
        if pipe.controlnet is not None and fork_enabled() and self.side is None:
            self.side = side_stream(x.device)
        _evaluate(pipe.unet, pipe.controlnet, x, self.cemb, None, self.cscale, self.cfg_pair, self.eps,
                  side=self.side if fork_enabled() else None)
        _update(self.sch, self.eps, x, self.mem, self.nimg, x.shape[1] * x.shape[2], pipe.cfgs["unet"]["out_channels"], self.cfg,
                self.guidance, self.branches, self.image_guidance, table=self.coefs, index=self.idx)
        ops.index_add(self.idx, 1)

    def run_on(self, x, cemb, ctx, ts, added=None, plan=None):
        self.plan = plan
        self.load(x, cemb, ctx, ts, added)
        return self.run()

    def run(self):
        """All steps: the first generation on this object runs step 0 eagerly (warms allocator / lazy state), restores
        the inputs, captures the step and replays; later generations only replay."""
        if self.graph is None:
            x0 = self.x.clone()
            self._step()                                   # eager warm-up step (also validates every launch argument)
            torch.cuda.synchronize()
            self.x.copy_(x0)
            self._rewind()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step()
            self.graph = g
        depth = replay_queue_depth()
        if depth <= 0:
            for _ in range(self.evals):
                self.graph.replay()
            return self.x
        # Host throttle (round 6): the HIP queue holds about five replays of the ~1 500-node step; once it is full, hipGraphLaunch
        # SPINS on the calling thread until a slot frees -- one host core per rank at 100 % for the whole run
        # (profiles/r6_config3_full_shard.json: 0.21 CPU-s per image in the launch thread alone; a replay itself costs the host
        # 1.4 ms, tools/graph_host_cost.py).  Keeping at most `depth` replays outstanding and SLEEPING until the oldest has finished
        # (ops.sleep_wait: event query + 1 ms naps -- hipEventSynchronize busy-waits here even with hipEventBlockingSync) leaves
        # the GPU the same backlog to chew on (3 replays = 70-100 ms) and gives the core back.  SASPA_REPLAY_DEPTH=0 = unthrottled.
        evs = self._replay_events
        for _ in range(self.evals):
            if len(evs) >= depth:
                ops.sleep_wait(evs.pop(0))
            self.graph.replay()
            e = torch.cuda.Event()
            e.record()
            evs.append(e)
        return self.x


XL_VAE_MODES = (None, "x3", "exact", "bf16", "f16")


def xl_vae_mode(value):
    """A VAE mode of the SDXL pipelines as `set_vae_mode` / SASPA_XL_VAE / run_aug.Settings.XL_VAE spell it -> one of XL_VAE_MODES
    (None, "" and "default": today's behaviour, `upcast_vae()` decides); anything else is a ValueError."""
    if value is None or value in ("", "default", "none", "None"):
        return None
    if value not in XL_VAE_MODES:
        raise ValueError(f"VAE mode must be one of {XL_VAE_MODES[1:]} (or None), got {value!r}")
    return value


def f32_mode(gemm, attn):
    """The fp32 modes as `set_f32_mode` / SASPA_F32_GEMM / SASPA_F32_ATTN spell them -> (gemm, attn); anything else is a ValueError."""
    if gemm not in ("exact", "x3"):
        raise ValueError(f"fp32 GEMM mode must be 'exact' or 'x3', got {gemm!r}")
    if attn not in ("unfused", "fused"):
        raise ValueError(f"fp32 attention mode must be 'unfused' or 'fused', got {attn!r}")
    return gemm, attn


class StableDiffusionControlNetPipeline:
    HAS_CONTROLNET = True
    CFG_PREFIX = True                 # _sample() evaluates the CFG-shared encoder prefix once per image (cfg_prefix_enabled)
    SUPPORTS_FP16 = True              # enable_fp16(): built for the SD-1.5 pipelines (the BLIP-Diffusion and SDXL subclasses refuse it)

    def __init__(self, state_dicts, cfgs=SD15, tokenizer=None, scheduler=None):
        self._state_dicts = state_dicts
        self.cfgs = cfgs
        self.scheduler = scheduler or DDIMScheduler()
        self.tokenizer = tokenizer or make_tokenizer(vocab=cfgs["text"]["vocab"], pad_id=cfgs["text"].get("pad_id"))
        self.device = None
        self.dtype = None
        self.noise_dtype = None
        self.unet = self.controlnet = self.vae = self.text_encoder = None
        self._graphs = {}                 # (shapes, steps, guidance, scale) -> _StepGraph, small LRU
        self.safety_checker = None        # built by .to() when the family ships one; assign None to disable (diffusers idiom)
        self.last_nsfw = None
        self._neg_cache = {}
        self._fp16 = False                # enable_fp16(): fp16 compute for text tower / UNet / ControlNet / scheduler steps
        self._fp16_vae = "bf16"
        self._f32_mode = None             # set_f32_mode(): (gemm, attn) of the fp32 compute dtype; None = SASPA_F32_GEMM / SASPA_F32_ATTN
        self.f32_gemm, self.f32_attn = "exact", "unfused"    # what .to() resolved: the modes the fp32 networks run in
        self.last_nonfinite = None        # SDXL VAE mode "f16": device bool [B], the decoder's output of that image was not finite

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, cfgs=SD15, seed=0):
        """Architecture-exact random weights (no checkpoint / network available)."""
        return cls(W.synth_family(cfgs, seed), cfgs)

    @classmethod
    def from_pretrained(cls, base_dir, controlnet_dir, cfgs=SD15):
        """Local diffusers-format checkpoints (the layout `from_pretrained` downloads):
        {base}/unet, {base}/vae, {base}/text_encoder, {base}/tokenizer and the ControlNet dir."""
        sds = cls._base_state_dicts(base_dir, cfgs)
        sds["controlnet"] = _first_safetensors(controlnet_dir, _WEIGHTS)
        return cls(sds, cfgs, tokenizer=make_tokenizer(os.path.join(base_dir, "tokenizer"), cfgs["text"]["vocab"]))

    @staticmethod
    def _base_state_dicts(base_dir, cfgs):
        sds = dict(unet=_first_safetensors(os.path.join(base_dir, "unet"), _WEIGHTS),
                   vae=_first_safetensors(os.path.join(base_dir, "vae"), _WEIGHTS),
                   text=_first_safetensors(os.path.join(base_dir, "text_encoder"), _TEXT_WEIGHTS))
        sc = os.path.join(base_dir, "safety_checker")
        if "safety" in cfgs and os.path.isdir(sc):
            sds["safety"] = _first_safetensors(sc, _TEXT_WEIGHTS)
        return sds

    def to(self, device, dtype=None):
        device = torch.device(device)
        if self._state_dicts is None:
            raise RuntimeError("this pipeline was already placed on a device; build a new one to change device / dtype")
        if device.type != "cuda":
            raise RuntimeError("saspa_aug_amd pipelines run on an MI355X only (no CPU path); got device %s" % device)
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible")
        fp16 = self._fp16 or os.environ.get("SASPA_FP16", "0") == "1"
        fp16_vae = self._fp16_vae if self._fp16 else os.environ.get("SASPA_FP16_VAE", "bf16")
        if dtype in (None, torch.float16, torch.bfloat16):
            cdt, ndt = torch.bfloat16, torch.float16   # noise is drawn in the reference's pipeline dtype
            if fp16:                                   # opt-in (enable_fp16 / SASPA_FP16=1): the reference's own arithmetic
                if not self.SUPPORTS_FP16:
                    raise NotImplementedError(f"fp16 compute (SASPA_FP16=1) is built for the SD-1.5 pipelines, not {type(self).__name__}")
                if fp16_vae not in ("bf16", "x3"):
                    raise ValueError(f"SASPA_FP16_VAE must be 'bf16' or 'x3', got {fp16_vae!r}")
                cdt = torch.float16
        elif dtype == torch.float32:
            cdt, ndt = torch.float32, torch.float32
            # opt-in (set_f32_mode / SASPA_F32_GEMM, SASPA_F32_ATTN): x3 GEMMs and fused x3 attention for the fp32 networks
            self.f32_gemm, self.f32_attn = self._f32_mode or f32_mode(os.environ.get("SASPA_F32_GEMM") or "exact",
                                                                      os.environ.get("SASPA_F32_ATTN") or "unfused")
        else:
            raise TypeError(f"unsupported pipeline dtype {dtype}")
        # fp16 compute keeps the VAE (its activations overflow fp16) and the safety checker out of fp16: the VAE stays bf16, or runs
        # on fp32 storage with SASPA_F32X3 GEMMs (vae="x3"); the hand-offs are explicit casts outside the captured step
        vdt = cdt if cdt != torch.float16 else (torch.float32 if fp16_vae == "x3" else torch.bfloat16)
        self._vae_dtype = vdt
        self._safety_dtype = cdt if cdt != torch.float16 else torch.bfloat16
        self.device, self.dtype, self.noise_dtype = device, cdt, ndt
        # the kernels launch on the CURRENT HIP device / torch's current stream of it: make the pipeline's device current
        # (the reference's idiom is editing DEVICE = "cuda:1"; without this tensors would live on GPU 1, launches on GPU 0)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(device)
        self.device = device
        sd, cf = self._state_dicts, self.cfgs
        fp8 = getattr(self, "_fp8", False) or os.environ.get("SASPA_FP8", "0") == "1"
        fp8_conv = fp8 and (getattr(self, "_fp8_conv", False) or os.environ.get("SASPA_FP8_CONV", "0") == "1")
        if fp8 and cdt == torch.float16:
            raise ValueError("fp8 together with fp16 compute is not supported: the fp8 projections quantise bf16 activations")
        fp8_ff = getattr(self, "_fp8_ff", "calibrated")
        if fp8_ff == "calibrated":
            fp8_ff = os.environ.get("SASPA_FP8_FF", "calibrated")
            if fp8_ff not in ("calibrated", "mx"):
                raise ValueError(f"SASPA_FP8_FF must be 'calibrated' or 'mx', got {fp8_ff!r}")
        self.unet = models.UNet(sd["unet"], cf["unet"], device, cdt, fp8=fp8, fp8_conv=fp8_conv, fp8_ff=fp8_ff)
        self.controlnet = (models.ControlNet(sd["controlnet"], cf["controlnet"], device, cdt, fp8=fp8, fp8_conv=fp8_conv, fp8_ff=fp8_ff)
                           if self.HAS_CONTROLNET else None)
        self.vae = models.VAEDecoder(sd["vae"], cf["vae"], device, vdt,
                                     f32_gemm="x3" if (cdt == torch.float16 and vdt == torch.float32) else "exact")
        self.text_encoder = models.CLIPText(sd["text"], cf["text"], device, cdt)
        self._build_extra(sd, cf, device, cdt)
        self._neg_cache = {}
        self._state_dicts = None      # the packed device copies are the weights now; free ~5.6 GB of host fp32
        return self

    def _build_extra(self, sd, cf, device, cdt):
        # StableDiffusionSafetyChecker of the SD-1.5 repo: the reference never passes safety_checker=None
        if "safety" in sd and "safety" in cf:
            self.safety_checker = models.SafetyChecker(sd["safety"], cf["safety"], device, self._safety_dtype)

    def enable_fp16(self, on=True, vae="bf16"):
        """Call BEFORE `.to()`: `.to(dev, torch.float16)` / `.to(dev)` then computes the text tower, UNet, ControlNet and the scheduler
        steps in IEEE fp16 -- the reference's own arithmetic (run_aug/run_aug.py:323) -- on the fp16 build of the kernels
        (libsaspa_hip_f16.so: f16 MFMAs, same schedules); the latents are fp16 too.  SASPA_FP16=1 (+ SASPA_FP16_VAE) does the same.
        Without it nothing changes: torch.float16 selects bf16.  The VAE and the safety checker do not run in fp16 (the SD VAE
        overflows there): vae="bf16" keeps them as they are, vae="x3" runs the VAE on fp32 storage with SASPA_F32X3 GEMMs (the form to
        use when the decoded image's parity is the point).  Not together with fp8."""
        if not self.SUPPORTS_FP16:
            raise NotImplementedError(f"enable_fp16() is built for the SD-1.5 pipelines (ControlNet, ControlNet img2img, img2img), "
                                      f"not for {type(self).__name__}")
        if self.unet is not None:
            raise RuntimeError("enable_fp16() must be called before .to(): the weights are packed in the compute dtype")
        if vae not in ("bf16", "x3"):
            raise ValueError(f"vae must be 'bf16' or 'x3', got {vae!r}")
        if on and getattr(self, "_fp8", False):
            raise ValueError("fp8 together with fp16 compute is not supported: the fp8 projections quantise bf16 activations")
        self._fp16, self._fp16_vae = bool(on), vae
        return self

    def set_f32_mode(self, gemm="exact", attn="unfused"):
        """Call BEFORE `.to()`: how `.to(dev, torch.float32)` -- the parity dtype -- runs the text tower(s), UNet, ControlNet and the
        BLIP front-end.  gemm="x3": their GEMMs / convs as three bf16 MFMAs per product (ops.f32_gemm_mode, at most 2^-17 per product);
        attn="fused": their attention with heads of at most 160 channels in one launch with x3 products and no score matrix
        (ops.f32_attn_mode, saspa_flash_attn_f32x3).  SASPA_F32_GEMM=x3 / SASPA_F32_ATTN=fused do the same.  The VAE keeps its own
        rule.  Off by default ("exact", "unfused": every launch as it was); with a 16-bit dtype the call changes nothing."""
        mode = f32_mode(gemm, attn)
        if self.unet is not None:
            raise RuntimeError("set_f32_mode() must be called before .to(): the modes are fixed when the pipeline is placed")
        self._f32_mode = mode
        return self

    def _f32_scope(self):
        """The context the fp32 networks run in: nothing unless .to(dev, torch.float32) resolved a mode other than the default."""
        if self.dtype != torch.float32 or (self.f32_gemm, self.f32_attn) == ("exact", "unfused"):
            return contextlib.nullcontext()
        stack = contextlib.ExitStack()
        stack.enter_context(ops.f32_gemm_mode(self.f32_gemm))
        stack.enter_context(ops.f32_attn_mode(self.f32_attn))
        return stack

    def enable_fp8(self, on=True, convs=False, ff="calibrated"):
        """Call BEFORE `.to()`: the LayerNorm-fed projections of the UNet / ControlNet transformer blocks (cross-attention
        query, GEGLU feed-forward) run as e4m3 W8A8 GEMMs (BASELINE.json configs[4] "fp8 MFMA"; SASPA_FP8=1 does the same).
        convs=True (SASPA_FP8_CONV=1, needs fp8 on): the ResnetBlock2D conv1 / conv2 also run as MX-fp8 (block-scaled e4m3) convs
        where models.mxfp8_conv_takes admits them (models._Net.fp8_convs lists those that ran).
        ff="mx" (SASPA_FP8_FF=mx, needs fp8 on): the feed-forward hidden state carries one exponent per row and 32 columns instead
        of the tensor-wide scale calibrated on the first batch a process runs (the default, ff="calibrated"): an image's bytes
        depend on that image alone, nothing saturates, a block can be captured without an eager run.  Same average error.
        Off by default: the headline metric is quoted in bf16."""
        if self.unet is not None:
            raise RuntimeError("enable_fp8() must be called before .to(): the weights are quantised at pack time")
        if ff not in ("calibrated", "mx"):
            raise ValueError(f"ff must be 'calibrated' or 'mx', got {ff!r}")
        if convs and not on:
            raise ValueError("fp8 convs need fp8 on: enable_fp8(True, convs=True)")
        if ff == "mx" and not on:
            raise ValueError("the MX feed-forward needs fp8 on: enable_fp8(True, ff='mx')")
        if on and self._fp16:
            raise ValueError("fp8 together with fp16 compute is not supported: the fp8 projections quantise bf16 activations")
        self._fp8 = bool(on)
        self._fp8_conv = bool(convs)
        self._fp8_ff = ff
        return self

    def upcast_vae(self, gemm=None):  # SDXL-only hook the reference calls at run_aug/run_aug.py:224
        return self

    def set_vae_mode(self, mode):
        """The 16-bit VAE modes belong to the SDXL pipelines, whose reference VAE is madebyollin/sdxl-vae-fp16-fix -- re-trained to
        stay inside fp16.  The VAE of this family is not that one (the SD-1.5 VAE overflows fp16, which is why enable_fp16() keeps it
        in bf16 or on fp32 storage): refused, whatever the mode."""
        mode = xl_vae_mode(mode)
        raise NotImplementedError(f"set_vae_mode({mode!r}): the VAE of {type(self).__name__} is not the fp16-fix one (the SD-1.5 "
                                  "VAE overflows fp16); the VAE modes exist for StableDiffusionXLControlNetPipeline, and "
                                  "enable_fp16(vae=...) chooses between bf16 and x3 here")

    def _nonfinite_guard(self, img):
        """Per-image non-finite flags of the decoder's output where a mode asks for them (SDXL, VAE mode "f16"); None otherwise."""
        return None

    def run_safety_checker(self, images_u8):
        """device u8 [B,H,W,3] -> (images with flagged ones replaced by black, device int32 flags [B] | None)."""
        if self.safety_checker is None:
            return images_u8, None
        return self.safety_checker.forward(images_u8)

    # ---- pieces ------------------------------------------------------------------------
    def _need_device(self):
        if self.unet is None:
            raise RuntimeError("pipeline not placed on a device: call .to('cuda:0', dtype) first")
        if torch.cuda.current_device() != self.device.index:       # another pipeline / caller switched devices since
            torch.cuda.set_device(self.device)

    def encode_prompts(self, ids):
        """ids: int array/tensor [n,77] -> [n,77,ctx_dim] device tensor (CLIP text tower)."""
        self._need_device()
        if not torch.is_tensor(ids):
            ids = torch.as_tensor(np.asarray(ids))
        with self._f32_scope():
            return self.text_encoder.forward(ops.h2d(ids, self.device))

    def _negative_context(self, neg_ids):
        key = np.asarray(neg_ids).tobytes()
        if key not in self._neg_cache:           # constant for a whole run -> encode once
            self._neg_cache[key] = self.encode_prompts(neg_ids)
        return self._neg_cache[key]

    def latents_to_device(self, latents):
        """[B,4,h,w] noise (any float dtype, CPU) -> channels-last [B,h,w,8] in compute dtype."""
        x = latents.to(torch.float32).permute(0, 2, 3, 1)
        x = torch.nn.functional.pad(x, (0, 8 - x.shape[-1]))
        return ops.h2d((x * self.scheduler.init_noise_sigma).contiguous(), self.device, self.dtype).contiguous()

    def _positive_context(self, prompt_ids, query_embeds=None):
        return self.encode_prompts(prompt_ids)

    @staticmethod
    def _guidance_context(neg, pos, branches=2):
        """Negative [1 | B,77,C] and positive [B,77,C] contexts -> [branches * B,77,C], unconditional groups first."""
        if neg.shape[0] == 1 and pos.shape[0] > 1:
            neg = neg.expand(pos.shape[0], -1, -1)
        if neg.shape[1] != pos.shape[1]:
            raise ValueError(f"negative context has {neg.shape[1]} tokens, positive {pos.shape[1]}")
        return torch.cat([neg] * (branches - 1) + [pos], 0).contiguous()

    def _device_u8(self, images_u8):
        """u8 [B,H,W,3], numpy or tensor -> contiguous device tensor."""
        # (np.array: a writable copy -- arrays that come out of PIL are read-only and torch warns about wrapping those)
        t = images_u8 if torch.is_tensor(images_u8) else torch.from_numpy(np.array(images_u8))
        return ops.h2d(t, self.device).contiguous()

    def _check_sides(self, images, what):
        """The UNet halves the latent (H/8 x W/8) once per level below the first and doubles it back exactly; the reference only
        ever feeds multiples of 64 (all_utils/utils.py:65-77 rounds both sides to 64)."""
        hh, ww = images.shape[1:3]
        mult = 8 << (len(self.cfgs["unet"]["block_out"]) - 1)
        if hh % mult or ww % mult:
            raise ValueError(f"{what} sides must be multiples of {mult} (got {hh}x{ww})")

    @staticmethod
    def _check_latents(latents, channels, images, what, on_device=False):
        b, hh, ww, _ = images.shape
        want = (b, hh // 8, ww // 8, 8) if on_device else (b, channels, hh // 8, ww // 8)
        if tuple(latents.shape) != want:
            raise ValueError(f"latents shape {tuple(latents.shape)} does not match the {what} image {hh}x{ww}")

    def _decode(self, x, return_latents=False):
        """Final latents [B,h,w,8] -> device u8 images [B,H,W,3] through the VAE decoder and the safety checker (flags in
        `last_nsfw`; None for a family without one); with return_latents also the latents and the decoder's output."""
        z = ops.scale(x, 1.0 / self.cfgs["vae"]["scaling_factor"])
        # (fp16 compute, SDXL's upcast_vae(): the hand-off to the bf16 / fp32 VAE; a no-op otherwise)
        img = self.vae.decode(z.to(self.vae.dtype))
        self.last_nonfinite = self._nonfinite_guard(img)
        out, self.last_nsfw = self.run_safety_checker(ops.act_to_u8(img))
        return (out, x, img) if return_latents else out

    def _sample(self, *a, **kw):
        """_sample_steps inside the pipeline's fp32 modes (set_f32_mode; nothing is entered by default or in a 16-bit dtype)."""
        with self._f32_scope():
            return self._sample_steps(*a, **kw)

    def _sample_steps(self, x2, b, hw, ctx, cemb2, steps, guidance_scale, cscale, t_start=0, branches=2, image_guidance=1.0, cfg=True,
                      added=None):
        """The denoising loop on the CFG-doubled latents x2 [2B,h,w,8] of b images (in place): the captured step replayed, or with
        SASPA_GRAPH=0 / under a launch recorder the same evaluation and update launched from Python.  t_start > 0 (img2img /
        SDEdit): only the timesteps from index t_start of the `steps`-step schedule run (DDIM only).  branches = 3
        (InstructPix2Pix): x2 is [3B,h,w,8] in the groups (uncond | image | text) and every update is ops.cfg3_ddim_step (DDIM
        only).  cfg = False (SDXL-Turbo): x2 is [B,h,w,8], no guidance.  added: SDXL's (pooled text embeddings, time ids)."""
        sch = self.scheduler
        pair = cfg and self.CFG_PREFIX and cfg_prefix_enabled() and branches == 2
        guidance_scale = guidance_scale if cfg else 0.0
        ts, plan = _schedule(sch, steps, t_start, branches)
        if graphs_enabled():
            g = self._step_graph(x2, cemb2, ctx, len(ts) if t_start else steps, cfg, guidance_scale, cscale, ts, cfg_pair=pair,
                                 branches=branches, image_guidance=image_guidance)
            x2.copy_(g.run_on(x2, cemb2, ctx, ts, added, plan=plan))
            return
        nets = [self.unet] + ([self.controlnet] if self.controlnet is not None else [])
        for net in nets:
            net.prepare_context(ctx)
        for net in nets:
            net.prepare_timesteps(ts, added)
        eps = torch.zeros_like(x2)
        mem = _multistep_state(sch, x2, b)
        for i, t in enumerate(ts):
            _evaluate(self.unet, self.controlnet, x2, cemb2, i, cscale, pair, eps)
            _update(sch, eps, x2, mem, b, hw, self.cfgs["unet"]["out_channels"], cfg, guidance_scale, branches, image_guidance,
                    row=t if plan is None else plan[i])

    def _step_graph(self, x, cemb, ctx, steps, cfg, guidance, cscale, ts, cfg_pair=False, branches=2, image_guidance=1.0):
        # the timesteps are part of the key: the cached time tables / coefficients follow the scheduler's configuration
        key = (tuple(x.shape), tuple(cemb.shape), tuple(ctx.shape), int(steps), bool(cfg), float(guidance), float(cscale), x.dtype,
               type(self.scheduler).__name__, tuple(int(t) for t in ts), bool(cfg_pair), int(branches), float(image_guidance))
        g = self._graphs.pop(key, None)
        if g is None:
            while len(self._graphs) >= 3:                   # each graph keeps one step's activations resident
                self._graphs.pop(next(iter(self._graphs)))
            g = _StepGraph(self, x.shape, cemb.shape, steps, cfg, guidance, cscale, cfg_pair, branches, image_guidance)
        self._graphs[key] = g                               # most recently used last
        return g

    @torch.no_grad()
    def generate_batch(self, prompt_ids, negative_ids, control_u8, latents, num_inference_steps,
                       guidance_scale=7.5, controlnet_conditioning_scale=0.75, return_latents=False,
                       latents_on_device=False, query_embeds=None):
        """prompt_ids [B,77], negative_ids [1,77] or [B,77], control_u8 u8 [B,H,W,3] (numpy or
        device tensor), latents [B,4,H/8,W/8] noise (or, with latents_on_device, the
        channels-last [B,H/8,W/8,8] device tensor from `latents_to_device`).
        Returns a device u8 tensor [B,H,W,3]."""
        self._need_device()
        if guidance_scale <= 1.0:
            raise NotImplementedError("guidance_scale <= 1 (no CFG) belongs to the SDXL-Turbo branch (SURVEY a9)")
        ctrl = self._device_u8(control_u8)
        b, hh, ww, _ = ctrl.shape
        self._check_sides(ctrl, "control image")
        self._check_latents(latents, self.cfgs["unet"]["in_channels"], ctrl, "control", latents_on_device)
        pos = self._positive_context(prompt_ids, query_embeds)
        ctx = self._guidance_context(self._negative_context(negative_ids), pos)
        with self._f32_scope():
            cemb = self.controlnet.cond_embedding(ops.u8_to_act(ctrl, self.dtype))
        cemb2 = torch.cat([cemb, cemb], 0)
        x = latents if latents_on_device else self.latents_to_device(latents)
        x2 = torch.cat([x, x], 0).contiguous()
        self._sample(x2, b, (hh // 8) * (ww // 8), ctx, cemb2, num_inference_steps, guidance_scale, controlnet_conditioning_scale)
        return self._decode(x2[:b], return_latents)

    # ---- the reference's call form ----------------------------------------------------
    def __call__(self, prompt=None, image=None, num_inference_steps=50, generator=None, guidance_scale=7.5,
                 negative_prompt=None, controlnet_conditioning_scale=1.0, **unused):
        self._need_device()
        if image is None or prompt is None:
            raise ValueError("`prompt` and `image` (the control image) are required")
        ctrl = _rgb_u8(image)
        if ctrl.ndim != 3 or ctrl.shape[2] != 3:
            raise ValueError("control image must be RGB")
        lat = self._noise(ctrl, generator)
        ids = self.tokenizer(str(prompt))
        neg = self.tokenizer(negative_prompt if negative_prompt is not None else "")
        return self._output(self.generate_batch(ids, neg, ctrl[None], lat, num_inference_steps, guidance_scale,
                                                controlnet_conditioning_scale))

    def _noise(self, image, generator, channels=None):
        """One [1,C,H/8,W/8] draw for an [H,W,3] image, in the reference's pipeline dtype, from its CPU generator."""
        if generator is not None and generator.device.type != "cpu":
            raise NotImplementedError("the reference passes the global CPU generator (run_aug/run_aug.py:324)")
        shape = (1, channels or self.cfgs["unet"]["in_channels"], image.shape[0] // 8, image.shape[1] // 8)
        return torch.randn(shape, generator=generator, dtype=self.noise_dtype)

    def _output(self, images):
        nsfw = None if self.last_nsfw is None else [bool(v) for v in self.last_nsfw.cpu().tolist()]
        return PipelineOutput([Image.fromarray(a) for a in images.cpu().numpy()], nsfw)


class StableDiffusionControlNetImg2ImgPipeline(StableDiffusionControlNetPipeline):
    """Drop-in for diffusers' `StableDiffusionControlNetImg2ImgPipeline` as the reference builds it with SDEDIT = 1
    (run_aug/run_aug.py:203-206) and calls it (:252-260, :274-276): `pipe(prompt, image=<source PIL>, control_image=<canny
    PIL>, strength, num_inference_steps, generator, guidance_scale, negative_prompt, controlnet_conditioning_scale)`.
    The source image is encoded by the VAE encoder (HIP launch graph), the latent is sampled from the posterior and noised
    to the first kept timestep in one kernel (`saspa_vae_sample_noise`; the two noise draws come from the CPU generator in
    the reference's order: posterior sample first, then the scheduler noise), and the last int(steps * strength) DDIM steps
    run exactly like the text-to-image loop (same captured step graph)."""

    def _build_extra(self, sd, cf, device, cdt):
        super()._build_extra(sd, cf, device, cdt)
        if "encoder.conv_in.weight" not in sd["vae"]:
            raise KeyError("the VAE checkpoint has no encoder half: img2img (SDEdit) needs vae/encoder.* and quant_conv")
        self.vae_encoder = models.VAEEncoder(sd["vae"], cf["vae"], device, self._vae_dtype)

    @staticmethod
    def kept_steps(num_inference_steps, strength):
        """get_timesteps: (index of the first kept timestep, number of kept steps)."""
        init = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init, 0)
        return t_start, num_inference_steps - t_start

    @torch.no_grad()
    def generate_batch_img2img(self, prompt_ids, negative_ids, source_u8, control_u8, sample_noise, noise, num_inference_steps,
                               strength, guidance_scale=7.5, controlnet_conditioning_scale=0.75, return_latents=False):
        """source_u8 / control_u8: u8 [B,H,W,3] (numpy or device); sample_noise / noise: [B,4,H/8,W/8] CPU draws."""
        self._need_device()
        if guidance_scale <= 1.0:
            raise NotImplementedError("guidance_scale <= 1 (no CFG) belongs to the SDXL-Turbo branch")
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        t_start, kept = self.kept_steps(num_inference_steps, strength)
        if kept < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline "
                             f"steps is {kept} which is < 1 and not appropriate for this pipeline.")
        dev, dt = self.device, self.dtype
        if (control_u8 is None) != (self.controlnet is None):
            raise ValueError("a control image is required by the ControlNet pipelines and refused by the ControlNet-free one")
        src = self._device_u8(source_u8)
        ctrl = self._device_u8(control_u8) if control_u8 is not None else src
        b, hh, ww, _ = ctrl.shape
        if tuple(src.shape) != tuple(ctrl.shape):
            raise ValueError("source and control images must have the same size")
        self._check_sides(ctrl, "image")
        moments = self._encode_image(src)
        sch = self.scheduler
        ts = list(sch.set_timesteps(num_inference_steps))
        a_t = float(sch.alphas_cumprod[int(ts[t_start])])
        x = ops.vae_sample_noise(moments, self.latents_to_device(sample_noise), self.latents_to_device(noise),
                                 self.cfgs["vae"]["scaling_factor"], a_t ** 0.5, (1.0 - a_t) ** 0.5)
        pos = self._positive_context(prompt_ids)
        ctx = self._guidance_context(self._negative_context(negative_ids), pos)
        if self.controlnet is not None:
            with self._f32_scope():
                cemb = self.controlnet.cond_embedding(ops.u8_to_act(ctrl, dt))
            cemb2 = torch.cat([cemb, cemb], 0)
        else:
            cemb2 = torch.zeros((1,), device=dev, dtype=dt)           # placeholder: nothing reads it
        x2 = torch.cat([x, x], 0).contiguous()
        self._sample(x2, b, (hh // 8) * (ww // 8), ctx, cemb2, num_inference_steps, guidance_scale,
                     controlnet_conditioning_scale, t_start=t_start)
        return self._decode(x2[:b], return_latents)

    def _encode_image(self, images_u8):
        """Device u8 [B,H,W,3] -> the VAE posterior's moments [B,H/8,W/8,8] (mean | logvar) in the compute dtype."""
        # VaeImageProcessor: [0,255] -> [-1,1], in the encoder's dtype (== the compute dtype unless fp16 compute is on)
        px = imageproc.normalize_u8(images_u8, self.vae_encoder.dtype, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        with ops.f32_gemm_mode(self.vae.f32_gemm):
            return self.vae_encoder.encode(px).to(self.dtype)

    def __call__(self, prompt=None, image=None, control_image=None, strength=0.8, num_inference_steps=50, generator=None,
                 guidance_scale=7.5, negative_prompt=None, controlnet_conditioning_scale=0.8, **unused):
        self._need_device()
        if image is None or control_image is None or prompt is None:
            raise ValueError("`prompt`, `image` (the source image) and `control_image` are required")
        src, ctrl = _rgb_u8(image), _rgb_u8(control_image)
        e1 = self._noise(ctrl, generator)                                                # latent_dist.sample(generator)
        e2 = self._noise(ctrl, generator)                                                # randn_tensor for add_noise
        ids = self.tokenizer(str(prompt))
        neg = self.tokenizer(negative_prompt if negative_prompt is not None else "")
        return self._output(self.generate_batch_img2img(ids, neg, src[None], ctrl[None], e1, e2, num_inference_steps, strength,
                                                        guidance_scale, controlnet_conditioning_scale))


class StableDiffusionImg2ImgPipeline(StableDiffusionControlNetImg2ImgPipeline):
    """Drop-in for diffusers' `StableDiffusionImg2ImgPipeline` -- the reference's CONTROLNET = None, SDEDIT = 1 branch
    (run_aug/run_aug.py:163-165; the Real-Guidance baseline, defaults in run_aug/run_aug_real_guidance.py:520-523), called
    as `pipe(prompt, image=<source PIL>, strength, num_inference_steps, generator, guidance_scale, negative_prompt)`
    (:235-241, :274-276).  Same VAE-encode / posterior sample / add-noise / last int(steps * strength) DDIM steps as the
    ControlNet img2img pipeline; every evaluation is the UNet alone (no ControlNet is built, no control image exists)."""
    HAS_CONTROLNET = False

    @classmethod
    def from_pretrained(cls, base_dir, cfgs=SD15):
        return cls(cls._base_state_dicts(base_dir, cfgs), cfgs,
                   tokenizer=make_tokenizer(os.path.join(base_dir, "tokenizer"), cfgs["text"]["vocab"], cfgs["text"].get("pad_id")),
                   scheduler=_checkpoint_scheduler(base_dir))

    def generate_batch_img2img(self, prompt_ids, negative_ids, source_u8, sample_noise, noise, num_inference_steps, strength,
                               guidance_scale=7.5, return_latents=False):
        """source_u8: u8 [B,H,W,3] (numpy or device); sample_noise / noise: [B,4,H/8,W/8] CPU draws (posterior, add_noise)."""
        return super().generate_batch_img2img(prompt_ids, negative_ids, source_u8, None, sample_noise, noise, num_inference_steps,
                                              strength, guidance_scale, 0.0, return_latents)

    def __call__(self, prompt=None, image=None, strength=0.8, num_inference_steps=50, generator=None, guidance_scale=7.5,
                 negative_prompt=None, **unused):
        self._need_device()
        if image is None or prompt is None:
            raise ValueError("`prompt` and `image` (the source image) are required")
        src = _rgb_u8(image)
        e1 = self._noise(src, generator)                                                 # latent_dist.sample(generator)
        e2 = self._noise(src, generator)                                                 # randn_tensor for add_noise
        ids = self.tokenizer(str(prompt))
        neg = self.tokenizer(negative_prompt if negative_prompt is not None else "")
        return self._output(self.generate_batch_img2img(ids, neg, src[None], e1, e2, num_inference_steps, strength, guidance_scale))


class StableDiffusionPipeline(StableDiffusionControlNetPipeline):
    """Drop-in for diffusers' `StableDiffusionPipeline` -- the reference's CONTROLNET = None, SDEDIT = 0 branch for sd_v1.5 and
    sd_v2.1 (run_aug/run_aug.py:165-169; the "no structural conditioning" row of the ablations), called as `pipe(prompt,
    num_inference_steps, generator, guidance_scale, negative_prompt)` (:235-241): text-to-image at the UNet's sample size (512 x 512
    unless height / width are given).  The ControlNet pipeline without its ControlNet: the same CPU-generator noise, negative-prompt
    cache, CFG (shared encoder prefix included) and the one-branch captured step of the ControlNet-free img2img pipeline; every
    evaluation is the UNet alone.  The safety checker is built when the family ships one (SD15) and absent otherwise (SD21)."""
    HAS_CONTROLNET = False

    @classmethod
    def from_pretrained(cls, base_dir, cfgs=SD15):
        return cls(cls._base_state_dicts(base_dir, cfgs), cfgs,
                   tokenizer=make_tokenizer(os.path.join(base_dir, "tokenizer"), cfgs["text"]["vocab"], cfgs["text"].get("pad_id")),
                   scheduler=_checkpoint_scheduler(base_dir))

    @torch.no_grad()
    def generate_batch(self, prompt_ids, negative_ids, latents, num_inference_steps, guidance_scale=7.5, return_latents=False,
                       latents_on_device=False):
        """prompt_ids [B,77], negative_ids [1,77] or [B,77], latents [B,4,h,w] noise (or, with latents_on_device, the channels-last
        [B,h,w,8] device tensor from `latents_to_device`); the images are 8h x 8w.  Returns a device u8 tensor [B,8h,8w,3]."""
        self._need_device()
        if guidance_scale <= 1.0:
            raise NotImplementedError("guidance_scale <= 1 (no CFG) belongs to the SDXL-Turbo branch (SURVEY a9)")
        nch = self.cfgs["unet"]["in_channels"]
        if latents.dim() != 4 or latents.shape[-1 if latents_on_device else 1] != (8 if latents_on_device else nch):
            raise ValueError(f"latents shape {tuple(latents.shape)}: expected [B,{nch},h,w] noise (or [B,h,w,8] on the device)")
        b, h, w = (latents.shape[0], latents.shape[1], latents.shape[2]) if latents_on_device else \
            (latents.shape[0], latents.shape[2], latents.shape[3])
        mult = 1 << (len(self.cfgs["unet"]["block_out"]) - 1)
        if h % mult or w % mult:
            raise ValueError(f"image sides must be multiples of {8 * mult} (got {8 * h}x{8 * w})")
        ctx = self._guidance_context(self._negative_context(negative_ids), self._positive_context(prompt_ids))
        x = latents if latents_on_device else self.latents_to_device(latents)
        x2 = torch.cat([x, x], 0).contiguous()
        cemb2 = torch.zeros((1,), device=self.device, dtype=self.dtype)           # placeholder: nothing reads it
        self._sample(x2, b, h * w, ctx, cemb2, num_inference_steps, guidance_scale, 0.0)
        return self._decode(x2[:b], return_latents)

    def __call__(self, prompt=None, height=None, width=None, num_inference_steps=50, generator=None, guidance_scale=7.5,
                 negative_prompt=None, **unused):
        self._need_device()
        if prompt is None:
            raise ValueError("`prompt` is required")
        side = 8 * self.cfgs["unet"].get("sample_size", 64)                       # diffusers: unet.config.sample_size * vae_scale_factor
        lat = self._noise(np.empty((height or side, width or side, 3), np.uint8), generator)
        ids = self.tokenizer(str(prompt))
        neg = self.tokenizer(negative_prompt if negative_prompt is not None else "")
        return self._output(self.generate_batch(ids, neg, lat, num_inference_steps, guidance_scale))


class StableDiffusionInstructPix2PixPipeline(StableDiffusionImg2ImgPipeline):
    """Drop-in for diffusers' `StableDiffusionInstructPix2PixPipeline` -- the reference's BASE_MODEL = "ip2p" branch
    (run_aug/run_aug.py:174-176; the editing model of the ALIA baseline), called as `pipe(prompt, image=<source PIL>,
    image_guidance_scale=1.3, num_inference_steps=100, generator, guidance_scale, negative_prompt)` (:235-241, :252-255).
    The UNet's conv_in takes 8 channels: the noisy latents and, next to them, the latents of the source image -- the MODE of the
    VAE posterior (the mean; no draw), not multiplied by the scaling factor.  One `randn` per image, as in text-to-image.  Every
    step evaluates the UNet on three groups, unconditional first like the other pipelines here:

        group 0  negative prompt   x | 0
        group 1  negative prompt   x | image latents
        group 2  prompt            x | image latents

    and e = e0 + gs (e2 - e1) + igs (e1 - e0) goes through the DDIM step (ops.cfg3_ddim_step: one launch, which also leaves the
    image-latent channels of the input as they are).  DDIM only; bf16 or fp32 (no fp16 / fp8 compute: untested on three groups)."""
    CFG_PREFIX = False                # (three groups: the pair prefix does not apply)
    SUPPORTS_FP16 = False

    def __init__(self, state_dicts, cfgs=IP2P, tokenizer=None, scheduler=None):
        super().__init__(state_dicts, cfgs, tokenizer, scheduler)

    @classmethod
    def from_synthetic(cls, cfgs=IP2P, seed=0):
        return cls(W.synth_family(cfgs, seed), cfgs)

    @classmethod
    def from_pretrained(cls, base_dir, cfgs=IP2P):
        return super().from_pretrained(base_dir, cfgs)

    def enable_fp8(self, on=True, convs=False, ff="calibrated"):
        raise NotImplementedError("enable_fp8() is not built for StableDiffusionInstructPix2PixPipeline (three guidance groups)")

    def to(self, device, dtype=None):
        if os.environ.get("SASPA_FP8", "0") == "1":
            raise NotImplementedError("fp8 (SASPA_FP8=1) is not built for StableDiffusionInstructPix2PixPipeline")
        return super().to(device, dtype)

    def generate_batch_img2img(self, *a, **k):
        raise NotImplementedError("the InstructPix2Pix UNet takes the image latents as input channels: use generate_batch_ip2p")

    @torch.no_grad()
    def generate_batch_ip2p(self, prompt_ids, negative_ids, source_u8, latents, num_inference_steps, guidance_scale=7.5,
                            image_guidance_scale=1.5, return_latents=False):
        """source_u8: u8 [B,H,W,3] (numpy or device); latents: [B,4,H/8,W/8] CPU noise, one draw per image.
        Returns a device u8 tensor [B,H,W,3]."""
        self._need_device()
        if not (guidance_scale > 1.0 and image_guidance_scale >= 1.0):
            raise NotImplementedError("guidance is on for guidance_scale > 1 and image_guidance_scale >= 1; the guidance-free "
                                      "form (one evaluation per step) is not built")
        dev, dt = self.device, self.dtype
        src = self._device_u8(source_u8)
        b, hh, ww, _ = src.shape
        self._check_sides(src, "image")
        h8, w8 = hh // 8, ww // 8
        nl = self.cfgs["vae"]["latent_channels"]
        self._check_latents(latents, nl, src, "source")
        moments = self._encode_image(src)                           # mean in channels 0..3: latent_dist.mode()
        x = self.latents_to_device(latents)
        # the UNet input of the three groups, built once: the sampling step rewrites channels < 4 only
        x3 = torch.zeros((3, b, h8, w8, 8), device=dev, dtype=dt)
        x3[..., :nl] = x[..., :nl]
        x3[1:, ..., nl:2 * nl] = moments[..., :nl]
        x3 = x3.view(3 * b, h8, w8, 8)
        pos = self._positive_context(prompt_ids)
        ctx = self._guidance_context(self._negative_context(negative_ids), pos, branches=3)     # [3B,77,C]: uncond | image | text
        cemb = torch.zeros((1,), device=dev, dtype=dt)               # placeholder: nothing reads it
        self._sample(x3, b, h8 * w8, ctx, cemb, num_inference_steps, guidance_scale, 0.0, branches=3,
                     image_guidance=image_guidance_scale)
        return self._decode(x3[:b], return_latents)                  # (group 0 carries zeros next to the latents: the VAE's layout)

    def __call__(self, prompt=None, image=None, num_inference_steps=100, generator=None, guidance_scale=7.5,
                 image_guidance_scale=1.5, negative_prompt=None, **unused):
        self._need_device()
        if image is None or prompt is None:
            raise ValueError("`prompt` and `image` (the image to edit) are required")
        src = _rgb_u8(image)
        # (the noise has the VAE's latent channels, not the UNet's 8 input channels)
        lat = self._noise(src, generator, self.cfgs["vae"]["latent_channels"])
        ids = self.tokenizer(str(prompt))
        neg = self.tokenizer(negative_prompt if negative_prompt is not None else "")
        return self._output(self.generate_batch_ip2p(ids, neg, src[None], lat, num_inference_steps, guidance_scale,
                                                     image_guidance_scale))


class BlipDiffusionControlNetPipeline(StableDiffusionControlNetPipeline):
    """Drop-in for diffusers' `BlipDiffusionControlNetPipeline` as the reference builds and calls it for every dataset
    but planes (run_aug/run_aug.py:181, :211, :243-250, :262-265, :521):

        pipe = BlipDiffusionControlNetPipeline.from_pretrained("Salesforce/blipdiffusion-controlnet").to(DEVICE, fp16)
        image = pipe(prompt=..., reference_image=<PIL same-class image>, condtioning_image=<canny PIL>,
                     source_subject_category="bird", target_subject_category="bird", height=H, width=W,
                     neg_prompt=..., num_inference_steps=..., generator=..., guidance_scale=7.5).images[0]

    Differences from the SD-1.5 pipeline, all mirrored: the PNDM / PLMS scheduler of the checkpoint is kept (N+1
    network evaluations), no ControlNet conditioning scale is passed (= 1.0), the prompt is rewritten
    "a {category} {prompt}" and repeated prompt_strength * prompt_reps (= 20) times, tokenised to 77 - 16 tokens,
    and the 16 subject tokens of the Q-Former front-end (saspa_aug_amd.blip.Blip2QFormer) are spliced into the
    CLIP token embeddings at position 2.  UNet / ControlNet / VAE are the SD-1.5 architectures (shared kernels)."""
    SUPPORTS_FP16 = False
    CFG_PREFIX = False                # (the multimodal context keeps today's evaluation)

    def __init__(self, state_dicts, cfgs=BLIP_DIFFUSION, tokenizer=None, scheduler=None, qformer_tokenizer=None):
        super().__init__(state_dicts, cfgs, tokenizer, scheduler or PNDMScheduler())
        self.qformer_tokenizer = qformer_tokenizer or make_bert_tokenizer(vocab=cfgs["qformer"]["vocab"])
        self.qformer = None

    @classmethod
    def from_synthetic(cls, cfgs=BLIP_DIFFUSION, seed=0):
        return cls(W.synth_family(cfgs, seed), cfgs)

    @classmethod
    def from_pretrained(cls, repo_dir, cfgs=BLIP_DIFFUSION):
        """Local copy of Salesforce/blipdiffusion-controlnet: unet/ vae/ text_encoder/ controlnet/ qformer/ tokenizer/."""
        names = _WEIGHTS + ("model.safetensors",)
        sds = {k: _first_safetensors(os.path.join(repo_dir, sub), names)
               for k, sub in (("unet", "unet"), ("vae", "vae"), ("text", "text_encoder"), ("controlnet", "controlnet"), ("qformer", "qformer"))}
        return cls(sds, cfgs, tokenizer=make_tokenizer(os.path.join(repo_dir, "tokenizer"), cfgs["text"]["vocab"]),
                   qformer_tokenizer=make_bert_tokenizer(os.path.join(repo_dir, "qformer"), cfgs["qformer"]["vocab"]))

    def _build_extra(self, sd, cf, device, cdt):
        from .blip import Blip2QFormer
        self.qformer = Blip2QFormer(sd["qformer"], cf["qformer"], device, cdt)      # (this pipeline has no safety checker)

    # ---- pieces ------------------------------------------------------------------------
    @staticmethod
    def build_prompt(prompt, tgt_subject, prompt_strength=1.0, prompt_reps=20):
        p = f"a {tgt_subject} {str(prompt).strip()}"
        return ", ".join([p] * int(prompt_strength * prompt_reps))

    def prompt_token_count(self):
        return self.cfgs["text"]["max_pos"] - self.cfgs["qformer"]["num_query"]

    def get_query_embeddings(self, reference_images, source_subject_categories):
        """reference images (PIL / u8 HWC) + category strings -> [B, 16, width] subject tokens (device)."""
        self._need_device()
        from .blip import preprocess_reference
        qc = self.cfgs["qformer"]
        def one(im):
            if torch.is_tensor(im) and im.is_cuda:          # device u8 [H,W,3] (run_aug): Pillow-exact bicubic on the device
                x =imageproc.resize_u8(im[None].contiguous(), qc["image_size"], qc["image_size"], filt="bicubic")
                return imageproc.normalize_u8(x, torch.float32, BLIP_IMAGE_MEAN, BLIP_IMAGE_STD)[0, :, :, :3].permute(2, 0, 1)
            return preprocess_reference(im, qc, BLIP_IMAGE_MEAN, BLIP_IMAGE_STD).to(self.device)
        px = torch.stack([one(im) for im in reference_images])
        ids = [self.qformer_tokenizer(c) for c in source_subject_categories]
        with self._f32_scope():
            if len({i.shape[1] for i in ids}) == 1:
                return self.qformer.forward(px, np.concatenate(ids))
            # categories of different token counts: no padding mask in the kernels -> one item at a time
            return torch.cat([self.qformer.forward(px[i:i + 1], ids[i]) for i in range(len(ids))], 0)

    def _positive_context(self, prompt_ids, query_embeds=None):
        if query_embeds is None:
            raise ValueError("BLIP-Diffusion needs the subject tokens (query_embeds); see get_query_embeddings")
        ids = torch.as_tensor(np.asarray(prompt_ids)) if not torch.is_tensor(prompt_ids) else prompt_ids
        if ids.shape[1] != self.prompt_token_count():
            raise ValueError(f"prompt must be tokenised to {self.prompt_token_count()} tokens (77 - subject tokens)")
        with self._f32_scope():
            return self.text_encoder.forward(ops.h2d(ids, self.device), query_embeds, self.cfgs["ctx_begin_pos"])

    # ---- the reference's call form (keyword names as diffusers spells them, typo included) ----
    def __call__(self, prompt=None, reference_image=None, condtioning_image=None, source_subject_category=None,
                 target_subject_category=None, height=512, width=512, neg_prompt="", num_inference_steps=50,
                 generator=None, guidance_scale=7.5, prompt_strength=1.0, prompt_reps=20, **unused):
        self._need_device()
        if prompt is None or reference_image is None or condtioning_image is None:
            raise ValueError("`prompt`, `reference_image` and `condtioning_image` are required")
        ctrl = condtioning_image.convert("RGB") if isinstance(condtioning_image, Image.Image) else Image.fromarray(np.asarray(condtioning_image))
        if ctrl.size != (width, height):        # prepare_control_image resizes the control image to (width, height)
            ctrl = ctrl.resize((width, height), resample=Image.LANCZOS)
        ctrl = np.asarray(ctrl, dtype=np.uint8)
        lat = self._noise(ctrl, generator)
        text = self.build_prompt(prompt, target_subject_category, prompt_strength, prompt_reps)
        ids = self.tokenizer(text, max_len=self.prompt_token_count())
        neg = self.tokenizer(neg_prompt or "")
        q = self.get_query_embeddings([reference_image], [source_subject_category])
        return self._output(self.generate_batch(ids, neg, ctrl[None], lat, num_inference_steps, guidance_scale, 1.0, query_embeds=q))


class StableDiffusionXLControlNetPipeline(StableDiffusionControlNetPipeline):
    """Drop-in for diffusers' `StableDiffusionXLControlNetPipeline` as the reference builds and calls it for
    `BASE_MODEL = "sd_xl-turbo"` (its choice for CUB; run_aug/run_aug.py:189-201, :223-228, :564-571):

        vae  = AutoencoderKL.from_pretrained("madebyollin/sdxl-vae-fp16-fix")
        pipe = StableDiffusionXLControlNetPipeline.from_pretrained("stabilityai/sdxl-turbo", controlnet=<canny-sdxl>, vae=vae)
        pipe.scheduler = DDIMScheduler.from_config(pipe.scheduler.config); pipe.upcast_vae()
        image = pipe(prompt=..., image=<canny PIL>, num_inference_steps=2, generator=..., guidance_scale=0,
                     negative_prompt=None, controlnet_conditioning_scale=0.75).images[0]

    Differences from the SD-1.5 pipeline, all mirrored: guidance_scale <= 1 -> NO classifier-free guidance (one
    conditional evaluation per step, the negative prompt is never encoded); two text towers read at
    hidden_states[-2] and concatenated to a 2048-wide context, the second tower's projected EOS state is the pooled
    embedding of the `text_time` conditioning together with add_time_ids = (H, W, 0, 0, H, W); three-level UNet /
    ControlNet with transformer depths (2, 10) and linear projections; VAE scaling factor 0.13025, decoded in fp32
    after `upcast_vae()` (the exact-fp32 MFMA kernels) even when the denoiser runs in bf16."""
    SUPPORTS_FP16 = False
    CFG_PREFIX = False                # (with guidance the added conditioning differs between the halves)

    def __init__(self, state_dicts, cfgs=SDXL_TURBO, tokenizer=None, scheduler=None, tokenizer_2=None):
        super().__init__(state_dicts, cfgs, tokenizer, scheduler or DDIMScheduler(**SDXL_TURBO_SCHEDULER_CONFIG))
        self.tokenizer_2 = tokenizer_2 or make_tokenizer(vocab=cfgs["text2"]["vocab"])
        self.text_encoder_2 = None
        self._vae_fp32 = False
        self._vae_gemm = None
        self._vae_sd = None
        self._vae_mode = None             # set_vae_mode(); when it was never called, `.to()` takes SASPA_XL_VAE
        self._vae_mode_set = False

    def set_vae_mode(self, mode):
        """How the VAE decodes, whatever `upcast_vae()` says.  Before or after `.to()` (after: the decoder is re-packed from the
        retained VAE state dict).  Never called: the environment's SASPA_XL_VAE, read by `.to()`.
        None     today's behaviour: the pipeline's dtype until `upcast_vae()`, then fp32 storage with SASPA_F32X3 GEMMs (or exact
                 fp32 with gemm="exact" / SASPA_VAE_EXACT_FP32=1).
        "x3" / "exact"   fp32 storage with that GEMM form, with or without `upcast_vae()`.
        "bf16"   a bf16 VAE; `upcast_vae()` is a no-op.
        "f16"    an IEEE fp16 VAE on the fp16 build of the kernels, whatever the denoiser's dtype -- what the reference loads
                 (madebyollin/sdxl-vae-fp16-fix in torch.float16, run_aug/run_aug.py:189).  The mid-block attention runs as the fused
                 wide-head launch (ops.attn_wide).  `upcast_vae()` is a no-op.  fp16 stores do not clamp, so the decoder's output is
                 checked per image with torch.isfinite before quantisation: `last_nonfinite` (device bool [B]); run_aug fails
                 such an item.  That the real checkpoint stays finite through this decoder is NOT verified (it is not available
                 offline; parity of the fp16 VAE is shown on synthetic weights only) -- hence the guard.
        The latents are cast at the hand-off in `_decode`; the denoiser and the text towers are untouched."""
        self._vae_mode, self._vae_mode_set = xl_vae_mode(mode), True
        if self.vae is not None:
            self._apply_vae_mode()
        return self

    def _apply_vae_mode(self):
        m = self._vae_mode
        if m in ("x3", "exact") or (m is None and self._vae_fp32):
            dt, gemm = torch.float32, (m or self._vae_gemm or ("exact" if os.environ.get("SASPA_VAE_EXACT_FP32", "0") == "1" else "x3"))
        elif m is None:
            dt, gemm = self._vae_dtype, "exact"
        else:
            dt, gemm = (torch.float16 if m == "f16" else torch.bfloat16), "exact"
        if self.vae.dtype != dt or self.vae.f32_gemm != (gemm if dt == torch.float32 else "exact"):
            self.vae = models.VAEDecoder(self._vae_sd, self.cfgs["vae"], self.device, dt, f32_gemm=gemm)

    def _nonfinite_guard(self, img):
        if self._vae_mode != "f16":
            return None
        return ~torch.isfinite(img[..., :3]).flatten(1).all(1)

    @classmethod
    def from_synthetic(cls, cfgs=SDXL_TURBO, seed=0):
        return cls(W.synth_family(cfgs, seed), cfgs)

    @classmethod
    def from_pretrained(cls, base_dir, controlnet_dir, vae_dir=None, cfgs=SDXL_TURBO):
        """Local copies of stabilityai/sdxl-turbo (unet/ text_encoder/ text_encoder_2/ tokenizer/ tokenizer_2/ vae/),
        diffusers/controlnet-canny-sdxl-1.0 and (optionally) madebyollin/sdxl-vae-fp16-fix."""
        def f(d):
            return _first_safetensors(d, _WEIGHTS + _TEXT_WEIGHTS)
        sds = dict(unet=f(os.path.join(base_dir, "unet")), vae=f(vae_dir or os.path.join(base_dir, "vae")),
                   text=f(os.path.join(base_dir, "text_encoder")), text2=f(os.path.join(base_dir, "text_encoder_2")),
                   controlnet=f(controlnet_dir))
        return cls(sds, cfgs, tokenizer=make_tokenizer(os.path.join(base_dir, "tokenizer"), cfgs["text"]["vocab"]),
                   tokenizer_2=make_tokenizer(os.path.join(base_dir, "tokenizer_2"), cfgs["text2"]["vocab"]))

    def to(self, device, dtype=None):
        self._vae_sd = None if self._state_dicts is None else self._state_dicts["vae"]
        if not self._vae_mode_set:
            self._vae_mode = xl_vae_mode(os.environ.get("SASPA_XL_VAE"))
        super().to(device, dtype)
        if self._vae_mode is not None:
            self._apply_vae_mode()
        elif self._vae_fp32:
            self.upcast_vae(self._vae_gemm)
        return self

    def _build_extra(self, sd, cf, device, cdt):
        self.text_encoder_2 = models.CLIPText(sd["text2"], cf["text2"], device, cdt)

    def upcast_vae(self, gemm=None):
        """run_aug/run_aug.py:224: the VAE decodes in float32.  Before `.to()` it is recorded; after, the decoder is
        re-packed for fp32 storage from the retained VAE state dict.  The reference upcasts because fp16 overflows in this
        VAE, not for the last mantissa bits: the decoder's GEMMs default to `SASPA_F32X3` (three bf16 MFMAs per product,
        ~1e-5 relative, well inside the 1e-3 per-pixel bar, several times the fp32 MFMA rate); `gemm="exact"` or
        SASPA_VAE_EXACT_FP32=1 selects the exact fp32 MFMA path.  GroupNorm / softmax / residuals are fp32 either way."""
        if self._vae_mode in ("bf16", "f16"):        # set_vae_mode / SASPA_XL_VAE: the 16-bit VAE stays
            return self
        self._vae_fp32 = True
        if gemm is None and self._vae_mode in ("x3", "exact"):
            gemm = self._vae_mode
        if gemm is None:
            gemm = "exact" if os.environ.get("SASPA_VAE_EXACT_FP32", "0") == "1" else "x3"
        self._vae_gemm = gemm
        if self.vae is not None and (self.vae.dtype != torch.float32 or self.vae.f32_gemm != gemm):
            self.vae = models.VAEDecoder(self._vae_sd, self.cfgs["vae"], self.device, torch.float32, f32_gemm=gemm)
        return self

    # ---- pieces ------------------------------------------------------------------------
    def pad_ids_2(self, ids):
        """tokenizer_2 pads with id 0 ("!") after the first EOS instead of repeating EOS."""
        ids = np.array(ids, np.int64, copy=True)
        eos = ids.max(axis=1, keepdims=True)
        first = (ids == eos).argmax(axis=1)
        for r in range(ids.shape[0]):
            ids[r, first[r] + 1:] = self.cfgs["text2"].get("pad_id", 0)
        return ids

    def encode_prompts_xl(self, ids1, ids2):
        """-> (context [B,77,ctx1+ctx2], pooled [B, proj] fp32)."""
        self._need_device()
        t = lambda a: ops.h2d(a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a)), self.device)   # noqa: E731
        with self._f32_scope():
            h1, _ = self.text_encoder.forward(t(ids1), penultimate=True)
            h2, pooled = self.text_encoder_2.forward(t(ids2), penultimate=True)
        return torch.cat([h1, h2], -1).contiguous(), pooled.float()

    @torch.no_grad()
    def generate_batch(self, prompt_ids, negative_ids, control_u8, latents, num_inference_steps, guidance_scale=0.0,
                       controlnet_conditioning_scale=0.75, return_latents=False, latents_on_device=False,
                       prompt_ids_2=None, negative_ids_2=None, **unused):
        """Same contract as the SD-1.5 form.  guidance_scale <= 1 (the reference's sd_xl-turbo operating point,
        run_aug/run_aug.py:568): no CFG, `negative_ids` ignored.  guidance_scale > 1: classifier-free guidance with the
        negative prompt (None -> zero embeddings).  `prompt_ids_2` / `negative_ids_2` default to the tokenizer_2 padding
        of the first tokenizer's ids."""
        self._need_device()
        cfg = guidance_scale > 1.0                         # diffusers: do_classifier_free_guidance = guidance_scale > 1
        ctrl = self._device_u8(control_u8)
        b, hh, ww, _ = ctrl.shape
        self._check_sides(ctrl, "control image")
        self._check_latents(latents, self.cfgs["unet"]["in_channels"], ctrl, "control", latents_on_device)

        def start():
            x = latents if latents_on_device else self.latents_to_device(latents)
            # (the loop runs in place: not on the caller's tensor; with guidance the doubling below copies)
            return x.clone(memory_format=torch.contiguous_format) if latents_on_device and not cfg else x
        return self._denoise_decode(prompt_ids, negative_ids, ctrl, start, num_inference_steps, guidance_scale,
                                    controlnet_conditioning_scale, return_latents, prompt_ids_2, negative_ids_2)

    def _denoise_decode(self, prompt_ids, negative_ids, ctrl, start, num_inference_steps, guidance_scale, controlnet_conditioning_scale,
                        return_latents, prompt_ids_2, negative_ids_2, t_start=0):
        """Text towers, added conditioning, control embedding, `start()` -> the initial latents [B,h,w,8], the steps from index
        t_start of the schedule, decode: what the text-to-image and the img2img form share."""
        cfg = guidance_scale > 1.0
        b, hh, ww, _ = ctrl.shape
        ids1 = np.asarray(prompt_ids.cpu() if torch.is_tensor(prompt_ids) else prompt_ids)
        ids2 = self.pad_ids_2(ids1) if prompt_ids_2 is None else prompt_ids_2
        ctx, pooled = self.encode_prompts_xl(ids1, ids2)
        if cfg:
            # BASELINE configs[4] family (guidance on): uncond first.  negative_prompt None -> ZERO embeddings (sdxl-turbo's
            # model_index.json has force_zeros_for_empty_prompt = true), otherwise both towers encode the negative prompt
            if negative_ids is None:
                nctx, npooled = torch.zeros_like(ctx), torch.zeros_like(pooled)
            else:
                n1 = np.asarray(negative_ids.cpu() if torch.is_tensor(negative_ids) else negative_ids)
                n2 = self.pad_ids_2(n1) if negative_ids_2 is None else negative_ids_2
                nctx, npooled = self.encode_prompts_xl(n1, n2)
            ctx = self._guidance_context(nctx, ctx)
            pooled = torch.cat([npooled.expand(b, -1), pooled], 0).contiguous()
        time_ids = [[hh, ww, 0, 0, hh, ww]] * ctx.shape[0]       # original_size + crops_coords_top_left + target_size
        with self._f32_scope():
            cemb = self.controlnet.cond_embedding(ops.u8_to_act(ctrl, self.dtype))
        x = start()
        if cfg:
            x = torch.cat([x, x], 0).contiguous()
            cemb = torch.cat([cemb, cemb], 0)
        # (DDIM, or UniPC: run_aug/run_aug.py:223-226 with sampler = "unipcmultistep")
        self._sample(x, b, (hh // 8) * (ww // 8), ctx, cemb, num_inference_steps, guidance_scale, controlnet_conditioning_scale,
                     t_start=t_start, cfg=cfg, added=(pooled, time_ids))
        return self._decode(x[:b], return_latents)

    def __call__(self, prompt=None, image=None, num_inference_steps=50, generator=None, guidance_scale=5.0,
                 negative_prompt=None, controlnet_conditioning_scale=1.0, **unused):
        self._need_device()
        if image is None or prompt is None:
            raise ValueError("`prompt` and `image` (the control image) are required")
        ctrl = _rgb_u8(image)
        if ctrl.ndim != 3 or ctrl.shape[2] != 3:
            raise ValueError("control image must be RGB")
        lat = self._noise(ctrl, generator)
        ids1 = self.tokenizer(str(prompt))
        ids2 = self.pad_ids_2(self.tokenizer_2(str(prompt)))
        n1 = n2 = None
        if negative_prompt is not None and guidance_scale > 1.0:
            n1 = self.tokenizer(str(negative_prompt))
            n2 = self.pad_ids_2(self.tokenizer_2(str(negative_prompt)))
        return self._output(self.generate_batch(ids1, n1, ctrl[None], lat, num_inference_steps, guidance_scale,
                                                controlnet_conditioning_scale, prompt_ids_2=ids2, negative_ids_2=n2))


def img2img_steps(num_inference_steps, strength):
    """diffusers' get_timesteps for img2img (SDEdit), on the host: (index of the first kept timestep, number of kept steps).
    init_timestep = min(int(steps * strength), steps), t_start = max(steps - init_timestep, 0); nothing left to run is a ValueError
    (RECALLED, as the class below marks it)."""
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
    t_start, kept = StableDiffusionControlNetImg2ImgPipeline.kept_steps(num_inference_steps, strength)
    if kept < 1:
        raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline "
                         f"steps is {kept} which is < 1 and not appropriate for this pipeline.")
    return t_start, kept


class StableDiffusionXLControlNetImg2ImgPipeline(StableDiffusionXLControlNetPipeline):
    """Drop-in for diffusers' `StableDiffusionXLControlNetImg2ImgPipeline` as the reference builds it for `BASE_MODEL =
    "sd_xl-turbo"`, `CONTROLNET = "canny"`, `SDEDIT = 1` (run_aug/run_aug.py:188-193) and calls it (:257-260, :274-276):
    `pipe(prompt, image=<source PIL>, control_image=<canny PIL>, strength, num_inference_steps, generator, guidance_scale,
    negative_prompt, controlnet_conditioning_scale)`.  The text-to-image XL form with the SD-1.5 img2img form's start: the source
    image goes through the VAE encoder, the latent is sampled from the posterior, scaled and noised to the first kept timestep in one
    kernel (`saspa_vae_sample_noise`), and the kept DDIM steps, the decode and the guards are the parent's.

    diffusers is not installed where this was written, so what is mirrored from it is RECALLED, not verified against its source:
    - RECALLED: get_timesteps -- init_timestep = min(int(steps * strength), steps), t_start = max(steps - init_timestep, 0); zero
      remaining steps raise ValueError (here before anything is encoded or launched: img2img_steps);
    - RECALLED: prepare_latents -- vae.encode(image).latent_dist.sample(generator) * 0.13025, then scheduler.add_noise at the first
      kept timestep with a second draw from the same generator (posterior sample first, then the step noise);
    - RECALLED: add_time_ids = (H, W, 0, 0, H, W) from the control image's size; sdxl-turbo's UNet has no aesthetic-score
      conditioning (requires_aesthetics_score = false), so none is appended;
    - RECALLED: the scheduler is DDIMScheduler.from_config(pipe.scheduler.config), timestep_spacing "trailing" (the reference,
      run_aug/run_aug.py:223);
    - RECALLED: guidance_scale <= 1 -> no classifier-free guidance, as in the text-to-image form.

    The encoder follows the pipeline's VAE mode (set_vae_mode / SASPA_XL_VAE / upcast_vae): it is packed from the retained VAE state
    dict in the decoder's dtype and fp32 GEMM form and re-packed whenever those change.  In "f16" mode the non-finite guard also
    covers the encoder's moments: such an item is flagged in `last_nonfinite` exactly as a non-finite decode is.  The fused fp32
    mid-block attention (ops.attn_wide_x3) is opt-in here as everywhere: SASPA_VAE_ATTN_F32=fused."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.vae_encoder = None
        self._enc_nonfinite = None

    def _sync_encoder(self):
        if self._vae_sd is None or "encoder.conv_in.weight" not in self._vae_sd:
            raise KeyError("the VAE checkpoint has no encoder half: img2img (SDEdit) needs vae/encoder.* and quant_conv")
        v, e = self.vae, self.vae_encoder
        if e is None or (e.dtype, e.f32_gemm) != (v.dtype, v.f32_gemm):
            self.vae_encoder = models.VAEEncoder(self._vae_sd, self.cfgs["vae"], self.device, v.dtype, f32_gemm=v.f32_gemm)

    def to(self, device, dtype=None):
        super().to(device, dtype)
        self._sync_encoder()
        return self

    def _apply_vae_mode(self):
        super()._apply_vae_mode()
        self._sync_encoder()

    def upcast_vae(self, gemm=None):
        super().upcast_vae(gemm)
        if self.vae is not None:
            self._sync_encoder()
        return self

    def _encode_image(self, images_u8):
        """Device u8 [B,H,W,3] -> the VAE posterior's moments [B,H/8,W/8,8] (mean | logvar) in the compute dtype."""
        enc = self.vae_encoder
        # VaeImageProcessor: [0,255] -> [-1,1] in the encoder's dtype; the fp16 VAE takes the fp32 pixels rounded once (the
        # normalising kernel lives in the default library, which has no fp16 stores)
        f16 = enc.dtype == torch.float16
        px = imageproc.normalize_u8(images_u8, torch.float32 if f16 else enc.dtype, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        moments = enc.encode(px.to(enc.dtype))
        # VAE mode "f16": fp16 stores do not clamp -- the guard of the decoder's output, on all eight moment channels
        self._enc_nonfinite = ~torch.isfinite(moments).flatten(1).all(1) if self._vae_mode == "f16" else None
        return moments.to(self.dtype)

    @torch.no_grad()
    def generate_batch_img2img(self, prompt_ids, negative_ids, source_u8, control_u8, sample_noise, noise, num_inference_steps,
                               strength, guidance_scale=0.0, controlnet_conditioning_scale=0.75, return_latents=False,
                               prompt_ids_2=None, negative_ids_2=None):
        """The contract of StableDiffusionControlNetImg2ImgPipeline.generate_batch_img2img plus the second tokenizer's ids:
        source_u8 / control_u8 u8 [B,H,W,3] (numpy or device); sample_noise / noise [B,4,H/8,W/8] CPU draws (posterior sample first,
        then the step noise).  guidance_scale <= 1: no CFG, `negative_ids` ignored, as in generate_batch."""
        self._need_device()
        t_start, _ = img2img_steps(num_inference_steps, strength)          # raises before anything is encoded or launched
        if control_u8 is None:
            raise ValueError("a control image is required by the ControlNet pipelines")
        src, ctrl = self._device_u8(source_u8), self._device_u8(control_u8)
        if tuple(src.shape) != tuple(ctrl.shape):
            raise ValueError("source and control images must have the same size")
        self._check_sides(ctrl, "image")
        for what, t in (("sample_noise", sample_noise), ("noise", noise)):
            self._check_latents(t, self.cfgs["unet"]["in_channels"], ctrl, what)

        def start():
            sch = self.scheduler
            a_t = float(sch.alphas_cumprod[int(list(sch.set_timesteps(num_inference_steps))[t_start])])
            return ops.vae_sample_noise(self._encode_image(src), self.latents_to_device(sample_noise), self.latents_to_device(noise),
                                        self.cfgs["vae"]["scaling_factor"], a_t ** 0.5, (1.0 - a_t) ** 0.5)
        out = self._denoise_decode(prompt_ids, negative_ids, ctrl, start, num_inference_steps, guidance_scale,
                                   controlnet_conditioning_scale, return_latents, prompt_ids_2, negative_ids_2, t_start=t_start)
        if self._enc_nonfinite is not None:              # "f16" mode: an item whose moments were not finite fails as a decode does
            self.last_nonfinite = self._enc_nonfinite if self.last_nonfinite is None else (self.last_nonfinite | self._enc_nonfinite)
        return out

    def __call__(self, prompt=None, image=None, control_image=None, strength=0.8, num_inference_steps=50, generator=None,
                 guidance_scale=5.0, negative_prompt=None, controlnet_conditioning_scale=0.8, **unused):
        self._need_device()
        if image is None or control_image is None or prompt is None:
            raise ValueError("`prompt`, `image` (the source image) and `control_image` are required")
        img2img_steps(num_inference_steps, strength)
        src, ctrl = _rgb_u8(image), _rgb_u8(control_image)
        e1 = self._noise(ctrl, generator)                                                # latent_dist.sample(generator)
        e2 = self._noise(ctrl, generator)                                                # randn_tensor for add_noise
        ids1 = self.tokenizer(str(prompt))
        ids2 = self.pad_ids_2(self.tokenizer_2(str(prompt)))
        n1 = n2 = None
        if negative_prompt is not None and guidance_scale > 1.0:
            n1 = self.tokenizer(str(negative_prompt))
            n2 = self.pad_ids_2(self.tokenizer_2(str(negative_prompt)))
        return self._output(self.generate_batch_img2img(ids1, n1, src[None], ctrl[None], e1, e2, num_inference_steps, strength,
                                                        guidance_scale, controlnet_conditioning_scale, prompt_ids_2=ids2,
                                                        negative_ids_2=n2))
