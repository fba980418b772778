"""Timings behind the SDXL-Turbo img2img (SDEdit) form and the fused fp32 VAE attention; writes profiles/xl_img2img_bench.txt.
  (a) ops.attn_wide_x3 alone against the unfused fp32 path (models.attention_core: scores GEMM -> row softmax -> PV GEMM, plus the
      transposed value projection's output as an input) under both fp32 GEMM forms: d = 512, n = 4096 and 16384, batch 1 and 8; time and
      peak device memory above the operands.  The unfused path runs one image per launch sequence where the n x n fp32 score matrices of
      the batch pass the kernels' 2 GiB operand limit, as VAEDecoder.decode does.
  (b) the full-width XL VAE (fp32 storage, x3 GEMMs), encode and decode, SASPA_VAE_ATTN_F32 off and on, 512 x 512 and 1024 x 1024,
      batch 8.
  (c) StableDiffusionXLControlNetImg2ImgPipeline at 512 x 512 / 2 steps and 1024 x 1024 / 4 steps, strength 0.5, beside the
      text-to-image form (the same object's generate_batch) from the same process; bf16 denoiser, the default (x3) VAE.
Every figure is the median of ROUNDS timed rounds that alternate the arms (one warm-up round first), host clock around a device
synchronise; all rounds are printed so the spread can be read.  usage: python tools/xl_img2img_bench.py [--sections a,b,c] [--out FILE]"""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import config as CFG, models, ops
from saspa_aug_amd import weights as W

ROUNDS = 3
dev = torch.device('cuda:0')
arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default   # noqa: E731
sections = arg("--sections", "a,b,c").split(",")
out_path = arg("--out", os.path.join(ROOT, "profiles", "xl_img2img_bench.txt"))
lines = []


def emit(rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def timed(fn, per):
    torch.cuda.synchronize()
    t = time.time()
    for _ in range(per):
        fn()
    torch.cuda.synchronize()
    return (time.time() - t) / per


def alternate(arms, per):
    """{name: fn} -> {name: [seconds per call, one per round]}, the arms alternating round by round; round 0 is the warm-up."""
    rec = {k: [] for k in arms}
    for rnd in range(ROUNDS + 1):
        for k, fn in arms.items():
            t = timed(fn, 1 if not rnd else per)
            if rnd:
                rec[k].append(t)
    return rec


def peak_above(fn):
    """Peak device memory of one call above what is allocated before it, MiB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


med = lambda v: sorted(v)[len(v) // 2]     # noqa: E731
r4 = lambda v: [round(x, 5) for x in v]    # noqa: E731

if "a" in sections:
    d = 512
    for n in (4096, 16384):
        for b in (1, 8):
            g = torch.Generator(device=dev).manual_seed(n + b)
            qkv = torch.randn(b, n, 3 * d, device=dev, generator=g)
            q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
            vt = v.transpose(1, 2).contiguous()
            out = torch.empty(b, n, d, device=dev)
            chunk = max(1, ((1 << 31) - 1) // (n * n * 4))          # images whose score matrices fit one operand

            def unfused(mode):
                def run():
                    with ops.f32_gemm_mode(mode):
                        for i in range(0, b, chunk):
                            models.attention_core(q[i:i + chunk], k[i:i + chunk], vt[i:i + chunk], 1, n, n)
                return run
            arms = {"fused x3": lambda: ops.attn_wide_x3(q, k, v, out, n, n, d ** -0.5), "unfused x3 GEMMs": unfused("x3"),
                    "unfused exact GEMMs": unfused("exact")}
            rec = alternate(arms, 3 if n == 4096 else 1)
            mem = {name: peak_above(fn) for name, fn in arms.items()}
            with ops.f32_gemm_mode("exact"):
                want = models.attention_core(q[:1], k[:1], vt[:1], 1, n, n)
            err = ((out[:1] - want).abs().max() / want.abs().max()).item()
            for name in arms:
                emit({"section": "a", "what": "one 512-wide head, fp32 storage", "arm": name, "batch": b, "n": n, "d": d,
                      "ms": round(1e3 * med(rec[name]), 3), "rounds_ms": r4([1e3 * t for t in rec[name]]), "peak_mib_above_operands": mem[name],
                      "fused_vs_unfused_exact_max_rel": round(err, 8)})
            del qkv, vt, out, want

if "b" in sections:
    cfg = CFG.SDXL_TURBO["vae"]
    sd = W.synth_state_dict("vae", cfg, 4)
    sd.update(W.synth_state_dict("vae_enc", cfg, 104))
    nets = {}
    for knob in ("unfused", "fused"):
        nets[knob] = (models.VAEEncoder(sd, cfg, dev, torch.float32, f32_gemm="x3", attn_f32=knob),
                      models.VAEDecoder(sd, cfg, dev, torch.float32, f32_gemm="x3", attn_f32=knob))
    b = 8
    for res in (512, 1024):
        x = torch.rand(b, res, res, 8, device=dev) * 2 - 1
        x[..., 3:] = 0
        z = torch.randn(b, res // 8, res // 8, 8, device=dev)
        z[..., 4:] = 0
        for what, idx, inp in (("encode", 0, x), ("decode", 1, z)):
            arms = {knob: (lambda net=nets[knob][idx], t=inp: net.encode(t) if what == "encode" else net.decode(t)) for knob in nets}
            rec = alternate(arms, 2)
            mem = {knob: peak_above(fn) for knob, fn in arms.items()}
            a, c = arms["unfused"](), arms["fused"]()
            err = ((a - c).abs().max() / a.abs().max()).item()
            for knob in nets:
                emit({"section": "b", "what": f"SDXL VAE {what}, fp32 storage, x3 GEMMs, synthetic weights", "SASPA_VAE_ATTN_F32": knob, "batch": b,
                      "res": res, "s": round(med(rec[knob]), 4), "rounds_s": r4(rec[knob]), "peak_mib_above_inputs": mem[knob],
                      "fused_vs_unfused_max_rel": round(err, 8), "finite": bool(torch.isfinite(c).all())})
            del a, c
        del x, z
    del nets, sd
    torch.cuda.empty_cache()

if "c" in sections:
    from saspa_aug_amd.pipeline import StableDiffusionXLControlNetImg2ImgPipeline, img2img_steps
    from saspa_aug_amd.synthetic import synthetic_image, synthetic_prompt_ids
    t0 = time.time()
    pipe = StableDiffusionXLControlNetImg2ImgPipeline.from_synthetic(CFG.SDXL_TURBO, 0).upcast_vae().to(dev, torch.bfloat16)
    print(f"built in {time.time() - t0:.0f} s", flush=True)
    b, strength = 8, 0.5
    ids = synthetic_prompt_ids(b)
    for res, steps in ((512, 2), (1024, 4)):
        imgs = torch.from_numpy(np.stack([synthetic_image(res, res, i) for i in range(b)])).to(dev)
        g = torch.manual_seed(1)
        e1, e2 = (torch.randn((b, 4, res // 8, res // 8), generator=g, dtype=torch.float16) for _ in range(2))
        arms = {"img2img": lambda: pipe.generate_batch_img2img(ids, None, imgs, ops.canny(imgs, 120, 200), e1, e2, steps, strength, 0.0, 0.75),
                "text-to-image": lambda: pipe.generate_batch(ids, None, ops.canny(imgs, 120, 200), e1, steps, 0.0, 0.75)}
        rec = alternate(arms, 2)
        out = arms["img2img"]()
        for name in arms:
            emit({"section": "c", "workload": f"SDXL-Turbo + Canny ControlNet, batch={b} {res}x{res}, {steps} DDIM steps, no CFG, ctrl-scale 0.75",
                  "form": name, "strength": strength if name == "img2img" else None,
                  "steps_run": img2img_steps(steps, strength)[1] if name == "img2img" else steps, "s_per_batch": round(med(rec[name]), 4),
                  "images_per_s": round(b / med(rec[name]), 3), "rounds_s_per_batch": r4(rec[name]), "vae": f"fp32 storage, {pipe.vae.f32_gemm} GEMMs",
                  "vae_attn_f32_fused": pipe.vae.attn_f32_fused, "finite": bool(out.float().isfinite().all()),
                  "deterministic": bool(torch.equal(out, arms["img2img"]())) if name == "img2img" else None, "dtype": "bf16", "data": "synthetic"})

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("tools/xl_img2img_bench.py on one MI355X: one JSON line per arm; medians of %d alternating rounds, every round listed.\n" % ROUNDS)
    f.write("\n".join(lines) + "\n")
