"""The fp32 parity mode's two switches (ops.f32_gemm_mode, ops.f32_attn_mode / pipe.set_f32_mode) measured in ONE process:
1. models.attention_core in fp32, fused (saspa_flash_attn_f32x3) against unfused (scores GEMM -> row softmax -> PV GEMM), on the
   level-0 self-attention shape of configs[0] (CFG batch 16, 8 heads of 40, 4096 tokens) and its 77-key cross-attention shape;
2. one fp32 evaluation of the full-width SD-1.5 UNet + ControlNet at 64 x 64 latents, batch 2, in the four mode combinations;
3. with --parity: the full-width pipeline at 128 x 128, 10 DDIM steps, under (exact, unfused) and (x3, fused) against the CPU oracle
   (the case of tests/test_models_gpu.py::test_pipeline_fp32_parity_sd15_config1; about a minute of CPU).
Per variant: warm-up, then `--rounds` timed rounds ALTERNATING between the variants (all see the same thermal state), the median,
the peak allocation above what was resident before the call, and the shader clock granted during that variant's timed rounds
(bench.ClockSampler).  ("exact", "unfused") is the path every fp32 pipeline took before the switch existed: same code, same launches.
usage: python tools/f32_mode_bench.py [--batch 16] [--rounds 5] [--parity] [--out profiles/f32_mode_bench.txt]"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import saspa_aug_amd  # noqa: E402,F401
from bench import ClockSampler  # noqa: E402
from saspa_aug_amd import models, ops  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402
from saspa_aug_amd.config import SD15  # noqa: E402
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline, _evaluate  # noqa: E402

MIB = float(1 << 20)


@contextlib.contextmanager
def modes(gemm, attn):
    with ops.f32_gemm_mode(gemm), ops.f32_attn_mode(attn):
        yield


def measure(variants, rounds, warmup, dev):
    """variants: {name: callable}.  -> {name: (median ms, [ms], peak MiB above the resident set, median shader clock MHz)}"""
    peak, times, clocks = {}, {n: [] for n in variants}, {n: [] for n in variants}
    for name, fn in variants.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / MIB
    for _ in range(rounds):
        for name, fn in variants.items():
            cs = ClockSampler(dev, period=0.02).start()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            c = cs.stop()
            times[name].append(a.elapsed_time(e))
            if c:
                clocks[name].append(c["sclk_mhz_median"])
    out = {}
    for name in variants:
        t, ck = sorted(times[name]), sorted(clocks[name])
        out[name] = (t[len(t) // 2], times[name], peak[name], ck[len(ck) // 2] if ck else float("nan"))
    return out


def fmt(name, r):
    return (f"  {name:18s} median {r[0]:9.3f} ms  peak +{r[2]:9.1f} MiB  shader clock {r[3]:5.0f} MHz  rounds "
            + " ".join(f"{v:.3f}" for v in r[1]))


def attention_shapes(args, dev, lines):
    heads, d = 8, 40
    c = heads * d
    g = torch.Generator(device=dev).manual_seed(0)
    for what, nq, nk in (("level-0 self-attention", 4096, 4096), ("level-0 cross-attention", 4096, 77)):
        b = args.batch
        q = torch.randn(b, nq, c, device=dev, generator=g)
        k = torch.randn(b, nk, c, device=dev, generator=g)
        vt = torch.zeros(b, c, ops.round8(nk), device=dev)
        vt[:, :, :nk] = torch.randn(b, c, nk, device=dev, generator=g)

        def run(attn):
            with ops.f32_attn_mode(attn):
                return models.attention_core(q, k, vt, heads, nq, nk)
        diff = (run("fused") - run("unfused")).abs().max().item()
        r = measure({"unfused": lambda: run("unfused"), "fused": lambda: run("fused")}, args.rounds, 2, dev)
        flops = 4.0 * b * heads * nq * nk * d
        lines.append(f"{what}: B {b}, {heads} heads of {d}, nq {nq}, nk {nk}, fp32; scores {b * heads * nq * ops.round8(nk) * 4 / MIB:.0f} MiB; "
                     f"max |fused - unfused| {diff:.2e}")
        for name in r:
            lines.append(fmt(name, r[name]) + f"  ({flops / r[name][0] / 1e9:.1f} TFLOP/s of products)")
        lines.append(f"  fused / unfused time {r['fused'][0] / r['unfused'][0]:.4f}")
        del q, k, vt
        torch.cuda.empty_cache()


def evaluation(args, dev, lines):
    b, h = 2, 64
    unet = models.UNet(W.synth_state_dict("unet", SD15["unet"], 0), SD15["unet"], dev, torch.float32)
    cn = models.ControlNet(W.synth_state_dict("controlnet", SD15["controlnet"], 1), SD15["controlnet"], dev, torch.float32)
    g = torch.Generator().manual_seed(11)
    ctx = torch.randn(b, 77, SD15["unet"]["ctx_dim"], generator=g).to(dev)
    x = torch.zeros(b, h, h, 8, device=dev)
    x[..., :4] = torch.randn(b, h, h, 4, generator=g).to(dev)
    cond = (torch.rand(b, 8 * h, 8 * h, 3, generator=g) > 0.9).to(torch.uint8) * 255
    ts = [801, 601]
    for net in (unet, cn):
        net.prepare_context(ctx)
        net.prepare_timesteps(ts)
    cemb = cn.cond_embedding(ops.u8_to_act(cond.to(dev), torch.float32))
    eps = torch.zeros_like(x)

    def run(gemm, attn):
        with modes(gemm, attn):
            return _evaluate(unet, cn, x, cemb, 0, 0.75, False, eps)
    combos = [("exact", "unfused"), ("exact", "fused"), ("x3", "unfused"), ("x3", "fused")]
    ref = run(*combos[0]).clone()
    rel = {cmb: ((run(*cmb) - ref).abs().max() / ref.abs().max()).item() for cmb in combos}
    r = measure({f"{gm}, {at}": (lambda gm=gm, at=at: run(gm, at)) for gm, at in combos}, args.rounds, 1, dev)
    lines.append(f"one fp32 evaluation, full-width SD-1.5 UNet + ControlNet, {h} x {h} latents, batch {b} (eager launches, one stream):")
    for (gm, at), name in zip(combos, r):
        lines.append(fmt(name, r[name]) + f"  max-rel difference to (exact, unfused) {rel[(gm, at)]:.2e}")
    base = r["exact, unfused"][0]
    lines.append("  time against (exact, unfused): " + "  ".join(f"({n}) {r[n][0] / base:.4f}" for n in r))


def parity(dev, lines):
    from oracle import pipeline as OP
    from oracle.canny import generate_canny_array
    from saspa_aug_amd.synthetic import synthetic_image
    cfgs, hh, steps = SD15, 128, 10
    fam = W.synth_family(cfgs, seed=0)
    ids = torch.from_numpy(np.random.RandomState(1).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    neg = torch.from_numpy(np.random.RandomState(2).randint(0, cfgs["text"]["vocab"] - 2, (1, 77)))
    ctrl = generate_canny_array(synthetic_image(hh, hh, 10), 120, 200)
    lat = torch.randn((1, 4, hh // 8, hh // 8), generator=torch.manual_seed(1), dtype=torch.float32)
    ref_u8, _, ref_img = OP.sd_controlnet_pipeline(fam, cfgs, ids, neg, ctrl, lat, steps, return_latents=True)
    for mode in (("exact", "unfused"), ("x3", "fused")):
        pipe = StableDiffusionControlNetPipeline(dict(fam), cfgs).set_f32_mode(*mode).to(dev, torch.float32)
        out, _, img = pipe.generate_batch(ids.numpy(), neg.numpy(), ctrl[None], lat, steps, return_latents=True)
        got = img.float().cpu()[..., :3].permute(0, 3, 1, 2)
        d01 = ((got / 2 + 0.5).clamp(0, 1) - (ref_img / 2 + 0.5).clamp(0, 1)).abs().max().item()
        du8 = int(np.abs(out.cpu().numpy().astype(int) - ref_u8.astype(int)).max())
        lines.append(f"parity, full-width SD-1.5 + ControlNet, 1 image {hh} x {hh}, {steps} DDIM steps, {mode}: max |d| {d01:.3e} "
                     f"(bar 1e-3: {'met' if d01 < 1e-3 else 'MISSED'}), u8 {du8}")
        del pipe
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"tools/f32_mode_bench.py: {torch.cuda.get_device_name(0)}; {args.rounds} timed rounds per variant, alternating; medians"]
    attention_shapes(args, dev, lines)
    evaluation(args, dev, lines)
    if args.parity:
        parity(dev, lines)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
