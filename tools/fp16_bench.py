"""bf16 against the opt-in fp16 compute mode on the flagship shape, in ONE process: batch 8, 512 x 512, 50 DDIM steps of the SD-1.5 +
ControlNet sampling loop with hipGraph replay (pipeline._sample: the 50 replays of the captured step, nothing else -- the VAE and
the text tower are the same code in both modes).  Per mode: warm-up runs (capture included), then `--runs` timed loops, alternating
bf16 / fp16 so that both see the same thermal state; reported: the median loop time, per-step time, and the shader clock the box
granted during the timed loops (bench.ClockSampler: one sleeping wave on a side stream).
usage: python tools/fp16_bench.py [--batch 8] [--size 512] [--steps 50] [--runs 5] [--out profiles/fp16_bench.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import saspa_aug_amd  # noqa: E402,F401
from bench import ClockSampler  # noqa: E402
from saspa_aug_amd import _lib, ops  # noqa: E402
from saspa_aug_amd.config import SD15  # noqa: E402
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, h8 = args.batch, args.size // 8
    g = torch.Generator().manual_seed(0)
    ctx32 = torch.randn(2 * b, 77, SD15["unet"]["ctx_dim"], generator=g)
    lat32 = torch.randn(b, h8, h8, 8, generator=g)
    lat32[..., 4:] = 0
    ctrl = (torch.rand(b, args.size, args.size, 3, generator=g) > 0.9).to(torch.uint8) * 255
    state = {}
    for mode in ("bf16", "fp16"):
        pipe = StableDiffusionControlNetPipeline.from_synthetic(SD15, seed=0)
        if mode == "fp16":
            pipe.enable_fp16()
        pipe.to(dev, torch.float16)
        dt = pipe.dtype
        assert dt is (torch.float16 if mode == "fp16" else torch.bfloat16)
        cemb = pipe.controlnet.cond_embedding(ops.u8_to_act(ctrl.to(dev), dt))
        state[mode] = dict(pipe=pipe, ctx=ctx32.to(dev, dt), cemb2=torch.cat([cemb, cemb], 0), x=lat32.to(dev, dt), times=[])

    def loop(mode):
        s = state[mode]
        x2 = torch.cat([s["x"], s["x"]], 0).contiguous()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s["pipe"]._sample(x2, b, h8 * h8, s["ctx"], s["cemb2"], args.steps, 7.5, 0.75)
        e.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(x2).all()), f"{mode}: non-finite latents"
        return a.elapsed_time(e)

    for _ in range(args.warmup):
        for mode in state:
            loop(mode)
    clocks = {}
    for mode in state:                        # the clock is sampled per mode, over that mode's timed loops only
        clocks[mode] = []
    for _ in range(args.runs):
        for mode in state:
            cs = ClockSampler(dev, period=0.05).start()
            state[mode]["times"].append(loop(mode))
            c = cs.stop()
            if c:
                clocks[mode].append(c["sclk_mhz_median"])
    lines = [f"tools/fp16_bench.py: SD-1.5 + ControlNet sampling loop, batch {b}, {args.size}x{args.size}, {args.steps} DDIM steps, hipGraph replay, "
             f"{args.runs} timed loops per mode (alternating) after {args.warmup} warm-up loops; {torch.cuda.get_device_name(0)}",
             f"fp16 library loaded: {_lib.f16_loaded()}"]
    med = {}
    for mode, s in state.items():
        t = sorted(s["times"])
        med[mode] = t[len(t) // 2]
        ck = sorted(clocks[mode])
        lines.append(f"{mode}: median {med[mode]:9.2f} ms per loop ({med[mode] / args.steps:7.3f} ms per step, {b * 1e3 / med[mode]:6.2f} img/s of sampling); "
                     f"loops {' '.join(f'{v:.1f}' for v in s['times'])}; shader clock median {ck[len(ck) // 2] if ck else float('nan'):.0f} MHz")
    lines.append(f"fp16 / bf16 loop time: {med['fp16'] / med['bf16']:.4f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
