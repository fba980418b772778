"""InstructPix2Pix (BASE_MODEL = "ip2p") at production width next to the UNet-only img2img pipeline of the same build, in ONE process:
batch 8, 512 x 512, 100 DDIM steps (the reference's count for ip2p, run_aug/run_aug.py:254), bf16, hipGraph replay, synthetic weights,
no safety checker.  Both are whole generations -- VAE encode, text tower, sampling loop, VAE decode, u8 -- and differ in what a step
evaluates: three UNet samples per image and the three-branch update (ip2p) against two and the CFG update (img2img at strength 1.0, so
that it runs the same 100 steps).  Per pipeline: warm-up generations (capture included), then `--runs` timed ones, alternating.
usage: python tools/ip2p_bench.py [--batch 8] [--size 512] [--steps 100] [--runs 3] [--out profiles/ip2p_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd.pipeline import StableDiffusionImg2ImgPipeline, StableDiffusionInstructPix2PixPipeline  # noqa: E402
from saspa_aug_amd.synthetic import negative_prompt_ids, synthetic_image, synthetic_prompt_ids  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, h8 = args.batch, args.size // 8
    imgs = torch.from_numpy(np.stack([synthetic_image(args.size, args.size, i) for i in range(b)])).to(dev)
    ids, neg = synthetic_prompt_ids(b), negative_prompt_ids()
    g = torch.manual_seed(1)
    e1, e2 = (torch.randn((b, 4, h8, h8), generator=g, dtype=torch.float16) for _ in range(2))
    ip2p_cfgs = {k: v for k, v in CFG.IP2P.items() if k != "safety"}
    sd_cfgs = {k: v for k, v in CFG.SD15.items() if k not in ("safety", "controlnet")}
    ip2p = StableDiffusionInstructPix2PixPipeline.from_synthetic(ip2p_cfgs, 0).to(dev, torch.bfloat16)
    i2i = StableDiffusionImg2ImgPipeline.from_synthetic(sd_cfgs, 0).to(dev, torch.bfloat16)
    runs = {"ip2p (3 UNet samples per image and step)": lambda: ip2p.generate_batch_ip2p(ids, neg, imgs, e1, args.steps, 7.5, 1.3),
            "img2img, UNet only (2 samples)": lambda: i2i.generate_batch_img2img(ids, neg, imgs, e1, e2, args.steps, 1.0, 7.5)}
    times = {k: [] for k in runs}

    def once(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = runs[name]()
        torch.cuda.synchronize()
        assert out.shape == (b, args.size, args.size, 3) and out.float().std().item() > 0
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        for name in runs:
            once(name)
    for _ in range(args.runs):
        for name in runs:
            times[name].append(once(name))
    lines = [f"tools/ip2p_bench.py: whole generations, batch {b}, {args.size}x{args.size}, {args.steps} DDIM steps, bf16, hipGraph replay, synthetic "
             f"weights, no safety checker; {args.runs} timed generations per pipeline (alternating) after {args.warmup} warm-up; "
             f"{torch.cuda.get_device_name(0)}"]
    med = {}
    for name, t in times.items():
        med[name] = sorted(t)[len(t) // 2]
        lines.append(f"{name}: median {med[name]:7.3f} s per batch = {b / med[name]:6.3f} images/s ({1e3 * med[name] / args.steps:7.2f} ms per step); "
                     f"generations {' '.join(f'{v:.3f}' for v in t)}")
    a, c = list(med.values())
    lines.append(f"ip2p / img2img time per batch: {a / c:.3f} (3 / 2 = 1.5 UNet samples per step)")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
