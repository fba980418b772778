"""The opt-in MX-fp8 resnet conv against the bf16 production path, per shape: GroupNorm(+SiLU) + bf16 ops.conv (the library's own
dispatch: tile family, split-K) against saspa_groupnorm_quant_mxfp8 + saspa_conv3x3_mxfp8, alternating in one process (CUDA
events, median of rounds).  Shapes: the ResnetBlock2D conv1 / conv2 of SDXL at 1024^2 and 512^2 and of SD-1.5 at 512^2, with the
batch of the timed runs (rows = batch x latent pixels).  The last column is models.mxfp8_conv_takes (the routing rule).
usage: python tools/mxfp8_conv_bench.py [--batch B] [--rounds R] [--json OUT]"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import models, ops  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402

# (latent side, C in, C out) of the distinct resnet 3x3 convs per level (down, mid, up; conv1 and conv2)
SDXL = [(1, 320, 320), (2, 320, 640), (2, 640, 640), (4, 640, 1280), (4, 1280, 1280), (4, 2560, 1280), (4, 1920, 1280),
        (2, 1920, 640), (2, 1280, 640), (2, 960, 640), (1, 960, 320), (1, 640, 320)]
SD15 = [(1, 320, 320), (2, 320, 640), (2, 640, 640), (4, 640, 1280), (4, 1280, 1280), (8, 1280, 1280), (8, 2560, 1280),
        (4, 2560, 1280), (4, 1920, 1280), (2, 1920, 640), (2, 1280, 640), (2, 960, 640), (1, 960, 320), (1, 640, 320)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for model, res, shapes in (("sdxl", 1024, SDXL), ("sdxl", 512, SDXL), ("sd15", 512, SD15)):
        for div, c, n in shapes:
            side = res // 8 // div
            b = args.batch
            g = torch.Generator().manual_seed(c + n)
            x = torch.randn(b, side, side, c, generator=g).bfloat16().to(dev)
            gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(dev)
            beta = (0.1 * torch.randn(c, generator=g)).to(dev)
            wt = torch.randn(n, c, 3, 3, generator=g) / math.sqrt(9 * c)
            wb = W.pack_conv(wt).to(dev, torch.bfloat16)
            w8, sw = (t.to(dev) for t in W.pack_conv_mxfp8(wt))
            bias = torch.zeros(n, device=dev)

            def bf16():
                h = ops.groupnorm(x, gamma, beta, 32, 1e-5, ops.ACT_SILU)
                return ops.conv(h, wb, bias, kh=3, kw=3, pad=1)

            def mx():
                q, qs = ops.groupnorm_quant_mxfp8(x, gamma, beta, 32, 1e-5, ops.ACT_SILU)
                return ops.conv3x3_mxfp8(q, qs, w8, sw, bias)
            m = b * side * side
            iters = max(3, min(50, int(2e11 / (2 * m * n * 9 * c) * 20)))
            bf16(), mx()
            torch.cuda.synchronize()
            tb, tm = [], []
            for _ in range(args.rounds):
                tb.append(timed(bf16, iters))
                tm.append(timed(mx, iters))
            tb, tm = sorted(tb)[len(tb) // 2], sorted(tm)[len(tm) // 2]
            fl = 2.0 * m * n * 9 * c
            row = dict(model=model, res=res, batch=b, hw=f"{side}x{side}", C=c, N=n, M=m, bf16_us=round(tb, 1), mx_us=round(tm, 1),
                       bf16_tflops=round(fl / tb / 1e6, 1), mx_tflops=round(fl / tm / 1e6, 1), speedup=round(tb / tm, 3),
                       routed=models.mxfp8_conv_takes(m, n, c))
            rows.append(row)
            print(f"{model:5s} {res:5d} {row['hw']:>8s} {c:5d}->{n:5d}  gn+bf16 {tb:8.1f} us {row['bf16_tflops']:6.1f} TF/s   "
                  f"quant+mx {tm:8.1f} us {row['mx_tflops']:6.1f} TF/s   x{row['speedup']:.2f}  routed={row['routed']}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
