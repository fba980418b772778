"""The feed-forward pair of an fp8 transformer block (GEGLU projection c -> 8c with the hidden state emitted as e4m3, output projection
4c -> c + residual), calibrated tensor scale (enable_fp8's default) against the calibration-free MX form (enable_fp8(ff="mx")):
  calibrated  saspa_gemm_fp8(GEGLU, out_fp8 under ONE calibrated scale) -> saspa_gemm_fp8(sa_broadcast)
  mx          saspa_gemm_fp8_geglu_mx (one E8M0 exponent per row and 32 columns) -> saspa_gemm_mxfp8 (exponents inside the MFMA)
alternating in one process (CUDA events, median of rounds; the min .. max of the calibrated arm's rounds is its run-to-run spread).
Shapes: the SDXL transformer levels (level 1: c = 640 at 1/2 latent side, level 2: c = 1280 at 1/4) at 1024^2 and 512^2.
usage: python tools/mxfp8_ff_bench.py [--batch B] [--rounds R] [--json OUT]"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import ops  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402

LEVELS = [(1, 2, 640), (2, 4, 1280)]          # (level, latent-side divisor, width)


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for res in (1024, 512):
        for level, div, c in LEVELS:
            side = res // 8 // div
            m = args.batch * side * side
            g = torch.Generator().manual_seed(c + res)
            h = torch.randn(m, c, generator=g).bfloat16().to(dev)
            gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
            w1, b1 = W.pack_geglu_tile(torch.randn(8 * c, c, generator=g) / math.sqrt(c), 0.1 * torch.randn(8 * c, generator=g), 128)
            w1q, sw1 = (t.to(dev) for t in W.quantize_fp8(w1))
            b1 = b1.float().to(dev)
            w2q, sw2 = (t.to(dev) for t in W.quantize_fp8(torch.randn(c, 4 * c, generator=g) / math.sqrt(4 * c)))
            b2 = torch.zeros(c, device=dev)
            q8, s8 = ops.layernorm_quant_fp8(h, gamma, beta)
            amax = torch.zeros(1, device=dev)
            ops.linear_fp8(q8, s8, w1q, sw1, b1, act=ops.ACT_GEGLU, amax=amax)
            scale = ops.fp8_pow2_scale(amax)

            def calibrated():
                ff8 = ops.linear_fp8(q8, s8, w1q, sw1, b1, act=ops.ACT_GEGLU, out_fp8_scale=scale)
                return ops.linear_fp8(ff8, scale, w2q, sw2, b2, residual=h)

            def mx():
                ff8, ffs = ops.linear_fp8(q8, s8, w1q, sw1, b1, act=ops.ACT_GEGLU, out_mx=True)
                return ops.linear_mxfp8(ff8, ffs, w2q, sw2, b2, residual=h)
            fl = 2.0 * m * c * (8 * c + 4 * c)
            iters = max(5, min(100, int(4e12 / fl)))
            oc, om = calibrated().float(), mx().float()
            torch.cuda.synchronize()
            rel = ((oc - om).pow(2).mean().sqrt() / oc.pow(2).mean().sqrt()).item()
            tc, tm = [], []
            for _ in range(args.rounds):
                tc.append(timed(calibrated, iters))
                tm.append(timed(mx, iters))
            tc, tm = sorted(tc), sorted(tm)
            mc, mm = tc[len(tc) // 2], tm[len(tm) // 2]
            row = dict(res=res, level=level, batch=args.batch, M=m, C=c, calibrated_us=round(mc, 1), calibrated_min_us=round(tc[0], 1),
                       calibrated_max_us=round(tc[-1], 1), mx_us=round(mm, 1), mx_min_us=round(tm[0], 1), mx_max_us=round(tm[-1], 1),
                       calibrated_tflops=round(fl / mc / 1e6, 1), mx_tflops=round(fl / mm / 1e6, 1), mx_over_calibrated=round(mm / mc, 4),
                       rms_rel_difference_of_the_outputs=float(f"{rel:.3e}"))
            rows.append(row)
            print(f"sdxl {res:5d} level {level} M={m:6d} c={c:5d}  calibrated {mc:8.1f} us [{tc[0]:.1f} .. {tc[-1]:.1f}] {row['calibrated_tflops']:6.1f} TF/s   "
                  f"mx {mm:8.1f} us [{tm[0]:.1f} .. {tm[-1]:.1f}] {row['mx_tflops']:6.1f} TF/s   mx / calibrated {mm / mc:.3f}   "
                  f"outputs differ by {rel:.2e} rms-rel", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
