"""The LPIPS (AlexNet) filter at batch B (default 32), full width, 256 x 256, synthetic weights: the time of each of the five
saspa_lpips_layer launches (the level kernel + its finishing launch) with the bytes the level needs from HBM over that time, the
AlexNet tower, the pre-processing, and the whole LPIPS decision per image -- next to the semantic (CLIP-RN50) filter's per-image
time from the same run.  Device events around `iters` back-to-back calls after a warm-up, median of `rounds`.  Nothing here is
gated: the file reports what was seen.
usage: python tools/lpips_bench.py [--batch B] [--rounds R] [--iters N] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import _lib, filters, ops  # noqa: E402
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402
from saspa_aug_amd.synthetic import synthetic_image  # noqa: E402
from saspa_aug_amd.tokenizer import HashTokenizer  # noqa: E402


def timed(fn, iters, rounds):
    """median over rounds of (device time of `iters` back-to-back calls) / iters, in microseconds"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs the MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    n, m = args.batch, max(1, args.batch // 2)             # two augmentations per original (NUM_PER_IMAGE = 2)
    model = filters.LpipsAlex(W.synth_state_dict("lpips_alex", CFG.LPIPS_ALEX, 13), CFG.LPIPS_ALEX, dev)
    aug = torch.from_numpy(np.stack([synthetic_image(512, 512, 100 + k) for k in range(n)])).to(dev)
    ref = torch.from_numpy(np.stack([synthetic_image(512, 512, k) for k in range(m)])).to(dev)
    idx = [k // 2 % m for k in range(n)]
    idx_d = torch.tensor(idx, dtype=torch.int32, device=dev)
    lines = [f"LPIPS (AlexNet) filter, batch {n} augmentations / {m} originals, 512x512 u8 -> grey -> 256x256, fp32 (exact MFMA path), "
             f"synthetic weights; median [min .. max] of {args.rounds} rounds x {args.iters} calls, device events", ""]
    apx, rpx = model.preprocess(aug), model.preprocess(ref)
    fa, fr = model.features(apx), model.features(rpx)
    dist = torch.empty(n, device=dev)
    ws = torch.empty(n * _lib.LPIPS_MAX_BLOCKS, device=dev)
    lines.append(f"{'saspa_lpips_layer':<22}{'hw':>6}{'C':>5}{'MB read':>9}{'us':>9}{'min':>8}{'max':>8}{'GB/s':>9}")
    total_layers = 0.0
    for i, (a, r) in enumerate(zip(fa, fr)):
        hw, c = a.shape[1] * a.shape[2], a.shape[3]
        # every augmentation's rows once + its original's rows once per pair (an original shared by two pairs may hit in L2)
        nbytes = 2 * n * hw * c * 4
        us, lo, hi = timed(lambda: ops.lpips_layer(a, r, idx_d, model.lin[i], dist, accumulate=i > 0, workspace=ws), args.iters, args.rounds)
        total_layers += us
        lines.append(f"{'level ' + str(i):<22}{hw:>6}{c:>5}{nbytes / 1e6:>9.2f}{us:>9.1f}{lo:>8.1f}{hi:>8.1f}{nbytes / us / 1e3:>9.1f}")
    lines.append(f"{'five levels':<22}{'':>20}{total_layers:>9.1f}")
    lines.append("")
    pre, *_ = timed(lambda: (model.preprocess(aug), model.preprocess(ref)), args.iters, args.rounds)
    tower, *_ = timed(lambda: (model.features(apx), model.features(rpx)), args.iters, args.rounds)
    whole, wlo, whi = timed(lambda: model.forward(aug, ref, idx), args.iters, args.rounds)
    lines.append(f"pre-processing (luma, bicubic resize, normalise; {n} + {m} images)   {pre:9.1f} us")
    lines.append(f"AlexNet tower ({n} + {m} images, 5 convs + 2 max-pools each)          {tower:9.1f} us")
    lines.append(f"whole distance, u8 batch -> fp32 [n] (incl. the index upload)       {whole:9.1f} us  [{wlo:.1f} .. {whi:.1f}]")
    lines.append(f"LPIPS decision per augmented image                                  {whole / n:9.1f} us")
    tok = HashTokenizer(CFG.CLIP_RN50["vocab"], pad_id=0)
    sem = filters.SemanticFilter(W.synth_state_dict("clip_rn50", CFG.CLIP_RN50, 11), CFG.CLIP_RN50, dev, "a photo of an airplane", tok)
    s_us, slo, shi = timed(lambda: sem.logits(aug), max(2, args.iters // 4), args.rounds)
    lines.append(f"semantic filter (CLIP-RN50 logits) per augmented image, same run    {s_us / n:9.1f} us  [{slo / n:.1f} .. {shi / n:.1f}]")
    lines.append("")
    share = total_layers / whole * 100.0
    lines.append(f"the five level launches are {share:.1f} % of the LPIPS distance; the rest is the tower and the pre-processing.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
