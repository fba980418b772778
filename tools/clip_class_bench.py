"""The per-class CLIP filter (Real-Guidance baseline) at batch B (default 32), full-width CLIP RN50, C (default 196) class prompts,
512 x 512 u8 inputs, synthetic weights: microseconds per augmented image for the per-class filter (pre-processing, image tower,
label upload, saspa_class_head), for the semantic filter in the same run, for both on one shared image tower, and the
saspa_class_head launch alone (embedding mode [B, 1024] x [C, 1024], and logits mode [B, C]).  Clock: HIP device events around
`iters` back-to-back calls after a warm-up of the same call; median [min .. max] of `rounds`.  Nothing here is gated: the file
reports what was seen.
usage: python tools/clip_class_bench.py [--batch B] [--classes C] [--rounds R] [--iters N] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import filters, ops  # noqa: E402
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402
from saspa_aug_amd.synthetic import synthetic_image  # noqa: E402
from saspa_aug_amd.tokenizer import HashTokenizer  # noqa: E402


def timed(fn, iters, rounds):
    """median, min, max over rounds of (device time of `iters` back-to-back calls) / iters, in microseconds"""
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
    ap.add_argument("--classes", type=int, default=196)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_class_bench needs the MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    n, c, cfg = args.batch, args.classes, CFG.CLIP_RN50
    sd = W.synth_state_dict("clip_rn50", cfg, 11)
    tok = HashTokenizer(cfg["vocab"], pad_id=0)
    cls = filters.ClassFilter(sd, cfg, dev, [f"model {k} sedan {2000 + k % 13}" for k in range(c)], filters.CLASS_PROMPT_TEMPLATES["cars"], tok)
    sem = filters.SemanticFilter(sd, cfg, dev, "a photo of a car", tok, visual=cls.visual)
    aug = torch.from_numpy(np.stack([synthetic_image(512, 512, 100 + k) for k in range(n)])).to(dev)
    labels = [k % c for k in range(n)]
    labels_d = torch.tensor(labels, dtype=torch.int32, device=dev)
    emb = cls.embed(aug)
    lg = torch.randn(n, (c + 7) // 8 * 8, device=dev)
    lines = [f"per-class CLIP filter, batch {n}, {c} class prompts, CLIP RN50 full width (embed_dim {cfg['embed_dim']}), 512x512 u8 -> 224x224, "
             f"fp32 (exact MFMA path), synthetic weights; HIP device events, median [min .. max] of {args.rounds} rounds x N calls", ""]

    def row(what, t, per_image=True, iters=args.iters):
        us, lo, hi = timed(t, iters, args.rounds)
        k = n if per_image else 1
        lines.append(f"{what:<86}{us / k:9.1f} us  [{lo / k:.1f} .. {hi / k:.1f}]")
        return us
    p_us = row("per-class filter per augmented image (pre-process, tower, labels h2d, class_head)", lambda: cls.probs(aug, labels))
    s_us = row("semantic filter (CLIP-RN50 logits) per augmented image, same run", lambda: sem.logits(aug))
    both = row("both on one shared image tower, per augmented image", lambda: (lambda e: (cls.probs(aug, labels, e), sem.logits(aug, e)))(cls.embed(aug)))
    lines.append("")
    h_us = row(f"saspa_class_head alone, embedding mode [{n}, {cfg['embed_dim']}] x [{c}, {cfg['embed_dim']}] (whole launch)",
               lambda: ops.class_head(emb, labels_d, cls.text_unit, cls.scale, True, width=cfg["embed_dim"]), False, 200)
    row(f"saspa_class_head alone, logits mode [{n}, {c}] (whole launch)", lambda: ops.class_head(lg, labels_d, width=c), False, 200)
    lines.append("")
    lines.append(f"the class head is {h_us / p_us * 100.0:.2f} % of the per-class filter; the filter costs {p_us / s_us:.3f} x the semantic filter, "
                 f"and both together {both / (p_us + s_us):.3f} x the sum of the two run separately.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
