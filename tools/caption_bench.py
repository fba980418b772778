"""The BLIP captioner at full width (config.BLIP_CAPTION), synthetic weights, batch B (default 32) images of 384 x 384, 3 beams,
LAVIS' generate defaults: captions per second, milliseconds per decode step, and the share of a decode step spent in the two decoder
kernels (saspa_decode_attn, saspa_logprob_topk) from HIP events around every launch of one recorded generate() -- next to
tests/caption_ref.py on the CPU (16 threads) for the same images.  The shader clock is sampled over the timed rounds.  Nothing here is
gated: the file reports what was seen.
usage: python tools/caption_bench.py [--batch B] [--rounds R] [--cpu-images N] [--out FILE]"""
import argparse
import collections
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import saspa_aug_amd  # noqa: E402,F401
import caption_ref as R  # noqa: E402
from bench import ClockSampler  # noqa: E402
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd import ops  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402
from saspa_aug_amd.captioner import BlipCaptioner  # noqa: E402


class EventRecorder:
    """ops launch recorder: a pair of HIP events around every launch, summed per kind after one synchronisation."""

    def __init__(self):
        self.ev = []

    def __call__(self, kind, flops, call, meta=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        self.ev.append((kind, a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        t = collections.OrderedDict()
        for kind, a, b in self.ev:
            t[kind] = t.get(kind, 0.0) + a.elapsed_time(b)
        return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=None, help="images the CPU reference captions (default: the whole batch)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caption_bench needs the MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    cfg, n, nb = CFG.BLIP_CAPTION, args.batch, CFG.BLIP_CAPTION["num_beams"]
    sd = W.synth_state_dict("blip_caption", cfg, 0)
    imgs = torch.randint(0, 256, (n, 384, 384, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    lines = [f"BLIP captioner, full width, synthetic weights, batch {n} x 384x384 u8, {nb} beams, max_length {cfg['max_length']}, "
             f"min_length {cfg['min_length']}; {torch.cuda.get_device_name(0)}; median [min .. max] of {args.rounds} rounds", ""]
    for dtype in (torch.bfloat16, torch.float32):
        cap = BlipCaptioner(sd, cfg, dev, dtype)
        dimgs = imgs.to(dev)
        ids = cap.generate(dimgs)                                       # warm-up
        steps = ids.shape[1] - len(cap.prompt_ids())
        torch.cuda.synchronize()
        whole, vis_t, clocks = [], [], []
        for _ in range(args.rounds):
            cs = ClockSampler(dev, period=0.02).start()
            t0 = time.perf_counter()
            vis = cap.vision(cap.preprocess(dimgs))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            cap.generate(image_tokens=vis)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            c = cs.stop()
            whole.append(t2 - t0)
            vis_t.append(t1 - t0)
            if c:
                clocks.append(c["sclk_mhz_median"])
        w, v = statistics.median(whole), statistics.median(vis_t)
        rec = EventRecorder()
        ops.set_recorder(rec)
        try:
            cap.generate(image_tokens=vis)
        finally:
            ops.set_recorder(None)
        tot = rec.totals()
        dev_ms = sum(tot.values())
        new = tot.get("decode_attn", 0.0) + tot.get("logprob_topk", 0.0)
        launches = collections.Counter(k for k, _, _ in rec.ev)
        ck = sorted(clocks)
        lines += [f"{str(dtype).replace('torch.', '')}: {n / w:8.1f} captions/s   whole {w * 1e3:8.1f} ms [{min(whole) * 1e3:.1f} .. {max(whole) * 1e3:.1f}]"
                  f"   vision + pre-processing {v * 1e3:7.1f} ms   decode {(w - v) * 1e3:7.1f} ms = {(w - v) * 1e3 / (steps + len(cap.prompt_ids())):6.2f} ms per "
                  f"decoder position ({len(cap.prompt_ids())} prompt + {steps} generated, wall clock incl. the host beam search)"
                  f"   shader clock median {ck[len(ck) // 2] if ck else float('nan'):.0f} MHz",
                  f"    one recorded generate(): {len(rec.ev)} launches, {dev_ms:8.2f} ms on the device by HIP events; decode_attn "
                  f"{tot.get('decode_attn', 0.0):7.2f} ms in {launches['decode_attn']} launches, logprob_topk {tot.get('logprob_topk', 0.0):6.2f} ms in "
                  f"{launches['logprob_topk']} launches: the two new kernels are {100.0 * new / dev_ms:5.1f} % of the decode's device time"]
        top = sorted(tot.items(), key=lambda kv: -kv[1])[:6]
        lines.append("    largest kinds: " + ", ".join(f"{k} {t:.2f} ms" for k, t in top))
        del cap
        torch.cuda.empty_cache()
    # the CPU reference on the same images (fp32, 16 threads)
    torch.set_num_threads(16)
    m = n if args.cpu_images is None else min(n, args.cpu_images)
    cap = BlipCaptioner(sd, cfg, dev, torch.float32)
    px = cap.preprocess(imgs[:m].to(dev))[..., :3].permute(0, 3, 1, 2).float().cpu()
    prompt = cap.prompt_ids()
    del cap
    t0 = time.perf_counter()
    with torch.no_grad():
        ref, _ = R.generate(sd, cfg, px, prompt)
    t = time.perf_counter() - t0
    lines += ["", f"tests/caption_ref.py on the CPU, fp32, {torch.get_num_threads()} threads, {m} of the same images: {t:7.1f} s = {m / t:6.2f} captions/s "
                  f"({ref.shape[1] - len(prompt)} generated positions)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
