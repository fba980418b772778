"""The T5 key-to-text generator at full width (config.T5_COMMON_GEN), synthetic weights, bf16: sentences per second for 30 and for 200
sampled sentences of ONE input (the two sizes prompts_engineering/txt2sentance_prompts.py asks for: per class and general), the decoder
step's launch count, the time between HIP events around every launch of one recorded generate() (per kind), and -- in a kernel-trace
run of its own, second usage line -- how much of a step is launch gaps.  Nothing here is gated: the file reports what was seen.
usage: python tools/t5_bench.py [--rounds R] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/t5_bench.py --once N [--repeat K]
           K identical generate() calls of N sentences and nothing else: the trace's kernel time / K against the printed wall time of
           one call is the share of a step its kernels fill; the rest is launch gaps and the host loop (tools/stats_summary.py reads
           the kernel_stats csv).  HIP events around a launch cannot give that share: a pair brackets the dispatch as well."""
import argparse
import collections
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd import ops  # noqa: E402
from saspa_aug_amd import weights as W  # noqa: E402
from saspa_aug_amd.txt2sentence import T5Generator  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", type=int, default=0, help="N: run --repeat identical generate() calls of N sentences and exit (for a kernel trace)")
    ap.add_argument("--repeat", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("t5_bench needs the MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    cfg = CFG.T5_COMMON_GEN
    gen = T5Generator(W.t5_synth_state_dict(cfg, 0), cfg, dev, torch.bfloat16)
    text = gen.format_input("airplane, of type Boeing 707-320")
    one_ids, one_len = gen.tokenize([text])
    if args.once:
        ids, lens = one_ids.repeat(args.once, 0), one_len.repeat(args.once)
        u = torch.rand((args.once, cfg["max_length"]), generator=torch.Generator().manual_seed(0))
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = gen.generate(ids, lens, do_sample=True, uniforms=u)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        print(f"{args.repeat} identical generate() calls of {args.once} sentences, {out.shape[1] - 1} decoder steps each; the last one took "
              f"{wall * 1e3:.2f} ms of wall time")
        return
    lines = [f"T5 key-to-text generator, full width (t5-base: 12 + 12 layers, d_model 768, vocabulary 32128), synthetic weights, bf16, "
             f"sampling with top_k {cfg['top_k']}, top_p {cfg['top_p']}, temperature {cfg['temperature']}, max_length {cfg['max_length']}; "
             f"input {text!r} = {int(one_len[0])} tokens; {torch.cuda.get_device_name(0)}; median [min .. max] of {args.rounds} rounds", ""]
    for num in (30, 200):
        ids, lens = one_ids.repeat(num, 0), one_len.repeat(num)
        rng = torch.Generator().manual_seed(0)
        u = torch.rand((num, cfg["max_length"]), generator=rng)
        out = gen.generate(ids, lens, do_sample=True, uniforms=u)                  # warm-up (the timed rounds repeat it exactly)
        steps = out.shape[1] - 1
        torch.cuda.synchronize()
        whole = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            gen.generate(ids, lens, do_sample=True, uniforms=u)
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t0)
        w = statistics.median(whole)
        rec = EventRecorder()
        ops.set_recorder(rec)
        try:
            gen.generate(ids, lens, do_sample=True, uniforms=u)
        finally:
            ops.set_recorder(None)
        tot = rec.totals()
        dev_ms = sum(tot.values())
        launches = collections.Counter(k for k, _, _ in rec.ev)
        n_launch = len(rec.ev)
        enc_launches = cfg["enc_layers"] * 7 + 1 + cfg["dec_layers"]                # encoder blocks + final norm + the cross K | V
        per_step = (n_launch - enc_launches) / steps
        _, entry_of, slot_seq, group = gen.plan_rows(ids, lens)
        lines += [f"{num:4d} sentences of one input ({len(slot_seq)} decoder rows = {len(entry_of)} entries x group {group}): "
                  f"{num / w:8.1f} sentences/s   whole {w * 1e3:8.1f} ms [{min(whole) * 1e3:.1f} .. {max(whole) * 1e3:.1f}] = "
                  f"{w * 1e3 / steps:6.2f} ms per decoder step ({steps} steps, wall clock incl. the per-step token copy)",
                  f"     one recorded generate(): {n_launch} launches ({enc_launches} encoder + cross K|V, {per_step:.0f} per decoder step), "
                  f"{dev_ms:8.2f} ms between the HIP events around the launches (a pair brackets the dispatch too: an upper bound of "
                  f"the kernels' time, {dev_ms * 1e3 / n_launch:.1f} us per launch)",
                  "     by kind: " + ", ".join(f"{k} {t:.2f} ms / {launches[k]}" for k, t in sorted(tot.items(), key=lambda kv: -kv[1]))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
