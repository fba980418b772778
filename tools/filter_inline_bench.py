"""What the filter stage costs end to end, and what FILTER_INLINE changes: `run_aug.main` with sd_v1.5 + canny, batch 8, 512 x 512,
full-width synthetic filter models (SASPA_SYNTHETIC_FILTERS=1: CLIP RN50 + WSDAN_CAL resnet101) in three arms

    A  filters off                       (the only configuration the other end-to-end tools measure)
    B  filters on, post-hoc              (today's default: rank 0 decodes every PNG again after the loop)
    C  filters on, in-line               (Settings.FILTER_INLINE: scored while generating, decided from the records)

Per arm: generation-loop images/s (start of main -> start of the JSON stage), JSON-stage seconds, PNGs decoded by the stage, total
wall time.  A - C is the recording cost, B - C what the mode saves; both only mean something inside one call on one box.
Every arm runs in a fresh child process under its own time limit, the arms alternated (A B C, C B A, ...); a child that fails or
runs out of time ends the whole call.  The filter models are built and one warm-up batch of the arm's own kind is run before the clock
starts; the shader clock is sampled during the timed run (bench.py's ClockSampler) and printed as the arm's `clock` line.
usage: python tools/filter_inline_bench.py [--images 96] [--steps 30] [--rounds 2] [--limit 420] [--out profiles/filter_inline_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def run_arm(arm, images, steps):
    os.environ["SASPA_SYNTHETIC_FILTERS"] = "1"
    import torch

    import saspa_aug_amd  # noqa: F401
    from bench import ClockSampler
    from saspa_aug_amd import filters, utils
    from saspa_aug_amd import run_aug as R
    from saspa_aug_amd.dataset_utils import SyntheticUtils
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix=f"saspa_filter_{arm}_")
    prompts = os.path.join(tmp, "prompts.txt")
    open(prompts, "w").write("".join(f"an airplane flying over landscape number {k}.\n" for k in range(20)))
    pipe = R.init_pipeline("sd_v1.5", "canny", 0).to("cuda:0", torch.float16)
    on = arm != "A"

    def settings(root, n, per):
        return R.Settings(DATASET="synthetic", BASE_MODEL="sd_v1.5", RESOLUTION=512, NUM_INFERENCE_STEPS=steps, NUM_PER_IMAGE=per, SEED=1,
                          SEMANTIC_FILTERING=int(on), MODEL_CONFIDENCE_BASED_FILTERING=int(on), FILTER_INLINE=arm == "C",
                          PROMPTS_FILE=prompts, BATCH_SIZE=8, DATASET_KWARGS=dict(root_path=root, n_images=n, sizes=((512, 512),)))
    warm = settings(os.path.join(tmp, "warm", "data"), 8, 1)
    ds = SyntheticUtils(**warm.DATASET_KWARGS, print_func=lambda *a: None)
    models = filters.build_filters(ds, dev, True, True, None) if on else None
    R.main(warm, pipe=pipe, filter_models=models)                   # this arm's step graph, filter kernels and allocator, off the clock
    s = settings(os.path.join(tmp, "run", "data"), images // 2, 2)
    SyntheticUtils(**s.DATASET_KWARGS, print_func=lambda *a: None)    # the dataset exists before the clock starts
    decoded, stage = [], {}
    real_load, real_json = filters._load_u8, utils.create_json_of_image_name_to_augmented_images_paths
    filters._load_u8 = lambda p: decoded.append(p) or real_load(p)

    def timed_json(*a, **k):
        torch.cuda.synchronize()
        stage["t0"] = time.time()
        out = real_json(*a, **k)
        torch.cuda.synchronize()
        stage["t1"] = time.time()
        return out
    utils.create_json_of_image_name_to_augmented_images_paths = timed_json
    sampler = ClockSampler(dev).start()
    torch.cuda.synchronize()
    t0 = time.time()
    res = R.main(s, pipe=pipe, filter_models=models)
    torch.cuda.synchronize()
    t1 = time.time()
    clock = sampler.stop()
    n = int((res["status"] == 1).sum())
    kept = sum(len(v) for v in json.load(open(res["json_path"])).values())
    print("RESULT " + json.dumps(dict(arm=arm, images=n, kept_by_the_filters=kept, loop_s=round(stage["t0"] - t0, 2),
                                      loop_images_per_s=round(n / (stage["t0"] - t0), 3), json_stage_s=round(stage["t1"] - stage["t0"], 2),
                                      pngs_decoded=len(decoded), total_s=round(t1 - t0, 2), steps=steps, clock=clock)), flush=True)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("A", "B", "C"))
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="seconds a single arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return run_arm(a.arm, a.images, a.steps)
    lines = [f"# tools/filter_inline_bench.py --images {a.images} --steps {a.steps} --rounds {a.rounds}: run_aug.main, sd_v1.5 + canny, "
             "batch 8, 512x512, synthetic full-width filters; A = filters off, B = post-hoc, C = in-line; one call, arms alternated"]
    results = []
    for r in range(a.rounds):
        for arm in ("ABC" if r % 2 == 0 else "CBA"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--arm", arm, "--images", str(a.images),
                   "--steps", str(a.steps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                print(p.stdout[-4000:])
                sys.exit(f"arm {arm} (round {r}) ended with status {p.returncode}: nothing more is started")
            res = json.loads(got[-1][7:])
            results.append(res)
            lines.append(f"round {r} arm {arm}: loop {res['loop_images_per_s']} images/s ({res['images']} images in {res['loop_s']} s), JSON stage "
                         f"{res['json_stage_s']} s, {res['pngs_decoded']} PNGs decoded, total {res['total_s']} s")
            lines.append(f"round {r} arm {arm} clock: {json.dumps(res['clock'])}")
            print("\n".join(lines[-2:]), flush=True)
    mean = {arm: {k: sum(x[k] for x in results if x["arm"] == arm) / max(1, sum(x["arm"] == arm for x in results))
                  for k in ("total_s", "json_stage_s", "loop_s")} for arm in "ABC"}
    lines.append("mean over rounds: " + "; ".join(f"{arm} total {m['total_s']:.2f} s (loop {m['loop_s']:.2f} s + JSON stage {m['json_stage_s']:.2f} s)"
                                                  for arm, m in mean.items()))
    lines.append(f"recording cost A - C = {mean['A']['total_s'] - mean['C']['total_s']:+.2f} s; the mode saves B - C = "
                 f"{mean['B']['total_s'] - mean['C']['total_s']:+.2f} s, on {a.images} images, one GPU")
    print("\n".join(lines[-2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
