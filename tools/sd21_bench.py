"""Throughput of the ControlNet-free forms at full width (synthetic weights, bf16): sd_v1.5 text-to-image, sd_v2.1 text-to-image and
sd_v2.1 SDEdit img2img (strength 0.85, the SaSPA setting) at 512 x 512, batch 8, 50 DDIM steps, guidance 7.5 -- beside the sd_v1.5 +
Canny ControlNet pipeline of the same build in the same process (the BASELINE workload's pipeline, timed here the same simple way, NOT
bench.py's method).  One pipeline is resident at a time: per form one warm-up generation (graph capture), then `rounds` timed
generations; the median round is reported, one JSON line per form.  usage: python tools/sd21_bench.py [batch] [--steps N] [--rounds N]"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import config as CFG, ops
from saspa_aug_amd import run_aug as R
from saspa_aug_amd.synthetic import synthetic_image, synthetic_prompt_ids


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


dev = torch.device('cuda:0')
b = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 8
steps, rounds, res = arg("--steps", 50), arg("--rounds", 3), 512
ids, neg = synthetic_prompt_ids(b), synthetic_prompt_ids(1, seed=9)
imgs = torch.from_numpy(np.stack([synthetic_image(res, res, i) for i in range(b)])).to(dev)
g = torch.manual_seed(1)
lat, lat2 = (torch.randn((b, 4, res // 8, res // 8), generator=g, dtype=torch.float16) for _ in range(2))
FORMS = (("sd_v1.5 + canny ControlNet, text-to-image", ("sd_v1.5", "canny", 0)), ("sd_v1.5, text-to-image", ("sd_v1.5", None, 0)),
         ("sd_v2.1, text-to-image", ("sd_v2.1", None, 0)), ("sd_v2.1, SDEdit img2img strength 0.85", ("sd_v2.1", None, 1)))
times = {name: [] for name, _ in FORMS}
for name, (base, cn, sdedit) in FORMS:
    t0 = time.time()
    pipe = R.init_pipeline(base, cn, sdedit).to(dev, torch.bfloat16)          # synthetic weights at the family's full width

    def once():
        if cn:
            return pipe.generate_batch(ids, neg, ops.canny(imgs, 120, 200), lat, steps, 7.5, 0.75)
        if sdedit:
            return pipe.generate_batch_img2img(ids, neg, imgs, lat, lat2, steps, 0.85, 7.5)
        return pipe.generate_batch(ids, neg, lat, steps, 7.5)
    out = once(); torch.cuda.synchronize()                                    # warm-up: graph capture, allocator
    print(f"{name}: built and warmed in {time.time() - t0:.0f} s", flush=True)
    for _ in range(rounds):
        t1 = time.time()
        out2 = once()
        torch.cuda.synchronize(); times[name].append(time.time() - t1)
    med = sorted(times[name])[len(times[name]) // 2]
    print(json.dumps({"workload": f"{name}, batch={b} {res}x{res}, {steps} DDIM steps, CFG 7.5", "images_per_s": round(b / med, 3),
                      "s_per_batch": round(med, 4), "rounds_s_per_batch": [round(v, 4) for v in times[name]],
                      "deterministic": bool(torch.equal(out, out2)), "finite": bool(out.float().isfinite().all()), "dtype": "bf16",
                      "data": "synthetic"}), flush=True)
    del pipe, out, out2
    torch.cuda.empty_cache()
