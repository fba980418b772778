"""The opt-in device PNG encoder (Settings.PNG_DEVICE, ops.png_deflate) against the default Pillow writer processes.
  a     GPU time of ops.png_deflate per batch of 8 at 512x512, 512x704 and 1024x1024 (HIP events, median of rounds), for
        smooth-plus-noise images (Huffman segments) and uniform noise (stored segments)
  e2e   run_aug.main end to end on a synthetic dataset at 512x512 with the writers on: no writer at all (the loop's own rate
        and the generation time of a batch; that run stops before the JSON stage, which needs files), default, device, default
        again (run-to-run spread); host CPU-s per image of the whole process and of its children (getrusage) for each; bytes of
        the written files against Pillow's default save
  d     file bytes against Pillow's default for a smooth-plus-noise set encoded through the device op
usage: python tools/png_bench.py a | e2e <sd_v1.5|sd_xl-turbo> [n_images] | d        (each prints its section; append them to
profiles/png_device_bench.txt)"""
import io
import os
import resource
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import ops, pngenc  # noqa: E402
from saspa_aug_amd import run_aug as R  # noqa: E402


def smooth_noise(n, h, w, sigma, seed=0):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        base = 128 + 70 * np.sin(x / (17.0 + k)) * np.cos(y / 13.0) + 30 * np.sin((x + y) / (29.0 + 2 * k))
        img = base[..., None] + np.array([0, 9, -14]) + rng.normal(0, sigma, (h, w, 3))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return np.stack(out)


def pillow_bytes(arr):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.tell()


def part_a():
    dev = torch.device("cuda:0")
    print("(a) ops.png_deflate, batch of 8, GPU time (HIP events, median of 20 after 3 warm-up calls; allocation of the outputs included)")
    for h, w in ((512, 512), (512, 704), (1024, 1024)):
        for name, imgs in (("smooth + noise (sigma 6)", smooth_noise(8, h, w, 6)),
                           ("uniform noise", np.random.RandomState(1).randint(0, 256, (8, h, w, 3)).astype(np.uint8))):
            x = torch.from_numpy(imgs).to(dev)
            for _ in range(3):
                streams, sizes = ops.png_deflate(x)
            torch.cuda.synchronize()
            ts = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                streams, sizes = ops.png_deflate(x)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            z = sizes.cpu().numpy()
            print(f"    {h}x{w}  {name:26s} {np.median(ts):8.1f} us per batch (min {min(ts):.1f})   "
                  f"{z.sum() / imgs.nbytes:.3f} bytes out per byte in", flush=True)


class _NullWriters:
    """No PNG is written: the generation loop's own rate."""
    def __init__(self, workers=4):
        self.submitted, self.max_depth = 0, 0

    def submit(self, arr, path):
        self.submitted += 1

    def submit_encoded(self, zbytes, h, w, c, path):
        self.submitted += 1

    def close(self):
        pass


def _cpu():
    s, c = resource.getrusage(resource.RUSAGE_SELF), resource.getrusage(resource.RUSAGE_CHILDREN)
    return np.array([s.ru_utime + s.ru_stime, c.ru_utime + c.ru_stime])


def part_e2e(base_model, n_images):
    turbo = base_model == "sd_xl-turbo"
    steps = 2 if turbo else 50
    if turbo:
        R.NEGATIVE_PROMPT = None                       # run_aug/run_aug.py does the same for sd_xl-turbo
    tmp = tempfile.mkdtemp(prefix="saspa_png_")
    prompts = os.path.join(tmp, "prompts.txt")
    open(prompts, "w").write("".join(f"an airplane flying over landscape number {k}.\n" for k in range(20)))
    pipe = R.init_pipeline(base_model, "canny", 0).to("cuda:0", torch.float16)
    from saspa_aug_amd.dataset_utils import SyntheticUtils

    def settings(tag, n, device_png):
        root = os.path.join(tmp, tag, "data")
        SyntheticUtils(root_path=root, n_images=n, sizes=((512, 512),), print_func=lambda *a: None)
        return R.Settings(DATASET="synthetic", BASE_MODEL=base_model, RESOLUTION=512, NUM_INFERENCE_STEPS=steps, NUM_PER_IMAGE=4, SEED=1,
                          GUIDANCE_SCALE=0 if turbo else 7.5, SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, PROMPTS_FILE=prompts,
                          BATCH_SIZE=8, DATASET_KWARGS=dict(root_path=root, n_images=n, sizes=((512, 512),)), PNG_DEVICE=device_png)

    def run(tag, device_png, writers=None):
        s = settings(tag, n_images, device_png)
        keep = R._PngWriters
        if writers is not None:
            R._PngWriters = writers
        try:
            torch.cuda.synchronize()
            c0, t0 = _cpu(), time.time()
            try:
                res = R.main(s, pipe=pipe)
            except FileNotFoundError:                   # no writer, no files: the JSON stage (after the loop and the flush) refuses
                assert writers is not None
                res = dict(status=torch.ones(4 * n_images, dtype=torch.int32), output_folder=None, png_max_queue=0)
            torch.cuda.synchronize()
            dt, dc = time.time() - t0, _cpu() - c0
        finally:
            R._PngWriters = keep
        n = int((res["status"] == 1).sum())
        return dict(tag=tag, n=n, rate=n / dt, seconds=dt, cpu_self=dc[0] / n, cpu_children=dc[1] / n, folder=res["output_folder"],
                    depth=res["png_max_queue"])

    for tag, flag in (("warm_default", False), ("warm_device", True)):          # step graph, kernels, allocator
        R.main(settings(tag, 8, flag), pipe=pipe)
    rows = [run("no_writer", False, _NullWriters), run("default_1", False), run("device", True), run("default_2", False)]
    print(f"(b, c) run_aug.main end to end, {base_model}, 512x512, {steps} steps, batch 8, {rows[0]['n']} images per run (synthetic weights, "
          "synthetic dataset; PNG decode + resize, Canny, sampling, safety checker, D2H, PNG files, JSON)")
    print("    run          images/s   seconds   CPU-s/image whole process   CPU-s/image children   deepest writer backlog")
    for r in rows:
        print(f"    {r['tag']:12s} {r['rate']:8.2f}  {r['seconds']:8.2f}   {r['cpu_self']:25.4f}   {r['cpu_children']:20.4f}   {r['depth']:6d}")
    nw, d1, dv, d2 = rows
    spread = abs(d1["rate"] - d2["rate"])
    worst_default = min(d1["rate"], d2["rate"])
    print(f"    generation time of a batch of 8 in this run (no writer): {8 / nw['rate'] * 1e3:.1f} ms")
    print(f"    run-to-run spread of the default path: {spread:.2f} images/s; device path {dv['rate']:.2f} against {worst_default:.2f} .. "
          f"{max(d1['rate'], d2['rate']):.2f}: {'NOT slower' if dv['rate'] >= worst_default - spread else 'SLOWER'} than the default by more than that spread")
    wd = (d1["cpu_self"] + d1["cpu_children"] + d2["cpu_self"] + d2["cpu_children"]) / 2 - nw["cpu_self"] - nw["cpu_children"]
    we = dv["cpu_self"] + dv["cpu_children"] - nw["cpu_self"] - nw["cpu_children"]
    print(f"    writer-side host CPU-s per image (process + children, minus the no-writer run): default {wd:.4f}, device {we:.4f}")
    bound = max(d1["rate"], d2["rate"]) < 0.95 * nw["rate"]
    print(f"    writer-bound before? default {max(d1['rate'], d2['rate']):.2f} against {nw['rate']:.2f} images/s without any writer: "
          f"{'YES' if bound else 'NO'} (rule: more than 5 % below the no-writer rate)")
    # (d) the files of the device run against Pillow's default save of the same pixels
    ours = pil = 0
    files = sorted(p for p in os.listdir(dv["folder"]) if "_prompt_" in p)[:32]
    for name in files:
        path = os.path.join(dv["folder"], name)
        ours += os.path.getsize(path)
        pil += pillow_bytes(np.asarray(Image.open(path)))
    print(f"(d) generated images of the device run ({len(files)} files; SYNTHETIC weights, so the images are noise-like and next to nothing "
          f"compresses): {ours} bytes against Pillow's default {pil} ({ours / pil:.4f}x)", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


def part_d():
    dev = torch.device("cuda:0")
    print("(d) smooth-plus-noise synthetic set, 8 images per row, device stream + pngenc.frame against Pillow's default save")
    for h, w, sigma in ((512, 512, 2), (512, 512, 6), (512, 512, 16), (512, 704, 6), (96, 80, 6)):
        imgs = smooth_noise(8, h, w, sigma, seed=sigma)
        streams, sizes = ops.png_deflate(torch.from_numpy(imgs).to(dev))
        s, z = streams.cpu().numpy(), sizes.cpu().numpy()
        ours = pil = 0
        for k in range(len(imgs)):
            data = pngenc.frame(s[k, :z[k]].tobytes(), h, w, 3)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), imgs[k])
            ours += len(data)
            pil += pillow_bytes(imgs[k])
        print(f"    {h}x{w} sigma {sigma:2d}: {ours} bytes against {pil} ({ours / pil:.4f}x)", flush=True)


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "a"
    if part == "a":
        part_a()
    elif part == "e2e":
        part_e2e(sys.argv[2] if len(sys.argv) > 2 else "sd_v1.5", int(sys.argv[3]) if len(sys.argv) > 3 else 8)
    elif part == "d":
        part_d()
    else:
        raise SystemExit(__doc__)
