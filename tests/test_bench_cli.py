"""bench.py's own launcher (`python bench.py --gpus N` with no torchrun around it) and the newest-profile lookup, on CPU.
`--dry` runs the N-rank plumbing -- rendezvous on 127.0.0.1, the one gather, max-over-ranks timing, ONE JSON line from
rank 0 -- on gloo with no GPU work; without `--dry` every rank must fail loudly on a box without a GPU and the launcher must
return non-zero (no silent single-rank run, no CPU fallback)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=300, env=e)


def test_gpus_n_self_launches_n_ranks_dry():
    r = _run("--gpus", "3", "--dry", "--steps", "2", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 3 and line["steps"] == 2 and line["data"] == "dry-run" and line["scaling"] == "weak"
    assert "not a valid result" in line["config"]["workload"]


def test_gpus_n_without_gpu_fails_loudly():
    r = _run("--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", env={"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert r.returncode != 0
    assert "no HIP device" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_world_size_mismatch_is_refused():
    r = _run("--gpus", "2", "--dry", env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_newest_traffic_profile_orders_by_round_then_version(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    for name in ("r1_pmc_traffic_v7.json", "r1_pmc_traffic_v13.json", "r1_pmc_traffic.json"):
        (prof / name).write_text("{}")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert os.path.basename(bench.newest_traffic_profile()) == "r1_pmc_traffic_v13.json"      # not _v7 (plain sort)
    (prof / "r2_pmc_traffic_v2.json").write_text("{}")
    assert os.path.basename(bench.newest_traffic_profile()) == "r2_pmc_traffic_v2.json"


def test_dump_outputs_keeps_to_64_mb(tmp_path):
    """--dump-outputs: float32 copies of what the step returned; whole leading items while they fit the budget, a fixed seeded
    sample of the first item when not even one does, 64 MB at most in all."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 1024, 1024, 3), dtype=torch.uint8, generator=g)        # 100 MB as float32
    flags = torch.tensor([0, 1] * 4, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "a"), imgs, flags)
    got = np.load(tmp_path / "a" / "images.npy")
    assert got.dtype == np.float32 and got.shape[0] >= 1 and got.shape[1:] == (1024, 1024, 3)
    assert np.array_equal(got, imgs[:got.shape[0]].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "nsfw.npy"), flags.numpy().astype(np.float32))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    one = torch.randint(0, 256, (1, 3000, 3000, 3), dtype=torch.uint8, generator=g)         # 108 MB as float32
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), one, None)
        assert sorted(os.listdir(tmp_path / d)) == ["images.npy"]
        assert (tmp_path / d / "images.npy").stat().st_size <= 64 << 20
    b, c = np.load(tmp_path / "b" / "images.npy"), np.load(tmp_path / "c" / "images.npy")
    assert b.dtype == np.float32 and b.size > 1 << 20 and np.array_equal(b, c)


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(dev, tmp_path):
    """A plain run: exactly --steps timed steps, `ms_per_step`, no secondary measurements; --dump-outputs writes the last timed
    step's images and NSFW flags, identical from run to run."""
    import numpy as np
    argv = ("--tiny", "--res", "64", "--batch", "2", "--ddim-steps", "3", "--steps", "3", "--warmup", "1")
    dumps = []
    for run in ("a", "b"):
        r = _run(*argv, "--dump-outputs", str(tmp_path / run))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "bf16"
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["clock"] is None
        assert abs(line["value"] - 2 * 3 / (3 * line["ms_per_step"] * 1e-3)) / line["value"] < 0.01
        assert sorted(os.listdir(tmp_path / run)) == ["images.npy", "nsfw.npy"]
        dumps.append([np.load(tmp_path / run / f) for f in ("images.npy", "nsfw.npy")])
    (img, nsfw), (img2, nsfw2) = dumps
    assert img.dtype == np.float32 and img.shape == (2, 64, 64, 3) and img.min() >= 0 and img.max() <= 255
    assert nsfw.dtype == np.float32 and nsfw.shape == (2,)
    assert np.array_equal(img, img2) and np.array_equal(nsfw, nsfw2)
