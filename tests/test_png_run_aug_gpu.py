"""run_aug.main with PNG_DEVICE on against the default writers: the same tree, the same pixels, the same JSON."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import config as CFG
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import weights as W
from saspa_aug_amd.pipeline import StableDiffusionControlNetPipeline

pytestmark = pytest.mark.gpu


def _settings(root, **kw):
    root.mkdir()
    prompts = root / "prompts.txt"
    prompts.write_text("".join(f"an airplane in scene {k}.\n" for k in range(6)))
    return R.Settings(DATASET="synthetic", BASE_MODEL="sd_v1.5", RESOLUTION=64, NUM_INFERENCE_STEPS=3, NUM_PER_IMAGE=2, SEED=1,
                      USE_ARTISTIC_PROMPTS=True, SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0,
                      PROMPTS_FILE=str(prompts), BATCH_SIZE=4,
                      DATASET_KWARGS=dict(root_path=str(root / "ds" / "data"), n_images=5, sizes=((64, 64), (64, 128))), **kw)


def test_device_png_tree_equals_the_default_tree(dev, tmp_path):
    cfgs = CFG.tiny()
    pipe = StableDiffusionControlNetPipeline(W.synth_family(cfgs, seed=3), cfgs).to("cuda:0", torch.float16)
    ref = R.main(_settings(tmp_path / "a"), pipe=pipe)
    got = R.main(_settings(tmp_path / "b", PNG_DEVICE=True), pipe=pipe)
    assert (ref["status"] == 1).all() and (got["status"] == 1).all() and len(got["items"]) == 10
    a, b = Path(ref["output_folder"]), Path(got["output_folder"])
    names = sorted(p.name for p in a.glob("*.png"))
    assert names == sorted(p.name for p in b.glob("*.png")) and len(names) == 20
    checked = 0
    for name in names:
        with Image.open(b / name) as im:
            im.verify()
        if "_prompt_" in name or name.endswith("_source.png"):
            x, y = np.asarray(Image.open(a / name)), np.asarray(Image.open(b / name))
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), name
            checked += 1
        else:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name       # control maps stay on the Pillow writers
    assert checked == 15
    assert got["png_submitted"] == ref["png_submitted"] == 20
    ja = json.loads(Path(ref["json_path"]).read_text().replace(str(tmp_path / "a"), "ROOT"))
    jb = json.loads(Path(got["json_path"]).read_text().replace(str(tmp_path / "b"), "ROOT"))
    assert ja == jb and len(ja) == 5
