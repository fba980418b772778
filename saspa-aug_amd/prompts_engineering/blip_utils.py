"""Per-image BLIP captions for PROMPT_TYPE = "captions" (the reference's prompts_engineering/blip_utils.py:28-58): every original image
is captioned once and the result is written as {image_path: {"caption": str}} -- the layout of the shipped captions/dtd_captions.json,
keyed by the paths `ds_utils.original_images_paths` gives.  The captioner runs on the device (captioner.BlipCaptioner); images are
decoded on a prefetch thread while the previous batch is captioned.  The VQA questions of the reference are not built."""
import json
import logging
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from .. import config as CFG
from ..captioner import BlipCaptioner

CAPTION_CONFIG = CFG.BLIP_CAPTION          # tests swap in config.tiny_blip_caption()


def load_captioner(weights_dir=None, device="cuda:0", dtype=torch.bfloat16):
    """The captioner from a checkpoint directory; without one it refuses unless SASPA_SYNTHETIC_CAPTIONER=1 (captioner.from_synthetic)."""
    if weights_dir:
        return BlipCaptioner.from_pretrained(weights_dir, device, dtype, CAPTION_CONFIG)
    cap = BlipCaptioner.from_synthetic(CAPTION_CONFIG, device, dtype)
    logging.warning("BLIP captioner: SASPA_SYNTHETIC_CAPTIONER=1 -> SYNTHETIC weights and a hash vocabulary; its captions are those of "
                    "a random model")
    return cap


def _load_batch(paths):
    out = []
    for p in paths:
        with Image.open(p) as im:
            out.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
    return out


def write_captions_of_a_dataset_to_json(dataset_name, image_paths, output_file, questions=[], *, weights_dir=None, batch_size=32,
                                        device="cuda:0", dtype=torch.bfloat16, captioner=None):
    """Caption every image of `image_paths` and write {path: {"caption": str}} to `output_file`.  questions: the reference also asks a
    VQA model per image; that model is not built, a non-empty list is refused."""
    if questions:
        raise NotImplementedError("the VQA questions of the reference's blip_utils are not built: captions only")
    image_paths = [str(p) for p in image_paths]
    cap = captioner if captioner is not None else load_captioner(weights_dir, device, dtype)
    batches = [image_paths[i:i + batch_size] for i in range(0, len(image_paths), batch_size)]
    result = {}
    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(_load_batch, batches[0]) if batches else None
        for bi, paths in enumerate(batches):
            images = nxt.result()
            nxt = pool.submit(_load_batch, batches[bi + 1]) if bi + 1 < len(batches) else None
            for path, text in zip(paths, cap.caption(images)):
                result[path] = {"caption": text}
    os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
    with open(output_file, "w") as f:
        json.dump(result, f, indent=1)
    logging.info(f"Wrote {len(result)} captions of {dataset_name} to {output_file}")
    return result


def read_captions_from_json(path):
    with open(path) as f:
        return json.load(f)
