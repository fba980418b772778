#!/usr/bin/env python3
"""Write the per-image BLIP captions of a dataset: the file PROMPT_TYPE = "captions" reads.  Edit the constants below and run

    python run_aug/write_captions.py

then point the generation at the result: Settings.PROMPTS_FILE / SASPA_PROMPTS_FILE=<OUTPUT> with PROMPT_TYPE = "captions".
Environment overlays (optional): SASPA_DATASET, SASPA_WEIGHTS_DIR (a directory with the BLIP caption checkpoint and its vocab.txt),
SASPA_CAPTIONS_FILE, SASPA_PRECISION.  Without a checkpoint the captioner refuses, unless SASPA_SYNTHETIC_CAPTIONER=1 asks for the
captions of a random model on purpose."""
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import saspa_aug_amd  # noqa: E402,F401

if __name__ == "__main__":
    import torch

    from saspa_aug_amd import dataset_utils
    from saspa_aug_amd.prompts_engineering import blip_utils

    DEVICE = "cuda:0"
    DATASET = os.environ.get("SASPA_DATASET", "dtd")
    DATASET_KWARGS = {}
    WEIGHTS_DIR = os.environ.get("SASPA_WEIGHTS_DIR") or None
    OUTPUT = os.environ.get("SASPA_CAPTIONS_FILE") or str(Path(__file__).resolve().parent.parent / "saspa-aug_amd" /
                                                          "prompts_engineering" / "captions" / f"{DATASET}_captions_generated.json")
    BATCH_SIZE = 32
    PRECISION = os.environ.get("SASPA_PRECISION", "bf16")          # "bf16" (production) | "fp32" (parity mode)

    logging.basicConfig(level=logging.INFO)
    ds_utils = dataset_utils.DS_UTILS_DICT[DATASET](**DATASET_KWARGS)
    blip_utils.write_captions_of_a_dataset_to_json(DATASET, ds_utils.original_images_paths, OUTPUT, weights_dir=WEIGHTS_DIR,
                                                   batch_size=BATCH_SIZE, device=DEVICE,
                                                   dtype=torch.float32 if PRECISION == "fp32" else torch.bfloat16)
