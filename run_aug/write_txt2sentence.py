#!/usr/bin/env python3
"""Write the txt2sentence prompts of a dataset: the {class: [sentences]} file PROMPT_TYPE = "txt2sentence" (ALL_CLASSES False: NUM
sentences about the dataset's general class) and "txt2sentence-per_class" (ALL_CLASSES True: NUM per class) read.  Edit the constants
below and run

    python run_aug/write_txt2sentence.py

then point the generation at the printed path: Settings.PROMPTS_FILE / SASPA_PROMPTS_FILE=<path>.
Environment overlays (optional): SASPA_DATASET, SASPA_T2S_NUM, SASPA_T2S_ALL_CLASSES (0 / 1), SASPA_T2S_OUTPUT_DIR, SASPA_WEIGHTS_DIR (a
directory with the T5 checkpoint: config.json, model.safetensors or pytorch_model.bin, tokenizer.json), SASPA_T2S_KEYWORDS
(comma-separated must-keywords instead of the dataset's), SASPA_T2S_SEED, SASPA_PRECISION.  Without a checkpoint the generator refuses,
unless SASPA_SYNTHETIC_T5=1 asks for the sentences of a random model on purpose."""
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import saspa_aug_amd  # noqa: E402,F401

if __name__ == "__main__":
    import torch

    from saspa_aug_amd.prompts_engineering import txt2sentance_prompts

    DEVICE = "cuda:0"
    DATASET = os.environ.get("SASPA_DATASET", "planes")
    DATASET_KWARGS = {}
    ALL_CLASSES = os.environ.get("SASPA_T2S_ALL_CLASSES", "1") == "1"   # True: per sub-class (30 in the reference); False: general (200)
    NUM = int(os.environ.get("SASPA_T2S_NUM", "30" if ALL_CLASSES else "200"))
    WEIGHTS_DIR = os.environ.get("SASPA_WEIGHTS_DIR") or None
    OUTPUT_DIR = os.environ.get("SASPA_T2S_OUTPUT_DIR") or str(Path(__file__).resolve().parent.parent / "saspa-aug_amd" /
                                                              "prompts_engineering" / "txt2sentance_prompts")
    KEYWORDS = [k for k in os.environ.get("SASPA_T2S_KEYWORDS", "").split(",") if k] or None
    BATCH_SIZE = 64
    SEED = int(os.environ.get("SASPA_T2S_SEED", "0"))
    PRECISION = os.environ.get("SASPA_PRECISION", "bf16")          # "bf16" (production) | "fp32" (parity mode)

    logging.basicConfig(level=logging.INFO)
    path = txt2sentance_prompts.main(DATASET, NUM, OUTPUT_DIR, ALL_CLASSES, weights_dir=WEIGHTS_DIR, batch_size=BATCH_SIZE, seed=SEED,
                                     device=DEVICE, dtype=torch.float32 if PRECISION == "fp32" else torch.bfloat16,
                                     dataset_kwargs=DATASET_KWARGS, must_keywords=KEYWORDS)
    print(path)
