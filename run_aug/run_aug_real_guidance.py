#!/usr/bin/env python3
"""Entry point of the Real-Guidance baseline (the reference's run_aug/run_aug_real_guidance.py:513-556): SD-1.5 img2img at a low
SDEdit strength without a ControlNet, "txt2sentence" prompts, and the per-class CLIP filter in place of the semantic and
model-confidence filters.  Same launch forms as run_aug/run_aug.py:

    python run_aug/run_aug_real_guidance.py                                   # one MI355X
    SASPA_GPUS=8 python run_aug/run_aug_real_guidance.py                      # 8 MI355X, supervised
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 run_aug/run_aug_real_guidance.py

and the same environment overlays: SASPA_DATASET, SASPA_WEIGHTS_DIR, SASPA_PROMPTS_FILE, SASPA_NUM_INFERENCE_STEPS,
SASPA_NUM_PER_IMAGE, SASPA_PRECISION, SASPA_BASE_MODEL (sd_v1.5 | sd_v2.1: the two ControlNet-free img2img pipelines), SASPA_LPIPS_MIN / SASPA_LPIPS_MAX, SASPA_CLIP_FILTERING (default
"per_class"; "none" switches the filter off), SASPA_CLIP_FILTERING_DISCOUNT, SASPA_PNG_DEVICE and SASPA_FP16 / SASPA_FP16_VAE.  The output folder carries the step count and
guidance scale after the seed (`..._seed_1_num_inf_steps_50_gs_7.5/images`), as the reference's script names it."""
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import saspa_aug_amd  # noqa: E402,F401

if __name__ == "__main__" and "WORLD_SIZE" not in os.environ and \
        (int(os.environ.get("SASPA_GPUS", "1")) > 1 or os.environ.get("SASPA_SUPERVISE", "0") == "1"):
    # become the launcher BEFORE torch is imported: the parent never touches the GPU (saspa_aug_amd/launcher.py)
    from saspa_aug_amd.launcher import launch_supervised  # noqa: E402
    sys.exit(launch_supervised(int(os.environ.get("SASPA_GPUS", "1")), __file__, sys.argv[1:]))

from saspa_aug_amd import run_aug as R  # noqa: E402


def real_guidance_settings(env=None):
    """The Settings of a Real-Guidance run: the baseline's constants, then the environment overlays."""
    env = os.environ if env is None else env

    def number(name, kind, default):
        return kind(env[name]) if env.get(name) else default
    clip_type = env.get("SASPA_CLIP_FILTERING", "per_class")
    return R.Settings(
        # ---------------------------- generation params ----------------------------
        DATASET=env.get("SASPA_DATASET", "cars"), BASE_MODEL=env.get("SASPA_BASE_MODEL") or "sd_v1.5", CONTROLNET=None,
        SDEDIT=1, SDEDIT_STRENGTH=0.15, NUM_PER_IMAGE=number("SASPA_NUM_PER_IMAGE", int, 2), SEED=1,
        PROMPT_TYPE="txt2sentence", PROMPT_WITH_SUB_CLASS=True, USE_ARTISTIC_PROMPTS=False, USE_CAMERA_VARIATIONS_PROMPTS=False,
        RESOLUTION=512, GUIDANCE_SCALE=7.5, NUM_INFERENCE_STEPS=number("SASPA_NUM_INFERENCE_STEPS", int, 50),
        # ---------------------------- json creation params ----------------------------
        LPIPS_MIN=number("SASPA_LPIPS_MIN", float, None), LPIPS_MAX=number("SASPA_LPIPS_MAX", float, None),
        CLIP_FILTERING_TYPE=None if clip_type.lower() in ("", "0", "none") else clip_type,
        CLIP_FILTERING_DISCOUNT=number("SASPA_CLIP_FILTERING_DISCOUNT", float, 1),
        SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0,
        # ---------------------------- this build ----------------------------
        FOLDER_STEPS_GS_SUFFIX=True, BATCH_SIZE=8, PRECISION=env.get("SASPA_PRECISION", "bf16"),
        WEIGHTS_DIR=env.get("SASPA_WEIGHTS_DIR"), PROMPTS_FILE=env.get("SASPA_PROMPTS_FILE"),
        PNG_DEVICE=env.get("SASPA_PNG_DEVICE", "0") == "1",
        FP16=env.get("SASPA_FP16", "0") == "1", FP16_VAE=env.get("SASPA_FP16_VAE", "bf16"),
        FILTER_INLINE=env.get("SASPA_FILTER_INLINE", "0") == "1")


if __name__ == "__main__":
    s = real_guidance_settings()
    assert s.DATASET in R.dataset_utils.DATASETS_SUPPORTED
    assert s.BASE_MODEL in R.BASE_MODEL_DICT.keys()
    assert s.NUM_PER_IMAGE > 0

    dist = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("SASPA_FORCE_DIST", "0") == "1":
        # one process per GPU, RCCL over xGMI (SASPA_FORCE_DIST=1: the same leg at world size 1 -- a one-GPU rehearsal)
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local_rank)
        s.DEVICE = f"cuda:{local_rank}"
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    result = R.main(s, dist=dist)
    if dist is not None:
        dist.destroy_process_group()
    if result["json_path"]:
        print(result["json_path"])
