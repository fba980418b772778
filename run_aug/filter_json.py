#!/usr/bin/env python3
"""Write an aug JSON for other filter settings from the score records of a FILTER_INLINE run -- on any machine, no GPU:

    python run_aug/filter_json.py <.../images> <dataset> [--top-k 10] [--too-high 0.9] [--discount 2] [--semantic | --no-semantic]

`filter_scores.json` beside the folder's aug JSONs holds threshold-free scores per augmented image (saspa_aug_amd/filters.py); every
choice of `conf_top_k`, `filter_confidence_higher_than`, `clip_filtering_discount` and semantic on / off is a lookup over them.  The
JSON gets the name and the body the filter stage itself would have written for those settings.  Which of the model-confidence and
per-class CLIP filters apply follows the sidecar (the one the run recorded; `--no-confidence` / `--no-per-class` switch it off).  An
image listed for the JSON without a record is an error: score it first (run the generation again with FILTER_INLINE, on a GPU)."""
import argparse
import json
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import saspa_aug_amd  # noqa: E402,F401


def main(argv=None, ds_utils=None):
    from saspa_aug_amd import dataset_utils, filters, utils
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("images", help="the run's images folder (its parent holds filter_scores.json)")
    ap.add_argument("dataset", help="dataset name (saspa_aug_amd.dataset_utils.DS_UTILS_DICT)")
    ap.add_argument("--top-k", type=int, default=10, help="conf_top_k of the model-confidence filter")
    ap.add_argument("--too-high", type=float, default=None, help="filter_confidence_higher_than")
    ap.add_argument("--discount", type=float, default=1, help="clip_filtering_discount of the per-class CLIP filter")
    ap.add_argument("--semantic", dest="semantic", action="store_true", default=None)
    ap.add_argument("--no-semantic", dest="semantic", action="store_false")
    ap.add_argument("--no-confidence", dest="confidence", action="store_false", default=None)
    ap.add_argument("--no-per-class", dest="per_class", action="store_false", default=None)
    ap.add_argument("--dataset-kwargs", default="{}", help="JSON keyword arguments of the dataset class (e.g. its root_path)")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    header = filters.load_scores(filters.scores_path(a.images))[0]
    if header is None:
        ap.exit(2, f"{filters.scores_path(a.images)} not found: the folder has no score records (generate it with FILTER_INLINE)\n")
    semantic = ("semantic" in header) if a.semantic is None else a.semantic
    confidence = ("confidence" in header) if a.confidence is None else a.confidence
    per_class = ("per_class" in header and not confidence) if a.per_class is None else a.per_class
    for on, key in ((semantic, "semantic"), (confidence, "confidence"), (per_class, "per_class")):
        if on and key not in header:
            ap.exit(2, f"the run recorded no {key} scores ({filters.scores_path(a.images)} lists {sorted(k for k in header if k in ('semantic', 'confidence', 'per_class'))})\n")
    if ds_utils is None:
        ds_utils = dataset_utils.DS_UTILS_DICT[a.dataset](**json.loads(a.dataset_kwargs))
    discount = int(a.discount) if float(a.discount).is_integer() else a.discount          # the file name says "discount_2", not "2.0"
    try:
        path = utils.create_json_of_image_name_to_augmented_images_paths(
            ds_utils, a.images, semantic_filtering=int(semantic), model_confidence_based_filtering=int(confidence), conf_top_k=a.top_k,
            filter_confidence_higher_than=a.too_high if confidence else None, clip_filtering="per_class" if per_class else False,
            clip_filtering_discount=discount, init_log=False, original_images_paths=ds_utils.original_images_paths, min_files=1, scores={},
            backfill=False)
    except FileNotFoundError as e:
        ap.exit(1, f"{e}\n")
    print(path)
    return path


if __name__ == "__main__":
    main()
