"""txt2sentence prompts (the reference's prompts_engineering/txt2sentance_prompts.py, its spelling kept): `num` sentences per class
from the T5 key-to-text generator (txt2sentence.T5Generator on the device), kept only when one of the dataset's must-keywords occurs in
them, written as {class: [sentences]} to LE_{num}_{dataset}_all_classes_{all_classes}.json -- the file PROMPT_TYPE = "txt2sentence"
(all_classes False, one general class list) and "txt2sentence-per_class" (all_classes True) read through Settings.PROMPTS_FILE.

Two deliberate differences from the reference:
  * the `num` samples of a class run as batches of one input (they share its encoder pass and cross K / V), not as `num` calls;
  * duplicates are removed in order of first appearance -- the reference's list(set(v)) order depends on the interpreter's hash seed.
The draws are this project's own (inverse-CDF on seeded uniforms), not torch.multinomial's stream."""
import json
import logging
from pathlib import Path

import torch

from .. import config as CFG
from .. import dataset_utils

T5_CONFIG = CFG.T5_COMMON_GEN            # tests swap in config.tiny_t5()

# one of the keywords must be in the sentence produced by the model (e.g. "car" for the cars dataset); the first one is the input
DATASET_TO_LABEL_DICT = {
    "planes": ["airplane", "plane", "aircraft", "jet", "aircraft"],
    "cars": ["car", "vehicle", "automobile", "auto", "motorcar"],
    "compcars": ["car", "vehicle", "automobile", "auto", "motorcar"],
    "compcars-parts": ["car", "vehicle", "automobile", "auto", "motorcar"],
    "cub": ["bird"],
    "dtd": ["texture"],
    "synthetic": ["airplane", "plane", "aircraft", "jet", "aircraft"],        # the seeded stand-in has the planes layout
}


def load_generator(weights_dir=None, device="cuda:0", dtype=torch.bfloat16):
    """The generator from a checkpoint directory; without one it refuses unless SASPA_SYNTHETIC_T5=1 (T5Generator.from_synthetic)."""
    from ..txt2sentence import T5Generator
    if weights_dir:
        return T5Generator.from_pretrained(weights_dir, device, dtype)
    gen = T5Generator.from_synthetic(T5_CONFIG, device, dtype)
    logging.warning("txt2sentence: SASPA_SYNTHETIC_T5=1 -> SYNTHETIC weights and a hash vocabulary; its sentences are those of a random model")
    return gen


def class_input(cls, all_classes, dataset):
    """The key-to-text input of a class, as the reference forms it."""
    if all_classes:
        return f"{DATASET_TO_LABEL_DICT[dataset][0]}, of type {cls}"
    return f"{cls}" if dataset == "compcars-parts" else f"{DATASET_TO_LABEL_DICT[dataset][0]}"


def word2sentence(classnames, num=200, save_path="", all_classes=False, must_keywords=(), dataset="", *, generator=None,
                  weights_dir=None, batch_size=64, seed=0, device="cuda:0", dtype=torch.bfloat16):
    """`num` sampled sentences per class -> {class: [kept sentences, duplicates removed in order]} written to save_path.  generator:
    anything with `sentences(list of inputs, do_sample=True, generator=torch.Generator) -> list of str` (default: load_generator).
    -> (the dict, counters)."""
    gen = generator if generator is not None else load_generator(weights_dir, device, dtype)
    rng = torch.Generator().manual_seed(seed)
    logging.info(f"Generating {num} sentences for each class: {classnames}")
    logging.info(f"Keywords that must be in the sentence: {must_keywords}")
    sentence_dict = {n: [] for n in classnames}
    skipped = 0
    for cls in classnames:
        inp = class_input(cls, all_classes, dataset)
        logging.info(f"Input for class {cls}: {inp}")
        done = 0
        while done < num:
            n = min(batch_size, num - done)
            for i, sentence in enumerate(gen.sentences([inp] * n, do_sample=True, generator=rng)):
                if done + i < 2:                                                     # 2 examples per class
                    logging.info(f" Example Input & Output for class: {cls}:\n input: {inp}\n output: {sentence}")
                if any(k in sentence.lower() for k in must_keywords):
                    sentence_dict[cls].append(sentence)
                else:
                    logging.info(f"Neither of the classes {must_keywords} is in the sentence: {sentence}, skipping...")
                    skipped += 1
            done += n
    counters = dict(num_skipped_due_to_no_class_in_sentence=skipped, total_sentences=sum(len(v) for v in sentence_dict.values()),
                    total_classes=len(sentence_dict))
    for k, v in counters.items():
        logging.info(f"{k}: {v}")
    sampled = {k: list(dict.fromkeys(v)) for k, v in sentence_dict.items()}          # ordered: no dependence on the hash seed
    with open(save_path, "w") as fp:
        json.dump(sampled, fp)
    return sampled, counters


def main(dataset, num, output_path, all_classes, *, generator=None, weights_dir=None, batch_size=64, seed=0, device="cuda:0",
         dtype=torch.bfloat16, dataset_kwargs=None, must_keywords=None):
    """Write LE_{num}_{dataset}_all_classes_{all_classes}.json under output_path; -> its path.  must_keywords: None = the dataset's
    (DATASET_TO_LABEL_DICT); a synthetic-weight run decodes to placeholder words ("t<id>") in which no real keyword can occur, so
    such a run passes its own (e.g. ["t"]) to keep anything."""
    assert dataset in DATASET_TO_LABEL_DICT and num > 0
    Path(output_path).mkdir(parents=True, exist_ok=True)
    save_path = Path(output_path) / f"LE_{num}_{dataset}_all_classes_{all_classes}.json"
    if not all_classes:
        if dataset == "compcars-parts":
            utils_to_use = dataset_utils.DS_UTILS_DICT[dataset](**(dataset_kwargs or {}))
            labels = [utils_to_use.get_basic_prompt(part) for part in range(1, 5)]
        else:
            labels = DATASET_TO_LABEL_DICT[dataset]
    else:
        labels = dataset_utils.DS_UTILS_DICT[dataset](**(dataset_kwargs or {})).get_classes()
    logging.info(f"Labels: {labels}")
    keywords = DATASET_TO_LABEL_DICT[dataset] if must_keywords is None else list(must_keywords)
    word2sentence(labels, num, str(save_path), all_classes=all_classes, must_keywords=keywords, dataset=dataset,
                  generator=generator, weights_dir=weights_dir, batch_size=batch_size, seed=seed, device=device, dtype=dtype)
    logging.info(f"saved to \n{save_path}")
    return str(save_path)
