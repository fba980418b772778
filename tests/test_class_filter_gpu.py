"""The per-class CLIP filter and the too-high-confidence bound on the MI355X, end to end through
`create_json_of_image_name_to_augmented_images_paths`: reduced-width CLIP RN50 / WSDAN_CAL with synthetic weights on the device
against the ORACLE models on the CPU (PIL pre-processing, torch-CPU networks, float64 softmax).

Set-up as in test_filters_gpu.test_filter_decisions_and_json_end_to_end: 6 synthetic originals of 6 classes, three augmentations
each, the third at 96 x 128 so that two size groups exist; cal seed 32, HashTokenizer.  The CLIP weights use seed 37, not that
test's 31: with the dataset's real class strings ("a photo of a Boeing 707-320, a type of aircraft." ...) seed 31 puts every
probability at 0 or 1 (one prompt wins for all 18 images, the semantic filter keeps none), so no discount could split the images
differently.  A CPU probe over seeds 1..79 picked 37: per-class probabilities from 7e-7 to 0.90, 5 images kept at 1/6 and 8 at 1/18
(nearest approaches 41 % and 26 %), the semantic filter keeps 12 of 18 (smallest argmax margin 0.011 in logits); the classifier's
softmax(label) among the 6 images that pass top-3 is 0.005 .. 0.987, so 0.5 splits them 3 / 3 (nearest approach 86 %).

The expected decisions come from the oracle alone, and the test first asserts ON THE ORACLE VALUES that none of them lies within
MARGIN = 3 % (relative) of the threshold it is compared with: 1/6 (discount 1), 1/6/DISCOUNT_2 and TOO_HIGH.

Model-level difference  max |p_dev - p_oracle| / p_oracle  over the 18 images, measured on the MI355X: see MEASURED_REL below; the
bound of the test is 10 x that (the factor covers the torch-CPU oracle's own summation order across builds) and must stay below a
third of the smallest oracle margin, which the test asserts as well."""
import json
import logging
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from oracle import filter_models as FM
from saspa_aug_amd import config as CFG
from saspa_aug_amd import dataset_utils as DU
from saspa_aug_amd import filters, utils
from saspa_aug_amd import weights as W
from saspa_aug_amd.synthetic import synthetic_image
from saspa_aug_amd.tokenizer import HashTokenizer

pytestmark = pytest.mark.gpu
MARGIN = 0.03
DISCOUNT_2 = 3            # the second discount: 1/18 splits the 18 images differently from 1/6
TOO_HIGH = 0.5            # filter_confidence_higher_than
TOP_K = 3
CLIP_SEED, CAL_SEED = 37, 32
MEASURED_REL = 1.162e-5       # max |p_dev - p_oracle| / p_oracle measured on the MI355X (per-class CLIP probabilities, 18 images)
MEASURED_REL_CAL = 8.619e-5   # the same for the classifier's softmax(label) among the images that pass top-k


class Case:
    """Files on disk, the models' weights and the oracle's values, built once per session."""

    def __init__(self, tmp, clip_seed=CLIP_SEED, cal_seed=CAL_SEED):
        self.cf = cf = CFG.tiny_filters(num_classes=6)
        root = tmp / "ds/data"
        self.ds = ds = DU.SyntheticUtils(root_path=str(root), n_images=6, sizes=((64, 64),), print_func=lambda *a, **k: None)
        self.folder = folder = root / "aug_data/regular/sd_v1.5-SDEdit_strength_0.15/None/run_seed_1_num_inf_steps_50_gs_7.5/images"
        folder.mkdir(parents=True)
        self.files = files = {}
        for k, p in enumerate(ds.original_images_paths):
            stem = Path(p).stem
            for v in range(3):
                img = synthetic_image(64 if v < 2 else 96, 64 if v < 2 else 128, 100 + 10 * k + v)
                name = f"{stem}_prompt_An airplane, oil painting_{v}.png"
                Image.fromarray(img).save(folder / name)
                files[str(folder / name)] = (Path(p).name, img)
            Image.fromarray(synthetic_image(64, 64, k)).save(folder / f"{stem}_source.png")
        self.sd_c, self.sd_w = W.synth_state_dict("clip_rn50", cf["clip_rn50"], clip_seed), W.synth_state_dict("cal", cf["cal"], cal_seed)
        self.tok = tok = HashTokenizer(cf["clip_rn50"]["vocab"], pad_id=0)
        self.classes, self.prompts = filters.class_prompts(ds)
        self.cls_label = filters.class_labels(ds, ds.original_images_paths, self.classes)
        cal_label = ds.get_image_path_to_class_id_dict()
        self.cal_label = {Path(p).name: cal_label[p] for p in ds.original_images_paths}
        ids_cls = torch.from_numpy(np.concatenate([tok(pr) for pr in self.prompts]))
        ids_sem = torch.from_numpy(np.concatenate([tok(pr) for pr in [ds.get_basic_prompt()] + filters.NEGATIVE_PROMPTS]))
        self.p_cls, self.ok_s, self.in_top_k, self.p_cal, self.sem_gap = {}, {}, {}, {}, {}
        for path, (orig, img) in files.items():
            with torch.no_grad():
                px = FM.rn50_preprocess(img, 64)[None]
                lg = FM.clip_selector_logits(self.sd_c, cf["clip_rn50"], px, ids_cls)[0].double()
                lg_s = FM.clip_selector_logits(self.sd_c, cf["clip_rn50"], px, ids_sem)[0]
                lg_c = FM.wsdan_cal_logits(self.sd_w, cf["cal"], FM.cal_preprocess(img, (64, 64))[None])[0]
            self.p_cls[path] = float(torch.softmax(lg, -1)[self.cls_label[orig]])
            self.ok_s[path] = bool(FM.semantic_pass(lg_s[None])[0])
            self.sem_gap[path] = float(lg_s[0] - lg_s[1:].max())           # the semantic decision is an argmax: its margin, in logits
            self.in_top_k[path] = FM.confidence_pass(lg_c[None], self.cal_label[orig], TOP_K)
            self.p_cal[path] = float(torch.softmax(lg_c.double(), -1)[self.cal_label[orig]])

    def margins(self):
        """Relative distance of every oracle value from the threshold it meets: (1/6, 1/6/DISCOUNT_2, TOO_HIGH among top-k)."""
        t1, t2 = filters.class_threshold(6, 1), filters.class_threshold(6, DISCOUNT_2)
        m1 = min(abs(p - t1) / t1 for p in self.p_cls.values())
        m2 = min(abs(p - t2) / t2 for p in self.p_cls.values())
        mh = min(abs(self.p_cal[k] - TOO_HIGH) / TOO_HIGH for k in self.files if self.in_top_k[k])
        return m1, m2, mh

    def expected(self, discount=None, semantic=False, conf=False, too_high=None):
        """(JSON body, counters) by the reference's order: top-k / too-high, per-class CLIP, semantic."""
        want = {Path(p).name: [] for p in self.ds.original_images_paths}
        n = dict(not_in_top_k=0, too_high_confidence=0, clip_filtering=0, semantic=0)
        for path, (orig, _) in self.files.items():
            if conf and not self.in_top_k[path]:
                n["not_in_top_k"] += 1
            elif conf and too_high and self.p_cal[path] > too_high:
                n["too_high_confidence"] += 1
            elif discount and not self.p_cls[path] >= filters.class_threshold(6, discount):
                n["clip_filtering"] += 1
            elif semantic and not self.ok_s[path]:
                n["semantic"] += 1
            else:
                want[orig].append(path)
        return {k: sorted(v) for k, v in want.items()}, n


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("class_filter"))


@pytest.fixture(scope="module")
def models(case, dev):
    cfg = case.cf["clip_rn50"]
    template = filters.CLASS_PROMPT_TEMPLATES["synthetic"]
    cls = {1: filters.ClassFilter(case.sd_c, cfg, dev, case.classes, template, case.tok, discount=1)}
    cls[DISCOUNT_2] = filters.ClassFilter(case.sd_c, cfg, dev, case.classes, template, case.tok, discount=DISCOUNT_2, visual=cls[1].visual)
    sem = filters.SemanticFilter(case.sd_c, cfg, dev, case.ds.get_basic_prompt(), case.tok, visual=cls[1].visual)
    conf = filters.ConfidenceFilter(case.sd_w, case.cf["cal"], dev, top_k=TOP_K, too_high=TOO_HIGH)
    return cls, sem, conf


def _counters(caplog):
    out = {}
    for rec in caplog.records:
        m = re.match(r"For filter = (\w+), filtered (\d+) images", rec.getMessage())
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def test_oracle_values_keep_their_distance_from_the_thresholds(case):
    m1, m2, mh = case.margins()
    print(f"oracle: p_class in [{min(case.p_cls.values()):.4f}, {max(case.p_cls.values()):.4f}], nearest to 1/6: {m1:.3f}, "
          f"to 1/6/{DISCOUNT_2}: {m2:.3f}; softmax(label) of the classifier in [{min(case.p_cal.values()):.4f}, "
          f"{max(case.p_cal.values()):.4f}], nearest to {TOO_HIGH} among top-{TOP_K}: {mh:.3f}")
    assert min(m1, m2, mh) >= MARGIN
    # every filter both keeps and drops, and the two discounts split differently
    for d in (1, DISCOUNT_2):
        n = case.expected(discount=d)[1]["clip_filtering"]
        assert 0 < n < len(case.files), d
    assert case.expected(discount=1)[0] != case.expected(discount=DISCOUNT_2)[0]
    n = case.expected(conf=True, too_high=TOO_HIGH)[1]
    assert n["not_in_top_k"] > 0 and n["too_high_confidence"] > 0 and n["not_in_top_k"] + n["too_high_confidence"] < len(case.files)
    n = case.expected(discount=DISCOUNT_2, semantic=True)[1]
    assert n["clip_filtering"] > 0 and n["semantic"] > 0 and n["clip_filtering"] + n["semantic"] < len(case.files)


def test_probabilities_against_the_oracle(case, models, dev):
    """max |p_dev - p_oracle| / p_oracle, printed, and bounded by 10 x the value measured on the MI355X; the bound stays below a
    third of the smallest oracle margin."""
    cls, _, conf = models
    rel, rel_cal = 0.0, 0.0
    for path, (orig, img) in case.files.items():
        batch = torch.from_numpy(img)[None].to(dev)
        p = float(cls[1].probs(batch, [case.cls_label[orig]]).cpu()[0])
        rel = max(rel, abs(p - case.p_cls[path]) / case.p_cls[path])
        in_k, high = conf.passes(batch, [case.cal_label[orig]])
        assert bool(in_k[0]) == case.in_top_k[path]
        if case.in_top_k[path]:
            lg = conf.logits(batch).float()
            st, _, _ = filters.ops.class_head(lg, torch.tensor([case.cal_label[orig]], dtype=torch.int32, device=dev), width=6)
            rel_cal = max(rel_cal, abs(float(st[0, 1]) - case.p_cal[path]) / case.p_cal[path])
    print(f"measured: per-class CLIP max |dp| / p = {rel:.3e}; classifier softmax(label) max |dp| / p = {rel_cal:.3e}")
    m1, m2, mh = case.margins()
    assert 10 * MEASURED_REL < min(m1, m2) / 3 and 10 * MEASURED_REL_CAL < mh / 3
    # d ln p = dz_label - sum_c p_c dz_c: the relative error of p IS the error of the logits, so the same bound guards the argmax
    assert 10 * MEASURED_REL < min(abs(g) for g in case.sem_gap.values()) / 3
    assert rel <= 10 * MEASURED_REL, (rel, MEASURED_REL)
    assert rel_cal <= 10 * MEASURED_REL_CAL, (rel_cal, MEASURED_REL_CAL)


@pytest.mark.parametrize("discount", [1, DISCOUNT_2])
def test_per_class_json_counters_and_name(case, models, dev, caplog, discount):
    cls, _, _ = models
    with caplog.at_level(logging.INFO):
        jp = utils.create_json_of_image_name_to_augmented_images_paths(
            case.ds, str(case.folder), clip_filtering="per_class", clip_filtering_discount=discount, init_log=False,
            original_images_paths=case.ds.original_images_paths, min_files=1, class_filter=cls[discount], device=dev)
    assert Path(jp).name == f"clip_filtering_per_class_discount_{discount}-aug.json"
    want, n = case.expected(discount=discount)
    assert {k: sorted(v) for k, v in json.load(open(jp)).items()} == want
    assert _counters(caplog) == dict(clip_filtering=n["clip_filtering"])
    assert any(f"using CLIP filtering with threshold = {1 / 6 / discount}" in r.getMessage() for r in caplog.records)


def test_per_class_with_semantic_shares_one_visual_pass(case, models, dev, caplog, monkeypatch):
    cls, sem, _ = models
    assert sem.visual is cls[DISCOUNT_2].visual
    calls = []
    forward = sem.visual.forward
    monkeypatch.setattr(sem.visual, "forward", lambda px: (calls.append(px.shape[0]), forward(px))[1])
    with caplog.at_level(logging.INFO):
        jp = utils.create_json_of_image_name_to_augmented_images_paths(
            case.ds, str(case.folder), clip_filtering="per_class", clip_filtering_discount=DISCOUNT_2, semantic_filtering=1, init_log=False,
            original_images_paths=case.ds.original_images_paths, min_files=1, filter_models=(sem, None), class_filter=cls[DISCOUNT_2],
            device=dev)
    assert Path(jp).name == f"clip_filtering_per_class_discount_{DISCOUNT_2}-semantic_filtering-aug.json"
    want, n = case.expected(discount=DISCOUNT_2, semantic=True)
    assert {k: sorted(v) for k, v in json.load(open(jp)).items()} == want
    assert _counters(caplog) == dict(clip_filtering=n["clip_filtering"], semantic_filtering=n["semantic"])
    assert sorted(calls) == [6, 12], "one image-tower pass per batch (two size groups), not one per filter"


def test_top_k_with_too_high_confidence(case, models, dev, caplog):
    _, _, conf = models
    with caplog.at_level(logging.INFO):
        jp = utils.create_json_of_image_name_to_augmented_images_paths(
            case.ds, str(case.folder), model_confidence_based_filtering=1, conf_top_k=TOP_K, filter_confidence_higher_than=TOO_HIGH,
            init_log=False, original_images_paths=case.ds.original_images_paths, min_files=1, filter_models=(None, conf), device=dev)
    assert Path(jp).name == f"model_confidence_based_filtering_top_{TOP_K}_classes-filter_confidence_higher_than_{TOO_HIGH}-aug.json"
    want, n = case.expected(conf=True, too_high=TOO_HIGH)
    assert {k: sorted(v) for k, v in json.load(open(jp)).items()} == want
    assert _counters(caplog) == {f"not_in_top_{TOP_K}": n["not_in_top_k"], "too_high_confidence": n["too_high_confidence"]}
    # too_high = None is the unchanged host path: one mask, the same top-k decisions
    plain = filters.ConfidenceFilter.__new__(filters.ConfidenceFilter)
    plain.__dict__.update(conf.__dict__, too_high=None)
    for path, (orig, img) in list(case.files.items())[:6]:
        one = plain.passes(torch.from_numpy(img)[None].to(dev), [case.cal_label[orig]])
        assert isinstance(one, np.ndarray) and bool(one[0]) == case.in_top_k[path]
