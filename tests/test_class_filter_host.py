"""Host side of the Real-Guidance baseline's filter (no GPU): class prompts and class lists per dataset, the label of an original
image, the threshold, file and folder names from Settings, the entrypoint's defaults, what is still refused, the order in which
`apply_filters` attributes a dropped image, and the host-side validation of `saspa_class_head`."""
import ctypes as C
import importlib.util
import json
import logging
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, filters, utils
from saspa_aug_amd import dataset_utils as DU
from saspa_aug_amd import run_aug as R

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))
import dataset_fixtures as FX  # noqa: E402

quiet = lambda *a, **k: None   # noqa: E731


@pytest.fixture()
def tree(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the datasets' default roots are relative to the CWD
    return tmp_path


def test_class_prompts_and_class_lists_per_dataset(tree):
    FX.build_cars(tree)
    FX.build_dtd(tree)
    FX.build_cub(tree)
    FX.build_compcars(tree)
    syn = DU.SyntheticUtils(root_path=str(tree / "syn/data"), n_images=6, sizes=((16, 16),), print_func=quiet)
    classes, prompts = filters.class_prompts(syn)
    assert classes == sorted({"Boeing 707-320", "Airbus A320", "Cessna 172", "Embraer ERJ 145", "Boeing 747-400", "Airbus A380"})
    assert prompts[0] == "a photo of a Airbus A320, a type of aircraft." and len(prompts) == 6
    assert filters.CLASS_PROMPT_TEMPLATES["planes"] == filters.CLASS_PROMPT_TEMPLATES["synthetic"]
    classes, prompts = filters.class_prompts(DU.CarsUtils(print_func=quiet))
    assert classes == ["AM General Hummer SUV 2000", "Acura RL Sedan 2012", "Audi S4 Sedan 2012"]
    assert prompts[2] == "a photo of a Audi S4 Sedan 2012, a type of car."
    classes, prompts = filters.class_prompts(DU.DTDUtils(print_func=quiet))
    assert classes == sorted(set(classes)) and {"banded", "blotchy", "woven"} <= set(classes)
    assert prompts[classes.index("banded")] == "a photo of a banded, a type of texture."
    cub = DU.CUBUtils(print_func=quiet)
    classes, prompts = filters.class_prompts(cub)
    assert classes == sorted(set(cub.get_classes())) and len(classes) == len(prompts) > 1
    assert prompts[0] == f"a photo of a {classes[0]}, a type of a bird."
    parts = DU.CompCarsPartsUtils(print_func=quiet)
    classes, prompts = filters.class_prompts(parts)
    assert classes == sorted(parts.part_to_string.values())                 # the photographed PART, not the car model
    assert prompts == [f"a photo of the {c}, of a car." for c in classes]

    class Other:
        name = "imagenet"
    with pytest.raises(NotImplementedError, match="imagenet"):
        filters.class_prompts(Other())


def test_label_of_an_original_image(tree):
    FX.build_cars(tree)
    FX.build_dtd(tree)
    FX.build_compcars(tree)
    # planes / synthetic / cars: stem -> class string, looked up by the part of the stem in front of the first "_"
    syn = DU.SyntheticUtils(root_path=str(tree / "syn/data"), n_images=6, sizes=((16, 16),), print_func=quiet)
    classes, _ = filters.class_prompts(syn)
    table = syn.get_image_stem_to_class_str_dict()
    p0 = syn.original_images_paths[0]
    renamed = str(Path(p0).with_name(Path(p0).stem + "_flipped_2.png"))
    got = filters.class_labels(syn, [p0, renamed], classes)
    assert got == {Path(p0).name: classes.index(table[Path(p0).stem]), Path(renamed).name: classes.index(table[Path(p0).stem])}
    cars = DU.CarsUtils(print_func=quiet)
    classes, _ = filters.class_prompts(cars)
    table = cars.get_image_stem_to_class_str_dict()
    got = filters.class_labels(cars, cars.original_images_paths, classes)
    assert got == {Path(p).name: classes.index(table[Path(p).stem]) for p in cars.original_images_paths} and len(set(got.values())) == 3
    # the others: path -> class string
    dtd = DU.DTDUtils(print_func=quiet)
    classes, _ = filters.class_prompts(dtd)
    got = filters.class_labels(dtd, dtd.original_images_paths, classes)
    assert got == {Path(p).name: classes.index(Path(p).parent.name) for p in dtd.original_images_paths}
    parts = DU.CompCarsPartsUtils(print_func=quiet)
    classes, _ = filters.class_prompts(parts)
    got = filters.class_labels(parts, parts.original_images_paths, classes)
    assert got == {Path(p).name: classes.index(parts.part_to_string[Path(p).parent.name]) for p in parts.original_images_paths}


def test_threshold_arithmetic():
    assert filters.class_threshold(196) == 1 / 196
    assert filters.class_threshold(6, 2) == 1 / 6 / 2 == 1 / 12
    assert filters.class_threshold(431, 1.5) == 1 / 431 / 1.5
    assert filters.class_threshold(1) == 1.0              # one class: softmax == 1.0 >= 1.0 passes


def test_settings_file_and_folder_names(tmp_path, caplog):
    s = R.Settings()
    assert (s.CLIP_FILTERING_TYPE, s.CLIP_FILTERING_DISCOUNT, s.FOLDER_STEPS_GS_SUFFIX) == (None, 1, False)
    # unchanged without the new settings
    assert R.output_folder_for(s, "/r") == "/r/aug_data/controlnet/sd_v1.5/canny/gpt-meta_class_prompt_w_sub_class_artistic_prompts_p_0.5_seed_1/images"
    assert Path(utils.get_aug_json_path(R.output_folder_for(s, "/r"), semantic_filtering=1, model_confidence_based_filtering=1)).name == \
        "semantic_filtering-model_confidence_based_filtering_top_10_classes-aug.json"
    rg = R.Settings(DATASET="cars", CONTROLNET=None, SDEDIT=1, SDEDIT_STRENGTH=0.15, PROMPT_TYPE="txt2sentence", USE_ARTISTIC_PROMPTS=False,
                    NUM_INFERENCE_STEPS=50, FOLDER_STEPS_GS_SUFFIX=True)
    assert R.output_folder_for(rg, "/r") == \
        "/r/aug_data/regular/sd_v1.5-SDEdit_strength_0.15/None/txt2sentence_prompt_w_sub_class_seed_1_num_inf_steps_50_gs_7.5/images"
    rg.FOLDER_STEPS_GS_SUFFIX = False
    assert R.output_folder_for(rg, "/r").endswith("txt2sentence_prompt_w_sub_class_seed_1/images")
    # main announces the JSON name the settings give, before it generates
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=2, sizes=((64, 64),), print_func=quiet)
    s = R.Settings(DATASET="synthetic", NUM_PER_IMAGE=1, RESOLUTION=64, USE_ARTISTIC_PROMPTS=False, PROMPT_WITH_SUB_CLASS=False,
                   SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, CLIP_FILTERING_TYPE="per_class", CLIP_FILTERING_DISCOUNT=2)
    want = utils.get_aug_json_path(R.output_folder_for(s, ds.root_path), clip_filtering="per_class", clip_filtering_discount=2)
    assert Path(want).name == "clip_filtering_per_class_discount_2-aug.json"

    class Reached(Exception):
        pass

    def generator(*a, **k):
        raise Reached()
    with caplog.at_level(logging.INFO):
        with pytest.raises(Reached):
            R.main(s, ds_utils=ds, batch_generator=generator, class_filter=object())
    assert any(want in rec.getMessage() for rec in caplog.records)
    # the two filters that cannot be combined, and an unknown type, stop main before anything is generated
    s.MODEL_CONFIDENCE_BASED_FILTERING = 1
    with pytest.raises(AssertionError, match="both"):
        R.main(s, ds_utils=ds, batch_generator=generator, class_filter=object(), filter_models=(None, object()))
    s.MODEL_CONFIDENCE_BASED_FILTERING, s.CLIP_FILTERING_TYPE = 0, "per_image"
    with pytest.raises(NotImplementedError, match="per_class"):
        R.main(s, ds_utils=ds, batch_generator=generator)


def test_main_checks_the_clip_checkpoint_before_generating(tmp_path, monkeypatch):
    monkeypatch.delenv("SASPA_SYNTHETIC_FILTERS", raising=False)
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=2, sizes=((64, 64),), print_func=quiet)
    s = R.Settings(DATASET="synthetic", NUM_PER_IMAGE=1, RESOLUTION=64, USE_ARTISTIC_PROMPTS=False, PROMPT_WITH_SUB_CLASS=False,
                   SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, CLIP_FILTERING_TYPE="per_class")

    def generator(*a, **k):
        raise AssertionError("the batch generator must not be touched")
    with pytest.raises(FileNotFoundError, match="per-class CLIP filter"):
        R.main(s, ds_utils=ds, batch_generator=generator)
    with pytest.raises(FileNotFoundError, match="per-class CLIP filter"):
        filters.filter_checkpoints(ds, str(tmp_path / "w"), semantic=False, confidence=False, per_class=True)
    (tmp_path / "w/clip").mkdir(parents=True)
    (tmp_path / "w/clip/RN50.pt").write_bytes(b"x")
    assert filters.filter_checkpoints(ds, str(tmp_path / "w"), False, False, per_class=True) == (str(tmp_path / "w/clip/RN50.pt"), None)
    monkeypatch.setenv("SASPA_SYNTHETIC_FILTERS", "1")
    assert filters.filter_checkpoints(ds, None, False, False, per_class=True) == (None, None)


def test_real_guidance_entrypoint_defaults():
    spec = importlib.util.spec_from_file_location("run_aug_real_guidance", HERE.parent / "run_aug" / "run_aug_real_guidance.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # importing it starts nothing
    s = mod.real_guidance_settings({})
    assert (s.DATASET, s.BASE_MODEL, s.CONTROLNET, s.SDEDIT, s.SDEDIT_STRENGTH) == ("cars", "sd_v1.5", None, 1, 0.15)
    assert (s.PROMPT_TYPE, s.USE_ARTISTIC_PROMPTS, s.NUM_INFERENCE_STEPS) == ("txt2sentence", False, 50)
    assert (s.CLIP_FILTERING_TYPE, s.CLIP_FILTERING_DISCOUNT, s.SEMANTIC_FILTERING, s.MODEL_CONFIDENCE_BASED_FILTERING) == ("per_class", 1, 0, 0)
    assert s.FOLDER_STEPS_GS_SUFFIX is True and s.LPIPS_MIN is None and s.LPIPS_MAX is None
    assert R.output_folder_for(s, "/r").endswith("/regular/sd_v1.5-SDEdit_strength_0.15/None/txt2sentence_prompt_w_sub_class_seed_1_num_inf_steps_50_gs_7.5/images")
    s = mod.real_guidance_settings({"SASPA_DATASET": "planes", "SASPA_NUM_INFERENCE_STEPS": "20", "SASPA_CLIP_FILTERING_DISCOUNT": "2",
                                    "SASPA_NUM_PER_IMAGE": "3", "SASPA_WEIGHTS_DIR": "/w", "SASPA_LPIPS_MIN": "0.1", "SASPA_LPIPS_MAX": "0.6"})
    assert (s.DATASET, s.NUM_INFERENCE_STEPS, s.CLIP_FILTERING_DISCOUNT, s.NUM_PER_IMAGE, s.WEIGHTS_DIR) == ("planes", 20, 2.0, 3, "/w")
    assert (s.LPIPS_MIN, s.LPIPS_MAX) == (0.1, 0.6)
    assert mod.real_guidance_settings({"SASPA_CLIP_FILTERING": "none"}).CLIP_FILTERING_TYPE is None


def test_what_is_still_refused_and_what_no_longer_is(tmp_path):
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=2, sizes=((16, 16),), print_func=quiet)
    folder = tmp_path / "aug/images"
    folder.mkdir(parents=True)
    for kw in (dict(clip_filtering=True), dict(clip_filtering="per_image"), dict(alia_conf_filtering=True)):
        with pytest.raises(NotImplementedError):
            utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, **kw)
    with pytest.raises(AssertionError):
        utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, clip_filtering="per_class",
                                                                  model_confidence_based_filtering=1)
    assert not list(folder.parent.glob("*.json")) and not list(folder.parent.glob("*.log")), "nothing is written before a refusal"
    # "per_class" gets past the refusals (and stops at the empty folder)
    with pytest.raises(FileNotFoundError, match="less than"):
        utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, clip_filtering="per_class",
                                                                  class_filter=object())


class _Fake:
    """Stand-in filter deciding from the grey level of the image; records what it was handed."""

    def __init__(self, fn, too_high=None, class_names=None, visual=None):
        self.fn, self.calls = fn, []
        if too_high is not None:
            self.too_high = too_high
        if class_names is not None:
            self.class_names, self.threshold = class_names, filters.class_threshold(len(class_names), 2)
        self.visual = visual

    def embed(self, batch):
        self.calls.append("embed")
        return batch.float().mean(dim=(1, 2, 3))

    def passes(self, batch, labels=None, embedding=None):
        self.calls.append(("passes", None if labels is None else list(labels), embedding is not None))
        m = batch.float().mean(dim=(1, 2, 3)).numpy()
        out = [self.fn(v) for v in m]
        if isinstance(out[0], tuple):
            return np.array([a for a, _ in out]), np.array([b for _, b in out])
        return np.array(out)


def test_apply_filters_order_of_attribution_and_shared_tower(tmp_path, monkeypatch, caplog):
    """top-k / too-high, (LPIPS,) per-class CLIP, semantic: a dropped image is counted once, under the first filter that drops it;
    two CLIP filters on one image tower get one `embed` per batch."""
    root = tmp_path / "ds/data"
    ds = DU.SyntheticUtils(root_path=str(root), n_images=2, sizes=((16, 16),), print_func=quiet)
    folder = root / "aug/images"
    folder.mkdir(parents=True)
    stems = [Path(p).stem for p in ds.original_images_paths]
    levels = [10, 60, 110, 160, 210]
    for stem in stems:
        for v, lv in enumerate(levels):
            Image.fromarray(np.full((16, 16, 3), lv, np.uint8)).save(folder / f"{stem}_prompt_x_{v}.png")
    monkeypatch.setattr(filters.ops, "h2d", lambda t, dev, dtype=None: t)
    classes, _ = filters.class_prompts(ds)
    want_labels = filters.class_labels(ds, ds.original_images_paths, classes)
    tower = object()
    conf = _Fake(lambda v: (v > 50, v > 50 and v > 200), too_high=0.9)     # drops level 10 (top-k) and level 210 (too sure)
    cls = _Fake(lambda v: v > 100, class_names=classes, visual=tower)      # would drop 10 and 60: only 60 is its own
    sem = _Fake(lambda v: v < 150, visual=tower)                           # would drop 160 and 210: only 160 is its own
    mapping = utils.match_augmented_images(ds.original_images_paths, sorted(p.name for p in folder.iterdir()), str(folder))
    out, counters = filters.apply_filters(mapping, ds.original_images_paths, ds, "cpu", sem, conf, class_filter=cls)
    assert counters == dict(not_in_top_k=2, too_high_confidence=2, clip_filtering=2, semantic=2)
    assert {k: [Path(p).name for p in v] for k, v in out.items()} == {f"{s}.png": [f"{s}_prompt_x_2.png"] for s in stems}
    assert cls.calls[0] == "embed" and cls.calls.count("embed") == 1 and "embed" not in sem.calls
    kind, labels, had_embedding = cls.calls[1]
    assert had_embedding and labels == [want_labels[f"{s}.png"] for s in stems for _ in levels]
    assert sem.calls == [("passes", None, True)]
    # separate towers: no shared embedding; without too_high / class filter the counters keep their old keys
    sem2, cls2 = _Fake(lambda v: v < 150, visual=object()), _Fake(lambda v: v > 100, class_names=classes, visual=object())
    _, counters = filters.apply_filters(mapping, ds.original_images_paths, ds, "cpu", sem2, None, class_filter=cls2)
    assert counters == dict(not_in_top_k=0, semantic=4, clip_filtering=4) and "embed" not in cls2.calls
    assert sem2.calls == [("passes", None, False)]
    # through create_json: file name, log lines, and a confidence model built with another bound is refused
    with caplog.at_level(logging.INFO):
        jp = utils.create_json_of_image_name_to_augmented_images_paths(
            ds, str(folder), semantic_filtering=1, clip_filtering="per_class", clip_filtering_discount=2, init_log=False,
            original_images_paths=ds.original_images_paths, min_files=1, filter_models=(sem, None), class_filter=cls, device="cpu")
    assert Path(jp).name == "clip_filtering_per_class_discount_2-semantic_filtering-aug.json"
    assert sorted(len(v) for v in json.load(open(jp)).values()) == [1, 1]
    msgs = [r.getMessage() for r in caplog.records]
    assert "For filter = clip_filtering, filtered 4 images" in msgs and "For filter = semantic_filtering, filtered 4 images" in msgs
    caplog.clear()
    with caplog.at_level(logging.INFO):
        jp = utils.create_json_of_image_name_to_augmented_images_paths(
            ds, str(folder), model_confidence_based_filtering=1, conf_top_k=3, filter_confidence_higher_than=0.9, init_log=False,
            original_images_paths=ds.original_images_paths, min_files=1, filter_models=(None, conf), device="cpu")
    assert Path(jp).name == "model_confidence_based_filtering_top_3_classes-filter_confidence_higher_than_0.9-aug.json"
    msgs = [r.getMessage() for r in caplog.records]
    assert "For filter = not_in_top_3, filtered 2 images" in msgs and "For filter = too_high_confidence, filtered 2 images" in msgs
    with pytest.raises(ValueError, match="too_high"):
        utils.create_json_of_image_name_to_augmented_images_paths(
            ds, str(folder), model_confidence_based_filtering=1, filter_confidence_higher_than=0.5, init_log=False,
            original_images_paths=ds.original_images_paths, min_files=1, filter_models=(None, conf), device="cpu")


def test_class_head_is_exported_and_validates_on_the_host():
    lib = _lib.load()
    assert "saspa_class_head" in _lib.SYMBOLS and hasattr(lib, "saspa_class_head")
    assert lib.saspa_abi_version() == 20
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) // 16 * 16
    feat, cls, labels, stats, idx, logits = base, base + 16, base + 32, base + 48, base + 64, base + 80

    def call(feat=feat, ldf=1024, cls=cls, ldc=1024, labels=labels, stats=stats, idx=idx, logits=None, ldl=0, rows=2, D=1024, C_=431):
        return lib.saspa_class_head(feat, ldf, cls, ldc, labels, 100.0, 1, stats, idx, logits, ldl, rows, D, C_, None)
    # null pointers (cls may be null: that is logits mode)
    for kw in (dict(feat=None), dict(labels=None), dict(stats=None), dict(idx=None), dict(rows=0)):
        assert call(**kw) == _lib.SASPA_EINVAL, kw
    # 16-byte operands and pitches
    for kw in (dict(feat=feat + 4), dict(cls=cls + 8), dict(ldf=1026), dict(ldc=1030), dict(ldf=1020), dict(ldc=512),
               dict(logits=logits + 4, ldl=432), dict(logits=logits, ldl=431), dict(logits=logits, ldl=428), dict(stats=stats + 2),
               dict(idx=idx + 1), dict(labels=labels + 3)):
        assert call(**kw) == _lib.SASPA_EALIGN, kw
    # what the LDS plan holds, and D == C in logits mode
    assert _lib.CLASS_HEAD_MAX_D >= 1024 and _lib.CLASS_HEAD_MAX_C >= 431
    for kw in (dict(C_=0), dict(D=0), dict(D=_lib.CLASS_HEAD_MAX_D + 4, ldf=4096, ldc=4096), dict(C_=_lib.CLASS_HEAD_MAX_C + 1),
               dict(cls=None, D=196, C_=200, ldf=200)):
        assert call(**kw) == _lib.SASPA_ERANGE, kw
    src = open(HERE.parent / "include" / "saspa_hip.h").read()
    assert f"#define SASPA_CLASS_HEAD_MAX_D {_lib.CLASS_HEAD_MAX_D}\n" in src and f"#define SASPA_CLASS_HEAD_MAX_C {_lib.CLASS_HEAD_MAX_C}\n" in src
