"""The in-line filter stage, host side (no GPU): `filters.decide` against `filters.apply_filters` run with torch-CPU oracle models over
a grid of settings, the score sidecar (exact fp32 / NaN round trip, stale records, header mismatch, merge on resume), the JSON written
from records by `create_json_of_image_name_to_augmented_images_paths(scores=...)` and by run_aug/filter_json.py, its refusal of a
missing record, FILTER_INLINE's refusals in `run_aug.main`, and the records gather at two ranks over gloo."""
import hashlib
import importlib.util
import itertools
import json
import logging
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from PIL import Image

import saspa_aug_amd  # noqa: F401
from oracle import filter_models as FM
from saspa_aug_amd import config as CFG
from saspa_aug_amd import dataset_utils as DU
from saspa_aug_amd import filters, utils
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import weights as W
from saspa_aug_amd.tokenizer import HashTokenizer

import filter_record_ref as REF

HERE = Path(__file__).resolve().parent
quiet = lambda *a, **k: None   # noqa: E731
C = 6                          # classes of the synthetic dataset = classes of the tiny classifier


# ---------------------------------------------------------------------------------------------------------------------
# torch-CPU oracle models (oracle/filter_models.py) behind the interfaces `apply_filters` calls
# ---------------------------------------------------------------------------------------------------------------------
class _Clip:
    def __init__(self, prompts, seed=31):
        self.cfg = CFG.tiny_filters(C)["clip_rn50"]
        self.sd = W.synth_state_dict("clip_rn50", self.cfg, seed)
        tok = HashTokenizer(self.cfg["vocab"], pad_id=0)
        self.prompts, self.dtype, self.dev = list(prompts), torch.float32, "cpu"
        self.ids = torch.from_numpy(np.concatenate([tok(p) for p in self.prompts])).long()
        self.visual = self
        self.calls = 0

    @torch.no_grad()
    def logits(self, batch, embedding=None):
        self.calls += 1
        px = torch.stack([FM.rn50_preprocess(im.numpy(), self.cfg["image_size"]) for im in batch])
        return FM.clip_selector_logits(self.sd, self.cfg, px, self.ids).float()


class SemOracle(_Clip):
    def passes(self, batch, embedding=None):
        return np.argmax(self.logits(batch).numpy(), axis=-1) == 0


class ClassOracle(_Clip):
    def __init__(self, class_names, discount):
        super().__init__([filters.CLASS_PROMPT_TEMPLATES["synthetic"].format(name=c) for c in class_names], seed=33)
        self.class_names, self.discount = list(class_names), discount
        self.threshold = filters.class_threshold(len(class_names), discount)
        self.scale = float(self.sd["logit_scale"].float().exp())

    def probs(self, batch, labels):
        p = torch.softmax(self.logits(batch), -1)
        return p[torch.arange(len(labels)), torch.as_tensor(labels).long()].numpy()

    def passes(self, batch, labels, embedding=None):
        return self.probs(batch, labels).astype(np.float64) >= self.threshold


class ConfOracle:
    def __init__(self, top_k, too_high=None):
        self.cfg = CFG.tiny_filters(C)["cal"]
        self.sd = W.synth_state_dict("cal", self.cfg, 32)
        self.top_k, self.too_high, self.dtype, self.dev = min(int(top_k), C), too_high or None, torch.float32, "cpu"
        self.model = type("M", (), dict(num_classes=C))()

    @torch.no_grad()
    def logits(self, batch):
        s = self.cfg["image_size"]
        return FM.wsdan_cal_logits(self.sd, self.cfg, torch.stack([FM.cal_preprocess(im.numpy(), (s, s)) for im in batch])).float()

    def passes(self, batch, labels):
        lg = self.logits(batch)
        ng = np.array([int((row > row[int(lb)]).sum()) for lb, row in zip(labels, lg.numpy())])
        if self.too_high is None:
            return ng < self.top_k
        p = torch.softmax(lg, -1)[torch.arange(len(labels)), torch.as_tensor(labels).long()].numpy()
        return ng < self.top_k, (p.astype(np.float64) > self.too_high) & (ng < self.top_k)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """3 originals x 4 augmented PNGs of random pixels, the oracle models' logits for every PNG, and the records the numpy
    restatement makes of them.  Computed once; nothing below changes it."""
    root = tmp_path_factory.mktemp("scores") / "ds/data"
    ds = DU.SyntheticUtils(root_path=str(root), n_images=3, sizes=((64, 64),), print_func=quiet)
    folder = root / "aug_data/controlnet/sd_v1.5/canny/run_seed_1/images"
    folder.mkdir(parents=True)
    rng = np.random.RandomState(5)
    for p in ds.original_images_paths:
        for v in range(4):
            base = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
            Image.fromarray(np.kron(base, np.ones((8, 8, 1), np.uint8))).save(folder / f"{Path(p).stem}_prompt_an airplane_{v}.png")
        Image.fromarray(np.full((64, 64, 3), 7, np.uint8)).save(folder / f"{Path(p).stem}_source.png")
    mapping = utils.match_augmented_images(ds.original_images_paths, sorted(os.listdir(folder)), str(folder))
    classes, _ = filters.class_prompts(ds)
    sem, cls, conf = SemOracle([ds.get_basic_prompt()] + filters.NEGATIVE_PROMPTS), ClassOracle(classes, 1), ConfOracle(3)
    conf_lb = {Path(p).name: ds.get_image_path_to_class_id_dict()[p] for p in ds.original_images_paths}
    pc_lb = filters.class_labels(ds, ds.original_images_paths, classes)
    records = {}
    for name, aps in mapping.items():
        for ap in aps:
            px = torch.from_numpy(filters._load_u8(ap).copy())[None]
            cl, pl = conf.logits(px)[0].numpy(), cls.logits(px)[0]
            p_conf = torch.softmax(torch.from_numpy(cl), -1)[conf_lb[name]].numpy()
            p_pc = torch.softmax(pl, -1)[pc_lb[name]].numpy()
            records[Path(ap).name] = REF.record(sem.logits(px)[0].numpy(), (p_conf, REF.class_head_pair(cl, conf_lb[name])[1]),
                                                (p_pc, REF.class_head_pair(pl.numpy(), pc_lb[name])[1]))
    return dict(ds=ds, folder=folder, mapping=mapping, classes=classes, sem=sem, records=records)


def test_decide_equals_apply_filters_over_the_grid(scene, monkeypatch):
    monkeypatch.setattr(filters.ops, "h2d", lambda t, dev, dtype=None: t)
    ds, mapping, records = scene["ds"], scene["mapping"], scene["records"]
    work = [ap for aps in mapping.values() for ap in aps]
    rec = np.stack([records[Path(ap).name] for ap in work])
    assert rec.shape == (12, 8) and (rec[:, 0] == 7).all()
    seen = set()
    for top_k, too_high, discount, semantic in itertools.product((1, 3, C), (None, 0.2, 0.9), (1, 2), (True, False)):
        conf, cls = ConfOracle(top_k, too_high), ClassOracle(scene["classes"], discount)
        want, want_counters = filters.apply_filters(mapping, ds.original_images_paths, ds, "cpu", scene["sem"] if semantic else None, conf,
                                                    class_filter=cls)
        keep, counters = filters.decide(rec, semantic=semantic, top_k=top_k, too_high=too_high, pc_threshold=cls.threshold)
        kept = {ap for ap, k in zip(work, keep) if k}
        assert {n: [ap for ap in aps if ap in kept] for n, aps in mapping.items()} == want, (top_k, too_high, discount, semantic)
        assert counters == want_counters, (top_k, too_high, discount, semantic)
        seen.add(tuple(sorted(counters.items())))
    assert len(seen) > 4, "the grid never changed a decision: the scene is too tame to test anything"
    # one filter at a time: the counters keep the keys of `apply_filters`
    _, counters = filters.decide(rec, semantic=True, top_k=None, too_high=None, pc_threshold=None)
    assert set(counters) == {"not_in_top_k", "semantic"} and counters["not_in_top_k"] == 0
    _, want_counters = filters.apply_filters(mapping, ds.original_images_paths, ds, "cpu", scene["sem"], None)
    assert counters == want_counters
    # a record that lacks what an enabled filter needs is refused, not guessed
    part = rec.copy()
    part[3] = REF.record(sem=rec[3, :1])                   # semantic only
    with pytest.raises(ValueError, match="lack a score"):
        filters.decide(part, semantic=True, top_k=3, too_high=None, pc_threshold=None)
    part[3] = np.float32("nan")                            # a row of the table nothing was written to
    with pytest.raises(ValueError, match="lack a score"):
        filters.decide(part, semantic=True, top_k=None, too_high=None, pc_threshold=None)
    assert filters.decide(part[:3], semantic=True, top_k=None, too_high=None, pc_threshold=None)[0].shape == (3,)


def test_sidecar_round_trip_stale_records_header_and_merge(tmp_path, caplog):
    folder = tmp_path / "run/images"
    folder.mkdir(parents=True)
    names = [f"img{k}_prompt_x_{k}.png" for k in range(4)]
    for k, n in enumerate(names):
        (folder / n).write_bytes(b"p" * (10 + k))
    tricky = np.array([np.float32(1) / np.float32(3), np.float32(1e-45), np.float32(3.4028235e38), np.float32(-0.0), np.float32("nan"),
                       np.float32("inf"), np.float32("-inf"), np.float32(16777217.0)], np.float32)
    recs = {names[0]: tricky, names[1]: REF.record(sem=np.float32([1, 2, 3])), names[2]: REF.record(bad=True)}
    header = dict(version=1, semantic=dict(weights="synthetic", prompts=["a", "b"]))
    assert filters.scores_path(str(folder)) == str(tmp_path / "run" / "filter_scores.json")
    kept, sizes = filters.merge_scores(str(folder), header, recs)
    assert sizes == {names[0]: 10, names[1]: 11, names[2]: 12}
    body = json.load(open(tmp_path / "run/filter_scores.json"))                 # strict JSON: NaN is null
    assert set(body) == {"header", "records", "sizes"} and body["records"][names[0]][4] is None
    got_header, got, got_sizes = filters.load_scores(filters.scores_path(str(folder)))
    assert got_header == header and got_sizes == sizes
    for n in recs:
        a, b = REF.bits(got[n]), REF.bits(recs[n])
        nan = np.isnan(recs[n])
        assert np.array_equal(a[~nan], b[~nan]) and np.isnan(got[n][nan]).all(), n      # fp32 exact, -0.0 and the denormal included
    # merge on resume: a new record replaces the old one, the others stay
    new = {names[1]: REF.record(sem=np.float32([5, 2, 3])), names[3]: REF.record(sem=np.float32([0, 2, 3]))}
    kept, _ = filters.merge_scores(str(folder), header, new)
    assert sorted(kept) == sorted(names) and kept[names[1]][2] == 2 and np.array_equal(REF.bits(kept[names[0]])[:4], REF.bits(tricky)[:4])
    # stale: a PNG that is gone, and a PNG of another size under the old name
    (folder / names[0]).unlink()
    (folder / names[3]).write_bytes(b"q" * 99)
    with caplog.at_level(logging.INFO):
        kept, _ = filters.merge_scores(str(folder), header, {})
    assert sorted(kept) == [names[1], names[2]] and any("stale" in r.getMessage() for r in caplog.records)
    # another header: the old records are discarded, with a log line
    caplog.clear()
    with caplog.at_level(logging.INFO):
        kept, _ = filters.merge_scores(str(folder), dict(header, version=2), {names[2]: recs[names[1]]})
    assert list(kept) == [names[2]] and any("header differs" in r.getMessage() for r in caplog.records)
    assert filters.load_scores(str(tmp_path / "nowhere.json")) == (None, {}, {})


def _load_filter_json():
    spec = importlib.util.spec_from_file_location("filter_json", HERE.parent / "run_aug" / "filter_json.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # importing it starts nothing
    return mod


def test_json_from_scores_and_filter_json_tool(scene, caplog, capsys):
    ds, folder, mapping, records = scene["ds"], scene["folder"], scene["mapping"], scene["records"]
    work = [ap for aps in mapping.values() for ap in aps]
    rec = np.stack([records[Path(ap).name] for ap in work])
    header = dict(version=1, semantic=dict(prompts=scene["sem"].prompts), confidence=dict(num_classes=C), per_class=dict(classes=scene["classes"]))
    # scores=: the JSON of the stage, no model, no GPU, no decode
    calls = []
    real = filters._load_u8
    filters._load_u8 = lambda p: calls.append(p) or real(p)
    try:
        with caplog.at_level(logging.INFO):
            jp = utils.create_json_of_image_name_to_augmented_images_paths(
                ds, str(folder), semantic_filtering=1, model_confidence_based_filtering=1, conf_top_k=3, init_log=False,
                original_images_paths=ds.original_images_paths, min_files=1, scores=records, scores_header=header, backfill=False)
    finally:
        filters._load_u8 = real
    assert not calls and Path(jp).name == "semantic_filtering-model_confidence_based_filtering_top_3_classes-aug.json"
    keep, counters = filters.decide(rec, semantic=True, top_k=3, too_high=None, pc_threshold=None)
    kept = {ap for ap, k in zip(work, keep) if k}
    assert json.load(open(jp)) == {n: [ap for ap in aps if ap in kept] for n, aps in mapping.items()}
    msgs = [r.getMessage() for r in caplog.records]
    assert f"For filter = semantic_filtering, filtered {counters['semantic']} images" in msgs
    assert f"For filter = not_in_top_3, filtered {counters['not_in_top_k']} images" in msgs
    assert Path(filters.scores_path(str(folder))).exists()
    # the tool: other settings from the same sidecar
    tool = _load_filter_json()
    jp2 = tool.main([str(folder), "synthetic", "--top-k", "1", "--too-high", "0.2", "--no-semantic"], ds_utils=ds)
    assert Path(jp2).name == "model_confidence_based_filtering_top_1_classes-filter_confidence_higher_than_0.2-aug.json"
    keep, _ = filters.decide(rec, semantic=False, top_k=1, too_high=0.2, pc_threshold=None)
    kept = {ap for ap, k in zip(work, keep) if k}
    assert json.load(open(jp2)) == {n: [ap for ap in aps if ap in kept] for n, aps in mapping.items()}
    jp3 = tool.main([str(folder), "synthetic", "--no-confidence", "--discount", "2"], ds_utils=ds)      # the per-class filter takes over
    assert Path(jp3).name == "clip_filtering_per_class_discount_2-semantic_filtering-aug.json"
    keep, _ = filters.decide(rec, semantic=True, top_k=None, too_high=None, pc_threshold=filters.class_threshold(len(scene["classes"]), 2))
    kept = {ap for ap, k in zip(work, keep) if k}
    assert json.load(open(jp3)) == {n: [ap for ap in aps if ap in kept] for n, aps in mapping.items()}
    # an image without a record: refused with a message that names it, nothing written
    extra = folder / f"{Path(ds.original_images_paths[0]).stem}_prompt_late_9.png"
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(extra)
    os.remove(jp3)
    try:
        with pytest.raises(SystemExit) as e:
            tool.main([str(folder), "synthetic", "--no-confidence", "--discount", "2"], ds_utils=ds)
        assert e.value.code == 1 and "have no record" in capsys.readouterr().err and not os.path.exists(jp3)
    finally:
        extra.unlink()


def test_filter_inline_refusals_and_no_op(tmp_path, caplog):
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=2, sizes=((64, 64),), print_func=quiet)
    assert R.Settings().FILTER_INLINE is False
    base = dict(DATASET="synthetic", NUM_PER_IMAGE=1, RESOLUTION=64, USE_ARTISTIC_PROMPTS=False, PROMPT_WITH_SUB_CLASS=False, FILTER_INLINE=True)

    def never(*a, **k):
        raise AssertionError("nothing may be generated")
    s = R.Settings(SEMANTIC_FILTERING=1, MODEL_CONFIDENCE_BASED_FILTERING=0, LPIPS_MIN=0.1, LPIPS_MAX=0.6, **base)
    with pytest.raises(ValueError, match="LPIPS"):
        R.main(s, ds_utils=ds, batch_generator=never, filter_models=(object(), None), lpips_model=object())
    # no filter on: one log line, then the run as it always was (unfiltered JSON, no sidecar)
    s = R.Settings(SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, **base)
    with caplog.at_level(logging.INFO):
        res = R.main(s, ds_utils=ds, batch_generator=_fake_generator)
    assert sum("FILTER_INLINE: no filter is on" in r.getMessage() for r in caplog.records) == 1
    assert Path(res["json_path"]).name == "aug.json" and res["filter_scores"] is None
    assert not Path(filters.scores_path(res["output_folder"])).exists()


def test_filter_record_is_exported_and_validates_on_the_host():
    """The entry point refuses bad arguments before any launch (no GPU is touched), and its limit is the header's."""
    import ctypes
    from saspa_aug_amd import _lib
    lib = _lib.load()
    assert "saspa_filter_record" in _lib.SYMBOLS and hasattr(lib, "saspa_filter_record")
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(sem=base, ld=8, p=7, cs=base, ci=base, ps=base, pi=base, bad=None, slot=base, table=base, n_rows=70, rows=5):
        return lib.saspa_filter_record(sem, ld, p, cs, ci, ps, pi, bad, slot, table, n_rows, rows, None)
    for kw in (dict(slot=None), dict(table=None), dict(rows=0), dict(n_rows=0), dict(ci=None), dict(ps=None)):
        assert call(**kw) == _lib.SASPA_EINVAL, kw
    for kw in (dict(p=0), dict(p=_lib.FILTER_RECORD_MAX_P + 1, ld=72), dict(ld=6), dict(rows=71)):
        assert call(**kw) == _lib.SASPA_ERANGE, kw
    for kw in (dict(table=base + 4), dict(sem=base + 2), dict(slot=base + 1), dict(ci=base + 2)):
        assert call(**kw) == _lib.SASPA_EALIGN, kw
    src = open(HERE.parent / "include" / "saspa_hip.h").read()
    assert f"#define SASPA_FILTER_RECORD_MAX_P {_lib.FILTER_RECORD_MAX_P}\n" in src and _lib.FILTER_RECORD_FIELDS == len(filters.RECORD_FIELDS)
    mk = open(HERE.parent / "saspa-aug_amd" / "csrc" / "Makefile").read()
    assert "saspa_filter_record.hip" in mk.split("F16_SRCS")[0]          # SRCS: the default and the ablation library


# ---------------------------------------------------------------------------------------------------------------------
# the records gather: two ranks over gloo == one process (the pattern of tests/test_distributed_gloo.py)
# ---------------------------------------------------------------------------------------------------------------------
def _fake_generator(batch, noises, sources):
    imgs = []
    for it, n, src in zip(batch, noises, sources):
        h = hashlib.sha256(it.prompt.encode() + n.numpy().tobytes() + src.tobytes()).digest()
        imgs.append(np.frombuffer(h * ((src.size // 32) + 1), np.uint8)[: src.size].reshape(src.shape).copy())
    return np.stack(imgs), sources.copy()


class _HostRecorder:
    """The recorder's interface on the CPU: 7 'semantic logits' per image out of its pixels, filed through the numpy restatement."""

    def __init__(self):
        self.semantic = type("S", (), dict(prompts=["p"] + filters.NEGATIVE_PROMPTS, dtype=torch.float32, cfg=dict(image_size=64)))()
        self.confidence = self.class_filter = None
        self.dev, self.table, self.batches = "cpu", None, []

    def reset(self, n_rows):
        self.table = np.full((n_rows, 8), np.float32("nan"), np.float32)

    def record(self, images_u8, conf_labels, pc_labels, slots, bad=None):
        assert conf_labels is None and pc_labels is None and len(slots) == images_u8.shape[0]
        self.batches.append(list(slots))
        for im, slot in zip(images_u8.numpy(), slots):
            lg = np.frombuffer(hashlib.sha256(im.tobytes()).digest()[:7], np.uint8).astype(np.float32)
            self.table[slot] = REF.record(sem=lg)

    def table_host(self):
        return self.table


def _inline_settings(prompts_file, root):
    return R.Settings(DATASET="synthetic", NUM_PER_IMAGE=3, SEED=1, RESOLUTION=64, BATCH_SIZE=4, PROMPTS_FILE=prompts_file,
                      DATASET_KWARGS=dict(root_path=root, n_images=7, sizes=((64, 64), (64, 128), (128, 64)), seed=2),
                      SEMANTIC_FILTERING=1, MODEL_CONFIDENCE_BASED_FILTERING=0, FILTER_INLINE=True)


def _worker(rank, world, port, prompts_file, root, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = _HostRecorder()
        res = R.main(_inline_settings(prompts_file, root), batch_generator=_fake_generator, dist=dist, filter_models=(rec.semantic, None),
                     filter_recorder=rec)
        if rank == 0:
            q.put((res["json_path"], res["status"].tolist(), {k: v.tolist() for k, v in res["filter_scores"].items()}))
        else:
            assert res["filter_scores"] is None
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


@pytest.mark.timeout(300)
def test_records_gather_at_two_ranks_equals_single_process(tmp_path):
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("\n".join(f"An airplane number {k} over a field." for k in range(20)) + "\n")
    root1 = str(tmp_path / "one" / "data")
    rec = _HostRecorder()
    r1 = R.main(_inline_settings(str(prompts), root1), batch_generator=_fake_generator, filter_models=(rec.semantic, None), filter_recorder=rec)
    assert (r1["status"] == 1).all() and len(r1["filter_scores"]) == 21
    assert sorted(s for b in rec.batches for s in b) == list(range(21))             # row = position among the rank's items
    assert all((v[0] == 1) and not np.isnan(v[1:3]).any() for v in r1["filter_scores"].values())
    _, side, sizes = filters.load_scores(filters.scores_path(r1["output_folder"]))
    assert sorted(side) == sorted(r1["filter_scores"]) and all(sizes[n] == os.path.getsize(Path(r1["output_folder"]) / n) for n in side)
    assert all(np.array_equal(REF.bits(side[n])[:3], REF.bits(r1["filter_scores"][n])[:3]) for n in side)
    assert Path(r1["json_path"]).name == "semantic_filtering-aug.json"
    root2 = str(tmp_path / "two" / "data")
    DU.SyntheticUtils(root_path=root2, n_images=7, sizes=((64, 64), (64, 128), (128, 64)), seed=2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(prompts), root2, q)) for r in range(2)]
    for p in procs:
        p.start()
    json2, status2, scores2 = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert status2 == [1] * 21 and sorted(scores2) == sorted(r1["filter_scores"])
    for n, v in r1["filter_scores"].items():
        assert np.array_equal(REF.bits(np.float32(scores2[n]))[:3], REF.bits(v)[:3]) and scores2[n][0] == 1, n
    strip = lambda body: {k: sorted(Path(p).name for p in v) for k, v in body.items()}  # noqa: E731
    assert strip(json.load(open(r1["json_path"]))) == strip(json.load(open(json2)))
    assert any(len(v) < 3 for v in json.load(open(json2)).values()), "the semantic decision never dropped an image"
