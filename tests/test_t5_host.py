"""The T5 key-to-text generator on the CPU (no GPU): what PINS tests/t5_ref.py and the host code of saspa_aug_amd/txt2sentence.py to
transformers (bucket function, model, greedy ids, warpers, tokenizer), the margins of the kernel budgets that tests/test_t5_gpu.py
asserts on the device, the conditions of its decision tests, the prompt tool with a fake generator, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import saspa_aug_amd  # noqa: F401
import t5_ref as R
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import tokenizer as T
from saspa_aug_amd import txt2sentence as T2S
from saspa_aug_amd import weights as W
from saspa_aug_amd.prompts_engineering import txt2sentance_prompts as TP

WEIGHT_SEED, UNIFORM_SEED, GROUP_UNIFORM_SEED = R.WEIGHT_SEED, R.UNIFORM_SEED, R.GROUP_UNIFORM_SEED
tiny_inputs = R.tiny_inputs


@pytest.fixture(scope="module")
def tiny():
    cfg = CFG.tiny_t5()
    sd = W.t5_synth_state_dict(cfg, WEIGHT_SEED)
    ids, lens = tiny_inputs(cfg)
    return cfg, sd, ids, lens


def hf_model(cfg, sd):
    tr = pytest.importorskip("transformers")
    hc = tr.T5Config(vocab_size=cfg["vocab"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], d_ff=cfg["d_ff"], num_layers=cfg["enc_layers"],
                     num_decoder_layers=cfg["dec_layers"], num_heads=cfg["heads"], relative_attention_num_buckets=cfg["buckets"],
                     relative_attention_max_distance=cfg["max_distance"], dropout_rate=0.0, layer_norm_epsilon=cfg["eps"],
                     feed_forward_proj="relu", pad_token_id=cfg["pad"], eos_token_id=cfg["eos"],
                     decoder_start_token_id=cfg["decoder_start"], tie_word_embeddings=True)
    model = tr.T5ForConditionalGeneration(hc).eval()
    full = dict(sd)
    for k in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight", "lm_head.weight"):
        full[k] = sd["shared.weight"]
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and all(k in full or "embed_tokens" in k or k == "lm_head.weight" for k in missing), (missing, unexpected)
    return model


# ---- 1. pinned to transformers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buckets,max_distance", [(32, 128), (8, 16)])
@pytest.mark.parametrize("bidirectional", [True, False])
def test_relative_bucket_equals_transformers(buckets, max_distance, bidirectional):
    m = pytest.importorskip("transformers.models.t5.modeling_t5")
    rel = torch.arange(-300, 301)
    want = m.T5Attention._relative_position_bucket(rel, bidirectional=bidirectional, num_buckets=buckets, max_distance=max_distance)
    assert torch.equal(T2S.relative_bucket(rel, bidirectional, buckets, max_distance), want)
    assert torch.equal(R.bucket(rel, bidirectional, buckets, max_distance), want)
    # the table the kernel indexes: column c holds the bucket of rel = center - c, and both ends are already saturated
    w = torch.randn((buckets, 3), generator=torch.Generator().manual_seed(0))
    tab, center = T2S.bias_table(w, bidirectional, buckets, max_distance)
    ncol = tab.shape[1]
    assert ncol == (2 * max_distance + 1 if bidirectional else max_distance + 1) and center == (max_distance if bidirectional else 0)
    for pos_minus_j in range(-300, 301):
        col = min(max(pos_minus_j + center, 0), ncol - 1)
        assert torch.equal(tab[:, col], w[want[300 - pos_minus_j]]), pos_minus_j          # rel = j - pos


def test_reference_equals_transformers(tiny):
    cfg, sd, ids, lens = tiny
    model = hf_model(cfg, sd)
    ref = R.Ref(sd, cfg)
    mask = (torch.arange(ids.shape[1])[None] < lens[:, None]).long()
    dec = torch.randint(2, cfg["vocab"], (8, 9), generator=torch.Generator().manual_seed(5))
    dec[:, 0] = cfg["decoder_start"]
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, decoder_input_ids=dec)
    enc = ref.encode(ids, lens)
    live = mask.bool()
    rel_e = ((enc - out.encoder_last_hidden_state)[live].abs().max() / out.encoder_last_hidden_state[live].abs().max()).item()
    logits = ref.decoder_logits(enc, lens, dec)
    rel_l = ((logits - out.logits).abs().max() / out.logits.abs().max()).item()
    print(f"t5_ref vs transformers: encoder max-rel {rel_e:.2e}, teacher-forced logits max-rel {rel_l:.2e}")
    assert rel_e < 1e-5 and rel_l < 1e-5
    with torch.no_grad():
        want = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_length=20, num_beams=1)
    got, gap, _ = ref.generate(ids, lens, do_sample=False, max_length=20)
    assert got.shape == want.shape and torch.equal(got, want), (got, want)
    assert len({tuple(r.tolist()) for r in got}) >= 6 and int((got[:, 1:] != got[:, 1:2]).any(1).sum()) >= 5    # not one token over and over
    # the loader round-trips transformers' own state dict
    back = W.t5_from_hf(model.state_dict(), cfg)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(KeyError):
        W.t5_from_hf({k: v for k, v in sd.items() if "block.1.layer.1.EncDecAttention.k" not in k}, cfg)


def test_from_pretrained_reads_a_transformers_checkpoint(tiny, tmp_path):
    """config.json + pytorch_model.bin as transformers writes them, and a tokenizer.json: the generator comes up with the checkpoint's
    config, weights and vocabulary (on the CPU nothing is launched)."""
    cfg, sd, _, _ = tiny
    model = hf_model(cfg, sd)
    with open(tmp_path / "config.json", "w") as f:
        f.write(model.config.to_json_string())
    torch.save(model.state_dict(), tmp_path / "pytorch_model.bin")
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        T2S.T5Generator.from_pretrained(str(tmp_path), "cpu", torch.float32)
    vocab = [["<pad>", 0.0], ["</s>", 0.0], ["<unk>", 0.0], ["\u2581", -1.0], ["a", -2.0], ["\u2581car", -3.0], ["r", -2.5], ["c", -2.5]]
    with open(tmp_path / "tokenizer.json", "w") as f:
        json.dump({"model": {"type": "Unigram", "unk_id": 2, "vocab": vocab}}, f)
    gen = T2S.T5Generator.from_pretrained(str(tmp_path), "cpu", torch.float32)
    for k in ("d_model", "enc_layers", "dec_layers", "heads", "d_kv", "d_ff", "vocab", "buckets", "max_distance", "eps", "pad", "eos"):
        assert gen.cfg[k] == cfg[k], k
    assert gen.cfg["tie_embeddings"] and gen.cfg["decoder_start"] == cfg["decoder_start"] and gen.cfg["top_k"] == 50
    assert torch.equal(gen.p["shared"], sd["shared.weight"]) and gen.p["encoder.bias"].shape == (cfg["heads"], 2 * cfg["max_distance"] + 1)
    ids, lens = gen.tokenize(["a car", "car"])
    assert ids.tolist() == [[3, 4, 5, 1], [5, 1, 0, 0]] and lens.tolist() == [4, 2]
    assert gen.tok.decode(ids[0]) == "a car"


@pytest.mark.parametrize("vocab", [40, 1000])
def test_reference_sampler_equals_transformers_warpers(vocab):
    lp = pytest.importorskip("transformers.generation.logits_process")
    for temperature, top_k, top_p in R.SAMPLE_GRID:
        x, u = R.sample_operands(16, vocab, 0)
        s = R.sample_ref64(x, vocab, temperature, top_k, top_p, u)
        scores = x[:, :vocab].clone()
        ids = torch.zeros((16, 1), dtype=torch.long)
        scores = lp.TemperatureLogitsWarper(temperature)(ids, scores)
        scores = lp.TopKLogitsWarper(top_k)(ids, scores)
        if top_p < 1.0:
            scores = lp.TopPLogitsWarper(top_p)(ids, scores)
        probs = torch.softmax(scores.double(), -1)
        for r in range(16):
            if not s["decidable"][r]:
                continue
            kept = set(torch.nonzero(probs[r] > 0).flatten().tolist())
            assert kept == set(s["kept"][r].tolist()), (temperature, top_k, top_p, r)
            assert torch.allclose(probs[r][s["kept"][r]], s["probs"][r], rtol=1e-5, atol=1e-9)


def test_unigram_tokenizer_equals_tokenizers(tmp_path):
    tk = pytest.importorskip("tokenizers")
    import random
    rnd = random.Random(0)
    words = ["airplane", "boeing", "737-400", "a", "photo", "of", "the", "car", "bird", "red", "blue", "sky", "flying", "over", "city", "type",
             "texture", "striped", "dotted", "wing", "engine", "2012", "audi", "bmw", "sedan", "Citroën", "hatchback", "parked", "road", "field"]
    corpus = [" ".join(rnd.choice(words) for _ in range(8)) for _ in range(300)]
    tok = tk.Tokenizer(tk.models.Unigram())
    tok.normalizer = tk.normalizers.Sequence([tk.normalizers.NFKC(), tk.normalizers.Strip(), tk.normalizers.Replace(tk.Regex(" {2,}"), " ")])
    tok.pre_tokenizer = tk.pre_tokenizers.Metaspace()
    tok.decoder = tk.decoders.Metaspace()
    tok.train_from_iterator(corpus, tk.trainers.UnigramTrainer(vocab_size=120, special_tokens=["<pad>", "</s>", "<unk>"], unk_token="<unk>",
                                                               show_progress=False))
    path = str(tmp_path / "tokenizer.json")
    tok.save(path)
    mine = T.UnigramTokenizer(path)
    assert mine.eos == 1 and mine.unk == 2
    for text in ["a photo of  a   boeing 737-400", "Citroën sedan, of type audi", "the red car flying over 2012 city", "zebra quux", " bmw ",
                 "airplane, of type Boeing 737-400", "ﬁeld road"]:
        want = tok.encode(text).ids + [1]
        got = mine.encode(text)
        assert got == want, (text, got, want)
        assert mine.decode(got) == tok.decode(want, skip_special_tokens=True), text
    assert mine.decode(mine.encode("the red car parked")) == "the red car parked"
    # the stand-in of a synthetic-weight run: stable ids, eos appended, a placeholder decode
    h = T.UnigramTokenizer(vocab_size=128)
    a = h.encode("airplane, of type 707-320")
    assert a[-1] == 1 and a == h.encode("airplane,  of type   707-320") and all(3 <= i < 128 for i in a[:-1])
    assert h.decode(a) == " ".join(f"t{i}" for i in a[:-1])


# ---- 2. the budgets of the kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rmsnorm_budget_margins(dtype):
    legit, raw, mut = R.rms_margins(dtype)
    print(f"rmsnorm {dtype}: legit worst / allowance {legit}; raw {raw}; weakest named mutant cases {mut}")
    assert max(legit.values()) <= 0.5 + 1e-9, legit
    assert set(mut) == set(R.RMS_MUTANTS)
    for m, rec in mut.items():
        assert rec[0] >= 2.0, (m, rec)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_relbias_budget_margins(dtype):
    legit, raw, mut = R.rel_margins(dtype)
    print(f"attn_relbias {dtype}: legit worst / allowance {legit}; raw {raw}; weakest named mutant cases {mut}")
    assert max(legit.values()) <= 0.5 + 1e-9, legit
    assert set(mut) == set(R.REL_MUTANTS)
    for m, rec in mut.items():
        assert rec[0] >= 2.0, (m, rec)


def test_relbias_cases_reach_every_column_and_both_clamped_ends():
    hit = {t: set() for t in range(len(R.REL_TABLES))}
    low, high = set(), set()
    for case in R.rel_cases():
        heads, d, nk, rpe, table = case
        _, _, _, ln, pos, bias, center = R.rel_operands(case, torch.float32, 0)
        ncol = bias.shape[1]
        raw = R.rel_columns(pos, nk, center, ncol, clamp=False)
        live = torch.arange(nk)[None, :] < ln.long()[:, None]
        hit[table] |= set(raw.clamp(0, ncol - 1)[live].tolist())
        if bool(((raw < 0) & live).any()):
            low.add(table)
        if bool(((raw > ncol - 1) & live).any()):
            high.add(table)
        assert int(ln.min()) == 0 and 1 in ln.tolist() and int(ln.max()) == nk
    for t, (nb, md, bidir) in enumerate(R.REL_TABLES):
        ncol = 2 * md + 1 if bidir else md + 1
        assert hit[t] == set(range(ncol)), (t, sorted(set(range(ncol)) - hit[t]))        # every column: every bucket boundary
    assert low == high == set(range(len(R.REL_TABLES)))


def test_sampler_cases_are_decidable_and_mutants_are_told_apart():
    total = und = 0
    told = {m: 0 for m in R.SAMPLE_MUTANTS}
    for vocab in (40, 1000):
        for temperature, top_k, top_p in R.SAMPLE_GRID:
            x, u = R.sample_operands(64, vocab, 0)
            s = R.sample_ref64(x, vocab, temperature, top_k, top_p, u)
            total += 64
            und += int((~s["decidable"]).sum())
            m = R.sample_ref64(x, vocab, temperature, top_k, top_p, u, mutant="topp_before_topk")
            told["topp_before_topk"] += int(((m["tok"] != s["tok"]) & s["decidable"]).sum())
    assert und <= 0.02 * total, (und, total)
    assert told["topp_before_topk"] > 0
    # the other three differ from the contract only on exact ties and exact boundaries: planted, and exact in any arithmetic
    x, u, want = planted_sampler_cases()
    ok = R.sample_ref64(x, 40, 1.0, 2, 0.5, u)["tok"].tolist()
    ok2 = R.sample_ref64(x, 40, 1.0, 2, 1.0, u)["tok"].tolist()
    assert (ok, ok2) == want
    assert R.sample_ref64(x, 40, 1.0, 2, 1.0, u, mutant="ties_highest")["tok"].tolist() != ok2
    assert R.sample_ref64(x, 40, 1.0, 2, 1.0, u, mutant="draw_ge")["tok"].tolist() != ok2
    assert R.sample_ref64(x, 40, 1.0, 2, 0.5, u, mutant="topp_gt")["tok"].tolist() != ok


def planted_sampler_cases():
    """Rows whose two best logits (tokens 7 and 30) are EXACTLY equal, far above the rest; kept probabilities 1/2 and 1/2 in any
    arithmetic.  u = 0, 0.25, 0.5 (exactly the boundary: `>` moves on to token 30), 0.75.  -> (x [4, 48], u, (ids with top_k 2 and
    top_p 0.5: the prefix {7} reaches 0.5 and is kept alone, ids with top_p 1))."""
    x = torch.randn((4, 48), generator=torch.Generator().manual_seed(2))
    x[:, 40:] = 1e30
    x[:, 7] = x[:, 30] = 50.0
    u = torch.tensor([0.0, 0.25, 0.5, 0.75])
    return x, u, ([7, 7, 7, 7], [7, 7, 30, 30])


def test_decision_seeds_meet_their_conditions(tiny):
    """The seeds of tests/test_t5_gpu.py's decision test: every greedy step's top-1 / top-2 gap exceeds 1e-3 relative, every sampled draw
    is decidable, and the synthetic init gives sequences that are not one token repeated."""
    cfg, sd, ids, lens = tiny
    ref = R.Ref(sd, cfg)
    got, gap, _ = ref.generate(ids, lens, do_sample=False, max_length=20)
    assert gap > 1e-3, gap
    u = torch.rand((8, 20), generator=torch.Generator().manual_seed(UNIFORM_SEED))
    smp, _, decidable = ref.generate(ids, lens, do_sample=True, top_k=50, top_p=0.9, temperature=0.7, max_length=20, uniforms=u)
    assert decidable
    assert not torch.equal(smp[:, :min(smp.shape[1], got.shape[1])], got[:, :min(smp.shape[1], got.shape[1])])
    assert sum(len(set(r[1:].tolist())) >= 2 for r in got) >= 5, got
    assert sum(len(set(r[1:].tolist())) >= 2 for r in smp) >= 5, smp
    # 11 samples of one input (tests/test_t5_gpu.py: a group of 8 + 3 on one cross K / V)
    u11 = torch.rand((11, 20), generator=torch.Generator().manual_seed(GROUP_UNIFORM_SEED))
    s11, _, decidable = ref.generate(ids[2:3].expand(11, -1), lens[2:3].expand(11), do_sample=True, top_k=50, top_p=1.0, temperature=1.0,
                                     max_length=20, uniforms=u11)
    assert decidable and len({tuple(r.tolist()) for r in s11}) >= 9


# ---- 3. the prompt tool ----------------------------------------------------------------------------------------------------------
class FakeGenerator:
    def __init__(self, outputs):
        self.outputs, self.calls = list(outputs), []

    def sentences(self, inputs, **kw):
        self.calls.append((list(inputs), kw))
        out, self.outputs = self.outputs[:len(inputs)], self.outputs[len(inputs):]
        return out


def test_word2sentence_filters_counts_and_dedups_in_order(tmp_path, caplog):
    outs = ["A plane in the sky", "a dog", "An AIRPLANE lands", "A plane in the sky", "jet on a runway", "a cat",           # class A
            "aircraft parked", "aircraft parked", "nothing", "a plane", "the jet", "a jet"]                               # class B
    gen = FakeGenerator(outs)
    path = tmp_path / "LE.json"
    with caplog.at_level("INFO"):
        d, counters = TP.word2sentence(["A 1", "B 2"], 6, str(path), all_classes=True, must_keywords=TP.DATASET_TO_LABEL_DICT["planes"],
                                       dataset="planes", generator=gen, batch_size=4, seed=5)
    assert d == {"A 1": ["A plane in the sky", "An AIRPLANE lands", "jet on a runway"], "B 2": ["aircraft parked", "a plane", "the jet", "a jet"]}
    assert json.load(open(path)) == d and list(json.load(open(path))) == ["A 1", "B 2"]
    assert counters == dict(num_skipped_due_to_no_class_in_sentence=3, total_sentences=9, total_classes=2)
    assert "num_skipped_due_to_no_class_in_sentence: 3" in caplog.text
    assert [(c[0][0], len(c[0])) for c in gen.calls] == [("airplane, of type A 1", 4), ("airplane, of type A 1", 2),
                                                          ("airplane, of type B 2", 4), ("airplane, of type B 2", 2)]
    assert all(c[1]["do_sample"] is True and isinstance(c[1]["generator"], torch.Generator) for c in gen.calls)
    assert TP.class_input("x", False, "cub") == "bird" and TP.class_input("close up of the door of a", False, "compcars-parts") == "close up of the door of a"


def test_main_names_the_file_and_run_aug_plans_on_it(tmp_path, monkeypatch):
    from saspa_aug_amd import run_aug, utils
    gen = FakeGenerator([f"an airplane number {i}." for i in range(100)])
    path = TP.main("planes", 3, str(tmp_path / "out"), False, generator=gen)
    assert os.path.basename(path) == "LE_3_planes_all_classes_False.json"
    d = json.load(open(path))
    assert list(d) == ["airplane", "plane", "aircraft", "jet"] and all(len(v) == 3 for k, v in d.items() if k != "aircraft")
    s = run_aug.Settings(DATASET="planes", PROMPT_TYPE="txt2sentence", NUM_PER_IMAGE=2, SEED=3, USE_ARTISTIC_PROMPTS=False,
                         PROMPT_WITH_SUB_CLASS=False, PROMPTS_FILE=path)
    prompts = run_aug.read_prompts_from_json(s.PROMPTS_FILE, s.DATASET, per_class=False)
    utils.set_seed(s.SEED)
    items = run_aug.plan_work(s, ["/d/img0.jpg", "/d/img1.jpg"], prompts, str(tmp_path), {"img0": "707", "img1": "A320"},
                              image_size_fn=lambda p: (512, 512))
    assert len(items) == 4 and all(it.prompt.startswith("an airplane number") and not it.prompt.endswith(".") for it in items)
    # per class
    gen = FakeGenerator([f"a jet {i}" for i in range(100)])
    _, _ = TP.word2sentence(["707", "A320"], 2, str(tmp_path / "pc.json"), all_classes=True, must_keywords=["jet"], dataset="planes", generator=gen)
    s = run_aug.Settings(DATASET="planes", PROMPT_TYPE="txt2sentence-per_class", NUM_PER_IMAGE=2, SEED=3, USE_ARTISTIC_PROMPTS=False,
                         PROMPT_WITH_SUB_CLASS=False, PROMPTS_FILE=str(tmp_path / "pc.json"))
    c2p = run_aug.read_prompts_from_json(s.PROMPTS_FILE, s.DATASET, per_class=True)
    utils.set_seed(s.SEED)
    items = run_aug.plan_work(s, ["/d/img0.jpg", "/d/img1.jpg"], None, str(tmp_path), {"img0": "707", "img1": "A320"},
                              image_size_fn=lambda p: (512, 512), class_to_prompts=c2p)
    assert [it.prompt in c2p[c] for it, c in zip(items, ["707", "707", "A320", "A320"])] == [True] * 4


# ---- 4. refusals, ABI ------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, monkeypatch):
    monkeypatch.delenv("SASPA_SYNTHETIC_T5", raising=False)
    with pytest.raises(RuntimeError, match="SASPA_SYNTHETIC_T5"):
        T2S.T5Generator.from_synthetic(CFG.tiny_t5(), "cpu", torch.float32)
    with pytest.raises(FileNotFoundError):
        T2S.T5Generator.from_pretrained(str(tmp_path / "nope"), "cpu", torch.float32)
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError):
        T2S.T5Generator.from_pretrained(str(tmp_path / "empty"), "cpu", torch.float32)
    with pytest.raises(TypeError):
        T2S.T5Generator(W.t5_synth_state_dict(CFG.tiny_t5(), 0), CFG.tiny_t5(), "cpu", torch.float16)
    monkeypatch.setenv("SASPA_SYNTHETIC_T5", "1")
    cfg = CFG.tiny_t5()
    gen = T2S.T5Generator.from_synthetic(cfg, "cpu", torch.float32)
    too_long = np.ones((1, cfg["max_input"] + 1), np.int64)
    with pytest.raises(ValueError, match="encoder cap"):
        gen.generate(too_long, [cfg["max_input"] + 1], do_sample=False)
    with pytest.raises(ValueError):
        gen.generate(np.ones((2, 4), np.int64), [4, 5], do_sample=False)
    # rows are planned by distinct input: 11 samples of one input and 2 of another -> 8 + 3 and 2, three entries of group 8
    ids = np.array([[5, 6, 1, 0]] * 11 + [[7, 1, 0, 0]] * 2)
    distinct, entry_of, slot_seq, group = gen.plan_rows(ids, [3] * 11 + [2] * 2)
    assert (distinct, entry_of, group) == ([0, 11], [0, 0, 1], 8)
    assert slot_seq == list(range(8)) + [8, 9, 10] + [-1] * 5 + [11, 12] + [-1] * 6
    assert gen.format_input(["red", "car"]) == "red car" and gen.format_input("['red', 'car']") == "red car"


def test_abi_is_still_20_and_the_new_symbols_are_exported():
    lib = _lib.load()
    assert lib.saspa_abi_version() == 20
    for name in ("saspa_rmsnorm", "saspa_attn_relbias", "saspa_sample_topk"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # refusals are decided on the host: no GPU needed
    p = _lib.AttnRelbiasParams()
    assert lib.saspa_attn_relbias(p, None) == _lib.SASPA_EINVAL
    assert lib.saspa_rmsnorm(_lib.SASPA_BF16, None, 8, None, 8, 1, 8, None, 1e-6, None) == _lib.SASPA_EINVAL
    assert lib.saspa_sample_topk(None, 8, 8, 1, 1.0, 1, 1.0, None, None, None, None) == _lib.SASPA_EINVAL
    assert (_lib.RMSNORM_MAX_C, _lib.RELBIAS_MAX_ROWS, _lib.SAMPLE_MAX_TOPK) == (8192, 1024, 64)
