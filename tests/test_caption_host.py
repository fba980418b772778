"""Host-side checks of the BLIP captioner (no GPU): tests/caption_ref.py pinned against transformers' BlipForConditionalGeneration
(skipped cleanly where the package is missing), the conditions the device tests rely on (the reference's captions depend on the
image; its candidate gaps), the error-budget tables of the two decoder kernels by the repository's rule (every limit at least 2x
above the legitimate emulations, every named mutant at least 2x beyond it), and the small host pieces (tokenizer decode, prompt
handling, the JSON writer, the refusals)."""
import json
import os

import numpy as np
import pytest
import torch

import caption_ref as R
import errbudget as E
import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import config as CFG
from saspa_aug_amd import tokenizer as T
from saspa_aug_amd import weights as W
from test_errbudget import SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT_SEED, IMAGE_SEED = 5, 105          # tests/test_caption_gpu.py uses the same pair
PROMPT_TOKENS = [1, 5, 6, 7, 2]           # [CLS] a picture of [SEP] of a tiny vocabulary
UNITS = {torch.bfloat16: E.UNIT_BF16, torch.float32: E.UNIT_F32}


def _tied(sd):
    """The trained model ties the LM-head decoder weight to the word embeddings; transformers loads only such a state dict."""
    sd = dict(sd)
    sd[R.C_ + ".decoder.weight"] = sd[R.B_ + ".embeddings.word_embeddings.weight"]
    return sd


@pytest.fixture(scope="module")
def tiny():
    cfg = CFG.tiny_blip_caption()
    sd = W.synth_state_dict("blip_caption", cfg, WEIGHT_SEED)
    px = torch.randn((8, 3, cfg["image_size"], cfg["image_size"]), generator=torch.Generator().manual_seed(IMAGE_SEED))
    return cfg, sd, px


# ---- 1. the pin ----------------------------------------------------------------------------------------------------------------------
def _hf_model(cfg, sd):
    tr = pytest.importorskip("transformers")
    hc = tr.BlipConfig(
        vision_config=dict(hidden_size=cfg["vis_width"], intermediate_size=cfg["vis_mlp"], num_hidden_layers=cfg["vis_layers"],
                           num_attention_heads=cfg["vis_heads"], image_size=cfg["image_size"], patch_size=cfg["patch"],
                           layer_norm_eps=cfg["vis_eps"]),
        text_config=dict(vocab_size=cfg["vocab"], hidden_size=cfg["width"], encoder_hidden_size=cfg["vis_width"],
                         intermediate_size=cfg["mlp"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                         max_position_embeddings=cfg["max_pos"], bos_token_id=cfg["bos"], eos_token_id=cfg["eos"],
                         pad_token_id=cfg["pad"], sep_token_id=cfg["eos"], layer_norm_eps=cfg["eps"]))
    model = tr.BlipForConditionalGeneration(hc).eval()
    hf_sd = dict(sd)
    hf_sd[R.C_ + ".bias"] = sd[R.C_ + ".decoder.bias"]
    missing, unexpected = model.load_state_dict(hf_sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)   # the spec's names ARE the port's
    return model


def test_reference_reproduces_transformers(tiny):
    cfg, sd, px = tiny
    sd = _tied(sd)
    model = _hf_model(cfg, sd)
    mine = W.blip_caption_from_transformers(model.state_dict())             # the transformers-layout loader, round trip
    assert set(mine) == set(sd) and all(torch.equal(mine[k], sd[k]) for k in sd)
    with torch.no_grad():
        ve = model.vision_model(pixel_values=px)[0]
        emb = R.vision(mine, cfg, px)
        assert (ve - emb).abs().max() <= 2e-5 * ve.abs().max()              # fp32 round-off
        ids = torch.randint(3, 90, (8, 9), generator=torch.Generator().manual_seed(9))
        ids[:, 0] = cfg["bos"]
        lg = model.text_decoder(input_ids=ids, encoder_hidden_states=ve).logits
        ml = R.teacher_forced_logits(mine, cfg, emb, ids)
        assert (lg - ml).abs().max() <= 2e-5 * lg.abs().max()
        early = 0
        for nb in (1, 3):
            out = model.generate(pixel_values=px, input_ids=torch.tensor([PROMPT_TOKENS] * 8), num_beams=nb, max_length=12, min_length=6)
            ref, _ = R.generate(mine, cfg, px, R.prompt_ids(cfg, PROMPT_TOKENS), nb, 12, 6)
            assert out.shape == ref.shape and torch.equal(out, ref), (nb, out, ref)
            early += sum(cfg["eos"] in row[4:-1].tolist() for row in ref)
        assert early >= 1                                                   # a case that finishes on EOS before max_length


# ---- the conditions of the decision tests ------------------------------------------------------------------------------------------
def test_reference_captions_depend_on_the_image(tiny):
    """synth_state_dict's unit-gain scales suffice (nothing of the test's state dict is rescaled): 8 distinct captions on 8 images, a
    dead cross-attention changes them, and at least 6 images keep every candidate gap of the whole search above 1e-4."""
    cfg, sd, px = tiny
    sd64 = R.cast(sd, torch.float64)
    prompt = R.prompt_ids(cfg, PROMPT_TOKENS)
    assert prompt == [cfg["bos"], 5, 6, 7]
    for nb in (1, 3):
        ids, gap = R.generate(sd64, cfg, px.double(), prompt, nb, 12, 6)
        assert len({tuple(r.tolist()) for r in ids}) >= 4
        dead, _ = R.generate(sd64, cfg, px.double(), prompt, nb, 12, 6, dead_cross=True)
        assert dead.shape != ids.shape or not torch.equal(dead, ids)
        px0 = px.double().clone()
        px0[0] = 0.0
        emb = R.vision(sd64, cfg, px0)
        emb[0] = 0.0                                                        # one image's tokens zeroed
        zeroed, _ = R.generate(sd64, cfg, None, prompt, nb, 12, 6, image_embeds=emb)
        n = min(zeroed.shape[1], ids.shape[1])
        assert zeroed.shape != ids.shape or zeroed[0, :n].tolist() != ids[0, :n].tolist()
        assert int((gap >= 1e-4).sum()) >= 6, gap


# ---- 2. the error-budget tables ------------------------------------------------------------------------------------------------------
def _attn_table(dtype):
    legit = {k: 0.0 for k in E.STATS}
    mut = {}
    for seed in SEEDS:
        for case in R.attn_cases():
            rows, heads, d, group, nk = case
            q, k, v, ln = R.attn_operands(rows, heads, d, group, nk, dtype, seed)
            scale = d ** -0.5
            ref, s = R.attn_ref64(q, k, v, ln, heads, group, scale)
            for order in R.ATTN_ORDERS:
                st = E.budget_stats(R.attn_emul(q, k, v, ln, heads, group, scale, order=order), ref, s, UNITS[dtype])
                a = E.allowance(st, R.ATTN_LIMITS[dtype])
                for key in E.STATS:
                    legit[key] = max(legit[key], abs(st[key]) / a[key])
            for m in R.ATTN_MUTANTS:
                if R.attn_mutant_applies(m, case, dtype):
                    st = E.budget_stats(R.attn_emul(q, k, v, ln, heads, group, scale, mutant=m), ref, s, UNITS[dtype])
                    r = E.ratio(st, R.ATTN_LIMITS[dtype])
                    if m not in mut or r < mut[m][0]:
                        mut[m] = (r, case, seed)
    return legit, mut


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_decode_attn_budget_margins(dtype):
    legit, mut = _attn_table(dtype)
    print(f"decode_attn {dtype}: legit worst / allowance {legit}; weakest named mutant cases {mut}")
    assert max(legit.values()) <= 0.5 + 1e-9, legit                         # the limits sit 2x above every legitimate emulation
    named = [m for m in R.ATTN_MUTANTS if m != "p_16bit" or dtype == torch.float32]
    assert set(mut) == set(named)                                           # p_16bit: not separable under bf16 storage (see caption_ref)
    for m, (r, case, seed) in mut.items():
        assert r >= 2.0, (m, r, case, seed)


def _topk_table():
    legit, mut = 0.0, {}
    for seed in SEEDS:
        for images, group, vocab, ld in R.topk_cases():
            for kw in (dict(), dict(dead_row=True), dict(ties=True), dict(plant_last=True)):
                for ban_on in (False, True):
                    x, sc, ban = R.topk_operands(images, group, vocab, ld, seed, **kw)
                    rs, ri = R.topk_ref64(x, vocab, group, sc, ban, ban_on)
                    banned_matters = ban_on and ban in R.topk_ref64(x, vocab, group, sc, ban, False)[1][0, :2 * group].tolist()
                    for order in R.TOPK_ORDERS:
                        gs, gi = R.topk_emul(x, vocab, group, sc, ban, ban_on, order=order)
                        err, mism = R.topk_check(gs, gi, rs, ri, R.TOPK_SCORE_LIMIT)
                        assert mism == 0, (order, images, group, vocab, kw, ban_on)
                        legit = max(legit, err)
                    for m in R.TOPK_MUTANTS:
                        # where a mutant is NAMED: the banned token would have been selected; the leading rows' scores are not 0
                        # (they are in the tie cases); pad columns exist; the planted ties /
                        # the planted last candidate are not the banned token (the first row's best: it is one of them)
                        named = {"ban_ignored": banned_matters, "score_not_added": not kw.get("ties"), "pad_in_lse": ld > vocab,
                                 "ties_highest": bool(kw.get("ties")) and not ban_on,
                                 "last_dropped": bool(kw.get("plant_last")) and not ban_on}[m]
                        if not named:
                            continue
                        ms, mi = R.topk_ref64(x, vocab, group, sc, ban, ban_on, mutant=m)
                        k = 2 * group
                        err, mism = R.topk_check(ms[:, :k].float(), mi[:, :k], rs, ri, R.TOPK_SCORE_LIMIT)
                        r = float("inf") if mism else err / R.TOPK_SCORE_LIMIT
                        if m not in mut or r < mut[m][0]:
                            mut[m] = (r, (images, group, vocab, ld), kw, ban_on, seed)
    return legit, mut


def test_logprob_topk_budget_margins():
    legit, mut = _topk_table()
    print(f"logprob_topk: legit worst {legit:.1f} units of {R.TOPK_SCORE_LIMIT}; weakest named mutant cases {mut}")
    assert legit <= 0.5 * R.TOPK_SCORE_LIMIT + 1e-9, legit
    assert set(mut) == set(R.TOPK_MUTANTS)
    for m, rec in mut.items():
        assert rec[0] >= 2.0, (m, rec)


def test_errbudget_file_records_the_limits():
    text = open(os.path.join(ROOT, "profiles", "caption_errbudget.txt")).read()
    for dtype in R.ATTN_LIMITS:
        for key, val in R.ATTN_LIMITS[dtype].items():
            assert f"{key}={val:g}" in text, (dtype, key, val)
    assert f"limit={R.TOPK_SCORE_LIMIT:g}" in text and "p_16bit" in text


# ---- 3. smaller host checks ------------------------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "picture", "of", "cat", "##s", "sit", "##ting", "on", "the", "mat", ".", ",", "'",
         "s", "it", "don", "t", "!", "?", "re", "they", "[DEC]", "[ENC]"]


def test_wordpiece_decode_matches_transformers(tmp_path):
    vf = tmp_path / "vocab.txt"
    vf.write_text("\n".join(VOCAB) + "\n")
    tok = T.BertWordPieceTokenizer(str(vf))
    seqs = [[26, 5, 6, 7, 5, 8, 9, 10, 11, 12, 13, 14, 15, 3, 0, 0],
            [2, 13, 8, 17, 18, 14, 16, 19, 20, 17, 21, 22, 1, 3], [26, 25, 17, 24, 10, 11, 23, 27, 3]]
    assert tok.decode(seqs[0]) == "a picture of a cats sitting on the mat."
    assert tok.decode(seqs[0], skip_special_tokens=False).startswith("[DEC] a picture")
    tr = pytest.importorskip("transformers")
    hf = tr.BertTokenizer(str(vf), do_lower_case=True, additional_special_tokens=["[DEC]", "[ENC]"])
    for ids in seqs:
        assert tok.decode(ids) == hf.decode(ids, skip_special_tokens=True, clean_up_tokenization_spaces=True), ids


def test_prompt_handling_and_stripping(tmp_path):
    """BOS replaces token 0, SEP is dropped, and the decoded caption loses the prompt as LAVIS does (output[len(prompt):])."""
    from saspa_aug_amd.captioner import BlipCaptioner
    vf = tmp_path / "vocab.txt"
    vf.write_text("\n".join(VOCAB) + "\n")
    cfg = CFG.tiny_blip_caption(bos=26, eos=3)
    cap = BlipCaptioner(W.synth_state_dict("blip_caption", cfg, 0), cfg, "cpu", torch.float32, tokenizer=T.BertWordPieceTokenizer(str(vf)))
    assert cap.tok("a picture of ")[0].tolist() == [2, 5, 6, 7, 3] and cap.prompt_ids() == [26, 5, 6, 7]
    assert cap.decode([26, 5, 6, 7, 5, 8, 10, 11, 3, 3, 3]) == "a cat sitting"
    cfg = CFG.tiny_blip_caption()                                           # the hash stand-in: [SEP] = 2 in a tiny vocabulary
    hashed = BlipCaptioner(W.synth_state_dict("blip_caption", cfg, 0), cfg, "cpu", torch.float32)
    assert hashed.prompt_ids()[0] == cfg["bos"] and len(hashed.prompt_ids()) == 4
    assert hashed.decode(hashed.prompt_ids() + [40, 41, cfg["eos"]]) == "t40 t41"


def test_hash_tokenizer_placeholder_decode():
    tok = T.BertHashTokenizer(96)
    assert tok.decode([1, 5, 6, 2, 0]) == "t5 t6" and tok.decode([5], skip_special_tokens=False) == "t5"


def test_lavis_layout_maps_onto_the_spec():
    """The LAVIS names are recalled and unverified; what IS checked: the mapping is a bijection onto the spec's names."""
    cfg = CFG.tiny_blip_caption()
    sd = W.synth_state_dict("blip_caption", cfg, 0)
    inv = {}
    for k, v in sd.items():
        lk = k
        if k.startswith("vision_model.encoder.layers."):
            lk = k.replace("vision_model.encoder.layers.", "visual_encoder.blocks.").replace(".layer_norm1.", ".norm1.") \
                .replace(".layer_norm2.", ".norm2.").replace(".self_attn.qkv.", ".attn.qkv.").replace(".self_attn.projection.", ".attn.proj.")
        else:
            for a, b in W._LAVIS_VIT:
                if k.startswith(b):
                    lk = a + k[len(b):]
        inv[lk] = v
    assert any(k.startswith("visual_encoder.blocks.0.attn.qkv") for k in inv) and "visual_encoder.cls_token" in inv
    back = W.blip_caption_from_lavis({"model": inv})
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_refusals(monkeypatch, tmp_path):
    from saspa_aug_amd import captioner
    from saspa_aug_amd.prompts_engineering import blip_utils
    monkeypatch.delenv("SASPA_SYNTHETIC_CAPTIONER", raising=False)
    with pytest.raises(RuntimeError, match="SASPA_SYNTHETIC_CAPTIONER"):
        captioner.BlipCaptioner.from_synthetic(CFG.tiny_blip_caption(), "cpu", torch.float32)
    with pytest.raises(NotImplementedError):
        blip_utils.write_captions_of_a_dataset_to_json("planes", [], str(tmp_path / "c.json"), questions=["what is it?"])
    with pytest.raises(FileNotFoundError):
        captioner.BlipCaptioner.from_pretrained(str(tmp_path), "cpu", torch.float32)


def test_json_writer_layout(tmp_path):
    from PIL import Image

    from saspa_aug_amd.prompts_engineering import blip_utils

    class Fake:
        def caption(self, images):
            assert all(im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 for im in images)
            return [f"a {im.shape[0]} by {im.shape[1]} thing" for im in images]

    paths = []
    for i in range(5):
        p = str(tmp_path / f"im{i}.png")
        Image.fromarray(np.full((8 + i, 9), 40 * i, np.uint8)).save(p)      # greyscale on disk: loaded with convert("RGB")
        paths.append(p)
    out = str(tmp_path / "sub" / "captions.json")
    got = blip_utils.write_captions_of_a_dataset_to_json("planes", paths, out, batch_size=2, captioner=Fake())
    data = blip_utils.read_captions_from_json(out)
    assert data == got and list(data) == paths and data[paths[3]] == {"caption": "a 11 by 9 thing"}
    shipped = json.load(open(os.path.join(ROOT, "saspa-aug_amd", "prompts_engineering", "captions", "dtd_captions.json")))
    assert {tuple(v) for v in shipped.values()} == {("caption",)}           # the same layout as the shipped file
