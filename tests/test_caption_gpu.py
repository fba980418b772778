"""The BLIP captioner on the device (saspa_aug_amd/captioner.py, csrc/saspa_decode.hip) against tests/caption_ref.py:
the two decoder kernels within the error budgets that tests/test_caption_host.py proves on the CPU, the tiny model against the
reference (tolerances of tests/test_blip_gpu.py::test_qformer_front_end, the same layer types), the decisions of greedy and beam
search in fp32, the full-width model once, and the entry point."""
import json
import os

import numpy as np
import pytest
import torch

import caption_ref as R
import errbudget as E
import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib
from saspa_aug_amd import config as CFG
from saspa_aug_amd import ops
from saspa_aug_amd import weights as W
from saspa_aug_amd.captioner import BlipCaptioner

pytestmark = pytest.mark.gpu

UNITS = {torch.bfloat16: E.UNIT_BF16, torch.float32: E.UNIT_F32}
WEIGHT_SEED, IMAGE_SEED = 5, 105          # chosen on the CPU (tests/test_caption_host.py::test_reference_captions_depend_on_the_image)


def _attn_dev(dev, q, k, v, ln, heads, group, scale):
    out = ops.decode_attn(q.to(dev), k.to(dev), v.to(dev), heads, k.shape[1], scale, group=group,
                          lens=None if ln is None else ln.to(dev))
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_attn_within_budget(dev, dtype):
    worst = 0.0
    for case in R.attn_cases():
        rows, heads, d, group, nk = case
        for lens in ("mixed", None):
            q, k, v, ln = R.attn_operands(rows, heads, d, group, nk, dtype, 0, lens=lens)
            scale = d ** -0.5
            ref, s = R.attn_ref64(q, k, v, ln, heads, group, scale)
            got = _attn_dev(dev, q, k, v, ln, heads, group, scale)
            st = E.check_budget(got, ref, s, UNITS[dtype], limits=R.ATTN_LIMITS[dtype], what=f"decode_attn {case} lens={lens}")
            worst = max(worst, E.ratio(st, R.ATTN_LIMITS[dtype]))
    print(f"decode_attn {dtype}: worst statistic at {worst:.3f} of its allowance")
    # negative control: a mutant's output fed to the same assertion
    case = (21, 12, 64, 3, 577)
    q, k, v, ln = R.attn_operands(*case, dtype, 0)
    ref, s = R.attn_ref64(q, k, v, ln, 12, 3, 0.125)
    with pytest.raises(AssertionError):
        E.check_budget(R.attn_emul(q, k, v, ln, 12, 3, 0.125, mutant="key_more"), ref, s, UNITS[dtype], limits=R.ATTN_LIMITS[dtype])


def test_decode_attn_dead_keys_are_never_read(dev):
    """Keys at or beyond a row's length may hold anything (an unwritten cache): NaN there must not reach the output."""
    q, k, v, ln = R.attn_operands(6, 4, 16, 3, 33, torch.float32, 1)
    ln[:3] = 20                                       # entry 0: no row sees keys >= 20
    ref, _ = R.attn_ref64(q, k, v, ln, 4, 3, 0.25)
    k[0, 20:], v[0, 20:] = float("nan"), float("nan")
    got = _attn_dev(dev, q, k, v, ln, 4, 3, 0.25)
    assert torch.isfinite(got).all() and (got.double() - ref).abs().max() < 1e-5


def test_decode_attn_row_alone_is_bit_identical(dev):
    for dtype in (torch.float32, torch.bfloat16):
        q, k, v, ln = R.attn_operands(21, 12, 64, 3, 577, dtype, 2)
        full = _attn_dev(dev, q, k, v, ln, 12, 3, 0.125)
        r = 10                                        # entry 3, second row of its group: alone, as a group of one
        alone = _attn_dev(dev, q[r:r + 1], k[3:4], v[3:4], ln[r:r + 1], 12, 1, 0.125)
        assert torch.equal(alone[0], full[r])
        q1, k1, v1, l1 = R.attn_operands(7, 4, 16, 1, 65, dtype, 3)
        full = _attn_dev(dev, q1, k1, v1, l1, 4, 1, 0.25)
        assert torch.equal(_attn_dev(dev, q1[4:5], k1[4:5], v1[4:5], l1[4:5], 4, 1, 0.25)[0], full[4])


def test_decode_attn_refusals_launch_nothing(dev):
    def call(rows=3, heads=2, d=16, nk=8, group=1, entries=3, ldk=None, off=0):
        c = heads * d
        q = torch.zeros((rows, c), device=dev)
        k = torch.zeros((entries, nk, ldk or c), device=dev)
        out = torch.full((rows, c), 7.0, device=dev)
        p = ops._decode_attn_params(q, k, k, out, None, heads, d, nk, group, 1.0)
        p.ldk = p.ldv = ldk or c
        p.k = k.data_ptr() + off
        rc = _lib.load().saspa_decode_attn(p, None)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), "a refused call wrote the output"
        return rc
    assert call(d=12) == _lib.SASPA_ERANGE            # d % 8
    assert call(heads=1, d=136) == _lib.SASPA_ERANGE  # d > 128
    assert call(nk=1025) == _lib.SASPA_ERANGE
    assert call(group=9, entries=1) == _lib.SASPA_ERANGE
    assert call(ldk=34) == _lib.SASPA_EALIGN          # a key pitch that is no multiple of 16 bytes
    assert call(off=4) == _lib.SASPA_EALIGN
    assert call(group=3, entries=0 + 1, rows=6) == _lib.SASPA_EINVAL    # 1 entry x 3 rows < 6 rows


def test_decode_attn_accepted_call_writes(dev):
    q, k, v, ln = R.attn_operands(3, 2, 16, 1, 8, torch.float32, 0)
    assert torch.isfinite(_attn_dev(dev, q, k, v, ln, 2, 1, 0.25)).all()


def _topk_dev(dev, x, vocab, group, sc, ban, ban_on):
    s, idx, _ = ops.logprob_topk(x.to(dev), vocab, group, sc.to(dev), ban, ban_on)
    idx = idx.cpu().long()
    return s.cpu(), idx[:, :, 0] * vocab + idx[:, :, 1], idx


@pytest.mark.parametrize("images,group,vocab,ld", R.topk_cases())
def test_logprob_topk_within_budget(dev, images, group, vocab, ld):
    worst = 0.0
    for kw in (dict(), dict(dead_row=True), dict(ties=True), dict(plant_last=True)):
        for ban_on in (False, True):
            x, sc, ban = R.topk_operands(images, group, vocab, ld, 0, **kw)
            rs, ri = R.topk_ref64(x, vocab, group, sc, ban, ban_on)
            gs, gi, raw = _topk_dev(dev, x, vocab, group, sc, ban, ban_on)
            assert not torch.isnan(gs).any(), kw
            assert (raw[:, :, 0] >= 0).all() and (raw[:, :, 0] < group).all() and (raw[:, :, 1] < vocab).all()
            err, mism = R.topk_check(gs, gi, rs, ri, R.TOPK_SCORE_LIMIT)
            worst = max(worst, err)
            assert err <= R.TOPK_SCORE_LIMIT and mism == 0, (kw, ban_on, err, mism, gs, rs)
            if kw.get("ties") and not ban_on:         # the planted exact ties, lowest flat index first (topk_check decides them)
                k = 2 * group
                tie = rs[:, :k - 1] == rs[:, 1:k]
                assert tie.any(1).all() and bool((gi[:, :-1][tie] < gi[:, 1:][tie]).all()) and bool((gs[:, :-1][tie] == gs[:, 1:][tie]).all())
            # pad columns: +1e30 there moved nothing -- the same launch on zero padding is bit-identical
            x0 = x.clone()
            x0[:, vocab:] = 0.0
            gs0, gi0, _ = _topk_dev(dev, x0, vocab, group, sc, ban, ban_on)
            assert torch.equal(gs0, gs) and torch.equal(gi0, gi)
    print(f"logprob_topk {images}x{group}x{vocab}: worst score error {worst:.2f} of {R.TOPK_SCORE_LIMIT} units")
    # negative control
    x, sc, ban = R.topk_operands(images, group, vocab, ld, 0)
    rs, ri = R.topk_ref64(x, vocab, group, sc, ban, True)
    ms, mi = R.topk_ref64(x, vocab, group, sc, ban, True, mutant="score_not_added")
    err, mism = R.topk_check(ms[:, :2 * group].float(), mi[:, :2 * group], rs, ri, R.TOPK_SCORE_LIMIT)
    assert err > 2 * R.TOPK_SCORE_LIMIT or mism > 0


def test_logprob_topk_image_alone_is_bit_identical(dev):
    x, sc, ban = R.topk_operands(5, 3, 30524, 30528, 4)
    gs, gi, _ = _topk_dev(dev, x, 30524, 3, sc, ban, True)
    s1, i1, _ = _topk_dev(dev, x[6:9], 30524, 3, sc[6:9], ban, True)
    assert torch.equal(s1[0], gs[2]) and torch.equal(i1[0], gi[2])


# ---- the model ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_case():
    """Weights, images and the CPU reference's results, computed once for the module and never changed."""
    cfg = CFG.tiny_blip_caption()
    sd = W.synth_state_dict("blip_caption", cfg, WEIGHT_SEED)
    px = torch.randn((8, 3, cfg["image_size"], cfg["image_size"]), generator=torch.Generator().manual_seed(IMAGE_SEED))
    sd64 = R.cast(sd, torch.float64)
    emb = R.vision(sd64, cfg, px.double())
    prompt = R.prompt_ids(cfg, [1, 5, 6, 7, 2])
    ids = torch.randint(3, 90, (8, 9), generator=torch.Generator().manual_seed(9))
    ids[:, 0] = cfg["bos"]
    gen = {nb: R.generate(sd64, cfg, None, prompt, nb, 12, 6, image_embeds=emb) for nb in (1, 3)}
    return dict(cfg=cfg, sd=sd, px=px, emb=emb, ids=ids, logits=R.teacher_forced_logits(sd64, cfg, emb, ids), prompt=prompt, gen=gen)


def _maxrel(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiny_model_against_reference(dev, tiny_case, dtype):
    c = tiny_case
    cap = BlipCaptioner(c["sd"], c["cfg"], dev, dtype)
    vis = cap.vision_from_pixels(c["px"])
    logits = cap.teacher_forced_logits(vis, c["ids"])
    rel_v, rel = _maxrel(vis, c["emb"]), _maxrel(logits, c["logits"])
    print(f"tiny captioner {dtype}: vision max-rel {rel_v:.3e}, teacher-forced logits (9 positions) max-rel {rel:.3e}")
    assert rel_v < (2e-4 if dtype == torch.float32 else 6e-2), rel_v          # test_qformer_front_end's bars
    assert rel < (3e-4 if dtype == torch.float32 else 8e-2), rel


@pytest.mark.parametrize("beams", [1, 3])
def test_decisions_fp32(dev, tiny_case, beams):
    c = tiny_case
    cfg = c["cfg"]
    cap = BlipCaptioner(c["sd"], cfg, dev, torch.float32)
    vis = cap.vision_from_pixels(c["px"])
    ref_ids, gap = c["gen"][beams]
    # the largest |delta log-prob| between the device and the reference under teacher forcing, on the reference's own sequences
    lp_dev = torch.log_softmax(cap.teacher_forced_logits(vis, ref_ids).double().cpu(), -1)
    lp_ref = torch.log_softmax(R.teacher_forced_logits(R.cast(c["sd"], torch.float64), cfg, c["emb"], ref_ids), -1)
    dlp = (lp_dev - lp_ref).abs().max().item()
    decided = gap >= 64 * dlp
    got = cap.generate(image_tokens=vis, num_beams=beams, max_length=12, min_length=6, prompt=c["prompt"])
    print(f"beams {beams}: max |dlogp| {dlp:.3e}, smallest gaps {[f'{g:.1e}' for g in gap.tolist()]}, decided {int(decided.sum())} of 8")
    assert int(decided.sum()) >= 6, (dlp, gap)
    assert got.shape[1] <= 12
    for i in range(8):
        if decided[i]:
            n = min(got.shape[1], ref_ids.shape[1])
            assert got.shape[1] == ref_ids.shape[1] and got[i, :n].tolist() == ref_ids[i, :n].tolist(), (i, got[i], ref_ids[i])
    # bf16: reported, never asserted
    cap16 = BlipCaptioner(c["sd"], cfg, dev, torch.bfloat16)
    got16 = cap16.generate(image_tokens=cap16.vision_from_pixels(c["px"]), num_beams=beams, max_length=12, min_length=6, prompt=c["prompt"])
    same = sum(got16[i].tolist() == ref_ids[i].tolist() for i in range(8)) if got16.shape[1] == ref_ids.shape[1] else 0
    print(f"beams {beams}: bf16 agrees with the reference on {same} of 8 id sequences")


def test_unbuilt_modes_raise(dev, tiny_case):
    cap = BlipCaptioner(tiny_case["sd"], tiny_case["cfg"], dev, torch.float32)
    with pytest.raises(NotImplementedError):
        cap.generate(image_tokens=None, use_nucleus_sampling=True)
    with pytest.raises(NotImplementedError):
        cap.generate(image_tokens=None, num_captions=3)


def test_full_width_once(dev):
    cfg = CFG.BLIP_CAPTION
    sd = W.synth_state_dict("blip_caption", cfg, 0)
    cap = BlipCaptioner(sd, cfg, dev, torch.float32)
    imgs = torch.randint(0, 256, (2, 300, 420, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    act = cap.preprocess(imgs)
    assert act.shape == (2, 384, 384, 8)
    vis = cap.vision(act)
    assert vis.shape == (2, 577, 768) and torch.isfinite(vis).all()
    ids = cap.generate(image_tokens=vis, num_beams=3, max_length=8)
    p0 = len(cap.prompt_ids())
    assert ids.shape[0] == 2 and p0 < ids.shape[1] <= 8 and ids[:, 0].tolist() == [cfg["bos"]] * 2 and (ids < cfg["vocab"]).all()
    # one image's first step, teacher-forced, against the reference
    first = cap.teacher_forced_logits(vis[:1], [[cfg["bos"]]])
    assert first.shape == (1, 1, cfg["vocab"]) and torch.isfinite(first).all()
    px = act[:1, :, :, :3].permute(0, 3, 1, 2).float().cpu()
    emb = R.vision(sd, cfg, px)
    ref = R.teacher_forced_logits(sd, cfg, emb, torch.tensor([[cfg["bos"]]]))
    rel = _maxrel(first, ref.double())
    print(f"full-width captioner fp32: first-step logits max-rel {rel:.3e}")
    assert rel < 5e-4, rel                                                   # test_qformer_full_width_fp32's bar


def test_entry_point_writes_captions_and_run_aug_plans_on_them(dev, tmp_path, monkeypatch):
    from PIL import Image

    from saspa_aug_amd import run_aug
    from saspa_aug_amd.prompts_engineering import blip_utils
    from saspa_aug_amd.synthetic import synthetic_image
    monkeypatch.setenv("SASPA_SYNTHETIC_CAPTIONER", "1")
    monkeypatch.setattr(blip_utils, "CAPTION_CONFIG", CFG.tiny_blip_caption())
    paths = []
    for i in range(5):
        p = str(tmp_path / f"img_{i}.png")
        Image.fromarray(synthetic_image(40 + 8 * i, 56, i)).save(p)
        paths.append(p)
    out = str(tmp_path / "captions.json")
    blip_utils.write_captions_of_a_dataset_to_json("planes", paths, out, batch_size=2)
    data = json.load(open(out))
    assert list(data) == paths and all(set(v) == {"caption"} and isinstance(v["caption"], str) for v in data.values())
    assert blip_utils.read_captions_from_json(out) == data
    s = run_aug.Settings()
    s.PROMPT_TYPE, s.NUM_PER_IMAGE = "captions", 2
    items = run_aug.plan_work(s, paths, None, str(tmp_path / "out"), {os.path.basename(p).split(".")[0]: 0 for p in paths},
                              image_size_fn=lambda p: (64, 64), captions=data)
    assert len(items) == 10
