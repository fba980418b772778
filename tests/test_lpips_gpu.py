"""LPIPS (AlexNet) min / max filter and diversity measure on the MI355X: the luma kernel and the pre-processing against Pillow,
`saspa_lpips_layer` against the float64 restatement (tests/lpips_ref.py) under a rounding-error bound with negative controls, the
whole model, and the decisions / counters / file names through `create_json_of_image_name_to_augmented_images_paths`."""
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
from saspa_aug_amd import filters, ops, utils
from saspa_aug_amd import weights as W
from saspa_aug_amd.synthetic import synthetic_image
from saspa_aug_amd.tokenizer import HashTokenizer
from tests import lpips_ref as LR
from tests.util import from_nhwc

pytestmark = pytest.mark.gpu

MODEL_RTOL = 3e-4          # the bar of the fp32 filter networks (test_wsdan_cal_vs_oracle_and_reference_golden)
PRODUCTION = [(3969, 64), (961, 192), (225, 384), (225, 256), (225, 256)]       # AlexNet taps of a 256 x 256 input
TINY = [(3969, 8), (961, 16), (225, 24), (225, 16)]                             # CFG.tiny_filters()["lpips_alex"]
ODD = [(2, 512), (7, 8), (130, 40)]


# ---- pre-processing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (7, 13), (64, 64), (333, 250)])
def test_u8_luma_bit_exact_against_pillow(dev, size):
    rng = np.random.RandomState(size[0] + size[1])
    img = rng.randint(0, 256, (2,) + size + (3,)).astype(np.uint8)
    got = ops.u8_luma(torch.from_numpy(img).to(dev)).cpu().numpy()
    for k in range(2):
        assert np.array_equal(got[k], np.asarray(Image.fromarray(img[k]).convert("L").convert("RGB")))


def test_lpips_preprocessing_equals_pil(dev):
    """luma -> Pillow-exact bicubic resize -> normalise with the folded ScalingLayer, against the PIL calls of the reference
    followed by x * 2 - 1 and the ScalingLayer in float64; 1e-5 is the bar of test_preprocessing_equals_pil.  (96, 128) upsamples."""
    model = filters.LpipsAlex(W.synth_state_dict("lpips_alex", CFG.tiny_filters()["lpips_alex"], 1), CFG.tiny_filters()["lpips_alex"], dev)
    for (h, w) in ((512, 512), (512, 704), (640, 512), (100, 333), (96, 128)):
        img = synthetic_image(h, w, 3)
        d = torch.from_numpy(img)[None].to(dev)
        for grey in (True, False):
            px = model.preprocess(d, (256, 256), grey)
            assert tuple(px.shape) == (1, 256, 256, 8) and bool((px[..., 3:] == 0).all())
            ref = LR.scaling(LR.pil_input(img, (256, 256), grey)[None])[0]
            err = (from_nhwc(px, 3)[0].double() - ref).abs().max().item()
            print(f"preprocess {h}x{w} grey={grey}: max |d| = {err:.3g}")
            assert err < 1e-5, (h, w, grey, err)
    img = synthetic_image(80, 72, 4)                                            # resize=None keeps the size
    px = model.preprocess(torch.from_numpy(img)[None].to(dev), None, True)
    assert (from_nhwc(px, 3)[0].double() - LR.scaling(LR.pil_input(img, None, True)[None])[0]).abs().max() < 1e-5


# ---- the layer kernel -------------------------------------------------------------------------------------------------------
def _operands(hw, c, dtype, seed, n=5, m=3):
    """Post-ReLU-like features (non-negative, many exact zeros, a per-pixel magnitude between 0.02 and 0.2), the special rows
    the issue names, a non-monotone many-to-one index.  Returns host tensors ALREADY rounded to the storage dtype."""
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(n, hw, c, generator=g)) * (0.02 + 0.18 * torch.rand(n, hw, 1, generator=g))
    r = torch.relu(torch.randn(m, hw, c, generator=g)) * (0.02 + 0.18 * torch.rand(m, hw, 1, generator=g))
    idx = [2, 0, 2, 1, 0][:n]
    a[0, 0] = 0                                       # zero in one input
    a[1, hw // 2] = 0
    r[idx[1], hw // 2] = 0                            # zero in both
    a[2, hw - 1] = r[idx[2], hw - 1]                  # an identical row
    a[3] = r[idx[3]]                                  # an identical pair: the distance is exactly 0.0
    w = torch.rand(c, generator=g) * (2.0 / c)
    return a.to(dtype).float(), r.to(dtype).float(), idx, w


def _run(dev, a, r, idx, w, dtype, pitch_pad=0, **kw):
    def up(t):
        if not pitch_pad:
            return t.to(dev, dtype).contiguous()
        buf = torch.full(t.shape[:-1] + (t.shape[-1] + pitch_pad,), 7.0, device=dev, dtype=dtype)      # junk in the pitch padding
        buf[..., :t.shape[-1]] = t.to(dev, dtype)
        return buf[..., :t.shape[-1]]
    return ops.lpips_layer(up(a), up(r), torch.tensor(idx, dtype=torch.int32, device=dev), w.to(dev), **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw,c", PRODUCTION[:4] + TINY + ODD)
def test_lpips_layer_against_float64_reference(dev, dtype, hw, c):
    """|got - ref| <= 2^-20 * T_j, T_j = mean_p sum_c w_c (|a_hat| + |r_hat|)^2 of the normalised values: about 16 fp32 roundings of
    the terms (three in each normalisation, the subtraction, the square and the weight, log-depth sums of non-negative terms).
    The reference is float64 on the same operands (the bf16-rounded ones for bf16 storage).  Negative controls: four wrong
    formulas, each evaluated in float64, must miss by more than twice the bound -- the bound separates them from the kernel."""
    a, r, idx, w = _operands(hw, c, dtype, 100 + hw + c)
    ref = LR.layer(a, r, idx, w)
    bound = LR.layer_scale(a, r, idx, w) * 2.0 ** -20
    got = _run(dev, a, r, idx, w, dtype).cpu()
    again = _run(dev, a, r, idx, w, dtype, pitch_pad=8).cpu()
    assert torch.equal(got, again), "two runs (the second with a pixel pitch > C) must be bit-equal"
    err = (got.double() - ref).abs()
    print(f"lpips_layer hw={hw} C={c} {dtype}: max err / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).tolist()
    assert got[3].item() == 0.0, "identical inputs: exactly 0.0"
    assert bool(torch.isfinite(got).all())
    # accumulate: the level is added to what the vector holds (one fp32 addition)
    base = torch.rand(len(idx), generator=torch.Generator().manual_seed(1))
    acc = _run(dev, a, r, idx, w, dtype, dist=base.clone().to(dev), accumulate=True).cpu()
    assert torch.equal(acc, base + got)
    # negative controls (float64)
    ad, rd, wd = a.double(), r.double()[torch.tensor(idx)], w.double()

    def dist(ua, ur, weights=wd, count=hw):
        d = ua - ur
        return (d * d * weights).sum(-1).sum(-1) / count

    def unit_eps_inside(x):
        return x / torch.sqrt((x * x).sum(-1, keepdim=True) + 1e-3)

    def unit_no_root(x):
        return x / ((x * x).sum(-1, keepdim=True) + LR.EPS)
    controls = {"eps inside the root at 1e-3": dist(unit_eps_inside(ad), unit_eps_inside(rd)),
                "weights rotated by one channel": dist(LR.unit(ad, -1), LR.unit(rd, -1), wd.roll(1)),
                "the norm without the root": dist(unit_no_root(ad), unit_no_root(rd))}
    if hw > 1:
        controls["mean over hw - 1"] = dist(LR.unit(ad, -1), LR.unit(rd, -1), count=hw - 1)
    live = [j for j in range(len(idx)) if j != 3]                            # pair 3 is 0 under every formula
    for name, wrong in controls.items():
        miss = ((wrong - ref).abs() / bound)[live]
        assert bool((miss > 2.0).all()), (name, miss.tolist())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw,c", [PRODUCTION[0], PRODUCTION[2], TINY[1]])
def test_lpips_layer_result_is_independent_of_the_batch(dev, dtype, hw, c):
    """A pair run alone is bit-equal to the same pair at any position of a batch of 32 (and with its original alone)."""
    g = torch.Generator().manual_seed(hw * c)
    a = torch.relu(torch.randn(32, hw, c, generator=g)).to(dev, dtype)
    r = torch.relu(torch.randn(4, hw, c, generator=g)).to(dev, dtype)
    w = (torch.rand(c, generator=g) / c).to(dev)
    idx = torch.tensor([(5 * k + 3) % 4 for k in range(32)], dtype=torch.int32, device=dev)
    full = ops.lpips_layer(a, r, idx, w)
    assert torch.equal(full, ops.lpips_layer(a, r, idx, w))
    for k in (0, 1, 7, 30, 31):
        alone = ops.lpips_layer(a[k:k + 1], r, idx[k:k + 1].clone(), w)
        assert alone[0].item() == full[k].item(), k
        i = int(idx[k])
        alone = ops.lpips_layer(a[k:k + 1], r[i:i + 1], torch.zeros(1, dtype=torch.int32, device=dev), w)
        assert alone[0].item() == full[k].item(), k
    for bsz in (3, 16):
        part = ops.lpips_layer(a[8:8 + bsz], r, idx[8:8 + bsz].clone(), w)
        assert torch.equal(part, full[8:8 + bsz])


def test_lpips_layer_wrapper_shape_checks(dev):
    a = torch.zeros(2, 9, 16, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    w = torch.ones(16, device=dev)
    with pytest.raises(ValueError):
        ops.lpips_layer(a, torch.zeros(2, 8, 16, device=dev), idx, w)                    # pixel counts differ
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a.bfloat16(), idx, w)
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a, idx.long(), w)
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a, idx, torch.ones(8, device=dev))
    with pytest.raises(ValueError):
        ops.lpips_layer(torch.zeros(2, 9, 12, device=dev), torch.zeros(2, 9, 12, device=dev), idx, torch.ones(12, device=dev))
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a, idx, w, accumulate=True)


# ---- the whole model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["tiny", "full"])
def test_lpips_alex_vs_float64_reference(dev, full):
    cfg = CFG.LPIPS_ALEX if full else CFG.tiny_filters()["lpips_alex"]
    sd = W.synth_state_dict("lpips_alex", cfg, 21)
    model = filters.LpipsAlex(sd, cfg, dev)
    refs = [synthetic_image(256, 256, 40), synthetic_image(256, 256, 41)]
    augs = [synthetic_image(256, 256, 50 + k) for k in range(5)]
    idx = [1, 0, 1, 1, 0]
    for grey in (True, False):
        got = model.forward(torch.from_numpy(np.stack(augs)).to(dev), torch.from_numpy(np.stack(refs)).to(dev), idx, resize=None,
                            grey=grey).cpu().double()
        want = torch.tensor([LR.distance(sd, refs[i], augs[j], None, grey) for j, i in enumerate(idx)], dtype=torch.float64)
        rel = ((got - want).abs() / want).max().item()
        print(f"LpipsAlex full={full} grey={grey}: distances {want.min().item():.4g} .. {want.max().item():.4g}, max rel err = {rel:.3g} "
              f"({rel / MODEL_RTOL:.3f} of the bound)")
        assert rel <= MODEL_RTOL, rel
    # resized inputs of unequal sizes, and the same image twice
    a = torch.from_numpy(synthetic_image(96, 128, 60))[None].to(dev)
    r = torch.from_numpy(synthetic_image(300, 200, 61))[None].to(dev)
    got = model.forward(a, r, [0]).item()
    want = LR.distance(sd, synthetic_image(300, 200, 61), synthetic_image(96, 128, 60))
    assert abs(got - want) <= MODEL_RTOL * want
    assert model.forward(r, r, [0]).item() == 0.0
    with pytest.raises(ValueError):
        model.forward(a, r, [0], resize=None)                                   # unequal sizes without resize
    with pytest.raises(ValueError):
        model.forward(a, r, [1])                                                # ref_index is checked on the host
    with pytest.raises(ValueError):
        model.forward(a, r, [-1])


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _tree(tmp_path):
    root = tmp_path / "ds/data"
    ds = DU.SyntheticUtils(root_path=str(root), n_images=6, sizes=((64, 64), (96, 80), (72, 120)), print_func=lambda *a, **k: None)
    folder = root / "aug_data/controlnet/sd_v1.5/canny/run_seed_1/images"
    folder.mkdir(parents=True)
    files = {}
    for k, p in enumerate(ds.original_images_paths):
        stem = Path(p).stem
        for v in range(3):
            img = synthetic_image(64 if v < 2 else 96, 64 if v < 2 else 128, 100 + 10 * k + v)
            name = f"{stem}_prompt_An airplane, oil painting_{v}.png"
            Image.fromarray(img).save(folder / name)
            files[str(folder / name)] = (p, img)
        Image.fromarray(synthetic_image(64, 64, k)).save(folder / f"{stem}_source.png")
    return ds, folder, files


def _thresholds(dists):
    """lpips_min / lpips_max in gaps of the sorted reference distances: every distance at least 10 x (3e-4 x the largest) from
    either threshold and at least one image on each side of each -- asserted, not assumed."""
    v = sorted(dists)
    margin = 10 * MODEL_RTOL * v[-1]
    gaps = [(v[i + 1] - v[i], i) for i in range(len(v) - 1) if v[i + 1] - v[i] >= 2 * margin]
    assert len(gaps) >= 2, f"the reference distances {v} leave no two gaps of {2 * margin:.3g}"
    lo, hi = min(i for _, i in gaps), max(i for _, i in gaps)
    lmin, lmax = (v[lo] + v[lo + 1]) / 2, (v[hi] + v[hi + 1]) / 2
    for t in (lmin, lmax):
        assert min(abs(d - t) for d in v) >= margin
        assert any(d < t for d in v) and any(d > t for d in v)
    assert lmin < lmax
    return lmin, lmax


def test_lpips_filter_decisions_counters_and_json_end_to_end(dev, tmp_path, caplog):
    """Tiny models through create_json on a SyntheticUtils tree (originals of three sizes, three augmentations each in two
    sizes): LPIPS alone and with both other filters.  The JSON lists equal the reference's decisions (PIL pre-processing +
    float64 LPIPS; the oracle models for the other two), the logged counters its order of attribution (top-k, LPIPS, semantic),
    the file name carries the lpips parts.  All 18 pairs are covered."""
    cf = CFG.tiny_filters(num_classes=6)
    ds, folder, files = _tree(tmp_path)
    sd_l = W.synth_state_dict("lpips_alex", cf["lpips_alex"], 33)
    lp = filters.LpipsAlex(sd_l, cf["lpips_alex"], dev)
    ref_d = {path: LR.distance(sd_l, orig, path) for path, (orig, _) in files.items()}
    assert len(ref_d) == 18
    lmin, lmax = _thresholds(list(ref_d.values()))
    print(f"reference distances {min(ref_d.values()):.4g} .. {max(ref_d.values()):.4g}; lpips_min = {lmin:.5g}, lpips_max = {lmax:.5g}")
    ok_l = {path: lmin <= d <= lmax for path, d in ref_d.items()}
    # the other two filters, as in test_filter_decisions_and_json_end_to_end
    sd_c, sd_w = W.synth_state_dict("clip_rn50", cf["clip_rn50"], 31), W.synth_state_dict("cal", cf["cal"], 32)
    tok = HashTokenizer(cf["clip_rn50"]["vocab"], pad_id=0)
    sem = filters.SemanticFilter(sd_c, cf["clip_rn50"], dev, ds.get_basic_prompt(), tok)
    conf = filters.ConfidenceFilter(sd_w, cf["cal"], dev, top_k=3)
    labels = ds.get_image_path_to_class_id_dict()
    ids = torch.from_numpy(np.concatenate([tok(pr) for pr in sem.prompts]))
    ok_c, ok_s = {}, {}
    for path, (orig, img) in files.items():
        with torch.no_grad():
            lg_c = FM.wsdan_cal_logits(sd_w, cf["cal"], FM.cal_preprocess(img, (64, 64))[None])[0]
            lg_s = FM.clip_selector_logits(sd_c, cf["clip_rn50"], FM.rn50_preprocess(img, 64)[None], ids)[0]
        ok_c[path] = bool(FM.confidence_pass(lg_c[None], labels[orig], 3))
        ok_s[path] = bool(FM.semantic_pass(lg_s[None])[0])

    def logged(what):
        hits = [int(m.group(1)) for rec in caplog.records for m in [re.match(rf"For filter = {what}, filtered (\d+) images", rec.getMessage())] if m]
        assert len(hits) == 1, (what, hits)
        return hits[0]

    for use_s, use_c in ((0, 0), (1, 1)):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            jp = utils.create_json_of_image_name_to_augmented_images_paths(
                ds, str(folder), lpips_min=lmin, lpips_max=lmax, semantic_filtering=use_s, model_confidence_based_filtering=use_c,
                conf_top_k=3, init_log=False, original_images_paths=ds.original_images_paths, min_files=1,
                filter_models=(sem, conf) if use_s else None, lpips_model=lp, device=dev)
        assert Path(jp).name.startswith(f"lpips_min_{lmin}-lpips_max_{lmax}-")
        assert Path(jp) == Path(utils.get_aug_json_path(str(folder), lmin, lmax, semantic_filtering=use_s,
                                                        model_confidence_based_filtering=use_c, conf_top_k=3))
        want = {Path(p).name: [] for p in ds.original_images_paths}
        n_c = n_l = n_s = 0
        for path, (orig, _) in files.items():
            c_ok, s_ok = ok_c[path] or not use_c, ok_s[path] or not use_s
            if not c_ok:
                n_c += 1
            elif not ok_l[path]:
                n_l += 1
            elif not s_ok:
                n_s += 1
            else:
                want[Path(orig).name].append(path)
        got = {k: sorted(v) for k, v in json.load(open(jp)).items()}
        assert got == {k: sorted(v) for k, v in want.items()}, (use_s, use_c)
        assert logged("lpips_min") == n_l and logged("lpips_max") == n_l
        if use_s:
            assert logged("semantic_filtering") == n_s and logged("not_in_top_3") == n_c
    assert 0 < sum(ok_l.values()) < len(files)
    # the batch cut does not move a decision
    mapping = utils.match_augmented_images(ds.original_images_paths, sorted(p.name for p in folder.iterdir()), str(folder))
    outs = [filters.apply_filters(mapping, ds.original_images_paths, ds, dev, lpips=lp, lpips_min=lmin, lpips_max=lmax, batch_size=b)
            for b in (1, 5, 32)]
    assert outs[0] == outs[1] == outs[2] and outs[0][1] == dict(not_in_top_k=0, semantic=0, lpips=sum(not v for v in ok_l.values()))


def test_calc_lpips_given_aug_json(dev, tmp_path):
    """The diversity measure on the same tree: RGB, no grey conversion.  Every value is within the model bound (relative 3e-4) of
    the float64 reference, hence the mean within 3e-4 of the reference mean and the population std within 3e-4 x the largest
    distance (|std(x + e) - std(x)| <= max |e|)."""
    cf = CFG.tiny_filters()
    ds, folder, files = _tree(tmp_path)
    sd_l = W.synth_state_dict("lpips_alex", cf["lpips_alex"], 33)
    lp = filters.LpipsAlex(sd_l, cf["lpips_alex"], dev)
    jp = utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, min_files=1,
                                                                   original_images_paths=ds.original_images_paths)
    assert Path(jp).name == "aug.json"
    mean, std, values = utils.calc_lpips_given_aug_json(ds, jp, net="alex", resize_to=(256, 256), lpips_model=lp)
    body = json.load(open(jp))
    want = [LR.distance(sd_l, files[ap][0], ap, (256, 256), grey=False) for name, aps in body.items() for ap in aps]
    assert len(values) == len(want) == 18
    rel = max(abs(g - w) / w for g, w in zip(values, want))
    print(f"calc_lpips_given_aug_json: mean {mean:.6g} (ref {np.mean(want):.6g}), std {std:.6g} (ref {np.std(want):.6g}), max rel err {rel:.3g}")
    assert rel <= MODEL_RTOL
    assert abs(mean - np.mean(want)) <= MODEL_RTOL * np.mean(want)
    assert abs(std - np.std(want)) <= MODEL_RTOL * max(want)
    grey = [LR.distance(sd_l, files[ap][0], ap, (256, 256), grey=True) for aps in body.values() for ap in aps]
    assert abs(np.mean(grey) - mean) > 10 * MODEL_RTOL * mean, "the measure is RGB: the grey distances differ"
    with pytest.raises(ValueError):
        utils.calc_lpips_given_aug_json(ds, jp, lpips_model=lp)                 # mixed sizes without resize_to
    with pytest.raises(NotImplementedError):
        utils.calc_lpips_given_aug_json(ds, jp, net="vgg", lpips_model=lp)
