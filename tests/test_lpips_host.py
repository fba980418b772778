"""LPIPS min / max filter and diversity measure, host side (no GPU): the two new entry points and their host-side refusals, the
integer luma against Pillow, the reference's pre-processing calls against the installed Pillow, the float64 restatement's own
properties (tests/lpips_ref.py), parameter counts, checkpoint loading / refusal, and the settings -> file-name plumbing."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, filters, utils
from saspa_aug_amd import config as CFG
from saspa_aug_amd import dataset_utils as DU
from saspa_aug_amd import run_aug as R
from saspa_aug_amd import weights as W
from saspa_aug_amd.synthetic import synthetic_image
from tests import lpips_ref as LR


def test_symbols_exported_and_abi_unchanged():
    lib = _lib.load()
    for name in ("saspa_lpips_layer", "saspa_u8_luma"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.saspa_abi_version() == 20


def test_lpips_layer_host_side_refusals_need_no_gpu():
    lib = _lib.load()
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) // 16 * 16
    F32, BF16 = _lib.SASPA_F32, _lib.SASPA_BF16

    def call(dtype=F32, a=base, lda=64, r=base, ldr=64, idx=base, w=base, dist=base, ws=base, n=2, hw=9, c=64, acc=0):
        return lib.saspa_lpips_layer(dtype, a, lda, r, ldr, idx, w, dist, ws, n, hw, c, acc, None)
    for null in ("a", "r", "idx", "w", "dist", "ws"):
        assert call(**{null: None}) == _lib.SASPA_EINVAL, null
    assert call(dtype=_lib.SASPA_F32X3) == _lib.SASPA_EINVAL and call(dtype=7) == _lib.SASPA_EINVAL      # storage dtype
    assert call(n=0) == _lib.SASPA_EINVAL and call(n=-3) == _lib.SASPA_EINVAL
    assert call(hw=0) == _lib.SASPA_EINVAL and call(c=0) == _lib.SASPA_EINVAL
    assert call(c=60, lda=64, ldr=64) == _lib.SASPA_EALIGN                                                # C % 8
    assert call(lda=68) == _lib.SASPA_EALIGN and call(ldr=60) == _lib.SASPA_EALIGN                        # pitch % 8
    assert call(lda=56) == _lib.SASPA_EALIGN                                                              # pitch < C
    assert call(a=base + 4) == _lib.SASPA_EALIGN and call(r=base + 8, dtype=BF16) == _lib.SASPA_EALIGN    # unaligned base
    assert call(w=base + 4) == _lib.SASPA_EALIGN
    assert call(c=_lib.LPIPS_MAX_C + 8, lda=1024, ldr=1024) == _lib.SASPA_ERANGE                          # register plan
    assert call(n=70000) == _lib.SASPA_ERANGE
    assert lib.saspa_u8_luma(None, base, 4, None) == _lib.SASPA_EINVAL
    assert lib.saspa_u8_luma(base, base, 0, None) == _lib.SASPA_EINVAL


@pytest.mark.parametrize("size", [(1, 1), (7, 13), (64, 64), (33, 250)])
def test_luma_restatement_equals_pillow(size):
    rng = np.random.RandomState(size[0] * 1000 + size[1])
    img = rng.randint(0, 256, size + (3,)).astype(np.uint8)
    img[0, 0] = (255, 255, 255)
    assert np.array_equal(LR.luma(img), np.asarray(Image.fromarray(img).convert("L")))
    back = np.asarray(Image.fromarray(img).convert("L").convert("RGB"))
    assert np.array_equal(back, np.repeat(LR.luma(img)[..., None], 3, -1))


def test_luma_is_exhaustively_the_identity_on_greys():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(LR.luma(np.stack([v, v, v], -1)), v)


@pytest.mark.parametrize("size", [(512, 512), (100, 333), (96, 128)])
def test_reference_preprocessing_is_explicit_bicubic_on_this_pillow(size):
    """`Image.resize(size)` without a filter argument is BICUBIC on the installed Pillow, and resizing the replicated grey
    image equals resizing the grey one -- what lets the device luma kernel sit in front of the unchanged resize."""
    im = Image.fromarray(synthetic_image(size[0], size[1], 5))
    ref = np.asarray(im.convert("L").convert("RGB").resize((256, 256)))
    assert np.array_equal(ref, np.asarray(im.convert("L").convert("RGB").resize((256, 256), Image.BICUBIC)))
    grey = np.asarray(im.convert("L").resize((256, 256), Image.BICUBIC))
    assert np.array_equal(ref, np.repeat(grey[..., None], 3, -1))


def test_scaling_layer_folds_into_mean_and_std():
    x = torch.rand(1, 3, 5, 5, dtype=torch.float64)
    mean = torch.tensor([(1 + s) / 2 for s in CFG.LPIPS_SHIFT], dtype=torch.float64)[None, :, None, None]
    std = torch.tensor([s / 2 for s in CFG.LPIPS_SCALE], dtype=torch.float64)[None, :, None, None]
    assert (LR.scaling(x * 2 - 1) - (x - mean) / std).abs().max() < 1e-14
    assert LR.SHIFT == CFG.LPIPS_SHIFT and LR.SCALE == CFG.LPIPS_SCALE


def test_float64_reference_properties():
    g = torch.Generator().manual_seed(0)
    a, r = torch.randn(3, 11, 16, generator=g, dtype=torch.float64), torch.randn(2, 11, 16, generator=g, dtype=torch.float64)
    w = torch.rand(16, generator=g, dtype=torch.float64)
    idx = [1, 0, 1]
    d = LR.layer(a, r, idx, w)
    assert (d >= 0).all() and (d > 0).any()
    assert torch.equal(LR.layer(a, a, [0, 1, 2], w), torch.zeros(3, dtype=torch.float64))           # d(x, x) == 0
    assert torch.allclose(LR.layer(r[idx], a, [0, 1, 2], w), d, rtol=0, atol=1e-15)                  # symmetry
    sa, sr = torch.rand(3, 11, 1, generator=g, dtype=torch.float64) + 0.1, torch.rand(2, 11, 1, generator=g, dtype=torch.float64) * 50 + 1
    assert torch.allclose(LR.layer(a * sa, r * sr, idx, w), d, rtol=1e-9, atol=1e-15)                # per-pixel positive scaling
    z = a.clone()
    z[0, 3] = 0                                                                                      # an all-zero pixel vector
    assert torch.isfinite(LR.layer(z, r, idx, w)).all() and torch.isfinite(LR.layer(z, z, [0, 1, 2], w)).all()
    # one pixel, two channels, by hand: a = (3, 4) -> (0.6, 0.8); r = (1, 0) -> (1, 0); w = (2, 0.5): 2 * 0.16 + 0.5 * 0.64 = 0.64
    one = LR.layer(torch.tensor([[[3.0, 4.0]]]), torch.tensor([[[1.0, 0.0]]]), [0], torch.tensor([2.0, 0.5]))
    assert abs(one.item() - 0.64) < 1e-9
    assert abs(LR.layer_scale(torch.tensor([[[3.0, 4.0]]]), torch.tensor([[[1.0, 0.0]]]), [0], torch.tensor([2.0, 0.5])).item() - (2 * 2.56 + 0.5 * 0.64)) < 1e-9


def test_parameter_counts_and_synthetic_weights():
    sd = W.synth_state_dict("lpips_alex", CFG.LPIPS_ALEX, 3)
    nf = sum(v.numel() for k, v in sd.items() if k.startswith("features."))
    nl = sum(v.numel() for k, v in sd.items() if k.startswith("lin"))
    assert (nf, nl) == (2469696, 1152) == (filters.N_PARAMS_ALEX_FEATURES, filters.N_PARAMS_LPIPS_LIN)
    assert all((v >= 0).all() for k, v in sd.items() if k.startswith("lin"))
    tiny = CFG.tiny_filters()["lpips_alex"]
    assert all(c % 8 == 0 for c in tiny["channels"]) and set(CFG.tiny_filters()) >= {"clip_rn50", "cal", "lpips_alex"}
    # the reference model runs on them (AlexNet needs at least 63 x 63 pixels to reach the last pool)
    x = torch.rand(2, 3, 64, 64, dtype=torch.float64) * 2 - 1
    d = LR.lpips_alex(W.synth_state_dict("lpips_alex", tiny, 1), x, x.flip(0))
    assert d.shape == (2,) and (d > 0).all() and abs(d[0] - d[1]) < 1e-12
    assert [f.shape[1:] for f in LR.alex_features(sd, torch.zeros(1, 3, 256, 256, dtype=torch.float64))] == \
        [(64, 63, 63), (192, 31, 31), (384, 15, 15), (256, 15, 15), (256, 15, 15)]


def _write_checkpoints(d, sd):
    """The two files in the layout of torchvision's AlexNet (features + classifier) and of the lpips package's alex.pth."""
    d.mkdir(parents=True)
    net = {k: v for k, v in sd.items() if k.startswith("features.")}
    net["classifier.1.weight"], net["classifier.1.bias"] = torch.zeros(4, 4), torch.zeros(4)
    torch.save(net, d / "alexnet-owt-7be5be79.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, d / "alex.pth")


def test_checkpoints_load_and_are_required(tmp_path, monkeypatch):
    monkeypatch.delenv("SASPA_SYNTHETIC_FILTERS", raising=False)
    with pytest.raises(FileNotFoundError, match="LPIPS filter"):
        filters.lpips_checkpoints(None)
    with pytest.raises(FileNotFoundError, match="LPIPS filter"):
        filters.lpips_checkpoints(str(tmp_path / "nothing"))
    sd = W.synth_state_dict("lpips_alex", CFG.LPIPS_ALEX, 4)
    _write_checkpoints(tmp_path / "w" / "lpips", sd)
    net, lin = filters.lpips_checkpoints(str(tmp_path / "w"))
    got = filters.load_lpips_alex(net, lin)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    (tmp_path / "w" / "lpips" / "alex.pth").unlink()
    with pytest.raises(FileNotFoundError, match="LPIPS filter"):
        filters.lpips_checkpoints(str(tmp_path / "w"))
    monkeypatch.setenv("SASPA_SYNTHETIC_FILTERS", "1")
    assert filters.lpips_checkpoints(None) == (None, None)


class _Reached(Exception):
    pass


class _Generator:
    def __call__(self, *a, **k):
        raise _Reached()


def _settings(**kw):
    return R.Settings(DATASET="synthetic", NUM_PER_IMAGE=1, RESOLUTION=64, USE_ARTISTIC_PROMPTS=False, PROMPT_WITH_SUB_CLASS=False,
                      SEMANTIC_FILTERING=0, MODEL_CONFIDENCE_BASED_FILTERING=0, **kw)


def test_main_checks_the_lpips_checkpoints_before_generating(tmp_path, monkeypatch):
    monkeypatch.delenv("SASPA_SYNTHETIC_FILTERS", raising=False)
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=4, sizes=((64, 64),), print_func=lambda *a: None)

    class Boom:
        def __getattr__(self, name):
            raise AssertionError("the batch generator must not be touched")

    with pytest.raises(FileNotFoundError, match="LPIPS filter"):
        R.main(_settings(LPIPS_MIN=0.1, LPIPS_MAX=0.6), ds_utils=ds, batch_generator=Boom())
    with pytest.raises(ValueError, match="both bounds"):
        R.main(_settings(LPIPS_MIN=0.1), ds_utils=ds, batch_generator=Boom())
    # opted in to synthetic filter weights: the check passes and generation starts
    monkeypatch.setenv("SASPA_SYNTHETIC_FILTERS", "1")
    with pytest.raises(_Reached):
        R.main(_settings(LPIPS_MIN=0.1, LPIPS_MAX=0.6), ds_utils=ds, batch_generator=_Generator())


def test_settings_defaults_and_file_name(tmp_path, caplog):
    s = R.Settings()
    assert s.LPIPS_MIN is None and s.LPIPS_MAX is None
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=2, sizes=((64, 64),), print_func=lambda *a: None)
    s = _settings(LPIPS_MIN=0.1, LPIPS_MAX=0.6)
    want = utils.get_aug_json_path(R.output_folder_for(s, ds.root_path), lpips_min=0.1, lpips_max=0.6)
    assert Path(want).name == "lpips_min_0.1-lpips_max_0.6-aug.json"
    import logging
    with caplog.at_level(logging.INFO):
        with pytest.raises(_Reached):
            R.main(s, ds_utils=ds, batch_generator=_Generator(), lpips_model=object())
    assert any(want in rec.getMessage() for rec in caplog.records), "main announces the file name get_aug_json_path gives"


def test_one_bound_alone_and_the_other_baseline_filters(tmp_path):
    ds = DU.SyntheticUtils(root_path=str(tmp_path / "data"), n_images=2, sizes=((64, 64),), print_func=lambda *a: None)
    folder = tmp_path / "aug/images"
    folder.mkdir(parents=True)
    touched = []

    class Model:
        dev = "cpu"

        def __getattr__(self, name):
            touched.append(name)
            raise AssertionError(name)
    for kw in (dict(lpips_min=0.2), dict(lpips_max=0.5), dict(lpips_min=0.2, lpips_max=None)):
        with pytest.raises(ValueError, match="both bounds"):
            utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, lpips_model=Model(),
                                                                      original_images_paths=ds.original_images_paths, **kw)
    assert not touched and not list(folder.parent.glob("*.json")), "nothing is read or written before the refusal"
    with pytest.raises(NotImplementedError):
        utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, clip_filtering=True)
    with pytest.raises(NotImplementedError):
        utils.create_json_of_image_name_to_augmented_images_paths(ds, str(folder), init_log=False, alia_conf_filtering=True)
    with pytest.raises(NotImplementedError):
        utils.calc_lpips_given_aug_json(ds, str(tmp_path / "x.json"), net="vgg")
    assert filters.lpips_bounds(None, None) is False and filters.lpips_bounds(0, 0.5) is True and filters.lpips_bounds(0.1, 0.5) is True
