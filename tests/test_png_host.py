"""The device PNG encoder without a device: the integer model (tests/png_ref.py) produces valid PNGs that decode exactly and covers
every branch of the format; its size against zlib's Huffman-only coder; the capacity bound; the library's host-side entry points;
the framing writer of run_aug; and the rule that nothing of the feature is imported while it is off."""
import ctypes as C
import io
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, pngenc
from saspa_aug_amd import run_aug as R

from tests import png_ref as P

_IDS = ["x".join(map(str, s)) for s in P.SHAPES]


def _smooth_noise(h, w, sigma, seed):
    """The smooth-plus-noise RGB image of the size measurements."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(x / 17.0) * np.cos(y / 13.0) + 30 * np.sin((x + y) / 29.0)
    img = base[..., None] + np.array([0, 9, -14]) + rng.normal(0, sigma, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", P.SHAPES, ids=_IDS)
def test_model_output_is_a_png_that_decodes_exactly(shape):
    for content in P.CONTENTS:
        img = P.make_image(shape, content)
        z, _ = P.deflate(img)
        assert zlib.decompress(z) == P.filter_rows(img, 0, shape[0])[0].tobytes()        # segments filter like the whole image
        data = P.frame(z, *shape)
        assert data == pngenc.frame(z, *shape)
        with Image.open(io.BytesIO(data)) as im:
            im.verify()
        with Image.open(io.BytesIO(data)) as im:
            assert im.mode == ("RGB" if shape[2] == 3 else "L") and im.size == (shape[1], shape[0])
            assert np.array_equal(np.asarray(im).reshape(shape), img), (shape, content)
        assert len(z) <= P.capacity(*shape)


def test_inputs_cover_every_branch_of_the_format():
    """Over the (shape, content) set of the GPU suite: all five filters chosen, a code of length 15, the stored fallback, Huffman
    segments, the single-literal code.

    Pad symbols: the construction leaves NO slack, so they never occur and neither the model's output nor the kernel has a use for
    them -- every weight 2^(15 - l) in use is a multiple of the smallest one, hence so is the slack 2^15 - sum; while it is positive
    the symbol of the longest code (l > 1, as two used symbols of length 1 already fill the code) can still be shortened, so the
    walk only stops at slack 0.  What is asserted instead is that consequence: every Huffman segment's code is complete (the model
    asserts the Kraft sum is exactly 1, which is what zlib demands) and uses no symbol above 256."""
    filters, maxlen, stored, huffman, single, pads = set(), 0, 0, 0, False, 0
    for shape in P.SHAPES:
        for content in P.CONTENTS:
            _, info = P.deflate(P.make_image(shape, content))
            filters |= info["filters"]
            maxlen = max(maxlen, info["maxlen"])
            stored += info["stored"]
            huffman += info["huffman"]
            single |= info["single"]
            pads = max(pads, info["pads"])
    assert filters == {0, 1, 2, 3, 4}
    assert maxlen == 15
    assert stored > 0 and huffman > 0
    assert single
    assert pads == 0
    # the slack argument, on histograms of every flavour: complete codes, nothing above end-of-block
    rng = np.random.RandomState(5)
    for trial in range(200):
        n = int(rng.randint(1, 257))
        hist = np.zeros(257, np.int64)
        syms = rng.choice(256, n, replace=False)
        hist[syms] = np.maximum(1, (rng.pareto(0.7, n) * 3).astype(np.int64)) if trial % 2 else rng.randint(1, 40, n)
        hist = np.minimum(hist, 32767 // n)
        hist[syms] = np.maximum(hist[syms], 1)
        hist[256] = 1
        lens, npad = P.code_lengths(hist, int(hist.sum()))
        assert npad == 0 and not any(lens[257:]) and all((lens[s] > 0) == (hist[s] > 0) for s in range(257))


def _size_set():
    imgs = [P.make_image(s, c) for s in P.SHAPES for c in P.CONTENTS]
    imgs += [_smooth_noise(96, 80, sigma, 11 + k) for k, sigma in enumerate((2, 6, 16))]
    return imgs


def test_huffman_segments_against_zlib_huffman_only():
    """Per Huffman segment: its bytes in the stream (153-byte header, body, end-of-block; the 5-byte join marker of a segment that is
    not the last taken off) against raw deflate of the same filtered bytes by zlib.compressobj(9, DEFLATED, -15, 9, Z_HUFFMAN_ONLY)
    -- optimal codes, run-length coded code lengths -- PLUS the 153 bytes of the flat header.  That reference isolates the code
    construction: without the allowance the ratio of a tiny, highly compressible segment is all header (16x5x3 zeros: 185 bytes
    against zlib's 44, 4.20x) and says nothing about the codes.
    Measured over the GPU suite's (shape, content) set plus 96x80 smooth-plus-noise images at sigma 2 / 6 / 16: worst ratio 1.0178
    (12x1100x3 smooth-plus-noise, second segment: 6018 bytes against 5760 + 153).  Without the allowance the 96x80 images give at
    worst 1.0956 (sigma 2), 1.0495 (sigma 6), 1.0405 (sigma 16).  Both are asserted with 2 % slack."""
    worst, worst_plain_96 = 0.0, 0.0
    for img in _size_set():
        _, info = P.deflate(img)
        for k, (raw, seg, stored) in enumerate(info["segments"]):
            if stored:
                continue
            co = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
            ref = len(co.compress(raw) + co.flush())
            ours = len(seg) - (0 if k == len(info["segments"]) - 1 else 5)
            worst = max(worst, ours / (ref + P.HEADER_BYTES))
            if img.shape == (96, 80, 3):
                worst_plain_96 = max(worst_plain_96, ours / ref)
    print(f"worst ratio with the header allowance {worst:.4f}, 96x80 without it {worst_plain_96:.4f}")
    assert 0.9 < worst <= 1.0178 * 1.02
    assert 1.0 < worst_plain_96 <= 1.0956 * 1.02


def test_capacity_is_a_hard_bound():
    rng = np.random.RandomState(3)
    for shape in P.SHAPES + [(40, 33, 3), (5, 10922, 3), (3, 32766, 1)]:
        img = rng.randint(0, 256, shape).astype(np.uint8)
        z, info = P.deflate(img)
        rowbytes, _, nseg = P.geometry(*shape)
        assert len(z) <= P.capacity(*shape)
        assert len(z) <= shape[0] * rowbytes + 5 * nseg + 6                  # uniform noise: filtered size + 5 per segment + 6
        assert info["stored"] > 0
    with pytest.raises(ValueError):
        P.capacity(4, 10923, 3)


def test_library_capacity_and_host_side_refusals():
    lib = _lib.load()
    for h, w, c in P.SHAPES + [(512, 512, 3), (512, 704, 3), (1024, 1024, 3), (7, 10922, 3), (100000, 3, 1), (1, 32766, 1)]:
        assert lib.saspa_png_capacity(h, w, c) == P.capacity(h, w, c), (h, w, c)
        assert lib.saspa_png_workspace(3, h, w, c) > 0
    assert lib.saspa_png_capacity(4, 10923, 3) == _lib.SASPA_ERANGE          # rowbytes 32770
    assert lib.saspa_png_capacity(4, 4, 2) == _lib.SASPA_ERANGE and lib.saspa_png_capacity(4, 4, 4) == _lib.SASPA_ERANGE
    assert lib.saspa_png_capacity(0, 4, 3) == _lib.SASPA_EINVAL and lib.saspa_png_workspace(0, 4, 4, 3) == _lib.SASPA_EINVAL
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16                                   # never dereferenced: every call below is refused
    cap, work = lib.saspa_png_capacity(8, 8, 3), lib.saspa_png_workspace(2, 8, 8, 3)

    def call(px=p, n=2, h=8, w=8, c=3, streams=p, capacity=cap, sizes=p, workspace=p, wbytes=work):
        return lib.saspa_png_deflate(px, n, h, w, c, streams, capacity, sizes, workspace, wbytes, None)
    for null in ("px", "streams", "sizes", "workspace"):
        assert call(**{null: None}) == _lib.SASPA_EINVAL, null
    assert call(n=0) == _lib.SASPA_EINVAL and call(h=0) == _lib.SASPA_EINVAL and call(w=-1) == _lib.SASPA_EINVAL
    assert call(c=2) == _lib.SASPA_ERANGE
    assert call(capacity=cap - 1) == _lib.SASPA_ERANGE
    assert call(wbytes=work - 1) == _lib.SASPA_ERANGE
    assert call(w=10923, capacity=1 << 30, wbytes=1 << 30) == _lib.SASPA_ERANGE
    assert call(workspace=p + 4) == _lib.SASPA_EALIGN and call(sizes=p + 2) == _lib.SASPA_EALIGN
    from saspa_aug_amd import ops
    assert "capacity" in ops._HOST_ONLY and "workspace" in ops._HOST_ONLY


def test_submit_encoded_writes_a_decodable_file(tmp_path, monkeypatch):
    monkeypatch.setenv("SASPA_PNG_PROCS", "0")           # no encoder children for this test: the framing pool is what it is about
    png = R._PngWriters(2)
    want = {}
    for k, (shape, content) in enumerate([((17, 7, 3), "smooth_noise"), ((33, 21, 1), "dramp"), ((64, 128, 3), "uniform")]):
        img = P.make_image(shape, content)
        want[tmp_path / f"img_{k}.png"] = img
        png.submit_encoded(P.deflate(img)[0], *shape, tmp_path / f"img_{k}.png")
    assert png.submitted == 3 and png.max_depth >= 1
    png.close()
    for path, img in want.items():
        with Image.open(path) as im:
            im.verify()
        assert np.array_equal(np.asarray(Image.open(path)).reshape(img.shape), img)


_OFF = """
import sys
import numpy as np
import saspa_aug_amd
from saspa_aug_amd import run_aug as R


def generator(batch, noises, sources):
    return np.stack([np.full(s.shape, 7 * k, np.uint8) for k, s in enumerate(sources)]), sources.copy()


s = R.Settings(DATASET="synthetic", NUM_PER_IMAGE=1, RESOLUTION=64, USE_ARTISTIC_PROMPTS=False, SEMANTIC_FILTERING=0,
               MODEL_CONFIDENCE_BASED_FILTERING=0, BATCH_SIZE=2, PROMPTS_FILE=sys.argv[1] + "/prompts.txt",
               DATASET_KWARGS=dict(root_path=sys.argv[1] + "/ds/data", n_images=3, sizes=((64, 64),)), PNG_DEVICE=sys.argv[2] == "1")
res = R.main(s, batch_generator=generator)
assert (res["status"] == 1).all() and res["png_submitted"] == 9, res
print("pngenc imported:", "saspa_aug_amd.pngenc" in sys.modules)
"""


@pytest.mark.parametrize("flag", ["0", "1"])
def test_pngenc_is_not_imported_while_the_setting_is_off(tmp_path, flag):
    """run_aug.main with an injected generator that returns arrays, in a fresh interpreter: nothing of the device path is imported
    with PNG_DEVICE off, and an array generator keeps working (through the Pillow writers) with it on."""
    assert R.Settings().PNG_DEVICE is False
    (tmp_path / "prompts.txt").write_text("an airplane in the sky.\nan airplane on a runway.\n")
    out = subprocess.run([sys.executable, "-c", _OFF, str(tmp_path), flag], capture_output=True, text=True, timeout=300,
                         cwd=str(Path(__file__).resolve().parent.parent))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "pngenc imported: False" in out.stdout
    files = sorted(p.name for p in (tmp_path / "ds").rglob("*.png") if "aug_data" in str(p))
    assert len(files) == 9
