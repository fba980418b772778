"""saspa_png_deflate on the device against the integer model of tests/png_ref.py: byte-equal streams for every (shape, content)
pair, exact decode in Pillow, independence of the batch, run-to-run identity, and guard bytes behind every slot."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib, ops, pngenc

from tests import png_ref as P

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5


@functools.lru_cache(maxsize=None)
def _images(shape):
    return np.stack([P.make_image(shape, c) for c in P.CONTENTS])


@functools.lru_cache(maxsize=None)
def _model(shape, k):
    return P.deflate(_images(shape)[k])[0]


def _deflate_guarded(images):
    """saspa_png_deflate with slots of capacity + GUARD bytes inside one pattern-filled allocation (GUARD more in front of the first
    slot) -> (streams u8 [n, capacity + GUARD] on the host, sizes, the bytes in front)."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, h, w, c = images.shape
    cap, work = lib.saspa_png_capacity(h, w, c), lib.saspa_png_workspace(n, h, w, c)
    assert cap == P.capacity(h, w, c) and work > 0
    px = torch.from_numpy(images).to(dev)
    buf = torch.full((GUARD + n * (cap + GUARD),), PATTERN, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -1, dtype=torch.int32, device=dev)
    workspace = torch.empty((work,), dtype=torch.uint8, device=dev)
    rc = lib.saspa_png_deflate(C.c_void_p(px.data_ptr()), n, h, w, c, C.c_void_p(buf.data_ptr() + GUARD), cap + GUARD,
                               C.c_void_p(sizes.data_ptr()), C.c_void_p(workspace.data_ptr()), work,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    host = buf.cpu().numpy()
    return host[GUARD:].reshape(n, cap + GUARD), sizes.cpu().numpy(), host[:GUARD]


@functools.lru_cache(maxsize=None)
def _device(shape):
    return _deflate_guarded(_images(shape))


@pytest.mark.parametrize("content", P.CONTENTS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_equals_the_model_and_decodes(dev, shape, content):
    k = P.CONTENTS.index(content)
    streams, sizes, _ = _device(shape)
    want = _model(shape, k)
    got = streams[k, :sizes[k]].tobytes()
    assert sizes[k] == len(want), (sizes[k], len(want))
    assert got == want, f"first differing byte {next(i for i in range(len(want)) if got[i] != want[i])} of {len(want)}"
    img = Image.open(io.BytesIO(pngenc.frame(got, *shape)))
    assert np.array_equal(np.asarray(img).reshape(shape), _images(shape)[k])


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_guard_bytes_batch_independence_and_determinism(dev, shape):
    streams, sizes, front = _device(shape)
    cap = P.capacity(*shape)
    assert (sizes > 0).all() and (sizes <= cap).all()
    assert (front == PATTERN).all() and (streams[:, cap:] == PATTERN).all(), "bytes outside a slot were written"
    for k in range(len(sizes)):
        assert (streams[k, sizes[k]:] == PATTERN).all(), "bytes behind the stream were written"
    again, sizes2, _ = _deflate_guarded(_images(shape))
    assert np.array_equal(sizes, sizes2) and np.array_equal(streams, again)
    five = _deflate_guarded(_images(shape)[1:6])                   # the same images at other positions of a batch of 5
    for k in (2, 5):
        alone, size1, _ = _deflate_guarded(_images(shape)[k:k + 1])
        assert size1[0] == sizes[k] == five[1][k - 1]
        assert np.array_equal(alone[0], streams[k]) and np.array_equal(five[0][k - 1], streams[k])


def test_ops_png_deflate(dev):
    """The public op: shapes, dtypes, the grey [n, H, W] form, and the same bytes as the library call."""
    imgs = _images((17, 7, 3))
    streams, sizes = ops.png_deflate(torch.from_numpy(imgs).to(dev))
    assert streams.dtype == torch.uint8 and sizes.dtype == torch.int32 and tuple(streams.shape) == (len(imgs), P.capacity(17, 7, 3))
    s, z = streams.cpu().numpy(), sizes.cpu().numpy()
    for k in range(len(imgs)):
        assert s[k, :z[k]].tobytes() == _model((17, 7, 3), k)
    grey = _images((33, 21, 1))
    streams, sizes = ops.png_deflate(torch.from_numpy(grey[..., 0].copy()).to(dev))
    assert streams.cpu().numpy()[3, :int(sizes[3])].tobytes() == _model((33, 21, 1), 3)
    with pytest.raises(ValueError):
        ops.png_deflate(torch.zeros((1, 4, 4, 3), device=dev))                      # not u8
    with pytest.raises(RuntimeError, match="SASPA_ERANGE"):
        ops.png_deflate(torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device=dev))   # two channels
