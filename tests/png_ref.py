"""The device PNG encoder's specification as code ("PNG encode on the device"): a numpy / integer model of the
row filters, the segment cut, the code-length construction, the canonical codes, the dynamic-block header, the bit packing, the
segment join and the stored fallback of saspa_png_deflate, and of pngenc.frame.  `deflate` returns the zlib stream the kernels
must produce byte for byte, plus what the stream exercised (so that tests can assert their coverage)."""
import struct
import zlib

import numpy as np

HEADER_BITS = 1222            # 3 + 5 + 5 + 4 + 19 * 3 + 286 * 4 + 4
HEADER_BYTES = 153
LEN_BIT0 = 74                 # bit offset of the first literal/length code length
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def geometry(H, W, C):
    """-> (rowbytes, rows per segment, number of segments)."""
    if C not in (1, 3) or H < 1 or W < 1:
        raise ValueError((H, W, C))
    rowbytes = 1 + W * C
    if rowbytes > 32767:
        raise ValueError(f"rowbytes {rowbytes} > 32767")
    R = max(1, min(16, 32767 // rowbytes))
    return rowbytes, R, -(-H // R)


def capacity(H, W, C):
    """Bytes of an image's slot: zlib header, every segment as a stored block (5 + segbytes), Adler-32."""
    rowbytes, _, nseg = geometry(H, W, C)
    return 2 + H * rowbytes + 5 * nseg + 4


def filter_rows(img, r0, r1):
    """PNG-filter rows [r0, r1) of a u8 [H, W, C] image -> (u8 [rows, 1 + W*C] type byte + residuals, chosen types).  The row
    above r0 comes from the raw image (zeros above row 0); the filter with the smallest sum |int8(residual)| wins, ties to
    the lowest index."""
    H, W, C = img.shape
    flat = img.reshape(H, W * C).astype(np.int32)
    cur = flat[r0:r1]
    up = np.zeros_like(cur)
    lo = max(r0, 1)
    up[lo - r0:] = flat[lo - 1:r1 - 1]
    a = np.zeros_like(cur)
    a[:, C:] = cur[:, :-C]
    c = np.zeros_like(cur)
    c[:, C:] = up[:, :-C]
    p = a + up - c
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    res = np.stack([cur, cur - a, cur - up, cur - ((a + up) >> 1), cur - pred]) & 255          # [5, rows, W*C]
    cost = np.where(res < 128, res, 256 - res).sum(-1)                                          # [5, rows]
    ftype = cost.argmin(0)
    rows = r1 - r0
    out = np.empty((rows, 1 + W * C), np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = res[ftype, np.arange(rows)]
    return out, ftype


def code_lengths(hist, T):
    """hist: 257 counts (256 literals + end-of-block, count 1), T = their sum.  -> (286 code lengths, number of symbols above
    end-of-block with a code: always 0)."""
    assert len(hist) == 257 and int(np.sum(hist)) == T and T <= 32768
    lens = [0] * 286
    used = [s for s in range(257) if hist[s] > 0]
    for s in used:
        l = 1
        while (int(hist[s]) << l) < T:
            l += 1
        lens[s] = l
    order = sorted(used, key=lambda s: (-int(hist[s]), s))
    slack = 32768 - sum(1 << (15 - lens[s]) for s in used)
    assert slack >= 0
    changed = True
    while changed and slack > 0:
        changed = False
        for s in order:
            w = 1 << (15 - lens[s])
            if lens[s] > 1 and w <= slack:
                lens[s] -= 1
                slack -= w
                changed = True
                if slack == 0:
                    break
    # The walk ends on slack 0: every weight in use is a multiple of the smallest one, so is the slack, and while it is positive the
    # longest code (l > 1, or two codes of length 1 would already fill the code) can take it.  So the code is complete, which zlib
    # demands, and no never-used length symbol (257..285) is needed as padding.
    assert slack == 0
    pads = sum(1 for l in lens[257:] if l)
    assert sum(1 << (15 - l) for l in lens if l) == 32768
    return lens, pads


def canonical_codes(lens):
    """RFC 1951 section 3.2.2, each code bit-reversed for the LSB-first stream."""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], f"0{l}b")[::-1], 2)
            nxt[l] += 1
    return out


def _rev4(v):
    return int(format(v, "04b")[::-1], 2)


def _pack(values, nbits):
    """LSB-first packing of `values[i]` in `nbits[i]` bits -> bool bit array."""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    start = np.concatenate([[0], np.cumsum(nbits)])
    bits = np.zeros(int(start[-1]), np.uint8)
    for k in range(int(nbits.max()) if len(nbits) else 0):
        m = nbits > k
        bits[start[:-1][m] + k] = (values[m] >> k) & 1
    return bits


def encode_segment(data, final):
    """One segment's filtered bytes -> (its bytes in the stream, info).  Huffman form unless that would take >= len + 5 bytes."""
    data = np.asarray(data, np.uint8).reshape(-1)
    n = len(data)
    hist = np.bincount(data, minlength=257)
    hist[256] = 1
    lens, pads = code_lengths(hist, n + 1)
    body = int(sum(int(hist[s]) * lens[s] for s in range(257)))
    hb = HEADER_BITS + body
    hbytes = (hb + 7) // 8 if final else (hb + 3 + 7) // 8 + 4
    info = dict(stored=hbytes >= n + 5, pads=pads, maxlen=max(lens), single=int((hist[:256] > 0).sum()) == 1, huffman_bytes=hbytes)
    if info["stored"]:
        return bytes([int(final)]) + struct.pack("<HH", n, n ^ 0xFFFF) + data.tobytes(), info
    codes = canonical_codes(lens)
    vals = [int(final) | 4, 29, 0, 15] + [0 if s > 15 else 4 for s in CL_ORDER] + [_rev4(l) for l in lens] + [_rev4(1)]
    nb = [3, 5, 5, 4] + [3] * 19 + [4] * 287
    assert sum(nb) == HEADER_BITS
    syms = np.concatenate([data.astype(np.int64), [256]])
    bits = np.concatenate([_pack(vals, nb), _pack(np.asarray(codes)[syms], np.asarray(lens)[syms])])
    assert len(bits) == hb
    if not final:
        bits = np.concatenate([bits, np.zeros(3, np.uint8)])               # empty stored block: BFINAL 0, BTYPE 00
    out = np.packbits(bits, bitorder="little").tobytes()
    if not final:
        out += b"\x00\x00\xff\xff"
    assert len(out) == hbytes
    return out, info


def deflate(img):
    """u8 [H, W, C] (C in {1, 3}) -> (zlib stream bytes, info).  info: filters (set of chosen types), maxlen (longest code of a
    Huffman segment), pads (most pad symbols in a Huffman segment), stored / huffman (segment counts), single (a Huffman segment
    with one literal), segments = [(filtered bytes, stream bytes, stored)]."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    rowbytes, R, nseg = geometry(H, W, C)
    out, adler = [b"\x78\x01"], 1
    info = dict(filters=set(), maxlen=0, pads=0, stored=0, huffman=0, single=False, segments=[])
    for s in range(nseg):
        r0, r1 = s * R, min(H, (s + 1) * R)
        filt, ftype = filter_rows(img, r0, r1)
        raw = filt.tobytes()
        seg, si = encode_segment(filt, s == nseg - 1)
        assert len(seg) <= len(raw) + 5
        adler = zlib.adler32(raw, adler)
        out.append(seg)
        info["filters"] |= set(int(f) for f in ftype)
        info["segments"].append((raw, seg, si["stored"]))
        if si["stored"]:
            info["stored"] += 1
        else:
            info["huffman"] += 1
            info["maxlen"] = max(info["maxlen"], si["maxlen"])
            info["pads"] = max(info["pads"], si["pads"])
            info["single"] |= si["single"]
    out.append(struct.pack(">I", adler))
    z = b"".join(out)
    assert len(z) <= capacity(H, W, C)
    return z, info


def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))


def frame(z, H, W, C):
    """zlib stream of the filtered rows -> PNG file: signature, IHDR (8 bit, colour type 2 / 0), one IDAT, IEND."""
    ihdr = struct.pack(">IIBBBBB", W, H, 8, {3: 2, 1: 0}[C], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", bytes(z)) + _chunk(b"IEND", b"")


# ---- the inputs of the tests: every (shape, content) pair of the GPU suite --------------------------------------------------
SHAPES = [(1, 1, 3), (1, 1, 1), (2, 3, 3), (16, 5, 3), (17, 7, 3), (33, 21, 1), (64, 128, 3), (12, 1100, 3)]
CONTENTS = ["constant", "zeros", "uniform", "smooth_noise", "hramp", "vramp", "dramp", "geometric"]


def make_image(shape, content, seed=0):
    """Deterministic u8 [H, W, C] test image.  "geometric": the FIRST segment's pixels follow a geometric histogram (value k about
    half as often as k - 1, so whichever filters win leave a long-tailed histogram: code lengths from 1 up to 15 where the segment is
    long enough); the rest of the image is zeros."""
    H, W, C = shape
    rng = np.random.RandomState(1000 * H + 10 * W + C + 7919 * seed)
    y, x = np.mgrid[0:H, 0:W]
    if content == "constant":
        img = np.full((H, W, C), 137)
    elif content == "zeros":
        img = np.zeros((H, W, C))
    elif content == "uniform":
        img = rng.randint(0, 256, (H, W, C))
    elif content == "smooth_noise":
        base = 128 + 90 * np.sin(x / 9.0 + 0.3) * np.cos(y / 7.0)
        img = base[..., None] + np.arange(C) * 11 + rng.normal(0, 4, (H, W, C))
    elif content == "hramp":
        img = (x * 3)[..., None] + np.arange(C)
    elif content == "vramp":
        img = (y * 5)[..., None] + np.arange(C) * 2
    elif content == "dramp":
        img = ((x + y) * 2)[..., None] + np.arange(C) * 3
    elif content == "geometric":
        _, R, _ = geometry(H, W, C)
        rows = min(R, H)
        k = np.minimum(rng.geometric(0.5, (rows, W, C)) - 1, 40)
        img = np.zeros((H, W, C))
        img[:rows] = k
    else:
        raise ValueError(content)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
