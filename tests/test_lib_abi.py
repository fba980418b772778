"""The C-ABI library loads on a CPU-only box and exports every symbol include/saspa_hip.h
declares (no compute calls without a GPU); argument validation happens on the host before
any launch."""
import ctypes as C
import json
import os
import re

import pytest

import saspa_aug_amd  # noqa: F401
from saspa_aug_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "saspa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(saspa_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    lib = _lib.load()
    declared = _declared_symbols()
    assert declared and set(declared) == set(_lib.SYMBOLS), (declared, sorted(_lib.SYMBOLS))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.saspa_abi_version() == 20 and lib.saspa_build_arch() == b"gfx950"


def test_host_side_argument_validation_needs_no_gpu():
    lib = _lib.load()
    p = _lib.GemmParams()
    assert lib.saspa_gemm(C.byref(p), None) == -1                    # null pointers
    a = (C.c_char * 64)()
    base = C.addressof(a)
    p.a0 = p.w = p.out = (base + 15) // 16 * 16
    p.dtype, p.M, p.N, p.K, p.batch = 0, 16, 16, 12, 1
    p.kh = p.kw = p.stride = 1
    p.c0, p.lda0, p.ldw, p.ldo, p.hin, p.win, p.hout, p.wout = 12, 12, 12, 16, 16, 1, 16, 1
    assert lib.saspa_gemm(C.byref(p), None) == -2                    # channels not a multiple of 8
    p.c0 = p.K = p.lda0 = p.ldw = 16
    p.K = 32
    assert lib.saspa_gemm(C.byref(p), None) == -3                    # K != kh*kw*(c0+c1)
    # ABI 18 deferred reduce without K slices (no workspace): nothing would write the slabs the consumer sums -> refused
    p.K = p.c0 = p.lda0 = p.ldw = 16
    p.nb1 = p.nb2 = 1
    p.alpha = 1.0
    assert lib.saspa_gemm_suggest_ksplit(C.byref(p)) == 1
    p.defer_reduce, p.ksplit, p.workspace = 1, 1, None
    assert lib.saspa_gemm(C.byref(p), None) == -3
    p.defer_reduce = 0
    # ABI 19: the halo conv's eligibility and K-slice arithmetic are host-side
    h = _lib.GemmParams()
    h.dtype, h.kh, h.kw, h.stride, h.pad, h.batch, h.hin, h.win, h.hout, h.wout = 0, 3, 3, 1, 1, 2, 16, 16, 16, 16
    h.c0, h.c1, h.N, h.K, h.M, h.ldw, h.lda0, h.ldo, h.korder, h.nb1, h.nb2 = 320, 0, 640, 2880, 512, 2880, 320, 640, 2, 1, 1
    assert lib.saspa_conv3x3_halo_eligible(C.byref(h), None) == 1
    assert lib.saspa_conv3x3_halo_ksplit(C.byref(h), 3) == 3 and lib.saspa_conv3x3_halo_ksplit(C.byref(h), 4) == 3   # 5 chunk pairs: 2 + 2 + 1
    # the `defer_reduce` contract of the halo conv (advisor, round 5): a deferred reduce that would end on ONE slice, or on fewer
    # slices than the caller's saspa_splitk_groupnorm will sum, is refused before anything is launched
    big = (C.c_char * 64)()
    ptr = (C.addressof(big) + 15) // 16 * 16
    h.a0 = h.w = h.out = h.workspace = ptr
    h.defer_reduce, h.ksplit = 1, 1
    assert lib.saspa_conv3x3_halo(C.byref(h), None, None) == -3
    h.ksplit = 4                                                                                                   # lands on 3 slices
    assert lib.saspa_conv3x3_halo(C.byref(h), None, None) == -3
    h.a0 = h.w = h.out = h.workspace = None
    h.defer_reduce, h.ksplit = 0, 1
    h.korder = 1
    assert lib.saspa_conv3x3_halo_eligible(C.byref(h), None) == 0                                                  # im2col packing
    h.korder, h.hin, h.hout = 2, 8, 8
    h.M = 2 * 8 * 16
    assert lib.saspa_conv3x3_halo_eligible(C.byref(h), None) == 0                                                  # 128 pixels per image
    assert lib.saspa_conv3x3_halo(C.byref(h), None, None) == -1                                                    # null operands
    q = _lib.AttnParams()
    assert lib.saspa_flash_attn_bf16(C.byref(q), None) == -1
    assert lib.saspa_canny(None, None, None, 1, 8, 8, 1, 2, None) == -1
    assert lib.saspa_canny(base, base, (base + 15) // 16 * 16, 1, 100000, 32, 1, 2, None) == -3   # bitmaps exceed LDS and W < 64


def test_as_auto_is_the_dispatch_predicate_not_mere_eligibility():
    """ABI 20 (advisor, round 5): `saspa_gemm_as_eligible` says 2 for every size the balanced A-stationary launch can take, but AUTO
    keeps its measured rule -- a ragged block count (352 blocks of 256 rows: 512x704) without LayerNorm / residual and with 320
    columns stays on the tiled kernel.  Callers that plan around the choice (ops.conv drops the epilogue GroupNorm statistics)
    ask `saspa_gemm_as_auto`, the predicate dispatch() itself uses."""
    lib = _lib.load()
    keep = []

    def mk(m, n=320, res=False, act=0):
        p = _lib.GemmParams()
        a = (C.c_char * 64)()
        keep.append(a)
        base = (C.addressof(a) + 15) // 16 * 16
        p.a0 = p.w = p.out = base
        if res:
            p.residual, p.ldr = base, n
        p.dtype, p.M, p.N, p.K, p.batch = _lib.SASPA_BF16, m, n, 320, 1
        p.kh = p.kw = p.stride = 1
        p.c0 = p.lda0 = p.ldw = 320
        p.ldo, p.hin, p.hout, p.win, p.wout, p.nb1, p.nb2, p.alpha, p.act = n, m, m, 1, 1, 1, 1, 1.0, act
        return p
    for m, n, res, act, elig, auto in [(65536, 320, False, 0, 2, 1), (352 * 256, 320, False, 0, 2, 0), (352 * 256, 320, True, 0, 2, 1),
                                       (352 * 256, 640, False, 0, 2, 1), (352 * 256, 2560, False, 3, 2, 0), (100 * 256, 320, False, 0, 0, 0)]:
        p = mk(m, n, res, act)
        assert lib.saspa_gemm_as_eligible(C.byref(p)) == elig, (m, n, res)
        assert lib.saspa_gemm_as_auto(C.byref(p)) == auto, (m, n, res)
    p = mk(65536)
    p.variant = 1                                   # pinned to the tiled kernel: AUTO's choice does not apply
    assert lib.saspa_gemm_as_auto(C.byref(p)) == 0


def test_gemm_which_is_a_dry_dispatch():
    """ABI 20: saspa_gemm_which runs saspa_gemm's validation and dispatch without launching anything (no GPU needed) and reports
    family | (ksplit << 8): the level-0 3x3 conv goes to the 8-wave kernel, a K = 320 pointwise layer with a residual to the
    A-stationary one, (16384, 640, 640) to the 4-wave tiles, (4096, 1280, 1280) to the wave-specialised kernel; invalid
    problems return saspa_gemm's own error code."""
    lib = _lib.load()
    a = (C.c_char * 64)()
    base = (C.addressof(a) + 15) // 16 * 16

    def conv(b, h, w, cin, n, kh=3, res=False):
        p = _lib.GemmParams()
        p.a0 = p.w = p.out = base
        p.dtype, p.batch, p.hin, p.hout, p.win, p.wout, p.kh, p.kw, p.stride, p.pad = _lib.SASPA_BF16, b, h, h, w, w, kh, kh, 1, kh // 2
        p.c0 = p.lda0 = cin
        p.K = p.ldw = kh * kh * cin
        p.N = p.ldo = n
        p.M, p.nb1, p.nb2, p.alpha = b * h * w, 1, 1, 1.0
        if res:
            p.residual, p.ldr = base, n
        return p
    for args, fam in [((16, 64, 64, 320, 320), 2), ((16, 64, 64, 320, 320, 1, True), 4), ((16, 32, 32, 640, 640, 1), 1), ((16, 16, 16, 1280, 1280, 1), 3)]:
        w = lib.saspa_gemm_which(C.byref(conv(*args)))
        assert (w & 0xff, w >> 8) == (fam, 1), (args, w)
    bad = conv(16, 64, 64, 320, 320)
    bad.K = 99
    assert lib.saspa_gemm_which(C.byref(bad)) == -3
    assert lib.saspa_gemm_which(None) == -1


# ---- the GEMM dispatch table ------------------------------------------------------------------------------------------------
# A deterministic corpus of SaspaGemmParams (the latent levels of every shipped bucket, SD-1.5 / SDXL widths, the operand options
# the dispatch looks at) and, per row, (saspa_gemm_which, saspa_gemm_suggest_ksplit, saspa_gemm_as_auto, saspa_gemm_as_eligible),
# compared with tests/golden/gemm_dispatch.json.  Any change of a threshold or an eligibility rule shows up as a changed row; a
# deliberate one rewrites the golden:  PYTHONPATH=. python tests/test_lib_abi.py --write-dispatch-golden
DISPATCH_GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json")
_A0, _A1, _W, _OUT, _AUX = (1 << 20) * 1, (1 << 20) * 2, (1 << 20) * 3, (1 << 20) * 4, (1 << 20) * 5   # never dereferenced
_LEVELS = [(64, 64), (64, 88), (64, 96), (32, 32), (32, 44), (32, 48), (16, 16), (16, 22), (16, 24), (8, 8), (8, 11), (8, 12),
           (128, 128)]
_SILU, _GEGLU = 1, 3


def _gemm(b, h, w, c0, n, kh=1, c1=0, up=False, dtype=0, res=False, act=0, variant=0, sharing=0, korder=0, ks=0, defer=False,
          gn=False, nb=(1, 1), w_split=0, ln=False, out_t=False, pad=None):
    p = _lib.GemmParams()
    p.dtype, p.batch, p.hout, p.wout, p.hin, p.win = dtype, b, h, w, (h // 2 if up else h), (w // 2 if up else w)
    p.kh = p.kw = kh
    p.stride, p.pad, p.upsample = 1, kh // 2 if pad is None else pad, int(up)
    p.a0, p.c0, p.lda0 = _A0, c0, c0
    if c1:
        p.a1, p.c1, p.lda1 = _A1, c1, c1
    p.w, p.K = _W, kh * kh * (c0 + c1)
    p.ldw, p.N, p.M = p.K, n, b * h * w
    p.out, p.ldo = _OUT, (n // 2 if act == _GEGLU else n)
    p.alpha, p.act, p.variant, p.sharing, p.korder, p.w_split = 1.0, act, variant, sharing, korder, w_split
    p.nb1, p.nb2 = nb
    if res:
        p.residual, p.ldr = _AUX, n
    if gn:
        p.gn_stats, p.gn_unit = _AUX, 10
    if ln:
        p.ln_gamma = p.ln_beta = _AUX
        p.ln_eps = 1e-5
    if out_t:
        p.out_t, p.n_split, p.rows_per_batch = _AUX, n - 64, h * w
        p.ldt, p.st = h * w, 64 * h * w
    if ks:
        p.ksplit = _lib.load().saspa_gemm_suggest_ksplit(C.byref(p)) if ks == "suggest" else ks
        p.workspace = _AUX
    p.defer_reduce = int(defer)
    return p


# the options the dispatch reads, one dict of _gemm keywords each
_MODS = [{}, {"res": True}, {"act": _SILU}, {"act": _GEGLU}, {"act": _SILU, "res": True}, {"dtype": 1}, {"dtype": 2},
         {"dtype": 2, "w_split": 1}, {"dtype": 1, "w_split": 1}, {"w_split": 1}, {"sharing": 1}, {"sharing": 1, "res": True},
         {"variant": 1}, {"variant": 2}, {"variant": 3}, {"variant": 4}, {"gn": True}, {"gn": True, "ks": "suggest"},
         {"gn": True, "ks": "suggest", "defer": True}, {"ks": "suggest"}, {"ks": 2}, {"ks": 4}, {"ks": "suggest", "defer": True},
         {"ks": 1, "defer": True}, {"sharing": 1, "ks": "suggest"}, {"sharing": 1, "gn": True, "ks": "suggest"}, {"nb": (2, 3)},
         {"korder": 1}, {"korder": 1, "dtype": 2, "w_split": 1}, {"ln": True}, {"out_t": True}, {"ln": True, "act": _GEGLU},
         {"variant": 2, "gn": True}, {"variant": 3, "gn": True}, {"variant": 4, "ks": 2, "defer": True}, {"variant": 3, "act": _GEGLU},
         {"variant": 2, "act": _GEGLU}, {"variant": 3, "ks": 2, "defer": True}, {"dtype": 1, "variant": 2}, {"dtype": 1, "variant": 3},
         {"act": _GEGLU, "sharing": 1}, {"res": True, "ks": "suggest", "sharing": 1}, {"pad": 2}, {"pad": 2, "korder": 1}]


def _geometries(c):
    """(kh, c0, c1, upsample, N) of the layers of a level of width c, plus the odd shapes the dispatch special-cases."""
    return [(1, c, 0, False, c), (1, c, 0, False, 3 * c), (1, c, 0, False, 8 * c), (1, 4 * c, 0, False, c), (1, c, 0, False, 32),
            (1, c, 0, False, 64), (3, c, 0, False, c), (3, c, 0, False, 2 * c), (3, c, c, False, c), (3, c, c // 2, False, c),
            (3, c, 0, True, c), (3, 8, 0, False, c), (1, c // 2, c // 2, False, c), (3, c, 0, False, 32)]


def _boundary_rows():
    """Linears (one image of M x 1 pixels) on both sides of every tile-count, K and row-block threshold of the policy."""
    rows = []

    def add(m, k, n, **kw):
        rows.append(((1, m, 1, 1, k, 0, False, n, kw), _gemm(1, m, 1, k, n, **kw)))
    for t in (23, 24, 63, 64, 95, 96, 127, 128, 143, 144, 256, 257, 332, 333):      # 256 x 320 wide tiles
        for k in (576, 640, 896, 960, 4032, 4096):
            for sharing in (0, 1):
                for ks in (0, 2, "suggest"):
                    add(256 * t, k, 320, sharing=sharing, ks=ks)
    for t in (383, 384):                                                             # GEGLU on wide tiles
        for k in (576, 640):
            add(256 * t, k, 320, act=_GEGLU)
    for m in (16256, 16384):                                                         # GEGLU: 254 / 256 tiles of 128 x 160
        for k in (384, 448):
            add(m, k, 320, act=_GEGLU)
    for t in (159, 160, 255, 256, 435, 436, 511, 512):                               # 128 x 160 / 128 x 128 tiles
        for k in (320, 1280, 1984, 2048):
            for n in (160, 128):
                add(128 * t, k, n)
                add(128 * t, k, n, sharing=1)
    for blocks in (191, 192, 217, 218, 255, 256, 435, 436):                          # A-stationary: 256-row blocks
        for n, act, res in ((320, 0, False), (320, _GEGLU, False), (320, 0, True), (576, 0, False), (640, 0, False)):
            add(256 * blocks, 320, n, act=act, res=res)
    for n in (32, 40, 64, 72):                                                       # skinny N
        add(16384, 2048, n)
    return rows


def dispatch_corpus():
    """[(description, SaspaGemmParams)] in a fixed order: every (level, batch, width, geometry) plain and under one of the
    options (cycled), every option on a core of levels at batch 16, then the thresholds' boundaries."""
    rows = [("null", None)]
    i = 0
    for (h, w) in _LEVELS:
        for b in (2, 8, 16):
            for c in (320, 640, 1280):
                for g in _geometries(c):
                    for j in (0, 1 + (7 * i) % (len(_MODS) - 1)):
                        kh, c0, c1, up, n = g
                        rows.append(((b, h, w, kh, c0, c1, up, n, _MODS[j]), _gemm(b, h, w, c0, n, kh, c1, up, **_MODS[j])))
                    i += 1
    for (h, w), c in [((64, 88), 320), ((32, 44), 640), ((8, 12), 1280)]:
        for kh, c0, c1, up, n in _geometries(c):
            for j in range(1, len(_MODS)):
                rows.append(((16, h, w, kh, c0, c1, up, n, _MODS[j]), _gemm(16, h, w, c0, n, kh, c1, up, **_MODS[j])))
    return rows + _boundary_rows()


def dispatch_table(lib):
    table = []
    for _, p in dispatch_corpus():
        q = None if p is None else C.byref(p)
        table.append([lib.saspa_gemm_which(q), lib.saspa_gemm_suggest_ksplit(q), lib.saspa_gemm_as_auto(q), lib.saspa_gemm_as_eligible(q)])
    return table


def _decode(row):
    fam = {1: "TILED", 2: "WIDE", 3: "WS", 4: "AS"}
    w = row[0]
    which = _lib.ERRORS.get(w, str(w)).split()[0] if w < 0 else f"{fam.get(w & 0xff, w & 0xff)} x{w >> 8}"
    return f"which {which}, suggest_ksplit {row[1]}, as_auto {row[2]}, as_eligible {row[3]}"


def test_gemm_dispatch_table():
    """The dispatch of the GEMM family, decision for decision, against the recorded table (no GPU: the dry dispatch)."""
    lib = _lib.load()
    got = dispatch_table(lib)
    with open(DISPATCH_GOLDEN) as f:
        want = json.load(f)
    assert len(got) == len(want), (len(got), len(want))
    keys = [k for k, _ in dispatch_corpus()]
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    msg = "\n".join(f"row {i} (b, h, w, kh, c0, c1, up, N, options) = {keys[i]}:\n  got  {_decode(got[i])}\n  want {_decode(want[i])}"
                    for i in bad[:8])
    assert not bad, f"{len(bad)} of {len(want)} dispatch decisions changed:\n{msg}"


# ---- the flash-attention dispatch table -------------------------------------------------------------------------------------
# A deterministic corpus of SaspaAttnParams under the SASPA_ATTN_* knobs and, per row, saspa_flash_attn_which (loop | plan bits, or
# the error code), compared with tests/golden/attn_dispatch.json.  The golden was recorded from the dispatch as it stood BEFORE
# plan_attn existed (its launch sites made to return the code of the instantiation they launch): plan_attn reproduces it row for row.
# A deliberate change of a rule rewrites it:  PYTHONPATH=. python tests/test_lib_abi.py --write-attn-dispatch-golden
ATTN_GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_dispatch.json")
_PRE, _VROW = 1, 2                                             # SASPA_ATTN_QPRESCALED, SASPA_ATTN_V_ROWMAJOR
_ATTN_KNOBS = ("SASPA_ATTN_MODE", "SASPA_ATTN_V4", "SASPA_ATTN_RING")
_ALL_D = list(range(8, 161, 8))
_CORE_D = [40, 64, 80, 96, 128, 160]
_PRODUCTION = [(16, 8, 4096, 4096, 40), (16, 8, 1024, 1024, 80), (16, 8, 256, 256, 160),                 # (batch, heads, nq, nk, d)
               (16, 8, 4096, 77, 40), (16, 8, 1024, 77, 80), (16, 8, 256, 77, 160), (16, 8, 64, 77, 160)]
# every (loop, plan bits) the dispatch can reach in the shipped libraries: (loop, keys per tile, v2 double buffer, v3 ring slots,
# row-major V, ones row)
ATTN_REACHABLE = (
    [(1, 64, False, 4, rm, ones) for rm in (False, True) for ones in (False, True)]
    + [(1, 128, False, 4, False, ones) for ones in (False, True)]
    + [(2, keys, db, 4, False, ones) for keys in (64, 128) for db in (False, True) for ones in (False, True)]
    + [(3, 64, False, 4, rm, ones) for rm in (False, True) for ones in (False, True)]
    + [(3, 64, False, 6, False, True), (4, 64, False, 4, False, True)])


def _attn_code(loop, keys, db, ring, rm, ones):
    return loop | (16 if keys == 128 else 0) | (32 if db else 0) | (64 if ring == 6 else 0) | (128 if rm else 0) | (256 if ones else 0)


def _attn(b, heads, nq, nk, d, flags=0, causal=0, over=None):
    """A valid launch over operands that are never dereferenced; `over` then overwrites fields (the invalid rows)."""
    p = _lib.AttnParams()
    c = heads * d
    p.q, p.ldq, p.sqb = _A0, c, nq * c
    p.k, p.ldk, p.skb = _A1, c, nk * c
    p.vt, p.ldvt = _W, (c if flags & _VROW else (nk + 7) // 8 * 8)
    p.svb = (nk if flags & _VROW else c) * p.ldvt
    p.o, p.ldo, p.sob = _OUT, c, nq * c
    p.batch, p.heads, p.D, p.nq, p.nk, p.scale, p.causal, p.flags = b, heads, d, nq, nk, d ** -0.5, causal, flags
    for name, v in (over or {}).items():
        setattr(p, name, v)
    return p


def _attn_invalid_rows():
    rows = [("null", None), ("all zero", _lib.AttnParams())]

    def add(what, *shape, **over):
        rows.append(((what,) + shape, _attn(*shape, flags=over.get("flags", 0), over=over)))
    base = (2, 8, 1024, 1024, 40)
    for field in ("q", "k", "vt", "o"):
        add(f"{field} null", *base, **{field: None})
        add(f"{field} misaligned", *base, **{field: _A0 + 8})
    for field in ("batch", "heads", "nq", "nk", "D"):
        add(f"{field} = 0", *base, **{field: 0})
    for d in (4, 12, 44, 164, 168, 320):                                       # D % 8, D > 160
        add("head dim", 2, 8, 1024, 1024, 40, D=d)
    for field, v in (("ldq", 324), ("ldk", 324), ("ldvt", 1028), ("ldo", 322), ("sqb", 4), ("skb", 4), ("svb", 4), ("sob", 2)):
        add(f"{field} misaligned", *base, **{field: v})
    for flags in (4, 8, 7, -1):
        add("unknown flag bits", *base, flags=flags)
    for field in ("ldq", "ldk", "ldo"):
        add(f"{field} short", *base, **{field: 312})
    add("ldvt short (V^T)", *base, ldvt=1016)
    add("ldvt short (row-major V)", *base, flags=_VROW, ldvt=312)
    # the 2 GiB limits of the kernels' 32-bit byte offsets, each alone and from both sides:
    for ldvt in (6710880, 6710888):                                            # D x ldvt x 2 (V^T rows)
        add("2 GiB: V^T", 1, 1, 128, 1024, 160, ldvt=ldvt)
    for nk in (3355440, 3355448):                                              # nk x ldvt x 2 (row-major V)
        add("2 GiB: row-major V", 1, 2, 128, nk, 80, flags=_VROW, ldvt=320)
    for nk in (6710880, 6710888):                                              # nk x ldk x 2
        add("2 GiB: K", 1, 2, 128, nk, 80)
    return rows


def attn_dispatch_corpus():
    """[(knobs, [(description, SaspaAttnParams)])] in a fixed order: the invalid rows; every head dimension x key count x flags x
    causal on a small and a large grid; both sides of the workgroup thresholds and the production shapes; the knobs on a core of head
    dimensions; the pinned modes at every head dimension."""
    def shapes(ds, nks, grids):
        return [((b, h, nq, nk, d, fl, ca), _attn(b, h, nq, nk, d, fl, ca)) for d in ds for nk in nks for (b, h, nq) in grids
                for fl in (0, _PRE, _VROW, _PRE | _VROW) for ca in (0, 1)]
    small, large = (1, 2, 1024), (16, 8, 1024)                                 # 8 and 512 workgroups of 256 queries
    groups = [({}, _attn_invalid_rows()), ({}, shapes(_ALL_D, (77, 511, 512, 4096), (small, large)))]
    # ceil(nq / 256) x heads x batch and ceil(nq / 512) x heads x batch at 511 and 512, by nq and by heads x batch
    edge = [(1, 1, 256 * 511), (1, 1, 256 * 511 + 1), (1, 1, 512 * 511), (1, 1, 512 * 511 + 1), (7, 73, 256), (8, 64, 256), (8, 64, 257),
            (7, 73, 512), (8, 64, 512), (16, 8, 768), (16, 8, 769), (16, 8, 1536), (16, 8, 1537), (16, 8, 2048)]
    groups.append(({}, shapes(_CORE_D + [48], (4096,), edge)))
    groups.append(({}, [((b, h, nq, nk, d, fl, ca), _attn(b, h, nq, nk, d, fl, ca)) for (b, h, nq, nk, d) in _PRODUCTION
                        for fl in (0, _PRE, _VROW, _PRE | _VROW) for ca in (0, 1)]))
    pins = [{"SASPA_ATTN_MODE": m} for m in "01234"]
    pins += [{"SASPA_ATTN_V4": v, **mode} for v in "02" for mode in ({}, {"SASPA_ATTN_MODE": "4"})]
    pins += [{"SASPA_ATTN_RING": "4", **mode, **v4} for mode in ({}, {"SASPA_ATTN_MODE": "4"}) for v4 in ({}, {"SASPA_ATTN_V4": "0"})]
    for knobs in pins:
        groups.append((knobs, shapes(_CORE_D, (77, 512, 4096), (small, large, (1, 1, 512 * 511 + 1)))))
    for mode in "14":
        groups.append(({"SASPA_ATTN_MODE": mode}, shapes(_ALL_D, (4096,), (large,))))
    return groups


def attn_dispatch_table(lib, setenv, delenv):
    table = []
    for knobs, rows in attn_dispatch_corpus():
        for name in _ATTN_KNOBS:
            if name in knobs:
                setenv(name, knobs[name])
            else:
                delenv(name)
        table += [lib.saspa_flash_attn_which(None if p is None else C.byref(p)) for _, p in rows]
    for name in _ATTN_KNOBS:
        delenv(name)
    return table


def _decode_attn(w):
    if w < 0:
        return _lib.ERRORS.get(w, str(w)).split()[0]
    bits = [name for bit, name in ((16, "128-key tiles"), (32, "double buffer"), (64, "six-slot ring"), (128, "row-major V"), (256, "ones row"))
            if w & bit]
    return f"v{w & 15} " + ", ".join(bits + ([f"ablation {w >> 12}"] if w >> 12 else []))


def test_attn_dispatch_table(monkeypatch):
    """The dispatch of saspa_flash_attn_bf16, decision for decision, against the table recorded from the dispatch that preceded
    plan_attn (no GPU: the dry plan), in the default library and, where it is built, the fp16 one.  On the invalid rows the launch
    entry itself returns the same code (it returns before it touches a stream)."""
    with open(ATTN_GOLDEN) as f:
        want = json.load(f)
    assert os.path.getsize(ATTN_GOLDEN) < 73848
    groups = attn_dispatch_corpus()
    keys = [(knobs, k) for knobs, rows in groups for k, _ in rows]
    params = [p for _, rows in groups for _, p in rows]
    assert len(want) == len(keys), (len(want), len(keys))
    # the golden itself reaches every (loop, plan bits) the dispatch can reach, and nothing else
    assert {w for w in want if w >= 0} == {_attn_code(*t) for t in ATTN_REACHABLE}, sorted({_decode_attn(w) for w in want if w >= 0})
    assert {w for w in want if w < 0} == {_lib.SASPA_EINVAL, _lib.SASPA_EALIGN, _lib.SASPA_ERANGE}
    libs = [("default", _lib.load())] + ([("fp16", _lib.load_f16())] if os.path.exists(_lib.F16_LIB_PATH) else [])
    for which, lib in libs:
        got = attn_dispatch_table(lib, monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False))
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        msg = "\n".join(f"row {i} knobs {keys[i][0]} (b, heads, nq, nk, d, flags, causal) = {keys[i][1]}:\n  got  {_decode_attn(got[i])}\n"
                        f"  want {_decode_attn(want[i])}" for i in bad[:8])
        assert not bad, f"{which} library: {len(bad)} of {len(want)} attention dispatch decisions changed:\n{msg}"
        for i, p in enumerate(params):
            if want[i] < 0:
                assert lib.saspa_flash_attn_bf16(None if p is None else C.byref(p), None) == want[i], keys[i]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--write-dispatch-golden"]:
        rows = dispatch_table(_lib.load())
        with open(DISPATCH_GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
        print(f"{DISPATCH_GOLDEN}: {len(rows)} rows")
    if sys.argv[1:] == ["--write-attn-dispatch-golden"]:
        rows = attn_dispatch_table(_lib.load(), os.environ.__setitem__, lambda name: os.environ.pop(name, None))
        with open(ATTN_GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(",".join(str(w) for w in rows[i:i + 32]) for i in range(0, len(rows), 32)) + "\n]\n")
        print(f"{ATTN_GOLDEN}: {len(rows)} rows")


def test_ff_block_host_side_validation():
    """saspa_ff_block (ABI 20): null operands, geometry (rows % 128, inner width % 32, pitches) and alignment are refused on the host."""
    lib = _lib.load()
    a = (C.c_char * 64)()
    base = (C.addressof(a) + 15) // 16 * 16
    p = _lib.FfBlockParams()
    assert lib.saspa_ff_block(C.byref(p), None) == -1
    p.x = p.residual = p.out = p.w1 = p.b1 = p.w2f = p.b2 = base
    p.ldx = p.ldr = p.ldo = p.ldw1 = 320
    p.M, p.F = 100, 1280
    assert lib.saspa_ff_block_eligible(C.byref(p)) == 0 and lib.saspa_ff_block(C.byref(p), None) == -3      # rows % 128
    p.M, p.F = 256, 1000
    assert lib.saspa_ff_block_eligible(C.byref(p)) == 0                                                      # inner width % 32
    p.F, p.ldo = 1280, 300
    assert lib.saspa_ff_block_eligible(C.byref(p)) == 0                                                      # pitch < 320
    p.ldo = 320
    assert lib.saspa_ff_block_eligible(C.byref(p)) == 1
    p.ln_gamma = base
    assert lib.saspa_ff_block(C.byref(p), None) == -1                                                        # gamma without beta
    p.ln_beta = base
    p.w2f = base + 8
    assert lib.saspa_ff_block(C.byref(p), None) == -2                                                        # alignment


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()
