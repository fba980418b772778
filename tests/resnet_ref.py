"""TEST INFRASTRUCTURE ONLY -- float64 references, magnitudes, fp32 emulations and mutants of the ResnetBlock2D path: the conv
epilogue forms, the GroupNorm statistics the epilogues leave, conv -> GroupNorm -> SiLU (saspa_splitk_groupnorm) and GroupNorm ->
SiLU -> conv (saspa_conv3x3_halo and the two launches it replaces).  CPU only; the CPU proof (tests/test_errbudget.py) and the GPU
tests (tests/test_resnet_errbudget_gpu.py) both import it.  Tensors are channels-last [B, H, W, C] float64 holding values of the
storage type; weights [N, C, kh, kw].  Rounding goes through tests/test_errbudget.py's q / rne / trunc, so the conv forms follow
the fp16 re-run of the gemm family; the three new families are bf16 only (gn_stats and the halo kernel exist in the default library).

Rounding points, as the kernels have them (csrc/):
- conv epilogue, 8-wave kernel (saspa_gemm_pp.hip): :771 add = bias + rowvec in fp32; :797-800 v = (acc + add) * alpha in fp32,
  packed to the storage type into the staging tile (Elem<T>::store4); `finish` :866-891: WITHOUT residual / activation the staged
  value IS the output (:890); WITH a residual it is unpacked (:869), the residual added in fp32 (:881) and packed AGAIN (:887).
  So out = rne(rne(alpha (acc + bias + rowvec)) + residual): two roundings, alpha before the residual.  The row vector of a row is
  its OWN image's (:807-808 where a 128-row half spans images).
- the 4-wave kernel (saspa_gemm.hip): :144-147 / :161-170 the same sum, alpha, pack; :180-204 the same unpack / + residual / pack.
- the halo kernel (saspa_conv_halo.hip): :639 alpha, `finish` :645-662 identical to the 8-wave kernel's.
- K slices: splitk_reduce_kernel (saspa_gemm.hip:906-935) sums the fp32 slabs in slab order (:910-914), + bias (:918) + rowvec
  (:922), * alpha (:925), + residual in fp32 (:930) and packs ONCE (:934): with a residual the reduce path has ONE rounding where
  the tile epilogue has two.  splitk_reduce_stats_kernel (:953-997) is the same arithmetic.
- epilogue statistics (include/saspa_hip.h:136-144, ABI 12): sums of the STORED values; common.h gn_tile_stats :262-288 (and its
  restatement saspa_gemm_pp.hip:935-968): thread (unit, row group) walks its rows rg, rg + rgs, ... and the unit's channels in
  pairs, one fdot2 per pair and sum (:274-275), fp32; then the row groups in order (:285).  rgs = threads / units of the tile: 8
  (8-wave, 320 columns, unit 10), 16 (4-wave, 160 columns), 32 (the reduce path's 80-column slabs, saspa_gemm.hip:1000).
- GroupNorm from those statistics: gn_apply_kernel (saspa_norm.hip:205-211) sc = gamma rstd, sh = beta - mean sc in fp32, :231-232
  y = x sc + sh, SiLU by v_exp + v_rcp (common.h:171), packed (:237).
- saspa_splitk_groupnorm (include/saspa_hip.h:289-296, ABI 18; saspa_norm.hip splitk_gn_kernel): :580-589 slabs summed in fp32 in
  slab order, :597-604 + bias + rowvec of image b, :607 * alpha, :608-610 ROUNDED to the storage type (the value the unfused path
  stores), :612-613 per-lane fp32 sum / sum of squares over the lane's items tid + 256 i, :617-627 combined in fp64, :629 mean and
  rstd rounded to fp32, :642-644 the arithmetic of gn_apply_kernel, :647 packed.
- saspa_conv3x3_halo (include/saspa_hip.h:300-311, ABI 19): :482-546 (mean, rstd) per group from the epilogue statistics or the
  statistics pass, fp64 combine, rounded to fp32 (:544-545); :247-248 sc / sh per channel as gn_apply_kernel; :290 padding stays
  zero (the conv pads the NORMALISED tensor); :296 silu_fast(v sc + sh) in fp32; :301 packed to bf16 before the product.
"""
import math

import torch
import torch.nn.functional as F

from tests.errbudget import _floor, chain_gemm_scale, chain_norm_scale, norm_scale

UNIT_GNSTAT = 2.0 ** -24               # the gnstat family: fp32 sums against sum |v| / sum v^2
GROUPS, EPS = 32, 1e-5


def _T():
    from tests import test_errbudget as T
    return T


def q(x):
    return _T().q(x)


def rne(x):
    return _T().rne(x)


def trunc(x):
    return _T().trunc(x)


def f32(x):
    return x.float()


def f32v(x):
    return x.float().double()


# ------------------------------------------------------------------ convolution pieces
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def conv_nhwc(x, w, stride=1, pad=None):
    """conv2d of a channels-last tensor in ITS dtype (float64: the reference; float32: an emulation in torch's own order)."""
    pad = w.shape[-1] // 2 if pad is None else pad
    return F.conv2d(_nchw(x), w.to(x.dtype), None, stride=stride, padding=pad).permute(0, 2, 3, 1)


def im2col(x, kh, stride=1, pad=None):
    """[B, H, W, C] -> [M, taps, C]: the A operand of the implicit GEMM, taps in (ky, kx) order."""
    pad = kh // 2 if pad is None else pad
    b, _, _, c = x.shape
    u = F.unfold(_nchw(x), kh, padding=pad, stride=stride)
    return u.reshape(b, c, kh * kh, -1).permute(0, 3, 2, 1).reshape(-1, kh * kh, c)


def pack_w(w):
    """[N, C, kh, kw] -> [N, taps, C]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1])


def _korder(t, order):
    """[R, taps, C] -> [R, K] in tap-major ("tap"), 64-channel chunk-major ("chunk") or 32-channel chunk-major ("chunk32") order."""
    r, taps, c = t.shape
    if order == "tap":
        return t.reshape(r, -1)
    bk = 64 if order == "chunk" else 32
    return t.reshape(r, taps, c // bk, bk).permute(0, 2, 1, 3).reshape(r, -1)


def acc32(a, wp, order="tap", rev=False, ks=1, bk=64):
    """fp32 accumulation of [M, taps, C] x [N, taps, C] over K-tiles of bk in the given K order (rev: last tile first), the tiles
    cut into ks contiguous slices, each an fp32 slab, the slabs added in slab order (the split-K reduce)."""
    a2, w2 = f32(_korder(a, order)), f32(_korder(wp, order))
    nt = -(-a2.shape[1] // bk)
    tiles = list(range(nt))[::-1] if rev else list(range(nt))
    bounds = [round(i * nt / ks) for i in range(ks + 1)]
    out = None
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        slab = torch.zeros(a2.shape[0], w2.shape[0])
        for t in tiles[s0:s1]:
            slab = slab + a2[:, t * bk:(t + 1) * bk] @ w2[:, t * bk:(t + 1) * bk].t()
        out = slab if out is None else out + slab
    return out


# ------------------------------------------------------------------ family gemm: the conv epilogue forms
# (name, b, h, w, c0, c1, n, kh, stride, flags): the GPU file launches exactly these.  "rv": per-image time-embedding row, "res":
# residual, alpha 0.5 with both; "ks": K slices 2 and 3
CONV_FORMS = [("plain", 3, 9, 7, 64, 0, 24, 3, 1, ""),
              ("multi-image tile", 5, 6, 7, 64, 0, 320, 3, 1, "rv res"),
              ("multi-image tile", 9, 8, 8, 64, 0, 320, 3, 1, "rv res"),
              ("stride 2", 2, 16, 16, 64, 0, 64, 3, 2, ""),
              ("concat", 2, 16, 16, 128, 64, 320, 3, 1, ""),
              ("1x1 concat", 2, 16, 16, 128, 64, 320, 1, 1, ""),
              ("K slices", 1, 16, 16, 512, 0, 320, 3, 1, "ks")]
CONV_FORMS_GPU_ONLY = [("wide tile", 2, 24, 24, 128, 0, 256, 3, 1, "")]


def conv_operands(rand, form, seed):
    _, b, h, w_, c0, c1, n, kh, stride, flags = form
    c = c0 + c1
    ho, wo = (h + 2 * (kh // 2) - kh) // stride + 1, (w_ + 2 * (kh // 2) - kh) // stride + 1
    op = dict(x=q(rand(b, h, w_, c0, seed=seed)), x2=q(rand(b, h, w_, c1, seed=seed + 1) * 0.7) if c1 else None,
              w=q(rand(n, c, kh, kh, seed=seed + 2, scale=1 / math.sqrt(c * kh * kh))), bias=f32v(rand(n, seed=seed + 3)),
              rowvec=f32v(rand(b, n, seed=seed + 4)) if "rv" in flags else None,
              res=q(rand(b, ho, wo, n, seed=seed + 5)) if "res" in flags else None, alpha=0.5 if "res" in flags else 1.0,
              stride=stride, kh=kh, hw=ho * wo)
    return op


def _xc(op):
    return op["x"] if op["x2"] is None else torch.cat([op["x"], op["x2"]], -1)


def _add64(op, n):
    add = torch.zeros(n, dtype=torch.float64) if op["bias"] is None else op["bias"]
    return add if op["rowvec"] is None else add + op["rowvec"][:, None, None, :]


def conv_ref(op, x=None, *, two_roundings=True):
    """float64 conv with the epilogue's rounding points -> (ref [B, Ho, Wo, N], magnitude).  two_roundings: the tile epilogue (the
    staged value is rounded before the residual is added); False: the split-K reduce path (one rounding, the output's)."""
    x = _xc(op) if x is None else x
    w, alpha = op["w"], op["alpha"]
    n = w.shape[0]
    pre = alpha * (conv_nhwc(x, w, op["stride"]) + _add64(op, n))
    s = conv_nhwc(x.abs(), w.abs(), op["stride"])
    if op["bias"] is not None:
        s = s + op["bias"].abs()
    if op["rowvec"] is not None:
        s = s + op["rowvec"].abs()[:, None, None, :]
    s = abs(alpha) * s
    if op["res"] is None:
        return pre, _floor(s)
    return (rne(pre) if two_roundings else pre) + op["res"], _floor(s + op["res"].abs())


def conv_epilogue(acc, op, *, rnd=rne, ks=1, reduce_path=False, rv_neighbour=False, rv_cols=None, res_before_alpha=False,
                  bias_per_slice=False):
    """The epilogue in fp32 on accumulators [M, N] -> [B, Ho, Wo, N].  The options are the mutants."""
    b = op["x"].shape[0]
    n = acc.shape[1]
    acc = acc.reshape(b, -1, n)
    add = torch.zeros(n) if op["bias"] is None else f32(op["bias"]) * (ks if bias_per_slice else 1)
    add = add.expand(b, 1, n)
    if op["rowvec"] is not None:
        rv = f32(op["rowvec"]).clone()
        if rv_cols is not None:
            rv[:, rv_cols[0]:rv_cols[1]] = 0.0
        rows = rv[:, None, :].expand(b, op["hw"], n)
        if rv_neighbour:
            # a row whose image is not the image of its 128-row block's first row takes the row vector of the image before its own
            m = torch.arange(b * op["hw"])
            img = m // op["hw"]
            img = torch.where((m // 128 * 128) // op["hw"] != img, img - 1, img)
            rows = rv[img].reshape(b, op["hw"], n)
        add = add + rows
    alpha = torch.tensor(op["alpha"], dtype=torch.float32)
    res = None if op["res"] is None else f32(op["res"]).reshape(b, -1, n)
    if res is not None and res_before_alpha:
        out = rnd((acc + add + res) * alpha)
    elif res is not None and reduce_path:
        out = rnd((acc + add) * alpha + res)
    else:
        out = rnd((acc + add) * alpha)
        if res is not None:
            out = rnd(f32(out) + res)
    return out.reshape(_out_shape(op, n))


def _out_shape(op, n):
    b, h, w_, _ = op["x"].shape
    kh, st = op["kh"], op["stride"]
    return (b, (h + 2 * (kh // 2) - kh) // st + 1, (w_ + 2 * (kh // 2) - kh) // st + 1, n)


def conv_cases(rand, residual_forms=True):
    """(name, got, ref, s, legit) for the conv epilogue forms: family 'gemm'.  residual_forms = False leaves the forms with a
    residual out (the fp16 re-run: see test_errbudget._gemm_family_cases)."""
    out = []
    for i, form in enumerate(CONV_FORMS):
        name, b, h, w_, c0, c1, n, kh, stride, flags = form
        if "res" in flags and not residual_forms:
            continue
        op = conv_operands(rand, form, 400 + 10 * i)
        xc = _xc(op)
        ref, s = conv_ref(op)
        tag = f"conv {name} {b}x{h}x{w_}x{c0}{'+' + str(c1) if c1 else ''}->{n} {kh}x{kh}"
        a, wp = im2col(xc, kh, stride), pack_w(op["w"])
        acc = acc32(a, wp)
        out.append((f"legit fp32 K-tile order, tap-major {tag}", conv_epilogue(acc, op), ref, s, True))
        out.append((f"legit fp32 reversed K-tile order {tag}", conv_epilogue(acc32(a, wp, rev=True), op), ref, s, True))
        if kh == 3:
            out.append((f"legit fp32 chunk-major {tag}", conv_epilogue(acc32(a, wp, "chunk"), op), ref, s, True))
        if "ks" in flags:
            for ks in (2, 3):
                out.append((f"legit {ks} K slices, fp32 slabs in slab order {tag}", conv_epilogue(acc32(a, wp, "chunk", ks=ks), op),
                            ref, s, True))
                out.append((f"mutant bias added once per K slice ({ks}) {tag}", conv_epilogue(acc, op, ks=ks, bias_per_slice=True),
                            ref, s, False))
        if b * op["hw"] * n >= 4096:
            out.append((f"mutant truncating store conv {tag}", conv_epilogue(acc, op, rnd=trunc), ref, s, False))
        if "rv" in flags:
            out.append((f"mutant time-embedding row of the neighbouring image in a tile that spans two images {tag}",
                        conv_epilogue(acc, op, rv_neighbour=True), ref, s, False))
            out.append((f"mutant rowvec missing on columns 256..319 {tag}", conv_epilogue(acc, op, rv_cols=(256, 320)), ref, s,
                        False))
        if "res" in flags:
            out.append((f"mutant residual added before alpha {tag}", conv_epilogue(acc, op, res_before_alpha=True), ref, s, False))
        if kh == 3 and stride == 1 and b > 1:
            # the pad row below image b holds image b + 1's first row (what follows it in memory)
            xp = F.pad(xc, (0, 0, 1, 1, 1, 1))
            xp[:-1, -1, 1:-1] = xc[1:, 0]
            leak = conv_nhwc(f32(xp), op["w"], pad=0).reshape(-1, n)
            out.append((f"mutant bottom-row taps read the next image's top row instead of zero padding {tag}",
                        conv_epilogue(leak, op), ref, s, False))
        if c1:
            wd = op["w"].clone()
            wd[:, -32:, kh // 2, kh - 1] = 0.0
            out.append((f"mutant second concat source's last 32 channels dropped from one tap {tag}",
                        conv_epilogue(conv_nhwc(f32(xc), wd, stride).reshape(-1, n), op), ref, s, False))
    return out


# ------------------------------------------------------------------ family gnstat: the statistics an epilogue leaves
def gnstat_ref(v, unit):
    """v [B, H, W, N] stored values -> (ref [M / 128, N / unit, 2] float64 (sum, sum of squares), magnitude (sum |v|, sum v^2))."""
    n = v.shape[-1]
    t = v.double().reshape(-1, 128, n // unit, unit)
    ref = torch.stack([t.sum((1, 3)), (t * t).sum((1, 3))], -1)
    s = torch.stack([t.abs().sum((1, 3)), (t * t).sum((1, 3))], -1)
    return ref, torch.stack([_floor(s[..., 0]), _floor(s[..., 1])], -1)


def gnstat_emul(v, unit, rgs, *, pairs=True, rows=128, shift_last_unit_of=None):
    """gn_tile_stats in fp32: rgs row groups, each walking its rows rg, rg + rgs, ... (< rows) and the unit's channels in pairs (one
    fdot2 per pair: the pair's sum, then the accumulator) or one at a time; then the row groups in order."""
    n = v.shape[-1]
    nu = n // unit
    t = f32(v).reshape(-1, 128 // rgs, rgs, nu, unit)
    if shift_last_unit_of is not None:
        # the LAST unit of every tile of shift_last_unit_of units reads the columns of the unit after it
        u = torch.arange(nu)
        t = t[:, :, :, torch.where((u + 1) % shift_last_unit_of == 0, (u + 1) % nu, u)]
    sm = torch.zeros(t.shape[0], rgs, nu)
    sq = torch.zeros(t.shape[0], rgs, nu)
    for k in range(128 // rgs):
        live = (torch.arange(rgs) + k * rgs < rows).float()[None, :, None]
        for j in range(0, unit, 2 if pairs else 1):
            a = t[:, k, :, :, j] * live
            if pairs:
                b = t[:, k, :, :, j + 1] * live
                sm = sm + (a + b)
                sq = sq + (a * a + b * b)
            else:
                sm = sm + a
                sq = sq + a * a
    s1 = torch.zeros(t.shape[0], nu)
    s2 = torch.zeros(t.shape[0], nu)
    for g in range(rgs):
        s1 = s1 + sm[:, g]
        s2 = s2 + sq[:, g]
    return torch.stack([s1, s2], -1).double()


GNSTAT_FORMS = [("plain", 2, 16, 16, 64, 0, 320, 3, 1, ""), ("rowvec + residual", 2, 16, 16, 64, 0, 320, 3, 1, "rv res"),
                ("3 blocks per image", 2, 16, 24, 64, 0, 320, 3, 1, "")]


def gnstat_cases(rand, unit=10):
    out = []
    for i, form in enumerate(GNSTAT_FORMS):
        op = conv_operands(rand, form, 500 + 10 * i)
        acc = acc32(im2col(_xc(op), 3), pack_w(op["w"]), "chunk")
        v = conv_epilogue(acc, op)
        ref, s = gnstat_ref(v, unit)
        tag = f"gnstat {form[0]} {form[1]}x{form[2]}x{form[3]}x{form[4]}->{form[6]} unit {unit}"
        out.append((f"legit fdot2 order, 8 row groups (8-wave epilogue) {tag}", gnstat_emul(v, unit, 8), ref, s, True))
        out.append((f"legit fdot2 order, 16 row groups (4-wave epilogue) {tag}", gnstat_emul(v, unit, 16), ref, s, True))
        out.append((f"legit fdot2 order, 32 row groups (split-K reduce path) {tag}", gnstat_emul(v, unit, 32), ref, s, True))
        out.append((f"legit plain sequential fp32 {tag}", gnstat_emul(v, unit, 1, pairs=False), ref, s, True))
        alpha = torch.tensor(op["alpha"], dtype=torch.float32)
        add = f32(_add64(op, v.shape[-1]))
        pre = (acc.reshape(v.shape) + add) * alpha
        raw = pre if op["res"] is None else f32(rne(pre)) + f32(op["res"])
        out.append((f"mutant statistics of the unrounded fp32 accumulators {tag}", gnstat_emul(raw.double(), unit, 8), ref, s, False))
        if op["res"] is not None:
            out.append((f"mutant statistics taken before the residual add {tag}", gnstat_emul(rne(pre), unit, 8), ref, s, False))
        out.append((f"mutant row 127 of a block left out {tag}", gnstat_emul(v, unit, 8, rows=127), ref, s, False))
        out.append((f"mutant unit u reads the columns of unit u+1 at a tile's last unit {tag}",
                    gnstat_emul(v, unit, 8, shift_last_unit_of=16), ref, s, False))
    return out


# ------------------------------------------------------------------ GroupNorm pieces
def _group_rows(y, groups):
    """[B, H, W, C] -> [B, groups, HW * C / groups]."""
    b, h, w_, c = y.shape
    return y.reshape(b, h * w_, groups, c // groups).permute(0, 2, 1, 3).reshape(b, groups, -1)


def exact_stats(y, groups, eps, *, eps_mul=1.0, unbiased=False):
    """float64 (mean, rstd) per (image, group), each rounded ONCE to fp32 as the kernels hand them on."""
    r = _group_rows(y.double(), groups)
    var = r.var(-1, unbiased=unbiased)
    return f32v(r.mean(-1)), f32v(1.0 / torch.sqrt(var + eps * eps_mul))


def _per_channel(t, c):
    """[B, groups] -> [B, 1, 1, C]."""
    return t.repeat_interleave(c // t.shape[1], 1)[:, None, None, :]


def gn_apply32(y, gamma, beta, mean, rstd, *, silu=True, silu_ulp=None, rnd=rne):
    """The apply arithmetic in fp32: sc = gamma rstd, sh = beta - mean sc, o = y sc + sh, SiLU as o * rcp(1 + exp(-o)); silu_ulp: a
    +-1 tensor, the SiLU result moved by one fp32 ulp in that direction (v_exp / v_rcp are accurate to about an ulp)."""
    c = y.shape[-1]
    sc = f32(gamma) * f32(_per_channel(rstd, c))
    sh = f32(beta) - f32(_per_channel(mean, c)) * sc
    o = f32(y) * sc + sh
    if silu:
        o = o * (1.0 / (1.0 + torch.exp(-o)))
        if silu_ulp is not None:
            o = o * (1.0 + silu_ulp.float() * 2.0 ** -23)
    return rnd(o)


def epilogue_form_stats(x, groups, eps, unit=2):
    """(mean, rstd) from the epilogue form of the statistics: fp32 sums per (128-row block, unit) as gn_tile_stats leaves them,
    combined in fp64 (gn_image_stats / saspa_conv_halo.hip:487-515)."""
    b, h, w_, c = x.shape
    st = gnstat_emul(x, unit, 8).reshape(b, -1, groups, c // groups // unit, 2).sum((1, 3))
    cnt = float(h * w_ * c // groups)
    mean = st[..., 0] / cnt
    var = (st[..., 1] / cnt - mean * mean).clamp_min(0)
    return f32v(mean), f32v(1.0 / torch.sqrt(var + eps))


# ------------------------------------------------------------------ family gn_chain: conv -> bf16 -> GroupNorm -> SiLU
# (b, h, w, cin, n, per-image rowvec?, kind): 320 items per (image, group) at 8x8x640 (the second slot of 256 partly filled), 440 at
# 8x11; "lowvar": weights of 3e-3 / sqrt(K) and no bias, the conv output's variance is about eps
GN_CHAIN_FORMS = [(3, 8, 8, 128, 640, True, "normal"), (2, 8, 11, 128, 640, False, "normal"), (2, 8, 8, 128, 640, True, "lowvar")]
GN_CHAIN_ALPHA = 0.75


def gn_chain_operands(rand, form, seed):
    b, h, w_, cin, n, per_image, kind = form
    low = kind == "lowvar"
    op = dict(x=q(rand(b, h, w_, cin, seed=seed)), x2=None,
              w=q(rand(n, cin, 3, 3, seed=seed + 2, scale=(3e-3 if low else 1.0) / math.sqrt(9 * cin))),
              bias=None if low else f32v(rand(n, seed=seed + 3)),
              rowvec=f32v(rand(b if per_image else 1, n, seed=seed + 4) * (1e-3 if low else 1.0)), res=None, alpha=GN_CHAIN_ALPHA,
              stride=1, kh=3, hw=h * w_, gamma=f32v(1 + 0.2 * rand(n, seed=seed + 6)), beta=f32v(0.3 * rand(n, seed=seed + 7)))
    return op


def _rv_rows(op):
    rv = op["rowvec"]
    return rv.expand(op["x"].shape[0], rv.shape[1])


def gn_chain_ref(op, groups=GROUPS, eps=EPS):
    """float64 conv -> rounded to the storage type (saspa_norm.hip:608-610) -> GroupNorm -> SiLU -> rounded (the output; :647) ->
    (ref, chain magnitude)."""
    o2 = dict(op, rowvec=_rv_rows(op))
    pre, s_y = conv_ref(o2)
    y = rne(pre)
    mean, rstd = exact_stats(y, groups, eps)
    n = y.shape[-1]
    mc, rc = _per_channel(mean, n), _per_channel(rstd, n)
    xhat = (y - mc) * rc
    z = xhat * op["gamma"] + op["beta"]
    return rne(z * torch.sigmoid(z)), chain_norm_scale(xhat, op["gamma"], op["beta"], s_y, rc, (mc * rc).expand_as(xhat))


def lane_stats(y, groups, eps, *, drop_tail=False, eps_mul=1.0, unbiased=False):
    """splitk_gn_kernel's statistics: item = 4 channels of one pixel of the group, lane tid sums items tid + 256 i in fp32 (:591-616),
    the 256 lanes are combined in fp64 (:617-627).  drop_tail: the items past the last whole 256 left out (mutant)."""
    b, h, w_, n = y.shape
    cpg = n // groups
    it = f32(y).reshape(b, h * w_, groups, cpg // 4, 4).permute(0, 2, 1, 3, 4).reshape(b, groups, -1, 4)
    items = it.shape[2]
    slots = -(-items // 256)
    it = F.pad(it, (0, 0, 0, slots * 256 - items)).reshape(b, groups, slots, 256, 4)
    sm = torch.zeros(b, groups, 256)
    sq = torch.zeros(b, groups, 256)
    for i in range(items // 256 if drop_tail else slots):
        for j in range(4):
            sm = sm + it[:, :, i, :, j]
            sq = sq + it[:, :, i, :, j] * it[:, :, i, :, j]
    cnt = float(h * w_ * cpg)
    mean = sm.double().sum(-1) / cnt
    var = (sq.double().sum(-1) / cnt - mean * mean).clamp_min(0)
    if unbiased:
        var = var * cnt / (cnt - 1)
    return f32v(mean), f32v(1.0 / torch.sqrt(var + eps * eps_mul))


def gn_chain_emul(op, rand, *, ks=2, groups=GROUPS, eps=EPS, stats="lane", silu_ulp=False, keep_fp32=False, alpha_after=False,
                  rv_prev=False, **stat_kw):
    a, wp = im2col(op["x"], 3), pack_w(op["w"])
    acc = acc32(a, wp, "chunk", ks=ks).reshape(*op["x"].shape[:3], -1)
    n = acc.shape[-1]
    t = acc if op["bias"] is None else acc + f32(op["bias"])
    rv = f32(_rv_rows(op))
    t = t + (rv.roll(1, 0) if rv_prev else rv)[:, None, None, :]
    alpha = torch.tensor(op["alpha"], dtype=torch.float32)
    y = (t * alpha).double() if keep_fp32 else (f32(rne(t)) * alpha).double() if alpha_after else rne(t * alpha)
    mean, rstd = lane_stats(y, groups, eps, **stat_kw) if stats == "lane" else exact_stats(y, groups, eps, **stat_kw)
    ulp = torch.sign(rand(*y.shape, seed=77)) if silu_ulp else None
    return gn_apply32(y, op["gamma"], op["beta"], mean, rstd, silu_ulp=ulp)


def gn_chain_cases(rand):
    out = []
    for i, form in enumerate(GN_CHAIN_FORMS):
        b, h, w_, cin, n, per_image, kind = form
        op = gn_chain_operands(rand, form, 600 + 10 * i)
        ref, s = gn_chain_ref(op)
        tag = f"gn_chain {b}x{h}x{w_}x{cin}->{n} {kind}{' shared rowvec' if not per_image else ''}"
        emu = lambda **kw: gn_chain_emul(op, rand, **kw)  # noqa: E731
        out.append((f"legit 2 slabs in slab order, lane statistics {tag}", emu(), ref, s, True))
        out.append((f"legit 3 slabs in slab order, lane statistics {tag}", emu(ks=3), ref, s, True))
        out.append((f"legit fp64 statistics {tag}", emu(stats="exact"), ref, s, True))
        out.append((f"legit SiLU through exp + rcp off by one fp32 ulp {tag}", emu(silu_ulp=True), ref, s, True))
        out.append((f"legit one output flipped by an ulp, worst placed {tag}", _T()._one_flip(ref, s), ref, s, True))
        out.append((f"mutant intermediate kept in fp32 (rounding point skipped) {tag}", emu(keep_fp32=True), ref, s, False))
        out.append((f"mutant alpha applied after the rounding {tag}", emu(alpha_after=True), ref, s, False))
        if per_image:
            out.append((f"mutant rowvec of image b-1 splitk_gn {tag}", emu(rv_prev=True), ref, s, False))
        if kind == "lowvar":
            out.append((f"mutant eps x 10 splitk_gn {tag}", emu(eps_mul=10.0), ref, s, False))
        else:
            out.append((f"mutant n-1 variance splitk_gn {tag}", emu(unbiased=True), ref, s, False))
        out.append((f"mutant tail items beyond a multiple of 256 left out of the statistics {tag}", emu(drop_tail=True), ref, s, False))
    return out


# ------------------------------------------------------------------ family conv_gn: GroupNorm -> SiLU -> bf16 -> 3x3 conv
# (b, h, w, c0, c1, n, kind, flags).  Inputs carry a mean offset and beta is near 1: SiLU(shift) is far from zero, so a pad pixel
# that was normalised instead of left zero shows; mean and spread differ from channel to channel (1 + z_c, 0.5 + 1.5 u_c), so that
# statistics or an affine taken from the wrong group / chunk show.  "lowvar": 0.01 + 1e-3 z (eps decides); N is 64 where the CPU
# proof needs no more, and the first form has 4 images so that the n-1 variance (n = 512: the smallest group the halo kernel
# serves) stands clear of the sampling noise of the bias
CONV_GN_FORMS = [(4, 16, 16, 64, 0, 320, "offset", "rv res"), (2, 16, 16, 64, 0, 64, "lowvar", ""),
                 (1, 32, 32, 96, 32, 64, "offset", ""), (2, 16, 16, 320, 0, 64, "offset", "ks")]


def conv_gn_operands(rand, form, seed):
    b, h, w_, c0, c1, n, kind, flags = form
    c = c0 + c1

    def src(cc, sd):
        z = rand(b, h, w_, cc, seed=sd)
        if kind == "lowvar":
            return q(z * 1e-3 + 0.01)
        spread = 0.5 + 0.75 * (1 + torch.erf(rand(cc, seed=sd + 20) / math.sqrt(2)))
        return q(z * spread + 1.0 + rand(cc, seed=sd + 30))
    return dict(x=src(c0, seed), x2=src(c1, seed + 1) if c1 else None,
                w=q(rand(n, c, 3, 3, seed=seed + 2, scale=1 / math.sqrt(9 * c))), bias=f32v(rand(n, seed=seed + 3)),
                rowvec=f32v(rand(b, n, seed=seed + 4)) if "rv" in flags else None,
                res=q(rand(b, h, w_, n, seed=seed + 5)) if "res" in flags else None, alpha=1.0, stride=1, kh=3, hw=h * w_,
                gamma=f32v(1 + 0.2 * rand(c, seed=seed + 6)), beta=f32v(1 + 0.3 * rand(c, seed=seed + 7)))


def conv_gn_ref(op, groups=GROUPS, eps=EPS, *, silu=True, two_roundings=True):
    """float64 GroupNorm -> SiLU -> rounded to bf16 (saspa_conv_halo.hip:301; gn_apply_kernel's store in the two-launch form) ->
    conv with the epilogue's rounding points -> (ref, chain magnitude, the normalised input)."""
    xc = _xc(op)
    c = xc.shape[-1]
    mean, rstd = exact_stats(xc, groups, eps)
    mc, rc = _per_channel(mean, c), _per_channel(rstd, c)
    xhat = (xc - mc) * rc
    z = xhat * op["gamma"] + op["beta"]
    xn = rne(z * torch.sigmoid(z) if silu else z)
    s_n = norm_scale(xhat, op["gamma"], op["beta"], (mc * rc).expand_as(xhat))
    ref, _ = conv_ref(op, xn, two_roundings=two_roundings)
    n = op["w"].shape[0]
    s = chain_gemm_scale(im2col(xn, 3).reshape(-1, 9 * c), pack_w(op["w"]).reshape(n, -1), prev=im2col(s_n, 3).reshape(-1, 9 * c))
    s = s.reshape(ref.shape)
    if op["bias"] is not None:
        s = s + op["bias"].abs()
    if op["rowvec"] is not None:
        s = s + op["rowvec"].abs()[:, None, None, :]
    s = abs(op["alpha"]) * s
    if op["res"] is not None:
        s = s + op["res"].abs()
    return ref, s, xn


def conv_gn_emul(op, *, groups=GROUPS, eps=EPS, order="chunk32", ks=1, stats="pass", rnd_n=rne, eps_mul=1.0, unbiased=False,
                 pad_first=False, prev_chunk=False, halo_rows=False, straddle=False):
    """The fused chain in fp32.  stats: "pass" (the statistics pass: test_errbudget.gn_kernel_stats), "epi" (a producer's epilogue
    statistics), "exact".  The other options are the mutants."""
    xc = _xc(op)
    b, h, w_, c = xc.shape
    n = op["w"].shape[0]
    cpg = c // groups
    if stats == "pass":
        mean, rstd = _T().gn_kernel_stats(xc.reshape(b, h * w_, c), groups, eps)
    elif stats == "epi":
        mean, rstd = epilogue_form_stats(xc, groups, eps)
    else:
        mean, rstd = exact_stats(xc, groups, eps)
    if eps_mul != 1.0 or unbiased:
        cnt = float(h * w_ * cpg)
        var = (rstd ** -2 - eps) * (cnt / (cnt - 1) if unbiased else 1.0)
        rstd = f32v((var + eps * eps_mul) ** -0.5)
    mch, rch = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)                    # [B, C]
    if straddle:
        first = torch.arange(c) // 32 * 32                                                       # a chunk's first channel
        mch, rch = mch[:, first], rch[:, first]
    sc = f32(op["gamma"]) * f32(rch)
    sh = f32(op["beta"]) - f32(mch) * sc

    def norm(x, sc_, sh_, silu=True):
        o = f32(x) * sc_[:, None, None, :] + sh_[:, None, None, :]
        return rnd_n(o * (1.0 / (1.0 + torch.exp(-o))) if silu else o)
    xn = norm(xc, sc, sh)
    if not (pad_first or prev_chunk or halo_rows):
        return conv_epilogue(acc32(im2col(xn, 3), pack_w(op["w"]), order, ks=ks), op, reduce_path=ks > 1)
    wf = f32(op["w"])
    if pad_first:
        acc = conv_nhwc(norm(F.pad(xc, (0, 0, 1, 1, 1, 1)), sc, sh).float(), wf, pad=0)
    else:
        acc = conv_nhwc(f32(xn), wf)
    if prev_chunk:
        # tap (0, 0) of chunk k >= 1 is normalised with the scale / shift of chunk k - 1
        scp, shp = sc.clone(), sh.clone()
        scp[:, 32:], shp[:, 32:] = sc[:, :-32], sh[:, :-32]
        w0 = torch.zeros_like(wf)
        w0[:, :, 0, 0] = wf[:, :, 0, 0]
        acc = acc + conv_nhwc(f32(norm(xc, scp, shp) - xn), w0)
    if halo_rows:
        # 256-pixel tiles of whole image rows: a tile's first / last row reads the row above / below it from the halo, un-SiLU'd
        rows = 256 // w_
        d = f32(norm(xc, sc, sh, silu=False) - xn)
        i = torch.arange(h)
        for ky, mask in ((0, (i % rows == 0) & (i > 0)), (2, (i % rows == rows - 1) & (i < h - 1))):
            wk = torch.zeros_like(wf)
            wk[:, :, ky] = wf[:, :, ky]
            acc = acc + conv_nhwc(d, wk) * mask.float()[None, :, None, None]
    return conv_epilogue(acc.reshape(-1, n), op)


def conv_gn_cases(rand):
    out = []
    for i, form in enumerate(CONV_GN_FORMS):
        b, h, w_, c0, c1, n, kind, flags = form
        op = conv_gn_operands(rand, form, 700 + 10 * i)
        ks = 3 if "ks" in flags else 1
        ref, s, _ = conv_gn_ref(op, two_roundings=ks == 1)
        tag = f"conv_gn {b}x{h}x{w_}x{c0}{'+' + str(c1) if c1 else ''}->{n} {kind}"
        emu = lambda **kw: conv_gn_emul(op, ks=ks, **kw)  # noqa: E731
        out.append((f"legit chunk32 K order, pass-form statistics {tag}", emu(), ref, s, True))
        out.append((f"legit chunk-major K order, epilogue-form statistics {tag}", emu(order="chunk", stats="epi"), ref, s, True))
        out.append((f"legit tap-major K order, exact statistics {tag}", emu(order="tap", stats="exact"), ref, s, True))
        if ks > 1:
            out.append((f"legit 2 slabs in slab order {tag}", conv_gn_emul(op, ks=2), ref, s, True))
        else:
            out.append((f"mutant zero padding applied before the normalisation {tag}", emu(pad_first=True), ref, s, False))
            out.append((f"mutant scale / shift of the previous 32-channel chunk for a chunk's first tap {tag}", emu(prev_chunk=True),
                        ref, s, False))
        out.append((f"mutant normalised input truncated to bf16 {tag}", emu(rnd_n=trunc), ref, s, False))
        if kind == "lowvar":
            out.append((f"mutant eps x 10 conv_gn {tag}", emu(eps_mul=10.0), ref, s, False))
        elif h * w_ * (c0 + c1) // GROUPS <= 512:        # (1 / 2n of the scale: beyond n = 512 it is inside the sampling noise)
            out.append((f"mutant n-1 variance conv_gn {tag}", emu(unbiased=True), ref, s, False))
        if 256 // w_ < h:
            out.append((f"mutant SiLU skipped on the halo rows {tag}", emu(halo_rows=True), ref, s, False))
        if ((c0 + c1) // GROUPS) % 32 and 32 % ((c0 + c1) // GROUPS):
            out.append((f"mutant a chunk that straddles groups takes the first group's statistics {tag}", emu(straddle=True), ref, s,
                        False))
    return out
