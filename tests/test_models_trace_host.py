"""What `models.py` and `blip.py` ask of `ops`, call for call, against a recorded trace (no GPU: tests/models_trace.py builds the
networks on the CPU and runs their methods on CPU tensors with a recording stand-in for `ops`), and what they pack: a manifest of
every network's `p` (shape, dtype, layout attributes, bytes, shared storage per key) and routing state.  Every form of the three
halves of a transformer block, the resnets' bf16 / MX-fp8 arms, the encoder stacks and the whole networks' walks are pinned.
`python tests/test_models_trace_host.py --write-golden` records tests/golden/models_call_trace.json; `--write-golden CASE...`
re-records the named cases only; `--show CASE...` prints their calls.

The fixture: the bf16 block-level cases at levels 0 and 1 and the method-level cases marked "full" hold their calls in full (every
distinct call once, in `lines`, delta-coded; a case lists indices).  Whole-network cases -- and, to stay under 64 KB, the fp16 / fp32
and mid-block repeats of the block cases and the encoder stacks -- hold models_trace.chain's running digests: as strict for pass and
fail, the first differing index is reported with the freshly computed call, and `--show CASE` prints the calls."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import saspa_aug_amd  # noqa: E402,F401
from saspa_aug_amd import config as CFG  # noqa: E402
from saspa_aug_amd import models, ops  # noqa: E402
import models_trace as MT  # noqa: E402
from models_trace import build, chain, run_case  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models_call_trace.json")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {BF16: "bf16", F16: "f16", F32: "f32"}
TINY, TINY_XL = CFG.tiny(), CFG.tiny_xl()
# the smallest networks that reach each branch: two levels of width 320 (the level-0 forms), 128 | 256 (fp8: multiples of 128),
# 128 | 192 (a block that stays bf16 next to an fp8 one), 320 | 960 (MX-fp8 resnet convs: N % 160 == 0, conv2's C > 640 at level 1)
W320 = dict(in_channels=4, out_channels=4, block_out=(320, 320), attn=(True, True), layers=1, heads=8, groups=32, ctx_dim=64, temb_dim=64)
W128 = dict(W320, block_out=(128, 256), heads=4)
W192 = dict(W320, block_out=(128, 192), heads=4)
W960 = dict(W320, block_out=(320, 960), attn=(False, False))
L0, L1, MID = "down_blocks.0.attentions.0", "down_blocks.1.attentions.0", "mid_block.attentions.0"
SIDE = {L0: (16, 16), L1: (8, 8), MID: (8, 8)}          # a 16 x 16 latent: n = 256 at level 0, 64 (no multiple of 256) below
CASES = []


def case(name, fn, store="full", **opts):
    CASES.append((name, fn, store, opts))


def z(log, name, shape, dtype):
    return log.name(torch.zeros(tuple(shape), dtype=dtype), name)


# ---- transformer blocks -------------------------------------------------------------------------------------------------------------
def block(pfx, dtype=BF16, cfg=W320, net="w320", cfg_pair=False, ctx_len=77, ctx_b=None, b=1, side=None, sd_edit=None, calls=1, **kw):
    """transformer(pfx) of a UNet on `b` samples; the trace starts behind prepare_context (which has cases of its own)."""
    def setup(log):
        n = build(log, f"{net} {DT[dtype]}", "unet", cfg, dtype, sd_edit, **kw)
        n.prepare_context(z(log, "ctx", (ctx_b or (2 * b if cfg_pair else b), ctx_len, cfg["ctx_dim"]), dtype))
        del log.lines[:]
        return n, side or SIDE[pfx]

    def fn(log):
        n, (hh, ww) = setup(log)
        c = n.p[pfx + ".norm.g"].numel()
        out = [n.transformer(pfx, z(log, "x", (b, hh, ww, c), dtype), cfg_pair=cfg_pair) for _ in range(calls)]
        return out + [{"calibrated": sorted(t for t, done in n.fp8_ffout.items() if done)}] if kw.get("fp8") else out
    fn.which = lambda log: (lambda n, hw: n.which(pfx, b, hw[0], hw[1], cfg_pair=cfg_pair))(*setup(log))
    return fn


def with_q_bias(sd):
    for k in [k for k in sd if k.endswith(".attn2.to_q.weight")]:
        sd[k[:-len("weight")] + "bias"] = torch.zeros(sd[k].shape[0])
    return sd


for _dt in (BF16, F16, F32):
    for _pfx, _lv in ((L0, "level 0"), (L1, "level 1"), (MID, "mid")):
        for _pred in (True, False):
            for _pair in (False, True):
                case(f"block {DT[_dt]} {_lv} predicates={int(_pred)} cfg_pair={int(_pair)}", block(_pfx, _dt, cfg_pair=_pair),
                     store="full" if (_dt == BF16 and _pfx != MID) else "digest", pred=_pred)
for _len in (96, 104):
    for _pair in (False, True):
        case(f"block bf16 level 0 context {_len} cfg_pair={int(_pair)}", block(L0, ctx_len=_len, cfg_pair=_pair), pred=True)
case("block bf16 level 0 SASPA_XATTN=0", block(L0), pred=True, env={"SASPA_XATTN": "0"})
case("block bf16 level 0 SASPA_XATTN=0 cfg_pair", block(L0, cfg_pair=True), pred=True, env={"SASPA_XATTN": "0"})
case("block bf16 level 0 SASPA_FF_BLOCK=0", block(L0, net="w320 ff_block=0"), pred=True,
     env={"SASPA_FF_BLOCK": "0", "SASPA_FF_BLOCK_MIN_ROWS": "0"})
for _pred in (True, False):
    case(f"block bf16 level 0 SASPA_FF_BLOCK_MIN_ROWS=0 predicates={int(_pred)}", block(L0), pred=_pred, env={"SASPA_FF_BLOCK_MIN_ROWS": "0"})
    case(f"block bf16 level 0 SASPA_FF_BLOCK_MIN_ROWS=0 cfg_pair predicates={int(_pred)}", block(L0, cfg_pair=True), pred=_pred,
         env={"SASPA_FF_BLOCK_MIN_ROWS": "0"})
case("block bf16 level 1 SASPA_FF_BLOCK_MIN_ROWS=0 (n = 64)", block(L1), pred=True, env={"SASPA_FF_BLOCK_MIN_ROWS": "0"})
case("block bf16 level 0 default rule, 96 samples: ff_block_takes(24576)", block(L0, b=96), pred=True)
case("block bf16 level 0 SASPA_ATTN_VROW=0", block(L0), pred=False, env={"SASPA_ATTN_VROW": "0"})
case("block bf16 level 0 30 tokens (n % 32 != 0)", block(L0, side=(6, 5)), pred=True, env={"SASPA_FF_BLOCK_MIN_ROWS": "0"})
case("block bf16 level 0 attn2.to_q.bias: no xattn pack", block(L0, net="w320 q bias", sd_edit=with_q_bias), pred=True)
# more than one block per transformer (tiny_xl: depth 2 at level 1): the rows double in block 0, block 1 runs at 2B rows throughout
_XL1 = "down_blocks.1.attentions.0"
case("block tiny_xl bf16 level 1, two blocks, cfg_pair", block(_XL1, cfg=TINY_XL["unet"], net="tiny_xl unet", cfg_pair=True, side=(4, 4)), "digest")
case("block bf16 level 0 cfg_pair, context of one sample", block(L0, cfg_pair=True, ctx_b=1), pred=True)
# fp8
case("fp8 calibrated level 0: calibration, then steady state", block(L0, cfg=W128, net="w128 fp8", fp8=True, calls=2))
case("fp8 calibrated level 1", block(L1, cfg=W128, net="w128 fp8", fp8=True))
case("fp8 calibrated level 0 under capture", block(L0, cfg=W128, net="w128 fp8", fp8=True), capturing=True)
case("fp8 mx level 0", block(L0, cfg=W128, net="w128 fp8 mx", fp8=True, fp8_ff="mx", calls=2), capturing=True)
case("fp8 SASPA_FP8_BREADTH=ln level 0", block(L0, cfg=W128, net="w128 fp8 ln", fp8=True), env={"SASPA_FP8_BREADTH": "ln"})
case("fp8 SASPA_ATTN_VROW=0 level 0", block(L0, cfg=W128, net="w128 fp8 vrow=0", fp8=True), env={"SASPA_ATTN_VROW": "0"})
case("fp8 net, width 192 stays bf16", block(L1, cfg=W192, net="w192 fp8", fp8=True), "digest")
case("fp8 net, width 128 next to it", block(L0, cfg=W192, net="w192 fp8", fp8=True), "digest")
case("fp8 with fp16", block(L0, F16, cfg=W128, net="w128 fp8 f16", fp8=True))
case("fp8_ff='block'", block(L0, cfg=W128, net="w128 fp8 block", fp8=True, fp8_ff="block"))
case("fp8 calibrated level 0 cfg_pair (dup_rows)", block(L0, cfg=W128, net="w128 fp8", fp8=True, cfg_pair=True))
case("fp8 mx level 0 cfg_pair (dup_rows)", block(L0, cfg=W128, net="w128 fp8 mx", fp8=True, fp8_ff="mx", cfg_pair=True))
for _len in (77, 96, 104):
    case(f"prepare_context bf16 context {_len}",
         lambda log, n=_len: build(log, "w320 bf16", "unet", W320, BF16).prepare_context(z(log, "ctx", (2, n, 64), BF16)), "digest")
case("prepare_context bf16 SASPA_XATTN=0", lambda log: build(log, "w320 bf16", "unet", W320, BF16).prepare_context(z(log, "ctx", (2, 77, 64), BF16)),
     store="digest", env={"SASPA_XATTN": "0"})


# ---- resnets --------------------------------------------------------------------------------------------------------------------------
def resnet(pfx, shape, dtype=BF16, cfg=None, net="tiny", kind="unet", step=0, x2=None, **kw):
    def fn(log):
        n = build(log, f"{net} {kind} {DT[dtype]}", kind, cfg or TINY[kind], dtype, **kw)
        n.prepare_timesteps([801, 401, 1])
        if step is None:
            n.bind_step_state(z(log, "temb_cur", (n.temb_total,), F32))
        del log.lines[:]
        x = z(log, "x", shape, dtype)
        out = n.resnet(pfx, x, step, 1e-5, x2=None if x2 is None else z(log, "x2", shape[:3] + (x2,), dtype))
        return [out, sorted(n.fp8_convs)]
    return fn


for _dt in (BF16, F32):
    case(f"resnet {DT[_dt]} no shortcut step=2", resnet("down_blocks.0.resnets.0", (2, 8, 8, 32), _dt, step=2))
    case(f"resnet {DT[_dt]} shortcut step=None", resnet("down_blocks.1.resnets.0", (2, 4, 4, 32), _dt, step=None))
    case(f"resnet {DT[_dt]} decoder concat", resnet("up_blocks.3.resnets.2", (2, 8, 8, 32), _dt, x2=32))
_fp8c = dict(cfg=W960, net="w960 fp8_conv", fp8=True, fp8_conv=True)
case("resnet fp8_conv: both convs MX (16384 pixels, 320 -> 320)", resnet("down_blocks.0.resnets.0", (1, 128, 128, 320), **_fp8c))
case("resnet fp8_conv: conv1 only (8192 pixels, 320 -> 960)", resnet("down_blocks.1.resnets.0", (1, 64, 128, 320), step=None, **_fp8c))
case("resnet fp8_conv: conv2 only (decoder concat, 960 + 320 -> 320)", resnet("up_blocks.1.resnets.0", (1, 128, 128, 960), x2=320, **_fp8c))
case("resnet fp8_conv: neither (64 pixels)", resnet("down_blocks.0.resnets.0", (1, 8, 8, 320), **_fp8c))
case("resnet fp8_conv: decoder concat, both convs MX", resnet("up_blocks.1.resnets.1", (1, 128, 128, 320), x2=320, **_fp8c))


# ---- whole networks ---------------------------------------------------------------------------------------------------------------------
def net_case(kind, fam, dtype, run, net=None, cfg=None, **kw):
    def fn(log):
        n = build(log, net or f"{'tiny_xl' if fam is TINY_XL else 'tiny'} {kind} {DT[dtype]}", kind, cfg or fam[kind], dtype, **kw)
        return run(log, n, dtype)
    return fn


def _added(log):
    return (z(log, "text_embeds", (2, 64), F32), np.arange(12, dtype=np.float32).reshape(2, 6))


def _prepared(log, n, dtype, b=2, ctx_b=None):
    n.prepare_timesteps([801, 401, 1], _added(log) if "add_embed" in n.cfg else None)
    n.prepare_context(z(log, "ctx", (ctx_b or b, 77, n.cfg["ctx_dim"]), dtype))
    del log.lines[:]
    return n


def _timesteps(log, n, dtype, added=False):
    n.prepare_timesteps([801, 401, 1], _added(log) if added else None)
    return [n.temb_all, MT.routing(n)["temb_off"]]


def _encode(cfg_pair=False, residual=False):
    def run(log, n, dtype):
        _prepared(log, n, dtype, ctx_b=4 if cfg_pair else 2)
        c = n.cfg["block_out"][0]
        return n.encode(z(log, "sample", (2, 8, 8, 8), dtype), 1, z(log, "cond_emb", (2, 8, 8, c), dtype) if residual else None, cfg_pair=cfg_pair)
    return run


def _skips(log, n, dtype, rows, first_rows):
    bo, out, side = n.cfg["block_out"], [], 8
    out.append(z(log, "skip", (first_rows, side, side, bo[0]), dtype))
    for i, c in enumerate(bo):
        out += [z(log, "skip", (rows, side, side, c), dtype) for _ in range(n.cfg["layers"])]
        if i != len(bo) - 1:
            side //= 2
            out.append(z(log, "skip", (rows, side, side, c), dtype))
    return z(log, "mid", (rows, side, side, bo[-1]), dtype), out


def _decode(log, n, dtype):
    _prepared(log, n, dtype)
    mid, skips = _skips(log, n, dtype, 2, 2)
    if dtype == BF16:
        n.bind_step_state(z(log, "temb_cur", (2, n.temb_total) if "add_embed" in n.cfg else (n.temb_total,), F32))
    return n.decode(mid, skips, None if dtype == BF16 else 2, out=z(log, "eps", (2, 8, 8, 8), dtype) if dtype == BF16 else None)


def _cn(what, with_unet, cfg_pair=False):
    def run(log, n, dtype):
        _prepared(log, n, dtype, ctx_b=4 if cfg_pair else 2)
        rows = 4 if cfg_pair else 2
        mid, feats = _skips(log, n, dtype, rows, 2)
        umid, uskips = _skips(log, n, dtype, rows, 2) if with_unet else (None, None)
        if what == "zero_convs":
            return n.zero_convs(mid, feats, 0.75, uskips, umid, cfg_pair=cfg_pair)
        return n.forward(z(log, "sample", (2, 8, 8, 8), dtype), 1, z(log, "cond_emb", (2, 8, 8, n.cfg["block_out"][0]), dtype), 0.75,
                         uskips, umid, cfg_pair=cfg_pair)
    return run


for _dt in (BF16, F32):
    case(f"unet tiny {DT[_dt]} prepare_timesteps", net_case("unet", TINY, _dt, _timesteps), "digest")
    case(f"unet tiny {DT[_dt]} prepare_context", net_case("unet", TINY, _dt, lambda log, n, dt: n.prepare_context(z(log, "ctx", (2, 77, 64), dt))), "digest")
    case(f"unet tiny {DT[_dt]} encode", net_case("unet", TINY, _dt, _encode()), "digest")
    case(f"unet tiny {DT[_dt]} encode cfg_pair", net_case("unet", TINY, _dt, _encode(cfg_pair=True)), "digest")
    case(f"unet tiny {DT[_dt]} decode", net_case("unet", TINY, _dt, _decode), "digest")
case("unet tiny_xl bf16 prepare_timesteps with added", net_case("unet", TINY_XL, BF16, lambda log, n, dt: _timesteps(log, n, dt, True)), "digest")
case("unet tiny_xl bf16 prepare_timesteps without added", net_case("unet", TINY_XL, BF16, _timesteps))
case("unet tiny_xl bf16 encode", net_case("unet", TINY_XL, BF16, _encode()), "digest")
case("unet tiny_xl bf16 decode", net_case("unet", TINY_XL, BF16, _decode), "digest")
case("unet tiny_xl bf16 encode cfg_pair refused", net_case("unet", TINY_XL, BF16, _encode(cfg_pair=True)))
# channel counts that are no multiples of 8: where a decoder resnet's (from below, skip) split shows in the packed bytes
_ODD = dict(W320, block_out=(12, 20), attn=(False, False), heads=2, groups=4, ctx_dim=16, temb_dim=16)
case("unet widths 12 | 20 fp32: packed only (manifest)",
     lambda log: [k for k in build(log, "odd widths unet f32", "unet", _ODD, F32).p if k.endswith("conv_shortcut.w")])
_NOATTN0 = dict(TINY["unet"], attn=(False, True, True, False))
case("unet tiny bf16, no attention at level 0: encode cfg_pair",
     net_case("unet", TINY, BF16, _encode(cfg_pair=True), net="tiny no-attn0 unet bf16", cfg=_NOATTN0), "digest")
case("controlnet tiny bf16 cond_embedding",
     net_case("controlnet", TINY, BF16, lambda log, n, dt: n.cond_embedding(z(log, "cond", (2, 64, 64, 8), dt))))
for _u in (False, True):
    for _pair in (False, True):
        _sfx = f"{' + unet skips' if _u else ''}{' cfg_pair' if _pair else ''}"
        case("controlnet tiny bf16 zero_convs" + _sfx, net_case("controlnet", TINY, BF16, _cn("zero_convs", _u, _pair)),
             "full" if (_u and _pair) else "digest")
        case("controlnet tiny bf16 forward" + _sfx, net_case("controlnet", TINY, BF16, _cn("forward", _u, _pair)), "digest")


class _TwoGiB(int):
    """block_out[1] of a VAE whose widest activation claims 2 GiB per image: decode() then takes one image per launch sequence."""

    def __rmul__(self, other):
        return 1 << 31
    __mul__ = __rmul__


def _vae(b=1, chunked=False):
    def run(log, n, dtype):
        if chunked:
            bo = n.cfg["block_out"]
            n.cfg = dict(n.cfg, block_out=(bo[0], _TwoGiB(bo[1])) + tuple(bo[2:]))
        return n.decode(z(log, "z", (b, 4, 4, 8), dtype))
    return run


case("vae tiny bf16 decode", net_case("vae", TINY, BF16, _vae()), "digest")
case("vae tiny bf16 decode, three images in chunks of one", net_case("vae", TINY, BF16, _vae(3, True)), "digest")
case("vae tiny fp32 exact decode", net_case("vae", TINY, F32, _vae()), "digest")
case("vae tiny fp32 x3 decode", net_case("vae", TINY, F32, _vae(), net="tiny vae f32 x3", f32_gemm="x3"), "digest")
case("vae tiny fp32 x3 decode SASPA_X3_PRESPLIT=0", net_case("vae", TINY, F32, _vae(), net="tiny vae f32 x3 presplit=0", f32_gemm="x3"), "digest",
     env={"SASPA_X3_PRESPLIT": "0"})
case("vae tiny resnet with shortcut + mid attention",
     net_case("vae", TINY, BF16, lambda log, n, dt: [n.resnet("decoder.up_blocks.2.resnets.0", z(log, "x", (1, 8, 8, 64), dt)),
                                                     n.mid_attention(z(log, "h", (1, 4, 4, 64), dt))]), "digest")
case("vae_encoder tiny bf16 encode",
     net_case("vae_encoder", TINY, BF16, lambda log, n, dt: n.encode(z(log, "x", (1, 32, 32, 8), dt)), cfg=TINY["vae"]), "digest")


# ---- encoder stacks ---------------------------------------------------------------------------------------------------------------------
def _ids(log, b=2, n=77):
    return log.name((torch.arange(b * n, dtype=torch.int64).reshape(b, n) * 7) % 500, "ids")


def _text(kind, fam, **kw):
    def run(log, n, dtype):
        ctx = z(log, "subject", (2, 16, n.cfg["width"]), F32) if kw.pop("ctx", False) else None
        return n.forward(_ids(log, n=61 if ctx is not None else 77), ctx=ctx, **kw)
    return net_case(kind, fam, BF16, run)


case("clip text tiny forward", _text("text", TINY), "digest")
case("clip text tiny forward with ctx", _text("text", TINY, ctx=True), "digest")
case("clip text tiny_xl penultimate (no text_projection)", _text("text", TINY_XL, penultimate=True), "digest")
case("clip text2 tiny_xl penultimate + text_projection, gelu", _text("text2", TINY_XL, penultimate=True))
case("safety checker tiny similarity", net_case("safety", TINY, BF16, lambda log, n, dt: n.similarity(z(log, "pixels", (2, 56, 56, 8), dt))), "digest")
_QF = dict(TINY["qformer"], vis_eps=1e-6)                    # (the vision tower's eps is not LayerNorm's default)
case("blip2 qformer tiny forward",
     net_case("qformer", TINY, BF16, lambda log, n, dt: n.forward(z(log, "pixel_values", (2, 3, 56, 56), F32), np.arange(8).reshape(2, 4) % 500),
              net="tiny qformer vis_eps=1e-6 bf16", cfg=_QF), "digest")
case("clip rn50 visual tiny forward",
     net_case("clip_rn50", None, F32, lambda log, n, dt: n.forward(z(log, "pixels", (2, 64, 64, 8), dt)), net="tiny clip_rn50 f32",
              cfg=CFG.tiny_filters()["clip_rn50"]), "digest")
case("attention_core fp32 (unfused)",
     lambda log: models.attention_core(z(log, "q", (2, 16, 64), F32), z(log, "k", (2, 12, 64), F32), z(log, "vt", (2, 64, 16), F32), 2, 16, 12))
case("attention_core bf16 head dim 512 (unfused)",
     lambda log: models.attention_core(z(log, "q", (1, 16, 512), BF16), z(log, "k", (1, 16, 512), BF16), z(log, "vt", (1, 512, 16), BF16), 1, 16, 16,
                                       causal=True))
case("attention_core bf16 flash, prescaled row-major V",
     lambda log: models.attention_core(z(log, "q", (1, 16, 64), BF16), z(log, "k", (1, 16, 64), BF16), z(log, "v", (1, 16, 64), BF16), 2, 16, 16,
                                       prescaled=True, v_rowmajor=True))
RAISES = {
    "block bf16 level 0 cfg_pair, context of one sample": ("ValueError", "cfg_pair: 1 shared samples need a context of 2 samples, not 1"),
    "fp8 calibrated level 0 under capture": ("RuntimeError", f"fp8 feed-forward scale of {L0}.transformer_blocks.0 is not calibrated: "
                                                             "run one eager evaluation before capture"),
    "fp8 with fp16": ("ValueError", "fp8 projections quantise bf16 activations: fp8 together with fp16 compute is not supported"),
    "fp8_ff='block'": ("ValueError", "fp8_ff must be 'calibrated' or 'mx', not 'block'"),
    "unet tiny_xl bf16 prepare_timesteps without added": ("ValueError", "this network needs the SDXL added conditioning (text_embeds, time_ids)"),
    "unet tiny_xl bf16 encode cfg_pair refused": ("ValueError", "cfg_pair: the added conditioning gives the two halves different time embeddings (SDXL)"),
}


# ---- records, fixture ---------------------------------------------------------------------------------------------------------------------
_RUN = {}


def traces(only=None):
    """[(name, store, record)] of the corpus, normalised through JSON; every case runs once per process."""
    names = [n for n, _, _, _ in CASES]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    out = []
    for name, fn, store, opts in CASES:
        if only is None or name in only:
            if name not in _RUN:
                _RUN[name] = json.loads(json.dumps(run_case(fn, **opts)))
            out.append((name, store, _RUN[name]))
    return out


def stored(name, store, r):
    """A record as the fixture holds it (before the `lines` table)."""
    if store == "full" or "exc" in r:
        return dict({"case": name}, **{k: r[k] for k in ("exc", "ret", "calls") if k in r})
    return {"case": name, "chain": chain(r["calls"] + [["returns", r["ret"]]])}


ABBR = [p + s for p in (L0, L1, MID, "down_blocks.0.resnets.0", "down_blocks.1.resnets.0") for s in (".transformer_blocks.0.", ".")]


def _abbr(v, decode):
    """A string that starts with ABBR[i] is stored as `~i~rest`, and `, ` (shapes) as `,`."""
    if isinstance(v, str):
        if decode:
            v = v.replace(",", ", ")
            return ABBR[int(v[1:v.index("~", 1)])] + v[v.index("~", 1) + 1:] if v.startswith("~") else v
        assert "," not in v.replace(", ", "") and "~" not in v, v
        i = next((i for i, a in enumerate(ABBR) if v.startswith(a)), None)
        return (v if i is None else f"~{i}~{v[len(ABBR[i]):]}").replace(", ", ",")
    if isinstance(v, list):
        return [_abbr(e, decode) for e in v]
    return {k: _abbr(e, decode) for k, e in v.items()} if isinstance(v, dict) else v


def _delta(table, decode):
    """The table's compression, lossless: the arguments of a call are stored as their difference from an earlier call of the same op
    in the table (`-`: the names that went away) -- the one that leaves least, named by its index as a third element unless it is
    the previous one of that op --, names through `_abbr`."""
    seen, out = {}, []                                  # op -> [(table index, full arguments)]
    for i, line in enumerate(table):
        if not (len(line) in (2, 3) and isinstance(line[1], dict)):
            out.append(line)
            continue
        op, a = line[0], line[1]
        earlier = seen.setdefault(op, [])
        if decode:
            a = _abbr(a, True)
            base = {} if not earlier else dict(earlier)[line[2]] if len(line) == 3 else earlier[-1][1]
            full = {k: v for k, v in dict(base, **a).items() if k != "-" and k not in a.get("-", ())}
            out.append([op, full])
        else:
            full, best = a, None
            for j, base in reversed(earlier or [(None, {})]):
                gone = [k for k in base if k not in a]
                d = _abbr(dict({k: v for k, v in a.items() if k not in base or base[k] != v}, **({"-": gone} if gone else {})), False)
                enc = [op, d] if (not earlier or j == earlier[-1][0]) else [op, d, j]
                if best is None or len(json.dumps(enc)) < len(json.dumps(best)):
                    best = enc
            out.append(best)
        earlier.append((i, full))
    return out


def read_golden():
    with open(GOLDEN) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    lines = _delta(rows[0]["lines"], decode=True)
    return rows[1]["manifests"], [dict(r, calls=[lines[i] for i in r["calls"]]) if "calls" in r else r for r in rows[2:]]


def write_golden(manifests, rows):
    table, index, out = [], {}, []
    for r in rows:
        if "calls" in r:
            calls = []
            for c in r["calls"]:
                k = json.dumps(c, separators=(",", ":"))
                if k not in index:
                    index[k] = len(table)
                    table.append(c)
                calls.append(index[k])
            r = dict(r, calls=calls)
        out.append(r)
    assert _delta(json.loads(json.dumps(_delta(table, decode=False))), decode=True) == table
    with open(GOLDEN, "w") as f:
        for r in [{"lines": _delta(table, decode=False)}, {"manifests": manifests}] + out:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")


def _first_difference(got, want, calls, got_ret=None):
    for key in ("exc", "ret"):
        if got.get(key) != want.get(key):
            return f"{key}:\n    got  {got.get(key)}\n    want {want.get(key)}"
    if "chain" in want:
        g, w = got["chain"], want["chain"]
        i = next((i for i in range(min(g["n"], w["n"])) if g["digits"][i] != w["digits"][i]), min(g["n"], w["n"]))
        return f"{g['n'] - 1} calls, want {w['n'] - 1}; the first digest that differs is that of call {i}:\n    got  " + \
            str((calls + [["returns", got_ret]])[i] if i < g["n"] else None)
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        if g != w:
            return f"call {i}:\n    got  {g}\n    want {w}"
    return f"{len(got['calls'])} calls, want {len(want['calls'])}: " + \
        str((got["calls"] + [None])[len(want["calls"])] if len(got["calls"]) > len(want["calls"]) else want["calls"][len(got["calls"])])


def test_models_call_trace():
    """Every call the networks make into ops for the corpus -- arguments, order, exceptions, returned tensors -- is the recorded one."""
    assert os.path.getsize(GOLDEN) < 64 * 1024, "the fixture outgrew the 64 KB of the other two trace fixtures"
    _, want = read_golden()
    got = traces()
    assert [n for n, _, _ in got] == [w["case"] for w in want], "the corpus and the fixture list different cases"
    bad = [(n, stored(n, s, r), w, r) for (n, s, r), w in zip(got, want) if stored(n, s, r) != w]
    msg = "\n".join(f"case {n!r}: {_first_difference(g, w, r['calls'], r.get('ret'))}" for n, g, w, r in bad[:8])
    assert not bad, f"{len(bad)} of {len(want)} call traces changed:\n{msg}"


def test_parameter_manifests():
    """What every network of the corpus packed: per key of `p` shape, dtype, layout attributes, bytes and shared storage, and the
    routing state the tools read (blocks, tr_info, the fp8 / xattn / ff_block sets, ...)."""
    want, _ = read_golden()
    traces()
    assert sorted(MT.MANIFESTS) == sorted(want), "the corpus and the fixture build different networks"
    for name in sorted(want):
        g, w = MT.MANIFESTS[name], want[name]
        assert g["keys"] == w["keys"], f"{name}: the keys of p changed ({g['keys'][0]} keys, {w['keys'][0]} recorded)"
        bad = [i for i in range(w["keys"][0]) if g["params"][i] != w["params"][i]]
        assert not bad and g["sha256"] == w["sha256"], f"{name}: packed parameters changed" + \
            (f", the first is number {bad[0]} in sorted key order ({len(bad)} digits differ)" if bad else "")
        bad = [a for i, a in enumerate(MT.ROUTING) if g["routing"][4 * i:4 * i + 4] != w["routing"][4 * i:4 * i + 4]]
        assert not bad, f"{name}: routing state changed: {bad}"


def test_host_sums_by_value():
    """What packing forms by a host matmul or normalisation (the manifest holds no bytes of these: they follow the host's BLAS) against
    a float64 recomputation from the state dict, within what fp32 accumulation in any order can be off by: the v bias folded into the
    out bias of the three encoder stacks, the Q-Former's attentions and the VAE's mid attention, the safety checker's unit rows, CLIP
    RN50's projected position table.  The UNet's out biases are plain copies and are byte-hashed like everything else."""
    traces()
    errors = MT.HOST_SUM_ERRORS
    want = {"tiny text bf16": 2, "tiny_xl text2 bf16": 3, "tiny safety bf16": 3, "tiny qformer vis_eps=1e-6 bf16": 6, "tiny vae bf16": 1,
            "tiny vae_encoder bf16": 1, "tiny clip_rn50 f32": 3, "tiny unet bf16": 0, "w320 bf16": 0}
    assert {n: len(errors[n]) for n in want} == want
    bad = {(n, k): e for n, ks in errors.items() for k, e in ks.items() if not e <= 1.0}
    assert not bad, f"packed host sums off by more than their rounding bound (in units of the bound): {bad}"


def test_refusals_by_type_and_text():
    got = {n: r for n, _, r in traces()}
    assert {n for n, r in got.items() if "exc" in r} == set(RAISES)
    for name, exc in RAISES.items():
        assert tuple(got[name]["exc"]) == exc, (name, got[name]["exc"])


# ---- which form did a block take?  read off the recorded calls ------------------------------------------------------------------------------
def forms_seen(calls, t):
    """(attn1, attn2, ff) form names of block `t` as its first execution in `calls` shows them; attn2 "xattn_block" with the shared
    rows is "xattn_block shared"."""
    a1 = a2 = ff = None
    for op, a in ([c[0], c[1]] for c in calls if c[0].startswith("ops.") and len(c) > 1 and isinstance(c[1], dict)):
        w = str(a.get("w", a.get("wq", "")))
        if a1 is None:
            if op == "ops.linear_fp8" and w == t + ".attn1.qkv.w8":
                a1 = "fp8"
            elif op == "ops.linear" and "out_t" in a:
                a1 = "as_fused"
            elif op == "ops.linear" and w.startswith(t + ".attn1.qk.w+0["):
                a1 = "qkv_rowmajor"
            elif op == "ops.linear" and w == t + ".attn1.qk.w":
                a1 = "qk_vt"
        if a2 is None:
            if op == "ops.xattn_block" and str(a["w"]) == t + ".attn2.xw":
                a2 = "xattn_block shared" if "x_rows" in a else "xattn_block"
            elif op == "ops.linear_fp8" and w == t + ".attn2.q.w8":
                a2 = "fp8"
            elif op == "ops.linear" and w == t + ".attn2.q.w":
                a2 = "ln_fused" if "ln" in a else "plain"
        if ff is None:
            if op == "ops.ff_block":
                ff = "ff_block"
            elif op == "ops.linear" and w == t + ".ff.net.0.proj.w":
                ff = "ln_fused_geglu" if "ln" in a else ("geglu" if a.get("act") == ops.ACT_GEGLU else "geglu_unfused")
            elif op == "ops.linear_mxfp8":
                ff = "fp8_mx"
            elif op == "ops.linear_fp8" and w == t + ".ff.net.2.w8":
                ff = "fp8_calibrated"
            elif op == "ops.linear" and w == t + ".ff.net.2.w" and any(c[0] == "ops.linear_fp8" for c in calls):
                ff = "fp8_bf16_out"
    return a1, a2, ff


BLOCK_CASES = [(n, o) for n, _, _, o in CASES if n.startswith(("block ", "fp8 ")) and n not in RAISES]


def _block_of(name):
    return L1 if ("level 1" in name or "192" in name) else MID if " mid " in name else L0


def test_corpus_takes_its_branches():
    """The corpus is not vacuous: every form of the three halves of a transformer block occurs in the recorded calls, the resnets'
    arms and the encoders' variants show, and the cases that are meant to raise do."""
    got = {n: r for n, _, r in traces()}
    seen = [forms_seen(got[n]["calls"], _block_of(n) + ".transformer_blocks.0") for n, _ in BLOCK_CASES]
    assert {s[0] for s in seen} == {"fp8", "as_fused", "qkv_rowmajor", "qk_vt"}
    assert {s[1] for s in seen} == {"xattn_block", "xattn_block shared", "ln_fused", "plain", "fp8"}
    assert {s[2] for s in seen} == {"ff_block", "ln_fused_geglu", "geglu", "geglu_unfused", "fp8_bf16_out", "fp8_calibrated", "fp8_mx"}
    names = lambda n: [c[0] for c in got[n]["calls"]]  # noqa: E731
    two = got["fp8 calibrated level 0: calibration, then steady state"]
    amax = [i for i, c in enumerate(two["calls"]) if c[0] == "ops.linear_fp8" and "amax" in c[1]]
    assert len(amax) == 1 and amax[0] < len(two["calls"]) // 2 and two["ret"][-1] == {"calibrated": [L0 + ".transformer_blocks.0"]}
    assert "ops.dup_rows" in names("fp8 calibrated level 0 cfg_pair (dup_rows)")
    assert "ops.layernorm_quant_fp8" not in names("fp8 net, width 192 stays bf16")
    r = "resnet fp8_conv: "
    assert names(r + "both convs MX (16384 pixels, 320 -> 320)").count("ops.conv3x3_mxfp8") == 2
    assert got[r + "both convs MX (16384 pixels, 320 -> 320)"]["ret"][1] == ["down_blocks.0.resnets.0.conv1", "down_blocks.0.resnets.0.conv2"]
    one = names(r + "conv1 only (8192 pixels, 320 -> 960)")
    assert one.count("ops.conv3x3_mxfp8") == 1 and one.count("ops.groupnorm") == 1 and one.count("ops.conv") == 2
    two = got[r + "conv2 only (decoder concat, 960 + 320 -> 320)"]
    assert two["ret"][1] == ["up_blocks.1.resnets.0.conv2"] and not any("fuse_gn" in c[1] for c in two["calls"] if c[0] == "ops.conv")
    assert "ops.conv3x3_mxfp8" not in names(r + "neither (64 pixels)") and got[r + "neither (64 pixels)"]["ret"][1] == []
    assert any("fuse_gn" in c[1] for c in got["resnet bf16 no shortcut step=2"]["calls"] if c[0] == "ops.conv")
    assert not any("gn_unit" in c[1] for c in got["resnet f32 no shortcut step=2"]["calls"] if c[0] == "ops.conv")
    assert names("vae tiny bf16 decode, three images in chunks of one").count("ops.f32_gemm_mode enter") == 1
    assert names("vae tiny bf16 decode, three images in chunks of one").count("ops.conv") == 3 * names("vae tiny bf16 decode").count("ops.conv")
    assert ["ops.f32_gemm_mode enter", "x3"] in got["vae tiny fp32 x3 decode"]["calls"]
    assert names("unet tiny bf16 encode cfg_pair").count("ops.dup_rows") == 2
    assert names("unet tiny bf16, no attention at level 0: encode cfg_pair").count("ops.dup_rows") == 1
    assert any(c[0] == "ops.activation" and c[1]["act"] == ops.ACT_GELU for c in got["clip text2 tiny_xl penultimate + text_projection, gelu"]["calls"])
    assert any(c[0] == "ops.layernorm" and c[1].get("eps") == 1e-6 for c in got["blip2 qformer tiny forward"]["calls"])
    assert "ops.softmax_rows" in names("clip rn50 visual tiny forward") and "ops.softmax_rows" in names("attention_core bf16 head dim 512 (unfused)")


def test_which_names_the_forms_taken():
    """`_Net.which()` -- the form functions asked without launching -- names for every block case what the recorded calls show, and
    asks nothing of ops that the trace would see."""
    got = {n: r for n, _, r in traces()}
    for name, opts in BLOCK_CASES:
        fn = next(f for n, f, _, _ in CASES if n == name)
        r = run_case(fn.which, **opts)
        seen = [list(forms_seen(got[name]["calls"], f"{_block_of(name)}.transformer_blocks.{d}")) for d in range(len(r["ret"]))]
        assert r["ret"] == seen and len(seen) == (2 if "two blocks" in name else 1), (name, r["ret"], seen)
        assert all(c[0] in ("ops.linear_ln_fusable", "ops.ff_block_eligible") for c in r["calls"]), (name, r["calls"])


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write-golden"]:
        only = set(sys.argv[2:])
        fresh = [stored(*t) for t in traces(only or None)]
        manifests = dict(MT.MANIFESTS)
        if only:
            assert only == {r["case"] for r in fresh}, only - {r["case"] for r in fresh}
            old_m, old = read_golden()
            fresh = {r["case"]: r for r in fresh}
            fresh, manifests = [fresh.get(w["case"], w) for w in old], dict(old_m, **manifests)
        write_golden(manifests, fresh)
        print(f"{GOLDEN}: {len(fresh)} cases, {len(manifests)} networks, {os.path.getsize(GOLDEN)} bytes")
    elif sys.argv[1:2] == ["--show"]:
        for name, _, r in traces(set(sys.argv[2:]) or None):
            print(name, r.get("exc") or r.get("ret"))
            for c in r["calls"]:
                print("   ", json.dumps(c))
