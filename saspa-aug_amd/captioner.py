"""BLIP captioner on the gfx950 kernels: the model behind PROMPT_TYPE = "captions" (prompts_engineering/blip_utils.py:28-58 of the
reference: LAVIS `blip_caption` / `base_coco`, `generate()` on every original image).

ViT-B/16 vision tower (models.encoder_layer) -> per decoder layer the cross-attention K / V of the image tokens, once per image -> a
BERT decoder run one token at a time against key/value caches (ops.decode_attn) -> LM head with fp32 logits -> one beam-search
step's selection on the device (ops.logprob_topk).  Launch graph only: every matmul / norm / attention / activation / selection is a
C-ABI kernel of libsaspa_hip.so; the torch calls below are views, copies, concatenations and gathers (data movement).  The beam
bookkeeping is host Python on the 2 * beams (score, row, token) triples per image that one small device-to-host copy brings per step;
it restates transformers' `_beam_search` / `_sample` (length_penalty 1, no early stopping, one EOS id), which tests/caption_ref.py pins.

Architecture values and the LAVIS checkpoint key names are RECALLED, not verified (config.BLIP_CAPTION, weights.blip_caption_from_lavis):
no checkpoint or vocabulary could be read when this was written."""
import os

import numpy as np
import torch

from . import config as CFG
from . import imageproc
from . import ops
from . import tokenizer as T
from . import weights as W
from .models import _Packed, _f32, _norm, _wb, encoder_layer

V = "vision_model"
B_ = "text_decoder.bert"
C_ = "text_decoder.cls.predictions"
DEAD = -1.0e9                 # transformers' score of a beam that must not be continued


def synthetic_weights_allowed():
    """Captions of a random model are noise: without a checkpoint the captioner refuses unless SASPA_SYNTHETIC_CAPTIONER=1 (the rule of
    the filter stage)."""
    return os.environ.get("SASPA_SYNTHETIC_CAPTIONER", "0") == "1"


def load_state_dict(weights_dir):
    """The captioner's state dict from a directory, in either key layout (transformers: vision_model.* / text_decoder.*; LAVIS:
    visual_encoder.* / text_decoder.*, recalled and unverified)."""
    for name in ("model.safetensors", "pytorch_model.bin", "model_base_caption_capfilt_large.pth"):
        path = os.path.join(weights_dir, name)
        if os.path.exists(path):
            break
    else:
        pth = sorted(f for f in os.listdir(weights_dir) if f.endswith((".pth", ".bin", ".safetensors")))
        if not pth:
            raise FileNotFoundError(f"no BLIP caption checkpoint (*.safetensors / *.bin / *.pth) under {weights_dir}")
        path = os.path.join(weights_dir, pth[0])
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    sd = sd.get("model", sd)
    if any(k.startswith("visual_encoder.") for k in sd):
        return W.blip_caption_from_lavis(sd)
    return W.blip_caption_from_transformers(sd)


class BlipCaptioner:
    def __init__(self, sd, cfg, dev, dtype, tokenizer=None):
        self.cfg, self.dev, self.dtype = cfg, torch.device(dev), dtype
        self.tok = tokenizer if tokenizer is not None else T.BertHashTokenizer(cfg["vocab"])
        pk = _Packed(sd, self.dev, dtype)
        p = self.p = pk.p
        vw, w = cfg["vis_width"], cfg["width"]
        p["patch.w"] = W.pack_linear(sd[V + ".embeddings.patch_embedding.weight"].reshape(vw, -1)).to(self.dev, dtype)
        p["patch.b"] = _f32(sd[V + ".embeddings.patch_embedding.bias"], self.dev)
        pos = sd[V + ".embeddings.position_embedding"][0]
        p["cls_pos"] = (sd[V + ".embeddings.class_embedding"][0, 0] + pos[0]).to(self.dev, dtype).reshape(1, 1, vw).contiguous()
        p["patch_pos"] = pos[1:].to(self.dev, dtype).contiguous()
        for i in range(cfg["vis_layers"]):
            lp = f"{V}.encoder.layers.{i}"
            pk.encoder_layer(lp, lp + ".self_attn", "projection", qkv="qkv")
        pk.norm(V + ".post_layernorm")
        p["word"] = sd[B_ + ".embeddings.word_embeddings.weight"].to(self.dev, dtype).contiguous()
        p["tpos"] = sd[B_ + ".embeddings.position_embeddings.weight"].to(self.dev, dtype).contiguous()
        pk.norm(B_ + ".embeddings.LayerNorm")
        for i in range(cfg["layers"]):
            lp = f"{B_}.encoder.layer.{i}"
            a = lp + ".attention"
            p[a + ".qkv.w"] = torch.cat([sd[f"{a}.self.{n}.weight"] for n in ("query", "key", "value")], 0).contiguous().to(self.dev, dtype)
            p[a + ".qkv.b"] = _f32(torch.cat([sd[f"{a}.self.{n}.bias"] for n in ("query", "key", "value")]), self.dev)
            c = lp + ".crossattention"
            pk.linear(c + ".self.query")
            p[c + ".kv.w"] = W.pack_linear(torch.cat([sd[c + ".self.key.weight"], sd[c + ".self.value.weight"]], 0)).to(self.dev, dtype)
            p[c + ".kv.b"] = _f32(torch.cat([sd[c + ".self.key.bias"], sd[c + ".self.value.bias"]]), self.dev)
            for n in (a, c):
                pk.linear(n + ".output.dense")
                pk.norm(n + ".output.LayerNorm")
            pk.linear(lp + ".intermediate.dense")
            pk.linear(lp + ".output.dense")
            pk.norm(lp + ".output.LayerNorm")
        pk.linear(C_ + ".transform.dense")
        pk.norm(C_ + ".transform.LayerNorm")
        # fp32 logits out: the vocabulary projection runs as an fp32 GEMM on the storage-rounded weights (its N = vocab is padded to a
        # multiple of 8 columns by ops.linear; saspa_logprob_topk never reads the pad into a sum)
        p["lm.w"] = sd[C_ + ".decoder.weight"].to(dtype).to(self.dev, torch.float32).contiguous()
        p["lm.b"] = _f32(sd[C_ + ".decoder.bias"], self.dev)
        pk.sd = None
        self.ntok = (cfg["image_size"] // cfg["patch"]) ** 2 + 1

    @classmethod
    def from_synthetic(cls, cfg=None, dev="cuda:0", dtype=torch.bfloat16, seed=0):
        if not synthetic_weights_allowed():
            raise RuntimeError("BlipCaptioner: no checkpoint given and SASPA_SYNTHETIC_CAPTIONER is not 1 -- captions of a random model "
                               "are noise; set SASPA_SYNTHETIC_CAPTIONER=1 to run with synthetic weights on purpose")
        cfg = CFG.BLIP_CAPTION if cfg is None else cfg
        return cls(W.synth_state_dict("blip_caption", cfg, seed), cfg, dev, dtype)

    @classmethod
    def from_pretrained(cls, weights_dir, dev="cuda:0", dtype=torch.bfloat16, cfg=None):
        cfg = CFG.BLIP_CAPTION if cfg is None else cfg
        vocab = os.path.join(weights_dir, "vocab.txt")
        if not os.path.exists(vocab):
            raise FileNotFoundError(f"{vocab} not found: the captioner decodes with the checkpoint's bert-base-uncased vocabulary")
        return cls(load_state_dict(weights_dir), cfg, dev, dtype, tokenizer=T.BertWordPieceTokenizer(vocab))

    # ---- image side --------------------------------------------------------------------------------------------------------------
    def preprocess(self, images_u8):
        """LAVIS blip_image_eval: Resize((S, S), bicubic) of the PIL image (Pillow-exact on u8, on the device), /255, normalise with
        the CLIP mean / std.  images_u8: u8 [n,H,W,3] (tensor / array) or a list of [H,W,3] of any sizes -> [n,S,S,8] activations."""
        s = self.cfg["image_size"]
        if isinstance(images_u8, (list, tuple)):
            batch = [ops.h2d(torch.from_numpy(np.array(im, dtype=np.uint8)), self.dev)[None] for im in images_u8]
            x = torch.cat([imageproc.resize_bicubic_u8(im.contiguous(), s, s) for im in batch], 0)
        else:
            x = ops.h2d(torch.as_tensor(images_u8), self.dev)
            x = imageproc.resize_bicubic_u8((x[None] if x.dim() == 3 else x).contiguous(), s, s)
        return imageproc.normalize_u8(x, self.dtype, CFG.BLIP_IMAGE_MEAN, CFG.BLIP_IMAGE_STD)

    def vision(self, act):
        """[n,S,S,>=3] channels-last normalised activations -> image tokens [n, 1 + (S/P)^2, vis_width]."""
        cfg, p = self.cfg, self.p
        n, s = act.shape[0], act.shape[1]
        ps, vw = cfg["patch"], cfg["vis_width"]
        g = s // ps
        patches = act[..., :3].reshape(n, g, ps, g, ps, 3).permute(0, 1, 3, 5, 2, 4).reshape(n * g * g, 3 * ps * ps)
        kpad = p["patch.w"].shape[1] - patches.shape[1]
        if kpad:
            patches = torch.nn.functional.pad(patches, (0, kpad))
        pos = p["patch_pos"][None].expand(n, -1, -1).reshape(n * g * g, vw).contiguous()
        tok = ops.linear(patches.contiguous(), p["patch.w"], p["patch.b"], residual=pos).view(n, g * g, vw)
        x = torch.cat([p["cls_pos"].expand(n, -1, -1), tok], 1).contiguous()
        for i in range(cfg["vis_layers"]):
            lp = f"{V}.encoder.layers.{i}"
            x = encoder_layer(p, lp, lp + ".self_attn", x, cfg["vis_heads"], ops.ACT_GELU, eps=cfg["vis_eps"])
        return ops.layernorm(x, *_norm(p, V + ".post_layernorm", cfg["vis_eps"]))

    def vision_from_pixels(self, pixel_values):
        """[n,3,S,S] normalised floats (the layout of the CPU reference) -> image tokens."""
        return self.vision(ops.h2d(pixel_values, self.dev, self.dtype).permute(0, 2, 3, 1).contiguous())

    def cross_kv(self, image_tokens):
        """Per decoder layer the cross-attention K | V of the image tokens, [n, ntok, 2 * width]: computed once per image."""
        return [ops.linear(image_tokens, *_wb(self.p, f"{B_}.encoder.layer.{i}.crossattention.kv")) for i in range(self.cfg["layers"])]

    # ---- text side ---------------------------------------------------------------------------------------------------------------
    def new_cache(self, rows, length):
        w = self.cfg["width"]
        return torch.zeros((2, self.cfg["layers"], rows, length, w), device=self.dev, dtype=self.dtype)

    def step(self, tokens, t, cache, ckv, group):
        """One decoder position: tokens (device int [rows]) at position t against the self cache [2, L, rows, T, w] (k, v of position t
        are appended) and the images' cross K | V (`group` rows per image) -> fp32 logits [rows, round8(vocab)]."""
        cfg, p = self.cfg, self.p
        w, h, eps = cfg["width"], cfg["heads"], cfg["eps"]
        scale = (w // h) ** -0.5
        x = ops.embed_tokens(tokens, p["word"], p["tpos"][t:t + 1], 1)
        x = ops.layernorm(x, *_norm(p, B_ + ".embeddings.LayerNorm", eps))
        for i in range(cfg["layers"]):
            lp = f"{B_}.encoder.layer.{i}"
            a, c = lp + ".attention", lp + ".crossattention"
            qkv = ops.linear(x, *_wb(p, a + ".qkv"))
            cache[0, i, :, t].copy_(qkv[:, w:2 * w])
            cache[1, i, :, t].copy_(qkv[:, 2 * w:3 * w])
            o = ops.decode_attn(qkv[:, :w], cache[0, i], cache[1, i], h, t + 1, scale, group=1)
            x = ops.layernorm(ops.linear(o, *_wb(p, a + ".output.dense"), residual=x), *_norm(p, a + ".output.LayerNorm", eps))
            q = ops.linear(x, *_wb(p, c + ".self.query"))
            o = ops.decode_attn(q, ckv[i][:, :, :w], ckv[i][:, :, w:2 * w], h, self.ntok, scale, group=group)
            x = ops.layernorm(ops.linear(o, *_wb(p, c + ".output.dense"), residual=x), *_norm(p, c + ".output.LayerNorm", eps))
            f = ops.activation(ops.linear(x, *_wb(p, lp + ".intermediate.dense")), ops.ACT_GELU)
            x = ops.layernorm(ops.linear(f, *_wb(p, lp + ".output.dense"), residual=x), *_norm(p, lp + ".output.LayerNorm", eps))
        hdn = ops.activation(ops.linear(x, *_wb(p, C_ + ".transform.dense")), ops.ACT_GELU)
        hdn = ops.layernorm(hdn, *_norm(p, C_ + ".transform.LayerNorm", eps))
        return ops.linear(hdn.float(), p["lm.w"], p["lm.b"])

    @torch.no_grad()
    def teacher_forced_logits(self, image_tokens, ids):
        """Logits fp32 [n, T, vocab] of the decoder fed ids [n, T], one position at a time through the caches (tests)."""
        ids = torch.as_tensor(np.asarray(ids))
        n, tt = ids.shape
        ckv, cache = self.cross_kv(image_tokens), self.new_cache(n, tt)
        dev_ids = ops.h2d(ids, self.dev)
        out = [self.step(dev_ids[:, t].contiguous(), t, cache, ckv, 1)[:, :self.cfg["vocab"]] for t in range(tt)]
        return torch.stack(out, 1)

    def prompt_ids(self, prompt=None):
        """The prompt as generate() feeds it: tokenised, token 0 replaced by BOS, the last token (SEP) dropped."""
        ids = [int(i) for i in self.tok(self.cfg["prompt"] if prompt is None else prompt)[0]]
        ids[0] = self.cfg["bos"]
        return ids[:-1]

    @torch.no_grad()
    def generate(self, images_u8=None, *, num_beams=None, max_length=None, min_length=None, prompt=None, image_tokens=None,
                 use_nucleus_sampling=False, num_captions=1):
        """Token ids int64 [n, L] (numpy), prompt included, as transformers' generate lays them out: rows shorter than the longest are
        filled (EOS after a beam search, PAD after a greedy one)."""
        if use_nucleus_sampling:
            raise NotImplementedError("nucleus sampling is not built: greedy and beam search only")
        if num_captions != 1:
            raise NotImplementedError("num_captions > 1 is not built")
        cfg = self.cfg
        nb = cfg["num_beams"] if num_beams is None else int(num_beams)
        max_length = cfg["max_length"] if max_length is None else int(max_length)
        min_length = cfg["min_length"] if min_length is None else int(min_length)
        if not 1 <= nb <= 8:
            raise ValueError("num_beams must be 1 .. 8")
        prompt = self.prompt_ids(prompt) if prompt is None or isinstance(prompt, str) else [int(i) for i in prompt]
        p0 = len(prompt)
        if not p0 < max_length <= cfg["max_pos"]:
            raise ValueError(f"max_length {max_length} must exceed the prompt's {p0} tokens and fit the {cfg['max_pos']} positions")
        if image_tokens is None:
            image_tokens = self.vision(self.preprocess(images_u8))
        n = image_tokens.shape[0]
        ckv = self.cross_kv(image_tokens)
        vocab, eos, pad = cfg["vocab"], cfg["eos"], cfg["pad"]

        # the prompt, one position at a time, one row per image; then the cache is replicated to the beams
        cache = self.new_cache(n, max_length)
        for t in range(p0):
            logits = self.step(torch.full((n,), prompt[t], device=self.dev, dtype=torch.int32), t, cache, ckv, 1)
        if nb > 1:
            cache = cache.repeat_interleave(nb, 2)
            logits = logits.repeat_interleave(nb, 0)
        rows = n * nb
        k = 2 * nb
        run_seq = [[list(prompt) for _ in range(nb)] for _ in range(n)]
        run_score = [[0.0] + [DEAD] * (nb - 1) for _ in range(n)]
        fin = [[] for _ in range(n)]                          # per image: finished hypotheses (score, tokens), best first, <= nb
        unsat = [True] * n                                    # transformers' is_early_stop_heuristic_unsatisfied
        open_ = [True] * n                                    # greedy: the row has not met EOS
        cur = p0
        while True:
            scores = torch.tensor([0.0 if nb == 1 else (s if s > DEAD / 10 else float("-inf")) for img in run_score for s in img],
                                  dtype=torch.float32)
            _, _, buf = ops.logprob_topk(logits, vocab, nb, ops.h2d(scores, self.dev), eos, cur < min_length)
            sel = buf.cpu().numpy()                           # the step's one device-to-host copy: [3, n, k]
            sel_score, sel_row, sel_tok = sel[0].view(np.float32), sel[1:].reshape(n, k, 2)[:, :, 0], sel[1:].reshape(n, k, 2)[:, :, 1]
            at_max = cur + 1 >= max_length
            if nb == 1:                                       # GenerationMixin._sample without sampling
                nxt = [int(sel_tok[i, 0]) if open_[i] else pad for i in range(n)]
                for i in range(n):
                    run_seq[i][0].append(nxt[i])
                    open_[i] = open_[i] and not (nxt[i] == eos or at_max)
                cur += 1
                if not any(open_):
                    return np.asarray([r[0] for r in run_seq], np.int64)
                src = list(range(n))
            else:                                             # GenerationMixin._beam_search
                nxt, src, all_hit = [], [], True
                for i in range(n):
                    cand = [(float(sel_score[i, j]), int(sel_row[i, j]), int(sel_tok[i, j])) for j in range(k)]
                    hits = [tok == eos or at_max for _, _, tok in cand]
                    all_hit = all_hit and all(hits)
                    seqs = [run_seq[i][r] + [tok] for _, r, tok in cand]
                    run_lp = [s + (DEAD if hit else 0.0) for (s, _, _), hit in zip(cand, hits)]
                    keep = sorted(range(k), key=lambda j: -run_lp[j])[:nb]            # stable: ties keep the candidates' order
                    if unsat[i]:
                        merged = fin[i] + [(cand[j][0] / (cur + 1 - p0), seqs[j]) for j in range(nb) if hits[j]]
                        fin[i] = sorted(merged, key=lambda e: -e[0])[:nb]
                    run_seq[i] = [seqs[j] for j in keep]
                    run_score[i] = [run_lp[j] for j in keep]
                    nxt += [cand[j][2] for j in keep]
                    src += [i * nb + cand[j][1] for j in keep]
                cur += 1
                for i in range(n):
                    worst = min(e[0] for e in fin[i]) if len(fin[i]) == nb else DEAD
                    unsat[i] = unsat[i] and run_score[i][0] / (cur - p0) > worst
                if not any(unsat) or all_hit:
                    length = max(len(fin[i][0][1]) for i in range(n))
                    fill = pad or eos
                    return np.asarray([fin[i][0][1] + [fill] * (length - len(fin[i][0][1])) for i in range(n)], np.int64)
                if src != list(range(rows)):                  # the self caches follow their beams: an out-of-place gather
                    cache = cache.index_select(2, ops.h2d(torch.tensor(src, dtype=torch.int64), self.dev))
            logits = self.step(ops.h2d(torch.tensor(nxt, dtype=torch.int32), self.dev), cur - 1, cache, ckv, nb)

    def decode(self, ids, prompt=None):
        """ids of one image -> caption: special tokens skipped, the prompt stripped as LAVIS does (`output[len(prompt):]`).  The hash
        stand-in has no text to strip a prompt from: its placeholder words of the generated tokens only."""
        prompt = self.cfg["prompt"] if prompt is None else prompt
        if isinstance(self.tok, T.BertWordPieceTokenizer):
            return self.tok.decode(ids, skip_special_tokens=True)[len(prompt):]
        return self.tok.decode(list(ids)[len(self.prompt_ids(prompt)):], skip_special_tokens=True)

    def caption(self, images_u8, **kw):
        """One caption per image (LAVIS BlipCaption.generate defaults: beam search, 3 beams, max_length 30, min_length 10)."""
        return [self.decode(row, kw.get("prompt")) for row in self.generate(images_u8, **kw)]
