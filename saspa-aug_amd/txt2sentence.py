"""T5 key-to-text generator on the gfx950 kernels: the model behind PROMPT_TYPE = "txt2sentence" (prompts_engineering/
txt2sentance_prompts.py of the reference: keytotext's pipeline around mrm8488/t5-base-finetuned-common_gen, one `do_sample=True` call
per sentence).

T5 v1.0 encoder-decoder: token embeddings -> encoder blocks (RMS norm, self-attention with a bidirectional relative-position bias,
ReLU feed-forward) -> per decoder layer the cross-attention K | V of the encoder output, once per distinct input -> a decoder run one
token at a time against key/value caches (causal relative-position bias; bias-free cross-attention through ops.decode_attn) -> tied LM
head with fp32 logits -> one sampling step on the device (ops.sample_topk: temperature, top-k, top-p, inverse-CDF draw on a supplied
uniform).  Launch graph only: every matmul / norm / attention / selection is a C-ABI kernel of libsaspa_hip.so (csrc/saspa_t5.hip for the
three T5 lacks elsewhere); the torch calls below are views, copies and gathers.  The bucket function of the relative positions runs on
the host, once per model, into the two tables the attention kernel indexes.

PINNED against transformers (tests/test_t5_host.py): the model, the bucket function, the warpers' kept set and probabilities, the
tokenizer.  RECALLED, unverified (config.T5_COMMON_GEN): the keytotext wrapper's input formatting and that its kwargs bypass its
beam-search defaults.  It does not reproduce torch.multinomial's random stream: draws are inverse-CDF on uniforms of its own."""
import json
import math
import os

import numpy as np
import torch

from . import config as CFG
from . import ops
from . import tokenizer as T
from . import weights as W
from .models import _f32

ENC, DEC = "encoder", "decoder"
GROUP_MAX = 8                 # SASPA_DECODE_MAX_GROUP: rows that share one entry of the cross K / V


def synthetic_weights_allowed():
    """Sentences of a random model are noise: without a checkpoint the generator refuses unless SASPA_SYNTHETIC_T5=1 (the rule of the
    captioner and the filter stage)."""
    return os.environ.get("SASPA_SYNTHETIC_T5", "0") == "1"


def relative_bucket(distance, bidirectional, num_buckets, max_distance):
    """transformers' T5Attention._relative_position_bucket on int64 `distance` = memory position - query position, with the same
    float32 operations (log of the float ratio, division by the host-double log, product, truncation)."""
    rp = torch.as_tensor(distance, dtype=torch.long)
    buckets = torch.zeros_like(rp)
    if bidirectional:
        num_buckets //= 2
        buckets = buckets + (rp > 0).to(torch.long) * num_buckets
        rp = torch.abs(rp)
    else:
        rp = -torch.min(rp, torch.zeros_like(rp))
    max_exact = num_buckets // 2
    is_small = rp < max_exact
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rp, large)


def bias_table(weight, bidirectional, num_buckets, max_distance):
    """The relative-position table of one stack for ops.attn_relbias: weight [buckets, heads] (block 0's relative_attention_bias) ->
    (fp32 [heads, ncol], center) with table[h][c] the bias of key j for a query at pos where c = pos - j + center.  Bidirectional:
    2 * max_distance + 1 columns, center = max_distance; causal: max_distance + 1 columns (distances 0 .. max_distance), center 0.
    Buckets saturate at max_distance, so the kernel's clamp makes the table exact at any length."""
    center = max_distance if bidirectional else 0
    ncol = 2 * max_distance + 1 if bidirectional else max_distance + 1
    rel = center - torch.arange(ncol)                                   # memory - query = -(pos - j)
    idx = relative_bucket(rel, bidirectional, num_buckets, max_distance)
    return weight.float()[idx].t().contiguous(), center


def load_state_dict(weights_dir, cfg):
    for name in ("model.safetensors", "pytorch_model.bin"):
        path = os.path.join(weights_dir, name)
        if os.path.exists(path):
            break
    else:
        raise FileNotFoundError(f"no T5 checkpoint (model.safetensors / pytorch_model.bin) under {weights_dir}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    return W.t5_from_hf(sd, cfg)


def config_from_hf(path, base=None):
    """config.json of a T5 checkpoint -> this module's config (the generation fields of `base` kept).  Anything but the v1.0
    feed-forward (ReLU, not gated) is refused."""
    with open(path) as f:
        c = json.load(f)
    if c.get("feed_forward_proj", "relu") != "relu":
        raise NotImplementedError(f"feed_forward_proj = {c['feed_forward_proj']!r}: only T5 v1.0's ReLU feed-forward is built")
    base = CFG.T5_COMMON_GEN if base is None else base
    return dict(base, d_model=c["d_model"], enc_layers=c["num_layers"], dec_layers=c.get("num_decoder_layers", c["num_layers"]),
                heads=c["num_heads"], d_kv=c["d_kv"], d_ff=c["d_ff"], vocab=c["vocab_size"],
                buckets=c.get("relative_attention_num_buckets", 32), max_distance=c.get("relative_attention_max_distance", 128),
                eps=c.get("layer_norm_epsilon", 1e-6), tie_embeddings=c.get("tie_word_embeddings", True), pad=c.get("pad_token_id", 0),
                decoder_start=c.get("decoder_start_token_id", 0), eos=c.get("eos_token_id", 1))


class T5Generator:
    def __init__(self, sd, cfg, dev, dtype, tokenizer=None):
        if dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("T5Generator runs in bf16 or fp32 (the fp16 library has no T5 kernels)")
        self.cfg, self.dev, self.dtype = cfg, torch.device(dev), dtype
        self.tok = tokenizer if tokenizer is not None else T.UnigramTokenizer(vocab_size=cfg["vocab"], eos=cfg["eos"], pad=cfg["pad"])
        self.inner = cfg["heads"] * cfg["d_kv"]
        p = self.p = {}

        def lin(*names):
            return W.pack_linear(torch.cat([sd[n + ".weight"] for n in names], 0)).to(self.dev, dtype)

        p["shared"] = sd["shared.weight"].to(self.dev, dtype).contiguous()
        for stack, layers in ((ENC, cfg["enc_layers"]), (DEC, cfg["dec_layers"])):
            for i in range(layers):
                b = f"{stack}.block.{i}.layer"
                a = f"{b}.0.SelfAttention"
                p[a + ".qkv"] = lin(a + ".q", a + ".k", a + ".v")
                p[a + ".o"] = lin(a + ".o")
                p[f"{b}.0.ln"] = _f32(sd[f"{b}.0.layer_norm.weight"], self.dev)
                j = 1
                if stack == DEC:
                    c = f"{b}.1.EncDecAttention"
                    p[c + ".q"], p[c + ".kv"], p[c + ".o"] = lin(c + ".q"), lin(c + ".k", c + ".v"), lin(c + ".o")
                    p[f"{b}.1.ln"] = _f32(sd[f"{b}.1.layer_norm.weight"], self.dev)
                    j = 2
                p[f"{b}.{j}.wi"], p[f"{b}.{j}.wo"] = lin(f"{b}.{j}.DenseReluDense.wi"), lin(f"{b}.{j}.DenseReluDense.wo")
                p[f"{b}.{j}.ln"] = _f32(sd[f"{b}.{j}.layer_norm.weight"], self.dev)
            p[stack + ".final"] = _f32(sd[stack + ".final_layer_norm.weight"], self.dev)
            # the relative-position bias: block 0's table, shared by every layer of its stack
            tab, center = bias_table(sd[f"{stack}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], stack == ENC,
                                     cfg["buckets"], cfg["max_distance"])
            p[stack + ".bias"], p[stack + ".center"] = tab.to(self.dev), center
        # fp32 logits out: the vocabulary projection runs as an fp32 GEMM on the storage-rounded weights; the tied head's
        # d_model ** -0.5 rides in the GEMM's alpha
        head = sd["shared.weight"] if cfg["tie_embeddings"] else sd["lm_head.weight"]
        p["lm"] = head.to(dtype).to(self.dev, torch.float32).contiguous()
        self.lm_alpha = cfg["d_model"] ** -0.5 if cfg["tie_embeddings"] else 1.0

    @classmethod
    def from_synthetic(cls, cfg=None, dev="cuda:0", dtype=torch.bfloat16, seed=0):
        if not synthetic_weights_allowed():
            raise RuntimeError("T5Generator: no checkpoint given and SASPA_SYNTHETIC_T5 is not 1 -- sentences of a random model are "
                               "noise; set SASPA_SYNTHETIC_T5=1 to run with synthetic weights on purpose")
        cfg = CFG.T5_COMMON_GEN if cfg is None else cfg
        return cls(W.t5_synth_state_dict(cfg, seed), cfg, dev, dtype)

    @classmethod
    def from_pretrained(cls, weights_dir, dev="cuda:0", dtype=torch.bfloat16):
        if not weights_dir or not os.path.isdir(weights_dir):
            raise FileNotFoundError(f"T5 checkpoint directory {weights_dir!r} not found")
        cfg = config_from_hf(os.path.join(weights_dir, "config.json"))
        tj = os.path.join(weights_dir, "tokenizer.json")
        if not os.path.exists(tj):
            raise FileNotFoundError(f"{tj} not found: the generator tokenises with the checkpoint's Unigram vocabulary")
        return cls(load_state_dict(weights_dir, cfg), cfg, dev, dtype, tokenizer=T.UnigramTokenizer(tj, eos=cfg["eos"], pad=cfg["pad"]))

    # ---- encoder -----------------------------------------------------------------------------------------------------------------
    def _check_input(self, ids, lens):
        ids = torch.as_tensor(np.asarray(ids)).long()
        lens = torch.as_tensor(np.asarray(lens)).long()
        if ids.dim() != 2 or lens.shape != (ids.shape[0],) or int(lens.min()) < 1 or int(lens.max()) > ids.shape[1]:
            raise ValueError("ids must be [n, L] padded token ids and lens [n] with 1 <= lens <= L")
        if ids.shape[1] > self.cfg["max_input"]:
            raise ValueError(f"input of {ids.shape[1]} tokens exceeds the encoder cap of {self.cfg['max_input']} (config max_input)")
        return ids, lens

    def _ff(self, x, b):
        p = self.p
        h = ops.rmsnorm(x, p[b + ".ln"], self.cfg["eps"])
        return ops.linear(ops.linear(h, p[b + ".wi"], None, act=ops.ACT_RELU), p[b + ".wo"], None, residual=x)

    @torch.no_grad()
    def encode(self, ids, lens):
        """Padded token ids [n, L] with lengths [n] -> encoder output [n, L, d_model] (rows at or beyond a sequence's length hold
        finite values nobody reads: every consumer masks by length)."""
        cfg, p, inner = self.cfg, self.p, self.inner
        ids, lens = self._check_input(ids, lens)
        n, ll = ids.shape
        x = p["shared"].index_select(0, ops.h2d(ids.reshape(-1), self.dev))
        pos = ops.h2d(torch.arange(ll, dtype=torch.int32).repeat(n), self.dev)
        rlen = ops.h2d(lens.to(torch.int32).repeat_interleave(ll), self.dev)
        for i in range(cfg["enc_layers"]):
            b = f"{ENC}.block.{i}.layer"
            a = f"{b}.0.SelfAttention"
            qkv = ops.linear(ops.rmsnorm(x, p[f"{b}.0.ln"], cfg["eps"]), p[a + ".qkv"], None)
            kv = qkv.view(n, ll, 3 * inner)
            o = ops.attn_relbias(qkv[:, :inner], kv[:, :, inner:2 * inner], kv[:, :, 2 * inner:], cfg["heads"], ll, 1.0, pos,
                                 p[ENC + ".bias"], p[ENC + ".center"], rows_per_entry=ll, lens=rlen)
            x = ops.linear(o, p[a + ".o"], None, residual=x)
            x = self._ff(x, f"{b}.1")
        return ops.rmsnorm(x, p[ENC + ".final"], cfg["eps"]).view(n, ll, cfg["d_model"])

    def cross_kv(self, enc_out, lens, entry_of=None, group=1):
        """Per decoder layer the cross-attention K | V of the encoder output, computed once per distinct input: [entries, L, 2 * inner].
        entry_of (optional): for every cache entry the input it replicates (inputs sampled more than `group` <= 8 times take several
        entries); lens [n] are the inputs' lengths.  -> the `ckv` operand of step()."""
        lens = torch.as_tensor(np.asarray(lens)).to(torch.int32)
        kv = [ops.linear(enc_out, self.p[f"{DEC}.block.{i}.layer.1.EncDecAttention.kv"], None) for i in range(self.cfg["dec_layers"])]
        if entry_of is not None:
            sel = torch.as_tensor(entry_of, dtype=torch.int64)
            lens = lens[sel]
            sel = ops.h2d(sel, self.dev)
            kv = [t.index_select(0, sel) for t in kv]
        if not 1 <= group <= GROUP_MAX:
            raise ValueError(f"group must be 1 .. {GROUP_MAX}")
        return dict(kv=kv, group=int(group), nk=enc_out.shape[1], lens=ops.h2d(lens.repeat_interleave(group), self.dev))

    # ---- decoder -----------------------------------------------------------------------------------------------------------------
    def new_cache(self, rows, length):
        return torch.zeros((2, self.cfg["dec_layers"], rows, length, self.inner), device=self.dev, dtype=self.dtype)

    def step(self, tokens, t, cache, ckv):
        """One decoder position: tokens (device int [rows]) at position t against the self cache [2, layers, rows, T, inner] (k, v of
        position t are appended) and the inputs' cross K | V (ckv["group"] rows per entry) -> fp32 logits [rows, round8(vocab)]."""
        cfg, p, inner, h = self.cfg, self.p, self.inner, self.cfg["heads"]
        rows = tokens.shape[0]
        x = p["shared"].index_select(0, tokens.long())
        pos = torch.full((rows,), t, device=self.dev, dtype=torch.int32)
        for i in range(cfg["dec_layers"]):
            b = f"{DEC}.block.{i}.layer"
            a, c = f"{b}.0.SelfAttention", f"{b}.1.EncDecAttention"
            qkv = ops.linear(ops.rmsnorm(x, p[f"{b}.0.ln"], cfg["eps"]), p[a + ".qkv"], None)
            cache[0, i, :, t].copy_(qkv[:, inner:2 * inner])
            cache[1, i, :, t].copy_(qkv[:, 2 * inner:3 * inner])
            o = ops.attn_relbias(qkv[:, :inner], cache[0, i], cache[1, i], h, t + 1, 1.0, pos, p[DEC + ".bias"], p[DEC + ".center"])
            x = ops.linear(o, p[a + ".o"], None, residual=x)
            q = ops.linear(ops.rmsnorm(x, p[f"{b}.1.ln"], cfg["eps"]), p[c + ".q"], None)
            kv = ckv["kv"][i]
            o = ops.decode_attn(q, kv[:, :, :inner], kv[:, :, inner:2 * inner], h, ckv["nk"], 1.0, group=ckv["group"],
                                lens=ckv["lens"])
            x = ops.linear(o, p[c + ".o"], None, residual=x)
            x = self._ff(x, f"{b}.2")
        hdn = ops.rmsnorm(x, p[DEC + ".final"], cfg["eps"])
        return ops.linear(hdn.float(), p["lm"], None, alpha=self.lm_alpha)

    @torch.no_grad()
    def teacher_forced_logits(self, enc, dec_ids):
        """Logits fp32 [n, T, vocab] of the decoder fed dec_ids [n, T], one position at a time through the caches (tests).  enc =
        (encoder output [n, L, d_model], lens [n])."""
        enc_out, lens = enc
        dec_ids = torch.as_tensor(np.asarray(dec_ids))
        n, tt = dec_ids.shape
        ckv, cache = self.cross_kv(enc_out, lens), self.new_cache(n, tt)
        dev_ids = ops.h2d(dec_ids.to(torch.int32), self.dev)
        out = [self.step(dev_ids[:, t].contiguous(), t, cache, ckv)[:, :self.cfg["vocab"]] for t in range(tt)]
        return torch.stack(out, 1)

    @staticmethod
    def plan_rows(ids, lens):
        """Group the sequences by distinct input.  -> (distinct [input index of a first occurrence], entry_of [per cache entry its
        position in `distinct`], slot_seq [per row slot the sequence it generates, -1 = an empty slot], group)."""
        key = [tuple(int(v) for v in row[:int(n)]) for row, n in zip(np.asarray(ids), np.asarray(lens))]
        first, members = {}, []
        for s, k in enumerate(key):
            if k not in first:
                first[k] = len(members)
                members.append([])
            members[first[k]].append(s)
        group = min(GROUP_MAX, max(len(m) for m in members))
        distinct = [m[0] for m in members]
        entry_of, slot_seq = [], []
        for d, m in enumerate(members):
            for i in range(0, len(m), group):
                part = m[i:i + group]
                entry_of.append(d)
                slot_seq += part + [-1] * (group - len(part))
        return distinct, entry_of, slot_seq, group

    @torch.no_grad()
    def generate(self, ids, lens, *, do_sample, top_k=None, top_p=None, temperature=None, max_length=None, uniforms=None,
                 generator=None):
        """Token ids int64 [n, <= max_length] (numpy), the decoder start token included, as transformers' generate lays them out:
        a finished row emits pad, generation stops once every row has emitted eos or at max_length.  do_sample=False is greedy
        (sample_topk with top_k = 1).  Sampling draws uniforms [n, max_length] once on the CPU from `generator` (or takes `uniforms`),
        indexed by the sequence's index in `ids` and the step: a sequence's tokens do not depend on how the work is batched.
        Identical inputs are encoded once and share their cross K / V, 8 rows to an entry."""
        cfg = self.cfg
        top_k = cfg["top_k"] if top_k is None else int(top_k)
        top_p = cfg["top_p"] if top_p is None else float(top_p)
        temperature = cfg["temperature"] if temperature is None else float(temperature)
        max_length = cfg["max_length"] if max_length is None else int(max_length)
        if max_length < 2:
            raise ValueError("max_length counts the decoder start token: at least 2")
        ids, lens = self._check_input(ids, lens)
        n = ids.shape[0]
        if not do_sample:
            top_k, top_p, temperature = 1, 1.0, 1.0
            uniforms = torch.zeros((n, max_length), dtype=torch.float32)
        elif uniforms is None:
            uniforms = torch.rand((n, max_length), generator=generator, dtype=torch.float32)
        uniforms = torch.as_tensor(np.asarray(uniforms), dtype=torch.float32)
        if uniforms.shape[0] != n or uniforms.shape[1] < max_length - 1:
            raise ValueError(f"uniforms must be [{n}, >= {max_length - 1}]")
        distinct, entry_of, slot_seq, group = self.plan_rows(ids, lens)
        enc_out = self.encode(ids[distinct], lens[distinct])
        ckv = self.cross_kv(enc_out, lens[distinct], entry_of, group)
        rows = len(slot_seq)
        live = [s >= 0 for s in slot_seq]
        seq_of = torch.tensor([max(s, 0) for s in slot_seq])
        u_dev = ops.h2d(uniforms[seq_of].t().contiguous(), self.dev)          # [steps, rows]
        pad, eos = cfg["pad"], cfg["eos"]
        cache = self.new_cache(rows, max_length - 1)
        out = [[cfg["decoder_start"]] for _ in range(rows)]
        open_ = list(live)
        tokens = torch.full((rows,), cfg["decoder_start"], device=self.dev, dtype=torch.int32)
        for t in range(max_length - 1):
            logits = self.step(tokens, t, cache, ckv)
            tok, _, _ = ops.sample_topk(logits, cfg["vocab"], u_dev[t], temperature=temperature, top_k=top_k, top_p=top_p)
            got = tok.cpu().tolist()                                          # the step's one device-to-host copy
            nxt = [g if o else pad for g, o in zip(got, open_)]
            for r in range(rows):
                out[r].append(nxt[r])
                open_[r] = open_[r] and nxt[r] != eos
            if not any(open_):
                break
            tokens = ops.h2d(torch.tensor(nxt, dtype=torch.int32), self.dev)
        res = np.zeros((n, len(out[0])), np.int64)
        for r, s in enumerate(slot_seq):
            if s >= 0:
                res[s] = out[r]
        return res

    # ---- text --------------------------------------------------------------------------------------------------------------------
    def format_input(self, keywords):
        """The keytotext wrapper's input string (RECALLED: config `join` / `strip`): a list of keywords joined into one string, list
        punctuation stripped; a string passes through the same stripping."""
        text = keywords if isinstance(keywords, str) else self.cfg["join"].join(str(k) for k in keywords)
        for ch in self.cfg["strip"]:
            text = text.replace(ch, "")
        return text

    def tokenize(self, texts):
        """Texts -> (padded ids [n, L], lens [n]); every text ends in </s>."""
        enc = [self.tok.encode(t) for t in texts]
        ll = max(len(e) for e in enc)
        ids = np.full((len(enc), ll), self.cfg["pad"], np.int64)
        for i, e in enumerate(enc):
            ids[i, :len(e)] = e
        return ids, np.asarray([len(e) for e in enc], np.int64)

    def sentences(self, keyword_lists, **kw):
        """One sentence per entry of keyword_lists (each a list of keywords or a string)."""
        ids, lens = self.tokenize([self.format_input(k) for k in keyword_lists])
        return [self.tok.decode(row) for row in self.generate(ids, lens, **kw)]
