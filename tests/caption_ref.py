"""CPU reference of the BLIP captioner (tests only; no `transformers` import: the GPU box may lack the package).

- the model: `vision`, `cross_kv`, `decoder_forward` (any number of new positions against a self-attention cache), `lm_head`,
  `teacher_forced_logits`: torch on the CPU in the dtype asked for (fp32 to pin against transformers, float64 as a reference);
- `generate`: greedy and beam search as transformers 5.x runs them (generation/utils.py `_sample` / `_beam_search`), restated on
  float64 log-probabilities, with the smallest gap between adjacent candidates that each image's search met;
- float64 references, fp32 emulations in other summation orders and mutants of the two decoder kernels (csrc/saspa_decode.hip), and
  the error-budget limits tests/test_caption_host.py proves against them (profiles/caption_errbudget.txt)."""
import math

import torch
import torch.nn.functional as F

V = "vision_model"
B_ = "text_decoder.bert"
C_ = "text_decoder.cls.predictions"


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def _lin(sd, name, x):
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def _ln(sd, name, x, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)


def _heads(x, h):
    b, n, c = x.shape
    return x.view(b, n, h, c // h).transpose(1, 2)


def _attend(q, k, v, heads, mask=None):
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    s = qh @ kh.transpose(-1, -2) * (qh.shape[-1] ** -0.5)
    if mask is not None:
        s = s + mask
    o = torch.softmax(s, -1) @ vh
    return o.transpose(1, 2).reshape(q.shape)


def vision(sd, cfg, pixel_values):
    """[B,3,S,S] -> [B, 1 + (S/P)^2, vis_width]: BlipVisionModel.last_hidden_state (post LayerNorm over all tokens)."""
    x = pixel_values.to(sd[V + ".embeddings.class_embedding"].dtype)
    p = F.conv2d(x, sd[V + ".embeddings.patch_embedding.weight"], sd[V + ".embeddings.patch_embedding.bias"], stride=cfg["patch"])
    p = p.flatten(2).transpose(1, 2)
    x = torch.cat([sd[V + ".embeddings.class_embedding"].expand(p.shape[0], -1, -1), p], 1) + sd[V + ".embeddings.position_embedding"]
    eps = cfg["vis_eps"]
    for i in range(cfg["vis_layers"]):
        lp = f"{V}.encoder.layers.{i}"
        h = _ln(sd, lp + ".layer_norm1", x, eps)
        q, k, v = _lin(sd, lp + ".self_attn.qkv", h).chunk(3, -1)
        x = x + _lin(sd, lp + ".self_attn.projection", _attend(q, k, v, cfg["vis_heads"]))
        h = _ln(sd, lp + ".layer_norm2", x, eps)
        x = x + _lin(sd, lp + ".mlp.fc2", F.gelu(_lin(sd, lp + ".mlp.fc1", h)))
    return _ln(sd, V + ".post_layernorm", x, eps)


def cross_kv(sd, cfg, image_embeds):
    """Per decoder layer the cross-attention (K, V) of the image tokens."""
    out = []
    for i in range(cfg["layers"]):
        a = f"{B_}.encoder.layer.{i}.crossattention.self"
        out.append((_lin(sd, a + ".key", image_embeds), _lin(sd, a + ".value", image_embeds)))
    return out


def decoder_forward(sd, cfg, ids, past, enc_kv, dead_cross=False):
    """ids [R, t] new tokens at positions len(past) .. ; past: per layer (K, V) [R, t0, w] or None; enc_kv: cross_kv of each row's
    image.  -> (hidden [R, t, w], new past).  dead_cross (a mutant for the host test): the cross-attention output is dropped."""
    r, t = ids.shape
    t0 = 0 if past is None else past[0][0].shape[1]
    eps, h = cfg["eps"], cfg["heads"]
    x = sd[B_ + ".embeddings.word_embeddings.weight"][ids] + sd[B_ + ".embeddings.position_embeddings.weight"][t0:t0 + t]
    x = _ln(sd, B_ + ".embeddings.LayerNorm", x, eps)
    mask = torch.full((t, t0 + t), float("-inf"), dtype=x.dtype).triu(t0 + 1)
    new = []
    for i in range(cfg["layers"]):
        lp = f"{B_}.encoder.layer.{i}"
        a = lp + ".attention"
        k, v = _lin(sd, a + ".self.key", x), _lin(sd, a + ".self.value", x)
        if past is not None:
            k, v = torch.cat([past[i][0], k], 1), torch.cat([past[i][1], v], 1)
        new.append((k, v))
        o = _attend(_lin(sd, a + ".self.query", x), k, v, h, mask)
        x = _ln(sd, a + ".output.LayerNorm", _lin(sd, a + ".output.dense", o) + x, eps)
        a = lp + ".crossattention"
        o = _attend(_lin(sd, a + ".self.query", x), enc_kv[i][0], enc_kv[i][1], h)
        if dead_cross:
            o = torch.zeros_like(o)
        x = _ln(sd, a + ".output.LayerNorm", _lin(sd, a + ".output.dense", o) + x, eps)
        f = F.gelu(_lin(sd, lp + ".intermediate.dense", x))
        x = _ln(sd, lp + ".output.LayerNorm", _lin(sd, lp + ".output.dense", f) + x, eps)
    return x, new


def lm_head(sd, cfg, x):
    x = _ln(sd, C_ + ".transform.LayerNorm", F.gelu(_lin(sd, C_ + ".transform.dense", x)), cfg["eps"])
    return _lin(sd, C_ + ".decoder", x)


def teacher_forced_logits(sd, cfg, image_embeds, ids):
    """Logits [B, T, vocab] of the decoder fed ids [B, T] (one causal pass)."""
    x, _ = decoder_forward(sd, cfg, ids, None, cross_kv(sd, cfg, image_embeds))
    return lm_head(sd, cfg, x)


def prompt_ids(cfg, tokens):
    """BlipForConditionalGeneration.generate's prompt handling on the tokenizer's output ([CLS] words [SEP]): token 0 becomes BOS and
    the last token (SEP) is dropped."""
    ids = [int(t) for t in tokens]
    ids[0] = cfg["bos"]
    return ids[:-1]


class _Decoder:
    """Cached decoding of rows = images * beams: step(tokens [R, t], beam_idx) -> fp32/64 logits [R, vocab] of the last position."""

    def __init__(self, sd, cfg, image_embeds, beams, dead_cross=False):
        self.sd, self.cfg, self.dead = sd, cfg, dead_cross
        self.enc = [(k.repeat_interleave(beams, 0), v.repeat_interleave(beams, 0)) for k, v in cross_kv(sd, cfg, image_embeds)]
        self.past = None

    def step(self, tokens, beam_idx=None):
        if beam_idx is not None:
            self.past = [(k.index_select(0, beam_idx), v.index_select(0, beam_idx)) for k, v in self.past]
        x, self.past = decoder_forward(self.sd, self.cfg, tokens, self.past, self.enc, self.dead)
        return lm_head(self.sd, self.cfg, x[:, -1])


def _adjacent_gap(sorted_vals):
    """Smallest difference between adjacent live values of a descending [B, n] tensor (dead beams sit at -1e9 and below)."""
    live = sorted_vals > -1e8
    d = sorted_vals[:, :-1] - sorted_vals[:, 1:]
    d = torch.where(live[:, 1:], d, torch.full_like(d, float("inf")))
    return d.min(1)[0]


def generate(sd, cfg, pixel_values, prompt, num_beams=None, max_length=None, min_length=None, image_embeds=None, dead_cross=False):
    """-> (ids [B, L] int64 as transformers' generate returns them, min_gap [B] float64).  prompt: prompt_ids(...)."""
    nb = cfg["num_beams"] if num_beams is None else num_beams
    max_length = cfg["max_length"] if max_length is None else max_length
    min_length = cfg["min_length"] if min_length is None else min_length
    eos, pad, vocab = cfg["eos"], cfg["pad"], cfg["vocab"]
    emb = vision(sd, cfg, pixel_values) if image_embeds is None else image_embeds
    b, p0 = emb.shape[0], len(prompt)
    dec = _Decoder(sd, cfg, emb, nb, dead_cross)
    min_gap = torch.full((b,), float("inf"), dtype=torch.float64)
    if nb == 1:                                                  # GenerationMixin._sample, do_sample=False
        seq = torch.tensor(prompt).repeat(b, 1)
        unfinished = torch.ones(b, dtype=torch.bool)
        tokens = seq
        while True:
            lp = torch.log_softmax(dec.step(tokens).double(), -1)
            if seq.shape[1] < min_length:
                lp[:, eos] = float("-inf")
            top2 = lp.topk(2, -1)[0]
            min_gap = torch.where(unfinished, torch.minimum(min_gap, top2[:, 0] - top2[:, 1]), min_gap)
            nxt = torch.where(unfinished, lp.argmax(-1), torch.full((b,), pad))
            seq = torch.cat([seq, nxt[:, None]], 1)
            unfinished = unfinished & ~((nxt == eos) | (seq.shape[1] >= max_length))
            if not unfinished.any():
                return seq, min_gap
            tokens = nxt[:, None]
    # GenerationMixin._beam_search: length_penalty 1, early_stopping False, one EOS id
    k = 2 * nb
    fill = pad or eos
    run_seq = torch.full((b, nb, max_length), fill, dtype=torch.int64)
    run_seq[:, :, :p0] = torch.tensor(prompt)
    seqs, seq_len = run_seq.clone(), torch.zeros((b, nb), dtype=torch.int64)
    run_scores = torch.zeros((b, nb), dtype=torch.float64)
    run_scores[:, 1:] = -1e9
    beam_scores = torch.full((b, nb), -1e9, dtype=torch.float64)
    finished = torch.zeros((b, nb), dtype=torch.bool)
    unsat = torch.ones((b, 1), dtype=torch.bool)
    top_mask = torch.arange(k) < nb
    cur, beam_idx = p0, None
    tokens = run_seq[:, :, :p0].reshape(b * nb, p0)
    while True:
        lp = torch.log_softmax(dec.step(tokens, beam_idx).double(), -1)
        if cur < min_length:
            lp[:, eos] = float("-inf")
        acc = (lp.view(b, nb, vocab) + run_scores[:, :, None]).view(b, nb * vocab)
        top_v, top_i = acc.topk(min(k + 1, acc.shape[1]), -1)
        min_gap = torch.where(unsat[:, 0], torch.minimum(min_gap, _adjacent_gap(top_v)), min_gap)
        top_v, top_i = top_v[:, :k], top_i[:, :k]
        src, tok = top_i // vocab, top_i % vocab
        cand = run_seq.gather(1, src[:, :, None].expand(-1, -1, max_length)).clone()
        cand[:, :, cur] = tok
        hits = (tok == eos) | (cur + 1 >= max_length)
        run_lp = top_v + hits.double() * -1e9
        nxt = run_lp.topk(nb, -1)[1]
        run_seq = cand.gather(1, nxt[:, :, None].expand(-1, -1, max_length))
        run_scores = run_lp.gather(1, nxt)
        beam_idx = (src.gather(1, nxt) + torch.arange(b)[:, None] * nb).reshape(-1)
        just = hits & top_mask[None]
        fs = top_v / (cur + 1 - p0) + (~unsat).double() * -1e9 + (~just).double() * -1e9
        m_scores = torch.cat([beam_scores, fs], 1)
        m_seqs = torch.cat([seqs, cand], 1)
        m_len = torch.cat([seq_len, torch.full((b, k), cur + 1 - p0)], 1)
        m_fin = torch.cat([finished, just], 1)
        pick = m_scores.topk(nb, -1)[1]
        beam_scores, seq_len, finished = m_scores.gather(1, pick), m_len.gather(1, pick), m_fin.gather(1, pick)
        seqs = m_seqs.gather(1, pick[:, :, None].expand(-1, -1, max_length))
        cur += 1
        worst = torch.where(finished, beam_scores.min(1, keepdim=True)[0].expand(-1, nb), torch.full_like(beam_scores, -1e9))
        unsat = unsat & (run_scores[:, :1] / (cur - p0) > worst).any(-1, keepdim=True)
        if not (unsat.any() and not hits.all()):
            break
        tokens = run_seq[:, :, cur - 1].reshape(b * nb, 1)
    return seqs[:, 0, :p0 + int(seq_len[:, 0].max())], min_gap


# ---------------------------------------------------------------------------------------------------------------------------------
# the two decoder kernels: float64 references, fp32 emulations, mutants
# ---------------------------------------------------------------------------------------------------------------------------------
def rne_store(x, dtype):
    """The kernels' ONE rounding: the fp32 result to the storage type (saspa_decode.hip: Elem<T>::store_chunk at the end of
    decode_attn_kernel; fp32 storage keeps the fp32 value)."""
    return x.to(torch.float32).to(dtype)


def attn_operands(rows, heads, d, group, nk, dtype, seed, lens="mixed", shift=2.0):
    """q [rows, C], caches k / v [entries, nk, C] already rounded to the storage dtype, lens int32 [rows] (1 and nk included)."""
    g = torch.Generator().manual_seed(1000 * seed + rows * 7 + nk)
    c = heads * d
    entries = -(-rows // group)
    q = (torch.randn((rows, c), generator=g) * shift).to(dtype)
    k = torch.randn((entries, nk, c), generator=g).to(dtype)
    v = (torch.randn((entries, nk, c), generator=g) + 0.25).to(dtype)
    if lens == "mixed":                                      # the full length first, then 1 and nk - 1, the rest drawn
        ln = torch.randint(1, nk + 1, (rows,), generator=g, dtype=torch.int32)
        if rows > 1:
            ln[-1] = 1
        if rows > 2:
            ln[1] = max(1, nk - 1)
        ln[0] = nk
    else:
        ln = None
    return q, k, v, ln


def _attn_terms(q, k, v, lens, heads, group, scale, wt):
    """Per (row, head): p [rows, heads, nk] (normalised, zero beyond the row's length) and the entry's V [rows, heads, nk, d], in wt."""
    rows, c = q.shape
    nk, d = k.shape[1], c // heads
    ent = torch.arange(rows) // group
    kk = k.to(wt)[ent].view(rows, nk, heads, d).transpose(1, 2)
    vv = v.to(wt)[ent].view(rows, nk, heads, d).transpose(1, 2)
    s = torch.einsum("rhd,rhkd->rhk", q.to(wt).view(rows, heads, d), kk) * scale
    n = torch.full((rows,), nk) if lens is None else lens.to(torch.int64)
    dead = torch.arange(nk)[None, None, :] >= n[:, None, None]
    s = s.masked_fill(dead, float("-inf"))
    return torch.softmax(s, -1), vv


def attn_ref64(q, k, v, lens, heads, group, scale):
    """-> (out float64 [rows, C] unrounded, magnitude sum_j p_j |v_j| for the budget)."""
    p, vv = _attn_terms(q, k, v, lens, heads, group, scale, torch.float64)
    o = torch.einsum("rhk,rhkd->rhd", p, vv).reshape(q.shape)
    s = torch.einsum("rhk,rhkd->rhd", p, vv.abs()).reshape(q.shape)
    return o, s.clamp_min(max(2.0 ** -10 * s.mean().item(), 1e-30))


def attn_emul(q, k, v, lens, heads, group, scale, *, order="torch", mutant=None):
    """fp32 arithmetic the way a right kernel could do it (order: "torch" = torch's own sums, "rev" = keys and channels reversed,
    "kernel" = saspa_decode.hip's slices: logits as one fma chain over d, the sum over 64 lanes then a butterfly, P V over 256 / (d /
    EPC) key slices summed in order), rounded once to the storage type; or one of the mutants of the catalogue."""
    dt = q.dtype
    rows, c = q.shape
    nk, d = k.shape[1], c // heads
    qq, kk, vv, ln = q, k, v, lens
    if mutant == "no_scale":
        scale = 1.0
    if mutant in ("key_more", "key_less"):
        n = torch.full((rows,), nk, dtype=torch.int64) if lens is None else lens.to(torch.int64)
        ln = (n + (1 if mutant == "key_more" else -1)).clamp(1, nk).to(torch.int32)
    if mutant == "entry_r":
        ent = torch.arange(rows) % k.shape[0]                 # row r reads entry r (wrapped) instead of r // group
        kk, vv, group = k[ent], v[ent], 1
    if mutant == "next_head_v":
        vv = v.view(v.shape[0], nk, heads, d).roll(-1, 2).reshape(v.shape)
    if order == "rev":
        p, vh = _attn_terms(qq.flip(-1).view(rows, heads, d).flip(1).reshape(rows, c), kk.flip(-1).view(-1, nk, heads, d).flip(2).reshape(kk.shape),
                            vv, ln, heads, group, scale, torch.float32)
        o = torch.einsum("rhk,rhkd->rhd", p.flip(-1), vh.flip(2))
    elif order == "kernel":
        p, vh = _attn_terms(qq, kk, vv, ln, heads, group, scale, torch.float32)
        epc = 4 if dt == torch.float32 else 8
        nsl = 256 // (d // epc)
        o = torch.zeros((rows, heads, d), dtype=torch.float32)
        parts = [torch.einsum("rhk,rhkd->rhd", p[:, :, s::nsl], vh[:, :, s::nsl]) for s in range(min(nsl, nk))]
        for part in parts:
            o = o + part
    else:
        p, vh = _attn_terms(qq, kk, vv, ln, heads, group, scale, torch.float32)
        if mutant == "p_16bit":
            p = p.to(torch.bfloat16).to(torch.float32)
        o = torch.einsum("rhk,rhkd->rhd", p, vh)
    return rne_store(o.reshape(rows, c), dt)


def attn_cases():
    """(rows, heads, d, group, nk) covering d in 16 / 64, heads 1 / 4 / 12, group 1 / 3, rows 1 / 3 / 21 and nk in 1, 31, 32, 33, 64, 65,
    577 (one key, around the 32- and 64-key slice boundaries, the 577 image tokens): each nk with three of eight shapes that between
    them hold every value of the other four."""
    shapes = [(1, 1, 16, 1), (3, 4, 64, 3), (21, 12, 64, 3), (3, 12, 16, 1), (21, 4, 16, 3), (1, 4, 64, 1), (21, 1, 64, 1), (3, 1, 16, 3)]
    out = []
    for i, nk in enumerate((1, 31, 32, 33, 64, 65, 577)):
        for j in range(3):
            rows, heads, d, group = shapes[(3 * i + j) % len(shapes)]
            out.append((rows, heads, d, group, nk))
    return out


def topk_cases():
    """(images, group, vocab, ld): the tiny vocabulary, BLIP's (30 524 padded to 30 528) and one that is no multiple of 4."""
    return [(2, 1, 96, 96), (2, 3, 96, 96), (2, 1, 30524, 30528), (2, 3, 30524, 30528), (1, 3, 30521, 30528), (2, 1, 30521, 30524)]


def attn_mutant_applies(mutant, case, dtype):
    """Where a mutant is NAMED: the cases on which it computes something else than the right kernel.  One key leaves nothing to
    scale, drop or round (p = 1); a single row has its full length (no key to add); group 1 reads entry r either way; one head has no
    neighbour.  P rounded to bf16 is named for fp32 storage only: under bf16 storage its error (2^-9 per weight, averaged over the
    keys) sits below the output rounding (2^-8) and CANNOT be separated from a right kernel (profiles/caption_errbudget.txt).  For the
    same reason one key too many / too few is named under bf16 storage only with a dozen or more softmax rows (rows x heads): the one
    key's weight is drawn per row and can sit far below 2^-8 in any single row; among a dozen rows one carries it."""
    rows, heads, d, group, nk = case
    few = dtype == torch.float32 or rows * heads >= 12    # bf16 storage: ONE key may weigh less than the output rounding
    return {"no_scale": nk > 1, "key_more": nk > 1 and rows > 1 and few, "key_less": nk > 1 and few, "p_16bit": nk > 1 and dtype == torch.float32,
            "entry_r": group > 1 and rows > group, "next_head_v": heads > 1}[mutant]


ATTN_MUTANTS = ("no_scale", "key_more", "key_less", "p_16bit", "entry_r", "next_head_v")
ATTN_ORDERS = ("torch", "rev", "kernel")


def topk_operands(images, group, vocab, ld, seed, *, dead_row=False, ties=False, plant_last=False, pad_value=1e30, spread=4.0):
    """fp32 logits [images * group, ld] (pad columns = pad_value), running scores [images * group], the banned token (the first row's
    best: banning it changes the selection).  ties: two equal logits inside each image's first row, above everything else, and --
    with group > 1 -- the image's last row an exact copy of its first with the same score (ties across rows).  plant_last: the last
    candidate of each image (last row, token vocab - 1) is its best."""
    g = torch.Generator().manual_seed(77 * seed + vocab + group)
    rows = images * group
    x = torch.full((rows, ld), pad_value, dtype=torch.float32)
    x[:, :vocab] = torch.randn((rows, vocab), generator=g) * spread
    sc = -torch.rand((rows,), generator=g) * 3.0
    if dead_row and group > 1:
        sc.view(images, group)[:, 1] = float("-inf")
    top = x[:, :vocab].max().item()
    for r in range(0, rows, group):
        if ties:
            x[r, 5], x[r, vocab - 2] = top + 1.0, top + 1.0
            sc[r] = 0.0                                                   # the tied candidates lead the image's selection
            if group > 1:
                x[r + group - 1], sc[r + group - 1] = x[r], sc[r]
        if plant_last:
            x[r + group - 1, vocab - 1] = top + 8.0
    return x, sc, int(x[0, :vocab].argmax())


def select_topk(cand, k, ties_highest=False):
    """[images, n] -> (values, flat indices) of the k best per image, descending, ties to the lowest (mutant: highest) index."""
    if ties_highest:
        v, i = torch.sort(cand.flip(-1), dim=-1, descending=True, stable=True)
        return v[:, :k], cand.shape[1] - 1 - i[:, :k]
    v, i = torch.sort(cand, dim=-1, descending=True, stable=True)
    return v[:, :k], i[:, :k]


def topk_candidates64(x, vocab, group, scores, ban, ban_on, *, mutant=None):
    """All candidates [images, group * vocab] in float64: (x - max) - log sum exp(x - max) over the live columns, the ban, + score."""
    live = x[:, :(x.shape[1] if mutant == "pad_in_lse" else vocab)].double()
    lp = live - live.max(-1, keepdim=True)[0]
    lp = (lp - lp.exp().sum(-1, keepdim=True).log())[:, :vocab]
    if ban_on and mutant != "ban_ignored":
        lp[:, ban] = float("-inf")
    if mutant != "score_not_added":
        lp = lp + scores.double()[:, None]
    return lp.reshape(x.shape[0] // group, group * vocab)


def topk_ref64(x, vocab, group, scores, ban, ban_on, *, mutant=None):
    """-> (score, flat index), each [images, 2 * group + 1]: the selection and the runner-up (for the gap below the last)."""
    cand = topk_candidates64(x, vocab, group, scores, ban, ban_on, mutant=mutant)
    if mutant == "last_dropped":
        cand = cand[:, :-1]
    return select_topk(cand, min(2 * group + 1, cand.shape[1]), mutant == "ties_highest")


def topk_emul(x, vocab, group, scores, ban, ban_on, *, order="torch"):
    """The selection from fp32 arithmetic in another order of operations: "torch" (torch.log_softmax in fp32), "rev" (the exp-sum over
    the columns reversed, one running sum), "kernel" (exp-sums over 1024 x 4-column strides, 64-lane butterflies, 16 waves in order:
    saspa_decode.hip logprob_topk_kernel).  -> (score fp32, flat index) [images, 2 * group]."""
    xs = x[:, :vocab]
    if order == "torch":
        lp = torch.log_softmax(xs, -1)
    else:
        m = xs.max(-1, keepdim=True)[0]
        e = (xs - m).exp()
        if order == "rev":
            s = e.flip(-1).cumsum(-1)[:, -1]
        else:
            e = F.pad(e, (0, -vocab % 4096)).view(x.shape[0], -1, 1024, 4)      # [rows, stride step, thread, 4]
            t = e.permute(0, 2, 1, 3).reshape(x.shape[0], 1024, -1)              # a thread's values in its own order
            acc = torch.zeros((x.shape[0], 1024))
            for j in range(t.shape[2]):
                acc = acc + t[:, :, j]
            w = acc.view(-1, 16, 64)
            for o in (32, 16, 8, 4, 2, 1):
                w = w + w[:, :, torch.arange(64) ^ o]
            s = torch.zeros((x.shape[0],))
            for wv in range(16):
                s = s + w[:, wv, 0]
        lp = (xs - m) - s.log()[:, None]
    if ban_on:
        lp = lp.clone()
        lp[:, ban] = float("-inf")
    return select_topk((lp + scores[:, None]).reshape(x.shape[0] // group, group * vocab), 2 * group)


TOPK_MUTANTS = ("ban_ignored", "score_not_added", "pad_in_lse", "ties_highest", "last_dropped")
TOPK_ORDERS = ("torch", "rev", "kernel")
TOPK_UNIT = 2.0 ** -24


def topk_check(got_score, got_idx, ref_score, ref_idx, limit):
    """A selection [images, k] (scores, flat indices) against topk_ref64's [images, k + 1].
    -> (score error, index mismatches): the largest |got - ref| in units of 2^-24 max(1, |ref|) over the finite reference scores
    (inf where a reference -inf is not reproduced), and the number of positions whose index differs although the reference decides
    it: both neighbours of the reference score are either further than 4 * limit units away or EXACTLY equal (planted ties: equal
    inputs, equal in any arithmetic -- they must go to the lowest flat index)."""
    k = got_score.shape[1]
    g, r = got_score.double(), ref_score.double()
    unit = TOPK_UNIT * r[:, :k].abs().clamp(1.0, 1e30)
    fin = torch.isfinite(r[:, :k])
    err = torch.where(fin, (g - r[:, :k]).abs() / unit, torch.where(g == r[:, :k], torch.zeros_like(g), torch.full_like(g, float("inf"))))
    err = torch.nan_to_num(err, nan=float("inf"))
    rr = torch.cat([torch.full_like(r[:, :1], float("inf")), r], 1)                      # a sentinel above the best
    if rr.shape[1] < k + 2:
        rr = torch.cat([rr, torch.full_like(r[:, :1], float("-inf"))], 1)
    up, down = rr[:, :k] - rr[:, 1:k + 1], rr[:, 1:k + 1] - rr[:, 2:k + 2]
    tol = 4.0 * limit * unit
    decided = ((up > tol) | (up == 0)) & ((down > tol) | (down == 0)) & fin
    return err.max().item(), int(((got_idx != ref_idx[:, :k]) & decided).sum())


# Limits: 2x the worst legitimate emulation over tests/test_errbudget.SEEDS on attn_cases() / topk_cases(), measured on the CPU by
# tests/test_caption_host.py (profiles/caption_errbudget.txt records both sides).
# decode_attn: errbudget's four statistics in units of the storage type (2^-8 bf16, 2^-24 fp32) of sum_j p_j |v_j|.  Legit worst: bf16
# max 0.99, rms 0.29, bias and slope of every emulation far inside their noise allowance (errbudget.Z_NOISE standard errors), so their
# systematic limits are a small floor, not a measured value; fp32 max 24.3, rms 2.7, and on a single row (1 x 4 heads x 64) bias 0.90
# and slope 3.2 at standard errors of 0.14 / 0.60 -- the rounding of a row's sum is common to the row, so the standard error
# understates it (as errbudget.py notes for "f32_tail"): the limits are what leaves those at half their allowance.
ATTN_LIMITS = {
    torch.bfloat16: dict(max=2.0, rms=0.6, bias=0.005, slope=0.01),
    torch.float32: dict(max=49.0, rms=5.5, bias=0.7, slope=1.7),
}
# logprob_topk: topk_check's score error.  Legit worst 63.9 units (the running sum over the reversed columns).
TOPK_SCORE_LIMIT = 130.0
