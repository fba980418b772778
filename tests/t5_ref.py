"""torch-CPU restatement of the T5 key-to-text generator (saspa_aug_amd/txt2sentence.py) and float64 references of the three kernels of
csrc/saspa_t5.hip (tests only).

The model (`encode`, `decoder_logits`, `generate`) is fp32 on the state dict in the public transformers key layout; `emul=torch.bfloat16`
rounds the weights and every activation at exactly the points where the device stores one (each linear, norm and attention output),
wt=torch.float64 runs it in double.  tests/test_t5_host.py pins it against transformers' T5ForConditionalGeneration (encoder output,
teacher-forced logits, greedy ids), `bucket` against T5Attention._relative_position_bucket and `sample_ref64` against the Temperature ->
TopK -> TopP warpers.

Kernel references: `rmsnorm_ref64`, `relbias_ref64`, `sample_ref64`, each with fp32 emulations in other orders of operations (what a
right kernel may do) and named mutants (what a wrong one would): the budgets below are 2x the worst emulation, every mutant must
exceed 2x the budget (tests/test_t5_host.py proves both on the CPU; profiles/t5_errbudget.txt records the figures)."""
import math

import torch

import errbudget as E

# Seeds of the decision tests, chosen on the CPU (tests/test_t5_host.py::test_decision_seeds_meet_their_conditions): every greedy step's
# top-1 / top-2 logit gap exceeds 1e-3 relative and every sampled draw is decidable (U_MARGIN / P_MARGIN below).
WEIGHT_SEED, INPUT_SEED, UNIFORM_SEED, GROUP_UNIFORM_SEED = 3, 11, 26, 40


def tiny_inputs(cfg, seed=INPUT_SEED, n=8):
    """n ragged inputs with lengths 1 .. 20 (1 and 20 included), eos-terminated, pad after."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(2, 20, (n,), generator=g)
    lens[0], lens[1] = 1, 20
    ids = torch.full((n, 20), 0, dtype=torch.long)
    for i, ln in enumerate(lens.tolist()):
        ids[i, :ln - 1] = torch.randint(3, cfg["vocab"], (ln - 1,), generator=g)
        ids[i, ln - 1] = cfg["eos"]
    return ids, lens


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------


def bucket(rel, bidirectional, num_buckets, max_distance):
    """T5's relative-position bucket of rel = memory position - query position (int64 tensor): the public algorithm, float32 log."""
    rel = rel.long()
    ret = torch.zeros_like(rel)
    n = num_buckets
    if bidirectional:
        n //= 2
        ret = ret + (rel > 0).long() * n
        rel = rel.abs()
    else:
        rel = (-rel).clamp_min(0)
    max_exact = n // 2
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (n - max_exact)).long()
    large = large.clamp_max(n - 1)
    return ret + torch.where(rel < max_exact, rel, large)


def position_bias(weight, qpos, klen, bidirectional, cfg):
    """[heads, len(qpos), klen] from the stack's table weight [buckets, heads]."""
    rel = torch.arange(klen)[None, :] - torch.as_tensor(qpos)[:, None]
    return weight[bucket(rel, bidirectional, cfg["buckets"], cfg["max_distance"])].permute(2, 0, 1)


class Ref:
    def __init__(self, sd, cfg, emul=None, wt=torch.float32):
        self.cfg, self.emul, self.wt = cfg, emul, wt
        keep = ("layer_norm.weight", "relative_attention_bias.weight")                  # fp32 on the device: never rounded
        self.sd = {k: (v.float() if emul is None or k.endswith(keep) else v.float().to(emul).float()).to(wt) for k, v in sd.items()}
        self.head = self.sd["shared.weight"] if cfg["tie_embeddings"] else self.sd["lm_head.weight"]

    def r(self, x):
        """A device storage point."""
        return x if self.emul is None else x.to(self.emul).to(self.wt)

    def rms(self, x, name):
        v = x.pow(2).mean(-1, keepdim=True)
        return self.r(self.sd[name] * (x * torch.rsqrt(v + self.cfg["eps"])))

    def attn(self, pfx, xq, xkv, bias, dead):
        """xq [n, Tq, d], xkv [n, Tk, d], bias [heads, Tq, Tk] or None, dead [n, 1|Tq, Tk] bool -> [n, Tq, inner]."""
        h, dk = self.cfg["heads"], self.cfg["d_kv"]
        n, tq, tk = xq.shape[0], xq.shape[1], xkv.shape[1]
        q = self.r(xq @ self.sd[pfx + ".q.weight"].t()).view(n, tq, h, dk).transpose(1, 2)
        k = self.r(xkv @ self.sd[pfx + ".k.weight"].t()).view(n, tk, h, dk).transpose(1, 2)
        v = self.r(xkv @ self.sd[pfx + ".v.weight"].t()).view(n, tk, h, dk).transpose(1, 2)
        s = q @ k.transpose(-1, -2)                                                     # T5: no 1 / sqrt(d_kv)
        if bias is not None:
            s = s + bias[None].to(self.wt)
        s = s.masked_fill(dead[:, None], float("-inf"))
        o = torch.softmax(s, -1) @ v
        return self.r(o.transpose(1, 2).reshape(n, tq, h * dk))

    def ff(self, x, b):
        hdn = self.rms(x, b + ".layer_norm.weight")
        f = self.r(torch.relu(hdn @ self.sd[b + ".DenseReluDense.wi.weight"].t()))
        return self.r(f @ self.sd[b + ".DenseReluDense.wo.weight"].t() + x)

    def encode(self, ids, lens):
        cfg = self.cfg
        ids, lens = torch.as_tensor(ids).long(), torch.as_tensor(lens).long()
        n, ll = ids.shape
        x = self.sd["shared.weight"][ids]
        dead = (torch.arange(ll)[None] >= lens[:, None])[:, None, :]
        bias = position_bias(self.sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], torch.arange(ll), ll, True, cfg)
        for i in range(cfg["enc_layers"]):
            b = f"encoder.block.{i}.layer"
            hdn = self.rms(x, b + ".0.layer_norm.weight")
            o = self.attn(b + ".0.SelfAttention", hdn, hdn, bias, dead)
            x = self.r(o @ self.sd[b + ".0.SelfAttention.o.weight"].t() + x)
            x = self.ff(x, b + ".1")
        return self.rms(x, "encoder.final_layer_norm.weight")

    def decoder_logits(self, enc_out, lens, dec_ids):
        """Teacher-forced: logits [n, T, vocab] for decoder inputs dec_ids [n, T]."""
        cfg = self.cfg
        dec_ids, lens = torch.as_tensor(dec_ids).long(), torch.as_tensor(lens).long()
        n, tt = dec_ids.shape
        ll = enc_out.shape[1]
        x = self.sd["shared.weight"][dec_ids]
        causal = (torch.arange(tt)[None, :] > torch.arange(tt)[:, None])[None].expand(n, -1, -1)
        cross_dead = (torch.arange(ll)[None] >= lens[:, None])[:, None, :]
        bias = position_bias(self.sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], torch.arange(tt), tt, False, cfg)
        for i in range(cfg["dec_layers"]):
            b = f"decoder.block.{i}.layer"
            hdn = self.rms(x, b + ".0.layer_norm.weight")
            o = self.attn(b + ".0.SelfAttention", hdn, hdn, bias, causal)
            x = self.r(o @ self.sd[b + ".0.SelfAttention.o.weight"].t() + x)
            hdn = self.rms(x, b + ".1.layer_norm.weight")
            o = self.attn(b + ".1.EncDecAttention", hdn, enc_out, None, cross_dead)
            x = self.r(o @ self.sd[b + ".1.EncDecAttention.o.weight"].t() + x)
            x = self.ff(x, b + ".2")
        hdn = self.rms(x, "decoder.final_layer_norm.weight")
        if cfg["tie_embeddings"]:
            hdn = hdn * cfg["d_model"] ** -0.5
        return hdn @ self.head.t()

    def generate(self, ids, lens, *, do_sample, top_k=50, top_p=1.0, temperature=1.0, max_length=20, uniforms=None):
        """-> (ids int64 [n, <= max_length] laid out as transformers' generate does (start token first, pad after eos), the smallest
        relative top-1 / top-2 logit gap of any live step, whether every live draw was decidable)."""
        cfg = self.cfg
        ids, lens = torch.as_tensor(ids).long(), torch.as_tensor(lens).long()
        n = ids.shape[0]
        if not do_sample:
            top_k, top_p, temperature, uniforms = 1, 1.0, 1.0, torch.zeros((n, max_length))
        uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
        enc = self.encode(ids, lens)
        out = torch.full((n, 1), cfg["decoder_start"], dtype=torch.long)
        open_ = torch.ones(n, dtype=torch.bool)
        min_gap, decidable = float("inf"), True
        for t in range(max_length - 1):
            logits = self.decoder_logits(enc, lens, out)[:, -1].float()
            top2 = logits.topk(2, -1)[0].double()
            gap = ((top2[:, 0] - top2[:, 1]) / top2[:, 0].abs().clamp_min(1e-30))[open_]
            s = sample_ref64(logits, cfg["vocab"], temperature, top_k, top_p, uniforms[:, t])
            if open_.any():
                min_gap = min(min_gap, gap.min().item())
                decidable = decidable and bool(s["decidable"][open_].all())
            nxt = torch.where(open_, s["tok"], torch.full_like(s["tok"], cfg["pad"]))
            out = torch.cat([out, nxt[:, None]], 1)
            open_ = open_ & (nxt != cfg["eos"])
            if not open_.any():
                break
        return out, min_gap, decidable


# ---------------------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------------------
U_MARGIN, P_MARGIN = 1e-5, 1e-4            # a draw / a top-p cut closer than this to a float64 boundary is not decidable in fp32
SAMPLE_MUTANTS = ("topp_before_topk", "draw_ge", "topp_gt", "ties_highest")


def sample_ref64(x, vocab, temperature, top_k, top_p, u, *, mutant=None):
    """One sampling step in float64 on fp32 logits x [rows, ld >= vocab] and uniforms u [rows] (saspa_hip.h, saspa_sample_topk):
    y = x / temperature (the fp32 division, as transformers' warper and the kernel do it), the top_k largest with ties to the lowest
    id, softmax over them, the shortest prefix reaching top_p, renormalised, the first token whose cumulative mass exceeds u.
    -> dict(tok [rows], logp [rows], kept: per row the kept token ids in order, probs: per row their probabilities, decidable [rows]).
    decidable: u is farther than U_MARGIN from every cumulative boundary below the last, and (top_p < 1) no cumulative mass of the
    top-k distribution is within P_MARGIN of top_p."""
    x = torch.as_tensor(x, dtype=torch.float32)
    rows = x.shape[0]
    y = (x[:, :vocab] / torch.tensor(temperature, dtype=torch.float32)).double()
    k = min(int(top_k), vocab)
    if mutant == "ties_highest":
        sv, si = torch.sort(y.flip(-1), dim=-1, descending=True, stable=True)
        si = vocab - 1 - si
    else:
        sv, si = torch.sort(y, dim=-1, descending=True, stable=True)
    u = torch.as_tensor(u, dtype=torch.float32).double()
    tok, logp, kept, probs, dec = [], [], [], [], []
    for r in range(rows):
        if mutant == "topp_before_topk" and top_p < 1.0:
            full = torch.softmax(sv[r], -1).cumsum(-1)
            nfull = int((full >= top_p).nonzero()[0]) + 1
            n = min(k, nfull)
            pr = torch.softmax(sv[r, :n], -1)
            cum_k = pr.cumsum(-1)
        else:
            pk = torch.softmax(sv[r, :k], -1)
            cum_k = pk.cumsum(-1)
            n = k
            if top_p < 1.0:
                hit = (cum_k > top_p) if mutant == "topp_gt" else (cum_k >= top_p)
                n = int(hit.nonzero()[0]) + 1 if hit.any() else k
            pr = pk[:n] / pk[:n].sum()
        cum = pr.cumsum(-1)
        over = (cum >= u[r]) if mutant == "draw_ge" else (cum > u[r])
        i = int(over.nonzero()[0]) if over.any() else n - 1
        tok.append(int(si[r, i]))
        logp.append(float(pr[i].log()))
        kept.append(si[r, :n].clone())
        probs.append(pr)
        ok = n == 1 or bool(((cum[:-1] - u[r]).abs() > U_MARGIN).all())
        if top_p < 1.0:
            ok = ok and bool(((cum_k - top_p).abs() > P_MARGIN).all())
        dec.append(ok)
    return dict(tok=torch.tensor(tok), logp=torch.tensor(logp, dtype=torch.float64), kept=kept, probs=probs, decidable=torch.tensor(dec))


def sample_operands(rows, vocab, seed, spread=3.0, pad_value=1e30):
    """fp32 logits [rows, ld] with ld = vocab rounded up to 8 plus 8 pad columns of +1e30 (a pad that reached a maximum or a sum would
    show), uniforms [rows] with 0 first and 1 - 2^-24 second."""
    g = torch.Generator().manual_seed(9000 + 31 * seed + vocab)
    ld = (vocab + 7) // 8 * 8 + 8
    x = torch.full((rows, ld), pad_value, dtype=torch.float32)
    x[:, :vocab] = torch.randn((rows, vocab), generator=g) * spread
    u = torch.rand((rows,), generator=g, dtype=torch.float32)
    u[0] = 0.0
    if rows > 1:
        u[1] = 1.0 - 2.0 ** -24
    return x, u


SAMPLE_GRID = [(t, k, p) for t in (1.0, 0.7) for k in (1, 50) for p in (1.0, 0.9)]
SAMPLE_VOCABS = (40, 1000, 32128)


# ---------------------------------------------------------------------------------------------------------------------------------
# RMS norm
# ---------------------------------------------------------------------------------------------------------------------------------
UNITS = {torch.bfloat16: E.UNIT_BF16, torch.float32: E.UNIT_F32}
RMS_MUTANTS = ("mean_sub", "eps_outside")
RMS_ORDERS = ("torch", "rev", "kernel")
RMS_SHAPES = [(rows, c) for rows in (1, 5, 33) for c in (64, 72, 768, 1024)]
RMS_EPS = 1e-6


def rne_store(x, dtype):
    """The kernels' ONE rounding: the fp32 result to the storage type."""
    return x.to(torch.float32).to(dtype)


def rms_operands(rows, c, dtype, seed):
    """x [rows, c] storage-rounded with a mean offset (a mean subtraction shows) and row magnitudes cycling through 1, 1e-3 and 30
    (at 1e-3 the mean square is eps-sized: where eps sits shows); gamma fp32 [c] of both signs."""
    g = torch.Generator().manual_seed(500 * seed + 3 * rows + c)
    mag = torch.tensor([1.0, 1e-3, 30.0])[torch.arange(rows) % 3][:, None]
    x = ((torch.randn((rows, c), generator=g) + 0.25) * mag).to(dtype)
    gamma = (1.0 + 0.5 * torch.randn((c,), generator=g)).float()
    return x, gamma


def rmsnorm_ref64(x, gamma, eps, *, mutant=None):
    """-> (out float64 unrounded, magnitude |out| floored)."""
    x64, g64 = x.double(), gamma.double()
    if mutant == "mean_sub":
        x64 = x64 - x64.mean(-1, keepdim=True)
    ms = x64.pow(2).mean(-1, keepdim=True)
    rs = 1.0 / (ms.sqrt() + eps) if mutant == "eps_outside" else torch.rsqrt(ms + eps)
    o = x64 * rs * g64
    return o, E.norm_scale(x64 * rs, g64, torch.zeros_like(g64))


def rmsnorm_emul(x, gamma, eps, *, order="torch", mutant=None):
    """fp32 arithmetic in the order a right kernel could take ("torch": torch's own mean; "rev": the channels reversed; "kernel":
    saspa_t5.hip's lanes -- 16-byte chunks dealt to 64 lanes, one running sum per lane, the butterfly, 1 / sqrt), rounded once."""
    dt = x.dtype
    if mutant is not None:
        return rne_store(rmsnorm_ref64(x, gamma, eps, mutant=mutant)[0], dt)
    xf = x.float()
    c = xf.shape[-1]
    if order == "torch":
        o = gamma * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))
    elif order == "rev":
        ss = xf.flip(-1).pow(2).cumsum(-1)[:, -1:]
        o = (xf * (1.0 / torch.sqrt(ss / c + eps))) * gamma
    else:
        epc = 4 if dt == torch.float32 else 8
        sq = torch.nn.functional.pad(xf.pow(2), (0, -c % (64 * epc))).view(xf.shape[0], -1, 64, epc)   # [rows, step, lane, element]
        lane = torch.zeros((xf.shape[0], 64))
        for s in range(sq.shape[1]):
            for e in range(epc):
                lane = lane + sq[:, s, :, e]
        for o_ in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, torch.arange(64) ^ o_]
        o = (xf * (1.0 / torch.sqrt(lane[:, :1] / c + eps))) * gamma
    return rne_store(o, dt)


def rms_mutant_applies(mutant, shape):
    """eps outside the root moves a row by eps / rms: named where a row of magnitude 1e-3 exists (rows > 1)."""
    return {"mean_sub": True, "eps_outside": shape[0] > 1}[mutant]


# ---------------------------------------------------------------------------------------------------------------------------------
# attention with a relative-position bias
# ---------------------------------------------------------------------------------------------------------------------------------
REL_MUTANTS = ("bias_before_scale", "col_off_by_one", "no_clamp", "wrong_head")
REL_ORDERS = ("torch", "rev", "kernel", "exp64")
REL_TABLES = [(8, 16, True), (32, 128, True), (8, 16, False), (32, 128, False)]       # (buckets, max distance, bidirectional)
ENTRIES = 6                    # rows = 6, 18, 120: rows 0 .. 4 are the planted ones (rel_operands)


def rel_cases():
    """(heads, d, nk, rows_per_entry, table index): every (heads, d) x nk x rows_per_entry of the issue, the four tables dealt round."""
    out = []
    for hd in ((4, 16), (12, 64)):
        for nk in (1, 7, 64, 65, 130):
            for rpe in (1, 3, 20):
                out.append(hd + (nk, rpe, len(out) % len(REL_TABLES)))
    return out


def rel_table(heads, table, seed):
    """(fp32 [heads, ncol], center) of REL_TABLES[table] from a random [buckets, heads] weight, built as the host model builds it."""
    from saspa_aug_amd.txt2sentence import bias_table
    nb, md, bidir = REL_TABLES[table]
    g = torch.Generator().manual_seed(70 + seed + 13 * table + heads)
    return bias_table(torch.randn((nb, heads), generator=g) * 2.0, bidir, nb, md)


def rel_operands(case, dtype, seed):
    """q [rows, C], caches k / v [entries, nk, C] storage-rounded, lens int32 [rows] (0, 1 and nk planted), pos int32 [rows] spread so
    that pos - j + center runs off both ends of the table (one row wholly beyond each end), the table and its center."""
    heads, d, nk, rpe, table = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * nk + rpe + heads)
    c, rows = heads * d, ENTRIES * rpe
    q = (torch.randn((rows, c), generator=g) * 2.0).to(dtype)
    k = torch.randn((ENTRIES, nk, c), generator=g).to(dtype)
    v = (torch.randn((ENTRIES, nk, c), generator=g) + 0.25).to(dtype)
    ln = torch.randint(1, nk + 1, (rows,), generator=g, dtype=torch.int32)
    bias, center = rel_table(heads, table, seed)
    ncol = bias.shape[1]
    pos = torch.randint(-ncol, nk + ncol, (rows,), generator=g, dtype=torch.int32)
    ln[0], ln[1], ln[2], ln[3], ln[4] = nk, 0, 1, nk, nk
    pos[0] = nk // 2                                      # every key near the query: the exact buckets and their boundaries
    pos[3] = nk + ncol                                    # every key of row 3 beyond the table's last column
    pos[4] = -ncol                                        # ... of row 4 before its first
    return q, k, v, ln, pos, bias, center


def rel_columns(pos, nk, center, ncol, clamp=True):
    col = pos.long()[:, None] - torch.arange(nk)[None, :] + center
    return col.clamp(0, ncol - 1) if clamp else col


def _rel_logits(q, k, v, ln, pos, bias, center, heads, rpe, scale, wt, mutant=None):
    """-> (logits [rows, heads, nk] with -inf on the dead keys, the rows' V [rows, heads, nk, d]) in wt."""
    rows, c = q.shape
    nk, d = k.shape[1], c // heads
    ncol = bias.shape[1]
    ent = torch.arange(rows) // rpe
    kk = k.to(wt)[ent].view(rows, nk, heads, d).transpose(1, 2)
    vv = v.to(wt)[ent].view(rows, nk, heads, d).transpose(1, 2)
    col = rel_columns(pos, nk, center, ncol)
    if mutant == "col_off_by_one":
        col = (col + 1).clamp_max(ncol - 1)
    if mutant == "no_clamp":
        col = rel_columns(pos, nk, center, ncol, clamp=False) % ncol      # an unclamped index wraps (or reads the next row)
    b = bias.to(wt)
    if mutant == "wrong_head":
        b = b.roll(-1, 0)
    bb = b[:, col].permute(1, 0, 2)                                        # [rows, heads, nk]
    s = torch.einsum("rhd,rhkd->rhk", q.to(wt).view(rows, heads, d), kk)
    s = (s + bb) * scale if mutant == "bias_before_scale" else s * scale + bb
    dead = torch.arange(nk)[None, None, :] >= ln.to(torch.int64)[:, None, None]
    return s.masked_fill(dead, float("-inf")), vv


def _rel_terms(q, k, v, ln, pos, bias, center, heads, rpe, scale, wt, mutant=None):
    s, vv = _rel_logits(q, k, v, ln, pos, bias, center, heads, rpe, scale, wt, mutant)
    return torch.nan_to_num(torch.softmax(s, -1), nan=0.0), vv             # len 0: a zero row


def relbias_ref64(q, k, v, ln, pos, bias, center, heads, rpe, scale, *, mutant=None):
    """-> (out float64 [rows, C] unrounded, magnitude sum_j p_j |v_j| floored)."""
    p, vv = _rel_terms(q, k, v, ln, pos, bias, center, heads, rpe, scale, torch.float64, mutant)
    o = torch.einsum("rhk,rhkd->rhd", p, vv).reshape(q.shape)
    s = torch.einsum("rhk,rhkd->rhd", p, vv.abs()).reshape(q.shape)
    return o, s.clamp_min(max(2.0 ** -10 * s.mean().item(), 1e-30))


def relbias_emul(q, k, v, ln, pos, bias, center, heads, rpe, scale, *, order="torch", mutant=None):
    """fp32 arithmetic as a right kernel could do it, rounded once; or a mutant.  order: "torch" (torch's softmax, then P V); "rev" (P V
    over the keys reversed); "kernel" (saspa_t5.hip: e = exp(logit - max) unnormalised, P V over its 256 / (d / EPC) key slices summed in
    order, ONE division by the sum); "exp64" (the same with a correctly rounded exp: expf implementations differ in the last place)."""
    dt = q.dtype
    rows, c = q.shape
    nk, d = k.shape[1], c // heads
    if order in ("kernel", "exp64"):
        s, vh = _rel_logits(q, k, v, ln, pos, bias, center, heads, rpe, scale, torch.float32, mutant)
        m = s.max(-1, keepdim=True)[0]
        z = torch.nan_to_num(s - m, nan=float("-inf"))                     # len 0: every key dead
        e = z.double().exp().float() if order == "exp64" else z.exp()
        nsl = 256 // (d // (4 if dt == torch.float32 else 8))
        o = torch.zeros((rows, heads, d))
        for sl in range(min(nsl, nk)):
            o = o + torch.einsum("rhk,rhkd->rhd", e[:, :, sl::nsl], vh[:, :, sl::nsl])
        l = e.sum(-1, keepdim=True)
        o = torch.where(l > 0, o / l, torch.zeros_like(o))
        return rne_store(o.reshape(rows, c), dt)
    p, vh = _rel_terms(q, k, v, ln, pos, bias, center, heads, rpe, scale, torch.float32, mutant)
    if order == "rev":
        o = torch.einsum("rhk,rhkd->rhd", p.flip(-1), vh.flip(2))
    else:
        o = torch.einsum("rhk,rhkd->rhd", p, vh)
    return rne_store(o.reshape(rows, c), dt)


def rel_mutant_applies(mutant, case, ln, pos, center, ncol):
    """Where a mutant is NAMED: with one key the softmax is 1 whatever the logit; one head has no neighbour; without a column off the
    table nothing is clamped.  Asked of rows x heads >= 12 softmax rows (as tests/caption_ref.py: a bias change on ONE row's keys can
    sit below the bf16 output rounding)."""
    heads, d, nk, rpe, table = case
    many = nk > 1
    raw = rel_columns(pos, nk, center, ncol, clamp=False)
    live = torch.arange(nk)[None, :] < ln.long()[:, None]
    multi = ln.long() > 1
    clamps = bool((((raw < 0) | (raw > ncol - 1)) & live & multi[:, None]).any())
    return {"bias_before_scale": many, "col_off_by_one": many, "no_clamp": many and clamps, "wrong_head": many and heads > 1}[mutant]


# Limits: 2x the worst legitimate emulation over SEEDS on RMS_SHAPES / rel_cases(), measured on the CPU by tests/test_t5_host.py
# (test_rmsnorm_budget_margins, test_relbias_budget_margins; profiles/t5_errbudget.txt records both sides).  errbudget's four
# statistics in units of the storage type (2^-8 bf16, 2^-24 fp32) of |out| (RMS norm) and of sum_j p_j |v_j| (attention).  bias and
# slope of every emulation sit inside their noise allowance (errbudget.Z_NOISE standard errors) except where one row's common
# rounding (its 1 / rms, its softmax sum) is systematic over the few outputs of a small case: their limits are what leaves those
# at half their allowance.
SEEDS = (0, 1, 2, 3)
RMS_LIMITS = {
    # legit worst: bf16 max 0.996, rms 0.469; fp32 max 4.00, rms 2.05 (torch's own rsqrt), and on the 64-channel single rows bias and
    # slope whose half-allowance needs 3.73 / 2.52 -- a row's 1 / rms is rounded once for the whole row
    torch.bfloat16: dict(max=2.0, rms=0.94, bias=0.01, slope=0.02),
    torch.float32: dict(max=8.1, rms=4.1, bias=3.8, slope=2.6),
}
REL_LIMITS = {
    # legit worst: bf16 max 0.995, rms 0.312; fp32 max 26.4, rms 2.44, half-allowance needs bias 0.129, slope 0.359
    torch.bfloat16: dict(max=2.0, rms=0.63, bias=0.005, slope=0.01),
    torch.float32: dict(max=53.0, rms=4.9, bias=0.13, slope=0.36),
}

# ---------------------------------------------------------------------------------------------------------------------------------
# the margins of the limits (tests/test_t5_host.py asserts them; `python tests/t5_ref.py` prints the raw statistics)
# ---------------------------------------------------------------------------------------------------------------------------------
def _fold(legit, raw, st, limits):
    """raw: the worst max / rms, and for bias / slope the systematic limit that would leave the worst case at half its allowance
    (2 |stat| - Z_NOISE standard errors)."""
    a = E.allowance(st, limits)
    for key in E.STATS:
        legit[key] = max(legit[key], abs(st[key]) / a[key])
    for key in ("max", "rms"):
        raw[key] = max(raw[key], abs(st[key]))
    for key in ("bias", "slope"):
        raw[key] = max(raw[key], 2.0 * abs(st[key]) - E.Z_NOISE * st["se_" + key])


def rms_margins(dtype, limits=None):
    """-> (legit worst statistic / allowance, the raw worst statistics, per mutant (weakest ratio, case, seed))."""
    limits = RMS_LIMITS[dtype] if limits is None else limits
    legit, raw, mut = {k: 0.0 for k in E.STATS}, {k: 0.0 for k in E.STATS}, {}
    for seed in SEEDS:
        for shape in RMS_SHAPES:
            x, gamma = rms_operands(*shape, dtype, seed)
            ref, s = rmsnorm_ref64(x, gamma, RMS_EPS)
            for order in RMS_ORDERS:
                _fold(legit, raw, E.budget_stats(rmsnorm_emul(x, gamma, RMS_EPS, order=order), ref, s, UNITS[dtype]), limits)
            for m in RMS_MUTANTS:
                if rms_mutant_applies(m, shape):
                    r = E.ratio(E.budget_stats(rmsnorm_emul(x, gamma, RMS_EPS, mutant=m), ref, s, UNITS[dtype]), limits)
                    if m not in mut or r < mut[m][0]:
                        mut[m] = (r, shape, seed)
    return legit, raw, mut


def rel_margins(dtype, limits=None):
    limits = REL_LIMITS[dtype] if limits is None else limits
    legit, raw, mut = {k: 0.0 for k in E.STATS}, {k: 0.0 for k in E.STATS}, {}
    for seed in SEEDS:
        for case in rel_cases():
            heads, d, nk, rpe, _ = case
            q, k, v, ln, pos, bias, center = rel_operands(case, dtype, seed)
            scale = d ** -0.5
            ref, s = relbias_ref64(q, k, v, ln, pos, bias, center, heads, rpe, scale)
            for order in REL_ORDERS:
                got = relbias_emul(q, k, v, ln, pos, bias, center, heads, rpe, scale, order=order)
                _fold(legit, raw, E.budget_stats(got, ref, s, UNITS[dtype]), limits)
            for m in REL_MUTANTS:
                if rel_mutant_applies(m, case, ln, pos, center, bias.shape[1]):
                    got = relbias_emul(q, k, v, ln, pos, bias, center, heads, rpe, scale, mutant=m)
                    r = E.ratio(E.budget_stats(got, ref, s, UNITS[dtype]), limits)
                    if m not in mut or r < mut[m][0]:
                        mut[m] = (r, case, seed)
    return legit, raw, mut


if __name__ == "__main__":
    for name, fn in (("rmsnorm", rms_margins), ("attn_relbias", rel_margins)):
        for dt in (torch.bfloat16, torch.float32):
            legit, raw, mut = fn(dt)
            print(name, dt, "\n  legit / allowance", {k: round(v, 3) for k, v in legit.items()}, "\n  raw worst", {k: round(v, 4) for k, v in raw.items()},
                  "\n  mutants", {m: (round(r[0], 2),) + r[1:] for m, r in mut.items()})
