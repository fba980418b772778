"""CLIP tokenizer front-end.

The reference tokenises inside diffusers (`CLIPTokenizer`, 77 tokens, BOS 49406, EOS = PAD =
49407).  The BPE vocabulary (`vocab.json` + `merges.txt`) ships with the HF
checkpoint, which is not available offline, so:
  * `CLIPBPETokenizer(vocab_dir)` implements the published CLIP byte-pair encoding and is
    used whenever a checkpoint directory provides the two files;
  * `HashTokenizer` is a deterministic stand-in for synthetic-weight runs: every lower-cased
    word piece maps to a stable id in [0, vocab-2).  It exists so that the run_aug entrypoint
    is runnable end to end without a checkpoint; it is NOT a CLIP vocabulary."""
import json
import os
import re
import unicodedata
import zlib
from functools import lru_cache

import numpy as np


class HashTokenizer:
    def __init__(self, vocab=49408, max_len=77, pad_id=None):
        self.vocab, self.max_len = vocab, max_len
        self.bos, self.eos = vocab - 2, vocab - 1
        self.pad = self.eos if pad_id is None else pad_id

    def __call__(self, text, max_len=None):
        max_len = max_len or self.max_len
        words = re.findall(r"[a-z0-9]+|[^\sa-z0-9]", (text or "").lower())
        ids = [self.bos] + [zlib.crc32(w.encode()) % (self.vocab - 2) for w in words][: max_len - 2] + [self.eos]
        ids += [self.pad] * (max_len - len(ids))
        return np.asarray(ids, np.int64)[None]


@lru_cache()
def _bytes_to_unicode():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


class CLIPBPETokenizer:
    def __init__(self, vocab_dir, max_len=77, pad_id=None):
        with open(os.path.join(vocab_dir, "vocab.json"), encoding="utf-8") as f:
            self.encoder = json.load(f)
        with open(os.path.join(vocab_dir, "merges.txt"), encoding="utf-8") as f:
            merges = f.read().strip().split("\n")[1:]
        self.ranks = {tuple(m.split()): i for i, m in enumerate(merges)}
        self.byte_enc = _bytes_to_unicode()
        self.max_len = max_len
        self.bos, self.eos = self.encoder["<|startoftext|>"], self.encoder["<|endoftext|>"]
        self.pad = self.eos if pad_id is None else pad_id      # HF CLIPTokenizer pads with EOS, OpenAI's clip.tokenize with 0
        # CLIP's pre-tokenisation pattern (openai/CLIP simple_tokenizer.py, transformers CLIPTokenizer): unicode letter /
        # number classes need the `regex` module -- `[a-z]+` would split accented sub-class names into punctuation tokens
        import regex
        self.pat = regex.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+",
                                 regex.IGNORECASE)
        self.cache = {}

    def _bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            out, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == a and word[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = tuple(out)
        self.cache[token] = word
        return word

    def __call__(self, text, max_len=None):
        max_len = max_len or self.max_len
        # CLIPTokenizer's normaliser (transformers: NFC, whitespace runs -> one space, lower-case; accents kept).  The slow
        # tokenizer's optional ftfy.fix_text pass (mojibake / HTML-entity repair) is NOT reproduced: it is the identity on
        # the ASCII prompts of the reference's prompt files.
        text = unicodedata.normalize("NFC", text or "")
        text = re.sub(r"\s+", " ", text).strip().lower()
        unk = self.encoder.get("<|endoftext|>")
        ids = []
        for tok in self.pat.findall(text):
            tok = "".join(self.byte_enc[b] for b in tok.encode("utf-8"))
            ids += [self.encoder.get(p, unk) for p in self._bpe(tok)]
        ids = [self.bos] + ids[: max_len - 2] + [self.eos]
        ids += [self.pad] * (max_len - len(ids))
        return np.asarray(ids, np.int64)[None]


def make_tokenizer(vocab_dir=None, vocab=49408, pad_id=None):
    if vocab_dir and os.path.exists(os.path.join(vocab_dir, "vocab.json")):
        return CLIPBPETokenizer(vocab_dir, pad_id=pad_id)
    return HashTokenizer(vocab, pad_id=pad_id)


# ---- BERT tokenizer of the BLIP-Diffusion Q-Former (subject category text, e.g. "bird") ----------------------
class BertHashTokenizer:
    """Stand-in for synthetic-weight runs ([CLS] words [SEP], no padding); NOT the bert-base-uncased vocabulary."""

    def __init__(self, vocab=30523):
        self.vocab = vocab
        self.cls, self.sep = (101, 102) if vocab > 1000 else (1, 2)

    def __call__(self, text):
        words = re.findall(r"[a-z0-9]+|[^\sa-z0-9]", (text or "").lower())
        lo = 1000 if self.vocab > 2000 else 3
        return np.asarray([self.cls] + [lo + zlib.crc32(w.encode()) % (self.vocab - lo) for w in words] + [self.sep], np.int64)[None]

    def decode(self, ids, skip_special_tokens=True):
        """Placeholder: a hash has no inverse and a synthetic-weight run has no vocabulary -- "t<id>" per token, so that captions of
        such a run are at least distinct and reproducible.  Special: everything below the first word id, and the two ids above
        the word range that the BLIP captioner appends ([DEC], [ENC])."""
        lo = 1000 if self.vocab > 2000 else 3
        ids = [int(i) for i in ids]
        if skip_special_tokens:
            ids = [i for i in ids if lo <= i < self.vocab]
        return " ".join(f"t{i}" for i in ids)


class BertWordPieceTokenizer:
    """bert-base-uncased WordPiece from the checkpoint's vocab.txt (lower-case, punctuation split, greedy
    longest-match-first with ## continuation pieces)."""

    def __init__(self, vocab_file):
        with open(vocab_file, encoding="utf-8") as f:
            self.vocab = {tok.rstrip("\n"): i for i, tok in enumerate(f)}
        self.cls, self.sep, self.unk = self.vocab["[CLS]"], self.vocab["[SEP]"], self.vocab["[UNK]"]

    def _pieces(self, word):
        out, start = [], 0
        while start < len(word):
            end, cur = len(word), None
            while start < end:
                sub = ("##" if start else "") + word[start:end]
                if sub in self.vocab:
                    cur = self.vocab[sub]
                    break
                end -= 1
            if cur is None:
                return [self.unk]
            out.append(cur)
            start = end
        return out

    def __call__(self, text):
        ids = [self.cls]
        for w in re.findall(r"[a-z0-9]+|[^\sa-z0-9]", (text or "").lower()):
            ids += self._pieces(w)
        return np.asarray(ids + [self.sep], np.int64)[None]

    # transformers' clean_up_tokenization (tokenization_utils_base), in its order
    _CLEAN_UP = ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"), (" 's", "'s"),
                 (" 've", "'ve"), (" 're", "'re"))
    SPECIAL = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[DEC]", "[ENC]")

    def decode(self, ids, skip_special_tokens=True, clean_up_tokenization_spaces=True):
        """ids -> text as transformers.BertTokenizer.decode does it: the pieces joined with spaces, " ##" removed, then the clean-up
        rules.  Special tokens ([PAD] [UNK] [CLS] [SEP] [MASK], BLIP's [DEC] / [ENC], and ids beyond the vocabulary file, which
        is where a checkpoint puts [DEC] / [ENC] when vocab.txt lacks them) are skipped."""
        if not hasattr(self, "_inv"):
            self._inv = {i: t for t, i in self.vocab.items()}
        toks = []
        for i in ids:
            t = self._inv.get(int(i))
            if skip_special_tokens and (t is None or t in self.SPECIAL):
                continue
            toks.append("[UNK]" if t is None else t)
        text = " ".join(toks).replace(" ##", "").strip()
        if clean_up_tokenization_spaces:
            for a, b in self._CLEAN_UP:
                text = text.replace(a, b)
        return text


def make_bert_tokenizer(vocab_dir=None, vocab=30523):
    if vocab_dir and os.path.exists(os.path.join(vocab_dir, "vocab.txt")):
        return BertWordPieceTokenizer(os.path.join(vocab_dir, "vocab.txt"))
    return BertHashTokenizer(vocab)


# ---- T5 Unigram tokenizer of the key-to-text generator (txt2sentence.py) --------------------------------------------------------
class UnigramTokenizer:
    """SentencePiece Unigram as T5 uses it, from the checkpoint's `tokenizer.json` (plain JSON: model.vocab = [[piece, score], ...],
    model.unk_id): NFKC normalisation, whitespace collapsed, every word prefixed with U+2581, then per word the segmentation of
    highest total score (Viterbi over the piece scores; the first best path wins a tie; a character no piece covers costs the lowest
    score - 10 and runs of such characters fuse into one <unk>, as `tokenizers`' Unigram does), and `</s>` appended.  decode() joins the
    pieces and turns U+2581 back into spaces.

    APPROXIMATED: SentencePiece normalises with a precompiled character map (nmt_nfkc); here that is `unicodedata.normalize("NFKC")`.
    The two agree on ASCII and Latin-1 text (tests/test_t5_host.py compares ids with `tokenizers` on such input) and may differ on
    rarer code points (some control and zero-width characters).

    Without a tokenizer.json (a synthetic-weight run has no vocabulary) it is a hash stand-in like the other towers': every
    lower-cased word maps to a stable id above the special ids, decode() writes "t<id>" per token.  NOT a T5 vocabulary."""

    SPACE = "▁"

    def __init__(self, path=None, vocab_size=32128, eos=1, pad=0):
        self.eos, self.pad = eos, pad
        self.pieces = None
        self.vocab_size = vocab_size
        if path is None:
            return
        with open(path, encoding="utf-8") as f:
            tj = json.load(f)
        model = tj["model"]
        if model.get("type", "Unigram") != "Unigram":
            raise ValueError(f"{path}: a {model.get('type')} tokenizer, not Unigram")
        self.vocab = [(p, float(s)) for p, s in model["vocab"]]
        self.vocab_size = len(self.vocab)
        self.unk = model.get("unk_id")
        self.pieces = {}
        for i, (p, s) in enumerate(self.vocab):
            self.pieces.setdefault(p, (i, s))
        self.max_piece = max(len(p) for p, _ in self.vocab)
        self.unk_score = min(s for _, s in self.vocab) - 10.0
        self.special = {p for p in ("<pad>", "</s>", "<unk>")} | {t["content"] for t in tj.get("added_tokens", []) if t.get("special")}
        if "</s>" in self.pieces:
            self.eos = self.pieces["</s>"][0]

    @classmethod
    def normalize(cls, text):
        return " ".join(unicodedata.normalize("NFKC", text or "").split())

    def _word(self, w):
        """Viterbi over one word (already prefixed): -> ids."""
        n = len(w)
        best = [(-1e300, -1, -1)] * (n + 1)          # (score, start, id) of the best path ending at i
        best[0] = (0.0, -1, -1)
        for b in range(n):
            sb = best[b][0]
            if sb <= -1e300:
                continue
            single = False
            for e in range(b + 1, min(n, b + self.max_piece) + 1):
                hit = self.pieces.get(w[b:e])
                if hit is None:
                    continue
                single = single or e == b + 1
                if sb + hit[1] > best[e][0]:
                    best[e] = (sb + hit[1], b, hit[0])
            if not single and sb + self.unk_score > best[b + 1][0]:
                best[b + 1] = (sb + self.unk_score, b, self.unk)
        ids, i = [], n
        while i > 0:
            _, b, t = best[i]
            ids.append(t)
            i = b
        ids.reverse()
        fused = []
        for t in ids:                                 # runs of <unk> fuse
            if not (t == self.unk and fused and fused[-1] == self.unk):
                fused.append(t)
        return fused

    def encode(self, text, add_eos=True):
        """text -> list of ids, `</s>` appended."""
        words = self.normalize(text).split(" ") if self.normalize(text) else []
        if self.pieces is None:
            lo = 3
            ids = [lo + zlib.crc32(w.lower().encode()) % (self.vocab_size - lo) for w in words]
        else:
            ids = [t for w in words for t in self._word(self.SPACE + w)]
        return ids + ([self.eos] if add_eos else [])

    def __call__(self, text):
        return np.asarray(self.encode(text), np.int64)[None]

    def decode(self, ids, skip_special_tokens=True):
        ids = [int(i) for i in ids]
        if self.pieces is None:
            return " ".join(f"t{i}" for i in ids if not (skip_special_tokens and i < 3))
        out = []
        for i in ids:
            p = self.vocab[i][0] if 0 <= i < len(self.vocab) else "<unk>"
            if skip_special_tokens and p in self.special:
                continue
            out.append(p)
        return "".join(out).replace(self.SPACE, " ").strip()
