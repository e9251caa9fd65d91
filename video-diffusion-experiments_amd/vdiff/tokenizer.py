"""CLIP's byte-level BPE tokenizer in pure Python, from local `vocab.json` + `merges.txt`
(the `tokenizer/` folder of an SD-1.5 directory): what transformers.CLIPTokenizer computes for
diffusers' `encode_prompt` — `tokenizer(prompt, padding="max_length", max_length=77,
truncation=True, return_tensors="pt").input_ids`.

Text handling, in transformers' order: special tokens (`<|startoftext|>`, `<|endoftext|>`) are
cut out of the raw text first; the rest is NFC-normalised, every whitespace run becomes one
space, and it is lower-cased; words are the matches of CLIP's split pattern

    's|'t|'re|'ve|'m|'ll|'d|[\\p{L}]+|[\\p{N}]|[^\\s\\p{L}\\p{N}]+

(whitespace is dropped); each word's UTF-8 bytes map to the GPT-2 byte alphabet, the last symbol
gets the `</w>` suffix, and the merges are applied lowest rank first.  There is no `ftfy` text
repair (transformers falls back the same way without it) and nothing is ever downloaded.

The `regex` module supplies \\p{L} / \\p{N} when it can be imported.  Without it the standard
`re` stands in: letters are `[^\\W\\d_]`, numbers `\\d`.  That is exact for ASCII text; outside it
the numbers are the decimal digits only, so characters such as '²' or '½' (\\p{No}) and 'Ⅷ' (\\p{Nl})
fall into the punctuation class instead of standing alone, and a few combining marks count as
letters.
"""
from __future__ import annotations

import json
import unicodedata
from pathlib import Path

try:
    import regex as _re
    _WORD = r"'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"
    HAVE_REGEX = True
except ImportError:  # ASCII-correct fallback (module docstring)
    import re as _re
    _WORD = r"'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+"
    HAVE_REGEX = False

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
EOW = "</w>"


def bytes_to_unicode() -> dict:
    """GPT-2's byte alphabet: printable latin-1 bytes stand for themselves, the other 68 bytes
    take the code points from 256 up."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


class BatchEncoding(dict):
    """{"input_ids", "attention_mask"} with attribute access, as transformers returns."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    def to(self, device):
        return BatchEncoding({k: v.to(device) if hasattr(v, "to") else v for k, v in self.items()})


def _token_content(v):
    return v.get("content") if isinstance(v, dict) else v


class CLIPTokenizer:
    def __init__(self, vocab: dict, merges: list, bos_token=BOS, eos_token=EOS, pad_token=None, unk_token=EOS,
                 model_max_length: int = 77):
        self.encoder = dict(vocab)
        self.bpe_ranks = {tuple(m): i for i, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        self.bos_token, self.eos_token, self.unk_token = bos_token, eos_token, unk_token
        self.pad_token = pad_token or eos_token
        for t in (self.bos_token, self.eos_token, self.pad_token, self.unk_token):
            if t not in self.encoder:
                raise KeyError(f"special token {t!r} is not in the vocabulary")
        self.bos_token_id, self.eos_token_id = self.encoder[self.bos_token], self.encoder[self.eos_token]
        self.pad_token_id, self.unk_token_id = self.encoder[self.pad_token], self.encoder[self.unk_token]
        self.model_max_length = int(model_max_length)
        self._specials = sorted({self.bos_token, self.eos_token}, key=len, reverse=True)
        self._special_pat = _re.compile("(" + "|".join(_re.escape(s) for s in self._specials) + ")")
        self._word_pat = _re.compile(_WORD)
        self._cache = {}

    @classmethod
    def from_pretrained(cls, path, **unused):
        """A LOCAL folder holding vocab.json and merges.txt (and, optionally, tokenizer_config.json /
        special_tokens_map.json for the pad token and model_max_length)."""
        d = Path(path)
        if not d.is_dir():
            raise FileNotFoundError(f"CLIPTokenizer.from_pretrained: {path!r} is not a local directory (hub "
                                    "checkpoints are unreachable offline: pass a folder with vocab.json + merges.txt)")
        with open(d / "vocab.json", encoding="utf-8") as f:
            vocab = json.load(f)
        merges = []
        with open(d / "merges.txt", encoding="utf-8") as f:
            for line in f.read().split("\n"):
                if not line or line.startswith("#version"):
                    continue
                parts = line.split()
                if len(parts) == 2:
                    merges.append((parts[0], parts[1]))
        kw = {}
        for name in ("special_tokens_map.json", "tokenizer_config.json"):  # the config wins
            p = d / name
            if not p.exists():
                continue
            with open(p, encoding="utf-8") as f:
                cfg = json.load(f)
            for k in ("bos_token", "eos_token", "pad_token", "unk_token"):
                if _token_content(cfg.get(k)):
                    kw[k] = _token_content(cfg[k])
            mml = cfg.get("model_max_length")
            if isinstance(mml, int) and 0 < mml < 1 << 20:
                kw["model_max_length"] = mml
        return cls(vocab, merges, **kw)

    def __len__(self):
        return len(self.encoder)

    # ------------------------------------------------------------------ BPE
    def bpe(self, word: str) -> list:
        """The merged symbols of one pre-token (already in the byte alphabet)."""
        if word in self._cache:
            return self._cache[word]
        sym = list(word[:-1]) + [word[-1] + EOW]
        while len(sym) > 1:
            best, at = None, -1
            for i in range(len(sym) - 1):
                r = self.bpe_ranks.get((sym[i], sym[i + 1]))
                if r is not None and (best is None or r < best):
                    best, at = r, i
            if best is None:
                break
            a, b = sym[at], sym[at + 1]
            out, i = [], 0
            while i < len(sym):  # every occurrence of the best pair, left to right
                if i + 1 < len(sym) and sym[i] == a and sym[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(sym[i])
                    i += 1
            sym = out
        self._cache[word] = sym
        return sym

    def tokenize(self, text: str) -> list:
        toks = []
        for part in self._special_pat.split(text):
            if part in self._specials:
                toks.append(part)
                continue
            part = unicodedata.normalize("NFC", part)
            part = _re.sub(r"\s+", " ", part).lower()
            for w in self._word_pat.findall(part):
                toks.extend(self.bpe("".join(self.byte_encoder[b] for b in w.encode("utf-8"))))
        return toks

    def convert_tokens_to_ids(self, tokens):
        return [self.encoder.get(t, self.unk_token_id) for t in tokens]

    def encode(self, text: str, max_length=None, truncation=True, add_special_tokens=True) -> list:
        ids = self.convert_tokens_to_ids(self.tokenize(text))
        n = self.model_max_length if max_length is None else int(max_length)
        if not add_special_tokens:
            return ids[:n] if truncation else ids
        if truncation and len(ids) > n - 2:
            ids = ids[:max(n - 2, 0)]  # the framing survives: the last token stays eos
        return [self.bos_token_id] + ids + [self.eos_token_id]

    def __call__(self, text, padding="max_length", max_length=None, truncation=True, return_tensors="pt", **unused):
        texts = [text] if isinstance(text, str) else list(text)
        n = self.model_max_length if max_length is None else int(max_length)
        rows = [self.encode(t, max_length=n, truncation=truncation) for t in texts]
        if padding in (True, "longest"):
            width = max(len(r) for r in rows)
        elif padding == "max_length":
            width = n
        elif padding in (False, None, "do_not_pad"):
            width = None
        else:
            raise ValueError(f"padding {padding!r}: 'max_length', 'longest' / True or 'do_not_pad' / False")
        mask = [[1] * len(r) for r in rows]
        if width is not None:
            mask = [m + [0] * (width - len(m)) for m in mask]
            rows = [r + [self.pad_token_id] * (width - len(r)) for r in rows]
        if return_tensors == "pt":
            import torch
            if len({len(r) for r in rows}) > 1:
                raise ValueError("return_tensors='pt' needs rows of one length: pad or truncate")
            rows, mask = torch.tensor(rows, dtype=torch.long), torch.tensor(mask, dtype=torch.long)
        elif return_tensors is not None:
            raise ValueError(f"return_tensors {return_tensors!r}: 'pt' or None")
        elif isinstance(text, str):
            rows, mask = rows[0], mask[0]
        return BatchEncoding(input_ids=rows, attention_mask=mask)
