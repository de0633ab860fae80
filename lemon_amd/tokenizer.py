"""Byte-pair-encoding tokenizer of the CLIP family, for the tokenizer call of the hot path
(run_lemon.py:149,151-154,183,186-189,220,222-226).

Two call conventions the reference uses, both served from ONE merges table:
  * `tokenize(texts, model)`            lib/models/chexzero_clip.py:481-493 (the in-tree CLIP branches of
    lib/models/utils.py:82-103): LongTensor [n, model.context_length], SOT + BPE ids + EOT, zero padded, over-long
    prompts cut to the context length with EOT forced into the last slot;
  * `tokenizer(list[str], padding="max_length", truncation=True)`  the HF CLIPTokenizer(Fast) call of the
    'huggingface_clip' branch: dict of lists, padded with the EOT id (openai/clip-vit-* use <|endoftext|> as pad),
    truncated to 77 with EOT last.
The BPE itself follows the published CLIP algorithm (OpenAI CLIP `simple_tokenizer.py`, which
lib/models/simple_tokenizer.py:86-156 vendors): lower-case, whitespace-collapse, split with the CLIP pattern,
bytes -> printable code points, then merge the lowest-ranked adjacent pair until none is ranked.

The merges table is DATA the user supplies (`bpe_simple_vocab_16e6.txt.gz`, or HF's `merges.txt`): nothing is
downloaded and no vocabulary ships with this package.  Text cleaning: `ftfy.fix_text` when ftfy is importable
(the reference requires it, simple_tokenizer.py:30,74-77), otherwise skipped -- identical on clean UTF-8 text.
"""
import gzip
import html
import os
import sys
from functools import lru_cache

import regex as re

SOT, EOT = "<|startoftext|>", "<|endoftext|>"
N_MERGES = 49152 - 256 - 2            # merges kept from the 16e6 vocabulary file (simple_tokenizer.py:91)
_PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""


@lru_cache()
def byte_alphabet():
    """byte -> printable unicode character (the 256 base symbols), in vocabulary order: the 188 printable latin-1
    bytes keep their own code point, the 68 others are mapped to 256, 257, ..."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    order, chars, extra = list(keep), [chr(b) for b in keep], 0
    for b in range(256):
        if b not in keep:
            order.append(b)
            chars.append(chr(256 + extra))
            extra += 1
    return dict(zip(order, chars))


def read_merges(path):
    """Merge rules in rank order from `bpe_simple_vocab_16e6.txt(.gz)` (header line + 'a b' lines; the first
    N_MERGES are used) or from an HF `merges.txt` (same format, already cut)."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        lines = f.read().decode("utf-8").split("\n")
    lines = lines[1:N_MERGES + 1]
    return [tuple(l.split()) for l in lines if len(l.split()) == 2]


class ClipBPE:
    """encode(text) -> list of ids.  `merges`: [(first, second), ...] in rank order, or {(first, second): rank}
    (a sparse table is enough to tokenise texts whose merge paths it covers: the tests' subset fixture)."""

    def __init__(self, merges):
        ranks = dict(merges) if isinstance(merges, dict) else {tuple(m): i for i, m in enumerate(merges)}
        self.ranks = ranks
        alphabet = list(byte_alphabet().values())
        self.encoder = {c: i for i, c in enumerate(alphabet)}
        self.encoder.update({c + "</w>": 256 + i for i, c in enumerate(alphabet)})
        for (a, b), r in sorted(ranks.items(), key=lambda kv: kv[1]):
            self.encoder[a + b] = 512 + r
        self.sot_id = 512 + N_MERGES
        self.eot_id = self.sot_id + 1
        self.encoder[SOT], self.encoder[EOT] = self.sot_id, self.eot_id
        self.vocab_size = self.eot_id + 1
        self._cache = {SOT: (SOT,), EOT: (EOT,)}
        self._pat = re.compile(_PATTERN, re.IGNORECASE)
        self._bytes = byte_alphabet()

    @classmethod
    def from_file(cls, path):
        return cls(read_merges(path))

    def _bpe(self, token):
        hit = self._cache.get(token)
        if hit is not None:
            return hit
        word = list(token[:-1]) + [token[-1] + "</w>"]
        while len(word) > 1:
            best, best_rank = None, None
            for pair in zip(word[:-1], word[1:]):
                r = self.ranks.get(pair)
                if r is not None and (best_rank is None or r < best_rank):
                    best, best_rank = pair, r
            if best is None:
                break
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == best[0] and word[i + 1] == best[1]:
                    merged.append(best[0] + best[1])
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        out = tuple(word)
        self._cache[token] = out
        return out

    @staticmethod
    def clean(text):
        try:
            import ftfy
            text = ftfy.fix_text(text)
        except ImportError:
            pass
        text = html.unescape(html.unescape(text)).strip()
        return re.sub(r"\s+", " ", text).strip().lower()

    def encode(self, text):
        ids = []
        for tok in re.findall(self._pat, self.clean(text)):
            tok = "".join(self._bytes[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self._bpe(tok))
        return ids


def tokenize(texts, model_or_context_length, bpe):
    """lib/models/chexzero_clip.py:481-493: LongTensor [n, context_length], zero padded."""
    import torch
    ctx = model_or_context_length if isinstance(model_or_context_length, int) else model_or_context_length.context_length
    out = torch.zeros(len(texts), ctx, dtype=torch.long)
    for i, t in enumerate(texts):
        ids = [bpe.sot_id] + bpe.encode(t) + [bpe.eot_id]
        if len(ids) > ctx:
            ids = ids[:ctx]
            ids[ctx - 1] = bpe.eot_id
        out[i, :len(ids)] = torch.tensor(ids)
    return out


class HFStyleClipTokenizer:
    """The call the 'huggingface_clip' branch makes (run_lemon.py:151-154): tokenizer(texts, padding="max_length",
    truncation=True) -> {"input_ids": [[...]], "attention_mask": [[...]]}, padded to 77 with the EOT id like
    openai/clip-vit-* tokenizers, built from a local merges file when no HF tokenizer directory is available."""

    def __init__(self, bpe, context_length=77):
        self.bpe, self.model_max_length = bpe, context_length

    def __call__(self, texts, padding="max_length", truncation=True, **_):
        ctx = self.model_max_length
        ids_all, mask_all = [], []
        for t in texts:
            ids = [self.bpe.sot_id] + self.bpe.encode(t) + [self.bpe.eot_id]
            if truncation and len(ids) > ctx:
                ids = ids[:ctx - 1] + [self.bpe.eot_id]
            n = len(ids)
            if padding == "max_length":
                ids = ids + [self.bpe.eot_id] * (ctx - n)
            ids_all.append(ids)
            mask_all.append([1] * n + [0] * (len(ids) - n))
        return {"input_ids": ids_all, "attention_mask": mask_all}


def find_bpe_file(hint=None):
    """Merges file from, in order: the explicit hint (file, or a directory holding merges.txt /
    bpe_simple_vocab_16e6.txt.gz), $LEMON_BPE_PATH.  None when nothing is found."""
    for cand in (hint, os.environ.get("LEMON_BPE_PATH")):
        if not cand:
            continue
        if os.path.isdir(cand):
            for fn in ("bpe_simple_vocab_16e6.txt.gz", "merges.txt"):
                if os.path.exists(os.path.join(cand, fn)):
                    return os.path.join(cand, fn)
        elif os.path.exists(cand):
            return cand
    return None


# ---- BERT WordPiece: the tokenizer of the `biomed_clip` branch (lib/models/utils.py:74; run_lemon.py:148-149) ------------------
# open_clip's `get_tokenizer('hf-hub:microsoft/BiomedCLIP-...')` is an HFTokenizer around the checkpoint's BERT uncased
# tokenizer, called as `tokenizer(texts)` -> LongTensor [n, 256]: whitespace-cleaned text, [CLS] pieces [SEP], cut to the
# context length ([SEP] kept last), padded with [PAD].  The algorithm is the published BERT one (BasicTokenizer: clean, CJK
# spacing, lower-case + accent stripping, punctuation split; then greedy longest-match-first WordPiece with '##' continuations),
# restated here from its description; tests/test_biomed.py compares it with `transformers.BertTokenizer`, token for token.  The vocabulary (vocab.txt of the checkpoint) is DATA the user supplies.
import unicodedata


def _is_punct(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp):
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class BertWordPiece:
    """tokenizer(texts, context_length=None) -> LongTensor [n, context_length] (open_clip HFTokenizer.__call__)."""

    def __init__(self, vocab, context_length=256, lower_case=True, max_chars_per_word=100):
        self.vocab = dict(vocab) if isinstance(vocab, dict) else {t: i for i, t in enumerate(vocab)}
        self.context_length, self.lower_case, self.max_chars = context_length, lower_case, max_chars_per_word
        for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"):
            if t not in self.vocab:
                raise ValueError(f"vocabulary lacks {t}")
        self.pad, self.unk, self.cls, self.sep = (self.vocab[t] for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"))
        self.never_split = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"}

    @classmethod
    def from_file(cls, path, context_length=256, lower_case=True):
        with open(path, encoding="utf-8") as f:
            toks = [l.rstrip("\n") for l in f]
        while toks and toks[-1] == "":
            toks.pop()
        return cls(toks, context_length, lower_case)

    # -- BasicTokenizer --
    def _clean(self, text):
        out = []
        for ch in text:
            cp = ord(ch)
            cat = unicodedata.category(ch)
            if cp == 0 or cp == 0xFFFD or (cat.startswith("C") and ch not in "\t\n\r"):
                continue
            out.append(" " if ch in " \t\n\r" or cat == "Zs" else ch)
        return "".join(out)

    def _split_word(self, w):
        if self.lower_case and w not in self.never_split:
            w = "".join(c for c in unicodedata.normalize("NFD", w.lower()) if unicodedata.category(c) != "Mn")
        if w in self.never_split:
            return [w]
        parts, cur = [], ""
        for ch in w:
            if _is_punct(ch):
                if cur:
                    parts.append(cur)
                parts.append(ch)
                cur = ""
            else:
                cur += ch
        if cur:
            parts.append(cur)
        return parts

    def basic(self, text):
        text = self._clean(text)
        text = "".join(f" {c} " if _is_cjk(ord(c)) else c for c in text)
        text = unicodedata.normalize("NFC", text)
        return [p for w in text.split() for p in self._split_word(w)]

    def wordpiece(self, word):
        if len(word) > self.max_chars:
            return [self.unk]
        ids, start = [], 0
        while start < len(word):
            end, hit = len(word), None
            while start < end:
                piece = ("##" if start else "") + word[start:end]
                if piece in self.vocab:
                    hit = self.vocab[piece]
                    break
                end -= 1
            if hit is None:
                return [self.unk]
            ids.append(hit)
            start = end
        return ids

    def encode(self, text):
        """ids without the special tokens"""
        return [i for w in self.basic(text) for i in self.wordpiece(w)]

    @staticmethod
    def clean_text(text):
        # open_clip's default `clean='whitespace'`: basic_clean (ftfy.fix_text when importable, html.unescape twice) + whitespace
        # collapse -- ftfy skipped when absent, as for the CLIP BPE above
        try:
            import ftfy
            text = ftfy.fix_text(text)
        except ImportError:
            pass
        text = html.unescape(html.unescape(text)).strip()
        return " ".join(text.split())

    def __call__(self, texts, context_length=None):
        import torch
        if isinstance(texts, str):
            texts = [texts]
        ctx = context_length or self.context_length
        out = torch.full((len(texts), ctx), self.pad, dtype=torch.long)
        for r, t in enumerate(texts):
            ids = [self.cls] + self.encode(self.clean_text(str(t)))[:ctx - 2] + [self.sep]
            out[r, :len(ids)] = torch.tensor(ids, dtype=torch.long)
        return out


def find_vocab_file(hint=None):
    """vocab.txt of a BERT tokenizer: `hint` (file, or a directory holding it), else $LEMON_VOCAB_PATH."""
    for h in (hint, os.environ.get("LEMON_VOCAB_PATH")):
        if not h:
            continue
        if os.path.isfile(h) and not h.endswith((".bin", ".pt", ".safetensors")):
            return h
        d = h if os.path.isdir(h) else os.path.dirname(h)
        if d and os.path.isfile(os.path.join(d, "vocab.txt")):
            return os.path.join(d, "vocab.txt")
    return None


# ---- the same tokenizers on the device (include/lemon_hip.h: lemon_tokenize), opt-in with LEMON_TOKENIZE=device -----------------
# The captions cross PCIe as raw bytes and the id matrix is written in HBM, where Embedder.embed_texts reads it.  The device serves
# the rows on which text cleaning is the identity up to whitespace and ASCII case (printable ASCII without '&' and "<|"); every
# other row comes back with a status and is tokenised here, by the host tokenizer itself, and scattered into the matrix.
class ClipTokenize:
    """`tokenizer(texts)` of the in-tree CLIP branches: tokenize(texts, context_length, bpe) -> LongTensor [n, context_length]."""

    def __init__(self, bpe, context_length):
        self.bpe, self.context_length = bpe, context_length

    def __call__(self, texts):
        return tokenize(texts, self.context_length, self.bpe)


def tokenize_mode():
    """$LEMON_TOKENIZE: 'host' (default) or 'device'."""
    mode = os.environ.get("LEMON_TOKENIZE", "host")
    if mode not in ("host", "device"):
        raise ValueError(f"LEMON_TOKENIZE={mode!r}: host or device")
    return mode


def _ftfy_present():
    import importlib.util
    try:
        return importlib.util.find_spec("ftfy") is not None
    except (ImportError, ValueError):
        return True


def bpe_id_table(bpe):
    """(left, right, rank, merged) int32 arrays of the merges that can fire -- both parts and the result have an id in
    `bpe.encoder` --, or None when the ids do not fit the device table (16 bits) or two symbols share an id."""
    import numpy as np
    enc = bpe.encoder
    if max(enc.values()) >= 65535 or len(set(enc.values())) != len(enc):
        return None
    rows = [(enc[a], enc[b], r, enc[a + b]) for (a, b), r in bpe.ranks.items() if a in enc and b in enc and 0 <= r < 2 ** 31]
    arr = np.array(rows, dtype=np.int32).reshape(-1, 4)
    return tuple(np.ascontiguousarray(arr[:, c]) for c in range(4))


class DeviceTokenizer:
    """texts -> LongTensor [n, context_length] on `device`, equal to the host tokenizer's matrix.  After a call: `lengths`
    (int32 [n], tokens before the padding) and `declined` (rows the device handed back, tokenised on the host)."""

    def __init__(self, host, device, home_buckets=0):
        import ctypes
        import numpy as np
        import torch
        from . import _lib
        self.host, self.device, self.lib = host, torch.device(device), _lib.load()
        self.handle, self.lengths, self.declined = ctypes.c_void_p(), None, 0
        if isinstance(host, BertWordPiece):
            self.ctx, self.pad = host.context_length, host.pad
            toks = [t.encode("utf-8", "surrogatepass") for t in host.vocab]
            offsets = np.zeros(len(toks) + 1, dtype=np.int64)
            np.cumsum([len(t) for t in toks], out=offsets[1:])
            blob = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8)
            ids = np.fromiter(host.vocab.values(), dtype=np.int64, count=len(toks))
            if ids.min(initial=0) < 0 or ids.max(initial=0) >= 65535:
                raise ValueError("vocabulary ids do not fit the device table")
            ids = ids.astype(np.int32)
            rc = self.lib.lemon_tokenizer_create_wordpiece(blob.ctypes.data, offsets.ctypes.data, ids.ctypes.data, len(toks), host.cls, host.sep,
                                                           host.unk, int(bool(host.lower_case)), min(int(host.max_chars), 2 ** 30), home_buckets,
                                                           ctypes.byref(self.handle))
        else:
            self.ctx = host.model_max_length if isinstance(host, HFStyleClipTokenizer) else host.context_length
            self.pad = host.bpe.eot_id if isinstance(host, HFStyleClipTokenizer) else 0
            table = bpe_id_table(host.bpe)
            if table is None:
                raise ValueError("vocabulary ids do not fit the device table")
            left, right, rank, merged = table
            rc = self.lib.lemon_tokenizer_create_bpe(left.ctypes.data, right.ctypes.data, rank.ctypes.data, merged.ctypes.data, len(left),
                                                     host.bpe.sot_id, host.bpe.eot_id, ctypes.byref(self.handle))
        _lib.check(rc, "lemon_tokenizer_create")

    def __del__(self):
        if getattr(self, "handle", None) and not sys.is_finalizing():      # at interpreter exit the runtime frees the table
            self.lib.lemon_tokenizer_free(self.handle)
            self.handle = None

    def table_info(self):
        """(slots, entries, longest probe sequence) of the hash table"""
        import ctypes
        from . import _lib
        slots, entries, probe = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _lib.check(self.lib.lemon_tokenizer_table_info(self.handle, ctypes.byref(slots), ctypes.byref(entries), ctypes.byref(probe)), "lemon_tokenizer_table_info")
        return slots.value, entries.value, probe.value

    @staticmethod
    def pack(texts):
        """(offsets int64 [n + 1], bytes): the rows' UTF-8 bytes back to back"""
        import numpy as np
        texts = [t if isinstance(t, str) else str(t) for t in texts]
        blob = "".join(texts).encode("utf-8", "surrogatepass")
        offsets = np.zeros(len(texts) + 1, dtype=np.int64)
        if len(blob) == sum(map(len, texts)):                        # ASCII only: a character is a byte
            np.cumsum(np.fromiter(map(len, texts), dtype=np.int64, count=len(texts)), out=offsets[1:])
        else:
            np.cumsum([len(t.encode("utf-8", "surrogatepass")) for t in texts], out=offsets[1:])
        return offsets, blob

    def host_rows(self, texts):
        """(ids LongTensor [m, ctx], lengths int32 [m]) from the host tokenizer"""
        import torch
        if isinstance(self.host, HFStyleClipTokenizer):
            enc = self.host(texts, padding="max_length", truncation=True)
            return torch.tensor(enc["input_ids"], dtype=torch.long), torch.tensor(enc["attention_mask"]).sum(-1).to(torch.int32)
        ids = self.host(texts)
        last = ids.shape[1] - 1 - (ids.flip(1) != self.pad).to(torch.int32).argmax(1)       # the last token is never the padding id
        return ids, (last + 1).to(torch.int32)

    def tokenize_host_loop(self, texts, ctx=None, pad=None):
        """lemon_tokenize_host on the same packed input: (ids int64 [n, ctx], length int32 [n], status uint8 [n]) as numpy arrays.
        Test support where there is no GPU."""
        import numpy as np
        from . import _lib
        ctx, pad = ctx or self.ctx, self.pad if pad is None else pad
        offsets, blob = self.pack(texts)
        n = len(offsets) - 1
        text = np.frombuffer(blob or b"\0", dtype=np.uint8)
        ids, length, status = np.full((n, ctx), -7, np.int64), np.full(n, -7, np.int32), np.full(n, 255, np.uint8)
        _lib.check(self.lib.lemon_tokenize_host(self.handle, text.ctypes.data, len(blob), offsets.ctypes.data, n, ctx, pad, ids.ctypes.data,
                                                length.ctypes.data, status.ctypes.data), "lemon_tokenize_host")
        return ids, length, status

    def __call__(self, texts, **_):
        import numpy as np
        import torch
        from . import _lib
        from .ops import ptr, stream_ptr
        if isinstance(texts, str):
            texts = [texts]
        n, ctx, dev = len(texts), self.ctx, self.device
        ids = torch.empty((n, ctx), dtype=torch.long, device=dev)
        self.lengths, self.declined = torch.zeros(n, dtype=torch.int32), 0
        if n == 0:
            return ids
        offsets, blob = self.pack(texts)
        head = offsets.nbytes                                             # one upload: the offsets, then the text
        staged = torch.from_numpy(np.concatenate([offsets.view(np.uint8), np.frombuffer(blob, dtype=np.uint8)])).to(dev)
        back = torch.empty(5 * n, dtype=torch.uint8, device=dev)          # one read-back: int32 lengths, then uint8 statuses
        with torch.cuda.device(dev):
            _lib.check(self.lib.lemon_tokenize(self.handle, staged.data_ptr() + head, len(blob), ptr(staged), n, ctx, self.pad, ptr(ids), ptr(back),
                                               back.data_ptr() + 4 * n, stream_ptr(dev)), "lemon_tokenize")
        back = back.cpu()
        lengths, status = back[:4 * n].view(torch.int32).clone(), back[4 * n:]
        rows = torch.nonzero(status).squeeze(1)
        if len(rows):
            host_ids, host_len = self.host_rows([texts[i] for i in rows.tolist()])
            ids[rows.to(dev)] = host_ids.to(dev)
            lengths[rows] = host_len
        self.lengths, self.declined = lengths, len(rows)
        return ids


def device_form(host_tokenizer, device):
    """The device form of a host tokenizer -- ClipTokenize, HFStyleClipTokenizer or BertWordPiece --: a callable texts ->
    LongTensor [n, context] on `device` with the host's ids.  None when there is none: another tokenizer class, `ftfy`
    importable (the host tokenizers then rewrite text in ways the device does not), a context length or a vocabulary that
    does not fit the device tables."""
    if not isinstance(host_tokenizer, (ClipTokenize, HFStyleClipTokenizer, BertWordPiece)) or _ftfy_present():
        return None
    ctx = host_tokenizer.model_max_length if isinstance(host_tokenizer, HFStyleClipTokenizer) else host_tokenizer.context_length
    if not 2 <= ctx <= 1024:                      # LEMON_TOKENIZE_MAX_CTX
        return None
    from ._lib import LemonHipError
    try:
        return DeviceTokenizer(host_tokenizer, device)
    except (ValueError, LemonHipError):
        return None
