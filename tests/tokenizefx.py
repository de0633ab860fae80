"""Vocabularies and seeded corpora shared by tests/test_tokenize_device_host.py and tests/test_gpu_tokenize.py.  Everything is
generated: the only file read is tests/golden/tokenizer.npz (the texts and the sparse merges table that tests/test_tokenizer.py
pins to the reference's SimpleTokenizer).  The yardstick is always lemon_amd/tokenizer.py's Python classes."""
import functools
import os

import numpy as np

from lemon_amd.tokenizer import BertWordPiece, ClipBPE, ClipTokenize, HFStyleClipTokenizer

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "tokenizer.npz"))
TEXTS = [str(t) for t in FX["texts"]]
# the four fixture texts outside the envelope and the status each must get (include/lemon_hip.h: LEMON_TOK_*)
DECLINED = {40: 1, 41: 1, 46: 3, 47: 2}          # accents, emoji, a literal <|startoftext|>, an '&'
SPACES = " \t\n\r"
PUNCT = "!\"#$%'()*+,-./:;<=>?@[\\]^_`{|}~"       # no '&'
LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
DIGITS = "0123456789"


def in_envelope(text):
    return all(c in SPACES or 33 <= ord(c) <= 126 for c in text) and "&" not in text and "<|" not in text


def fixture_bpe():
    return ClipBPE({(str(a), str(b)): int(r) for a, b, r in zip(FX["merge_first"], FX["merge_second"], FX["merge_rank"])})


def random_bpe(seed=5, alphabet="abcde'.-1", n_merges=400):
    """A dense random merges table over a small alphabet: long merge chains, many ties to break by rank, and pairs of merges
    that produce one string (the later rank owns the string's id, as ClipBPE.encoder resolves it)."""
    rs = np.random.RandomState(seed)
    inner, final = list(alphabet), [c + "</w>" for c in alphabet]
    merges, seen = [], set()
    while len(merges) < n_merges:
        a = inner[rs.randint(len(inner))]
        b = (inner + final)[rs.randint(len(inner) + len(final))]
        if (a, b) in seen or len(a + b) > 12:
            continue
        seen.add((a, b))
        merges.append((a, b))
        (final if b.endswith("</w>") else inner).append(a + b)
    return ClipBPE(merges)


def fixture_words():
    words = sorted({w.lower() for t in TEXTS if in_envelope(t) for w in t.replace("_", " ").replace(".", " ").split() if w.isalpha()})
    assert len(words) > 40
    return words


def synthetic_vocab(seed=9):
    """[PAD] [UNK] [CLS] [SEP] [MASK], single letters and digits (some only as ## pieces), punctuation, and random prefixes and
    infixes of the fixture's words with and without ##: greedy longest-match has real choices and real misses."""
    rs = np.random.RandomState(seed)
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    toks += list("abcdefghijklmnoprstuw") + ["##" + c for c in "abcdefghiklmnoprstuvwy"] + list("0123456") + ["##" + c for c in "0123789"]
    toks += list("!\"#$%'()*+,-./:;=?@[]_")
    for w in fixture_words():
        for _ in range(3):
            a = rs.randint(0, len(w))
            b = rs.randint(a + 1, len(w) + 1)
            toks.append(("##" if a else "") + w[a:b])
        toks.append(w[:rs.randint(1, len(w) + 1)])
    toks += ["x" * 100, "##" + "y" * 30]
    out = []
    for t in toks:
        if t not in out:
            out.append(t)
    return out


def soup(rs, n, chars, lo=0, hi=60):
    return ["".join(chars[i] for i in rs.randint(0, len(chars), rs.randint(lo, hi + 1))) for _ in range(n)]


def clean(texts):
    """keep the corpus inside the envelope ('&' never generated; "<|" broken up)"""
    return [t.replace("<|", "< |") for t in texts]


@functools.lru_cache(maxsize=None)
def corpus(kind, n, seed):
    """n in-envelope strings: punctuation / apostrophe soup, contraction soup, word salads, everything mixed.  kind: 'fixture'
    (the fixture's words), 'small' (the random merges table's alphabet) or 'wordpiece' (with a 101-character word)."""
    rs = np.random.RandomState(seed)
    words = fixture_words() + ["it's", "I'm", "you're", "we've", "he'll", "she'd", "don't", "'tis", "rock'n'roll", "3.14", "10:45pm"]
    if kind == "wordpiece":
        words.append("x" * 101)                            # beyond max_input_chars_per_word: [UNK]
    q = n // 4
    out = soup(rs, q, PUNCT + "'''   " + "st", 0, 40)
    out += soup(rs, q, "'''stmdrevlRE ' .1", 0, 50)
    if kind == "small":                                   # the random merges table's alphabet
        out += soup(rs, q, "abcde'.-1 abcde  \t", 0, 90)
    else:
        out += soup(rs, q, LETTERS + DIGITS + PUNCT + SPACES + "     ", 0, 80)
    seps = [" ", "  ", "\t", "\n", ", ", ". ", "-", "'", " '", "' ", "!", "?! ", "/", " \r\n "]
    while len(out) < n:
        k = rs.randint(1, 14)
        parts = []
        for _ in range(k):
            w = words[rs.randint(len(words))]
            parts.append(w.upper() if rs.randint(5) == 0 else w.capitalize() if rs.randint(4) == 0 else w)
            parts.append(seps[rs.randint(len(seps))])
        out.append("".join(parts))
    out = clean(out)
    assert all(in_envelope(t) for t in out)
    return tuple(out)


def boundary_texts():
    """a token, a contraction and a whitespace run placed so that they end at, straddle and begin at bytes 63 / 64 / 65 and
    127 / 128 of the caption (the kernel flags 64 bytes per step)"""
    out = []
    for edge in (64, 128):
        for shift in (-3, -2, -1, 0, 1, 2):
            for probe in ("photo", "they've", "it's", "   \t ", "!!?", "12", "can't've"):
                at = edge + shift
                head = ("a photo of a cat " * 10)[:at - 1] + " "
                out.append(head + probe + " and a dog's bowl.")
                out.append(("a photo of a cat " * 10)[:at] + probe + "tail")          # glued to whatever byte comes before
    return out


def mixed_batch(n, seed=3):
    """rows of mixed lengths with declined rows interleaved (every reason but LEMON_TOK_BUFFER)"""
    rs = np.random.RandomState(seed)
    base = corpus("fixture", 2000, 77)
    bad = ["café au lait", "a cat & a dog", "<|endoftext|> again", "z" * 70 + " is one long word", "w " * 2100, "emoji \U0001F600", ""]
    return [bad[rs.randint(len(bad))] if rs.randint(6) == 0 else base[rs.randint(len(base))] for _ in range(n)]


def host_matrix(tok, texts):
    """the host tokenizer's id matrix as int64 numpy, for ClipTokenize / HFStyleClipTokenizer / BertWordPiece"""
    if isinstance(tok, HFStyleClipTokenizer):
        return np.array(tok(list(texts), padding="max_length", truncation=True)["input_ids"], dtype=np.int64).reshape(len(texts), -1)
    return tok(list(texts)).numpy()


def host_tokenizers(ctx_clip=77, ctx_bert=256):
    bpe = fixture_bpe()
    return {"clip": ClipTokenize(bpe, ctx_clip), "hf": HFStyleClipTokenizer(bpe, ctx_clip),
            "bert": BertWordPiece(synthetic_vocab(), ctx_bert)}
