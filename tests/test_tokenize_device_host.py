"""CPU: the device tokenizers' algorithm with the lanes looped on the host (lemon_tokenize_host: the functions of
lemon_amd/csrc/tokenize_core.hpp that the kernel runs) against lemon_amd/tokenizer.py's Python classes -- tokenize(),
HFStyleClipTokenizer, BertWordPiece.__call__ --, which tests/test_tokenizer.py and tests/test_biomed.py pin to the reference and
to transformers.  The criterion is equality of ids; no row is left out of a comparison.  Also: the statuses of rows outside the
envelope, the size limits, the table builders, the C ABI's three descriptions, device_form's refusals and the sanitizer fuzz."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from lemon_amd import tokenizer as tk
from lemon_amd.tokenizer import BertWordPiece, ClipBPE, ClipTokenize, DeviceTokenizer, HFStyleClipTokenizer
from tests import tokenizefx as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lemon_tokenizer_create_bpe", "lemon_tokenizer_create_wordpiece", "lemon_tokenizer_free", "lemon_tokenizer_table_info",
               "lemon_tokenize", "lemon_tokenize_host"]
NON_ASCII, AMPERSAND, SPECIAL, TOO_LONG, WORD, BUFFER = 1, 2, 3, 4, 5, 6


def with_ctx(tok, ctx):
    if isinstance(tok, BertWordPiece):
        return BertWordPiece(tok.vocab, ctx, tok.lower_case, tok.max_chars)
    return type(tok)(tok.bpe, ctx)


def check_equal(tok, texts, expect_declined=None):
    """host loop == Python tokenizer on every row the device serves; returns the statuses"""
    texts = list(texts)
    dev = DeviceTokenizer(tok, "cpu")
    ids, length, status = dev.tokenize_host_loop(texts)
    want = F.host_matrix(tok, texts)
    assert ids.shape == want.shape and ids.dtype == np.int64
    declined = {} if expect_declined is None else expect_declined
    for r in range(len(texts)):
        assert status[r] == declined.get(r, 0), (r, texts[r][:80], int(status[r]))
        if status[r]:
            assert length[r] == 0 and (ids[r] == dev.pad).all()
        else:
            assert np.array_equal(ids[r], want[r]), (r, texts[r][:120], ids[r][:24], want[r][:24])
            last = dev.host_rows([texts[r]])[1][0]
            assert length[r] == last, (r, texts[r][:80])
    return status


@pytest.fixture(scope="module")
def toks():
    return F.host_tokenizers()


@pytest.mark.parametrize("ctx", [16, 77, 256])
@pytest.mark.parametrize("name", ["clip", "hf", "bert"])
def test_fixture_texts(toks, name, ctx):
    tok = with_ctx(toks[name], ctx)
    assert sum(F.in_envelope(t) for t in F.TEXTS) == 46 and len(F.TEXTS) == 50
    assert sorted(F.DECLINED) == [r for r, t in enumerate(F.TEXTS) if not F.in_envelope(t)]
    check_equal(tok, F.TEXTS, F.DECLINED)
    if name == "clip":                    # the reference's own ids: the fixture's truncated rows are among the served ones
        ids, _, status = DeviceTokenizer(tok, "cpu").tokenize_host_loop(F.TEXTS)
        ok = status == 0
        assert np.array_equal(ids[ok], F.FX[f"ids_ref_{ctx}"][ok])
        cut = F.FX[f"ids_ref_{ctx}"][:, -1] != 0
        assert int(cut.sum()) == {16: 7, 77: 2, 256: 2}[ctx] and int((cut & ok).sum()) == {16: 6, 77: 2, 256: 2}[ctx]


def test_fuzz_clip_fixture_table(toks):
    texts = F.corpus("fixture", 20000, 101)
    check_equal(toks["clip"], texts)
    check_equal(with_ctx(toks["hf"], 24), texts[:4000])


def test_fuzz_clip_random_table():
    bpe = F.random_bpe()
    check_equal(ClipTokenize(bpe, 48), F.corpus("small", 20000, 202))


def test_fuzz_wordpiece(toks):
    texts = F.corpus("wordpiece", 20000, 303)
    assert any("x" * 101 in t for t in texts)
    check_equal(with_ctx(toks["bert"], 64), texts)
    cased = BertWordPiece(F.synthetic_vocab(), 32, lower_case=False)
    check_equal(cased, texts[:4000])
    short = BertWordPiece(F.synthetic_vocab(), 32, max_chars_per_word=5)
    check_equal(short, texts[:4000])


def test_wordpiece_reserved_words_and_specials(toks):
    texts = ["a [PAD] b", "[MASK]", "x [SEP]", "[CLS] y", "an [UNK] word", "[pad] [PAD]x x[PAD] [ PAD ] [PADS] [MASK]] a[MASK]", "a <| b", "R&D"]
    check_equal(toks["bert"], texts, {0: SPECIAL, 1: SPECIAL, 2: SPECIAL, 3: SPECIAL, 4: SPECIAL, 6: SPECIAL, 7: AMPERSAND})
    check_equal(toks["clip"], texts, {6: SPECIAL, 7: AMPERSAND})
    both = ["café & <|", "\x0b", "\x7f", "tab\tok", "\x00"]
    check_equal(toks["clip"], both, {0: NON_ASCII, 1: NON_ASCII, 2: NON_ASCII, 4: NON_ASCII})


@pytest.mark.parametrize("name", ["clip", "hf", "bert"])
def test_edges_of_the_row(toks, name):
    ctx = 12
    tok = with_ctx(toks[name], ctx)
    texts = ["", " ", " \t\n\r  "]
    # exactly ctx - 3 .. ctx + 1 tokens: "a" is one id in both vocabularies
    for total in range(ctx - 3, ctx + 2):
        texts.append(" ".join(["a"] * (total - 2)))
    check_equal(tok, texts)
    dev = DeviceTokenizer(tok, "cpu")
    _, length, _ = dev.tokenize_host_loop(texts)
    assert length.tolist() == [2, 2, 2, ctx - 3, ctx - 2, ctx - 1, ctx, ctx]
    ids, length, status = dev.tokenize_host_loop([])
    assert ids.shape == (0, ctx) and len(length) == 0 and len(status) == 0


def test_size_limits(toks):
    word64, word65 = "ab" * 32, "ab" * 32 + "c"
    check_equal(toks["clip"], [word64, word65, "ok " + word65, " ".join(["a"] * 90) + " " + word65], {1: WORD, 2: WORD})
    # the last row: the long word lies beyond the 77 tokens that reach the row and is never looked at
    cap4096 = ("photo " * 683)[:4096]
    assert len(cap4096) == 4096
    for name in ("clip", "hf", "bert"):          # 4 096 letters: one CLIP word of too many symbols, one WordPiece word beyond max_chars
        check_equal(toks[name], [cap4096, cap4096 + "x", "a" * 4096, " " * 4097], {1: TOO_LONG, 3: TOO_LONG, **({} if name == "bert" else {2: WORD})})
    # WordPiece: a word of more than 64 pieces is handed back, a word longer than max_chars is [UNK]
    bert = toks["bert"]
    check_equal(bert, ["a" * 64, "a" * 65, "a" * 100, "a" * 101], {1: WORD, 2: WORD})           # pieces a, ##a, ##a, ...
    pieces = BertWordPiece(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "##a"], 256)
    check_equal(pieces, ["a" * 64, "a" * 65, "a" * 101], {1: WORD})


def test_unordered_offsets_are_not_read(toks):
    dev = DeviceTokenizer(toks["clip"], "cpu")
    text = np.frombuffer(b"a photo of a cat", dtype=np.uint8)
    offsets = np.array([0, 7, 3, 16, 40], dtype=np.int64)
    ids, length, status = np.zeros((4, 77), np.int64), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    rc = dev.lib.lemon_tokenize_host(dev.handle, text.ctypes.data, len(text), offsets.ctypes.data, 4, 77, 0, ids.ctypes.data,
                                     length.ctypes.data, status.ctypes.data)
    assert rc == 0 and status.tolist() == [0, BUFFER, 0, BUFFER]
    assert np.array_equal(ids[0], F.host_matrix(toks["clip"], ["a photo"])[0])
    assert np.array_equal(ids[2], F.host_matrix(toks["clip"], ["hoto of a cat"])[0])
    for ctx in (1, 1025):
        assert dev.lib.lemon_tokenize_host(dev.handle, text.ctypes.data, len(text), offsets.ctypes.data, 1, ctx, 0, ids.ctypes.data,
                                           length.ctypes.data, status.ctypes.data) == -1


def test_duplicate_string_merges_resolve_like_the_encoder():
    # "abc" is produced by (ab, c) at rank 2 and by (a, bc) at rank 3: the encoder gives the string the later id, whichever merge fired
    bpe = ClipBPE([("a", "b"), ("b", "c</w>"), ("ab", "c</w>"), ("a", "bc</w>"), ("b", "c"), ("ab", "c"), ("a", "bc")])
    assert bpe.encoder["abc</w>"] == 512 + 3 and bpe.encoder["abc"] == 512 + 6
    texts = ["abc", "abcabc abc", "bc abc", "xabc", "abcx"]
    check_equal(ClipTokenize(bpe, 20), texts)
    left, right, rank, merged = tk.bpe_id_table(bpe)
    assert sorted(merged[rank == 2].tolist() + merged[rank == 3].tolist()) == [515, 515]
    # a merge whose part has no id can never fire and is left out
    sparse = ClipBPE({("q", "u"): 7, ("zz", "y"): 3})
    assert len(tk.bpe_id_table(sparse)[0]) == 1
    check_equal(ClipTokenize(sparse, 20), ["quzzy zzy"])


def test_tables_are_at_most_half_full(toks):
    for tok in (toks["clip"], toks["bert"], ClipTokenize(F.random_bpe(), 16)):
        slots, entries, probe = DeviceTokenizer(tok, "cpu").table_info()
        assert entries > 0 and 2 * entries <= slots and slots & (slots - 1) == 0 and 1 <= probe <= 64
    assert DeviceTokenizer(toks["clip"], "cpu").table_info()[1] == len(tk.bpe_id_table(toks["clip"].bpe)[0])
    assert DeviceTokenizer(toks["bert"], "cpu").table_info()[1] == len(toks["bert"].vocab)


def test_forced_collisions_cannot_change_an_id():
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "cat", "##s", "cats", "ca", "##t", "##ts", "dog", "do", "##g", "##gs", "a", "of", "photo", "ph", "##oto", ".", "'"]
    tok = BertWordPiece(vocab, 24)
    forced = DeviceTokenizer(tok, "cpu", home_buckets=2)
    slots, entries, probe = forced.table_info()
    assert entries == len(vocab) and probe >= len(vocab) // 2          # two home slots: long probe chains, every lookup collides
    texts = ["A photo of cats.", "dogs cat's dog photos", "phot cat catss gs", "", "do ca ph"]
    ids, length, status = forced.tokenize_host_loop(texts)
    assert (status == 0).all() and np.array_equal(ids, F.host_matrix(tok, texts))
    # too many tokens for two home slots: the builder refuses instead of exceeding the probe bound
    with pytest.raises(Exception, match="vocabulary"):
        DeviceTokenizer(BertWordPiece(F.synthetic_vocab(), 24), "cpu", home_buckets=2)


def test_header_exports_and_binding_agree():
    from lemon_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lemon_hip.h")).read(), flags=re.S)
    declared = dict(re.findall(r"\b(lemon_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.SO_PATH), name), name
        assert len(getattr(lib, name).argtypes) == declared[name].count(",") + 1, name
    assert "tokenize.hip" in build.SOURCES and "tokenize_core.hpp" in build.HEADERS
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"k_tokenize" in blob
    for code, macro in ((NON_ASCII, "NON_ASCII"), (AMPERSAND, "AMPERSAND"), (SPECIAL, "SPECIAL"), (TOO_LONG, "TOO_LONG"), (WORD, "WORD"), (BUFFER, "BUFFER")):
        assert re.search(rf"#define LEMON_TOK_{macro} {code}\b", hdr)
    for site in ("lib/models/simple_tokenizer.py:86-104", "lib/models/chexzero_clip.py:481-493", "run_lemon.py:140-154", "lib/models/utils.py:72-78"):
        assert site in open(os.path.join(ROOT, "include", "lemon_hip.h")).read()


def test_device_form_refusals(toks, tmp_path, monkeypatch):
    from lemon_amd.clip import SyntheticTokenizer
    assert tk.device_form(SyntheticTokenizer(300, 16, 299), "cpu") is None
    assert tk.device_form(lambda texts: None, "cpu") is None
    assert tk.device_form(ClipTokenize(toks["clip"].bpe, 2000), "cpu") is None              # context beyond LEMON_TOKENIZE_MAX_CTX
    big = BertWordPiece({"[PAD]": 0, "[UNK]": 1, "[CLS]": 2, "[SEP]": 3, "a": 70000}, 16)
    assert tk.device_form(big, "cpu") is None                                               # ids beyond 16 bits
    assert isinstance(tk.device_form(toks["hf"], "cpu"), DeviceTokenizer)
    (tmp_path / "ftfy.py").write_text("def fix_text(t):\n    return t\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    assert tk.device_form(toks["clip"], "cpu") is None and tk.device_form(toks["bert"], "cpu") is None
    monkeypatch.setenv("LEMON_TOKENIZE", "gpu")
    with pytest.raises(ValueError):
        tk.tokenize_mode()
    monkeypatch.delenv("LEMON_TOKENIZE")
    assert tk.tokenize_mode() == "host"


def test_in_tree_branch_returns_the_same_tokenizer(tmp_path):
    """algorithm_class_from_scratch's in-tree CLIP branch now returns a ClipTokenize: same ids as tokenize(texts, model, bpe)"""
    from lemon_amd.clip import algorithm_class_from_scratch
    merges = tmp_path / "merges.txt"
    ranked = sorted(zip(F.FX["merge_rank"].tolist(), F.FX["merge_first"].tolist(), F.FX["merge_second"].tolist()))
    merges.write_text("#version: 0.2\n" + "".join(f"{a} {b}\n" for _, a, b in ranked))
    model, tok = algorithm_class_from_scratch("cc3m_clip_from_scratch", "random", return_tokenizer=True, bpe_path=str(merges))
    assert isinstance(tok, ClipTokenize) and tok.context_length == model.context_length
    assert np.array_equal(tok(F.TEXTS[:5]).numpy(), tk.tokenize(F.TEXTS[:5], model, tok.bpe).numpy())


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_core_fuzz_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "tokenize_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "tokenize_fuzz.cpp"), "-o", exe])
    for seed in ("1", "20261018"):
        r = subprocess.run([exe, "4000", seed], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "tokenize_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_kernel_does_not_spill():
    from tests.test_build_guard import HIPCC, _kernel_meta
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    meta = _kernel_meta("tokenize.hip")
    hits = [n for n in meta if "k_tokenize" in n]
    assert hits
    for n in hits:
        assert meta[n]["vgpr_spill_count"] == 0 and meta[n]["private_segment_fixed_size"] == 0, (n, meta[n])
