"""GPU: lemon_tokenize (lemon_amd/csrc/tokenize.hip) against lemon_tokenize_host and against lemon_amd/tokenizer.py's Python
tokenizers.  The criterion is equality of ids, lengths and statuses.  Output buffers are poisoned before every launch; the
Python reference of a corpus is computed once per module.  Then the wrapper (tokenizer.device_form) end to end, the text towers on
device ids against host ids, and cli_common.prepare's `tokenize` under LEMON_TOKENIZE=device."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from lemon_amd import tokenizer as tk
from lemon_amd.tokenizer import BertWordPiece, ClipTokenize, DeviceTokenizer, HFStyleClipTokenizer
from tests import tokenizefx as F

pytestmark = pytest.mark.gpu
NON_ASCII, AMPERSAND, SPECIAL, TOO_LONG, WORD, BUFFER = 1, 2, 3, 4, 5, 6


def device_raw(dev_tok, texts, ctx=None, pad=None):
    """lemon_tokenize on poisoned buffers -> (ids, length, status) as numpy"""
    from lemon_amd import _lib
    from lemon_amd.ops import ptr, stream_ptr
    ctx, pad = ctx or dev_tok.ctx, dev_tok.pad if pad is None else pad
    offsets, blob = dev_tok.pack(texts)
    n = len(texts)
    d = torch.device("cuda")
    text = torch.from_numpy(np.frombuffer(blob or b"\0", dtype=np.uint8).copy()).to(d)
    off = torch.from_numpy(offsets).to(d)
    ids = torch.full((n, ctx), -7, dtype=torch.long, device=d)
    length = torch.full((n,), -7, dtype=torch.int32, device=d)
    status = torch.full((n,), 255, dtype=torch.uint8, device=d)
    _lib.check(dev_tok.lib.lemon_tokenize(dev_tok.handle, ptr(text), len(blob), ptr(off), n, ctx, pad, ptr(ids), ptr(length), ptr(status),
                                          stream_ptr(d)), "lemon_tokenize")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), length.cpu().numpy(), status.cpu().numpy()


def check(tok, texts, want=None):
    """device == host loop (ids, lengths, statuses, every row) and == the Python tokenizer on every served row"""
    texts = list(texts)
    dev_tok = DeviceTokenizer(tok, "cuda")
    got = device_raw(dev_tok, texts)
    ref = dev_tok.tokenize_host_loop(texts)
    for g, r, what in zip(got, ref, ("ids", "length", "status")):
        bad = np.flatnonzero((g != r).reshape(len(texts), -1).any(1)) if len(texts) else []
        assert len(bad) == 0, (what, [(int(i), texts[i][:60]) for i in bad[:5]])
    want = F.host_matrix(tok, texts) if want is None else want
    served = got[2] == 0
    assert np.array_equal(got[0][served], want[served])
    return got


@functools.lru_cache(maxsize=None)
def tokenizers():
    return F.host_tokenizers()


@functools.lru_cache(maxsize=None)
def reference(name, kind, n, seed):
    return F.host_matrix(tokenizers()[name], F.corpus(kind, n, seed))


@pytest.mark.parametrize("name", ["clip", "hf", "bert"])
def test_fixture_texts_and_statuses(hip, name):
    ids, length, status = check(tokenizers()[name], F.TEXTS)
    assert {r: int(s) for r, s in enumerate(status) if s} == F.DECLINED
    if name == "clip":
        assert np.array_equal(ids[status == 0], F.FX["ids_ref_77"][status == 0])


@pytest.mark.parametrize("name,kind,seed", [("clip", "fixture", 101), ("bert", "wordpiece", 303)])
def test_corpus(hip, name, kind, seed):
    texts = F.corpus(kind, 4000, seed)
    _, _, status = check(tokenizers()[name], texts, reference(name, kind, 4000, seed))
    assert (status == 0).all()


def test_corpus_random_merges_table(hip):
    tok = ClipTokenize(F.random_bpe(), 48)
    _, _, status = check(tok, F.corpus("small", 4000, 202))
    assert (status == 0).all()


@pytest.mark.parametrize("name", ["clip", "bert"])
def test_chunk_edges(hip, name):
    texts = F.boundary_texts()
    assert any(t[60:70].count("'") for t in texts) and any(t[124:132].count("'") for t in texts)
    _, _, status = check(tokenizers()[name], texts)
    assert (status == 0).all()


@pytest.mark.parametrize("name", ["clip", "hf", "bert"])
def test_row_edges_and_size_limits(hip, name):
    ctx = 12
    host = tokenizers()[name]
    tok = BertWordPiece(host.vocab, ctx) if name == "bert" else type(host)(host.bpe, ctx)
    texts = ["", " ", " \t\n\r  "] + [" ".join(["a"] * (total - 2)) for total in range(ctx - 3, ctx + 2)]
    _, length, status = check(tok, texts)
    assert (status == 0).all() and length.tolist() == [2, 2, 2, ctx - 3, ctx - 2, ctx - 1, ctx, ctx]
    cap4096 = ("photo " * 683)[:4096]
    _, _, status = check(host, [cap4096, cap4096 + "x", "ab" * 32, "ab" * 32 + "c", " ".join(["a"] * 300) + " " + "ab" * 40])
    assert status.tolist() == [0, TOO_LONG, 0, WORD, 0]          # 65 symbols / 65 pieces; the last row's long word is never reached
    dev_tok = DeviceTokenizer(host, "cuda")
    ids, length, status = device_raw(dev_tok, [])
    assert ids.shape == (0, dev_tok.ctx) and len(length) == 0 and len(status) == 0


def test_forced_collisions_and_cased_vocabulary(hip):
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "cat", "##s", "cats", "ca", "##t", "##ts", "dog", "do", "##g", "##gs", "a", "of", "photo", "ph", "##oto", ".", "'"]
    tok = BertWordPiece(vocab, 24)
    texts = ["A photo of cats.", "dogs cat's dog photos", "phot cat catss gs", "", "do ca ph"]
    forced = DeviceTokenizer(tok, "cuda", home_buckets=2)
    ids, _, status = device_raw(forced, texts)
    assert (status == 0).all() and np.array_equal(ids, F.host_matrix(tok, texts))
    check(BertWordPiece(F.synthetic_vocab(), 32, lower_case=False), F.corpus("wordpiece", 4000, 303)[:1000])
    check(BertWordPiece(F.synthetic_vocab(), 32, max_chars_per_word=5), F.corpus("wordpiece", 4000, 303)[:1000])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batches_with_declined_rows_interleaved(hip, n):
    texts = F.mixed_batch(n, seed=n)
    for name in ("clip", "bert"):
        _, _, status = check(tokenizers()[name], texts)
        if n == 1000:
            assert set(status.tolist()) == ({0, NON_ASCII, AMPERSAND, SPECIAL, TOO_LONG, WORD} if name == "clip" else {0, NON_ASCII, AMPERSAND, SPECIAL, TOO_LONG})


def test_unordered_offsets_are_not_read(hip):
    from lemon_amd import _lib
    from lemon_amd.ops import ptr, stream_ptr
    dev_tok = DeviceTokenizer(tokenizers()["clip"], "cuda")
    d = torch.device("cuda")
    text = torch.from_numpy(np.frombuffer(b"a photo of a cat", dtype=np.uint8).copy()).to(d)
    off = torch.tensor([0, 7, 3, 16, 40], dtype=torch.long, device=d)
    ids = torch.full((4, 77), -7, dtype=torch.long, device=d)
    length, status = torch.full((4,), -7, dtype=torch.int32, device=d), torch.full((4,), 255, dtype=torch.uint8, device=d)
    _lib.check(dev_tok.lib.lemon_tokenize(dev_tok.handle, ptr(text), 16, ptr(off), 4, 77, 0, ptr(ids), ptr(length), ptr(status), stream_ptr(d)), "lemon_tokenize")
    want = F.host_matrix(tokenizers()["clip"], ["a photo", "hoto of a cat"])
    assert status.tolist() == [0, BUFFER, 0, BUFFER] and length.tolist() == [4, 0, int((want[1] != 0).sum()), 0]
    assert np.array_equal(ids[0].cpu().numpy(), want[0]) and np.array_equal(ids[2].cpu().numpy(), want[1])
    assert (ids[1] == 0).all() and (ids[3] == 0).all()


@pytest.mark.parametrize("name", ["clip", "hf", "bert"])
def test_wrapper_end_to_end(hip, name):
    host = tokenizers()[name]
    dev_tok = tk.device_form(host, torch.device("cuda"))
    assert isinstance(dev_tok, DeviceTokenizer)
    texts = F.mixed_batch(300, seed=11) + F.TEXTS
    ids = dev_tok(texts)
    want = F.host_matrix(host, texts)
    assert ids.is_cuda and ids.dtype == torch.long and np.array_equal(ids.cpu().numpy(), want)
    assert dev_tok.declined == sum(not F.in_envelope(t) or len(t) > 4096 or (name != "bert" and "z" * 70 in t) for t in texts) > 10
    if name == "hf":
        last = np.array(host(texts, padding="max_length", truncation=True)["attention_mask"]).sum(-1)
    else:
        last = np.array([np.flatnonzero(row != dev_tok.pad)[-1] + 1 for row in want])
    assert np.array_equal(dev_tok.lengths.numpy(), last)
    assert dev_tok([]).shape == (0, dev_tok.ctx) and dev_tok("a cat").shape == (1, dev_tok.ctx)


def test_clip_tower_on_device_ids(hip):
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.pipeline import Embedder
    torch.manual_seed(0)
    cfg = dataclasses.replace(ClipConfig.named("tiny"), vocab_size=49408, eos_token_id=49407)
    emb = Embedder(LemonCLIP(cfg), torch.device("cuda"), batch_size=64)
    host = ClipTokenize(F.fixture_bpe(), cfg.context_length)
    texts = F.TEXTS + list(F.corpus("fixture", 2000, 77)[:150])
    a = emb.embed_texts(host(texts))
    b = emb.embed_texts(tk.device_form(host, emb.device)(texts))
    assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize("bucket", [0, 8])
def test_bert_tower_on_device_ids(hip, bucket):
    from lemon_amd.biomed import BiomedCLIP, BiomedConfig
    from lemon_amd.pipeline import Embedder
    torch.manual_seed(0)
    vocab = F.synthetic_vocab()
    cfg = dataclasses.replace(BiomedConfig.named("biomed-tiny"), vocab_size=len(vocab))
    model = BiomedCLIP(cfg)
    model.text.length_bucket = bucket              # what $LEMON_BERT_BUCKET sets when the tower is built
    emb = Embedder(model, torch.device("cuda"), batch_size=64)
    host = BertWordPiece(vocab, cfg.context_length)
    texts = F.TEXTS + list(F.corpus("wordpiece", 4000, 303)[3000:3150])
    a = emb.embed_texts(host(texts))
    b = emb.embed_texts(tk.device_form(host, emb.device)(texts))
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_cli_tokenize_under_the_environment_knob(hip, tmp_path, monkeypatch):
    """cli_common.prepare's `tokenize`: a device tensor equal to the default's output, from a merges file written from the fixture"""
    from lemon_amd import clip as clip_mod
    from lemon_amd.cli_common import prepare
    from lemon_amd.run_lemon import build_parser
    merges = tmp_path / "merges.txt"
    ranked = sorted(zip(F.FX["merge_rank"].tolist(), F.FX["merge_first"].tolist(), F.FX["merge_second"].tolist()))
    merges.write_text("#version: 0.2\n" + "".join(f"{a} {b}\n" for _, a, b in ranked))
    named = clip_mod.ClipConfig.named
    monkeypatch.setattr(clip_mod.ClipConfig, "named", staticmethod(
        lambda name: dataclasses.replace(named("tiny"), vocab_size=49408, eos_token_id=49407) if name == "tiny" else named(name)))
    # a dense merges file ranks its lines 0, 1, ...: the reference here is the host tokenizer built from the same file
    out = {}
    for branch in ("cc3m_clip_from_scratch", "huggingface_clip"):
        for mode in ("host", "device"):
            monkeypatch.setenv("LEMON_TOKENIZE", mode)
            args = build_parser().parse_args(["--output_dir", str(tmp_path / f"{branch}_{mode}"), "--dataset", "mscoco", "--noise_type", "random",
                                              "--data_root", "synthetic:60", "--clip_model", branch, "--clip_path", "random:tiny",
                                              "--bpe_path", str(merges), "--debug"])
            out[mode] = prepare(args).tokenize(F.TEXTS)
        assert not out["host"].is_cuda and out["device"].is_cuda
        assert out["device"].dtype == torch.long and torch.equal(out["device"].cpu(), out["host"])
