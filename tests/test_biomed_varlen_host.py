"""CPU: the host side of BertTextTower.length_bucket ($LEMON_BERT_BUCKET) -- pipeline.Embedder cuts micro-batches per token-count
BUCKET instead of per exact count and hands the captions' own counts to encode_text; bucket 0 is the behaviour
tests/test_biomed.py pins, call for call."""
import pytest
import torch

from lemon_amd.biomed import BertTextTower, BiomedCLIP, BiomedConfig

from .biomed_recipe import caption_ids, hf_pair

LENS = [9, 4, 9, 2, 9, 9, 4, 24, 9]


def _embedder(ours, bucket, batch=3, budget=None):
    from lemon_amd.pipeline import Embedder
    ours.text.length_bucket = bucket
    emb = Embedder.__new__(Embedder)
    emb.model, emb.device, emb.text_batch_size, emb.length_bucketing, emb.range_fallback, emb.text_tokens_run = ours, torch.device("cpu"), batch, False, False, 0
    emb.text_token_budget = budget
    return emb


def _spy(monkeypatch, ours, check=None):
    seen = []
    real = ours.encode_text

    def spy(rows, seq_len=None, lengths=None, **kw):
        if check is not None:
            check(rows, lengths)
        seen.append((int(seq_len), lengths.tolist()))
        return real(rows)

    monkeypatch.setattr(ours, "encode_text", spy)
    return seen, real


def _ceil(n, b):
    return (n + b - 1) // b * b


def test_micro_batches_hold_one_bucket_and_carry_the_true_counts(monkeypatch):
    _, _, ours = hf_pair("tiny", seed=7)
    emb = _embedder(ours, 8)
    assert ours.text.exact_lengths is False
    ids = caption_ids(ours.cfg, LENS)
    seen, real = _spy(monkeypatch, ours, lambda rows, lengths: bool(((rows != ours.cfg.pad_token_id).sum(-1) == lengths).all()) or pytest.fail("counts"))
    out = emb._embed_texts(ids)
    # shortest captions first; a micro-batch never straddles an 8-token bucket; at most text_batch_size captions
    assert seen == [(8, [2, 4, 4]), (16, [9, 9, 9]), (16, [9, 9]), (24, [24])], seen
    assert all(_ceil(n, 8) == s for s, l in seen for n in l)
    assert emb.text_tokens_run == sum(_ceil(n, 8) for n in LENS)
    assert (out - real(ids)).abs().max() < 1e-5              # results come back in caption order


def test_token_budget_cuts_the_buckets(monkeypatch):
    _, _, ours = hf_pair("tiny", seed=7)
    emb = _embedder(ours, 8, budget=40)                      # 40 // 8 = 5, 40 // 16 = 2, 40 // 24 = 1 captions per micro-batch
    seen, _ = _spy(monkeypatch, ours)
    emb._embed_texts(caption_ids(ours.cfg, LENS))
    assert seen == [(8, [2, 4, 4]), (16, [9, 9]), (16, [9, 9]), (16, [9]), (24, [24])], seen
    assert all(s * len(l) <= 40 for s, l in seen)


def test_bucket_is_capped_at_the_context_length(monkeypatch):
    _, _, ours = hf_pair("tiny", seed=7)                     # context 24, 32 positions
    t = ours.text
    t.length_bucket = 32
    assert [t.seq_len_for(n - 1) for n in (1, 9, 24)] == [24, 24, 24]
    t.length_bucket = 16
    assert [t.seq_len_for(n - 1) for n in (1, 16, 17, 24)] == [16, 16, 24, 24]
    t.length_bucket = 0
    assert [t.seq_len_for(n - 1) for n in (1, 9, 24)] == [1, 9, 24]
    emb = _embedder(ours, 32)
    seen, _ = _spy(monkeypatch, ours)
    emb._embed_texts(caption_ids(ours.cfg, LENS))
    assert [s for s, _ in seen] == [24, 24, 24] and [n for _, l in seen for n in l] == sorted(LENS)


def test_rows_with_padding_inside_are_held_out_of_the_buckets(monkeypatch):
    _, _, ours = hf_pair("tiny", seed=7)
    emb = _embedder(ours, 8)
    lens = LENS + [12]
    ids = caption_ids(ours.cfg, lens)
    ids[2, 3] = ids[7, 1] = ids[9, 4] = ids[9, 8] = ours.cfg.pad_token_id
    eot, inner = emb._caption_marks(ids)
    assert eot.tolist() == [n - 1 for n in lens] and inner.tolist() == [r in (2, 7, 9) for r in range(len(lens))]
    masked = []
    real_masked = ours.text._masked
    seen, _ = _spy(monkeypatch, ours, lambda rows, lengths: bool(((rows != ours.cfg.pad_token_id).sum(-1) == lengths).all()) or pytest.fail("a held-out row reached encode_text"))

    def spy_masked(rows):
        masked.append(tuple(rows.shape))
        return real_masked(rows)

    monkeypatch.setattr(ours.text, "_masked", spy_masked)
    out = emb._embed_texts(ids)
    assert seen == [(8, [2, 4, 4]), (16, [9, 9, 9]), (16, [9])], seen
    assert masked[-1] == (3, 24)                             # the three held-out rows, at the bucket of the longest
    assert emb.text_tokens_run == 3 * 8 + 4 * 16 + 3 * 24
    monkeypatch.undo()
    assert (out - ours.text._masked(ids[:, :24])).abs().max() < 1e-5


def test_bucket_zero_makes_the_calls_of_the_exact_length_grouping(monkeypatch):
    _, _, ours = hf_pair("tiny", seed=7)
    assert ours.text.length_bucket == 0 and ours.text.exact_lengths is True     # the default
    emb = _embedder(ours, 0)
    seen, real = _spy(monkeypatch, ours)
    ids = caption_ids(ours.cfg, LENS)
    out = emb._embed_texts(ids)
    assert seen == [(2, [2]), (4, [4, 4]), (9, [9, 9, 9]), (9, [9, 9]), (24, [24])], seen
    assert emb.text_tokens_run == sum(LENS)
    assert (out - real(ids)).abs().max() < 1e-5


def test_environment_value_is_validated(monkeypatch):
    cfg = BiomedConfig.named("biomed-tiny")
    monkeypatch.delenv("LEMON_BERT_BUCKET", raising=False)
    assert BertTextTower(cfg).length_bucket == 0
    for good in ("0", "8", "32", " 16 "):
        monkeypatch.setenv("LEMON_BERT_BUCKET", good)
        assert BiomedCLIP(cfg).text.length_bucket == int(good)
    for bad in ("12", "-8", "7", "abc", "8.0", ""):
        monkeypatch.setenv("LEMON_BERT_BUCKET", bad)
        with pytest.raises(ValueError, match="LEMON_BERT_BUCKET"):
            BertTextTower(cfg)
    monkeypatch.setenv("LEMON_BERT_BUCKET", "0")
    t = BertTextTower(cfg)
    t.length_bucket = 12                                     # set on the object: refused where it is used
    with pytest.raises(ValueError, match="length_bucket"):
        t.seq_len_for(5)
    with pytest.raises(ValueError, match="length_bucket"):
        t.exact_lengths


def test_lengths_need_the_kernels_that_take_them():
    from lemon_amd import ops
    assert ops.attention_varlen_supported(768, 12, 256) and ops.attention_varlen_supported(256, 4, 1) and ops.attention_varlen_supported(128, 2, 288)
    assert not ops.attention_varlen_supported(768, 12, 289) and not ops.attention_varlen_supported(1280, 16, 40)
    assert not ops.attention_varlen_supported(768, 12, 0)
