"""GPU: the BERT text tower with captions batched by length BUCKET (BertTextTower.length_bucket, $LEMON_BERT_BUCKET): every
caption's own token count goes to the attention kernels (lemon_attention_*_varlen) instead of every micro-batch holding one exact
count.  A two-layer mid-size tower against HF BertModel on the CPU (the recipe of tests/biomed_recipe.py) at the bars of
tests/test_gpu_biomed.py, with the plain-PyTorch formulations made to raise."""
import copy

import pytest
import torch

from lemon_amd.biomed import BertTextTower, BiomedConfig
from lemon_amd.clip import Block, TowerConfig

from . import biomed_recipe as R

pytestmark = pytest.mark.gpu

# 24 captions, 3 .. 70 tokens, with repeats: 19 distinct counts in the 8-token buckets 8, 16, 24, 32, 40, 48, 64, 72
LENS = [3, 70, 9, 17, 9, 33, 64, 40, 8, 16, 24, 41, 9, 65, 57, 5, 12, 33, 70, 31, 32, 48, 3, 20]
MODES = ("f16x3", "bf16x6", "f32")


def _config():
    # every width a multiple of 256 (the hand-written GEMM chain runs), two layers: a chained block and the pooled last block
    return BiomedConfig(embed_dim=64, image_size=64, patch_size=16, vision=TowerConfig(256, 1, 4, 512), text=TowerConfig(256, 2, 4, 512),
                        vocab_size=500, context_length=72, max_positions=80, proj_hidden=160)


_CASE = {}


def _case():
    """(ours on the GPU, ids, HF features on the CPU), made once and never changed by a test (weights are restored)"""
    if not _CASE:
        cfg, real = _config(), R.config
        R.config = lambda size: cfg
        try:
            _, bert, ours = R.hf_pair("varlen", seed=5)
        finally:
            R.config = real
        ids = R.caption_ids(cfg, LENS, seed=6)
        ref = R.hf_text_features(bert, ours, ids)              # on the CPU, before .cuda() moves the projections in place
        _CASE["v"] = (ours.cuda(), ids, ref, bert)
    return _CASE["v"]


def _check(got, ref, what, raw=1e-4, normed=1e-5):
    sc = float(ref.abs().max())
    d = float((got - ref).abs().max())
    dn = float((torch.nn.functional.normalize(got, dim=1) - torch.nn.functional.normalize(ref, dim=1)).abs().max())
    print(f"biomed varlen {what}: raw max abs diff {d:.3e} (scale {sc:.3f}), unit-norm max abs diff {dn:.3e}")
    assert d <= raw * max(1.0, sc), f"{what}: raw max abs diff {d} (scale {sc})"
    assert dn <= normed, f"{what}: normalised max abs diff {dn}"


def _refuse(monkeypatch):
    def no_sdpa(*a, **k):
        raise AssertionError("Block._sdpa was called: the attention kernels must take the lengths")

    def no_masked(*a, **k):
        raise AssertionError("BertTextTower._masked was called for captions without padding inside")

    monkeypatch.setattr(Block, "_sdpa", no_sdpa)
    monkeypatch.setattr(BertTextTower, "_masked", no_masked)


class _bucket:
    def __init__(self, tower, n):
        self.tower, self.n = tower, n

    def __enter__(self):
        self.prev, self.tower.length_bucket = self.tower.length_bucket, self.n

    def __exit__(self, *a):
        self.tower.length_bucket = self.prev


@pytest.mark.parametrize("mode", MODES)
def test_bucketed_tower_vs_hf_bert(hip, mode, monkeypatch):
    monkeypatch.setenv("LEMON_GEMM", mode)
    ours, ids, ref, _ = _case()
    assert ours.text.length_bucket == 0
    base = ours.encode_text(ids.cuda()).cpu()                # exact-length groups: today's path
    _check(base, ref, f"{mode}/bucket 0")
    _refuse(monkeypatch)
    for n in (8, 32):
        with _bucket(ours.text, n):
            # the whole batch in one call: every caption at the longest one's bucket (72 tokens), 3 .. 70 of them its own
            got = ours.encode_text(ids.cuda()).cpu()
            _check(got, ref, f"{mode}/bucket {n}/one call")
            print(f"biomed varlen {mode}/bucket {n}: max abs diff to the bucket-0 embeddings {float((got - base).abs().max()):.3e}")
            # one bucket at a time with host lengths, as pipeline.Embedder calls it
            lens = torch.tensor(LENS)
            for Lb in sorted({ours.text.seq_len_for(v - 1) for v in LENS}):
                sel = torch.tensor([i for i, v in enumerate(LENS) if ours.text.seq_len_for(v - 1) == Lb])
                part = ours.encode_text(ids[sel].cuda(), seq_len=Lb, lengths=lens[sel]).cpu()
                _check(part, ref[sel], f"{mode}/bucket {n}/group {Lb}")


def test_caption_with_padding_inside_still_takes_the_masked_formulation(hip, monkeypatch):
    ours, ids, _, bert = _case()
    ids = ids.clone()
    ids[5, 7] = ids[11, 1] = ours.cfg.pad_token_id           # 33 and 41 tokens, a pad id inside
    ref = R.hf_text_features(bert, copy.deepcopy(ours).cpu(), ids)
    calls = []
    real = BertTextTower._masked

    def spy(self, rows):
        calls.append(tuple(rows.shape))
        return real(self, rows)

    monkeypatch.setattr(BertTextTower, "_masked", spy)
    with _bucket(ours.text, 8):
        got = ours.encode_text(ids.cuda()).cpu()
    assert calls == [(2, 41)], calls
    _check(got, ref, "inner pads/bucket 8")


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_nan_in_the_pad_token_embedding_changes_no_bit(hip, mode, monkeypatch):
    monkeypatch.setenv("LEMON_GEMM", mode)
    ours, ids, _, _ = _case()
    _refuse(monkeypatch)
    pad = ours.cfg.pad_token_id
    with _bucket(ours.text, 8):
        want = ours.encode_text(ids.cuda())
        keep = ours.text.tok.weight.data[pad].clone()
        try:
            ours.text.tok.weight.data[pad] = float("nan")   # every position behind every caption
            got = ours.encode_text(ids.cuda())
        finally:
            ours.text.tok.weight.data[pad] = keep
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


def test_embedder_cuts_micro_batches_per_bucket(hip, monkeypatch):
    from lemon_amd.pipeline import Embedder
    ours, ids, ref, _ = _case()
    _refuse(monkeypatch)
    refn = torch.nn.functional.normalize(ref, dim=1)
    calls = []
    real = ours.encode_text

    def spy(rows, **kw):
        calls.append((int(kw["seq_len"]), len(kw["lengths"])))
        return real(rows, **kw)

    with _bucket(ours.text, 8):
        emb = Embedder(ours, torch.device("cuda"), batch_size=4, text_batch_size=64, text_token_budget=4096)
        monkeypatch.setattr(ours, "encode_text", spy)
        got = emb.embed_texts(ids)
        emb.raise_if_nonfinite()
    assert emb.text_tokens_run == sum((v + 7) // 8 * 8 for v in LENS)
    assert emb.fallback_rows == 0 and emb.fold_fallback_rows == 0
    distinct = len(set(LENS))
    print(f"biomed varlen embedder: {len(calls)} encode_text calls {calls} for {distinct} distinct token counts")
    assert sum(n for _, n in calls) == len(LENS) and len(calls) == len({(v + 7) // 8 for v in LENS}) and 2 * len(calls) <= distinct
    assert float((got.cpu() - refn).abs().max()) <= 1e-5
