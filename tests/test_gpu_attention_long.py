"""GPU: the streaming attention kernels (csrc/attention.hip: k_attention_hd64_stream, k_attention_hd64_stream_f16) that serve
sequences beyond 288 tokens -- the 577 tokens of ViT-L/14@336, 1025 at 448 px, text contexts of 512 -- in both arithmetic forms
(lemon_attention_set_f16(1): split products on the fp16 matrix cores, (0): v_mfma_f32_32x32x2_f32) and all four output forms.

Kernel level: float64 reference at the project's bar, bit equality with the one-workgroup kernels when forced onto 64 < L <= 288
(lemon_attention_set_stream_min), the split output forms, poisoned buffers through the C ABI, batch independence, the limits.
Tower level: a 336-px ViT-L/14 and a 512-token text tower against HF CLIP with the SDPA fallback made to raise.
(Every block edge from 289 to 577 tokens, stress input for the online softmax, the per-element bound and NaN neighbours:
tests/test_gpu_attention_stream_edges.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from .attention_ref import OUT_FILL, TAIL, TM, _arith, _reference64, _tiled_index

pytestmark = pytest.mark.gpu

LONG_SHAPES = [(1, 289, 3, False), (2, 577, 16, False), (1, 577, 12, True), (2, 512, 8, True), (1, 1025, 12, False),
               (1, 2049, 2, True), (1, 4096, 1, False)]
# the shapes of tests/test_gpu_parity.py::test_long_sequence_attention_kernels_agree_bit_for_bit
SHIPPED_SHAPES = [(2, 65, 3, False), (3, 77, 8, True), (2, 197, 12, False), (1, 257, 16, False), (2, 288, 2, True),
                  (1, 256, 4, True), (2, 96, 1, False)]


def _lib():
    from lemon_amd import _lib as L
    return L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. float64 reference beyond 288 tokens --------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("B,L,H,causal", LONG_SHAPES)
def test_streaming_attention_matches_float64_reference(hip, B, L, H, causal, f16):
    # recipe and bar of test_fused_attention_matches_float64_reference (tests/test_gpu_parity.py)
    from lemon_amd.ops import attention
    qkv = torch.randn(B, L, 3 * 64 * H, generator=torch.Generator().manual_seed(B * 1000 + L)) * 1.5
    ref = _reference64(qkv, H, causal)
    with _arith(f16):
        got = attention(qkv.cuda().contiguous(), H, causal).cpu().double()
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    print(f"attention_long float64 B={B} L={L} H={H} causal={causal} f16={f16}: max abs err {err:.3e}")
    assert err < 2e-5, err


# ---- 2. forced onto 64 < L <= 288: the bits of the shipped kernels ----------------------------------------------------------
def _all_forms(qkv, H, causal):
    from lemon_amd.ops import attention, attention_split, attention_t, unpack_act_t
    B, L, _ = qkv.shape
    return (attention(qkv, H, causal), attention_split(qkv, H, causal, "f16x3"), attention_split(qkv, H, causal, "bf16x6"),
            unpack_act_t(attention_t(qkv, H, causal), B * L, H * 64))


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("B,L,H,causal", SHIPPED_SHAPES)
def test_streaming_kernels_reproduce_the_shipped_kernels_bit_for_bit(hip, B, L, H, causal, f16):
    lib = _lib()
    qkv = (torch.randn(B, L, 3 * H * 64, generator=torch.Generator().manual_seed(B * 1000 + L)) * 1.5).cuda()
    with _arith(f16):
        shipped = _all_forms(qkv, H, causal)
        prev = lib.lemon_attention_set_stream_min(64)
        assert prev == 288
        try:
            streamed = _all_forms(qkv, H, causal)
        finally:
            assert lib.lemon_attention_set_stream_min(prev) == 64
    for i, (a, b) in enumerate(zip(streamed, shipped)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))


# ---- 3. the split output forms hold the split of what attention() returns ----------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("B,L,H,causal", [(2, 577, 16, False), (2, 512, 8, True)])
def test_streaming_output_forms_equal_split_of_attention(hip, B, L, H, causal, f16):
    from lemon_amd.ops import attention, attention_split, attention_t, split_operand, unpack_act_t
    qkv = torch.randn(B, L, 3 * H * 64, generator=torch.Generator().manual_seed(B * 100 + L)).cuda()
    with _arith(f16):
        y = attention(qkv, H, causal)
        for scheme in ("bf16x6", "f16x3"):
            assert torch.equal(attention_split(qkv, H, causal, scheme), split_operand(y, scheme)), scheme
        y3 = split_operand(y, "f16x3").view(B * L, 3, H * 64)
        assert torch.equal(unpack_act_t(attention_t(qkv, H, causal), B * L, H * 64), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0))


# ---- 4. nothing outside the result is written, nothing depends on neighbours -------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("B,L,H,causal", [(3, 577, 2, False), (2, 300, 3, True), (1, 1025, 1, True)])
def test_streaming_attention_writes_exactly_its_result(hip, B, L, H, causal, f16):
    lib = _lib()
    from lemon_amd import _lib as L_
    W = 64 * H
    qkv = (torch.randn(B, L, 3 * W, generator=torch.Generator().manual_seed(B * 1000 + L)) * 1.5).cuda()
    rows_t = (B * L + TM - 1) // TM * TM
    assert rows_t > B * L                                     # (the tile-major form has rows it must leave alone)
    forms = [("lemon_attention_f32", B * L * W, torch.float32), ("lemon_attention_split3", B * L * 3 * W, torch.bfloat16),
             ("lemon_attention_f16x3", B * L * 3 * W // 2, torch.float16), ("lemon_attention_f16x3t", rows_t * W, torch.float16)]
    with _arith(f16):
        for name, nw, dtype in forms:
            buf = torch.full((nw + TAIL,), OUT_FILL, dtype=torch.int32, device="cuda")
            L_.check(getattr(lib, name)(_p(qkv), B, L, H, 64, int(causal), _p(buf), _stream()), name)
            torch.cuda.synchronize()
            assert bool((buf[nw:] == OUT_FILL).all()), f"{name}: the canary behind the output was written"
            body = buf[:nw].view(dtype)
            if name.endswith("f16x3t"):
                idx = _tiled_index(B * L, W).reshape(-1)
                owed = torch.zeros(body.numel(), dtype=torch.bool, device="cuda")
                owed[idx] = True
                owed[idx + TM * 16] = True
                assert int(owed.sum()) == 2 * B * L * W
                assert bool(torch.isfinite(body[owed].float()).all()), f"{name}: an owed element was not written"
                rest = body.view(torch.int16)[~owed]
                assert bool((rest == 0x7FF1).all()), f"{name}: rows beyond batch * seq_len were written"
            else:
                assert bool(torch.isfinite(body.float()).all()), f"{name}: an owed element was not written"


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("B,L,H,causal", [(3, 577, 4, False), (4, 300, 2, True)])
def test_streaming_attention_rows_do_not_depend_on_the_batch(hip, B, L, H, causal, f16):
    from lemon_amd.ops import attention, attention_t, unpack_act_t
    qkv = (torch.randn(B, L, 3 * H * 64, generator=torch.Generator().manual_seed(B * 1000 + L)) * 1.5).cuda()
    with _arith(f16):
        full = attention(qkv, H, causal)
        full_t = unpack_act_t(attention_t(qkv, H, causal), B * L, H * 64).view(B, L, H * 64)
        for i in range(B):
            one = qkv[i:i + 1].contiguous()
            assert torch.equal(attention(one, H, causal)[0], full[i]), i
            assert torch.equal(unpack_act_t(attention_t(one, H, causal), L, H * 64), full_t[i]), i


# ---- 5. limits ------------------------------------------------------------------------------------------------------------
def test_streaming_attention_limits(hip):
    from lemon_amd import _lib as L_, ops
    lib = _lib()
    limit = ops.ATTENTION_MAX_SEQ
    assert limit >= 4096
    qkv = (torch.randn(1, limit + 1, 3 * 64, generator=torch.Generator().manual_seed(5)) * 1.5).cuda()
    out = torch.full((1, limit + 1, 64), float("nan"), device="cuda")
    at_limit = qkv[:, :limit].contiguous()
    y = ops.attention(at_limit, 1, True)
    ref = _reference64(at_limit.cpu(), 1, True)
    assert float((y.cpu().double() - ref).abs().max()) < 2e-5
    for fn in (lib.lemon_attention_f32, lib.lemon_attention_split3, lib.lemon_attention_f16x3, lib.lemon_attention_f16x3t):
        rc = fn(_p(qkv), 1, limit + 1, 1, 64, 0, _p(out), _stream())
        assert rc != 0
        assert str(limit) in lib.lemon_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                       # a refused call writes nothing
    with pytest.raises(L_.LemonHipError):
        L_.check(lib.lemon_attention_f32(_p(qkv), 1, 577, 1, 80, 0, _p(out), _stream()), "lemon_attention_f32")
    assert "head_dim" in lib.lemon_last_error().decode()
    prev = lib.lemon_attention_set_stream_min(100)
    try:
        assert prev == 288
        for bad in (63, 289, 0, -5, 4096):
            assert lib.lemon_attention_set_stream_min(bad) < 0, bad
            assert "64 .. 288" in lib.lemon_last_error().decode()
        assert lib.lemon_attention_set_stream_min(64) == 100      # refused values changed nothing
        assert lib.lemon_attention_set_stream_min(288) == 64
    finally:
        lib.lemon_attention_set_stream_min(288)


# ---- 6 / 7. towers beyond 288 tokens against HF CLIP ----------------------------------------------------------------------------
L14 = dict(projection_dim=768, v=(1024, 24, 16, 4096, 14), t=(768, 12, 12, 3072))
_REF = {}                     # HF references on the CPU, computed once per module


def _hf_model(projection_dim, v, t, image_size, context, seed=0):
    """HF CLIPModel with the seeded weights of tests/test_gpu_encoder.py::hf_model, at another image size / context length"""
    from transformers import CLIPConfig, CLIPModel
    cfg = CLIPConfig(projection_dim=projection_dim,
                     vision_config=dict(hidden_size=v[0], num_hidden_layers=v[1], num_attention_heads=v[2],
                                        intermediate_size=v[3], image_size=image_size, patch_size=v[4]),
                     text_config=dict(hidden_size=t[0], num_hidden_layers=t[1], num_attention_heads=t[2],
                                      intermediate_size=t[3], vocab_size=49408, max_position_embeddings=context,
                                      eos_token_id=2, bos_token_id=0, pad_token_id=1))     # legacy ids => argmax EOT pooling
    torch.manual_seed(seed)
    hf = CLIPModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in hf.named_parameters():
            if p.dim() >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (0.02 if "embedding" in name else fan_in ** -0.5))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return hf


def _unwrap(o):
    return o if torch.is_tensor(o) else o.pooler_output


def _check_bars(tag, got, ref):
    # the bars of tests/test_gpu_encoder.py:90-92
    sc = float(ref.abs().max())
    d = float((got - ref).abs().max())
    dn = float((torch.nn.functional.normalize(got, dim=1) - torch.nn.functional.normalize(ref, dim=1)).abs().max())
    print(f"attention_long encoder {tag}: raw max abs diff {d:.3e} (scale {sc:.3f}), unit-norm max abs diff {dn:.3e}")
    assert d <= 1e-4 * max(1.0, sc), f"{tag}: raw max abs diff {d} (scale {sc})"
    assert dn <= 5e-6, f"{tag}: normalised max abs diff {dn}"


class _no_fallback:
    """Block._sdpa raises, ops.attention_t is counted: the forward inside must use the HIP attention and, in f16x3 mode, the chain"""

    def __init__(self, monkeypatch):
        from lemon_amd import ops
        from lemon_amd.clip import Block
        self.calls = 0
        real = ops.attention_t

        def counted(*a, **k):
            self.calls += 1
            return real(*a, **k)

        def refuse(*a, **k):
            raise AssertionError("Block._sdpa was called: the SDPA fallback is still taken beyond 288 tokens")

        monkeypatch.setattr(Block, "_sdpa", refuse)
        monkeypatch.setattr(ops, "attention_t", counted)


def _image_case():
    if "img" not in _REF:
        from lemon_amd.data import gpu_transform_batch
        hf = _hf_model(L14["projection_dim"], L14["v"], L14["t"], 336, 77)
        u8 = torch.randint(0, 256, (2, 48, 40, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).cuda()
        px = gpu_transform_batch(u8, 336)
        patches = gpu_transform_batch(u8, 336, patch=14)
        with torch.no_grad():
            ref = _unwrap(hf.get_image_features(pixel_values=px.cpu()))
        _REF["img"] = (hf.state_dict(), px, patches, ref)
    return _REF["img"]


@pytest.mark.parametrize("gemm", ["f16x3", "split", "f32"])
def test_encoder_336px_vit_l14_vs_hf_clip_without_the_sdpa_fallback(hip, gemm, monkeypatch):
    # the recipe of test_fused_gpu_encoder_vs_hf_clip_at_full_size at image_size 336: 577 tokens per image
    monkeypatch.setenv("LEMON_GEMM", gemm)
    from lemon_amd.clip import ClipConfig, LemonCLIP
    sd, px, patches, ref = _image_case()
    cfg = ClipConfig.named("vit-l-14-336")
    assert px.shape == (2, 3, 336, 336) and patches.shape == (2, 576, 3 * 14 * 14)
    ours = LemonCLIP(cfg).load_hf_state_dict(sd).eval().cuda()
    watch = _no_fallback(monkeypatch)
    got_nchw = ours.encode_image(px).cpu()
    n_first = watch.calls
    got_patch = ours.encode_image(patches).cpu()
    if gemm == "f16x3":        # one tile-major attention per chained block, twice (the pooled-row last block takes another route)
        assert (n_first, watch.calls) == (cfg.vision.layers - 1, 2 * (cfg.vision.layers - 1)), (n_first, watch.calls)
    _check_bars(f"vit-l-14-336/{gemm}/nchw", got_nchw, ref)
    _check_bars(f"vit-l-14-336/{gemm}/patch-major", got_patch, ref)


def _text_case():
    if "txt" not in _REF:
        import sys, os
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from test_gpu_encoder import ragged_ids
        # (a one-layer 64-wide vision tower: only the text tower is evaluated)
        hf = _hf_model(512, (64, 1, 1, 128, 32), (512, 12, 8, 2048), 224, 512)
        ids, mask = ragged_ids(7, 512, 49408, seed=3)                 # lengths 512, 3, 8, 9 and three in 4 .. 511
        short, smask = ragged_ids(7, 290, 49408, seed=4)              # every prompt at most 290 tokens, padded to the context
        ids2, mask2 = torch.zeros(7, 512, dtype=torch.long), torch.zeros(7, 512, dtype=torch.long)
        ids2[:, :290], mask2[:, :290] = short, smask
        with torch.no_grad():
            ref = _unwrap(hf.get_text_features(input_ids=ids, attention_mask=mask))
            ref2 = _unwrap(hf.get_text_features(input_ids=ids2, attention_mask=mask2))
        _REF["txt"] = (hf.state_dict(), ids, mask, ref, ids2, ref2)
    return _REF["txt"]


@pytest.mark.parametrize("gemm", ["f16x3", "split", "f32"])
def test_encoder_512_token_text_tower_vs_hf_clip_without_the_sdpa_fallback(hip, gemm, monkeypatch):
    # ragged prompts of 3 .. 512 tokens in one batch: the streaming kernel with the causal mask, EOT rows at very different depths
    monkeypatch.setenv("LEMON_GEMM", gemm)
    from lemon_amd.clip import ClipConfig, LemonCLIP, TowerConfig
    sd, ids, mask, ref, ids2, ref2 = _text_case()
    cfg = ClipConfig(context_length=512, vision=TowerConfig(64, 1, 1, 128))
    ours = LemonCLIP(cfg).load_hf_state_dict(sd).eval().cuda()
    watch = _no_fallback(monkeypatch)
    got = ours.encode_text(ids.cuda(), mask.cuda()).cpu()
    n_first = watch.calls
    got2 = ours.encode_text(ids2.cuda(), seq_len=296).cpu()          # the first bucket past the old limit
    if gemm == "f16x3":
        assert (n_first, watch.calls) == (cfg.text.layers - 1, 2 * (cfg.text.layers - 1)), (n_first, watch.calls)
    _check_bars(f"text-512/{gemm}/L=512", got, ref)
    _check_bars(f"text-512/{gemm}/L=296", got2, ref2)
