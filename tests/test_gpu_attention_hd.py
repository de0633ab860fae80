"""GPU: attention at head dims 72 .. 128 (csrc/attention_hd.hip: k_attention_hdx_stream<HDP, SPLIT>) behind
lemon_attention_set_head_dims -- the ViT-H/14 (80), g/14 (88) and bigG/14 (104) towers on the hand-written path.

Kernel level: float64 reference at the project's bar for this input distribution (2e-5, tests/test_gpu_attention_long.py), bit
equality with the shipped fp32-arithmetic kernels at head_dim 64 (mode 2), the split output forms, poisoned buffers through the
C ABI, batch independence, the switch.  GEMM level: the hand-written GEMM at the shapes of a 1280-wide tower (n-tile counts 5,
15 and 20) with the recipe and bars of tests/test_gpu_gemm_forms.py.  Tower level: ViT-H/14-shaped towers against HF CLIPModel
on the CPU with the SDPA fallback made to raise.  (Every tile and key-block edge at five head dims, stress input for the online
softmax, the per-element bound and NaN neighbours: tests/test_gpu_attention_stream_edges.py.)"""
import ctypes

import pytest
import torch

from . import test_gpu_gemm_forms as F
from .attention_ref import OUT_FILL, TAIL, TM, _arith, _tiled_index

pytestmark = pytest.mark.gpu

HEAD_DIMS = [72, 80, 88, 96, 104, 128]
SHAPES = [(1, 1, 1, False), (2, 33, 2, True), (1, 64, 3, False), (2, 65, 1, True), (1, 129, 2, False), (2, 257, 2, False),
          (1, 300, 1, True), (1, 577, 2, False)]
CASES_1 = [(hd,) + s for hd in HEAD_DIMS for s in SHAPES] + [(128, 1, 4096, 1, True)]


def _lib():
    from lemon_amd import _lib as L
    return L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _mode:
    """with _mode(m): the head-dim mode of the calling thread, restored on exit"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = _lib().lemon_attention_set_head_dims(self.mode)
        assert self.prev >= 0

    def __exit__(self, *a):
        _lib().lemon_attention_set_head_dims(self.prev)


def _qkv(B, L, H, hd, seed=None):
    g = torch.Generator().manual_seed(B * 1000 + L + 7919 * hd if seed is None else seed)
    return torch.randn(B, L, 3 * H * hd, generator=g) * 1.5


_REF64 = {}


def _reference64(B, L, H, hd, causal):
    """float64 attention of _qkv(B, L, H, hd) on the CPU, once per case"""
    key = (B, L, H, hd, causal)
    if key not in _REF64:
        q, k, v = _qkv(B, L, H, hd).double().view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
        s = q @ k.transpose(-1, -2) / float(hd) ** 0.5
        if causal:
            s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
        _REF64[key] = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, hd * H)
    return _REF64[key]


# ---- 1. float64 reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("hd,B,L,H,causal", CASES_1)
def test_head_dim_attention_matches_float64_reference(hip, hd, B, L, H, causal, f16):
    from lemon_amd.ops import attention
    ref = _reference64(B, L, H, hd, causal)
    with _mode(1), _arith(f16):
        got = attention(_qkv(B, L, H, hd).cuda().contiguous(), H, causal).cpu().double()
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    print(f"attention_hd float64 hd={hd} B={B} L={L} H={H} causal={causal} f16={f16}: max abs err {err:.3e}")
    assert err < 2e-5, err


# ---- 2. head_dim 64 through the new kernel: the bits of the shipped fp32-arithmetic kernels ----------------------------------
@pytest.mark.parametrize("B,L,H,causal", [(2, 65, 3, False), (3, 77, 8, True), (1, 257, 16, False), (2, 288, 2, True), (1, 577, 2, False)])
def test_mode_2_reproduces_the_shipped_kernels_bit_for_bit_at_head_dim_64(hip, B, L, H, causal):
    from lemon_amd.ops import attention, attention_split, attention_t, unpack_act_t
    qkv = _qkv(B, L, H, 64).cuda()

    def forms():
        return (attention(qkv, H, causal), attention_split(qkv, H, causal, "f16x3"), attention_split(qkv, H, causal, "bf16x6"),
                unpack_act_t(attention_t(qkv, H, causal), B * L, H * 64))

    with _arith(0):
        with _mode(0):
            shipped = forms()
        with _mode(2):
            new = forms()
    for i, (a, b) in enumerate(zip(new, shipped)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))


# ---- 3. the split output forms hold the split of what attention() returns ----------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("hd,B,L,H,causal", [(80, 2, 257, 16, False), (104, 2, 130, 4, True), (80, 1, 77, 2, True), (104, 1, 300, 8, False)])
def test_head_dim_output_forms_equal_split_of_attention(hip, hd, B, L, H, causal, f16):
    from lemon_amd.ops import attention, attention_split, attention_t, split_operand, unpack_act_t
    W = H * hd
    qkv = _qkv(B, L, H, hd).cuda()
    with _mode(1), _arith(f16):
        y = attention(qkv, H, causal)
        for scheme in ("bf16x6", "f16x3"):
            assert torch.equal(attention_split(qkv, H, causal, scheme), split_operand(y, scheme)), scheme
        y3 = split_operand(y, "f16x3").view(B * L, 3, W)
        assert torch.equal(unpack_act_t(attention_t(qkv, H, causal), B * L, W), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0))


# ---- 4. the hand-written GEMM at the shapes of a 1280-wide tower ---------------------------------------------------------------
GEMM_SHAPES = [(1280, 1280), (3840, 1280), (5120, 1280), (1280, 5120)]          # (n, k): n-tile counts 5, 15, 20 and 5
GEMM_M = (1, 130, 257)


def _gemm_cases():
    # bias and residual rotate with the form and m as in test_gpu_gemm_forms._cases: every form sees both settings of each
    out = []
    for form in sorted(F.FORMS):
        spec = F.FORMS[form]
        for n, k in GEMM_SHAPES:
            for i, m in enumerate(GEMM_M):
                j = i + form
                res = bool(spec.get("res_t")) or (spec["act"] is None and bool((j // 2) % 2))
                out.append((form, m, n, k, bool(j % 2), res))
    return out


GEMM_CASES = _gemm_cases()


@pytest.mark.parametrize("form,m,n,k,bias,res", GEMM_CASES,
                         ids=[f"f{c[0]}-m{c[1]}-n{c[2]}-k{c[3]}-{'b' if c[4] else 'nob'}-{'r' if c[5] else 'nor'}" for c in GEMM_CASES])
def test_gemm_forms_at_the_wide_tower_shapes(hip, form, m, n, k, bias, res):
    # every launch form (plain, FOLD, EMIT / chain) through the float64 check of tests/test_gpu_gemm_forms.py itself: poisoned
    # outputs, canary tails, the per-element bound C 2^-21 S, the emitted operands and row statistics
    F.test_gemm_form_against_float64(hip, form, m, n, k, bias, res)


# ---- 5. nothing outside the result is written, nothing depends on neighbours -------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("hd,B,L,H,causal", [(80, 3, 257, 2, False), (104, 2, 300, 2, True), (72, 1, 33, 2, True), (128, 1, 577, 1, False)])
def test_head_dim_attention_writes_exactly_its_result(hip, hd, B, L, H, causal, f16):
    lib = _lib()
    from lemon_amd import _lib as L_
    W = hd * H
    assert W % 16 == 0
    qkv = _qkv(B, L, H, hd).cuda()
    rows_t = (B * L + TM - 1) // TM * TM
    assert rows_t > B * L                                     # (the tile-major form has rows it must leave alone)
    forms = [("lemon_attention_f32", B * L * W, torch.float32), ("lemon_attention_split3", B * L * 3 * W, torch.bfloat16),
             ("lemon_attention_f16x3", B * L * 3 * W // 2, torch.float16), ("lemon_attention_f16x3t", rows_t * W, torch.float16)]
    with _mode(1), _arith(f16):
        for name, nw, dtype in forms:
            buf = torch.full((nw + TAIL,), OUT_FILL, dtype=torch.int32, device="cuda")
            L_.check(getattr(lib, name)(_p(qkv), B, L, H, hd, int(causal), _p(buf), _stream()), name)
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


@pytest.mark.parametrize("hd,B,L,H,causal", [(80, 3, 257, 4, False), (104, 4, 130, 2, True)])
def test_head_dim_attention_rows_do_not_depend_on_the_batch(hip, hd, B, L, H, causal):
    from lemon_amd.ops import attention, attention_t, unpack_act_t
    W = H * hd
    qkv = _qkv(B, L, H, hd).cuda()
    with _mode(1):
        full = attention(qkv, H, causal)
        full_t = unpack_act_t(attention_t(qkv, H, causal), B * L, W).view(B, L, W)
        for i in range(B):
            one = qkv[i:i + 1].contiguous()
            assert torch.equal(attention(one, H, causal)[0], full[i]), i
            assert torch.equal(unpack_act_t(attention_t(one, H, causal), L, W), full_t[i]), i


# ---- 6. the switch ----------------------------------------------------------------------------------------------------------
def test_head_dims_switch(hip):
    from lemon_amd import ops
    lib = _lib()
    assert lib.lemon_attention_get_head_dims() == 0, "the default is off"
    fns = (lib.lemon_attention_f32, lib.lemon_attention_split3, lib.lemon_attention_f16x3, lib.lemon_attention_f16x3t)
    L, H = 130, 2
    out = torch.full((4 * 256 * H * 136,), float("nan"), device="cuda")       # (room for every form at every head dim below)

    def refused(hd):
        qkv = _qkv(1, L, H, hd).cuda()
        for fn in fns:
            assert fn(_p(qkv), 1, L, H, hd, 0, _p(out), _stream()) != 0, hd
            assert "head_dim" in lib.lemon_last_error().decode()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), hd                  # a refused call writes nothing

    refused(80)                                                   # mode 0
    with _mode(1):
        assert lib.lemon_attention_get_head_dims() == 1
        for hd in (60, 68, 136, 32):
            refused(hd)
        for bad in (3, -1, 17):
            assert lib.lemon_attention_set_head_dims(bad) < 0, bad
            assert "mode" in lib.lemon_last_error().decode()
            assert lib.lemon_attention_get_head_dims() == 1       # a refused mode changes nothing
        with pytest.raises(Exception):
            ops.set_attention_head_dims(5)
        assert ops.attention_head_dims() == 1
        # head_dim 64 keeps its kernels under mode 1, in both arithmetic selections and on both sides of the streaming threshold
        for f16 in (1, 0):
            for (B, L64, H64, causal) in [(2, 50, 2, True), (1, 257, 4, False), (1, 577, 2, False)]:
                qkv = _qkv(B, L64, H64, 64).cuda()
                with _arith(f16):
                    on = ops.attention(qkv, H64, causal), ops.unpack_act_t(ops.attention_t(qkv, H64, causal), B * L64, 64 * H64)
                    with _mode(0):
                        off = ops.attention(qkv, H64, causal), ops.unpack_act_t(ops.attention_t(qkv, H64, causal), B * L64, 64 * H64)
                assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]), (f16, L64)
    assert lib.lemon_attention_get_head_dims() == 0
    assert ops.set_attention_head_dims(1) == 0 and ops.set_attention_head_dims(0) == 1


# ---- 7. ViT-H/14-shaped towers against HF CLIPModel on the CPU -----------------------------------------------------------------
_REF = {}


def _hf_model(projection_dim, v, t, image_size, context, hidden_act, seed=0):
    """HF CLIPModel with the seeded weights of _hf_model in tests/test_gpu_attention_long.py, with `hidden_act` in both towers"""
    from transformers import CLIPConfig, CLIPModel
    cfg = CLIPConfig(projection_dim=projection_dim,
                     vision_config=dict(hidden_size=v[0], num_hidden_layers=v[1], num_attention_heads=v[2], hidden_act=hidden_act,
                                        intermediate_size=v[3], image_size=image_size, patch_size=v[4]),
                     text_config=dict(hidden_size=t[0], num_hidden_layers=t[1], num_attention_heads=t[2], hidden_act=hidden_act,
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
    print(f"attention_hd encoder {tag}: raw max abs diff {d:.3e} (scale {sc:.3f}), unit-norm max abs diff {dn:.3e}")
    assert d <= 1e-4 * max(1.0, sc), f"{tag}: raw max abs diff {d} (scale {sc})"
    assert dn <= 5e-6, f"{tag}: normalised max abs diff {dn}"


MODELS = {
    # ViT-H/14 with two layers per tower: head_dim 80, 257 tokens, width 1280 = five n-tiles of the hand-written GEMM
    "h14": dict(projection_dim=1024, v=(1280, 2, 16, 5120, 14), t=(1024, 2, 16, 4096)),
    # head_dim 88 (g/14) at a width that is no multiple of 256: the library-GEMM route
    "w1408": dict(projection_dim=64, v=(1408, 1, 16, 5632, 14), t=(64, 1, 1, 128)),
}


def _case(name):
    if name not in _REF:
        import os
        import sys
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from test_gpu_encoder import ragged_ids
        from lemon_amd.data import gpu_transform_batch
        m = MODELS[name]
        hf = _hf_model(m["projection_dim"], m["v"], m["t"], 224, 77, "gelu")
        u8 = torch.randint(0, 256, (2, 48, 40, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).cuda()
        px = gpu_transform_batch(u8, 224)
        ids, mask = ragged_ids(5, 77, 49408, seed=3)
        with torch.no_grad():
            ref = _unwrap(hf.get_image_features(pixel_values=px.cpu()))
            ref_t = _unwrap(hf.get_text_features(input_ids=ids, attention_mask=mask))
        _REF[name] = (hf.config.to_dict(), hf.state_dict(), px, ref, ids, mask, ref_t)
    return _REF[name]


class _no_fallback:
    """Block._sdpa raises, ops.attention_t is counted"""

    def __init__(self, monkeypatch):
        from lemon_amd import ops
        from lemon_amd.clip import Block
        self.calls = 0
        real = ops.attention_t

        def counted(*a, **k):
            self.calls += 1
            return real(*a, **k)

        def refuse(*a, **k):
            raise AssertionError("Block._sdpa was called: the SDPA fallback is still taken at this head dim")

        monkeypatch.setattr(Block, "_sdpa", refuse)
        monkeypatch.setattr(ops, "attention_t", counted)


@pytest.mark.parametrize("gemm", ["f16x3", "split", "f32"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_wide_towers_vs_hf_clip_without_the_sdpa_fallback(hip, name, gemm, monkeypatch):
    monkeypatch.setenv("LEMON_GEMM", gemm)
    from lemon_amd.clip import ClipConfig, LemonCLIP
    cfg_dict, sd, px, ref, ids, mask, ref_t = _case(name)
    cfg = ClipConfig.from_hf_dict(cfg_dict)
    v = MODELS[name]["v"]
    assert cfg.hidden_act == "gelu" and (cfg.vision.width, cfg.vision.layers, cfg.vision.heads, cfg.vision.mlp) == v[:4]
    ours = LemonCLIP(cfg).load_hf_state_dict(sd).eval().cuda()
    watch = _no_fallback(monkeypatch)
    with _mode(1):
        got = ours.encode_image(px).cpu()
        n_img = watch.calls
        got_t = ours.encode_text(ids.cuda(), mask.cuda()).cpu()
    if gemm == "f16x3" and name == "h14":
        # one tile-major attention per chained block (the pooled-row last block takes another route): the chain ran at width 1280
        assert n_img == cfg.vision.layers - 1, n_img
    if name == "w1408":
        assert n_img == 0, n_img
    _check_bars(f"{name}/{gemm}/image", got, ref)
    _check_bars(f"{name}/{gemm}/text", got_t, ref_t)
