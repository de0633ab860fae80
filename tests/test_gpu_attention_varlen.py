"""GPU: attention with a key length per sequence (csrc/attention_varlen.hip: lemon_attention_{f32,split3,f16x3,f16x3t}_varlen),
the padding mask of the BERT text tower.

Every case goes through the C ABI on outputs pre-filled with attention_ref.OUT_FILL with attention_ref.TAIL canary words behind
them, B = 4 sequences of H = 2 heads, the families `gauss`, `peaked` and `onekey` of tests/attention_ref.py, both arithmetic
selections:
  1. float64: rows t < n_b within attention_ref.bound() of the float64 attention over qkv[b, :n_b], rows t >= n_b exactly 0,
     every row < seq_len written, the canaries intact -- at the tile counts 1, 2, 3, 5, 7 (two-block staging) and 9;
  2. the bits of the plain kernels: lengths = seq_len and lengths_dev = NULL in all four output forms, and rows t < n_b against
     the plain call on qkv[b, :n_b] wherever both have the same tile count;
  3. poison: NaN, +Inf and 1e30 in the Q, K and V of rows t >= n_b change no bit of any output form, with the operand lying in
     an arena of NaN;
  4. the split forms are the split / tile-major image of the fp32 form;
  5. sequences are independent (permutation), lengths are clamped to 1 .. seq_len;
  6. refusals write nothing."""
import ctypes

import pytest
import torch

from . import attention_ref as R
from .attention_ref import OUT_FILL, TAIL, TM, _arith, _tiled_index

pytestmark = pytest.mark.gpu

B, H, W = 4, 2, 128
FAMILIES = ("gauss", "peaked", "onekey")
SEQ_LENS = (8, 32, 40, 64, 72, 160, 224, 288)          # key tiles 1, 1, 2, 2, 3, 5, 7, 9
FORMS = ("f32", "split3", "f16x3", "f16x3t")
GUARD = 4096 + 4                                      # floats of NaN around the operand (16-byte aligned, not 256)
E_INVALID = -1


def _lib():
    from lemon_amd import _lib as L
    return L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _words(form, rows):
    """int32 words of an output of `rows` token rows in the given form"""
    if form == "f16x3t":
        return (rows + TM - 1) // TM * TM * W
    return {"f32": rows * W, "split3": rows * 3 * W, "f16x3": rows * 3 * W // 2}[form]


_QKV = {}


def _qkv(family, L):
    """[B, L, 3 W] float32 on the CPU, made once per (family, seq_len) and never written"""
    key = (family, L)
    if key not in _QKV:
        _QKV[key] = R.families()[family](B, L, H)
    return _QKV[key]


def _arena(qkv):
    """the operand as a view inside an allocation whose remainder is NaN"""
    n = qkv.numel()
    arena = torch.full((GUARD + n + GUARD,), float("nan"), device="cuda")
    arena[GUARD:GUARD + n] = qkv.reshape(-1).cuda()
    return arena, arena[GUARD:GUARD + n].view(qkv.shape)


def _run(form, qkv_dev, lengths, f16, varlen=True, hd=64, heads=H, expect=0):
    """one call through the C ABI -> the whole poisoned buffer (int32 words, canary checked).  lengths: list, None (NULL pointer)"""
    lib = _lib()
    nb, L = qkv_dev.shape[0], qkv_dev.shape[1]
    nw = _words(form, nb * L)
    buf = torch.full((nw + TAIL,), OUT_FILL, dtype=torch.int32, device="cuda")
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    with _arith(f16):
        if varlen:
            rc = getattr(lib, f"lemon_attention_{form}_varlen")(_p(qkv_dev), nb, L, heads, hd, _p(ln), _p(buf), _stream())
        else:
            rc = getattr(lib, f"lemon_attention_{form}")(_p(qkv_dev), nb, L, heads, hd, 0, _p(buf), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (form, rc, lib.lemon_last_error().decode())
    assert bool((buf[nw:] == OUT_FILL).all()), f"{form}: the canary behind the output was written"
    return buf[:nw]


def _f32(buf, nb, L):
    return buf.view(torch.float32).view(nb, L, W)


def _tiles(L):
    return (L + 31) // 32


def _lengths(L):
    return [1, L, 32 * (_tiles(L) - 1) + 1, L - 1]


def _clamp(n, L):
    return max(1, min(L, n))


# ---- 1. float64 -----------------------------------------------------------------------------------------------------------------
_BOUND = {}


def _bound(family, L, b, n):
    """(ref, bnd) of attention_ref.bound on qkv[b, :n], once per case"""
    key = (family, L, b, n)
    if key not in _BOUND:
        _BOUND[key] = R.bound(_qkv(family, L)[b:b + 1, :n].contiguous(), H, False)
    return _BOUND[key]


def _check_float64(tag, family, L, lengths, f16):
    qkv = _qkv(family, L)
    buf = _run("f32", qkv.cuda(), lengths, f16)
    assert not bool((buf == OUT_FILL).any()), f"{tag}: a row below seq_len was not written"
    got = _f32(buf, B, L).cpu().double()
    worst = 0.0
    for b, n in enumerate(lengths):
        n = _clamp(n, L)
        ref, bnd = _bound(family, L, b, n)
        ratio = float(((got[b, :n] - ref[0]).abs() / bnd[0]).max())
        worst = max(worst, ratio)
        assert bool(torch.isfinite(got[b, :n]).all()) and ratio <= 1.0, (tag, b, n, ratio)
        assert bool((got[b, n:] == 0).all()), f"{tag}: sequence {b}: rows >= {n} are not zero"
    print(f"attention_varlen float64 {tag}: lengths {lengths} worst error / bound {worst:.3f}")


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L", SEQ_LENS)
def test_varlen_rows_match_float64_and_pads_are_zero(hip, L, family, f16):
    tag = f"{family} L={L} f16={f16}"
    _check_float64(tag, family, L, _lengths(L), f16)
    if L > 32:
        _check_float64(tag, family, L, [32, min(33, L), 31, 32], f16)


# ---- 2. the bits of the plain kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("L", SEQ_LENS)
def test_full_lengths_and_null_lengths_give_the_plain_bits_in_every_form(hip, L, f16):
    qkv = _qkv("gauss", L).cuda()
    for form in FORMS:
        plain = _run(form, qkv, None, f16, varlen=False)
        assert torch.equal(_run(form, qkv, [L] * B, f16), plain), (form, "lengths = seq_len")
        assert torch.equal(_run(form, qkv, None, f16), plain), (form, "lengths_dev = NULL")


PAIRS = {32: (1, 17, 32), 40: (33, 40), 64: (33, 57, 64), 160: (129, 160), 224: (193, 200, 224), 288: (257, 288)}


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L", sorted(PAIRS))
def test_rows_inside_a_sequence_carry_the_bits_of_the_plain_call_on_its_own_tokens(hip, L, family, f16):
    qkv = _qkv(family, L)
    ns = PAIRS[L]
    assert all(_tiles(n) == _tiles(L) for n in ns)           # same tile count, hence the same kernel family and walk
    lengths = [ns[b % len(ns)] for b in range(B)]
    got = _f32(_run("f32", qkv.cuda(), lengths, f16), B, L)
    for n in ns:
        cut = qkv[:, :n].contiguous().cuda()
        plain = _f32(_run("f32", cut, None, f16, varlen=False), B, n)
        for b in range(B):
            if lengths[b] == n:
                assert torch.equal(got[b, :n].view(torch.int32), plain[b].view(torch.int32)), (L, n, b)
                assert bool((got[b, n:] == 0).all()), (L, n, b)


# ---- 3. poison ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), 1e30], ids=["nan", "inf", "1e30"])
@pytest.mark.parametrize("L", [32, 64, 160, 224, 288])
def test_rows_beyond_a_sequence_reach_no_output(hip, L, poison, f16):
    lengths = _lengths(L)
    lengths[1] = max(1, L - 9)                               # (every sequence but one of full length has padded rows)
    lengths[3] = L
    clean = _qkv("gauss", L).clone()
    dirty = clean.clone()
    for b, n in enumerate(lengths):
        clean[b, n:] = 0.0
        dirty[b, n:] = poison                                # q, k and v of every head
    arena_c, qc = _arena(clean)
    arena_d, qd = _arena(dirty)
    for form in FORMS:
        want = _run(form, qc, lengths, f16)
        got = _run(form, qd, lengths, f16)
        assert torch.equal(got, want), (form, poison)
        if form == "f32":
            y = _f32(got, B, L)
            for b, n in enumerate(lengths):
                assert bool(torch.isfinite(y[b, :n]).all()) and bool((y[b, n:] == 0).all()), (b, n)
                assert bool((y[b, n:].view(torch.int32) == 0).all())
    n_el = clean.numel()
    for arena in (arena_c, arena_d):
        assert bool(torch.isnan(arena[:GUARD]).all()) and bool(torch.isnan(arena[GUARD + n_el:]).all())


# ---- 4. the split forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("L", [40, 72, 224, 288])
def test_split_forms_are_the_image_of_the_fp32_form(hip, L, f16):
    from lemon_amd.ops import split_operand, unpack_act_t
    qkv = _qkv("peaked", L).cuda()
    lengths = _lengths(L)
    y = _f32(_run("f32", qkv, lengths, f16), B, L).contiguous()
    got6 = _run("split3", qkv, lengths, f16).view(torch.bfloat16).view(B, L, 6 * W)
    got3 = _run("f16x3", qkv, lengths, f16).view(torch.float16).view(B, L, 3 * W)
    assert torch.equal(got6.view(torch.int16), split_operand(y, "bf16x6").view(torch.int16))
    want3 = split_operand(y, "f16x3")
    assert torch.equal(got3.view(torch.int16), want3.view(torch.int16))
    for b, n in enumerate(lengths):
        assert bool((got6[b, n:].view(torch.int16) == 0).all()) and bool((got3[b, n:].view(torch.int16) == 0).all()), b
    # tile-major: hi and lo 2^11 of every owed element, nothing else written
    bt = _run("f16x3t", qkv, lengths, f16)
    body = bt.view(torch.float16)
    idx = _tiled_index(B * L, W).reshape(-1)
    owed = torch.zeros(body.numel(), dtype=torch.bool, device="cuda")
    owed[idx] = True
    owed[idx + TM * 16] = True
    assert bool((body.view(torch.int16)[~owed] == 0x7FF1).all()), "rows beyond batch * seq_len were written"
    w3 = want3.view(B * L, 3, W)
    assert torch.equal(body[idx].view(torch.int16), w3[:, 0].reshape(-1).view(torch.int16))
    assert torch.equal(body[idx + TM * 16].view(torch.int16), w3[:, 2].reshape(-1).view(torch.int16))
    assert torch.equal(unpack_act_t(body, B * L, W), w3[:, 0].float() + w3[:, 2].float() * (1.0 / 2048.0))


# ---- 5. independence and clamping ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("L", [40, 160, 224])
def test_sequences_are_independent_and_lengths_are_clamped(hip, L, f16):
    qkv = _qkv("onekey", L)
    lengths = _lengths(L)
    perm = [2, 0, 3, 1]
    for form in ("f32", "f16x3"):
        a = _run(form, qkv.cuda(), lengths, f16).view(B, -1)
        p = _run(form, qkv[perm].contiguous().cuda(), [lengths[i] for i in perm], f16).view(B, -1)
        assert torch.equal(p, a[perm]), form
    lo_hi = _run("f32", qkv.cuda(), [0, L + 5, -7, 2 ** 31 - 1], f16)
    assert torch.equal(lo_hi, _run("f32", qkv.cuda(), [1, L, 1, L], f16))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_are_refused_and_write_nothing(hip):
    lib = _lib()

    def refused(form, qkv, lengths, word, hd=64, heads=H, batch=None):
        nb = qkv.shape[0] if batch is None else batch
        nw = _words(form, qkv.shape[0] * qkv.shape[1])
        buf = torch.full((nw + TAIL,), OUT_FILL, dtype=torch.int32, device="cuda")
        ln = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        rc = getattr(lib, f"lemon_attention_{form}_varlen")(_p(qkv), nb, qkv.shape[1], heads, hd, _p(ln), _p(buf), _stream())
        torch.cuda.synchronize()
        assert rc == E_INVALID, (form, rc)
        assert word in lib.lemon_last_error().decode(), lib.lemon_last_error().decode()
        assert bool((buf == OUT_FILL).all()), f"{form}: a refused call wrote"

    long = torch.randn(2, 289, 3 * W, device="cuda")
    wide = torch.randn(2, 40, 3 * H * 80, device="cuda")
    ok = torch.randn(2, 40, 3 * W, device="cuda")
    for f16 in (1, 0):
        with _arith(f16):
            for form in FORMS:
                refused(form, long, [289, 5], "seq_len")
                refused(form, ok, [40, 5], "batch", batch=-1)
                for mode in (0, 1):
                    prev = lib.lemon_attention_set_head_dims(mode)
                    try:
                        refused(form, wide, [40, 5], "head_dim", hd=80)
                    finally:
                        lib.lemon_attention_set_head_dims(prev)
    assert lib.lemon_attention_get_head_dims() == 0
