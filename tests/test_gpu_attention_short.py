"""GPU: the one-workgroup attention kernels of csrc/attention.hip that serve every sequence up to 288 tokens --
k_attention_hd64_short<1|2> (L <= 64), k_attention_hd64_f16 (staged, 64 < L <= 288, default arithmetic), k_attention_hd64<.., false>
(fp32 arithmetic, lemon_attention_set_f16(0)) and k_attention_hd64<.., true> (the first general fp16 kernel, set_f16(2)) -- at every
tile count TJ = ceil(L / 32) = 1 .. 9, on the last row of a tile, one short of it and one past it, in all four output forms.

  a. float64 reference with the per-element bound of tests/attention_ref.py on six input families (and the project's 2e-5 bar)
  b. the split output forms hold exactly the split of what attention() returns
  c. staged kernel = first general kernel = streaming kernel forced onto 64 < L <= 288, bit for bit, at every tile count
  d. poisoned buffers through the C ABI: a call writes exactly its result
  e. NaN / Inf neighbours in memory (the next batch element, the bytes around the operand) cannot reach a result
  f. limits

Worst |got - ref| / bound of (a), C = 2, per kernel and arithmetic (1.0 = the bound), one MI355X run (a record, not a threshold;
test (a) prints them, one "attention_short ratio | kernel | ..." line per case and family, pytest -s):
  k_attention_hd64_short<1|2>  fp32 / split-fp16     0.167 / 0.160  (L 63 causal, offset)
  k_attention_hd64<false>      fp32                  0.395  (L 224 causal, offset)
  k_attention_hd64_f16 (staged) and k_attention_hd64<true> (first general fp16)   0.480  (L 255 causal, tail_v)
On the CPU a plain fp32 evaluation reaches 0.32 and the emulation of the split arithmetic 0.44
(tests/test_attention_bound_host.py).  Wall time of this file on an MI355X: 4.3 s for its 409 cases.  The streaming kernels
beyond 288 tokens and the head dims beyond 64: tests/test_gpu_attention_stream_edges.py."""
import ctypes

import pytest
import torch

from .attention_ref import OUT_FILL, TAIL, TM, _arith, _lib, _p, _stream, _tiled_index, bound, families

pytestmark = pytest.mark.gpu

GRID = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256, 257, 287, 288]
B = 2
FORMS = ("f32", "bf16x6", "f16x3", "tiled")
_CASES = {}                   # (family, L, causal) -> (qkv on the CPU, float64 reference, bound): computed once, never modified


def _heads(L):
    """2 or 3 heads, alternating along the grid: with 3 the head offsets are odd multiples of 256 bytes"""
    return 2 + GRID.index(L) % 2 if L in GRID else 2 + L % 2


def _case(family, L, causal):
    key = (family, L, causal)
    if key not in _CASES:
        qkv = families()[family](B, L, _heads(L))
        _CASES[key] = (qkv,) + bound(qkv, _heads(L), causal)
    return _CASES[key]


def _kernel(L, f16):
    if L <= 64:
        return f"k_attention_hd64_short<{(L + 31) // 32}> " + ("fp32" if f16 == 0 else "split-fp16")
    return {1: "k_attention_hd64_f16 (staged)", 0: "k_attention_hd64<false> fp32", 2: "k_attention_hd64<true> first general fp16"}[f16]


def _form(qkv, H, causal, form):
    """one output form as a [B, L, *] tensor"""
    from lemon_amd.ops import attention, attention_split, attention_t, unpack_act_t
    Bq, L, _ = qkv.shape
    if form == "f32":
        return attention(qkv, H, causal)
    if form == "tiled":
        return unpack_act_t(attention_t(qkv, H, causal), Bq * L, H * 64).view(Bq, L, H * 64)
    return attention_split(qkv, H, causal, form)


def _all_forms(qkv, H, causal):
    return [_form(qkv, H, causal, f) for f in FORMS]


# ---- a. float64 reference at every tile edge ---------------------------------------------------------------------------------
# (arithmetic 2, the first general fp16 kernel, is another kernel only beyond 64 tokens)
@pytest.mark.parametrize("L,causal,f16", [(L, causal, f16) for L in GRID for causal in (False, True) for f16 in (1, 0, 2) if f16 != 2 or L > 64])
def test_attention_matches_float64_within_the_bound(hip, L, causal, f16):
    from lemon_amd.ops import attention
    H = _heads(L)
    worst = 0.0
    for family in families():
        qkv, ref, bnd = _case(family, L, causal)
        with _arith(f16):
            got = attention(qkv.cuda(), H, causal).cpu().double()
        assert got.shape == ref.shape
        assert bool(torch.isfinite(got).all()), family
        err = (got - ref).abs()
        ratio = float((err / bnd).max())
        worst = max(worst, ratio)
        print(f"attention_short ratio | {_kernel(L, f16)} | L={L} causal={causal} H={H} {family}: {ratio:.3f} of the bound, max abs err {float(err.max()):.3e}")
        assert bool((err <= bnd).all()), (family, ratio)
        if family == "gauss":
            assert float(err.max()) < 2e-5, float(err.max())
    print(f"attention_short worst | {_kernel(L, f16)} | L={L} causal={causal}: {worst:.3f}")


# ---- b. the split output forms hold the split of what attention() returns -----------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", GRID)
def test_output_forms_equal_split_of_attention(hip, L, causal, f16):
    from lemon_amd.ops import attention, attention_split, attention_t, split_operand, unpack_act_t
    H = _heads(L)
    for family in ("gauss", "onekey"):
        qkv = _case(family, L, causal)[0].cuda()
        with _arith(f16):
            y = attention(qkv, H, causal)
            for scheme in ("bf16x6", "f16x3"):
                assert torch.equal(attention_split(qkv, H, causal, scheme), split_operand(y, scheme)), (family, scheme)
            y3 = split_operand(y, "f16x3").view(B * L, 3, H * 64)
            assert torch.equal(unpack_act_t(attention_t(qkv, H, causal), B * L, H * 64), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0)), family


# ---- c. the equality chain at every tile count ----------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [L for L in GRID if L > 64])
def test_staged_general_and_streaming_kernels_agree_bit_for_bit(hip, L, causal):
    lib = _lib()
    H = _heads(L)
    qkv = _case("gauss", L, causal)[0].cuda()
    with _arith(1):
        staged = _all_forms(qkv, H, causal)
    with _arith(2):
        general = _all_forms(qkv, H, causal)
    for form, a, b in zip(FORMS, staged, general):
        assert torch.equal(a, b), ("staged vs first general kernel", form, float((a.float() - b.float()).abs().max()))
    for f16 in (1, 0):
        with _arith(f16):
            shipped = staged if f16 == 1 else _all_forms(qkv, H, causal)
            prev = lib.lemon_attention_set_stream_min(64)
            try:
                streamed = _all_forms(qkv, H, causal)
            finally:
                assert lib.lemon_attention_set_stream_min(prev) == 64
        for form, a, b in zip(FORMS, streamed, shipped):
            assert torch.equal(a, b), ("streaming vs shipped kernel", f16, form, float((a.float() - b.float()).abs().max()))


# ---- d. a call writes exactly its result ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("Bq,L,H", [(3, 1, 2), (3, 33, 3), (5, 50, 2), (3, 77, 2), (1, 130, 3), (2, 197, 2), (1, 288, 1), (2, 64, 2)])
def test_attention_writes_exactly_its_result(hip, Bq, L, H, f16):
    lib = _lib()
    from lemon_amd import _lib as L_
    W = 64 * H
    qkv = families()["gauss"](Bq, L, H).cuda()
    rows_t = (Bq * L + TM - 1) // TM * TM
    forms = [("lemon_attention_f32", Bq * L * W, torch.float32), ("lemon_attention_split3", Bq * L * 3 * W, torch.bfloat16),
             ("lemon_attention_f16x3", Bq * L * 3 * W // 2, torch.float16), ("lemon_attention_f16x3t", rows_t * W, torch.float16)]
    with _arith(f16):
        for causal in (0, 1):
            for name, nw, dtype in forms:
                buf = torch.full((nw + TAIL,), OUT_FILL, dtype=torch.int32, device="cuda")
                L_.check(getattr(lib, name)(_p(qkv), Bq, L, H, 64, causal, _p(buf), _stream()), name)
                torch.cuda.synchronize()
                assert bool((buf[nw:] == OUT_FILL).all()), f"{name}: the canary behind the output was written"
                body = buf[:nw].view(dtype)
                if name.endswith("f16x3t"):
                    idx = _tiled_index(Bq * L, W).reshape(-1)
                    owed = torch.zeros(body.numel(), dtype=torch.bool, device="cuda")
                    owed[idx] = True
                    owed[idx + TM * 16] = True
                    assert int(owed.sum()) == 2 * Bq * L * W
                    if rows_t == Bq * L:                              # no spare rows: the operand is all result
                        assert bool(owed.all())
                    else:
                        assert not bool(owed.all())
                    assert bool(torch.isfinite(body[owed].float()).all()), f"{name}: an owed element was not written"
                    rest = body.view(torch.int16)[~owed]
                    assert rest.numel() == 2 * (rows_t - Bq * L) * W
                    assert bool((rest == 0x7FF1).all()), f"{name}: rows beyond batch * seq_len were written"
                else:
                    assert bool(torch.isfinite(body.float()).all()), f"{name}: an owed element was not written"


# ---- e. neighbours in memory cannot reach a result ---------------------------------------------------------------------------------
NEIGHBOUR_L = [1, 33, 50, 77, 130, 197, 288]
GUARD = 16384 + 4             # floats of NaN in front of the operand (64 KB and one 16-byte step: aligned to 16 bytes, not to 256)


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", NEIGHBOUR_L)
def test_a_poisoned_batch_element_does_not_reach_its_neighbours(hip, L, causal, f16):
    H = _heads(L)
    clean = families()["gauss"](3, L, H).cuda()
    with _arith(f16):
        alone = [_all_forms(clean[i:i + 1].contiguous(), H, causal) for i in (0, 2)]
        for poison in (float("nan"), float("inf")):
            qkv = clean.clone()
            qkv[1] = poison
            for form, y in zip(FORMS, _all_forms(qkv, H, causal)):
                for n, i in enumerate((0, 2)):
                    assert bool(torch.isfinite(y[i].float()).all()), (form, poison, i)
                    assert torch.equal(y[i], alone[n][FORMS.index(form)][0]), (form, poison, i)


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", NEIGHBOUR_L)
def test_bytes_around_the_operand_do_not_reach_a_result(hip, L, causal, f16):
    # the operand is a view inside one larger allocation of the test's own whose remainder is NaN: a read that strays past either
    # end of qkv stays inside memory this test owns and shows up in the result
    H = _heads(L)
    fresh = families()["gauss"](B, L, H).cuda()
    n = fresh.numel()
    assert n % 4 == 0
    arena = torch.full((GUARD + n + GUARD,), float("nan"), device="cuda")
    inside = arena[GUARD:GUARD + n].view(B, L, 3 * H * 64)
    inside.copy_(fresh)
    assert inside.data_ptr() % 16 == 0 and inside.data_ptr() % 256 != 0 and inside.is_contiguous()
    assert inside.data_ptr() - arena.data_ptr() >= 65536 and (arena.numel() - GUARD - n) * 4 >= 65536
    with _arith(f16):
        for form, a, b in zip(FORMS, _all_forms(inside, H, causal), _all_forms(fresh, H, causal)):
            assert bool(torch.isfinite(b.float()).all()), form
            assert torch.equal(a, b), form
    assert bool(torch.isnan(arena[:GUARD]).all()) and bool(torch.isnan(arena[GUARD + n:]).all())


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", NEIGHBOUR_L)
def test_rows_do_not_depend_on_the_batch(hip, L, causal, f16):
    H = _heads(L)
    qkv = families()["gauss"](4, L, H).cuda()
    with _arith(f16):
        full = _all_forms(qkv, H, causal)
        for i in range(4):
            for form, y, one in zip(FORMS, full, _all_forms(qkv[i:i + 1].contiguous(), H, causal)):
                assert torch.equal(one[0], y[i]), (form, i)


# ---- f. limits -------------------------------------------------------------------------------------------------------------------
def test_attention_limits(hip):
    lib = _lib()
    H, L = 2, 50
    qkv = families()["gauss"](2, L, H).cuda()
    out = torch.full((2 * L * 3 * 64 * H + TAIL,), OUT_FILL, dtype=torch.int32, device="cuda")     # room for the largest form
    fns = (lib.lemon_attention_f32, lib.lemon_attention_split3, lib.lemon_attention_f16x3, lib.lemon_attention_f16x3t)
    for f16 in (1, 0):
        with _arith(f16):
            for fn in fns:
                assert fn(_p(qkv), 0, L, H, 64, 0, _p(out), _stream()) == 0                        # an empty batch is no error
                assert fn(_p(qkv), 2, 0, H, 64, 0, _p(out), _stream()) != 0
                assert "seq_len > 0" in lib.lemon_last_error().decode()
                assert fn(_p(qkv), 2, L, 0, 64, 0, _p(out), _stream()) != 0
                assert "heads > 0" in lib.lemon_last_error().decode()
                assert fn(ctypes.c_void_p(qkv.data_ptr() + 4), 1, L, H, 64, 0, _p(out), _stream()) != 0
                assert "alignment" in lib.lemon_last_error().decode()
                assert fn(_p(qkv), 1, L, H, 64, 0, ctypes.c_void_p(out.data_ptr() + 4), _stream()) != 0
                assert "alignment" in lib.lemon_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == OUT_FILL).all())                                                           # none of these calls wrote
