"""GPU: the streaming attention kernels at every block edge -- k_attention_hd64_stream (fp32 arithmetic, 4 waves, 64 keys per
block), k_attention_hd64_stream_f16 (split-fp16 arithmetic, 8 waves, 128 keys per block; both csrc/attention.hip, L > 288) and
k_attention_hdx_stream<96|128> (csrc/attention_hd.hip: head dims 72 .. 128 at every L) -- on the nine input families of
tests/attention_ref.py: stream_families(), three of them built for the online softmax (tests/test_attention_stream_host.py shows on
the CPU what each is for and that the bound rejects a wrong rescale, a wrong skip of it and a causal workgroup that stops early).

STREAM_GRID: TJ = ceil(L / 32) = 10 .. 19, so the even deal of query tiles gives 3, 4 and 5 workgroups of the fp32 form and 2 and
3 of the split-fp16 form, even deals (TJ 12, 16) and deals with an idle wave (10, 13, 17, 19), full and partial last key blocks
in both forms, and the last row of a tile, one short of it and one past it.  HD_GRID: the same around every tile and key-block
edge of the hdx kernel from one token up, at the narrowest head dim of either instantiation (72, 104), the widest (96, 128), 80.

  a. hd 64 beyond 288 tokens: float64 reference with the per-element bound (and the project's 2e-5 bar on gauss), nine families
  b. the same for hdx at five head dims
  c. equality chains on stress input, bit for bit in all four output forms: the streaming kernels forced onto 64 < L <= 288 =
     the one-workgroup kernels; hdx at head dim 64 (mode 2) = the shipped fp32-arithmetic kernels
  d. the split output forms hold exactly the split of what attention() returns
  e. NaN / Inf neighbours in memory (the next batch element, the bytes around the operand) cannot reach a result

Records of one MI355X run (records, not thresholds: the threshold is the bound with C = 2).  Worst |got - ref| / bound of (a) and
(b), 1.0 = the bound; they are printed, one "attention_stream_edges ratio | kernel | ..." line per case and family and one
"... worst | kernel | ..." line per case (pytest -s):
  k_attention_hd64_stream      fp32                  0.290  (L 513 causal, offset)
  k_attention_hd64_stream_f16  split-fp16            0.469  (L 577 causal, onekey)
  k_attention_hdx_stream<96>   set_f16(1) / (0)      0.364  (hd 96, L 31 causal, offset) / 0.263
  k_attention_hdx_stream<128>  set_f16(1) / (0)      0.406  (hd 104, L 256 causal, offset) / 0.333
(on the CPU the emulations reach 0.48, tests/test_attention_stream_host.py).  Wall time of this file: 12.5 s for its 514 cases,
most of it the float64 references.  With the rescale skipped on __any(alpha == 1) instead of __all, or with a causal workgroup
stopping one key tile early, built into all three kernels, 314 and 191 of the cases fail, (a) and (b) with the ratios the CPU
emulation of that fault predicts."""
import collections

import pytest
import torch

from .attention_ref import _arith, _lib, bound, stream_families
from .test_gpu_attention_hd import _mode
from .test_gpu_attention_short import GRID as SHORT_GRID
from .test_gpu_attention_short import _heads as _short_heads

pytestmark = pytest.mark.gpu

STREAM_GRID = [289, 319, 320, 321, 352, 353, 384, 385, 416, 417, 448, 449, 480, 481, 512, 513, 544, 545, 576, 577]
HD_GRID = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 161, 256, 257, 289, 321]
HEAD_DIMS = [72, 80, 96, 104, 128]
HD_F32_L = {72: 33, 80: 65, 96: 129, 104: 257, 128: 321}     # arithmetic selection 0 is the same kernel: one length per head dim
MODE2_GRID = [65, 129, 288, 289, 321, 417, 577]
B = 2
FORMS = ("f32", "bf16x6", "f16x3", "tiled")
NAMES = list(stream_families())
CHAIN_FAMILIES = ("peaked", "onekey", "ascending", "onerow")
_CASES = collections.OrderedDict()    # (hd, L, H, causal) -> {family: (qkv on the CPU, float64 reference, bound)}: never modified
_KEEP = 2                             # groups held (the arithmetic selections of a case follow each other: computed once)
_WORST = {}                           # kernel -> worst ratio of this run


def _heads(grid, L):
    """2 or 3 heads, alternating along the grid: with 3 the head offsets are odd multiples of 256 bytes at head dim 64"""
    return 2 + grid.index(L) % 2


def _group(hd, L, H, causal):
    key = (hd, L, H, causal)
    if key not in _CASES:
        fam = stream_families(hd)
        group = {}
        for name in NAMES:
            qkv = fam[name](B, L, H)
            group[name] = (qkv,) + bound(qkv, H, causal, hd=hd)
        _CASES[key] = group
        while len(_CASES) > _KEEP:
            _CASES.popitem(last=False)
    return _CASES[key]


def _form(qkv, H, causal, form):
    """one output form as a [B, L, *] tensor"""
    from lemon_amd.ops import attention, attention_split, attention_t, unpack_act_t
    Bq, L, W3 = qkv.shape
    if form == "f32":
        return attention(qkv, H, causal)
    if form == "tiled":
        return unpack_act_t(attention_t(qkv, H, causal), Bq * L, W3 // 3).view(Bq, L, W3 // 3)
    return attention_split(qkv, H, causal, form)


def _all_forms(qkv, H, causal):
    return [_form(qkv, H, causal, f) for f in FORMS]


def _within_the_bound(kernel, hd, L, H, causal, f16):
    from lemon_amd.ops import attention
    worst = 0.0
    for family, (qkv, ref, bnd) in _group(hd, L, H, causal).items():
        with _mode(0 if hd == 64 else 1), _arith(f16):
            got = attention(qkv.cuda(), H, causal).cpu().double()
        assert got.shape == ref.shape
        assert bool(torch.isfinite(got).all()), family
        err = (got - ref).abs()
        ratio = float((err / bnd).max())
        worst = max(worst, ratio)
        print(f"attention_stream_edges ratio | {kernel} | hd={hd} L={L} causal={causal} H={H} {family}: {ratio:.3f} of the bound, "
              f"max abs err {float(err.max()):.3e}")
        assert bool((err <= bnd).all()), (family, ratio)
        if family == "gauss":
            assert float(err.max()) < 2e-5, float(err.max())
    _WORST[kernel] = max(_WORST.get(kernel, 0.0), worst)
    print(f"attention_stream_edges worst | {kernel} | hd={hd} L={L} causal={causal}: {worst:.3f} (this run so far: {_WORST[kernel]:.3f})")


# ---- a. head dim 64 beyond 288 tokens: float64 reference at every block edge ------------------------------------------------------
@pytest.mark.parametrize("L,causal,f16", [(L, causal, f16) for L in STREAM_GRID for causal in (False, True) for f16 in (1, 0)])
def test_streaming_attention_matches_float64_within_the_bound(hip, L, causal, f16):
    kernel = "k_attention_hd64_stream_f16 split-fp16" if f16 else "k_attention_hd64_stream fp32"
    _within_the_bound(kernel, 64, L, _heads(STREAM_GRID, L), causal, f16)


# ---- b. head dims 72 .. 128 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,L,causal,f16", [(hd, L, causal, f16) for hd in HEAD_DIMS for L in HD_GRID for causal in (False, True)
                                             for f16 in ((1, 0) if L == HD_F32_L[hd] else (1,))])
def test_head_dim_attention_matches_float64_within_the_bound(hip, hd, L, causal, f16):
    kernel = f"k_attention_hdx_stream<{96 if hd <= 96 else 128}> set_f16({f16})"
    _within_the_bound(kernel, hd, L, _heads(HD_GRID, L), causal, f16)


# ---- c. equality chains on stress input -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [L for L in SHORT_GRID if L > 64])
def test_forced_streaming_equals_the_one_workgroup_kernels_on_stress_input(hip, L, causal, f16):
    lib = _lib()
    H = _short_heads(L)
    fam = stream_families(64)
    for family in CHAIN_FAMILIES:
        qkv = fam[family](B, L, H).cuda()
        with _arith(f16):
            shipped = _all_forms(qkv, H, causal)
            prev = lib.lemon_attention_set_stream_min(64)
            try:
                streamed = _all_forms(qkv, H, causal)
            finally:
                assert lib.lemon_attention_set_stream_min(prev) == 64
        for form, a, b in zip(FORMS, streamed, shipped):
            assert bool(torch.isfinite(b.float()).all()), (family, form)
            assert torch.equal(a, b), ("streaming vs shipped kernel", family, form, float((a.float() - b.float()).abs().max()))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", MODE2_GRID)
def test_mode_2_equals_the_shipped_fp32_kernels_on_stress_input(hip, L, causal):
    H = _heads(MODE2_GRID, L)
    fam = stream_families(64)
    for family in CHAIN_FAMILIES:
        qkv = fam[family](B, L, H).cuda()
        with _arith(0):
            with _mode(0):
                shipped = _all_forms(qkv, H, causal)
            with _mode(2):
                new = _all_forms(qkv, H, causal)
        for form, a, b in zip(FORMS, new, shipped):
            assert bool(torch.isfinite(b.float()).all()), (family, form)
            assert torch.equal(a, b), ("hdx at head dim 64 vs shipped kernel", family, form, float((a.float() - b.float()).abs().max()))


# ---- d. the split output forms hold the split of what attention() returns -----------------------------------------------------------
def _forms_equal_the_split(hd, L, H, causal, f16):
    from lemon_amd.ops import attention, attention_split, attention_t, split_operand, unpack_act_t
    W = H * hd
    assert W % 16 == 0
    fam = stream_families(hd)
    for family in ("onekey", "ascending"):
        qkv = fam[family](B, L, H).cuda()
        with _mode(0 if hd == 64 else 1), _arith(f16):
            y = attention(qkv, H, causal)
            assert bool(torch.isfinite(y).all()), family
            for scheme in ("bf16x6", "f16x3"):
                assert torch.equal(attention_split(qkv, H, causal, scheme), split_operand(y, scheme)), (family, scheme)
            y3 = split_operand(y, "f16x3").view(B * L, 3, W)
            assert torch.equal(unpack_act_t(attention_t(qkv, H, causal), B * L, W), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0)), family


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", STREAM_GRID[::3])
def test_streaming_output_forms_equal_split_of_attention(hip, L, causal, f16):
    _forms_equal_the_split(64, L, _heads(STREAM_GRID, L), causal, f16)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [33, 65, 129, 257, 321])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_head_dim_output_forms_equal_split_of_attention(hip, hd, L, causal):
    _forms_equal_the_split(hd, L, 2, causal, 1)           # (two heads: the tile-major form wants heads * hd a multiple of 16)


# ---- e. neighbours in memory cannot reach a result ------------------------------------------------------------------------------------
NEIGHBOUR_CASES = [(64, L, f16) for L in (289, 321, 417, 577) for f16 in (1, 0)] + [(72, 33, 1), (80, 65, 1), (96, 129, 1), (104, 257, 1), (128, 321, 1)]
GUARD = 16384 + 4             # floats of NaN in front of the operand (64 KB and one 16-byte step: aligned to 16 bytes, not to 256)


def _neighbour_heads(hd, L):
    return 2 if hd != 64 else 2 + L % 2                   # (321 and 417 with two heads, 289 and 577 with three)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("hd,L,f16", NEIGHBOUR_CASES)
def test_a_poisoned_batch_element_does_not_reach_its_neighbours(hip, hd, L, f16, causal):
    H = _neighbour_heads(hd, L)
    clean = stream_families(hd)["gauss"](3, L, H).cuda()
    with _mode(0 if hd == 64 else 1), _arith(f16):
        alone = [_all_forms(clean[i:i + 1].contiguous(), H, causal) for i in (0, 2)]
        for poison in (float("nan"), float("inf")):
            qkv = clean.clone()
            qkv[1] = poison
            for form, y in zip(FORMS, _all_forms(qkv, H, causal)):
                for n, i in enumerate((0, 2)):
                    assert bool(torch.isfinite(y[i].float()).all()), (form, poison, i)
                    assert torch.equal(y[i], alone[n][FORMS.index(form)][0]), (form, poison, i)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("hd,L,f16", NEIGHBOUR_CASES)
def test_bytes_around_the_operand_do_not_reach_a_result(hip, hd, L, f16, causal):
    # the operand is a view inside one larger allocation of the test's own whose remainder is NaN: a read that strays past either
    # end of qkv stays inside memory this test owns and shows up in the result
    H = _neighbour_heads(hd, L)
    fresh = stream_families(hd)["gauss"](B, L, H).cuda()
    n = fresh.numel()
    assert n % 4 == 0
    arena = torch.full((GUARD + n + GUARD,), float("nan"), device="cuda")
    inside = arena[GUARD:GUARD + n].view(B, L, 3 * H * hd)
    inside.copy_(fresh)
    assert inside.data_ptr() % 16 == 0 and inside.data_ptr() % 256 != 0 and inside.is_contiguous()
    assert inside.data_ptr() - arena.data_ptr() >= 65536 and (arena.numel() - GUARD - n) * 4 >= 65536
    with _mode(0 if hd == 64 else 1), _arith(f16):
        for form, a, b in zip(FORMS, _all_forms(inside, H, causal), _all_forms(fresh, H, causal)):
            assert bool(torch.isfinite(b.float()).all()), form
            assert torch.equal(a, b), form
    assert bool(torch.isnan(arena[:GUARD]).all()) and bool(torch.isnan(arena[GUARD + n:]).all())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("hd,L,f16", NEIGHBOUR_CASES)
def test_rows_do_not_depend_on_the_batch(hip, hd, L, f16, causal):
    H = _neighbour_heads(hd, L)
    qkv = stream_families(hd)["gauss"](4, L, H).cuda()
    with _mode(0 if hd == 64 else 1), _arith(f16):
        full = _all_forms(qkv, H, causal)
        for i in range(4):
            for form, y, one in zip(FORMS, full, _all_forms(qkv[i:i + 1].contiguous(), H, causal)):
                assert torch.equal(one[0], y[i]), (form, i)
