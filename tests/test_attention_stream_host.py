"""CPU: what tests/test_gpu_attention_stream_edges.py asserts of the streaming attention kernels (k_attention_hd64_stream,
k_attention_hd64_stream_f16, k_attention_hdx_stream) can tell a correct online softmax from a subtly wrong one.  On the nine input
families of tests/attention_ref.py: stream_families(), at 289 .. 577 tokens and head dims 64, 80 and 128, a plain fp32 evaluation,
an emulation of the kernels' per-tile running maximum / sum / rescale (the deal of query tiles to workgroups and the key blocks of
both streaming geometries) and, at head dim 64, the emulation of the split-fp16 arithmetic stay within half the bound; the
emulation with one planted fault -- an accumulator or a running sum that is not rescaled, a rescale skipped on __any instead of
__all, a causal workgroup that stops one key tile early -- leaves the bound on every family of SHOWS_ON.  The three families built
for the online softmax have the property they are named for: in `ascending` the maximum moves in every tile, in `firstkey` never
after the first, in `onerow` for some rows of a wave and not for others.  No kernel has to be broken to know that."""
import pytest
import torch

from .attention_ref import (FAULTS, STREAM_FAULTS, bound, emulate_split, emulate_stream, evaluate_f32, families, stream_deal,
                            stream_families)

CASES = [(289, False), (321, True), (417, True), (577, False), (577, True)]
GEOMETRIES = [(64, 4, 2), (80, 4, 2), (128, 4, 2), (64, 8, 4)]          # (hd, wmax, tb): fp32 form, hdx narrow, hdx wide, split-fp16 form
B, H = 2, 2
NAMES = ["gauss", "peaked", "flat", "offset", "tail_v", "onekey", "ascending", "firstkey", "onerow"]
# established here on the CPU: where the maximum never moves after the first tile (flat: all logits 0; firstkey) alpha is 1 and a
# missing rescale changes nothing
# missing rescale changes nothing; where it moves for every row in every tile (ascending) __any(alpha == 1) is as false as __all
_MOVING = ("gauss", "peaked", "offset", "tail_v", "onekey", "ascending", "onerow")
SHOWS_ON = {"no_rescale": _MOVING, "any_skip": tuple(f for f in _MOVING if f != "ascending"), "stale_l": _MOVING,
            "early_stop": tuple(NAMES)}
SPLIT_SHOWS_ON = {"drop_qlo": ("gauss", "peaked", "tail_v", "onerow"),
                  "drop_plo": ("gauss", "peaked", "tail_v", "onekey", "onerow"),
                  "padkey": ("gauss", "flat", "tail_v", "onekey", "firstkey", "onerow"),
                  "strict": tuple(NAMES)}
_CACHE = {}
_TRACES = {}


def _case(family, hd, L, causal):
    key = (family, hd, L, causal)
    if key not in _CACHE:
        qkv = stream_families(hd)[family](B, L, H)
        _CACHE[key] = (qkv,) + bound(qkv, H, causal, hd=hd)
    return _CACHE[key]


def _traced(family, hd, wmax, tb, L, causal):
    """the correct emulation and its (query tile, key tile, alpha == 1) steps, once per case"""
    key = (family, hd, wmax, tb, L, causal)
    if key not in _TRACES:
        trace = []
        _TRACES[key] = (emulate_stream(_case(family, hd, L, causal)[0], H, causal, hd, wmax, tb, trace=trace), trace)
    return _TRACES[key]


def _ratio(got, ref, bnd):
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bnd).max())


def test_stream_families_are_deterministic_and_inside_the_fp16_range():
    assert list(families()) == NAMES[:6]
    for hd in (64, 72, 80, 128):
        fam = stream_families(hd)
        assert list(fam) == NAMES
        for name, make in fam.items():
            for L in (33, 577):
                a, b = make(2, L, 3), make(2, L, 3)
                assert a.shape == (2, L, 3 * 3 * hd) and a.dtype == torch.float32 and torch.equal(a, b), name
                assert not torch.equal(a, make(2, L, 3, seed=1)), name
                assert float(a.abs().max()) < 65504.0 / 8, name
    for name in NAMES[:6]:                                # (salts of their own: not the tensors the short tests cache)
        assert not torch.equal(stream_families(64)[name](2, 33, 3), families()[name](2, 33, 3)), name


def test_the_deal_of_query_tiles_covers_every_tile_once():
    for wmax in (4, 8):
        for TJ in range(1, 130):
            deal = stream_deal(TJ, wmax)
            assert len(deal) == (TJ + wmax - 1) // wmax and deal[0][0] == 0 and sum(n for _, n in deal) == TJ
            assert all(1 <= n <= wmax for _, n in deal) and all(a[0] + a[1] == b[0] for a, b in zip(deal, deal[1:]))


@pytest.mark.parametrize("L,causal", CASES)
@pytest.mark.parametrize("hd,wmax,tb", GEOMETRIES)
@pytest.mark.parametrize("family", NAMES)
def test_correct_arithmetic_stays_within_half_the_bound(family, hd, wmax, tb, L, causal):
    qkv, ref, bnd = _case(family, hd, L, causal)
    assert ref.shape == bnd.shape == (B, L, H * hd) and float(bnd.min()) >= 2.0 ** -24
    r32 = _ratio(evaluate_f32(qkv, H, causal, hd), ref, bnd)
    rst = _ratio(_traced(family, hd, wmax, tb, L, causal)[0], ref, bnd)
    rsp = _ratio(emulate_split(qkv, H, causal, hd=hd), ref, bnd) if hd == 64 else 0.0
    print(f"attention_stream {family} hd={hd} wmax={wmax} tb={tb} L={L} causal={causal} fault=None: fp32 {2 * r32:.3f}, "
          f"stream emulation {2 * rst:.3f}, split emulation {2 * rsp:.3f} (units of C = 1)")
    assert r32 <= 0.5 and rst <= 0.5 and rsp <= 0.5, (r32, rst, rsp)


@pytest.mark.parametrize("L,causal", CASES)
@pytest.mark.parametrize("hd,wmax,tb", GEOMETRIES)
def test_the_stress_families_have_the_property_they_are_named_for(hd, wmax, tb, L, causal):
    # ascending: in no key tile does the maximum stay for all rows of a query tile (the skip of the rescale is never taken)
    for gt, tj, one in _traced("ascending", hd, wmax, tb, L, causal)[1]:
        assert not bool(one.all(dim=-1).any()), (gt, tj)
    # firstkey: after the first key tile it stays for every row (the skip is taken in every later tile)
    steps = _traced("firstkey", hd, wmax, tb, L, causal)[1]
    assert any(tj > 0 for _, tj, _ in steps)
    for gt, tj, one in steps:
        assert bool(one.all()) == (tj > 0) and bool(one.any()) == (tj > 0), (gt, tj)
    # onerow: some (query tile, key tile) has rows whose maximum moved next to rows whose maximum stayed -- in the key tile of a
    # dominant key (index 37, tile 1) for every head, so that __any and __all differ there
    mixed = [(gt, tj) for gt, tj, one in _traced("onerow", hd, wmax, tb, L, causal)[1]
             if bool((one.any(dim=-1) & ~one.all(dim=-1)).all())]
    assert any(tj == 1 for _, tj in mixed), mixed
    # every query tile is visited once per key tile it may see
    TJ = (L + 31) // 32
    assert len(steps) == (TJ * (TJ + 1) // 2 if causal else TJ * TJ)


@pytest.mark.parametrize("L,causal", CASES)
@pytest.mark.parametrize("hd,wmax,tb", GEOMETRIES)
@pytest.mark.parametrize("fault", STREAM_FAULTS)
def test_every_planted_stream_fault_leaves_the_bound(fault, hd, wmax, tb, L, causal):
    if fault == "early_stop" and not causal:
        qkv, ref, bnd = _case("gauss", hd, L, causal)    # (without a causal mask every workgroup needs every key tile: same bits)
        assert torch.equal(emulate_stream(qkv, H, causal, hd, wmax, tb, fault), _traced("gauss", hd, wmax, tb, L, causal)[0])
        return
    assert SHOWS_ON[fault] and (fault != "any_skip" or "onerow" in SHOWS_ON[fault])
    for family in SHOWS_ON[fault]:
        qkv, ref, bnd = _case(family, hd, L, causal)
        r = _ratio(emulate_stream(qkv, H, causal, hd, wmax, tb, fault), ref, bnd)
        print(f"attention_stream {family} hd={hd} wmax={wmax} tb={tb} L={L} causal={causal} fault={fault}: {2 * r:.1f} (units of C = 1)")
        assert r > 1.0, (family, r)


@pytest.mark.parametrize("L,causal", [(321, True), (577, False), (577, True)])
@pytest.mark.parametrize("fault", FAULTS)
def test_the_split_faults_leave_the_bound_beyond_288_tokens(fault, L, causal):
    if fault == "strict" and not causal:
        qkv, ref, bnd = _case("gauss", 64, L, causal)
        assert torch.equal(emulate_split(qkv, H, causal, fault), emulate_split(qkv, H, causal))
        return
    for family in SPLIT_SHOWS_ON[fault]:
        qkv, ref, bnd = _case(family, 64, L, causal)
        r = _ratio(emulate_split(qkv, H, causal, fault), ref, bnd)
        print(f"attention_stream {family} hd=64 L={L} causal={causal} fault={fault}: {2 * r:.1f} (units of C = 1)")
        assert r > 1.0, (family, r)
