"""CPU: the error bound the GPU attention tests assert (tests/attention_ref.py: bound) can tell a correct kernel from a subtly
wrong one.  On every input family and shape below a plain fp32 evaluation and an emulation of the kernels' split-fp16 arithmetic
stay within half of it; the same emulation with one planted fault -- a dropped cross product, an unmasked padding key, an
off-by-one causal mask -- leaves it on every family the fault can show on.  No kernel has to be broken to know that."""
import pytest
import torch

from .attention_ref import FAULTS, bound, emulate_split, evaluate_f32, families

CASES = [(50, False), (77, True), (129, True), (197, False), (288, True), (31, True)]
B, H = 2, 2
SHOWS_ON = {"drop_qlo": ("gauss", "peaked", "tail_v"),
            "drop_plo": ("gauss", "peaked", "tail_v", "onekey"),
            "padkey": ("gauss", "flat", "tail_v", "onekey"),
            "strict": ("gauss", "peaked", "flat", "offset", "tail_v", "onekey")}
_CACHE = {}


def _case(family, L, causal):
    key = (family, L, causal)
    if key not in _CACHE:
        qkv = families()[family](B, L, H)
        _CACHE[key] = (qkv,) + bound(qkv, H, causal)
    return _CACHE[key]


def _ratio(got, ref, bnd):
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bnd).max())


def test_families_are_deterministic_and_inside_the_fp16_range():
    fam = families()
    assert list(fam) == ["gauss", "peaked", "flat", "offset", "tail_v", "onekey"]
    for name, make in fam.items():
        a, b = make(2, 33, 3), make(2, 33, 3)
        assert a.shape == (2, 33, 3 * 3 * 64) and a.dtype == torch.float32 and torch.equal(a, b), name
        assert not torch.equal(a, make(2, 33, 3, seed=1)), name
        assert float(a.abs().max()) < 65504.0 / 8, name


@pytest.mark.parametrize("L,causal", CASES)
@pytest.mark.parametrize("family", list(families()))
def test_correct_arithmetic_stays_within_half_the_bound(family, L, causal):
    qkv, ref, bnd = _case(family, L, causal)
    assert ref.shape == bnd.shape == (B, L, H * 64) and float(bnd.min()) >= 2.0 ** -24
    r32 = _ratio(evaluate_f32(qkv, H, causal), ref, bnd)
    rsp = _ratio(emulate_split(qkv, H, causal), ref, bnd)
    print(f"attention_bound {family} L={L} causal={causal}: fp32 {2 * r32:.3f}, split emulation {2 * rsp:.3f} (units of C = 1)")
    assert r32 <= 0.5 and rsp <= 0.5, (r32, rsp)


@pytest.mark.parametrize("L,causal", CASES)
@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_leaves_the_bound(fault, L, causal):
    if fault == "strict" and not causal:
        qkv, ref, bnd = _case("gauss", L, causal)       # (without a causal mask there is nothing to get wrong: same bits)
        assert torch.equal(emulate_split(qkv, H, causal, fault), emulate_split(qkv, H, causal))
        return
    for family in SHOWS_ON[fault]:
        qkv, ref, bnd = _case(family, L, causal)
        r = _ratio(emulate_split(qkv, H, causal, fault), ref, bnd)
        print(f"attention_bound {family} L={L} causal={causal} fault={fault}: {2 * r:.1f} (units of C = 1)")
        assert r > 1.0, (family, r)
