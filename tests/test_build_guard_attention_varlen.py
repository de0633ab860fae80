"""CPU (hipcc cross-compiles gfx950 here): the per-sequence-length attention kernels (csrc/attention_varlen.hip) are the VL = true
instantiations of the three bodies in csrc/attention_hd64.hpp, whose VL = false instantiations are kernels of csrc/attention.hip,
in a translation unit of their own.  Checked on the generated code object:
  * the new unit holds its 24 instantiations (short form: TJ 1, 2 x four output forms x both arithmetics; the fp32 general and
    the staged split-fp16 form x four output forms), under names the guards of the existing units do not count;
  * attention.hip and attention_hd.hip hold what they held;
  * the short and the fp32 general form spill nothing; the staged form keeps scratch out of every loop that issues MFMAs (its
    sibling is allowed the same few staging addresses around the loops);
  * registers: only what the launch bounds need -- 64 * TJ threads with three workgroups per CU for the short form (168), nine
    waves per workgroup for the general forms (168), four waves per SIMD for the staged form (128)."""
import os

import pytest

from .test_build_guard import HIPCC, _kernel_asm, _kernel_bodies, _kernel_meta, _loops_with_mfma_and_scratch

SRC = "attention_varlen.hip"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# fragments the guards of attention.hip / attention_hd.hip count
FOREIGN = ("k_attention_hd64_f16ILi", "k_attention_hd64_streamILi", "k_attention_hd64_shortILi", "k_attention_hd64ILi")


def test_new_unit_holds_its_instantiations_under_names_of_its_own():
    meta = _kernel_meta(SRC)
    short = [n for n in meta if "k_attnvl_shortILi" in n]
    f32 = [n for n in meta if "k_attnvl_f32ILi" in n]
    f16 = [n for n in meta if "k_attnvl_f16ILi" in n]
    assert len(short) == 16 and len(f32) == 4 and len(f16) == 4, sorted(meta)
    assert len(meta) == 24, sorted(meta)
    for tj in (1, 2):
        for split in range(4):
            for arith in (0, 1):
                assert any(f"k_attnvl_shortILi{tj}ELi{split}ELb{arith}E" in n for n in short), (tj, split, arith)
    for split in range(4):
        assert any(f"k_attnvl_f32ILi{split}E" in n for n in f32) and any(f"k_attnvl_f16ILi{split}E" in n for n in f16), split
    for n in meta:
        assert not any(f in n for f in FOREIGN), n


def test_existing_units_hold_what_they_held():
    meta = _kernel_meta("attention.hip")
    assert len([n for n in meta if "k_attention_hd64_f16ILi" in n]) == 4
    assert len([n for n in meta if "k_attention_hd64_shortILi" in n]) == 16
    assert len([n for n in meta if "k_attention_hd64ILi" in n]) == 8
    assert len([n for n in meta if "k_attention_hd64_streamILi" in n]) == 4
    assert not any("k_attnvl" in n for n in meta)
    hd = _kernel_meta("attention_hd.hip")
    assert len([n for n in hd if "k_attention_hdx_streamILi" in n]) == 8 and not any("k_attnvl" in n for n in hd)


def test_short_and_general_forms_do_not_spill():
    meta = _kernel_meta(SRC)
    for n, m in meta.items():
        if "k_attnvl_short" in n or "k_attnvl_f32" in n:
            assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (n, m)
            assert m["vgpr_count"] <= 168, (n, m)            # 512 registers per lane / three waves of a SIMD


def test_staged_form_fits_four_waves_and_keeps_scratch_out_of_its_mfma_loops():
    meta = _kernel_meta(SRC)
    bodies = _kernel_bodies(_kernel_asm(SRC))
    hits = [n for n in meta if "k_attnvl_f16ILi" in n]
    assert len(hits) == 4
    for n in hits:
        print(n, meta[n])
        assert meta[n]["vgpr_count"] <= 128, (n, meta[n])    # __launch_bounds__(576, 4)
        assert _loops_with_mfma_and_scratch(bodies[n]) == [], n
        assert _loops_with_mfma_and_scratch(bodies[n], _probe=True), "the parser must see the MFMA loops"
