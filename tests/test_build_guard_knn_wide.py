"""CPU (hipcc cross-compiles gfx950 here): the wide Q-stationary filter scan k_scan_f16_qsw (pitches 1024 / 1280, inner product
and squared L2) issues its LDS reads, LDS-DMA and MFMAs by hand and pins 256 AccVGPRs of stationary query fragments; like its
siblings it must hold everything in registers -- one wave per SIMD, no spill, no scratch -- and the compiler must keep its hands
off the registers of in-flight asm loads.  The same parser as tests/test_build_guard.py (its helpers are imported; that file
stays as it is and its fragments keep matching exactly the kernels they matched before)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_build_guard as g   # noqa: E402

# k_scan_f16_qsw<KT, l2>: KT = pitch / 64
WIDE = ["k_scan_f16_qswILi16ELb0E", "k_scan_f16_qswILi16ELb1E", "k_scan_f16_qswILi20ELb0E", "k_scan_f16_qswILi20ELb1E"]

# what tests/test_build_guard.py lists for knn_bf16.hip, with the number of kernels each fragment matched before k_scan_f16_qsw
# (the QS / QS2 fragments as they read since the PROF and ACCV template parameters were retired)
EXISTING = {"k_scan_bf16_qsILi12ELb0E": 1, "k_scan_bf16_qsILi8ELb0E": 1, "k_scan_bf16_qsILi4ELb0E": 1,
            "k_scan_bf16_qs2ILi12ELi16ELb0E": 1, "k_scan_bf16_qs2ILi12ELi20ELb1E": 1,
            "k_scan_bf16_qs2ILi8ELi0ELb0E": 1, "k_bf16_finalILb0ELb1E": 1, "k_bf16_finalILb1ELb1E": 1,
            "k_scan_f16_qs4ILi12ELi16ELb0E": 1, "k_scan_f16_qs4ILi8ELi0ELb0E": 1, "k_scan_f16_qs4ILi8ELi0ELb1E": 1}


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
def test_wide_scan_instantiations_exist_and_hold_everything_in_registers():
    meta = g._kernel_meta("knn_bf16.hip")
    assert len([n for n in meta if "k_scan_f16_qswILi" in n]) == len(WIDE), sorted(n for n in meta if "qsw" in n)
    for frag in WIDE:
        hits = [n for n in meta if frag in n]
        assert len(hits) == 1, (frag, hits)
        m = meta[hits[0]]
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (hits[0], m)


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
def test_wide_scan_asm_is_left_alone_by_the_compiler():
    bodies = g._kernel_bodies(g._kernel_asm("knn_bf16.hip"))
    for frag in WIDE:
        hits = [n for n in bodies if frag in n]
        assert len(hits) == 1, (frag, hits)
        problems = g._check_asm_discipline(hits[0], bodies[hits[0]])
        assert not problems, "\n".join(problems[:10])


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
def test_existing_guard_fragments_match_the_kernels_they_matched_before():
    meta = g._kernel_meta("knn_bf16.hip")
    for frag, count in EXISTING.items():
        assert len([n for n in meta if frag in n]) == count, (frag, [n for n in meta if frag in n])
