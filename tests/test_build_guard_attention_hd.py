"""CPU (hipcc cross-compiles gfx950 here): k_attention_hdx_stream (csrc/attention_hd.hip, head dims 72 .. 128) exists in its
eight instantiations -- two padded head dims x four output forms --, spills no register and keeps scratch out of the loops
that issue MFMAs.  No register ceiling: the occupancy these kernels reach is a measured outcome (DESIGN.md section 4,
"attention at head dims 72 .. 128").  The parser is that of tests/test_build_guard.py, imported as
tests/test_build_guard_attention_long.py does."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_build_guard as g   # noqa: E402

FRAG = "k_attention_hdx_streamILi"


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
def test_head_dim_kernels_are_eight_do_not_spill_and_keep_scratch_out_of_their_loops():
    meta = g._kernel_meta("attention_hd.hip")
    bodies = g._kernel_bodies(g._kernel_asm("attention_hd.hip"))
    hits = sorted(n for n in meta if FRAG in n)
    assert len(hits) == 8, sorted(meta)
    for hdp in (96, 128):
        for split in range(4):
            assert len([n for n in hits if f"{FRAG}{hdp}ELi{split}E" in n]) == 1, (hdp, split, hits)
    for n in hits:
        print(f"[attention_hd guard] {n}: {meta[n]}")
        assert meta[n]["vgpr_spill_count"] == 0, (n, meta[n])
        assert g._loops_with_mfma_and_scratch(bodies[n]) == [], n
        assert g._loops_with_mfma_and_scratch(bodies[n], _probe=True), "the parser must see the MFMA loops"


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
def test_attention_hip_keeps_its_kernels_and_lists_the_new_unit():
    from lemon_amd import build
    assert "attention_hd.hip" in build.SOURCES and "attention.hip" in build.SOURCES
    meta = g._kernel_meta("attention.hip")
    assert not [n for n in meta if "k_attention_hdx" in n], "the new kernel lives in its own translation unit"
    assert len([n for n in meta if "k_attention_hd64_streamILi" in n]) == 4, sorted(meta)
