"""CPU (hipcc cross-compiles gfx950 here): the streaming attention kernels (seq_len > 288) are built for two workgroups of up
to eight waves per CU -- four waves per SIMD, i.e. at most 128 registers ("streaming attention") -- and
must keep scratch out of the loops that issue MFMAs.  The same parser as tests/test_build_guard.py (its helpers are imported,
that file itself stays as it is and keeps counting four k_attention_hd64_f16 instantiations)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_build_guard as g   # noqa: E402

STREAM_F32 = "k_attention_hd64_streamILi"
STREAM_F16 = "k_attention_hd64_stream_f16ILi"
WAVES_PER_SIMD = 4             # two workgroups of <= 8 waves on the four SIMDs of a CU
MAX_VGPRS = 512 // WAVES_PER_SIMD


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("frag", [STREAM_F32, STREAM_F16])
def test_streaming_attention_kernels_fit_four_waves_and_keep_scratch_out_of_their_loops(frag):
    meta = g._kernel_meta("attention.hip")
    bodies = g._kernel_bodies(g._kernel_asm("attention.hip"))
    hits = [n for n in meta if frag in n]
    assert len(hits) == 4, sorted(meta)          # the four output forms (SPLIT 0..3)
    for n in hits:
        assert meta[n]["vgpr_count"] <= MAX_VGPRS, (n, meta[n])
        assert meta[n]["vgpr_spill_count"] <= 20, (n, meta[n])
        assert g._loops_with_mfma_and_scratch(bodies[n]) == [], n
        assert g._loops_with_mfma_and_scratch(bodies[n], _probe=True), "the parser must see the MFMA loops"


@pytest.mark.skipif(not os.path.exists(g.HIPCC), reason="hipcc not available")
def test_streaming_kernels_did_not_add_an_instantiation_of_the_shipped_kernel():
    meta = g._kernel_meta("attention.hip")
    assert len([n for n in meta if "k_attention_hd64_f16ILi" in n]) == 4, sorted(meta)
    # the two streaming families do not match each other's fragment
    assert not [n for n in meta if STREAM_F32 in n and "stream_f16" in n]
