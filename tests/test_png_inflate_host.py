"""CPU: the inflate of the PNG path (csrc/png_inflate_core.hpp) through its host twin lemon_png_inflate_host -- the device's
schedule with the lanes looped -- against zlib.decompressobj() under the rule of png_host.fill_record: (a) streams zlib writes
over its settings, none of which may be declined; (b) streams written token by token (tests/deflatefx.py) at every edge of the
decoder; (c) everything that has to be declined; (d) pack_stream + inflate_host + decode_host against PIL's pixels."""
import ctypes

import numpy as np
import pytest

from tests import deflatefx as fx
from tests import inflatefx, pngfx

POISON = 0xA5
STREAM = 12


@pytest.fixture(scope="module")
def png_host():
    from lemon_amd import png_host as m
    m.load()
    return m


def inflate(png_host, z, want, in_skew=0, out_skew=0):
    """The host twin with the input at address in_skew mod 16 and the rows at address out_skew mod 16 inside a poisoned
    buffer (the 16-byte pieces of both sides are cut by address).  -> (status, rows); asserts that nothing outside the rows
    changed and the input is untouched."""
    src = np.empty(len(z) + 32, np.uint8)
    a = (16 - (src.ctypes.data % 16) + in_skew) % 16
    src[a:a + len(z)] = np.frombuffer(z, np.uint8)
    before = src[a:a + len(z)].copy()
    out = np.full(want + 64, POISON, np.uint8)
    o = 16 + (16 - (out.ctypes.data % 16) + out_skew) % 16
    st = ctypes.c_int32(-1)
    rc = png_host.load().lemon_png_inflate_host(src.ctypes.data + a, len(z), out.ctypes.data + o, want, ctypes.byref(st))
    assert rc == 0 and st.value in (0, STREAM)
    assert (out[:o] == POISON).all() and (out[o + want:] == POISON).all() and np.array_equal(src[a:a + len(z)], before)
    return st.value, out[o:o + want].tobytes()


def test_no_stream_zlib_writes_is_declined_and_every_byte_is_zlibs(png_host):
    cases = inflatefx.zlib_cases()
    assert len(cases) == 2880 and {c[2] for c in cases} == set(inflatefx.WANTS)
    for k, (name, z, want) in enumerate(cases):
        ok, rows = fx.zlib_verdict(z, want)
        assert ok, name                                   # zlib accepts all of its own streams
        st, got = inflate(png_host, z, want, k % 16, (5 * k) % 16)
        assert st == 0, name
        assert got == rows, name


def test_hand_written_streams_at_every_edge_equal_zlib(png_host):
    cases = inflatefx.edge_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) >= 45
    for k, (name, z, want) in enumerate(cases):
        ok, rows = fx.zlib_verdict(z, want)
        assert ok, f"{name}: the fixture is not a valid stream"
        skews = [(i, (3 * i + 1) % 16) for i in range(16)] if name in ("straddle_pieces", "piece_crossing", "wrap_minus_1") else [(k % 16, (7 * k) % 16)]
        for a, b in skews:
            st, got = inflate(png_host, z, want, a, b)
            assert st == 0, (name, a, b)
            assert got == rows, (name, a, b)


def test_the_dynamic_fixtures_reach_the_table_edges_they_name():
    cases = dict((c[0], c) for c in inflatefx.edge_cases())
    # HCLEN is the 4 bits behind BFINAL, BTYPE, HLIT, HDIST of the first dynamic block: bits 17 .. 20 of the deflate data
    def hclen(name, skip_stored=0):
        raw = cases[name][1][2 + skip_stored:]
        v = int.from_bytes(raw[:4], "little")
        assert (v >> 1) & 3 == 2, name
        return 4 + ((v >> 13) & 15)
    assert hclen("lit_code_15_bits") == 19 and hclen("hclen_5_rle0") == 5 and hclen("hclen_5_rle1") == 5
    # the run-coded sequences of the repeat fixtures cross the literal / distance boundary with the symbol they name
    lit = [1, 2] + [0] * 252 + [4, 4, 4, 4]
    for sym, lens, hlit in ((16, lit + [4] * 16, 258),
                            (17, fx.flat_lengths([1, 2, 256, 257], 288)[:261] + [0, 0, 0, 0, 1, 1], 261),
                            (18, fx.flat_lengths([1, 2, 256, 257], 288)[:286] + [0] * 20 + [1, 1], 286)):
        at, crossing = 0, None
        for s, extra in fx.rle_cl_sequence(lens):
            n = 1 if s < 16 else extra + (3 if s < 18 else 11)
            if at < hlit < at + n:
                crossing = s
            at += n
        assert at == len(lens) and crossing == sym, (sym, crossing)


def test_every_decline_is_declined_and_zlib_rejects_it_too(png_host):
    cases = inflatefx.decline_cases()
    seen = set()
    for name, z, want, strict in cases:
        ok, rows = fx.zlib_verdict(z, want)
        st, got = inflate(png_host, z, want, len(name) % 16, (3 * len(name)) % 16)
        if strict is None:                                # the control of the dynamic-header declines: a valid stream
            assert ok and st == 0 and got == rows, name
        elif strict:
            assert not ok, f"{name}: zlib accepts the fixture"
            assert st == STREAM, name
            seen.add(name)
        else:                                             # zlib's non-strict rules accept it: either verdict, equal bytes
            assert ok, name
            assert st == STREAM or got == rows, name
    for must in ("block_type_3", "stored_nlen_mismatch", "hlit_287", "hdist_31", "repeat_nothing_to_repeat", "repeat18_past_the_end",
                 "lit_oversubscribed", "dist_oversubscribed", "cl_oversubscribed", "lit_incomplete", "dist_incomplete_two_codes",
                 "cl_incomplete", "missing_end_of_block_code", "literal_length_symbol_286", "literal_length_symbol_287",
                 "distance_symbol_30", "distance_symbol_31", "distance_beyond_output", "want_one_less", "want_one_more",
                 "trailing_byte", "truncated_1", "adler_bit_0", "fdict", "cm_7", "bad_fcheck", "hclen_4_names_no_code"):
        assert must in seen, must


def test_a_flipped_bit_anywhere_is_never_accepted_with_other_bytes(png_host):
    """Single-bit flips over whole small streams: whatever the decoder accepts, zlib accepts with the same bytes."""
    picked = [c for c in inflatefx.edge_cases() if c[0] in ("lengths_dynamic", "single_dist_code_4", "stored_at_bit_3", "repeat17_crosses")]
    picked += [c for c in inflatefx.zlib_cases() if c[2] == 259 and "_l6_default_w15_m9" in c[0]]
    assert len(picked) >= 6
    accepted = 0
    for name, z, want in picked:
        for bit in range(0, 8 * len(z), 3 if len(z) > 300 else 1):
            bad = bytearray(z)
            bad[bit >> 3] ^= 1 << (bit & 7)
            st, got = inflate(png_host, bytes(bad), want)
            if st == 0:
                ok, rows = fx.zlib_verdict(bytes(bad), want)
                assert ok and got == rows, (name, bit)
                accepted += 1
    assert accepted < 200                                 # (a flip in a stored block's skipped bits and the like)


def test_invalid_arguments_are_refused(png_host):
    lib = png_host.load()
    st = ctypes.c_int32(-1)
    buf = np.zeros(16, np.uint8)
    assert lib.lemon_png_inflate_host(None, 0, buf.ctypes.data, 1, ctypes.byref(st)) == 1
    assert lib.lemon_png_inflate_host(buf.ctypes.data, -1, buf.ctypes.data, 1, ctypes.byref(st)) == 1
    assert lib.lemon_png_inflate_host(buf.ctypes.data, 4, None, 1, ctypes.byref(st)) == 1
    assert lib.lemon_png_inflate_host(buf.ctypes.data, 4, buf.ctypes.data, -1, ctypes.byref(st)) == 1
    assert st.value == -1


def test_pack_stream_inflate_host_and_decode_host_equal_pil(png_host):
    cases = pngfx.accepted_cases()
    assert {"idat_1byte", "idat_split_header", "idat_empty_chunks", "stored"} <= {c[0] for c in cases}
    for name, raw in cases:
        s, head = png_host.pack_stream(raw)
        assert s is not None and head.status == 0, name
        assert s.data.size == 1024 + head.idat_bytes == 1024 + s.z_bytes and (s.w, s.h) == (head.width, head.height), name
        rec, st = png_host.inflate_host(s)
        assert st == 0, name
        ref, _ = png_host.decode_record(raw)
        assert np.array_equal(rec.data, ref.data), name                       # the record zlib fills, palette included
        px, dst = png_host.decode_host(rec)
        assert dst == 0 and np.array_equal(px, pngfx.pil_rgb(raw)), name
    # the chunk walk's declines are pack_stream's; the stream's defects are the inflate's
    for name, raw, status in pngfx.declined_cases():
        s, head = png_host.pack_stream(raw)
        if status == STREAM:
            assert s is not None and png_host.inflate_host(s) == (None, STREAM), name
        else:
            assert s is None and head.status == status, name
    out = np.empty(8, np.uint8)
    s, head = png_host.pack_stream(cases[0][1], out)
    assert s is None and head.status == png_host.BUFFER


def test_workers_hand_over_streams_without_inflating_and_the_knob_has_three_values(png_host, tmp_path, monkeypatch):
    from lemon_amd import loader
    from lemon_amd.loader import DecodePool
    good = pngfx.accepted_cases()[::7]
    walk_declines = [c for c in pngfx.declined_cases() if c[0] in ("depth16", "depth4", "actl", "plte_missing")]
    stream_defects = [c for c in pngfx.declined_cases() if c[0] in ("stream_long", "stream_garbage")]
    cases = good + walk_declines + stream_defects
    paths = pngfx.write_all(str(tmp_path), cases)
    kinds = []
    with DecodePool(paths, workers=2, ring_bytes=4 << 20, png=True, png_streams=True) as pool:
        assert pool.torch_in_worker == [False, False]
        for i, item in pool.images():
            assert pool.held <= pool.ring_bytes
            if isinstance(item, png_host.PngStream):
                kinds.append("stream")
                ref, _ = png_host.pack_stream(cases[i][1])
                assert np.array_equal(item.data, ref.data) and tuple(item[1:]) == tuple(ref[1:]), cases[i][0]
                assert item.data.ctypes.data % 16 == 0
            else:
                kinds.append("pixels")
                assert np.array_equal(item, pngfx.pil_rgb(cases[i][1])), cases[i][0]
    # what the chunk walk declines goes to PIL in the worker; a defect of the zlib stream is the device's to find
    assert kinds == ["stream"] * len(good) + ["pixels"] * len(walk_declines) + ["stream"] * len(stream_defects)
    with DecodePool(paths[:4], workers=1, ring_bytes=1 << 20, png=False, png_streams=True) as pool:      # needs png
        assert all(isinstance(a, np.ndarray) for _, a in pool.images())
    for value, png, inflate in (("", False, False), ("pil", False, False), ("gpu", True, False), ("device", True, True), ("DEVICE ", True, True)):
        monkeypatch.setenv("LEMON_PNG", value)
        assert loader.png_default() is png and loader.png_inflate_default() is inflate, value
    monkeypatch.delenv("LEMON_PNG")
    assert loader.png_default() is False and loader.png_inflate_default() is False
    monkeypatch.setenv("LEMON_PNG", "host")
    with pytest.raises(ValueError, match="LEMON_PNG"):
        loader.png_inflate_default()
