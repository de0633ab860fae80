"""CPU: the coefficient-domain JPEG writer of tests/jpegcoeffx.py and the host side of the JPEG decode pinned against each
other and against PIL on every list the GPU module (tests/test_gpu_jpeg_coef.py) runs: the host pass gives the writer's record
bit for bit, the reconstruction gives PIL's pixels, the parallel pass looped on the host gives the same record at five lane
sizes, and what is declined is declined alike by every path.  PLACEMENTS holds, per list, the assertions on what the files
are (lane counts, interval sizes, bit positions, plane borders): both modules call them, so a list that stopped aiming at its
kernel edge fails here first."""
import numpy as np
import pytest

from tests import jpegcoeffx as fx
from tests import jpegfx

LANE_SIZES = (16, 20, 36, 0, 4096)
SMALL_LANES = (16, 20, 36)
DECLINING = ("envelope", "dc_range")          # the lists that hold files outside the arithmetic envelope, by construction


def lanes_of(nbytes, subseq=16):
    return max(1, -(-nbytes // subseq))


# ---------------------------------------------------------------------------------------------------------------- placements
def place_intervals(cases):
    n = {c.name: len(c.jpeg.interval_bytes) for c in cases}
    assert [n[f"gray_{k}x1_r1"] for k in (255, 256, 257, 513)] == [255, 256, 257, 513]
    assert n["420_257x1_r1"] == 257 and n["420_150x2_r7"] == 43 and n["422_130x3_r3"] == 130
    by = {c.name: c.jpeg for c in cases}
    assert by["420_150x2_r7"].record.size == 384 + 128 * 300 * 6 and 7 * 6 * 6 % 256 != 0       # heads inside the 256-block chunks
    assert by["420_257x1_r1"].record.size == 384 + 128 * 257 * 6
    return {"cases": len(cases), "intervals": sorted(n.values())}


def place_lanes(cases):
    got = []
    for c in cases:
        assert c.jpeg.scan_bytes == c.note[0] and len(c.jpeg.interval_bytes) == 1, c.name
        assert lanes_of(c.jpeg.scan_bytes) == c.note[1], c.name
        got.append((c.jpeg.scan_bytes, lanes_of(c.jpeg.scan_bytes)))
    assert {n for _, n in got} == {255, 256, 257, 512, 513}
    assert {b for b, n in got if n == 256} >= {16 * 256 - 15, 16 * 256} and (16 * 256 + 1, 257) in got
    return {"cases": len(cases), "scan_bytes_and_lanes": got}


def place_interval_sizes(cases):
    out = {"cases": len(cases)}
    for c in cases:
        assert c.jpeg.interval_bytes == c.note and set(c.note) == set(fx.INTERVAL_SIZES), c.name
        first = np.concatenate([[0], np.cumsum([lanes_of(b) for b in c.jpeg.interval_bytes])])       # first lane of every interval
        assert first[-1] > 256
        between = 256 in first
        assert between == (c.name == "between"), (c.name, first[:60])
        out[c.name] = {"intervals": len(c.note), "lanes": int(first[-1]), "lane_256_starts_an_interval": bool(between)}
    return out


def place_big(cases):
    from lemon_amd import jpeg_host
    out = {"cases": len(cases)}
    for c in cases:
        assert tuple(c.jpeg.interval_bytes) == c.note and c.one_byte, c.name
        pk, head = jpeg_host.pack(c.jpeg.raw)
        assert pk is not None and pk.intervals == 3 and pk.scan_bytes == sum(c.note)
        nbig = int(pk.data[:64].view(np.int32)[12])                                     # (csrc/jpeg_par.hpp: kPkBig)
        assert nbig == sum(b >= 65535 for b in c.note), (c.name, nbig)
        len16 = pk.data[2688:2688 + 6].view(np.uint16)
        assert [int(v) for v in len16] == [min(b, 0xFFFF) for b in c.note]
        out[c.name] = {"interval_bytes": list(c.note), "nbig": nbig}
    assert [out[c.name]["nbig"] for c in cases] == [1, 2, 2]
    return out


def place_symbols(cases):
    placed = {}
    for c in cases:
        j = c.jpeg
        if c.note and c.note[0] in ("dc", "ac"):
            kind, blk, bit = c.note
            k = int(j.block_symbol[0][blk]) + (kind == "ac")
            start, size = int(j.symbol_start[0][k]), int(j.symbol_start[0][k + 1] - j.symbol_start[0][k])
            assert start % 128 == bit and size == (27 if kind == "dc" else 26), (c.name, start, size)
            assert int(j.block_start[0][blk]) == start - (8 if kind == "ac" else 0)
            placed[c.name] = (start, size)
        elif c.note:
            ends = [c.jpeg.raw.count(b"\xff\x00" + b"\xff" * (int(c.name[-1]) + 1) + bytes([m])) for m in (0xD0, 0xD1, 0xD2, 0xD9)]
            assert ends == [1, 1, 1, 1], (c.name, ends)                                 # every interval ends in a stuffed FF
    assert len(placed) == 6
    return {"cases": len(cases), "long_symbol_start_bit_and_size": placed}


def place_selectors(cases):
    straddle, totals, sels = 0, set(), set()
    for c in cases:
        j = c.jpeg
        n0 = (-(-j.w // (8 * j.hs)) * j.hs) * (-(-j.h // (8 * j.vs)) * j.vs)
        nc = (j.record.size - 384) // 128 - n0 if j.components == 3 else 0
        totals.add((j.record.size - 384) // 128)
        if j.components == 3 and n0 % 32 and (n0 + nc // 2) % 32 and n0 // 32 == (n0 + nc // 2) // 32:
            straddle += 1                                                               # one workgroup holds Y, Cb and Cr blocks
        q = j.record[:384].view(np.uint16).reshape(3, 64)
        if j.components == 3:
            assert not np.array_equal(q[0], q[1]) and not np.array_equal(q[1], q[2]) and not np.array_equal(q[0], q[2]), c.name
        sels.add(c.name.split("_d")[1][:3])
    assert totals >= {31, 32, 33, 36} and straddle >= 3 and sels == {"101", "023", "330"}
    return {"cases": len(cases), "block_totals": sorted(totals), "one_workgroup_all_components": straddle}


def place_padding(cases):
    by = {c.name: c for c in cases}
    pairs = [n for n in by if n + "_twin" in by]
    for n in pairs:
        a, b = by[n].jpeg, by[n + "_twin"].jpeg
        diff = np.flatnonzero((a.record[384:].view(np.int16).reshape(-1, 64) != b.record[384:].view(np.int16).reshape(-1, 64)).any(1))
        cols = -(-a.w // (8 * a.hs)) * a.hs
        assert len(diff) and all(8 * (d // cols) >= a.h or 8 * (d % cols) >= a.w for d in diff), n      # luma blocks outside only
    assert len(cases) - len(pairs) == 4 * len(fx.PAD_SIDES) ** 2 and len(pairs) >= 100
    return {"cases": len(cases), "pairs": len(pairs)}


def place_envelope(cases):
    from lemon_amd import jpeg_host
    assert len(cases) == fx.N_ENVELOPE_RANDOM + 128
    exact = declined = 0
    for c in cases[:fx.N_ENVELOPE_RANDOM]:
        info = jpeg_host.decode_record(c.jpeg.raw)[1]
        assert info.status in (0, 12), (c.name, info.status)
        exact += info.status == 0 and info.exact_blocks > 0
        declined += info.status == 12
    assert exact >= 50 and declined >= 50, (exact, declined)
    seen, levels = set(), set()
    for c in cases[fx.N_ENVELOPE_RANDOM:]:
        pos, v = c.note
        info = jpeg_host.decode_record(c.jpeg.raw)[1]
        assert info.status == 0 and info.exact_blocks == 1, c.name                      # accepted, by the exact form
        more = fx._single(pos, v + (1 if v > 0 else -1))
        assert jpeg_host.decode_record(more.raw)[1].status == 12, c.name                # and one step further is declined
        px = fx.pil_rgb(c.jpeg.raw)
        levels |= {int(px.min()), int(px.max())}
        seen.add((pos, v > 0))
    assert len(seen) == 128 and {0, 255} <= levels                                      # both ends of the clamp are reached
    return {"cases": len(cases), "random_accepted_exact": int(exact), "random_declined": int(declined), "single": 128}


def place_dc_range(cases):
    assert len(cases) == 2
    return {"cases": len(cases)}


PLACEMENTS = {"intervals": place_intervals, "lanes": place_lanes, "interval_sizes": place_interval_sizes, "big": place_big,
              "symbols": place_symbols, "selectors": place_selectors, "padding": place_padding, "envelope": place_envelope,
              "dc_range": place_dc_range}


# --------------------------------------------------------------------------------------------------------------------- tests
def test_the_annex_k_tables_in_the_writer_are_the_ones_pil_writes():
    raw = jpegfx.jpeg_bytes(jpegfx.pixels(16, 16, np.random.default_rng(0)), quality=90)
    p, found = 2, {}
    while raw[p + 1] != 0xDA:
        n = (raw[p + 2] << 8) | raw[p + 3]
        if raw[p + 1] == 0xC4:
            s, o = raw[p + 4:p + 2 + n], 0
            while o < len(s):
                k = sum(s[o + 1:o + 17])
                found[s[o]] = (s[o + 1:o + 17], s[o + 17:o + 17 + k])
                o += 17 + k
        p += 2 + n
    for key, t in ((0x00, fx.K_DC_LUMA), (0x01, fx.K_DC_CHROMA), (0x10, fx.K_AC_LUMA), (0x11, fx.K_AC_CHROMA)):
        assert found[key] == (t.counts, t.vals), hex(key)


def test_the_table_builder_refuses_counts_that_are_no_prefix_code_or_use_the_all_ones_code():
    fx.huff_table(fx.counts_of({8: 255}), range(255))
    fx.huff_table(fx.counts_of({1: 1, 16: 255}), range(256))
    for counts, n in ((fx.counts_of({8: 256}), 256), (fx.counts_of({1: 2}), 2), (fx.counts_of({1: 1, 2: 1, 3: 3}), 5)):
        with pytest.raises(AssertionError):
            fx.huff_table(counts, range(n))
    for t in (fx.L_DC, fx.L_AC):
        assert sorted(length for _, length in t.codes.values())[-1] == 16
    assert fx.L_DC.codes[11][1] == 16 and fx.L_AC.codes[0x0A][1] == 16 and fx.L_AC.codes[0xEA][1] == 16


def test_every_list_is_there_and_seeded():
    assert set(fx.LISTS) == set(PLACEMENTS)
    a, b = fx.symbols_cases(), fx.symbols_cases.__wrapped__()
    assert [c.jpeg.raw for c in a] == [c.jpeg.raw for c in b]


@pytest.mark.parametrize("name", list(fx.LISTS))
def test_placements(name):
    print(name, PLACEMENTS[name](fx.LISTS[name]()))


def host_reference(c):
    """(record or None, status) of the sequential host pass, after checking it against the writer and PIL."""
    from lemon_amd import jpeg_host
    rec, info = jpeg_host.decode_record(c.jpeg.raw)
    if rec is None:
        return None, info.status
    assert (rec.w, rec.h, rec.components, rec.hs, rec.vs) == (c.jpeg.w, c.jpeg.h, c.jpeg.components, c.jpeg.hs, c.jpeg.vs), c.name
    assert np.array_equal(rec.data, c.jpeg.record), (c.name, int((rec.data != c.jpeg.record).sum()))
    return rec, 0


@pytest.mark.parametrize("name", list(fx.LISTS))
def test_host_pass_gives_the_writers_record_and_the_reconstruction_gives_pils_pixels(name):
    from lemon_amd import jpeg_host
    declined = 0
    for c in fx.LISTS[name]():
        rec, st = host_reference(c)
        if rec is None:
            assert name in DECLINING and st == 12, (c.name, st)
            declined += 1
            continue
        got, ref = jpeg_host.reconstruct(rec), fx.pil_rgb(c.jpeg.raw)
        assert np.array_equal(got, ref), (c.name, int((got != ref).sum()), int(np.abs(got.astype(int) - ref).max()))
    assert (declined > 0) == (name in DECLINING)


def test_files_that_differ_only_outside_the_image_decode_to_the_same_pixels():
    by = {c.name: c for c in fx.padding_cases()}
    for n in by:
        if n + "_twin" in by:
            assert np.array_equal(fx.pil_rgb(by[n].jpeg.raw), fx.pil_rgb(by[n + "_twin"].jpeg.raw)), n


@pytest.mark.parametrize("name", list(fx.LISTS))
def test_parallel_pass_on_the_host_gives_the_writers_record_at_every_lane_size(name):
    from lemon_amd import jpeg_host
    cases = fx.LISTS[name]()
    sync = set()
    for c in cases:
        want = jpeg_host.decode_record(c.jpeg.raw)[1].status
        pk, head = jpeg_host.pack(c.jpeg.raw)
        assert pk is not None and head.status == 0, (c.name, head.status)            # the packer reads no coefficient: it accepts
        assert (pk.scan_bytes, pk.intervals) == (c.jpeg.scan_bytes, len(c.jpeg.interval_bytes)), c.name
        for subseq in LANE_SIZES:
            rec = np.full(head.record_bytes, 0xA5, np.uint8)
            st = jpeg_host.entropy_par_host(pk.data, rec, subseq)
            if st == 16 and want == 0:
                assert subseq in SMALL_LANES, (c.name, subseq)
                sync.add(c.name)
                continue
            assert st == want, (c.name, subseq, st, want)                            # a declined file: the host pass's status
            if st == 0:
                assert np.array_equal(rec, c.jpeg.record), (c.name, subseq, int((rec != c.jpeg.record).sum()))
    assert sync == {c.name for c in cases if c.one_byte}, sync
