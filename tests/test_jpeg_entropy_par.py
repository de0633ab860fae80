"""CPU: the scan packer (lemon_jpeg_pack) and the parallel Huffman decode of lemon_amd/csrc/jpeg_par.hpp with its lanes looped on
the host (lemon_jpeg_entropy_par_host: the functions, workgroups and rounds the kernels of csrc/jpeg_entropy.hip run) against the
sequential host pass: equal records on every accepted file, verdicts on corrupt scans, the declined files, a sanitizer fuzz, and
the decode pool delivering packets."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpegfx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANT_BASES = ("640x480", "optimize_q100", "restart_rows")
N_MUTANTS = 2001


@pytest.fixture(scope="module")
def accepted():
    return jpegfx.accepted_cases()


def scan_range(raw):
    """[first byte of the entropy-coded segment, offset of the EOI marker) of a file PIL wrote."""
    at = raw.index(b"\xff\xda")
    return at + 2 + ((raw[at + 2] << 8) | raw[at + 3]), len(raw) - 2


def mutants(n=N_MUTANTS, seed=20261017):
    """[(name, bytes)]: seeded corruptions inside the scans of the three base files: bit flips, byte deletions, truncations and
    inserted markers, one to three per mutant."""
    cases = dict(jpegfx.accepted_cases())
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        base = MUTANT_BASES[k % len(MUTANT_BASES)]
        m = bytearray(cases[base])
        what = []
        for _ in range(int(rng.integers(1, 4))):
            lo, hi = scan_range(cases[base])
            hi = min(hi, len(m))
            at = int(rng.integers(lo, max(lo + 1, hi)))
            kind = int(rng.integers(0, 4))
            if kind == 0:
                m[at] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:
                del m[at]
            elif kind == 2:
                del m[at:]
                if rng.integers(0, 2):
                    m += b"\xff\xd9"
            else:
                marker = int(rng.choice([0xD0 + int(rng.integers(0, 8)), 0xD9, 0xFF, 0x00, 0xC4, 0xDA]))
                m[at:at] = bytes([0xFF, marker])
            what.append("fdtm"[kind])
        out.append((f"{base}_{k}_{''.join(what)}", bytes(m)))
    return out


def slow_sync_jpeg(event_at, w=1024, h=960):
    """A valid gray baseline file built so that a decoder started in the wrong state stays wrong for kilobytes.  Both Huffman
    tables hold four 8-bit codes (DC: all category 0; AC: two EOB, two ZRL), so every symbol is one byte and any byte is a code
    of either table.  The scan is: one block `D ZRL EOB` (3 bytes), then blocks `D EOB` at odd offsets -- a decoder that starts
    at an even offset expecting a DC symbol reads every EOB as a DC code and every DC code as EOB, for ever, completing as many
    blocks as the true decoder --; at byte `event_at` + 1 (odd) one block whose DC code is 2: the wrong decoder reads it as ZRL,
    so both are at a block start two bytes later, the wrong one a block short; then `D ZRL EOB` again, after which blocks start
    at even offsets and every guess is right.  All coefficients are zero."""
    nblk = (w // 8) * (h // 8)
    scan, n = bytearray([0, 2, 0]), 1
    while n < nblk:
        if len(scan) == event_at + 1:
            scan += bytes([2, 0, 0, 2, 0])
            n += 2
        else:
            scan += bytes([0, 0])
            n += 1
    assert n == nblk and event_at % 2 == 0 and event_at + 8 < len(scan)
    seg = lambda m, body: bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body
    counts = bytes([0] * 7 + [4] + [0] * 8)
    return (b"\xff\xd8" + seg(0xDB, bytes([0]) + bytes([1] * 64)) + seg(0xC0, bytes([8]) + struct.pack(">HH", h, w) + bytes([1, 1, 0x11, 0]))
            + seg(0xC4, bytes([0x00]) + counts + bytes([0, 0, 0, 0])) + seg(0xC4, bytes([0x10]) + counts + bytes([0, 0, 0xF0, 0xF0]))
            + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + bytes(scan) + b"\xff\xd9")


def par_decode(raw, subseq):
    """(status of pack or of the parallel decode, record or None)."""
    from lemon_amd import jpeg_host
    pk, head = jpeg_host.pack(raw)
    if pk is None:
        return head.status, None
    rec = np.full(head.record_bytes, 0xA5, np.uint8)
    return jpeg_host.entropy_par_host(pk.data, rec, subseq), rec


def test_parallel_decode_equals_the_host_pass_on_every_accepted_file(accepted):
    from lemon_amd import jpeg_host
    assert len(accepted) >= 82
    small = large = 0
    for name, raw in accepted:
        ref, info = jpeg_host.decode_record(raw)
        pk, head = jpeg_host.pack(raw)
        assert pk is not None and head.status == 0, (name, head.status)
        assert pk.data.nbytes % 16 == 0 and pk.data.nbytes <= len(raw) + jpeg_host.PACKET_BOUND, name
        assert (head.width, head.height, head.record_bytes) == (info.width, info.height, info.record_bytes), name
        small += pk.scan_bytes <= 128
        large += pk.scan_bytes > 1024
        for subseq in (jpeg_host.SUBSEQ_MIN, 0):
            rec = np.full(head.record_bytes, 0xA5, np.uint8)
            st = jpeg_host.entropy_par_host(pk.data, rec, subseq)
            assert st == 0, (name, subseq, st, jpeg_host.STATUS.get(st))       # never declined, never LEMON_JPEG_SYNC
            assert np.array_equal(rec, ref.data), (name, subseq, int((rec != ref.data).sum()))
    assert small >= 20 and large >= 30, (small, large)       # scans inside one lane, and scans across workgroups


def test_verdicts_on_corrupt_scans():
    from lemon_amd import jpeg_host
    cases = mutants()
    assert len(cases) >= 2000
    both = host_declined = sync_only = 0
    for k, (name, raw) in enumerate(cases):
        ref, info = jpeg_host.decode_record(raw)
        subseq = jpeg_host.SUBSEQ_MIN if k % 2 == 0 else 0
        st, rec = par_decode(raw, subseq)
        if ref is None:
            host_declined += 1
            assert st != 0, (name, subseq, info.status)                         # whatever the host pass declines is declined
        elif st == 0:
            both += 1
            assert np.array_equal(rec, ref.data), (name, subseq)
        else:
            sync_only += 1
            assert st == 16, (name, subseq, st)                                 # only LEMON_JPEG_SYNC may decline more
    assert host_declined > 500 and both > 50, (host_declined, both, sync_only)


def test_states_that_meet_again_after_different_block_counts_are_not_accepted():
    # The first lane of the fourth workgroup (16-byte lanes: byte 3 * 256 * 16) holds the one place where a wrong start and the
    # right one meet again, after a different number of blocks.  Three rounds carry the truth across three workgroup borders at
    # most, so that lane's stored exit and block count come from the wrong start although its exit equals the right one: the
    # image must be LEMON_JPEG_SYNC -- never 0 with blocks written one off, never a wrong LEMON_JPEG_STREAM.  With the event inside
    # the first three workgroups, and at the default lane size (one workgroup spans 64 KB), the states settle and the file is accepted.
    from lemon_amd import jpeg_host
    for event_at, subseq, want in ((3 * 256 * 16, 16, 16), (5 * 256 * 16, 16, 16), (2 * 256 * 16, 16, 0), (3 * 256 * 16, 0, 0),
                                   (3 * 256 * 32, 32, 16)):
        raw = slow_sync_jpeg(event_at)
        ref, info = jpeg_host.decode_record(raw)
        assert ref is not None, info.status                                     # the host pass accepts the file
        st, rec = par_decode(raw, subseq)
        assert st == want, (event_at, subseq, st)
        if st == 0:
            assert np.array_equal(rec, ref.data), (event_at, subseq)


def test_declined_files_are_declined_by_the_packer_with_the_host_status():
    from lemon_amd import jpeg_host
    for name, raw, _ in jpegfx.declined_cases():
        head = jpeg_host.info(raw)
        full = jpeg_host.decode_record(raw)[1]
        pk, got = jpeg_host.pack(raw)
        assert pk is None and got.status == (head.status or full.status) and got.status > 0, (name, got.status, head.status, full.status)
    # a capacity that is too small is refused, not overrun
    raw = jpegfx.accepted_cases()[4][1]
    small = np.full(jpeg_host.PACKET_BOUND + 8, 0xA5, np.uint8)
    pk, got = jpeg_host.pack(raw, small[:jpeg_host.PACKET_BOUND])
    assert pk is None and got.status == 13 and (small[jpeg_host.PACKET_BOUND:] == 0xA5).all()


def test_pool_delivers_packets_that_decode_to_the_host_record(tmp_path):
    from lemon_amd import jpeg_host
    from lemon_amd.loader import DecodePool
    good = jpegfx.accepted_cases()[70:]
    bad = [c for c in jpegfx.declined_cases() if c[2]][:2]
    cases = good[:3] + bad + good[3:]
    paths = jpegfx.write_all(str(tmp_path), cases)
    with DecodePool(paths, workers=2, ring_bytes=2 << 20, packets=True) as pool:
        assert pool.torch_in_worker == [False, False]
        for i, item in pool.images():
            assert pool.held <= pool.ring_bytes
            if len(cases[i]) == 3:
                assert isinstance(item, np.ndarray), cases[i][0]                # the packer declined it: PIL pixels
                continue
            assert isinstance(item, jpeg_host.JpegPacket), cases[i][0]
            ref = jpeg_host.decode_record(cases[i][1])[0]
            rec = np.zeros(ref.data.size, np.uint8)
            assert jpeg_host.entropy_par_host(item.data.copy(), rec, 0) == 0
            assert np.array_equal(rec, ref.data) and (item.w, item.h) == (ref.w, ref.h), cases[i][0]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_packer_and_parallel_decode_fuzz_under_asan_and_ubsan(tmp_path, accepted):
    exe = str(tmp_path / "jpeg_par_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "jpeg_par_fuzz.cpp"), "-o", exe])
    rng = np.random.default_rng(2)
    cases = dict(accepted)
    seeds = [("s420", jpegfx.jpeg_bytes(jpegfx.pixels(48, 40, rng), quality=90, subsampling=2)),
             ("s444_opt", jpegfx.jpeg_bytes(jpegfx.pixels(23, 17, rng), quality=60, subsampling=0, optimize=True)),
             ("s422_rst", jpegfx.jpeg_bytes(jpegfx.pixels(40, 24, rng), quality=95, subsampling=1, restart_marker_blocks=2)),
             ("gray", jpegfx.jpeg_bytes(jpegfx.pixels(31, 33, rng, channels=1), quality=80)),
             ("noise", jpegfx.jpeg_bytes(jpegfx.pixels(16, 16, rng, noise=True), quality=100, subsampling=2, comment=b"hello")),
             ("restart_rows", cases["restart_rows"]), ("optimize_q100", cases["optimize_q100"])]
    paths = jpegfx.write_all(str(tmp_path), seeds)
    for n, seed in (("10000", "1"), ("10000", "20261017")):
        r = subprocess.run([exe, n, seed] + paths, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "jpeg_par_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
