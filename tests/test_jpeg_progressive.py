"""CPU: progressive JPEGs (csrc/jpeg_prog.hpp, csrc/jpeg_prog_par.hpp).  The sequential host pass + the device arithmetic on the
host against PIL, bit for bit; the device algorithm with its waves looped against the host pass, byte for byte; what must be
declined; the decode pool delivering records and packets; a sanitizer fuzz of all three."""
import io
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
from PIL import Image

from tests import jpegfx, jpegprogfx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pil(raw):
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


@pytest.fixture(scope="module")
def accepted():
    """[(name, bytes, host record, Info)] -- decoded once, shared, never written to."""
    from lemon_amd import jpeg_host
    out = []
    for name, raw in jpegprogfx.accepted_cases():
        rec, info = jpeg_host.decode_record(raw, progressive=True)
        assert rec is not None, (name, info.status, jpeg_host.STATUS.get(info.status))      # no file is declined
        rec.data.setflags(write=False)
        out.append((name, raw, rec, info))
    return out


def test_host_pass_equals_pil_bit_for_bit_and_declines_no_file(accepted):
    from lemon_amd import jpeg_host
    assert len(accepted) == 59
    for name, raw, rec, info in accepted:
        assert isinstance(rec, jpeg_host.JpegProgRecord) and jpeg_host.info(raw).status == 3, name       # (the baseline pass declines it)
        ref = _pil(raw)
        got = jpeg_host.reconstruct(rec)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))
        assert info.max_abs > 0 and info.record_bytes == rec.data.size, name
    blocks = {name: info.blocks for name, _, _, info in accepted}
    assert blocks["flat_gray_1456"] > 32767                              # one EOB run cannot cover the scan


def test_device_algorithm_looped_on_the_host_writes_the_same_record(accepted):
    from lemon_amd import jpeg_host
    levels, many = set(), 0
    for name, raw, rec, info in accepted:
        pk, head = jpeg_host.pack(raw, progressive=True)
        assert isinstance(pk, jpeg_host.JpegProgPacket) and head.status == 0, (name, head.status)
        assert pk.data.nbytes % 16 == 0 and pk.data.nbytes <= len(raw) + 2 * (len(raw) // 3) + jpeg_host.PROG_PACKET_BOUND, name
        assert (head.width, head.height, head.record_bytes) == (info.width, info.height, info.record_bytes), name
        assert pk.scans == (6 if info.components == 1 else 10) and pk.items >= pk.scans, (name, pk.scans)
        levels.add(pk.levels)
        many += pk.items > pk.scans
        out = np.full(head.record_bytes, 0xA5, np.uint8)
        st = jpeg_host.prog_entropy_par_host(pk.data, out)
        assert st == 0, (name, st, jpeg_host.STATUS.get(st))
        assert np.array_equal(out, rec.data), (name, int((out != rec.data).sum()))
    assert levels == {3} and many >= 2, (levels, many)                  # levels 0, 1, 2; both restart_blocks files have scans of several items


def test_files_that_must_be_declined():
    from lemon_amd import jpeg_host
    cases = jpegprogfx.declined_cases()
    assert len(cases) == 20
    for name, raw, want in cases:
        room = np.zeros(1 << 20, np.uint8)
        info = jpeg_host.prog_entropy(raw, room)
        assert info.status != 0, name
        if want is not None:
            assert info.status == want, (name, info.status)
        pk, head = jpeg_host.prog_pack(raw)
        assert pk is None and head.status == info.status, (name, head.status, info.status)
        if name.startswith("cut_after_"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                px = _pil(raw)                                           # PIL decodes an incomplete progression, smoothed
            assert px.shape == (80, 64, 3)
    # with the switch on, a baseline file still takes the baseline pass and the declined ones stay declined
    assert isinstance(jpeg_host.decode_record(cases[0][1], progressive=True)[0], jpeg_host.JpegRecord)
    assert jpeg_host.decode_record(cases[1][1], progressive=True)[0] is None
    assert jpeg_host.decode_record(jpegprogfx.accepted_cases()[0][1])[1].status == 3       # and without it nothing changes


def test_incomplete_progressions_differ_in_pil_from_the_complete_file():
    # (why they are declined: libjpeg smooths blocks whose progression is incomplete, so no plain inverse DCT gives its pixels)
    rng = np.random.default_rng(4)
    raw = jpegfx.jpeg_bytes(jpegfx.pixels(64, 80, rng), quality=90, subsampling=2, progressive=True)
    ref = _pil(raw)
    for k in range(1, 10):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            px = _pil(jpegprogfx.cut_after_scans(raw, k))
        assert not np.array_equal(px, ref), k


def test_accepted_single_byte_mutants_decode_like_pil_and_the_packer_declines_what_the_host_pass_does():
    from lemon_amd import jpeg_host
    cases = jpegprogfx.byte_mutants()
    assert len(cases) >= 2000
    accepted = declined = 0
    for name, raw in cases:
        first = jpeg_host.prog_info(raw)
        if first.record_bytes > 8 << 20:                                # (a mutated dimension: too large to be worth decoding here)
            continue
        room = np.zeros(max(int(first.record_bytes), 16), np.uint8)
        info = jpeg_host.prog_entropy(raw, room)
        pk, head = jpeg_host.prog_pack(raw)
        if pk is None:
            assert head.status == info.status, (name, head.status, info.status)          # header and marker checks: the same verdict
        else:
            assert info.status in (0, 10, 11, 12), (name, info.status)                   # what only decoding the scans can find
            out = np.zeros(head.record_bytes, np.uint8)
            assert jpeg_host.prog_entropy_par_host(pk.data, out) == info.status, name
        if info.status != 0:
            declined += 1
            continue
        accepted += 1
        rec = jpeg_host.JpegProgRecord(room[:info.record_bytes], info.width, info.height, info.components, info.hs, info.vs)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                              # accepted: libjpeg has nothing to warn about either
            ref = _pil(raw)
        got = jpeg_host.reconstruct(rec)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))
    assert accepted > 100 and declined > 500, (accepted, declined)


def test_pool_delivers_records_and_packets_for_progressive_files(tmp_path, accepted):
    from lemon_amd import jpeg_host
    from lemon_amd.loader import DecodePool
    prog = [(name, raw) for name, raw, _, _ in accepted if name in ("37x53_ss2_q90", "gray_41x67", "restart_rows1", "exif_com")]
    base = jpegfx.accepted_cases()[66:69]                     # (baseline files; names unlike the progressive ones)
    cmyk = [c[:2] for c in jpegfx.declined_cases() if c[0] == "cmyk"]
    cases = prog[:2] + base + cmyk + prog[2:]
    paths = jpegfx.write_all(str(tmp_path), cases)
    is_prog = [c in prog for c in cases]
    for kw in (dict(records=True), dict(packets=True)):
        with DecodePool(paths, workers=2, ring_bytes=2 << 20, progressive=True, **kw) as pool:
            assert pool.torch_in_worker == [False, False]
            for i, item in pool.images():
                name, raw = cases[i]
                if cases[i] in cmyk:
                    assert isinstance(item, np.ndarray) and np.array_equal(item, _pil(raw)), name
                    continue
                ref = jpeg_host.decode_record(raw, progressive=True)[0]
                if "records" in kw:
                    assert type(item) is (jpeg_host.JpegProgRecord if is_prog[i] else jpeg_host.JpegRecord), name
                    assert np.array_equal(item.data, ref.data), name
                    continue
                assert type(item) is (jpeg_host.JpegProgPacket if is_prog[i] else jpeg_host.JpegPacket), name
                out = np.zeros(ref.data.size, np.uint8)
                st = jpeg_host.prog_entropy_par_host(item.data.copy(), out) if is_prog[i] else jpeg_host.entropy_par_host(item.data.copy(), out, 0)
                assert st == 0 and np.array_equal(out, ref.data) and (item.w, item.h) == (ref.w, ref.h), name
        # without the flag a progressive file arrives as PIL's pixels, as before
        with DecodePool(paths, workers=2, ring_bytes=2 << 20, **kw) as pool:
            for i, item in pool.images():
                if is_prog[i]:
                    assert isinstance(item, np.ndarray) and np.array_equal(item, _pil(cases[i][1])), cases[i][0]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_pass_packer_and_looped_device_algorithm_fuzz_under_asan_and_ubsan(tmp_path, accepted):
    exe = str(tmp_path / "jpeg_prog_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "jpeg_prog_fuzz.cpp"), "-o", exe])
    rng = np.random.default_rng(2)
    jb = lambda px, **kw: jpegfx.jpeg_bytes(px, progressive=True, **kw)
    seeds = [("s420", jb(jpegfx.pixels(48, 40, rng), quality=90, subsampling=2)),
             ("s444", jb(jpegfx.pixels(23, 17, rng), quality=60, subsampling=0)),
             ("s422_rst", jb(jpegfx.pixels(40, 24, rng), quality=95, subsampling=1, restart_marker_blocks=2)),
             ("gray", jb(jpegfx.pixels(31, 33, rng, channels=1), quality=80)),
             ("noise", jb(jpegfx.pixels(16, 16, rng, noise=True), quality=95, subsampling=2, comment=b"hello")),
             ("rows", jb(jpegfx.pixels(40, 40, rng), quality=85, subsampling=2, restart_marker_rows=1))]
    paths = jpegfx.write_all(str(tmp_path), seeds)
    for n, seed in (("10000", "1"), ("10000", "20261017")):
        r = subprocess.run([exe, n, seed] + paths, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "jpeg_prog_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
