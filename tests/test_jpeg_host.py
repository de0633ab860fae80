"""CPU: the host half of the GPU JPEG decode (lemon_amd/csrc/jpeg_entropy.hpp, liblemon_jpeg_host.so) and the device
arithmetic built for the host (csrc/jpeg_core.hpp): bit-equality with PIL, declined files, a sanitizer fuzz of the parser, and
the decode pool delivering coefficient records."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import jpegfx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pil(raw):
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


@pytest.fixture(scope="module")
def accepted():
    return jpegfx.accepted_cases()


def test_host_pass_plus_host_arithmetic_equal_pil_bit_for_bit(accepted):
    from lemon_amd import jpeg_host
    assert len(accepted) >= 82
    for name, raw in accepted:
        rec, info = jpeg_host.decode_record(raw)
        assert rec is not None, (name, info.status, jpeg_host.STATUS.get(info.status))      # none of these may be declined
        ref = _pil(raw)
        assert (rec.h, rec.w) == ref.shape[:2], name
        assert info.record_bytes == jpeg_host.QUANT_BYTES + 128 * jpeg_host.blocks_of(rec.w, rec.h, rec.components, rec.hs, rec.vs)
        got = jpeg_host.reconstruct(rec)
        assert np.array_equal(got, ref), (name, int(np.abs(got.astype(int) - ref).max()), int((got != ref).sum()))
        assert 0 < info.max_abs <= 16383, (name, info.max_abs)


def test_both_libraries_export_the_same_host_pass(accepted):
    from lemon_amd import _lib, jpeg_host
    hip = ctypes.CDLL(_lib.SO_PATH)
    hip.lemon_jpeg_entropy.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(jpeg_host.Info)]
    for name, raw in accepted[::9]:
        rec, _ = jpeg_host.decode_record(raw)
        other = np.zeros_like(rec.data)
        info = jpeg_host.Info()
        assert hip.lemon_jpeg_entropy(raw, len(raw), other.ctypes.data, other.size, ctypes.byref(info)) == 0, name
        assert np.array_equal(other, rec.data), name
    # the host library does not pull in the HIP runtime
    out = subprocess.run(["ldd", jpeg_host.SO_PATH], capture_output=True, text=True).stdout
    assert "amdhip" not in out and "hsa" not in out and "torch" not in out, out


def test_declined_files_are_declined_not_guessed():
    from lemon_amd import jpeg_host
    cases = jpegfx.declined_cases()
    names = [c[0] for c in cases]
    assert {"progressive", "cmyk", "png", "truncated_60", "huffman_flip"} <= set(names)
    for name, raw, _ in cases:
        rec, info = jpeg_host.decode_record(raw)
        assert rec is None and info.status > 0, (name, info.status)
    # a record buffer that is too small is refused, not overrun
    raw = jpegfx.accepted_cases()[4][1]
    small = np.zeros(100, np.uint8)
    assert jpeg_host.entropy(raw, small).status == 13 and not small.any()


def test_envelope_declines_coefficients_the_16_bit_forms_cannot_hold():
    # a quantiser of 255 on a file written at quality 100 (all ones): dequantised values 255 times larger than any 8-bit image's
    from lemon_amd import jpeg_host
    raw = bytearray(jpegfx.jpeg_bytes(jpegfx.pixels(64, 80, np.random.default_rng(3), noise=True), quality=100, subsampling=0))
    at = raw.index(b"\xff\xdb") + 5
    assert raw[at:at + 64] == b"\x01" * 64
    raw[at:at + 64] = b"\xff" * 64
    rec, info = jpeg_host.decode_record(bytes(raw))
    assert rec is None and info.status == 12, info.status


def test_pool_with_records_declined_files_come_as_pil_pixels(tmp_path):
    from lemon_amd import jpeg_host
    from lemon_amd.loader import DecodeError, DecodePool
    good = jpegfx.accepted_cases()[60:]
    bad = [c for c in jpegfx.declined_cases() if c[2]]
    cases = []
    for i, c in enumerate(good):              # declined files spread among the accepted ones
        cases.append(c)
        if i < len(bad):
            cases.append(bad[i])
    paths = jpegfx.write_all(str(tmp_path), cases)
    ring = 4 << 20
    kinds = []
    with DecodePool(paths, workers=2, ring_bytes=ring, records=True) as pool:
        assert pool.torch_in_worker == [False, False]
        seen = []
        for i, item in pool.images():
            assert pool.held <= pool.ring_bytes
            seen.append(i)
            ref = _pil(cases[i][1])
            if isinstance(item, jpeg_host.JpegRecord):
                kinds.append("record")
                got = jpeg_host.reconstruct(item._replace(data=item.data.copy()))
            else:
                kinds.append("pixels")
                got = item
            assert np.array_equal(got, ref), cases[i][0]
        assert seen == list(range(len(paths)))
        assert 0 < pool.peak_held <= pool.ring_bytes == ring
    for c, k in zip(cases, kinds):
        assert k == ("pixels" if len(c) == 3 else "record"), c[0]
    # a corrupt file: declined by the host pass, and PIL's own exception reaches the caller with the path
    corrupt = [c for c in jpegfx.declined_cases() if not c[2]]
    for c in corrupt:
        p = jpegfx.write_all(str(tmp_path), [c])
        with DecodePool(p, workers=1, ring_bytes=1 << 20, records=True) as pool:
            with pytest.raises(DecodeError, match=c[0]):
                list(pool.images())
    # records off (the default): pixels only, as before
    with DecodePool(paths[:4], workers=1, ring_bytes=1 << 20) as pool:
        assert all(isinstance(a, np.ndarray) for _, a in pool.images())


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_jpeg_parser_fuzz_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "jpeg_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "jpeg_fuzz.cpp"), "-o", exe])
    rng = np.random.default_rng(2)
    seeds = [("s420", jpegfx.jpeg_bytes(jpegfx.pixels(48, 40, rng), quality=90, subsampling=2)),
             ("s444_opt", jpegfx.jpeg_bytes(jpegfx.pixels(23, 17, rng), quality=60, subsampling=0, optimize=True)),
             ("s422_rst", jpegfx.jpeg_bytes(jpegfx.pixels(40, 24, rng), quality=95, subsampling=1, restart_marker_blocks=2)),
             ("gray", jpegfx.jpeg_bytes(jpegfx.pixels(31, 33, rng, channels=1), quality=80)),
             ("noise", jpegfx.jpeg_bytes(jpegfx.pixels(16, 16, rng, noise=True), quality=100, subsampling=2, comment=b"hello"))]
    paths = jpegfx.write_all(str(tmp_path), seeds)
    total = 0
    for cases, seed in (("12000", "1"), ("12000", "20261017")):
        r = subprocess.run([exe, cases, seed] + paths, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "jpeg_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
        total += int(cases)
    assert total >= 20000
