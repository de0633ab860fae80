"""CPU: tests/native/png_fuzz.cpp -- a stand-alone program that mutates seeded valid PNG files into the chunk parser
(csrc/png_core.hpp: lemon_png_info, lemon_png_idat) and feeds random and spoiled records to the device schedule looped on the host
(lemon_png_decode_host), checked against a row-by-row reference -- built with AddressSanitizer + UBSan and run as a program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pngfx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_png_parser_and_host_unfilter_fuzz_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "png_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "png_fuzz.cpp"), "-o", exe])
    rng = np.random.default_rng(4)
    seeds = [("grey", pngfx.png_bytes(pngfx.pixels(20, 17, 0, rng), 0)),
             ("rgb_split", pngfx.png_bytes(pngfx.pixels(9, 30, 2, rng), 2, splits=40, before_idat=[(b"gAMA", b"\0\0\xb1\x8f")])),
             ("palette_trns", pngfx.png_bytes(pngfx.pixels(12, 12, 3, rng, plte_count=9), 3, plte=pngfx.palette(9, rng), trns=b"\0\1\2")),
             ("grey_alpha_stored", pngfx.png_bytes(pngfx.pixels(5, 7, 4, rng), 4, level=0)),
             ("rgba_1byte", pngfx.png_bytes(pngfx.pixels(3, 4, 6, rng), 6, splits=1))]
    paths = pngfx.write_all(str(tmp_path), seeds)
    total = 0
    for cases, seed in (("12000", "1"), ("12000", "20261021")):
        r = subprocess.run([exe, cases, seed] + paths, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "png_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
        total += int(cases)
    assert total >= 20000
