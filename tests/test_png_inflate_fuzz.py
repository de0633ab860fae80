"""CPU: tests/native/png_inflate_fuzz.cpp -- a stand-alone program that mutates seeded valid zlib streams into the inflate of the
PNG path (csrc/png_inflate_core.hpp, the device's schedule looped on the host), checking termination, bounds and determinism,
and against zlib's inflate() where zlib.h is installed -- built with AddressSanitizer + UBSan and run as a program."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import inflatefx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_zlib_headers(tmp_path):
    """Whether `#include <zlib.h>` compiles and links here (the cross-check is skipped where it does not)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <zlib.h>\nint main() { return zlibVersion() == nullptr; }\n")
    r = subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe"), "-lz"], capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_inflate_fuzz_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "png_inflate_fuzz")
    cross = _have_zlib_headers(tmp_path)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "png_inflate_fuzz.cpp"), "-o", exe]
                          + (["-DPZ_FUZZ_ZLIB", "-lz"] if cross else []))
    edge = dict((c[0], c) for c in inflatefx.edge_cases())
    seeds = [edge[n] for n in ("lengths_dynamic", "lengths_fixed", "stored_at_bit_5", "final_after_100_blocks", "dist_code_15_bits",
                               "lit_code_15_bits", "single_dist_code_4", "repeat18_crosses", "match_as_token_64", "hclen_5_rle1")]
    seeds += [c for c in inflatefx.zlib_cases() if c[2] in (259, 32769) and c[0].startswith(("rows", "runs")) and "_w15_m9" in c[0]
              and ("_l6_default" in c[0] or "_l1_fixed" in c[0] or "_l0_default" in c[0])]
    assert len(seeds) >= 20
    paths = []
    for k, (name, z, want) in enumerate(seeds):
        p = str(tmp_path / f"seed{k:02d}.bin")
        with open(p, "wb") as fh:
            fh.write(struct.pack("<q", want) + z)
        paths.append(p)
    for cases, seed in (("6000", "1"), ("6000", "20261021")):
        r = subprocess.run([exe, cases, seed] + paths, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "png_inflate_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
