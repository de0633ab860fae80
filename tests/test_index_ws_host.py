"""The index handle's buffers without a GPU: csrc/index_ws.hpp -- LemonBuf and the one rule by which every workspace of a handle
grows -- driven by tests/native/index_ws_fuzz.cpp with a fake allocator that fails where it is told to."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemon_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_buffer_header_alone(tmp_path, flags):
    """random reserve / group reserve / release sequences with an allocation failure at every position, and the named
    xh / xh_stats sequence (the stand-alone program only: nothing is loaded into Python)"""
    exe = str(tmp_path / "index_ws_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + [os.path.join(ROOT, "tests", "native", "index_ws_fuzz.cpp"), "-o", exe])
    for seed in ("1", "20261020"):
        r = subprocess.run([exe, "20000", seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "index_ws_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_the_buffer_header_is_plain_cxx():
    text = open(os.path.join(CSRC, "index_ws.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    for word in ("hip", "getenv", "static "):
        assert word not in code, word
    from lemon_amd import build
    assert "index_ws.hpp" in build.HEADERS

