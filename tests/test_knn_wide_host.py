"""CPU: the host side of the wide fp16 filter scan -- the two new ABI entry points, their Python faces, and the host-only
arithmetic of lemon_amd/csrc/knn_wide.hpp (pitch rule, fragment homes) against values written out by hand."""
import os
import re
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemon_amd", "csrc")
NEW = ("lemon_index_set_wide_filter", "lemon_index_last_scan_kernel")


def test_header_and_binding_carry_the_new_entry_points():
    from lemon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    assert re.search(r"\bint\s+lemon_index_set_wide_filter\s*\(\s*lemon_index_t\s*\*\s*idx\s*,\s*int\s+enabled\s*\)\s*;", hdr)
    assert re.search(r"\bconst\s+char\s*\*\s*lemon_index_last_scan_kernel\s*\(\s*const\s+lemon_index_t\s*\*\s*idx\s*\)\s*;", hdr)
    for name in NEW:
        assert _lib.EXPORTS.count(name) == 1, name
    # lemon_search_info_t did not grow: the kernel's name has its own entry point
    struct = re.search(r"typedef struct \{(.*?)\} lemon_search_info_t;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)\s*(?:,\s*(\w+)\s*)?;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    names = [n for pair in fields for n in pair if n]
    assert names == ["algo", "grid", "block", "query_panel", "db_splits", "nq", "n", "d", "k", "nq_distinct"], names
    assert [f for f, _ in _lib.SearchInfo._fields_] == names


def test_both_index_classes_have_the_switch_and_the_kernel_name():
    from lemon_amd.index import IndexFlatIP, IndexFlatL2
    for cls in (IndexFlatIP, IndexFlatL2):
        assert callable(getattr(cls, "set_wide_filter")) and callable(getattr(cls, "last_scan_kernel"))


def test_the_library_exports_the_new_symbols():
    from lemon_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.lemon_index_last_scan_kernel(None) == b""            # a null handle names no kernel


_PROBE = r"""
#include <stdio.h>
#include "knn_wide.hpp"
int main() {
    const int ds[] = {1, 256, 257, 512, 513, 768, 769, 772, 800, 1000, 1024, 1025, 1028, 1276, 1280, 1281, 2048};
    for (int d : ds) printf("pitch %d %d %d\n", d, lemon_bf16_pitch(d, false), lemon_bf16_pitch(d, true));
    const int ps[] = {1024, 1280};
    for (int p : ps) {
        int a, f, t;
        lemon_qsw_register_homes(p, &a, &f, &t);
        printf("homes %d %d %d %d %d\n", p, lemon_qsw_steps(p), a, f, t);
    }
    printf("frag %d %d %d %d\n", lemon_qsw_frag_index(1024, 1, 0), (int)lemon_qsw_frag_in_acc(1024, 1, 31),
           lemon_qsw_frag_index(1280, 1, 24), (int)lemon_qsw_frag_in_acc(1280, 1, 24));
    printf("frag2 %d %d\n", (int)lemon_qsw_frag_in_acc(1280, 1, 23), (int)lemon_qsw_frag_in_acc(1280, 0, 39));
    return 0;
}
"""


def test_pitch_rule_and_fragment_homes_by_hand(tmp_path):
    cxx = next(p for p in (shutil.which(c) for c in ("g++", "c++", "clang++")) if p)   # (the build itself needs one: build.py)
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)])
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    # d, pitch with the switch off (as before the wide kernel: 256 / 512 / 768, then the next multiple of 64), pitch with it on
    pitches = {1: (256, 256), 256: (256, 256), 257: (512, 512), 512: (512, 512), 513: (768, 768), 768: (768, 768),
               769: (832, 1024), 772: (832, 1024), 800: (832, 1024), 1000: (1024, 1024), 1024: (1024, 1024),
               1025: (1088, 1280), 1028: (1088, 1280), 1276: (1280, 1280), 1280: (1280, 1280), 1281: (1344, 1344),
               2048: (2048, 2048)}
    seen = {}
    for ln in got:
        w = ln.split()
        if w and w[0] == "pitch":
            seen[int(w[1])] = (int(w[2]), int(w[3]))
    assert seen == pitches
    # pitch, k32 steps per tile, AccVGPRs, fragment VGPRs, accumulator-tile VGPRs:
    # 1024: 2 x 32 = 64 fragments x 4 = 256 AccVGPRs; 1280: 80 fragments = 64 in AccVGPRs + 16 x 4 = 64 VGPRs; tiles 4 x 2 x 4
    assert "homes 1024 32 256 0 32" in got and "homes 1280 40 256 64 32" in got
    # (1024: group 1 step 0 is fragment 32, its last step (63) still an AccVGPR home; 1280: group 1 step 24 is fragment 64,
    #  the first in VGPRs, step 23 the last in AccVGPRs, all of group 0 in AccVGPRs)
    assert "frag 32 1 64 0" in got and "frag2 1 1" in got
