"""CPU: the host-side plan of the 16-bit filter scan (lemon_amd/csrc/knn_bf16_plan.hpp: kernel, chunk cut, database splits,
Infinity-Cache chunks, carried state) against recorded decisions.

tests/golden/knn_bf16_plan.txt was NOT produced by the header under test: it was written by a stand-alone program holding the
decision lines of lemon_search_bf16 and lemon_plan_splits as they stood at commit f7bbf08 (the parent of the commit that
introduced the header; HIP calls stubbed out, the CU count an argument, the knobs through the same environment variables), one
row per query chunk.  The same program and plan_chunk() agreed on all 109 396 rows of a much larger product of shapes and knobs
when the header was written; the committed subset keeps every kernel, the 1 M x 1 M x 768 headline shape for both metrics,
whole rounds with a ragged rest through QS4 and through QSW, LEMON_CHUNK_MB per kernel family, streaming at d % 4 != 0,
n < 64, and LEMON_QS4=0 / LEMON_QS2=0.  The rows behind the table's last comment line (the shapes of tests/indexfx.py) were added
later, from the header itself: they pin it down from then on, and tests/test_gpu_index_state.py holds the launches against them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemon_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "knn_bf16_plan.txt")

# reads cases "knob d wide l2 n nq cus" (knob: "defaults" or NAME=VALUE of one LEMON_<NAME> variable), prints the table's rows
_PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "knn_wide.hpp"
#include "knn_bf16_plan.hpp"
using namespace lemon_bf16_plan;
int main() {
    char knob[64]; int d, wide, l2, cus; long long n, nq;
    while (scanf("%63s %d %d %d %lld %lld %d", knob, &d, &wide, &l2, &n, &nq, &cus) == 7) {
        Knobs kn;
        const char *v = strchr(knob, '=') ? strchr(knob, '=') + 1 : "";
        if (!strncmp(knob, "QS2_MIN_PANELS=", 15)) kn.qs2_min_panels = atoi(v);
        else if (!strncmp(knob, "QS4=", 4)) kn.qs4 = v[0] != '0';
        else if (!strncmp(knob, "QS2=", 4)) kn.qs2 = v[0] != '0';
        else if (!strncmp(knob, "QS4_REST=", 9)) kn.rest_split = v[0] != '0';
        else if (!strncmp(knob, "CHUNK_MB=", 9)) kn.chunk_mb = atof(v);
        else if (!strncmp(knob, "SPLITS=", 7)) kn.forced_splits = atoi(v);
        else if (strcmp(knob, "defaults")) return 2;
        const int pitch = lemon_bf16_pitch(d, wide != 0);
        Kernel prev = SCAN_BF16;
        int chunk = 0;
        for (long long c0 = 0; c0 < nq; ++chunk) {
            const Plan p = plan_chunk(nq - c0, c0 == 0, prev, n, d, pitch, l2 != 0, wide != 0, cus, kn);
            printf("%s %d %d %d %lld %lld %d | %d %s %lld %d %d %d %d %d %d %d %lld %lld %d\n", knob, d, wide, l2, n, nq, cus, chunk,
                   p.name, (long long)p.cn, p.panel, p.tile, p.n_tiles, p.panels, p.splits, p.tiles_per_split, p.chunk_tiles,
                   (long long)p.state_elems, (long long)p.cnt_elems, p.segs);
            prev = p.kernel; c0 += p.cn;
        }
    }
    return 0;
}
"""

FIELDS = ("chunk", "kernel", "cn", "query_panel", "tile_rows", "n_tiles", "panels", "splits", "tiles_per_split", "chunk_tiles",
          "state_elems", "cnt_elems", "segs")


def table_rows():
    """[(case, row)] of the committed table, case and row as the text on either side of the bar"""
    rows = []
    for ln in open(TABLE):
        if ln.strip() and not ln.startswith("#"):
            case, row = ln.strip().split(" | ")
            rows.append((case, row))
    return rows


def planned(knob, d, wide, l2, n, nq, cus=256):
    """the recorded rows of one case as dicts, one per query chunk"""
    case = f"{knob} {d} {int(wide)} {int(l2)} {n} {nq} {cus}"
    out = []
    for c, row in table_rows():
        if c == case:
            w = row.split()
            out.append({f: (w[i] if f == "kernel" else int(w[i])) for i, f in enumerate(FIELDS)})
    assert out, f"no recorded row for {case}"
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next(p for p in (shutil.which(c) for c in ("g++", "c++", "clang++")) if p)   # (the build itself needs one: build.py)
    tmp = tmp_path_factory.mktemp("bf16_plan")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(_PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def test_the_plan_reproduces_every_recorded_decision(probe):
    rows = table_rows()
    cases = list(dict.fromkeys(c for c, _ in rows))
    got = subprocess.run([probe], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    want = {}
    for c, r in rows:
        want.setdefault(c, []).append(f"{c} | {r}")
    expect = [ln for c in cases for ln in want[c]]
    assert len(got) == len(expect) >= 250
    assert got == expect


def test_the_table_covers_what_it_has_to():
    rows = table_rows()
    kernels = {r.split()[1] for _, r in rows}
    assert kernels == {"scan_bf16", "qs", "qs2", "qs4", "qsw"}
    # the headline shape: whole rounds, then the rest -- 67 panels in 3 splits through QS4, 133 one-block panels x 6 behind QS2
    ip, l2 = (planned("defaults", 768, 0, m, 1000000, 1000000) for m in (0, 1))
    for head in (ip, l2):
        assert [r["cn"] for r in head] == [524288, 458752, 16960]
    assert [(r["kernel"], r["panels"], r["splits"]) for r in ip] == [("qs4", 2048, 1), ("qs4", 1792, 1), ("qs4", 67, 3)]
    assert [(r["kernel"], r["panels"], r["splits"]) for r in l2] == [("qs2", 2048, 1), ("qs2", 1792, 1), ("qs", 133, 6)]
    # one whole round plus a 114-panel rest in 2 splits, through QS4 and through QSW
    for d, wide, nq, name in ((512, 0, 94536, "qs4"), (1024, 1, 47268, "qsw")):
        a, b = planned("QS2_MIN_PANELS=256", d, wide, 0, 20000, nq)
        assert (a["kernel"], a["panels"], b["kernel"], b["panels"], b["splits"]) == (name, 256, name, 114, 2)
    for d, wide, l2, name in ((256, 0, 0, "qs"), (768, 0, 1, "qs2"), (512, 0, 0, "qs4"), (1024, 1, 0, "qsw")):
        r = planned("CHUNK_MB=0.01", d, wide, l2, 20000, 262144)[0]
        assert r["kernel"] == name and r["splits"] == 1 and r["chunk_tiles"] == 8 < r["n_tiles"]
    assert planned("defaults", 1001, 0, 0, 5000, 1100)[0]["kernel"] == "scan_bf16"          # d % 4 != 0, streamed
    assert planned("QS2_MIN_PANELS=0", 768, 0, 0, 63, 257)[0]["n_tiles"] == 1                # n < 64
    assert planned("QS4=0", 512, 0, 0, 20000, 262144)[0]["kernel"] == "qs2"
    assert planned("QS2=0", 512, 0, 0, 20000, 262144)[0]["kernel"] == "qs"


def test_the_plan_header_is_plain_cxx():
    text = open(os.path.join(CSRC, "knn_bf16_plan.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    for word in ("hip", "getenv", "static "):
        assert word not in code, word
