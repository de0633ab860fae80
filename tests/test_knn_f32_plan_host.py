"""CPU: the host-side plan of the exact fp32 scan (lemon_amd/csrc/scan_plan.hpp: chunk cut, segment plan or (panel, split)
rectangles, grid, splits, fair-share bit, shared bounds, re-selection trigger) against recorded decisions.

tests/golden/knn_f32_plan.txt was NOT produced by the header under test: it was written by a stand-alone program holding the
decision lines of lemon_plan_splits, lemon_plan_segments and the chunk loop of lemon_search_f32_pass (up to `grid`, and from
`share` to `p.fair`) as they stood at commit e7c5dca (the parent of the commit that moved them into the header), with that
commit's scan_plan.hpp included unchanged, HIP calls stubbed out, the CU count an argument and the knobs through the same
environment variables -- one process per knob setting and CU count, since that code latched them per process.  One row per query
chunk; plan_hash is the 64-bit FNV-1a (offset 14695981039346656037, prime 1099511628211) over the ints of seg_begin, pieces and
segs in that order, each int as its four bytes from the least significant, and 0 for a chunk without a segment plan: it pins the
whole segment table in one word.  The same program and plan_chunk() agreed on all 351 540 rows of a much larger product of shapes
and knobs when the header was extended; the committed subset keeps what test_the_table_covers_what_it_has_to lists."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemon_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "knn_f32_plan.txt")

# reads cases "knob d l2 n nq cus" (knob: "defaults" or NAME=VALUE of one LEMON_<NAME> variable, parsed as read_scan_knobs() of
# knn_f32.hip parses the variable), prints the table's rows
_PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scan_plan.hpp"
using namespace lemon_f32_plan;
static unsigned long long fnv(unsigned long long h, const std::vector<int> &v) {
    for (int x : v)
        for (int b = 0; b < 4; ++b) { h ^= ((unsigned)x >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    return h;
}
int main() {
    char knob[64]; int d, l2, cus; long long n, nq;
    while (scanf("%63s %d %d %lld %lld %d", knob, &d, &l2, &n, &nq, &cus) == 6) {
        Knobs kn;
        const char *v = strchr(knob, '=') ? strchr(knob, '=') + 1 : "";
        if (!strncmp(knob, "SPLITS=", 7)) { kn.splits_set = true; kn.splits = atoi(v); }
        else if (!strncmp(knob, "XCDS=", 5)) { if (atoi(v) > 0) kn.xcds = atoi(v); }
        else if (!strncmp(knob, "SEG_COST=", 9)) kn.seg_cost = atoi(v);
        else if (!strncmp(knob, "SHARE_BOUNDS=", 13)) kn.share_bounds = v[0] != '0';
        else if (!strncmp(knob, "STALE=", 6)) { if (atoi(v) > 0) kn.stale = atoi(v); }
        else if (!strncmp(knob, "FAIR=", 5)) kn.fair = atoi(v);
        else if (strcmp(knob, "defaults")) return 2;
        int chunk = 0;
        for (long long c0 = 0; c0 < nq; ++chunk) {
            Chunk c = plan_chunk(nq - c0, n, d, cus, kn);
            unsigned long long h = 0;
            int n_segs = 0;
            if (c.planned) {
                LemonPlan plan;
                plan_segments(c, plan);
                set_geometry(c, plan.grid, plan.splits);
                h = fnv(fnv(fnv(14695981039346656037ull, plan.seg_begin), plan.pieces), plan.segs);
                n_segs = (int)(plan.segs.size() / 4);
            }
            printf("%s %d %d %lld %lld %d | %d %lld %d %d %d %d %d %d %d %d %d %d %016llx\n", knob, d, l2, n, nq, cus, chunk,
                   (long long)c.cn, c.panels, c.n_tiles, (int)c.planned, c.grid, c.splits, c.tiles_per_split, c.fair, (int)c.share,
                   c.stale, n_segs, h);
            c0 += c.cn;
        }
    }
    return 0;
}
"""

FIELDS = ("chunk", "cn", "panels", "n_tiles", "planned", "grid", "splits", "tiles_per_split", "fair", "share", "stale", "n_segs")


def table_rows():
    """[(case, row)] of the committed table, case and row as the text on either side of the bar"""
    rows = []
    for ln in open(TABLE):
        if ln.strip() and not ln.startswith("#"):
            case, row = ln.strip().split(" | ")
            rows.append((case, row))
    return rows


def planned(knob, d, l2, n, nq, cus=256):
    """the recorded rows of one case as dicts, one per query chunk"""
    case = f"{knob} {d} {int(l2)} {n} {nq} {cus}"
    out = []
    for c, row in table_rows():
        if c == case:
            w = row.split()
            out.append(dict({f: int(w[i]) for i, f in enumerate(FIELDS)}, plan_hash=w[len(FIELDS)]))
    assert out, f"no recorded row for {case}"
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next(p for p in (shutil.which(c) for c in ("g++", "c++", "clang++")) if p)   # (the build itself needs one: build.py)
    tmp = tmp_path_factory.mktemp("f32_plan")
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
    assert 200 <= len(got) == len(expect) <= 300
    assert got == expect


def test_the_table_covers_what_it_has_to():
    rows = table_rows()
    # the shape the fp32 tools time; 131 072^2 x 512; the shapes of the per-call knob tests (tests/test_gpu_index_state.py)
    head = planned("defaults", 512, 0, 40000, 50000)
    assert [(r["cn"], r["panels"], r["n_tiles"], r["planned"], r["grid"]) for r in head] == [(50000, 391, 313, 1, 512)]
    assert planned("defaults", 512, 0, 131072, 131072)[0]["grid"] == 512
    small = planned("defaults", 64, 0, 3000, 300)[0]
    assert (small["panels"], small["n_tiles"], small["planned"], small["grid"]) == (3, 24, 1, 9)
    assert [planned(kn, 64, 0, 2048, 256)[0]["splits"] for kn in ("defaults", "SEG_COST=0")] == [3, 2]
    # 1 M x 1 M x 768, both metrics: two chunks of at most 2^19 queries; 1.1 M queries: three
    for l2 in (0, 1):
        assert [r["cn"] for r in planned("defaults", 768, l2, 1000000, 1000000)] == [1 << 19, 1000000 - (1 << 19)]
    three = planned("defaults", 768, 0, 1000000, 1100000)
    assert [r["chunk"] for r in three] == [0, 1, 2] and three[2]["cn"] == 1100000 - (1 << 20)
    # a unit space below 2 is unplanned; nq and n on either side of 128
    edge = {(nq, n): planned("defaults", 64, 0, n, nq)[0] for nq in (128, 129) for n in (128, 129)}
    assert [edge[key]["planned"] for key in ((128, 128), (129, 128), (128, 129), (129, 129))] == [0, 1, 1, 1]
    assert (edge[(128, 128)]["grid"], edge[(128, 128)]["splits"], edge[(128, 128)]["plan_hash"]) == (1, 1, "0" * 16)
    assert planned("defaults", 64, 0, 100, 77)[0]["planned"] == 0
    # every knob at a non-default value, two CU counts
    knobs = {c.split()[0] for c, _ in rows}
    assert knobs >= {"defaults", "SPLITS=0", "SPLITS=1", "SPLITS=2", "XCDS=1", "SEG_COST=0", "SEG_COST=6", "FAIR=0", "FAIR=13",
                     "FAIR=100", "STALE=32", "SHARE_BOUNDS=0"}
    assert {int(c.split()[5]) for c, _ in rows} >= {256, 304}
    by_knob = lambda kn: [dict(zip(FIELDS, map(int, r.split()[:len(FIELDS)]))) for c, r in rows if c.split()[0] == kn]
    assert all(r["planned"] == 0 and r["n_segs"] == 0 for kn in ("SPLITS=0", "SPLITS=1", "SPLITS=2") for r in by_knob(kn))
    assert any(r["splits"] == 2 and r["grid"] == 2 * r["panels"] for r in by_knob("SPLITS=2"))
    assert all(r["splits"] == 1 for r in by_knob("SPLITS=1")) and any(r["splits"] > 2 for r in by_knob("SPLITS=0"))
    for kn, fair in (("FAIR=0", 0), ("FAIR=13", 13), ("FAIR=100", 100)):
        assert {r["fair"] for r in by_knob(kn)} == {fair}
    assert {r["stale"] for r in by_knob("STALE=32")} == {32} and {r["stale"] for r in by_knob("defaults")} == {96}
    assert any(r["splits"] > 1 for r in by_knob("SHARE_BOUNDS=0")) and not any(r["share"] for r in by_knob("SHARE_BOUNDS=0"))
    assert all(r["share"] == (r["splits"] > 1) for r in by_knob("defaults"))
    # derived fair bits: both clamps and strictly between
    derived = {r["fair"] for r in by_knob("defaults")}
    assert {13, 19} <= derived <= set(range(13, 20)) and derived & set(range(14, 19))
    # XCDS=1 and the other CU count really change a segment table that the defaults also record
    for other, cus in (("XCDS=1", 256), ("defaults", 304)):
        assert planned(other, 512, 0, 131072, 131072, cus)[0]["plan_hash"] != planned("defaults", 512, 0, 131072, 131072)[0]["plan_hash"]


def test_the_plan_header_is_plain_cxx():
    """beyond its `static inline` functions (plan_group, lemon_plan_segments_host: as before), no HIP, no getenv, no static"""
    text = open(os.path.join(CSRC, "scan_plan.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines()).replace("static inline void plan_group(", "").replace(
        "static inline void lemon_plan_segments_host(", "")
    for word in ("hip", "getenv", "static "):
        assert word not in code, word
