"""CPU: the host-side plan of the attention family (lemon_amd/csrc/attention_plan.hpp: which of the 68 instantiations serves a call,
its grid, threads, dynamic LDS and LDS attribute, or the refusal) against recorded decisions.

tests/golden/attention_plan.txt was NOT produced by the header under test: it was written by a stand-alone program holding the
host lines of the three dispatchers as they stood at commit 974b7fe (the parent of the commit that introduced the header:
attention.hip from lemon_attention_set_f16 to the end, launch / lemon_attention_hdx of attention_hd.hip, attention_varlen_impl and
the entries of attention_varlen.hip; HIP calls stubbed out, LEMON_REQUIRE as it is, the launch macro recording the instantiation
it was handed with grid, block and LDS bytes, the attribute call recording kernel and value), one row per call, one process per
(LEMON_ATTN_SHORT, LEMON_ATTN_GENERAL) pair.  The same program and plan() agreed on all 1 881 632 rows of: entry {plain, varlen} x
output form 0..3 x seq_len {1, 32, 33, 64, 65, 96, 160, 161, 192, 256, 257, 288, 289, 577, 1025, 4096, 4097} x head_dim {64, 72,
80, 96, 104, 128, 136, 60} x heads {2, 16, 19417, 19418, 19419, 43689, 43690, 43691} x arithmetic 0..2 x stream_min {64, 200, 288} x
head-dim mode 0..2 x short_off x old_general x batch {0, 2}, plus 1 568 rows beside the product (batch * heads on either side of
2^31, which no batch of the product reaches; seq_len 128 and 224 for the tile counts 4 and 7; seq_len 0, heads 0, batch -1; a tile-major
output with heads * head_dim = 240).  (The offset guards' messages say heads < 19 418 and < 43 690; their conditions take these
values and refuse the next, and so does the plan.)  The committed subset keeps, per (entry, seq_len, head_dim, heads beside a guard, outcome without grid x and output form), one or two
rows with the other axes rotated through their values, and the 77 rows tests/test_gpu_attention_plan.py runs on the GPU (recorded
by the same program)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemon_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "attention_plan.txt")

# reads the table's cases and prints its rows; `facts`: FACTS[] ("form split unit slot tj f16 max_threads attr | name") and MESSAGES[]
_PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "attention_plan.hpp"
using namespace lemon_attn_plan;
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "facts")) {
        for (int f = 0; f < N_FORMS; ++f)
            for (int s = 0; s < 4; ++s)
                printf("%d %d %d %d %d %d %d %d | %s\n", f, s, (int)FACTS[f].unit, FACTS[f].slot, FACTS[f].tj, (int)FACTS[f].f16, FACTS[f].max_threads,
                       FACTS[f].attr, FACTS[f].name[s]);
        for (int r = 1; r < N_REFUSALS; ++r) printf("message | %s\n", MESSAGES[r]);
        return 0;
    }
    char entry[16]; int split, seq, hd, heads, arith, smin, hdm, so, og; long long batch;
    while (scanf("%15s %d %d %d %d %d %d %d %d %d %lld", entry, &split, &seq, &hd, &heads, &arith, &smin, &hdm, &so, &og, &batch) == 11) {
        const Knobs k = {arith, smin, hdm, so != 0, og != 0};
        const Plan p = plan(k, batch, seq, heads, hd, split, !strcmp(entry, "varlen"));
        printf("%s %d %d %d %d %d %d %d %d %d %lld | ", entry, split, seq, hd, heads, arith, smin, hdm, so, og, batch);
        const Refusal r = p.early != ACCEPTED ? p.early : p.late;
        if (r != ACCEPTED) printf("refused %d %s\n", E_INVALID, MESSAGES[r]);
        else if (batch == 0) printf("nothing\n");
        else printf("%s %u %u %d %d %d\n", FACTS[p.form].name[split], p.grid_x, p.grid_y, p.threads, p.lds, FACTS[p.form].attr);
    }
    return 0;
}
"""

CASE_FIELDS = ("entry", "split", "seq_len", "head_dim", "heads", "arithmetic", "stream_min", "head_dims", "short_off", "old_general", "batch")
ROW_FIELDS = ("grid_x", "grid_y", "threads", "lds", "attr")


def table_rows():
    """[(case, row)] of the committed table, case and row as the text on either side of the bar"""
    rows = []
    for ln in open(TABLE):
        if ln.strip() and not ln.startswith("#"):
            case, row = ln.rstrip("\n").split(" | ")
            rows.append((case, row))
    return rows


def parsed_rows():
    """the table as dicts: the case's fields and `kernel` + the launch's fields, or `refused` (the message), or neither (batch == 0)"""
    out = []
    for case, row in table_rows():
        d = {f: (v if f == "entry" else int(v)) for f, v in zip(CASE_FIELDS, case.split())}
        d["kernel"] = d["refused"] = None
        if row.startswith("refused "):
            code, d["refused"] = row.split(" ", 2)[1:]
            assert code == "-1"
        elif row != "nothing":
            d["kernel"] = row.rsplit(" ", len(ROW_FIELDS))[0]
            d.update({f: int(v) for f, v in zip(ROW_FIELDS, row.split()[-len(ROW_FIELDS):])})
            d["tj"] = (d["seq_len"] + 31) // 32
        out.append(d)
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next(p for p in (shutil.which(c) for c in ("g++", "c++", "clang++")) if p)   # (the build itself needs one: build.py)
    tmp = tmp_path_factory.mktemp("attention_plan")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(_PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def facts(probe):
    """({name: dict of its FACTS row}, [refusal messages]) of the header"""
    names, messages = {}, []
    for ln in subprocess.run([probe, "facts"], capture_output=True, text=True, check=True).stdout.splitlines():
        left, right = ln.split(" | ", 1)
        if left == "message":
            messages.append(right)
        else:
            names[right] = dict(zip(("form", "split", "unit", "slot", "tj", "f16", "max_threads", "attr"), map(int, left.split())))
    return names, messages


def test_the_plan_reproduces_every_recorded_decision(probe):
    rows = table_rows()
    got = subprocess.run([probe], input="\n".join(c for c, _ in rows) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    expect = [f"{c} | {r}" for c, r in rows]
    assert len(got) == len(expect) >= 1500
    assert got == expect


def test_the_table_covers_what_it_has_to(facts):
    names, messages = facts
    rows = parsed_rows()
    launched = [r for r in rows if r["kernel"]]
    assert len(names) == 68 and len({f["form"] for f in names.values()}) == 17
    assert {r["kernel"] for r in launched} == set(names)                                 # every form in every output form
    one_wg = [r for r in launched if "stream" not in r["kernel"]]                         # the <= 288 families
    for entry in ("plain", "varlen"):
        assert {r["tj"] for r in one_wg if r["entry"] == entry} == set(range(1, 10)), entry
    # both branches of the staged form's key-block rule (the plain entry reaches tj 1 and 2 with LEMON_ATTN_SHORT=0)
    for frag, first in (("k_attention_hd64_f16<", 1), ("k_attnvl_f16<", 3)):
        staged = {r["tj"]: r["lds"] for r in launched if r["kernel"].startswith(frag)}
        assert set(staged) == set(range(first, 10)), frag
        for tj, lds in staged.items():
            tb = tj if (tj <= 5 or tj > 8) else (tj + 1) // 2
            assert lds == max(4 * 32 * tb * 128, 32 * tj * 256), (frag, tj, lds)
    for frag, wmax in (("k_attention_hd64_stream<", 4), ("k_attention_hd64_stream_f16<", 8)):
        assert {1, 2, 3} <= {r["grid_y"] for r in launched if r["kernel"].startswith(frag)}, frag
        assert all(r["grid_y"] == -(-r["tj"] // wmax) for r in launched if r["kernel"].startswith(frag)), frag
    assert {r["lds"] for r in launched if "hdx_stream<96" in r["kernel"]} == {2 * 64 * 100 * 4}
    assert {r["lds"] for r in launched if "hdx_stream<128" in r["kernel"]} == {2 * 64 * 132 * 4}
    assert len(messages) == 10 and {r["refused"] for r in rows if r["refused"]} == set(messages)
    for entry in ("plain", "varlen"):                                                    # batch == 0 does not hide a bad head_dim
        assert any(r["batch"] == 0 and r["head_dim"] in (60, 136) and r["refused"] and "head_dim must be 64" in r["refused"]
                   for r in rows if r["entry"] == entry), entry
    assert any(r["batch"] == 0 and not r["refused"] and not r["kernel"] for r in rows)
    # every value of every axis, and both sides of every threshold
    for f, values in (("split", range(4)), ("arithmetic", range(3)), ("stream_min", (64, 200, 288)), ("head_dims", range(3)),
                      ("short_off", (0, 1)), ("old_general", (0, 1)), ("head_dim", (64, 72, 80, 96, 104, 128, 136, 60)),
                      ("heads", (2, 16, 19417, 19418, 19419, 43689, 43690, 43691)),
                      ("seq_len", (1, 32, 33, 64, 65, 96, 160, 161, 192, 256, 257, 288, 289, 577, 1025, 4096, 4097))):
        assert {r[f] for r in rows} >= set(values), f
    for entry, frag, ok, bad in (("varlen", "heads < 19 418", 19418, 19419), ("plain", "heads < 43 690", 43690, 43691),
                                 ("plain", "64 * 3 * heads * head_dim", 43690, 43691)):
        hit = [r for r in rows if r["refused"] and frag in r["refused"]]
        assert hit and min(r["heads"] for r in hit) == bad, frag
        assert any(r["entry"] == entry and r["heads"] == ok and r["kernel"] and (r["head_dim"] == 128 or "head_dim" not in frag)
                   and ("stream" in r["kernel"] or entry == "varlen") for r in rows), frag
    grid = [r for r in rows if r["refused"] and "batch * heads < 2^31" in r["refused"]]
    assert {r["entry"] for r in grid} == {"plain", "varlen"} and all(r["batch"] * r["heads"] == 2 ** 31 for r in grid)
    assert any(r["kernel"] and r["grid_x"] == 2 ** 31 - 16 for r in rows)
    # the asymmetries the plan has to keep: the varlen entries ignore both environment knobs and run the staged form under
    # arithmetic 2; head-dim mode 2 sends head_dim 64 to the hdx kernel on the plain entries only, under every arithmetic
    assert any(r["entry"] == "varlen" and r["short_off"] and r["kernel"] and "k_attnvl_short" in r["kernel"] for r in rows)
    assert any(r["entry"] == "plain" and r["short_off"] and r["tj"] <= 2 and r["kernel"].startswith("k_attention_hd64<") for r in launched)
    assert any(r["entry"] == "varlen" and (r["old_general"] or r["arithmetic"] == 2) and r["kernel"].startswith("k_attnvl_f16<") for r in launched)
    assert any(r["arithmetic"] == 1 and r["old_general"] and r["kernel"].endswith(", true>") and r["kernel"].startswith("k_attention_hd64<")
               for r in launched)
    mode2 = [r for r in launched if r["head_dims"] == 2 and r["head_dim"] == 64]
    assert {r["arithmetic"] for r in mode2 if r["entry"] == "plain"} == {0, 1, 2}
    assert all(("hdx_stream<96" in r["kernel"]) == (r["entry"] == "plain") for r in mode2)


def test_every_planned_launch_fits_its_kernel(facts):
    names, _ = facts
    for r in parsed_rows():
        if not r["kernel"]:
            continue
        f = names[r["kernel"]]
        assert r["attr"] == f["attr"] and r["lds"] <= (f["attr"] or 64 * 1024), r
        assert r["threads"] % 64 == 0 and 64 <= r["threads"] <= f["max_threads"] <= 576, r
        assert r["grid_y"] * (r["threads"] // 64) >= r["tj"] and r["grid_x"] == r["batch"] * r["heads"], r
        assert f["tj"] in (0, r["tj"]) and f["split"] == r["split"], r


def test_the_plan_header_is_plain_cxx():
    text = open(os.path.join(CSRC, "attention_plan.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    for word in ("hip", "getenv", "static "):
        assert word not in code, word
