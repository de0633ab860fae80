"""CPU: the host-side plan of the hand-written split-fp16 GEMM (lemon_amd/csrc/gemm_f16x3_plan.hpp: launch form, tile walk, grid)
against recorded decisions.

tests/golden/gemm_f16x3_plan.txt was NOT produced by the header under test: it was written by a stand-alone program holding the
three C entries and the decision lines of linear_f16x3t_impl as they stood at commit a37fab2 (the parent of the commit that
introduced the header; HIP calls stubbed out, the launch macro recording the instantiation it was handed, the MFMA shape and
the walk override its arguments), one row per call.  The same program and select_form() / plan_walk() agreed on all 16 416 rows
of the product of m in {1, 127, 128, 129, 4100, 18557}, the eight n of test_gpu_gemm_forms.py, k in {16, 32, 48, 768, 3072},
every (act, out_operand, fold, emit, out, residual_t) combination the three entries accept, MFMA shapes 16 and 32 and the walk
overrides none, 32,1 and 8,3 when the header was written; the committed subset keeps every combination under every shape and
override, with m, n and k rotated through their values."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lemon_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_f16x3_plan.txt")

# reads cases "abi mfma gm,gn m n k act out_operand fold emit out residual_t" (gm,gn = 0,0: no override), prints the table's rows
_PROBE = r"""
#include <stdio.h>
#include "gemm_f16x3_plan.hpp"
using namespace lemon_gemm_plan;
int main() {
    char abi[16]; int mfma, gm, gn, n, k, act, oo, fold, emit, out, rt; long long m;
    while (scanf("%15s %d %d,%d %lld %d %d %d %d %d %d %d %d", abi, &mfma, &gm, &gn, &m, &n, &k, &act, &oo, &fold, &emit, &out, &rt) == 13) {
        const Walk w = plan_walk(m, n, k, gm, gn);
        const Form f = select_form(mfma, w.ks, act, oo != 0, fold != 0, emit != 0, out != 0, rt != 0);
        printf("%s %d %d,%d %lld %d %d %d %d %d %d %d %d | %s %d %d %d %d %d %lld\n", abi, mfma, gm, gn, m, n, k, act, oo, fold, emit, out, rt,
               FACTS[f].name, w.m_tiles, w.n_tiles, w.ks, w.gm, w.gn, (long long)w.vblocks);
    }
    return 0;
}
"""

CASE_FIELDS = ("abi", "mfma", "walk", "m", "n", "k", "act", "out_operand", "fold", "emit", "out", "residual_t")
ROW_FIELDS = ("m_tiles", "n_tiles", "ks", "gm", "gn", "vblocks")


def table_rows():
    """[(case, row)] of the committed table, case and row as the text on either side of the bar"""
    rows = []
    for ln in open(TABLE):
        if ln.strip() and not ln.startswith("#"):
            case, row = ln.strip().split(" | ")
            rows.append((case, row))
    return rows


def parsed_rows():
    """the table as dicts: the case's fields, `kernel`, and the walk's fields"""
    out = []
    for case, row in table_rows():
        d = {f: (v if f in ("abi", "walk") else int(v)) for f, v in zip(CASE_FIELDS, case.split())}
        kernel, rest = row.rsplit(" ", len(ROW_FIELDS))[0], row.split()[-len(ROW_FIELDS):]
        d["kernel"] = kernel
        d.update({f: int(v) for f, v in zip(ROW_FIELDS, rest)})
        out.append(d)
    return out


def facts_names():
    """the reported names of FACTS[] in the header, in table order"""
    text = open(os.path.join(CSRC, "gemm_f16x3_plan.hpp")).read()
    body = text[text.index("FACTS[N_FORMS] = {"):]
    body = body[:body.index("};")]
    return [ln.split('"')[1] for ln in body.splitlines() if ln.strip().startswith('{"')]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next(p for p in (shutil.which(c) for c in ("g++", "c++", "clang++")) if p)   # (the build itself needs one: build.py)
    tmp = tmp_path_factory.mktemp("gemm_plan")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(_PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def test_the_plan_reproduces_every_recorded_decision(probe):
    rows = table_rows()
    got = subprocess.run([probe], input="\n".join(c for c, _ in rows) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    expect = [f"{c} | {r}" for c, r in rows]
    assert len(got) == len(expect) >= 300
    assert got == expect


def test_the_table_covers_what_it_has_to():
    rows = parsed_rows()
    names = facts_names()
    assert len(names) == 13 and {r["kernel"] for r in rows} == set(names)               # all 13 forms
    assert {r["gn"] for r in rows if r["walk"] == "0,0"} == {1, 2, 3, 4}
    assert any(r["n_tiles"] % r["gn"] for r in rows)                                     # a gn that does not divide the tile count
    assert any(r["walk"] == "8,3" and r["n_tiles"] < 3 and r["gn"] == r["n_tiles"] for r in rows)   # gn clamped to the tile count
    # odd k / 16 under shape 16 falls to the 32x32 forms; the fold and emit forms stay on 16x16x32 under shape 32
    odd = [r for r in rows if r["mfma"] == 16 and r["ks"] % 2]
    assert odd and all(r["kernel"].startswith("k_gemm_f16x3t<") for r in odd)
    assert any(r["mfma"] == 32 and (r["fold"] or r["emit"]) and r["kernel"].startswith("k_gemm_f16x3t16<") for r in rows)
    assert {r["walk"] for r in rows} == {"0,0", "32,1", "8,3"} and {r["mfma"] for r in rows} == {16, 32}
    assert {r["m"] for r in rows} == {1, 127, 128, 129, 4100, 18557}
    assert {r["n"] for r in rows} == {256, 512, 768, 1024, 1280, 1792, 2304, 3072}
    assert {r["k"] for r in rows} == {16, 32, 48, 768, 3072}
    # every accepted argument combination of the three entries
    combos = {(r["abi"], r["act"], r["out_operand"], r["fold"], r["emit"], r["out"], r["residual_t"]) for r in rows}
    assert len(combos) == 15 and {c[0] for c in combos} == {"plain", "ln", "chain"}
    # the grid is padded to whole super-blocks on all 8 XCDs and covers every tile
    for r in rows:
        assert r["vblocks"] % (8 * r["gm"] * r["gn"]) == 0 and r["vblocks"] >= r["m_tiles"] * r["n_tiles"]


def test_the_plan_header_is_plain_cxx():
    text = open(os.path.join(CSRC, "gemm_f16x3_plan.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    for word in ("hip", "getenv", "static "):
        assert word not in code, word
