"""GPU: what lemon_search_bf16 launches is what knn_bf16_plan.hpp planned -- after a search, last_scan_kernel() and
last_search_info()'s grid / query_panel / db_splits equal the first chunk's row of tests/golden/knn_bf16_plan.txt (recorded from the
parent commit's logic: tests/test_knn_bf16_plan_host.py), and the results equal the exact fp32 scan's bit for bit.  Every kernel,
both panel widths, a split with merge and a multi-chunk launch; all shapes have fewer panels than any device has CUs, so the rows
do not depend on the device."""
import numpy as np
import pytest

from tests.synth import unit_rows
from tests.test_gpu_parity import _assert_knn_equal, cu
from tests.test_knn_bf16_plan_host import planned

pytestmark = pytest.mark.gpu
F32, BF16 = 1, 2

# knob, nq, n, d, wide, the kernel expected for (ip, l2) -- written down here, the geometry comes from the table
CASES = [
    ("defaults", 300, 2049, 768, False, ("qs", "qs")),
    ("QS2_MIN_PANELS=0", 300, 2049, 768, False, ("qs4", "qs2")),
    ("defaults", 64, 5000, 512, False, ("qs", "qs")),
    ("QS2_MIN_PANELS=0", 64, 5000, 512, False, ("qs4", "qs4")),
    ("defaults", 1100, 3000, 100, False, ("qs", "qs")),                     # one-block kernel, pitch 256
    ("defaults", 150, 3000, 1000, False, ("scan_bf16", "scan_bf16")),       # streaming
    ("QS2_MIN_PANELS=0", 150, 3000, 1000, True, ("qsw", "qsw")),            # pitch 1024
    ("CHUNK_MB=0.01", 300, 3000, 768, False, ("qs", "qs")),                 # 3 database splits: one launch, chunks need splits == 1
    ("CHUNK_MB=0.01", 300, 1900, 768, False, ("qs", "qs")),                 # 15 tiles, too few to split: launches of 8 and 7, state carried
]


def test_the_cases_cover_a_split_with_merge_a_chunked_launch_and_both_panel_widths():
    rows = [planned(knob, d, wide, l2, n, nq)[0] for knob, nq, n, d, wide, _ in CASES for l2 in (0, 1)]
    assert {r["kernel"] for r in rows} == {"scan_bf16", "qs", "qs2", "qs4", "qsw"}
    assert {r["query_panel"] for r in rows} == {128, 256}
    assert any(r["splits"] > 1 for r in rows) and any(r["splits"] == 1 and r["chunk_tiles"] < r["n_tiles"] for r in rows)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("knob,nq,n,d,wide,kernels", CASES)
def test_the_launch_is_the_planned_one(hip, monkeypatch, metric, knob, nq, n, d, wide, kernels):
    if knob != "defaults":
        name, value = knob.split("=")
        monkeypatch.setenv("LEMON_" + name, value)
    rows = planned(knob, d, wide, metric == "l2", n, nq)
    assert len(rows) == 1 and rows[0]["kernel"] == kernels[metric == "l2"]
    row = rows[0]
    rng = np.random.default_rng(nq * 7 + n * 3 + d)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    if metric == "l2":
        X *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        Q *= rng.uniform(0.5, 2.0, (nq, 1)).astype(np.float32)
    out = {}
    for algo in (F32, BF16):
        idx = (hip.IndexFlatIP if metric == "ip" else hip.IndexFlatL2)(d)
        idx.set_algo(algo)
        idx.set_wide_filter(wide)
        idx.add(cu(X))
        D, I = idx.search(cu(Q), 10)
        out[algo] = (D.cpu().numpy(), I.cpu().numpy())
    info = idx.last_search_info()
    assert info["algo"] == BF16 and idx.last_scan_kernel() == row["kernel"]
    assert info["grid"] == row["panels"] * row["splits"]
    assert info["query_panel"] == row["query_panel"] and info["db_splits"] == row["splits"]
    _assert_knn_equal(out[BF16], out[F32])
