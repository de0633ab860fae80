"""CPU: the shapes of tests/test_gpu_index_state.py really do to a reused index handle what that file claims -- the fp32
sequence walks through more plans than the handle has slots and lays differently sized merge grids over one workspace, the 16-bit
sequences carry scan state across chunked launches, split the database and use both panel widths.  Checked with the host-only
lemon_debug_scan_plan and the recorded plan rows of tests/golden/knn_bf16_plan.txt; no device is touched.  The data makers'
outranking property (the dirtying call beats the checked call) is checked here against the CPU oracle, so that a GPU run does not
find it out."""
import numpy as np
import pytest

from tests import indexfx as fx

PLAN_SLOTS = 4          # lemon_index::plan_slots


def test_fp32_sequence_evicts_and_reloads_plans_and_relays_the_merge_grid():
    steps = fx.f32_steps()
    assert len(steps) == len(fx.F32_SEQUENCE) - 1 and fx.F32_SEQUENCE.count((0, 3)) == 1      # one empty call, skipped by the plan
    assert fx.F32_SEQUENCE[-1] == fx.F32_SEQUENCE[0]
    # only pairs of at least 2 units are planned and cached (lemon_search_f32_pass); the dirtying call has its checked call's pair
    keys = [(s["panels"], s["n_tiles"]) for s in steps if s["panels"] * s["n_tiles"] >= 2]
    assert len(keys) == len(steps)
    assert len(set(keys)) >= 6
    between = set(keys[1:-1]) - {keys[0]}
    assert keys[-1] == keys[0] and keys[0] not in keys[1:-1] and len(between) >= PLAN_SLOTS       # slot evicted, plan uploaded again
    assert any(s["splits"] > 1 for s in steps) and any(s["splits"] == 1 for s in steps)
    ragged = [s for s in steps if s["splits"] > 1 and len(set(s["pieces"].tolist())) > 1]
    assert ragged, "no plan whose panels are scanned in different numbers of pieces"
    assert all(int(s["pieces"].max()) == s["splits"] for s in steps)
    grid = [s["nq_pad"] * s["splits"] * s["kk"] for s in steps]
    assert any(a > b for a, b in zip(grid, grid[1:]))
    # the dirtying call (k = MAX_K) lays a grid at least as large as its checked call's, and a different one wherever k differs
    assert all(s["kk"] <= fx.MAX_K for s in steps)


def test_fp32_sequence_has_the_edges_it_names():
    nqs = [nq for nq, _ in fx.F32_SEQUENCE]
    assert 0 in nqs and 1 in nqs and any(nq % fx.ROWS == 1 for nq in nqs if nq > fx.ROWS) and max(nqs) > 65536
    ks = [k for _, k in fx.F32_SEQUENCE]
    assert 1 in ks and fx.MAX_K in ks
    assert fx.F32_N % fx.ROWS == 0 and fx.F32_D % 4 == 0


@pytest.mark.parametrize("l2", [False, True])
def test_bf16_sequences_chunk_split_and_use_both_panel_widths(l2):
    stationary, streaming, toggled = (fx.bf16_steps(h, l2) for h in fx.BF16_HANDLES)
    assert all(r["kernel"] in ("qs", "qs2", "qs4") for r in stationary)
    assert any(r["splits"] == 1 and r["chunk_tiles"] < r["n_tiles"] and r["state_elems"] > 0 for r in stationary)
    assert any(r["splits"] > 1 for r in stationary)
    assert {r["query_panel"] for r in stationary} == {128, 256}
    # the chunked launch is followed by a smaller one (fewer queries, smaller k) and by another kernel form over the same state
    chunked = [i for i, r in enumerate(stationary) if r["splits"] == 1 and r["chunk_tiles"] < r["n_tiles"]]
    first = chunked[0]
    nxt = stationary[first + 1]
    assert nxt["nq"] < stationary[first]["nq"] and nxt["k"] < stationary[first]["k"] and nxt["n"] == stationary[first]["n"]
    assert any(r["chunk_tiles"] >= r["n_tiles"] and r["n"] == stationary[first]["n"] for r in stationary[first + 1:])
    assert len({r["state_elems"] + r["cnt_elems"] for r in stationary}) >= 3                    # ws_state is re-laid, not just reused
    assert all(r["kernel"] == "scan_bf16" for r in streaming) and any(r["splits"] > 1 for r in streaming)
    assert len({r["nq"] for r in streaming}) >= 2
    assert [(r["kernel"], r["wide"]) for r in toggled] == [("scan_bf16", False), ("qsw", True), ("scan_bf16", False)]


def test_chunked_fp32_call_has_a_large_and_a_small_chunk():
    (nq, k), (nq2, _) = fx.CHUNKED_SEQUENCE
    qchunk = 1 << 19                                                      # QCHUNK of knn_f32.hip
    assert qchunk < nq < 2 * qchunk and 0 < (nq - qchunk) % fx.ROWS and nq2 < qchunk
    tiles = -(-fx.CHUNKED_N // fx.ROWS)
    big, rest = fx.scan_plan(qchunk // fx.ROWS, tiles), fx.scan_plan(-(-(nq - qchunk) // fx.ROWS), tiles)
    assert big["splits"] == 1 and rest["splits"] > 1                      # the second chunk merges pieces, the first does not


def test_the_scan_plan_reads_its_knobs_per_call(monkeypatch):
    """the shapes of the two per-call knob tests: 3 x 24 units in 9 workgroups; 2 x 16 units in 3 pieces per panel, 2 at segment
    cost 0 and 3 again without it, in one process"""
    for knob in ("LEMON_XCDS", "LEMON_SEG_COST"):
        monkeypatch.delenv(knob, raising=False)
    assert fx.scan_plan(3, 24)["grid"] == 9
    splits = []
    for cost in (None, "0", None):
        if cost is not None:
            monkeypatch.setenv("LEMON_SEG_COST", cost)
        splits.append(fx.scan_plan(2, 16)["splits"])
        monkeypatch.delenv("LEMON_SEG_COST", raising=False)
    assert splits == [3, 2, 3]


def test_switch_sequence_alternates_and_moves_nq_both_ways():
    algos = [a for a, _, _ in fx.SWITCH_SEQUENCE]
    assert all(a != b for a, b in zip(algos, algos[1:])) and algos.count(fx.F32) >= 2 and algos.count(fx.BF16) >= 2
    nqs = [nq for _, nq, _ in fx.SWITCH_SEQUENCE]
    steps = [b - a for a, b in zip(nqs, nqs[1:])]
    assert any(s > 0 for s in steps) and any(s < 0 for s in steps)
    assert fx.SWITCH_D * 4 == 3072 and fx.SWITCH_D * 2 == 1536            # the two row sizes ws_qp is shared between
    # a split fp32 call (th_pub in use) in front of a 16-bit one
    f32 = fx.f32_steps([(nq, k) for a, nq, k in fx.SWITCH_SEQUENCE if a == fx.F32], fx.SWITCH_N)
    assert any(s["splits"] > 1 for s in f32)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,d,nq", [(fx.F32_N, fx.F32_D, 700), (1900, 768, 300), (90, 48, 37), (300, 32, 200)])
def test_the_dirtying_queries_outrank_the_checked_ones(oracle, metric, n, d, nq):
    """what assert_outranked asks on the GPU, here with the oracle: the data makers deliver it with room to spare"""
    rng = np.random.default_rng(n + d)
    X = fx.make_db(rng, n, d, metric)
    Q = fx.make_queries(rng, nq, d, metric)
    Qd = fx.dirty_queries(X, Q, metric)
    assert Qd.shape == Q.shape and Qd.dtype == np.float32
    Dd, _ = oracle.knn(metric, X, Qd, fx.MAX_K)
    Dc, _ = oracle.knn(metric, X, Q, 1)
    last, best = Dd[:, min(fx.MAX_K, n) - 1], Dc[:, 0]
    if fx.is_l2(metric):
        assert (last * 4 < best).all(), (last.max(), best.min())
        assert not (Dc[:, 0] == 0).any()                                 # no checked query is a database row
    else:
        assert (last > 1.25 * best).all() and (best > 0).all(), (last.min(), best.max())


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_add_cycle_rows_reach_the_lists_and_stay_outranked(oracle, metric):
    """the add life cycle: the second and third adds stay within / exceed the capacity as claimed, their rows have four times the
    norm of the others, reach the k best of at least ADD_MIN_HITS queries of every later call, and the dirtying call still wins"""
    assert fx.ADD_STEPS[0] + fx.ADD_STEPS[1] == -(-fx.ADD_STEPS[0] // fx.ROWS) * fx.ROWS          # 1900 + 20 fills the capacity
    rng = np.random.default_rng(7)
    X = np.zeros((0, fx.ADD_D), np.float32)
    big = []
    for i, (rows, Q) in enumerate(fx.add_cycle(rng, metric)):
        assert rows.shape == (fx.ADD_STEPS[i], fx.ADD_D) and Q.shape == (fx.ADD_NQ, fx.ADD_D)
        if i in fx.ADD_BIG_STEPS:
            big += list(range(len(X), len(X) + len(rows)))
            norms = np.linalg.norm(rows, axis=1)
            others = np.delete(np.linalg.norm(X, axis=1), [b for b in big if b < len(X)])
            assert (np.abs(norms - 4.0) < 1e-3).all() and others.max() <= 1.26
        X = np.concatenate([X, rows])
        Dc, Ic = oracle.knn(metric, X, Q, fx.ADD_K)
        Dd, _ = oracle.knn(metric, X, fx.dirty_queries(X, Q, metric), fx.MAX_K)
        ok = Dd[:, -1] < Dc[:, 0] if fx.is_l2(metric) else Dd[:, -1] > Dc[:, 0]
        assert ok.all(), (i, int((~ok).sum()))
        if big:
            assert np.isin(Ic, big).any(axis=1).sum() >= fx.ADD_MIN_HITS, i


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", [32, 64])
def test_lemon_db_splits_keep_the_image_side_outranked(oracle, metric, d):
    """the very data of test_lemon_db_across_splits: every image-side dirtying result beats the split's best, a train query's own
    row included where the split has such queries"""
    for data in fx.lemon_db_case(d, metric):
        ndb = data["img"].shape[0]
        assert fx.n_distinct(data["txt"]) <= fx.DB_CLASSES + fx.L2_BLOB
        for name in ("train", "val"):
            s = data[name]
            assert 0 < s["in_db"].sum() < len(s["in_db"]) if name == "train" and ndb > fx.L2_BLOB else not s["in_db"].any()
            Dd, _ = oracle.knn(metric, data["img"], fx.dirty_queries(data["img"], s["q_img"], metric), min(fx.MAX_K, ndb))
            Dc, _ = oracle.knn(metric, data["img"], s["q_img"], 2)
            best = np.where(s["in_db"] == 1, Dc[:, 1], Dc[:, 0])          # a train query's own row is dropped from its record
            if fx.is_l2(metric):
                assert (Dd[:, -1] * 2 < best).all()
            else:
                best = np.where(s["in_db"] == 1, np.maximum(best, 1.0 + 1e-3), best)       # (also beyond the self match <q, q> = 1)
                assert (Dd[:, -1] > 1.25 * best).all(), (Dd[:, -1] / best).min()


def test_sample_rows_and_repeated_rows():
    assert fx.sample_rows(0).size == 0 and fx.sample_rows(1).tolist() == [0]
    r = fx.sample_rows(66000)
    assert len(r) == fx.ORACLE_SAMPLE and r[0] == 0 and r[-1] == 65999 and (np.diff(r) > 0).all()
    assert fx.sample_rows(5).tolist() == [0, 1, 2, 3, 4]
    rng = np.random.default_rng(0)
    Q = fx.repeated(rng, fx.make_queries(rng, 100, 16, "cosine"), 4096)
    assert Q.shape == (4096, 16) and fx.n_distinct(Q) == 100
