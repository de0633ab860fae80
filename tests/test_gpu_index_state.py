"""GPU: what an index handle keeps from one call to the next -- the grow-only workspaces (ws_qp, ws_qnorm, ws_cand, ws_part), the
four plan slots, the 16-bit copy and its statistics, the carried scan state, the de-duplication, deep-k, neighbour and discrepancy
workspaces -- and the stream argument of every entry point.

Every checked call on a reused handle comes right behind a DIRTYING call on that handle (same nq, k = LEMON_MAX_K) whose every
result outranks the checked call's best (tests/indexfx.py says how; each test asserts it from the two results), so that anything
a workspace leaks would win the merge.  The checked result must equal, bit for bit, the same call on a fresh handle and the CPU
oracle.  tests/test_index_state_host.py shows on the CPU that the shapes used here evict plans, re-lay the merge grid, chunk, split
and switch panel widths."""
import numpy as np
import pytest
import torch

from tests import indexfx as fx
from tests.indexfx import BF16, F32, MAX_K, bits_equal, checked_search, cu, new_index

pytestmark = pytest.mark.gpu
METRICS = ["cosine", "euclidean"]
KNOBS = ("LEMON_QS2_MIN_PANELS", "LEMON_CHUNK_MB")
REC_KEYS = ("d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m", "I_n", "I_m")      # lemon_amd.neighbors.REC_KEYS


def set_knob(monkeypatch, knob):
    """one knob of the 16-bit plan for the calls that follow (read per call), the other at its default"""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if knob != "defaults":
        name, value = knob.split("=")
        monkeypatch.setenv("LEMON_" + name, value)


def key_of(info, *fields):
    return tuple(info[f] for f in fields)


# ---- 1. fp32 scan: one handle, a sequence of shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_fp32_scan_sequence_on_one_handle(hip, oracle, metric):
    rng = np.random.default_rng(11)
    d, n = fx.F32_D, fx.F32_N
    X = fx.make_db(rng, n, d, metric)
    reused = new_index(hip, metric, d, F32, X)
    plans = iter(fx.f32_steps())
    same_cus = torch.cuda.get_device_properties(0).multi_processor_count == 256      # what the host-side plan assumes
    first_q, results = None, []
    for nq, k in fx.F32_SEQUENCE:
        if nq == 0:                                         # an empty call between two real ones: nothing written, nothing broken
            D, I = reused.search(torch.empty((0, d), device="cuda"), k)
            assert D.shape == (0, k) and I.shape == (0, k)
            continue
        plan = next(plans)
        Q = first_q if (nq, k) == fx.F32_SEQUENCE[0] and first_q is not None else fx.make_queries(rng, nq, d, metric)
        first_q = Q if first_q is None else first_q
        D, I = checked_search(reused, new_index(hip, metric, d, F32, X), X, Q, k, metric, oracle)
        info = reused.last_search_info()
        assert reused.last_scan_kernel() == "scan_f32" and key_of(info, "algo", "nq", "n", "d", "k") == (F32, nq, n, d, k)
        if same_cus:
            assert key_of(info, "grid", "db_splits") == (plan["grid"], plan["splits"])
        results.append((D, I))
    assert bits_equal(results[0][0], results[-1][0]) and bits_equal(results[0][1], results[-1][1])


@pytest.mark.parametrize("metric", METRICS)
def test_fp32_call_of_two_query_chunks_then_a_small_one(hip, oracle, metric):
    """more than 2^19 queries run as two chunks over one workspace: 4096 panels without a merge, then 2 panels with one"""
    rng = np.random.default_rng(13)
    d, n = fx.CHUNKED_D, fx.CHUNKED_N
    X = fx.make_db(rng, n, d, metric)
    reused = new_index(hip, metric, d, F32, X)
    for nq, k in fx.CHUNKED_SEQUENCE:
        Q = fx.make_queries(rng, nq, d, metric)
        checked_search(reused, new_index(hip, metric, d, F32, X), X, Q, k, metric, oracle)
        assert key_of(reused.last_search_info(), "algo", "nq", "n", "k") == (F32, nq, n, k)


# ---- 2. 16-bit scan: one handle per kernel family, knobs changed between calls ------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("which", [0, 1, 2], ids=["stationary_d768", "streaming_d1000", "wide_toggled_d1000"])
def test_bf16_scan_sequence_on_one_handle(hip, oracle, monkeypatch, metric, which):
    handle = fx.BF16_HANDLES[which]
    d = handle["d"]
    rows = iter(fx.bf16_steps(handle, fx.is_l2(metric)))
    rng = np.random.default_rng(23 + which)
    wide = handle["wide"]
    reused = new_index(hip, metric, d, BF16, wide=wide)
    X = np.zeros((0, d), np.float32)
    for step in handle["steps"]:
        if step[0] == "wide":
            wide = step[1]
            reused.set_wide_filter(wide)
            continue
        if step[0] == "add":
            more = fx.make_db(rng, step[1], d, metric) if not len(X) else fx.more_rows(rng, step[1], d, metric)
            reused.add(cu(more))
            X = np.concatenate([X, more])
            assert reused.ntotal == len(X)
            continue
        _, knob, nq, k = step
        row = next(rows)
        set_knob(monkeypatch, knob)
        Q = fx.make_queries(rng, nq, d, metric)

        def planned_launch(ix):
            info = ix.last_search_info()
            assert ix.last_scan_kernel() == row["kernel"] and info["algo"] == BF16
            assert key_of(info, "grid", "query_panel", "db_splits") == (row["panels"] * row["splits"], row["query_panel"], row["splits"])

        checked_search(reused, new_index(hip, metric, d, BF16, X, wide=wide), X, Q, k, metric, oracle, after_dirty=planned_launch)
        planned_launch(reused)
        assert key_of(reused.last_search_info(), "nq", "n", "k") == (nq, len(X), k)


# ---- 2b. fp32 scan: its knobs are read per call, and a plan slot belongs to the knobs it was made under ------------------------
F32_KNOBS = ("LEMON_SPLITS", "LEMON_XCDS", "LEMON_SEG_COST", "LEMON_SHARE_BOUNDS", "LEMON_STALE", "LEMON_FAIR")


def _plain_knob_plain(hip, oracle, monkeypatch, metric, n, nq, name, value):
    """search(Q, 10) at d = 64 on one handle three times -- no knob set, LEMON_<name> = value, no knob set -- each held against
    the oracle bit for bit (every query: nq <= ORACLE_SAMPLE); -> [(grid, db_splits)] of the three searches, and of the plans
    lemon_debug_scan_plan gives under the same three settings"""
    rng = np.random.default_rng(29)
    d, k = 64, 10
    X, Q = fx.make_db(rng, n, d, metric), fx.make_queries(rng, nq, d, metric)
    assert nq <= fx.ORACLE_SAMPLE
    ix = new_index(hip, metric, d, F32, X)
    for knob in F32_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    panels, tiles = -(-nq // fx.ROWS), -(-n // fx.ROWS)
    seen, plans = [], []
    for setting in (None, value, None):
        if setting is not None:
            monkeypatch.setenv(name, setting)
        plan = fx.scan_plan(panels, tiles)
        plans.append((plan["grid"], plan["splits"]))
        D, I = ix.search(cu(Q), k)
        monkeypatch.delenv(name, raising=False)
        assert ix.last_scan_kernel() == "scan_f32"
        fx.assert_equals_oracle(oracle, metric, X, Q, k, D, I)
        seen.append(key_of(ix.last_search_info(), "grid", "db_splits"))
    return seen, plans


@pytest.mark.parametrize("metric", METRICS)
def test_fp32_scan_reads_lemon_splits_per_call(hip, oracle, monkeypatch, metric):
    """3 panels x 24 tiles: planned, then 3 panels x 2 forced splits, then planned again -- whatever the process ran before"""
    seen, plans = _plain_knob_plain(hip, oracle, monkeypatch, metric, 3000, 300, "LEMON_SPLITS", "2")
    assert seen[1] == (6, 2)
    assert seen[0] == seen[2] == plans[0] == plans[2] != seen[1]


@pytest.mark.parametrize("metric", METRICS)
def test_fp32_plan_slot_is_not_reused_under_another_segment_cost(hip, oracle, monkeypatch, metric):
    """2 panels x 16 tiles in 4 workgroups (on any device of at least 2 CUs): 3 pieces per panel by default, 2 at cost 0;
    a slot keyed on (panels, tiles) alone would serve the first plan to all three calls"""
    seen, plans = _plain_knob_plain(hip, oracle, monkeypatch, metric, 2048, 256, "LEMON_SEG_COST", "0")
    assert plans[0] == plans[2] and plans[0][1] != plans[1][1]
    assert seen == plans


# ---- 3. switching algorithms on one handle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_switching_algorithms_on_one_handle(hip, oracle, metric):
    """ws_qp holds 3072-byte rows for one scan and 1536-byte rows for the other; ws_qnorm's tail is th_pub for one and
    qres2 / qhn2 for the other"""
    rng = np.random.default_rng(31)
    d, n = fx.SWITCH_D, fx.SWITCH_N
    X = fx.make_db(rng, n, d, metric)
    reused = new_index(hip, metric, d, F32, X)
    for algo, nq, k in fx.SWITCH_SEQUENCE:
        reused.set_algo(algo)
        Q = fx.make_queries(rng, nq, d, metric)
        checked_search(reused, new_index(hip, metric, d, algo, X), X, Q, k, metric, oracle)
        assert reused.last_search_info()["algo"] == algo
        assert (reused.last_scan_kernel() == "scan_f32") == (algo == F32)


# ---- 4. add life cycle with searches in between -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("algo", [F32, BF16], ids=["f32", "bf16"])
def test_add_life_cycle_with_searches_in_between(hip, oracle, metric, algo):
    """add within the capacity (the 16-bit copy converts the new rows only and recomputes its maxima), add beyond it (the copy is
    dropped and rebuilt), add again; the rows of the second and third add have four times the norm of the others, so a stale
    maximum would make the filter's band too narrow exactly where they matter"""
    rng = np.random.default_rng(7)
    d, k = fx.ADD_D, fx.ADD_K
    reused = new_index(hip, metric, d, algo)
    X = np.zeros((0, d), np.float32)
    big = []
    for i, (rows, Q) in enumerate(fx.add_cycle(rng, metric)):
        if i in fx.ADD_BIG_STEPS:
            big += list(range(len(X), len(X) + len(rows)))
        reused.add(cu(rows))
        X = np.concatenate([X, rows])
        assert reused.ntotal == len(X)
        assert bits_equal(reused.data(), cu(X)) and bits_equal(reused.reconstruct_n(len(X) - len(rows), len(rows)), cu(rows))
        D, I = checked_search(reused, new_index(hip, metric, d, algo, X), X, Q, k, metric, oracle)
        assert reused.last_search_info()["algo"] == algo and reused.last_search_info()["n"] == len(X)
        if big:     # (I equals the oracle's on every query: ADD_NQ <= ORACLE_SAMPLE)
            hits = int(torch.isin(I, cu(np.array(big))).any(dim=1).sum())
            assert Q.shape[0] <= fx.ORACLE_SAMPLE and hits >= fx.ADD_MIN_HITS, hits


# ---- 5. de-duplication on one handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("algo", [F32, BF16], ids=["f32", "bf16"])
def test_query_dedup_sequence_on_one_handle(hip, oracle, metric, algo):
    rng = np.random.default_rng(43)
    d, n = 96, 3000
    X = fx.make_db(rng, n, d, metric)
    X[2001::7] = X[2000]                                                    # duplicate rows too: ties go to the lower index
    reused = new_index(hip, metric, d, algo, X)                              # de-duplication is on by default
    calls = [(4096, 100, 11), (1500, 1500, 11), (2048, 900, 51), (1024, 1, 3)]
    queries = [fx.repeated(rng, fx.make_queries(rng, C, d, metric), nq) for nq, C, _ in calls]
    dedup = [True]

    def folded(Q):
        """nq_distinct of a search of Q under the handle's current setting (as test_gpu_dedup.py states it)"""
        nq, u = Q.shape[0], fx.n_distinct(Q)
        return u if dedup[0] and nq >= 1024 and 2 * u <= nq else nq

    def run(Q, k):
        Qd = fx.dirty_queries(X, Q, metric)
        fresh = new_index(hip, metric, d, algo, X, dedup=False)

        def dirtying_call_folded_too(ix):
            assert key_of(ix.last_search_info(), "nq", "nq_distinct", "k") == (Q.shape[0], folded(Qd), MAX_K)

        checked_search(reused, fresh, X, Q, k, metric, oracle, after_dirty=dirtying_call_folded_too)
        assert key_of(reused.last_search_info(), "nq", "nq_distinct", "k") == (Q.shape[0], folded(Q), k)
        assert key_of(fresh.last_search_info(), "nq", "nq_distinct", "k") == (Q.shape[0], Q.shape[0], k)

    for Q, (nq, C, k) in zip(queries, calls):
        assert fx.n_distinct(Q) == C
        run(Q, k)
    reused.set_query_dedup(False)
    dedup[0] = False
    run(queries[0], calls[0][2])
    reused.set_query_dedup(True)                                            # and back: the next call folds again
    dedup[0] = True
    run(queries[2], calls[2][2])


# ---- 6. deep and shallow lists on one handle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [700, 90])
def test_deep_and_shallow_lists_on_one_handle(hip, oracle, metric, n):
    """k = 200, 5, 65, 64, 130 on one handle: the key-bounded passes (ub, k_place_pass) between plain searches.  n = 700 holds 140
    exact duplicates, a tie group that straddles the 64 / 128 pass boundaries; with n = 90 every deep list ends in padding."""
    rng = np.random.default_rng(53)
    d, nq = 48, 37
    X = fx.make_db(rng, n, d, metric)
    Q = fx.make_queries(rng, nq, d, metric)
    if n >= 240:
        X[100] *= np.float32(1.25) / np.linalg.norm(X[100])
        X[100:240] = X[100]
        q0 = X[100] + 0.2 * rng.standard_normal(d).astype(np.float32) / np.float32(np.sqrt(d))
        Q[0] = q0 if fx.is_l2(metric) else q0 / np.linalg.norm(q0)      # near the group, not on it: the group leads its list
    reused = new_index(hip, metric, d, F32, X)
    got = {}
    for k in (200, 5, 65, 64, 130):
        D, I = checked_search(reused, new_index(hip, metric, d, F32, X), X, Q, k, metric, oracle)
        assert reused.last_search_info()["k"] == k
        got[k] = (D, I)
        if k > n:
            pad = float(np.finfo(np.float32).max) * (1.0 if fx.is_l2(metric) else -1.0)
            assert bool((I[:, n:] == -1).all()) and bool((D[:, n:] == pad).all()) and bool((I[:, :n] >= 0).all())
    if n >= 240:
        top = got[200][1][0]
        assert set(top[:140].tolist()) == set(range(100, 240)) and top[:140].tolist() == sorted(top[:140].tolist())
    for deep, shallow in ((200, 130), (130, 65), (65, 64), (64, 5)):
        assert bits_equal(got[deep][0][:, :shallow].contiguous(), got[shallow][0])
        assert bits_equal(got[deep][1][:, :shallow].contiguous(), got[shallow][1])


# ---- 7. LemonDB across splits -------------------------------------------------------------------------------------------------
def _neighbors(db, s, k, drop_self, discrete):
    return db.neighbors(cu(s["q_img"]), cu(s["q_txt"]), k, drop_self=drop_self, in_db=s["in_db"] if drop_self else None,
                        discrete=discrete, q_label_id=s["q_lab"] if discrete else None)


def _dirty_db(db, data, s, metric):
    """the dirtying call of a LemonDB: image and text queries that outrank the split's, k = MAX_K, plain record"""
    return db.neighbors(cu(fx.dirty_queries(data["img"], s["q_img"], metric)), cu(fx.dirty_queries(data["txt"], s["q_txt"], metric)), MAX_K)


def _checked_record(hip, oracle, reused, data, s, k, drop_self, discrete, metric, algo):
    dirty = _dirty_db(reused, data, s, metric)
    rec = _neighbors(reused, s, k, drop_self, discrete)
    # the image side is outranked (D_n is -<q, x> or the squared distance, smaller is better; the discrete cosine record keeps +<q, x>).
    # A train query's own row is no part of its record: the record's best is what the dirtying results are held against.  For the
    # cosine metric they beat that self match (<q, q> = 1) too; at distance 0 (euclidean) nothing can.
    n_db = data["img"].shape[0]
    last = dirty["D_n"][:, min(MAX_K, n_db) - 1]
    best = rec["D_n"][:, 0] * (-1.0 if discrete and not fx.is_l2(metric) else 1.0)
    assert bool((last < best).all())
    if drop_self and s["in_db"].any() and not fx.is_l2(metric):
        assert bool((last < -1.001).all())
    fresh = hip.LemonDB(cu(data["img"]), cu(data["txt"]), metric, tr_label_id=data["lab"], algo=algo)
    want = _neighbors(fresh, s, k, drop_self, discrete)
    for key in REC_KEYS:
        assert bits_equal(rec[key], want[key]), key
    rows = fx.sample_rows(s["q_img"].shape[0])
    ref = oracle.neighbors(metric, data["img"], data["txt"], s["q_img"][rows], s["q_txt"][rows], k, drop_self=drop_self,
                           in_db=s["in_db"][rows] if drop_self else None, discrete=discrete, tr_label_id=data["lab"],
                           q_label_id=s["q_lab"][rows])
    rt = cu(rows)
    for key in REC_KEYS:
        assert np.array_equal(rec[key][rt].cpu().numpy(), ref[key], equal_nan=True), key
    return rec


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete"])
@pytest.mark.parametrize("algo", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [32, 64])
def test_lemon_db_across_splits(hip, oracle, metric, discrete, algo, d):
    data, small = fx.lemon_db_case(d, metric)
    reused = hip.LemonDB(cu(data["img"]), cu(data["txt"]), metric, tr_label_id=data["lab"], algo=algo)
    train, val = data["train"], data["val"]
    args = (hip, oracle, reused, data)
    first = _checked_record(*args, train, fx.DB_K, True, discrete, metric, algo)
    _checked_record(*args, val, fx.DB_K, False, discrete, metric, algo)
    _checked_record(*args, val, 1, False, discrete, metric, algo)
    again = _checked_record(*args, train, fx.DB_K, True, discrete, metric, algo)
    for key in REC_KEYS:
        assert bits_equal(first[key], again[key]), key
    # a database smaller than k: -1 / NaN tails, behind a dirtying call whose own tail is padding
    reused_small = hip.LemonDB(cu(small["img"]), cu(small["txt"]), metric, tr_label_id=small["lab"], algo=algo)
    for s, drop_self in ((small["val"], False), (small["train"], True)):
        rec = _checked_record(hip, oracle, reused_small, small, s, fx.DB_K, drop_self, discrete, metric, algo)
        assert bool((rec["I_n"][:, fx.DB_SMALL_N:] == -1).all()) and bool(torch.isnan(rec["dists_n"][:, fx.DB_SMALL_N:]).all())
    if fx.is_l2(metric) or discrete:
        return
    # the discrepancy baselines on the text handle (cosine indices only): dis(train), div(val), dis(val)
    from lemon_amd.baselines import discrepancy_scores
    for method, s, is_train in (("dis_x", train, True), ("div_y", val, False), ("dis_y", val, False)):
        _dirty_db(reused, data, s, metric)
        got = discrepancy_scores(reused, cu(s["q_img"]), cu(s["q_txt"]), 10, method, is_train=is_train)
        fresh = hip.LemonDB(cu(data["img"]), cu(data["txt"]), metric, tr_label_id=data["lab"], algo=algo)
        assert bits_equal(got, discrepancy_scores(fresh, cu(s["q_img"]), cu(s["q_txt"]), 10, method, is_train=is_train)), method


# ---- 8. two handles interleaved -----------------------------------------------------------------------------------------------
def test_two_handles_interleaved(hip, oracle):
    """an IP handle at d = 40 and an L2 handle at d = 96, called alternately: each one's results are those it gives alone, and
    each one's last_* fields are its own"""
    rng = np.random.default_rng(71)
    spec = [dict(metric="cosine", d=40, n=2000, algo=F32), dict(metric="euclidean", d=96, n=1500, algo=BF16)]
    calls = [(300, 20), (70, 64), (1100, 5), (130, 33)]
    for h in spec:
        h["X"] = fx.make_db(rng, h["n"], h["d"], h["metric"])
        h["Q"] = [fx.make_queries(rng, nq, h["d"], h["metric"]) for nq, _ in calls]
        alone = new_index(hip, h["metric"], h["d"], h["algo"], h["X"])
        h["alone"] = []
        for Q, (_, k) in zip(h["Q"], calls):
            alone.search(cu(fx.dirty_queries(h["X"], Q, h["metric"])), MAX_K)
            h["alone"].append(alone.search(cu(Q), k))
        h["ix"] = new_index(hip, h["metric"], h["d"], h["algo"], h["X"])
    for i, (nq, k) in enumerate(calls):
        dirty = [h["ix"].search(cu(fx.dirty_queries(h["X"], h["Q"][i], h["metric"])), MAX_K)[0] for h in spec]
        for h in spec:      # (each handle's last call is still its own dirtying call, whatever the other one did since)
            assert key_of(h["ix"].last_search_info(), "algo", "nq", "n", "d", "k") == (h["algo"], nq, h["n"], h["d"], MAX_K)
        got = [h["ix"].search(cu(h["Q"][i]), k) for h in spec]
        for h, Dd, (D, I) in zip(spec, dirty, got):
            fx.assert_outranked(Dd, D, h["metric"], h["n"])
            assert key_of(h["ix"].last_search_info(), "algo", "nq", "n", "d", "k") == (h["algo"], nq, h["n"], h["d"], k)
            assert (h["ix"].last_scan_kernel() == "scan_f32") == (h["algo"] == F32)
            assert bits_equal(D, h["alone"][i][0]) and bits_equal(I, h["alone"][i][1])
            fx.assert_equals_oracle(oracle, h["metric"], h["X"], h["Q"][i], k, D, I)


# ---- 9. a side stream ---------------------------------------------------------------------------------------------------------
def _stream_workload(hip, seeds, metric):
    """queries made by kernels on the current stream, then -- with no synchronisation of this function's own -- add, an fp32
    search, a 16-bit search, a de-duplicated search, a k = 200 search, LemonDB.neighbors and lemon_grid_f1_ks, each search behind
    its dirtying call.  Every tensor is allocated here, under the caller's stream."""
    from lemon_amd.ops import grid_f1_ks
    d, n, nq = 64, 1500, 1200
    X, base, mix, axis, protos = (cu(seeds[key]) for key in ("X", "base", "mix", "axis", "protos"))
    Q = hip.normalize_vectors(axis[None, :] + 0.8 * (base @ mix))            # a matmul and a normalisation, on this stream
    cycled = lambda t, count, period: t[torch.arange(count, device="cuda") % period].contiguous()
    dirty = (lambda q: q * 4.0) if not fx.is_l2(metric) else (lambda q: cycled(X, q.shape[0], fx.L2_BLOB))     # as fx.dirty_queries
    out = {"Q": Q}
    ix = new_index(hip, metric, d, F32)
    ix.add(X)
    for name, algo, q, k in (("f32", F32, Q, 20), ("bf16", BF16, Q, 20), ("dedup", F32, cycled(Q, nq, 100), 11),
                             ("deep", F32, Q[:70].contiguous(), 200)):
        ix.set_algo(algo)
        out[name + "_dirty"] = ix.search(dirty(q), MAX_K)[0]
        out[name + "_D"], out[name + "_I"] = ix.search(q, k)
        out[name + "_distinct"] = ix.last_search_info()["nq_distinct"]
    txt, q_txt = cycled(protos, n, protos.shape[0]), cycled(protos, nq, protos.shape[0])
    db = hip.LemonDB(X, txt, metric)
    out["nb_dirty"] = db.neighbors(dirty(Q), q_txt * 4.0 if not fx.is_l2(metric) else txt[:nq].contiguous(), MAX_K)["D_n"]
    rec = db.neighbors(Q, q_txt, 20)
    out.update({"nb_" + key: v for key, v in rec.items()})
    y = np.arange(nq) % 3 == 0
    hps = [[5, 5, 0.1, 5, 0.1, 5], [1, 2, 0.5, 1, 0.5, 1]]
    out["f1"], out["thres"] = grid_f1_ks(rec, y, hps, [1, 5, 20])
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_every_entry_point_on_a_side_stream(hip, oracle, metric):
    rng = np.random.default_rng(83)
    d, n, nq = 64, 1500, 1200
    X = fx.make_db(rng, n, d, metric)
    base = fx.make_queries(rng, nq, 48, "euclidean")                          # unit rows; base @ mix has rows of norm ~1
    mix = (rng.standard_normal((48, d)) / np.sqrt(d)).astype(np.float32)
    axis = (fx.cone_axis(d) * (0.0 if fx.is_l2(metric) else 1.0)).astype(np.float32)      # cosine: queries inside the data's cone
    seeds = dict(X=X, base=base, mix=mix, axis=axis, protos=fx.make_queries(rng, 10, d, metric))
    want = _stream_workload(hip, seeds, metric)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _stream_workload(hip, seeds, metric)
    side.synchronize()
    assert bits_equal(got["Q"], want["Q"]), "the query-producing kernels themselves differ between the streams"
    for key, v in want.items():
        if torch.is_tensor(v):
            assert bits_equal(got[key], v), key
        elif isinstance(v, np.ndarray):
            assert np.array_equal(got[key].view(np.int64), v.view(np.int64)), key
        else:
            assert got[key] == v, key
    assert got["dedup_distinct"] == 100 and got["f32_distinct"] == nq
    # the dirtying calls did outrank, and the side-stream results are the oracle's
    Qn = got["Q"].cpu().numpy()
    for name, q, k in (("f32", Qn, 20), ("bf16", Qn, 20), ("dedup", Qn[np.arange(nq) % 100], 11), ("deep", Qn[:70], 200)):
        fx.assert_outranked(got[name + "_dirty"], got[name + "_D"], metric, n)
        fx.assert_equals_oracle(oracle, metric, X, q, k, got[name + "_D"], got[name + "_I"])
    assert bool((got["nb_dirty"][:, -1] < got["nb_D_n"][:, 0]).all())


# ---- 10. the two-sided search and the image handle's de-duplication setting ------------------------------------------------------
def _distinct(ix):
    return ix.last_search_info()["nq_distinct"]


@pytest.mark.parametrize("metric", METRICS)
def test_two_sided_search_leaves_the_image_handles_dedup_setting_alone(hip, oracle, metric):
    """LemonDB.neighbors and neighbors_metrics never fold the image side, and say so in the call: at nq = 1024 (the smallest
    count at which folding is attempted) with 4 distinct image and 8 distinct text queries the image handle searches all nq
    rows and the text handle 8, whatever the image handle's own setting is -- and that setting is the same after the call"""
    rng = np.random.default_rng(97)
    d, n, nq, k = 32, 512, 1024, 5
    data = dict(img=fx.make_db(rng, n, d, metric), txt=fx.make_db(rng, n, d, metric), lab=rng.integers(0, 10, n).astype(np.int32))
    s = dict(q_img=fx.repeated(rng, fx.make_queries(rng, 4, d, metric), nq), q_txt=fx.repeated(rng, fx.make_queries(rng, 8, d, metric), nq),
             q_lab=rng.integers(0, 10, nq).astype(np.int32), in_db=np.zeros(nq, np.uint8))
    assert (fx.n_distinct(s["q_img"]), fx.n_distinct(s["q_txt"])) == (4, 8)
    q_img, q_txt = cu(s["q_img"]), cu(s["q_txt"])
    want = new_index(hip, metric, d, F32, data["img"], dedup=False).search(q_img, k)

    def direct_search(db, folded):
        """the image queries on the image handle itself: folded or not as the handle's own setting says"""
        D, I = db.index_img.search(q_img, k)
        assert _distinct(db.index_img) == (4 if folded else nq)
        assert bits_equal(D, want[0]) and bits_equal(I, want[1])

    reused = hip.LemonDB(cu(data["img"]), cu(data["txt"]), metric, tr_label_id=data["lab"], algo=F32)
    for setting in (True, False):
        reused.index_img.set_query_dedup(setting)
        _checked_record(hip, oracle, reused, data, s, k, False, False, metric, F32)
        assert (_distinct(reused.index_img), _distinct(reused.index_txt)) == (nq, 8)
        direct_search(reused, setting)
    if fx.is_l2(metric):
        return
    sweep = hip.LemonDB(cu(data["img"]), cu(data["txt"]), ("cosine", "euclidean"), tr_label_id=data["lab"], algo=F32)
    fresh = hip.LemonDB(cu(data["img"]), cu(data["txt"]), ("cosine", "euclidean"), tr_label_id=data["lab"], algo=F32)
    recs_want, _ = fresh.neighbors_metrics(q_img, q_txt, k)
    for setting in (True, False):
        sweep.index_img.set_query_dedup(setting)
        _dirty_db(sweep, data, s, metric)
        recs, _ = sweep.neighbors_metrics(q_img, q_txt, k)
        assert (_distinct(sweep.index_img), _distinct(sweep.index_txt)) == (nq, 8)
        for name in ("cosine", "euclidean"):
            for key in REC_KEYS:
                assert bits_equal(recs[name][key], recs_want[name][key]), (name, key)
        direct_search(sweep, setting)
