"""CPU: the fixtures of tests/test_gpu_scan_f32_edges.py and of the dedup edge tests have the properties those tests rely on --
every geometry gives the plan its table row claims (lemon_debug_scan_plan, host only), the tie-heavy data really ties across
every piece, the ascending data really admits every row, the deep-k tie groups cross the boundaries they are meant to cross, the
planted non-finite rows score as stated under the fmaf chain, and the dedup inputs hold the numbers of distinct rows the GPU
tests expect.  No device is touched."""
import numpy as np
import pytest

from tests import indexfx as fx
from tests import scanfx as sx

METRICS = ["cosine", "euclidean"]


def _plan(monkeypatch, env, geometry):
    sx.apply_env(monkeypatch, env)
    return fx.scan_plan(*sx.shape_of(geometry))


@pytest.mark.parametrize("geometry,extra", [(g, {}) for g in sx.GEOMETRIES] + [("G3", {"LEMON_XCDS": "1"})])
def test_every_geometry_gives_the_plan_its_row_claims(monkeypatch, geometry, extra):
    g = sx.GEOMETRIES[geometry]
    pl = _plan(monkeypatch, sx.env_of(geometry, extra), geometry)
    per_wg = np.diff(pl["seg_begin"])
    assert (pl["grid"], pl["splits"]) == (g["grid"], g["splits"])
    assert (int(pl["pieces"].min()), int(pl["pieces"].max())) == g["pieces"]
    assert int(per_wg.max()) == g["max_segs"]
    assert bool((pl["segs"][:, 2] == 1).any()) == g["one_tile"]
    assert sx.expected_launch(*sx.shape_of(geometry)) == (g["grid"], g["splits"])


def test_the_table_rows_have_the_edges_they_name(monkeypatch):
    g1, g3 = sx.GEOMETRIES["G1"], sx.GEOMETRIES["G3"]
    assert g1["nq"] % sx.ROWS and g1["n"] % sx.ROWS                        # ragged last panel and last tile
    assert sx.shape_of("G1") == (2, 16) and sx.shape_of("G2") == (8, 5) and sx.shape_of("G3") == (65, 10)
    assert sx.shape_of("G4") == (9, 3) and sx.shape_of("G5") == (1, 2) and sx.shape_of("G6") == (3, 24) and sx.shape_of("G7") == (2, 12)
    assert sx.shape_of("G3")[0] >= 64 and g3["grid"] >= 64                 # XCD groups on: panels and grid >= 8 x 8
    # G4: every workgroup walks three WHOLE panels; G1: a segment of at least 6 tiles (the `full` trigger needs them)
    pl = _plan(monkeypatch, {}, "G4")
    assert (pl["segs"][:, 1] == 0).all() and (pl["segs"][:, 2] == 3).all() and np.diff(pl["seg_begin"]).tolist() == [3, 3, 3]
    assert int(_plan(monkeypatch, {}, "G1")["segs"][:, 2].max()) >= 6
    # LEMON_SPLITS on G1: 7 gives 6 splits of 3 tiles -- 6 x 64 keys are two trips of k_merge's 192 -- and the last split holds
    # the ragged tile; 0 is the automatic count
    assert sx.plan_splits(2, 16, 7) == (6, 3) and 192 < 6 * sx.MAX_K <= 2 * 192
    assert sx.plan_splits(2, 16, 1) == (1, 16) and sx.plan_splits(2, 16, 2) == (2, 8) and sx.plan_splits(2, 16, 0) == (2, 8)
    assert sx.plan_splits(3, 24, 2) == (2, 12)
    sx.apply_env(monkeypatch, {"LEMON_SPLITS": "7"})
    assert sx.expected_launch(2, 16) == (12, 6)
    last = [r for r in sx.piece_ranges(2, 16, g1["n"]) if r[1] == 5]
    assert all(r[3] == g1["n"] and (r[3] - r[2]) % sx.ROWS for r in last)
    # G2 under segment cost 10 has a workgroup WITHOUT a segment: the matrix runs that too
    pl = _plan(monkeypatch, {"LEMON_SEG_COST": "10"}, "G2")
    assert 0 in np.diff(pl["seg_begin"]).tolist()
    # the matrix: six knobs, the four the suite never held to the oracle among them
    named = {k for s in sx.SETTINGS for k in s}
    assert named == set(sx.KNOBS)
    fair = [int(s["LEMON_FAIR"]) for s in sx.SETTINGS if "LEMON_FAIR" in s]
    assert sorted(fair) == [0, 13, 18, 100, 101]                           # no value >= 32 but the two diagnostics


@pytest.mark.parametrize("geometry,extra", [("G1", {}), ("G1", {"LEMON_SEG_COST": "0"}), ("G1", {"LEMON_SPLITS": "7"}),
                                            ("G2", {}), ("G6", {}), ("G6", {"LEMON_SPLITS": "2"})])
def test_every_piece_holds_every_prototype(monkeypatch, geometry, extra):
    g = sx.GEOMETRIES[geometry]
    X, Q = sx.make("prototypes", g["nq"], g["n"], 64, "cosine")
    assert fx.n_distinct(X) == sx.N_PROTOS and fx.n_distinct(Q) == 2 * sx.N_PROTOS
    sx.apply_env(monkeypatch, sx.env_of(geometry, extra))
    ranges = sx.piece_ranges(*sx.shape_of(geometry), g["n"])
    assert len(ranges) >= 2 * sx.shape_of(geometry)[0] or geometry == "G2"
    for panel, piece, a, b in ranges:
        assert fx.n_distinct(X[a:b]) == sx.N_PROTOS, (panel, piece, a, b)
    for t0 in range(0, g["n"], sx.ROWS):                                   # and so does every tile (G3's last is a single row)
        assert fx.n_distinct(X[t0:t0 + sx.ROWS]) == min(sx.N_PROTOS, g["n"] - t0)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("geometry", ["G1", "G2", "G3", "G6"])
def test_prototype_top64_is_one_tie_group(oracle, metric, geometry):
    g = sx.GEOMETRIES[geometry]
    X, Q = sx.make("prototypes", g["nq"], g["n"], 64, metric)
    D, I = oracle.knn(metric, X, Q, sx.MAX_K)
    assert (D == D[:, :1]).all() and (I >= 0).all()                        # a single score value per query
    assert (np.diff(I, axis=1) > 0).all()
    # the winners are spread over more than one piece's worth of tiles only in index order: the whole group is larger than 64
    # and present in every tile (test_every_piece_holds_every_prototype), so any piece's bound, once warm, IS the tie score
    cls_pos = (Q @ fx.cone_axis(64)) > 0                                   # the prototypes themselves; the others are negations
    assert cls_pos.any() and (~cls_pos).any()
    if fx.is_l2(metric):
        assert (D[cls_pos] == 0).all()                                     # own prototype at distance exactly 0 (score -0.0)
        assert (D[~cls_pos] > 0).all()
    else:
        Dall, _ = oracle.knn(metric, X, Q[~cls_pos], 1)
        assert (Dall < 0).all()                                            # a whole query class has all-negative scores
        assert (D[cls_pos] > 0).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("geometry", ["G1", "G2", "G3", "G4", "G5"])
def test_ascending_rows_are_all_admitted(oracle, metric, geometry):
    """the oracle's running top-k changes at every row <=> every row beats all earlier ones, strictly"""
    g = sx.GEOMETRIES[geometry]
    X, Q = sx.make("ascending", g["nq"], g["n"], 64, metric)
    assert fx.n_distinct(Q) == 1 and Q.shape[0] == g["nq"]                 # the same query in every row of every panel
    D, I = oracle.knn(metric, X, Q[:1], g["n"])
    assert np.array_equal(I[0], np.arange(g["n"])[::-1])
    assert (np.diff(D[0]) > 0).all() if fx.is_l2(metric) else (np.diff(D[0]) < 0).all()


@pytest.mark.parametrize("geometry", ["G1", "G2", "G3"])
def test_around_zero_scores_straddle_zero_with_exact_zeros(oracle, monkeypatch, geometry):
    g = sx.GEOMETRIES[geometry]
    X, Q = sx.make("around_zero", g["nq"], g["n"], 64, "cosine")
    assert fx.n_distinct(Q) == 2 and np.array_equal(Q[0], -Q[1])
    D, I = oracle.knn("cosine", X, Q[:2], g["n"])
    t = sx.around_zero_t(g["n"])
    for row, sign in ((0, 1.0), (1, -1.0)):
        s = np.empty(g["n"], np.float32)
        s[I[row]] = D[row]
        assert np.array_equal(np.sign(s), np.sign(sign * t))               # sign and exact zero survive the chain
        assert (s.view(np.uint32)[t == 0] == 0).all()                      # +0.0, never -0.0: the chain starts from +0
        nz = np.abs(s[t != 0])
        assert nz.min() >= 5e-19 and nz.max() <= 2e-3                      # far from the subnormal range (1.2e-38)
        n_pos = int((s > 0).sum())
        assert 0 < n_pos < sx.MAX_K < n_pos + int((s == 0).sum())          # a top-64 list ends inside the zero tie group
        assert (D[row, n_pos:sx.MAX_K] == 0).all() and (np.diff(I[row, n_pos:sx.MAX_K]) > 0).all()
    # every piece holds zeros, positives or not: a piece's bound reaches 0 from below or sits at it
    sx.apply_env(monkeypatch, sx.env_of(geometry, {}))
    for panel, piece, a, b in sx.piece_ranges(*sx.shape_of(geometry), g["n"]):
        assert int((t[a:b] == 0).sum()) >= min(b - a, sx.MAX_K) // 2, (panel, piece)


def test_identical_rows_are_identical():
    g = sx.GEOMETRIES["G1"]
    for metric in METRICS:
        X, Q = sx.make("identical", g["nq"], g["n"], 64, metric)
        assert fx.n_distinct(X) == 1 and fx.n_distinct(Q) == g["nq"]


def test_data_sets_are_seeded_and_shaped():
    for name in sx.DATASETS:
        for metric in METRICS:
            (X, Q), (X2, Q2) = sx.make(name, 200, 1957, 64, metric), sx.make(name, 200, 1957, 64, metric)
            assert X.shape == (1957, 64) and Q.shape == (200, 64) and X.dtype == Q.dtype == np.float32
            assert np.array_equal(X, X2) and np.array_equal(Q, Q2) and X.flags.c_contiguous and Q.flags.c_contiguous
    for d in sx.WIDTHS:
        for name in ("random", "prototypes"):
            X, Q = sx.make(name, 200, 1957, d, "cosine")
            assert X.shape == (1957, d) and np.isfinite(X).all() and np.isfinite(Q).all()
    # L2 rows are rescaled into [0.5, 2] where the issue says so, and not where a property depends on the scale
    for name, lo, hi in (("random", 0.5, 2.0), ("prototypes", 1.0, 1.0), ("identical", 1.0, 1.0)):
        nrm = np.linalg.norm(sx.make(name, 200, 1957, 64, "euclidean")[0], axis=1)
        assert nrm.min() >= lo - 1e-3 and nrm.max() <= hi + 1e-3 and (name != "random" or nrm.max() - nrm.min() > 1.0)


def test_deep_tie_groups_cross_tile_piece_and_pass_boundaries(oracle, monkeypatch):
    g = sx.GEOMETRIES["G6"]
    X, Q = sx.deep_data()
    (a0, b0), (a1, b1) = sx.DEEP_TIES
    assert fx.n_distinct(X[a0:b0]) == 1 and fx.n_distinct(X[a1:b1]) == 1 and fx.n_distinct(X) == g["n"] - (b0 - a0) - (b1 - a1) + 2
    assert np.array_equal(Q[0], X[a0]) and np.array_equal(Q[1], X[a1])
    assert len({r // sx.ROWS for r in range(a0, b0)}) >= 3                 # tile boundaries
    # the first group fills query 0's best 300: it crosses the pass boundaries 64 / 128 / 192 / 256
    for metric in METRICS:
        D, I = oracle.knn(metric, X, Q[:2], max(sx.DEEP_KS))
        assert np.array_equal(I[0], np.arange(a0, a0 + 300)) and (D[0] == D[0, 0]).all()
        assert np.array_equal(I[1], np.arange(a1, a1 + 300)) and (D[1] == D[1, 0]).all()
    assert b0 - a0 >= 300 > 256
    # piece boundaries: the default plan's first (row 1152) and that of LEMON_SPLITS=2 (row 1536) lie inside the second group
    for env in ({}, {"LEMON_SPLITS": "2"}):
        sx.apply_env(monkeypatch, env)
        ends = sorted({r[3] for r in sx.piece_ranges(*sx.shape_of("G6"), g["n"]) if r[3] < g["n"]})
        assert a1 < ends[0] < b1, (env, ends)
        assert not a0 < ends[0] < b0                                       # (the first group alone would not have met one)
    assert all(k > sx.MAX_K for k in sx.DEEP_KS) and 65 in sx.DEEP_KS and 128 in sx.DEEP_KS and 129 in sx.DEEP_KS


def test_deep_passes_run_past_the_end_of_the_database():
    g = sx.GEOMETRIES["G7"]
    passes = -(-sx.MAX_K_DEEP // sx.MAX_K)
    assert passes == 32 and passes - -(-g["n"] // sx.MAX_K) - (g["n"] % sx.MAX_K == 0) == 8
    # passes 0 .. 23 deliver rows (the 24th only 28), passes 24 .. 31 start from an exhausted bound, ub = 0; the pass that
    # finds fewer rows than it asks for sets it
    assert 23 * sx.MAX_K < g["n"] < 24 * sx.MAX_K


def test_nonfinite_rows_score_as_stated(monkeypatch):
    X, Q = sx.nonfinite_data()
    g = sx.GEOMETRIES["G1"]
    rows = sx.NONFINITE_ROWS
    planted = np.concatenate(list(rows.values()))
    assert len(set(planted.tolist())) == len(planted)
    ip = sx.chain_scores(X, Q)
    q0 = np.array(sx.NONFINITE_Q0)[np.arange(g["nq"]) % 3]
    assert np.array_equal(Q[:, 0], q0.astype(np.float32))
    plus, minus, zero = q0 == 2, q0 == -2, q0 == 0
    assert np.isnan(ip[:, rows["nan"]]).all()
    assert (ip[plus][:, rows["big"]] == np.inf).all() and (ip[minus][:, rows["big"]] == -np.inf).all()
    assert (ip[zero][:, rows["big"]] == 0).all()                           # finite: a finite row gives no NaN
    assert (ip[plus][:, rows["inf"]] == np.inf).all() and (ip[minus][:, rows["inf"]] == -np.inf).all()
    assert np.isnan(ip[zero][:, rows["inf"]]).all()
    others = np.setdiff1d(np.arange(g["n"]), planted)
    assert np.isfinite(ip[:, others]).all()
    # what is never returned: IP NaN and -inf; L2 distance +inf (a NaN distance becomes 0 and ranks first)
    drop = sx.never_returned(X, Q, "cosine")
    assert drop[:, rows["nan"]].all() and not drop[:, others].any()
    assert not drop[plus][:, rows["big"]].any() and drop[minus][:, rows["big"]].all() and not drop[zero][:, rows["big"]].any()
    assert not drop[plus][:, rows["inf"]].any() and drop[minus][:, rows["inf"]].all() and drop[zero][:, rows["inf"]].all()
    drop2 = sx.never_returned(X, Q, "euclidean")
    assert not drop2[:, rows["nan"]].any() and not drop2[:, others].any()
    assert not drop2[plus][:, rows["big"]].any() and drop2[minus][:, rows["big"]].all() and drop2[zero][:, rows["big"]].all()
    assert not drop2[plus][:, rows["inf"]].any() and drop2[minus][:, rows["inf"]].all() and not drop2[zero][:, rows["inf"]].any()
    # one piece of panel 1 is planted solid: it delivers no key to a query with q[0] = -2 under IP and fewer than 64 to one with
    # q[0] = 0
    sx.apply_env(monkeypatch, {})
    solid = [(a, b) for panel, piece, a, b in sx.piece_ranges(2, 16, g["n"]) if panel == 1 and np.isin(np.arange(a, b), planted).all()]
    assert solid == [(1280, 1408)]
    a, b = solid[0]
    in_panel1 = np.arange(g["nq"]) >= sx.ROWS
    assert drop[in_panel1 & minus][:, a:b].all() and (in_panel1 & minus).any()
    assert ((~drop[in_panel1 & zero][:, a:b]).sum(axis=1) == len(rows["big"][(rows["big"] >= a) & (rows["big"] < b)])).all()
    assert 0 < (~drop[in_panel1 & zero][:, a:b]).sum(axis=1).max() < sx.MAX_K
    # and enough +inf rows overall that a k = 10 list of a q[0] = +2 query is +inf throughout, ties by index
    assert len(rows["big"]) + len(rows["inf"]) >= 70


def test_dedup_inputs_hold_the_distinct_rows_the_gpu_tests_expect():
    for d in sx.DEDUP_WIDTHS:
        assert d % 64 != 0
        for nq in sx.DEDUP_NQS:
            Q = sx.dedup_edge_queries(d, nq)
            assert Q.shape == (nq, d) and fx.n_distinct(Q) == sx.DEDUP_PROTOS
    assert sorted(nq % 4 for nq in sx.DEDUP_NQS) == [0, 1, 2, 3] and min(sx.DEDUP_NQS) == 1024   # LEMON_DEDUP_MIN_NQ
    assert fx.n_distinct(sx.dedup_boundary_queries(512)) == 512 and fx.n_distinct(sx.dedup_boundary_queries(513)) == 513
    assert 2 * 512 <= 1024 < 2 * 513
    Q, rows = sx.dedup_bit_queries()
    assert Q.shape == (sx.DEDUP_BITS_NQ, sx.DEDUP_BITS_D) and fx.n_distinct(Q) == 8
    base = Q[0]
    bits = lambda r: Q[r].view(np.uint32)
    assert (bits(1000) != bits(0)).sum() == 1 and abs(int(bits(1000)[64]) - int(bits(0)[64])) == 1
    zp, zn = rows["zero_pos"][0], rows["zero_neg"][0]
    assert np.array_equal(Q[zp], Q[zn]) and (bits(zp) != bits(zn)).sum() == 1 and bits(zn)[64] == 0x80000000
    assert np.array_equal(bits(rows["zero_pos"][0]), bits(rows["zero_pos"][1]))
    a, b = Q[rows["perm_a"][0]], Q[rows["perm_b"][0]]
    assert np.array_equal(np.sort(a), np.sort(b)) and np.array_equal(np.sort(a), np.sort(base)) and not np.array_equal(a, b)
    nan = rows["nan"]
    assert all(np.array_equal(bits(nan[0]), bits(r)) for r in nan) and np.isnan(Q[nan]).all()
    assert np.isnan(Q[rows["nan_payload"][0]]).all() and not np.array_equal(bits(rows["nan_payload"][0]), bits(nan[0]))
