"""GPU: the exact fp32 scan (k_scan_f32, k_merge, k_place_pass in knn_f32.hip; the pair lists of knn_common.hpp) against the CPU
oracle at every piece, knob and pass edge.  Bit for bit in D and I, every query of every call, no tolerance anywhere: the scan's
contract is equality with oracle.knn under the fp32 fmaf chain in ascending k, ties to the lower index.

What each test adds to the suite is in its docstring; the geometries, settings and data sets are in tests/scanfx.py, and
tests/test_scan_f32_edges_host.py proves on the CPU that they are what they are said to be (the plan of every geometry, ties
across every piece, every row admitted, ...).  Each search also asserts, from last_search_info(), that it ran the grid and the
split count the host plan gives for its knobs: a case cannot quietly run as one workgroup.

Race timing.  WHEN a piece imports the bound another piece of its panel has published depends on how the workgroups interleave,
which a test cannot force.  The tie-heavy data sets (prototypes, identical, around_zero) are built so that ANY import meets a
tie: every tile of every piece holds rows of the score every other piece will publish, so a piece that drops a row tying an
imported bound (the bound itself instead of the next lower float, or a wrong order encoding at a sign change or at zero) loses a
row that wins on the index whenever the import comes before the row.  Nothing here sleeps, spins or repeats a run to chase an
interleaving; LEMON_STALE=1 publishes a bound after every tile, which makes early imports the rule rather than the exception.

Expected values come from oracle.knn or numpy alone; comparisons between two GPU calls are only ever added on top."""
import numpy as np
import pytest
import torch

from tests import indexfx as fx
from tests import scanfx as sx
from tests.indexfx import BF16, F32, bits_equal, cu, new_index
from tests.synth import unit_rows

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "euclidean"]


class Checked:
    """one handle (dedup off: the data sets repeat queries, and a folded call has other panels), its queries on the device,
    and the oracle's answers on the device, uploaded once per k"""

    def __init__(self, hip, oracle, monkeypatch, key, metric, X, Q):
        self.oracle, self.mp, self.key, self.metric, self.X, self.Q = oracle, monkeypatch, key, metric, X, Q
        self.ix = new_index(hip, metric, X.shape[1], F32, X, dedup=False)
        self.qt = cu(Q)
        self.panels, self.tiles = -(-Q.shape[0] // sx.ROWS), -(-X.shape[0] // sx.ROWS)
        self.want = {}

    def expect(self, k, DI=None):
        if k not in self.want:
            Do, Io = DI if DI is not None else sx.expected(self.oracle, self.key, self.metric, self.X, self.Q, k)
            self.want[k] = (Do, Io, cu(Do.copy()), cu(Io.copy()))           # (the shared arrays are read-only)
        return self.want[k]

    def search(self, env, k):
        """search(Q, k) under exactly the knobs `env`; the call ran the exact scan on the planned grid; -> (D, I)"""
        sx.apply_env(self.mp, env)
        launch = sx.expected_launch(self.panels, self.tiles)
        D, I = self.ix.search(self.qt, k)
        info = self.ix.last_search_info()
        assert self.ix.last_scan_kernel() == "scan_f32" and info["algo"] == F32
        assert (info["grid"], info["db_splits"]) == launch, (env, k)
        assert (info["nq"], info["n"], info["k"], info["nq_distinct"]) == (self.Q.shape[0], self.X.shape[0], k, self.Q.shape[0])
        return D, I

    def check(self, env, k, DI=None):
        Do, Io, Dt, It = self.expect(k, DI)
        D, I = self.search(env, k)
        if not (bits_equal(I, It) and bits_equal(D, Dt)):
            sx.assert_bits(D, I, Do, Io, f"{self.key} {self.metric} k={k} {sx.setting_id(env)}")
        return D, I


def _case(hip, oracle, monkeypatch, geometry, dataset, metric, d=64):
    g = sx.GEOMETRIES[geometry]
    X, Q = sx.make(dataset, g["nq"], g["n"], d, metric)
    return Checked(hip, oracle, monkeypatch, (dataset, geometry, d), metric, X, Q)


# ---- 1. the knob matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dataset", sx.DATASETS)
@pytest.mark.parametrize("geometry", sx.MATRIX_GEOMETRIES)
def test_every_knob_setting_equals_the_oracle(hip, oracle, monkeypatch, geometry, dataset, metric):
    """all six per-call knobs (LEMON_SHARE_BOUNDS, LEMON_STALE, LEMON_FAIR and LEMON_XCDS for the first time) on multi-piece
    plans with hard data: one handle per (geometry, data set, metric), the settings in sequence on it, k = 1, 10, 64.
    `prototypes`, `identical` and `around_zero` make every import of a bound meet a tie -- at positive, all-negative, exactly
    zero scores and at L2 distance 0; `ascending` admits every row."""
    c = _case(hip, oracle, monkeypatch, geometry, dataset, metric)
    for k in sx.MATRIX_KS:
        for setting in sx.SETTINGS:
            c.check(sx.env_of(geometry, setting), k)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("stale", ["100000", "1"])
def test_full_lists_alone_trigger_the_selection(hip, oracle, monkeypatch, metric, stale):
    """`ascending` at k = 64 in pieces of 16, 10 and 8 tiles with LEMON_STALE=100000: `warm` fires once, `stale` never, every
    row is admitted (64 per lane and tile), so only `full` (ccnt > PAIR_CAP/2 - BX/2) stands between the lists and
    append_slot's clamp, which would overwrite the best rows without a fault.  The same with LEMON_STALE=1: a selection and a
    published bound after every tile."""
    c = _case(hip, oracle, monkeypatch, "G1", "ascending", metric)
    for plan in ({"LEMON_SPLITS": "1"}, {}, {"LEMON_SEG_COST": "0"}, {"LEMON_SPLITS": "2"}):
        c.check({**plan, "LEMON_STALE": stale}, sx.MAX_K)
        c.check({**plan, "LEMON_STALE": stale, "LEMON_SHARE_BOUNDS": "0"}, sx.MAX_K)


# ---- 2. widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dataset", ["random", "prototypes"])
@pytest.mark.parametrize("d", sx.WIDTHS)
def test_widths_around_a_dpad_step(hip, oracle, monkeypatch, d, dataset, metric):
    """d = 1 and d on either side of a step of dpad (63 / 65, 127 is next to 129's lower step): the zero padding of the last
    k-slice, on G1's multi-piece plan and on forced splits"""
    c = _case(hip, oracle, monkeypatch, "G1", dataset, metric, d)
    for setting in ({}, {"LEMON_SPLITS": "7"}, {"LEMON_STALE": "1"}):
        c.check(setting, 10)


# ---- 3. whole panels per workgroup --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dataset", ["prototypes", "ascending"])
@pytest.mark.parametrize("geometry", ["G4", "G5"])
def test_whole_panels_per_workgroup(hip, oracle, monkeypatch, geometry, dataset, metric):
    """splits == 1: three whole panels per workgroup, pair_final_topk<true> and a direct write-out per segment, LDS and lists
    reused behind the __syncthreads() (G4); one workgroup, two tiles (G5)"""
    c = _case(hip, oracle, monkeypatch, geometry, dataset, metric)
    for k in (1, sx.MAX_K):
        for setting in ({}, {"LEMON_STALE": "1"}, {"LEMON_STALE": "100000"}):
            c.check(setting, k)
    if geometry == "G5":
        # k > ntotal through the deep passes on one workgroup: -1 / -+FLT_MAX from column n on (k = n itself: no padding)
        n = sx.GEOMETRIES["G5"]["n"]
        D, I = c.check({}, n)
        assert bool((I >= 0).all())
        D, I = c.check({}, n + 100)
        assert bool((I[:, n:] == -1).all()) and bool((D[:, n:] == float(sx.padding(metric))).all()) and bool((I[:, :n] >= 0).all())


# ---- 4. deep passes on split plans --------------------------------------------------------------------------------------------
def _deep_case(hip, oracle, monkeypatch, metric):
    X, Q = sx.deep_data()
    return Checked(hip, oracle, monkeypatch, ("deep", "G6", sx.DEEP_D), metric, X, Q)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", sx.DEEP_KS)
def test_deep_passes_on_split_plans(hip, oracle, monkeypatch, metric, k):
    """key-bounded passes (the UB = true instantiations) with several pieces per panel: shared bounds, pair_final_topk<false>
    and k_merge behind every pass.  Two groups of identical rows cross tile, piece and pass boundaries."""
    c = _deep_case(hip, oracle, monkeypatch, metric)
    for setting in sx.DEEP_SETTINGS:
        D, I = c.check(setting, k)
        sx.assert_ties_ascend(D, I)
        D64, I64 = c.check(setting, sx.MAX_K)
        assert bits_equal(I[:, :sx.MAX_K].contiguous(), I64) and bits_equal(D[:, :sx.MAX_K].contiguous(), D64)
    Io = c.expect(k)[1]
    for g, (a, b) in enumerate(sx.DEEP_TIES):
        assert np.array_equal(Io[g], np.arange(a, a + k))


# ---- 5. deep passes past the end of the database ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_deepest_k_runs_past_the_end_of_the_database(hip, oracle, monkeypatch, metric):
    """k = LEMON_MAX_K_DEEP on 1500 rows in 2 pieces per panel: 32 passes, the last of them from an exhausted bound (ub = 0:
    nothing is admissible, every piece delivers no key).  k = 2049 is refused with nothing written."""
    from lemon_amd import _lib
    from lemon_amd.ops import ptr, stream_ptr
    g = sx.GEOMETRIES["G7"]
    rng = np.random.default_rng(13)
    X, Q = unit_rows(rng, g["n"], 64), unit_rows(rng, g["nq"], 64)
    c = Checked(hip, oracle, monkeypatch, ("random", "G7", 64), metric, X, Q)
    D, I = c.check({}, sx.MAX_K_DEEP)
    assert bool((I[:, g["n"]:] == -1).all()) and bool((D[:, g["n"]:] == float(sx.padding(metric))).all())
    assert bool((I[:, :g["n"]] >= 0).all())
    with pytest.raises(ValueError):
        c.ix.search(c.qt, sx.MAX_K_DEEP + 1)
    k = sx.MAX_K_DEEP + 1
    Ds = torch.full((g["nq"], k), 12345.0, dtype=torch.float32, device="cuda")
    Is = torch.full((g["nq"], k), -7, dtype=torch.int64, device="cuda")
    rc = _lib.load().lemon_index_search(c.ix._h, ptr(c.qt), g["nq"], k, ptr(Ds), ptr(Is), stream_ptr(c.ix.device))
    torch.cuda.synchronize()
    assert rc == -1                                                        # LEMON_E_INVALID
    assert bool((Ds == 12345.0).all()) and bool((Is == -7).all())
    c.check({}, 3)                                                         # the handle still serves


# ---- 6. deep passes behind dedup and on a filter handle -----------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_deep_passes_behind_query_dedup(hip, oracle, monkeypatch, metric):
    """1024 queries drawn from 100 rows over G6's database, k = 130: the folded call (100 queries: one panel, three passes)
    equals the unfolded one (8 panels) and the oracle"""
    sx.apply_env(monkeypatch, {})
    X, _ = sx.deep_data()
    rng = np.random.default_rng(5)
    protos = unit_rows(rng, 100, sx.DEEP_D)
    protos[0], protos[1] = X[sx.DEEP_TIES[0][0]], X[sx.DEEP_TIES[1][0]]
    Q = fx.repeated(rng, protos, 1024)
    assert fx.n_distinct(Q) == 100
    k = 130
    Do, Io = oracle.knn(metric, X, Q, k)
    on, off = new_index(hip, metric, sx.DEEP_D, F32, X), new_index(hip, metric, sx.DEEP_D, F32, X, dedup=False)
    qt = cu(Q)
    Da, Ia = on.search(qt, k)
    Db, Ib = off.search(qt, k)
    assert on.last_search_info()["nq_distinct"] == 100 and off.last_search_info()["nq_distinct"] == 1024
    assert on.last_search_info()["nq"] == 1024 and on.last_search_info()["k"] == k
    assert on.last_scan_kernel() == off.last_scan_kernel() == "scan_f32"
    sx.assert_bits(Da, Ia, Do, Io, "dedup on")
    sx.assert_bits(Db, Ib, Do, Io, "dedup off")
    assert bits_equal(Da, Db) and bits_equal(Ia, Ib)


@pytest.mark.parametrize("metric", METRICS)
def test_deep_k_on_a_filter_handle_is_rerouted_and_the_filter_returns(hip, oracle, monkeypatch, metric):
    """a handle set to the 16-bit filter serves k = 65 with the exact scan's passes (api.hip reroutes it), and k = 20 behind
    it with the filter again, over the workspaces the rerouted call left"""
    sx.apply_env(monkeypatch, {})
    rng = np.random.default_rng(17)
    d, n, nq = 512, 3000, 300
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    ix = new_index(hip, metric, d, BF16, X)
    qt = cu(Q)
    for k, exact in ((20, False), (65, True), (20, False), (sx.MAX_K, False), (129, True), (20, False)):
        D, I = ix.search(qt, k)
        assert (ix.last_scan_kernel() == "scan_f32") == exact, k
        assert (ix.last_search_info()["algo"] == F32) == exact
        sx.assert_bits(D, I, *sx.expected(oracle, ("filter", d), metric, X, Q, k), f"k={k}")


# ---- 7. non-finite scores at k > 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,k", [("cosine", 10), ("cosine", 70), ("euclidean", 10)])
def test_non_finite_scores_follow_the_faiss_contract(hip, oracle, monkeypatch, metric, k):
    """The contract (include/lemon_hip.h, lemon_index_search): a NaN inner product is never returned; an inner product of -inf
    or a distance of +inf is never returned (the lists start at -inf and admit with '>', as faiss's heaps start at -+FLT_MAX);
    +inf inner products rank first, ties by ascending index; L2 takes max(0, fma(-2, ip, |q|^2 + |x|^2)) literally, so a NaN
    there is distance 0.  Expected: oracle.knn over the rows that CAN be returned to a query, indices mapped back -- the
    oracle's own lo_push would admit a -inf score and is therefore never shown one.  One piece of panel 1 holds planted rows
    only: zero keys in `part` for a whole class of queries, and k_merge over short pieces."""
    X, Q = sx.nonfinite_data()
    drop = sx.never_returned(X, Q, metric)
    DI = sx.expected_without(oracle, metric, X, Q, k, drop)
    c = Checked(hip, oracle, monkeypatch, ("nonfinite", "G1", 64), metric, X, Q)
    for setting in ({}, {"LEMON_SPLITS": "7"}, {"LEMON_SHARE_BOUNDS": "0"}, {"LEMON_STALE": "1"}, {"LEMON_SPLITS": "1"}):
        D, I = c.check(setting, k, DI)
        Dg, Ig = D.cpu().numpy(), I.cpu().numpy()
        assert not np.isnan(Dg).any() and (Ig >= 0).all()
        assert not drop[np.arange(len(Ig))[:, None], Ig].any()             # no never-returned pair among the results
        if metric == "cosine":
            assert not (Dg == -np.inf).any()
            plus = np.flatnonzero(Q[:, 0] == 2)
            first = np.sort(np.concatenate([sx.NONFINITE_ROWS["big"], sx.NONFINITE_ROWS["inf"]]))[:k]
            assert (Dg[plus] == np.inf).all() and (Ig[plus] == first[None, :]).all()
        else:
            assert not np.isinf(Dg).any()
            assert (Dg[:, 0] == 0).all() and (Ig[:, 0] == sx.NONFINITE_ROWS["nan"][0]).all()    # NaN norm: distance 0, first
