"""Shared by tests/test_scan_f32_edges_host.py (CPU) and tests/test_gpu_scan_f32_edges.py (GPU): the geometries, knob settings
and data sets that hold the exact fp32 scan (k_scan_f32, k_merge, k_place_pass in knn_f32.hip, the pair lists of knn_common.hpp)
to the CPU oracle at every piece, knob and pass edge, and the compare helpers.  Handles, plans and bit comparison come from
tests/indexfx.py; nothing of it is repeated here.

Every comparison is bit for bit, in D and I, on ALL queries of a call (the pieces differ per panel, a sample could miss one).
The oracle's answer is computed once per (data set, metric, k) and shared by every knob setting (expected()).

The host file proves, without a device, that the geometries give the plans the table claims and that the data sets have the
properties the GPU tests rely on; the GPU file then only has to search and compare."""
import os

import numpy as np

from tests import indexfx as fx
from tests.synth import unit_rows

ROWS = fx.ROWS
MAX_K = fx.MAX_K
MAX_K_DEEP = 2048       # LEMON_MAX_K_DEEP
PAIR_CAP = 512          # knn_common.hpp: a query's candidate list, one half per lane of its pair
N_PROTOS = 7

PLAN_KNOBS = ("LEMON_SPLITS", "LEMON_XCDS", "LEMON_SEG_COST")
KNOBS = PLAN_KNOBS + ("LEMON_SHARE_BOUNDS", "LEMON_STALE", "LEMON_FAIR")

# ---- geometries (BQ = BX = 128; plans for 512 resident slots = lemon_debug_scan_plan's) ---------------------------------------
# env: the setting the row is planned under.  The expectations are what the issue's table states; the host test holds
# lemon_debug_scan_plan to every one of them, so that the GPU tests cannot drift onto one-workgroup plans unnoticed.
GEOMETRIES = {
    # 2-3 pieces per panel, a workgroup with 2 segments, a 1-tile segment, ragged last panel and last tile
    "G1": dict(nq=200, n=1957, env={}, grid=4, splits=3, pieces=(2, 3), max_segs=2, one_tile=True),
    "G1c": dict(nq=200, n=1957, env={"LEMON_SEG_COST": "0"}, grid=4, splits=2, pieces=(2, 2), max_segs=1, one_tile=False),
    # 1-3 pieces per panel, 3 segments per workgroup, 1-tile segments
    "G2": dict(nq=974, n=521, env={"LEMON_SEG_COST": "0"}, grid=5, splits=3, pieces=(1, 3), max_segs=3, one_tile=True),
    # XCD groups on (65 panels >= 8 x 8), 2 pieces per panel, up to 9 segments per workgroup
    "G3": dict(nq=8315, n=1153, env={"LEMON_SEG_COST": "0"}, grid=81, splits=2, pieces=(2, 2), max_segs=9, one_tile=True),
    # splits == 1: 3 whole panels per workgroup, pair_final_topk<true> per segment
    "G4": dict(nq=1100, n=300, env={}, grid=3, splits=1, pieces=(1, 1), max_segs=3, one_tile=False),
    "G5": dict(nq=100, n=200, env={}, grid=1, splits=1, pieces=(1, 1), max_segs=1, one_tile=False),
    # the deep-k geometry: 3 pieces per panel
    "G6": dict(nq=300, n=3000, env={}, grid=9, splits=3, pieces=(3, 3), max_segs=1, one_tile=False),
    # deep passes past the end of the database: 2 pieces per panel
    "G7": dict(nq=256, n=1500, env={}, grid=3, splits=2, pieces=(2, 2), max_segs=2, one_tile=False),
}
MATRIX_GEOMETRIES = ("G1", "G2", "G3")
WIDTHS = (1, 63, 65, 129)           # d = 1, and d on either side of a dpad step (dpad is a multiple of 64)
MATRIX_KS = (1, 10, 64)

# ---- knob settings of the matrix: each is laid over the geometry's own env ----------------------------------------------------
# LEMON_FAIR 100 / 101 are the static-priority diagnostics (they only change the issue priority); 13 and 18 are the ends of the
# derived range.  LEMON_SPLITS: 7 on G1 gives 6 splits of 3 tiles (with kk = 64 k_merge takes two trips of 192 keys, the last
# split holds the ragged tile), 0 is the automatic count.
SETTINGS = [
    {},
    {"LEMON_SHARE_BOUNDS": "0"},
    {"LEMON_STALE": "1"},                 # a selection, and a published bound, after every tile
    {"LEMON_STALE": "100000"},            # `stale` never fires: `warm` once, then `full` alone keeps the lists in their halves
    {"LEMON_FAIR": "0"}, {"LEMON_FAIR": "13"}, {"LEMON_FAIR": "18"}, {"LEMON_FAIR": "100"}, {"LEMON_FAIR": "101"},
    {"LEMON_XCDS": "1"},
    {"LEMON_SEG_COST": "0"}, {"LEMON_SEG_COST": "10"},
    {"LEMON_SPLITS": "1"}, {"LEMON_SPLITS": "2"}, {"LEMON_SPLITS": "7"}, {"LEMON_SPLITS": "0"},
]
DEEP_SETTINGS = [{}, {"LEMON_SPLITS": "2"}, {"LEMON_SHARE_BOUNDS": "0"}, {"LEMON_STALE": "1"}]


def setting_id(s):
    return ",".join(f"{k[6:]}={v}" for k, v in s.items()) or "default"


def env_of(geometry, setting):
    return {**GEOMETRIES[geometry]["env"], **setting}


def apply_env(monkeypatch, env):
    """exactly `env` among the scan's knobs, whatever the process had set before"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def shape_of(geometry):
    g = GEOMETRIES[geometry]
    return -(-g["nq"] // ROWS), -(-g["n"] // ROWS)


def plan_splits(panels, n_tiles, forced):
    """(splits, tiles per split) of the (panel, split) rectangles LEMON_SPLITS selects: `forced` > 0 fixes the count (at most one
    split per tile), 0 asks for enough workgroups to fill 768 slots while every split keeps 8 tiles; the count is then what
    equal splits of whole tiles really need"""
    splits = 1
    if forced > 0:
        splits = min(forced, n_tiles)
    elif panels < 768:
        splits = min(-(-768 // panels), max(n_tiles // 8, 1))
    per = -(-n_tiles // splits)
    return -(-n_tiles // per), per


def expected_launch(panels, n_tiles):
    """(grid, db_splits) last_search_info() must report for a search of panels x n_tiles units under the knobs now in the
    environment (set them with apply_env first): the segment plan's, or the rectangles' under LEMON_SPLITS"""
    if "LEMON_SPLITS" in os.environ:
        splits, _ = plan_splits(panels, n_tiles, int(os.environ["LEMON_SPLITS"]))
        return panels * splits, splits
    if panels * n_tiles < 2:
        return 1, 1
    pl = fx.scan_plan(panels, n_tiles)
    return pl["grid"], pl["splits"]


def piece_ranges(panels, n_tiles, n):
    """[(panel, piece, first row, end row)] of every piece under the knobs now in the environment"""
    if "LEMON_SPLITS" in os.environ:
        splits, per = plan_splits(panels, n_tiles, int(os.environ["LEMON_SPLITS"]))
        return [(p, s, s * per * ROWS, min((s + 1) * per * ROWS, n)) for p in range(panels) for s in range(splits)]
    segs = fx.scan_plan(panels, n_tiles)["segs"]
    return [(int(p), int(c), int(t0) * ROWS, min(int(t0 + nt) * ROWS, n)) for p, t0, nt, c in segs]


# ---- data sets ----------------------------------------------------------------------------------------------------------------
DATASETS = ("random", "prototypes", "ascending", "around_zero", "identical")
_SEEDS = {name: 1009 * (i + 1) for i, name in enumerate(DATASETS)}


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _rescale(rng, A):
    """IndexFlatL2 is a general index: rows of norm 0.5 .. 2, as in test_flat_search_bit_exact"""
    return _f32c(A * rng.uniform(0.5, 2.0, (A.shape[0], 1)).astype(np.float32))


def prototypes(rng, d):
    """N_PROTOS unit rows in a cone: every inner product of two of them is positive, so that a negated prototype scores
    negative against EVERY row"""
    return fx.cone_rows(rng, N_PROTOS, d)


def prototype_pattern(rng, n):
    """prototype number of every database row: inside every 128-row tile, blocks of N_PROTOS rows from the tile's start and
    the tile's last N_PROTOS rows are permutations of all prototypes -- every tile of at least N_PROTOS rows, hence every piece made of such tiles, holds
    each of them"""
    lab = np.empty(n, np.int64)
    for t0 in range(0, n, ROWS):
        t1 = min(t0 + ROWS, n)
        if t1 - t0 < N_PROTOS:               # a last tile too short to hold them all (G3: one row)
            lab[t0:t1] = rng.permutation(N_PROTOS)[:t1 - t0]
            continue
        for b in range(t0, t1, N_PROTOS):
            lab[b:min(b + N_PROTOS, t1)] = rng.permutation(N_PROTOS)[:min(b + N_PROTOS, t1) - b]
        lab[t1 - N_PROTOS:t1] = rng.permutation(N_PROTOS)
    return lab


def around_zero_t(n):
    """the multiple of the axis in every row: one row in 40 a tiny positive value, one in 40 a tiny negative one (1e-18 ..
    1e-3 in magnitude, well clear of the subnormal range), all others exactly 0 -- fewer than 64 rows of either sign at the
    sizes used here, so that a top-64 list runs through the tie group of exact zeros"""
    mags = np.array([1e-18, 1e-15, 1e-12, 1e-9, 1e-6, 1e-3])
    i = np.arange(n)
    t = np.zeros(n)
    pos, neg = i % 40 == 7, i % 40 == 19
    t[pos] = mags[(i[pos] // 40) % len(mags)]
    t[neg] = -mags[(i[neg] // 40) % len(mags)]
    return t


AXIS_COLS = 4           # around_zero: the axis is 0.5 on the first four columns (norm exactly 1), the rows are 0 there


def make(name, nq, n, d, metric):
    """(X [n, d], Q [nq, d]) float32 of one data set, seeded by its name and shape"""
    l2 = fx.is_l2(metric)
    rng = np.random.default_rng(_SEEDS[name] + 7 * nq + 3 * n + d)
    if name == "random":
        X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
        return (_rescale(rng, X), _rescale(rng, Q)) if l2 else (X, Q)
    if name == "prototypes":
        # every top-k list is ONE tie group spread over all tiles; IP scores are exactly equal within a group (equal rows,
        # equal chains); under L2 (unit scale, not rescaled) a query's own prototype is at distance exactly 0: with s the
        # chain <p, p>, fma(-2, s, s + s) = 0
        P = prototypes(rng, d)
        X = P[prototype_pattern(rng, n)]
        cls = rng.integers(0, 2 * N_PROTOS, nq)
        cls[:2 * N_PROTOS] = np.arange(2 * N_PROTOS)
        Q = np.where((cls >= N_PROTOS)[:, None], -P[cls % N_PROTOS], P[cls % N_PROTOS])
        return _f32c(X), _f32c(Q)
    if name == "ascending":
        # every later row beats all earlier ones, for every query: every row is admitted, whatever the bound.  IP: the
        # construction of test_flat_search_ascending_scores_worst_case with the noise made orthogonal to q, so that the
        # order is strict; L2 (not rescaled): rows at distance r from q, r falling from 2 to 0.5 in equal steps
        q = unit_rows(rng, 1, d).astype(np.float64)
        u = rng.standard_normal((n, d))
        u -= (u @ q.T) * q
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        if l2:
            X = q + np.linspace(2.0, 0.5, n)[:, None] * u
        else:
            t = np.linspace(0.0, 1.0, n)[:, None]
            X = t * q + (1 - t) * 0.1 * u
        return _f32c(X), _f32c(np.repeat(q, nq, axis=0))
    if name == "around_zero":
        # IP scores straddle 0 closely, with many exact zeros: the products of the axis with the rest of a row are exact
        # zeros, so the chain gives t (to rounding, sign and zero kept) for +a and -t for -a
        assert d >= 2 * AXIS_COLS
        a = np.zeros(d)
        a[:AXIS_COLS] = 0.5
        R = unit_rows(rng, n, d).astype(np.float64)
        R[:, :AXIS_COLS] = 0.0
        X = R + around_zero_t(n)[:, None] * a
        Q = np.where((np.arange(nq) % 2 == 0)[:, None], a, -a)
        X, Q = _f32c(X), _f32c(Q)
        return (_rescale(rng, X), _rescale(rng, Q)) if l2 else (X, Q)
    if name == "identical":
        X = np.tile(unit_rows(rng, 1, d), (n, 1))
        Q = unit_rows(rng, nq, d)
        return _f32c(X), (_rescale(rng, Q) if l2 else Q)
    raise KeyError(name)


# ---- deep passes (k > 64) -----------------------------------------------------------------------------------------------------
DEEP_D = 64
DEEP_KS = (65, 128, 129, 300)
DEEP_TIES = ((100, 400), (1100, 1600))     # [first, end) of the two groups of identical rows; query g is group g's row


def deep_data(n=None, nq=None):
    """G6's data: the existing deep test's, larger.  Rows 100..399 are one row: a 300-row tie group across the tile boundaries
    128 / 256 / 384 and -- for query 0, whose 300 best they are -- across the pass boundaries 64 / 128 / 192 / 256.  Rows
    1100..1599 are another (query 1): it crosses the first piece boundary of G6's plan (row 1152) and that of LEMON_SPLITS=2
    (row 1536), which the first group does not reach."""
    g = GEOMETRIES["G6"]
    n, nq = n or g["n"], nq or g["nq"]
    rng = np.random.default_rng(77)
    X, Q = unit_rows(rng, n, DEEP_D), unit_rows(rng, nq, DEEP_D)
    for i, (a, b) in enumerate(DEEP_TIES):
        X[a:b] = X[a]
        Q[i] = X[a]
    return X, Q


# ---- non-finite scores --------------------------------------------------------------------------------------------------------
BIG = np.float32(3e38)
# planted rows of G1 (n = 1957; the default plan's pieces of panel 0 are rows [0, 1280) and [1280, 1957), those of panel 1
# [0, 1280), [1280, 1408) and [1408, 1957)): the one-tile piece [1280, 1408) is planted solid, so that it delivers no key at
# all to a query that can return none of these rows, and fewer than kk otherwise
NONFINITE_ROWS = dict(
    nan=np.r_[3:9, 1280:1320],                       # all-NaN rows
    big=np.r_[20:60, 700, 1320:1370, 1950:1957],     # 3e38 * e_0
    inf=np.r_[100:104, 1370:1408],                   # +inf * e_0
)
NONFINITE_Q0 = (2.0, -2.0, 0.0)                       # query i has q[0] = NONFINITE_Q0[i % 3]


def nonfinite_data():
    """G1 at d = 64 with planted rows.  By the fp32 fmaf chain a query with q[0] = +2 / -2 / 0 scores
         3e38 * e_0 rows   +inf / -inf / 0     (2 x 3e38 overflows; a FINITE row cannot give a NaN through a chain from +0)
         +inf * e_0 rows   +inf / -inf / NaN   (0 x inf)
         all-NaN rows      NaN / NaN / NaN
    under IP.  The issue names the first and third kind and expects NaN for q[0] = 0 from the first; only an infinite entry
    gives that, so the second kind is planted as well and the classes above are what the host test asserts."""
    g = GEOMETRIES["G1"]
    rng = np.random.default_rng(99)
    X, Q = unit_rows(rng, g["n"], 64), unit_rows(rng, g["nq"], 64)
    X[NONFINITE_ROWS["nan"]] = np.nan
    for kind, v in (("big", BIG), ("inf", np.float32(np.inf))):
        X[NONFINITE_ROWS[kind]] = 0.0
        X[NONFINITE_ROWS[kind], 0] = v
    Q[:, 0] = np.array(NONFINITE_Q0, np.float32)[np.arange(g["nq"]) % 3]
    return X, Q


def chain_scores(X, Q):
    """<q, x> of every pair by the float32 fmaf chain in ascending k from +0, in plain numpy: a float64 product of two float32
    values is exact and one rounding of (product + acc) to float32 is the fused operation's, so long as that sum is exact in
    float64 -- it is not always (53 bits), so this is only used to CLASSIFY scores (NaN, +inf, -inf, finite), which rounding
    in the last place cannot change at the magnitudes planted"""
    acc = np.zeros((Q.shape[0], X.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for k in range(X.shape[1]):
            acc = (Q[:, k:k + 1].astype(np.float64) * X[None, :, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def chain_norms(A):
    """<a, a> of every row by the same chain"""
    acc = np.zeros(A.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for k in range(A.shape[1]):
            acc = (A[:, k].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)
    return acc


def l2_from_ip(ip, qn, xn):
    """the contract's distance max(0, fma(-2, ip, qn + xn)), literally: a NaN fails the '> 0' test and becomes 0"""
    with np.errstate(all="ignore"):
        v = (-2.0 * ip.astype(np.float64) + (qn[:, None] + xn[None, :]).astype(np.float32).astype(np.float64)).astype(np.float32)
        return np.where(v > 0, v, np.float32(0.0))


def never_returned(X, Q, metric):
    """bool [nq, n]: the pairs the search never returns -- an IP score of -inf or NaN, an L2 distance of +inf.  (The kernel's
    lists start at -inf and admit with '>', as faiss's heaps start at -/+FLT_MAX.)"""
    ip = chain_scores(X, Q)
    if not fx.is_l2(metric):
        return np.isnan(ip) | (ip == -np.inf)
    return l2_from_ip(ip, chain_norms(Q), chain_norms(X)) == np.inf


def expected_without(oracle, metric, X, Q, k, drop):
    """the contract's answer where drop [nq, n] marks the never-returned pairs: per group of queries with one drop pattern,
    oracle.knn over the rows that remain, indices mapped back.  The oracle's OWN handling of -inf (lo_push admits it) is not
    used: no such row is ever shown to it."""
    nq = Q.shape[0]
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    pats, inv = np.unique(drop, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for p, pat in enumerate(pats):
        keep = np.flatnonzero(~pat)
        rows = np.flatnonzero(inv == p)
        Dp, Ip = oracle.knn(metric, X[keep], Q[rows], k)
        D[rows] = Dp
        I[rows] = np.where(Ip >= 0, keep[np.maximum(Ip, 0)], -1)
    return D, I


# ---- compare ------------------------------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(oracle, key, metric, X, Q, k):
    """oracle.knn(metric, X, Q, k) on ALL queries, computed once per (key, metric, k); the arrays are shared: read only"""
    full = (key, metric, k)
    if full not in _EXPECTED:
        D, I = oracle.knn(metric, X, Q, k)
        D.setflags(write=False)
        I.setflags(write=False)
        _EXPECTED[full] = (D, I)
    return _EXPECTED[full]


def assert_bits(D, I, Do, Io, what=""):
    """(D, I) tensors of a search against expected arrays, bit for bit, every query"""
    Ig, Dg = I.cpu().numpy(), D.cpu().numpy()
    assert Ig.shape == Io.shape and Dg.shape == Do.shape and Dg.dtype == np.float32 and Ig.dtype == np.int64
    bad = np.flatnonzero((Ig != Io).any(axis=1) | (Dg.view(np.int32) != Do.view(np.int32)).any(axis=1))
    if len(bad):
        q = int(bad[0])
        c = int(np.flatnonzero((Ig[q] != Io[q]) | (Dg[q].view(np.int32) != Do[q].view(np.int32)))[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(Ig)} queries differ from the oracle; first: query {q} column {c}: "
                             f"got ({Dg[q, c]!r}, {Ig[q, c]}), expected ({Do[q, c]!r}, {Io[q, c]})")


def assert_ties_ascend(D, I):
    """within equal D, I ascends (the tie rule itself); padding (-1) excluded"""
    Dg, Ig = D.cpu().numpy(), I.cpu().numpy()
    same = (Dg[:, 1:] == Dg[:, :-1]) & (Ig[:, 1:] >= 0)
    assert (Ig[:, 1:][same] > Ig[:, :-1][same]).all()


def padding(metric):
    return np.float32(np.finfo(np.float32).max) * (1 if fx.is_l2(metric) else -1)


# ---- query dedup edges (tests/test_gpu_dedup.py) ------------------------------------------------------------------------------
DEDUP_N, DEDUP_K, DEDUP_PROTOS = 500, 3, 40
DEDUP_WIDTHS = (1, 63, 65, 100)          # d % 64 != 0: a lane's second trip through the hash and compare loops (or none at d = 1)
DEDUP_NQS = (1024, 1025, 1026, 1027)     # every nq % 4: the `row >= n` guard inside a 4-row block
DEDUP_BITS_D, DEDUP_BITS_NQ = 65, 2048


def dedup_db(d):
    return _f32c(np.random.default_rng(500 + d).standard_normal((DEDUP_N, d)))


def dedup_edge_queries(d, nq):
    """nq rows drawn from DEDUP_PROTOS distinct rows (plain normal values: distinct at d = 1 too), each at least once"""
    rng = np.random.default_rng(41 * d + nq)
    return fx.repeated(rng, _f32c(rng.standard_normal((DEDUP_PROTOS, d))), nq)


def dedup_boundary_queries(distinct, nq=1024, d=65):
    """nq rows with exactly `distinct` distinct ones: 2 U <= nq folds, one more distinct row does not"""
    rng = np.random.default_rng(distinct)
    return fx.repeated(rng, _f32c(rng.standard_normal((distinct, d))), nq)


def dedup_bit_queries():
    """2048 rows at d = 65 (column 64 is a lane's second trip), copies of one base row except, -> (Q, {what: row numbers}):
         ulp        the base with column 64 one ulp up
         zero_pos   the base with column 64 = +0.0 (twice), zero_neg the same with -0.0: equal as numbers, not as bits
         perm_a/b   the base with columns (3, 10) / (5, 64) exchanged: permutations of each other and of the base
         nan        four all-NaN rows of equal bits (merged), nan_payload one all-NaN row with another payload"""
    rng = np.random.default_rng(0)
    d, nq = DEDUP_BITS_D, DEDUP_BITS_NQ
    base = rng.standard_normal(d).astype(np.float32)
    Q = np.tile(base, (nq, 1))
    rows = dict(ulp=[1000], zero_pos=[300, 1301], zero_neg=[77], perm_a=[5], perm_b=[2047], nan=[9, 640, 641, 1999], nan_payload=[1500])
    Q[1000, 64] = np.nextafter(base[64], np.float32(10))
    Q[rows["zero_pos"], 64] = 0.0
    Q[77, 64] = -0.0
    Q[5, [3, 10]] = base[[10, 3]]
    Q[2047, [5, 64]] = base[[64, 5]]
    Q[rows["nan"]] = np.float32(np.nan)
    Q.view(np.uint32)[1500] = 0x7fc00001
    return Q, rows
