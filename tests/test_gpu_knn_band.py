"""GPU: the 16-bit kNN filter scan (lemon_search_bf16) where its error band is nearly tight, and at the edges of the fp16 format.

The band  s~ > tau~ - 2 eps  is the only reason the scan's output equals the exact scan's, and random data stays 10-30 times inside
it.  tests/bandfx.py builds data on which the rows of the exact top-k lie 0.63-0.94 of the band below the k-th filter score
(tests/test_knn_band_host.py holds that on the CPU), so a band half as wide -- tau - eps, a missing L2 doubling, a residual maximum
taken over the wrong rows -- loses rows of the oracle at every one of the places that apply it: the tile epilogues of the five
scan kernels, their light compactions and k_bf16_final's prefilter.  Every case is (D, I) of the CPU oracle, bit for bit."""
import numpy as np
import pytest

from tests import bandfx as fx
from tests.synth import unit_rows
from tests.test_gpu_parity import _assert_knn_equal, _search, cu
from tests.test_knn_bf16_plan_host import planned

pytestmark = pytest.mark.gpu
F32, BF16 = 1, 2

_reference = {}     # (metric, d, k, layout, n) -> (D, I) of the oracle: computed once, shared by the kernels that see the same data


def _case(oracle, metric, d, k, layout, n):
    X, Q = fx.case_data(metric, d, k, layout, n)
    key = (metric, d, k, layout, n)
    if key not in _reference:
        _reference[key] = oracle.knn(metric, X, Q, k)
    return X, Q, _reference[key]


def _bf16_search(hip, metric, X, Q, k, wide=False):
    idx = (hip.IndexFlatIP if metric == "ip" else hip.IndexFlatL2)(X.shape[1])
    idx.set_algo(BF16)
    idx.set_wide_filter(wide)
    idx.add(cu(X))
    D, I = idx.search(cu(Q), k)
    return D.cpu().numpy(), I.cpu().numpy(), idx


# ---- 1. worst-case rounding: every kernel, both metrics, all four layouts ---------------------------------------------------
@pytest.mark.parametrize("kernel,env,wide,metric,d,layout,k,n", fx.rounding_cases(),
                         ids=[f"{c[0]}-{c[3]}-d{c[4]}-{c[5]}-k{c[6]}" for c in fx.rounding_cases()])
def test_worst_case_rounding_keeps_every_oracle_row(hip, oracle, monkeypatch, kernel, env, wide, metric, d, layout, k, n):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    X, Q, ref = _case(oracle, metric, d, k, layout, n)
    D, I, idx = _bf16_search(hip, metric, X, Q, k, wide)
    info = idx.last_search_info()
    assert info["algo"] == BF16 and idx.last_scan_kernel() == kernel
    assert info["db_splits"] == 1           # (a split has a tau of its own: victims and impostors have to meet in one list)
    _assert_knn_equal((D, I), ref)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_worst_case_rounding_across_two_database_splits(hip, oracle, monkeypatch, metric):
    # victims in the first split, impostors in the second: each split builds its own tau, k_merge joins the exact lists
    kernel, env, wide, d, layout, k, n = fx.SPLIT_CASE
    monkeypatch.setenv("LEMON_SPLITS", env["LEMON_SPLITS"])
    X, Q, ref = _case(oracle, metric, d, k, layout, n)
    D, I, idx = _bf16_search(hip, metric, X, Q, k, wide)
    info = idx.last_search_info()
    assert info["algo"] == BF16 and idx.last_scan_kernel() == kernel and info["db_splits"] == 2
    _assert_knn_equal((D, I), ref)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_worst_case_rounding_across_two_chunked_launches(hip, oracle, monkeypatch, metric):
    # victims in the first launch (8 tiles), impostors in the second (7): tau and the lists are carried in the state
    kernel, env, wide, d, layout, k, n = fx.CHUNK_CASE
    monkeypatch.setenv("LEMON_CHUNK_MB", env["LEMON_CHUNK_MB"])
    row, = planned("CHUNK_MB=0.01", d, wide, metric == "l2", n, fx.N_QUERIES)
    assert row["kernel"] == kernel and row["splits"] == 1 and row["chunk_tiles"] < row["n_tiles"]
    X, Q, ref = _case(oracle, metric, d, k, layout, n)
    D, I, idx = _bf16_search(hip, metric, X, Q, k, wide)
    info = idx.last_search_info()
    assert info["algo"] == BF16 and idx.last_scan_kernel() == kernel and info["db_splits"] == 1
    _assert_knn_equal((D, I), ref)


# ---- 2. the format edges of k_convert_bf16: saturation at +-65 504, flushed subnormals, the residual carries the excess -------
N_EDGE, NQ_EDGE, K_EDGE = 700, 150, 10      # more rows than a candidate list holds (CAPH = 512), a ragged query panel
EDGE_DIMS = [96, 768]


def _edge_check(hip, oracle, metric, X, Q, k=K_EDGE, f32_too=False):
    ref = oracle.knn(metric, X, Q, k)
    D, I, idx = _bf16_search(hip, metric, X, Q, k)
    assert idx.last_search_info()["algo"] == BF16
    _assert_knn_equal((D, I), ref)
    if f32_too:
        D, I, idx = _search(hip, metric, X, Q, k, algo=F32)
        assert idx.last_search_info()["algo"] == F32
        _assert_knn_equal((D, I), ref)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", EDGE_DIMS)
def test_saturated_rows_and_queries(hip, oracle, metric, d):
    # (a) components of 1e5 .. 1e6 in a few rows and a few queries: the copies hold +-65 504 and the residual the rest
    rng = np.random.default_rng(100 + d)
    X, Q = unit_rows(rng, N_EDGE, d), unit_rows(rng, NQ_EDGE, d)
    for A, rows in ((X, [0, 63, 64, 300, 511, 512, N_EDGE - 1]), (Q, [0, 31, 127, 128, NQ_EDGE - 1])):
        A[rows] = (rng.uniform(1e5, 1e6, (len(rows), d)) * rng.choice([-1.0, 1.0], (len(rows), d))).astype(np.float32)
    assert np.abs(fx.to_fp16(X)).max() == 65504.0 and np.isfinite(fx.to_fp16(Q).astype(np.float32)).all()
    _edge_check(hip, oracle, metric, X, Q, f32_too=True)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", EDGE_DIMS)
def test_a_database_whose_every_component_flushes_to_zero(hip, oracle, metric, d):
    # (b) xh = 0: every row is in every band, and 700 rows > CAPH force the exact compaction at each overflow
    rng = np.random.default_rng(200 + d)
    X = unit_rows(rng, N_EDGE, d) * np.float32(2.0 ** -22)
    Q = unit_rows(rng, NQ_EDGE, d)
    assert not fx.to_fp16(X).any()
    _edge_check(hip, oracle, metric, X, Q)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", EDGE_DIMS)
def test_half_of_the_rows_flushed_half_normal(hip, oracle, metric, d):
    # (c) the residual maximum comes from the normal rows, the flushed rows' scores are all 0 (ip) / -|q|^2 - |x|^2 (l2)
    rng = np.random.default_rng(300 + d)
    # normal rows on one side of a direction m, two thirds of the queries on the other: for those the flushed rows win under
    # either metric (s~ = 0 for all of them: only the exact pass can order them), for the rest the normal rows do
    m = unit_rows(rng, 1, d)
    X, Q = unit_rows(rng, N_EDGE, d) - m, unit_rows(rng, NQ_EDGE, d) + m
    Q[::3] -= 2.0 * m
    flushed = rng.permutation(N_EDGE) < N_EDGE // 2
    X[flushed] *= np.float32(2.0 ** -23)
    assert not fx.to_fp16(X[flushed]).any() and fx.to_fp16(X[~flushed]).any(axis=1).all()
    _edge_check(hip, oracle, metric, X, Q, k=64)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", EDGE_DIMS)
def test_zero_rows_and_an_all_zero_query(hip, oracle, metric, d):
    # (d) |q| = 0: eps is its 1e-30 floor (ip) and every score ties at 0; zero rows tie with each other for every query
    rng = np.random.default_rng(400 + d)
    X, Q = unit_rows(rng, N_EDGE, d), unit_rows(rng, NQ_EDGE, d)
    X[[0, 5, 63, 64, 127, 128, 400, N_EDGE - 1]] = 0.0
    X[200:230] = 0.0
    Q[[0, 77, NQ_EDGE - 1]] = 0.0
    _edge_check(hip, oracle, metric, X, Q, k=64)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", EDGE_DIMS)
def test_fp16_exact_operands_leave_the_fp32_sum_term_alone(hip, oracle, metric, d):
    # (e) xr2 = qres2 = 0: the band is 3 d 2^-24 |q| max|x| and nothing else.  Every row is a permutation of one vector's components,
    # so for the constant-magnitude queries all 700 exact scores tie up to the ORDER of summation -- the chain's against the MFMA's
    rng = np.random.default_rng(500 + d)
    base = fx.to_fp16(rng.uniform(0.5, 1.5, d) / np.sqrt(d)).astype(np.float32)
    sigma = rng.choice([-1.0, 1.0], d).astype(np.float32)
    X = np.stack([sigma * base[rng.permutation(d)] for _ in range(N_EDGE)]).astype(np.float32)
    c = np.float32(np.float16(1.0 / np.sqrt(d)))
    Q = fx.to_fp16(unit_rows(rng, NQ_EDGE, d)).astype(np.float32)
    Q[::2] = c * sigma[None, :] * np.float32(2.0) ** rng.integers(-2, 3, (len(Q[::2]), 1)).astype(np.float32)
    for A in (X, Q):
        assert np.array_equal(fx.to_fp16(A).astype(np.float32), A)
    _edge_check(hip, oracle, metric, X, Q, k=64)


@pytest.mark.parametrize("d", EDGE_DIMS)
def test_a_residual_that_overflows_float32(hip, oracle, d):
    # (f) inner product: one component of 3e19 makes max|x - xh|^2 and max|x|^2 +inf.  The band of an ordinary query is then +inf
    # (everything is re-scored exactly); for an all-zero query it is 0 * inf, which must mean the same and not NaN (as NaN it emptied
    # the lists of the three zero queries at the first light compaction: 30 of 1 500 indices wrong at either width)
    rng = np.random.default_rng(600 + d)
    X, Q = unit_rows(rng, N_EDGE, d), unit_rows(rng, NQ_EDGE, d)
    X[333, d // 2] = np.float32(3e19)
    Q[[0, 64, NQ_EDGE - 1]] = 0.0
    with np.errstate(over="ignore"):
        assert np.isinf((X[333] * X[333]).sum()) and np.isfinite(X).all()
    _edge_check(hip, oracle, "ip", X, Q, f32_too=True)
