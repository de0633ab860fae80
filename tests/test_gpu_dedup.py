"""GPU: query de-duplication (csrc/dedup.hip) is exact and actually folds duplicates."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("nq,C", [(5000, 100), (1024, 1), (3000, 1400), (4096, 4096)])
def test_search_with_duplicate_queries_is_bit_identical(hip, oracle, metric, nq, C):
    from lemon_amd.index import IndexFlatIP, IndexFlatL2
    from tests.synth import unit_rows
    rng = np.random.default_rng(nq + C)
    d, n, k = 96, 3000, 11
    X = unit_rows(rng, n, d)
    X[1::7] = X[0]                                             # duplicate DB rows too: ties go to the lower index
    protos = unit_rows(rng, C, d)
    protos[0] = X[5]
    assign = rng.integers(0, C, nq)
    assign[:C] = np.arange(C)                                  # every prototype occurs
    Q = np.ascontiguousarray(protos[assign])
    cls = IndexFlatIP if metric == "cosine" else IndexFlatL2
    a, b = cls(d), cls(d)
    b.set_query_dedup(False)
    xt, qt = torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda()
    a.add(xt); b.add(xt)
    Da, Ia = a.search(qt, k)
    Db, Ib = b.search(qt, k)
    assert torch.equal(Ia, Ib) and torch.equal(Da, Db)
    info_a, info_b = a.last_search_info(), b.last_search_info()
    n_distinct = len({r.tobytes() for r in Q})
    assert info_b["nq_distinct"] == nq
    assert info_a["nq_distinct"] == (n_distinct if 2 * n_distinct <= nq else nq)
    Do, Io = oracle.knn(metric, X, Q[:300], k)
    assert np.array_equal(Ia[:300].cpu().numpy(), Io) and np.array_equal(Da[:300].cpu().numpy(), Do)


def test_rows_differing_in_one_bit_are_not_merged(hip):
    from lemon_amd.index import IndexFlatIP
    rng = np.random.default_rng(0)
    d = 64
    base = rng.standard_normal(d).astype(np.float32)
    Q = np.tile(base, (2048, 1))
    Q[1000, 63] = np.nextafter(Q[1000, 63], np.float32(10))   # one ulp in the last column
    Q[7, 0] = -Q[7, 0]
    X = rng.standard_normal((500, d)).astype(np.float32)
    ix = IndexFlatIP(d)
    ix.add(torch.from_numpy(X).cuda())
    ix.search(torch.from_numpy(Q).cuda(), 3)
    assert ix.last_search_info()["nq_distinct"] == 3


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("k", [65, 100, 200])
def test_deep_k_equals_oracle_and_extends_shallow_search(hip, oracle, metric, k):
    """k > 64 (faiss has no limit): key-bounded passes of the exact scan.  The deep list equals the oracle's bit for bit,
    its first 64 columns equal a plain k=64 search, ties (duplicate rows) keep ascending index across pass boundaries,
    and k > ntotal pads with -1 / +-FLT_MAX."""
    from lemon_amd.index import IndexFlatIP, IndexFlatL2
    from tests.synth import unit_rows
    rng = np.random.default_rng(k)
    d, n, nq = 48, 700, 37
    X = unit_rows(rng, n, d)
    X[100:240] = X[100]                         # 140 exact duplicates: a tie group straddling the 64 / 128 boundaries
    Q = unit_rows(rng, nq, d)
    Q[0] = X[100]
    ix = (IndexFlatIP if metric == "cosine" else IndexFlatL2)(d)
    ix.add(torch.from_numpy(X).cuda())
    D, I = ix.search(torch.from_numpy(Q).cuda(), k)
    Do, Io = oracle.knn(metric, X, Q, k)
    assert np.array_equal(I.cpu().numpy(), Io) and np.array_equal(D.cpu().numpy(), Do)
    D64, I64 = ix.search(torch.from_numpy(Q).cuda(), 64)
    assert torch.equal(I[:, :64], I64) and torch.equal(D[:, :64], D64)
    small = (IndexFlatIP if metric == "cosine" else IndexFlatL2)(d)
    small.add(torch.from_numpy(X[:90]).cuda())
    Ds, Is = small.search(torch.from_numpy(Q).cuda(), k)
    Dso, Iso = oracle.knn(metric, X[:90], Q, k)
    assert np.array_equal(Is.cpu().numpy(), Iso) and np.array_equal(Ds.cpu().numpy(), Dso)
    assert (Is[:, 90:] == -1).all()


def test_index_data_view_and_reconstruct(hip):
    from lemon_amd.index import IndexFlatIP
    x = torch.randn(50, 24, device="cuda")
    ix = IndexFlatIP(24)
    assert ix.data().shape == (0, 24)
    ix.add(x)
    assert torch.equal(ix.data(), x) and torch.equal(ix.reconstruct_n(10, 5), x[10:15])


# ---- edges of the five dedup kernels (inputs: tests/scanfx.py, their distinct-row counts: tests/test_scan_f32_edges_host.py) ----
def _on_off(hip, metric, X, Q, k):
    """search(Q, k) with dedup on and off -> (D, I, nq_distinct) of the folded handle; the two results are bit-identical and the
    unfolded handle searched every row"""
    from tests.indexfx import F32, bits_equal, cu, new_index
    on, off = new_index(hip, metric, X.shape[1], F32, X), new_index(hip, metric, X.shape[1], F32, X, dedup=False)
    qt = cu(Q)
    Da, Ia = on.search(qt, k)
    Db, Ib = off.search(qt, k)
    assert bits_equal(Ia, Ib), f"I differs in {int((Ia != Ib).sum())} places"
    assert bits_equal(Da, Db), "D differs"
    assert off.last_search_info()["nq_distinct"] == Q.shape[0] and on.last_search_info()["nq"] == Q.shape[0]
    return Da, Ia, on.last_search_info()["nq_distinct"]


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("nq", [1024, 1025, 1026, 1027])
@pytest.mark.parametrize("d", [1, 63, 65, 100])
def test_dedup_at_odd_widths_and_ragged_row_blocks(hip, oracle, metric, d, nq):
    """d % 64 != 0: a lane's second trip through the hash and compare loops (none for most lanes at d = 1); nq % 4 != 0: the
    `row >= n` guard inside a block of four rows"""
    from tests import scanfx as sx
    assert (d, nq) in [(a, b) for a in sx.DEDUP_WIDTHS for b in sx.DEDUP_NQS]
    X, Q = sx.dedup_db(d), sx.dedup_edge_queries(d, nq)
    D, I, distinct = _on_off(hip, metric, X, Q, sx.DEDUP_K)
    assert distinct == sx.DEDUP_PROTOS == 40
    sx.assert_bits(D, I, *oracle.knn(metric, X, Q, sx.DEDUP_K))


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_dedup_compares_bits_not_values(hip, oracle, metric):
    """rows one ulp apart, +0.0 against -0.0 (not merged; the results may be equal), permutations of one another, all-NaN rows
    of equal bits (merged: they get what the unfolded search gives them) and one of another payload (not merged)"""
    from tests import scanfx as sx
    Q, rows = sx.dedup_bit_queries()
    X = sx.dedup_db(sx.DEDUP_BITS_D)
    D, I, distinct = _on_off(hip, metric, X, Q, sx.DEDUP_K)
    assert distinct == len({r.tobytes() for r in Q}) == 8
    sx.assert_bits(D, I, *oracle.knn(metric, X, Q, sx.DEDUP_K))
    Ic = I.cpu()
    assert torch.equal(Ic[rows["zero_pos"][0]], Ic[rows["zero_neg"][0]])


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("distinct,folded", [(512, 512), (513, 1024)])
def test_dedup_folds_exactly_up_to_half_the_queries(hip, oracle, metric, distinct, folded):
    """the 2 U <= nq boundary at nq = 1024: 512 distinct rows fold, 513 do not"""
    from tests import scanfx as sx
    Q = sx.dedup_boundary_queries(distinct)
    X = sx.dedup_db(Q.shape[1])
    D, I, got = _on_off(hip, metric, X, Q, sx.DEDUP_K)
    assert got == folded
    sx.assert_bits(D, I, *oracle.knn(metric, X, Q, sx.DEDUP_K))
