"""GPU: the stage between the search and the score on every row-walk path -- k_neighbors_finalize and k_discrepancy
(lemon_amd/csrc/api.hip), the fp32 scan and the 16-bit filter at d % 4 != 0 (knn_f32.hip, knn_bf16.hip), the batched Brent
search k_grid_brent (gridf1.hip) at degenerate rows, and the row-alignment contract of the search entry points.

References: the CPU oracle (oracle.neighbors / discrepancy / knn: the chain numerics bit for bit), plain float64 numpy, and
scipy's fminbound through lemon_amd.metrics.  All shapes are tiny (databases and query sets of a few hundred rows).

Which case launches which kernel form (d % 4 == 0 -> the staged, wave-cooperative row walk; otherwise per-lane walks):

  k_neighbors_finalize<L2=false, STAGED=true>    test_neighbors_record_at_every_dimension[cosine-d],    d in STAGED_D
  k_neighbors_finalize<L2=true,  STAGED=true>    test_neighbors_record_at_every_dimension[euclidean-d], d in STAGED_D
  k_neighbors_finalize<L2=false, STAGED=false>   test_neighbors_record_at_every_dimension[cosine-d],    d in UNSTAGED_D
  k_neighbors_finalize<L2=true,  STAGED=false>   test_neighbors_record_at_every_dimension[euclidean-d], d in UNSTAGED_D
      chain_dist_wave: one fetching lane per row d = 4; one live lane in the second chunk d = 36, 68; ragged last chunk
      d = 28, 60, 100, 132; whole chunks d = 32, 96; 16 chunks d = 512
      idle lanes of the last workgroup (staged: shadow the last pair; unstaged: return early), nq * k = 1, 63, 64, 65, 127,
      128, 129: test_neighbors_record_around_the_workgroup_size
      -1 / +-FLT_MAX / NaN padding at an unstaged d: test_neighbors_record_padding_unstaged
      the text-side query de-duplication in front of both forms: test_neighbors_record_with_text_queries_folded
  k_discrepancy<STAGED=true>                     test_discrepancy_pair_loop[k-is_train-d], d in (36, 100)
  k_discrepancy<STAGED=false>                    test_discrepancy_pair_loop[k-is_train-d], d in (3, 33)
      pair loop: one iteration k = 4 (20 / 16 pairs); exactly one full iteration k = 8 div (64); two, the second ragged,
      k = 8 dis (72) and k = 8 train (81); exactly full iterations k = 31 train (1024 = 16 x 64) and k = 63 train (4096 =
      64 x 64); 63 iterations, the last ragged for div, k = 63 (4032 / 3969)
      j < 0 padding and the empty mean (NaN): test_discrepancy_padding_and_empty_mean
  fp32 scan at d % 4 != 0 (and the dpad boundaries 63 / 65, 127 / 129)    test_flat_search_fp32_scan_odd_dimensions
  16-bit filter + unstaged k_bf16_final at the same d                      test_bf16_filter_odd_dimensions
  k_grid_brent: loop never entered (constant row, N = 1), pos = 0, pos = N, ties, negative scores, lanes with one sample
      or none (N = 2, 63, 64, 65, 129): test_grid_f1_degenerate_rows; the num >= maxfun exit: test_grid_f1_maxfun_exit

Row alignment.  Reading every device function that receives a caller-owned query or embedding row:
  k_permute_rows, k_rowchain (rowwise.hip: lemon_paired_distance, the query norms), k_convert_bf16, k_row_hash,
  k_group_heads, k_gather_rows, hipMemcpy2DAsync in the AUTO probe                    scalar (or 32-bit) loads: any float pointer
  chain_dist, k_neighbors_finalize, k_discrepancy                                     test the pointers before a float4 load
  exact_score (knn_bf16.hip; three scan kernels call it with the caller's query row)  float4 on d % 4 == 0 alone
  k_bf16_final<.., STAGED = true> (stages the caller's query row into LDS)            float4 on d % 4 == 0 alone
So lemon_index_search, lemon_neighbors and lemon_discrepancy refuse query / embedding rows that are not 16-byte aligned when
d % 4 == 0 (LEMON_E_INVALID before any launch), ops.dev_f32 copies such a view, and lemon_paired_distance keeps taking any
float pointer (its kernel is scalar; tests/test_gpu_rowwise.py runs it 4 bytes off a boundary).  The tests below hold both
halves: views through the Python API give the bits of their aligned copies, the C entry points return the error code and
leave their outputs alone, and with d % 4 != 0 a 4-byte aligned pointer is served and gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests.synth import unit_rows
from tests.test_gpu_parity import BF16, _assert_knn_equal, _search, cu

pytestmark = pytest.mark.gpu

REC_KEYS = ("d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m", "I_n", "I_m")
UNSTAGED_D = (1, 2, 3, 5, 30, 33, 63, 65, 301)
STAGED_D = (4, 8, 28, 32, 36, 60, 68, 96, 100, 132, 512)
PROTO_TEXT_D = (2, 5, 33, 301, 8, 36, 100, 512)       # text side drawn from a few prototypes: ties in every text search
E_INVALID = -1


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _rows(rng, n, d, metric):
    """unit rows for cosine, rows scaled by a factor in [0.5, 2] for euclidean"""
    x = unit_rows(rng, n, d)
    if metric == "euclidean":
        x *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    return x


def _nb_inputs(metric, d, n_tr, nq, seed, proto_text, train_queries=False, C=7):
    rng = np.random.default_rng(seed)
    img_tr = _rows(rng, n_tr, d, metric)
    proto = _rows(rng, C, d, metric)
    lab_tr, lab_q = rng.integers(0, C, n_tr).astype(np.int32), rng.integers(0, C, nq).astype(np.int32)
    txt_tr = np.ascontiguousarray(proto[lab_tr]) if proto_text else _rows(rng, n_tr, d, metric)
    if train_queries:
        q_img, q_txt, lab_q = img_tr[:nq].copy(), txt_tr[:nq].copy(), lab_tr[:nq].copy()
    else:
        q_img = _rows(rng, nq, d, metric)
        q_txt = np.ascontiguousarray(proto[lab_q]) if proto_text else _rows(rng, nq, d, metric)
    return dict(img_tr=img_tr, txt_tr=txt_tr, q_img=q_img, q_txt=q_txt, lab_tr=lab_tr, lab_q=lab_q)


def _assert_record(got, ref, what=""):
    for key in REC_KEYS:
        g = got[key].cpu().numpy() if torch.is_tensor(got[key]) else got[key]
        assert g.dtype == ref[key].dtype and g.shape == ref[key].shape, (what, key)
        assert np.array_equal(g, ref[key], equal_nan=True), \
            f"{what} {key}: {int((~((g == ref[key]) | ((g != g) & (ref[key] != ref[key])))).sum())} of {g.size} differ"


def _assert_chain_within_float64_bound(metric, d, q_rows, tr_rows, I, dist, what):
    """An independent opinion on the chain contract the kernel and the oracle share: the float64 distance of the gathered
    rows, with the forward bound of a length-d fused chain.  cosine: d roundings of at most 2^-24 sum |a_k b_k| each, and one
    of 1 - acc (a value below 2: 2^-24).  euclidean: the difference, its square and the chain, (d + 2) 2^-24 relative to the
    sum of squares, with a factor two of room."""
    valid = I >= 0
    a = q_rows.astype(np.float64)[:, None, :]
    b = tr_rows.astype(np.float64)[np.where(valid, I, 0)]
    if metric == "cosine":
        exact = 1.0 - (a * b).sum(-1)
        bound = d * 2.0 ** -24 * np.abs(a * b).sum(-1) + 2.0 ** -24
    else:
        exact = ((a - b) ** 2).sum(-1)
        bound = (d + 2) * 2.0 ** -23 * exact
    err = np.abs(dist.astype(np.float64) - exact)
    assert np.all(err[valid] <= bound[valid]), (what, float((err[valid] / np.maximum(bound[valid], 1e-300)).max()))


# ---- 1. neighbour record ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", UNSTAGED_D + STAGED_D)
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_neighbors_record_at_every_dimension(hip, oracle, metric, d):
    k, n_tr, nq = 5, 150, 37                              # 185 pairs: two workgroups, the second 57 lanes wide
    c = _nb_inputs(metric, d, n_tr, nq, seed=1000 + d, proto_text=d in PROTO_TEXT_D)
    ref = oracle.neighbors(metric, c["img_tr"], c["txt_tr"], c["q_img"], c["q_txt"], k)
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric)
    got = db.neighbors(cu(c["q_img"]), cu(c["q_txt"]), k)
    assert np.array_equal(db.dists_tr.cpu().numpy(), ref["dists_tr"])
    _assert_record(got, ref, f"{metric} d={d}")
    _assert_chain_within_float64_bound(metric, d, c["q_txt"], c["txt_tr"], ref["I_n"], got["dists_n"].cpu().numpy(), "dists_n")
    _assert_chain_within_float64_bound(metric, d, c["q_img"], c["img_tr"], ref["I_m"], got["dists_m"].cpu().numpy(), "dists_m")


@pytest.mark.parametrize("d", [33, 36])
@pytest.mark.parametrize("drop_self,discrete", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_neighbors_record_drop_self_and_discrete(hip, oracle, metric, drop_self, discrete, d):
    k, n_tr, nq = 6, 150, 45
    c = _nb_inputs(metric, d, n_tr, nq, seed=2000 + d, proto_text=True, train_queries=drop_self)
    in_db = None
    if drop_self:
        in_db = np.ones(nq, np.uint8)
        in_db[::4] = 0                                    # a mask that mixes 0 and 1
    ref = oracle.neighbors(metric, c["img_tr"], c["txt_tr"], c["q_img"], c["q_txt"], k, drop_self=drop_self, in_db=in_db,
                           discrete=discrete, tr_label_id=c["lab_tr"], q_label_id=c["lab_q"])
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric, tr_label_id=c["lab_tr"])
    got = db.neighbors(cu(c["q_img"]), cu(c["q_txt"]), k, drop_self=drop_self, in_db=in_db, discrete=discrete,
                       q_label_id=c["lab_q"])
    _assert_record(got, ref, f"{metric} d={d} drop_self={drop_self} discrete={discrete}")


@pytest.mark.parametrize("d", [33, 36])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_neighbors_record_around_the_workgroup_size(hip, oracle, metric, d):
    # nq * k = 1, 63, 64, 65, 127, 128, 129 and 65 = 13 x 5 against the 128-thread workgroup: at d = 36 the idle lanes of the
    # last workgroup walk the last pair's rows with the others, at d = 33 they leave before the walk
    c = _nb_inputs(metric, d, 120, 129, seed=3000 + d, proto_text=False)
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric)
    for k, nq in [(1, 1), (1, 63), (1, 64), (1, 65), (1, 127), (1, 128), (1, 129), (5, 13)]:
        ref = oracle.neighbors(metric, c["img_tr"], c["txt_tr"], c["q_img"][:nq], c["q_txt"][:nq], k)
        got = db.neighbors(cu(c["q_img"][:nq]), cu(c["q_txt"][:nq]), k)
        _assert_record(got, ref, f"{metric} d={d} nq={nq} k={k}")


@pytest.mark.parametrize("n_tr,k,drop_self", [(3, 5, False), (5, 5, True), (1, 2, False), (2, 63, True)])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_neighbors_record_padding_unstaged(hip, oracle, metric, n_tr, k, drop_self):
    # n_tr < k + drop_self at d = 5: I = -1, D = -+FLT_MAX, NaN distances, exactly as the oracle pads
    nq = min(n_tr, 3) if drop_self else 4
    c = _nb_inputs(metric, 5, n_tr, nq, seed=4000 + n_tr, proto_text=False, train_queries=drop_self)
    in_db = np.array([1, 0, 1], np.uint8)[:nq] if drop_self else None
    ref = oracle.neighbors(metric, c["img_tr"], c["txt_tr"], c["q_img"], c["q_txt"], k, drop_self=drop_self, in_db=in_db)
    assert (ref["I_n"] == -1).any() and np.isnan(ref["dists_n"]).any() and np.isnan(ref["dists_tr_m"]).any()
    assert np.isin(np.abs(ref["D_n"][ref["I_n"] == -1]), np.float32(np.finfo(np.float32).max)).all()
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric)
    got = db.neighbors(cu(c["q_img"]), cu(c["q_txt"]), k, drop_self=drop_self, in_db=in_db)
    _assert_record(got, ref, f"{metric} n_tr={n_tr} k={k}")


@pytest.mark.parametrize("d", [33, 36])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_neighbors_record_with_text_queries_folded(hip, oracle, metric, d):
    # the query de-duplication starts at 1024 queries: 1030 text queries drawn from 7 prototypes are searched as 7
    k, n_tr, nq = 3, 150, 1030
    c = _nb_inputs(metric, d, n_tr, nq, seed=5000 + d, proto_text=True)
    ref = oracle.neighbors(metric, c["img_tr"], c["txt_tr"], c["q_img"], c["q_txt"], k)
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric)
    got = db.neighbors(cu(c["q_img"]), cu(c["q_txt"]), k)
    assert db.index_txt.last_search_info()["nq_distinct"] == len(np.unique(c["lab_q"]))
    assert db.index_img.last_search_info()["nq_distinct"] == nq
    _assert_record(got, ref, f"{metric} d={d} folded")


# ---- 2. discrepancy baselines ----------------------------------------------------------------------------------------------
METHODS = ("dis_x", "dis_y", "div_x", "div_y")


def _disc_texts(rng, n_tr, nq_max, d, C=6):
    """(database text, query text) twice: rows that are exact copies of a few prototypes, and the same rows jittered"""
    proto = unit_rows(rng, C, d)
    lab_tr, lab_q = rng.integers(0, C, n_tr), rng.integers(0, C, nq_max)

    def jitter(x):
        y = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
        return np.ascontiguousarray(y / np.linalg.norm(y, axis=1, keepdims=True), dtype=np.float32)

    dup = (np.ascontiguousarray(proto[lab_tr]), np.ascontiguousarray(proto[lab_q]))
    return {"duplicates": dup, "jittered": (jitter(dup[0]), jitter(dup[1]))}


def _assert_discrepancy(hip, oracle, db, img_tr, txt_tr, q_img, q_txt, k, is_train, what):
    """The device sums the oracle's float32 distances in float64 in another order (lane-strided, then a shuffle tree) and
    rounds once to float32: the two results are the roundings of float64 sums that differ by about pairs * 2^-53 relative,
    so they agree to one float32 ulp, and NaN (the empty mean) sits in the same places."""
    from lemon_amd.baselines import discrepancy_scores
    for method in METHODS:
        got = discrepancy_scores(db, cu(q_img), cu(q_txt), k, method, is_train=is_train).cpu().numpy()
        E, qv = (img_tr, q_img) if method.endswith("_x") else (txt_tr, q_txt)
        ref = oracle.discrepancy(method[:3], E, txt_tr, qv, q_txt, k, is_train)
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, method, "NaN positions")
        ok = ~np.isnan(ref)
        err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
        ulp = np.spacing(np.abs(ref[ok]).astype(np.float32)).astype(np.float64)
        assert np.all(err <= ulp), (what, method, float((err / ulp).max()))
    return ref


@pytest.mark.parametrize("d", [3, 33, 36, 100])
@pytest.mark.parametrize("k,is_train", [(4, False), (8, False), (8, True), (31, True), (63, False), (63, True)])
def test_discrepancy_pair_loop(hip, oracle, k, is_train, d):
    n_tr = 200
    rng = np.random.default_rng(6000 + 10 * k + d)
    img_tr, q_img_new = unit_rows(rng, n_tr, d), unit_rows(rng, 64, d)
    for kind, (txt_tr, q_txt_new) in _disc_texts(rng, n_tr, 64, d).items():
        db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
        for nq in (1, 7, 64):                             # one wave; an odd count (the last workgroup's second wave leaves)
            q_img, q_txt = (img_tr[:nq], txt_tr[:nq]) if is_train else (q_img_new[:nq], q_txt_new[:nq])
            _assert_discrepancy(hip, oracle, db, img_tr, txt_tr, q_img, q_txt, k, is_train, f"{kind} k={k} d={d} nq={nq}")


@pytest.mark.parametrize("d", [33, 36])
def test_discrepancy_padding_and_empty_mean(hip, oracle, d):
    rng = np.random.default_rng(7000 + d)
    # five rows, k = 8: the neighbour lists end in -1 (j < 0), and so do the rows of the second-order cache
    img_tr, txt_tr = unit_rows(rng, 5, d), unit_rows(rng, 5, d)
    q_img, q_txt = unit_rows(rng, 3, d), unit_rows(rng, 3, d)
    assert (oracle.knn("ip", txt_tr, q_txt, 8)[1] == -1).any()
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
    for is_train in (False, True):
        ref = _assert_discrepancy(hip, oracle, db, img_tr, txt_tr, q_img, q_txt, 8, is_train, f"n_tr=5 d={d}")
        assert np.isfinite(ref).all()
    # one row: its only second-order neighbour is itself and is removed -> the mean of nothing is NaN (dis); div stays finite
    db1 = hip.LemonDB(cu(img_tr[:1]), cu(txt_tr[:1]), "cosine")
    for k in (1, 8):
        assert np.isnan(oracle.discrepancy("dis", img_tr[:1], txt_tr[:1], q_img, q_txt, k, False)).all()
        assert np.isfinite(oracle.discrepancy("div", img_tr[:1], txt_tr[:1], q_img, q_txt, k, False)).all()
        _assert_discrepancy(hip, oracle, db1, img_tr[:1], txt_tr[:1], q_img, q_txt, k, False, f"n_tr=1 k={k} d={d}")


# ---- 3. flat search at d % 4 != 0 ------------------------------------------------------------------------------------------
ODD_D_CASES = [(70, 300, 1, 1), (130, 1000, 3, 7), (257, 1300, 5, 51), (260, 700, 33, 64), (129, 1025, 63, 51),
               (70, 513, 65, 64), (200, 300, 127, 7), (255, 1300, 129, 1), (100, 900, 301, 51)]


def _flat_case(metric, nq, n, d, k):
    rng = np.random.default_rng(nq * 7 + n * 3 + d + k)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    if metric == "l2":
        X *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        Q *= rng.uniform(0.5, 2.0, (nq, 1)).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq,n,d,k", ODD_D_CASES)
def test_flat_search_fp32_scan_odd_dimensions(hip, oracle, metric, nq, n, d, k):
    X, Q = _flat_case(metric, nq, n, d, k)
    D, I, idx = _search(hip, metric, X, Q, k, algo=1)
    assert idx.last_search_info()["algo"] == 1
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq,n,d,k", ODD_D_CASES)
def test_bf16_filter_odd_dimensions(hip, oracle, metric, nq, n, d, k):
    X, Q = _flat_case(metric, nq, n, d, k)
    D, I, idx = _search(hip, metric, X, Q, k, algo=BF16)
    assert idx.last_search_info()["algo"] == BF16
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


# ---- 4. grid-F1 at degenerate rows -----------------------------------------------------------------------------------------
GRID = [[0, 0, 0, 0, 0, 0], [5, 5, 0.1, 5, 0.1, 5], [1, 0, 1, 0, 0, 0], [0, 3, 0, 0, 1, 1], [100, 0, 10, 0, 10, 0]]


def _grid_rec(d_1, seed, k=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    N = len(d_1)
    rnd = lambda: torch.rand(N, k, generator=g, device="cuda")
    return {"d_1": cu(np.asarray(d_1, np.float32)), "D_n": -rnd(), "dists_tr_n": rnd(), "dists_n": rnd(), "D_m": -rnd(),
            "dists_tr_m": rnd(), "dists_m": rnd()}


def _grid_cases():
    rng = np.random.default_rng(8)
    u = lambda n: rng.random(n).astype(np.float32)
    yb = lambda n: rng.random(n) < 0.4
    cases = {"constant": (np.full(50, 0.3, np.float32), yb(50)),
             "one sample, positive": (u(1), np.array([True])),
             "one sample, negative": (u(1), np.array([False])),
             "no positives": (u(100), np.zeros(100, bool)),
             "all positives": (u(100), np.ones(100, bool)),
             "four distinct scores": (rng.choice(np.array([0, .25, .5, .75], np.float32), 200), yb(200)),
             "negative scores": (-1.0 - u(100), yb(100))}
    for n in (2, 63, 64, 65, 129):
        cases[f"N={n}"] = (u(n), yb(n))
    return cases


GRID_CASES = _grid_cases()


@pytest.mark.parametrize("name", list(GRID_CASES))
def test_grid_f1_degenerate_rows(hip, name):
    from lemon_amd import metrics as M, ops
    d_1, y = GRID_CASES[name]
    rec = _grid_rec(d_1, seed=len(d_1))
    f1, thres, scores = ops.grid_f1(rec, y, GRID, return_scores=True)
    assert np.array_equal(scores[0], d_1.astype(np.float64)), "hp = 0: the score row is d_1 itself"
    for j, hp in enumerate(GRID):
        assert np.array_equal(scores[j], ops.lemon_score(rec, dict(zip(M.HP_NAMES, hp))).cpu().numpy())
        ref_f1, ref_t = M.optimize_f1_efficient(y, scores[j], return_thres=True)
        assert np.isfinite(ref_f1) and np.isfinite(ref_t)
        assert f1[j] == ref_f1 and thres[j] == ref_t, (name, j, f1[j], ref_f1, thres[j], ref_t)


@pytest.mark.parametrize("maxfun", [1, 2, 5])
def test_grid_f1_maxfun_exit(hip, maxfun):
    # scipy counts the evaluation at the first point, enters the loop, evaluates once more and only then tests num >= maxfun
    from scipy.optimize import fminbound
    from lemon_amd import metrics as M, ops
    rng = np.random.default_rng(9)
    y = rng.random(300) < 0.4
    rec = _grid_rec((rng.random(300) + 0.2 * y).astype(np.float32), seed=300)
    f1, thres, scores = ops.grid_f1(rec, y, GRID, maxfun=maxfun, return_scores=True)
    full = ops.grid_f1(rec, y, GRID)
    for j in range(len(GRID)):
        s = scores[j]
        neg = lambda t: -M.f1_binary(y, s >= t)
        x = fminbound(neg, s.min(), s.max(), xtol=1e-8, maxfun=maxfun, disp=0)
        assert thres[j] == x and f1[j] == -neg(x), (maxfun, j, thres[j], x, f1[j], -neg(x))
    assert not np.array_equal(thres, full[1]), "the limit did not cut the search short"


# ---- 5. row alignment ------------------------------------------------------------------------------------------------------
def _off_by_one(a):
    """the array on the GPU as a view that starts at element 1 of a flat buffer: 4 bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((1 + t.numel() + 3,), float("nan"), dtype=torch.float32, device="cuda")
    buf[1:1 + t.numel()] = t.reshape(-1).cuda()
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _same_bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sentinel(shape, dtype):
    return torch.full(shape, -12345, dtype=dtype, device="cuda")


def _intact(*outs):
    torch.cuda.synchronize()
    return all(bool((o == -12345).all()) for o in outs)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_views_off_a_16_byte_boundary_give_the_bits_of_their_aligned_copies(hip, metric):
    from lemon_amd.baselines import discrepancy_scores
    k, d = 5, 64
    c = _nb_inputs(metric, d, 150, 70, seed=9000, proto_text=False)
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric)
    db_v = hip.LemonDB(_off_by_one(c["img_tr"]), _off_by_one(c["txt_tr"]), metric)
    assert _same_bits(db.dists_tr, db_v.dists_tr)
    want = db.neighbors(cu(c["q_img"]), cu(c["q_txt"]), k)
    for name, dbx, qi, qt in [("both queries", db, _off_by_one(c["q_img"]), _off_by_one(c["q_txt"])),
                              ("q_img only", db, _off_by_one(c["q_img"]), cu(c["q_txt"])),
                              ("q_txt only", db, cu(c["q_img"]), _off_by_one(c["q_txt"])),
                              ("database", db_v, cu(c["q_img"]), cu(c["q_txt"]))]:
        got = dbx.neighbors(qi, qt, k)
        for key in REC_KEYS:
            assert _same_bits(got[key], want[key]), (name, key)
    for algo in (1, BF16):
        idx = (hip.IndexFlatIP if metric == "cosine" else hip.IndexFlatL2)(d)
        idx.set_algo(algo)
        idx.add(_off_by_one(c["img_tr"]))
        D, I = idx.search(cu(c["q_img"]), k)
        Dv, Iv = idx.search(_off_by_one(c["q_img"]), k)
        assert _same_bits(D, Dv) and _same_bits(I, Iv) and _same_bits(I, want["I_n"]), algo
    assert _same_bits(hip.paired_distance(metric, _off_by_one(c["q_img"]), cu(c["q_txt"])), want["d_1"])
    if metric == "cosine":
        for method in METHODS:
            a = discrepancy_scores(db, cu(c["q_img"]), cu(c["q_txt"]), k, method)
            b = discrepancy_scores(db_v, _off_by_one(c["q_img"]), _off_by_one(c["q_txt"]), k, method)
            assert _same_bits(a, b), method


def _neighbors_c(lib, db, q_img, q_txt, nq, k, outs):
    d1, Dn, dn, trn, In, Dm, dm, trm, Im = outs
    return lib.lemon_neighbors(db.index_img._h, db.index_txt._h, _p(db.dists_tr), _p(q_img), _p(q_txt), nq, k, 0, None, 0, None,
                               None, _p(d1), _p(Dn), _p(dn), _p(trn), _p(In), _p(Dm), _p(dm), _p(trm), _p(Im), _stream())


def _neighbor_outs(nq, k):
    f, i = (lambda *s: _sentinel(s, torch.float32)), (lambda *s: _sentinel(s, torch.int64))
    return [f(nq), f(nq, k), f(nq, k), f(nq, k), i(nq, k), f(nq, k), f(nq, k), f(nq, k), i(nq, k)]


def test_c_entry_points_refuse_rows_off_a_16_byte_boundary(hip):
    from lemon_amd import _lib as L
    lib = L.load()
    k, d, nq = 5, 64, 70
    c = _nb_inputs("cosine", d, 150, nq, seed=9100, proto_text=False)
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), "cosine")
    qi, qt, qi_v, qt_v, E_v = cu(c["q_img"]), cu(c["q_txt"]), _off_by_one(c["q_img"]), _off_by_one(c["q_txt"]), _off_by_one(c["img_tr"])

    def refused(rc):
        return rc == E_INVALID and b"16-byte aligned" in lib.lemon_last_error()

    for algo in (0, 1, BF16):
        db.index_img.set_algo(algo)
        D, I = _sentinel((nq, k), torch.float32), _sentinel((nq, k), torch.int64)
        assert refused(lib.lemon_index_search(db.index_img._h, _p(qi_v), nq, k, _p(D), _p(I), _stream())), algo
        assert _intact(D, I), algo
    db.index_img.set_algo(0)
    for name, a, b in [("q_img", qi_v, qt), ("q_txt", qi, qt_v), ("both", qi_v, qt_v)]:
        outs = _neighbor_outs(nq, k)
        assert refused(_neighbors_c(lib, db, a, b, nq, k, outs)), name
        assert _intact(*outs), name
    for method in (0, 1):
        for name, E, qv, q in [("E_tr", E_v, qi, qt), ("qv", db.img, qi_v, qt), ("q_txt", db.img, qi, qt_v)]:
            out = _sentinel((nq,), torch.float32)
            assert refused(lib.lemon_discrepancy(method, db.index_txt._h, _p(E), _p(qv), _p(q), nq, k, 0, _p(out), _stream())), (method, name)
            assert _intact(out), (method, name)
    # the same handles still serve aligned rows afterwards
    outs = _neighbor_outs(nq, k)
    assert _neighbors_c(lib, db, qi, qt, nq, k, outs) == 0
    want = db.neighbors(qi, qt, k)
    assert _same_bits(outs[0], want["d_1"]) and _same_bits(outs[4], want["I_n"]) and _same_bits(outs[6], want["dists_m"])
    # lemon_paired_distance reads scalars: it takes the view at d % 4 == 0 and gives the aligned call's bits
    out = _sentinel((nq,), torch.float32)
    assert lib.lemon_paired_distance(L.METRIC_IP, _p(qi_v), _p(qt), nq, d, _p(out), _stream()) == 0
    assert _same_bits(out, want["d_1"])


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_c_entry_points_serve_any_float_pointer_when_d_is_no_multiple_of_four(hip, metric):
    # d = 33: every kernel walks rows one float at a time, and rows of 132 bytes are off a 16-byte boundary anyway
    from lemon_amd import _lib as L
    lib = L.load()
    k, d, nq = 5, 33, 70
    c = _nb_inputs(metric, d, 150, nq, seed=9200, proto_text=False)
    db = hip.LemonDB(cu(c["img_tr"]), cu(c["txt_tr"]), metric)
    qi, qt, qi_v, qt_v = cu(c["q_img"]), cu(c["q_txt"]), _off_by_one(c["q_img"]), _off_by_one(c["q_txt"])
    want = db.neighbors(qi, qt, k)
    for name, a, b in [("q_img", qi_v, qt), ("both", qi_v, qt_v)]:
        outs = _neighbor_outs(nq, k)
        assert _neighbors_c(lib, db, a, b, nq, k, outs) == 0, (name, lib.lemon_last_error())
        for key, o in zip(("d_1", "D_n", "dists_n", "dists_tr_n", "I_n", "D_m", "dists_m", "dists_tr_m", "I_m"), outs):
            assert _same_bits(o, want[key]), (name, key)
    for algo in (1, BF16):
        db.index_img.set_algo(algo)
        Dw, Iw = db.index_img.search(qi, k)
        D, I = _sentinel((nq, k), torch.float32), _sentinel((nq, k), torch.int64)
        assert lib.lemon_index_search(db.index_img._h, _p(qi_v), nq, k, _p(D), _p(I), _stream()) == 0, algo
        assert _same_bits(D, Dw) and _same_bits(I, Iw), algo
