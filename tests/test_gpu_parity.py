"""GPU parity tests: HIP path (through the C ABI) vs the CPU oracle on the same seeded inputs.

Bar: bit-exact D / I for the flat search (integer + chain-numerics float), bit-exact per-sample
arrays for the neighbour quantities, 1e-9 relative for the float64 score aggregation.
"""
import numpy as np
import pytest
import torch

from tests.synth import planted, unit_rows

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_library_loaded_in_process(hip):
    maps = open("/proc/self/maps").read()
    assert "liblemon_hip.so" in maps


@pytest.mark.parametrize("n,d", [(1, 1), (7, 33), (300, 512), (1000, 768), (257, 100)])
def test_normalize_rows(hip, oracle, n, d):
    rng = np.random.default_rng(n * 1000 + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.01, 30, (n, 1))).astype(np.float32)
    if n > 5:
        x[3] = 0.0  # zero row -> zeros (F.normalize eps semantics)
    y = hip.normalize_vectors(cu(x)).cpu().numpy()
    ref = oracle.normalize_rows(x)
    assert np.array_equal(y, ref), f"max abs diff {np.abs(y - ref).max()}"
    tref = torch.nn.functional.normalize(torch.from_numpy(x), p=2, dim=1).numpy()
    assert np.abs(y - tref).max() <= 2e-7


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,d", [(1, 8), (130, 40), (1000, 512), (333, 768)])
def test_paired_distance(hip, oracle, metric, n, d):
    rng = np.random.default_rng(d + n)
    a, b = unit_rows(rng, n, d), unit_rows(rng, n, d)
    got = hip.paired_distance(metric, cu(a), cu(b)).cpu().numpy()
    assert np.array_equal(got, oracle.paired_distance(metric, a, b))


def _search(hip, metric, X, Q, k, algo=None):
    cls = hip.IndexFlatIP if metric == "ip" else hip.IndexFlatL2
    idx = cls(X.shape[1] if X.ndim == 2 and X.shape[0] else Q.shape[1])
    if algo is not None:
        idx.set_algo(algo)
    if X.shape[0]:
        idx.add(cu(X))
    D, I = idx.search(cu(Q), k)
    return D.cpu().numpy(), I.cpu().numpy(), idx


def _assert_knn_equal(got, ref):
    (D, I), (Dr, Ir) = got, ref
    assert np.array_equal(I, Ir), f"{(I != Ir).sum()} index mismatches of {I.size}"
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), f"max |dD| {np.abs(D - Dr).max()}"


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq,n,d,k", [
    (1, 1, 8, 1), (5, 3, 16, 5), (130, 1000, 40, 10), (128, 128, 32, 64), (257, 1300, 64, 51),
    (64, 5000, 512, 50), (300, 2049, 768, 5), (1100, 3000, 100, 1), (33, 40000, 96, 51),
    # balanced decomposition: workgroup ranges that cross panel boundaries, 1-3 pieces per panel
    (700, 128 * 37, 64, 20), (900, 5000, 48, 33), (70000, 1500, 32, 10), (66000, 128 * 9, 40, 64),
])
def test_flat_search_bit_exact(hip, oracle, metric, nq, n, d, k):
    rng = np.random.default_rng(nq * 7 + n * 3 + d + k)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    if metric == "l2":  # IndexFlatL2 is a general index: exercise non-unit norms too
        X *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        Q *= rng.uniform(0.5, 2.0, (nq, 1)).astype(np.float32)
    D, I, _ = _search(hip, metric, X, Q, k)
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_flat_search_ties_lower_index_wins(hip, oracle, metric):
    # CIFAR text side: every DB row is one of C prototypes => the whole top-k is ties
    rng = np.random.default_rng(5)
    C, n, d, k = 10, 4000, 64, 51
    proto = unit_rows(rng, C, d)
    lab = rng.integers(0, C, n)
    X = proto[lab]
    Q = proto[rng.integers(0, C, 300)]
    D, I, _ = _search(hip, metric, X, Q, k)
    Dr, Ir = oracle.knn(metric, X, Q, k)
    _assert_knn_equal((D, I), (Dr, Ir))
    # the tie rule itself: within equal D, indices ascend
    same = D[:, 1:] == D[:, :-1]
    assert (I[:, 1:][same] > I[:, :-1][same]).all()


def test_flat_search_all_rows_identical(hip, oracle):
    # adversarial: every candidate ties, every tile passes the filter until the list is full
    X = np.tile(unit_rows(np.random.default_rng(1), 1, 48), (1500, 1))
    Q = unit_rows(np.random.default_rng(2), 70, 48)
    D, I, _ = _search(hip, "ip", X, Q, 20)
    assert np.array_equal(I, np.tile(np.arange(20), (70, 1)))
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, 20))


def test_flat_search_ascending_scores_worst_case(hip, oracle):
    # database sorted so that every later row beats all earlier ones: maximal list churn
    rng = np.random.default_rng(3)
    d, n = 32, 3000
    q = unit_rows(rng, 1, d)
    noise = unit_rows(rng, n, d)
    t = np.linspace(0.0, 1.0, n, dtype=np.float32)[:, None]
    X = (t * q + (1 - t) * 0.1 * noise).astype(np.float32)
    Q = np.repeat(q, 129, axis=0)
    D, I, _ = _search(hip, "ip", X, Q, 50)
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, 50))


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_flat_search_padding_and_empty(hip, oracle, metric):
    rng = np.random.default_rng(9)
    X, Q = unit_rows(rng, 3, 16), unit_rows(rng, 4, 16)
    D, I, idx = _search(hip, metric, X, Q, 6)       # k > ntotal -> faiss-style padding
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, 6))
    assert (I[:, 3:] == -1).all()
    assert idx.ntotal == 3 and idx.d == 16
    D0, I0 = idx.search(cu(Q[:0]), 3)                # empty query batch
    assert D0.shape == (0, 3) and I0.shape == (0, 3)
    De, Ie, _ = _search(hip, metric, X[:0], Q, 2)    # empty index
    assert (Ie == -1).all()


def test_flat_search_incremental_add_and_numpy_io(hip, oracle):
    rng = np.random.default_rng(11)
    X, Q = unit_rows(rng, 700, 64), unit_rows(rng, 90, 64)
    idx = hip.IndexFlatIP(64)
    idx.add(X[:100]); idx.add(X[100:513]); idx.add(X[513:])     # appends, numpy in
    D, I = idx.search(Q, 7)                                      # numpy in -> numpy out (faiss contract)
    assert isinstance(D, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, 7))
    with pytest.raises(AssertionError):
        idx.add(X.astype(np.float64))
    with pytest.raises(ValueError):
        idx.search(Q, 0)


def test_flat_search_cifar_scale(hip, oracle):
    # C2 shape: 5 000 val queries x 40 000 DB x 512, k+1 = 51
    rng = np.random.default_rng(21)
    X, Q = unit_rows(rng, 40000, 512), unit_rows(rng, 2048, 512)
    D, I, idx = _search(hip, "ip", X, Q, 51)
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, 51))
    info = idx.last_search_info()
    assert info["n"] == 40000 and info["k"] == 51 and info["grid"] >= 256


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("drop_self,discrete", [(False, False), (True, False), (False, True), (True, True)])
def test_neighbors_record_bit_exact(hip, oracle, metric, drop_self, discrete):
    k = 5
    s = planted(seed=0, n_tr=2048, n_q=256, d=64, C=16)
    img_tr, txt_tr, _, noisy_tr = s["train"]
    if drop_self:   # train split: queries ARE (mostly) DB rows; a few are not in the DB subset
        q_img, q_txt, noisy_q = img_tr[:300].copy(), txt_tr[:300].copy(), noisy_tr[:300]
        in_db = np.ones(300, np.uint8)
        in_db[::7] = 0
    else:
        q_img, q_txt, _, noisy_q = s["query"]
        in_db = None
    ref = oracle.neighbors(metric, img_tr, txt_tr, q_img, q_txt, k, drop_self=drop_self, in_db=in_db,
                           discrete=discrete, tr_label_id=noisy_tr, q_label_id=noisy_q)
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), metric, tr_label_id=noisy_tr)
    got = db.neighbors(cu(q_img), cu(q_txt), k, drop_self=drop_self, in_db=in_db, discrete=discrete,
                       q_label_id=noisy_q)
    assert np.array_equal(db.dists_tr.cpu().numpy(), ref["dists_tr"])
    for key in ("I_n", "I_m", "d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m"):
        g = got[key].cpu().numpy()
        assert np.array_equal(g, ref[key]), f"{key}: {(g != ref[key]).sum()} mismatches"
    # score aggregation (K5) on the device arrays vs the oracle, fixed hparams of train_clip_from_scratch.py:102-109
    hp = dict(beta=5, gamma=5, tau_1_n=0.1, tau_2_n=5, tau_1_m=0.1, tau_2_m=5)
    sc = hip.lemon_score(got, hp).cpu().numpy()
    sref = oracle.score(ref, hp)
    assert np.allclose(sc, sref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n_tr,n_q,k,drop_self", [(3, 4, 5, False), (4, 4, 5, True), (1, 3, 1, False), (70, 9, 63, True), (64, 5, 64, False)])
def test_neighbors_record_padding_and_extreme_k(hip, oracle, metric, n_tr, n_q, k, drop_self):
    # k (+1 on the train split) larger than the DB: -1 / +-FLT_MAX / NaN padding exactly as the oracle; k at
    # the LEMON_MAX_K limit; single-row DB
    rng = np.random.default_rng(n_tr * 100 + k)
    img_tr, txt_tr = unit_rows(rng, n_tr, 24), unit_rows(rng, n_tr, 24)
    if drop_self:
        q_img, q_txt = img_tr[:n_q].copy(), txt_tr[:n_q].copy()
    else:
        q_img, q_txt = unit_rows(rng, n_q, 24), unit_rows(rng, n_q, 24)
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), metric)
    rec = db.neighbors(cu(q_img), cu(q_txt), k, drop_self=drop_self)
    ref = oracle.neighbors(metric, img_tr, txt_tr, q_img, q_txt, k, drop_self=drop_self)
    for key in ("d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m", "I_n", "I_m"):
        assert np.array_equal(rec[key].cpu().numpy(), ref[key], equal_nan=True), key


def test_d1_normalized(hip, oracle):
    s = planted(seed=4, n_tr=10, n_q=300, d=64, C=100)
    q_img, _, _, noisy = s["query"]
    for metric in ("cosine", "euclidean"):
        got = hip.d1_normalized(metric, cu(q_img), cu(s["proto"]), torch.from_numpy(noisy)).cpu().numpy()
        ref = oracle.d1_normalized(metric, q_img, s["proto"], noisy)
        assert np.abs(got - ref).max() <= 1e-6


def test_cpu_tensor_is_refused(hip):
    with pytest.raises(Exception):
        hip.normalize_vectors(torch.zeros(4, 4))


# ------------------------------------------------------------------ bf16 filter + exact re-rank (LEMON_ALGO_BF16_FILTER)
BF16 = 2


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq,n,d,k", [
    (1, 1, 8, 1), (5, 3, 16, 5), (130, 1000, 40, 10), (128, 128, 32, 64), (257, 1300, 64, 51),
    (64, 5000, 512, 50), (300, 2049, 768, 5), (1100, 3000, 100, 1), (33, 40000, 96, 51), (700, 9000, 72, 64),
    (150, 3000, 1000, 10), (40, 700, 800, 3),      # d > 768: streaming bf16 kernel (queries not register-resident)
    (70, 900, 30, 7), (65, 600, 301, 9),           # d % 4 != 0: k_bf16_final re-scores with per-lane row walks (no staging)
])
def test_bf16_filter_bit_exact(hip, oracle, metric, nq, n, d, k):
    rng = np.random.default_rng(nq * 7 + n * 3 + d + k)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    if metric == "l2":
        X *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        Q *= rng.uniform(0.5, 2.0, (nq, 1)).astype(np.float32)
    D, I, idx = _search(hip, metric, X, Q, k, algo=BF16)
    assert idx.last_search_info()["algo"] == BF16
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


@pytest.mark.parametrize("qs4", ["1", "0"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq,n,d,k", [(300, 2049, 768, 5), (64, 5000, 512, 50), (513, 1300, 300, 51), (1000, 9000, 700, 64),
                                       (257, 63, 768, 10), (130, 129, 400, 64), (700, 20000, 768, 51), (256, 64 * 7 + 1, 512, 64), (300, 3000, 768, 1),
                                       (1025, 64 * 9, 640, 2)])
def test_bf16_two_block_kernel_forced_on_small_shapes(hip, oracle, monkeypatch, metric, nq, n, d, k, qs4):
    # k_scan_f16_qs4 (16x16x32 MFMAs, round 5; LEMON_QS4=0: its predecessor k_scan_bf16_qs2) normally serves >= 196 608 queries;
    # LEMON_QS2_MIN_PANELS=0 puts the oracle-sized cases through them:
    # ragged last panel (nq % 256), database tails (n % 64, n < 64), database splits with merge, pitches 512 and 768
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    monkeypatch.setenv("LEMON_QS4", qs4)
    rng = np.random.default_rng(nq * 7 + n * 3 + d + k)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    if metric == "l2":
        X *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
        Q *= rng.uniform(0.5, 2.0, (nq, 1)).astype(np.float32)
    D, I, idx = _search(hip, metric, X, Q, k, algo=BF16)
    info = idx.last_search_info()
    assert info["algo"] == BF16 and info["query_panel"] == 256
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_bf16_filter_ties_and_clusters(hip, oracle, metric):
    # prototypes (exact duplicates) + tight clusters whose spread is far below the bf16 band:
    # the filter cannot separate them, only the exact re-rank can
    rng = np.random.default_rng(17)
    C, n, d, k = 12, 6000, 128, 51
    proto = unit_rows(rng, C, d)
    lab = rng.integers(0, C, n)
    X = proto[lab].copy()
    jitter = rng.standard_normal((n, d)).astype(np.float32) * 1e-4
    X[n // 2:] += jitter[n // 2:]                      # half exact duplicates, half 1e-4-perturbed
    Q = proto[rng.integers(0, C, 260)] + rng.standard_normal((260, d)).astype(np.float32) * 1e-3
    Q = Q.astype(np.float32)
    D, I, _ = _search(hip, metric, X, Q, k, algo=BF16)
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


@pytest.mark.parametrize("qs4", ["1", "0"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_bf16_two_block_kernel_ties_and_clusters(hip, oracle, monkeypatch, metric, qs4):
    # the band-overflow path (exact compaction on the spot) and the all-ties path of k_scan_f16_qs4 / k_scan_bf16_qs2: duplicates +
    # clusters far tighter than the bf16 band at pitch 512, every row of the ascending-score worst case admitted at pitch 768
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    monkeypatch.setenv("LEMON_QS4", qs4)
    rng = np.random.default_rng(19)
    C, n, d, k = 12, 6000, 400, 51
    proto = unit_rows(rng, C, d)
    X = proto[rng.integers(0, C, n)].copy()
    X[n // 2:] += rng.standard_normal((n - n // 2, d)).astype(np.float32) * 1e-4
    Q = (proto[rng.integers(0, C, 300)] + rng.standard_normal((300, d)).astype(np.float32) * 1e-3).astype(np.float32)
    D, I, idx = _search(hip, metric, X, Q, k, algo=BF16)
    assert idx.last_search_info()["query_panel"] == 256
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))
    base = unit_rows(rng, 1, 768)[0]
    X = (base[None, :] * np.linspace(0.2, 1.0, 64 * 50, dtype=np.float32)[:, None]).astype(np.float32)
    Q = (base[None, :] * np.linspace(0.5, 1.5, 300, dtype=np.float32)[:, None]).astype(np.float32)
    D, I, _ = _search(hip, "ip", X, Q, k, algo=BF16)
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, k))


def test_bf16_filter_unnormalised_and_wide_dynamic_range(hip, oracle):
    rng = np.random.default_rng(23)
    n, d, k = 5000, 200, 20
    X = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
    Q = (rng.standard_normal((150, d)) * np.exp(rng.uniform(-3, 3, (150, 1)))).astype(np.float32)
    for metric in ("ip", "l2"):
        D, I, _ = _search(hip, metric, X, Q, k, algo=BF16)
        _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


def test_bf16_filter_equals_f32_scan_at_cifar_scale(hip):
    # size-independent property at a size the oracle would need minutes for: the two GPU algorithms
    # (independent inner products: bf16 MFMA + re-rank vs fp32 MFMA) agree bit for bit
    g = torch.Generator(device="cuda").manual_seed(5)
    X = hip.normalize_vectors(torch.randn(40000, 512, generator=g, device="cuda"))
    Q = hip.normalize_vectors(torch.randn(20000, 512, generator=g, device="cuda"))
    out = []
    for algo in (1, BF16):
        idx = hip.IndexFlatIP(512)
        idx.set_algo(algo)
        idx.add(X)
        out.append(idx.search(Q, 51))
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][0], out[1][0])


def test_disagreements_with_an_independent_fp32_search_are_near_ties(hip):
    # round-4 verdict: against an independent float32 search (torch.mm + top-k: blocked summation order) 2 % of the rows of the
    # bench's sample have another neighbour SET than the exact-chain scan.  SURVEY 7 predicted it (near-ties vs summation order);
    # this shows it: at the headline shape (40 000 x 512, k = 50, embeddings with planted class structure so that near-ties
    # exist) every differing row is adjudicated in float64 over the whole DB -- the rows in dispute are closer than float32 noise.
    from oracle import reference_loop as rl
    g = torch.Generator(device="cuda").manual_seed(11)
    n, nq, d, k, C = 40000, 4096, 512, 50, 100
    proto = hip.normalize_vectors(torch.randn(C, d, generator=g, device="cuda"))
    lab = torch.randint(0, C, (n + nq,), generator=g, device="cuda")
    E = hip.normalize_vectors(proto[lab] + 0.005 * torch.randn(n + nq, d, generator=g, device="cuda"))    # tight clusters: crowded top-k
    X, Q = E[:n].contiguous(), E[n:].contiguous()
    idx = hip.IndexFlatIP(d)
    idx.add(X)
    D, I = idx.search(Q, k)
    s32 = Q @ X.t()                                            # an independent float32 product (library GEMM)
    It = torch.topk(s32, k, dim=1).indices
    rep = rl.adjudicate_near_ties(Q.cpu().numpy(), X.cpu().numpy(), I.cpu().numpy(), It.cpu().numpy(), "cosine")
    print("near-tie adjudication:", rep)
    assert rep["rows_differing"] > 0, "the planted clusters must produce near-ties (else this test shows nothing)"
    assert rep["max_gap_at_swap"] <= 2e-6, rep
    # neither float32 search is the float64 truth on such rows; the exact-chain scan must not be the worse one by more than noise
    assert rep["rows_a_equals_f64_set"] >= rep["rows_b_equals_f64_set"] - 0.01, rep


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_headline_size_fp32_scan_independent_of_work_decomposition(hip, oracle, metric):
    # BASELINE configs[1] shape (50 000 queries x 40 000 x 512, k+1 = 51): the balanced decomposition cuts the
    # panels x tiles space differently for 50 000 queries (510 workgroups, pieces merged per panel) than for a
    # 1 000-query subset; both must agree bit for bit, and the subset agrees with the oracle
    rng = np.random.default_rng(77)
    X, Q = unit_rows(rng, 40000, 512), unit_rows(rng, 50000, 512)
    Xg, Qg = torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda()
    idx = hip.IndexFlatIP(512) if metric == "ip" else hip.IndexFlatL2(512)
    idx.set_algo(1)
    idx.add(Xg)
    D, I = idx.search(Qg, 51)
    sub = torch.arange(0, 50000, 50, device="cuda")
    Ds, Is = idx.search(Qg[sub].contiguous(), 51)
    assert torch.equal(I[sub], Is) and torch.equal(D[sub], Ds)
    Dr, Ir = oracle.knn(metric, X, Q[::50][:200], 51)
    assert np.array_equal(Is[:200].cpu().numpy(), Ir) and np.array_equal(Ds[:200].cpu().numpy().view(np.uint32), Dr.view(np.uint32))


def test_full_size_1m_self_join_bf16_rows_equal_f32_scan(hip):
    # BASELINE configs[3] at full size (1 000 000 x 768, k+1 = 51): the bf16 filter scan over ALL queries
    # (chunked database, state carried between launches) must reproduce, bit for bit, what the exact fp32
    # scan returns for a strided subset of the queries -- the size-independent property that ties the
    # full-size run to the oracle-checked small cases
    n, d, k = 1_000_000, 768, 51
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.empty((n, d), device="cuda")
    for i in range(0, n, 100_000):
        x[i:i + 100_000].normal_(generator=g)
    x = hip.normalize_vectors(x)
    idx = hip.IndexFlatIP(d)
    idx.set_algo(2)
    idx.add(x)
    D, I = idx.search(x, k)
    assert idx.last_search_info()["algo"] == 2
    sub = torch.arange(0, n, 123, device="cuda")[:8192]
    assert torch.equal(I[sub, 0], sub)                         # self is its own nearest neighbour
    ref = hip.IndexFlatIP(d)
    ref.set_algo(1)
    ref.add(x)
    Dr, Ir = ref.search(x[sub].contiguous(), k)
    assert torch.equal(I[sub], Ir) and torch.equal(D[sub], Dr)


@pytest.mark.parametrize("algo,bad", [(BF16, "2"), (BF16, "16"), (BF16, "junk"), (1, "64"), (1, "-1"), (1, "4")])
def test_unknown_ablate_bits_are_refused_before_any_launch(hip, monkeypatch, algo, bad):
    # round 2's recorded GPU fault: a working-tree diagnostic skipped list maintenance on LEMON_ABLATE=2 and the
    # lane-private half-lists (256 entries) ran 1 MiB past the candidate workspace.  Diagnostic knobs are now
    # validated (no kernel is launched on an unknown bit) and the append slot is clamped (knn_common.hpp append_slot)
    from lemon_amd._lib import LemonHipError
    rng = np.random.default_rng(3)
    X, Q = unit_rows(rng, 3000, 64), unit_rows(rng, 200, 64)
    idx = hip.IndexFlatIP(64)
    idx.set_algo(algo)
    idx.add(cu(X))
    monkeypatch.setenv("LEMON_ABLATE", bad)
    with pytest.raises(LemonHipError, match="LEMON_ABLATE"):
        idx.search(cu(Q), 10)
    monkeypatch.delenv("LEMON_ABLATE")
    D, I = idx.search(cu(Q), 10)                      # the index is still usable afterwards
    assert I.shape == (200, 10) and int(I.min()) >= 0


@pytest.mark.parametrize("algo", [1, BF16])
def test_half_lists_at_capacity_ascending_scores_every_row_admitted(hip, oracle, algo):
    # the append-pressure worst case: scores ascend with the row index, so EVERY row beats the running k-th best and each
    # lane appends its full 64 entries per tile -- the half-lists sit exactly at their `full` bound (192 + 64 = 256)
    # tile after tile; D / I stay bit-exact and nothing is written beyond a list
    n, d, k = 128 * 40, 64, 51
    rng = np.random.default_rng(5)
    base = unit_rows(rng, 1, d)[0]
    X = (base[None, :] * np.linspace(0.2, 1.0, n, dtype=np.float32)[:, None]).astype(np.float32)
    Q = (base[None, :] * np.linspace(0.5, 1.5, 300, dtype=np.float32)[:, None]).astype(np.float32)
    D, I, _ = _search(hip, "ip", X, Q, k, algo=algo)
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, k))


def test_neighbors_record_bf16_algo(hip, oracle):
    s = planted(seed=1, n_tr=3000, n_q=300, d=64, C=16)
    img_tr, txt_tr, _, noisy_tr = s["train"]
    q_img, q_txt, _, noisy_q = s["query"]
    ref = oracle.neighbors("cosine", img_tr, txt_tr, q_img, q_txt, 10)
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine", algo=BF16)
    got = db.neighbors(cu(q_img), cu(q_txt), 10)
    for key in ("I_n", "I_m", "d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m"):
        assert np.array_equal(got[key].cpu().numpy(), ref[key]), key


@pytest.mark.parametrize("d,nq,metric", [(64, 131072 + 77, "ip"), (300, 196608 + 77, "ip"), (768, 196608 + 300, "ip"), (768, 196608 + 300, "l2")])
def test_bf16_filter_chunked_database_state_carry(hip, oracle, monkeypatch, d, nq, metric):
    # >= 1024 query panels -> one launch per Infinity-Cache-sized database chunk with the per-query
    # state carried between launches; force tiny chunks (8 tiles) so several launches happen.
    # d = 64: one query block per wave (k_scan_bf16_qs); d = 300 / 768 from 768 panels of 256 queries on: two blocks per
    # wave (k_scan_bf16_qs2, 64-row tiles, two states per lane; at 768 part of block 1 is parked in LDS)
    monkeypatch.setenv("LEMON_CHUNK_MB", "0.01")
    g = torch.Generator(device="cuda").manual_seed(9)
    X = hip.normalize_vectors(torch.randn(5000, d, generator=g, device="cuda"))
    Q = hip.normalize_vectors(torch.randn(nq, d, generator=g, device="cuda"))
    out = []
    for algo in (1, BF16):
        idx = (hip.IndexFlatIP if metric == "ip" else hip.IndexFlatL2)(d)
        idx.set_algo(algo)
        idx.add(X)
        out.append(idx.search(Q, 51))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0])
    Dr, Ir = oracle.knn(metric, X.cpu().numpy(), Q[:512].cpu().numpy(), 51)
    assert np.array_equal(out[1][1][:512].cpu().numpy(), Ir)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_ragged_query_rest_behind_whole_round_chunks_uses_the_split_kernel(hip, oracle, monkeypatch, metric):
    # 1 M queries leave a ragged rest of 67 panels behind the whole-round chunks; since round 5 it goes through k_scan_f16_qs4 with
    # the database split between a few workgroups per panel (lemon_search_bf16: rest_splits) and k_merge.  Scaled down: with 256
    # panels as the QS2 / QS4 entry, 94 536 queries = one whole round of 256 panels + a rest of 114 panels (x 2 splits at 20 000 rows).
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "256")
    d, n, nq = 512, 20000, 256 * 256 + 29000
    g = torch.Generator(device="cuda").manual_seed(21)
    X = hip.normalize_vectors(torch.randn(n, d, generator=g, device="cuda"))
    Q = hip.normalize_vectors(torch.randn(nq, d, generator=g, device="cuda"))
    if metric == "l2":
        X = X * (0.5 + 1.5 * torch.rand(n, 1, generator=g, device="cuda"))
    out = []
    for algo in (1, BF16):
        idx = (hip.IndexFlatIP if metric == "ip" else hip.IndexFlatL2)(d)
        idx.set_algo(algo)
        idx.add(X)
        out.append(idx.search(Q, 51))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0])
    rows = torch.cat([torch.arange(0, 256), torch.arange(nq - 256, nq)])
    Dr, Ir = oracle.knn(metric, X.cpu().numpy(), Q[rows.cuda()].cpu().numpy(), 51)
    assert np.array_equal(out[1][1][rows.cuda()].cpu().numpy(), Ir)


def test_auto_picks_bf16_on_spread_data_and_f32_on_band_crowded_data(hip):
    g = torch.Generator(device="cuda").manual_seed(3)
    n, nq, d = 65536, 131072, 64
    spread = hip.normalize_vectors(torch.randn(n, d, generator=g, device="cuda"))
    q = hip.normalize_vectors(torch.randn(nq, d, generator=g, device="cuda"))
    proto = hip.normalize_vectors(torch.randn(10, d, generator=g, device="cuda"))
    crowded = proto[torch.randint(0, 10, (n,), generator=g, device="cuda")]       # class-prompt style duplicates
    crowded_q = proto[torch.randint(0, 10, (nq,), generator=g, device="cuda")]
    for X, Q, expect in ((spread, q, 2), (crowded, crowded_q, 1)):   # expect: LEMON_ALGO_BF16_FILTER / LEMON_ALGO_F32_MFMA
        auto = hip.IndexFlatIP(d)
        auto.add(X)
        Da, Ia = auto.search(Q, 10)
        assert auto.last_search_info()["algo"] == expect
        ref = hip.IndexFlatIP(d)
        ref.set_algo(1)
        ref.add(X)
        Dr, Ir = ref.search(Q, 10)
        assert torch.equal(Ia, Ir) and torch.equal(Da, Dr)


def test_tiny_encoder_gpu_vs_cpu(hip):
    from lemon_amd.clip import ClipConfig, LemonCLIP
    m = LemonCLIP(ClipConfig.named("tiny")).eval()
    px = torch.randn(9, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    ids = torch.randint(1, 290, (9, 16), generator=torch.Generator().manual_seed(2))
    ids[:, 7] = 299
    ci, ct = m.encode_image(px), m.encode_text(ids)
    mg = LemonCLIP(ClipConfig.named("tiny")).eval().cuda()
    gi, gt = mg.encode_image(px.cuda()).cpu(), mg.encode_text(ids.cuda()).cpu()
    assert (gi - ci).abs().max() < 1e-4 and (gt - ct).abs().max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("N,k", [(700, 5), (5000, 50), (63, 1)])
def test_grid_f1_batch_bit_identical_to_host_loop(hip, N, k):
    # lemon_grid_f1 (scores + bounded-Brent threshold search per grid point on the GPU) vs the host loop
    # K5 -> numpy -> scipy.fminbound that maximize_metric runs per grid point (lib/metrics/utils.py:151-196,286-296)
    from lemon_amd import metrics as M, ops
    g = torch.Generator(device="cuda").manual_seed(N + k)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda")
    y = (rnd(N) < 0.4).cpu().numpy()
    rec = {"d_1": rnd(N) + torch.as_tensor(y, device="cuda") * 0.2, "D_n": -rnd(N, k), "dists_tr_n": rnd(N, k),
           "dists_n": rnd(N, k), "D_m": -rnd(N, k), "dists_tr_m": rnd(N, k), "dists_m": rnd(N, k)}
    rng = np.random.default_rng(0)
    hps = [[0, 0, 0, 0, 0, 0], [5, 5, 0.1, 5, 0.1, 5], [100, 0, 10, 0, 10, 0], [0, 100, 0, 10, 0, 10], [1, 1, 1, 1, 1, 1]]
    hps += [list(rng.choice([0, 5, 10, 50, 100], 2)) + list(rng.choice([0, 1, 5, 10], 4)) for _ in range(120)]
    hps += [[1e308, 1e308, 800, 800, 800, 800]]                     # overflows to inf/nan scores: objective 0
    f1, thres, scores = ops.grid_f1(rec, y, hps, return_scores=True)
    for j, hp in enumerate(hps):
        s = ops.lemon_score(rec, dict(zip(M.HP_NAMES, hp))).cpu().numpy()
        assert np.array_equal(s, scores[j], equal_nan=True), f"scores differ at grid point {j}"
        if not np.all(np.isfinite(s)):
            assert f1[j] == 0.0
            continue
        ref_f1, ref_t = M.optimize_f1_efficient(y, s, return_thres=True)
        assert f1[j] == ref_f1 and thres[j] == ref_t, (j, hp, f1[j], ref_f1, thres[j], ref_t)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(32, 32), (48, 64), (300, 200), (500, 375), (37, 91), (224, 224), (640, 480), (225, 224)])
def test_gpu_preprocess_bit_identical_to_pil_pipeline(hip, h, w):
    # lemon_preprocess_u8 vs generic_transform (PIL bicubic resize -> center crop -> /255 -> normalise)
    from PIL import Image
    from lemon_amd.data import generic_transform, gpu_transform_batch
    rng = np.random.default_rng(h * 1000 + w)
    imgs = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    ref = torch.stack([generic_transform(Image.fromarray(im), 224) for im in imgs])
    got = gpu_transform_batch(torch.from_numpy(imgs).cuda(), 224).cpu()
    assert got.shape == ref.shape == (3, 3, 224, 224)
    assert torch.equal(got, ref), (got - ref).abs().max()
    # patch-major variant: same values where the patch-embedding GEMM expects them
    pm = gpu_transform_batch(torch.from_numpy(imgs).cuda(), 224, patch=32).cpu()
    expect = ref.view(3, 3, 7, 32, 7, 32).permute(0, 2, 4, 1, 3, 5).reshape(3, 49, 3 * 32 * 32)
    assert torch.equal(pm, expect)
    # an output size that is not a multiple of 4 (the kernel's one-pixel-per-lane form), with and without patches
    if min(h, w) >= 30:
        ref30 = torch.stack([generic_transform(Image.fromarray(im), 30) for im in imgs])
        assert torch.equal(gpu_transform_batch(torch.from_numpy(imgs).cuda(), 30).cpu(), ref30)
        pm30 = gpu_transform_batch(torch.from_numpy(imgs).cuda(), 30, patch=6).cpu()
        assert torch.equal(pm30, ref30.view(3, 3, 5, 6, 5, 6).permute(0, 2, 4, 1, 3, 5).reshape(3, 25, 3 * 36))


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,H,causal", [
    (3, 50, 12, False), (2, 77, 8, True), (5, 8, 8, True), (1, 197, 12, False), (1, 257, 16, False),
    (2, 1, 2, False), (2, 33, 3, True), (2, 64, 2, True), (1, 288, 1, True),
])
def test_fused_attention_matches_float64_reference(hip, B, L, H, causal):
    # lemon_attention_f32 on the packed qkv projection vs softmax(q k^T / 8 [+ causal]) v in float64
    from lemon_amd.ops import attention
    W = 64 * H
    qkv = torch.randn(B, L, 3 * W, generator=torch.Generator().manual_seed(B * 1000 + L)) * 1.5
    q, k, v = qkv.double().view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, W)
    got = attention(qkv.cuda().contiguous(), H, causal).cpu().double()
    assert got.shape == ref.shape
    assert (got - ref).abs().max() < 2e-5, (got - ref).abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,H,causal", [(2, 65, 3, False), (3, 77, 8, True), (2, 197, 12, False), (1, 257, 16, False), (2, 288, 2, True),
                                           (1, 256, 4, True), (2, 96, 1, False)])
def test_long_sequence_attention_kernels_agree_bit_for_bit(hip, B, L, H, causal):
    # 64 < L <= 288, split-fp16 arithmetic: k_attention_hd64_f16 (K and V split once at staging, V read transposed by
    # ds_read_b64_tr_b16, Q and the output through LDS) against the first general kernel (lemon_attention_set_f16(2)): same
    # arithmetic in the same order, so every output form must hold the same bits
    from lemon_amd import _lib
    from lemon_amd.ops import attention, attention_split, attention_t
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * 1000 + L)
    qkv = (torch.randn(B, L, 3 * H * 64, generator=g) * 1.5).cuda()
    prev = lib.lemon_attention_set_f16(1)
    try:
        new = (attention(qkv, H, causal), attention_split(qkv, H, causal, "f16x3"), attention_split(qkv, H, causal, "bf16x6"), attention_t(qkv, H, causal))
        lib.lemon_attention_set_f16(2)
        old = (attention(qkv, H, causal), attention_split(qkv, H, causal, "f16x3"), attention_split(qkv, H, causal, "bf16x6"), attention_t(qkv, H, causal))
    finally:
        lib.lemon_attention_set_f16(prev)
    rows = (B * L + 127) // 128 * 128
    for i, (a, b) in enumerate(zip(new, old)):
        if i == 3:      # tile-major operand: rows beyond B*L are uninitialised in both
            from lemon_amd.ops import unpack_act_t
            a, b = unpack_act_t(a, B * L, H * 64), unpack_act_t(b, B * L, H * 64)
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))


@pytest.mark.parametrize("B,L,H,causal", [(3, 50, 12, False), (5, 8, 8, True), (2, 77, 8, True), (2, 197, 12, False)])
def test_attention_split_output_equals_split_of_attention(hip, B, L, H, causal):
    # lemon_attention_split3 / _f16x3 store the split of exactly the values lemon_attention_f32 stores (all three kernels)
    from lemon_amd.ops import attention, attention_split, split_operand
    g = torch.Generator().manual_seed(B * 100 + L)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g).cuda()
    for scheme in ("bf16x6", "f16x3"):
        assert torch.equal(attention_split(qkv, H, causal, scheme), split_operand(attention(qkv, H, causal), scheme)), scheme


@pytest.mark.parametrize("B,L,H,causal", [(3, 50, 12, False), (5, 8, 8, True), (2, 77, 8, True), (2, 197, 12, False), (7, 33, 4, False)])
def test_attention_tile_major_operand_equals_split_of_attention(hip, B, L, H, causal):
    # lemon_attention_f16x3t: the tile-major operand of the hand-written GEMM holds exactly the fp16 split of lemon_attention_f32
    from lemon_amd.ops import attention, attention_t, split_operand, unpack_act_t
    g = torch.Generator().manual_seed(B * 100 + L)
    qkv = torch.randn(B, L, 3 * H * 64, generator=g).cuda()
    y3 = split_operand(attention(qkv, H, causal), "f16x3").view(B * L, 3, H * 64)
    assert torch.equal(unpack_act_t(attention_t(qkv, H, causal), B * L, H * 64), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0))


def test_f16x3_parts_and_layernorm_split_equals_layernorm_then_split(hip):
    # lemon_split_f16x3: activation rows [hi | hi | lo 2^11], weight rows [hi | lo | hi 2^-11] of w * wscale, hi = RNE f16,
    # lo = the exact fp32 remainder; |v - hi - lo| <= 2^-23 |v| inside the fp16 range; beyond it the parts are not finite
    from lemon_amd.ops import layer_norm, layer_norm_split, split_operand, weight_scale_f16x3
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(37, 96, generator=g) * torch.exp(torch.randn(37, 1, generator=g) * 2)).cuda()
    x[3, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, 1e-3, 4097.5])
    xd = x.double().cpu()
    y = split_operand(x, "f16x3").view(37, 3, 96).cpu()
    hi = x.cpu().to(torch.float16)
    assert torch.equal(y[:, 0], hi) and torch.equal(y[:, 1], hi)
    assert torch.equal(y[:, 2], ((x.cpu() - hi.float()) * 2048.0).to(torch.float16))
    err = (y[:, 0].double() + y[:, 2].double() / 2048.0 - xd).abs()
    assert bool((err <= xd.abs() * 2.0 ** -23 + 2.0 ** -36).all()), err.max()          # (+ half an fp16 subnormal step / 2^11)
    w = (torch.randn(64, 96, generator=g) * 0.02).cuda()
    ws = weight_scale_f16x3(w)
    assert 2.0 ** 14 <= float(w.abs().max()) * ws < 2.0 ** 15
    yw = split_operand(w, "f16x3", weight=True, wscale=ws).view(64, 3, 96).cpu()
    sw = w.cpu() * ws
    whi = sw.to(torch.float16)
    assert torch.equal(yw[:, 0], whi) and torch.equal(yw[:, 1], (sw - whi.float()).to(torch.float16))
    assert torch.equal(yw[:, 2], (whi.float() / 2048.0).to(torch.float16))
    big = torch.full((1, 8), 7.0e4).cuda()
    assert not bool(torch.isfinite(split_operand(big, "f16x3").float()).all())          # loud, not clamped
    lw, lb = torch.randn(96, generator=g).cuda(), torch.randn(96, generator=g).cuda()
    assert torch.equal(layer_norm_split(x, lw, lb, 1e-5, "f16x3"), split_operand(layer_norm(x, lw, lb), "f16x3"))
    x8 = torch.randn(5, 768, generator=g).cuda()                                         # the 16-byte-store kernel
    l8, b8 = torch.randn(768, generator=g).cuda(), torch.randn(768, generator=g).cuda()
    assert torch.equal(layer_norm_split(x8, l8, b8, 1e-5, "f16x3"), split_operand(layer_norm(x8, l8, b8), "f16x3"))


def test_split3_parts_are_exact_and_layernorm_split_equals_layernorm_then_split(hip):
    # lemon_split3_f32: v = hi + mid + lo in bf16 with exact differences (24 significant bits); both operand layouts;
    # lemon_layernorm_split3 == lemon_layernorm_f32 followed by the split, bit for bit
    from lemon_amd.ops import layer_norm, layer_norm_split3, split3
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(37, 96, generator=g) * torch.exp(torch.randn(37, 1, generator=g) * 3)).cuda()
    x[3, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1e-38, 65504.0])
    for weight, order in ((False, (0, 0, 1, 0, 1, 2)), (True, (0, 1, 0, 2, 1, 0))):
        y = split3(x, weight=weight).view(37, 6, 96).float().double().cpu()
        parts = [y[:, order.index(i)] for i in range(3)]                      # hi, mid, lo
        for seg, which in enumerate(order):
            assert torch.equal(y[:, seg], parts[which])
        err = (parts[0] + parts[1] + parts[2] - x.double().cpu()).abs()
        assert bool((err <= x.double().cpu().abs() * 2.0 ** -24 + 1e-40).all()), err.max()      # (+ one bf16 subnormal step)
        assert torch.equal(parts[0].float(), x.cpu().to(torch.bfloat16).float())                       # hi = RNE bf16(x)
    w, b = torch.randn(96, generator=g).cuda(), torch.randn(96, generator=g).cuda()
    assert torch.equal(layer_norm_split3(x, w, b), split3(layer_norm(x, w, b)))


@pytest.mark.parametrize("m,n,k", [(100, 64, 48), (7, 512, 512), (3000, 2304, 768), (2500, 768, 3072), (5000, 1536, 512), (1, 32, 40)])
@pytest.mark.parametrize("mode", ["plain", "bias", "bias_gelu", "bias_residual"])
@pytest.mark.parametrize("scheme", ["bf16x6", "f16x3"])
def test_split_bf16x3_linear_is_at_least_as_accurate_as_the_fp32_gemm(hip, m, n, k, mode, scheme):
    # lemon_linear_bf16x6 / lemon_linear_f16x3 against float64: the emulation must meet the bar of the fp32 GEMM test below AND
    # be no worse than the fp32 GEMM itself on the same operands (measured: bf16x6 ~50x better)
    from lemon_amd.ops import linear, linear_split, split_operand, weight_scale_f16x3
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k)
    x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g) if "bias" in mode else None
    r = torch.randn(m, n, generator=g) if "residual" in mode else None
    ref = x.double() @ w.double().T
    if b is not None:
        ref = ref + b.double()
    if "gelu" in mode:
        ref = ref * torch.sigmoid(1.702 * ref)
    if r is not None:
        ref = ref + r.double()
    ws = weight_scale_f16x3(w) if scheme == "f16x3" else 1.0
    x6, w6 = split_operand(x.cuda(), scheme), split_operand(w.cuda(), scheme, weight=True, wscale=ws)
    bc, rc = (None if b is None else b.cuda()), (None if r is None else r.cuda())
    if "gelu" in mode:
        got = linear_split(x6, w6, 1.702 * bc, None, "silu", alpha=1.702 / ws).cpu().double() / 1.702
        f32 = linear(x.cuda(), w.cuda(), 1.702 * bc, None, "silu", alpha=1.702).cpu().double() / 1.702
    else:
        got = linear_split(x6, w6, bc, rc, alpha=1.0 / ws).cpu().double()
        f32 = linear(x.cuda(), w.cuda(), bc, rc).cpu().double()
    e_split, e_f32 = float((got - ref).abs().max()), float((f32 - ref).abs().max())
    assert e_split < 2e-5 * max(1.0, k ** 0.5 / 8), e_split
    assert e_split <= 1.5 * e_f32 + 1e-6, (e_split, e_f32)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(100, 64, 48), (7, 512, 512), (3000, 2304, 768), (2500, 768, 3072), (1, 32, 40)])
@pytest.mark.parametrize("mode", ["plain", "bias", "bias_gelu", "gelu", "bias_residual", "residual"])
def test_fused_linear_matches_float64_reference(hip, m, n, k, mode):
    # lemon_linear_f32: y = act(alpha x W^T + b) (+ residual) in one hipBLASLt GEMM (SiLU epilogue)
    from lemon_amd.ops import linear
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k)
    x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g) if "bias" in mode else None
    r = torch.randn(m, n, generator=g) if "residual" in mode else None
    ref = x.double() @ w.double().T
    if b is not None:
        ref = ref + b.double()
    if "gelu" in mode:
        ref = ref * torch.sigmoid(1.702 * ref)
    if r is not None:
        ref = ref + r.double()
    if "gelu" in mode:      # QuickGELU(z) = silu(1.702 z) / 1.702 (how lemon_amd/clip.py composes it)
        got = linear(x.cuda(), w.cuda(), None if b is None else 1.702 * b.cuda(), None, "silu", alpha=1.702).cpu().double() / 1.702
    else:
        got = linear(x.cuda(), w.cuda(), None if b is None else b.cuda(), None if r is None else r.cuda()).cpu().double()
    assert got.shape == ref.shape
    assert (got - ref).abs().max() < 2e-5 * max(1.0, k ** 0.5 / 8), (got - ref).abs().max()


@pytest.mark.gpu
def test_encoder_vit_b32_block_fused_attention_vs_sdpa(hip):
    # one full-size transformer block (width 768, 12 heads, L=50): fused HIP attention vs torch SDPA path
    from lemon_amd.clip import Block, TowerConfig
    torch.manual_seed(0)
    blk = Block(TowerConfig(768, 1, 12, 3072), 1e-5).eval()
    x = torch.randn(4, 50, 768)
    with torch.no_grad():
        ref = blk(x, causal=False)                       # CPU: SDPA branch
        got = blk.cuda()(x.cuda(), causal=False).cpu()   # GPU, no grad: fused branch
    assert (got - ref).abs().max() < 1e-4


@pytest.mark.gpu
def test_patch_major_preprocess_feeds_patch_embedding_gemm(hip):
    # raw uint8 -> lemon_preprocess_u8(patch=P) -> GEMM patch embedding  ==  PIL transform -> Conv2d patch embedding
    from PIL import Image
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.data import generic_transform, gpu_transform_batch
    cfg = ClipConfig.named("tiny")                                   # 32x32 images, 8x8 patches
    m = LemonCLIP(cfg).eval().cuda()
    imgs = np.random.default_rng(5).integers(0, 256, (6, 40, 56, 3), dtype=np.uint8)
    px = torch.stack([generic_transform(Image.fromarray(im), cfg.image_size) for im in imgs]).cuda()
    patches = gpu_transform_batch(torch.from_numpy(imgs).cuda(), cfg.image_size, patch=cfg.patch_size)
    a, b = m.encode_image(px), m.encode_image(patches)
    assert a.shape == b.shape and (a - b).abs().max() < 1e-4


@pytest.mark.parametrize("arch,B,hw", [("vit-b-32", 37, (32, 32)), ("vit-b-16", 9, (40, 56))])
def test_preprocess_writes_the_patch_embedding_operand(hip, arch, B, hw):
    # lemon_preprocess_u8_f16x3t: the tile-major operand holds exactly the fp16 split of lemon_preprocess_u8's patch rows, and the
    # tower fed with it (patch embedding in the hand-written GEMM) gives the embeddings of the fp32 patch-major path
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.data import gpu_transform_batch
    from lemon_amd.ops import normalize_vectors, split_operand, unpack_act_t
    cfg = ClipConfig.named(arch)
    imgs = torch.from_numpy(np.random.default_rng(B).integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)).cuda()
    patches = gpu_transform_batch(imgs, cfg.image_size, patch=cfg.patch_size)
    po = gpu_transform_batch(imgs, cfg.image_size, patch=cfg.patch_size, operand=True)
    m_rows, K = B * po.n_patches, po.k
    assert patches.shape == (B, po.n_patches, K)
    y3 = split_operand(patches.reshape(m_rows, K), "f16x3").view(m_rows, 3, K)
    assert torch.equal(unpack_act_t(po.at, m_rows, K), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0))
    torch.manual_seed(3)
    model = LemonCLIP(cfg).eval().cuda()
    with torch.no_grad():
        a, b = normalize_vectors(model.encode_image(patches).float()), normalize_vectors(model.encode_image(po).float())
    assert bool(torch.isfinite(b).all()) and float((a - b).abs().max()) < 5e-6


def test_fused_split_scoring_equals_per_split_calls(hip, oracle):
    # pipeline.score_splits sends train (k+1, self-exclusion) and val/test (k) through ONE neighbours call
    from lemon_amd.pipeline import score_splits
    s = planted(seed=2, n_tr=1500, n_q=200, d=64, C=16)
    img_tr, txt_tr, _, noisy_tr = s["train"]
    q_img, q_txt, _, noisy_q = s["query"]
    in_db = np.ones(1500, np.uint8); in_db[::9] = 0
    for discrete in (False, True):
        db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine", tr_label_id=noisy_tr)
        recs = score_splits(db, [dict(name="train", img=cu(img_tr), txt=cu(txt_tr), drop_self=True, in_db=in_db, label_id=noisy_tr),
                                 dict(name="val", img=cu(q_img), txt=cu(q_txt), label_id=noisy_q)], 5, discrete=discrete)
        ref_tr = oracle.neighbors("cosine", img_tr, txt_tr, img_tr, txt_tr, 5, drop_self=True, in_db=in_db,
                                  discrete=discrete, tr_label_id=noisy_tr, q_label_id=noisy_tr)
        ref_va = oracle.neighbors("cosine", img_tr, txt_tr, q_img, q_txt, 5, discrete=discrete,
                                  tr_label_id=noisy_tr, q_label_id=noisy_q)
        for name, ref in (("train", ref_tr), ("val", ref_va)):
            for key in ("I_n", "I_m", "d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m"):
                assert np.array_equal(recs[name][key].cpu().numpy(), ref[key]), (name, key, discrete)


def test_our_metric_matches_sklearn_pairwise_diagonal(hip):
    # lib/metrics/distance_metrics.py:48-73 takes np.diagonal of sklearn's full pairwise matrices
    from sklearn.metrics.pairwise import cosine_similarity, euclidean_distances, manhattan_distances
    from lemon_amd.ops import our_metric
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((300, 96)) * 3).astype(np.float32)
    b = (rng.standard_normal((300, 96)) * 0.5).astype(np.float32)
    ref = {"cosine": 1 - np.diagonal(cosine_similarity(a, b)), "euclidean": np.diagonal(euclidean_distances(a, b)),
           "manhattan": np.diagonal(manhattan_distances(a, b))}
    for dist, r in ref.items():
        got = our_metric(cu(a), cu(b), dist).cpu().numpy()
        assert np.allclose(got, r, rtol=2e-5, atol=2e-5), dist


@pytest.mark.parametrize("is_train", [False, True])
def test_discrepancy_baselines_match_oracle(hip, oracle, is_train):
    from lemon_amd.baselines import discrepancy_scores
    s = planted(seed=6, n_tr=1200, n_q=150, d=48, C=12)
    img_tr, txt_tr, _, _ = s["train"]
    if is_train:
        q_img, q_txt = img_tr[:200], txt_tr[:200]
    else:
        q_img, q_txt, _, _ = s["query"]
    txt_j = (txt_tr + 0.05 * np.random.default_rng(0).standard_normal(txt_tr.shape)).astype(np.float32)
    txt_j /= np.linalg.norm(txt_j, axis=1, keepdims=True)        # captions: no exact duplicates
    for tr_txt in (txt_tr, txt_j):
        db = hip.LemonDB(cu(img_tr), cu(tr_txt), "cosine")
        for method in ("dis_x", "dis_y", "div_x", "div_y"):
            got = discrepancy_scores(db, cu(q_img), cu(q_txt), 4, method, is_train=is_train).cpu().numpy()
            E, qv = (img_tr, q_img) if method.endswith("_x") else (tr_txt, q_txt)
            ref = oracle.discrepancy(method[:3], E, tr_txt, qv, q_txt, 4, is_train)
            assert np.allclose(got, ref, rtol=1e-6, atol=1e-6, equal_nan=True), (method, np.abs(got - ref).max())


def test_cos_distance_topk_matches_reference_golden(hip):
    import os
    from lemon_amd.baselines import cos_distance_topk, count_knn_distribution
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "cosdistance_topk.npz"))
    vals, idx = cos_distance_topk(cu(g["feat"]), 6)
    assert np.array_equal(idx.cpu().numpy(), g["idx"])
    assert np.abs(vals.cpu().numpy() - g["vals"]).max() < 5e-7
    prob = count_knn_distribution(4, 0.0, cu(g["feat"]), np.arange(64) % 4, 6)
    assert prob.shape == (64, 4) and torch.allclose(prob.norm(dim=1), torch.ones(64, device="cuda"), atol=1e-5)


@pytest.mark.parametrize("algo", [1, BF16])
def test_flat_search_against_reference_second_opinion_n2048_k51(hip, algo):
    """lib/metrics/utils.py:198-214 (cosDistance + topk) and lib/metrics/distance_metrics.py:48-73 (sklearn euclidean)
    executed by tools/make_golden_knn.py: both scan kernels against the reference's own brute-force arithmetic."""
    from tests.test_oracle_golden import check_second_opinion

    def knn(metric, X, Q, k):
        D, I, _ = _search(hip, metric, X, Q, k, algo=algo)
        return D, I
    check_second_opinion(knn, lambda x: hip.normalize_vectors(cu(x)).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("dist", ["cosine", "euclidean", "manhattan"])
def test_clip_logits_confidence_matches_reference_golden(hip, dist):
    """Zero-shot CLIP-logits baseline (lib/baselines/train_zero_shot_clip_baseline.py:207-224): golden produced with the
    reference's own DistanceEvaluator.our_metric + scipy softmax (tools/make_golden.py -> zero_shot.npz)."""
    import os
    from lemon_amd.baselines import clip_logits_confidence
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "zero_shot.npz"))
    got = clip_logits_confidence(torch.from_numpy(g["img"]).cuda(), torch.from_numpy(g["cls"]).cuda(), g["lab"], dist).cpu().numpy()
    assert np.abs(got - g[f"conf_{dist}"]).max() <= 2e-6, np.abs(got - g[f"conf_{dist}"]).max()
    assert np.all((got > 0) & (got < 1))


@pytest.mark.gpu
@pytest.mark.parametrize("m,width,mlp", [(300, 256, 512), (129, 512, 2048), (5000, 768, 3072), (1, 256, 256)])
def test_fused_mlp_in_the_hand_written_gemm_matches_float64(hip, m, width, mlp):
    # gemm_f16x3.hip: LayerNorm -> tile-major operand -> fc1 (+ bias, QuickGELU, fp16 split in the epilogue, stored as fc2's
    # operand) -> fc2 (+ bias, residual) against the same chain in float64, and against the library path (lemon_linear_f16x3 +
    # split pass).  Rows beyond m of the tile-major operands are uninitialised memory: they must not reach a stored result.
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m * 13 + width)
    x = torch.randn(m, width, generator=g) * 2.0
    lw, lb = 1.0 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    w1, b1 = torch.randn(mlp, width, generator=g) / width ** 0.5, 0.1 * torch.randn(mlp, generator=g)
    w2, b2 = torch.randn(width, mlp, generator=g) / mlp ** 0.5, 0.1 * torch.randn(width, generator=g)
    s = ops.QUICK_GELU_SCALE
    xd = x.double()
    xn = torch.nn.functional.layer_norm(xd, (width,), lw.double(), lb.double(), 1e-5)
    z = xn @ w1.double().T + b1.double()
    hd = z * torch.sigmoid(s * z)
    ref = hd @ w2.double().T + b2.double() + xd
    xc, lwc, lbc = x.cuda(), lw.cuda(), lb.cuda()
    poison = torch.full((8 << 20,), float("nan"), device="cuda")        # (so that fresh allocations below are likely to hold NaNs)
    del poison
    s1, s2 = ops.weight_scale_f16x3(w1), ops.weight_scale_f16x3(w2)
    at = ops.layer_norm_t(xc, lwc, lbc, 1e-5)
    # the LayerNorm operand holds exactly the split of lemon_layernorm_f32's values
    y3 = ops.split_operand(ops.layer_norm(xc, lwc, lbc, 1e-5), "f16x3").view(m, 3, width)
    assert torch.equal(ops.unpack_act_t(at, m, width), y3[:, 0].float() + y3[:, 2].float() * (1.0 / 2048.0))
    ht = ops.linear_t(at, ops.pack_weight_t(w1.cuda(), s1), m, mlp, width, (b1 * s).cuda(), act="silu", alpha=s / s1)
    h_got = ops.unpack_act_t(ht, m, mlp).cpu().double() / s
    assert float((h_got - hd).abs().max()) < 2e-5 * max(1.0, width ** 0.5 / 8)
    got = ops.linear_t(ht, ops.pack_weight_t(w2.cuda(), s2), m, width, mlp, b2.cuda(), residual=xc, alpha=1.0 / (s * s2)).cpu().double()
    e_fused = float((got - ref).abs().max())
    assert torch.isfinite(got).all() and e_fused < 3e-5 * max(1.0, mlp ** 0.5 / 8), e_fused
    # the library path on the same inputs
    a3 = ops.layer_norm_split(xc, lwc, lbc, 1e-5, "f16x3")
    h = ops.linear_split(a3, ops.split_operand(w1.cuda(), "f16x3", weight=True, wscale=s1), (b1 * s).cuda(), act="silu", alpha=s / s1)
    lib = ops.linear_split(ops.split_operand(h, "f16x3"), ops.split_operand(w2.cuda(), "f16x3", weight=True, wscale=s2), b2.cuda(),
                           residual=xc, alpha=1.0 / (s * s2)).cpu().double()
    e_lib = float((lib - ref).abs().max())
    assert e_fused <= 2.0 * e_lib + 2e-6, (e_fused, e_lib)


def _heavy_tailed(shape, g, typical, big, frac):
    """N(0, typical) with a fraction `frac` of the entries multiplied up to magnitude ~big."""
    x = torch.randn(shape, generator=g) * typical
    mask = torch.rand(shape, generator=g) < frac
    return torch.where(mask, torch.randn(shape, generator=g) * big, x)


@pytest.mark.gpu
@pytest.mark.parametrize("m,width,mlp", [(700, 768, 3072), (300, 512, 2048)])
def test_split_gemms_on_real_checkpoint_statistics(hip, m, width, mlp):
    # what real CLIP checkpoints do to the f16x3 operands and the N(0, sigma) tests do not: rows that hold 1e3 next to 1e-4,
    # LayerNorm gains up to 30 in a few channels, weight tensors whose largest entries are 1e3 x the typical one (so that
    # wscale leaves the typical weight at 2^4 and its lo part near the fp16 subnormals), activations far below 2^-14 (fp16
    # subnormal hi AND lo parts).  Bar: the split GEMM's error against float64 is no worse than 1.5 x the fp32 GEMM's on the
    # same operands (relative to the largest output) -- through the library kernel (lemon_linear_f16x3) and through the
    # hand-written one (LayerNorm -> fc1 -> QuickGELU -> fc2 on tile-major operands, both MFMA shapes).
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m + width)
    # ---- library kernel on raw heavy-tailed operands ----
    x = _heavy_tailed((m, width), g, 1e-4, 1e3, 0.01)                      # 1e-4 typical, 1 % of the entries ~1e3
    x[:, 5] = 1e-7 * torch.randn(m, generator=g)                          # a channel of fp16-subnormal magnitudes
    w = _heavy_tailed((mlp, width), g, 0.02, 20.0, 0.0005)                  # max / typical ~ 1e3
    ref = x.double() @ w.double().T
    ws = ops.weight_scale_f16x3(w)
    got = ops.linear_split(ops.split_operand(x.cuda(), "f16x3"), ops.split_operand(w.cuda(), "f16x3", weight=True, wscale=ws),
                           alpha=1.0 / ws).cpu().double()
    f32 = ops.linear(x.cuda(), w.cuda()).cpu().double()
    scale = float(ref.abs().max())
    e_split, e_f32 = float((got - ref).abs().max()) / scale, float((f32 - ref).abs().max()) / scale
    assert torch.isfinite(got).all() and e_split <= 1.5 * e_f32 + 1e-6, (e_split, e_f32)
    # ---- hand-written kernel: LayerNorm with outlier gains -> fc1 (heavy-tailed W1) -> QuickGELU -> fc2 (+ residual) ----
    x = _heavy_tailed((m, width), g, 1.0, 40.0, 0.003)                       # outlier channels in the residual stream
    lw = 1.0 + 0.1 * torch.randn(width, generator=g)
    lw[torch.randperm(width, generator=g)[:6]] = torch.tensor([30.0, -25.0, 18.0, 30.0, 0.001, 1e-5])
    lb = 0.1 * torch.randn(width, generator=g)
    w1, b1 = _heavy_tailed((mlp, width), g, 0.03, 1.5, 0.0005), 0.1 * torch.randn(mlp, generator=g)
    w2, b2 = _heavy_tailed((width, mlp), g, 0.02, 1.0, 0.0005), 0.1 * torch.randn(width, generator=g)
    s = ops.QUICK_GELU_SCALE
    xd = x.double()
    xn = torch.nn.functional.layer_norm(xd, (width,), lw.double(), lb.double(), 1e-5)
    z = xn @ w1.double().T + b1.double()
    ref = (z * torch.sigmoid(s * z)) @ w2.double().T + b2.double() + xd
    xc, lwc, lbc = x.cuda(), lw.cuda(), lb.cuda()
    # the fp32 chain on the same inputs (lemon_layernorm_f32 + two lemon_linear_f32)
    h32 = ops.linear(ops.layer_norm(xc, lwc, lbc, 1e-5), w1.cuda(), (b1 * s).cuda(), act="silu", alpha=s)
    f32 = ops.linear(h32, w2.cuda(), b2.cuda(), residual=xc, alpha=1.0 / s).cpu().double()
    scale = float(ref.abs().max())
    e_f32 = float((f32 - ref).abs().max()) / scale
    s1, s2 = ops.weight_scale_f16x3(w1), ops.weight_scale_f16x3(w2)
    from lemon_amd import _lib
    lib_ = _lib.load()
    for shape in (16, 32):
        assert lib_.lemon_linear_f16x3t_set_mfma(shape) >= 0
        at = ops.layer_norm_t(xc, lwc, lbc, 1e-5)
        ht = ops.linear_t(at, ops.pack_weight_t(w1.cuda(), s1), m, mlp, width, (b1 * s).cuda(), act="silu", alpha=s / s1)
        got = ops.linear_t(ht, ops.pack_weight_t(w2.cuda(), s2), m, width, mlp, b2.cuda(), residual=xc, alpha=1.0 / (s * s2)).cpu().double()
        e_hand = float((got - ref).abs().max()) / scale
        assert torch.isfinite(got).all() and e_hand <= 1.5 * e_f32 + 1e-6, (shape, e_hand, e_f32)
    lib_.lemon_linear_f16x3t_set_mfma(0)


@pytest.mark.gpu
@pytest.mark.parametrize("m,width,mlp", [(720, 768, 3072), (320, 512, 2048)])
def test_folded_layernorm_chain_on_real_checkpoint_statistics(hip, m, width, mlp):
    # the DEFAULT encoder path (LEMON_LNFOLD=1, LEMON_MLP=block) on what real CLIP checkpoints produce -- the round-4 stress test
    # above goes through layer_norm_t -> linear_t, the UN-folded path.  Here: rowstats_t -> fold_layernorm_weight -> linear_t_ln
    # with both epilogues and the EMIT -> ln_finalize -> FOLD hand-over of a block chain:
    #     h = QuickGELU(LN1(x) W1^T + b1)            FOLD, SiLU -> operand epilogue     (mlp.fc1 behind layer_norm2)
    #     y = h W2^T + b2 + x                        EMIT: fp32 + residual, y as the next operand + row statistics (mlp.fc2)
    #     z = LN2(y) W3^T + b3                       FOLD, fp32 epilogue                (q/k/v_proj behind the next layer_norm1)
    # LayerNorm gains {30, -25, 18, 1e-3, 1e-5} folded into heavy-tailed weights, residual rows with 40 x ... 1000 x outlier
    # channels, rows at |mean| / sigma in {0.1, 1, 4, 7.9}.  Contract: the fold carries x instead of LN(x) in the split operand,
    # so its error may exceed the fp32 GEMM chain's by sqrt(1 + (mean / sigma)^2) of the row (<= 8.06 at the fold's bound, beyond
    # which the row is poisoned and re-embedded): bar = 1.5 e_f32 sqrt(1 + shift^2) + 1e-6 per row; the measured factor is printed.
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m + width + 5)
    x = _heavy_tailed((m, width), g, 1.0, 40.0, 0.003)
    x[:, 7] *= 25.0                                                         # one channel 1 000 x the typical magnitude in a few rows,
    x[:, 100] = 60.0 * torch.randn(m, generator=g)                          # one channel at 60 x in every row (CLIP's massive activations)
    want_shift = torch.tensor([0.1, 1.0, 4.0, 7.9])[torch.arange(m) % 4]
    x = x - x.mean(1, keepdim=True)
    x = x + (want_shift * x.std(1, unbiased=False))[:, None]
    def gains():
        lw = 1.0 + 0.1 * torch.randn(width, generator=g)
        lw[torch.randperm(width, generator=g)[:6]] = torch.tensor([30.0, -25.0, 18.0, 30.0, 1e-3, 1e-5])
        return lw, 0.1 * torch.randn(width, generator=g)
    g1, be1 = gains()
    g2, be2 = gains()
    w1, b1 = _heavy_tailed((mlp, width), g, 0.03, 1.5, 0.0005), 0.1 * torch.randn(mlp, generator=g)
    w2, b2 = _heavy_tailed((width, mlp), g, 0.02, 1.0, 0.0005), 0.1 * torch.randn(width, generator=g)
    w3, b3 = _heavy_tailed((3 * width, width), g, 0.03, 1.5, 0.0005), 0.1 * torch.randn(3 * width, generator=g)
    s, eps = ops.QUICK_GELU_SCALE, 1e-5
    xd = x.double()
    ln1 = torch.nn.functional.layer_norm(xd, (width,), g1.double(), be1.double(), eps)
    zz = ln1 @ w1.double().T + b1.double()
    y_ref = (zz * torch.sigmoid(s * zz)) @ w2.double().T + b2.double() + xd
    z_ref = torch.nn.functional.layer_norm(y_ref, (width,), g2.double(), be2.double(), eps) @ w3.double().T + b3.double()
    xc = x.cuda()
    c = lambda t: t.cuda()
    # the fp32 chain on the same inputs (LayerNorm kernel + fp32 library GEMMs)
    h32 = ops.linear(ops.layer_norm(xc, c(g1), c(be1), eps), c(w1), c(b1 * s), act="silu", alpha=s)
    y32 = ops.linear(h32, c(w2), c(b2), residual=xc, alpha=1.0 / s)
    z32 = ops.linear(ops.layer_norm(y32, c(g2), c(be2), eps), c(w3), c(b3)).cpu().double()
    y32 = y32.cpu().double()
    # the folded chain
    xt, aff = ops.rowstats_t(xc, eps)
    w1t, a1, cs1, b1p = ops.fold_layernorm_weight(c(w1), c(b1), c(g1), c(be1), s)
    ht = ops.linear_t_ln(xt, w1t, m, mlp, width, b1p, act="silu", alpha=s * a1, row_aff=aff, colsum=cs1)
    s2 = ops.weight_scale_f16x3(c(w2))
    y, yt, st = ops.linear_t_ln(ht, ops.pack_weight_t(c(w2), s2), m, width, mlp, c(b2), residual=xc, alpha=1.0 / (s * s2), emit=True)
    aff2 = ops.ln_finalize(st, m, width, eps)
    w3t, a3, cs3, b3p = ops.fold_layernorm_weight(c(w3), c(b3), c(g2), c(be2), 1.0)
    z = ops.linear_t_ln(yt, w3t, m, 3 * width, width, b3p, alpha=a3, row_aff=aff2, colsum=cs3).cpu().double()
    y = y.cpu().double()
    sh_x = xd.mean(1).abs() / torch.sqrt(xd.var(1, unbiased=False) + eps)
    sh_y = y_ref.mean(1).abs() / torch.sqrt(y_ref.var(1, unbiased=False) + eps)
    assert float((sh_x - want_shift.double()).abs().max()) < 1e-3
    near_x, near_y = sh_x < 0.999 * ops.LN_FOLD_MAX_SHIFT, sh_y < 0.999 * ops.LN_FOLD_MAX_SHIFT
    far_y = sh_y > 1.001 * ops.LN_FOLD_MAX_SHIFT
    assert bool(near_x.all()) and int((near_y & (want_shift.double() > 7.0)).sum()) > m // 16     # rows right below the bound are in
    assert bool(torch.isfinite(y).all())                                   # (every x row is inside the bound)
    assert bool(torch.isfinite(z[near_y]).all()) and not bool(torch.isfinite(z[far_y]).any())
    # y: fc1 folded (factor by the x row's shift), fc2 plain
    sy, sz = float(y_ref.abs().max()), float(z_ref.abs().max())
    e32_y, e32_z = float((y32 - y_ref).abs().max()), float((z32 - z_ref)[near_y].abs().max())
    ey = (y - y_ref).abs().max(1).values
    bar_y = 1.5 * e32_y * torch.sqrt(1.0 + sh_x ** 2) + 1e-6 * sy
    assert bool((ey <= bar_y).all()), (float((ey / bar_y).max()), e32_y / sy)
    # z: both folds behind it; a row's factor is the larger of its two shifts
    ez = (z - z_ref).abs().max(1).values[near_y]
    bar_z = (1.5 * e32_z * torch.sqrt(1.0 + torch.maximum(sh_x, sh_y) ** 2) + 1e-6 * sz)[near_y]
    assert bool((ez <= bar_z).all()), (float((ez / bar_z).max()), e32_z / sz)
    zero_mean = (want_shift < 0.5)
    print(f"fold stress m={m} width={width}: e_fold/e_f32  y: all rows {float(ey.max()) / e32_y:.2f}, |mean|/sigma <= 0.1 rows {float(ey[zero_mean].max()) / e32_y:.2f}; "
          f"z: all rows {float(ez.max()) / e32_z:.2f}, zero-mean rows {float((z - z_ref).abs().max(1).values[near_y & zero_mean].max()) / e32_z:.2f} "
          f"(e_f32 / max|ref|: y {e32_y / sy:.2e}, z {e32_z / sz:.2e}; factor allowed up to {float(torch.sqrt(1 + sh_y[near_y] ** 2).max()):.2f})")
    for _ in range(2):      # (bit-identical repeats: see the packed-multiply fault of round 4)
        again = ops.linear_t_ln(yt, w3t, m, 3 * width, width, b3p, alpha=a3, row_aff=aff2, colsum=cs3).cpu().double()
        assert torch.equal(again[near_y], z[near_y])


@pytest.mark.gpu
def test_hand_written_gemm_is_position_independent(hip):
    # identical rows in, identical rows out, wherever they sit in the batch (the text tower folds identical prompts)
    from lemon_amd import ops
    g = torch.Generator().manual_seed(3)
    row = torch.randn(1, 512, generator=g)
    x = row.repeat(1000, 1).cuda()
    lw, lb = torch.ones(512).cuda(), torch.zeros(512).cuda()
    w1 = (torch.randn(2048, 512, generator=g) / 512 ** 0.5).cuda()
    w2 = (torch.randn(512, 2048, generator=g) / 2048 ** 0.5).cuda()
    s1, s2 = ops.weight_scale_f16x3(w1), ops.weight_scale_f16x3(w2)
    ht = ops.linear_t(ops.layer_norm_t(x, lw, lb), ops.pack_weight_t(w1, s1), 1000, 2048, 512, None, act="silu", alpha=1.0 / s1)
    y = ops.linear_t(ht, ops.pack_weight_t(w2, s2), 1000, 512, 2048, None, residual=x, alpha=1.0 / s2)
    assert bool((y == y[0]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n", [(70, 48, 256), (200, 16, 512), (129, 80, 256), (1000, 272, 768)])
def test_hand_written_gemm_odd_k_step_counts(hip, m, k, n):
    # k / 16 odd or 1: the two-steps-per-iteration main loop leaves through its middle; ring prologue shorter than the ring
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m + k + n)
    x = torch.randn(m, k, generator=g)
    w, b = torch.randn(n, k, generator=g) / k ** 0.5, 0.1 * torch.randn(n, generator=g)
    lw, lb = torch.ones(k), torch.zeros(k)
    xn = torch.nn.functional.layer_norm(x.double(), (k,), lw.double(), lb.double(), 1e-5)
    z = xn @ w.double().T + b.double()
    ref = z * torch.sigmoid(z)
    ws = ops.weight_scale_f16x3(w)
    at = ops.layer_norm_t(x.cuda(), lw.cuda(), lb.cuda(), 1e-5)
    ht = ops.linear_t(at, ops.pack_weight_t(w.cuda(), ws), m, n, k, b.cuda(), act="silu", alpha=1.0 / ws)
    got = ops.unpack_act_t(ht, m, n).cpu().double()
    assert float((got - ref).abs().max()) < 2e-5
    # and the fp32 epilogue on the operand just produced (k' = n): y = h W2^T + x2
    w2 = torch.randn(256, n, generator=g) / n ** 0.5
    x2 = torch.randn(m, 256, generator=g)
    ws2 = ops.weight_scale_f16x3(w2)
    y = ops.linear_t(ht, ops.pack_weight_t(w2.cuda(), ws2), m, 256, n, None, residual=x2.cuda(), alpha=1.0 / ws2).cpu().double()
    assert float((y - (ref @ w2.double().T + x2.double())).abs().max()) < 3e-5


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n,mean_over_sigma", [(300, 128, 512, 0.0), (1000, 768, 2304, 3.0), (129, 512, 256, 30.0), (2500, 768, 3072, 0.3)])
def test_layernorm_folded_into_the_gemm_matches_float64(hip, m, k, n, mean_over_sigma):
    # LN(x) W^T + b through lemon_linear_f16x3t_ln (raw x as the operand, (rstd, -mean rstd) and the weight-row sums in the
    # epilogue) against float64, for both epilogues (fp32 + residual, SiLU -> operand) and rows whose mean is far from 0 in
    # units of their spread: the bar is the un-folded path's own error on the same operands (x 1.5) widened by the documented
    # factor max over rows of sqrt(1 + mean^2 / var) of the fold (1.0x for zero-mean rows; ops.LN_FOLD_MAX_SHIFT bounds it in
    # the product: a micro-batch beyond it is re-embedded with LayerNorm kernels).
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m + k + n)
    x = torch.randn(m, k, generator=g) * (0.5 + torch.rand(m, 1, generator=g) * 4) + mean_over_sigma * torch.randn(m, 1, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    w, b = 0.03 * torch.randn(n, k, generator=g), 0.1 * torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    eps = 1e-5
    xd = x.double()
    ln = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta.double()
    want = ln @ w.double().t() + b.double()
    xc, wc, bc, gc, bec, rc = (t.cuda() for t in (x, w, b, gamma, beta, res))
    # un-folded: LayerNorm kernel -> GEMM
    ws = ops.weight_scale_f16x3(wc)
    plain = ops.linear_t(ops.layer_norm_t(xc, gc, bec, eps), ops.pack_weight_t(wc, ws), m, n, k, bc, residual=rc, alpha=1.0 / ws).cpu().double() - res.double()
    e_plain = float((plain - want).abs().max())
    # folded
    xt, aff = ops.rowstats_t(xc, eps)
    wt, a, cs, bp = ops.fold_layernorm_weight(wc, bc, gc, bec, 1.0)
    got = ops.linear_t_ln(xt, wt, m, n, k, bp, residual=rc, alpha=a, row_aff=aff, colsum=cs).cpu().double() - res.double()
    e_fold = float((got - want).abs().max())
    scale = float(want.abs().max())
    # rows whose |mean| rstd exceeds ops.LN_FOLD_MAX_SHIFT must come out non-finite (the caller then redoes them without the
    # fold); the others within the un-folded error x the fold's documented factor sqrt(1 + mean^2 / var)
    shift = (xd.mean(1).abs() / torch.sqrt(xd.var(1, unbiased=False) + eps))
    near, far = shift < 0.999 * ops.LN_FOLD_MAX_SHIFT, shift > 1.001 * ops.LN_FOLD_MAX_SHIFT
    assert not bool(torch.isfinite(got[far]).any()) and bool(torch.isfinite(got[near]).all())
    if mean_over_sigma >= 30:
        assert int(far.sum()) > 10
    ratio = float(torch.sqrt(1.0 + shift[near] ** 2).max())
    e_fold = float((got - want)[near].abs().max())
    bar = 1.5 * max(e_plain, 2e-7 * scale) * ratio
    assert e_fold <= bar, (e_fold, e_plain, scale, ratio)
    for _ in range(3):      # (the same call again: the packed-multiply fault this path once had was sporadic, ~1e3 wrong values per call)
        again = ops.linear_t_ln(xt, wt, m, n, k, bp, residual=rc, alpha=a, row_aff=aff, colsum=cs).cpu().double() - res.double()
        assert torch.equal(again[near], got[near])
    # the SiLU -> operand form
    s = 1.702
    wt, a, cs, bp = ops.fold_layernorm_weight(wc, bc, gc, bec, s)
    ht = ops.linear_t_ln(xt, wt, m, n, k, bp, act="silu", alpha=s * a, row_aff=aff, colsum=cs)
    got = ops.unpack_act_t(ht, m, n).cpu().double()
    z = s * want
    want_h = z * torch.sigmoid(z)
    assert float((got - want_h)[near].abs().max()) <= 2.0 * bar * s + 1e-6 * float(want_h.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n", [(300, 128, 256), (1000, 768, 768), (129, 2048, 768), (2600, 64, 512)])
def test_chain_gemm_with_the_residual_in_operand_form_and_no_fp32_result(hip, m, k, n):
    # lemon_linear_f16x3t_chain (the output projection / fc2 of a block chain): (a) with an fp32 residual and an fp32 result it is
    # lemon_linear_f16x3t_ln's emit form bit for bit; (b) with the residual handed over as the operand an emitting GEMM left
    # (hi + lo 2^-11) the result is that of the fp32 call on the operand's own values -- bit for bit --, i.e. within 2^-22 of
    # the residual's magnitude of the call on the original fp32 residual; (c) without an fp32 result the operand and the row
    # statistics it leaves are the same bits
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m + 3 * k + n)
    x = torch.randn(m, k, generator=g)
    w, b = 0.05 * torch.randn(n, k, generator=g), 0.1 * torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g) * (0.2 + 3 * torch.rand(m, 1, generator=g)) + 5.0 * torch.randn(m, 1, generator=g)
    xc, wc, bc, rc = (t.cuda() for t in (x, w, b, res))
    ws = ops.weight_scale_f16x3(wc)
    wt = ops.pack_weight_t(wc, ws)
    at, _ = ops.rowstats_t(xc, 1e-5)
    rt, _ = ops.rowstats_t(rc, 1e-5)                         # the residual as a tile-major operand
    r_back = ops.unpack_act_t(rt, m, n)                     # ... and the values it holds
    assert bool(((r_back - rc).abs() <= 2.0 ** -21 * rc.abs() + 1e-30).all())
    out0, et0, st0 = ops.linear_t_ln(at, wt, m, n, k, bc, residual=rc, alpha=1.0 / ws, emit=True)
    out1, et1, st1 = ops.linear_t_chain(at, wt, m, n, k, bc, residual=rc, alpha=1.0 / ws)
    assert torch.equal(out0, out1) and torch.equal(st0, st1)
    assert torch.equal(ops.unpack_act_t(et0, m, n), ops.unpack_act_t(et1, m, n))        # (rows of the tile padding are not defined)
    want, wet, wst = ops.linear_t_chain(at, wt, m, n, k, bc, residual=r_back, alpha=1.0 / ws)
    out2, et2, st2 = ops.linear_t_chain(at, wt, m, n, k, bc, residual_t=rt, alpha=1.0 / ws)
    assert torch.equal(out2, want) and torch.equal(st2, wst) and torch.equal(ops.unpack_act_t(et2, m, n), ops.unpack_act_t(wet, m, n))
    assert float((out2 - out1).abs().max()) <= 2.0 ** -21 * float(rc.abs().max())
    none, et3, st3 = ops.linear_t_chain(at, wt, m, n, k, bc, residual_t=rt, alpha=1.0 / ws, fp32_out=False)
    assert none is None and torch.equal(st3, st2) and torch.equal(ops.unpack_act_t(et3, m, n), ops.unpack_act_t(et2, m, n))
    with pytest.raises(AssertionError):
        ops.linear_t_chain(at, wt, m, n, k, bc, residual=rc, residual_t=rt)              # one residual only


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,n", [(300, 128, 256), (1000, 768, 768), (129, 2048, 768), (2600, 64, 512)])
def test_gemm_emits_the_next_layernorms_operand_and_statistics(hip, m, k, n):
    # the producing side of the fold: the fp32 result is the plain kernel's (same products, the bias / residual additions in
    # another order: last-bit differences), the operand it also writes is the fp16 split of exactly what it stored, and the
    # finished row statistics are those of the stored values (float64), also for rows with a large common offset
    from lemon_amd import ops
    g = torch.Generator().manual_seed(m + k + n)
    x = torch.randn(m, k, generator=g)
    w, b = 0.05 * torch.randn(n, k, generator=g), 0.1 * torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g) * (0.2 + 3 * torch.rand(m, 1, generator=g)) + 20.0 * torch.randn(m, 1, generator=g)
    xc, wc, bc, rc = (t.cuda() for t in (x, w, b, res))
    ws = ops.weight_scale_f16x3(wc)
    wt = ops.pack_weight_t(wc, ws)
    at, _ = ops.rowstats_t(xc, 1e-5)
    plain = ops.linear_t(at, wt, m, n, k, bc, residual=rc, alpha=1.0 / ws)
    out, et, st = ops.linear_t_ln(at, wt, m, n, k, bc, residual=rc, alpha=1.0 / ws, emit=True)
    assert float((out - plain).abs().max()) <= 4e-7 * float(plain.abs().max())
    back = ops.unpack_act_t(et, m, n)
    assert float((back - out).abs().max()) <= 2.0 ** -21 * float(out.abs().max())
    assert bool(((back - out).abs() <= 2.0 ** -21 * out.abs() + 1e-30).all())
    eps = 1e-5
    aff = ops.ln_finalize(st, m, n, eps).cpu().double()
    od = out.cpu().double()
    mean, var = od.mean(1), od.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    shift = mean.abs() * rstd                 # rows beyond ops.LN_FOLD_MAX_SHIFT are poisoned (NaN): the caller falls back
    near, far = shift < 0.999 * ops.LN_FOLD_MAX_SHIFT, shift > 1.001 * ops.LN_FOLD_MAX_SHIFT
    assert int(near.sum()) > m // 8 and int(far.sum()) > m // 8
    assert not bool(torch.isfinite(aff[far]).any())
    assert float(((aff[near, 0] - rstd[near]).abs() / rstd[near]).max()) <= 2e-6
    assert float((aff[near, 1] + (mean * rstd)[near]).abs().max()) <= 2e-6 * (ops.LN_FOLD_MAX_SHIFT + 1.0)
    # and through the first-block kernel
    _, aff0 = ops.rowstats_t(out, eps)
    aff0 = aff0.cpu().double()
    assert not bool(torch.isfinite(aff0[far]).any())
    assert float(((aff0[near, 0] - rstd[near]).abs() / rstd[near]).max()) <= 2e-6
