"""GPU: the wide fp16 filter scan k_scan_f16_qsw (768 < d <= 1280, opt-in through set_wide_filter / LEMON_WIDE_FILTER) against the
float64 CPU oracle, bit for bit; where a shape is too large for the oracle, against the fp32 scan bit for bit plus the oracle on
a row sample (as tests/test_gpu_parity.py does for its large cases).

The kernel serves inner product AND squared L2 at both pitches (1024, 1280), so every forced case expects the family name
"qsw" from last_scan_kernel() for either metric."""
import numpy as np
import pytest
import torch

from tests.synth import planted, unit_rows
from tests.test_gpu_parity import _assert_knn_equal, _search, cu

pytestmark = pytest.mark.gpu
F32, BF16 = 1, 2
WIDE = "qsw"                 # family name of k_scan_f16_qsw
WIDE_SERVES_L2 = True        # (written down, not read from the library: squared L2 builds without spills at both pitches)


def _index(hip, metric, d, algo=None, wide=None):
    idx = (hip.IndexFlatIP if metric == "ip" else hip.IndexFlatL2)(d)
    if algo is not None:
        idx.set_algo(algo)
    if wide is not None:
        idx.set_wide_filter(wide)
    return idx


def _wide_search(hip, metric, X, Q, k):
    idx = _index(hip, metric, X.shape[1], BF16, True)
    idx.add(cu(X))
    D, I = idx.search(cu(Q), k)
    return D.cpu().numpy(), I.cpu().numpy(), idx


def _rescale(rng, X, Q):
    X *= rng.uniform(0.5, 2.0, (X.shape[0], 1)).astype(np.float32)
    Q *= rng.uniform(0.5, 2.0, (Q.shape[0], 1)).astype(np.float32)


def test_no_search_yet_names_no_kernel(hip):
    assert hip.IndexFlatIP(1024).last_scan_kernel() == ""


# ---- 1. forced onto small shapes ------------------------------------------------------------------------------------------
# ragged last panel (nq % 128, nq < 128), database tails (n % 64, n < 64), enough tiles for database splits with the merge
# (n >= 2048: lemon_plan_splits), k in {1, 51, 64}, d at both ends of both pitches and inside them
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq,n,d,k", [
    (100, 700, 772, 51), (300, 2049, 1024, 5), (257, 63, 1028, 10), (130, 129, 1000, 64), (513, 1300, 1276, 51),
    (256, 64 * 7 + 1, 1280, 64), (64, 20000, 1024, 51), (300, 3000, 1280, 1), (129, 9000, 1276, 64),
])
def test_wide_kernel_forced_on_small_shapes(hip, oracle, monkeypatch, metric, nq, n, d, k):
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    rng = np.random.default_rng(nq * 7 + n * 3 + d + k)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    if metric == "l2":
        _rescale(rng, X, Q)
    D, I, idx = _wide_search(hip, metric, X, Q, k)
    info = idx.last_search_info()
    assert info["algo"] == BF16 and info["query_panel"] == 128
    assert idx.last_scan_kernel() == (WIDE if (metric == "ip" or WIDE_SERVES_L2) else "scan_bf16")
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


# ---- 2. ties and clusters: the data sets of test_bf16_two_block_kernel_ties_and_clusters ----------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", [1000, 1280])
def test_wide_kernel_ties_and_clusters(hip, oracle, monkeypatch, metric, d):
    # duplicates + clusters far tighter than the fp16 band: band overflow, exact compaction on the spot
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    rng = np.random.default_rng(19)
    C, n, k = 12, 6000, 51
    proto = unit_rows(rng, C, d)
    X = proto[rng.integers(0, C, n)].copy()
    X[n // 2:] += rng.standard_normal((n - n // 2, d)).astype(np.float32) * 1e-4
    Q = (proto[rng.integers(0, C, 300)] + rng.standard_normal((300, d)).astype(np.float32) * 1e-3).astype(np.float32)
    D, I, idx = _wide_search(hip, metric, X, Q, k)
    assert idx.last_scan_kernel() == WIDE
    _assert_knn_equal((D, I), oracle.knn(metric, X, Q, k))


@pytest.mark.parametrize("d", [1000, 1280])
def test_wide_kernel_ascending_scores_every_row_admitted(hip, oracle, monkeypatch, d):
    # the append-pressure worst case: every row beats the running k-th best
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    rng = np.random.default_rng(19)
    k = 51
    base = unit_rows(rng, 1, d)[0]
    X = (base[None, :] * np.linspace(0.2, 1.0, 64 * 50, dtype=np.float32)[:, None]).astype(np.float32)
    Q = (base[None, :] * np.linspace(0.5, 1.5, 300, dtype=np.float32)[:, None]).astype(np.float32)
    D, I, idx = _wide_search(hip, "ip", X, Q, k)
    assert idx.last_scan_kernel() == WIDE
    _assert_knn_equal((D, I), oracle.knn("ip", X, Q, k))


# ---- 3. chunked launches: splits == 1 (>= 768 panels), several database chunks, state carried in between --------------------
@pytest.mark.parametrize("d,metric", [(1024, "ip"), (1280, "ip"), (1280, "l2")])
def test_wide_kernel_chunked_database_state_carry(hip, oracle, monkeypatch, d, metric):
    # 768 whole panels of 128 queries (three rounds of 256 workgroups) + a ragged rest of 77 queries that the streaming kernel
    # takes; 8-tile chunks (512 rows) of a 3 000-row database: six launches, the last one a partial chunk with a ragged tile
    monkeypatch.setenv("LEMON_CHUNK_MB", "0.01")
    nq, n = 768 * 128 + 77, 3000
    g = torch.Generator(device="cuda").manual_seed(9)
    X = hip.normalize_vectors(torch.randn(n, d, generator=g, device="cuda"))
    Q = hip.normalize_vectors(torch.randn(nq, d, generator=g, device="cuda"))
    if metric == "l2":
        X = X * (0.5 + 1.5 * torch.rand(n, 1, generator=g, device="cuda"))
    out = []
    for algo in (F32, BF16):
        idx = _index(hip, metric, d, algo, True)
        idx.add(X)
        out.append(idx.search(Q, 51))
        if algo == BF16:
            info = idx.last_search_info()
            assert info["db_splits"] == 1 and info["grid"] == 768 and idx.last_scan_kernel() == WIDE
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0])
    rows = torch.cat([torch.arange(0, 256), torch.arange(nq - 256, nq)]).cuda()
    Dr, Ir = oracle.knn(metric, X.cpu().numpy(), Q[rows].cpu().numpy(), 51)
    _assert_knn_equal((out[1][0][rows].cpu().numpy(), out[1][1][rows].cpu().numpy()), (Dr, Ir))


# ---- 4. AUTO: the width limit follows the switch ----------------------------------------------------------------------------
def test_auto_takes_the_wide_kernel_on_spread_data_only_with_the_switch_on(hip):
    g = torch.Generator(device="cuda").manual_seed(3)
    n, nq, d = 65536, 131072, 1024
    spread = hip.normalize_vectors(torch.randn(n, d, generator=g, device="cuda"))
    q = hip.normalize_vectors(torch.randn(nq, d, generator=g, device="cuda"))
    proto = hip.normalize_vectors(torch.randn(10, d, generator=g, device="cuda"))
    crowded = proto[torch.randint(0, 10, (n,), generator=g, device="cuda")]       # class-prompt style duplicates
    crowded_q = proto[torch.randint(0, 10, (nq,), generator=g, device="cuda")]
    for X, Q, expect_on in ((spread, q, BF16), (crowded, crowded_q, F32)):
        ref = _index(hip, "ip", d, F32)
        ref.add(X)
        Dr, Ir = ref.search(Q, 10)
        for wide, expect in ((True, expect_on), (False, F32)):
            auto = _index(hip, "ip", d, None, wide)
            auto.add(X)
            Da, Ia = auto.search(Q, 10)
            assert auto.last_search_info()["algo"] == expect, (wide, expect)
            assert auto.last_scan_kernel() == (WIDE if expect == BF16 else "scan_f32")
            assert torch.equal(Ia, Ir) and torch.equal(Da, Dr)


# ---- 5. the switch and the 16-bit copy: d = 800 is pitch 832 with the switch off and 1024 with it on ------------------------
def test_toggling_the_switch_rebuilds_the_copy_at_the_other_pitch(hip, oracle, monkeypatch):
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    rng = np.random.default_rng(41)
    d, k = 800, 20
    X, X2, Q = unit_rows(rng, 3000, d), unit_rows(rng, 700, d), unit_rows(rng, 200, d)
    idx = _index(hip, "ip", d, BF16, False)
    idx.add(cu(X))

    def check(rows, name):
        D, I = idx.search(cu(Q), k)
        assert idx.last_scan_kernel() == name
        _assert_knn_equal((D.cpu().numpy(), I.cpu().numpy()), oracle.knn("ip", rows, Q, k))

    check(X, "scan_bf16")
    idx.set_wide_filter(True)
    check(X, WIDE)
    idx.add(cu(X2))                                  # the new rows are converted at the copy's pitch
    both = np.concatenate([X, X2])
    check(both, WIDE)
    idx.set_wide_filter(False)
    check(both, "scan_bf16")


# ---- 6. through the product path ------------------------------------------------------------------------------------------
def test_neighbors_records_identical_with_the_switch_on_and_off(hip, monkeypatch):
    monkeypatch.setenv("LEMON_QS2_MIN_PANELS", "0")
    s = planted(seed=2, n_tr=3000, n_q=300, d=1024, C=16)
    img_tr, txt_tr, _, _ = s["train"]
    q_img, q_txt, _, _ = s["query"]
    recs = []
    for wide in (False, True):
        db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine", algo=BF16)
        db.index_img.set_wide_filter(wide)
        db.index_txt.set_wide_filter(wide)
        recs.append(db.neighbors(cu(q_img), cu(q_txt), 10))
        assert db.index_img.last_scan_kernel() == (WIDE if wide else "scan_bf16")
        assert db.index_txt.last_scan_kernel() == (WIDE if wide else "scan_bf16")
    for key in ("I_n", "I_m", "d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m"):
        a, b = recs[0][key].cpu().numpy(), recs[1][key].cpu().numpy()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), key
