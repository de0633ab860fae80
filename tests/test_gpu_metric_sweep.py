"""GPU: the metric sweep.  k_l2_from_ip against its host twin bit for bit (ragged wave counts, guard rows, refusals);
IndexFlatIP.search + derive_l2 + the fallback against IndexFlatL2.search under both scan algorithms; LemonDB.neighbors_metrics
against one LemonDB.neighbors call per metric on every record array; `run_lemon --dist_type_sweep` against the single runs.

Shapes: databases shorter than, equal to and longer than the list (40, 55, 64, 2048 rows against kd = 3, 5, 55, 64), k = 1, 2,
6, the reference's 50 + 1 and LEMON_MAX_K, d = 64 and 67 (d % 4 != 0), 1 / 3 / 130 queries (under a block of four waves, a
ragged block, many blocks with a tail), and one 65 536-row database so that the fp16 filter scan serves the IP search."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

from tests import metricfx as fx

pytestmark = pytest.mark.gpu

KDS, KS = (3, 5, 55, 64), (1, 2, 6, 51, 64)
REC_KEYS = ("d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m", "I_n", "I_m")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_raw(a), _raw(b))


def _guarded_call(index, q, Dip, Iip, k):
    """lemon_index_l2_from_ip into outputs with a poisoned row in front and behind: (rc, D, I, cert) with the guards checked"""
    import torch
    from lemon_amd.ops import ptr, stream_ptr
    nq = q.shape[0]
    kd = Dip.shape[1] if Dip is not None else 1
    D = torch.full((nq + 2, max(k, 1)), -7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq + 2, max(k, 1)), -7, dtype=torch.int64, device="cuda")
    c = torch.full((nq + 2,), 7, dtype=torch.uint8, device="cuda")
    rc = index._lib.lemon_index_l2_from_ip(index._h, ptr(q), nq, ptr(Dip), ptr(Iip), kd, k, ptr(D[1:]), ptr(I[1:]),
                                           ctypes.c_void_p(c.data_ptr() + 1), stream_ptr(index.device))
    torch.cuda.synchronize()
    for t, v in ((D, -7.0), (I, -7), (c, 7)):
        assert bool((t[0] == v).all()) and bool((t[-1] == v).all()), "a guard row was written"
    return rc, D[1:-1], I[1:-1], c[1:-1]


@pytest.mark.parametrize("d", [64, 67])
@pytest.mark.parametrize("n", [40, 55, 64, 2048])
def test_kernel_equals_the_host_twin(hip, oracle, n, d):
    import torch
    certified = uncertified = 0
    for name in ("random", "clustered", "duplicates"):
        X, Q = fx.family(oracle, name, n, 130, d, seed=n + d)
        xx, qq = fx.norms(oracle, X), fx.norms(oracle, Q)
        index = hip.IndexFlatIP(d)
        index.add(_cuda(X))
        q = _cuda(Q)
        for kd in KDS:
            Dip, Iip = index.search(q, kd)
            hD, hI = Dip.cpu().numpy(), Iip.cpu().numpy()
            for k in KS:
                if k > kd:
                    continue
                want = fx.host_derive(qq, xx, hD, hI, k)
                for nq in (1, 3, 130):
                    rc, D, I, c = _guarded_call(index, q[:nq], Dip[:nq].contiguous(), Iip[:nq].contiguous(), k)
                    assert rc == 0, (name, kd, k, nq)
                    assert fx.same_bits(D.cpu().numpy(), want[0][:nq]) and np.array_equal(I.cpu().numpy(), want[1][:nq]), (name, kd, k, nq)
                    assert np.array_equal(c.cpu().numpy().astype(bool), want[2][:nq]), (name, kd, k, nq)
                certified += int(want[2].sum())
                uncertified += int((~want[2]).sum())
        del index
    assert certified > 0 and (uncertified > 0 or n < 64)


def test_a_nan_query_and_a_nan_database_row(hip, oracle):
    import torch
    X, Q = fx.family(oracle, "random", 2048, 8, 64, seed=3)
    Q[5, 3] = np.nan
    index = hip.IndexFlatIP(64)
    index.add(_cuda(X))
    q = _cuda(Q)
    D, I = index.search(q, 55)
    _, _, cert = index.derive_l2(q, D, I, 51)
    assert cert.cpu().tolist() == [True] * 5 + [False] + [True] * 2
    X[100, 0] = np.nan                                       # its stored norm is NaN: the L2 search ranks it first, the IP search never
    index = hip.IndexFlatIP(64)
    index.add(_cuda(X))
    D, I = index.search(q, 55)
    assert not bool(index.derive_l2(q, D, I, 51)[2].any())


def test_refusals_write_nothing(hip, oracle):
    import torch
    X, Q = fx.family(oracle, "random", 128, 4, 64, seed=1)
    ip, l2 = hip.IndexFlatIP(64), hip.IndexFlatL2(64)
    ip.add(_cuda(X)), l2.add(_cuda(X))
    q = _cuda(Q)
    Dip, Iip = ip.search(q, 8)

    def refused(index, qv, Dv, Iv, k, kd=None):
        if kd is not None:                                   # a kd the arrays do not have: only the check may look at it
            Dv = torch.zeros((qv.shape[0], kd), dtype=torch.float32, device="cuda")
            Iv = torch.zeros((qv.shape[0], kd), dtype=torch.int64, device="cuda")
        rc, D, I, c = _guarded_call(index, qv, Dv, Iv, k)
        return rc != 0 and bool((D == -7.0).all()) and bool((I == -7).all()) and bool((c == 7).all())

    assert not refused(ip, q, Dip, Iip, 8)
    assert refused(l2, q, Dip, Iip, 4)                       # not an IP index
    assert refused(ip, q, Dip, Iip, 0) and refused(ip, q, Dip, Iip, 9)          # k < 1, k > kd
    assert refused(ip, q, None, None, 65, kd=65)             # kd > LEMON_MAX_K
    assert refused(ip, q, None, Iip, 4) and refused(ip, q, Dip, None, 4)        # a null pointer
    pad = torch.zeros(4 * 64 + 1, dtype=torch.float32, device="cuda")
    pad[1:] = q.flatten()
    assert refused(ip, pad[1:].view(4, 64), Dip, Iip, 4)     # rows 4 bytes off a 16-byte boundary, d % 4 == 0
    from lemon_amd.ops import ptr, stream_ptr
    out = torch.full((4, 4), -7.0, device="cuda")
    assert ip._lib.lemon_index_l2_from_ip(None, ptr(q), 4, ptr(Dip), ptr(Iip), 8, 4, ptr(out), ptr(Iip), ptr(out), stream_ptr(ip.device)) != 0
    assert ip._lib.lemon_index_l2_from_ip(ip._h, ptr(q), 4, ptr(Dip), ptr(Iip), 8, 4, None, None, None, stream_ptr(ip.device)) != 0
    for kw in (dict(k=0), dict(k=9)):
        with pytest.raises(ValueError):
            ip.derive_l2(q, Dip, Iip, **kw)
    assert not hasattr(l2, "derive_l2")


def _derive_with_fallback(ip, l2, q, k, kd):
    D, I = ip.search(q, kd)
    Dl, Il, cert = ip.derive_l2(q, D, I, k)
    rows = (~cert).nonzero().flatten()
    if rows.numel():
        Dl[rows], Il[rows] = l2.search(q[rows].contiguous(), k)
    return Dl, Il, cert


@pytest.mark.parametrize("algo", ["f32", "filter"])
@pytest.mark.parametrize("n", [40, 2048])
def test_search_derive_fallback_equals_the_l2_search(hip, oracle, algo, n):
    from lemon_amd import _lib
    code = {"f32": _lib.ALGO_F32_MFMA, "filter": _lib.ALGO_BF16_FILTER}[algo]
    for name in ("random", "clustered", "duplicates", "tight"):
        X, Q = fx.family(oracle, name, n, 70, 64, seed=n + 5)
        ip, l2 = hip.IndexFlatIP(64), hip.IndexFlatL2(64)
        for index in (ip, l2):
            index.set_algo(code)
            index.add(_cuda(X))
        q = _cuda(Q)
        for k, kd in ((1, 2), (1, 5), (6, 10), (51, 55), (60, 64), (64, 64)):
            want = l2.search(q, k)
            D, I, cert = _derive_with_fallback(ip, l2, q, k, kd)
            assert _same(D, want[0]) and _same(I, want[1]), (name, k, kd)
            Dc, Ic, _ = ip.derive_l2(q, *ip.search(q, kd), k)                  # the certified rows alone, nothing put back
            assert _same(Dc[cert], want[0][cert]) and _same(Ic[cert], want[1][cert]), (name, k, kd)
            if n < kd or (name == "random" and kd > k):
                assert bool(cert.all()), (name, k, kd)
            if n == 2048 and name == "duplicates":
                assert not bool(cert.any()), (name, k, kd)
            if n == 2048 and name == "clustered" and (k, kd) == (51, 55):
                assert bool(cert.sum() * 2 > 70)                              # most rows certified, and NOT as the cosine prefix
                assert bool(((Ic != ip.search(q, k)[1]).any(dim=1) & cert).sum() * 2 > 70)


def test_the_filter_scan_serves_the_ip_leg(hip, oracle):
    """65 536 x 64 rows, 256 queries: the IP lists come from the fp16 filter scan (exact by its re-rank)"""
    from lemon_amd import _lib
    A, _ = fx.clustered(oracle, 65536 + 256, 64, seed=9, noise=0.2, protos=64)
    X, Q = A[:65536], A[65536:]
    ip, l2 = hip.IndexFlatIP(64), hip.IndexFlatL2(64)
    for index in (ip, l2):
        index.set_algo(_lib.ALGO_BF16_FILTER)
        index.add(_cuda(X))
    q = _cuda(Q)
    want = l2.search(q, 51)
    D, I, cert = _derive_with_fallback(ip, l2, q, 51, 55)
    assert ip.last_scan_kernel() not in ("", "scan_f32")
    assert _same(D, want[0]) and _same(I, want[1])
    Dc, Ic, _ = ip.derive_l2(q, *ip.search(q, 55), 51)
    assert bool(cert.any()) and _same(Dc[cert], want[0][cert]) and _same(Ic[cert], want[1][cert])


def _pairs(oracle, name, n, nq, d, seed):
    """image / text DB rows and queries of one family; the first half of the queries are DB rows (in_db), the rest fresh"""
    Xi, Qi = fx.family(oracle, name, n, nq, d, seed)
    Xt, Qt = fx.family(oracle, name, n, nq, d, seed + 50)
    in_db = np.zeros(nq, np.uint8)
    in_db[:nq // 2] = 1
    take = np.arange(nq // 2) * 3 % n
    Qi[:nq // 2], Qt[:nq // 2] = Xi[take], Xt[take]
    rng = np.random.default_rng(seed)
    return Xi, Xt, Qi, Qt, in_db, rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 5, nq).astype(np.int32)


@pytest.mark.parametrize("d", [64, 67])
@pytest.mark.parametrize("name", ["clustered", "duplicates"])
def test_neighbors_metrics_equals_a_call_per_metric(hip, oracle, name, d):
    from lemon_amd.neighbors import LemonDB
    n, nq = 2048, 90
    Xi, Xt, Qi, Qt, in_db, lab_db, lab_q = _pairs(oracle, name, n, nq, d, seed=d)
    xi, xt, qi, qt = _cuda(Xi), _cuda(Xt), _cuda(Qi), _cuda(Qt)
    both = LemonDB(xi, xt, ("cosine", "euclidean"), tr_label_id=lab_db)
    single = {m: LemonDB(xi, xt, m, tr_label_id=lab_db) for m in ("cosine", "euclidean")}
    certified = fallback = 0
    for ks in (2, 51, 64):
        for drop_self, discrete in ((True, False), (False, True), (True, True)):
            k = ks - int(drop_self)
            kw = dict(drop_self=drop_self, in_db=in_db if drop_self else None, discrete=discrete, q_label_id=lab_q)
            recs, counts = both.neighbors_metrics(qi, qt, k, **kw)
            assert sorted(recs) == ["cosine", "euclidean"]
            for m in recs:
                want = single[m].neighbors(qi, qt, k, **kw)
                assert sorted(recs[m]) == sorted(want) == sorted(REC_KEYS)
                for key in REC_KEYS:
                    assert _same(recs[m][key], want[key]), (m, key, ks, drop_self, discrete)
            assert counts["rows"] == nq and 0 <= counts["fallback"] <= nq
            assert counts["fallback"] >= nq - min(counts["certified_n"], counts["certified_m"])
            certified += nq - counts["fallback"]
            fallback += counts["fallback"]
        plain = both.neighbors(qi, qt, k, **kw)                                # a sweep DB's own `neighbors` is the cosine call
        assert all(_same(plain[key], recs["cosine"][key]) for key in REC_KEYS)
    if name == "clustered":
        assert certified > 0
    else:
        assert fallback > 0 and both._l2 is not None
    none = both.neighbors_metrics(qi, qt, 5, return_indices=False)[0]
    assert "I_n" not in none["cosine"] and "I_m" not in none["euclidean"]
    with pytest.raises(ValueError):
        single["cosine"].neighbors_metrics(qi, qt, 5)
    with pytest.raises(ValueError):
        LemonDB(xi, xt, ("cosine", "cosine"))


def test_score_splits_on_a_sweep_db_equals_a_db_per_metric(hip, oracle):
    from lemon_amd.neighbors import LemonDB
    from lemon_amd.pipeline import FIXED_HPARAMS, score_splits
    Xi, Xt, Qi, Qt, in_db, lab_db, lab_q = _pairs(oracle, "clustered", 600, 80, 64, seed=21)
    xi, xt, qi, qt = _cuda(Xi), _cuda(Xt), _cuda(Qi), _cuda(Qt)
    splits = [dict(name="train", img=qi, txt=qt, drop_self=True, in_db=in_db, label_id=lab_q),
              dict(name="val", img=qi[40:], txt=qt[40:], drop_self=False, in_db=None, label_id=lab_q[40:])]
    both = LemonDB(xi, xt, ("euclidean", "cosine"), tr_label_id=lab_db)
    calls = []
    plain = both.neighbors_metrics
    both.neighbors_metrics = lambda *a, **kw: (calls.append(a[2]), plain(*a, **kw))[1]
    for k in (5, [10, 1, 5]):
        del calls[:]
        got = score_splits(both, splits, k, FIXED_HPARAMS)
        assert calls == [10 if isinstance(k, list) else 5] and list(got) == ["euclidean", "cosine"]
        for m in got:
            want = score_splits(LemonDB(xi, xt, m, tr_label_id=lab_db), splits, k, FIXED_HPARAMS)
            for kk in ([None] if not isinstance(k, list) else sorted(want)):
                g, w = (got[m], want) if kk is None else (got[m][kk], want[kk])
                assert set(g) == set(w) == {"train", "val"}
                for name in w:
                    assert set(g[name]) == set(w[name])
                    for key in w[name]:
                        a, b = g[name][key].contiguous(), w[name][key].contiguous()
                        assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (m, kk, name, key)
        c = both.last_sweep_counts
        assert c["train"]["rows"] == 80 and c["val"]["rows"] == 40 and 0 <= c["val"]["fallback"] <= 40


# ---- the CLI sweep against the single runs -----------------------------------------------------------------------------------
SWEEP_K = [1, 5]
BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:1500", "--clip_path", "random:tiny",
        "--hparam_grid", "small", "--debug", "--lbfgs_polish", "device"]       # (the host polish takes seconds a run)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_tree(a, b, path="agg_results"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for key in a:
            _same_tree(a[key], b[key], f"{path}[{key!r}]")
    elif isinstance(a, (list, tuple, np.ndarray)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path
    elif isinstance(a, (float, np.floating)):
        assert _bits64(a) == _bits64(b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def _load(out):
    return pickle.load(open(os.path.join(out, "res.pkl"), "rb"))


def _assert_same_run(sub, one, m, k):
    import pandas as pd
    for f in ("args.json", "res.pkl", "know_val_labels_scores.csv", "done"):
        assert os.path.exists(os.path.join(sub, f)), (m, k, f)
    got, want = _load(sub), _load(one)
    pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
    _same_tree(got["agg_results"], want["agg_results"])
    csv = "know_val_labels_scores.csv"
    assert open(os.path.join(sub, csv), "rb").read() == open(os.path.join(one, csv), "rb").read(), (m, k)
    a, b = json.load(open(os.path.join(sub, "args.json"))), json.load(open(os.path.join(one, "args.json")))
    assert a["knn_k"] == k and a["dist_type"] == m and a["output_dir"] == sub
    for skip in ("output_dir", "knn_k", "knn_k_sweep", "dist_type", "dist_type_sweep", "dist_sweep_margin"):
        a.pop(skip), b.pop(skip)
    assert a == b


@pytest.mark.parametrize("extra", [[], ["--hparam_search", "device", "--normalize_d1"]], ids=["plain", "device-search-normalize_d1"])
def test_cli_sweep_equals_the_single_runs(hip, tmp_path, extra):
    from lemon_amd.run_lemon import main
    cache = str(tmp_path / "cache")
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, *extra, "--embedding_cache", cache, "--dist_type_sweep", "cosine,euclidean",
                 "--knn_k_sweep", "1,5"]) == 0
    for m in ("cosine", "euclidean"):
        for k in SWEEP_K:
            one = str(tmp_path / f"single_{m}_{k}")
            assert main(["--output_dir", one, *BASE, *extra, "--embedding_cache", cache, "--dist_type", m, "--knn_k", str(k)]) == 0
            _assert_same_run(os.path.join(out, f"dist_type={m}", f"knn_k={k}"), one, m, k)
        sel = json.load(open(os.path.join(out, f"dist_type={m}", "k_selection.json")))
        assert sel["ks"] == SWEEP_K and os.path.exists(os.path.join(out, f"dist_type={m}", "done"))
    info = json.load(open(os.path.join(out, "dist_sweep.json")))
    assert info["metrics"] == ["cosine", "euclidean"] and info["margin"] == 4 and info["knn_k"] == 5
    df = _load(os.path.join(out, "dist_type=cosine", "knn_k=1"))["df"]
    assert sorted(info["splits"]) == sorted(df.sset.unique())
    for sset, c in info["splits"].items():
        assert c["rows"] == int((df.sset == sset).sum())
        assert 0 <= c["certified_n"] <= c["rows"] and 0 <= c["certified_m"] <= c["rows"]
        assert c["rows"] - min(c["certified_n"], c["certified_m"]) <= c["fallback"] <= c["rows"]
        assert c["fallback"] <= (c["rows"] - c["certified_n"]) + (c["rows"] - c["certified_m"])
    assert os.path.exists(os.path.join(out, "done"))


def test_cli_metric_sweep_alone(hip, tmp_path):
    """without --knn_k_sweep the files of a run stand directly under dist_type=<m>/; one name is a sweep of one"""
    from lemon_amd.run_lemon import main
    cache = str(tmp_path / "cache")
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, "--embedding_cache", cache, "--dist_type_sweep", "euclidean,cosine", "--knn_k", "3",
                 "--dist_sweep_margin", "1"]) == 0
    for m in ("cosine", "euclidean"):
        one = str(tmp_path / f"single_{m}")
        assert main(["--output_dir", one, *BASE, "--embedding_cache", cache, "--dist_type", m, "--knn_k", "3"]) == 0
        _assert_same_run(os.path.join(out, f"dist_type={m}"), one, m, 3)
    info = json.load(open(os.path.join(out, "dist_sweep.json")))
    assert info["metrics"] == ["euclidean", "cosine"] and info["margin"] == 1
    alone = str(tmp_path / "alone")
    assert main(["--output_dir", alone, *BASE, "--embedding_cache", cache, "--dist_type_sweep", "euclidean", "--knn_k", "3"]) == 0
    _assert_same_run(os.path.join(alone, "dist_type=euclidean"), str(tmp_path / "single_euclidean"), "euclidean", 3)
    assert json.load(open(os.path.join(alone, "dist_sweep.json")))["splits"]["val"]["fallback"] is None
