"""GPU: the knn_k sweep.  lemon_grid_f1_ks against lemon_grid_f1 on the contiguous prefix of the record (bit for bit), what its
ABI refuses, the prefix property of the neighbour record (an exact top-k list, self-exclusion included, is a prefix of every
deeper one) and `run_lemon --knn_k_sweep` against the single --knn_k runs.

Shapes are the smallest at which the kernels can go wrong: n = 1 (one thread), 63 (under a wave), 256 (an exact block), 257
(a block plus one), 1031 (several blocks with a tail); kmax = 1, 2, the reference's 50 + 1, and LEMON_MAX_K - 1 / LEMON_MAX_K."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REC_ARRAYS = ("D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m")
REF_KS = [1, 2, 5, 10, 15, 20, 30, 50]
SHAPES = [(1, [1]), (2, [1, 2]), (51, REF_KS), (63, [63]), (64, [1, 64])]
POISON = 0x7FF4DEADBEEF0BAD          # a NaN no kernel produces


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _record(n, kmax, seed, nan_from=None):
    import torch
    rng = np.random.default_rng(seed)
    rec = {"d_1": rng.uniform(0.0, 1.0, n).astype(np.float32)}
    for side in "nm":
        rec["D_" + side] = rng.uniform(-1.0, 1.0, (n, kmax)).astype(np.float32)       # both signs: a negative tau overflows
        rec["dists_tr_" + side] = rng.uniform(0.0, 2.0, (n, kmax)).astype(np.float32)
        rec["dists_" + side] = rng.uniform(0.0, 2.0, (n, kmax)).astype(np.float32)
    if nan_from is not None:
        for key in REC_ARRAYS:
            rec[key][:, nan_from:] = np.nan
    return {k: torch.from_numpy(v).cuda() for k, v in rec.items()}


def _small_grid(force_zero=()):
    from lemon_amd import metrics as M
    grid = {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}       # run_lemon --hparam_grid small
    return [[hp[n] for n in M.HP_NAMES] for hp in M.grid_points(grid, force_zero)]


def _random_rows():
    rng = np.random.default_rng(7)
    rows = rng.uniform(0.0, 6.0, (40, 6))
    rows[5], rows[17], rows[33] = rows[2], rows[2], rows[11]           # repeated rows
    rows[8, 2:4] = (0.0, 1.5)
    rows[9, 2:4] = (-0.0, 1.5)                                          # the same pair by value, another by bit pattern
    rows[20, 4:6] = rows[21, 2:4]                                       # an n pair of one row that is an m pair of another
    return rows.tolist()


OVERFLOW_ROW = [[1.0, 1.0, -1e4, -1e4, -1e4, -1e4]]


def _hp_sets():
    return {"small": _small_grid(), "small_force_zero": _small_grid(("tau_1_n", "tau_1_m")), "random40": _random_rows(),
            "G1": [[5.0, 10.0, 1.0, 5.0, 0.5, 2.0]], "overflow": OVERFLOW_ROW}


def _labels(n, kind):
    if kind == "mixed":
        y = (np.random.default_rng(n).uniform(size=n) < 0.4).astype(np.uint8)
        y[0] = 1
        return y
    return np.zeros(n, np.uint8) if kind == "zeros" else np.ones(n, np.uint8)


def _check_against_prefixes(ops, rec, y, hps, ks, what):
    from lemon_amd.neighbors import prefix_record
    f1, th, sc = ops.grid_f1_ks(rec, y, hps, ks, return_scores=True)
    G, n = len(hps), rec["d_1"].shape[0]
    assert f1.shape == th.shape == (len(ks), G) and sc.shape == (len(ks), G, n)
    f1b, thb = ops.grid_f1_ks(rec, y, hps, ks)
    assert np.array_equal(_bits(f1b), _bits(f1)) and np.array_equal(_bits(thb), _bits(th)), what
    for t, k in enumerate(ks):
        rf1, rth, rsc = ops.grid_f1(prefix_record(rec, k), y, hps, return_scores=True)
        assert np.array_equal(_bits(sc[t]), _bits(rsc)), (what, k, "scores")
        assert np.array_equal(_bits(f1[t]), _bits(rf1)), (what, k, "f1", f1[t], rf1)
        assert np.array_equal(_bits(th[t]), _bits(rth)), (what, k, "thres", th[t], rth)
    return f1, th


@pytest.mark.parametrize("kmax,ks", SHAPES, ids=[f"kmax{s[0]}" for s in SHAPES])
@pytest.mark.parametrize("n", [1, 63, 256, 257, 1031])
def test_grid_f1_ks_equals_grid_f1_on_every_prefix(hip, n, kmax, ks):
    from lemon_amd import ops
    rec = _record(n, kmax, seed=1000 * n + kmax)
    for name, hps in _hp_sets().items():
        for kind in ("mixed", "zeros", "ones"):
            f1, th = _check_against_prefixes(ops, rec, _labels(n, kind), hps, ks, (name, kind))
            if name == "overflow":       # non-finite scores: F1 = 0, thres = NaN at every k, as lemon_grid_f1 gives it
                assert np.all(f1 == 0.0) and np.all(np.isnan(th)), (kind, f1, th)


@pytest.mark.parametrize("n", [63, 257])
def test_grid_f1_ks_record_with_nan_tail(hip, n):
    """lemon_neighbors writes NaN for neighbours that do not exist (ntotal < k): prefixes up to the 7 real columns are finite,
    deeper ones follow the non-finite rule."""
    from lemon_amd import ops
    rec = _record(n, 51, seed=n, nan_from=7)
    ks = [1, 2, 5, 7, 8, 10, 30, 50]
    f1, th = _check_against_prefixes(ops, rec, _labels(n, "mixed"), _small_grid(), ks, "nan tail")
    assert np.all(np.isfinite(th[:4])) and np.all(np.isfinite(f1[:4]))      # (the search is local: F1 itself may be 0)
    assert np.all(f1[4:] == 0.0) and np.all(np.isnan(th[4:]))


def _abi_call(lib, rec, y, ks, K, kmax, hp, G, pad=64, ws_extra=4096, scores=False):
    """A direct lemon_grid_f1_ks call with every device buffer filled with a poison pattern and padded behind its end.
    -> (rc, f1 bits, thres bits, scores bits or None, workspace bytes as uint8, needed workspace bytes)"""
    import torch
    from lemon_amd.ops import ptr, stream_ptr
    n = rec["d_1"].shape[0]
    hp = np.ascontiguousarray(np.asarray(hp, dtype=np.float64).reshape(-1, 6))
    dp = hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    need = lib.lemon_grid_f1_ks_workspace_bytes(n, min(max(K, 1), 16), G, dp)
    assert need > 0
    poison = lambda count: torch.full((count,), POISON, dtype=torch.int64, device="cuda")
    kk = max(K, 1)
    f1, th = poison(kk * G + pad), poison(kk * G + pad)
    sc = poison(kk * G * n + pad) if scores else None
    ws = poison((need + ws_extra) // 8 + 1)
    c_ks = (ctypes.c_int * max(len(ks), 1))(*ks)
    yb = torch.from_numpy(np.asarray(y, np.uint8)).cuda()
    rc = lib.lemon_grid_f1_ks(ptr(rec["d_1"]), *[ptr(rec[key]) for key in REC_ARRAYS], ptr(yb), n, kmax, c_ks, K, dp, G, 1e-8, 500,
                              ptr(ws), need, ptr(sc), ptr(f1), ptr(th), stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy().view(np.uint64)
    return rc, host(f1), host(th), host(sc), host(ws), need


@pytest.mark.parametrize("n,kmax,ks", [(257, 51, REF_KS), (1, 1, [1]), (1031, 64, [1, 64])])
def test_grid_f1_ks_touches_nothing_outside_its_outputs(hip, n, kmax, ks):
    from lemon_amd import _lib, ops
    lib = _lib.load()
    rec, y, hps = _record(n, kmax, seed=3), _labels(n, "mixed"), _random_rows()
    K, G = len(ks), len(hps)
    rc, f1, th, sc, ws, need = _abi_call(lib, rec, y, ks, K, kmax, hps, G, scores=True)
    assert rc == 0, lib.lemon_last_error()
    ref_f1, ref_th, ref_sc = ops.grid_f1_ks(rec, y, hps, ks, return_scores=True)
    assert np.array_equal(f1[:K * G], _bits(ref_f1).ravel()) and np.all(f1[K * G:] == POISON)
    assert np.array_equal(th[:K * G], _bits(ref_th).ravel()) and np.all(th[K * G:] == POISON)
    assert np.array_equal(sc[:K * G * n], _bits(ref_sc).ravel()) and np.all(sc[K * G * n:] == POISON)
    assert need % 8 == 0 and np.all(ws[need // 8:] == POISON)            # nothing behind the bytes the library asked for
    # without a score buffer the scores live in the workspace: same results, same guard
    rc, f1b, thb, _, ws, _ = _abi_call(lib, rec, y, ks, K, kmax, hps, G)
    assert rc == 0 and np.array_equal(f1b, f1) and np.array_equal(thb, th) and np.all(ws[need // 8:] == POISON)


BAD_CALLS = {
    "unsorted ks": dict(ks=[5, 2, 10]),
    "repeated ks": dict(ks=[2, 5, 5]),
    "k = 0": dict(ks=[0, 2, 5]),
    "k > kmax": dict(ks=[2, 5, 21]),
    "kmax > 64": dict(ks=[2, 5, 10], kmax=65),
    "K = 0": dict(ks=[], K=0),
    "K = 17": dict(ks=list(range(1, 18)), K=17),
}


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_grid_f1_ks_refuses_what_is_out_of_contract(hip, case):
    from lemon_amd import _lib
    lib = _lib.load()
    n, depth = 100, 80                      # the arrays are deep enough for every pitch a refused call names
    rec, y = _record(n, depth, seed=5), _labels(n, "mixed")
    bad = BAD_CALLS[case]
    ks = bad["ks"]
    rc, f1, th, sc, ws, _ = _abi_call(lib, rec, y, ks, bad.get("K", len(ks)), bad.get("kmax", 20), _small_grid(), 36, scores=True)
    assert rc == -1, (case, rc)             # LEMON_E_INVALID
    assert lib.lemon_last_error()
    for buf in (f1, th, sc, ws):
        assert np.all(buf == POISON), case


# ---- the prefix property of the neighbour record ---------------------------------------------------------------------------
def _embeddings(ndb, nq, d, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    unit = lambda t: t / t.norm(dim=1, keepdim=True)
    db_img, db_txt = unit(torch.randn(ndb, d, generator=g)), unit(torch.randn(ndb, d, generator=g))
    dup = min(20, ndb // 2)
    db_img[ndb - dup:], db_txt[ndb - dup:] = db_img[:dup], db_txt[:dup]                  # duplicated rows: ties
    from_db = torch.arange(120) * 7 % ndb                                                # 120 queries are DB rows
    q_img = torch.cat([db_img[from_db], unit(torch.randn(nq - 120, d, generator=g))])
    q_txt = torch.cat([db_txt[from_db], unit(torch.randn(nq - 120, d, generator=g))])
    in_db = np.r_[np.ones(120, np.uint8), np.zeros(nq - 120, np.uint8)]
    lab_db = torch.randint(0, 5, (ndb,), generator=g).numpy().astype(np.int32)
    lab_q = torch.randint(0, 5, (nq,), generator=g).numpy().astype(np.int32)
    return db_img.cuda(), db_txt.cuda(), q_img.cuda(), q_txt.cuda(), in_db, lab_db, lab_q


@pytest.mark.parametrize("discrete", [False, True], ids=["text", "discrete"])
@pytest.mark.parametrize("algo", ["f32", "bf16"])
@pytest.mark.parametrize("dist", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("ndb", [300, 20])
def test_prefix_of_a_deep_neighbour_record_is_the_shallow_record(hip, ndb, d, dist, algo, discrete):
    """prefix_record(neighbors(k = 51), k') == neighbors(k = k') on every array, indices included, bit for bit -- also where the
    sample itself is dropped (position 0 where it is in the DB, the last position otherwise) and, with a DB of 20 rows,
    where the I = -1 / NaN tails begin inside the deeper record."""
    import torch
    from lemon_amd import _lib
    from lemon_amd.neighbors import LemonDB, prefix_record
    db_img, db_txt, q_img, q_txt, in_db, lab_db, lab_q = _embeddings(ndb, 200, d, seed=ndb + d)
    db = LemonDB(db_img, db_txt, dist, tr_label_id=lab_db, algo={"f32": _lib.ALGO_F32_MFMA, "bf16": _lib.ALGO_BF16_FILTER}[algo])
    raw = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    for drop_self in (False, True):
        kw = dict(drop_self=drop_self, in_db=in_db if drop_self else None, discrete=discrete, q_label_id=lab_q)
        deep = db.neighbors(q_img, q_txt, 51, **kw)
        if ndb == 20:
            assert bool((deep["I_n"][:, -1] == -1).all()) and bool((deep["I_m"][:, 20:] == -1).all())
            assert any(bool(torch.isnan(v[:, -1]).all()) for v in deep.values() if v.dtype == torch.float32 and v.dim() == 2)
        for k in (1, 2, 5, 30, 50):
            want, got = db.neighbors(q_img, q_txt, k, **kw), prefix_record(deep, k)
            assert set(got) == set(want)
            for key in want:
                assert got[key].is_contiguous() and got[key].shape == want[key].shape, (key, k)
                assert torch.equal(raw(got[key]), raw(want[key])), (key, k, drop_self)


def test_score_splits_with_a_list_of_ks_equals_one_call_per_k(hip):
    """pipeline.score_splits(k = [..]): one neighbour call at max(ks), {k: records} equal to the records of a call per k."""
    import torch
    from lemon_amd.neighbors import LemonDB
    from lemon_amd.pipeline import FIXED_HPARAMS, score_splits
    db_img, db_txt, q_img, q_txt, in_db, lab_db, lab_q = _embeddings(300, 200, 32, seed=11)
    db = LemonDB(db_img, db_txt, "cosine", tr_label_id=lab_db)
    splits = [dict(name="train", img=q_img, txt=q_txt, drop_self=True, in_db=in_db, label_id=lab_q),
              dict(name="val", img=q_img[100:], txt=q_txt[100:], drop_self=False, in_db=None, label_id=lab_q[100:])]
    calls = []
    plain = db.neighbors
    db.neighbors = lambda *a, **kw: (calls.append(a[2]), plain(*a, **kw))[1]
    got = score_splits(db, splits, [10, 1, 5], FIXED_HPARAMS)
    assert calls == [10] and sorted(got) == [1, 5, 10]
    raw = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)
    for k in (1, 5, 10):
        want = score_splits(db, splits, k, FIXED_HPARAMS)
        assert set(got[k]) == set(want) == {"train", "val"}
        for name in want:
            assert set(got[k][name]) == set(want[name])
            for key in want[name]:
                assert torch.equal(raw(got[k][name][key].contiguous()), raw(want[name][key].contiguous())), (k, name, key)


# ---- the CLI sweep against the single runs -----------------------------------------------------------------------------------
SWEEP = [1, 5, 10]
BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:1500", "--clip_path", "random:tiny",
        "--hparam_grid", "small"]
MODES = {"debug": ["--debug"], "train": ["--compr_dataset_size_limit", "800"]}


def _same(a, b, path="agg_results"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for key in a:
            _same(a[key], b[key], f"{path}[{key!r}]")
    elif isinstance(a, (list, tuple, np.ndarray)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path
    elif isinstance(a, (float, np.floating)):
        assert _bits(a) == _bits(b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def _load(out):
    return pickle.load(open(os.path.join(out, "res.pkl"), "rb"))


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ksweep_cache"))


@pytest.fixture(scope="module")
def single_runs(hip, tmp_path_factory, cache_dir):
    """{mode: {k: output dir}} of the single --knn_k runs, made once per mode on first use."""
    from lemon_amd.run_lemon import main
    done = {}

    def get(mode):
        if mode not in done:
            done[mode] = {}
            for k in SWEEP:
                out = str(tmp_path_factory.mktemp(f"single_{mode}_{k}"))
                assert main(["--output_dir", out, *BASE, *MODES[mode], "--embedding_cache", cache_dir, "--knn_k", str(k)]) == 0
                done[mode][k] = out
        return done[mode]
    return get


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_sweep_equals_the_single_runs(hip, tmp_path, cache_dir, single_runs, mode):
    import pandas as pd
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, *MODES[mode], "--embedding_cache", cache_dir, "--knn_k_sweep", "10,1,5,5"]) == 0
    singles = single_runs(mode)
    selected = {}
    for k in SWEEP:
        sub, one = os.path.join(out, f"knn_k={k}"), singles[k]
        for f in ("args.json", "res.pkl", "know_val_labels_scores.csv", "done"):
            assert os.path.exists(os.path.join(sub, f)), (k, f)
        assert not os.path.exists(os.path.join(sub, "need_hparam_optim"))
        got, want = _load(sub), _load(one)
        pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
        assert got["df"]["D_n"].iloc[0].shape == (k,)
        if mode == "train":
            assert (got["df"].sset == "train").sum() == 1200
        _same(got["agg_results"], want["agg_results"])
        csv = "know_val_labels_scores.csv"
        assert open(os.path.join(sub, csv), "rb").read() == open(os.path.join(one, csv), "rb").read(), k
        a, b = json.load(open(os.path.join(sub, "args.json"))), json.load(open(os.path.join(one, "args.json")))
        assert a["knn_k"] == k and a["output_dir"] == sub
        for skip in ("output_dir", "knn_k", "knn_k_sweep"):
            a.pop(skip), b.pop(skip)
        assert a == b
        selected[k] = want["agg_results"]["know_val_labels"]["selected_val"]
    sel = json.load(open(os.path.join(out, "k_selection.json")))
    best = min(selected, key=lambda k: (-selected[k], k))
    assert sel["best_k"] == best and sel["ks"] == SWEEP
    for k in SWEEP:
        entry, agg = sel["per_k"][str(k)], _load(singles[k])["agg_results"]["know_val_labels"]
        assert entry["selected_val"] == agg["selected_val"] and entry["thres"] == agg["thres"]
        assert [entry[name] for name in ("beta", "gamma", "tau_1_n", "tau_2_n", "tau_1_m", "tau_2_m")] == \
            [float(agg[name]) for name in ("beta", "gamma", "tau_1_n", "tau_2_n", "tau_1_m", "tau_2_m")]
        for sset in ("val", "test"):
            assert entry["splits"][sset] == {"AUROC": agg[sset]["AUROC"], "F1_optimal": agg[sset]["F1_optimal"]}
    assert os.path.exists(os.path.join(out, "done"))


def test_cli_sweep_without_hparam_optim_selects_nothing(hip, tmp_path, cache_dir, single_runs):
    import pandas as pd
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep_skip")
    assert main(["--output_dir", out, *BASE, "--debug", "--embedding_cache", cache_dir, "--knn_k_sweep", "1,5,10",
                 "--skip_hparam_optim"]) == 0
    sel = json.load(open(os.path.join(out, "k_selection.json")))
    assert sel["best_k"] is None and sel["per_k"] == {"1": None, "5": None, "10": None}
    singles = single_runs("debug")
    for k in SWEEP:
        sub = os.path.join(out, f"knn_k={k}")
        res = _load(sub)
        assert "agg_results" not in res and os.path.exists(os.path.join(sub, "need_hparam_optim"))
        assert os.path.exists(os.path.join(sub, "done"))
        pd.testing.assert_frame_equal(res["df"], _load(singles[k])["df"][list(res["df"].columns)], check_exact=True)
    assert os.path.exists(os.path.join(out, "done"))
