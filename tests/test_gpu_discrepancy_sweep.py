"""GPU: lemon_discrepancy_ks / lemon_discrepancy_cache (k_discrepancy_ks, discrepancy_ks.hip) -- every method and every knn_k of
a list from one search -- against what they replace: discrepancy_scores per (method, k) bit for bit, the host twin bit for bit,
the cache's life across splits and adds, the refusals, and the CLI's --method_sweep / --knn_k_sweep against single runs and the
reference script's recorded runs, on one rank and on two."""
import ctypes
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import discsweep as ds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
E_INVALID = -1
PATTERN = 0x7FC12345                                    # a quiet NaN no kernel produces


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pattern(*shape):
    return torch.full(shape, PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)


def _is_pattern(t):
    return t.contiguous().view(torch.int32) == PATTERN


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ks_c(ks):
    return (ctypes.c_int32 * len(ks))(*ks)


def _sweep_into(out, db, qi, qt, ks, methods, is_train, cache):
    """lemon_discrepancy_ks into a buffer of the test's own ([4, K, nq] in the order of ds.METHODS); returns the status"""
    from lemon_amd import _lib as L
    bits = sum(1 << ds.METHODS.index(m) for m in methods)
    return L.load().lemon_discrepancy_ks(db.index_txt._h, _p(db.img), _p(db.txt), _p(qi), _p(qt), qt.shape[0], _ks_c(ks), len(ks),
                                         int(is_train), bits, _p(cache), 0 if cache is None else cache.shape[0],
                                         0 if cache is None else cache.shape[1], _p(out), _stream())


# ---- 1. equality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DIMS)                  # 3, 33: every lane walks its rows; 36, 100: the staged walk
def test_sweep_equals_single_calls_and_the_host_twin(hip, oracle, d):
    from lemon_amd.baselines import discrepancy_cache, discrepancy_scores, discrepancy_sweep
    for db_case in ds.databases(d):
        _, img_tr, txt_tr, _, _ = db_case
        db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
        cache = discrepancy_cache(db, ds.KS[-1])
        assert cache.shape == (img_tr.shape[0], ds.KS[-1] + 1) and cache.dtype == torch.int64
        for what, q_img, q_txt, is_train in ds.query_sets(db_case):                # nq = 1, 7 (odd), 64
            qi, qt = cu(q_img), cu(q_txt)
            out = _pattern(4, len(ds.KS), q_txt.shape[0])
            assert _sweep_into(out, db, qi, qt, ds.KS, ds.METHODS, is_train, cache) == 0
            assert not bool(_is_pattern(out).any()), (what, "an element was not written")
            got = discrepancy_sweep(db, qi, qt, ds.KS, is_train=is_train, cache=cache)
            assert torch.equal(got.view(torch.int32), out.view(torch.int32)), what
            got = got.cpu().numpy()
            for mi, m in enumerate(ds.METHODS):
                for t, k in enumerate(ds.KS):
                    one = discrepancy_scores(db, qi, qt, k, m, is_train=is_train).cpu().numpy()
                    assert ds.same_bits(got[mi, t], one), (what, d, m, k)
                twin = ds.host_sweep(oracle, m, img_tr, txt_tr, q_img, q_txt, ds.KS, is_train)
                assert ds.same_bits(got[mi], twin), (what, d, m, "host twin")


@pytest.mark.parametrize("d", [33, 36])
def test_one_method_leaves_the_other_rows_alone(hip, d):
    from lemon_amd.baselines import discrepancy_cache, discrepancy_sweep
    db_case = ds.databases(d)[1]
    _, img_tr, txt_tr, q_img, q_txt = db_case
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
    qi, qt = cu(q_img[:7]), cu(q_txt[:7])
    ks = [2, 5, 31]
    full = discrepancy_sweep(db, qi, qt, ks)
    cache = discrepancy_cache(db, ks[-1])
    for mi, m in enumerate(ds.METHODS):
        out = _pattern(4, len(ks), 7)
        assert _sweep_into(out, db, qi, qt, ks, [m], False, cache if m.startswith("dis") else None) == 0
        got = discrepancy_sweep(db, qi, qt, ks, methods=[m])                       # (builds its own cache for dis_*)
        assert got.shape == (1, len(ks), 7) and torch.equal(got[0].view(torch.int32), full[mi].view(torch.int32)), m
        assert torch.equal(out[mi].view(torch.int32), full[mi].view(torch.int32)), m
        others = [r for r in range(4) if r != mi]
        assert bool(_is_pattern(out[others]).all()) and not bool(_is_pattern(out[mi]).any()), m
    # the orders given are the orders returned
    got = discrepancy_sweep(db, qi, qt, ks, methods=["div_y", "dis_x"])
    assert torch.equal(got.view(torch.int32), full[[3, 0]].view(torch.int32))


# ---- 2. one cache for several splits -----------------------------------------------------------------------------------------
def test_one_cache_serves_three_query_sets(hip):
    from lemon_amd.baselines import discrepancy_cache, discrepancy_scores, discrepancy_sweep
    _, img_tr, txt_tr, q_img, q_txt = ds.databases(36)[1]
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
    cache = discrepancy_cache(db, 20)
    kept = cache.clone()
    ks = [1, 5, 20]
    for q_i, q_t, is_train in [(img_tr[:64], txt_tr[:64], True), (q_img[:33], q_txt[:33], False), (q_img[33:], q_txt[33:], False)]:
        got = discrepancy_sweep(db, cu(q_i), cu(q_t), ks, is_train=is_train, cache=cache).cpu().numpy()
        for mi, m in enumerate(ds.METHODS):
            for t, k in enumerate(ks):
                assert ds.same_bits(got[mi, t], discrepancy_scores(db, cu(q_i), cu(q_t), k, m, is_train=is_train).cpu().numpy()), (m, k)
    assert torch.equal(cache, kept)                      # the single calls in between use the index's workspace, not the cache
    # a wider cache than the list needs serves as well (an exact list is a prefix of every deeper one)
    a = discrepancy_sweep(db, cu(q_img), cu(q_txt), [1, 5], cache=cache)
    b = discrepancy_sweep(db, cu(q_img), cu(q_txt), [1, 5])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 3. / 4. refusals --------------------------------------------------------------------------------------------------------
def test_stale_and_narrow_caches_are_refused(hip):
    from lemon_amd import _lib as L
    from lemon_amd.baselines import discrepancy_cache, discrepancy_sweep
    lib = L.load()
    _, img_tr, txt_tr, q_img, q_txt = ds.databases(36)[1]
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
    qi, qt, nq = cu(q_img[:7]), cu(q_txt[:7]), 7
    cache = discrepancy_cache(db, 10)
    n = db.index_txt.ntotal

    def call(ks, methods, Ic, rows, kc, out):
        return lib.lemon_discrepancy_ks(db.index_txt._h, _p(db.img), _p(db.txt), _p(qi), _p(qt), nq, _ks_c(ks), len(ks), 0, methods,
                                        _p(Ic), rows, kc, _p(out), _stream())

    def intact(out):
        torch.cuda.synchronize()
        return bool(_is_pattern(out).all())

    # narrower than max(ks) + 1
    out = _pattern(4, 2, nq)
    assert call([5, 11], 15, cache, n, cache.shape[1], out) == E_INVALID and intact(out)
    with pytest.raises(ValueError):
        discrepancy_sweep(db, qi, qt, [5, 11], cache=cache)
    # ... which div alone does not read
    assert call([5, 11], 12, None, 0, 0, out) == 0 and not bool(_is_pattern(out[2:]).any()) and bool(_is_pattern(out[:2]).all())
    # lists and method sets out of contract
    for ks, methods in [([5, 5], 15), ([5, 2], 15), ([0, 2], 15), ([2, 64], 12), ([2, 5], 0), ([2, 5], 16)]:
        out = _pattern(4, 2, nq)
        assert call(ks, methods, cache, n, cache.shape[1], out) == E_INVALID and intact(out), (ks, methods)
    out = _pattern(4, 2, nq)
    assert call([2, 5], 3, None, n, 11, out) == E_INVALID and intact(out)          # dis without a cache
    assert call([2, 5], 15, cache, n, cache.shape[1], out) == 0
    # rows added to the index: the cache belongs to the old row count
    db.index_txt.add(cu(txt_tr[:3]))
    assert db.index_txt.ntotal == n + 3
    out = _pattern(4, 2, nq)
    assert call([2, 5], 15, cache, cache.shape[0], cache.shape[1], out) == E_INVALID and intact(out)
    assert b"cache" in lib.lemon_last_error()
    with pytest.raises(ValueError):
        discrepancy_sweep(db, qi, qt, [2, 5], cache=cache)
    out = _pattern(4, 2, nq)
    assert lib.lemon_discrepancy_cache(db.index_txt._h, 1, _p(out), _stream()) == E_INVALID and intact(out)
    assert lib.lemon_discrepancy_cache(db.index_txt._h, 65, _p(out), _stream()) == E_INVALID and intact(out)


def test_rows_off_a_16_byte_boundary_are_refused(hip):
    from lemon_amd import _lib as L
    from lemon_amd.baselines import discrepancy_cache
    from tests.test_gpu_record_paths import _off_by_one
    lib = L.load()
    _, img_tr, txt_tr, q_img, q_txt = ds.databases(36)[1]                          # d % 4 == 0
    db = hip.LemonDB(cu(img_tr), cu(txt_tr), "cosine")
    nq, ks = 7, [2, 5]
    cache = discrepancy_cache(db, 5)
    qi, qt = cu(q_img[:nq]), cu(q_txt[:nq])
    qi_v, qt_v, Ei_v, Et_v = _off_by_one(q_img[:nq]), _off_by_one(q_txt[:nq]), _off_by_one(img_tr), _off_by_one(txt_tr)
    for name, Ei, Et, a, b in [("E_img", Ei_v, db.txt, qi, qt), ("E_txt", db.img, Et_v, qi, qt), ("q_img", db.img, db.txt, qi_v, qt),
                               ("q_txt", db.img, db.txt, qi, qt_v)]:
        out = _pattern(4, len(ks), nq)
        rc = lib.lemon_discrepancy_ks(db.index_txt._h, _p(Ei), _p(Et), _p(a), _p(b), nq, _ks_c(ks), len(ks), 0, 15, _p(cache),
                                      cache.shape[0], cache.shape[1], _p(out), _stream())
        assert rc == E_INVALID and b"16-byte aligned" in lib.lemon_last_error(), name
        torch.cuda.synchronize()
        assert bool(_is_pattern(out).all()), name


# ---- 5. the CLI on the reference script's fixtures ---------------------------------------------------------------------------
def _fixture(m):
    fx = np.load(os.path.join(G, f"disc_{m}.npz"))
    argv = json.loads(str(fx["argv"]))
    return fx, argv, int(argv[argv.index("--knn_k") + 1])


def _pred(path):
    return pickle.load(open(os.path.join(path, "res.pkl"), "rb"))


@pytest.mark.parametrize("m", ds.METHODS)
def test_cli_sweep_reproduces_single_runs_and_the_reference_run(hip, m, monkeypatch, tmp_path):
    from types import SimpleNamespace
    from lemon_amd.discrepancy_baseline import main
    from tests import planted
    fx, argv, k = _fixture(m)
    extra = planted.install(SimpleNamespace(fx=fx, is_caption=False, dataset="cifar10"), monkeypatch, tmp_path)
    sweep, single = str(tmp_path / "sweep"), str(tmp_path / "single")
    ks = [1, k, k + 3]
    assert main(["--output_dir", sweep] + argv + extra + ["--method_sweep", "all", "--knn_k_sweep", ",".join(map(str, ks))]) == 0
    assert main(["--output_dir", single] + argv + extra) == 0
    assert sorted(os.listdir(single)) == sorted(str(f) for f in fx["out_files"])
    top = sorted(os.listdir(sweep))
    assert top == sorted(["args.json", "out.txt", "err.txt", "sweep.json", "done"] + [f"method={x}" for x in ds.METHODS])
    record = json.load(open(os.path.join(sweep, "sweep.json")))
    assert record["methods"] == list(ds.METHODS) and record["ks"] == ks
    sub_files = sorted(set(os.listdir(single)) - {"out.txt", "err.txt"})
    for x in ds.METHODS:
        assert sorted(os.listdir(os.path.join(sweep, f"method={x}"))) == sorted(f"knn_k={v}" for v in ks)
        for v in ks:
            sub = os.path.join(sweep, f"method={x}", f"knn_k={v}")
            assert sorted(os.listdir(sub)) == sub_files, (x, v)
            sub_args = json.load(open(os.path.join(sub, "args.json")))
            assert (sub_args["method"], sub_args["knn_k"], sub_args["output_dir"]) == (x, v, sub)
            res = _pred(sub)
            for s, r in res["agg_results"].items():
                assert record["results"][x][str(v)][s]["AUROC"] == float(r["AUROC"]), (x, v, s)
                assert record["results"][x][str(v)][s]["F1_optimal"] == float(r["F1_optimal"]), (x, v, s)
    mine, one = _pred(os.path.join(sweep, f"method={m}", f"knn_k={k}"))["df"], _pred(single)["df"]
    assert list(mine.columns) == list(one.columns) and len(mine) == len(one)
    assert np.array_equal(mine["pred_score"].values.view(np.uint64), one["pred_score"].values.view(np.uint64))
    for col in ("sset", "idx", "is_mislabel", "noisy_label_text"):
        assert (mine[col].values == one[col].values).all(), col
    for s in fx["ssets"]:
        s = str(s)
        assert np.abs(mine[mine.sset == s]["pred_score"].values - fx[f"{s}_pred_score"]).max() <= 2e-6, (m, s)


# ---- 6. two ranks on one card -------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(m, out_dir, data_dir, world, sweep_args):
    port = _free_port()
    procs = []
    os.makedirs(out_dir, exist_ok=True)
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LEMON_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        if world == 1:
            for k_ in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
                env.pop(k_)
        log = open(os.path.join(out_dir, f"rank{r}.log"), "wb")      # a file per rank: no pipe to fill while a rank waits in a collective
        procs.append((subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "disc_sweep_worker.py"), m, out_dir, data_dir] + sweep_args,
                                       env=env, stdout=log, stderr=subprocess.STDOUT), log))
    for pr, log in procs:
        pr.wait(timeout=600)
        log.close()
    outs = [open(os.path.join(out_dir, f"rank{r}.log")).read() for r in range(world)]
    assert all(pr.returncode == 0 for pr, _ in procs), "\n".join(outs)[-3000:]


def test_two_ranks_on_one_card_equal_one_rank(hip, tmp_path):
    m = "dis_x"
    fx, argv, k = _fixture(m)
    ks = [1, k, k + 3]
    sweep_args = ["--method_sweep", "all", "--knn_k_sweep", ",".join(map(str, ks))]
    w1, w2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    _launch(m, w1, str(tmp_path / "d1"), 1, sweep_args)
    _launch(m, w2, str(tmp_path / "d2"), 2, sweep_args)
    assert json.load(open(os.path.join(w1, "sweep.json")))["results"] == json.load(open(os.path.join(w2, "sweep.json")))["results"]
    for x in ds.METHODS:
        for v in ks:
            a = _pred(os.path.join(w1, f"method={x}", f"knn_k={v}"))["df"]
            b = _pred(os.path.join(w2, f"method={x}", f"knn_k={v}"))["df"]
            assert len(a) == len(b) and (a["sset"].values == b["sset"].values).all() and (a["idx"].values == b["idx"].values).all()
            assert np.array_equal(a["pred_score"].values.view(np.uint64), b["pred_score"].values.view(np.uint64)), (x, v)
    one = _pred(os.path.join(w2, f"method={m}", f"knn_k={k}"))["df"]
    for s in fx["ssets"]:
        s = str(s)
        assert np.abs(one[one.sset == s]["pred_score"].values - fx[f"{s}_pred_score"]).max() <= 2e-6, s
