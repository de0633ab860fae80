"""GPU: the cell sweep (run_lemon --ablation_sweep / --subset_val_set_sweep, composed with --knn_k_sweep / --dist_type_sweep)
against the single runs it stands for, and ops.local_search / ops.lbfgs_polish with cells= against one call per cell.
Comparison rules: every float bit for bit (viewed as integers, NaN included), frames with check_exact, files byte for byte; no
tolerances.

ops shapes: records of n = 1 (one thread), 63 (under a wave), 257 (a block and one more), depth kmax = 2 and 51 (shallow; the
reference's deepest + the train split's one more), ks = [1, kmax], the mask pairs of all seven ablations that search and one of
them again.  The searches run under the iteration caps of lemon_hparam_search_set_test_knobs, which bind every search alike.

CLI: synthetic:600 splits 480 / 60 / 60; at data_seed 0 the validation set has 19 mislabels, the m = 10 draw 5 (both classes
present), the m = 2 draw none (AUROC = nan, F1 = 0), and m = 1 fails in gaussian_kde as the single run does."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import hparamfx as fx

pytestmark = pytest.mark.gpu

CELLS = [fx.ABLATIONS[a] for a in ("none", "tau_1", "tau_2", "tau_1_2", "beta", "gamma", "d1")] + [fx.ABLATIONS["tau_1"]]
STARTS = [list(s) for s in fx.STARTS]


def _cuda(rec):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in rec.items()}


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.int64)


def _same_rows(got, want, what):
    """two results of local_search / lbfgs_polish with return_info: arrays and floats by their bits, integers equal"""
    assert len(got) == len(want), what
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 5, what
        for i, (a, b) in enumerate(zip(g, w)):
            if isinstance(b, (np.ndarray, float)):
                assert np.array_equal(_bits(a), _bits(b)), (what, s, i, a, b)
            else:
                assert isinstance(b, int) and a == b, (what, s, i, a, b)


@pytest.fixture()
def capped(hip):
    from lemon_amd import _lib
    lib = _lib.load()
    lib.lemon_hparam_search_set_test_knobs(0, 25, 40, 2, 60)           # Nelder-Mead maxiter / maxfev, Powell maxiter / maxfev
    yield
    lib.lemon_hparam_search_set_test_knobs(0, 0, 0, 0, 0)


@pytest.mark.parametrize("kmax", [2, 51])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_local_search_cells_equal_one_call_per_cell(hip, capped, n, kmax):
    from lemon_amd import ops
    rec, y = fx.record(n, kmax=kmax, seed=5)
    dev, ks = _cuda(rec), [1, kmax]
    together = ops.local_search(dev, y, STARTS, fx.METHODS, ks=ks, return_info=True, cells=CELLS)
    assert len(together) == len(CELLS) and all(len(c) == 2 and all(len(per_k) == 8 for per_k in c) for c in together)
    for c, (fz, fo) in enumerate(CELLS):
        one = ops.local_search(dev, y, STARTS, fx.METHODS, fz, fo, ks=ks, return_info=True)
        for t, k in enumerate(ks):
            _same_rows(together[c][t], one[t], f"n={n} kmax={kmax} cell={c} k={k}")
    assert any(g[2] > 1 for g in together[0][1])                                          # the searches did move
    _same_rows(together[-1][1], together[1][1], "the repeated pair")
    # without ks: the record's own depth, one flat list per cell; the plain form is (x, fun)
    flat = ops.local_search(dev, y, STARTS[:2], fx.METHODS, cells=CELLS[:3])
    assert len(flat) == 3 and all(len(c) == 4 and len(c[0]) == 2 for c in flat)
    for c in range(3):
        want = ops.local_search(dev, y, STARTS[:2], fx.METHODS, *CELLS[c])
        assert all(np.array_equal(_bits(g[0]), _bits(w[0])) and _bits(g[1]) == _bits(w[1]) for g, w in zip(flat[c], want))


@pytest.mark.parametrize("kmax", [2, 51])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_lbfgs_polish_cells_equal_one_call_per_cell(hip, n, kmax):
    from lemon_amd import ops
    rec, y = fx.record(n, kmax=kmax, seed=5)
    dev, ks = _cuda(rec), [1, kmax]
    together = ops.lbfgs_polish(dev, y, STARTS, ks=ks, return_info=True, cells=CELLS)
    assert len(together) == len(CELLS) and all(len(c) == 2 and all(len(per_k) == 4 for per_k in c) for c in together)
    for c, (fz, fo) in enumerate(CELLS):
        one = ops.lbfgs_polish(dev, y, STARTS, fz, fo, ks=ks, return_info=True)
        for t, k in enumerate(ks):
            _same_rows(together[c][t], one[t], f"n={n} kmax={kmax} cell={c} k={k}")
    _same_rows(together[-1][1], together[1][1], "the repeated pair")
    flat = ops.lbfgs_polish(dev, y, STARTS[:2], cells=CELLS[:3])
    assert len(flat) == 3 and all(len(c) == 2 and len(c[0]) == 2 for c in flat)
    for c in range(3):
        want = ops.lbfgs_polish(dev, y, STARTS[:2], *CELLS[c])
        assert all(np.array_equal(_bits(g[0]), _bits(w[0])) and g[1] == w[1] for g, w in zip(flat[c], want))


def test_refused_calls_still_raise(hip):
    from lemon_amd import ops
    rec, y = fx.record(63, kmax=2)
    dev = _cuda(rec)
    for fn in (ops.local_search, ops.lbfgs_polish):
        with pytest.raises(ValueError):
            fn(dev, y, STARTS, cells=[])
        with pytest.raises(ValueError):
            fn(dev, y, STARTS, cells=[((), ()), (("tau_3",), ())])
        with pytest.raises(ValueError):
            fn(dev, y, STARTS, force_zero=("tau_3",))
        with pytest.raises(ValueError):
            fn(dev, y, STARTS, ks=[3], cells=[((), ())])
        with pytest.raises(ValueError):
            fn(dev, y, STARTS, force_zero=("beta",), cells=[((), ())])


# ---- the CLI sweep against the single runs it stands for ---------------------------------------------------------------------
BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:600", "--clip_path", "random:tiny",
        "--hparam_grid", "small"]
DEVICE = ["--hparam_search", "device", "--lbfgs_polish", "device"]
SWEPT_KEYS = ("output_dir", "knn_k", "knn_k_sweep", "dist_type", "dist_type_sweep", "dist_sweep_margin", "ablation", "ablation_sweep",
              "subset_val_set", "subset_val_set_sweep")
HP = ("beta", "gamma", "tau_1_n", "tau_2_n", "tau_1_m", "tau_2_m")
CSV = "know_val_labels_scores.csv"


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
    return str(tmp_path_factory.mktemp("cell_sweep_cache"))


@pytest.fixture(scope="module")
def single(hip, tmp_path_factory, cache_dir):
    """the single run of a cell, made once on first use -> its output directory"""
    from lemon_amd.run_lemon import main
    done = {}

    def get(m, a, k, dist="cosine", mode=("--debug",), where=DEVICE, rc=0):
        key = (m, a, k, dist, tuple(mode), tuple(where))
        if key not in done:
            out = str(tmp_path_factory.mktemp("single"))
            assert main(["--output_dir", out, *BASE, *mode, *where, "--embedding_cache", cache_dir, "--subset_val_set", str(m),
                         "--ablation", a, "--knn_k", str(k), "--dist_type", dist]) == rc
            done[key] = out
        return done[key]
    return get


def _assert_cell_is_the_single_run(sub, one, m, a, k, dist="cosine"):
    import pandas as pd
    for f in ("args.json", "res.pkl", CSV, "done"):
        assert os.path.exists(os.path.join(sub, f)), (sub, f)
    assert not os.path.exists(os.path.join(sub, "need_hparam_optim"))
    got, want = _load(sub), _load(one)
    pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
    assert got["df"]["D_n"].iloc[0].shape == (k,)
    _same(got["agg_results"], want["agg_results"])
    assert open(os.path.join(sub, CSV), "rb").read() == open(os.path.join(one, CSV), "rb").read(), sub
    x, y = json.load(open(os.path.join(sub, "args.json"))), json.load(open(os.path.join(one, "args.json")))
    assert (x["subset_val_set"], x["ablation"], x["knn_k"], x["dist_type"], x["output_dir"]) == (m, a, k, dist, sub)
    for skip in SWEPT_KEYS:
        x.pop(skip), y.pop(skip)
    assert x == y
    return want


def _assert_entry_is_the_single_run(entry, want):
    agg = want["agg_results"]["know_val_labels"]
    assert entry["status"] == "ok" and "error" not in entry
    assert entry["selected_val"] == agg.get("selected_val") and entry["thres"] == agg.get("thres")      # None: only_beta / only_gamma
    assert [entry[name] for name in HP] == [float(agg[name]) for name in HP]
    for sset in want["df"].sset.unique():
        _same(entry["splits"][sset], {"AUROC": float(agg[sset]["AUROC"]), "F1_optimal": float(agg[sset]["F1_optimal"])})


SUBSETS, ABLS, KS = [-1, 10, 59, 60, 500], ["none", "multimodal_baseline", "tau_1", "d1", "only_beta"], [1, 5]
COMPARED = [(-1, "none", 1), (500, "d1", 5), (10, "multimodal_baseline", 5), (10, "none", 5), (59, "tau_1", 1), (60, "only_beta", 1),
            (-1, "d1", 5), (60, "tau_1", 5)]


@pytest.fixture(scope="module")
def debug_sweep(hip, tmp_path_factory, cache_dir):
    from lemon_amd.run_lemon import main
    out = str(tmp_path_factory.mktemp("sweep"))
    rc = main(["--output_dir", out, *BASE, "--debug", *DEVICE, "--embedding_cache", cache_dir, "--subset_val_set_sweep",
               "-1,10,59,60,500,10", "--ablation_sweep", ",".join(ABLS), "--knn_k_sweep", "5,1"])
    return out, rc


def test_the_sweep_lays_out_every_cell(debug_sweep):
    out, rc = debug_sweep
    assert rc == 0 and os.path.exists(os.path.join(out, "done"))
    info = json.load(open(os.path.join(out, "cell_sweep.json")))
    assert info["axes"] == {"dist_type": None, "subset_val_set": SUBSETS, "ablation": ABLS, "knn_k": KS}
    assert [c["path"] for c in info["cells"]] == [f"subset_val_set={m}/ablation={a}/knn_k={k}" for m in SUBSETS for a in ABLS for k in KS]
    for c in info["cells"]:
        assert c["status"] == "ok" and (c["subset_val_set"], c["ablation"], c["knn_k"], c["dist_type"]) == \
            tuple(int(v) if v.lstrip("-").isdigit() else v for v in (p.split("=")[1] for p in c["path"].split("/"))) + ("cosine",)
        for f in ("args.json", "res.pkl", CSV, "done"):
            assert os.path.exists(os.path.join(out, c["path"], f)), (c["path"], f)
    for m in SUBSETS:
        n_val = 60 if m == -1 else min(m, 60)
        for a in ABLS:
            above = os.path.join(out, f"subset_val_set={m}", f"ablation={a}")
            sel = json.load(open(os.path.join(above, "k_selection.json")))             # one level above knn_k=
            assert sel["ks"] == KS and sorted(sel["per_k"]) == ["1", "5"] and os.path.exists(os.path.join(above, "done"))
            df = _load(os.path.join(above, "knn_k=5"))["df"]
            assert (df.sset == "val").sum() == n_val and list(df[df.sset == "val"].idx) == list(range(n_val))
    # the two classes of the draws this file's cases rest on
    whole = _load(os.path.join(out, "subset_val_set=-1", "ablation=none", "knn_k=5"))["df"]
    ten = _load(os.path.join(out, "subset_val_set=10", "ablation=none", "knn_k=5"))["df"]
    assert whole[whole.sset == "val"].is_mislabel.sum() == 19 and ten[ten.sset == "val"].is_mislabel.sum() == 5
    # cells do not see each other's writes: d_1 is zero in the d1 cells and nowhere else
    for a in ABLS:
        d1 = _load(os.path.join(out, "subset_val_set=10", f"ablation={a}", "knn_k=1"))["df"].d_1.values
        assert bool((d1 == 0).all()) == (a == "d1")


@pytest.mark.parametrize("m,a,k", COMPARED, ids=[f"{m}-{a}-{k}" for m, a, k in COMPARED])
def test_cli_sweep_equals_the_single_runs(debug_sweep, single, m, a, k):
    out, _ = debug_sweep
    path = f"subset_val_set={m}/ablation={a}/knn_k={k}"
    want = _assert_cell_is_the_single_run(os.path.join(out, path), single(m, a, k), m, a, k)
    entry = next(c for c in json.load(open(os.path.join(out, "cell_sweep.json")))["cells"] if c["path"] == path)
    _assert_entry_is_the_single_run(entry, want)
    sel = json.load(open(os.path.join(out, f"subset_val_set={m}", f"ablation={a}", "k_selection.json")))["per_k"][str(k)]
    assert sel == {key: v for key, v in entry.items() if key in sel} and "selected_val" in sel


def test_cli_sweep_with_the_train_split_and_a_subset_db(hip, tmp_path, cache_dir, single):
    """without --debug: the train rows exclude themselves; --compr_dataset_size_limit 300: the DB is a drawn subset of them"""
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    mode = ("--compr_dataset_size_limit", "300")
    assert main(["--output_dir", out, *BASE, *mode, *DEVICE, "--embedding_cache", cache_dir, "--subset_val_set_sweep", "-1,10",
                 "--ablation_sweep", "none,d1", "--knn_k", "5"]) == 0
    for m in (-1, 10):
        for a in ("none", "d1"):
            sub = os.path.join(out, f"subset_val_set={m}", f"ablation={a}")
            want = _assert_cell_is_the_single_run(sub, single(m, a, 5, mode=mode), m, a, 5)
            assert (want["df"].sset == "train").sum() == 480
            assert not os.path.exists(os.path.join(sub, "k_selection.json"))
    assert os.path.exists(os.path.join(out, "done")) and os.path.exists(os.path.join(out, "out.txt"))


def test_cli_sweep_crossed_with_the_metric_sweep(hip, tmp_path, cache_dir, single):
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, "--debug", *DEVICE, "--embedding_cache", cache_dir, "--dist_type_sweep", "cosine,euclidean",
                 "--subset_val_set_sweep", "-1,10", "--ablation_sweep", "none,tau_2", "--knn_k", "5"]) == 0
    info = json.load(open(os.path.join(out, "cell_sweep.json")))
    assert info["axes"] == {"dist_type": ["cosine", "euclidean"], "subset_val_set": [-1, 10], "ablation": ["none", "tau_2"], "knn_k": None}
    assert [c["path"] for c in info["cells"]] == [f"dist_type={d}/subset_val_set={m}/ablation={a}" for d in ("cosine", "euclidean")
                                                  for m in (-1, 10) for a in ("none", "tau_2")]
    for c in info["cells"]:
        assert c["status"] == "ok" and os.path.exists(os.path.join(out, c["path"], "done"))
        assert not os.path.exists(os.path.join(out, c["path"], "knn_k=5"))
    assert sorted(os.listdir(os.path.join(out, "dist_type=euclidean"))) == ["args.json", "subset_val_set=-1", "subset_val_set=10"]
    assert os.path.exists(os.path.join(out, "dist_sweep.json")) and os.path.exists(os.path.join(out, "done"))
    path = "dist_type=euclidean/subset_val_set=10/ablation=tau_2"
    want = _assert_cell_is_the_single_run(os.path.join(out, path), single(10, "tau_2", 5, dist="euclidean"), 10, "tau_2", 5, "euclidean")
    _assert_entry_is_the_single_run(next(c for c in info["cells"] if c["path"] == path), want)


def test_one_cell_in_the_host_modes(hip, tmp_path, cache_dir, single):
    """--hparam_search host --lbfgs_polish host (the defaults): scipy and torch.optim.LBFGS on the cell's own 10 rows"""
    import pandas as pd
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, "--debug", "--embedding_cache", cache_dir, "--subset_val_set_sweep", "10",
                 "--ablation_sweep", "none", "--knn_k_sweep", "1"]) == 0
    got = _load(os.path.join(out, "subset_val_set=10", "ablation=none", "knn_k=1"))
    want = _load(single(10, "none", 1, where=()))
    pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
    assert "know_val_labels_pred_score" in got["df"].columns
    g, w = got["agg_results"]["know_val_labels"], want["agg_results"]["know_val_labels"]
    for key in ("selected_val", "thres") + HP:
        assert _bits(g[key]) == _bits(w[key]), key


def test_a_failing_cell_is_recorded_and_the_sweep_goes_on(hip, tmp_path, cache_dir, single):
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, "--debug", *DEVICE, "--embedding_cache", cache_dir, "--subset_val_set_sweep", "-1,1",
                 "--knn_k", "5"]) == 1
    info = json.load(open(os.path.join(out, "cell_sweep.json")))
    assert info["axes"] == {"dist_type": None, "subset_val_set": [-1, 1], "ablation": None, "knn_k": None}
    whole, one = info["cells"]
    assert (whole["path"], one["path"]) == ("subset_val_set=-1", "subset_val_set=1")
    assert one["status"] == "error" and one["error"] and "selected_val" not in one
    assert os.path.exists(os.path.join(out, "subset_val_set=1", "args.json")) and not os.path.exists(os.path.join(out, "subset_val_set=1", "done"))
    assert not os.path.exists(os.path.join(out, "done"))
    want = _assert_cell_is_the_single_run(os.path.join(out, "subset_val_set=-1"), single(-1, "none", 5), -1, "none", 5)
    _assert_entry_is_the_single_run(whole, want)


def test_a_degenerate_cell_that_does_not_raise_is_the_single_run(hip, tmp_path, cache_dir, single):
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, "--debug", *DEVICE, "--embedding_cache", cache_dir, "--subset_val_set_sweep", "-1,2",
                 "--knn_k", "5"]) == 0
    want = _assert_cell_is_the_single_run(os.path.join(out, "subset_val_set=2"), single(2, "none", 5), 2, "none", 5)
    agg = want["agg_results"]["know_val_labels"]
    assert (want["df"].sset == "val").sum() == 2 and want["df"][want["df"].sset == "val"].is_mislabel.sum() == 0
    assert np.isnan(agg["val"]["AUROC"]) and agg["val"]["F1_optimal"] == 0
    got = _load(os.path.join(out, "subset_val_set=2"))["agg_results"]["know_val_labels"]
    assert np.isnan(got["val"]["AUROC"]) and got["val"]["F1_optimal"] == 0
    assert os.path.exists(os.path.join(out, "done"))


def test_cells_without_hparam_optim_do_what_the_single_run_does(hip, tmp_path, cache_dir):
    """--skip_hparam_optim is no parser error: every cell holds the record, need_hparam_optim and done; d1 still zeroes d_1"""
    import pandas as pd
    from lemon_amd.run_lemon import main
    out, one = str(tmp_path / "sweep"), str(tmp_path / "single")
    assert main(["--output_dir", out, *BASE, "--debug", "--embedding_cache", cache_dir, "--skip_hparam_optim",
                 "--subset_val_set_sweep", "10", "--ablation_sweep", "none,d1", "--knn_k", "5"]) == 0
    assert main(["--output_dir", one, *BASE, "--debug", "--embedding_cache", cache_dir, "--skip_hparam_optim",
                 "--subset_val_set", "10", "--ablation", "d1", "--knn_k", "5"]) == 0
    for a in ("none", "d1"):
        sub = os.path.join(out, "subset_val_set=10", f"ablation={a}")
        res = _load(sub)
        assert "agg_results" not in res and os.path.exists(os.path.join(sub, "need_hparam_optim")) and os.path.exists(os.path.join(sub, "done"))
        assert bool((res["df"].d_1 == 0).all()) == (a == "d1")
    pd.testing.assert_frame_equal(_load(os.path.join(out, "subset_val_set=10", "ablation=d1"))["df"], _load(one)["df"], check_exact=True)
    cells = json.load(open(os.path.join(out, "cell_sweep.json")))["cells"]
    assert [c["status"] for c in cells] == ["ok", "ok"] and all("selected_val" not in c for c in cells)
