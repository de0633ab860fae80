"""GPU: the local searches of the hyper-parameter search in one launch (lemon_hparam_search, ops.local_search) against the
path they replace: scipy.optimize.minimize(options={}) on maximize_metric's host objective (ops.lemon_score -> a copy ->
optimize_f1_efficient).  Comparison rules (tests/hparamfx.py): x bit for bit, fun ==, nfev / nit / status equal; no tolerances.

Shapes: n = 1 (one thread), 64 / 65 (a wave and one more), 257, 1031 (every thread of the 512 with two or three samples and a
tail); k = 5 and 50, and k = 5 as the prefix of a kmax = 51 record; the score row in LDS and in the workspace."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import hparamfx as fx

pytestmark = pytest.mark.gpu


def _cuda(rec):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in rec.items()}


def _prefix(rec, k):
    return {key: (v if key == "d_1" else np.ascontiguousarray(v[:, :k])) for key, v in rec.items()}


def _host_objective(rec_dev, y, force_zero=(), force_one=()):
    """maximize_metric.objective on the product's score_fn"""
    from lemon_amd import metrics as M, ops

    def objective(x):
        score = ops.lemon_score(rec_dev, M.unpack_vector(x, force_zero, force_one)).cpu().numpy()
        if not np.all(np.isfinite(score)):
            return 0.0
        return -M.optimize_f1_efficient(y, score)
    return objective


def _against_scipy(rec, y, k, starts=fx.STARTS, force_zero=(), force_one=(), what=""):
    """ops.local_search at depth k of `rec` against scipy on the contiguous [n, k] record"""
    from lemon_amd import ops
    got = ops.local_search(_cuda(rec), y, list(starts), fx.METHODS, force_zero, force_one, ks=[k], return_info=True)[0]
    objective = _host_objective(_cuda(_prefix(rec, k)), y, force_zero, force_one)
    assert len(got) == len(starts) * len(fx.METHODS)
    s = 0
    for start in starts:
        for method in fx.METHODS:
            fx.assert_same(got[s], fx.scipy_search(objective, list(start), method), f"{what} k={k} x0={start[0]} {method}")
            s += 1


@pytest.fixture()
def knobs(hip):
    from lemon_amd import _lib
    lib = _lib.load()
    yield lib.lemon_hparam_search_set_test_knobs
    lib.lemon_hparam_search_set_test_knobs(0, 0, 0, 0, 0)


@pytest.mark.parametrize("n", [1, 64, 65, 1031])
def test_the_objective_the_kernel_sees_is_grid_f1s(hip, knobs, n):
    """A Powell search capped at one evaluation returns (x0, objective(x0)): for 32 random x, plain and under every ablation's
    masks, that value is -F1 of lemon_grid_f1 at the masked x, in LDS and in the workspace form, at full depth and on a prefix."""
    from lemon_amd import metrics as M, ops
    rec, y = fx.record(n, kmax=7, seed=3)
    rng = np.random.default_rng(n)
    xs = rng.uniform(0.0, 12.0, (32, 6))
    xs[3] = 0.0
    xs[4, 2:] = -9000.0                                   # overflows: the objective is 0.0, lemon_grid_f1 reports F1 = 0
    knobs(0, 0, 0, 0, 1)
    for k in (7, 3):
        dev_k = _cuda(_prefix(rec, k))
        for name, (fz, fo) in fx.ABLATIONS.items():
            want = -ops.grid_f1(dev_k, y, [[M.unpack_vector(x, fz, fo)[nm] for nm in M.HP_NAMES] for x in xs])[0]
            for force_ws in (0, 1):
                knobs(force_ws, 0, 0, 0, 1)
                got = ops.local_search(_cuda(rec), y, xs, ("Powell",), fz, fo, ks=[k], return_info=True)[0]
                assert [g[2:] for g in got] == [(1, 0, 1)] * 32                        # one evaluation, maxfev reached
                assert np.array_equal(np.array([g[0] for g in got]).view(np.int64), xs.view(np.int64))
                assert np.array_equal(np.array([g[1] for g in got]), want), (name, k, force_ws)
    assert want[4] == 0.0


@pytest.mark.parametrize("n,k", [(65, 5), (65, 50), (257, 5), (257, 50), (1031, 5), (1031, 50)])
def test_all_eight_searches_equal_scipy_on_the_host_objective(hip, n, k):
    rec, y = fx.record(n, kmax=k)
    _against_scipy(rec, y, k, what=f"n={n}")


def test_prefix_of_a_deeper_record(hip):
    rec, y = fx.record(257, kmax=fx.KMAX)
    _against_scipy(rec, y, 5, what="prefix of kmax=51")


@pytest.mark.parametrize("labels", ["zeros", "ones"])
def test_flat_labels(hip, labels):
    rec, y = fx.record(65, kmax=5, labels=labels)
    _against_scipy(rec, y, 5, what=labels)


def test_overflowing_start(hip):
    rec, y = fx.overflow_record(65, kmax=50)
    objective = _host_objective(_cuda(rec), y)
    assert objective(np.full(6, 800.0)) == 0.0 and objective(np.full(6, 0.5)) < 0.0
    _against_scipy(rec, y, 50, starts=([800] * 6,), what="overflow")


def test_ablation_masks(hip):
    rec, y = fx.record(65, kmax=5)
    fz, fo = fx.ABLATIONS["tau_1_2"]
    _against_scipy(rec, y, 5, starts=([0.5] * 6,), force_zero=fz, what="tau_1_2")
    rec["d_1"] = np.zeros_like(rec["d_1"])
    _against_scipy(rec, y, 5, starts=([1] * 6,), force_one=fx.ABLATIONS["d1"][1], what="d1")


def test_workspace_form_returns_the_bits_of_the_lds_form(hip, knobs):
    from lemon_amd import ops
    rec, y = fx.record(1031, kmax=50)
    dev = _cuda(rec)
    lds = ops.local_search(dev, y, list(fx.STARTS), ks=[5, 50], return_info=True)
    knobs(1, 0, 0, 0, 0)
    ws = ops.local_search(dev, y, list(fx.STARTS), ks=[5, 50], return_info=True)
    for a, b in zip(sum(lds, []), sum(ws, [])):
        fx.assert_same(b, a, "workspace form against LDS form")
        assert np.signbit(a[1]) == np.signbit(b[1])


def test_sixty_four_searches_in_one_call_equal_the_single_calls(hip):
    from lemon_amd import ops
    ks = [1, 2, 5, 10, 15, 20, 30, 50]
    rec, y = fx.record(257, kmax=50)
    dev = _cuda(rec)
    together = ops.local_search(dev, y, list(fx.STARTS), ks=ks, return_info=True)
    assert len(together) == 8 and all(len(t) == 8 for t in together)
    for t, k in enumerate(ks):
        s = 0
        for start in fx.STARTS:
            for method in fx.METHODS:
                one = ops.local_search(dev, y, [list(start)], (method,), ks=[k], return_info=True)[0][0]
                fx.assert_same(together[t][s], one, f"k={k} x0={start[0]} {method}")
                s += 1
    assert ops.local_search(dev, y, list(fx.STARTS))[3][1] == together[-1][3][1]         # ks=None: the record's own depth
    with pytest.raises(ValueError):
        ops.local_search(dev, y, list(fx.STARTS), ks=[51])
    with pytest.raises(ValueError):
        ops.local_search(dev, y, list(fx.STARTS), methods=("BFGS",))


def test_maximize_metric_with_and_without_local_search(hip):
    from lemon_amd import metrics as M, ops
    rec, y = fx.record(257, kmax=5)
    dev = _cuda(rec)
    grid = {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}
    score_fn = lambda hp: ops.lemon_score(dev, hp).cpu().numpy()
    batch = lambda hps: ops.grid_f1(dev, y, [[hp[nm] for nm in M.HP_NAMES] for hp in hps])[0]
    for fz, fo in (((), ()), fx.ABLATIONS["tau_2"]):
        host = M.maximize_metric(score_fn, y, grid, [list(s) for s in fx.STARTS], force_zero=fz, force_one=fo, batch_grid=batch)
        device = M.maximize_metric(score_fn, y, grid, [list(s) for s in fx.STARTS], force_zero=fz, force_one=fo, batch_grid=batch,
                                   local_search=lambda x0s, methods, z, o: ops.local_search(dev, y, x0s, methods, z, o))
        assert np.array_equal(np.asarray(host[0], np.float64).view(np.int64), np.asarray(device[0], np.float64).view(np.int64))
        assert host[1] == device[1] and host[2] == device[2]


# ------------------------------------------------------------------------------------------------------------- run_lemon
BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:1500", "--clip_path", "random:tiny",
        "--hparam_grid", "small", "--debug"]


def _same(a, b, path="agg_results"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for key in a:
            _same(a[key], b[key], f"{path}.{key}")
    elif isinstance(a, (list, tuple, np.ndarray)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path
    elif isinstance(a, (float, np.floating)):
        assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (path, a, b)
    else:
        assert a == b, (path, a, b)


def _equal_runs(a, b):
    _same(pickle.load(open(os.path.join(a, "res.pkl"), "rb"))["agg_results"],
          pickle.load(open(os.path.join(b, "res.pkl"), "rb"))["agg_results"])
    csv = "know_val_labels_scores.csv"
    assert open(os.path.join(a, csv), "rb").read() == open(os.path.join(b, csv), "rb").read()


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hparam_search_cache"))


def test_cli_device_search_equals_host_search(hip, tmp_path, cache_dir):
    from lemon_amd.run_lemon import main
    outs = {}
    for where in ("host", "device"):
        outs[where] = str(tmp_path / where)
        assert main(["--output_dir", outs[where], *BASE, "--embedding_cache", cache_dir, "--knn_k", "5",
                     "--hparam_search", where]) == 0
    _equal_runs(outs["device"], outs["host"])
    assert json.load(open(os.path.join(outs["device"], "args.json")))["hparam_search"] == "device"


def test_cli_device_search_equals_host_search_under_the_sweep(hip, tmp_path, cache_dir):
    from lemon_amd.run_lemon import main
    outs = {}
    for where in ("host", "device"):
        outs[where] = str(tmp_path / where)
        assert main(["--output_dir", outs[where], *BASE, "--embedding_cache", cache_dir, "--knn_k_sweep", "1,5,10",
                     "--hparam_search", where]) == 0
    for k in (1, 5, 10):
        _equal_runs(os.path.join(outs["device"], f"knn_k={k}"), os.path.join(outs["host"], f"knn_k={k}"))
    sel = [json.load(open(os.path.join(outs[w], "k_selection.json"))) for w in ("device", "host")]
    assert sel[0] == sel[1] and sel[0]["best_k"] in (1, 5, 10)
