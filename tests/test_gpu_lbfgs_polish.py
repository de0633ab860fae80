"""GPU: the LBFGS polish of the hyper-parameter search in one launch (lemon_lbfgs_polish, ops.lbfgs_polish) against its host
twin (lemon_lbfgs_polish_host: the same header with the threads looped on the host, tests/test_lbfgs_polish_host.py pins it to
torch).  Comparison rule: x bit for bit (float64 viewed as int64, NaN payloads included), loss bit for bit, nfev / nit / status
equal, after all 20 outer steps; no tolerances.

Shapes: with T = 256 threads a workgroup, n = 1 (one thread), 63 (less than a wave), T - 1, T, T + 1 (a thread with two rows)
and 2 T + 7 (every thread with two or three rows and a tail); k = 1, 5, 17, 50 as prefixes of a kmax = 51 record and 51, its
full depth: the smallest shapes that hit every edge of the row partition, the butterfly and the prefix depth."""
import json
import os
import pickle

import numpy as np
import pytest

from tests import hparamfx as fx
from tests import lbfgsfx as lx

pytestmark = pytest.mark.gpu

T = lx.THREADS
NS = [1, 63, T - 1, T, T + 1, 2 * T + 7]
KS = [1, 5, 17, 50, 51]
ABLATION_START = [0.5] * 6


def _cuda(rec):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in rec.items()}


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.int64)


def _assert_same(got, want, what):
    """got: (x, status, loss, nfev, nit) of ops.lbfgs_polish(return_info=True); want: (x, loss, nfev, nit, status) of the twin"""
    gx, gstatus, gloss, gnfev, gnit = got
    wx, wloss, wnfev, wnit, wstatus = want
    assert (gnfev, gnit, gstatus) == (wnfev, wnit, wstatus), f"{what}: (nfev, nit, status) {(gnfev, gnit, gstatus)} != the twin's {(wnfev, wnit, wstatus)}"
    assert np.array_equal(_bits(gx), _bits(wx)), f"{what}: x {gx!r} != the twin's {wx!r}"
    assert _bits([gloss])[0] == _bits([wloss])[0], f"{what}: loss {gloss!r} != the twin's {wloss!r}"


def _device_against_twin(rec, y, ks, starts, force_zero=(), force_one=(), what=""):
    from lemon_amd import ops
    got = ops.lbfgs_polish(_cuda(rec), y, [list(s) for s in starts], force_zero, force_one, ks=ks, return_info=True)
    want = lx.HostPolish(rec, y).polish_parallel(*lx.polishes(ks, force_zero, force_one, starts=starts))
    assert len(got) == len(ks) and all(len(g) == len(starts) for g in got)
    for t, k in enumerate(ks):
        for s, start in enumerate(starts):
            _assert_same(got[t][s], want[t * len(starts) + s], f"{what} k={k} x0={start[0]}")
    return got


@pytest.mark.parametrize("n", NS)
def test_device_equals_host_twin_bit_for_bit(hip, n):
    rec, y = fx.record(n, kmax=fx.KMAX)
    got = _device_against_twin(rec, y, KS, fx.STARTS, what=f"n={n}")
    assert any(g[1] == 0 for per_k in got for g in per_k)                         # finite results are among them
    for name in ("none", "tau_1", "beta", "d1"):
        fz, fo = fx.ABLATIONS[name]
        rec_a = dict(rec, d_1=np.zeros_like(rec["d_1"])) if name == "d1" else rec   # run_lemon._tail: df["d_1"] = 0.0
        got = _device_against_twin(rec_a, y, KS, (ABLATION_START,), fz, fo, what=f"n={n} {name}")
        for per_k in got:
            for nm in fz + fo:                                                     # a forced coordinate never moves
                assert per_k[0][1] == 1 or per_k[0][0][fx.HP_NAMES.index(nm)] == 0.5


@pytest.mark.parametrize("labels", ["zeros", "ones"])
def test_flat_labels(hip, labels):
    rec, y = fx.record(T + 1, kmax=fx.KMAX, labels=labels)
    _device_against_twin(rec, y, [5, 51], fx.STARTS, what=labels)


def test_overflowing_start(hip):
    rec, y = fx.overflow_record(T + 1, kmax=fx.KMAX)
    got = _device_against_twin(rec, y, [50], ([800] * 6, [0.5] * 6), what="overflow")
    assert got[0][0][1] == 1 and got[0][1][1] == 0                                 # status 1 on both sides; a tame start is fine


def test_twelve_polishes_in_one_call_equal_the_single_calls(hip):
    from lemon_amd import ops
    ks = [1, 5, 50]
    rec, y = fx.record(T + 1, kmax=fx.KMAX)
    dev = _cuda(rec)
    starts = [list(s) for s in fx.STARTS]
    together = ops.lbfgs_polish(dev, y, starts, ks=ks, return_info=True)
    assert len(together) == 3 and all(len(t) == 4 for t in together)
    for t, k in enumerate(ks):
        for s, start in enumerate(starts):
            one = ops.lbfgs_polish(dev, y, [start], ks=[k], return_info=True)[0][0]
            assert np.array_equal(_bits(together[t][s][0]), _bits(one[0])) and _bits([together[t][s][2]]) == _bits([one[2]]), (k, start[0])
            assert together[t][s][1] == one[1] and together[t][s][3:] == one[3:], (k, start[0])
    # ks=None: the record's own depth; the plain form is (x, status)
    deep = ops.lbfgs_polish(dev, y, starts)
    want = ops.lbfgs_polish(dev, y, starts, ks=[fx.KMAX], return_info=True)[0]
    assert len(deep) == 4 and all(len(d) == 2 for d in deep)
    for d, w in zip(deep, want):
        assert np.array_equal(_bits(d[0]), _bits(w[0])) and d[1] == w[1]
    assert ops.lbfgs_polish(dev, y, []) == [] and ops.lbfgs_polish(dev, y, [], ks=[1, 5]) == [[], []]
    with pytest.raises(ValueError):
        ops.lbfgs_polish(dev, y, starts, ks=[52])
    with pytest.raises(ValueError):
        ops.lbfgs_polish(dev, y, starts, ks=[0])
    with pytest.raises(ValueError):
        ops.lbfgs_polish(dev, y, starts, force_zero=("tau_3",))


def test_device_entry_refuses_a_bad_spec_before_launching(hip):
    import torch
    from lemon_amd import _lib, ops
    rec, y = fx.record(63, kmax=fx.KMAX)
    dev = _cuda(rec)
    arrs = [ops.ptr(dev[key]) for key in fx.REC_KEYS]
    yb = torch.from_numpy(y).cuda()
    x0, spec = lx.polishes((5,))
    x0_d = torch.from_numpy(x0).cuda()
    lib = _lib.load()
    for col, val, word in ((0, 52, "k"), (0, 0, "k"), (1, 64, "mask"), (2, 128, "mask")):
        bad = spec.copy()
        bad[2, col] = val
        out = torch.full((4 * 72,), 0x5a, dtype=torch.uint8, device="cuda")
        rc = lib.lemon_lbfgs_polish(*arrs, ops.ptr(yb), 63, fx.KMAX, 4, ops.ptr(x0_d), ops.ptr(torch.from_numpy(bad).cuda()), 20,
                                    ops.ptr(out), ops.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and word in lib.lemon_last_error().decode(), (col, val, rc)
        assert bool((out == 0x5a).all()), "a refused call writes nothing"


def test_maximize_metric_with_the_device_polish(hip):
    """the polish only competes: with its candidates the best value is at least the value without them; and it is repeatable"""
    from lemon_amd import metrics as M, ops
    rec, y = fx.record(T + 1, kmax=5)
    dev = _cuda(rec)
    grid = {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}
    score_fn = lambda hp: ops.lemon_score(dev, hp).cpu().numpy()
    batch = lambda hps: ops.grid_f1(dev, y, [[hp[nm] for nm in M.HP_NAMES] for hp in hps])[0]
    starts = [list(s) for s in fx.STARTS]
    for fz, fo in (((), ()), fx.ABLATIONS["tau_2"]):
        polish = lambda x0s, z, o: [x for x, _ in ops.lbfgs_polish(dev, y, x0s, z, o)]
        kw = dict(force_zero=fz, force_one=fo, batch_grid=batch, scipy_methods=())
        a = M.maximize_metric(score_fn, y, grid, starts, lbfgs_polish=polish, **kw)
        b = M.maximize_metric(score_fn, y, grid, starts, lbfgs_polish=polish, **kw)
        none = M.maximize_metric(score_fn, y, grid, starts, lbfgs_polish=lambda x0s, z, o: [[np.nan] * 6] * len(x0s), **kw)
        assert a[1] >= none[1]
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1:] == b[1:]


# ------------------------------------------------------------------------------------------------------------- run_lemon
BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:1500", "--clip_path", "random:tiny",
        "--hparam_grid", "small", "--debug", "--hparam_search", "device", "--lbfgs_polish", "device"]
FILES = ("res.pkl", "know_val_labels_scores.csv", "args.json", "done")


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("lbfgs_polish_cache"))


def _selected(out):
    sel = pickle.load(open(os.path.join(out, "res.pkl"), "rb"))["agg_results"]["know_val_labels"]
    return [np.float64(sel[nm]) for nm in fx.HP_NAMES], float(sel["selected_val"]), float(sel["thres"])


def _three_runs(tmp_path, cache_dir, monkeypatch, extra):
    """the run, the run again, and the run with the polish candidates removed (every polish reported as diverged)"""
    from lemon_amd import ops
    from lemon_amd.run_lemon import main
    outs = {}
    for name in ("first", "second"):
        outs[name] = str(tmp_path / name)
        assert main(["--output_dir", outs[name], *BASE, "--embedding_cache", cache_dir, *extra]) == 0
    real, calls = ops.lbfgs_polish, []

    def removed(*args, **kw):
        res = real(*args, **kw)
        calls.append(kw.get("ks"))
        blank = lambda rows: [(np.full(6, np.nan),) + tuple(r[1:]) for r in rows]
        return blank(res) if kw.get("ks") is None else [blank(rows) for rows in res]

    monkeypatch.setattr(ops, "lbfgs_polish", removed)
    outs["removed"] = str(tmp_path / "removed")
    assert main(["--output_dir", outs["removed"], *BASE, "--embedding_cache", cache_dir, *extra]) == 0
    return outs, calls


def test_cli_device_polish(hip, tmp_path, cache_dir, monkeypatch):
    outs, calls = _three_runs(tmp_path, cache_dir, monkeypatch, ["--knn_k", "5"])
    assert calls == [None]                                                         # one launch served the run
    for f in FILES:
        assert os.path.exists(os.path.join(outs["first"], f)), f
    assert json.load(open(os.path.join(outs["first"], "args.json")))["lbfgs_polish"] == "device"
    first, second, removed = (_selected(outs[name]) for name in ("first", "second", "removed"))
    assert first[1] >= removed[1]
    assert np.array_equal(_bits(first[0]), _bits(second[0])) and first[1:] == second[1:]


def test_cli_device_polish_under_the_sweep(hip, tmp_path, cache_dir, monkeypatch):
    outs, calls = _three_runs(tmp_path, cache_dir, monkeypatch, ["--knn_k_sweep", "1,5"])
    assert calls == [[1, 5]]                                                       # all ks' polishes from one call on the deep record
    assert os.path.exists(os.path.join(outs["first"], "k_selection.json"))
    for k in (1, 5):
        sub = {name: os.path.join(out, f"knn_k={k}") for name, out in outs.items()}
        for f in FILES:
            assert os.path.exists(os.path.join(sub["first"], f)), (k, f)
        assert json.load(open(os.path.join(sub["first"], "args.json")))["lbfgs_polish"] == "device"
        first, second, removed = (_selected(sub[name]) for name in ("first", "second", "removed"))
        assert first[1] >= removed[1], k
        assert np.array_equal(_bits(first[0]), _bits(second[0])) and first[1:] == second[1:], k
