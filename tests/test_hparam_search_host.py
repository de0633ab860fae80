"""The local searches of the hyper-parameter search on the host twin (no GPU): lemon_hparam_search_host against
scipy.optimize.minimize(options={}) driving lemon_hparam_objective_host on the same record.  Comparison rules
(tests/hparamfx.py): x bit for bit, fun ==, nfev / nit / status equal; no tolerances.

Nelder-Mead orders tied simplex vertices as np.argsort does.  On x86-64 with AVX-512 numpy runs an 8-lane network there (not a
stable sort); csrc/hparam_search_core.hpp restates that network, test_simplex_sort_is_numpys pins the assumption."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import hparamfx as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 63, 65, 257)
KS = (1, 5, 50)


@pytest.fixture(scope="module")
def records():
    return {n: fx.HostRecord(*fx.record(n)) for n in NS}


def _compare(hr, ks, force_zero=(), force_one=(), starts=fx.STARTS, options=None, what=""):
    x0, spec, labels = fx.searches(ks, force_zero, force_one, starts=starts)
    got = hr.search(x0, spec)
    nfev = []
    for s, (k, start, method) in enumerate(labels):
        want = fx.scipy_search(hr.objective(k, force_zero, force_one), list(start), method, options)
        fx.assert_same(got[s], want, f"{what} n={hr.n} k={k} x0={start[0]} {method}")
        nfev.append(want[2])
    return got, nfev


@pytest.mark.parametrize("n", NS)
def test_the_eight_searches_match_scipy(records, n):
    _, nfev = _compare(records[n], KS)
    assert len(nfev) == 8 * len(KS)


@pytest.mark.parametrize("ablation", ["tau_1", "tau_2", "tau_1_2", "beta", "gamma", "d1"])
def test_ablation_masks_match_scipy(records, ablation):
    """the masks of run_lemon._grid_setup: the optimiser moves the forced coordinates, the objective ignores them"""
    import argparse
    from lemon_amd import run_lemon
    _, fz, fo = run_lemon._grid_setup(argparse.Namespace(real_dataset=False, skip_hparam_optim=False, ablation=ablation,
                                                         hparam_grid="small"))
    assert (tuple(fz), tuple(fo)) == fx.ABLATIONS[ablation]
    rec, y = fx.record(65)
    if ablation == "d1":
        rec["d_1"] = np.zeros_like(rec["d_1"])           # run_lemon._tail: df["d_1"] = 0.0
    _compare(fx.HostRecord(rec, y), (5,), fz, fo, what=ablation)


def test_forced_coordinates_do_not_reach_the_objective(records):
    hr = records[65]
    f = hr.objective(5, ("tau_1_n", "beta"), ("gamma", "beta"))
    g = hr.objective(5)
    x = np.array([3.0, 0.25, 7.0, 0.5, 0.125, 2.0])
    assert f(x) == g(np.array([1.0, 1.0, 0.0, 0.5, 0.125, 2.0]))          # zeros first, then ones: beta ends at 1
    assert f(x) == f(np.array([-9.0, 1e300, np.nan, 0.5, 0.125, 2.0]))


@pytest.mark.parametrize("labels", ["zeros", "ones"])
def test_flat_labels_go_through_the_bracket_recovery(labels):
    """y all zero / all one: F1 does not separate anything, line searches end in BracketError and its recovery, Nelder-Mead
    runs on ties.  Not vacuous: scipy's own run is counted through a wrapped bracket()."""
    import scipy.optimize._optimize as so
    hr = fx.HostRecord(*fx.record(65, labels=labels))
    raised = [0]
    real = so.bracket

    def counting(*a, **kw):
        try:
            return real(*a, **kw)
        except so.BracketError:
            raised[0] += 1
            raise

    so.bracket = counting
    try:
        _, nfev = _compare(hr, (5, 50), what=labels)
    finally:
        so.bracket = real
    assert raised[0] >= 8, f"scipy met BracketError {raised[0]} times: the flat case did not exercise the recovery"
    if labels == "zeros":                                # every Powell line search: three bracket points, all equal
        assert [v for v in nfev[0::2]] == [1 + 6 * 3] * 8


def test_overflowing_start_matches_scipy():
    rec, y = fx.overflow_record(65)
    hr = fx.HostRecord(rec, y)
    f = hr.objective(50)
    v = f(np.full(6, 800.0))
    assert v == 0.0 and not np.signbit(v), "scores overflow at x0 = [800] * 6: the objective is +0.0 there"
    assert f(np.full(6, 0.5)) < 0.0
    _compare(hr, (5, 50), starts=([800] * 6,), what="overflow")


def test_simplex_sort_is_numpys(records):
    """Ties between simplex vertices: on flat labels every vertex of every simplex ties, so Nelder-Mead's trajectory is decided
    by np.argsort's order of equal values alone -- scipy, with the numpy of this machine, is the judge."""
    hr = fx.HostRecord(*fx.record(63, labels="zeros"))
    x0, spec, labels = fx.searches((1, 5), methods=("Nelder-Mead",))
    got = hr.search(x0, spec)
    for s, (k, start, method) in enumerate(labels):
        fx.assert_same(got[s], fx.scipy_search(hr.objective(k), list(start), method), f"ties k={k} x0={start[0]}")


@pytest.mark.parametrize("caps", [dict(nm=(1200, 40), pw=(6000, 100)), dict(nm=(9, 1200), pw=(1, 6000)),
                                  dict(nm=(30, 61), pw=(2, 157))])
def test_caps_report_scipys_status_and_nfev(records, caps):
    """None of the fixture searches reaches scipy's default caps (1200 / 6000), so the caps of the core header are lowered
    through the test knob and scipy is given the same maxiter / maxfev.  (maxiter, maxfev) per method; at least seven
    evaluations, so that the first simplex is complete."""
    from lemon_amd import _lib
    lib = _lib.load()
    hr = records[65]
    (nm_it, nm_fev), (pw_it, pw_fev) = caps["nm"], caps["pw"]
    lib.lemon_hparam_search_set_test_knobs(0, nm_it, nm_fev, pw_it, pw_fev)
    try:
        statuses = set()
        for method, opts in (("Nelder-Mead", dict(maxiter=nm_it, maxfev=nm_fev)), ("Powell", dict(maxiter=pw_it, maxfev=pw_fev))):
            x0, spec, labels = fx.searches((5,), methods=(method,))
            got = hr.search(x0, spec)
            for s, (k, start, m) in enumerate(labels):
                want = fx.scipy_search(hr.objective(k), list(start), m, opts)
                fx.assert_same(got[s], want, f"caps {opts} x0={start[0]} {m}")
                statuses.add(want[4])
        assert statuses & {1, 2}, f"no search reached a cap ({statuses}): the case is vacuous"
    finally:
        lib.lemon_hparam_search_set_test_knobs(0, 0, 0, 0, 0)
    assert hr.search(*fx.searches((5,))[:2])[0][2] > 157   # the defaults are back (Powell from x0 = 0)


def test_surface_declared_bound_exported():
    from lemon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("lemon_hparam_search_workspace_bytes", "lemon_hparam_search", "lemon_hparam_search_host",
                 "lemon_hparam_objective_host"):
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "LEMON_SEARCH_NELDER_MEAD 0" in hdr and "LEMON_SEARCH_POWELL 1" in hdr
    assert ctypes.sizeof(_lib.SearchResult) == 72
    assert "hparam_search.hip" in __import__("lemon_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.load().lemon_hparam_search_workspace_bytes(1031, 64) >= 1031 * 64 * 8


def test_bad_arguments_are_refused_with_a_message(records):
    from lemon_amd import _lib
    lib = _lib.load()
    hr = records[63]
    good_x0, good_spec, _ = fx.searches((5,))

    def refused(spec=good_spec, x0=good_x0, n=hr.n, null=None, ws_bytes=None):
        arrs = [ctypes.c_void_p(a.ctypes.data) for a in hr.arrs] + [ctypes.c_void_p(hr.y.ctypes.data)]
        if null is not None:
            arrs[null] = None
        spec = np.ascontiguousarray(spec, np.int32)
        S = spec.shape[0]
        out = (_lib.SearchResult * S)()
        ws = np.empty(S * hr.n, np.float64)
        rc = lib.lemon_hparam_search_host(*arrs, n, hr.kmax, S, ctypes.c_void_p(x0.ctypes.data), ctypes.c_void_p(spec.ctypes.data),
                                          ctypes.c_void_p(ws.ctypes.data), ws.nbytes if ws_bytes is None else ws_bytes,
                                          ctypes.byref(out))
        return rc, lib.lemon_last_error().decode()

    assert refused()[0] == 0
    for kw, word in ((dict(null=0), "null"), (dict(null=7), "null"), (dict(n=0), "n > 0"), (dict(ws_bytes=8), "workspace")):
        rc, msg = refused(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for col, val, word in ((0, 2, "method"), (0, -1, "method"), (1, 0, "k"), (1, hr.kmax + 1, "k"), (2, 64, "mask"), (3, -1, "mask")):
        spec = good_spec.copy()
        spec[3, col] = val
        rc, msg = refused(spec=spec)
        assert rc == -1 and word in msg, (col, val, rc, msg)
    assert lib.lemon_hparam_search_workspace_bytes(0, 8) < 0 and "n > 0" in lib.lemon_last_error().decode()
    assert lib.lemon_hparam_search_workspace_bytes(10, -1) < 0
    # the device entry refuses the same before it touches the device: n <= 0 and null pointers need no GPU
    rc = lib.lemon_hparam_search(*[None] * 8, 0, 5, 1, None, None, None, 0, None, None)
    assert rc == -1 and "n > 0" in lib.lemon_last_error().decode()
    assert np.isnan(hr.objective(hr.kmax + 1)(np.zeros(6))) and "k <= kmax" in lib.lemon_last_error().decode()


def test_flag_defaults_to_host_and_changes_nothing_else():
    from lemon_amd.run_lemon import build_parser
    args = vars(build_parser().parse_args(["--output_dir", "x"]))
    assert args["hparam_search"] == "host"
    dev = vars(build_parser().parse_args(["--output_dir", "x", "--hparam_search", "device"]))
    assert dev["hparam_search"] == "device"
    assert {k: v for k, v in dev.items() if k != "hparam_search"} == {k: v for k, v in args.items() if k != "hparam_search"}
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--output_dir", "x", "--hparam_search", "gpu"])


def test_maximize_metric_consumes_local_search_in_order_under_strict_greater(records):
    """the stub's results replace the scipy loop: first of equal values wins (strict >), order = for each x0, each method"""
    from lemon_amd import metrics as M
    rec, y = fx.record(65)
    score = lambda hp: (rec["d_1"].astype(np.float64) + hp["beta"] * rec["dists_n"][:, :5].mean(1)
                        + hp["gamma"] * rec["dists_m"][:, :5].mean(1))
    grid = {"beta": [0.0], "gamma": [0.0], "tau_1": [0.0], "tau_2": [0.0]}
    asked = []

    def stub(vals):
        def f(x0s, methods, force_zero, force_one):
            asked.append(([list(x) for x in x0s], tuple(methods), tuple(force_zero), tuple(force_one)))
            return [(np.full(6, float(i)), v) for i, v in enumerate(vals)]
        return f

    x0s = [[0] * 6, [1] * 6]
    # -fun: 2.0, 3.0, 3.0, 1.0 -> the first 3.0 (index 1) wins and beats the grid (F1 <= 1)
    best, val, _ = M.maximize_metric(score, y, grid, x0s, local_search=stub([-2.0, -3.0, -3.0, -1.0]), force_zero=("gamma",))
    assert val == 3.0 and best == [1.0, 0.0, 1.0, 1.0, 1.0, 1.0]         # gamma forced to zero in the returned vector
    assert asked == [([[0] * 6, [1] * 6], ("Powell", "Nelder-Mead"), ("gamma",), ())]
    # nothing beats the grid's value: the grid point is returned
    best, val, _ = M.maximize_metric(score, y, grid, x0s, local_search=stub([0.0, 0.0, 0.0, 0.0]))
    assert best == [0.0] * 6 and 0.0 < val <= 1.0
    with pytest.raises(AssertionError):
        M.maximize_metric(score, y, grid, x0s, local_search=stub([-1.0]))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_core_header_alone_under_asan_and_ubsan(tmp_path):
    """csrc/hparam_search_core.hpp driven by a stand-alone program on a quadratic, plateaus and NaN-returning objectives"""
    exe = str(tmp_path / "hparam_search_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "hparam_search_fuzz.cpp"), "-o", exe])
    for seed in ("1", "20261019"):
        r = subprocess.run([exe, "1500", seed], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "hparam_search_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
