"""CPU: the host twin of lemon_eval_metrics (csrc/eval_metrics_core.hpp with the lanes looped) against lemon_amd.metrics, scipy
and sklearn as installed.  Thresholds of the optimize_f1, bisect and fminbound paths, all counts and every count-derived float:
by their bits and Python types.  AUROC / AUPRC: within n 2^-52 of sklearn -- at most n + 1 terms, each rounded a few times at
relative 2^-53, the result at most 1; one mis-ordered pair costs 1 / (2 P N) > 1e-9 at these sizes.  The KDE threshold: by its
bits on inputs whose scipy density separates every pair of neighbouring grid points by more than 1e-9 relative (checked here
with scipy), the twin's density within 1e-12 relative of scipy's.  Every branch on an input of its own, scipy's branch
asserted first."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lemon_amd import metrics as M
from tests import evalfx as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 5, 17, 63, 64, 65, 257, 600, 1000, 5000)


def _auc_bound(n):
    return n * 2.0 ** -52


def _run_pattern(score, y, prevalence, cuts):
    """the val -> splits pattern of a run: the free rows [0, cuts[0]), then a fixed segment per cut interval (the first is a
    second copy of the free rows: segments do not overlap) -> (twin dicts, host dicts)"""
    bounds = [0] + list(cuts)
    n0 = cuts[0]
    segments = [(0, n0, prevalence, -1)] + [(n0 + lo, hi - lo, prevalence, 0) for lo, hi in zip(bounds[:-1], bounds[1:])]
    got = fx.host_dicts(np.concatenate([score[:n0], score]), np.concatenate([y[:n0], y]), segments)
    free = M.eval_metrics(y[:cuts[0]], score[:cuts[0]], prevalence)
    want = [free] + [M.eval_metrics(y[lo:hi], score[lo:hi], prevalence, fix_thress=free) for lo, hi in zip(bounds[:-1], bounds[1:])]
    return got, want


@pytest.fixture(scope="module")
def sweep():
    """(name, n of the free segment, twin dicts, host dicts, KDE separated) of every case of the sweep, computed once"""
    cases = []
    for n in SIZES:
        for tied in (False, True):
            score, y = fx.mixture(n + 40, 100 + n, p_pos=0.25)
            if tied:
                score = np.round(score, 2 if n > 17 else 0)
            y[:2] = [True, False]
            y[n:n + 2] = [True, False]
            prevalence = y[:n].sum() / n
            got, want = _run_pattern(score, y, prevalence, [n, n + 40])
            separated = len(np.unique(score[:n])) > 1 and fx.kde_separated(score[:n])[0]
            cases.append((f"n={n}{'-tied' if tied else ''}", n, got, want, separated))
    return cases


def test_thresholds_counts_and_derived_values_equal_the_host_path_by_bits(sweep):
    compared_heuristic = 0
    for name, n, got, want, separated in sweep:
        skip = () if separated else fx.heuristic_keys()
        compared_heuristic += bool(separated)
        for g, w in zip(got, want):
            fx.same_dict(g, w, skip=skip, auc_bound=_auc_bound(n + 40))
    print(f"heuristic threshold compared by bits on {compared_heuristic} of {len(sweep)} cases")
    assert compared_heuristic >= len(sweep) // 2


def test_auroc_and_auprc_within_n_ulp_of_sklearn(sweep):
    worst = 0.0
    for name, n, got, want, _ in sweep:
        for g, w, rows in zip(got, want, (n, n, 40)):
            for key in ("AUROC", "AUPRC"):
                ratio = abs(g[key] - w[key]) / _auc_bound(rows)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, key, g[key], w[key])
    print(f"worst |twin - sklearn| / (n 2^-52) over the sweep: {worst:.4f}")


@pytest.mark.parametrize("n,seed", [(50, 1), (257, 2), (600, 3)])
def test_kde_threshold_equals_scipy_on_separated_mixtures(n, seed):
    score, y = fx.mixture(n, seed)
    holds, gap = fx.kde_separated(score)
    assert holds, f"the input does not separate scipy's own density: smallest neighbour gap {gap:.3g}"
    xs, dens, _, _ = fx.scipy_kde(score)
    grid, twin = fx.twin_kde(score)
    assert np.array_equal(fx.bits(grid), fx.bits(xs))
    rel = float(np.max(np.abs(twin - dens) / dens))
    print(f"n={n}: twin density within {rel:.3g} relative of scipy's; the input's neighbour gap is {gap:.3g}")
    assert rel <= 1e-12
    want = M.f1_with_local_minima_finder(y, score, True)[1]
    rc, (rec,) = fx.host_records(score, y, [(0, n, y.mean(), -1)])
    assert rc == 0 and rec.status == 0 and rec.kde_branch == fx.scipy_branch(score)
    assert fx.bits(rec.thres[2]) == fx.bits(want)


def _branch_case(score, y, branch):
    assert fx.scipy_branch(score) == branch, f"scipy takes branch {fx.scipy_branch(score)} on this input, not {branch}"
    holds, gap = fx.kde_separated(score) if branch != 3 else (True, None)      # branch 3 lives on an underflowed plateau
    assert holds, gap
    want = M.f1_with_local_minima_finder(y, score, True)[1]
    rc, (rec,) = fx.host_records(score, y, [(0, len(score), 0.3, -1)])
    assert rc == 0 and rec.status == 0
    assert rec.kde_branch == branch and fx.bits(rec.thres[2]) == fx.bits(want), (rec.kde_branch, rec.thres[2], want)
    return rec


def test_kde_branch_median_of_an_odd_and_an_even_count_of_minima():
    score, y = fx.mixture(900, 5, centres=(0.0, 6.0, 12.0, 18.0), sd=0.8)
    _, _, minima, _ = fx.scipy_kde(score)
    assert len(minima) == 3
    _branch_case(score, y, 1)
    score, y = fx.mixture(900, 6, centres=(0.0, 6.0, 12.0), sd=0.8)
    _, _, minima, _ = fx.scipy_kde(score)
    assert len(minima) == 2
    _branch_case(score, y, 1)


def test_kde_branch_exactly_one_minimum():
    score, y = fx.mixture(400, 7, centres=(0.0, 6.0), sd=0.8)
    _branch_case(score, y, 2)


def test_kde_branch_no_minimum_and_two_maxima():
    # a tight cluster, one row far below it and the grid's two ends: between the two interior maxima the density underflows
    # to exact zeros, so no grid point is strictly below both neighbours
    rng = np.random.default_rng(8)
    n = 4000
    score = 0.01 * rng.standard_normal(n)
    score[:3] = [-1000.0, -500.0, 1000.0]
    y = rng.random(n) < 0.3
    _, dens, minima, maxima = fx.scipy_kde(score)
    assert len(minima) == 0 and len(maxima) == 2 and (dens == 0).any()
    _branch_case(score, y, 3)


@pytest.mark.parametrize("n", [7, 8, 129, 8192, 8193])
def test_kde_branch_mean_in_numpys_summation_order(n):
    score, y = fx.normal_quantiles(n, 40 + n, scale=3.7, shift=0.1)
    rec = _branch_case(score, y, 4)
    assert fx.bits(rec.thres[2]) == fx.bits(np.mean(score))


def test_bisect_returns_an_end_point_on_an_exact_zero():
    from scipy.optimize import bisect
    score = np.array([0.1, 0.9, 0.4, 0.2])
    y = np.array([0, 1, 1, 0], bool)
    for prevalence, end in ((0.25, score.max()), (1.0, score.min())):
        assert bisect(lambda t: (score >= t).sum() / len(score) - prevalence, score.min(), score.max()) == end
        rc, (rec,) = fx.host_records(score, y, [(0, 4, prevalence, -1)])
        assert rc == 0 and rec.status == 0 and rec.bisect_fallback == 0
        assert fx.bits(rec.thres[1]) == fx.bits(end) == fx.bits(M.f1_with_pred_prev_constraint(y, score, prevalence, True)[1])


def test_bisect_sign_error_falls_back_to_fminbound():
    from scipy.optimize import bisect
    rng = np.random.default_rng(11)
    score = rng.random(20)
    score[:8] = 2.0                                     # 8 of 20 rows tied at the maximum > prevalence * n = 6
    y = rng.random(20) < 0.4
    y[:2] = [True, False]
    with pytest.raises(ValueError):
        bisect(lambda t: (score >= t).sum() / 20 - 0.3, score.min(), score.max())
    got, want = fx.host_dicts(score, y, [(0, 20, 0.3, -1)])[0], M.eval_metrics(y, score, 0.3)
    rc, (rec,) = fx.host_records(score, y, [(0, 20, 0.3, -1)])
    assert rec.bisect_fallback == 1 and isinstance(want["F1_prev_thres"], np.float64)
    skip = () if fx.kde_separated(score)[0] else fx.heuristic_keys()
    fx.same_dict(got, want, skip=skip, auc_bound=_auc_bound(20))


def _host_raises(score, y, prevalence=0.3):
    with pytest.raises(Exception) as e:
        M.eval_metrics(y, score, prevalence)
    return type(e.value)


@pytest.mark.parametrize("name", ["nan", "inf", "one-class", "one-row", "zero-variance", "zero-variance-one-class"])
def test_every_status_raises_what_the_host_path_raises_first(name):
    from lemon_amd import _lib, ops
    rng = np.random.default_rng(12)
    score, y = rng.random(12), rng.random(12) < 0.5
    y[:2] = [True, False]
    status = {"nan": _lib.EVAL_NONFINITE, "inf": _lib.EVAL_NONFINITE, "one-class": _lib.EVAL_ONE_CLASS, "one-row": _lib.EVAL_FEW_ROWS,
              "zero-variance": _lib.EVAL_ZERO_VARIANCE, "zero-variance-one-class": _lib.EVAL_ZERO_VARIANCE}[name]
    if name == "nan":
        score[5] = np.nan
    elif name == "inf":
        score[5] = np.inf
    elif name == "one-class":
        y[:] = True
    elif name == "one-row":
        score, y = score[:1], y[:1]
    else:
        score[:] = 0.5
        if name.endswith("one-class"):
            y[:] = False
    n = len(score)
    if name == "one-class":        # sklearn >= 1.7 warns and returns NaN where it used to raise; the device path keeps ValueError
        want = ValueError
    elif name == "inf":            # the host path dies in bisect (RuntimeError: no convergence); non-finite is ValueError here
        assert _host_raises(score, y) is RuntimeError
        want = ValueError
    else:
        want = _host_raises(score, y)
    assert want is (np.linalg.LinAlgError if status == _lib.EVAL_ZERO_VARIANCE else ValueError)
    # the bad segment between two good ones: its status is its own, the good ones equal their own call
    good_s, good_y = fx.mixture(60, 13)
    both_s, both_y = np.concatenate([good_s, score, good_s]), np.concatenate([good_y, y, good_y])
    segments = [(0, 60, 0.3, -1), (60, n, 0.3, -1), (60 + n, 60, 0.3, 0)]
    rc, recs = fx.host_records(both_s, both_y, segments)
    assert rc == 0 and [r.status for r in recs] == [0, status, 0]
    assert type(ops.eval_status_error(1, status)) is want
    with pytest.raises(want):
        ops.eval_records_dicts(recs, segments)
    alone = fx.host_dicts(np.tile(good_s, 2), np.tile(good_y, 2), [(0, 60, 0.3, -1), (60, 60, 0.3, 0)])
    for got, ref in zip((recs[0], recs[2]), alone):
        fx.same_dict(ops.eval_record_dict(got, recs[0]), ref, auc_bound=0.0)
    if name in ("nan", "one-class"):                    # the same rows as a fixed segment
        if name == "nan":
            with pytest.raises(ValueError):
                M.eval_metrics(y, score, 0.3, fix_thress=M.eval_metrics(good_y, good_s, 0.3))
        rc, recs = fx.host_records(both_s, both_y, [(0, 60, 0.3, -1), (60, n, 0.3, 0)])
        assert rc == 0 and [r.status for r in recs] == [0, status]
    # a fixed segment behind a free one that failed
    rc, recs = fx.host_records(both_s, both_y, [(60, n, 0.3, -1), (0, 60, 0.3, 0)])
    assert rc == 0 and [r.status for r in recs] == [status, _lib.EVAL_SOURCE]
    with pytest.raises(want):
        ops.eval_records_dicts(recs, [(60, n, 0.3, -1), (0, 60, 0.3, 0)])


def test_signed_zeros_two_decimals_and_a_single_positive():
    rng = np.random.default_rng(14)
    score = np.round(rng.standard_normal(300), 2)
    score[10:20], score[20:30] = -0.0, 0.0              # both zeros inside the range: one group of equal scores
    y = rng.random(300) < 0.3
    y[10:30] = np.tile([True, False], 10)
    for labels in (y, np.arange(300) == 15):           # P = 1: the one positive sits in the group of zeros
        prevalence = labels.sum() / 300
        got, want = _run_pattern(score, labels, prevalence, [300])
        skip = () if fx.kde_separated(score)[0] else fx.heuristic_keys()
        for g, w in zip(got, want):
            fx.same_dict(g, w, skip=skip, auc_bound=_auc_bound(300))
        swapped = score.copy()
        swapped[10:20], swapped[20:30] = 0.0, -0.0      # the order of the tied zeros reaches no result
        again, _ = _run_pattern(swapped, labels, prevalence, [300])
        for g, a in zip(got, again):
            fx.same_dict(g, a, auc_bound=0.0)


def test_golden_eval_metrics_vector():
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"), allow_pickle=False)
    y, score = g["in_y"], g["score_fixed"]
    ev = fx.host_dicts(np.tile(score, 2), np.tile(y, 2), [(0, len(y), y.mean(), -1), (len(y), len(y), y.mean(), 0)])
    keys, vals = g["eval_keys"].tolist(), g["eval_vals"]
    assert sorted(k for k, v in ev[0].items() if np.isscalar(v)) == keys
    for k, v in zip(keys, vals):
        assert abs(float(ev[0][k]) - v) < 1e-9, k
    assert ev[1]["F1_optimal"] == ev[0]["F1_optimal"] and ev[1]["F1_prev_thres"] == ev[0]["F1_prev_thres"]


def test_numpy_sum_order_restated():
    """the chunked pairwise rule behind the mean fall-back, through the twin: all scores but the zero-variance guard aside,
    a one-maximum KDE returns np.mean(score) bit for bit at the chunk and block edges"""
    for n in (2, 9, 127, 128, 130, 1000, 8191, 16385):
        score, y = fx.normal_quantiles(n, n, scale=1e3, shift=-7.0)
        if fx.scipy_branch(score) != 4:
            continue
        rc, (rec,) = fx.host_records(score, y, [(0, n, 0.4, -1)])
        assert rc == 0 and rec.status == 0 and rec.kde_branch == 4 and fx.bits(rec.thres[2]) == fx.bits(np.mean(score)), n


def test_refusals_write_nothing():
    from lemon_amd import _lib, ops
    lib = _lib.load()
    score, y = fx.mixture(50, 15)
    y8 = y.astype(np.uint8)

    def call(segments, S=None, total=50, null=None):
        segs = ops.eval_segments(segments)
        out = (_lib.EvalRecord * max(len(segments), 1))()
        ctypes.memset(ctypes.addressof(out), 0xA5, ctypes.sizeof(out))
        args = [score.ctypes.data, y8.ctypes.data, total, ctypes.addressof(segs), len(segments) if S is None else S, ctypes.addressof(out)]
        if null is not None:
            args[null] = None
        rc = lib.lemon_eval_metrics_host(*args)
        assert bytes(out) == b"\xa5" * ctypes.sizeof(out), "a refused call wrote into out"
        return rc

    good = [(0, 30, 0.3, -1), (30, 20, 0.3, 0)]
    assert fx.host_records(score, y, good)[0] == 0
    for null in (0, 1, 3):
        assert call(good, null=null) == -1
    assert call(good, S=0) == -1 and call(good, S=65536) == -1
    for bad in ([(-1, 10, 0.3, -1)], [(0, -5, 0.3, -1)], [(0, 0, 0.3, -1)], [(45, 6, 0.3, -1)], [(0, 30, 0.3, -1), (29, 10, 0.3, 0)],
                [(0, 30, 0.3, -1), (30, 20, 0.3, 1)], [(0, 30, 0.3, -1), (30, 20, 0.3, 2)], [(0, 30, 0.3, -2)], [(0, 30, 0.3, 0)]):
        assert call(bad) == -1, bad
    assert lib.lemon_eval_metrics_workspace_bytes(50, 0, 0) == -1 and lib.lemon_eval_metrics_workspace_bytes(0, 1, 1) == -1
    assert lib.lemon_eval_metrics_workspace_bytes(50, 2, 3) == -1 and lib.lemon_eval_metrics_workspace_bytes(1 << 31, 1, 1) == -1
    assert lib.lemon_eval_metrics_workspace_bytes(50, 1, 1) > 50 * 13 + 8000       # S > 1 asks hipcub, which asks for a device


def test_abi_is_declared_bound_and_built():
    from lemon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("lemon_eval_metrics_workspace_bytes", "lemon_eval_metrics", "lemon_eval_metrics_host", "lemon_eval_metrics_kde_host"):
        assert name + "(" in hdr and _lib.EXPORTS.count(name) == 1 and hasattr(lib, name), name
    assert "lib/metrics/utils.py:273-441" in hdr
    assert "eval_metrics.hip" in build.SOURCES and "eval_metrics_core.hpp" in build.HEADERS
    assert ctypes.sizeof(_lib.EvalRecord) == 152 and ctypes.sizeof(_lib.EvalSegment) == 32
    core = open(os.path.join(ROOT, "lemon_amd", "csrc", "eval_metrics_core.hpp")).read()
    assert not re.search(r"\bexp\(|\bpow\(|\blog\(", re.sub(r"//.*", "", core)), "libm's exp / pow / log differ between host and device"


def test_cli_flag_and_its_default():
    from lemon_amd import discrepancy_baseline, run_lemon
    for mod in (run_lemon, discrepancy_baseline):
        acts = {a.dest: a for a in mod.build_parser()._actions}
        assert acts["eval_metrics"].default == "host" and list(acts["eval_metrics"].choices) == ["host", "device"]
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--output_dir", "o", "--eval_metrics", "gpu"])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_core_header_alone_under_asan_and_ubsan(tmp_path):
    """csrc/eval_metrics_core.hpp driven by a stand-alone program against brute-force counts and straight-line sums"""
    exe = str(tmp_path / "eval_metrics_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "eval_metrics_fuzz.cpp"), "-o", exe])
    for seed in ("1", "20261021"):
        r = subprocess.run([exe, "400", seed], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "eval_metrics_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
