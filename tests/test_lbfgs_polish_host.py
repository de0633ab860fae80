"""The LBFGS polish of the hyper-parameter search on the host twin (no GPU): csrc/lbfgs_core.hpp through
lemon_lbfgs_proxy_host / lemon_lbfgs_polish_host / lemon_lbfgs_math_host and through tests/native/lbfgs_fuzz.cpp.

What is compared with what, and the bounds:
  * the proxy against torch autograd in float64 on the same expression: |dloss| <= 1e-12 max(1, |loss|), |dgrad| <= 1e-10
    max(1, |grad|_inf) (float64 sums of at most 51 * 257 terms: about 1e4 * 2.2e-16, two decades of margin); measured here:
    4.4e-16 and 3.3e-16;
  * the restated exp / log1p against libm: special cases identical, elsewhere <= 4 ulp; measured: 1 ulp each;
  * the optimiser against torch.optim.LBFGS.  A whole run on the proxy cannot be compared (a rounding-sized change grows to
    O(1) within six outer steps: DESIGN.md section 5), so (a) ONE outer step on the proxy, both sides fed by
    lemon_lbfgs_proxy_host: nfev equal in all 12 pairs, x within 100 x the measured gap (7.2e-9 at n = 257, k = 17,
    x0 = 0.5, the other eleven below 2.6e-9; torch's dot products and axpy use FMA and another order) = 7.2e-7 < 1e-6;
    (b) all 20 outer steps on a convex quadratic and on Rosenbrock's function, where rounding does not grow: after every
    step (nfev, nit) equal and x within 100 x the measured gap.  Rosenbrock: measured 1.2e-12, bar 1.2e-10.  Quadratic:
    measured 0 (the same bits after every step), so the bar comes from the number format instead: 100 ulp of 1.0 = 2.2e-14.
    Both < 1e-8."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import hparamfx as fx
from tests import lbfgsfx as lx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 63, 257)
KS = (1, 5, 51)


@pytest.fixture(scope="module")
def records():
    return {n: (fx.record(n), lx.HostPolish(*fx.record(n))) for n in NS}


# ---------------------------------------------------------------------------------------------------------------- the proxy
@pytest.mark.parametrize("n", NS)
def test_proxy_value_and_gradient_match_autograd(records, n):
    (rec, y), hp = records[n]
    rng = np.random.default_rng(n)
    points = [[float(v) for v in s] for s in fx.STARTS] + [list(rng.uniform(0.0, 3.0, 6)), list(rng.uniform(-1.0, 12.0, 6))]
    worst_loss = worst_grad = 0.0
    for k in KS:
        for name, (fz, fo) in fx.ABLATIONS.items():
            f = hp.proxy(k, fz, fo)
            for x in points:
                loss, grad = f(x)
                want_loss, want_grad = lx.torch_proxy(rec, y, k, x, fz, fo)
                worst_loss = max(worst_loss, abs(loss - want_loss) / max(1.0, abs(want_loss)))
                worst_grad = max(worst_grad, float(np.max(np.abs(grad - want_grad))) / max(1.0, float(np.max(np.abs(want_grad)))))
                for nm in fz + fo:
                    assert grad[fx.HP_NAMES.index(nm)] == 0.0 and want_grad[fx.HP_NAMES.index(nm)] == 0.0, (name, nm)
    print(f"n={n}: worst |dloss| {worst_loss:.3g}, worst |dgrad| {worst_grad:.3g}")
    assert worst_loss <= 1e-12 and worst_grad <= 1e-10, (worst_loss, worst_grad)


def test_forced_coordinates_enter_as_constants(records):
    (rec, y), hp = records[63]
    a = hp.proxy(5, ("tau_1_n", "beta"), ("gamma", "beta"))([3.0, 4.0, 5.0, 0.25, 0.5, 0.75])
    b = hp.proxy(5)([1.0, 1.0, 0.0, 0.25, 0.5, 0.75])                     # zeros first, then ones: beta ends at 1
    assert a[0] == b[0]
    assert list(a[1][:3]) == [0.0, 0.0, 0.0] and np.array_equal(a[1][3:], b[1][3:])


@pytest.mark.parametrize("n", [63, 257])
def test_overflow_is_not_clamped(n):
    rec, y = fx.overflow_record(n)
    hp = lx.HostPolish(rec, y)
    loss, grad = hp.proxy(50)([800.0] * 6)
    assert not np.isfinite(loss)
    x0, spec = lx.polishes((50,), starts=([800] * 6,))
    x, loss, nfev, nit, status = hp.polish(x0, spec)[0]
    assert status == 1 and not (np.isfinite(loss) and np.all(np.isfinite(x)))
    assert 1 <= nfev <= 26 * lx.OUTER_STEPS and 0 <= nit <= 20 * lx.OUTER_STEPS      # a NaN ends within torch's own counters
    assert hp.polish(*lx.polishes((50,), starts=([0.5] * 6,)))[0][4] == 0            # a tame start on the same record is fine


# ---------------------------------------------------------------------------------------------------- restated exp / log1p
def _ulps(a, b):
    key = lambda v: np.where(v.view(np.int64) < 0, np.int64(-2 ** 63) - v.view(np.int64), v.view(np.int64))
    return np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b)))


def _math(fn, xs):
    from lemon_amd import _lib
    xs = np.ascontiguousarray(xs, np.float64)
    out = np.full_like(xs, 123.0)
    _lib.check(_lib.load().lemon_lbfgs_math_host(fn, fx._p(xs), len(xs), fx._p(out)), "lemon_lbfgs_math_host")
    return out


def _against_libm(fn, ref_fn, xs, what):
    got = _math(fn, xs)
    with np.errstate(all="ignore"):
        want = ref_fn(xs)
    special = ~np.isfinite(want) | (want == 0.0)                           # NaN, +-inf, +-0: identical, sign included
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    s = special & ~np.isnan(want)
    assert np.array_equal(got[s], want[s]) and np.array_equal(np.signbit(got[s]), np.signbit(want[s])), what
    worst = int(_ulps(got[~special], want[~special]).max())
    print(f"{what}: largest difference from libm {worst} ulp over {int((~special).sum())} arguments")
    assert worst <= 4, (what, worst)
    return worst


def test_restated_exp_against_libm():
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(-746.0, 710.0, 60000), rng.normal(0.0, 1.0, 20000), rng.uniform(-745.2, -707.0, 12000),
                         rng.uniform(709.0, 710.0, 5000), rng.uniform(-1e-8, 1e-8, 3000),
                         [0.0, -0.0, np.inf, -np.inf, np.nan, 709.782712893384, 709.7827128933841, 710.0, 711.0, 1e300,
                          -745.1332191019411, -745.1332191019412, -745.2, -746.0, -747.0, -1e300, 1e-300, -1e-300, 5e-324]])
    assert len(xs) >= 100000
    _against_libm(0, np.exp, xs, "exp")
    assert _math(0, [709.782712893384])[0] < np.inf and _math(0, [709.7827128933841])[0] == np.inf      # the overflow edge
    sub = _math(0, [-740.0])[0]
    assert 0.0 < sub < 2.2250738585072014e-308                               # a subnormal result


def test_restated_log1p_against_libm():
    rng = np.random.default_rng(6)
    xs = np.concatenate([np.exp(rng.uniform(-745.0, 709.0, 50000)), -np.exp(rng.uniform(-745.0, 0.0, 20000)),
                         rng.uniform(-1.0, 1.0, 20000), rng.uniform(-0.3, 0.45, 10000),
                         [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1.0000000000000002, -0.9999999999999999, -2.0, 5e-324, -5e-324,
                          1e-17, -1e-17, 1.7976931348623157e308, 0.4142, 0.41421356237309515, -0.2928, -0.2928932188134524]])
    assert len(xs) >= 100000
    _against_libm(1, np.log1p, xs, "log1p")


# --------------------------------------------------------------------------------------- the optimiser against torch.optim.LBFGS
ONE_STEP_CASES = [(250, 50), (257, 17), (63, 5)]
ONE_STEP_BAR = 100 * 7.2e-9            # 100 x the largest gap measured over the 12 pairs (docstring)


def test_one_outer_step_on_the_proxy_matches_torch():
    """(a): torch.optim.LBFGS and the restatement see the same function (lemon_lbfgs_proxy_host); no pair is left out."""
    assert ONE_STEP_BAR < 1e-6
    worst = 0.0
    for n, k in ONE_STEP_CASES:
        hp = lx.HostPolish(*fx.record(n))
        got = hp.polish(*lx.polishes((k,)), outer_steps=1)
        for s, start in enumerate(fx.STARTS):
            want_x, want_nfev = lx.torch_lbfgs(hp.proxy(k), start, 1)
            assert got[s][2] == want_nfev, (n, k, start[0], got[s][2], want_nfev)
            gap = lx.rel_gap(got[s][0], want_x)
            print(f"n={n} k={k} x0={start[0]}: nfev {want_nfev}, gap {gap:.3g}")
            worst = max(worst, gap)
    print(f"largest gap {worst:.3g}")
    assert worst <= ONE_STEP_BAR, worst


QUAD_C = np.array([1.0, 20.8, 40.6, 60.4, 80.2, 100.0])
QUAD_A = np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.25])
BENIGN_BARS = {"quadratic": 100 * 2.220446049250313e-16, "rosenbrock": 100 * 1.2e-12}     # the module docstring derives them


def _quadratic(x):
    return 0.5 * float(np.sum(QUAD_C * (x - QUAD_A) ** 2)), QUAD_C * (x - QUAD_A)


def _rosenbrock(x):
    a, b = x[1:] - x[:-1] ** 2, 1.0 - x[:-1]
    g = np.zeros(6)
    g[:-1] += -400.0 * a * x[:-1] - 2.0 * b
    g[1:] += 200.0 * a
    return float(np.sum(100.0 * a * a + b * b)), g


def _build_fuzz(tmp_path, sanitize):
    exe = str(tmp_path / ("lbfgs_fuzz_san" if sanitize else "lbfgs_fuzz"))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, os.path.join(ROOT, "tests", "native", "lbfgs_fuzz.cpp"),
                           "-o", exe])
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_twenty_outer_steps_on_benign_functions_match_torch(tmp_path):
    """(b): the header alone (tests/native/lbfgs_fuzz.cpp trace) against torch on the same two functions, after every step"""
    assert all(bar < 1e-8 for bar in BENIGN_BARS.values())
    r = subprocess.run([_build_fuzz(tmp_path, False), "trace"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {"quadratic": [], "rosenbrock": []}
    for line in r.stdout.split("\n"):
        parts = line.split()
        if parts:
            rows[parts[0]].append((int(parts[2]), int(parts[3]), np.array([float.fromhex(v) for v in parts[4:]])))
    for name, f, x0 in (("quadratic", _quadratic, [1.0] * 6), ("rosenbrock", _rosenbrock, [-1.2, 1.0] * 3)):
        import torch
        x = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
        opt = torch.optim.LBFGS([x], lr=0.1, max_iter=20, line_search_fn="strong_wolfe")

        def closure():
            loss, grad = f(x.detach().numpy().copy())
            x.grad = torch.as_tensor(grad).clone()
            return torch.tensor(loss, dtype=torch.float64)

        assert len(rows[name]) == lx.OUTER_STEPS
        worst, counters = 0.0, []
        for s in range(lx.OUTER_STEPS):
            opt.step(closure)
            st = opt.state[x]
            counters.append((st["func_evals"], st["n_iter"]))
            assert rows[name][s][:2] == counters[-1], (name, s, rows[name][s][:2], counters[-1])
            worst = max(worst, lx.rel_gap(rows[name][s][2], x.detach().numpy()))
        print(f"{name}: largest gap over the 20 steps {worst:.3g}; (nfev, nit) {counters[0]} .. {counters[-1]}")
        assert worst <= BENIGN_BARS[name], (name, worst)
        if name == "quadratic":
            # later steps find opt_cond true at once: one evaluation, no iteration
            early = [s for s in range(1, lx.OUTER_STEPS) if counters[s] == (counters[s - 1][0] + 1, counters[s - 1][1])]
            assert len(early) >= 10, counters
            assert np.max(np.abs(_quadratic(rows[name][-1][2])[1])) <= 1e-7
        else:
            assert np.max(np.abs(rows[name][-1][2] - 1.0)) < 1e-4         # the valley's end


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_core_header_alone_under_asan_and_ubsan(tmp_path):
    """csrc/lbfgs_core.hpp driven by a stand-alone program: NaN-returning and constant objectives, history eviction, exp / log1p"""
    exe = _build_fuzz(tmp_path, True)
    for seed in ("1", "20261020"):
        r = subprocess.run([exe, "1500", seed], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "lbfgs_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    r = subprocess.run([exe, "trace"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.strip().split("\n")) == 2 * lx.OUTER_STEPS, r.stderr[-2000:]


def test_host_polish_is_deterministic_and_sees_the_prefix(records):
    (rec, y), hp = records[257]
    x0, spec = lx.polishes((5, 51))
    a, b = hp.polish(x0, spec), hp.polish(x0, spec)
    for p, q in zip(a, b):
        assert np.array_equal(p[0].view(np.int64), q[0].view(np.int64)) and p[1:] == q[1:]
    shallow = lx.HostPolish({key: (v if key == "d_1" else np.ascontiguousarray(v[:, :5])) for key, v in rec.items()}, y)
    for p, q in zip(a[:4], shallow.polish(*lx.polishes((5,)))):
        assert np.array_equal(p[0].view(np.int64), q[0].view(np.int64)) and p[1:] == q[1:]


# ------------------------------------------------------------------------------------------------------------ maximize_metric
def _toy():
    rec, y = fx.record(65)
    score = lambda hp: (rec["d_1"].astype(np.float64) + hp["beta"] * rec["dists_n"][:, :5].mean(1)
                        + hp["gamma"] * rec["dists_m"][:, :5].mean(1))
    return rec, y, score


def test_maximize_metric_consumes_polished_candidates_in_order_under_strict_greater():
    from lemon_amd import metrics as M
    rec, y, score = _toy()
    grid = {"beta": [0.0], "gamma": [0.0], "tau_1": [0.0], "tau_2": [0.0]}
    x0s = [[0] * 6, [1] * 6, [2] * 6]
    asked, scored = [], []

    def counting_score(hp):
        scored.append([hp[nm] for nm in M.HP_NAMES])
        return score(hp)

    def polish(cands):
        def f(x0s_, force_zero, force_one):
            asked.append(([list(x) for x in x0s_], tuple(force_zero), tuple(force_one)))
            return cands
        return f

    search = lambda vals: (lambda x0s_, methods, fz, fo: [(np.full(6, 9.0), v) for v in vals])
    f1 = lambda x: M.optimize_f1_efficient(y, score(M.unpack_vector(x)))
    c1, c2 = [0.0, 7.0, 0, 0, 0, 0], [3.0, 0.0, 0, 0, 0, 0]
    assert f1(c1) != f1(c2) and f1(c1) > 0 and f1(c2) > 0
    hi, lo = (c1, c2) if f1(c1) > f1(c2) else (c2, c1)
    # after the scipy results: a local search worth more than any F1 keeps the lead, the candidates are still scored, in order
    best, val, _ = M.maximize_metric(counting_score, y, grid, x0s, local_search=search([-2.0] * 6), lbfgs_polish=polish([lo, hi, lo]))
    assert val == 2.0 and best == [9.0] * 6
    assert scored[:3] == [lo, hi, lo] and asked == [([[0] * 6, [1] * 6, [2] * 6], (), ())]
    # strict '>': of two equal candidates the first wins; a non-finite one is skipped and never scored; the grid comes after
    nan = [np.nan] * 6
    twin = list(hi)
    twin[5] = 4.0                                   # tau_2_m is multiplied by gamma = 0 or acts on a constant: same scores
    assert f1(twin) == f1(hi)
    del scored[:]
    best, val, _ = M.maximize_metric(counting_score, y, grid, x0s, local_search=search([0.0] * 6), lbfgs_polish=polish([nan, hi, twin]))
    assert best == hi and val == f1(hi) and val > f1([0.0] * 6)
    assert scored[:2] == [hi, twin] and not any(np.isnan(v).any() for v in scored)
    best, val, _ = M.maximize_metric(score, y, grid, x0s, local_search=search([0.0] * 6), lbfgs_polish=polish([[np.inf] * 6, nan, nan]))
    assert best == [0.0] * 6 and val == f1([0.0] * 6)                        # nothing left but the grid point
    with pytest.raises(AssertionError):
        M.maximize_metric(score, y, grid, x0s, local_search=search([0.0] * 6), lbfgs_polish=polish([hi]))
    # the forced coordinates of the winner are pinned in what is returned
    best, _, _ = M.maximize_metric(score, y, grid, x0s, local_search=search([0.0] * 6), lbfgs_polish=polish([hi, lo, lo]),
                                   force_zero=("tau_2_m",), force_one=("tau_1_n",))
    assert best[5] == 0.0 and best[2] == 1.0 and best[:2] == hi[:2]


def test_maximize_metric_without_the_hook_is_unchanged(oracle):
    """lbfgs_polish=None on the record of test_metrics_golden: the full protocol still gives the reference's golden result"""
    from lemon_amd import metrics as M
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"), allow_pickle=False)
    rec = {nm: g[f"in_{nm}"] for nm in fx.REC_KEYS}
    grid = {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}
    bx, bv, bt = M.maximize_metric(lambda hp: oracle.score(rec, hp), g["in_y"], grid, [[0] * 6, [1] * 6],
                                   scipy_methods=("Nelder-Mead",), rec_for_lbfgs=rec, lbfgs_polish=None)
    assert abs(bv - float(g["search_best_val"])) < 1e-9
    assert np.allclose(bx, g["search_best_x"], rtol=1e-6, atol=1e-8)
    assert abs(bt - float(g["search_best_thres"])) < 1e-6


# ------------------------------------------------------------------------------------------------------------------- parser
def test_flag_defaults_to_host_and_changes_nothing_else():
    from lemon_amd.run_lemon import build_parser
    args = vars(build_parser().parse_args(["--output_dir", "x"]))
    assert args["lbfgs_polish"] == "host" and args["hparam_search"] == "host" and args["lbfgs_device"] == "cuda"
    dev = vars(build_parser().parse_args(["--output_dir", "x", "--lbfgs_polish", "device"]))
    assert dev["lbfgs_polish"] == "device"
    assert {k: v for k, v in dev.items() if k != "lbfgs_polish"} == {k: v for k, v in args.items() if k != "lbfgs_polish"}
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--output_dir", "x", "--lbfgs_polish", "cuda"])


# ---------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("lemon_lbfgs_polish", "lemon_lbfgs_polish_host", "lemon_lbfgs_proxy_host", "lemon_lbfgs_math_host")


def test_abi_names_layout_and_unit():
    from lemon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.PolishResult) == 72
    assert "LemonPolishResult { double x[6]; double loss; int32_t nfev, nit, status, pad; }" in hdr
    assert "lbfgs_polish.hip" in build.SOURCES and "lbfgs_core.hpp" in build.HEADERS
    assert _lib.POLISH_OUTER_STEPS == 20
    core = open(os.path.join(ROOT, "lemon_amd", "csrc", "lbfgs_core.hpp")).read()
    assert f"constexpr int THREADS = {lx.THREADS}," in core            # the GPU tests size their records by it


def test_bad_arguments_are_refused_with_a_message(records):
    from lemon_amd import _lib
    lib = _lib.load()
    (rec, y), hp = records[63]
    good_x0, good_spec = lx.polishes((5,))

    def refused(spec=good_spec, x0=good_x0, n=hp.n, null=None, outer=20, S=None):
        arrs = [ctypes.c_void_p(a.ctypes.data) for a in hp.arrs] + [ctypes.c_void_p(hp.y.ctypes.data)]
        if null is not None:
            arrs[null] = None
        spec = np.ascontiguousarray(spec, np.int32)
        count = spec.shape[0] if S is None else S
        out = (_lib.PolishResult * spec.shape[0])()
        ctypes.memset(ctypes.byref(out), 0x5a, ctypes.sizeof(out))
        rc = lib.lemon_lbfgs_polish_host(*arrs, n, hp.kmax, count, ctypes.c_void_p(x0.ctypes.data), ctypes.c_void_p(spec.ctypes.data),
                                         outer, ctypes.byref(out))
        untouched = bytes(out) == b"\x5a" * ctypes.sizeof(out)
        return rc, lib.lemon_last_error().decode(), untouched

    assert refused()[0] == 0 and not refused()[2]
    for kw, word in ((dict(null=0), "null"), (dict(null=7), "null"), (dict(n=0), "n > 0"), (dict(outer=0), "outer_steps"),
                     (dict(outer=21), "outer_steps"), (dict(S=65536), "65535"), (dict(S=-1), "S")):
        rc, msg, untouched = refused(**kw)
        assert rc == -1 and word in msg and untouched, (kw, rc, msg)
    for col, val, word in ((0, 0, "k"), (0, hp.kmax + 1, "k"), (1, 64, "mask"), (2, -1, "mask")):
        spec = good_spec.copy()
        spec[3, col] = val
        rc, msg, untouched = refused(spec=spec)
        assert rc == -1 and word in msg and untouched, (col, val, rc, msg)
    # the device entry refuses the same before it touches the device: n <= 0 and null pointers need no GPU
    rc = lib.lemon_lbfgs_polish(*[None] * 8, 0, 5, 1, None, None, 20, None, None)
    assert rc == -1 and "n > 0" in lib.lemon_last_error().decode()
    one = ctypes.c_void_p(hp.arrs[0].ctypes.data)
    rc = lib.lemon_lbfgs_polish(*[one] * 8, 5, 5, 1, None, None, 20, None, None)
    assert rc == -1 and "null" in lib.lemon_last_error().decode()
    loss, _ = hp.proxy(hp.kmax + 1)(np.zeros(6))
    assert np.isnan(loss) and "k <= kmax" in lib.lemon_last_error().decode()
    assert lib.lemon_lbfgs_math_host(2, None, 0, None) == -1
