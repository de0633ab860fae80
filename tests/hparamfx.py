"""Fixtures of the hyper-parameter local-search tests (test_hparam_search_host.py, test_gpu_hparam_search.py): seeded records
whose scores depend on the label, the product's searches, scipy as the reference and the comparison rules.

Comparison rules (every scipy comparison): x bit for bit (float64 viewed as int64), fun ==, nfev / nit / status equal.  No
tolerances anywhere."""
import ctypes

import numpy as np

REC_KEYS = ("d_1", "D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m")
HP_NAMES = ("beta", "gamma", "tau_1_n", "tau_2_n", "tau_1_m", "tau_2_m")
STARTS = ([0] * 6, [0.5] * 6, [1] * 6, [10] * 6)          # run_lemon._tail
METHODS = ("Powell", "Nelder-Mead")                        # maximize_metric's scipy_methods
KMAX = 51
# run_lemon._grid_setup: ablation -> (force_zero, force_one)
ABLATIONS = {"none": ((), ()), "tau_1": (("tau_1_n", "tau_1_m"), ()), "tau_2": (("tau_2_n", "tau_2_m"), ()),
             "tau_1_2": (("tau_1_n", "tau_1_m", "tau_2_n", "tau_2_m"), ()), "beta": (("beta",), ()), "gamma": (("gamma",), ()),
             "d1": ((), ("beta",))}


def record(n, kmax=KMAX, seed=0, labels="mixed"):
    """(rec: dict of numpy float32 arrays, y uint8 [n]).  A mislabelled sample sits further from its caption (d_1) and from
    the captions of its neighbours (dists_*), with overlap, so that F1 moves with every hyper-parameter.  labels: 'mixed'
    (about 40 % mislabelled, at least one of each where n >= 2), 'zeros', 'ones'."""
    rng = np.random.default_rng(1000 * seed + n)
    y = (rng.uniform(size=n) < 0.4).astype(np.uint8)
    if n >= 2:
        y[0], y[1] = 1, 0
    shift = y.astype(np.float64)
    rec = {"d_1": (rng.normal(0.55, 0.12, n) + 0.10 * shift).astype(np.float32)}
    for side in "nm":
        rec["D_" + side] = np.sort(rng.uniform(0.05, 1.2, (n, kmax)), axis=1).astype(np.float32)
        rec["dists_tr_" + side] = rng.uniform(0.2, 1.4, (n, kmax)).astype(np.float32)
        rec["dists_" + side] = (rng.normal(0.7, 0.15, (n, kmax)) + 0.12 * shift[:, None]).astype(np.float32)
    if labels == "zeros":
        y[:] = 0
    elif labels == "ones":
        y[:] = 1
    return rec, y


def overflow_record(n, kmax=KMAX, seed=0):
    """dists_tr near 0.9, negative D: at x0 = [800] * 6 exp(-tau_1 D) overflows, the objective is 0.0 there."""
    rec, y = record(n, kmax, seed)
    rng = np.random.default_rng(77 + n)
    for side in "nm":
        rec["D_" + side] = -rng.uniform(0.8, 1.0, (n, kmax)).astype(np.float32)
        rec["dists_tr_" + side] = rng.uniform(0.88, 0.92, (n, kmax)).astype(np.float32)
    return rec, y


def mask(names):
    return sum(1 << HP_NAMES.index(nm) for nm in names)


def searches(ks, force_zero=(), force_one=(), starts=STARTS, methods=METHODS):
    """(x0 [S,6] float64, spec [S,4] int32, labels) in ops.local_search's order: for each k, for each x0, for each method."""
    from lemon_amd import _lib
    x0, spec, labels = [], [], []
    for k in ks:
        for s in starts:
            for m in methods:
                x0.append([float(v) for v in s])
                spec.append([_lib.SEARCH_METHODS[m], k, mask(force_zero), mask(force_one)])
                labels.append((k, tuple(s), m))
    return np.asarray(x0, np.float64).reshape(-1, 6), np.asarray(spec, np.int32).reshape(-1, 4), labels


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class HostRecord:
    """The record as contiguous host arrays + the two host entry points of the library."""

    def __init__(self, rec, y):
        from lemon_amd import _lib
        self.lib = _lib.load()
        self.arrs = [np.ascontiguousarray(rec[k], np.float32) for k in REC_KEYS]
        self.y = np.ascontiguousarray(np.asarray(y).astype(bool).astype(np.uint8))
        self.n, self.kmax = self.arrs[1].shape

    def objective(self, k, force_zero=(), force_one=()):
        fz, fo = mask(force_zero), mask(force_one)

        def f(x):
            x = np.ascontiguousarray(x, np.float64)
            return self.lib.lemon_hparam_objective_host(*[_p(a) for a in self.arrs], _p(self.y), self.n, self.kmax, int(k), fz,
                                                        fo, _p(x))
        return f

    def search(self, x0, spec):
        from lemon_amd import _lib
        x0 = np.ascontiguousarray(x0, np.float64)
        spec = np.ascontiguousarray(spec, np.int32)
        S = spec.shape[0]
        out = (_lib.SearchResult * max(S, 1))()
        ws = np.empty(max(S * self.n, 1), np.float64)
        rc = self.lib.lemon_hparam_search_host(*[_p(a) for a in self.arrs], _p(self.y), self.n, self.kmax, S, _p(x0), _p(spec),
                                               _p(ws), ws.nbytes, ctypes.byref(out))
        _lib.check(rc, "lemon_hparam_search_host")
        return [result_tuple(out[s]) for s in range(S)]


def result_tuple(r):
    return (np.array(list(r.x), np.float64), float(r.fun), int(r.nfev), int(r.nit), int(r.status))


def scipy_search(objective, x0, method, options=None):
    import warnings
    from scipy.optimize import minimize
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = minimize(objective, x0, method=method, options=dict(options or {}))
    return (np.asarray(res.x, np.float64), float(res.fun), int(res.nfev), int(res.nit), int(res.status))


def assert_same(got, want, what=""):
    """the comparison rules of the module docstring"""
    gx, gf, gnfev, gnit, gst = got
    wx, wf, wnfev, wnit, wst = want
    assert (gnfev, gnit, gst) == (wnfev, wnit, wst), f"{what}: (nfev, nit, status) {(gnfev, gnit, gst)} != scipy's {(wnfev, wnit, wst)}"
    assert np.array_equal(gx.view(np.int64), wx.view(np.int64)), f"{what}: x {gx!r} != scipy's {wx!r}"
    assert gf == wf, f"{what}: fun {gf!r} != scipy's {wf!r}"
