"""What the eval_metrics tests share: the host twin (lemon_eval_metrics_host) called on numpy arrays, seeded inputs, the
comparison rules.  A segment list is [(offset, n, prevalence, thres_from), ...] as ops.eval_metrics takes it."""
import ctypes

import numpy as np

COUNT_KEYS = ("accuracy", "F1", "n_samples", "TN", "FN", "TP", "FP", "error", "TPR", "FNR", "FPR", "TNR", "PPV", "NPV",
              "pred_prevalence", "prevalence", "balanced_acc")
SUFFIXES = ("_optimal", "_prev", "_heuristic")


def bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.int64)


def host_records(score, y, segments):
    """-> (rc, [LemonEvalRecord, ...]) of the host twin on numpy arrays"""
    from lemon_amd import _lib, ops
    lib = _lib.load()
    score = np.ascontiguousarray(score, np.float64)
    y = np.ascontiguousarray(np.asarray(y).astype(bool).astype(np.uint8))
    segs = ops.eval_segments(segments)
    out = (_lib.EvalRecord * len(segments))()
    rc = lib.lemon_eval_metrics_host(score.ctypes.data, y.ctypes.data, len(score), ctypes.addressof(segs), len(segments),
                                     ctypes.addressof(out))
    return rc, list(out)


def host_dicts(score, y, segments):
    from lemon_amd import ops
    rc, recs = host_records(score, y, segments)
    assert rc == 0, rc
    return ops.eval_records_dicts(recs, [tuple(g) for g in segments])


def twin_kde(score):
    """-> (grid [1000], density [1000]) as the twin evaluates gaussian_kde(score) on linspace(min, max, 1000)"""
    from lemon_amd import _lib
    score = np.ascontiguousarray(score, np.float64)
    grid, dens = np.empty(1000), np.empty(1000)
    rc = _lib.load().lemon_eval_metrics_kde_host(score.ctypes.data, len(score), grid.ctypes.data, dens.ctypes.data)
    assert rc == 0, rc
    return grid, dens


def scipy_kde(score):
    """-> (grid, density, minima indices, maxima indices) as f1_with_local_minima_finder sees them"""
    from scipy.signal import argrelextrema
    from scipy.stats import gaussian_kde
    score = np.asarray(score, np.float64)
    xs = np.linspace(score.min(), score.max(), 1000)
    dens = gaussian_kde(score).evaluate(xs)
    return xs, dens, argrelextrema(dens, np.less)[0], argrelextrema(dens, np.greater)[0]


def scipy_branch(score):
    """the branch of f1_with_local_minima_finder in LemonEvalRecord.kde_branch's numbering"""
    _, _, minima, maxima = scipy_kde(score)
    return 1 if len(minima) > 1 else 2 if len(minima) == 1 else 3 if len(maxima) >= 2 else 4


def kde_separated(score, gap=1e-9):
    """the condition on the inputs: scipy's own density differs between every pair of neighbouring grid points by more than
    `gap` relative -> (holds, the smallest relative difference)"""
    _, dens, _, _ = scipy_kde(score)
    rel = np.abs(np.diff(dens)) / np.maximum(np.abs(dens[1:]), np.abs(dens[:-1]))
    return bool(rel.min() > gap), float(rel.min())


def mixture(n, seed, centres=(0.0, 4.0), sd=1.0, p_pos=0.3):
    """a seeded mixture of Gaussians: the positives lean to the upper centres -> (score float64 [n], y bool [n])"""
    rng = np.random.default_rng(seed)
    comp = rng.integers(0, len(centres), n)
    score = np.asarray(centres)[comp] + sd * rng.standard_normal(n)
    y = rng.random(n) < np.where(comp >= len(centres) / 2, 1 - p_pos, p_pos)
    if y.all() or not y.any():
        y[0], y[-1] = True, False
    return score, y


def normal_quantiles(n, seed, scale=1.0, shift=0.0):
    """the n mid-quantiles of the central 80 % of a log-normal law (skewed: no two grid points mirror each other; no sparse
    tail for a bump to sit in) in a seeded order: a KDE with one maximum and no minimum at every n"""
    from scipy.special import ndtri
    rng = np.random.default_rng(seed)
    score = shift + scale * np.exp(0.25 * ndtri(0.1 + 0.8 * (np.arange(n) + 0.5) / n))
    rng.shuffle(score)
    y = rng.random(n) < 0.4
    y[0], y[-1] = True, False
    return score, y


def same_value(a, b, what):
    """equal by type and, for floats, by bits"""
    assert type(a) is type(b), (what, type(a), type(b))
    if isinstance(a, (float, np.floating)):
        assert bits(a) == bits(b), (what, a, b)
    else:
        assert a == b, (what, a, b)


def same_dict(got, want, skip=(), auc_bound=None):
    """every key in order; values by bits and type, except AUROC / AUPRC within auc_bound and the keys in `skip`"""
    assert list(got) == list(want)
    for key in want:
        if key in skip:
            continue
        if key in ("AUROC", "AUPRC"):
            assert type(got[key]) is type(want[key]) is float, key
            assert abs(got[key] - want[key]) <= auc_bound, (key, got[key], want[key], auc_bound)
        else:
            same_value(got[key], want[key], key)


def heuristic_keys():
    return ["F1_heuristic_thres"] + [f"{k}_heuristic" for k in COUNT_KEYS]
