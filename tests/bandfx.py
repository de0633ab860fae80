"""Worst-case-rounding inputs for the 16-bit kNN filter scan (lemon_amd/csrc/knn_bf16.hip) and a numpy model of its error band.

The scan drops a row when its fp16 filter score s~ is at most tau~ - 2 eps (tau~: the k-th largest s~, eps: band_eps_raw).  On
random data the d rounding errors of a score cancel and |s~ - s| stays 10-30 times inside eps, so a band half as wide would lose
nothing.  adversarial() builds data on which they all ADD:

* the query is c * sigma * 2^j: c the fp16 value nearest 1/sqrt(d), sigma a sign vector -- fp16-exact (qres2 = 0), constant
  magnitude, so that Cauchy-Schwarz in  sum q (x - xh) <= ||q|| ||x - xh||  is an equality for every row whose rounding residual is
  sigma times a constant;
* a VICTIM has components sigma_i (g_i + h (1 - DELTA)): g_i on the fp16 grid just above a power of two 2^e (where the half-ulp h is
  largest relative to g), so every component sits one float32 ulp below an fp16 rounding midpoint and rounds DOWN: s~ = s - eps_r;
* an IMPOSTOR has components sigma_i (g'_i + h (1 + DELTA)), every one rounds UP: s~ = s + eps_r.  g' is g with `t` components one
  grid step lower, so the exact score is below the victims' by (t - d DELTA) grid steps: enough for the fmaf chain's own rounding
  (LOWERED), far too little to matter next to eps_r (d/2 grid steps);
* a NEUTRAL row is fp16-exact (s~ = s) with an exact score a little below the victims': inside the band, in nobody's top-k.  They
  are what is appended after the contested rows arrived, so that the lists are light-compacted (every REFRESH = 96 appends) while
  they hold victims and impostors.  There are as many as fit a list next to the contested rows without overflowing the smallest
  capacity (192 keys: the one-block kernel's pair of half-lists) -- an overflowing band is settled exactly on the spot, which
  would take the decision away from the light compaction;
* a FILLER is a victim-like row scaled by 0.60 ... 0.98, ascending with its position: clearly below the contested range in both
  scores (2 % against a band of 0.15 %), but every one beats all fillers before it, so a list that has seen nothing else admits them
  all and is light-compacted every 96 rows.

2^e is chosen below c (x is about 0.5-0.8 of q, component by component, and the queries are scaled UP by 2^j only): then a lower
component is a worse row for squared L2 as well, and one construction serves both metrics.  The victims are the exact top-k, the
impostors the filter's top-k, and the victims' filter scores lie rho * 2 eps below tau~ with rho close to eps_r / eps: what is left
is the band's fp32-sum term 3 d 2^-24 ||q|| max||x||, which rounding cannot fill.
"""
import numpy as np

DELTA = 2.0 ** -12          # distance from the fp16 midpoint in half-ulps: ONE float32 ulp of g + h, the least there is
LAYOUTS = ("impostors_first", "victims_first", "interleaved", "apart")
REFRESH = 96                # knn_bf16.hip: new candidates per query that trigger a light compaction
N_FILLER_MIN = 3 * REFRESH
BAND_ROWS = 184            # victims + impostors + neutral rows: what a query's band holds (< 192, see the module docstring)


def n_neutral(k):
    return min(160, BAND_ROWS - (2 * k + 8))

# components of an impostor that are one grid step lower, per d: the exact score gap to the victims is (t - d DELTA) grid steps
# c * 2h.  The fmaf chain over d terms of one sign has a rounding error of about 0.3 sqrt(d) 2^-24 s = 2.6e-5 d^1.5 (t = 1) steps for
# inner product, and squared L2 adds the roundings of |x|^2 and of |q|^2 + |x|^2 on a four times smaller step (x is 0.5-0.8 of
# q); the values keep that noise 6-10 times below the gap and cost t / d of the tightness (< 2.5 %)
LOWERED = {64: 2, 200: 3, 512: 8, 768: 12, 1000: 18, 1280: 24}

# tightness rho = (tau~ - min over the oracle's top-k of s~) / (2 eps) that at least half of a case's queries must reach
# (tests/test_knn_band_host.py).  d: (floor, reached).  `reached` is the smallest per-case MEDIAN over all layouts, both metrics
# and both query families as measured with this generator; floor = reached - 0.03.  Every floor is above 0.5, so a band half as
# wide cannot pass at any kernel.  The rest to 1 is the fp32-sum term's share of eps: 3 d 2^-24 / (2^-11 + 3 d 2^-24).
FLOORS = {
    64:   (0.91, 0.944),
    200:  (0.88, 0.913),
    512:  (0.79, 0.827),
    768:  (0.73, 0.765),
    1000: (0.68, 0.716),
    1280: (0.63, 0.666),
}


def to_fp16(v):
    """what k_convert_bf16 stores: clamp to +-65 504, round to nearest even, fp16 subnormals flushed to zero"""
    b = np.clip(np.asarray(v, dtype=np.float32), np.float32(-65504.0), np.float32(65504.0)).astype(np.float16)
    b[np.abs(b.astype(np.float32)) < np.float32(2.0 ** -14)] = 0
    return b


def band_eps(d, qn, qres2, xn2, xr2, xh2, l2):
    """band_eps_raw of knn_bf16.hip, float32 operation by operation (qn, qres2: per query; xn2, xr2, xh2: database maxima)"""
    f = np.float32
    qn, qres2 = np.asarray(qn, dtype=f), np.asarray(qres2, dtype=f)
    xn2, xr2, xh2 = f(xn2), f(xr2), f(xh2)
    with np.errstate(all="ignore"):
        nq = np.sqrt(qn) * f(1.0005)
        eps = (nq * np.sqrt(xr2) + np.sqrt(qres2) * np.sqrt(xh2)) * f(1.002) \
            + f(3.0) * f(d) * f(5.9604645e-8) * nq * np.sqrt(xn2) * f(1.002) + f(1e-30)
        if l2:
            eps = f(2.0) * eps + f(4.8e-7) * (qn + xn2)
        eps = np.where(np.isnan(eps), f(np.inf), eps)          # 0 * inf: the band admits everything
    return eps.astype(f)


def filter_scores(metric, X, Q):
    """(S [nq, n] float64, eps [nq] float32): the filter's score of every pair -- float64 dot of the fp16 copies; for l2 the
    kernels' proxy 2 s~ - |x|^2 - |q|^2 with float32 norms of the originals -- and every query's band"""
    X, Q = np.asarray(X, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    Xh, Qh = to_fp16(X).astype(np.float64), to_fp16(Q).astype(np.float64)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    xn = (X64 * X64).sum(1).astype(np.float32)
    qn = (Q64 * Q64).sum(1).astype(np.float32)
    S = Qh @ Xh.T
    if metric == "l2":
        S = 2.0 * S - xn.astype(np.float64)[None, :] - qn.astype(np.float64)[:, None]
    eps = band_eps(X.shape[1], qn, ((Q64 - Qh) ** 2).sum(1), xn.max(), ((X64 - Xh) ** 2).sum(1).max(), (Xh * Xh).sum(1).max(),
                   metric == "l2")
    return S, eps


def filter_topk(S, k):
    """the k rows of largest filter score per query (as a set: unordered)"""
    return np.argpartition(-S, k - 1, axis=1)[:, :k]


def tightness(metric, X, Q, k, I_oracle, scores=None):
    """per query rho = (tau~ - min over the ORACLE's top-k of s~) / (2 eps); tau~ = k-th largest s~ over the whole database"""
    S, eps = scores if scores is not None else filter_scores(metric, X, Q)
    tau = -np.partition(-S, k - 1, axis=1)[:, k - 1]
    low = np.take_along_axis(S, np.asarray(I_oracle, dtype=np.int64), axis=1).min(1)
    return (tau - low) / (2.0 * eps.astype(np.float64))


def _grid(d):
    """(c, g0, step): the queries' magnitude and the binade [g0, 2 g0) of the contested rows with its fp16 grid step.  g0 is the
    largest power of two that leaves g0 * 1.05 <= 0.8 c"""
    c = float(np.float16(1.0 / np.sqrt(d)))
    m, ex = np.frexp(c)                         # c = m * 2^ex, 0.5 <= m < 1
    g0 = 2.0 ** (ex - 1) if 2.0 * m >= 1.3125 else 2.0 ** (ex - 2)
    return c, g0, g0 * 2.0 ** -10


def _positions(layout, n, nv, ni, nn, rng):
    """database rows of the victims, impostors and neutral rows; every other row is a filler"""
    if layout == "impostors_first":             # tau~ is the impostors' from the first tile on; the victims meet `a > th` in the last
        I = np.arange(ni)
        V = np.arange(n - nv, n)
        N = np.linspace(ni + 8, n - nv - 8, nn).astype(np.int64)
    elif layout == "victims_first":             # 3 x 96 fillers, victims, neutral rows, impostors, neutral rows, fillers
        V = N_FILLER_MIN + 12 + np.arange(nv)
        mid = n // 2 + 37
        I = mid + np.arange(ni)
        N = np.concatenate([np.linspace(V[-1] + 5, mid - 5, nn // 3).astype(np.int64),
                            np.linspace(I[-1] + 5, n - 40, nn - nn // 3).astype(np.int64)])
    elif layout == "apart":                     # opposite ends: database splits and chunked launches separate them.  The impostors
        V = np.arange(nv)                       # end where the last whole 128-row tile before the final one begins, and that tile
        tail = ((n - 1) // 128 - 1) * 128       # holds up to 100 neutral rows: the streaming kernel settles the final tile exactly,
        I = tail - ni + np.arange(ni)           # so this is the last light compaction that can see both kinds
        nt = min(nn, 100)
        N = np.concatenate([np.linspace(nv + 8, I[0] - 8, nn - nt).astype(np.int64), tail + np.linspace(0, 127, nt).astype(np.int64)])
    elif layout == "interleaved":               # all three kinds, shuffled, on both sides of every 64-row tile boundary
        slots = []
        for p in range(n):
            for b in range(64, n, 64):
                slots += [b - 1 - p, b + p] if b + p < n else [b - 1 - p]
            if len(slots) >= nv + ni + nn:
                break
        slots = np.array(slots[:nv + ni + nn])
        kind = rng.permutation(np.repeat([0, 1, 2], [nv, ni, nn]))
        V, I, N = slots[kind == 0], slots[kind == 1], slots[kind == 2]
    else:
        raise ValueError(layout)
    assert len(np.unique(np.concatenate([V, I, N]))) == nv + ni + nn and max(V.max(), I.max(), N.max()) < n
    return V, I, N


def adversarial(metric, d, k, layout, seed, n=1900, nq=300):
    """(X [n, d], Q [nq, d]) float32: k victims, k + 8 impostors, n_neutral(k) neutral rows, the rest fillers (module docstring).
    Queries: two thirds c sigma 2^j with j in {0, 1, 2} (qres2 = 0), one third the same with every component off by a random
    factor 1 + eta, |eta| <= 2^-16 (rounds back to c sigma 2^j: qres2 != 0; that term of the band is then slack)."""
    assert metric in ("ip", "l2")               # (one construction serves both: see the module docstring)
    rng = np.random.default_rng(seed)
    c, g0, step = _grid(d)
    h, t = step / 2.0, LOWERED[d]
    nv, ni, nn = k, k + 8, n_neutral(k)
    assert n - nv - ni - nn >= N_FILLER_MIN and n % 64 != 0
    sigma = rng.choice([-1.0, 1.0], d)
    V, I, N = _positions(layout, n, nv, ni, nn, rng)
    kind = np.full(n, 3)
    kind[V], kind[I], kind[N] = 0, 1, 2
    F = np.flatnonzero(kind == 3)
    lam = np.empty(n)
    lam[F] = np.linspace(0.60, 0.98, len(F))    # ascending with the position
    X = np.empty((n, d))
    for r in range(n):
        gm = (np.arange(d) % 4)[rng.permutation(d)].astype(np.float64)      # grid offsets: the same multiset in every row
        if kind[r] == 0:
            a = g0 + gm * step + h * (1.0 - DELTA)
        elif kind[r] == 1:
            gm[rng.choice(np.flatnonzero(gm >= 1), t, replace=False)] -= 1  # which components are the odd ones varies
            a = g0 + gm * step + h * (1.0 + DELTA)
        elif kind[r] == 2:                      # d/2 - t - u components a step higher: (t + u - d DELTA / 2) steps below the victims
            u = int(rng.integers(1, max(2, d // 8)))
            gm[rng.choice(d, d // 2 - t - u, replace=False)] += 1
            a = g0 + gm * step
        else:
            a = lam[r] * (g0 + gm * step + h * (1.0 - DELTA))
        X[r] = sigma * a
    X32 = X.astype(np.float32)
    contested = kind != 3
    assert np.array_equal(X32[contested].astype(np.float64), X[contested])      # 24 significant bits: exact in float32
    j = rng.integers(0, 3, nq)
    Q = c * sigma[None, :] * (2.0 ** j)[:, None]
    off = np.arange(nq) % 3 == 2
    Q[off] *= 1.0 + rng.uniform(-1.0, 1.0, (int(off.sum()), d)) * 2.0 ** -16
    Q32 = Q.astype(np.float32)
    assert np.array_equal(Q32[~off].astype(np.float64), Q[~off])
    assert len(np.unique(X32, axis=0)) == n
    return np.ascontiguousarray(X32), np.ascontiguousarray(Q32)


# ---- the cases of tests/test_gpu_knn_band.py; tests/test_knn_band_host.py checks the data of every one on the CPU -------------
DIMS = (64, 200, 512, 768, 1000, 1280)
# 29 tiles of 64 (14 of 128) + 44 rows: fewer than the 16 tiles from which the plan splits the database between workgroups (a
# split scans its rows with a tau of its own, so victims and impostors in different splits never meet); two panels of 128 (one
# of 256) + 44 queries
N_ROWS, N_QUERIES = 1900, 300

# kernel, LEMON_* environment, wide filter, d, metrics: how each of the five scan kernels is reached (knn_bf16_plan.hpp)
_FORCED = {"LEMON_QS2_MIN_PANELS": "0"}
_FORCED_QS2 = {"LEMON_QS2_MIN_PANELS": "0", "LEMON_QS4": "0"}
KERNELS = [
    ("qs", {}, False, 64, ("ip", "l2")), ("qs", {}, False, 200, ("ip", "l2")), ("qs", {}, False, 512, ("ip", "l2")),
    ("qs4", _FORCED, False, 512, ("ip", "l2")), ("qs4", _FORCED, False, 768, ("ip",)),
    ("qs2", _FORCED_QS2, False, 512, ("ip", "l2")), ("qs2", _FORCED_QS2, False, 768, ("ip", "l2")),
    ("scan_bf16", {}, False, 1000, ("ip", "l2")),
    ("qsw", _FORCED, True, 1000, ("ip", "l2")), ("qsw", _FORCED, True, 1280, ("ip", "l2")),
]


def case_k(d, layout):
    """k of a case: 1, 10 and 64 rotate over the layouts and the widths, so that every kernel sees all three"""
    return (1, 10, 64)[(LAYOUTS.index(layout) + DIMS.index(d)) % 3]


def case_seed(d, layout):
    return 8 * d + LAYOUTS.index(layout)


def rounding_cases():
    """[(kernel, env, wide, metric, d, layout, k, n)]: every kernel x its metrics x every layout"""
    return [(kernel, env, wide, metric, d, layout, case_k(d, layout), N_ROWS)
            for kernel, env, wide, d, metrics in KERNELS for metric in metrics for layout in LAYOUTS]


# layout `apart` at d = 768 once more: two database splits with the merge, and a two-launch chunked scan with carried state
# (15 tiles of 128: launches of 8 and 7 -- the recorded plan of tests/golden/knn_bf16_plan.txt)
SPLIT_CASE = ("qs", {"LEMON_SPLITS": "2"}, False, 768, "apart", 64, N_ROWS)
CHUNK_CASE = ("qs", {"LEMON_CHUNK_MB": "0.01"}, False, 768, "apart", 10, N_ROWS)


def data_cases():
    """the distinct data sets behind all of the above: sorted [(metric, d, k, layout, n)]"""
    out = {(metric, d, k, layout, n) for _, _, _, metric, d, layout, k, n in rounding_cases()}
    for _, _, _, d, layout, k, n in (SPLIT_CASE, CHUNK_CASE):
        out |= {(metric, d, k, layout, n) for metric in ("ip", "l2")}
    return sorted(out)


def case_data(metric, d, k, layout, n=N_ROWS):
    return adversarial(metric, d, k, layout, case_seed(d, layout), n=n, nq=N_QUERIES)
