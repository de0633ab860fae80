"""Case builders for the k-means edge tests (tests/test_gpu_kmeans_edges.py on the device, tests/test_kmeans_edges_host.py for
the fairness of the same inputs on the CPU).  numpy only: importable without a GPU.  The references are tests/kmeans_ref.py."""
import numpy as np

from tests import kmeans_ref as R

# ---- 1. assign at tile, slice and panel edges -------------------------------------------------------------------------
# lemon_amd/csrc/kmeans.hip: a workgroup owns 128 points, centroids stream in 128-row tiles, k in slices of 32, 16384 is the
# largest C (128 tiles)
ASSIGN_N = (1, 127, 128, 129, 257)
ASSIGN_C = (1, 2, 127, 128, 129, 255, 256, 257, 16384)
ASSIGN_D = (4, 8, 28, 32, 36, 64, 68, 1020, 1024)
ASSIGN_REQUIRED = [(129, 129, 4), (257, 257, 4), (128, 129, 28), (129, 257, 28), (127, 129, 32), (257, 257, 32),   # one k-slice, several tiles
                   (129, 129, 1024), (129, 16384, 4), (129, 16384, 36)]


def assign_shapes():
    """(n, C, d): the required combinations, then three of every four (C, d) pairs below the largest C with n cycling
    through its values."""
    shapes = list(ASSIGN_REQUIRED)
    have = {(C, d) for _, C, d in shapes}
    for i, C in enumerate(ASSIGN_C[:-1]):
        for j, d in enumerate(ASSIGN_D):
            if (i + j) % 4 != 3 and (C, d) not in have:
                shapes.append((ASSIGN_N[(2 * i + j) % len(ASSIGN_N)], C, d))
    return shapes


def unit_rows(rs, n, d):
    x = rs.randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)


def assign_case(n, C, d, unit_centroids):
    """Unit-norm points; centroids of unit norm or with row scales in [0.2, 3] (tests/test_gpu_kmeans.py::_case).  From
    C = 8 on two exact duplicate pairs, (5, C - 1) with the lower index in the upper lane half of the kernel's merge and
    (0, C / 2) with it in the lower one, and up to three points equal to a centroid."""
    rs = np.random.RandomState(1000003 * n + 1009 * C + 2 * d + int(unit_centroids))
    x = unit_rows(rs, n, d)
    c = unit_rows(rs, C, d) if unit_centroids else (rs.randn(C, d) * rs.uniform(0.2, 3.0, (C, 1))).astype(np.float32)
    if C >= 8:
        c[C - 1] = c[5]
        c[C // 2] = c[0]
    for j in range(min(n, 3)):
        x[j] = c[(j * 7) % C]
    return x, c


def chain_bound(d, xnorm, cnorm):
    """|float32 chain distance - exact distance| <= (d + 3) 2^-24 (|x| + |c|)^2 (derived in tests/test_gpu_kmeans.py)."""
    return (d + 3) * 2.0 ** -24 * (xnorm + cnorm) ** 2


def check_against_float64(x, c, a, dist=None):
    """The checks of an assignment `a` (and its distances) against float64: the distance of the chosen centroid within the
    chain bound; where `a` is not the float64 arg-min the float64 gap is at most twice that bound (the two distances
    compared), at most n // 1000 such points.  Returns their number."""
    n, d = x.shape
    d64 = R.sqdist(x, c)
    a64 = d64.argmin(1)
    a = np.asarray(a, np.int64)
    rows = np.arange(n)
    xn = np.linalg.norm(x.astype(np.float64), axis=1)
    cn = np.linalg.norm(c.astype(np.float64), axis=1)
    if dist is not None:
        err = np.abs(np.asarray(dist, np.float64) - d64[rows, a])
        bound = chain_bound(d, xn, cn[a])
        assert (err <= bound).all(), (float((err / bound).max()), int((err > bound).sum()))
    diff = np.flatnonzero(a != a64)
    assert len(diff) <= n // 1000, (len(diff), n)
    if len(diff):
        gap = d64[diff, a[diff]] - d64[diff, a64[diff]]
        cap = 2.0 * chain_bound(d, xn[diff], np.maximum(cn[a[diff]], cn[a64[diff]]))
        assert (gap <= cap).all(), (gap, cap)
    return len(diff)


# ---- 2. tie table ---------------------------------------------------------------------------------------------------
# (source row, row that receives the copy).  Lane l of the kernel holds the centroid rows with j % 8 < 4, lane l + 32 those
# with j % 8 >= 4; wave-level groups are 32 rows, tiles 128 rows.
TIE_C = 300
TIE_PAIRS = [(4, 8), (3, 4), (5, 6), (7, 128), (132, 257), (0, 127), (12, 9)]


def lane_half(j):
    return int(j % 8 >= 4)


def tie_case(pair, d, n_random=200):
    """(x [1 + n_random, d], c [300, d], lo, hi): c[pair[1]] = c[pair[0]] and no other duplicate; x[0] is that row, half of
    the others are drawn around it (so that the pair is what many points are nearest to), half over the whole sphere."""
    src, dst = pair
    rs = np.random.RandomState(97 * src + dst + 7 * d)
    c = unit_rows(rs, TIE_C, d)
    c[dst] = c[src]
    near = c[src][None, :] + 0.05 * rs.randn(n_random // 2, d).astype(np.float32)
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    x = np.concatenate([c[src][None, :], near.astype(np.float32), unit_rows(rs, n_random - n_random // 2, d)])
    return np.ascontiguousarray(x, np.float32), c, min(pair), max(pair)


# ---- 3. non-finite rows ----------------------------------------------------------------------------------------------
def nonfinite_case(centroid_nan):
    """n = 130, C = 5, d = 8: a row with a NaN, one with +Inf (at a coordinate where centroid 0 is negative and a later one
    positive, so that both signs of the infinite product occur), one all-zero; optionally a NaN in centroid 3."""
    rs = np.random.RandomState(130)
    x, c = unit_rows(rs, 130, 8), unit_rows(rs, 5, 8)
    c[0, 2], c[1, 2] = -abs(c[0, 2]), abs(c[1, 2])
    x[0, 5] = np.nan
    x[1, 2] = np.inf
    x[2] = 0.0
    if centroid_nan:
        c[3, 1] = np.nan
    return x, c


# ---- 4. update with crafted assignments ----------------------------------------------------------------------------------
UPDATE_SIZES = (0, 1, 2, 3, 4, 5, 8, 9)      # the 4-wide loop of k_km_means and its tail
OUT_OF_RANGE = (-1, None, 2 ** 31 - 1)       # None: C itself
#               (n, C, d, pattern)
UPDATE_CASES = [(5000, 1, 36, "all"), (1, 1, 4, "all"), (300, 1, 4, "none"), (300, 1, 132, "some"),
                (5000, 255, 36, "sizes"), (300, 255, 128, "sizes"), (300, 256, 132, "sizes"), (300, 256, 4, "all"),
                (300, 257, 1024, "sizes"), (300, 257, 4, "some"), (300, 16384, 4, "sizes"), (300, 16384, 132, "sizes"),
                (300, 16384, 36, "all"), (300, 16384, 128, "none")]


def crafted_assign(n, C, pattern, seed=0):
    """int32 [n] built by hand (never taken from an assign):
    all    every point in one cluster (C / 2)
    none   every point outside [0, C): -1, C and 2^31 - 1 in turn
    some   thirty out-of-range entries, the rest in cluster C - 1
    sizes  clusters of exactly 0, 1, 2, 3, 4, 5, 8 and 9 points spread from cluster 0 to cluster C - 1, thirty out-of-range
           entries, the rest in one large cluster; everything else stays empty"""
    rs = np.random.RandomState(seed + n + C)
    oor = [C if v is None else v for v in OUT_OF_RANGE]
    if pattern == "all":
        return np.full(n, C // 2, np.int32)
    if pattern == "none":
        return np.array([oor[i % 3] for i in range(n)], np.int32)
    a = [oor[i % 3] for i in range(30)]
    if pattern == "sizes":
        ids = np.linspace(0, C - 1, len(UPDATE_SIZES)).astype(int)
        sizes = (1, 4, 0, 8, 3, 5, 2, 9)                     # cluster 0 has one point, cluster C - 1 nine
        assert len(set(ids.tolist())) == len(sizes) and sorted(sizes) == list(UPDATE_SIZES)
        for k, s in zip(ids, sizes):
            a += [int(k)] * s
        a += [int(ids[2]) + 1] * (n - len(a))                # the large cluster sits right behind the empty one
    else:
        assert pattern == "some", pattern
        a += [C - 1] * (n - len(a))
    a = np.array(a, np.int64)
    assert len(a) == n
    return a[rs.permutation(n)].astype(np.int32)


def update_expected(x, a, c):
    """(centroids float32 with the float64 mean of every non-empty cluster, count int64): out-of-range points count nowhere."""
    ok = (a >= 0) & (a < len(c))
    return R.update_ref(x[ok], a[ok].astype(np.int64), c)


# ---- 5. objective -----------------------------------------------------------------------------------------------------
OBJ_N = (1, 1023, 1024, 1025, 5000)          # k_km_obj: one block of 1024 threads


# ---- 6. split at reduction edges ---------------------------------------------------------------------------------------
# k_km_split: one block of 1024 threads = 16 waves, strided scan over C, dynamic LDS above 48 KiB from C = 12257
SPLIT_C = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 12288, 16384)
SPLIT_PATTERNS = ("random", "equal", "giant", "zero_one", "full")


def split_cases():
    """(C, d, pattern): every pattern at every C with d alternating between 4 and 36, and d = 1024 up to C = 4097."""
    cases = []
    for i, C in enumerate(SPLIT_C):
        for j, p in enumerate(SPLIT_PATTERNS):
            cases.append((C, (4, 36)[(i + j) % 2], p))
    cases += [(1, 1024, "giant"), (65, 1024, "equal"), (1025, 1024, "random"), (4097, 1024, "equal"), (4097, 1024, "giant")]
    return cases


def split_counts(C, pattern):
    """random    1..49 with 10 % zeros
    equal     every non-empty count is 5 and half of the clusters are empty: the tie spans every wave and every stride, the
              lowest index donates first, and the counts fall from 5 to 3 | 2 to 2 | 1, so later donors walk upward
    giant     one cluster of 5000 (an odd number of halvings away from 1), all others empty: a halving cascade
    zero_one  0 or 1 only: the first empty cluster finds nothing to halve, nothing may change
    full      no empties"""
    rs = np.random.RandomState(31 * C + len(pattern))
    if pattern == "random":
        count = rs.randint(1, 50, C)
        count[rs.rand(C) < 0.1] = 0
    elif pattern == "equal":
        count = np.where(rs.rand(C) < 0.5, 0, 5)
    elif pattern == "giant":
        count = np.zeros(C, int)
        count[(2 * C) // 3] = 5000
    elif pattern == "zero_one":
        count = (rs.rand(C) < 0.5).astype(int)
        count[C // 2] = 0
    else:
        assert pattern == "full", pattern
        count = rs.randint(1, 50, C)
    return count.astype(np.int64)


def split_case(C, d, pattern):
    rs = np.random.RandomState(C + d)
    return rs.randn(C, d).astype(np.float32), split_counts(C, pattern)


# ---- 7. train with splits inside the loop -------------------------------------------------------------------------------
#               (C, d, per, ndup)
TRAIN_CASES = [(12, 36, 40, 2), (16, 64, 120, 3)]
TRAIN_NITER = 8


def train_case(C, d, per, ndup):
    """kmeans_ref.planted with the start rows of clusters C - 1 - j replaced by those of clusters j (j < ndup): the higher
    index of every duplicate pair is empty after the first assign, so the first iteration splits."""
    x, rows, _ = R.planted(C, d, per)
    rows = rows.copy()
    for j in range(ndup):
        rows[C - 1 - j] = rows[j]
    return x, rows


def train_bound(d):
    """2 (d + 3) 2^-24 2.4^2: the chain's rounding bound for the difference of two distances, norms below 1.2."""
    return 2.0 * (d + 3) * 2.0 ** -24 * 2.4 ** 2


def lloyd_trace(x, init, niter, dtype=np.float64):
    """kmeans_ref.lloyd_ref with a record per iteration: empties after the update, assignments changed against the previous
    iteration, and the smallest gap between a point's nearest centroid and the nearest one whose row is not bitwise the
    same (0 would be an exact tie between different rows).  Returns (lloyd_ref's tuple, records)."""
    c = np.asarray(init, np.float32).copy()
    obj = np.zeros(niter, np.float64)
    prev, trace = None, []
    for it in range(niter + 1):
        d2 = R.sqdist(x, c, dtype)
        a = d2.argmin(1)
        best = d2[np.arange(len(x)), a]
        same = (c[a][:, None, :].view(np.int32) == c[None, :, :].view(np.int32)).all(2)      # [n, C]
        gap = float((np.where(same, np.inf, d2) - best[:, None]).min()) if not same.all() else np.inf
        if it == niter:
            trace.append(dict(empties=None, changed=int((a != prev).sum()), gap=gap))
            break
        obj[it] = best.astype(np.float64).sum()
        c, count = R.update_ref(x, a, c)
        trace.append(dict(empties=int((count == 0).sum()), changed=len(x) if prev is None else int((a != prev).sum()), gap=gap))
        c, count = R.split_ref(c, count)
        prev = a
    return (c, obj, count, a), trace
