"""numpy restatement of lemon_amd/csrc/kmeans.hip's rules (test helper, no GPU): Lloyd's iteration with float64 (or, for the
fairness checks, float32) distances, float64 means rounded once to the centroid dtype, the deterministic empty-cluster
split, fixed niter.  Same initial rows as lemon_amd.kmeans (initial_rows / subsample_rows)."""
import numpy as np

EPS = 1.0 / 1024.0


def sqdist(x, c, dtype=np.float64):
    """[n, C] squared distances max(0, |x|^2 + |c|^2 - 2 <x, c>) evaluated in `dtype`."""
    x = np.asarray(x, dtype=dtype)
    c = np.asarray(c, dtype=dtype)
    d2 = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)
    return np.maximum(d2, 0)


def assign_ref(x, c, dtype=np.float64, chunk=8192):
    """(assign int64 [n], dist [n]) -- np.argmin returns the FIRST minimum: ties go to the lower index."""
    a = np.empty(len(x), np.int64)
    dist = np.empty(len(x), dtype)
    for s in range(0, len(x), chunk):
        d2 = sqdist(x[s:s + chunk], c, dtype)
        a[s:s + chunk] = d2.argmin(1)
        dist[s:s + chunk] = d2[np.arange(len(d2)), a[s:s + chunk]]
    return a, dist


def update_ref(x, a, c):
    """float64 means rounded once to c.dtype; a cluster without points keeps its centroid.  Returns (new c, count int64)."""
    C, d = c.shape
    count = np.bincount(a, minlength=C).astype(np.int64)
    order = np.argsort(a, kind="stable")
    xs = np.asarray(x, np.float64)[order]
    out = c.copy()
    starts = np.concatenate([[0], np.cumsum(count)])
    for k in range(C):
        if count[k]:
            out[k] = (xs[starts[k]:starts[k + 1]].sum(0) / count[k]).astype(c.dtype)
    return out, count


def split_ref(c, count):
    """In ascending index, every empty cluster takes half of the currently largest one (ties: lower index); the pair is
    perturbed symmetrically in the centroid dtype.  Returns new (c, count)."""
    c, count = c.copy(), count.copy()
    up, dn = c.dtype.type(1.0 + EPS), c.dtype.type(1.0 - EPS)
    even = (np.arange(c.shape[1]) % 2) == 0
    for e in range(len(count)):
        if count[e] != 0:
            continue
        donor = int(np.argmax(count))               # first maximum = lower index
        half = int(count[donor]) // 2
        if half == 0:
            break
        v = c[donor].copy()
        c[e] = np.where(even, v * up, v * dn)
        c[donor] = np.where(even, v * dn, v * up)
        count[e], count[donor] = half, count[donor] - half
    return c, count


def lloyd_ref(x, init, niter, dtype=np.float64, centroid_dtype=np.float32):
    """niter x (assign, update, split) + a last assign: (centroids, obj_hist float64 [niter], count, assign)."""
    c = np.asarray(init, centroid_dtype).copy()
    obj = np.zeros(niter, np.float64)
    count = np.zeros(len(c), np.int64)
    for it in range(niter):
        a, dist = assign_ref(x, c, dtype)
        obj[it] = dist.astype(np.float64).sum()
        c, count = update_ref(x, a, c)
        c, count = split_ref(c, count)
    a, _ = assign_ref(x, c, dtype)
    return c, obj, count, a


def planted(C=16, d=64, per=120, seed=0):
    """C unit-norm centres and `per` points around each with noise of norm below 1/8 of the smallest gap between two centres,
    plus one data row per centre to start from: every point is then closer to its own centre's start row (<= gap / 4) than to
    any other (>= 3 gap / 4), so float32 rounding cannot move a point across a boundary.  Returns (x float32, init rows, truth)."""
    rs = np.random.RandomState(seed)
    centres = rs.randn(C, d)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    gap = min(np.linalg.norm(centres[i] - centres[j]) for i in range(C) for j in range(i))
    truth = np.repeat(np.arange(C), per)
    noise = rs.randn(C * per, d)
    noise *= (rs.rand(C * per, 1) * 0.99 * gap / 8.0) / np.linalg.norm(noise, axis=1, keepdims=True)
    perm = rs.permutation(C * per)
    x = (centres[truth] + noise)[perm].astype(np.float32)
    truth = truth[perm]
    init_rows = np.array([int(np.flatnonzero(truth == k)[0]) for k in range(C)])
    return x, init_rows, truth


def label_disagreement_ref(I, k, db_label, q_label, drop_self=False, in_db=None):
    nq, kk = I.shape
    out = np.zeros(nq, np.float32)
    for i in range(nq):
        first = 1 if (drop_self and (in_db is None or in_db[i])) else 0
        bad = 0
        for s in range(k):
            j = I[i, first + s]
            same = 0 <= j < len(db_label) and q_label[i] >= 0 and db_label[j] == q_label[i]
            bad += not same
        out[i] = np.float32(bad) / np.float32(k)
    return out
