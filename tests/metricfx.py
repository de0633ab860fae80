"""Fixtures of the metric sweep tests (CPU and GPU): embedding families on which the euclidean list derived from a cosine list
is certified everywhere (random unit rows, clusters with 0.01 noise), nowhere (exact duplicates, clusters with 1e-4 noise) or
somewhere (a database that is not normalised), and the host twin lemon_l2_from_ip_host driven from the oracle's IP search."""
import ctypes

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def unit_rows(oracle, n, d, seed):
    return oracle.normalize_rows(np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32))


def clustered(oracle, n, d, seed, noise, protos=16):
    """`protos` unit prototypes, every row one of them + a randn vector of expected length `noise` (noise / sqrt(d) a
    coordinate), normalised: returns (rows, prototype of each row).  At 0.01 the members of a cluster are about 1e-4 apart in
    cosine distance and the gaps between neighbours come down to the last bits, where the norms' own last bits reorder them;
    at 1e-4 whole clusters tie."""
    rng = np.random.default_rng(seed)
    P = oracle.normalize_rows(rng.standard_normal((protos, d)).astype(np.float32))
    which = rng.integers(0, protos, n)
    return oracle.normalize_rows(P[which] + np.float32(noise / np.sqrt(d)) * rng.standard_normal((n, d)).astype(np.float32)), which


def duplicates(oracle, n, d, seed, distinct=16):
    """`distinct` unit rows tiled to n: every neighbour list of depth <= n / distinct is one tie"""
    base = unit_rows(oracle, distinct, d, seed)
    return np.ascontiguousarray(base[np.arange(n) % distinct])


def family(oracle, name, n, nq, d, seed):
    """(X [n, d], Q [nq, d]) of a named family; the queries are fresh draws of the same family (same prototypes)"""
    if name == "random":
        return unit_rows(oracle, n, d, seed), unit_rows(oracle, nq, d, seed + 1000)
    if name in ("clustered", "tight"):
        A, _ = clustered(oracle, n + nq, d, seed, 0.01 if name == "clustered" else 1e-4)
        return np.ascontiguousarray(A[:n]), np.ascontiguousarray(A[n:])
    if name == "duplicates":
        A = duplicates(oracle, n + nq, d, seed)
        return np.ascontiguousarray(A[:n]), np.ascontiguousarray(A[n:])
    if name == "spread":                                   # not normalised: norms between 1 and 2, squared norms 1 .. 4
        rng = np.random.default_rng(seed + 7)
        X = unit_rows(oracle, n, d, seed) * rng.uniform(1.0, 2.0, (n, 1)).astype(np.float32)
        return np.ascontiguousarray(X.astype(np.float32)), unit_rows(oracle, nq, d, seed + 1000)
    raise ValueError(name)


def norms(oracle, A):
    return np.array([oracle.dot_chain(r, r) for r in A], dtype=np.float32)


def xx_min_of(xx):
    if xx.size == 0:
        return FLT_MAX
    return np.float32(xx.min()) if np.isfinite(xx).all() else np.float32(np.nan)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_derive(qq, xx, Dip, Iip, k, xx_min=None):
    """lemon_l2_from_ip_host: (D [nq, k] f32, I [nq, k] i64, cert [nq] bool)"""
    from lemon_amd import _lib
    qq, xx = np.ascontiguousarray(qq, np.float32), np.ascontiguousarray(xx, np.float32)
    Dip, Iip = np.ascontiguousarray(Dip, np.float32), np.ascontiguousarray(Iip, np.int64)
    nq, kd = Dip.shape
    D = np.full((nq, k), np.float32(-7.0), np.float32)
    I = np.full((nq, k), -7, np.int64)
    cert = np.full(nq, 7, np.uint8)
    xm = xx_min_of(xx) if xx_min is None else np.float32(xx_min)
    _lib.check(_lib.load().lemon_l2_from_ip_host(_vp(qq), _vp(xx), xx.shape[0], ctypes.c_float(float(xm)), _vp(Dip), _vp(Iip), nq, kd,
                                                 k, _vp(D), _vp(I), _vp(cert)), "lemon_l2_from_ip_host")
    assert set(np.unique(cert).tolist()) <= {0, 1}
    return D, I, cert.astype(bool)


def oracle_derive(oracle, X, Q, kd, k):
    """the host twin on the oracle's IP list at depth kd: (D, I, cert, I_ip)"""
    Dip, Iip = oracle.knn("ip", X, Q, kd)
    D, I, cert = host_derive(norms(oracle, Q), norms(oracle, X), Dip, Iip, k)
    return D, I, cert, Iip


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
