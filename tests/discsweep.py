"""What the discrepancy-sweep tests share (tests/test_discrepancy_sweep_host.py on the CPU, tests/test_gpu_discrepancy_sweep.py
on the GPU): the shapes of tests/test_gpu_record_paths.py::test_discrepancy_pair_loop -- database texts as exact duplicates of
six prototypes and as jittered rows, nq in {1, 7, 64}, the train split's k + 1 search both ways -- plus a five-row database
(lists that end in -1) and a one-row database (the empty mean), and the host twin lemon_discrepancy_ks_host driven from the
oracle's neighbour lists."""
import ctypes

import numpy as np

from tests.synth import unit_rows

METHODS = ("dis_x", "dis_y", "div_x", "div_y")
KS = (1, 2, 5, 10, 15, 20, 30, 50, 63)                # the reference grid (experiments.py:141-177) and the limit
DIMS = (3, 33, 36, 100)                               # d % 4 != 0: every lane walks its rows; d % 4 == 0: the staged walk
NQS = (1, 7, 64)


def _texts(rng, n_tr, nq_max, d, C=6):
    proto = unit_rows(rng, C, d)
    lab_tr, lab_q = rng.integers(0, C, n_tr), rng.integers(0, C, nq_max)

    def jitter(x):
        y = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
        return np.ascontiguousarray(y / np.linalg.norm(y, axis=1, keepdims=True), dtype=np.float32)

    dup = (np.ascontiguousarray(proto[lab_tr]), np.ascontiguousarray(proto[lab_q]))
    return {"duplicates": dup, "jittered": (jitter(dup[0]), jitter(dup[1]))}


def databases(d):
    """[(name, img_tr, txt_tr, q_img_new [64, d], q_txt_new [64, d])] for one width"""
    rng = np.random.default_rng(8100 + d)
    out = []
    img_tr, q_img = unit_rows(rng, 200, d), unit_rows(rng, 64, d)
    for kind, (txt_tr, q_txt) in _texts(rng, 200, 64, d).items():
        out.append((f"n_tr=200 {kind}", img_tr, txt_tr, q_img, q_txt))
    for n_tr in (5, 1):
        out.append((f"n_tr={n_tr}", unit_rows(rng, n_tr, d), unit_rows(rng, n_tr, d), q_img, unit_rows(rng, 64, d)))
    return out


def query_sets(db):
    """[(what, q_img, q_txt, is_train)]: new queries, and the database's own first rows as the train split"""
    name, img_tr, txt_tr, q_img, q_txt = db
    out = []
    for nq in NQS:
        out.append((f"{name} nq={nq}", q_img[:nq], q_txt[:nq], False))
        if nq <= img_tr.shape[0]:
            out.append((f"{name} nq={nq} train", img_tr[:nq], txt_tr[:nq], True))
    return out


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def host_sweep(oracle, method, img_tr, txt_tr, q_img, q_txt, ks, is_train, kc=None):
    """lemon_discrepancy_ks_host on the oracle's lists: float32 [len(ks), nq]"""
    from lemon_amd import _lib
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    E, qv = (f32(img_tr), f32(q_img)) if method.endswith("_x") else (f32(txt_tr), f32(q_txt))
    ks = [int(k) for k in ks]
    kq = ks[-1] + int(bool(is_train))
    Im = np.ascontiguousarray(oracle.knn("ip", txt_tr, q_txt, kq)[1], dtype=np.int64)
    Ic = None
    if method.startswith("dis"):
        kc = kc or ks[-1] + 1
        Ic = np.ascontiguousarray(oracle.knn("ip", txt_tr, txt_tr, kc)[1], dtype=np.int64)
    nq = qv.shape[0]
    out = np.full((len(ks), nq), -7.0, np.float32)
    ks_c = (ctypes.c_int32 * len(ks))(*ks)
    _lib.check(_lib.load().lemon_discrepancy_ks_host(0 if method.startswith("dis") else 1, _vp(E), E.shape[0], E.shape[1], _vp(qv),
                                                     _vp(Im), nq, _vp(Ic), kc or 0, ks_c, len(ks), int(bool(is_train)), _vp(out)),
               "lemon_discrepancy_ks_host")
    return out


def oracle_scores(oracle, method, img_tr, txt_tr, q_img, q_txt, k, is_train):
    E, qv = (img_tr, q_img) if method.endswith("_x") else (txt_tr, q_txt)
    return oracle.discrepancy(method[:3], E, txt_tr, qv, q_txt, k, is_train)


def same_bits(a, b):
    """the same float32 bits wherever there is a number, NaN in the same places"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])
