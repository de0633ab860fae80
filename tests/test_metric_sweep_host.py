"""The metric sweep without a GPU: lemon_l2_from_ip_host runs csrc/l2_from_ip_core.hpp -- the derivation k_l2_from_ip makes
with a lane per candidate -- on the oracle's IP lists.  Wherever it certifies a row, that row must be the oracle's L2 list bit
for bit; the families say where it must certify (random unit rows, loose clusters), where it must not (duplicates, tight
clusters, a NaN query) and that a pass-through of the cosine neighbours would be wrong (loose clusters)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import metricfx as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lemon_index_l2_from_ip", "lemon_l2_from_ip_host", "lemon_neighbors_metrics")
NQ = 24


def test_surface():
    from lemon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + "(" in hdr and _lib.EXPORTS.count(name) == 1 and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    from lemon_amd import build
    assert "metric_sweep.hip" in build.SOURCES and "l2_from_ip_core.hpp" in build.HEADERS


@functools.lru_cache(maxsize=None)
def _case(oracle, name, n, d):
    X, Q = fx.family(oracle, name, n, NQ, d, seed=n + d)
    return X, Q, fx.norms(oracle, X), fx.norms(oracle, Q)


@functools.lru_cache(maxsize=None)
def _lists(oracle, name, n, d, metric, k):
    X, Q, _, _ = _case(oracle, name, n, d)
    return oracle.knn(metric, X, Q, k)


def _derive(oracle, name, n, d, kd, k):
    _, _, xx, qq = _case(oracle, name, n, d)
    Dip, Iip = _lists(oracle, name, n, d, "ip", kd)
    return fx.host_derive(qq, xx, Dip, Iip, k)


def _assert_certified_rows_exact(oracle, name, n, d, kd, k):
    D, I, cert = _derive(oracle, name, n, d, kd, k)
    Dl, Il = _lists(oracle, name, n, d, "l2", k)
    assert fx.same_bits(D[cert], Dl[cert]) and np.array_equal(I[cert], Il[cert]), (name, n, d, kd, k)
    return D, I, cert


@pytest.mark.parametrize("d", [64, 67])
@pytest.mark.parametrize("n", [40, 55, 64, 2048])
def test_certified_rows_equal_the_oracle(oracle, n, d):
    seen = 0
    for name in ("random", "clustered"):
        for kd in (3, 5, 55, 64):
            for k in (1, 2, 6, 51, 64):
                if k > kd:
                    continue
                D, I, cert = _assert_certified_rows_exact(oracle, name, n, d, kd, k)
                seen += int(cert.sum())
                if n < kd:                                   # the last slot is padding, the list holds the whole DB: certified
                    assert cert.all(), (name, n, d, kd, k)
                    assert (I[:, n:] == -1).all() and (D[:, n:] == fx.FLT_MAX).all()
                assert (I[:, :min(n, k)] >= 0).all()
    assert seen > 0


@pytest.mark.parametrize("d", [64, 67])
def test_random_unit_rows_are_certified_at_a_margin_of_one(oracle, d):
    for k, kd in ((1, 2), (2, 3), (6, 7), (51, 52), (51, 55), (63, 64)):
        _, _, cert = _assert_certified_rows_exact(oracle, "random", 2048, d, kd, k)
        assert cert.all(), (d, k, kd, int(cert.sum()))


def test_loose_clusters_are_certified_and_are_not_the_cosine_prefix(oracle):
    """16 prototypes + 0.01 randn: the norms differ in the last bits, so the L2 order is NOT the IP order -- handing the cosine
    neighbours through would be wrong in most rows -- and four extra neighbours certify every row"""
    k, kd = 51, 55
    D, I, cert = _assert_certified_rows_exact(oracle, "clustered", 2048, 64, kd, k)
    assert cert.all()
    Iip = _lists(oracle, "clustered", 2048, 64, "ip", kd)[1]
    differs = (I != Iip[:, :k]).any(axis=1)
    assert differs.sum() * 2 > NQ, int(differs.sum())


@pytest.mark.parametrize("name", ["duplicates", "tight"])
def test_ties_are_not_certified(oracle, name):
    for k, kd in ((1, 5), (6, 10), (51, 55), (51, 64)):
        _, _, cert = _assert_certified_rows_exact(oracle, name, 2048, 64, kd, k)
        assert not cert.any(), (name, k, kd, int(cert.sum()))


def test_a_database_that_is_not_normalised(oracle):
    """norms between 1 and 2: the L2 order has little to do with the IP order and almost nothing is certified unless the list
    holds the whole database (n = 40) or is much deeper than k"""
    some = 0
    for n in (40, 2048):
        for d in (64, 67):
            for k, kd in ((1, 5), (1, 64), (6, 10), (6, 64), (51, 55), (51, 64)):
                _, _, cert = _assert_certified_rows_exact(oracle, "spread", n, d, kd, k)
                some += int(cert.sum()) if n == 2048 else 0
    assert some > 0                                          # (so "whatever is certified" is not an empty statement)


def test_a_nan_query_row_is_not_certified_and_touches_no_other_row(oracle):
    X, Q, xx, qq = _case(oracle, "random", 2048, 64)
    for n_db in (2048, 40):                                  # a list without padding, and one that holds the whole DB
        Xs, xs = X[:n_db], xx[:n_db]
        Qn = Q.copy()
        Qn[5, 3] = np.nan
        qn = fx.norms(oracle, Qn)
        ref = fx.host_derive(qq, xs, *oracle.knn("ip", Xs, Q, 55), 51)
        got = fx.host_derive(qn, xs, *oracle.knn("ip", Xs, Qn, 55), 51)
        keep = np.arange(NQ) != 5
        assert not got[2][5] and ref[2].all()
        for a, b in zip(got, ref):
            assert fx.same_bits(a[keep], b[keep])


def test_a_norm_that_is_not_finite_certifies_nothing(oracle):
    """a DB row with a NaN in it scores NaN: the IP search never selects it, the L2 expression gives it distance 0"""
    X, Q, xx, qq = _case(oracle, "random", 2048, 64)
    bad = xx.copy()
    bad[100] = np.nan
    Dip, Iip = _lists(oracle, "random", 2048, 64, "ip", 55)
    assert not fx.host_derive(qq, bad, Dip, Iip, 51)[2].any()
    assert not fx.host_derive(qq[:4], xx[:40], *oracle.knn("ip", X[:40], Q[:4], 55), 51, xx_min=np.inf)[2].any()


def test_equality_with_the_bound_is_not_certified():
    """D_(k-1) == B: a row nobody has seen could tie and win on its id"""
    qq = np.array([1.0], np.float32)
    xx = np.ones(8, np.float32)
    Dip = np.array([[0.75, 0.5, 0.5]], np.float32)
    Iip = np.array([[4, 2, 6]], np.int64)
    D, I, cert = fx.host_derive(qq, xx, Dip, Iip, 2)
    assert I.tolist() == [[4, 2]] and D.tolist() == [[0.5, 1.0]] and not cert[0]
    D, I, cert = fx.host_derive(qq, xx, Dip, Iip, 1)
    assert I.tolist() == [[4]] and cert[0]
    xx[4] = 2.0                                              # the best score has the larger norm: the order turns round
    D, I, cert = fx.host_derive(qq, xx, np.array([[0.75, 0.5, 0.25]], np.float32), Iip, 2)
    assert I.tolist() == [[2, 4]] and D.tolist() == [[1.0, 1.5]] and not cert[0]      # B = 1.5
    D, I, cert = fx.host_derive(qq, xx, np.array([[0.75, 0.5, 0.125]], np.float32), Iip, 2)
    assert I.tolist() == [[2, 4]] and cert[0]                                          # B = 1.75


def test_refusals_write_nothing():
    from lemon_amd import _lib
    lib = _lib.load()
    qq, xx = np.ones(2, np.float32), np.ones(8, np.float32)
    Dip, Iip = np.zeros((2, 4), np.float32), np.zeros((2, 4), np.int64)
    for kd, k in ((4, 0), (4, 5), (65, 1)):
        D, I, c = np.full((2, 64), -7, np.float32), np.full((2, 64), -7, np.int64), np.full(2, 7, np.uint8)
        rc = lib.lemon_l2_from_ip_host(fx._vp(qq), fx._vp(xx), 8, 1.0, fx._vp(Dip), fx._vp(Iip), 2, kd, k, fx._vp(D), fx._vp(I),
                                       fx._vp(c))
        assert rc != 0 and (D == -7).all() and (I == -7).all() and (c == 7).all(), (kd, k)
    assert lib.lemon_l2_from_ip_host(None, fx._vp(xx), 8, 1.0, fx._vp(Dip), fx._vp(Iip), 2, 4, 2, None, None, None) != 0


def test_parse_dist_sweep():
    from lemon_amd.run_lemon import parse_dist_sweep
    assert parse_dist_sweep("cosine,euclidean") == ["cosine", "euclidean"]
    assert parse_dist_sweep(" euclidean , cosine,euclidean,") == ["euclidean", "cosine"]          # order kept, de-duplicated
    assert parse_dist_sweep("euclidean") == ["euclidean"] and parse_dist_sweep("cosine,cosine") == ["cosine"]
    for bad in ("", ",", " , ", "l2", "cosine,manhattan", "cosine;euclidean", "Cosine"):
        with pytest.raises(ValueError):
            parse_dist_sweep(bad)


@pytest.mark.parametrize("argv", [["--dist_type_sweep", ""], ["--dist_type_sweep", ","], ["--dist_type_sweep", "cosine,l1"],
                                  ["--dist_type_sweep", "cosine,euclidean", "--dist_sweep_margin", "-1"]])
def test_cli_refuses_a_bad_sweep_before_anything_runs(argv, tmp_path, capsys):
    from lemon_amd.run_lemon import main
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        main(["--output_dir", str(out)] + argv)
    assert e.value.code == 2 and not out.exists()
    assert argv[-2] in capsys.readouterr().err


def test_cli_defaults_leave_the_sweep_off():
    from lemon_amd.run_lemon import build_parser
    a = build_parser().parse_args(["--output_dir", "o", "--dist_type", "euclidean"])
    assert a.dist_type_sweep is None and a.dist_sweep_margin == 4 and a.dist_type == "euclidean"


def test_a_sweep_db_takes_both_metrics_once_each():
    """(refused before any device is touched)"""
    from lemon_amd.neighbors import LemonDB
    for bad in (("cosine",), ("cosine", "cosine"), ("cosine", "euclidean", "cosine"), ()):
        with pytest.raises(ValueError):
            LemonDB(None, None, bad)
    with pytest.raises(ValueError):
        LemonDB(None, None, ("cosine", "manhattan"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_core_header_alone(tmp_path, flags):
    """csrc/l2_from_ip_core.hpp driven by a stand-alone program against a sort of the whole database"""
    exe = str(tmp_path / "l2_from_ip_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags +
                          [os.path.join(ROOT, "tests", "native", "l2_from_ip_fuzz.cpp"), "-o", exe])
    for seed in ("1", "20261020"):
        r = subprocess.run([exe, "4000", seed], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "l2_from_ip_fuzz: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
