"""The discrepancy sweep without a GPU: lemon_discrepancy_ks_host runs discrepancy_core.hpp -- the summation replay of
k_discrepancy_ks -- with the 64 lanes looped, on the oracle's neighbour lists at kmax = 63.  Every k of the list must give what
the oracle gives for that k alone (lib/baselines/discrepancy_baseline.py:164-242), the reference script's recorded scores on
the disc_* fixtures, and the same bits whatever else is in the list and however wide the cache is."""
import glob
import json
import os

import numpy as np
import pytest

from tests import discsweep as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NAMES = ("lemon_discrepancy_cache", "lemon_discrepancy_ks", "lemon_discrepancy_ks_host")


def test_surface():
    from lemon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def _assert_one_ulp(got, ref, what):
    """The twin sums the oracle's float32 distances in float64 in another order (lane-strided, then a shuffle tree) and rounds
    once to float32: the roundings of two float64 sums that differ by about pairs * 2^-53 relative agree to one float32 ulp."""
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN positions")
    ok = ~np.isnan(ref)
    err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
    ulp = np.spacing(np.abs(ref[ok]).astype(np.float32)).astype(np.float64)
    assert np.all(err <= ulp), (what, float((err / ulp).max()))


@pytest.mark.parametrize("d", ds.DIMS)
def test_host_twin_equals_the_oracle_at_every_k(oracle, d):
    nan_seen = short_seen = False
    for db in ds.databases(d):
        _, img_tr, txt_tr, _, _ = db
        for what, q_img, q_txt, is_train in ds.query_sets(db):
            short_seen |= bool((oracle.knn("ip", txt_tr, q_txt, 8)[1] == -1).any())
            for m in ds.METHODS:
                got = ds.host_sweep(oracle, m, img_tr, txt_tr, q_img, q_txt, ds.KS, is_train)
                for t, k in enumerate(ds.KS):
                    ref = ds.oracle_scores(oracle, m, img_tr, txt_tr, q_img, q_txt, k, is_train)
                    nan_seen |= bool(np.isnan(ref).any())
                    _assert_one_ulp(got[t], ref, f"{what} d={d} {m} k={k}")
    assert nan_seen and short_seen          # the empty mean and the lists that end in -1 were among the cases


FIXTURES = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(G, "disc_*.npz")))


@pytest.mark.parametrize("m", ["dis_x", "dis_y", "div_x", "div_y"])
def test_host_twin_on_the_reference_scripts_fixtures(oracle, m):
    assert m in FIXTURES
    fx = np.load(os.path.join(G, f"disc_{m}.npz"))
    argv = json.loads(str(fx["argv"]))
    k = int(argv[argv.index("--knn_k") + 1])
    ks = sorted({1, 2, k, k + 3, 30})
    for s in fx["ssets"]:
        s = str(s)
        q_img = oracle.normalize_rows(fx[f"{s}_q_img_raw"])
        got = ds.host_sweep(oracle, m, fx["db_img"], fx["db_txt"], q_img, fx[f"{s}_q_txt"], ks, s == "train")
        assert np.abs(got[ks.index(k)] - fx[f"{s}_pred_score"]).max() <= 2e-6, (m, s)


@pytest.mark.parametrize("d", [33, 36])
def test_a_k_does_not_depend_on_the_list_or_the_cache_pitch(oracle, d):
    for db in ds.databases(d):
        _, img_tr, txt_tr, _, _ = db
        for what, q_img, q_txt, is_train in ds.query_sets(db)[-2:]:
            for m in ds.METHODS:
                full = ds.host_sweep(oracle, m, img_tr, txt_tr, q_img, q_txt, ds.KS, is_train)
                wide = ds.host_sweep(oracle, m, img_tr, txt_tr, q_img, q_txt, ds.KS, is_train, kc=64)
                assert ds.same_bits(full, wide), (what, m, "cache pitch 64")
                for t, k in enumerate(ds.KS):
                    alone = ds.host_sweep(oracle, m, img_tr, txt_tr, q_img, q_txt, [k], is_train)      # cache pitch k + 1
                    assert ds.same_bits(alone[0], full[t]), (what, m, k)


@pytest.mark.parametrize("argv", [["--method_sweep", "dis_x,dis_z"], ["--method_sweep", ","], ["--method_sweep", ""],
                                  ["--knn_k_sweep", "1,5,64"], ["--knn_k_sweep", ""], ["--method_sweep", "all", "--knn_k", "64"]])
def test_cli_refuses_a_bad_sweep_before_anything_runs(argv, tmp_path, capsys):
    from lemon_amd.discrepancy_baseline import main
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        main(["--output_dir", str(out)] + argv)
    assert e.value.code == 2 and not out.exists()
    assert argv[0] in capsys.readouterr().err


def test_cli_sweep_axes():
    from lemon_amd.discrepancy_baseline import build_parser, sweep_axes
    parse = lambda *a: sweep_axes(build_parser().parse_args(["--output_dir", "o"] + list(a)))
    assert parse() is None and parse("--method", "div_y", "--knn_k", "7") is None
    assert parse("--method_sweep", "all", "--knn_k_sweep", "5,1,5") == (["dis_x", "dis_y", "div_x", "div_y"], [1, 5])
    assert parse("--method_sweep", "div_y,dis_x,div_y", "--knn_k", "7") == (["div_y", "dis_x"], [7])
    assert parse("--knn_k_sweep", "63,2", "--method", "dis_y") == (["dis_y"], [2, 63])


@pytest.mark.parametrize("ks", [[], [5, 5], [5, 2], [0, 3], [3, 64], ["a"], None])
def test_discrepancy_sweep_refuses_a_bad_list(ks):
    from lemon_amd.baselines import discrepancy_sweep
    with pytest.raises(ValueError):
        discrepancy_sweep(None, None, None, ks)


def test_discrepancy_sweep_refuses_bad_methods():
    from lemon_amd.baselines import discrepancy_cache, discrepancy_sweep
    for methods in ([], ["dis_z"]):
        with pytest.raises(ValueError):
            discrepancy_sweep(None, None, None, [1, 2], methods=methods)
    for kmax in (0, 64):
        with pytest.raises(ValueError):
            discrepancy_cache(None, kmax)
