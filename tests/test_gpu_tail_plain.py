"""GPU: what a run_lemon run leaves in a directory against tests/tailfx.plain_tail -- the tail of a run in a straight line,
which shares no code with run_lemon's cell loop -- on that directory's own record: res.pkl is loaded, the three score columns
are dropped, and plain_tail runs on the frame with that directory's args.json as its namespace.  Single runs of every kind of
ablation (searched, d_1 zeroed, masked, the host formulas), of the host modes and of --skip_hparam_optim, and two cells of a
subset x ablation x knn_k sweep.  Comparison rules: frames with check_exact, every float of agg_results by its bits (NaN
included), the csv byte for byte, the same set of files; no tolerances.

Shape: synthetic:600 splits 480 / 60 / 60, --debug (validation and test rows), the 3 x 3 x 2 x 2 grid, knn_k 5."""
import argparse
import json
import os
import pathlib
import pickle

import numpy as np
import pytest

from tests import tailfx

pytestmark = pytest.mark.gpu

BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:600", "--clip_path", "random:tiny",
        "--hparam_grid", "small", "--debug"]
DEVICE = ["--hparam_search", "device", "--lbfgs_polish", "device"]
CSV = "know_val_labels_scores.csv"
SINGLES = {"none": ["--ablation", "none", *DEVICE], "d1": ["--ablation", "d1", *DEVICE], "tau_1_2": ["--ablation", "tau_1_2", *DEVICE],
           "multimodal_baseline": ["--ablation", "multimodal_baseline", *DEVICE], "only_gamma": ["--ablation", "only_gamma", *DEVICE],
           "none-host": ["--ablation", "none"], "none-skip": ["--ablation", "none", "--skip_hparam_optim"]}
CELLS = ["subset_val_set=10/ablation=d1/knn_k=1", "subset_val_set=-1/ablation=none/knn_k=5"]


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.int64)


def _same(a, b, path="agg_results"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for key in a:
            _same(a[key], b[key], f"{path}[{key!r}]")
    elif isinstance(a, (list, tuple, np.ndarray)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path
    elif isinstance(a, (float, np.floating)):
        assert isinstance(b, (float, np.floating)) and _bits(a) == _bits(b), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.fixture(scope="module")
def run_dir(hip, tmp_path_factory):
    """the directory a case is checked in, its run made once on first use"""
    from lemon_amd.run_lemon import main
    cache, done = str(tmp_path_factory.mktemp("tail_plain_cache")), {}

    def get(flags):
        if flags not in done:
            out = str(tmp_path_factory.mktemp("run"))
            assert main(["--output_dir", out, *BASE, "--embedding_cache", cache, *flags]) == 0
            done[flags] = out
        return done[flags]
    return get


def _assert_is_the_plain_tail(got_dir, tmp_path):
    import pandas as pd
    import torch
    got = pickle.load(open(os.path.join(got_dir, "res.pkl"), "rb"))
    args = argparse.Namespace(**json.load(open(os.path.join(got_dir, "args.json"))))
    scores = [c for c in got["df"].columns if c.startswith("know_val_labels_")]
    assert len(scores) == (0 if args.skip_hparam_optim else 3)
    want_dir = pathlib.Path(tmp_path / "plain")
    want_dir.mkdir()
    tailfx.plain_tail(args, got["df"].drop(columns=scores), want_dir, torch.device("cuda", torch.cuda.current_device()))
    want = pickle.load(open(want_dir / "res.pkl", "rb"))
    assert list(got) == list(want)
    pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
    assert got["df"]["D_n"].iloc[0].shape == (args.knn_k,)
    if not args.skip_hparam_optim:
        _same(got["agg_results"], want["agg_results"])
        assert open(os.path.join(got_dir, CSV), "rb").read() == open(want_dir / CSV, "rb").read()
    assert set(os.listdir(got_dir)) - {"args.json"} == set(os.listdir(want_dir))
    return got


@pytest.mark.parametrize("case", list(SINGLES))
def test_a_single_run_is_the_plain_tail_on_its_record(run_dir, tmp_path, case):
    got = _assert_is_the_plain_tail(run_dir(("--knn_k", "5", *SINGLES[case])), tmp_path)
    assert bool((got["df"].d_1 == 0).all()) == (case == "d1") and (got["df"].sset == "val").sum() == 60
    if case != "none-skip":
        agg = got["agg_results"]["know_val_labels"]
        assert ("selected_val" in agg) == (case != "only_gamma") and set(got["df"].sset.unique()) <= set(agg)


@pytest.mark.parametrize("cell", CELLS)
def test_a_cell_of_a_sweep_is_the_plain_tail_on_its_record(run_dir, tmp_path, cell):
    out = run_dir(("--subset_val_set_sweep", "-1,10", "--ablation_sweep", "none,d1", "--knn_k_sweep", "1,5", *DEVICE))
    got = _assert_is_the_plain_tail(os.path.join(out, cell), tmp_path)
    m, a, k = (level.split("=")[1] for level in cell.split("/"))
    assert (got["df"].sset == "val").sum() == (60 if m == "-1" else int(m)) and got["df"]["D_n"].iloc[0].shape == (int(k),)
    assert bool((got["df"].d_1 == 0).all()) == (a == "d1")
