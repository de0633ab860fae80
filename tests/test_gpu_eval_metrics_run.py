"""GPU: runs with --eval_metrics device against the host path on the same record.  run_lemon: what a single run and the two
cells of an ablation sweep leave in their directories against tests/tailfx.plain_tail (metrics.eval_metrics on the host) on
that directory's own record; discrepancy_baseline: a device-mode run against the host-mode run of the same flags.  Same files,
frames and csv exact, every key of agg_results equal by bits and Python type -- except AUROC / AUPRC, where the device value is
the exact (correctly rounded) one and sklearn's trapezoid lies within n 2^-52 of it.

Shape: synthetic:600 splits 480 / 60 / 60, --debug (validation and test rows), the 3 x 3 x 2 x 2 grid, knn_k 5."""
import argparse
import json
import os
import pathlib
import pickle

import numpy as np
import pytest

from tests import evalfx as fx
from tests import tailfx

pytestmark = pytest.mark.gpu

BASE = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", "synthetic:600", "--clip_path", "random:tiny", "--debug"]
LEMON = ["--hparam_grid", "small", "--hparam_search", "device", "--lbfgs_polish", "device", "--knn_k", "5", "--eval_metrics", "device"]
CSV = "know_val_labels_scores.csv"
CELLS = ["ablation=none", "ablation=d1"]


def _same_results(got, want, rows):
    """agg_results of one run: {sset: eval_metrics dict} beside the selected hyper-parameters"""
    assert list(got) == list(want)
    for key in want:
        if key in rows:
            fx.same_dict(got[key], want[key], auc_bound=rows[key] * 2.0 ** -52)
        else:
            fx.same_value(got[key], want[key], key)


@pytest.fixture(scope="module")
def cache(hip, tmp_path_factory):
    return str(tmp_path_factory.mktemp("eval_run_cache"))


def _assert_is_the_plain_tail(got_dir, tmp_path):
    import pandas as pd
    import torch
    got = pickle.load(open(os.path.join(got_dir, "res.pkl"), "rb"))
    args = argparse.Namespace(**json.load(open(os.path.join(got_dir, "args.json"))))
    assert args.eval_metrics == "device"
    scores = [c for c in got["df"].columns if c.startswith("know_val_labels_")]
    want_dir = pathlib.Path(tmp_path / "plain")
    want_dir.mkdir()
    tailfx.plain_tail(args, got["df"].drop(columns=scores), want_dir, torch.device("cuda", torch.cuda.current_device()))
    want = pickle.load(open(want_dir / "res.pkl", "rb"))
    assert list(got) == list(want)
    pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
    rows = got["df"].sset.value_counts().to_dict()
    assert set(rows) == {"val", "test"} and list(got["agg_results"]) == ["know_val_labels"]
    _same_results(got["agg_results"]["know_val_labels"], want["agg_results"]["know_val_labels"], rows)
    assert open(os.path.join(got_dir, CSV), "rb").read() == open(want_dir / CSV, "rb").read()
    assert set(os.listdir(got_dir)) - {"args.json"} == set(os.listdir(want_dir))


def test_a_single_run_is_the_plain_tail_on_its_record(cache, tmp_path):
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "run")
    assert main(["--output_dir", out, *BASE, *LEMON, "--embedding_cache", cache, "--ablation", "none"]) == 0
    _assert_is_the_plain_tail(out, tmp_path)


def test_the_cells_of_a_sweep_are_the_plain_tail_on_their_records(cache, tmp_path):
    from lemon_amd.run_lemon import main
    out = str(tmp_path / "sweep")
    assert main(["--output_dir", out, *BASE, *LEMON, "--embedding_cache", cache, "--ablation_sweep", "none,d1"]) == 0
    cells = json.load(open(os.path.join(out, "cell_sweep.json")))["cells"]
    assert [c["path"] for c in cells] == CELLS and all(c["status"] == "ok" for c in cells)
    for cell in CELLS:
        where = tmp_path / cell.replace("=", "_")
        where.mkdir()
        _assert_is_the_plain_tail(os.path.join(out, cell), where)


def test_a_discrepancy_baseline_run_equals_its_host_mode_run(cache, tmp_path):
    import pandas as pd
    from lemon_amd.discrepancy_baseline import main
    runs = {}
    for mode in ("host", "device"):
        out = str(tmp_path / mode)
        assert main(["--output_dir", out, *BASE, "--embedding_cache", cache, "--method", "div_x", "--knn_k", "5",
                     "--eval_metrics", mode]) == 0
        runs[mode] = out
    got, want = (pickle.load(open(os.path.join(runs[mode], "res.pkl"), "rb")) for mode in ("device", "host"))
    pd.testing.assert_frame_equal(got["df"], want["df"], check_exact=True)
    rows = got["df"].sset.value_counts().to_dict()
    _same_results(got["agg_results"], want["agg_results"], rows)
    assert set(got["agg_results"]) == {"val", "test"}
    assert open(os.path.join(runs["device"], "scores.csv"), "rb").read() == open(os.path.join(runs["host"], "scores.csv"), "rb").read()
    assert set(os.listdir(runs["device"])) == set(os.listdir(runs["host"]))


def test_without_the_flag_nothing_calls_the_device_form(cache, tmp_path, monkeypatch):
    from lemon_amd import ops
    from lemon_amd.discrepancy_baseline import main
    monkeypatch.setattr(ops, "eval_metrics", lambda *a, **k: pytest.fail("ops.eval_metrics called in host mode"))
    assert main(["--output_dir", str(tmp_path / "host"), *BASE, "--embedding_cache", cache, "--method", "dis_y", "--knn_k", "5"]) == 0
    assert np.isfinite(pickle.load(open(tmp_path / "host" / "res.pkl", "rb"))["agg_results"]["val"]["AUROC"])
