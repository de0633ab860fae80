"""Host side of the knn_k sweep (no GPU): the --knn_k_sweep flag and its refusals, the selection rule, prefix_record on CPU
tensors, and the new names in the header, the binding and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# run_lemon.py:35-57 of the reference: every flag's default
REFERENCE_DEFAULTS = dict(exp_name=None, dataset="cifar100", noise_type="real", noise_level=0.4, dist_type="cosine",
                          normalize_d1=False, clip_model="huggingface_clip", knn_k=5, batch_size=128, seed=0, data_seed=0,
                          compr_dataset_size_limit=50000, ablation="none", use_discrete_for_text=False, real_dataset=False,
                          custom_cifar_prompt=None, subset_val_set=-1, debug=False, skip_train=False, skip_hparam_optim=False)


def test_sweep_list_is_sorted_and_deduplicated():
    from lemon_amd.run_lemon import parse_k_sweep
    assert parse_k_sweep("1,2,5,10,15,20,30,50") == [1, 2, 5, 10, 15, 20, 30, 50]
    assert parse_k_sweep("10, 1,5,5 ,1") == [1, 5, 10]
    assert parse_k_sweep("63") == [63]                       # 63 + 1 == LEMON_MAX_K: the deepest the train split can search
    assert parse_k_sweep("7,") == [7]


@pytest.mark.parametrize("text,word", [("", "empty"), (" , ,", "empty"), ("0,5", ">= 1"), ("-3", ">= 1"), ("5,64", "LEMON_MAX_K"),
                                       ("1,2,200", "LEMON_MAX_K"), ("1,two", "integers"), ("1.5", "integers")])
def test_sweep_list_refusals_say_why(text, word):
    from lemon_amd.run_lemon import parse_k_sweep
    with pytest.raises(ValueError) as e:
        parse_k_sweep(text)
    assert "--knn_k_sweep" in str(e.value) and word in str(e.value)


def test_sweep_limit_is_the_headers():
    from lemon_amd import _lib, run_lemon
    hdr = open(os.path.join(ROOT, "include", "lemon_hip.h")).read()
    assert int(re.search(r"#define LEMON_MAX_K (\d+)", hdr).group(1)) == _lib.MAX_K == run_lemon.MAX_SWEEP_K + 1
    assert int(re.search(r"#define LEMON_KSWEEP_MAX_KS (\d+)", hdr).group(1)) == _lib.KSWEEP_MAX_KS == 16


def test_cli_refuses_a_bad_sweep_before_any_work(tmp_path, capsys):
    from lemon_amd.run_lemon import main
    out = tmp_path / "never"
    for bad in ("", "0", "64"):
        with pytest.raises(SystemExit) as e:
            main(["--output_dir", str(out), "--knn_k_sweep", bad])
        assert e.value.code == 2
        assert "--knn_k_sweep" in capsys.readouterr().err
    assert not out.exists()


def test_new_flag_leaves_the_reference_flags_alone():
    from lemon_amd.run_lemon import build_parser
    args = vars(build_parser().parse_args(["--output_dir", "x"]))
    for name, default in REFERENCE_DEFAULTS.items():
        assert args[name] == default, name
    assert args["knn_k_sweep"] is None
    swept = vars(build_parser().parse_args(["--output_dir", "x", "--knn_k_sweep", "1,5"]))
    assert swept["knn_k_sweep"] == "1,5"
    assert {k: v for k, v in swept.items() if k != "knn_k_sweep"} == {k: v for k, v in args.items() if k != "knn_k_sweep"}


def test_selection_rule():
    from lemon_amd.run_lemon import select_best_k
    assert select_best_k({1: 0.5, 5: 0.7, 10: 0.6}) == 5
    assert select_best_k({10: 0.7, 5: 0.7, 1: 0.2}) == 5            # ties go to the smaller k, whatever the dict's order
    assert select_best_k({1: 0.7, 5: 0.7, 10: 0.7}) == 1
    assert select_best_k({50: 0.0}) == 50
    assert select_best_k({}) is None and select_best_k({1: 0.5, 5: None}) is None


def test_grid_points_are_what_maximize_metric_hands_to_batch_grid():
    from lemon_amd import metrics as M
    grid = {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}
    y = np.array([0, 1, 0, 1, 1, 0])
    seen = []

    def batch_grid(hps):
        seen.append(hps)
        return np.zeros(len(hps))
    for force_zero, force_one in (((), ()), (("tau_1_n", "tau_1_m"), ()), ((), ("beta",))):
        del seen[:]
        M.maximize_metric(lambda hp: np.arange(6.0), y, grid, [[0] * 6], force_zero=force_zero, force_one=force_one,
                          scipy_methods=(), batch_grid=batch_grid)
        pts = M.grid_points(grid, force_zero, force_one)
        assert seen == [pts] and len(pts) == 36
        assert len({(p["tau_1_n"], p["tau_2_n"]) for p in pts}) == (2 if force_zero else 4)


def test_prefix_record_on_cpu_tensors():
    import torch
    from lemon_amd.neighbors import REC_KEYS, prefix_record
    n, depth = 7, 12
    rec = {"d_1": torch.rand(n)}
    for key in REC_KEYS[1:7]:
        rec[key] = torch.rand(n, depth)
    rec["D_n"][3, 5:] = float("nan")
    rec["I_n"] = torch.arange(n * depth).reshape(n, depth)
    rec["I_m"] = -rec["I_n"]
    for k in (1, 5, 12):
        pre = prefix_record(rec, k)
        assert list(pre) == list(rec)
        assert pre["d_1"] is rec["d_1"]
        for key in REC_KEYS[1:]:
            assert pre[key].shape == (n, k) and pre[key].is_contiguous() and pre[key].dtype == rec[key].dtype
            assert torch.equal(pre[key].view(torch.int32) if pre[key].dtype == torch.float32 else pre[key],
                               rec[key][:, :k].contiguous().view(torch.int32) if pre[key].dtype == torch.float32 else rec[key][:, :k])
    no_idx = {key: v for key, v in rec.items() if key not in ("I_n", "I_m")}
    assert "I_n" not in prefix_record(no_idx, 3) and prefix_record(no_idx, 3)["dists_m"].shape == (n, 3)
    assert prefix_record(prefix_record(rec, 9), 4)["D_m"].equal(prefix_record(rec, 4)["D_m"])
    for bad in (0, 13, -1):
        with pytest.raises(ValueError):
            prefix_record(rec, bad)
    assert rec["D_n"].shape == (n, depth)                   # the deep record is left as it was


def test_header_binding_and_library_agree_on_the_new_names():
    from lemon_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lemon_hip.h")).read(), flags=re.S)
    declared = dict(re.findall(r"\b(lemon_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", hdr))
    assert os.path.exists(_lib.SO_PATH), "liblemon_hip.so is not built (python -m lemon_amd.build)"
    raw, bound = ctypes.CDLL(_lib.SO_PATH), _lib.load()
    for name in ("lemon_grid_f1_ks", "lemon_grid_f1_ks_workspace_bytes"):
        assert name in declared and _lib.EXPORTS.count(name) == 1 and hasattr(raw, name), name
        assert len(getattr(bound, name).argtypes) == declared[name].count(",") + 1, name
    assert re.search(r"\bint64_t\s+lemon_grid_f1_ks_workspace_bytes\s*\(", hdr)
    assert bound.lemon_grid_f1_ks_workspace_bytes.restype is ctypes.c_int64
    assert "ksweep.hip" in build.SOURCES and "gridf1_brent.hpp" in build.HEADERS
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"k_ks_terms" in blob and b"k_ks_combine" in blob


def test_workspace_bytes_follow_the_documented_formula():
    """8 n K (P + G) + 16 P + 24 G bytes, P = the distinct (tau_1, tau_2) bit patterns of the n side plus those of the m side
    (host arithmetic: needs no device)."""
    from lemon_amd import _lib
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    formula = lambda n, K, G, P: 8 * n * K * (P + G) + 16 * P + 24 * G
    rows = np.array([[1, 2, 0.0, 1, 0.0, 1], [3, 4, 0.0, 1, 0.0, 1], [5, 6, -0.0, 1, 5, 1], [7, 8, 0.0, 1, 5, 1]], dtype=np.float64)
    assert lib.lemon_grid_f1_ks_workspace_bytes(1000, 8, 4, dp(rows)) == formula(1000, 8, 4, 2 + 2)     # -0.0 is its own pair
    assert lib.lemon_grid_f1_ks_workspace_bytes(1, 1, 1, dp(rows)) == formula(1, 1, 1, 2)
    big = np.zeros((65535, 6))
    big[:, 2] = np.arange(65535)
    assert lib.lemon_grid_f1_ks_workspace_bytes(5000, 16, 65535, dp(big)) == formula(5000, 16, 65535, 65535 + 1)    # beyond 2^32
    for n, K, G in ((0, 1, 1), (10, 0, 1), (10, 17, 1), (10, 1, -1), (10, 1, 65536)):
        assert lib.lemon_grid_f1_ks_workspace_bytes(n, K, G, dp(rows)) == -1, (n, K, G)
