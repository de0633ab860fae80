"""Host side of the cell sweep (no GPU): the --ablation_sweep / --subset_val_set_sweep flags and their refusals, the frame of a
subset cell against the draw of a --subset_val_set run recomputed here, the directory of a cell, and the record the cells of a
subset share (on the CPU: it only indexes and slices)."""
import itertools

import numpy as np
import pytest

from lemon_amd.run_lemon import (ABLATIONS, NEIGHBOR_COLUMNS, build_parser, cell_path, main, parse_ablation_sweep,
                                 parse_subset_sweep, subset_val_frame)

N_TRAIN, N_VAL, N_TEST, DEPTH = 7, 5, 4, 3


# ---- the flags -------------------------------------------------------------------------------------------------------------------
def test_ablation_sweep_values():
    assert parse_ablation_sweep("d1,none,d1, tau_1 ,none") == ["d1", "none", "tau_1"]
    assert parse_ablation_sweep("none") == ["none"]
    assert parse_ablation_sweep("all") == list(ABLATIONS)
    choices = next(a for a in build_parser()._actions if a.dest == "ablation").choices
    assert parse_ablation_sweep("all") == list(choices) and len(choices) == 10


@pytest.mark.parametrize("bad,word", [("", "empty"), (" , ", "empty"), ("none,tau_3", "tau_3"), ("all,none", "all"), ("None", "None")])
def test_ablation_sweep_refusals(bad, word):
    with pytest.raises(ValueError) as e:
        parse_ablation_sweep(bad)
    assert "--ablation_sweep" in str(e.value) and word in str(e.value)


def test_subset_sweep_values():
    assert parse_subset_sweep("10,-1,500,10, 50 ,-1") == [10, -1, 500, 50]
    assert parse_subset_sweep("-1") == [-1] and parse_subset_sweep("1") == [1]


@pytest.mark.parametrize("bad,word", [("", "empty"), (",", "empty"), ("10,0", "0"), ("-2", "-2"), ("10,x", "integers"),
                                      ("1.5", "integers"), ("all", "integers")])
def test_subset_sweep_refusals(bad, word):
    with pytest.raises(ValueError) as e:
        parse_subset_sweep(bad)
    assert "--subset_val_set_sweep" in str(e.value) and word in str(e.value)


@pytest.mark.parametrize("flag,bad", [("--ablation_sweep", ""), ("--ablation_sweep", "none,nope"), ("--subset_val_set_sweep", ""),
                                      ("--subset_val_set_sweep", "0"), ("--subset_val_set_sweep", "-3,10"),
                                      ("--subset_val_set_sweep", "ten")])
def test_a_bad_list_is_a_parser_error_before_anything_runs(tmp_path, capsys, flag, bad):
    out = tmp_path / "never"
    with pytest.raises(SystemExit) as e:
        main(["--output_dir", str(out), flag, bad])
    assert e.value.code == 2 and flag in capsys.readouterr().err and not out.exists()


def test_the_flags_default_to_none_and_change_nothing_else():
    args = vars(build_parser().parse_args(["--output_dir", "x"]))
    assert args["ablation_sweep"] is None and args["subset_val_set_sweep"] is None
    swept = vars(build_parser().parse_args(["--output_dir", "x", "--ablation_sweep", "all", "--subset_val_set_sweep", "-1,10"]))
    assert swept["ablation_sweep"] == "all" and swept["subset_val_set_sweep"] == "-1,10"
    new = ("ablation_sweep", "subset_val_set_sweep")
    assert {k: v for k, v in swept.items() if k not in new} == {k: v for k, v in args.items() if k not in new}


# ---- the directory of a cell -----------------------------------------------------------------------------------------------------
def test_cell_path_has_a_level_per_swept_axis_in_nesting_order():
    values = {"dist_type": "euclidean", "subset_val_set": -1, "ablation": "tau_1_2", "knn_k": 5}
    order = ["dist_type", "subset_val_set", "ablation", "knn_k"]
    seen = set()
    for r in range(5):
        for axes in itertools.combinations(order, r):
            path = cell_path(**{a: values[a] for a in axes})
            assert path == "/".join(f"{a}={values[a]}" for a in order if a in axes)
            seen.add(path)
    assert len(seen) == 16 and "" in seen
    assert cell_path("cosine", 10, "none", 1) == "dist_type=cosine/subset_val_set=10/ablation=none/knn_k=1"


# ---- the frame of a subset cell --------------------------------------------------------------------------------------------------
def _frame(seed=0):
    """a frame as run_lemon._run leaves it: 7 train / 5 val / 4 test rows, the blocks in that order, idx from 0 in each"""
    import pandas as pd
    rng = np.random.default_rng(seed)
    blocks = []
    for sset, n in (("train", N_TRAIN), ("val", N_VAL), ("test", N_TEST)):
        flips = rng.integers(0, 2, n)
        blocks.append(pd.DataFrame({
            "sset": sset, "idx": np.arange(n), "actual_label": list(rng.integers(0, 10, n)), "noisy_label": list(rng.integers(0, 10, n)),
            "is_mislabel": flips, "is_correct_label": 1 - flips, "d_1": rng.uniform(size=n),
            **{c: list(rng.uniform(size=(n, DEPTH)).astype(np.float32)) for c in NEIGHBOR_COLUMNS}}))
    return pd.concat(blocks, ignore_index=True)


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("m", [-1, 1, 4, 5, 9])
def test_subset_val_frame_is_the_draw_of_a_subset_run(m, seed):
    import pandas as pd
    df = _frame()
    before = df.copy(deep=True)
    got = subset_val_frame(df, m, seed)
    pd.testing.assert_frame_equal(df, before, check_exact=True)                       # the source frame is not written to
    if m == -1:
        assert got is df
        return
    pick = np.random.default_rng(seed).choice(np.arange(N_VAL), min(m, N_VAL), replace=False)      # cli_common.prepare
    n_sub = len(pick)
    assert n_sub == min(m, N_VAL) and len(got) == N_TRAIN + n_sub + N_TEST
    assert list(got.index) == list(range(len(got)))
    assert list(got.sset) == ["train"] * N_TRAIN + ["val"] * n_sub + ["test"] * N_TEST
    assert list(got.columns) == list(df.columns) and list(got.dtypes) == list(df.dtypes)
    pd.testing.assert_frame_equal(got[got.sset == "train"], df[df.sset == "train"], check_exact=True)
    pd.testing.assert_frame_equal(got[got.sset == "test"].reset_index(drop=True),
                                  df[df.sset == "test"].reset_index(drop=True), check_exact=True)
    val, src = got[got.sset == "val"].reset_index(drop=True), df[df.sset == "val"].reset_index(drop=True)
    assert list(val.idx) == list(range(n_sub))                                         # renumbered, as Dataset.subset's rows are
    want = src.iloc[pick].reset_index(drop=True)
    pd.testing.assert_frame_equal(val.drop(columns="idx"), want.drop(columns="idx"), check_exact=True)
    if m >= N_VAL:                                                                     # a permutation, not the identity
        assert sorted(pick) == list(range(N_VAL)) and list(pick) != list(range(N_VAL))
        assert sorted(val.d_1) == sorted(src.d_1) and list(val.d_1) != list(src.d_1)


def test_the_draws_of_different_m_are_no_prefixes_of_one_another():
    import pandas as pd
    df = pd.DataFrame({"sset": "val", "idx": np.arange(60), "d_1": np.arange(60.0)})
    first = lambda m: [int(v) for v in subset_val_frame(df, m, 0).d_1[:2]]
    assert first(5) == [36, 29] and first(10) == [43, 48]


# ---- what the cells of one subset share ------------------------------------------------------------------------------------------
def test_cells_share_the_neighbour_arrays_and_not_what_they_write():
    import torch
    from lemon_amd.run_lemon import _Record as _CellRecord
    from tests.tailfx import device_rec as _device_rec
    df = _frame()
    before = df.copy(deep=True)
    deep = {c: np.stack(df[c].values) for c in NEIGHBOR_COLUMNS}
    cell = _CellRecord(df, deep, None, "cpu", [1, DEPTH], ["none", "d1", "only_beta"])
    a, b = cell.frame(2), cell.frame(2)
    a["d_1"] = 0.0                                                                     # run_lemon._tail, the d1 ablation
    a["know_val_labels_pred_score"] = 1.0
    assert list(b.columns) == list(df.columns) and np.array_equal(b.d_1.values, before.d_1.values)
    assert np.array_equal(df.d_1.values, before.d_1.values) and list(df.columns) == list(before.columns)
    for c in NEIGHBOR_COLUMNS:
        assert all(x is y for x, y in zip(a[c].values, b[c].values))                   # shared, not copied
        assert np.array_equal(np.stack(a[c].values), deep[c][:, :2]) and a[c].iloc[0].shape == (2,)
        assert np.array_equal(np.stack(cell.frame(None)[c].values), deep[c])
    for k in (1, 2, None):
        for val_only in (False, True):
            frame = cell.frame(k)
            frame = frame[frame.sset == "val"] if val_only else frame
            for zero in (False, True):
                if zero:
                    frame = frame.copy()
                    frame["d_1"] = 0.0
                got, want = cell.rec(k, zero, val_only), _device_rec(frame, "cpu")
                assert set(got) == set(want)
                for key in want:
                    assert got[key].is_contiguous() and got[key].dtype == torch.float32
                    assert torch.equal(got[key], want[key]), (key, k, val_only, zero)
    assert np.array_equal(cell.y_val, df[df.sset == "val"].is_mislabel.values)
    # a subset's record: the rows of the stacked arrays, in the subset's order
    from lemon_amd.run_lemon import _subset_rows
    rows = _subset_rows(df, 4, 0)
    sub = subset_val_frame(df, 4, 0)
    cell = _CellRecord(sub, deep, rows, "cpu", None, ["none"])
    want = _device_rec(sub, "cpu")
    for key, v in cell.rec(None, False, False).items():
        assert torch.equal(v, want[key]), key
