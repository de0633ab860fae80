"""python -m lemon_amd.run_lemon -- drop-in for the reference's `python -m run_lemon` (run_lemon.py).

Same 21 flags, defaults and choices (run_lemon.py:35-57), same outputs (args.json, out.txt, err.txt,
res.pkl {'df','agg_results'}, know_val_labels_scores.csv, need_hparam_optim, done) and the same
per-sample record schema (:291-307).  Differences, all explicit:
  * embeddings stay in HBM; kNN + per-sample quantities + scores run in liblemon_hip.so (no faiss, no
    per-sample Python loop); the train split is embedded once and reused as DB and as queries;
  * weights/data come from LOCAL paths (extension flags --clip_path, --data_root, --arch, --algo,
    --encoder_batch); `--clip_path random[:arch]` / `--data_root synthetic:N` run without any files;
  * under torchrun (WORLD_SIZE>1) samples are sharded over ranks, DB shards all-gathered over RCCL;
  * extension flag --knn_k_sweep 1,2,5,...: the validation protocol's choice of knn_k in ONE run -- embed, DB build and search
    once at the largest k, then the tail of a run per k on the prefix of the record (<output_dir>/knn_k=<k>/, k_selection.json);
  * extension flag --dist_type_sweep cosine,euclidean: both metrics of the reference's grid in ONE run -- embed once, one pair
    of IP indices, one search per modality and split; the euclidean lists are derived from the cosine lists and certified row
    by row, the rest searched again (<output_dir>/dist_type=<m>/, dist_sweep.json).  Composes with --knn_k_sweep.
  * extension flags --subset_val_set_sweep -1,10,50,... / --ablation_sweep none,multimodal_baseline,...|all: the two axes of the
    reference's grid that only change the tail of a run, in ONE run -- embed and search once on the whole validation set, then
    the tail of a run per cell on the rows that run would have drawn, the record kept on the device across the cells
    (<output_dir>/[dist_type=<d>/][subset_val_set=<m>/][ablation=<a>/][knn_k=<k>/], cell_sweep.json).  Compose with both others.
  * extension flag --eval_metrics device: the threshold metrics behind the score -- metrics.eval_metrics on the validation rows
    and on every split -- as ONE ops.eval_metrics call per cell on the score tensor (lemon_eval_metrics); default host.
Behind the per-sample record every run takes one path: _cell_tails walks the cells of dist_type x subset_val_set x ablation x
knn_k -- an axis that is not swept has one level, a plain run is the one cell -- and runs _tail on each, on a frame and on
device arrays that the _Record of its (metric, subset) hands out; that class makes every grid, search and polish launch.
"""
import argparse
import copy
import json
import os
import pickle
import re
import sys
from datetime import datetime

import numpy as np
import pandas as pd
import torch

from .cli_common import CLF_DATASETS, add_eval_metrics_flag, add_extension_flags  # noqa: F401  (CLF_DATASETS re-exported: run_lemon.py:32)


ABLATIONS = ("none", "tau_1", "tau_2", "tau_1_2", "beta", "gamma", "multimodal_baseline", "d1", "only_gamma",
             "only_beta")                                                      # run_lemon.py:49-50, in the parser's order
FORCE_MASKS = {"none": ([], []), "d1": ([], ["beta"]), "tau_1": (["tau_1_n", "tau_1_m"], []), "tau_2": (["tau_2_n", "tau_2_m"], []),
               "tau_1_2": (["tau_1_n", "tau_1_m", "tau_2_n", "tau_2_m"], []), "beta": (["beta"], []),
               "gamma": (["gamma"], [])}                  # the ablations that search: ablation -> (force_zero, force_one)
SEARCH_STARTS = [[0] * 6, [0.5] * 6, [1] * 6, [10] * 6]       # the start points and methods the reference hands to maximize_metric
SEARCH_METHODS = ("Powell", "Nelder-Mead")
NEIGHBOR_COLUMNS = ("dists_n", "D_n", "dists_tr_n", "dists_m", "D_m", "dists_tr_m")      # of the per-sample record, beside d_1


def build_parser():
    p = argparse.ArgumentParser(description="LEMoN")
    p.add_argument("--exp_name", type=str)
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--dataset", type=str, default="cifar100",
                   choices=["cifar10", "cifar100", "flickr30k", "mscoco", "mimiccxr_caption", "mmimdb", "cifar10_full",
                            "cifar100_full", "mini_imagenet", "stanford_cars", "cc3m"])
    p.add_argument("--noise_type", type=str, default="real",
                   choices=["real", "asymmetric", "symmetric", "random", "noun", "cat"])
    p.add_argument("--noise_level", type=float, default=0.4)
    p.add_argument("--dist_type", type=str, default="cosine", choices=["cosine", "euclidean"])
    p.add_argument("--normalize_d1", action="store_true",
                   help="normalize CLIP sim by all possible labels. Only for CIFAR-10 and CIFAR-100")
    p.add_argument("--clip_model", type=str, default="huggingface_clip",
                   choices=["huggingface_clip", "biomed_clip", "mimic_clip_from_scratch_random",
                            "mimic_clip_from_scratch_cat", "chexzero", "cc3m_clip_from_scratch"])
    p.add_argument("--knn_k", default=5, type=int)
    p.add_argument("--batch_size", default=128, type=int)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--data_seed", default=0, type=int)
    p.add_argument("--compr_dataset_size_limit", default=50000, type=int)
    p.add_argument("--ablation", default="none", choices=list(ABLATIONS))
    p.add_argument("--use_discrete_for_text", action="store_true", help="use the discrete metric for text comparisons")
    p.add_argument("--real_dataset", action="store_true", help="Running on real dataset, do not optimize hparams")
    p.add_argument("--custom_cifar_prompt", default=None)
    p.add_argument("--subset_val_set", default=-1, type=int)
    p.add_argument("--debug", action="store_true")
    p.add_argument("--skip_train", action="store_true")
    p.add_argument("--skip_hparam_optim", action="store_true")
    # ---- extensions (not in the reference) ----
    add_extension_flags(p)
    p.add_argument("--lbfgs_device", default="cuda", choices=["cuda", "cpu"],
                   help="where the SoftMargin/LBFGS polish of the hyper-parameter search runs (lib/metrics/utils.py:121-149)")
    p.add_argument("--hparam_grid", default="full", choices=["full", "small"],
                   help="'small' = 3x3x2x2 grid for smoke runs (reference grid is 21x21x4x4)")
    p.add_argument("--hparam_search", default="host", choices=["host", "device"],
                   help="where the Powell / Nelder-Mead searches in front of the grid run: 'host' = scipy.optimize.minimize, one "
                        "score launch and one copy per objective evaluation (the reference's way); 'device' = all searches of a "
                        "run in one launch (lemon_hparam_search), the same optimisers restated in IEEE double, same results")
    p.add_argument("--lbfgs_polish", default="host", choices=["host", "device"],
                   help="where the SoftMargin/LBFGS polish of the hyper-parameter search runs: 'host' = torch.optim.LBFGS driven "
                        "from Python on --lbfgs_device (the reference's way; a few seconds a knn_k, launch-bound); 'device' = every "
                        "polish of a run in one launch (lemon_lbfgs_polish), the same optimiser restated in fixed-order IEEE double: "
                        "the candidates are a function of the record alone; they are scored exactly afterwards, as before")
    add_eval_metrics_flag(p)
    p.add_argument("--knn_k_sweep", default=None, type=str,
                   help="comma-separated knn_k values, e.g. 1,2,5,10,15,20,30,50 (the reference's grid, experiments.py:86): embed, build "
                        "the DB and search ONCE at the largest, then run the tail of a --knn_k run for every value on the prefix "
                        "of the record -> <output_dir>/knn_k=<k>/ and <output_dir>/k_selection.json; --knn_k is ignored")
    p.add_argument("--dist_type_sweep", default=None, type=str,
                   help="comma-separated dist_type values, cosine,euclidean (experiments.py crosses the two with every other axis): "
                        "embed, build ONE pair of IP indices and search once per modality and split; the euclidean neighbour lists "
                        "are derived from the cosine lists searched --dist_sweep_margin deeper and certified row by row, rows that "
                        "cannot be certified are searched again on an L2 pair; then the tail of a --dist_type run per metric -> "
                        "<output_dir>/dist_type=<m>/ and <output_dir>/dist_sweep.json; --dist_type is ignored")
    p.add_argument("--dist_sweep_margin", default=4, type=int,
                   help="extra neighbours the cosine search of --dist_type_sweep keeps to certify the euclidean lists (the search "
                        "depth stays within LEMON_MAX_K = 64)")
    p.add_argument("--ablation_sweep", default=None, type=str,
                   help="comma-separated values of --ablation, or 'all' for the ten of them (the component table; experiments.py "
                        "crosses every grid with none,multimodal_baseline): embed, build the DB and search ONCE, then the tail of "
                        "an --ablation run for every value on the same record -> <output_dir>/ablation=<a>/ and "
                        "<output_dir>/cell_sweep.json; --ablation is ignored")
    p.add_argument("--subset_val_set_sweep", default=None, type=str,
                   help="comma-separated values of --subset_val_set, e.g. -1,10,50,100,500,1000 (experiments.py:205; -1 = the whole "
                        "validation set): embed and search the whole validation set ONCE, then the tail of a --subset_val_set run "
                        "for every value on the rows that run would have drawn -> <output_dir>/subset_val_set=<m>/ and "
                        "<output_dir>/cell_sweep.json; --subset_val_set is ignored.  The sweeps compose: a cell is "
                        "dist_type=<d>/subset_val_set=<m>/ablation=<a>/knn_k=<k>/, a level for every sweep flag given")
    # a list that begins with -1 is a value, as a lone negative number is to argparse, not an unknown option
    p._negative_number_matcher = re.compile(r"^-\d+(,\s*-?\d+)*,?$|^-\d*\.\d+$")
    return p


DIST_TYPES = ("cosine", "euclidean")
MAX_SWEEP_K = 63       # max + 1 <= LEMON_MAX_K: the train split searches k + 1 (include/lemon_hip.h)


def _parse_list(flag, text, such_as, convert=str, refuse=lambda value: None):
    """The values of a sweep flag, comma-separated in `text`: converted, de-duplicated, in the given order.  Refused
    (ValueError): an empty list, a list `convert` cannot read, a value `refuse` has a sentence about."""
    parts = [t.strip() for t in str(text).split(",") if t.strip()]
    if not parts:
        axis = flag[len("--"):-len("_sweep")]
        raise ValueError(f"{flag}: the list is empty; expected comma-separated values of {axis} such as {such_as}")
    try:
        values = [convert(t) for t in parts]
    except ValueError:
        raise ValueError(f"{flag}: {text!r} is not a comma-separated list of integers") from None
    out = []
    for value in values:
        why = refuse(value)
        if why:
            raise ValueError(f"{flag}: {why}")
        if value not in out:
            out.append(value)
    return out


def parse_dist_sweep(text):
    """'euclidean,cosine,cosine' -> ['euclidean', 'cosine']: de-duplicated, order kept.  Refused (ValueError): an empty list, a
    name that is not a dist_type."""
    return _parse_list("--dist_type_sweep", text, "cosine,euclidean",
                       refuse=lambda t: None if t in DIST_TYPES else f"{t!r} is not a dist_type (cosine|euclidean)")


def parse_k_sweep(text):
    """'10,1,5,5' -> [1, 5, 10]: sorted, de-duplicated.  Refused (ValueError): an empty list, anything that is not an integer,
    a value < 1, a largest value whose train-split search (k + 1) would pass LEMON_MAX_K."""
    ks = sorted(_parse_list("--knn_k_sweep", text, "1,2,5,10", int))
    if ks[0] < 1:
        raise ValueError(f"--knn_k_sweep: every knn_k must be >= 1, got {ks[0]}")
    if ks[-1] > MAX_SWEEP_K:
        raise ValueError(f"--knn_k_sweep: the largest knn_k is {ks[-1]}, but knn_k + 1 (the train split's search) must not "
                         f"exceed LEMON_MAX_K = {MAX_SWEEP_K + 1}")
    return ks


def parse_ablation_sweep(text):
    """'d1,none,d1' -> ['d1', 'none']: de-duplicated, order kept; 'all' -> the ten values of --ablation in the parser's order.
    Refused (ValueError): an empty list, a name that is not an ablation."""
    if str(text).replace(",", " ").split() == ["all"]:
        return list(ABLATIONS)
    return _parse_list("--ablation_sweep", text, "none,multimodal_baseline, or all", refuse=lambda t: None if t in ABLATIONS else
                       f"{t!r} is not an ablation ({'|'.join(ABLATIONS)}, or all alone)")


def parse_subset_sweep(text):
    """'-1,10,50,10' -> [-1, 10, 50]: de-duplicated, order kept; -1 = the whole validation set.  Refused (ValueError): an empty
    list, anything that is not an integer, 0, a value below -1."""
    return _parse_list("--subset_val_set_sweep", text, "-1,10,50,100", int, lambda m: None if m == -1 or m > 0 else
                       f"a subset has at least one row (or is -1, the whole validation set), got {m}")


SWEEP_FLAGS = {"dist_type_sweep": parse_dist_sweep, "subset_val_set_sweep": parse_subset_sweep,
               "ablation_sweep": parse_ablation_sweep, "knn_k_sweep": parse_k_sweep}       # outermost to innermost level


def parse_sweeps(args):
    """{axis: its parsed list, None where its flag is not given}; ValueError with the refusal of the first list that has one"""
    return {flag[:-len("_sweep")]: None if getattr(args, flag) is None else parse(getattr(args, flag))
            for flag, parse in SWEEP_FLAGS.items()}


def cell_path(dist_type=None, subset_val_set=None, ablation=None, knn_k=None):
    """The directory of a cell below <output_dir>: dist_type=<d>/subset_val_set=<m>/ablation=<a>/knn_k=<k>, outermost to
    innermost, a level for every axis that is swept (not None); '' where none is."""
    levels = (("dist_type", dist_type), ("subset_val_set", subset_val_set), ("ablation", ablation), ("knn_k", knn_k))
    return "/".join(f"{name}={value}" for name, value in levels if value is not None)


def _subset_rows(df, m, data_seed):
    """Positions in `df` of the rows of subset_val_frame(df, m, data_seed), in its order."""
    sset = df["sset"].values
    val = np.flatnonzero(sset == "val")
    rng = np.random.default_rng(data_seed)         # a generator of its own per m, as a run has: the draws are no prefixes
    pick = rng.choice(np.arange(len(val)), min(m, len(val)), replace=False)
    return np.concatenate([np.flatnonzero(sset == "train"), val[pick], np.flatnonzero(sset == "test")])


def subset_val_frame(df, m, data_seed, rows=None):
    """The per-sample frame a `--subset_val_set m --data_seed data_seed` run builds, from the frame `df` of the run on the whole
    validation set (cli_common.prepare draws the subset in front of the embedding pass; validation rows are never in the
    DB, so a row's record does not depend on which other validation rows exist): train and test rows as they are, the
    validation rows rng.choice(arange(n_val), min(m, n_val), replace=False) of default_rng(data_seed) in that order -- for
    m >= n_val a permutation, not the identity -- with idx renumbered 0 .. m'-1, the blocks in the order train, val, test.
    m = -1: `df` itself.  The neighbour arrays of the rows are shared with `df`, not copied."""
    if m == -1:
        return df
    out = df.iloc[_subset_rows(df, m, data_seed) if rows is None else rows].reset_index(drop=True)
    is_val = (out["sset"] == "val").values
    idx = out["idx"].values.copy()
    idx[is_val] = np.arange(int(is_val.sum()), dtype=idx.dtype)
    out["idx"] = idx
    return out


def select_best_k(selected_val):
    """{k: selected_val} -> the k with the highest value, ties to the smaller k; None when there is nothing to select on
    (no k, or a k without a value)."""
    if not selected_val or any(v is None for v in selected_val.values()):
        return None
    best = None
    for k in sorted(selected_val):
        if best is None or selected_val[k] > selected_val[best]:
            best = k
    return best


def main(argv=None):
    from .cli_common import run_with_tee
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        parse_sweeps(args)
    except ValueError as e:
        parser.error(str(e))
    if args.dist_type_sweep is not None and args.dist_sweep_margin < 0:
        parser.error("--dist_sweep_margin: must be >= 0")
    return run_with_tee(_run, args)


def _run(args):
    from . import _lib, metrics as M, ops
    from .cli_common import meta_columns, prepare
    from .neighbors import LemonDB
    from .pipeline import all_gather_rows

    if args.real_dataset:
        assert args.noise_level == 0.0
    ctx = prepare(args)
    out_dir, world, rank, device = ctx.out_dir, ctx.world, ctx.rank, ctx.device
    is_clf, label_set, embedder = ctx.is_clf, ctx.label_set, ctx.embedder
    embed_split, ids_of, sets = ctx.embed_split, ctx.ids_of, ctx.sets
    train_set, train_indices_in_compr = sets["train"], ctx.train_indices_in_compr

    start_t = datetime.now()
    emb = {"train": embed_split(train_set, "train")}
    # DB = train rows listed in train_indices_in_compr, in that order (Subset order, run_lemon.py:124)
    n_train = len(train_set)
    full_img = all_gather_rows(emb["train"][0], n_train)
    full_txt = all_gather_rows(emb["train"][1], n_train)
    tr_prompt_ids = ids_of(emb["train"][2])
    full_pid = all_gather_rows(torch.from_numpy(tr_prompt_ids).to(device), n_train) if world > 1 else \
        torch.from_numpy(tr_prompt_ids).to(device)
    sel = torch.from_numpy(np.asarray(train_indices_in_compr)).to(device)
    algo = {"auto": None, "f32": _lib.ALGO_F32_MFMA, "bf16": _lib.ALGO_BF16_FILTER}[args.algo]
    swept = parse_sweeps(args)              # axis -> its values, None where the run has the one value of `args`
    metrics, sweep = swept["dist_type"], swept["knn_k"]
    dist_names = metrics or [args.dist_type]
    both = len(dist_names) == 2             # one IP pair serves both metrics (LemonDB.neighbors_metrics)
    db = LemonDB(full_img[sel], full_txt[sel], tuple(dist_names) if both else dist_names[0], tr_label_id=full_pid[sel], algo=algo)

    cls_txt = None
    if is_clf:   # class-prompt embeddings, only used by --normalize_d1 (:180-190)
        cls_txt = embedder.embed_texts(ctx.tokenize([ctx.prompt_fn(t) for t in label_set]))

    in_db_mask = np.zeros(n_train, dtype=np.uint8)
    in_db_mask[train_indices_in_compr] = 1
    names = ["val", "test"] if (args.debug or args.skip_train) else ["train", "val", "test"]
    k = sweep[-1] if sweep else args.knn_k        # a sweep searches once, at its largest k
    frames = {m: [] for m in dist_names}
    sweep_counts = {}
    for sname in names:
        if sname not in emb:
            emb[sname] = embed_split(sets[sname], sname)
        e_img, e_txt, meta = emb[sname]
        nq, lo = e_img.shape[0], meta["lo"]
        kw = dict(drop_self=(sname == "train"), in_db=in_db_mask[lo:lo + nq] if sname == "train" else None,
                  discrete=args.use_discrete_for_text, q_label_id=ids_of(meta), return_indices=False)
        n_total = len(sets[sname])
        if both:
            recs, counts = db.neighbors_metrics(e_img, e_txt, k, margin=args.dist_sweep_margin, **kw)
            flags = torch.stack([counts["cert_n"], counts["cert_m"]], dim=1).to(torch.uint8)
            flags = all_gather_rows(flags, n_total).cpu().numpy().astype(bool)       # [n_total, 2]: every rank's shard
            sweep_counts[sname] = {"rows": int(n_total), "certified_n": int(flags[:, 0].sum()), "certified_m": int(flags[:, 1].sum()),
                                   "fallback": int((~(flags[:, 0] & flags[:, 1])).sum())}
        else:
            recs = {dist_names[0]: db.neighbors(e_img, e_txt, k, **kw)}
            sweep_counts[sname] = {"rows": int(n_total), "certified_n": None, "certified_m": None, "fallback": None}
        noisy_shard = None
        if args.normalize_d1:                     # this rank's rows, before the metadata of all ranks replaces them
            assert is_clf
            noisy_shard = torch.from_numpy(np.asarray(meta["noisy"], dtype=np.int32))
        meta, flips = ctx.gather_meta(meta)       # metadata to every rank (small python objects)
        for m in dist_names:
            rec = recs[m]
            if args.normalize_d1:
                rec["d_1"] = ops.d1_normalized(m, e_img, cls_txt, noisy_shard)
            host = {key: all_gather_rows(v, n_total).cpu().numpy() for key, v in rec.items()}
            if rank == 0:
                frames[m].append(pd.DataFrame({
                    **meta_columns(sname, n_total, meta, flips),
                    "d_1": host["d_1"].astype(np.float64),
                    **{c: list(host[c]) for c in NEIGHBOR_COLUMNS},
                }))
    torch.cuda.synchronize(device)
    timedelta = (datetime.now() - start_t).total_seconds()
    if rank != 0:
        if world > 1:
            torch.distributed.destroy_process_group()
        return 0
    n_samples = sum(len(f) for f in frames[dist_names[0]])
    print(f"Finished {n_samples} samples in {timedelta} seconds; avg of {timedelta / n_samples}s per sample")
    cell_sweep = swept["subset_val_set"] is not None or swept["ablation"] is not None
    cells = []
    for m in dist_names:
        df = pd.concat(frames[m], ignore_index=True)
        args_m, out_m = args, out_dir
        if metrics is not None:             # the tail of a --dist_type m run, under its own directory
            out_m = out_dir / f"dist_type={m}"
            out_m.mkdir(exist_ok=True, parents=True)
            args_m = copy.copy(args)
            args_m.dist_type, args_m.output_dir = m, str(out_m)
            with open(out_m / "args.json", "w") as f:
                json.dump(vars(args_m), f, default=str)
            print(f"==== dist_type = {m} ====")
        cells += _cell_tails(args_m, df, out_dir, device, m if metrics is not None else None, swept["subset_val_set"],
                             swept["ablation"], sweep, record_errors=cell_sweep)
    failed = [c for c in cells if c["status"] != "ok"]
    if cell_sweep:
        with open(out_dir / "cell_sweep.json", "w") as f:
            json.dump({"axes": swept, "cells": cells}, f, indent=1)
        for c in failed:
            print(f"cell {c['path']}: {c['error']}", file=sys.stderr)
    if metrics is not None:
        with open(out_dir / "dist_sweep.json", "w") as f:
            json.dump({"metrics": list(dist_names), "margin": int(args.dist_sweep_margin) if both else None, "knn_k": int(k),
                       "splits": sweep_counts}, f, indent=1)
    if (metrics is not None or cell_sweep) and not failed:
        with open(os.path.join(out_dir, "done"), "w") as f:
            f.write("done")
    if world > 1:
        torch.distributed.destroy_process_group()
    return 1 if failed else 0


def _grid_setup(args):
    """(grid, force_zero, force_one) of the hyper-parameter search, or None where the run never reaches the grid."""
    if args.real_dataset or args.skip_hparam_optim or args.ablation in ("only_beta", "only_gamma", "multimodal_baseline"):
        return None
    grid = {"beta": np.arange(0, 100.01, 5), "gamma": np.arange(0, 100.01, 5), "tau_1": [0, 1, 5, 10],
            "tau_2": [0, 1, 5, 10]} if args.hparam_grid == "full" else \
           {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}
    force_zero, force_one = FORCE_MASKS[args.ablation]
    return grid, list(force_zero), list(force_one)


def _selection_entry(sel_res, ssets):
    """agg_results' entry as k_selection.json and cell_sweep.json record it; None for a run that selects nothing."""
    from . import metrics as M
    if sel_res is None:
        return None
    entry = {"selected_val": sel_res.get("selected_val"), **{name: float(sel_res[name]) for name in M.HP_NAMES},
             "thres": sel_res.get("thres"),
             "splits": {sset: {"AUROC": float(sel_res[sset]["AUROC"]), "F1_optimal": float(sel_res[sset]["F1_optimal"])}
                        for sset in ssets}}
    for key in ("selected_val", "thres"):
        entry[key] = None if entry[key] is None else float(entry[key])
    return entry


def _attempt(record_errors, fn, *args):
    """-> (fn(*args), None).  record_errors (a cell sweep): an exception is printed and kept, -> (None, its text), and the
    sweep goes on; elsewhere there is no handler in the way and it propagates."""
    if not record_errors:
        return fn(*args), None
    try:
        return fn(*args), None
    except Exception as e:
        import traceback
        traceback.print_exc()
        return None, f"{type(e).__name__}: {e}"


class _Record:
    """The record of one (metric, subset), for every tail on it: of the one cell of a plain run as of all cells of a sweep.
    The only place that uploads record arrays and that calls ops.grid_f1 / grid_f1_ks / local_search / lbfgs_polish /
    eval_metrics.  The
    neighbour arrays are uploaded ONCE, at the depth they were searched at, and stay on the device: the prefix of a knn_k, the
    validation rows and the zeroed d_1 of the d1 ablation are taken there (the same float32 bits an upload of a cell's own
    frame gives).  frame(k): the frame of a cell, its neighbour columns shared between the cells of a k.  grid_fn / search_fn /
    polish_fn: what maximize_metric asks for.  With a k axis (`ks`) the grid of an ablation is ONE ops.grid_f1_ks for all ks
    (grid_ks); the searches and the polishes are ONE ops.local_search / ops.lbfgs_polish launch per distinct d_1 column -- the
    real one and the zeroed one -- that covers every ablation of the run that searches and every k, made on first use, inside
    the cell that asks."""

    def __init__(self, df, deep, rows, device, ks, ablations):
        self.df, self.device, self.ks, self.ablations = df, device, ks, [a for a in ablations if a in FORCE_MASKS]
        self.host = deep if rows is None else {c: v[rows] for c, v in deep.items()}       # numpy [n, depth] a neighbour column
        self.dev = {c: torch.from_numpy(v.astype(np.float32)).to(device) for c, v in self.host.items()}
        d1 = torch.from_numpy(df["d_1"].values.astype(np.float32)).to(device)
        self.d1 = {False: d1, True: torch.zeros_like(d1)}
        is_val = (df["sset"] == "val").values
        self.val_rows = torch.from_numpy(np.flatnonzero(is_val)).to(device)
        self.y_val = df["is_mislabel"].values[is_val]
        self._recs, self._frames, self._grids, self._launched, self._layout = {}, {}, {}, {}, None

    def rec(self, k, zero_d1, val_only):
        """the device arrays of the frame of knn_k = k (None: the depth searched at), of all rows or of the validation rows"""
        if (k, val_only) not in self._recs:
            out = {}
            for c, v in self.dev.items():
                v = v[self.val_rows] if val_only else v
                out[c] = (v if k is None else v[:, :k]).contiguous()
            self._recs[(k, val_only)] = out
        d1 = self.d1[bool(zero_d1)]
        return {**self._recs[(k, val_only)], "d_1": d1[self.val_rows] if val_only else d1}

    def frame(self, k):
        """A cell's frame at knn_k = k (None: the record as searched): its own columns, so that what it writes (d_1, the score
        columns) stays its own; the arrays of the neighbour columns are shared."""
        if k not in self._frames:
            base = self.df.copy(deep=False)
            if k is not None:
                for c in NEIGHBOR_COLUMNS:
                    base[c] = list(np.ascontiguousarray(self.host[c][:, :k]))
            self._frames[k] = base
        return self._frames[k].copy(deep=False)

    def eval_metrics(self, score, prevalence):
        """--eval_metrics device: (the validation call's dict, {sset: its dict}) of `score`, the device tensor over all rows of
        the frame, in ONE ops.eval_metrics call; the row indices and labels of the splits are uploaded once for the record"""
        from .cli_common import EvalLayout
        if self._layout is None:
            self._layout = EvalLayout(self.df, self.device)
        return self._layout(score, prevalence)

    def grid_ks(self, ablation, grid):
        """(the points of `grid` under the masks of `ablation`, their F1 [len(ks), G]): ONE ops.grid_f1_ks, kept"""
        from . import metrics as M, ops
        if ablation not in self._grids:
            hps = M.grid_points(grid, *FORCE_MASKS[ablation])
            f1 = ops.grid_f1_ks(self.rec(None, "d1" in ablation, True), self.y_val, [[hp[n] for n in M.HP_NAMES] for hp in hps],
                                self.ks)[0]
            self._grids[ablation] = hps, f1
        return self._grids[ablation]

    def _launch(self, what, ablation):
        from . import ops
        zero = "d1" in ablation
        if (what, zero) not in self._launched:
            group = [a for a in self.ablations if ("d1" in a) == zero]
            rec, masks = self.rec(None, zero, True), [FORCE_MASKS[a] for a in group]
            # one mask pair goes as force_zero / force_one, several as cells=: the same launch, the result per cell
            how = dict(cells=masks) if len(masks) > 1 else dict(force_zero=masks[0][0], force_one=masks[0][1])
            if what == "search":
                res = ops.local_search(rec, self.y_val, SEARCH_STARTS, SEARCH_METHODS, ks=self.ks, **how)
            else:
                res = ops.lbfgs_polish(rec, self.y_val, SEARCH_STARTS, ks=self.ks, **how)
            self._launched[(what, zero)] = dict(zip(group, res if len(masks) > 1 else [res]))
        return self._launched[(what, zero)][ablation]

    def grid_fn(self, ablation, grid, t=None):
        """maximize_metric's batch_grid for a cell of `ablation`: its own ops.grid_f1 at the record's depth, or row t of grid_ks"""
        def serve(asked):
            from . import metrics as M, ops
            if t is None:
                return ops.grid_f1(self.rec(None, "d1" in ablation, True), self.y_val, [[hp[n] for n in M.HP_NAMES] for hp in asked])[0]
            hps, f1 = self.grid_ks(ablation, grid)
            assert asked == hps, "the grid of maximize_metric is not the grid lemon_grid_f1_ks was called with"
            return f1[t]
        return serve

    def search_fn(self, ablation, t=None):
        """maximize_metric's local_search for a cell of `ablation` (and of the t-th k of the sweep)"""
        def serve(x0s, methods, force_zero, force_one):
            asked = ([list(x0) for x0 in x0s], tuple(methods), (list(force_zero), list(force_one)))
            assert asked == (SEARCH_STARTS, SEARCH_METHODS, FORCE_MASKS[ablation]), \
                "the searches of maximize_metric are not the ones lemon_hparam_search was called with"
            res = self._launch("search", ablation)
            return res if t is None else res[t]
        return serve

    def polish_fn(self, ablation, t=None):
        """maximize_metric's lbfgs_polish for a cell of `ablation` (and of the t-th k of the sweep)"""
        def serve(x0s, force_zero, force_one):
            asked = ([list(x0) for x0 in x0s], (list(force_zero), list(force_one)))
            assert asked == (SEARCH_STARTS, FORCE_MASKS[ablation]), \
                "the polishes of maximize_metric are not the ones lemon_lbfgs_polish was called with"
            res = self._launch("polish", ablation)
            return [x for x, _ in (res if t is None else res[t])]
        return serve


def _cell_tails(args, df, out_root, device, dist, subsets, ablations, ks, record_errors):
    """The tail of a run for every cell of dist_type x subset_val_set x ablation x knn_k of one metric, on the record `df` that
    was searched once (at max(ks)) -> the entries of cell_sweep.json.  dist / subsets / ablations / ks: the swept axes (None:
    not swept -- the value of `args` holds, the directory has no such level; a plain run is the one cell with no level at all).
    A cell below <output_dir>[/dist_type=<d>] gets its own args.json; k_selection.json and done sit one level above knn_k=.
    record_errors: a cell whose tail raises is recorded with the exception's text and the sweep goes on (_attempt)."""
    deep = {c: np.stack(df[c].values) for c in NEIGHBOR_COLUMNS}       # stacked once a metric; a subset takes rows of it
    entries = []
    for m in subsets or [None]:
        rows = None if m in (None, -1) else _subset_rows(df, m, args.data_seed)
        frame = df if rows is None else subset_val_frame(df, m, args.data_seed, rows)
        record = _Record(frame, deep, rows, device, ks, ablations or [args.ablation])
        for a in ablations or [None]:
            where = dict(dist_type=dist, subset_val_set=m, ablation=a)
            out_a = out_root / cell_path(**where)
            args_a = copy.copy(args)
            if m is not None:
                args_a.subset_val_set = m
            if a is not None:
                args_a.ablation = a
            if m is not None or a is not None:
                print(f"==== {cell_path(**where)} ====")
            setup, failed = _grid_setup(args_a), None
            if ks and setup is not None:            # in front of the k loop: a failure is that of every k
                _, failed = _attempt(record_errors, record.grid_ks, args_a.ablation, setup[0])
            results = {}
            for t, k in enumerate(ks) if ks else [(None, None)]:
                out_k = out_root / cell_path(**where, knn_k=k)
                out_k.mkdir(exist_ok=True, parents=True)
                args_k = copy.copy(args_a)
                if k is not None:
                    args_k.knn_k = k
                if not (m is None and a is None and k is None):
                    args_k.output_dir = str(out_k)
                    with open(out_k / "args.json", "w") as f:
                        json.dump(vars(args_k), f, default=str)
                if k is not None:
                    print(f"---- knn_k = {k} ----")

                def tail():
                    if failed is not None:
                        raise RuntimeError(f"the grid of all ks: {failed}")
                    return _selection_entry(_tail(args_k, record.frame(k), out_k, record, t), frame.sset.unique())
                results[k] = _attempt(record_errors, tail)
            if ks:
                best = None if any(entry is None for entry, _ in results.values()) else \
                    select_best_k({k: entry["selected_val"] for k, (entry, _) in results.items()})
                with open(out_a / "k_selection.json", "w") as f:
                    json.dump({"ks": list(ks), "best_k": best, "per_k": {str(k): entry for k, (entry, _) in results.items()}}, f,
                              indent=1)
                if not any(error for _, error in results.values()):
                    with open(os.path.join(out_a, "done"), "w") as f:
                        f.write("done")
            for k, (entry, error) in results.items():
                entries.append({"path": cell_path(**where, knn_k=k), "dist_type": args_a.dist_type,
                                "subset_val_set": int(args_a.subset_val_set), "ablation": args_a.ablation,
                                "knn_k": int(args_a.knn_k if k is None else k),
                                **({"status": "ok"} if error is None else {"status": "error", "error": error}), **(entry or {})})
    return entries


def _tail(args, df, out_dir, record, t=None):
    """Everything behind the per-sample record: the d1 ablation, the hyper-parameter search, the final score, the metrics and
    the files of a run.  Returns agg_results' entry (None with --real_dataset / --skip_hparam_optim).  df: the cell's own frame,
    written to; record: the _Record it is a frame of, which holds the device arrays and serves the grid, the local searches of
    --hparam_search device and the polishes of --lbfgs_polish device; t: the index of the cell's k in record.ks (None: no k
    axis, the record as searched)."""
    from . import metrics as M, ops
    k, zero_d1 = None if t is None else record.ks[t], "d1" in args.ablation
    sel_res = None
    if zero_d1:
        df["d_1"] = 0.0

    if args.real_dataset or args.skip_hparam_optim:
        res = {"df": df}
    else:
        df_val = df.query('sset == "val"')
        rec_val = record.rec(k, zero_d1, True)
        y_val = df_val["is_mislabel"].values
        score_fn = lambda hp: ops.lemon_score(rec_val, hp).cpu().numpy()      # K5 on the device-resident val arrays
        crit = "know_val_labels"
        zero6 = dict(beta=0, gamma=0, tau_1_n=0, tau_2_n=0, tau_1_m=0, tau_2_m=0)
        if args.ablation == "only_beta":
            sel_res = {**zero6, "beta": 1}
        elif args.ablation == "only_gamma":
            sel_res = {**zero6, "gamma": 1}
        else:
            if args.ablation == "multimodal_baseline":
                best = [0] * 6
                best_f1, best_thres = M.optimize_f1_efficient(y_val, df_val["d_1"].values, return_thres=True)
            else:
                grid, force_zero, force_one = _grid_setup(args)
                local_search = record.search_fn(args.ablation, t) if args.hparam_search == "device" else None
                lbfgs_polish = record.polish_fn(args.ablation, t) if args.lbfgs_polish == "device" else None
                rec_lbfgs = None if lbfgs_polish is not None else \
                    {c: (df_val[c].values if c == "d_1" else np.stack(df_val[c].values))      # the host polish's own copy
                     for c in ("d_1",) + NEIGHBOR_COLUMNS}
                best, best_f1, best_thres = M.maximize_metric(
                    score_fn, y_val, grid, SEARCH_STARTS, M.optimize_f1_efficient, {}, scipy_methods=SEARCH_METHODS,
                    local_search=local_search, lbfgs_polish=lbfgs_polish,
                    force_zero=force_zero, force_one=force_one, rec_for_lbfgs=rec_lbfgs,
                    lbfgs_device=str(record.device) if args.lbfgs_device == "cuda" else "cpu",
                    batch_grid=record.grid_fn(args.ablation, grid, t))
            sel_res = dict(zip(M.HP_NAMES, best))
            sel_res.update(thres=best_thres, selected_val=best_f1)
        s, dn, dm = ops.lemon_score(record.rec(k, zero_d1, False), sel_res, return_dn=True)
        df[f"{crit}_pred_score"] = s.cpu().numpy()
        df[f"{crit}_d_n"], df[f"{crit}_d_m"] = dn.cpu().numpy(), dm.cpu().numpy()
        df_val = df.query('sset == "val"')
        prev = df.loc[df.sset == "val", "is_mislabel"].sum() / (df.sset == "val").sum()
        if args.eval_metrics == "device":              # the free validation rows and every split in one call, on the score tensor
            sel_res.update(record.eval_metrics(s, prev)[1])
        else:
            thress = M.eval_metrics(df_val["is_mislabel"], df_val[f"{crit}_pred_score"], prevalence=prev)
            for sset in df.sset.unique():
                sub = df.loc[df.sset == sset]
                sel_res[sset] = M.eval_metrics(sub["is_mislabel"], sub[f"{crit}_pred_score"], prevalence=prev,
                                               fix_thress=thress)
        df[["sset", "idx", "actual_label", "noisy_label", "is_mislabel", f"{crit}_pred_score"]].rename(
            columns={f"{crit}_pred_score": "pred_score"}).to_csv(out_dir / f"{crit}_scores.csv")
        res = {"df": df, "agg_results": {crit: sel_res}}
        for sset in df.sset.unique():
            print(f"{sset}: AUROC {sel_res[sset]['AUROC']:.4f}  F1 {sel_res[sset]['F1_optimal']:.4f}")

    pickle.dump(res, (out_dir / "res.pkl").open("wb"))
    if args.skip_hparam_optim:
        with open(os.path.join(out_dir, "need_hparam_optim"), "w") as f:
            f.write("need_hparam_optim")
    with open(os.path.join(out_dir, "done"), "w") as f:
        f.write("done")
    return sel_res


if __name__ == "__main__":
    sys.exit(main())
