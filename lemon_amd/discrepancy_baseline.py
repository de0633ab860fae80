"""python -m lemon_amd.discrepancy_baseline -- drop-in for the reference's
`python -m lib.baselines.discrepancy_baseline` (lib/baselines/discrepancy_baseline.py), the baseline from
"Emphasizing Complementary Samples for Non-literal Cross-modal Retrieval".

Same flags, defaults and choices (:33-50), same outputs (args.json, out.txt, err.txt, scores.csv unless --skip_train,
res.pkl {'df','agg_results'}, done) and the same record columns (:231-241).  The embedding pass is run_lemon's
(lemon_amd/cli_common.py); the four scores -- dis_x / dis_y second-order neighbours through the DB self-kNN cache
(:164-169,213-220), div_x / div_y k x k neighbour Gram sums (:221-226) -- are one lemon_discrepancy launch per split.

Extension flags --knn_k_sweep / --method_sweep: the grid of experiments.py:141-177 (four methods x eight knn_k) in ONE run --
embed, DB build and the self-kNN cache once, one lemon_discrepancy_ks launch per split for every (method, knn_k), then the
files of a single run per pair under <output_dir>/method=<m>/knn_k=<k>/ and <output_dir>/sweep.json.  Each pair's pred_score
has the bits of its own single run."""
import argparse
import copy
import json
import os
import pickle
import sys

import numpy as np
import pandas as pd
import torch

from .cli_common import add_eval_metrics_flag, add_extension_flags


METHODS = ("dis_x", "dis_y", "div_x", "div_y")


def build_parser():
    p = argparse.ArgumentParser(description="Baseline from ``Emphasizing Complementary Samples for Non-literal Cross-modal Retrieval``")
    p.add_argument("--exp_name", type=str)
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--dataset", type=str, default="cifar100",
                   choices=["cifar10", "cifar100", "flickr30k", "mscoco", "mimiccxr_caption", "mmimdb", "cifar10_full",
                            "cifar100_full", "mini_imagenet", "stanford_cars", "cc3m"])
    p.add_argument("--noise_type", type=str, default="real",
                   choices=["real", "asymmetric", "symmetric", "random", "noun", "cat"])
    p.add_argument("--method", type=str, default="dis_x", choices=list(METHODS))
    p.add_argument("--noise_level", type=float, default=0.4)
    p.add_argument("--clip_model", type=str, default="huggingface_clip", choices=["huggingface_clip", "biomed_clip"])
    p.add_argument("--knn_k", default=5, type=int)
    p.add_argument("--batch_size", default=128, type=int)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--data_seed", default=0, type=int)
    p.add_argument("--compr_dataset_size_limit", default=50000, type=int)
    p.add_argument("--custom_cifar_prompt", default=None)
    p.add_argument("--debug", action="store_true")
    p.add_argument("--skip_train", action="store_true")
    add_extension_flags(p)          # local weights / data (not in the reference)
    add_eval_metrics_flag(p)
    p.add_argument("--knn_k_sweep", default=None, type=str,
                   help="comma-separated knn_k values, e.g. 1,2,5,10,15,20,30,50 (the reference's grid, experiments.py:141-177): "
                        "embed, build the DB and its self-kNN cache and search ONCE at the largest, then write a run per value "
                        "-> <output_dir>/method=<m>/knn_k=<k>/ and <output_dir>/sweep.json; --knn_k is ignored")
    p.add_argument("--method_sweep", default=None, type=str,
                   help="comma-separated methods (dis_x,dis_y,div_x,div_y) or 'all': every method from the same search, laid out "
                        "as with --knn_k_sweep; --method is ignored.  With one of the two flags the other axis is --knn_k / --method")
    return p


def parse_method_sweep(text):
    """'div_x,dis_x,dis_x' -> ['div_x', 'dis_x']: the order given, de-duplicated; 'all' -> the four methods.  Refused
    (ValueError): an empty list, an unknown name."""
    parts = [t.strip() for t in str(text).split(",") if t.strip()]
    if not parts:
        raise ValueError("--method_sweep: the list is empty; expected comma-separated methods such as dis_x,div_y, or all")
    if parts == ["all"]:
        return list(METHODS)
    for t in parts:
        if t not in METHODS:
            raise ValueError(f"--method_sweep: unknown method {t!r}; expected some of {','.join(METHODS)}, or all")
    return list(dict.fromkeys(parts))


def sweep_axes(args):
    """(methods, ks) of a sweep run, None without either flag; the axis whose flag is absent is the single --method / --knn_k."""
    from .run_lemon import MAX_SWEEP_K, parse_k_sweep
    if args.knn_k_sweep is None and args.method_sweep is None:
        return None
    methods = parse_method_sweep(args.method_sweep) if args.method_sweep is not None else [args.method]
    if args.knn_k_sweep is not None:
        ks = parse_k_sweep(args.knn_k_sweep)
    elif 1 <= args.knn_k <= MAX_SWEEP_K:
        ks = [args.knn_k]
    else:
        raise ValueError(f"--method_sweep: --knn_k must lie in 1 .. {MAX_SWEEP_K}, got {args.knn_k}")
    return methods, ks


def main(argv=None):
    from .cli_common import run_with_tee
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        sweep_axes(args)
    except ValueError as e:
        parser.error(str(e))
    return run_with_tee(_run, args)


def _run(args):
    from .baselines import discrepancy_cache, discrepancy_scores, discrepancy_sweep
    from .cli_common import meta_columns, prepare
    from .neighbors import LemonDB
    from .pipeline import all_gather_rows

    sweep = sweep_axes(args)
    ctx = prepare(args)
    rank, world, device, sets = ctx.rank, ctx.world, ctx.device, ctx.sets
    emb = {"train": ctx.embed_split(sets["train"], "train")}
    n_train = len(sets["train"])
    sel = torch.from_numpy(np.asarray(ctx.train_indices_in_compr)).to(device)
    db = LemonDB(all_gather_rows(emb["train"][0], n_train)[sel], all_gather_rows(emb["train"][1], n_train)[sel], "cosine")  # :150-155
    names = ["val", "test"] if (args.debug or args.skip_train) else ["train", "val", "test"]
    cache = None
    if sweep is not None and any(m.startswith("dis") for m in sweep[0]):
        cache = discrepancy_cache(db, sweep[1][-1])          # the DB's own text neighbours (:165-169): once for the run
    frames, scores = [], []
    for sname in names:
        if sname not in emb:
            emb[sname] = ctx.embed_split(sets[sname], sname)
        e_img, e_txt, meta = emb[sname]
        n_total = len(sets[sname])
        # NOTE (:209): the train split searches k+1 and keeps ALL k+1 neighbours (no self-exclusion of the query here;
        # only the cache of second-order neighbours drops self, :167-169) -- lemon_discrepancy reproduces that
        if sweep is None:
            score = discrepancy_scores(db, e_img, e_txt, args.knn_k, args.method, is_train=(sname == "train"))
            host = all_gather_rows(score, n_total).cpu().numpy()
        else:
            score = discrepancy_sweep(db, e_img, e_txt, sweep[1], sweep[0], is_train=(sname == "train"), cache=cache)
            host = all_gather_rows(score.permute(2, 0, 1).contiguous(), n_total).cpu().numpy()      # [n_total, M, K]
        meta, flips = ctx.gather_meta(meta)
        if rank == 0:
            frames.append(pd.DataFrame(meta_columns(sname, n_total, meta, flips)))
            scores.append(host)
    torch.cuda.synchronize(device)
    if world > 1:
        torch.distributed.destroy_process_group()
    if rank != 0:
        return 0
    df = pd.concat(frames, ignore_index=True)
    scores = np.concatenate(scores)
    out_dir = ctx.out_dir
    layout = None
    if args.eval_metrics == "device":       # the rows of the validation set and of every split: uploaded once for the run
        from .cli_common import EvalLayout
        layout = EvalLayout(df, device)
    if sweep is None:
        df["pred_score"] = scores.astype(np.float64)
        _tail(args, df, out_dir, layout)
        return 0
    methods, ks = sweep
    results = {}
    for mi, m in enumerate(methods):
        for ti, k in enumerate(ks):
            out_mk = out_dir / f"method={m}" / f"knn_k={k}"
            out_mk.mkdir(exist_ok=True, parents=True)
            args_mk = copy.copy(args)
            args_mk.method, args_mk.knn_k, args_mk.output_dir = m, k, str(out_mk)
            with open(out_mk / "args.json", "w") as f:
                json.dump(vars(args_mk), f, default=str)
            df_mk = df.copy()
            df_mk["pred_score"] = scores[:, mi, ti].astype(np.float64)
            print(f"---- method = {m}, knn_k = {k} ----")
            res = _tail(args_mk, df_mk, out_mk, layout)
            results.setdefault(m, {})[str(k)] = {sset: {"AUROC": float(r["AUROC"]), "F1_optimal": float(r["F1_optimal"])}
                                                 for sset, r in res.items()}
    with open(out_dir / "sweep.json", "w") as f:
        json.dump({"methods": methods, "ks": ks, "results": results}, f, indent=1)
    with open(os.path.join(out_dir, "done"), "w") as f:
        f.write("done")
    return 0


def _tail(args, df, out_dir, layout=None):
    """Everything behind the per-sample scores: the files of a run (scores.csv unless --skip_train, res.pkl, done) and its
    metrics.  Returns agg_results.  layout: the EvalLayout of `df` with --eval_metrics device -- the metrics of the validation
    rows and of every split are one ops.eval_metrics call on the uploaded score; None: metrics.eval_metrics on the host."""
    from . import metrics as M
    if not args.skip_train:
        df.to_csv(out_dir / "scores.csv", index=False)
    prev = df.loc[df.sset == "val", "is_mislabel"].sum() / (df.sset == "val").sum()
    if layout is not None:
        selection_results = layout(torch.from_numpy(df["pred_score"].values.astype(np.float64)), prev)[1]
    else:
        df_val = df.query('sset == "val"')
        thress = M.eval_metrics(df_val["is_mislabel"], df_val["pred_score"], prevalence=prev)
        selection_results = {}
        for sset in df.sset.unique():
            sub = df.loc[df.sset == sset]
            selection_results[sset] = M.eval_metrics(sub["is_mislabel"], sub["pred_score"], prevalence=prev, fix_thress=thress)
    for sset in df.sset.unique():
        print(f"{sset}: AUROC {selection_results[sset]['AUROC']:.4f}  F1 {selection_results[sset]['F1_optimal']:.4f}")
    pickle.dump({"df": df, "agg_results": selection_results}, (out_dir / "res.pkl").open("wb"))
    with open(os.path.join(out_dir, "done"), "w") as f:
        f.write("done")
    return selection_results


if __name__ == "__main__":
    sys.exit(main())
