"""The tail of a run_lemon run in a straight line, kept as test code: everything behind the per-sample record -- the d1
ablation, the hyper-parameter search, the final score, the metrics and the files -- on ONE frame, with the frame's own arrays
uploaded here and ops.grid_f1 / ops.local_search / ops.lbfgs_polish called directly.  It shares no code with the cell loop of
run_lemon.py (only its constants), so that "a cell equals plain_tail on its own record" also catches an error that every path
through that loop would have in common."""
import os
import pickle

import numpy as np

from lemon_amd.run_lemon import FORCE_MASKS, SEARCH_METHODS, SEARCH_STARTS

REC_COLUMNS = ("D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m")


def device_rec(frame, device):
    """the record of a frame on `device`: the neighbour columns stacked to float32 [n, k], d_1 as float32 [n]"""
    import torch
    return {c: torch.from_numpy(np.stack(frame[c].values).astype(np.float32)).to(device) for c in REC_COLUMNS} | \
           {"d_1": torch.from_numpy(frame["d_1"].values.astype(np.float32)).to(device)}


def plain_tail(args, df, out_dir, device):
    """-> agg_results' entry (None with --real_dataset / --skip_hparam_optim); writes res.pkl, know_val_labels_scores.csv,
    need_hparam_optim and done into `out_dir` (a pathlib.Path).  `df` is written to."""
    from lemon_amd import metrics as M, ops
    sel_res = None
    if "d1" in args.ablation:
        df["d_1"] = 0.0

    if args.real_dataset or args.skip_hparam_optim:
        res = {"df": df}
    else:
        df_val = df.query('sset == "val"')
        rec_val = device_rec(df_val, device)
        y_val = df_val["is_mislabel"].values
        score_fn = lambda hp: ops.lemon_score(rec_val, hp).cpu().numpy()
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
                grid = {"beta": np.arange(0, 100.01, 5), "gamma": np.arange(0, 100.01, 5), "tau_1": [0, 1, 5, 10],
                        "tau_2": [0, 1, 5, 10]} if args.hparam_grid == "full" else \
                       {"beta": [0, 5, 10], "gamma": [0, 5, 10], "tau_1": [0, 1], "tau_2": [0, 5]}
                force_zero, force_one = (list(names) for names in FORCE_MASKS[args.ablation])
                local_search = lbfgs_polish = None
                if args.hparam_search == "device":
                    local_search = lambda x0s, methods, fz, fo: ops.local_search(rec_val, y_val, x0s, methods, fz, fo)
                if args.lbfgs_polish == "device":
                    lbfgs_polish = lambda x0s, fz, fo: [x for x, _ in ops.lbfgs_polish(rec_val, y_val, x0s, fz, fo)]
                rec_lbfgs = None if lbfgs_polish is not None else \
                    {c: (df_val[c].values if c == "d_1" else np.stack(df_val[c].values)) for c in ("d_1",) + REC_COLUMNS}
                best, best_f1, best_thres = M.maximize_metric(
                    score_fn, y_val, grid, SEARCH_STARTS, M.optimize_f1_efficient, {}, scipy_methods=SEARCH_METHODS,
                    local_search=local_search, lbfgs_polish=lbfgs_polish,
                    force_zero=force_zero, force_one=force_one, rec_for_lbfgs=rec_lbfgs,
                    lbfgs_device=str(device) if args.lbfgs_device == "cuda" else "cpu",
                    batch_grid=lambda hps: ops.grid_f1(rec_val, y_val, [[hp[n] for n in M.HP_NAMES] for hp in hps])[0])
            sel_res = dict(zip(M.HP_NAMES, best))
            sel_res.update(thres=best_thres, selected_val=best_f1)
        s, dn, dm = ops.lemon_score(device_rec(df, device), sel_res, return_dn=True)
        df[f"{crit}_pred_score"] = s.cpu().numpy()
        df[f"{crit}_d_n"], df[f"{crit}_d_m"] = dn.cpu().numpy(), dm.cpu().numpy()
        df_val = df.query('sset == "val"')
        prev = df.loc[df.sset == "val", "is_mislabel"].sum() / (df.sset == "val").sum()
        thress = M.eval_metrics(df_val["is_mislabel"], df_val[f"{crit}_pred_score"], prevalence=prev)
        for sset in df.sset.unique():
            sub = df.loc[df.sset == sset]
            sel_res[sset] = M.eval_metrics(sub["is_mislabel"], sub[f"{crit}_pred_score"], prevalence=prev,
                                           fix_thress=thress)
        df[["sset", "idx", "actual_label", "noisy_label", "is_mislabel", f"{crit}_pred_score"]].rename(
            columns={f"{crit}_pred_score": "pred_score"}).to_csv(out_dir / f"{crit}_scores.csv")
        res = {"df": df, "agg_results": {crit: sel_res}}

    pickle.dump(res, (out_dir / "res.pkl").open("wb"))
    if args.skip_hparam_optim:
        with open(os.path.join(out_dir, "need_hparam_optim"), "w") as f:
            f.write("need_hparam_optim")
    with open(os.path.join(out_dir, "done"), "w") as f:
        f.write("done")
    return sel_res
