"""Time the cell sweep on the GPU (diagnostic; writes profiles/cell_sweep/cell_sweep.json).

One `run_lemon --subset_val_set_sweep -1,10,50,100,500,1000 --ablation_sweep none,multimodal_baseline --knn_k_sweep
1,2,5,10,15,20,30,50` (the grid of experiments.py:203-205: 6 x 2 x 8 = 96 cells) against the 96 single `--subset_val_set m
--ablation a --knn_k k` runs it replaces, both on a warm embedding cache and with --hparam_search device --lbfgs_polish device,
each run a fresh process.  The wall time of a run is split by timers around the functions that do the work (synchronised, so
GPU time lands where it is spent):
  startup_s  process start -> cli_common.prepare returns (imports, device, model, dataset), without the embedding pass
  embed_s    the per-split embedding pass (here: loads from the warm cache)
  search_s   the DB build and the neighbour search
  tune_s     the local searches, the polish and the grid: maximize_metric and the ops launches made in front of it
  rest_s     everything else: the host tail -- frames, final score, metrics, res.pkl, the CSV

  python tools/cell_sweep_time.py [--repeats 2] [--data_root synthetic:2500] [--hparam_grid full|small] [--out DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = [1, 2, 5, 10, 15, 20, 30, 50]
SUBSETS = [-1, 10, 50, 100, 500, 1000]
ABLATIONS = ["none", "multimodal_baseline"]
PHASES = ("startup_s", "embed_s", "search_s", "tune_s", "rest_s")
MARK = "CELL_SWEEP_TIME "


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "repeats": len(xs)}


def child(argv, t_launch):
    import torch
    from lemon_amd import cli_common, metrics as M, neighbors, ops, run_lemon
    acc = dict.fromkeys(("prepare_s", "embed_s", "search_s", "tune_s"), 0.0)
    depth = {"tune_s": 0}
    prepared = []

    def timed(key, fn):
        def wrapper(*a, **kw):
            if depth.get(key, 0):                  # maximize_metric calls the ops: the outermost timer counts
                return fn(*a, **kw)
            depth[key] = 1
            if torch.cuda.is_initialized():
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                if torch.cuda.is_initialized():
                    torch.cuda.synchronize()
                acc[key] += time.perf_counter() - t0
                depth[key] = 0
        return wrapper

    plain_prepare = cli_common.prepare

    def prepare(args):
        ctx = plain_prepare(args)
        prepared.append(time.time())
        ctx.embed_split = timed("embed_s", ctx.embed_split)
        return ctx
    cli_common.prepare = prepare
    neighbors.LemonDB.__init__ = timed("search_s", neighbors.LemonDB.__init__)
    neighbors.LemonDB.neighbors = timed("search_s", neighbors.LemonDB.neighbors)
    for name in ("grid_f1", "grid_f1_ks", "local_search", "lbfgs_polish"):
        setattr(ops, name, timed("tune_s", getattr(ops, name)))
    M.maximize_metric = timed("tune_s", M.maximize_metric)
    rc = run_lemon.main(argv)
    total = time.time() - t_launch
    out = {"total_s": total, "startup_s": prepared[0] - t_launch, "embed_s": acc["embed_s"], "search_s": acc["search_s"],
           "tune_s": acc["tune_s"]}
    out["rest_s"] = total - sum(out[p] for p in PHASES if p != "rest_s")
    print(MARK + json.dumps(out), flush=True)
    return rc


def run_child(argv, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(argv), "--t_launch", repr(time.time())]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith(MARK)]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"run failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return json.loads(lines[-1][len(MARK):])


def measure(repeats, data_root, hparam_grid, limit, save):
    import pickle
    flag = lambda m: f"--subset_val_set_sweep={m}" if isinstance(m, str) else ["--subset_val_set", str(m)]
    with tempfile.TemporaryDirectory() as tmp:
        base = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", data_root, "--clip_path", "random:tiny",
                "--hparam_grid", hparam_grid, "--hparam_search", "device", "--lbfgs_polish", "device",
                "--embedding_cache", os.path.join(tmp, "cache")]
        for m in SUBSETS:                          # fills the cache: a subset run keys its validation split by m
            run_child(["--output_dir", os.path.join(tmp, f"warm{m}"), *base, *flag(m), "--knn_k", "1", "--skip_hparam_optim"], limit)
        sweeps, singles, res = [], [], {}
        for r in range(repeats):
            out = os.path.join(tmp, f"sweep{r}")
            sweeps.append(run_child(["--output_dir", out, *base, flag(",".join(map(str, SUBSETS))), "--ablation_sweep",
                                     ",".join(ABLATIONS), "--knn_k_sweep", ",".join(map(str, KS))], limit))
            print(f"repeat {r}: sweep {sweeps[-1]['total_s']:.1f} s", flush=True)
            per, agree = [], True
            for m in SUBSETS:
                for a in ABLATIONS:
                    for k in KS:
                        one = os.path.join(tmp, "single")
                        per.append(run_child(["--output_dir", one, *base, *flag(m), "--ablation", a, "--knn_k", str(k)], limit))
                        load = lambda d: pickle.load(open(os.path.join(d, "res.pkl"), "rb"))["agg_results"]["know_val_labels"]
                        cell = load(os.path.join(out, f"subset_val_set={m}", f"ablation={a}", f"knn_k={k}"))
                        agree = agree and cell["selected_val"] == load(one)["selected_val"] and cell["thres"] == load(one)["thres"]
                print(f"repeat {r}: subset_val_set {m}: {sum(p['total_s'] for p in per):.1f} s of single runs so far", flush=True)
            singles.append({key: sum(p[key] for p in per) for key in per[0]})
            df = pickle.load(open(os.path.join(out, "subset_val_set=-1", "ablation=none", f"knn_k={KS[0]}", "res.pkl"), "rb"))["df"]
            cells = json.load(open(os.path.join(out, "cell_sweep.json")))["cells"]
            leaf = os.path.getsize(os.path.join(out, "subset_val_set=-1", "ablation=none", f"knn_k={KS[-1]}", "res.pkl"))
            keys = ("total_s",) + PHASES
            res = {"data_root": data_root, "hparam_grid": hparam_grid, "modes": "--hparam_search device --lbfgs_polish device",
                   "subsets": SUBSETS, "ablations": ABLATIONS, "ks": KS, "cells": len(cells),
                   "split_sizes": {s: int((df.sset == s).sum()) for s in df.sset.unique()},
                   "same_selected_val_and_thres": bool(agree), "all_cells_ok": all(c["status"] == "ok" for c in cells),
                   "largest_leaf_res_pkl_bytes": int(leaf),
                   "sweep": {key: stats([s[key] for s in sweeps]) for key in keys},
                   "single_runs": {key: stats([s[key] for s in singles]) for key in keys}}
            res["sweep_rest_share"] = res["sweep"]["rest_s"]["median"] / res["sweep"]["total_s"]["median"]
            save(res)                              # after every repeat: a run that is cut short keeps the repeats it finished
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--data_root", default="synthetic:2500", help="synthetic:N gives splits of 0.8 N / 0.1 N / 0.1 N")
    ap.add_argument("--hparam_grid", default="full", choices=["full", "small"])
    ap.add_argument("--limit", type=float, default=600.0, help="time limit of one run, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_sweep"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--t_launch", type=float, default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(json.loads(args.child), args.t_launch)
    if args.repeats < 2:
        ap.error("--repeats: at least 2, the spread is part of the record")
    os.makedirs(args.out, exist_ok=True)

    def save(res):
        with open(os.path.join(args.out, "cell_sweep.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(measure(args.repeats, args.data_root, args.hparam_grid, args.limit, save)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
