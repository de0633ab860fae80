"""Time --eval_metrics device on the GPU (diagnostic; writes profiles/eval_metrics/eval_metrics.json).

  cell     the metrics of one cell -- the free validation rows, then train / val / test at the validation thresholds -- as one
           ops.eval_metrics call against the four metrics.eval_metrics calls of the same commit on the host, at the split
           sizes 250 / 2 000 / 250 and 5 000 / 40 000 / 5 000 (val / train / test); the device time includes the gather of
           the score by the uploaded row indices, the copy back and the dicts, the host time starts from numpy arrays
  fixed3m  a free segment of 250 rows and ONE fixed segment of 3 000 000 rows (one workgroup walks it), against
           metrics.eval_metrics(..., fix_thress=...) on the same rows
  sweep    tools/cell_sweep_time.py's phases of the 96-cell sweep (fresh processes, warm embedding cache) with
           --eval_metrics host and with --eval_metrics device: rest_s is the host tail the flag shortens
Times are recorded, not asserted: median, min .. max over the repeats after one warm-up; there is no pass mark, the host path
of the same commit is the yardstick.

  python tools/eval_metrics_time.py [--repeats 3] [--skip_sweep] [--data_root synthetic:2500] [--out DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CELL_SIZES = [(250, 2000, 250), (5000, 40000, 5000)]        # val, train, test


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "repeats": len(xs)}


def scores(n, seed):
    rng = np.random.default_rng(seed)
    y = rng.random(n) < 0.4
    return rng.standard_normal(n) + 1.5 * y, y


def timed(fn, repeats, sync):
    fn()                                           # warm-up: first launches, allocator, imports
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return stats(out)


def cell(sizes, repeats, dev):
    import pandas as pd
    import torch
    from lemon_amd import metrics as M
    from lemon_amd.cli_common import EvalLayout
    n_val, n_train, n_test = sizes
    score, y = scores(n_train + n_val + n_test, sum(sizes))
    df = pd.DataFrame({"sset": ["train"] * n_train + ["val"] * n_val + ["test"] * n_test, "is_mislabel": y, "pred_score": score})
    prev = df.loc[df.sset == "val", "is_mislabel"].sum() / (df.sset == "val").sum()
    layout, score_d = EvalLayout(df, dev), torch.from_numpy(score).to(dev)

    def host():
        val = df.query('sset == "val"')
        thress = M.eval_metrics(val["is_mislabel"], val["pred_score"], prevalence=prev)
        return {s: M.eval_metrics(df.loc[df.sset == s, "is_mislabel"], df.loc[df.sset == s, "pred_score"], prevalence=prev,
                                  fix_thress=thress) for s in df.sset.unique()}
    got, want = layout(score_d, prev)[1], host()
    same = all(got[s][k] == want[s][k] for s in want for k in want[s] if k not in ("AUROC", "AUPRC"))
    return {"val_train_test": list(sizes), "same_thresholds_and_counts": bool(same),
            "device_s": timed(lambda: layout(score_d, prev), repeats, lambda: torch.cuda.synchronize(dev)),
            "host_s": timed(host, repeats, lambda: None)}


def fixed3m(repeats, dev, n=3_000_000):
    import torch
    from lemon_amd import metrics as M, ops
    s_val, y_val = scores(250, 1)
    s_big, y_big = scores(n, 2)
    prev = y_val.sum() / 250
    score_d = torch.from_numpy(np.concatenate([s_val, s_big])).to(dev)
    y_d = torch.from_numpy(np.concatenate([y_val, y_big]).astype(np.uint8)).to(dev)
    segments = [(0, 250, prev, -1), (250, n, prev, 0)]
    thress = M.eval_metrics(y_val, s_val, prev)
    got, want = ops.eval_metrics(score_d, y_d, segments)[1], M.eval_metrics(y_big, s_big, prev, fix_thress=thress)
    same = all(got[k] == want[k] for k in want if k not in ("AUROC", "AUPRC"))
    return {"rows": n, "same_thresholds_and_counts": bool(same), "auroc_device_minus_host": got["AUROC"] - want["AUROC"],
            "device_s": timed(lambda: ops.eval_metrics(score_d, y_d, segments), repeats, lambda: torch.cuda.synchronize(dev)),
            "host_s": timed(lambda: M.eval_metrics(y_big, s_big, prev, fix_thress=thress), repeats, lambda: None)}


def sweep(repeats, data_root, limit):
    import cell_sweep_time as C
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        base = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", data_root, "--clip_path", "random:tiny",
                "--hparam_grid", "full", "--hparam_search", "device", "--lbfgs_polish", "device",
                "--embedding_cache", os.path.join(tmp, "cache")]
        for m in C.SUBSETS:                        # fills the cache: a subset run keys its validation split by m
            C.run_child(["--output_dir", os.path.join(tmp, f"warm{m}"), *base, "--subset_val_set", str(m), "--knn_k", "1",
                         "--skip_hparam_optim"], limit)
            print(f"cache warm for subset_val_set {m}", flush=True)
        for mode in ("host", "device"):
            runs = []
            for r in range(repeats):
                runs.append(C.run_child(["--output_dir", os.path.join(tmp, f"{mode}{r}"), *base, "--eval_metrics", mode,
                                         "--subset_val_set_sweep=" + ",".join(map(str, C.SUBSETS)), "--ablation_sweep",
                                         ",".join(C.ABLATIONS), "--knn_k_sweep", ",".join(map(str, C.KS))], limit))
                print(f"--eval_metrics {mode}, repeat {r}: total {runs[-1]['total_s']:.1f} s, rest {runs[-1]['rest_s']:.1f} s", flush=True)
            out[mode] = {key: stats([run[key] for run in runs]) for key in ("total_s",) + C.PHASES}
    return {"data_root": data_root, "cells": len(C.SUBSETS) * len(C.ABLATIONS) * len(C.KS), **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip_sweep", action="store_true")
    ap.add_argument("--data_root", default="synthetic:2500", help="synthetic:N gives splits of 0.8 N / 0.1 N / 0.1 N")
    ap.add_argument("--limit", type=float, default=600.0, help="time limit of one run of the sweep, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics"))
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats: at least 3, the spread is part of the record")
    import torch
    from lemon_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "cells": [], "fixed3m": None, "sweep": None}

    def save():
        with open(os.path.join(args.out, "eval_metrics.json"), "w") as f:
            json.dump(res, f, indent=1)
    for sizes in CELL_SIZES:
        res["cells"].append(cell(sizes, args.repeats, dev))
        save()
    res["fixed3m"] = fixed3m(args.repeats, dev)
    save()
    if not args.skip_sweep:
        res["sweep"] = sweep(args.repeats, args.data_root, args.limit)
        save()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
