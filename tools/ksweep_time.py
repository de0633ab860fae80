"""Time the knn_k sweep on the GPU (diagnostic; writes profiles/ksweep/ksweep.json).

  (a) grid alone: ops.grid_f1_ks at n = 5 000, kmax = 50, the reference's eight ks and the full 7 056-row grid, against the
      path without it: eight ops.grid_f1 calls on contiguous prefixes of the same record.
  (b) whole sweep: one `run_lemon --knn_k_sweep` on a warm embedding cache against eight single `--knn_k` runs on the same
      cache, each run a fresh process, its wall time split into start-up + load / index build / neighbours / grid / scipy
      searches / the rest by timers around the functions that do the work (synchronised, so GPU time lands where it is spent).

  python tools/ksweep_time.py [--repeats 5] [--part a|b|ab] [--data_root synthetic:N] [--hparam_grid full|small] [--out DIR]
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
PHASES = ("startup_load_s", "index_build_s", "neighbours_s", "grid_s", "scipy_searches_s", "rest_s")


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "repeats": len(xs)}


def part_a(repeats):
    import numpy as np
    import torch
    from lemon_amd import metrics as M, ops
    from lemon_amd.neighbors import prefix_record
    n, kmax = 5000, 50
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda")
    y = (rnd(n) < 0.4).cpu().numpy()
    rec = {"d_1": rnd(n) + torch.as_tensor(y, device="cuda") * 0.1, "D_n": -rnd(n, kmax), "dists_tr_n": rnd(n, kmax),
           "dists_n": rnd(n, kmax), "D_m": -rnd(n, kmax), "dists_tr_m": rnd(n, kmax), "dists_m": rnd(n, kmax)}
    grid = {"beta": np.arange(0, 100.01, 5), "gamma": np.arange(0, 100.01, 5), "tau_1": [0, 1, 5, 10], "tau_2": [0, 1, 5, 10]}
    hps = [[hp[name] for name in M.HP_NAMES] for hp in M.grid_points(grid)]

    def sweep():
        return ops.grid_f1_ks(rec, y, hps, KS)

    def eight():
        out = [ops.grid_f1(prefix_record(rec, k), y, hps) for k in KS]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    a, b = sweep(), eight()                       # warm-up, and the two paths must agree bit for bit
    same = all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(a, b))
    times = {"grid_f1_ks": [], "eight_grid_f1": []}
    for _ in range(repeats):                      # interleaved, so that drift hits both alike
        for name, fn in (("grid_f1_ks", sweep), ("eight_grid_f1", eight)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return {"n": n, "kmax": kmax, "ks": KS, "G": len(hps), "bit_identical": bool(same),
            "seconds": {name: stats(v) for name, v in times.items()}}


# ---- (b): a child process runs run_lemon with timers around the phases ----------------------------------------------------------
def child(argv, t_launch):
    import torch
    from lemon_amd import metrics as M, neighbors, ops, run_lemon
    acc = dict.fromkeys(("index_build_s", "neighbours_s", "grid_s", "search_total_s"), 0.0)
    first_db = []

    def timed(key, fn, mark=None):
        def wrapper(*a, **kw):
            if mark is not None and not mark:
                mark.append(time.time())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            acc[key] += time.perf_counter() - t0
            return out
        return wrapper
    neighbors.LemonDB.__init__ = timed("index_build_s", neighbors.LemonDB.__init__, first_db)
    neighbors.LemonDB.neighbors = timed("neighbours_s", neighbors.LemonDB.neighbors)
    ops.grid_f1 = timed("grid_s", ops.grid_f1)
    ops.grid_f1_ks = timed("grid_s", ops.grid_f1_ks)
    M.maximize_metric = timed("search_total_s", M.maximize_metric)
    rc = run_lemon.main(argv)
    total = time.time() - t_launch
    grid_inside = acc["grid_s"] if "--knn_k_sweep" not in argv else 0.0     # the sweep's grid call runs in front of the searches
    out = {"total_s": total, "startup_load_s": first_db[0] - t_launch, "index_build_s": acc["index_build_s"],
           "neighbours_s": acc["neighbours_s"], "grid_s": acc["grid_s"], "scipy_searches_s": acc["search_total_s"] - grid_inside}
    out["rest_s"] = total - sum(out[p] for p in PHASES if p != "rest_s")
    print("KSWEEP_TIME " + json.dumps(out), flush=True)
    return rc


def run_child(argv, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(argv), "--t_launch", repr(time.time())]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("KSWEEP_TIME ")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"run failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return json.loads(lines[-1][len("KSWEEP_TIME "):])


def part_b(repeats, data_root, hparam_grid, limit):
    with tempfile.TemporaryDirectory() as tmp:
        base = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", data_root, "--clip_path", "random:tiny",
                "--hparam_grid", hparam_grid, "--embedding_cache", os.path.join(tmp, "cache")]
        run_child(["--output_dir", os.path.join(tmp, "warm"), *base, "--knn_k", "1", "--skip_hparam_optim"], limit)   # fills the cache
        sweeps, singles, sizes = [], [], None
        for r in range(repeats):
            sweeps.append(run_child(["--output_dir", os.path.join(tmp, f"sweep{r}"), *base, "--knn_k_sweep",
                                     ",".join(map(str, KS))], limit))
            per_k = [run_child(["--output_dir", os.path.join(tmp, f"single{r}_{k}"), *base, "--knn_k", str(k)], limit) for k in KS]
            singles.append({key: sum(p[key] for p in per_k) for key in per_k[0]})
            if sizes is None:
                import pickle
                df = pickle.load(open(os.path.join(tmp, f"single{r}_{KS[0]}", "res.pkl"), "rb"))["df"]
                sizes = {s: int((df.sset == s).sum()) for s in df.sset.unique()}
                sel = json.load(open(os.path.join(tmp, f"sweep{r}", "k_selection.json")))
                agree = all(pickle.load(open(os.path.join(tmp, f"single{r}_{k}", "res.pkl"), "rb"))["agg_results"]["know_val_labels"]
                            ["selected_val"] == sel["per_k"][str(k)]["selected_val"] for k in KS)
        keys = ("total_s",) + PHASES
        return {"data_root": data_root, "hparam_grid": hparam_grid, "ks": KS, "split_sizes": sizes, "same_selected_val": bool(agree),
                "sweep": {key: stats([s[key] for s in sweeps]) for key in keys},
                "eight_single_runs": {key: stats([s[key] for s in singles]) for key in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--data_root", default="synthetic:50000", help="synthetic:N gives splits of 0.8 N / 0.1 N / 0.1 N")
    ap.add_argument("--hparam_grid", default="full", choices=["full", "small"])
    ap.add_argument("--limit", type=float, default=600.0, help="time limit of one run of (b), seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksweep"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--t_launch", type=float, default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(json.loads(args.child), args.t_launch)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ksweep.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    for part, key, fn in (("a", "grid_alone", lambda: part_a(args.repeats)),
                          ("b", "whole_sweep", lambda: part_b(args.repeats, args.data_root, args.hparam_grid, args.limit))):
        if part in args.part:
            res[key] = fn()
            print(json.dumps(res[key]), flush=True)
            with open(path, "w") as f:              # after every part: a part that runs out of time keeps the other's result
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
