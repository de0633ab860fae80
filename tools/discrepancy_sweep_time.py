"""Time the discrepancy sweep on the GPU (diagnostic; writes profiles/discrepancy_sweep/discrepancy_sweep.json).

  (a) scores alone, on device-resident embeddings: n_db = 50 000, d = 512, nq = 5 000 and nq = 40 000 (the train split), the
      reference's eight ks and all four methods -- one discrepancy_cache + one discrepancy_sweep against the 32
      discrepancy_scores calls they replace.  Both sides include their searches.
  (b) whole runs: one `discrepancy_baseline --method_sweep all --knn_k_sweep ...` on a warm embedding cache against the 32 single
      `--method m --knn_k k` runs on the same cache, each run a fresh process, its wall time split into start-up + load / index
      build / self-kNN cache / scores / the rest by timers around the functions that do the work (synchronised, so GPU time lands
      where it is spent; a single run's self-kNN search is inside its scores).

  python tools/discrepancy_sweep_time.py [--repeats 5] [--part a|b|ab] [--nq 5000,40000] [--data_root synthetic:N] [--out DIR]
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
METHODS = ["dis_x", "dis_y", "div_x", "div_y"]
PHASES = ("startup_load_s", "index_build_s", "cache_s", "scores_s", "rest_s")
TAG = "DISC_SWEEP_TIME "


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "repeats": len(xs)}


def part_a(repeats, nq, n_db=50000, d=512):
    import torch
    from lemon_amd.baselines import discrepancy_cache, discrepancy_scores, discrepancy_sweep
    from lemon_amd.neighbors import LemonDB
    g = torch.Generator(device="cuda").manual_seed(nq)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    img_tr, txt_tr = unit(n_db), unit(n_db)
    db = LemonDB(img_tr, txt_tr, "cosine")
    is_train = nq > 5000                              # the large query set is the train split: the database's own rows
    q_img, q_txt = (img_tr[:nq], txt_tr[:nq]) if is_train else (unit(nq), unit(nq))

    def sweep():
        return discrepancy_sweep(db, q_img, q_txt, KS, METHODS, is_train=is_train, cache=discrepancy_cache(db, KS[-1]))

    def singles():
        return torch.stack([torch.stack([discrepancy_scores(db, q_img, q_txt, k, m, is_train=is_train) for k in KS]) for m in METHODS])

    a, b = sweep(), singles()                         # warm-up, and the two paths must agree bit for bit
    same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    times = {"cache_and_sweep": [], "32_discrepancy_scores": []}
    for _ in range(repeats):                          # interleaved, so that drift hits both alike
        for name, fn in (("cache_and_sweep", sweep), ("32_discrepancy_scores", singles)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return {"n_db": n_db, "d": d, "nq": nq, "is_train": is_train, "ks": KS, "methods": METHODS, "bit_identical": same,
            "seconds": {name: stats(v) for name, v in times.items()}}


# ---- (b): a child process runs the CLI with timers around the phases -----------------------------------------------------------
def child(argv, t_launch):
    import torch
    from lemon_amd import baselines, discrepancy_baseline, neighbors
    acc = dict.fromkeys(("index_build_s", "cache_s", "scores_s"), 0.0)
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
    baselines.discrepancy_cache = timed("cache_s", baselines.discrepancy_cache)
    baselines.discrepancy_scores = timed("scores_s", baselines.discrepancy_scores)
    baselines.discrepancy_sweep = timed("scores_s", baselines.discrepancy_sweep)
    rc = discrepancy_baseline.main(argv)
    total = time.time() - t_launch
    out = {"total_s": total, "startup_load_s": first_db[0] - t_launch, **acc}
    out["rest_s"] = total - sum(out[p] for p in PHASES if p != "rest_s")
    print(TAG + json.dumps(out), flush=True)
    return rc


def run_child(argv, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(argv), "--t_launch", repr(time.time())]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith(TAG)]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"run failed (rc={res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return json.loads(lines[-1][len(TAG):])


def part_b(repeats, data_root, limit):
    import pickle

    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        base = ["--dataset", "cifar10", "--noise_type", "asymmetric", "--data_root", data_root, "--clip_path", "random:tiny",
                "--embedding_cache", os.path.join(tmp, "cache")]
        run_child(["--output_dir", os.path.join(tmp, "warm"), *base, "--knn_k", "1"], limit)          # fills the cache
        sweeps, singles, sizes, same = [], [], None, None
        for r in range(repeats):
            sweeps.append(run_child(["--output_dir", os.path.join(tmp, f"sweep{r}"), *base, "--method_sweep", ",".join(METHODS),
                                     "--knn_k_sweep", ",".join(map(str, KS))], limit))
            per = [run_child(["--output_dir", os.path.join(tmp, f"single{r}_{m}_{k}"), *base, "--method", m, "--knn_k", str(k)], limit)
                   for m in METHODS for k in KS]
            singles.append({key: sum(p[key] for p in per) for key in per[0]})
            print(f"repeat {r}: sweep {sweeps[-1]['total_s']:.2f} s, 32 single runs {singles[-1]['total_s']:.2f} s", file=sys.stderr, flush=True)
            if sizes is None:
                load = lambda p: pickle.load(open(os.path.join(p, "res.pkl"), "rb"))["df"]
                df = load(os.path.join(tmp, f"single{r}_{METHODS[0]}_{KS[0]}"))
                sizes = {s: int((df.sset == s).sum()) for s in df.sset.unique()}
                same = all(np.array_equal(load(os.path.join(tmp, f"single{r}_{m}_{k}"))["pred_score"].values.view(np.uint64),
                                          load(os.path.join(tmp, f"sweep{r}", f"method={m}", f"knn_k={k}"))["pred_score"].values.view(np.uint64))
                           for m in METHODS for k in KS)
        keys = ("total_s",) + PHASES
        return {"data_root": data_root, "ks": KS, "methods": METHODS, "split_sizes": sizes, "bit_identical": bool(same),
                "sweep": {key: stats([s[key] for s in sweeps]) for key in keys},
                "32_single_runs": {key: stats([s[key] for s in singles]) for key in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--nq", default="5000,40000", help="query counts of (a); above 5 000 the queries are the database's own rows")
    ap.add_argument("--data_root", default="synthetic:2500", help="synthetic:N gives splits of 0.8 N / 0.1 N / 0.1 N")
    ap.add_argument("--limit", type=float, default=300.0, help="time limit of one run of (b), seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discrepancy_sweep"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--t_launch", type=float, default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(json.loads(args.child), args.t_launch)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "discrepancy_sweep.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    jobs = [("a", f"scores_alone_nq{nq}", lambda nq=nq: part_a(args.repeats, nq)) for nq in map(int, args.nq.split(","))]
    jobs.append(("b", "whole_runs", lambda: part_b(args.repeats, args.data_root, args.limit)))
    for part, key, fn in jobs:
        if part in args.part:
            res[key] = fn()
            print(json.dumps(res[key]), flush=True)
            with open(path, "w") as f:              # after every part: a part that runs out of time keeps the others' results
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
