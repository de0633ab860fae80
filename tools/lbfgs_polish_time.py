"""Time the LBFGS polish of one hyper-parameter search, the torch path against the one-launch path, in one process
(diagnostic; writes profiles/hparam_search/lbfgs_polish.json).  Recorded, not asserted.

  torch   metrics._torch_lbfgs on the device for the four start points, as maximize_metric runs it with --lbfgs_polish host
          and --lbfgs_device cuda: the record goes to the device once per k, then 20 optimizer.step calls a start, every
          closure evaluation a handful of torch kernels plus autograd
  device  ops.lbfgs_polish: every polish in one lemon_lbfgs_polish launch and one copy back (--lbfgs_polish device)

Sizes (n, k) = (250, 50) and (5 000, 50), each for one k and for the sweep's eight ks (the torch path then runs eight times, on
the prefix records).  Interleaved repeats, median and spread; nfev, nit and status of every device polish; how many of the two
paths' candidates are finite.  The two paths do not return the same candidates and are not expected to.

  python tools/lbfgs_polish_time.py [--repeats 5] [--sizes 250,5000] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KS = [1, 2, 5, 10, 15, 20, 30, 50]
STARTS = [[0] * 6, [0.5] * 6, [1] * 6, [10] * 6]


def measure(n, kmax, ks, repeats):
    import numpy as np
    import torch
    from hparam_search_time import record, stats
    from lemon_amd import metrics as M, ops
    from lemon_amd.neighbors import prefix_record
    rec, y = record(n, kmax)
    host = {k: {key: v.cpu().numpy().astype(np.float64 if key == "d_1" else np.float32) for key, v in prefix_record(rec, k).items()}
            for k in ks}

    def torch_path():
        out = []
        for k in ks:                                   # maximize_metric: the record of this k to the device, then the four starts
            rec_t = {key: torch.as_tensor(v, dtype=torch.float64 if key == "d_1" else torch.float32).to("cuda") for key, v in host[k].items()}
            out.append([M._torch_lbfgs(rec_t, y, x0, (), ()) for x0 in STARTS])
        return out

    def device_path():
        return ops.lbfgs_polish(rec, y, STARTS, ks=ks, return_info=True)

    t, d = torch_path(), device_path()                 # warm-up
    times = {"torch": [], "device": []}
    for _ in range(repeats):                           # interleaved, so that drift hits both alike
        for name, fn in (("torch", torch_path), ("device", device_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            print(f"  n={n} ks={len(ks)} {name}: {times[name][-1]:.4f} s", file=sys.stderr, flush=True)
    return {"n": n, "kmax": kmax, "ks": list(ks), "polishes": len(ks) * len(STARTS),
            "finite_candidates": {"torch": int(sum(bool(np.all(np.isfinite(c))) for per_k in t for c in per_k)),
                                  "device": int(sum(r[1] == 0 for per_k in d for r in per_k))},
            "device_nfev": {str(k): [int(r[3]) for r in per_k] for k, per_k in zip(ks, d)},
            "device_nit": {str(k): [int(r[4]) for r in per_k] for k, per_k in zip(ks, d)},
            "seconds": {name: stats(v) for name, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="250,5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hparam_search"))
    args = ap.parse_args()
    import torch
    runs = []
    for n in [int(t) for t in args.sizes.split(",")]:
        for ks in ([50], KS):
            r = measure(n, 50, ks, args.repeats)
            print(json.dumps({k: r[k] for k in ("n", "ks", "finite_candidates", "seconds")}), flush=True)
            runs.append(r)
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "lbfgs_polish.json"), "w") as f:      # after every size: a cut-off run keeps its part
                json.dump({"device": torch.cuda.get_device_name(0), "order": "for each k, for each x0", "starts": STARTS,
                           "outer_steps": 20, "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
