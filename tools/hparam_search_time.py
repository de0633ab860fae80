"""Time the local searches of one maximize_metric call, host path against device path, in one process (diagnostic; writes
profiles/hparam_search/hparam_search.json).  Recorded, not asserted.

  host    scipy.optimize.minimize from the four start points with Powell and Nelder-Mead; every objective evaluation is one
          ops.lemon_score launch, a device -> host copy and a fminbound in numpy (what --hparam_search host runs)
  device  ops.local_search: all searches in one lemon_hparam_search launch and one copy back (--hparam_search device)
  lbfgs   the SoftMargin / LBFGS polish of the four starts on the device, timed on its own (it is not part of either path)

Sizes (n, k) = (250, 50) and (5 000, 50), each for one k and for the sweep's eight ks (the host path then runs eight times, on
the prefix records).  Interleaved repeats, median and spread; the nfev of every search; whether the two paths returned the
same bits.

  python tools/hparam_search_time.py [--repeats 5] [--sizes 250,5000] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = [1, 2, 5, 10, 15, 20, 30, 50]
STARTS = [[0] * 6, [0.5] * 6, [1] * 6, [10] * 6]
METHODS = ("Powell", "Nelder-Mead")


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "repeats": len(xs)}


def record(n, kmax, seed=0):
    """a record whose scores depend on the label: mislabelled samples sit further out, with overlap"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    y = (rng.uniform(size=n) < 0.4).astype(np.uint8)
    shift = y.astype(np.float64)
    rec = {"d_1": (rng.normal(0.55, 0.12, n) + 0.10 * shift).astype(np.float32)}
    for side in "nm":
        rec["D_" + side] = np.sort(rng.uniform(0.05, 1.2, (n, kmax)), axis=1).astype(np.float32)
        rec["dists_tr_" + side] = rng.uniform(0.2, 1.4, (n, kmax)).astype(np.float32)
        rec["dists_" + side] = (rng.normal(0.7, 0.15, (n, kmax)) + 0.12 * shift[:, None]).astype(np.float32)
    return {k: torch.from_numpy(v).cuda() for k, v in rec.items()}, y


def measure(n, kmax, ks, repeats):
    import numpy as np
    import torch
    from scipy.optimize import minimize
    from lemon_amd import metrics as M, ops
    from lemon_amd.neighbors import prefix_record
    rec, y = record(n, kmax)
    prefixes = {k: {key: v.contiguous() for key, v in prefix_record(rec, k).items()} for k in ks}

    def objective_of(k):
        def objective(x):
            score = ops.lemon_score(prefixes[k], M.unpack_vector(x)).cpu().numpy()
            if not np.all(np.isfinite(score)):
                return 0.0
            return -M.optimize_f1_efficient(y, score)
        return objective

    def host():
        out = []
        for k in ks:
            f = objective_of(k)
            out.append([minimize(f, x0, method=m, options={}) for x0 in STARTS for m in METHODS])
        return [[(r.x, r.fun, r.nfev, r.nit, r.status) for r in per_k] for per_k in out]

    def device():
        return ops.local_search(rec, y, STARTS, METHODS, ks=ks, return_info=True)

    def lbfgs():
        for k in ks:
            rec_t = {key: (v.double() if key == "d_1" else v.float()) for key, v in prefixes[k].items()}
            f = objective_of(k)
            for x0 in STARTS:
                cand = M._torch_lbfgs(rec_t, y, x0, (), ())
                if np.all(np.isfinite(cand)):
                    f(cand)

    h, d = host(), device()                       # warm-up, and the comparison
    same = all(np.array_equal(np.asarray(a[0], np.float64).view(np.int64), np.asarray(b[0], np.float64).view(np.int64))
               and a[1] == b[1] and tuple(a[2:]) == tuple(b[2:]) for hk, dk in zip(h, d) for a, b in zip(hk, dk))
    lbfgs()
    times = {"host": [], "device": [], "lbfgs": []}
    for _ in range(repeats):                      # interleaved, so that drift hits all alike
        for name, fn in (("host", host), ("device", device), ("lbfgs", lbfgs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            print(f"  n={n} ks={len(ks)} {name}: {times[name][-1]:.3f} s", file=sys.stderr, flush=True)
    return {"n": n, "kmax": kmax, "ks": list(ks), "searches": len(ks) * len(STARTS) * len(METHODS), "bit_identical": bool(same),
            "nfev": {str(k): [int(r[2]) for r in per_k] for k, per_k in zip(ks, d)},
            "nfev_host": {str(k): [int(r[2]) for r in per_k] for k, per_k in zip(ks, h)},
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
            print(json.dumps({k: r[k] for k in ("n", "ks", "bit_identical", "seconds")}), flush=True)
            runs.append(r)
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "hparam_search.json"), "w") as f:     # after every size: a cut-off run keeps its part
                json.dump({"device": torch.cuda.get_device_name(0), "order": "for each k, for each x0, for each method",
                           "starts": STARTS, "methods": list(METHODS), "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
