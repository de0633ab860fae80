"""Times the device k-means (lemon_amd/kmeans.py) on the GPU and writes one JSON document.

Per shape (n, C, d) and draw (seeded random unit vectors, initial centroids = data rows):
  * per-iteration time of assign / update / split (device events around `reps` back-to-back launches, after a warm-up);
  * the same assignment through IndexFlatL2(d).add(c).search(x, 1) -- what a fit without the dedicated kernel would call --
    measured in the same process, the two alternating;
  * whole-fit time of lemon_kmeans_train (host clock around enqueue + one synchronise) beside the same loop with the index
    search in place of the assign kernel;
  * at the small shape only, a float32 torch Lloyd on the CPU (16 threads) with the same niter.
The assign kernel's rate is 2 n C d flop over its time, quoted against the 157.3 TFLOP/s fp32-MFMA peak.

    python tools/kmeans_time.py --out profiles/kmeans/kmeans.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
SHAPES = [(102400, 100, 512, 20), (1024000, 1000, 768, 10)]       # (n, C, d, niter of the whole-fit timing)


def unit_rows(n, d, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=device, dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def index_assign(x, c):
    from lemon_amd import IndexFlatL2
    idx = IndexFlatL2(c.shape[1], c.device)
    idx.add(c)
    D, I = idx.search(x, 1)
    return I[:, 0].to(torch.int32), D[:, 0].contiguous()


def fit_with_index(x, init, niter):
    from lemon_amd import kmeans
    c = init.clone()
    for _ in range(niter):
        a, dist = index_assign(x, c)
        count, _ = kmeans.update(x, a, dist, c)
        kmeans.split_empty(c, count)
    return index_assign(x, c)[0]


def cpu_lloyd(x, init, niter):
    """float32 torch Lloyd on the host: expanded distances, index_add means (no split: no cluster empties on this input)"""
    c = init.clone()
    for _ in range(niter):
        d2 = (x * x).sum(1, keepdim=True) + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)
        a = d2.argmin(1)
        s = torch.zeros_like(c).index_add_(0, a, x)
        cnt = torch.bincount(a, minlength=c.shape[0]).clamp(min=1).to(torch.float32)
        c = s / cnt[:, None]
    return c


def one_draw(n, C, d, niter, seed, reps, device, with_cpu):
    from lemon_amd import kmeans
    x = unit_rows(n, d, seed, device)
    init = x[torch.from_numpy(kmeans.initial_rows(n, C, seed, 0)).to(device)].contiguous()
    a, dist = kmeans.assign(x, init)
    ai, di = index_assign(x, init)
    same = bool(torch.equal(a, ai) and torch.equal(dist.view(torch.int32), di.view(torch.int32)))
    c = init.clone()
    count, _ = kmeans.update(x, a, dist, c)                       # warm-up of every kernel below
    kmeans.split_empty(c, count)
    torch.cuda.synchronize()
    out = {"seed": seed, "assign_equals_index": same, "assign_ms": [], "index_assign_ms": []}
    for _ in range(3):                                            # alternate the two
        out["assign_ms"].append(event_ms(lambda: kmeans.assign(x, c), reps))
        out["index_assign_ms"].append(event_ms(lambda: index_assign(x, c), reps))
    out["update_ms"] = event_ms(lambda: kmeans.update(x, a, dist, c.clone()), reps)
    out["split_ms"] = event_ms(lambda: kmeans.split_empty(c, count), reps)
    best = min(out["assign_ms"])
    out["assign_tflops"] = 2.0 * n * C * d / (best * 1e-3) / 1e12
    out["assign_fraction_of_f32_mfma_peak"] = out["assign_tflops"] * 1e12 / PEAK_F32_MFMA
    fits = {"train_ms": [], "index_fit_ms": []}
    for _ in range(2):
        torch.cuda.synchronize(); t = time.perf_counter()
        kmeans.train(x, init, niter); torch.cuda.synchronize()
        fits["train_ms"].append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        fit_with_index(x, init, niter); torch.cuda.synchronize()
        fits["index_fit_ms"].append((time.perf_counter() - t) * 1e3)
    out.update(fits, fit_niter=niter)
    if with_cpu:
        torch.set_num_threads(16)
        xc, ic = x.cpu(), init.cpu()
        t = time.perf_counter()
        cpu_lloyd(xc, ic, niter)
        out["cpu_torch_f32_fit_ms"] = (time.perf_counter() - t) * 1e3
        out["cpu_threads"] = torch.get_num_threads()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--draws", type=int, default=3)
    ap.add_argument("--small_only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_time.py measures on the GPU: no HIP device is visible")
    device = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(device), "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12, "shapes": []}
    for n, C, d, niter in SHAPES[:1 if args.small_only else None]:
        reps = 20 if n <= 200000 else 5
        draws = [one_draw(n, C, d, niter, 100 + i, reps, device, with_cpu=(n <= 200000)) for i in range(args.draws)]
        key = [min(dr["assign_ms"]) for dr in draws]
        med = int(np.argsort(key)[len(key) // 2])
        for i, dr in enumerate(draws):
            dr["median_draw"] = (i == med)
        doc["shapes"].append({"n": n, "C": C, "d": d, "draws": draws})
        print(json.dumps({"n": n, "C": C, "d": d, "median": draws[med]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
