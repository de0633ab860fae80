"""Times the kNN self-join at the embedding widths of the wide CLIP towers (ViT-H/14, g/14: 1024; bigG/14: 1280) on the GPU and
writes one JSON document.

Per width d, unit-norm randn data generated on the device, n = nq = 262 144, k = 51, inner product, three configurations:
  * f32        the fp32 scan                                     (algo 1)
  * stream     the streaming fp16 filter, k_scan_bf16            (algo 2, wide filter off)
  * wide       the Q-stationary fp16 filter, k_scan_f16_qsw      (algo 2, wide filter on)
Each gets one warm-up call, then five timed calls; the timed rounds alternate the three configurations, so that clock drift and
other tenants of the host hit them alike.  The figure is the in-library kernel time (set_profiling / profile_read: device events
around every scan launch, the final exact re-rank included); the wall time of the call (device events around index.search) is
recorded beside it.  All three must return bit-equal (D, I), or the run fails.

Run discipline: the driver itself never touches the GPU.  Every width is one child process under its own `timeout`; a child that
fails, faults or runs out of time ends the run and nothing further is started.

    python tools/knn_wide_time.py --out profiles/knn_wide/knn_wide.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("f32", 1, False), ("stream", 2, False), ("wide", 2, True)]       # (name, algo, wide filter)
EXPECT_KERNEL = {"f32": "scan_f32", "stream": "scan_bf16", "wide": "qsw"}


def gpu_clocks():
    """Current shader / memory clock as the driver reports them (read-only query; None when the tool is not there)."""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower()}
    except Exception:
        return None


def child(d, n, k, rounds, out_path):
    import torch
    import lemon_amd as hip
    if not torch.cuda.is_available():
        raise SystemExit("knn_wide_time.py measures on the GPU: no HIP device is visible")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000 + d)
    X = hip.normalize_vectors(torch.randn(n, d, generator=g, device=dev))
    idxs, res = {}, {}
    for name, algo, wide in CONFIGS:
        idx = hip.IndexFlatIP(d)
        idx.set_algo(algo)
        idx.set_wide_filter(wide)
        idx.add(X)
        D, I = idx.search(X, k)                                 # warm-up: code objects, workspaces, the 16-bit copy
        torch.cuda.synchronize()
        kern = idx.last_scan_kernel()
        if kern != EXPECT_KERNEL[name]:
            raise SystemExit(f"d={d} {name}: served by {kern!r}, expected {EXPECT_KERNEL[name]!r}")
        idxs[name] = idx
        res[name] = {"kernel": kern, "info": idx.last_search_info(), "kernel_ms": [], "call_ms": [], "launches": [], "clocks": []}
        if name == "f32":
            D0, I0 = D, I
        elif not (torch.equal(D.view(torch.int32), D0.view(torch.int32)) and torch.equal(I, I0)):
            raise SystemExit(f"d={d}: {name} and f32 return different (D, I)")
        del D, I
    for _ in range(rounds):
        for name, _, _ in CONFIGS:
            idx = idxs[name]
            idx.set_profiling(True)
            idx.profile_read()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            idx.search(X, k)
            b.record()
            b.synchronize()
            pr = idx.profile_read()
            idx.set_profiling(False)
            res[name]["kernel_ms"].append(pr["kernel_ms"])
            res[name]["launches"].append(pr["launches"])
            res[name]["call_ms"].append(a.elapsed_time(b))
            res[name]["clocks"].append(gpu_clocks())
    for name, r in res.items():
        ms = r["kernel_ms"]
        r["median_ms"] = statistics.median(ms)
        r["spread_ms"] = max(ms) - min(ms)
        r["tflops"] = 2.0 * n * n * d / (r["median_ms"] * 1e-3) / 1e12
    doc = {"d": d, "n": n, "nq": n, "k": k, "metric": "ip", "device": torch.cuda.get_device_name(dev), "bit_equal": True, "configs": res}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({"d": d, **{nm: [round(r["median_ms"], 2), round(r["spread_ms"], 2)] for nm, r in res.items()}}), flush=True)


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--widths", default="1024,1280")
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--k", type=int, default=51)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step_timeout", type=int, default=420, help="seconds one width may take")
    ap.add_argument("--commit", default=None, help="recorded as is (default: git rev-parse of the tree)")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.n, args.k, args.rounds, args.out)
        return 0
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    doc = {"commit": args.commit or commit(), "rounds": args.rounds, "widths": []}
    for d in [int(w) for w in args.widths.split(",")]:
        part = f"{out}.d{d}.part"
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(d),
               "--n", str(args.n), "--k", str(args.k), "--rounds", str(args.rounds), "--out", part]
        rc = subprocess.call(cmd)
        if rc != 0:                                            # a failure, a fault or the time limit: nothing further is started
            print(f"knn_wide_time: width {d} ended with status {rc}; stopping", file=sys.stderr)
            return rc
        with open(part) as f:
            doc["widths"].append(json.load(f))
        os.remove(part)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
