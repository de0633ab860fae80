"""Time the metric sweep on the GPU (diagnostic; writes profiles/dist_sweep/dist_sweep.json).

Two legs, interleaved repeat by repeat on the same device so that drift hits both alike, builds included in both (and timed
apart from the neighbour calls, with a device synchronisation between):
  two_dbs   what two runs do between them: LemonDB(cosine) + neighbors, then LemonDB(euclidean) + neighbors
  one_db    LemonDB(("cosine", "euclidean")) + ONE neighbors_metrics call (margin 4), its fallback -- and the L2 pair the
            fallback builds on first need -- included
on device-resident synthetic embeddings of three families: random unit rows, unit rows around prototypes (a mixture, noise of
length 0.3), and a class dataset (random images, the text side 100 prompts repeated: every text list is one tie, so every row
falls back -- the sweep's worst case).  Per shape also: the share of rows certified per side at margin 1, 4 and 8, the rows that fall back, and the time
of the fallback alone (the L2 neighbours of just those rows on a pair that is already built).  The records of both legs are
compared bit for bit once per shape.

Shapes: small = 40 000 rows, 50 000 queries (the database's own rows first, drop_self), d = 512, k = 50;
        large = 1 000 000 rows, a 65 536-query slice, d = 768, k = 50 (the L2 scan at this pitch is the older QS2 kernel).

  python tools/dist_sweep_time.py [--repeats 5] [--shapes small,large] [--families random,mixture,class] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"small": dict(n_db=40000, nq=50000, d=512, k=50, own_rows=40000),
          "large": dict(n_db=1000000, nq=65536, d=768, k=50, own_rows=0)}
REC = ("d_1", "D_n", "dists_n", "dists_tr_n", "D_m", "dists_m", "dists_tr_m", "I_n", "I_m")


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "repeats": len(xs)}


def embeddings(family, n, d, seed, protos=None):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, device="cuda")
    if family == "mixture":
        which = torch.randint(0, protos.shape[0], (n,), generator=g, device="cuda")
        x = protos[which] + (0.3 / d ** 0.5) * x
    return torch.nn.functional.normalize(x, dim=1)


def one_shape(name, family, repeats):
    import torch
    from lemon_amd.neighbors import LemonDB
    sh = SHAPES[name]
    n, nq, d, k, own = sh["n_db"], sh["nq"], sh["d"], sh["k"], sh["own_rows"]
    protos = {m: embeddings("random", 1000, d, 5 + i) for i, m in enumerate(("img", "txt"))} if family == "mixture" else {}
    fresh = nq - own
    if family == "class":                             # a class dataset: random images, the text side is 100 prompts repeated
        prompts = embeddings("random", 100, d, 6)
        g = torch.Generator(device="cuda").manual_seed(7)
        img_tr, txt_tr = embeddings("random", n, d, 1), prompts[torch.randint(0, 100, (n,), generator=g, device="cuda")].contiguous()
        q_img = torch.cat([img_tr[:own], embeddings("random", fresh, d, 3)]).contiguous()
        q_txt = torch.cat([txt_tr[:own], prompts[torch.randint(0, 100, (fresh,), generator=g, device="cuda")]]).contiguous()
    else:
        img_tr, txt_tr = embeddings(family, n, d, 1, protos.get("img")), embeddings(family, n, d, 2, protos.get("txt"))
        q_img = torch.cat([img_tr[:own], embeddings(family, fresh, d, 3, protos.get("img"))]).contiguous()
        q_txt = torch.cat([txt_tr[:own], embeddings(family, fresh, d, 4, protos.get("txt"))]).contiguous()
    kw = dict(drop_self=own > 0)
    if own:
        kw["in_db"] = torch.cat([torch.ones(own, dtype=torch.uint8), torch.zeros(fresh, dtype=torch.uint8)]).cuda()

    kernels = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def two_dbs():                                    # -> (build seconds, call seconds, records)
        out, build, call = {}, 0.0, 0.0
        for m in ("cosine", "euclidean"):
            t, db = timed(lambda: LemonDB(img_tr, txt_tr, m))
            build += t
            t, out[m] = timed(lambda: db.neighbors(q_img, q_txt, k, **kw))
            call += t
            kernels["two_dbs_" + m] = db.index_img.last_scan_kernel()
            del db
        return build, call, out

    def one_db(margin=4):
        build, db = timed(lambda: LemonDB(img_tr, txt_tr, ("cosine", "euclidean")))
        call, (out, _) = timed(lambda: db.neighbors_metrics(q_img, q_txt, k, margin=margin, **kw))
        kernels["one_db"] = db.index_img.last_scan_kernel()
        return build, call, out

    a, b = two_dbs()[2], one_db()[2]                  # warm-up, and the two legs must agree bit for bit
    raw = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    same = all(bool(torch.equal(raw(a[m][key]), raw(b[m][key]))) for m in a for key in REC)
    del a, b
    times = {leg + part: [] for leg in ("two_dbs", "one_db") for part in ("", "_build", "_call")}
    for _ in range(repeats):
        for leg, fn in (("two_dbs", two_dbs), ("one_db", one_db)):
            build, call, _ = fn()
            times[leg].append(build + call)
            times[leg + "_build"].append(build)
            times[leg + "_call"].append(call)
    shares, fallback_s = {}, None
    db = LemonDB(img_tr, txt_tr, ("cosine", "euclidean"))
    for margin in (1, 4, 8):
        _, c = db.neighbors_metrics(q_img, q_txt, k, margin=margin, **kw)
        shares[str(margin)] = {"certified_n": c["certified_n"] / nq, "certified_m": c["certified_m"] / nq, "fallback_rows": c["fallback"]}
        if margin == 4 and c["fallback"]:
            rows = torch.nonzero(~(c["cert_n"] & c["cert_m"])).flatten()
            sub = dict(kw, in_db=kw["in_db"][rows]) if own else kw
            pair = db.l2_pair()
            fallback_s = stats([timed(lambda: pair.neighbors(q_img[rows], q_txt[rows], k, **sub))[0] for _ in range(repeats)])
    return {"shape": name, "family": family, **sh, "bit_identical": same, "seconds": {leg: stats(v) for leg, v in times.items()},
            "scan_kernels": kernels, "certified_share_by_margin": shares, "fallback_alone_seconds_margin4": fallback_s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--families", default="random,mixture")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_sweep"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "dist_sweep.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    for name in args.shapes.split(","):
        for family in args.families.split(","):
            res[f"{name}_{family}"] = one_shape(name, family, args.repeats)
            print(json.dumps(res[f"{name}_{family}"]), flush=True)
            with open(path, "w") as f:              # after every shape: one that runs out of time keeps the others' results
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
