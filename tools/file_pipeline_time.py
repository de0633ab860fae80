"""Throughput of the file-backed image path (lemon_amd/loader.py + lemon_preprocess_ragged) on one GPU.

Writes N seeded JPEGs (PIL, quality 90, 4:2:0) per size mix to a temp dir and prints one JSON line per mix:
  decode_images_per_s      the decode pool alone (no GPU)
  resident_images_per_s    the same images pre-decoded in HBM: ragged transform + image tower
  from_files_images_per_s  files -> pool -> pinned uint8 -> H2D on the copy stream -> ragged transform + image tower
  gpu_idle_frac            1 - (resident GPU time of the images) / (from-files wall time)
  h2d_GBs                  the uint8 copies (device events)
  ragged_us_per_image      lemon_preprocess_ragged alone (operand form), device events
  warm_ring_images_per_s   from files, timed only after the pool has decoded as far ahead as it may
  pack_images_per_s        the packing thread's copies out of the rings into pinned memory
  pool_wait_s, ready_wait_s, status_wait_s   of the from-files run's from_files_s: the packing thread waiting for the workers,
                           the caller waiting for a packed chunk, the caller waiting for the device Huffman pass's statuses
  threads_path_images_per_s  LEMON_DECODE_WORKERS=0 (in-process PIL decode + CPU transform), first <= 512 images
  --jpeg gpu|pil|device    from-files and pool figures with baseline JPEGs decoded on the GPU (gpu: the workers run only the
                           Huffman pass; device: the workers only write scan packets, the Huffman pass runs on the GPU too) or
                           by PIL in the workers (LEMON_JPEG); default: the library's default
  --progressive K          every K-th file is written progressive (1 = all, 4 = one in four); --progressive_switch 0|1 sets
                           LEMON_JPEG_PROGRESSIVE for the run (0: those files are decoded by PIL in the workers, as before the
                           switch existed); the line then carries progressive_files, jpeg_progressive and the switch
Every timed region is bracketed by a device synchronise.  Needs a HIP device.

  python tools/file_pipeline_time.py --arch vit-b-16 --n 2048 --out profiles/r6/file_pipeline.jsonl
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXES = {
    "mscoco": [(480, 640)] * 8 + [(640, 480)] * 3 + [(427, 640)] * 5 + [(375, 500)] * 3 + [(612, 612)] * 2 + [(1200, 1600)],
    "cars": None,      # short side 400..2000, aspect 4:3 .. 16:9
}


def write_jpegs(d, mix, n, seed=0, reuse=False, progressive_every=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        if mix == "cars":
            s = int(rng.integers(400, 2001))
            h, w = s, int(s * rng.uniform(4 / 3, 16 / 9))
        else:
            h, w = MIXES[mix][i % len(MIXES[mix])]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        base = 128 + 90 * np.sin(yy[..., None] / rng.uniform(5, 40) + xx[..., None] / rng.uniform(5, 40) + np.arange(3))
        px = np.clip(base + rng.normal(0, 12, (h, w, 1)), 0, 255).astype(np.uint8)
        prog = bool(progressive_every) and i % progressive_every == 0
        p = os.path.join(d, f"{mix}_{i:05d}{'_p' if prog else ''}.jpg")
        if reuse and os.path.exists(p):          # (the random draws above still advance: file i is the same in every run)
            paths.append(p)
            continue
        Image.fromarray(px).save(p, quality=90, subsampling=2, progressive=prog)
        paths.append(p)
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="vit-b-16")
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--n_cars", type=int, default=384)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mixes", default="mscoco,cars")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--jpeg", choices=("gpu", "pil", "device"), default=None)
    ap.add_argument("--progressive", type=int, default=0, help="every K-th file is progressive (0: none)")
    ap.add_argument("--progressive_switch", choices=("0", "1"), default=None, help="LEMON_JPEG_PROGRESSIVE for this run")
    ap.add_argument("--skip_threads", action="store_true", help="leave out the LEMON_DECODE_WORKERS=0 figure")
    ap.add_argument("--keep_dir", default=None, help="write the JPEGs here and keep them; files already there are reused")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.jpeg:
        os.environ["LEMON_JPEG"] = a.jpeg
    if a.progressive_switch is not None:
        os.environ["LEMON_JPEG_PROGRESSIVE"] = a.progressive_switch
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("file_pipeline_time.py needs a HIP device")
    from lemon_amd import _lib, loader
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.data import RaggedImages, gpu_transform_ragged
    from lemon_amd.pipeline import Embedder
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = ClipConfig.named(a.arch)
    torch.manual_seed(0)
    emb = Embedder(LemonCLIP(cfg), dev, batch_size=a.batch)
    workers = a.workers if a.workers is not None else loader.default_workers(1)
    jpeg_gpu = loader.device_jpeg_default()
    prog_on = bool(jpeg_gpu) and loader.progressive_default()
    lines = []
    if a.keep_dir:
        os.makedirs(a.keep_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = a.keep_dir or tmp
        for mix in a.mixes.split(","):
            n = a.n if mix == "mscoco" else a.n_cars
            t0 = time.perf_counter()
            paths = write_jpegs(tmp, mix, n, reuse=bool(a.keep_dir), progressive_every=a.progressive)
            n_prog = len(range(0, n, a.progressive)) if a.progressive else 0
            write_s = time.perf_counter() - t0
            # decode pool alone (pixels: what the resident figure needs)
            t0 = time.perf_counter()
            decoded = []
            with loader.DecodePool(paths, workers) as pool:
                for _, img in pool.images():
                    decoded.append(img.copy())
            decode_s = pixels_decode_s = time.perf_counter() - t0
            if jpeg_gpu:                             # ... and as the from-files path runs it: coefficient records
                t0 = time.perf_counter()
                with loader.DecodePool(paths, workers, records=True, packets=jpeg_gpu == "device", progressive=prog_on) as pool:
                    n_rec = sum(not isinstance(x, np.ndarray) for _, x in pool.images())
                decode_s = time.perf_counter() - t0
                assert n_rec == (n if prog_on else n - n_prog), (n_rec, n, n_prog)
            # resident: pre-decoded uint8 in HBM
            chunks = [RaggedImages.from_arrays(decoded[s:s + a.batch], dev) for s in range(0, n, a.batch)]
            del decoded
            emb.embed_images(chunks[0])                      # warm-up (plans, kernels, workspace)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c in chunks:
                emb.embed_images(c)
            torch.cuda.synchronize()
            resident_s = time.perf_counter() - t0
            patch_ok = cfg.vision.width % 256 == 0
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for c in chunks:
                gpu_transform_ragged(c, cfg.image_size, patch=cfg.patch_size, operand=patch_ok)
            ev[1].record()
            torch.cuda.synchronize()
            ragged_us = ev[0].elapsed_time(ev[1]) * 1e3 / n
            del chunks
            # from files
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _, _, r in loader.ragged_batches(paths, a.batch, 0, n, dev, workers=workers, stats=stats):
                emb.embed_images(r)
            torch.cuda.synchronize()
            files_s = time.perf_counter() - t0
            emb.raise_if_nonfinite()
            # warm ring: after the first chunk, wait until the pool has decoded as far ahead as it may (LOOKAHEAD_PER_WORKER
            # tasks per worker, within the ring's bytes), then time the chunks it holds: GPU-bound if nothing waits on the host
            ahead = min(workers * loader.LOOKAHEAD_PER_WORKER, n - a.batch) // a.batch * a.batch
            warm = None
            if ahead >= a.batch:
                gen = loader.ragged_batches(paths, a.batch, 0, a.batch + ahead, dev, workers=workers)
                emb.embed_images(next(gen)[2])
                torch.cuda.synchronize()
                time.sleep(1.5 * (a.batch + ahead) / (n / decode_s) + 0.5)
                t0 = time.perf_counter()
                for _, _, r in gen:
                    emb.embed_images(r)
                torch.cuda.synchronize()
                warm = ahead / (time.perf_counter() - t0)
            # the in-process thread path (LEMON_DECODE_WORKERS=0): PIL decode + CPU generic_transform, float32 across PCIe
            from lemon_amd.data import ImageLabelSet
            nt = 0 if a.skip_threads else min(n, 512)
            old = os.environ.get("LEMON_DECODE_WORKERS")
            os.environ["LEMON_DECODE_WORKERS"] = "0"
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for px, _, _ in ImageLabelSet(paths[:nt], [0] * nt, [0] * nt, cfg.image_size).batches(a.batch, device=dev):
                    emb.embed_images(px)
                torch.cuda.synchronize()
                threads_s = time.perf_counter() - t0
            finally:
                if old is None:
                    os.environ.pop("LEMON_DECODE_WORKERS")
                else:
                    os.environ["LEMON_DECODE_WORKERS"] = old
            h2d_ms = sum(s.elapsed_time(e) for s, e, _ in stats["h2d"])
            h2d_bytes = sum(b for _, _, b in stats["h2d"])
            rec = dict(mix=mix, arch=a.arch, n=n, batch=a.batch, workers=workers, usable_cpus=loader.usable_cpus(),
                       decode_images_per_s=n / decode_s, resident_images_per_s=n / resident_s, from_files_images_per_s=n / files_s,
                       gpu_idle_frac=max(0.0, 1.0 - resident_s / files_s), h2d_GBs=h2d_bytes / max(h2d_ms, 1e-9) / 1e6,
                       h2d_MB_per_image=h2d_bytes / n / 1e6, ragged_us_per_image=ragged_us,
                       tower_us_per_image=resident_s * 1e6 / n, write_s=write_s,
                       warm_ring_images=ahead, warm_ring_images_per_s=warm, pack_images_per_s=n / max(stats["pack_s"], 1e-9),
                       threads_path_images_per_s=nt / threads_s if nt else None, threads_path_images=nt,
                       jpeg="device" if jpeg_gpu == "device" else "gpu" if jpeg_gpu else "pil", pil_pool_images_per_s=n / pixels_decode_s,
                       jpeg_images=stats.get("jpeg_images", 0), jpeg_fallback=stats.get("jpeg_fallback", 0),
                       progressive_files=n_prog, progressive_switch=int(prog_on), jpeg_progressive=stats.get("jpeg_progressive", 0),
                       from_files_s=files_s, pool_wait_s=stats.get("pool_wait_s"), ready_wait_s=stats.get("ready_wait_s"),
                       status_wait_s=stats.get("status_wait_s", 0.0), pack_s=stats["pack_s"],
                       device=torch.cuda.get_device_name(0))
            rec["ratio_vs_min"] = rec["from_files_images_per_s"] / min(rec["resident_images_per_s"], rec["decode_images_per_s"])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            if not a.keep_dir:
                for p in paths:
                    os.unlink(p)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
