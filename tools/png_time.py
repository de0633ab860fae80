"""What LEMON_PNG=gpu changes for PNG files, on one GPU: recorded, not asserted.

Writes N seeded PNGs per set -- grey 512 x 512 (the shape of lib/datasets/dataloader.py:177-184's down-sampled radiographs) and
RGB 640 x 480, smooth images with noise, written by PIL's encoder at its default level -- and records per set, one JSON line each:
  images_per_s_pil / images_per_s_gpu   loader.ragged_batches over the files with device_png off / on, the same worker count,
                                        every chunk synchronised (median of --reps passes after one warm-up)
  ring_bytes_per_image_*                what the workers hand over (DecodePool): h * w * 3 pixels, or the record
  h2d_bytes_per_image_*                 what the chunks' copies carry (stats["h2d"])
  kernel_us_per_batch                   lemon_png_decode alone on one batch of all N records, device events (median)
  worker_us_per_image_pil / _gpu        one core: `Image.open(p).convert("RGB")` into an array, against chunk walk + inflate
Needs a HIP device.

  python tools/png_time.py --n 256 --out profiles/png/png.json
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = {"grey_512": (512, 512, "L"), "rgb_640x480": (480, 640, "RGB")}


def write_pngs(directory, name, n, seed=0):
    from PIL import Image
    h, w, mode = SETS[name]
    rng = np.random.default_rng(seed)
    c = 1 if mode == "L" else 3
    yy, xx = np.mgrid[0:h, 0:w]
    paths = []
    for i in range(n):
        fx, fy = rng.uniform(0.005, 0.05, 2)
        base = 127 + 90 * np.sin(xx * fx + i)[:, :, None] * np.cos((yy * fy)[:, :, None] + np.arange(c)[None, None, :])
        px = np.clip(base + rng.normal(0, 4, (h, w, c)), 0, 255).astype(np.uint8)
        p = os.path.join(directory, f"{name}_{i:05d}.png")
        Image.fromarray(px.squeeze(), mode).save(p)
        paths.append(p)
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--sets", default="grey_512,rgb_640x480")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "png", "png.json"))
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("png_time.py needs a HIP device")
    from PIL import Image
    from lemon_amd import _lib, jpeg_host, png_host
    from lemon_amd.data import launch_png_decode
    from lemon_amd.loader import DecodePool, ragged_batches
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.sets.split(","):
            paths = write_pngs(tmp, name, a.n)
            raws = [open(p, "rb").read() for p in paths]
            rec = dict(set=name, n=a.n, workers=a.workers, chunk=a.chunk, reps=a.reps, file_MB=sum(len(r) for r in raws) / 1e6,
                       device=torch.cuda.get_device_name(0))
            # one core: the worker's work per image in each mode
            t0 = time.perf_counter()
            for r in raws:
                np.asarray(Image.open(io.BytesIO(r)).convert("RGB"), dtype=np.uint8)
            rec["worker_us_per_image_pil"] = (time.perf_counter() - t0) * 1e6 / a.n
            t0 = time.perf_counter()
            records = [png_host.decode_record(r)[0] for r in raws]
            rec["worker_us_per_image_gpu"] = (time.perf_counter() - t0) * 1e6 / a.n
            assert all(r is not None for r in records)
            # the loader, both modes
            for mode, on in (("pil", False), ("gpu", True)):
                with DecodePool(paths, workers=a.workers, png=on) as pool:
                    rec[f"ring_bytes_per_image_{mode}"] = sum((x.data if on else x).nbytes for _, x in pool.images()) / a.n
                rates, h2d = [], 0
                for rep in range(a.reps + 1):
                    stats = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s, e, px in ragged_batches(paths, a.chunk, 0, a.n, dev, workers=a.workers, stats=stats, device_jpeg=False,
                                                   device_png=on):
                        torch.cuda.synchronize()
                    if rep:
                        rates.append(a.n / (time.perf_counter() - t0))
                    h2d = sum(b for _, _, b in stats["h2d"]) / a.n
                    rec[f"png_fallback_{mode}"] = stats.get("png_fallback", 0)
                rec[f"images_per_s_{mode}"] = float(np.median(rates))
                rec[f"images_per_s_{mode}_all"] = rates
                rec[f"h2d_bytes_per_image_{mode}"] = h2d
            # the kernel alone, one batch of all records
            lay, off, items = jpeg_host.BatchLayout(), 0, []
            for r in records:
                lay.add_png_record(off, r)
                items.append((off, r.data))
                off = (off + r.data.nbytes + 15) & ~15
            aux = lay.finish(off)
            buf = np.zeros(lay.payload_bytes, np.uint8)
            for o, d in items:
                buf[o:o + d.nbytes] = d
            buf[lay.aux_off:] = aux.view(np.uint8)
            data = torch.empty((lay.total_bytes,), dtype=torch.uint8, device=dev)
            data[:buf.size].copy_(torch.from_numpy(buf))
            us, status = [], None
            for rep in range(a.reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                ev[0].record()
                status = launch_png_decode(data, lay)
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    us.append(ev[0].elapsed_time(ev[1]) * 1e3)
            rec["kernel_us_per_batch"] = float(np.median(us))
            rec["kernel_us_per_batch_all"] = us
            rec["kernel_declined"] = int((status.cpu().numpy() != 0).sum())
            rec["kernel_equals_pil"] = bool(all(np.array_equal(
                data[lay.desc[i][0]:lay.desc[i][0] + lay.desc[i][1] * lay.desc[i][2] * 3].cpu().numpy().reshape(lay.desc[i][1], lay.desc[i][2], 3),
                np.asarray(Image.open(io.BytesIO(raws[i])).convert("RGB"))) for i in range(0, a.n, max(1, a.n // 8))))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
