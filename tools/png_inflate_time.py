"""What LEMON_PNG=device changes for PNG files, on one GPU: recorded, not asserted.

Writes seeded PNGs with tools/png_time.py's generator -- 512 grey 512 x 512 (the shape of lib/datasets/dataloader.py:177-184's
down-sampled radiographs) and 256 RGB 640 x 480, written by PIL's encoder at its default level -- and records per set, one JSON
line each:
  images_per_s_pil / _gpu / _device     loader.ragged_batches over the files in the three LEMON_PNG modes, the same worker
                                        count, every chunk synchronised (median of --reps passes after one warm-up); the
                                        yardstick is the gpu mode of the same run
  ring_bytes_per_image_*                what the workers hand over (DecodePool): h * w * 3 pixels, the record, or palette + stream
  h2d_bytes_per_image_*                 what the chunks' copies carry (stats["h2d"])
  inflate_us_per_batch                  lemon_png_inflate alone on one batch of all N streams, device events (median)
  decode_us_per_batch                   lemon_png_decode alone behind it
  inflate_MBps_per_stream               the inflated bytes of one image over the kernel's time for the batch when the batch fits
                                        the device's resident streams (4 per CU), else scaled by the number of rounds
  worker_us_per_image_*                 one core: PIL's whole decode, chunk walk + zlib, chunk walk alone
Needs a HIP device.

  python tools/png_inflate_time.py --out profiles/png/inflate.json
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COUNTS = {"grey_512": 512, "rgb_640x480": 256}
MODES = (("pil", False, False), ("gpu", True, False), ("device", True, True))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="grey_512,rgb_640x480")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the sets' image counts (a quick run)")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "png", "inflate.json"))
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("png_inflate_time.py needs a HIP device")
    from PIL import Image
    from png_time import write_pngs
    from lemon_amd import _lib, jpeg_host, png_host
    from lemon_amd.data import launch_png_decode, launch_png_inflate
    from lemon_amd.loader import DecodePool, ragged_batches
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.sets.split(","):
            n = max(1, int(COUNTS[name] * a.scale))
            paths = write_pngs(tmp, name, n)
            raws = [open(p, "rb").read() for p in paths]
            rec = dict(set=name, n=n, workers=a.workers, chunk=a.chunk, reps=a.reps, file_MB=sum(len(r) for r in raws) / 1e6,
                       device=torch.cuda.get_device_name(0), resident_streams=resident)
            for mode, work in (("pil", lambda r: np.asarray(Image.open(io.BytesIO(r)).convert("RGB"), dtype=np.uint8)),
                               ("gpu", lambda r: png_host.decode_record(r)[0]), ("device", lambda r: png_host.pack_stream(r)[0])):
                t0 = time.perf_counter()
                made = [work(r) for r in raws]
                rec[f"worker_us_per_image_{mode}"] = (time.perf_counter() - t0) * 1e6 / n
            streams = made
            assert all(s is not None for s in streams)
            for mode, png, inflate in MODES:
                with DecodePool(paths, workers=a.workers, png=png, png_streams=inflate) as pool:
                    rec[f"ring_bytes_per_image_{mode}"] = sum((x.data if png else x).nbytes for _, x in pool.images()) / n
                rates, h2d = [], 0
                for rep in range(a.reps + 1):
                    stats = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s, e, px in ragged_batches(paths, a.chunk, 0, n, dev, workers=a.workers, stats=stats, device_jpeg=False,
                                                   device_png=png, png_inflate=inflate):
                        torch.cuda.synchronize()
                    if rep:
                        rates.append(n / (time.perf_counter() - t0))
                    h2d = sum(b for _, _, b in stats["h2d"]) / n
                    rec[f"png_fallback_{mode}"] = stats.get("png_fallback", 0)
                rec[f"images_per_s_{mode}"] = float(np.median(rates))
                rec[f"images_per_s_{mode}_all"] = rates
                rec[f"h2d_bytes_per_image_{mode}"] = h2d
            # the kernels alone, one batch of all streams
            lay, off, items = jpeg_host.BatchLayout(), 0, []
            for s in streams:
                lay.add_png_stream(off, s)
                items.append((off, s.data))
                off = (off + s.data.nbytes + 15) & ~15
            aux = lay.finish(off)
            buf = np.zeros(lay.payload_bytes, np.uint8)
            for o, d in items:
                buf[o:o + d.nbytes] = d
            buf[lay.aux_off:] = aux.view(np.uint8)
            data = torch.empty((lay.total_bytes,), dtype=torch.uint8, device=dev)
            data[:buf.size].copy_(torch.from_numpy(buf))
            us_z, us_d, zst, dst = [], [], None, None
            for rep in range(a.reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                torch.cuda.synchronize()
                ev[0].record()
                zst = launch_png_inflate(data, lay)
                ev[1].record()
                dst = launch_png_decode(data, lay)
                ev[2].record()
                torch.cuda.synchronize()
                if rep:
                    us_z.append(ev[0].elapsed_time(ev[1]) * 1e3)
                    us_d.append(ev[1].elapsed_time(ev[2]) * 1e3)
            rec["inflate_us_per_batch"] = float(np.median(us_z))
            rec["inflate_us_per_batch_all"] = us_z
            rec["decode_us_per_batch"] = float(np.median(us_d))
            want = (lay.png_rec_end - lay.png_rec_off) / n - 1024
            rec["inflated_bytes_per_image"] = want
            rec["inflate_MBps_per_stream"] = want * -(-n // resident) / rec["inflate_us_per_batch"]
            rec["kernel_declined"] = int((zst.cpu().numpy() != 0).sum() + (dst.cpu().numpy() != 0).sum())
            rec["kernel_equals_pil"] = bool(all(np.array_equal(
                data[lay.desc[i][0]:lay.desc[i][0] + lay.desc[i][1] * lay.desc[i][2] * 3].cpu().numpy().reshape(lay.desc[i][1], lay.desc[i][2], 3),
                np.asarray(Image.open(io.BytesIO(raws[i])).convert("RGB"))) for i in range(0, n, max(1, n // 8))))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
