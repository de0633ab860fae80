"""Kernel time of the device Huffman pass of progressive JPEGs (lemon_jpeg_prog_entropy_device, csrc/jpeg_prog.hip) on one GPU.

Writes N seeded JPEGs per size mix (the mixes of tools/file_pipeline_time.py, every file progressive), packs them on the host
(lemon_jpeg_prog_pack), copies one batch of packets to the device and times the launches of lemon_jpeg_prog_entropy_device alone
and of lemon_jpeg_decode behind it with device events, `--reps` times after one warm-up.  One JSON line per mix:
entropy_us_per_image and entropy_us_per_MB (median; compressed MB = the packets' entropy-coded bytes), every repetition,
decode_us_per_image, the wave items and levels of the batch, declined (statuses != 0), and beside them the host pass of the same
files on one CPU core (host_us_per_image) and PIL's whole decode (pil_us_per_image).  Needs a HIP device.

  python tools/jpeg_progressive_time.py --n 256 --out profiles/jpeg/progressive_time.jsonl
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n_cars", type=int, default=64)
    ap.add_argument("--mixes", default="mscoco,cars")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_progressive_time.py needs a HIP device")
    from PIL import Image
    from file_pipeline_time import write_jpegs
    from lemon_amd import _lib, jpeg_host
    from lemon_amd.data import launch_jpeg_decode, launch_jpeg_entropy
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for mix in a.mixes.split(","):
            n = a.n if mix == "mscoco" else a.n_cars
            raws = [open(p, "rb").read() for p in write_jpegs(tmp, mix, n, progressive_every=1)]
            packets = [jpeg_host.prog_pack(r)[0] for r in raws]
            assert all(p is not None for p in packets)
            t0 = time.perf_counter()
            for r in raws:
                assert jpeg_host.decode_record(r, progressive=True)[0] is not None
            host_us = (time.perf_counter() - t0) * 1e6 / n
            t0 = time.perf_counter()
            for r in raws:
                np.asarray(Image.open(io.BytesIO(r)).convert("RGB"))
            pil_us = (time.perf_counter() - t0) * 1e6 / n
            lay, off, items = jpeg_host.BatchLayout(), 0, []
            for pk in packets:
                lay.add_packet(off, pk)
                items.append((off, pk.data))
                off = (off + pk.data.nbytes + 15) & ~15
            aux = lay.finish(off)
            buf = np.zeros(lay.payload_bytes, np.uint8)
            for o, d in items:
                buf[o:o + d.nbytes] = d
            buf[lay.aux_off:] = aux.view(np.uint8)
            data = torch.empty((lay.total_bytes,), dtype=torch.uint8, device=dev)
            data[:buf.size].copy_(torch.from_numpy(buf))
            ent, dec, status = [], [], None
            for rep in range(a.reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                torch.cuda.synchronize()
                ev[0].record()
                status = launch_jpeg_entropy(data, lay)
                ev[1].record()
                launch_jpeg_decode(data, lay)
                ev[2].record()
                torch.cuda.synchronize()
                if rep:
                    ent.append(ev[0].elapsed_time(ev[1]) * 1e3)
                    dec.append(ev[1].elapsed_time(ev[2]) * 1e3)
            st = status.cpu().numpy()
            mb = sum(int(pk.data[:64].view(np.int32)[12]) for pk in packets) / 1e6      # (kHDataBytes)
            rec = dict(mix=mix, n=n, reps=a.reps, compressed_MB=mb, file_MB=sum(len(r) for r in raws) / 1e6, items=lay.prog_items,
                       levels=lay.prog_levels, entropy_us_per_image=float(np.median(ent)) / n,
                       entropy_us_per_image_all=[e / n for e in ent], entropy_us_per_MB=float(np.median(ent)) / mb,
                       decode_us_per_image=float(np.median(dec)) / n, declined=int((st != 0).sum()), host_us_per_image=host_us,
                       pil_us_per_image=pil_us, device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
