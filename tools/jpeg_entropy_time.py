"""Kernel time of the device Huffman pass (lemon_jpeg_entropy_device, csrc/jpeg_entropy.hip) on one GPU, per subseq_bytes.

Writes N seeded JPEGs per size mix (the mixes of tools/file_pipeline_time.py), packs them on the host (lemon_jpeg_pack), copies
one batch of packets to the device and times the launches of lemon_jpeg_entropy_device alone and of lemon_jpeg_decode behind it
with device events, `--reps` times after one warm-up.  One JSON line per (mix, subseq_bytes): entropy_us_per_image,
entropy_us_per_MB (compressed, the packets' scan bytes), decode_us_per_image, declined (statuses != 0; LEMON_JPEG_SYNC counted
apart: the round cap), sync_iterations_max (the most decodes any lane of a workgroup needed before its states settled).  Needs a HIP device.

  python tools/jpeg_entropy_time.py --n 256 --subseq 16,32,64,128,256 --out profiles/jpeg/entropy_time.jsonl
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n_cars", type=int, default=64)
    ap.add_argument("--mixes", default="mscoco,cars")
    ap.add_argument("--subseq", default="16,32,64,128,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_entropy_time.py needs a HIP device")
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
            raws = [open(p, "rb").read() for p in write_jpegs(tmp, mix, n)]
            packets = [jpeg_host.pack(r)[0] for r in raws]
            assert all(p is not None for p in packets)
            for subseq in [int(v) for v in a.subseq.split(",")]:
                lay, off, items = jpeg_host.BatchLayout(subseq), 0, []
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
                ent, dec, status, ws = [], [], None, None
                for rep in range(a.reps + 1):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    torch.cuda.synchronize()
                    ev[0].record()
                    status, ws = launch_jpeg_entropy(data, lay, return_workspace=True)
                    ev[1].record()
                    launch_jpeg_decode(data, lay)
                    ev[2].record()
                    torch.cuda.synchronize()
                    if rep:
                        ent.append(ev[0].elapsed_time(ev[1]) * 1e3)
                        dec.append(ev[1].elapsed_time(ev[2]) * 1e3)
                st = status.cpu().numpy()
                iters = ws[:16 * len(packets)].cpu().numpy().view(np.int32).reshape(-1, 4)[:, 2]
                mb = sum(p.scan_bytes for p in packets) / 1e6
                rec = dict(mix=mix, n=n, subseq_bytes=subseq, reps=a.reps, compressed_MB=mb, workgroups=lay.groups,
                           entropy_us_per_image=float(np.median(ent)) / n, entropy_us_per_image_all=[e / n for e in ent],
                           entropy_us_per_MB=float(np.median(ent)) / mb, decode_us_per_image=float(np.median(dec)) / n,
                           declined=int((st != 0).sum()), sync=int((st == 16).sum()), sync_iterations_max=int(iters.max()), device=torch.cuda.get_device_name(0))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
