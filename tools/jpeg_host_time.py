"""Host cost of a JPEG decode on one CPU core: PIL (`Image.open(p).convert("RGB")`, the whole decode) against the entropy
pass alone (lemon_jpeg_entropy: header + Huffman decoding into a coefficient record, what is left on the host when the GPU does
the rest), for the mscoco-like and cars-like mixes of tools/file_pipeline_time.py.  The ratio is the ceiling of what decoding
on the GPU can gain in decode-bound pipelines.  Also timed: the packer (lemon_jpeg_pack: header + the scan walk, what a worker
does when the GPU decodes the Huffman stream too) and, on progressive re-encodings of the same pixels, the progressive host
pass and packer (lemon_jpeg_prog_entropy, lemon_jpeg_prog_pack).  Needs no GPU.

  python tools/jpeg_host_time.py --out profiles/jpeg/host_time.json
"""
import argparse
import io
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--n_cars", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    from PIL import Image
    import PIL
    from lemon_amd import jpeg_host
    from tools.file_pipeline_time import write_jpegs
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})       # one core
    except (AttributeError, OSError):
        pass
    rec = dict(cpu=cpu_model(), pillow=PIL.__version__, repeats=a.repeats, mixes={})
    with tempfile.TemporaryDirectory() as tmp:
        for mix, n in (("mscoco", a.n), ("cars", a.n_cars)):
            raws = [open(p, "rb").read() for p in write_jpegs(tmp, mix, n)]
            os.makedirs(os.path.join(tmp, "prog_" + mix))
            progs = [open(p, "rb").read() for p in write_jpegs(os.path.join(tmp, "prog_" + mix), mix, n, progressive_every=1)]
            buf = np.empty(max(jpeg_host.info(r).record_bytes for r in raws), np.uint8)
            pkt = np.empty(max(max(jpeg_host.packet_cap(len(r)) for r in raws), max(jpeg_host.prog_packet_cap(len(r)) for r in progs)),
                           np.uint8)
            draws = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                for r in raws:
                    np.asarray(Image.open(io.BytesIO(r)).convert("RGB"))
                t1 = time.perf_counter()
                exact = blocks = 0
                for r in raws:
                    info = jpeg_host.entropy(r, buf)
                    assert info.status == 0, info.status
                    exact += info.exact_blocks
                    blocks += info.blocks
                t2 = time.perf_counter()
                for r in raws:
                    assert jpeg_host.pack(r, pkt)[1].status == 0
                t3 = time.perf_counter()
                for r in progs:
                    assert jpeg_host.prog_entropy(r, buf).status == 0
                t4 = time.perf_counter()
                for r in progs:
                    assert jpeg_host.prog_pack(r, pkt)[1].status == 0
                t5 = time.perf_counter()
                draws.append(dict(pil_ms_per_image=(t1 - t0) * 1e3 / n, entropy_ms_per_image=(t2 - t1) * 1e3 / n,
                                  ratio=(t2 - t1) / (t1 - t0), pack_ms_per_image=(t3 - t2) * 1e3 / n,
                                  prog_entropy_ms_per_image=(t4 - t3) * 1e3 / n, prog_pack_ms_per_image=(t5 - t4) * 1e3 / n))
            rec["mixes"][mix] = dict(n=n, file_KB=sum(map(len, raws)) / n / 1e3, exact_envelope_block_frac=exact / blocks, draws=draws)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
