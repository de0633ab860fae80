"""Image decode worker of lemon_amd.loader.DecodePool: a fresh interpreter that imports PIL and numpy only (never torch, never
the HIP library, never the GPU) and decodes exactly `Image.open(p).convert("RGB")` -- the reference's loader step
(lib/datasets/dataloader.py:167-198) without its transform, which runs on the GPU -- into a shared-memory ring of its own.

With RECORDS = 1 a file that starts with FF D8 goes through the JPEG host pass instead (jpeg_host.py -> liblemon_jpeg_host.so,
which links no HIP runtime): its Huffman decoding runs straight into the ring and the ring receives the coefficient record that
lemon_jpeg_decode turns into the same pixels on the GPU.  A file the host pass declines (progressive, CMYK, corrupt, ...) is
decoded with PIL exactly as without RECORDS, PIL's own exception for a corrupt file included.  With RECORDS = 2 the worker
does not even decode Huffman codes: it writes the file's scan packet (lemon_jpeg_pack: markers parsed, byte stuffing removed)
into the ring, and lemon_jpeg_entropy_device decodes it on the GPU; a file whose header the packer declines goes to PIL.

With PROGRESSIVE = 1 (beside RECORDS 1 or 2) a progressive file is not left to PIL: the progressive host pass writes its record
(kind 3, the same record) or the progressive packer its packet (kind 4, lemon_jpeg_prog_pack) into the ring.

With PNG = 1 a file that starts with the PNG signature goes through png_host (chunk walk in liblemon_jpeg_host.so, inflate by
Python's zlib) and the ring receives its record -- palette + filtered scanlines, kind 5 -- which lemon_png_decode unfilters and
expands to the same pixels on the GPU; a file png_host declines falls through to the PIL branch unchanged.  With PNG_STREAMS = 1
(beside PNG = 1) the worker does not inflate either: after the chunk walk and the CRCs the ring receives the palette and the
concatenated IDAT payload, still compressed -- kind 6 --, and lemon_png_inflate writes the record on the GPU.

Run as a script by path (`python decode_worker.py SHM_PATH CAPACITY [RECORDS [PROGRESSIVE [PNG [PNG_STREAMS]]]]`), so that not even the lemon_amd package is imported.
Protocol (pickled frames on stdin / stdout, in order):
  parent -> worker: ("task", seq, path) | ("free", nbytes) | ("stop",)
  worker -> parent: ("hello", pid, torch_imported)
                    ("ok", seq, offset, h, w, consumed, oversize_path or None, kind, nbytes, (components, hs, vs) or None)
                    | ("err", seq, path, message)
`kind` 0: nbytes = h * w * 3 of RGB pixels; `kind` 1: nbytes of coefficient record; `kind` 2: nbytes of scan packet, with
(components, hs, vs, intervals, scan_bytes); `kind` 3: a record from the progressive host pass; `kind` 4: nbytes of progressive
packet, with (components, hs, vs, scans, items, levels); `kind` 5: nbytes of PNG record, with (colour_type, channels, plte_count);
`kind` 6: nbytes of palette + compressed PNG stream, with (colour_type, channels, plte_count, stream bytes).
The ring is a circular byte buffer of CAPACITY bytes.  An image is written at `offset` once `consumed` bytes (its own plus the
unused tail skipped when it wraps) are free; the parent returns them with "free" after it has copied the image, in the order
the results came.  An image larger than the whole ring waits until the ring is empty and goes to a one-off segment
(`oversize_path`) that the parent unlinks."""
import mmap
import os
import pickle
import sys
from collections import deque


def _send(out, msg):
    pickle.dump(msg, out, protocol=pickle.HIGHEST_PROTOCOL)
    out.flush()


def main(argv):
    import numpy as np
    from PIL import Image
    shm_path, cap = argv[0], int(argv[1])
    records = len(argv) > 2 and argv[2] == "1"
    packets = len(argv) > 2 and argv[2] == "2"
    progressive = len(argv) > 3 and argv[3] == "1"
    png = len(argv) > 4 and argv[4] == "1"
    png_streams = png and len(argv) > 5 and argv[5] == "1"
    if records or packets or png:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if records or packets:
        import jpeg_host
    if png:
        import png_host
    inp, out = sys.stdin.buffer, sys.stdout.buffer
    fd = os.open(shm_path, os.O_RDWR)
    ring = mmap.mmap(fd, cap)
    os.close(fd)
    view = np.frombuffer(ring, np.uint8)
    _send(out, ("hello", os.getpid(), "torch" in sys.modules))
    tasks = deque()
    head = used = 0

    def take(msg):
        nonlocal used
        if msg[0] == "task":
            tasks.append(msg)
        elif msg[0] == "free":
            used -= msg[1]
        else:
            raise SystemExit(0)

    def reserve(n):
        """(offset, bytes consumed) of n <= cap free contiguous bytes of the ring; waits for the parent to free them."""
        nonlocal head
        while True:
            if used == 0:
                head = 0
            if head + n <= cap and used + n <= cap:
                return head, n
            if head + n > cap and used + (cap - head) + n <= cap:
                return 0, (cap - head) + n
            take(pickle.load(inp))

    while True:
        if not tasks:
            try:
                take(pickle.load(inp))
            except EOFError:
                return 0
            continue
        _, seq, path = tasks.popleft()
        if png:
            # the chunk walk, then the inflate straight behind the palette in the ring.  Nothing is committed (head, used) until
            # the stream has ended exactly where the header says; a declined file falls through to PIL below
            data = None
            try:
                with open(path, "rb") as fh:
                    data = fh.read()
            except OSError:
                pass                    # (PIL below reports it)
            if data is not None and data[:8] == png_host.SIGNATURE:
                head_info = png_host.info(data)
                if png_streams and head_info.status == 0 and png_host.stream_bytes_of(head_info) + 15 <= cap:
                    n = png_host.stream_bytes_of(head_info)
                    off, consumed = reserve(n + 15)         # (the palette starts at a multiple of 16)
                    at = (off + 15) & ~15
                    png_host.fill_stream(data, head_info, view[at:at + n])
                    head = off + n + 15
                    used += consumed
                    _send(out, ("ok", seq, at, head_info.height, head_info.width, consumed, None, 6, n,
                                (head_info.colour_type, head_info.channels, head_info.plte_count, n - png_host.PALETTE_BYTES)))
                    continue
                n = head_info.record_bytes
                if not png_streams and head_info.status == 0 and n + 15 <= cap:
                    off, consumed = reserve(n + 15)         # (the record starts at a multiple of 16)
                    at = (off + 15) & ~15
                    if png_host.fill_record(data, head_info, view[at:at + n]) == 0:
                        head = off + n + 15
                        used += consumed
                        _send(out, ("ok", seq, at, head_info.height, head_info.width, consumed, None, 5, n,
                                    (head_info.colour_type, head_info.channels, head_info.plte_count)))
                        continue
            del data
        if packets:
            # the scan packet, straight into the ring: its capacity is known from the file size, its size after the call; only
            # the bytes it took are committed
            data = None
            try:
                with open(path, "rb") as fh:
                    data = fh.read()
            except OSError:
                pass                    # (PIL below reports it)
            prog = progressive and data is not None and jpeg_host.info(data).status == 3
            need = (jpeg_host.prog_packet_cap(len(data)) if prog else jpeg_host.packet_cap(len(data))) + 15 if data is not None else 0
            if data is not None and data[:2] == b"\xff\xd8" and need <= cap:
                off, consumed = reserve(need)
                at = (off + 15) & ~15
                pk, full = (jpeg_host.prog_pack if prog else jpeg_host.pack)(data, view[at:at + need - 15])
                if pk is not None:
                    took = at - off + pk.data.nbytes
                    head = off + took
                    used += consumed - (need - took)
                    meta = (pk.scans, pk.items, pk.levels) if prog else (pk.intervals, pk.scan_bytes)
                    _send(out, ("ok", seq, at, full.height, full.width, consumed - (need - took), None, 4 if prog else 2, pk.data.nbytes,
                                (full.components, full.hs, full.vs) + meta))
                    continue
            del data
        if records:
            # the host pass, straight into the ring: the record size is known after the frame header.  Nothing is committed
            # (head, used) until the pass has accepted the file; a declined file falls through to PIL below
            data = None
            try:
                with open(path, "rb") as fh:
                    data = fh.read()
            except OSError:
                pass                    # (PIL below reports it)
            if data is not None and data[:2] == b"\xff\xd8":
                head_info = jpeg_host.info(data)
                prog = progressive and head_info.status == 3
                if prog:
                    head_info = jpeg_host.prog_info(data)
                n = head_info.record_bytes
                if head_info.status == 0 and n + 15 <= cap:
                    off, consumed = reserve(n + 15)         # (the record's int16 blocks start at a multiple of 16)
                    at = (off + 15) & ~15
                    full = (jpeg_host.prog_entropy if prog else jpeg_host.entropy)(data, view[at:at + n])
                    if full.status == 0:
                        head = off + n + 15
                        used += consumed
                        _send(out, ("ok", seq, at, full.height, full.width, consumed, None, 3 if prog else 1, n, (full.components, full.hs, full.vs)))
                        continue
            del data
        try:
            img = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
        except Exception as e:          # noqa: BLE001  (reported to the parent, which raises naming the path)
            _send(out, ("err", seq, path, f"{type(e).__name__}: {e}"))
            continue
        h, w = img.shape[:2]
        n = img.nbytes
        if n > cap:                     # larger than the ring: alone, in a segment of its own
            while used:
                take(pickle.load(inp))
            big = f"{shm_path}.{seq}"
            bfd = os.open(big, os.O_CREAT | os.O_EXCL | os.O_RDWR, 0o600)
            os.ftruncate(bfd, max(n, 1))
            with mmap.mmap(bfd, max(n, 1)) as m:
                np.frombuffer(m, np.uint8)[:n] = img.reshape(-1)
                del m
            os.close(bfd)
            _send(out, ("ok", seq, 0, h, w, 0, big, 0, n, None))
            continue
        off, consumed = reserve(n)
        view[off:off + n] = img.reshape(-1)
        head = off + n
        used += consumed
        _send(out, ("ok", seq, off, h, w, consumed, None, 0, n, None))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
