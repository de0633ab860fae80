"""Image decode worker of lemon_amd.loader.DecodePool: a fresh interpreter that imports PIL and numpy only (never torch, never
the HIP library, never the GPU) and decodes exactly `Image.open(p).convert("RGB")` -- the reference's loader step
(lib/datasets/dataloader.py:167-198) without its transform, which runs on the GPU -- into a shared-memory ring of its own.

Run as a script by path (`python decode_worker.py SHM_PATH CAPACITY`), so that not even the lemon_amd package is imported.
Protocol (pickled frames on stdin / stdout, in order):
  parent -> worker: ("task", seq, path) | ("free", nbytes) | ("stop",)
  worker -> parent: ("hello", pid, torch_imported)
                    ("ok", seq, offset, h, w, consumed, oversize_path or None) | ("err", seq, path, message)
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

    while True:
        if not tasks:
            try:
                take(pickle.load(inp))
            except EOFError:
                return 0
            continue
        _, seq, path = tasks.popleft()
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
            _send(out, ("ok", seq, 0, h, w, 0, big))
            continue
        while True:
            if used == 0:
                head = 0
            if head + n <= cap and used + n <= cap:
                off, consumed = head, n
                break
            if head + n > cap and used + (cap - head) + n <= cap:
                off, consumed = 0, (cap - head) + n
                break
            take(pickle.load(inp))      # wait for the parent to free space
        view[off:off + n] = img.reshape(-1)
        head = off + n
        used += consumed
        _send(out, ("ok", seq, off, h, w, consumed, None))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
