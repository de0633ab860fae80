"""File-backed image datasets on the GPU path: a process pool that only decodes, and ragged device batches.

The reference decodes and transforms every image in 8 forked DataLoader workers (run_lemon.py:129-131,199-201,
lib/datasets/dataloader.py:167-198).  Here:
  * worker processes are fresh interpreters (lemon_amd/decode_worker.py run by path: PIL + numpy only, no torch, no GPU) that
    decode `Image.open(p).convert("RGB")` into shared-memory rings, ahead of the consumer, in dataset order;
  * the parent packs a chunk of decoded images into a pinned buffer and copies it to the device as uint8 on a copy stream;
    the compute stream waits on the copy's event;
  * the GPU does resize, crop, normalise and the patch-operand packing of the ragged batch (data.gpu_transform_ragged).
  * with device JPEG decoding on (LEMON_JPEG=gpu; the default is pil, see device_jpeg_default) a worker runs only the serial
    half of a baseline JPEG's decode, the Huffman pass (csrc/jpeg_entropy.hpp), and hands over a coefficient record; the
    records travel in the same pinned buffer and copy as the PIL pixels of the files it declines, and lemon_jpeg_decode
    reconstructs bit-identical RGB pixels on the compute stream, in the same device buffer, before the ragged transform.
The held decoded bytes are bounded by `ring_bytes` (one ring of ring_bytes / workers per worker; an image larger than a whole
ring is decoded alone, when its worker's ring is empty)."""
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np

from .jpeg_host import BatchLayout, JpegRecord

_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_worker.py")
DEFAULT_RING_BYTES = 1 << 30
LOOKAHEAD_PER_WORKER = 64      # queued tasks per worker (keeps every pipe far below its buffer size)


def usable_cpus():
    """CPUs this process may run on (sched_getaffinity), capped by OMP_NUM_THREADS when it is set -- never os.cpu_count():
    a container or a job slot may see many more CPUs than it owns."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    omp = os.environ.get("OMP_NUM_THREADS", "").strip()
    if omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


def device_jpeg_default():
    """Whether file batches decode baseline JPEGs on the GPU: LEMON_JPEG=gpu / pil.  Default pil: the end-to-end comparison
    that would turn it on has not been recorded yet; results are identical either way."""
    env = os.environ.get("LEMON_JPEG", "").strip().lower()
    if env == "gpu":
        return True
    if env in ("", "pil"):
        return False
    raise ValueError(f"LEMON_JPEG={env!r}: expected 'gpu' or 'pil'")


def default_workers(world=1):
    """LEMON_DECODE_WORKERS when set (0 = the in-process thread path), else min(8, usable_cpus() // world), at least 1."""
    env = os.environ.get("LEMON_DECODE_WORKERS", "").strip()
    if env:
        return max(0, int(env))
    return max(1, min(8, usable_cpus() // max(1, world)))


class DecodeError(RuntimeError):
    pass


class DecodePool:
    """`workers` decode processes over `paths`; images(lo, hi) yields (i, uint8 [H, W, 3] view of shared memory) in order, each
    view valid until the next item is requested.  With records=True a baseline JPEG the host pass accepts is yielded as
    (i, JpegRecord) instead -- its coefficient record, `data` a view of shared memory under the same rule -- and every other
    file as pixels."""

    def __init__(self, paths, workers=None, ring_bytes=DEFAULT_RING_BYTES, world=1, records=False):
        self.paths = list(paths)
        self.n_workers = default_workers(world) if workers is None else int(workers)
        self.records = bool(records)
        assert self.n_workers >= 1
        self.cap = max(1 << 20, int(ring_bytes) // self.n_workers)
        self.ring_bytes = self.cap * self.n_workers
        shm_dir = "/dev/shm" if os.path.isdir("/dev/shm") else None
        if shm_dir is None:
            import tempfile
            shm_dir = tempfile.gettempdir()
        self.prefix = os.path.join(shm_dir, f"lemon_decode_{os.getpid()}_{uuid.uuid4().hex[:8]}")
        self.procs, self.rings, self.worker_pids, self.torch_in_worker = [], [], [], []
        self.held = self.peak_held = 0
        self._closed = False
        import mmap
        try:
            for k in range(self.n_workers):
                path = f"{self.prefix}.{k}"
                fd = os.open(path, os.O_CREAT | os.O_EXCL | os.O_RDWR, 0o600)
                os.ftruncate(fd, self.cap)
                self.rings.append(np.frombuffer(mmap.mmap(fd, self.cap), np.uint8))
                os.close(fd)
                self.procs.append(subprocess.Popen([sys.executable, _WORKER, path, str(self.cap), "1" if self.records else "0"], stdin=subprocess.PIPE,
                                                   stdout=subprocess.PIPE, close_fds=True))
            for p in self.procs:
                msg = self._read(p, "worker start")
                self.worker_pids.append(msg[1])
                self.torch_in_worker.append(msg[2])
        except BaseException:
            self.close()
            raise

    def _read(self, proc, what):
        try:
            return pickle.load(proc.stdout)
        except EOFError:
            raise DecodeError(f"decode worker {proc.pid} exited (code {proc.poll()}) while waiting for {what}") from None

    def _send(self, proc, msg):
        pickle.dump(msg, proc.stdin, protocol=pickle.HIGHEST_PROTOCOL)
        proc.stdin.flush()

    def images(self, lo=0, hi=None):
        hi = len(self.paths) if hi is None else hi
        W = self.n_workers
        nxt = lo
        last = None                      # (worker, consumed, oversize) of the image handed out last: freed on the next request
        for i in range(lo, hi):
            if last is not None:
                self._release(*last)
            while nxt < hi and nxt - i < W * LOOKAHEAD_PER_WORKER:
                self._send(self.procs[(nxt - lo) % W], ("task", nxt, self.paths[nxt]))
                nxt += 1
            k = (i - lo) % W
            msg = self._read(self.procs[k], self.paths[i])
            if msg[0] == "err":
                raise DecodeError(f"cannot decode image {msg[2]}: {msg[3]}")
            _, seq, off, h, w, consumed, big, kind, n, meta = msg
            assert seq == i, (seq, i)
            assert kind == 1 or n == h * w * 3, (kind, n, h, w)
            if big is not None:
                import mmap
                fd = os.open(big, os.O_RDONLY)
                arr = np.frombuffer(mmap.mmap(fd, max(n, 1), prot=mmap.PROT_READ), np.uint8)[:n]
                os.close(fd)
                os.unlink(big)
            else:
                arr = self.rings[k][off:off + n]
                self.held += consumed
                self.peak_held = max(self.peak_held, self.held)
            last = (k, consumed, big)
            yield i, (JpegRecord(arr, w, h, *meta) if kind == 1 else arr.reshape(h, w, 3))
        if last is not None:
            self._release(*last)

    def _release(self, k, consumed, big):
        if big is None and consumed:
            self.held -= consumed
            self._send(self.procs[k], ("free", consumed))

    def close(self):
        if self._closed:
            return
        self._closed = True
        for p in self.procs:
            try:
                self._send(p, ("stop",))
                p.stdin.close()
            except (OSError, ValueError):
                pass
        for p in self.procs:
            try:
                p.wait(timeout=5)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
            if p.stdout:
                p.stdout.close()
        self.rings = []
        import glob
        for f in glob.glob(self.prefix + ".*"):
            try:
                os.unlink(f)
            except FileNotFoundError:
                pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


def ragged_batches(paths, chunk, lo, hi, device, workers=None, ring_bytes=DEFAULT_RING_BYTES, world=1, stats=None, slots=3,
                   device_jpeg=None):
    """Yield (s, e, RaggedImages of paths[s:e]) over paths[lo:hi] in chunks of `chunk` images, decoded by a DecodePool.

    A packing thread copies each chunk's decoded images out of the workers' rings into one of `slots` pinned staging buffers
    while the caller embeds the previous chunk; a buffer is refilled only after its last H2D copy has completed.  The copy runs
    as uint8 on a copy stream, into memory allocated on that stream, and only the current stream waits on the copy's event:
    copies overlap the compute already queued.  `stats` (a dict) collects the copies' timing events and bytes
    ("h2d": [(start, end, bytes)]) and the packing thread's seconds ("pack_s").  `device_jpeg` (None: device_jpeg_default()):
    the workers deliver coefficient records for the JPEGs their host pass accepts; the chunk's records, PIL pixels and the aux
    table of lemon_jpeg_decode are packed into the same pinned buffer and copied once into a device buffer laid out
    [copied payload | decoded RGB]; lemon_jpeg_decode runs on the current stream after the copy's event, and the RaggedImages
    offsets point into the payload (PIL images) or the decoded region (JPEGs).  The pool closes (workers exit, segments
    unlinked) when the generator ends, is closed early or raises."""
    import queue
    import threading
    import time

    import torch

    from .data import RaggedImages, RaggedPlans, launch_jpeg_decode
    if device_jpeg is None:
        device_jpeg = device_jpeg_default()
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    copy_stream = torch.cuda.Stream(device)
    free, ready = queue.Queue(), queue.Queue(maxsize=max(1, slots - 1))
    for k in range(slots):
        free.put((k, None, None))                    # (slot, pinned buffer, event of its last copy)
    stop = threading.Event()
    if stats is not None:
        stats.setdefault("pack_s", 0.0)

    def put(q, item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def get(q):
        while not stop.is_set():
            try:
                return q.get(timeout=0.1)
            except queue.Empty:
                pass
        return None

    def pack(pool):
        try:
            torch.cuda.set_device(device)
            it = pool.images(lo, hi)
            for s in range(lo, hi, chunk):
                e = min(hi, s + chunk)
                slot = get(free)
                if slot is None:
                    return
                k, buf, ev = slot
                if ev is not None:
                    ev.synchronize()                 # the buffer's previous H2D copy has completed
                lay, off = BatchLayout(), 0

                def room(buf, off, need):
                    if buf is None or buf.numel() < need:
                        size = (max(need * 2, 64 << 20) + 15) & ~15      # a multiple of 16: holds the rounded `off` below
                        grown = torch.empty((size,), dtype=torch.uint8).pin_memory()
                        if buf is not None and off:
                            grown[:off].copy_(buf[:off])
                        buf = grown
                    return buf

                for _ in range(s, e):
                    _, a = next(it)                  # (a view of the worker's ring, valid until the next image is asked for)
                    t1 = time.perf_counter()
                    src = a.data if isinstance(a, JpegRecord) else a.reshape(-1)
                    need = off + src.nbytes
                    buf = room(buf, off, need)
                    np.copyto(buf.numpy()[off:need], src)
                    if isinstance(a, JpegRecord):
                        lay.add_record(off, a)
                    else:
                        lay.add_pixels(off, a.shape[0], a.shape[1])
                    off = (need + 15) & ~15
                    if stats is not None:
                        stats["pack_s"] += time.perf_counter() - t1
                aux = lay.finish(off)
                if aux.size:
                    buf = room(buf, off, lay.payload_bytes)
                    np.copyto(buf.numpy()[lay.aux_off:lay.payload_bytes], aux.view(np.uint8))
                if not put(ready, (s, e, k, buf, lay)):
                    return
            put(ready, None)
        except BaseException as exc:                 # noqa: BLE001  (re-raised by the consumer)
            put(ready, exc)

    with DecodePool(paths, workers, ring_bytes, world, records=device_jpeg) as pool:
        th = threading.Thread(target=pack, args=(pool,), daemon=True)
        th.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                s, e, k, buf, lay = item
                off = lay.payload_bytes
                n = max(off, 1)
                cur = torch.cuda.current_stream(device)
                timed = stats is not None
                with torch.cuda.stream(copy_stream):
                    data = torch.empty((max(lay.total_bytes, n),), dtype=torch.uint8, device=device)
                    if timed:
                        t0 = torch.cuda.Event(enable_timing=True)
                        t0.record(copy_stream)
                    data[:n].copy_(buf[:n], non_blocking=True)
                    ev = torch.cuda.Event(enable_timing=timed)
                    ev.record(copy_stream)
                data.record_stream(cur)                  # freed only after the compute stream is done with it
                cur.wait_event(ev)
                free.put((k, buf, ev))
                if timed:
                    stats.setdefault("h2d", []).append((t0, ev, off))
                    stats["jpeg_images"] = stats.get("jpeg_images", 0) + lay.n_jpeg
                launch_jpeg_decode(data, lay)            # (on the current stream, after the copy's event; nothing without records)
                yield s, e, RaggedImages(data, np.array(lay.desc, np.int64).reshape(-1, 4), RaggedPlans(lay.shapes))
        finally:
            stop.set()
            th.join()
