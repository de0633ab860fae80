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
  * with LEMON_JPEG=device the workers do not decode at all: they strip a baseline JPEG down to its scan packet (lemon_jpeg_pack),
    the file crosses PCIe compressed, and lemon_jpeg_entropy_device runs the Huffman pass on the GPU in front of
    lemon_jpeg_decode.  The statuses come back through pinned memory behind an event; a chunk is handed out after it, one chunk
    behind the one being enqueued, so the wait falls into the previous chunk's embedding.  The rare image the device declines is
    decoded with PIL in the parent and copied into its slot.
The held decoded bytes are bounded by `ring_bytes` (one ring of ring_bytes / workers per worker; an image larger than a whole
ring is decoded alone, when its worker's ring is empty)."""
import os
import pickle
import subprocess
import sys
import uuid

import numpy as np

from .jpeg_host import BatchLayout, JpegPacket, JpegProgPacket, JpegProgRecord, JpegRecord
from .png_host import PngRecord, PngStream

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
    """How file batches decode baseline JPEGs: LEMON_JPEG=pil (False: all by PIL in the workers), gpu (True: Huffman pass in the
    workers, the rest on the GPU) or device ("device": the Huffman pass on the GPU too).  Default pil: the recorded end-to-end
    comparison does not yet justify another default; results are identical in all three."""
    env = os.environ.get("LEMON_JPEG", "").strip().lower()
    if env == "gpu":
        return True
    if env == "device":
        return "device"
    if env in ("", "pil"):
        return False
    raise ValueError(f"LEMON_JPEG={env!r}: expected 'pil', 'gpu' or 'device'")


def progressive_default():
    """Whether file batches send progressive JPEGs through the progressive Huffman pass: LEMON_JPEG_PROGRESSIVE=1 (default 0:
    PIL decodes them in the workers).  Ignored under LEMON_JPEG=pil."""
    env = os.environ.get("LEMON_JPEG_PROGRESSIVE", "").strip()
    if env in ("", "0"):
        return False
    if env == "1":
        return True
    raise ValueError(f"LEMON_JPEG_PROGRESSIVE={env!r}: expected '0' or '1'")


def png_default():
    """How file batches decode PNGs: LEMON_PNG=pil (False: all by PIL in the workers), gpu (True: chunk walk and inflate in the
    workers, unfiltering and the expansion to RGB on the GPU) or device (True: the inflate on the GPU as well,
    png_inflate_default()).  Default pil until a recorded comparison exists; results are identical in
    all three."""
    env = os.environ.get("LEMON_PNG", "").strip().lower()
    if env in ("gpu", "device"):
        return True
    if env in ("", "pil"):
        return False
    raise ValueError(f"LEMON_PNG={env!r}: expected 'pil', 'gpu' or 'device'")


def png_inflate_default():
    """Whether the PNGs of file batches cross to the GPU compressed and are inflated there: LEMON_PNG=device only."""
    return png_default() and os.environ.get("LEMON_PNG", "").strip().lower() == "device"


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
    file as pixels.  With packets=True a baseline JPEG whose header the packer accepts is yielded as (i, JpegPacket): its scan
    packet for lemon_jpeg_entropy_device.  progressive=True (with records or packets): a progressive JPEG is not left to PIL
    but yielded as (i, JpegProgRecord) -- the same record, from the progressive host pass -- or (i, JpegProgPacket).
    png=True: a PNG that png_host accepts is yielded as (i, PngRecord) -- palette + filtered scanlines for lemon_png_decode.
    png_streams=True (with png): the workers do not inflate; a PNG whose chunk walk passes is yielded as (i, PngStream) -- palette
    + compressed IDAT payload for lemon_png_inflate."""

    def __init__(self, paths, workers=None, ring_bytes=DEFAULT_RING_BYTES, world=1, records=False, packets=False, progressive=False,
                 png=False, png_streams=False):
        self.paths = list(paths)
        self.png_streams = bool(png_streams) and bool(png)
        self.progressive = bool(progressive)
        self.png = bool(png)
        self.n_workers = default_workers(world) if workers is None else int(workers)
        self.records, self.packets = bool(records) and not packets, bool(packets)
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
                self.procs.append(subprocess.Popen([sys.executable, _WORKER, path, str(self.cap), "2" if self.packets else "1" if self.records else "0",
                                                    "1" if self.progressive else "0"] + (["1"] if self.png else []) + (["1"] if self.png_streams else []),
                                                   stdin=subprocess.PIPE,
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
            assert kind in (1, 2, 3, 4, 5, 6) or n == h * w * 3, (kind, n, h, w)
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
            made = {1: JpegRecord, 2: JpegPacket, 3: JpegProgRecord, 4: JpegProgPacket, 5: PngRecord, 6: PngStream}.get(kind)
            yield i, (made(arr, w, h, *meta) if made else arr.reshape(h, w, 3))
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
                   device_jpeg=None, progressive=None, device_png=None, png_inflate=None):
    """Yield (s, e, RaggedImages of paths[s:e]) over paths[lo:hi] in chunks of `chunk` images, decoded by a DecodePool.

    A packing thread copies each chunk's decoded images out of the workers' rings into one of `slots` pinned staging buffers
    while the caller embeds the previous chunk; a buffer is refilled only after its last H2D copy has completed.  The copy runs
    as uint8 on a copy stream, into memory allocated on that stream, and only the current stream waits on the copy's event:
    copies overlap the compute already queued.  `stats` (a dict) collects the copies' timing events and bytes
    ("h2d": [(start, end, bytes)]), the packing thread's seconds copying ("pack_s") and waiting for the workers ("pool_wait_s"),
    the caller's seconds waiting for a packed chunk ("ready_wait_s") and for the statuses of the device Huffman pass
    ("status_wait_s").  `device_jpeg` (None: device_jpeg_default()):
    the workers deliver coefficient records for the JPEGs their host pass accepts; the chunk's records, PIL pixels and the aux
    table of lemon_jpeg_decode are packed into the same pinned buffer and copied once into a device buffer laid out
    [copied payload | decoded RGB]; lemon_jpeg_decode runs on the current stream after the copy's event, and the RaggedImages
    offsets point into the payload (PIL images) or the decoded region (JPEGs).  device_jpeg="device": the workers deliver scan
    packets, lemon_jpeg_entropy_device, lemon_jpeg_decode and an asynchronous copy of the statuses to (reused) pinned memory are
    enqueued behind the chunk's copy on a stream of their own, and the chunk is handed out after its status event, when the
    compute stream joins that stream, while the next chunk is already enqueued; an
    image the device declines is read again from its path, decoded by PIL here and copied into its RGB slot (a file PIL cannot
    decode raises DecodeError as in pil mode).  `progressive` (None: LEMON_JPEG_PROGRESSIVE=1; ignored in pil mode): progressive
    files are not left to PIL in the workers but take the progressive Huffman pass, in the workers (gpu) or on the device behind
    the baseline pass (device); stats["jpeg_progressive"] counts them.  `device_png` (None: png_default(), LEMON_PNG=gpu): the
    workers deliver the PNGs they accept as records (palette + filtered scanlines); these ride in the same pinned buffer,
    lemon_png_decode is enqueued behind the chunk's copy and its statuses take the route of the device Huffman pass's -- an
    asynchronous copy to pinned memory, the chunk handed out one chunk later, PIL filling the slots of the images the kernel
    declined (a filter byte above 4, a palette index beyond PLTE); stats["png_records"] counts the records, stats["png_fallback"]
    those slots.  `png_inflate` (None: png_inflate_default(), LEMON_PNG=device; needs device_png): the workers deliver the PNGs
    whose chunk walk passes as streams (palette + compressed IDAT payload); the records are allocated on the device only,
    lemon_png_inflate writes them and lemon_png_decode runs next on the same stream; an image either kernel declines (the first
    non-zero of the two statuses) is filled by PIL; stats["png_streams"] counts the streams.  Both compose with every
    `device_jpeg` mode.  The pool closes (workers exit, segments
    unlinked) when the generator ends, is closed early or raises."""
    import queue
    import threading
    import time

    import torch

    from .data import RaggedImages, RaggedPlans, launch_jpeg_decode, launch_jpeg_entropy, launch_png_decode, launch_png_inflate, first_png_status
    if device_jpeg is None:
        device_jpeg = device_jpeg_default()
    if device_png is None:
        device_png = png_default()
    device_png = bool(device_png)
    if png_inflate is None:
        png_inflate = png_inflate_default()
    png_inflate = bool(png_inflate) and device_png
    packets = device_jpeg == "device"
    if progressive is None:
        progressive = progressive_default()
    progressive = bool(progressive) and bool(device_jpeg)
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
                    t0 = time.perf_counter()
                    _, a = next(it)                  # (a view of the worker's ring, valid until the next image is asked for)
                    t1 = time.perf_counter()
                    if stats is not None:
                        stats["pool_wait_s"] = stats.get("pool_wait_s", 0.0) + t1 - t0
                    src = a.data if isinstance(a, (JpegRecord, JpegPacket, JpegProgRecord, JpegProgPacket, PngRecord, PngStream)) else a.reshape(-1)
                    need = off + src.nbytes
                    buf = room(buf, off, need)
                    np.copyto(buf.numpy()[off:need], src)
                    if isinstance(a, (JpegPacket, JpegProgPacket)):
                        lay.add_packet(off, a)
                    elif isinstance(a, (JpegRecord, JpegProgRecord)):
                        lay.add_record(off, a)
                    elif isinstance(a, PngRecord):
                        lay.add_png_record(off, a)
                    elif isinstance(a, PngStream):
                        lay.add_png_stream(off, a)
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

    def finished(s, e, data, lay, status, ev, png_status=None):
        """The chunk once its statuses have arrived: the images the device declined are decoded by PIL into their slots."""
        torch.cuda.current_stream(device).wait_event(ev)
        if status is not None or png_status is not None:
            t0 = time.perf_counter()
            ev.synchronize()
            if stats is not None:
                stats["status_wait_s"] = stats.get("status_wait_s", 0.0) + time.perf_counter() - t0
            declined = [(lay.records[lay.status_record(k)][0], "jpeg_fallback") for k in np.flatnonzero(status.numpy())] if status is not None else []
            if png_status is not None:
                declined += [(lay.png_records[k][0], "png_fallback") for k in np.flatnonzero(png_status.numpy())]
            for i, counter in declined:
                from PIL import Image
                o, h, w, _ = lay.desc[i]
                try:
                    px = np.asarray(Image.open(paths[s + i]).convert("RGB"), dtype=np.uint8)
                except Exception as exc:             # noqa: BLE001  (what the worker reports in pil mode)
                    raise DecodeError(f"cannot decode image {paths[s + i]}: {type(exc).__name__}: {exc}") from None
                if px.shape != (h, w, 3):
                    raise DecodeError(f"cannot decode image {paths[s + i]}: PIL reads {px.shape}, its header says {(h, w, 3)}")
                data[o:o + px.size].copy_(torch.from_numpy(px.reshape(-1).copy()))
                if stats is not None:
                    stats[counter] = stats.get(counter, 0) + 1
        return s, e, RaggedImages(data, np.array(lay.desc, np.int64).reshape(-1, 4), RaggedPlans(lay.shapes))

    with DecodePool(paths, workers, ring_bytes, world, records=bool(device_jpeg), packets=packets, progressive=progressive,
                    png=device_png, png_streams=png_inflate) as pool:
        th = threading.Thread(target=pack, args=(pool,), daemon=True)
        th.start()
        pending, n_chunks, pinned_status, pinned_png = None, 0, [None, None, None], [None, None, None]
        jpeg_stream = torch.cuda.Stream(device) if packets or device_png else None
        try:
            while True:
                t_wait = time.perf_counter()
                item = ready.get()
                if stats is not None:
                    stats["ready_wait_s"] = stats.get("ready_wait_s", 0.0) + time.perf_counter() - t_wait
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
                    stats["jpeg_progressive"] = stats.get("jpeg_progressive", 0) + lay.n_progressive
                if timed and device_png:
                    stats["png_records"] = stats.get("png_records", 0) + lay.n_png
                if timed and png_inflate:
                    stats["png_streams"] = stats.get("png_streams", 0) + len(lay.png_streams)
                if not packets and not device_png:
                    launch_jpeg_decode(data, lay)        # (on the current stream, after the copy's event; nothing without records)
                    yield s, e, RaggedImages(data, np.array(lay.desc, np.int64).reshape(-1, 4), RaggedPlans(lay.shapes))
                    continue
                # the Huffman pass, the rest of the decode and the statuses' way back run on a stream of their own, behind the
                # copy only: they overlap the embedding queued on the compute stream, and waiting for the statuses waits for
                # nothing else.  The compute stream joins when the chunk is handed out (finished()).
                status = sev = None
                with torch.cuda.stream(jpeg_stream):
                    jpeg_stream.wait_event(ev)
                    status_dev = launch_jpeg_entropy(data, lay)
                    launch_jpeg_decode(data, lay)
                    if status_dev is not None:
                        if pinned_status[n_chunks % 3] is None or pinned_status[n_chunks % 3].numel() < status_dev.numel():
                            pinned_status[n_chunks % 3] = torch.empty((max(chunk, status_dev.numel()),), dtype=torch.int32).pin_memory()
                        status = pinned_status[n_chunks % 3][:status_dev.numel()]      # (at most two chunks are in flight)
                        status.copy_(status_dev, non_blocking=True)
                    png_status = None
                    png_dev = first_png_status(launch_png_inflate(data, lay), launch_png_decode(data, lay)) if device_png else None
                    if png_dev is not None:
                        if pinned_png[n_chunks % 3] is None or pinned_png[n_chunks % 3].numel() < png_dev.numel():
                            pinned_png[n_chunks % 3] = torch.empty((max(chunk, png_dev.numel()),), dtype=torch.int32).pin_memory()
                        png_status = pinned_png[n_chunks % 3][:png_dev.numel()]
                        png_status.copy_(png_dev, non_blocking=True)
                    sev = torch.cuda.Event()
                    sev.record(jpeg_stream)
                data.record_stream(jpeg_stream)
                n_chunks += 1
                # hand out the chunk enqueued before this one: its statuses arrived while this one was being packed
                if pending is not None:
                    yield finished(*pending)
                pending = (s, e, data, lay, status, sev, png_status)
            if pending is not None:
                yield finished(*pending)
        finally:
            stop.set()
            th.join()
