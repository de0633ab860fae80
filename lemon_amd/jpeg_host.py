"""ctypes binding of liblemon_jpeg_host.so (the JPEG host pass, csrc/jpeg_entropy.hpp) and the batch layout of
lemon_jpeg_decode (include/lemon_hip.h).  Imports ctypes and numpy only -- never torch, never the HIP library -- because the
decode workers (decode_worker.py, run by path) import it as a top-level module; the package imports it as lemon_amd.jpeg_host.
"""
import ctypes
import os
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "liblemon_jpeg_host.so")
IDCT_GROUP = 32          # blocks per inverse-DCT workgroup (csrc/jpeg.hip: JPEG_GROUP)
RGB_PIXELS = 4           # pixels per lane of the colour kernel (JPEG_PIX), 256 lanes per workgroup
QUANT_BYTES = 384
STATUS = {0: "ok", 1: "not a JPEG", 2: "truncated header", 3: "progressive / arithmetic / lossless process", 4: "not 8-bit",
          5: "not 1 or 3 components", 6: "unsupported sampling factors", 7: "not YCbCr (Adobe marker or component ids)",
          8: "bad or unsupported table", 9: "not one interleaved scan", 10: "bad Huffman code or coefficient",
          11: "bit stream ends early or runs past its last MCU", 12: "outside the arithmetic envelope", 13: "record buffer too small",
          14: "zero dimension", 15: "unexpected marker", 16: "parallel Huffman states did not settle",
          17: "progression incomplete at EOI"}
PACKET_BOUND = 2752      # include/lemon_hip.h: LEMON_JPEG_PACKET_BOUND
PROG_PACKET_BOUND = 5424  # include/lemon_hip.h: LEMON_JPEG_PROG_PACKET_BOUND
SUBSEQ_MIN, SUBSEQ_DEFAULT, PAR_GROUP = 16, 256, 256      # bytes per lane (smallest, default), lanes per workgroup (csrc/jpeg_par.hpp)


class Info(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32),
                ("max_abs", ctypes.c_int32), ("exact_blocks", ctypes.c_int32), ("blocks", ctypes.c_int64),
                ("record_bytes", ctypes.c_int64), ("quant", (ctypes.c_uint16 * 64) * 3)]


# a coefficient record of one accepted file: `data` uint8 [record_bytes] (a view; copy it to keep it)
JpegRecord = namedtuple("JpegRecord", "data w h components hs vs")

# the scan packet of one file whose header pass accepts it (csrc/jpeg_par.hpp): `data` uint8 [packet bytes] (a view)
JpegPacket = namedtuple("JpegPacket", "data w h components hs vs intervals scan_bytes")

# the record of a progressive file: the same record, told apart only to be counted
JpegProgRecord = namedtuple("JpegProgRecord", "data w h components hs vs")

# the packet of one progressive file (csrc/jpeg_prog_par.hpp): `items` waves decode it in `levels` launches
JpegProgPacket = namedtuple("JpegProgPacket", "data w h components hs vs scans items levels")

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: build it with `python -m lemon_amd.build`")
        lib = ctypes.CDLL(SO_PATH)
        vp, c_i64, c_i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
        lib.lemon_jpeg_info.argtypes = [ctypes.c_char_p, c_i64, ctypes.POINTER(Info)]
        lib.lemon_jpeg_entropy.argtypes = [ctypes.c_char_p, c_i64, vp, c_i64, ctypes.POINTER(Info)]
        lib.lemon_jpeg_reconstruct_host.argtypes = [vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, vp]
        lib.lemon_jpeg_pack.argtypes = [ctypes.c_char_p, c_i64, vp, c_i64, ctypes.POINTER(Info), ctypes.POINTER(c_i64)]
        lib.lemon_jpeg_entropy_par_host.argtypes = [vp, c_i64, c_i32, vp, c_i64, ctypes.POINTER(c_i32)]
        lib.lemon_jpeg_prog_info.argtypes = [ctypes.c_char_p, c_i64, ctypes.POINTER(Info)]
        lib.lemon_jpeg_prog_entropy.argtypes = [ctypes.c_char_p, c_i64, vp, c_i64, ctypes.POINTER(Info)]
        lib.lemon_jpeg_prog_pack.argtypes = [ctypes.c_char_p, c_i64, vp, c_i64, ctypes.POINTER(Info), ctypes.POINTER(c_i64)]
        lib.lemon_jpeg_prog_entropy_par_host.argtypes = [vp, c_i64, vp, c_i64, ctypes.POINTER(c_i32)]
        _lib = lib
    return _lib


def info(data, progressive=False):
    """Header pass over the bytes of a file -> Info (status 0: accepted so far, record_bytes known).  progressive: a file the
    baseline pass declines as status 3 is given to the progressive pass (csrc/jpeg_prog.hpp)."""
    out = Info()
    load().lemon_jpeg_info(data, len(data), ctypes.byref(out))
    return prog_info(data) if progressive and out.status == 3 else out


def prog_info(data):
    """Header pass of the progressive decode (csrc/jpeg_prog.hpp): SOF2 files only, a baseline file is status 3."""
    out = Info()
    load().lemon_jpeg_prog_info(data, len(data), ctypes.byref(out))
    return out


def entropy(data, record, progressive=False):
    """The host pass over the bytes of a file into `record` (a writable contiguous uint8 numpy array) -> Info."""
    assert record.dtype == np.uint8 and record.flags.c_contiguous and record.flags.writeable
    out = Info()
    load().lemon_jpeg_entropy(data, len(data), record.ctypes.data, record.size, ctypes.byref(out))
    return prog_entropy(data, record) if progressive and out.status == 3 else out


def prog_entropy(data, record):
    """The host pass over the bytes of a progressive file into `record` -> Info."""
    assert record.dtype == np.uint8 and record.flags.c_contiguous and record.flags.writeable
    out = Info()
    load().lemon_jpeg_prog_entropy(data, len(data), record.ctypes.data, record.size, ctypes.byref(out))
    return out


def decode_record(data, progressive=False):
    """bytes -> (JpegRecord, Info) or (None, Info) when the host pass declines the file.  progressive: a progressive file
    goes through the progressive pass -> (JpegProgRecord, Info)."""
    head = info(data)
    prog = progressive and head.status == 3
    if prog:
        head = prog_info(data)
    if head.status != 0:
        return None, head
    rec = np.empty(head.record_bytes, np.uint8)
    full = prog_entropy(data, rec) if prog else entropy(data, rec)
    if full.status != 0:
        return None, full
    return (JpegProgRecord if prog else JpegRecord)(rec, full.width, full.height, full.components, full.hs, full.vs), full


def packet_cap(n):
    """A capacity that holds the packet of any n-byte file."""
    return n + n // 8192 + PACKET_BOUND + 16


def prog_packet_cap(n):
    """A capacity that holds the progressive packet of any n-byte file (csrc/jpeg_prog_par.hpp)."""
    return n + 2 * (n // 3) + PROG_PACKET_BOUND + 16


def pack(data, out=None, progressive=False):
    """Header pass + scan packet of the bytes of a file -> (JpegPacket or None when declined, Info).  `out`: a writable
    contiguous uint8 array of at least packet_cap(len(data)) bytes, 16-byte aligned, to write into (default: a new one).
    progressive: a file declined as status 3 is packed by lemon_jpeg_prog_pack -> JpegProgPacket; `out` then needs
    max(packet_cap, prog_packet_cap)(len(data)) bytes."""
    if out is None:
        out = np.empty(max(packet_cap(len(data)), prog_packet_cap(len(data)) if progressive else 0), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable
    head, nbytes = Info(), ctypes.c_int64(0)
    load().lemon_jpeg_pack(data, len(data), out.ctypes.data, out.size, ctypes.byref(head), ctypes.byref(nbytes))
    if progressive and head.status == 3:
        return prog_pack(data, out)
    if head.status != 0:
        return None, head
    pk = out[:nbytes.value]
    meta = pk[:64].view(np.int32)          # (csrc/jpeg_par.hpp: kPkIntervals = 7, kPkScanBytes = 8)
    return JpegPacket(pk, head.width, head.height, head.components, head.hs, head.vs, int(meta[7]), int(meta[8])), head


def prog_pack(data, out=None):
    """All header and marker checks + the packet of a progressive file (csrc/jpeg_prog_par.hpp) -> (JpegProgPacket or None when
    declined, Info).  `out`: as pack(), of at least prog_packet_cap(len(data)) bytes."""
    if out is None:
        out = np.empty(prog_packet_cap(len(data)), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable
    head, nbytes = Info(), ctypes.c_int64(0)
    load().lemon_jpeg_prog_pack(data, len(data), out.ctypes.data, out.size, ctypes.byref(head), ctypes.byref(nbytes))
    if head.status != 0:
        return None, head
    pk = out[:nbytes.value]
    meta = pk[:64].view(np.int32)          # (csrc/jpeg_prog_par.hpp: kHScans = 6, kHItems = 8, kHLevels = 9)
    return JpegProgPacket(pk, head.width, head.height, head.components, head.hs, head.vs, int(meta[6]), int(meta[8]), int(meta[9])), head


def entropy_par_host(packet, record, subseq=0):
    """The device's parallel Huffman pass with its lanes looped on the host: packet (uint8 array) -> `record`, returns the
    status.  For tests."""
    packet = np.ascontiguousarray(packet)
    assert record.dtype == np.uint8 and record.flags.c_contiguous and record.flags.writeable
    st = ctypes.c_int32(-1)
    if load().lemon_jpeg_entropy_par_host(packet.ctypes.data, packet.size, subseq, record.ctypes.data, record.size, ctypes.byref(st)) != 0:
        raise ValueError("lemon_jpeg_entropy_par_host: bad arguments")
    return st.value


def prog_entropy_par_host(packet, record):
    """The device's progressive Huffman pass with its waves looped on the host: packet (uint8 array, 16-byte aligned) ->
    `record`, returns the status.  For tests."""
    packet = np.ascontiguousarray(packet)
    assert record.dtype == np.uint8 and record.flags.c_contiguous and record.flags.writeable
    st = ctypes.c_int32(-1)
    if load().lemon_jpeg_prog_entropy_par_host(packet.ctypes.data, packet.size, record.ctypes.data, record.size, ctypes.byref(st)) != 0:
        raise ValueError("lemon_jpeg_prog_entropy_par_host: bad arguments")
    return st.value


def groups_of(scan_bytes, intervals, subseq=0):
    """Workgroups lemon_jpeg_entropy_device needs for a packet (include/lemon_hip.h)."""
    s = subseq or SUBSEQ_DEFAULT
    return -(-(-(-scan_bytes // s) + intervals) // PAR_GROUP)


def reconstruct(rec):
    """The device arithmetic on the host (csrc/jpeg_core.hpp): JpegRecord -> uint8 [h, w, 3].  For tests."""
    out = np.empty((rec.h, rec.w, 3), np.uint8)
    data = np.ascontiguousarray(rec.data)
    rc = load().lemon_jpeg_reconstruct_host(data.ctypes.data, data.size, rec.w, rec.h, rec.components, rec.hs, rec.vs, out.ctypes.data)
    if rc != 0:
        raise ValueError("lemon_jpeg_reconstruct_host: bad record geometry")
    return out


def blocks_of(w, h, components, hs, vs):
    """8x8 blocks of all components over the MCU-padded grid (csrc/jpeg_core.hpp::jpeg_geometry)."""
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    return mx * hs * my * vs + (2 * mx * my if components == 3 else 0)


def _up(n, a=16):
    return (n + a - 1) // a * a


class BatchLayout:
    """Layout of one device buffer [payload: packets, PIL pixels, records, aux | records of the packets, baseline then progressive | decoded RGB] for a chunk
    of images.  The payload (filled by the caller, `off` bytes so far) holds PIL pixels, coefficient records and scan packets at
    16-byte aligned offsets; finish() appends the int64 aux tables of lemon_jpeg_decode and lemon_jpeg_entropy_device to the
    payload, gives every packet a record in the device-only region after it (written by lemon_jpeg_entropy_device) and places
    every JPEG's pixels after that.  `desc` is the RaggedImages table (byte offset, H, W, plan index) in the order the images
    were added.  `subseq`: bytes per lane of the device Huffman pass (0 = its default).
    PNG records (png_host.PngRecord, add_png_record) ride in the same payload; a batch that holds some gains, behind everything a
    JPEG-only batch holds -- whose bytes and offsets stay what they are --, the aux table of lemon_png_decode at the end of the
    payload (png_aux_off) and the PNGs' pixels at the end of the buffer (png_decoded_off).
    PNG streams (png_host.PngStream, add_png_stream: palette + compressed IDAT payload, LEMON_PNG=device) ride in the payload
    instead of their records; their records are device-only, between everything else and the PNGs' pixels (png_rec_off ..
    png_rec_end), written by lemon_png_inflate from its own table (png_zaux_off, behind lemon_png_decode's).  A batch's PNGs are
    all records or all streams."""

    def __init__(self, subseq=0):
        self.shapes, self.desc, self.records, self.packets, self.subseq = {}, [], [], [], subseq
        self.prog_packets, self.n_progressive = [], 0
        self.png_records, self.n_png, self.png_work_bytes = [], 0, 16
        self.png_streams = []

    def add_png_record(self, off, rec):
        """A PNG record (png_host.PngRecord) at payload offset `off`, a multiple of 16."""
        self.png_records.append((len(self.desc), off, rec.h, rec.w, rec.colour_type, rec.plte_count))
        self.desc.append([-1, rec.h, rec.w, self.shapes.setdefault((rec.h, rec.w), len(self.shapes))])

    def add_png_stream(self, off, s):
        """A PNG stream (png_host.PngStream) at payload offset `off`, a multiple of 16: its record's offset is known after
        finish()."""
        self.png_streams.append((len(self.png_records), off, s.z_bytes, 1024 + s.h * (s.w * s.channels + 1)))
        self.png_records.append((len(self.desc), -1, s.h, s.w, s.colour_type, s.plte_count))
        self.desc.append([-1, s.h, s.w, self.shapes.setdefault((s.h, s.w), len(self.shapes))])

    def add_packet(self, off, pk):
        """A scan packet at payload offset `off`: its record lies in the device-only region (offset known after finish()).
        A JpegProgPacket goes to the progressive pass's own table (`prog_packets`)."""
        if isinstance(pk, JpegProgPacket):
            self.prog_packets.append((len(self.records), off, pk.data.nbytes, pk.items, pk.levels))
        else:
            self.packets.append((len(self.records), off, pk.data.nbytes, pk.intervals, pk.scan_bytes))
        self.add_record(-1, pk)

    def status_record(self, k):
        """Index into `records` of entry k of launch_jpeg_entropy's statuses: the baseline packets, then the progressive ones."""
        return self.packets[k][0] if k < len(self.packets) else self.prog_packets[k - len(self.packets)][0]

    def add_pixels(self, off, h, w):
        self.desc.append([off, h, w, self.shapes.setdefault((h, w), len(self.shapes))])

    def add_record(self, off, rec):
        self.n_progressive += isinstance(rec, (JpegProgRecord, JpegProgPacket))
        self.records.append((len(self.desc), off, rec.w, rec.h, rec.components, rec.hs, rec.vs))
        self.desc.append([-1, rec.h, rec.w, self.shapes.setdefault((rec.h, rec.w), len(self.shapes))])

    def aux_bytes(self):
        n = len(self.records)
        return 8 * (8 * n + 2 * (n + 1)) + 64 * (len(self.packets) + len(self.prog_packets)) if n else 0

    def finish(self, off):
        """`off`: end of the images' payload.  -> the aux table (int64, to be copied to payload offset self.aux_off)."""
        n = len(self.records)
        self.aux_off = _up(off)
        self.payload_bytes = self.aux_off + self.aux_bytes()
        self.n_png = len(self.png_records)
        if self.n_png:                 # the PNG aux table: the payload's last part
            self.png_aux_off = _up(self.payload_bytes)
            self.payload_bytes = self.png_aux_off + 64 * self.n_png
            assert len(self.png_streams) in (0, self.n_png), "a batch's PNGs are all records or all streams"
            self.png_zaux_off = self.payload_bytes
            self.payload_bytes += 32 * len(self.png_streams)
        # records of the packets: device-only, after the copied payload
        rec = _up(self.payload_bytes)
        self.edesc_off = self.aux_off + 8 * (8 * n + 2 * (n + 1))
        edesc = np.zeros((len(self.packets), 8), np.int64)
        groups = intervals = 0
        for k, (j, poff, pbytes, nivl, scan_bytes) in enumerate(self.packets):
            i, _, w, h, nc, hs, vs = self.records[j]
            self.records[j] = (i, rec, w, h, nc, hs, vs)
            ng = groups_of(scan_bytes, nivl, self.subseq)
            edesc[k] = (poff, pbytes, rec, nivl, groups, intervals, ng, 0)
            groups, intervals = groups + ng, intervals + nivl
            rec += QUANT_BYTES + 128 * blocks_of(w, h, nc, hs, vs)
        # the progressive packets' records follow, with a descriptor table of their own (lemon_jpeg_prog_entropy_device)
        self.pdesc_off = self.edesc_off + 64 * len(self.packets)
        pdesc = np.zeros((len(self.prog_packets), 8), np.int64)
        items = levels = 0
        for k, (j, poff, pbytes, nitems, nlevels) in enumerate(self.prog_packets):
            i, _, w, h, nc, hs, vs = self.records[j]
            self.records[j] = (i, rec, w, h, nc, hs, vs)
            pdesc[k] = (poff, pbytes, rec, items, nitems, 0, 0, 0)
            items, levels = items + nitems, max(levels, nlevels)
            rec += QUANT_BYTES + 128 * blocks_of(w, h, nc, hs, vs)
        self.n_prog, self.prog_items, self.prog_levels = len(self.prog_packets), items, levels
        self.rec_end = rec if self.packets or self.prog_packets else self.payload_bytes
        self.n_packets, self.groups, self.intervals = len(self.packets), groups, intervals
        out, work = _up(self.rec_end), 0
        d8 = np.zeros((n, 8), np.int64)
        apre, bpre = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        for j, (i, roff, w, h, nc, hs, vs) in enumerate(self.records):
            nb = blocks_of(w, h, nc, hs, vs)
            d8[j] = (roff, out, w, h, nc, hs, vs, work)
            self.desc[i][0] = out
            apre[j + 1] = apre[j] + -(-nb // IDCT_GROUP)
            bpre[j + 1] = bpre[j] + -(-(h * -(-w // RGB_PIXELS)) // 256)
            out = _up(out + h * w * 3)
            work += nb * 64
        self.decoded_off = _up(self.rec_end)
        self.total_bytes, self.work_bytes = max(out, 1), max(work, 16)
        self.idct_blocks, self.rgb_blocks, self.n_jpeg = int(apre[-1]), int(bpre[-1]), n
        aux = np.concatenate([d8.ravel(), apre, bpre, edesc.ravel(), pdesc.ravel()]) if n else np.zeros(0, np.int64)
        if not self.n_png:
            return aux
        # the PNGs' pixels follow everything else; lemon_png_decode's table: record offset, h, w, colour type, PLTE count, output
        # offset, work offset (one uint32 per pixel of a row, include/lemon_hip.h), 0
        out = _up(self.total_bytes)
        # the streams' records, device-only; lemon_png_inflate's table: stream offset, stream bytes, offset of the scanlines, want
        z4 = np.zeros((len(self.png_streams), 4), np.int64)
        self.png_rec_off = out
        for j, (k, zoff, zbytes, rbytes) in enumerate(self.png_streams):
            i, _, h, w, ct, plte = self.png_records[k]
            self.png_records[k] = (i, out, h, w, ct, plte)
            z4[j] = (zoff + 1024, zbytes, out + 1024, rbytes - 1024)
            out = _up(out + rbytes)
        self.png_rec_end = out if self.png_streams else self.payload_bytes
        self.png_decoded_off = out
        g8, work = np.zeros((self.n_png, 8), np.int64), 0
        for j, (i, roff, h, w, ct, plte) in enumerate(self.png_records):
            g8[j] = (roff, h, w, ct, plte, out, work, 0)
            self.desc[i][0] = out
            out = _up(out + h * w * 3)
            work += _up(4 * w)
        self.total_bytes, self.png_work_bytes = out, max(work, 16)
        pad = np.zeros((self.png_aux_off - self.aux_off) // 8 - aux.size, np.int64)      # (up to the 16-byte boundary)
        return np.concatenate([aux, pad, g8.ravel(), z4.ravel()])
