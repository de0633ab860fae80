"""The workers' half of the PNG decode (lib/datasets/dataloader.py:177-184 opens the file with PIL): ctypes binding of the chunk
parser in liblemon_jpeg_host.so (csrc/png_core.hpp) and the inflate step, Python's zlib.  Imports ctypes, zlib and numpy only --
never torch, never the HIP library -- because the decode workers (decode_worker.py, run by path) import it as a top-level
module; the package imports it as lemon_amd.png_host.

Record of an accepted file (csrc/png_core.hpp): 256 x 4 palette bytes (R, G, B, 0; zeros beyond the PLTE count), then the
filtered scanlines exactly as inflated, each row behind its filter-type byte: 1024 + h * (w * channels + 1) bytes.  The device
(lemon_png_decode) unfilters and expands it to RGB.

With LEMON_PNG=device the inflate moves to the device as well (lemon_png_inflate): pack_stream does the chunk walk and the CRCs
and hands over a PngStream -- the palette and the concatenated IDAT payload, still compressed -- and no zlib runs here."""
import ctypes
import os
import zlib
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "liblemon_jpeg_host.so")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
PALETTE_BYTES = 1024
# LemonPngStatus (csrc/png_core.hpp) and the two device verdicts (include/lemon_hip.h)
OK, NOT_PNG, TRUNCATED, CRC, HEADER, DEPTH, INTERLACE, PALETTE, CHUNK_ORDER, ANIMATED, DIMENSION, BUFFER, STREAM, FILTER, INDEX = range(15)
STATUS = {OK: "ok", NOT_PNG: "not a PNG", TRUNCATED: "truncated file", CRC: "chunk CRC mismatch", HEADER: "bad header or unknown critical chunk",
          DEPTH: "not 8-bit samples", INTERLACE: "interlaced (Adam7)", PALETTE: "missing or malformed PLTE",
          CHUNK_ORDER: "chunks out of order", ANIMATED: "animated (acTL)", DIMENSION: "zero or oversized dimension",
          BUFFER: "buffer too small", STREAM: "zlib stream does not yield exactly the scanlines", FILTER: "filter type above 4",
          INDEX: "palette index beyond PLTE"}


class Info(ctypes.Structure):      # LemonPngInfo
    _fields_ = [("status", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("colour_type", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("plte_count", ctypes.c_int32), ("idat_spans", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("stride", ctypes.c_int64), ("record_bytes", ctypes.c_int64), ("idat_bytes", ctypes.c_int64),
                ("idat_offset", ctypes.c_int64), ("plte_offset", ctypes.c_int64)]


# the record of one accepted file: `data` uint8 [record_bytes] (a view; copy it to keep it)
PngRecord = namedtuple("PngRecord", "data w h colour_type channels plte_count")

# an accepted file before the inflate: `data` uint8 [1024 + z_bytes] (a view), the palette then the concatenated IDAT payload
PngStream = namedtuple("PngStream", "data w h colour_type channels plte_count z_bytes")

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: build it with `python -m lemon_amd.build`")
        lib = ctypes.CDLL(SO_PATH)
        vp, c_i64, c_i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
        lib.lemon_png_info.argtypes = [ctypes.c_char_p, c_i64, ctypes.POINTER(Info)]
        lib.lemon_png_idat.argtypes = [ctypes.c_char_p, c_i64, vp, c_i64]
        lib.lemon_png_idat.restype = c_i64
        lib.lemon_png_decode_host.argtypes = [vp, c_i64, c_i32, c_i32, c_i32, c_i32, vp, ctypes.POINTER(c_i32)]
        lib.lemon_png_inflate_host.argtypes = [vp, c_i64, vp, c_i64, ctypes.POINTER(c_i32)]
        _lib = lib
    return _lib


def info(data):
    """Chunk walk over the bytes of a file -> Info (status 0: inside the envelope, record_bytes known)."""
    out = Info()
    load().lemon_png_info(data, len(data), ctypes.byref(out))
    return out


def idat(data, head=None):
    """The concatenated IDAT payload of an accepted file (a view of `data` when it is one chunk)."""
    head = head or info(data)
    assert head.status == OK
    if head.idat_spans == 1:
        return memoryview(data)[head.idat_offset:head.idat_offset + head.idat_bytes]
    buf = ctypes.create_string_buffer(max(int(head.idat_bytes), 1))
    n = load().lemon_png_idat(data, len(data), ctypes.cast(buf, ctypes.c_void_p), head.idat_bytes)
    assert n == head.idat_bytes, n
    return memoryview(buf)[:n]


def _fill_palette(data, head, palette):
    palette[:PALETTE_BYTES] = 0
    if head.plte_count:
        pal = np.frombuffer(data, np.uint8, 3 * head.plte_count, head.plte_offset).reshape(-1, 3)
        palette[:PALETTE_BYTES].reshape(256, 4)[:head.plte_count, :3] = pal


def stream_bytes_of(head):
    """Bytes of the PngStream of an accepted file: the palette and the IDAT payload."""
    return PALETTE_BYTES + int(head.idat_bytes)


def fill_stream(data, head, out):
    """The palette and the concatenated IDAT payload of an accepted file into `out` (writable contiguous uint8
    [stream_bytes_of(head)]).  No inflate: whether the payload is a zlib stream of the scanlines is the device's verdict."""
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable and out.size == stream_bytes_of(head)
    _fill_palette(data, head, out)
    if head.idat_spans == 1:
        out[PALETTE_BYTES:] = np.frombuffer(data, np.uint8, int(head.idat_bytes), int(head.idat_offset))
    elif head.idat_bytes:
        n = load().lemon_png_idat(data, len(data), out.ctypes.data + PALETTE_BYTES, head.idat_bytes)
        assert n == head.idat_bytes, n


def pack_stream(data, out=None):
    """bytes -> (PngStream, Info) or (None, Info) when the chunk walk declines the file (Info.status says why).  Chunk walk,
    CRCs and IDAT concatenation only.  `out`: a writable contiguous uint8 array of at least 1024 + idat_bytes to write into
    (default: a new one)."""
    head = info(data)
    if head.status != OK:
        return None, head
    n = stream_bytes_of(head)
    if out is None:
        out = np.empty(n, np.uint8)
    if out.size < n:
        head.status = BUFFER
        return None, head
    fill_stream(data, head, out[:n])
    return PngStream(out[:n], head.width, head.height, head.colour_type, head.channels, head.plte_count, n - PALETTE_BYTES), head


def record_bytes_of(s):
    """Bytes of the record a PngStream or PngRecord inflates to: 1024 + h * (w * channels + 1)."""
    return PALETTE_BYTES + s.h * (s.w * s.channels + 1)


def inflate_host(stream):
    """The device inflate's schedule on the host (csrc/png_inflate_core.hpp): PngStream -> (PngRecord, 0) or (None, STREAM).
    For tests."""
    rec = np.empty(record_bytes_of(stream), np.uint8)
    src = np.ascontiguousarray(stream.data)
    rec[:PALETTE_BYTES] = src[:PALETTE_BYTES]
    st = ctypes.c_int32(-1)
    rc = load().lemon_png_inflate_host(src.ctypes.data + PALETTE_BYTES, stream.z_bytes, rec.ctypes.data + PALETTE_BYTES,
                                       rec.size - PALETTE_BYTES, ctypes.byref(st))
    if rc != 0:
        raise ValueError("lemon_png_inflate_host: bad arguments")
    if st.value != OK:
        return None, st.value
    return PngRecord(rec, stream.w, stream.h, stream.colour_type, stream.channels, stream.plte_count), OK


def fill_record(data, head, record):
    """Inflate the file's scanlines into `record` (writable contiguous uint8 [head.record_bytes]) behind its palette.  -> a
    status: OK, or STREAM unless the zlib stream yields exactly h * (stride + 1) bytes, ends there with no unused data and
    raises no error."""
    assert record.dtype == np.uint8 and record.flags.c_contiguous and record.flags.writeable and record.size == head.record_bytes
    want = head.record_bytes - PALETTE_BYTES
    z = zlib.decompressobj()
    try:
        rows = z.decompress(idat(data, head), want + 1)
    except zlib.error:
        return STREAM
    if len(rows) != want or not z.eof or z.unused_data or z.unconsumed_tail:
        return STREAM
    _fill_palette(data, head, record)
    record[PALETTE_BYTES:] = np.frombuffer(rows, np.uint8)
    return OK


def decode_record(data, out=None):
    """bytes -> (PngRecord, Info) or (None, Info) when the file is declined (Info.status says why; STREAM from the inflate
    step).  `out`: a writable contiguous uint8 array of at least record_bytes to write into (default: a new one)."""
    head = info(data)
    if head.status != OK:
        return None, head
    n = int(head.record_bytes)
    if out is None:
        out = np.empty(n, np.uint8)
    if out.size < n:
        head.status = BUFFER
        return None, head
    head.status = fill_record(data, head, out[:n])
    if head.status != OK:
        return None, head
    return PngRecord(out[:n], head.width, head.height, head.colour_type, head.channels, head.plte_count), head


def decode_host(rec):
    """The device's schedule and arithmetic on the host (csrc/png_core.hpp): PngRecord -> (uint8 [h, w, 3], status).  For tests."""
    out = np.empty((rec.h, rec.w, 3), np.uint8)
    data = np.ascontiguousarray(rec.data)
    st = ctypes.c_int32(-1)
    rc = load().lemon_png_decode_host(data.ctypes.data, data.size, rec.h, rec.w, rec.colour_type, rec.plte_count, out.ctypes.data,
                                      ctypes.byref(st))
    if rc != 0:
        raise ValueError("lemon_png_decode_host: bad record geometry")
    return out, st.value


def work_bytes_of(w):
    """An image's share of lemon_png_decode's work buffer (include/lemon_hip.h): one uint32 per pixel of a row, rounded to 16."""
    return (4 * w + 15) // 16 * 16
