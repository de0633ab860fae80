"""A PNG writer the tests control (tests/test_png_host.py, tests/test_png_fuzz.py, tests/test_gpu_png.py): the filter type of
every row, the zlib level (0 = stored blocks), where the zlib stream is cut into IDAT chunks, optional PLTE / tRNS / other
chunks, and deliberate defects.  PIL's own encoder never emits the Average filter, so files that exercise all five filters
have to be written here; PIL reads them back as grey-replicate, RGB, alpha-drop and palette-lookup (checked by the tests)."""
import io
import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
COLOUR_TYPES = (0, 2, 3, 4, 6)
WIDTHS = (1, 2, 15, 16, 17, 63, 64, 65, 67)          # lane, 16-byte piece and staging-block edges
HEIGHTS = (1, 2, 63, 64, 65, 130)                    # band edges: one short band, one full, full + 1, two full + 2


def chunk(kind, body=b"", bad_crc=False):
    crc = zlib.crc32(kind + body) ^ (0x5A5A5A5A if bad_crc else 0)
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", crc & 0xFFFFFFFF)


def ihdr(w, h, colour_type, depth=8, interlace=0, compression=0, filter_method=0, bad_crc=False):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, compression, filter_method, interlace), bad_crc)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(pix, filters):
    """pix uint8 [h, w, channels], filters: one type per row -> the filtered scanlines (bytes), each behind its type byte.  A
    type above 4 is written as the byte it is, over unfiltered data."""
    h, w, bpp = pix.shape
    rows = pix.reshape(h, w * bpp).astype(np.int32)
    out = bytearray()
    zero = np.zeros(w * bpp, np.int32)
    for r in range(h):
        cur, up = rows[r], rows[r - 1] if r else zero
        left = np.concatenate([zero[:bpp], cur[:-bpp]]) if w * bpp > bpp else zero[:w * bpp]
        upleft = np.concatenate([zero[:bpp], up[:-bpp]]) if w * bpp > bpp else zero[:w * bpp]
        ft = int(filters[r])
        pred = {0: zero, 1: left, 2: up, 3: (left + up) >> 1, 4: _paeth(left, up, upleft)}.get(ft, zero)
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def split_stream(stream, splits):
    """Cut the zlib stream: `splits` None = one IDAT; an int n = chunks of n bytes; a list = cut positions."""
    if splits is None:
        return [stream]
    if isinstance(splits, int):
        return [stream[i:i + splits] for i in range(0, len(stream), splits)] or [b""]
    cuts = [0] + sorted(splits) + [len(stream)]
    return [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def png_bytes(pix, colour_type, filters=None, level=6, splits=None, plte=None, trns=None, before_idat=(), between_idat=None,
              after_idat=(), plte_after_idat=False, bad_crc=None, scan_tail=b"", scan_cut=0, stream_tail=b"", iend=True,
              header=None):
    """The file.  pix uint8 [h, w, CHANNELS[colour_type]] (palette indices for type 3; plte: uint8 [n, 3]).  filters: a type
    per row, an int for all rows, or None = the five types cycling.  before_idat / after_idat: extra (kind, body) chunks;
    between_idat: one (kind, body) chunk placed after the first IDAT (the stream is then cut in two if it is not already).
    Defects: plte_after_idat; bad_crc = b"IHDR" | b"IDAT" | b"IEND"; scan_tail: bytes appended to the scanlines before
    compression; scan_cut: scanline bytes dropped from the end; stream_tail: bytes after the zlib stream inside IDAT; iend=False;
    header: keyword overrides for ihdr() (depth, interlace, w, h, ...)."""
    pix = np.ascontiguousarray(pix, np.uint8)
    if pix.ndim == 2:
        pix = pix[:, :, None]
    h, w, c = pix.shape
    assert c == CHANNELS[colour_type], (c, colour_type)
    if filters is None:
        filters = [r % 5 for r in range(h)]
    elif isinstance(filters, int):
        filters = [filters] * h
    scan = filter_rows(pix, filters) + scan_tail
    if scan_cut:
        scan = scan[:-scan_cut]
    stream = zlib.compress(scan, level) + stream_tail
    hd = dict(w=w, h=h, colour_type=colour_type)
    hd.update(header or {})
    out = [SIGNATURE, ihdr(bad_crc=bad_crc == b"IHDR", **hd)]
    plte_chunk = chunk(b"PLTE", np.ascontiguousarray(plte, np.uint8).tobytes()) if plte is not None else b""
    if not plte_after_idat:
        out.append(plte_chunk)
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    out += [chunk(k, b) for k, b in before_idat]
    pieces = split_stream(stream, splits)
    if between_idat is not None and len(pieces) == 1:
        pieces = split_stream(stream, [len(stream) // 2])
    for i, p in enumerate(pieces):
        out.append(chunk(b"IDAT", p, bad_crc == b"IDAT" and i == 0))
        if i == 0 and between_idat is not None:
            out.append(chunk(*between_idat))
    if plte_after_idat:
        out.append(plte_chunk)
    out += [chunk(k, b) for k, b in after_idat]
    if iend:
        out.append(chunk(b"IEND", b"", bad_crc == b"IEND"))
    return b"".join(out)


def pixels(h, w, colour_type, rng, kind="random", plte_count=256):
    """Test pixels [h, w, channels]: "random" bytes, "ones" = all 255 (Paeth ties, the Average carry), "smooth" = a gradient with
    a little noise (what a photograph's filters see).  Type 3: indices below plte_count."""
    c = CHANNELS[colour_type]
    if kind == "ones":
        a = np.full((h, w, c), 255, np.uint8)
    elif kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        base = (yy * 3 + xx * 2)[:, :, None] + np.arange(c)[None, None, :] * 40
        a = ((base + rng.integers(0, 6, (h, w, c))) & 255).astype(np.uint8)
    else:
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if colour_type == 3:
        a = (a.astype(np.int32) % plte_count).astype(np.uint8)
    return a


def palette(n, rng):
    return rng.integers(0, 256, (n, 3), dtype=np.uint8)


def expected_rgb(pix, colour_type, plte=None):
    """What convert("RGB") gives for these pixels: grey replicated, alpha dropped, the palette looked up."""
    if colour_type in (0, 4):
        return np.repeat(pix[:, :, :1], 3, axis=2)
    if colour_type in (2, 6):
        return pix[:, :, :3].copy()
    return np.asarray(plte, np.uint8)[pix[:, :, 0]]


def pil_rgb(raw):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


def accepted_cases(seed=11):
    """[(name, bytes)]: every colour type x every single filter, the filters cycling and in random order, the edge widths and
    heights, all-255 and random bytes, stored blocks, 1-byte IDAT chunks, a split inside the zlib header, tRNS / gAMA chunks, and
    PIL-written files of the same kind of images.  Largest image 130 x 131."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, h, w, ct, filters=None, kind="random", **kw):
        n = int(rng.integers(1, 257)) if ct == 3 else None
        plte = palette(n, rng) if ct == 3 else None
        pix = pixels(h, w, ct, rng, kind, n or 256)
        cases.append((name, png_bytes(pix, ct, filters, plte=plte, **kw)))

    for ct in COLOUR_TYPES:
        for ft in range(5):
            add(f"ct{ct}_f{ft}", 9, 21, ct, ft)
        add(f"ct{ct}_cycle", 70, 37, ct)
        add(f"ct{ct}_shuffled", 67, 33, ct, list(rng.integers(0, 5, 67)))
        add(f"ct{ct}_ones", 66, 19, ct, None, "ones")
        add(f"ct{ct}_smooth", 130, 131, ct, list(rng.integers(0, 5, 130)), "smooth")
    for k, w in enumerate(WIDTHS):
        for j, h in enumerate(HEIGHTS):
            ct = COLOUR_TYPES[(k + j) % 5]
            add(f"w{w}_h{h}_ct{ct}", h, w, ct, list(rng.integers(0, 5, h)))
    add("stored", 20, 30, 2, level=0)
    add("idat_1byte", 12, 17, 6, splits=1)
    add("idat_split_header", 12, 17, 0, splits=[1, 2, 7])
    add("idat_empty_chunks", 12, 17, 4, splits=[0, 5, 5])
    add("trns_grey", 14, 15, 0, trns=b"\x00\x07")
    add("trns_palette", 14, 15, 3, trns=bytes(range(40)))
    add("ancillary", 14, 15, 2, before_idat=[(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"k\x00v")], after_idat=[(b"tIME", b"\x07\xe8\x01\x01\x00\x00\x00")])
    for mode, ct in (("L", 0), ("RGB", 2), ("LA", 4), ("RGBA", 6), ("P", 3)):
        for kind in ("smooth", "random"):
            if mode == "P":
                im = Image.fromarray(pixels(97, 61, 2, rng, kind)).quantize(200)
            else:
                im = Image.fromarray(pixels(97, 61, ct, rng, kind).squeeze(), mode)
            buf = io.BytesIO()
            im.save(buf, "PNG")
            cases.append((f"pil_{mode}_{kind}", buf.getvalue()))
    return cases


def declined_cases(seed=12):
    """[(name, bytes, expected LemonPngStatus)]: each defect is declined with its own status."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    g = pixels(10, 12, 0, rng)
    rgb = pixels(10, 12, 2, rng)
    idx = pixels(10, 12, 3, rng, plte_count=4)
    pal = palette(4, rng)
    good = png_bytes(rgb, 2)

    def pil(img, **kw):
        buf = io.BytesIO()
        img.save(buf, "PNG", **kw)
        return buf.getvalue()

    return [
        ("depth16", pil(Image.fromarray(rng.integers(0, 65536, (9, 7), dtype=np.uint16))), 5),
        ("depth1", pil(Image.fromarray(rng.integers(0, 2, (9, 7), dtype=np.uint8) * 255).convert("1")), 5),
        ("depth2", pil(Image.fromarray(pixels(9, 7, 2, rng)).quantize(4)), 5),
        ("depth4", pil(Image.fromarray(pixels(9, 7, 2, rng)).quantize(16)), 5),
        ("adam7", png_bytes(g, 0, header=dict(interlace=1)), 6),
        ("crc_ihdr", png_bytes(g, 0, bad_crc=b"IHDR"), 3),
        ("crc_idat", png_bytes(g, 0, bad_crc=b"IDAT"), 3),
        ("crc_iend", png_bytes(g, 0, bad_crc=b"IEND"), 3),
        ("plte_missing", png_bytes(idx, 3), 7),
        ("plte_after_idat", png_bytes(idx, 3, plte=pal, plte_after_idat=True), 8),
        ("plte_after_idat_rgb", png_bytes(rgb, 2, plte=pal, plte_after_idat=True), 8),
        ("idat_split_by_chunk", png_bytes(rgb, 2, between_idat=(b"tEXt", b"k\x00v")), 8),
        ("actl", png_bytes(rgb, 2, before_idat=[(b"acTL", struct.pack(">II", 1, 0))]), 9),
        ("stream_short", png_bytes(rgb, 2, scan_cut=1), 12),
        ("stream_long", png_bytes(rgb, 2, scan_tail=b"\x00"), 12),
        ("stream_garbage", png_bytes(rgb, 2, stream_tail=b"junk"), 12),
        ("truncated", good[:len(good) // 2], 2),
        ("no_iend", png_bytes(rgb, 2, iend=False), 2),
        ("zero_width", png_bytes(g, 0, header=dict(w=0)), 10),
        ("not_png", b"\xff\xd8\xff\xe0" + good[4:], 1),
    ]


def write_all(directory, cases, ext=".png"):
    paths = []
    for c in cases:
        p = os.path.join(directory, c[0] + ext)
        with open(p, "wb") as fh:
            fh.write(c[1])
        paths.append(p)
    return paths
