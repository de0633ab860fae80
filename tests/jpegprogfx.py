"""Progressive JPEG files written by PIL at test time for tests/test_jpeg_progressive.py and tests/test_gpu_jpeg_progressive.py:
the accepted set (every case must decode bit for bit like PIL, none may be declined) and the files and packets that must be
declined."""
import struct

import numpy as np

from tests import jpegfx


def accepted_cases(seed=3):
    """[(name, bytes)], all progressive: 8 shapes x subsampling 0/1/2 x quality 30/90 = 48, then 17x24 at 4:2:0, noise at
    quality 95, grayscale, restart markers by blocks (3 and 1) and by rows (the DRI value then changes from scan to scan), a flat
    image (one EOB run over a whole scan), a flat grayscale image of more than 32767 blocks (the run splits), 640x480, and 4 KB
    of EXIF / COM segments."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    jb = lambda px, **kw: jpegfx.jpeg_bytes(px, progressive=True, **kw)
    out = []
    for w, h in jpegfx.SHAPES:
        for ss in (0, 1, 2):
            for q in (30, 90):
                out.append((f"{w}x{h}_ss{ss}_q{q}", jb(jpegfx.pixels(w, h, rng), quality=q, subsampling=ss)))
    assert len(out) == 48
    out.append(("17x24_ss2", jb(jpegfx.pixels(17, 24, rng), quality=75, subsampling=2)))
    out.append(("noise_q95", jb(jpegfx.pixels(64, 80, rng, noise=True), quality=95, subsampling=0)))
    out.append(("gray_41x67", jb(jpegfx.pixels(41, 67, rng, channels=1), quality=90)))
    out.append(("gray_1x1", jb(jpegfx.pixels(1, 1, rng, noise=True, channels=1).reshape(1, 1), quality=75)))
    out.append(("restart_blocks3", jb(jpegfx.pixels(100, 75, rng), quality=90, subsampling=2, restart_marker_blocks=3)))
    out.append(("restart_blocks1", jb(jpegfx.pixels(100, 75, rng), quality=50, subsampling=0, restart_marker_blocks=1)))
    out.append(("restart_rows1", jb(jpegfx.pixels(100, 75, rng), quality=90, subsampling=1, restart_marker_rows=1)))
    out.append(("flat_64x80", jb(np.full((80, 64, 3), 93, np.uint8), quality=90, subsampling=2)))
    out.append(("flat_gray_1456", jb(np.full((1456, 1456), 200, np.uint8), quality=90)))
    out.append(("640x480", jb(jpegfx.pixels(640, 480, rng), quality=90, subsampling=2)))
    exif = Image.Exif()
    exif[0x010E] = "x" * 2000
    out.append(("exif_com", jb(jpegfx.pixels(64, 80, rng), quality=90, subsampling=2, exif=exif, comment=b"c" * 2100)))
    return out


def sos_offsets(raw):
    """Offsets of the SOS markers of a file PIL wrote (walks the segments; entropy-coded bytes hold no FF xx but FF 00 / RSTn)."""
    out, p = [], 2
    while p + 4 <= len(raw):
        assert raw[p] == 0xFF, p
        m = raw[p + 1]
        if m == 0xD9:
            break
        n = (raw[p + 2] << 8) | raw[p + 3]
        if m == 0xDA:
            out.append(p)
            p += 2 + n
            while not (raw[p] == 0xFF and raw[p + 1] != 0 and not 0xD0 <= raw[p + 1] <= 0xD7):
                p += 1
        else:
            p += 2 + n
    return out


def cut_after_scans(raw, k):
    """The file's first k scans, closed with EOI (the tables in front of scan k + 1 dropped with it)."""
    sos = sos_offsets(raw)
    end = sos[k]
    # back over the DHT / DRI segments that belong to the next scan
    p, last = 2, 2
    while p < end:
        n = (raw[p + 2] << 8) | raw[p + 3]
        if raw[p + 1] == 0xDA:
            q = p + 2 + n
            while not (raw[q] == 0xFF and raw[q + 1] != 0 and not 0xD0 <= raw[q + 1] <= 0xD7):
                q += 1
            p = last = q
        else:
            p += 2 + n
    return raw[:last] + b"\xff\xd9"


def patched_sos(raw, scan, **kw):
    """The file with fields of SOS number `scan` replaced: ss, se, ah, al, or ns3 (the component count byte set to 3)."""
    at = sos_offsets(raw)[scan]
    m = bytearray(raw)
    ns = m[at + 4]
    tail = at + 5 + 2 * ns
    if "ss" in kw:
        m[tail] = kw["ss"]
    if "se" in kw:
        m[tail + 1] = kw["se"]
    if "ah" in kw:
        m[tail + 2] = (kw["ah"] << 4) | (m[tail + 2] & 15)
    if "al" in kw:
        m[tail + 2] = (m[tail + 2] & 0xF0) | kw["al"]
    if kw.get("ns3"):                     # a 3-component AC scan: the header grows by two component entries
        body = bytes([3, 1, m[at + 6], 2, 0x11, 3, 0x11]) + bytes(m[tail:tail + 3])
        m[at + 2:tail + 3] = struct.pack(">H", len(body) + 2) + body
    return bytes(m)


def declined_cases(seed=4):
    """[(name, bytes, status or None)]: files the progressive pass must decline, with the status where the issue names one."""
    rng = np.random.default_rng(seed)
    px = jpegfx.pixels(64, 80, rng)
    base = jpegfx.jpeg_bytes(px, quality=90, subsampling=2, progressive=True)
    out = [("baseline", jpegfx.jpeg_bytes(px, quality=90, subsampling=2), 3)]
    for k in range(1, 10):
        out.append((f"cut_after_{k}", cut_after_scans(base, k), 17))
    out.append(("truncated_60", base[:len(base) * 6 // 10], None))
    flipped = bytearray(base)
    flipped[base.index(b"\xff\xc4") + 5] ^= 0xFF
    out.append(("huffman_flip", bytes(flipped), None))
    out.append(("ah", patched_sos(base, 1, ah=1), None))
    out.append(("al", patched_sos(base, 1, al=14), None))
    out.append(("al_refine", patched_sos(base, 5, al=0), None))
    out.append(("se_lt_ss", patched_sos(base, 1, ss=6, se=5), None))
    out.append(("se_64", patched_sos(base, 2, se=64), None))
    out.append(("dc_se", patched_sos(base, 0, se=5), None))
    out.append(("ac_3comp", patched_sos(base, 1, ns3=True), None))
    sof10 = bytearray(base)
    sof10[base.index(b"\xff\xc2") + 1] = 0xCA
    out.append(("sof10", bytes(sof10), None))
    return out


def byte_mutants(n=2001, seed=20261017):
    """[(name, bytes)]: seeded single-byte mutants of three small progressive files (anywhere in the file)."""
    rng = np.random.default_rng(seed)
    bases = [jpegfx.jpeg_bytes(jpegfx.pixels(24, 16, rng), quality=85, subsampling=2, progressive=True),
             jpegfx.jpeg_bytes(jpegfx.pixels(19, 21, rng, channels=1), quality=60, progressive=True),
             jpegfx.jpeg_bytes(jpegfx.pixels(32, 24, rng), quality=95, subsampling=0, progressive=True, restart_marker_blocks=2)]
    out = []
    for k in range(n):
        m = bytearray(bases[k % 3])
        at = int(rng.integers(2, len(m)))
        m[at] = (m[at] + int(rng.integers(1, 256))) & 255 if k % 2 else m[at] ^ (1 << int(rng.integers(0, 8)))
        out.append((f"m{k}_at{at}", bytes(m)))
    return out


def _scan_row(pk, s):
    return pk[512 + 64 * s:512 + 64 * s + 64].view(np.int32)


def corrupt_packets(raw):
    """[(name, packet bytes)]: the packet of `raw` (a colour file PIL wrote progressive, without restart markers) with one scan
    corrupted in the ways a broken file reaches the device: a code that is in no table, data that ends early, bytes left over, an
    EOB run past the last block, a refinement symbol of size 2.  (Rows of the scan table: csrc/jpeg_prog_par.hpp.)"""
    from lemon_amd import jpeg_host
    pk, head = jpeg_host.prog_pack(raw)
    assert pk is not None, head.status
    base = pk.data.copy()
    hd = base[:128].view(np.int32)
    pool_off, data_off = int(hd[10]), int(hd[11])
    out = []

    def spec_of(p, idx):
        at = int(p[pool_off:pool_off + 4 * int(hd[7])].view(np.uint32)[idx])
        return at, int(p[at:at + 16].sum())

    # a refinement scan (Ah != 0, Ss > 0): its table gets the values 0x02 (size 2) / 0xE0 (an EOB run of 2^14 blocks) everywhere
    ref = next(s for s in range(int(hd[6])) if _scan_row(base, s)[3] != 0 and _scan_row(base, s)[1] > 0)
    for name, val in (("refine_size_2", 0x02), ("eob_run_past_end", 0xE0)):
        p = base.copy()
        at, total = spec_of(p, int(_scan_row(p, ref)[11]))
        p[at + 16:at + 16 + total] = val
        out.append((name, p))
    # the first AC scan: an incomplete code (one code of length 1), so a 1 bit is no code
    first = next(s for s in range(int(hd[6])) if _scan_row(base, s)[3] == 0 and _scan_row(base, s)[1] > 0)
    p = base.copy()
    at, total = spec_of(p, int(_scan_row(p, first)[11]))
    p[at:at + 16] = 0
    p[at] = 1
    out.append(("bad_code", p))
    # data that ends early / bytes left over: the scan's byte count shrinks or grows into its neighbour's bytes
    for name, delta in (("early_end", -3), ("left_over", 2)):
        p = base.copy()
        row = _scan_row(p, first)
        assert row[9] > 8 and row[8] + row[9] + 2 <= hd[12]
        row[9] += delta
        out.append((name, p))
    return out
