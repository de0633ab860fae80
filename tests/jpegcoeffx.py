"""Baseline JPEG files written coefficient by coefficient, for tests/test_jpeg_coef_host.py and tests/test_gpu_jpeg_coef.py.

write() takes quantised DCT coefficients over the MCU-padded block grids and returns the file together with everything a test
needs to assert a placement rather than hope for it: the coefficient record the decoders must produce (the layout of
lemon_amd/csrc/jpeg_entropy.hpp), the destuffed size of every restart interval and the start bit of every block and symbol.
An encoder that starts from pixels cannot reach most of what the decoders accept (hundreds of restart intervals, intervals of
64 KB, table ids other than 0 / 1, arbitrary MCU padding, blocks at the edge of the arithmetic envelope, 16-bit codes); the case
builders below aim one named list at each of those.  Every random choice is seeded; every list is built once per process."""
import functools
import io
import struct
import warnings
from collections import namedtuple

import numpy as np
from PIL import Image

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])         # natural index of zig-zag position k
GRAY, S444, S422, S420 = (1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)          # (components, hs, vs)
SAMPLINGS = (GRAY, S444, S422, S420)

# ------------------------------------------------------------------------------------------------------------ Huffman tables
HuffTable = namedtuple("HuffTable", "counts vals codes")         # 16 counts, the values, {value: (code, length)}


def huff_table(counts, vals):
    """A table from 16 counts and the values in code order.  The counts must describe a prefix code that leaves the all-ones
    code of 16 bits unused (T.81 C.2): sum counts[l] 2^(16 - l) <= 65535."""
    counts, vals = [int(c) for c in counts], [int(v) for v in vals]
    assert len(counts) == 16 and sum(counts) == len(vals) <= 256 and len(set(vals)) == len(vals) and all(0 <= c < 256 for c in counts)
    assert sum(c << (15 - i) for i, c in enumerate(counts)) <= 65535, "Kraft sum: no prefix code, or the all-ones code is used"
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return HuffTable(bytes(counts), bytes(vals), codes)


DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]          # EOB, ZRL, 160 (run, size)

# the tables of T.81 Annex K.3, as data
_K_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_K_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
K_DC_LUMA = huff_table([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], DC_SYMBOLS)
K_DC_CHROMA = huff_table([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], DC_SYMBOLS)
K_AC_LUMA = huff_table([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], _K_AC_LUMA)
K_AC_CHROMA = huff_table([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _K_AC_CHROMA)


def counts_of(lengths):
    """{code length: number of codes} -> the 16 counts."""
    return [lengths.get(length, 0) for length in range(1, 17)]


# every symbol an 8-bit code: symbols without magnitude bits are whole bytes, so a block's size is known in bytes
B_DC = huff_table(counts_of({8: 12}), DC_SYMBOLS)
B_AC = huff_table(counts_of({8: 162}), AC_SYMBOLS)


def long_table(symbols, last, short=8):
    """The symbols of `last` get 16-bit codes, all others `short`-bit ones."""
    first = [s for s in symbols if s not in last]
    return huff_table(counts_of({short: len(first), 16: len(last)}), first + list(last))


L_DC = long_table(DC_SYMBOLS, [11])                   # category 11: a 16-bit code and 11 bits
L_AC = long_table(AC_SYMBOLS, [0x0A, 0xEA])           # run 0 / run 14 with size 10: a 16-bit code and 10 bits

# --------------------------------------------------------------------------------------------------------------- the writer
CoefJpeg = namedtuple("CoefJpeg", "raw record w h components hs vs scan_bytes interval_bytes block_start symbol_start block_symbol")
# raw             the file
# record          uint8: uint16 quant[3][64], then int16 blocks, planar, natural order (csrc/jpeg_entropy.hpp)
# scan_bytes      destuffed bytes of the scan; interval_bytes: of every restart interval
# block_start     per interval: the start bit, within the interval, of each of its blocks in scan order
# symbol_start    per interval: the start bit of every symbol (a code with its magnitude bits)
# block_symbol    per interval: index into symbol_start of each block's DC symbol


def grids(w, h, sampling):
    """Block grids [(rows, cols)] of the components over the MCU-padded image, and the MCU grid (my, mx)."""
    nc, hs, vs = sampling
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    return [(my * vs, mx * hs)] + [(my, mx)] * (nc - 1), (my, mx)


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def _pack_bits(vals, lens):
    """Symbols (value, bit count), MSB first -> (bytes padded with one bits, the start bit of every symbol)."""
    vals, lens = np.asarray(vals, np.uint64), np.asarray(lens, np.int64)
    ends = np.cumsum(lens)
    starts = ends - lens
    total = int(ends[-1])
    which = np.repeat(np.arange(len(lens)), lens)
    shift = (lens[which] - 1 - (np.arange(total) - starts[which])).astype(np.uint64)
    bits = ((vals[which] >> shift) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-total % 8, np.uint8)])
    return np.packbits(bits).tobytes(), starts


def write(w, h, sampling, coefs, quants, tq=(0, 1, 1), restart=0, td=(0, 1, 1), ta=(0, 1, 1), dc_tables=None, ac_tables=None,
          fill=0, merged=False):
    """coefs: per component an integer array [block rows, block cols, 64] of quantised coefficients in natural order (DC as
    its value, not its difference) over the grids of grids().  quants: {table id: 64 values in natural order, 1..255};
    dc_tables / ac_tables: {table id: HuffTable} (default: Annex K under ids 0 and 1).  tq / td / ta: the components' table
    ids.  A Huffman table id above 1 makes the frame SOF1 (extended sequential), as T.81 requires.
    Without effect on the decoded image: `fill` bytes FF in front of every RSTn and EOI; merged: one DQT and one DHT segment
    holding all tables rather than a segment each."""
    nc, hs, vs = sampling
    shapes, (my, mx) = grids(w, h, sampling)
    dc_tables = dc_tables or {0: K_DC_LUMA, 1: K_DC_CHROMA}
    ac_tables = ac_tables or {0: K_AC_LUMA, 1: K_AC_CHROMA}
    coefs = [np.asarray(c, np.int64) for c in coefs]
    assert len(coefs) == nc and all(c.shape == s + (64,) for c, s in zip(coefs, shapes)), ([c.shape for c in coefs], shapes)
    assert 0 <= restart <= 65535 and all(0 <= t <= 3 for t in tuple(tq) + tuple(td) + tuple(ta))
    # ---- entropy coding
    zz = [c[..., ZIGZAG] for c in coefs]
    has_ac = [(z[..., 1:] != 0).any(-1) for z in zz]
    slots = [(0, by, bx) for by in range(vs if nc == 3 else 1) for bx in range(hs if nc == 3 else 1)] + [(c, 0, 0) for c in range(1, nc)]
    mcus = mx * my
    per = restart or mcus
    intervals, block_start, symbol_start, block_symbol = [], [], [], []
    for m0 in range(0, mcus, per):
        vals, lens, first = [], [], []
        pred = [0, 0, 0]
        for m in range(m0, min(m0 + per, mcus)):
            yy, xx = divmod(m, mx)
            for c, by, bx in slots:
                r, q = (yy * vs + by, xx * hs + bx) if c == 0 and nc == 3 else (yy, xx)
                z = zz[c][r, q]
                dcc, acc = dc_tables[td[c]].codes, ac_tables[ta[c]].codes
                first.append(len(vals))
                diff = int(z[0]) - pred[c]
                pred[c] = int(z[0])
                s = abs(diff).bit_length()
                assert s <= 11, ("DC difference beyond category 11", diff)
                code, length = dcc[s]
                vals.append((code << s) | (diff if diff >= 0 else diff + (1 << s) - 1))
                lens.append(length + s)
                k = 1
                if has_ac[c][r, q]:
                    for pos in np.flatnonzero(z[1:]) + 1:
                        run, v = int(pos) - k, int(z[pos])
                        while run >= 16:
                            vals.append(acc[0xF0][0]); lens.append(acc[0xF0][1])
                            run -= 16
                        s = abs(v).bit_length()
                        assert s <= 10, ("AC coefficient beyond size 10", v)
                        code, length = acc[(run << 4) | s]
                        vals.append((code << s) | (v if v >= 0 else v + (1 << s) - 1))
                        lens.append(length + s)
                        k = int(pos) + 1
                if k <= 63:
                    vals.append(acc[0][0]); lens.append(acc[0][1])
        data, starts = _pack_bits(vals, lens)
        intervals.append(data)
        symbol_start.append(starts)
        block_symbol.append(np.array(first))
        block_start.append(starts[np.array(first)])
    # ---- the file
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")]
    qbody = [bytes([t]) + bytes(int(v) for v in np.asarray(quants[t])[ZIGZAG]) for t in sorted(quants)]
    assert all(1 <= v <= 255 for t in quants for v in np.asarray(quants[t]).ravel()) and all(len(b) == 65 for b in qbody)
    hbody = [bytes([t]) + dc_tables[t].counts + dc_tables[t].vals for t in sorted(dc_tables)]
    hbody += [bytes([0x10 | t]) + ac_tables[t].counts + ac_tables[t].vals for t in sorted(ac_tables)]
    out += [_segment(0xDB, b"".join(qbody))] if merged else [_segment(0xDB, b) for b in qbody]
    sof = 0xC1 if max(max(dc_tables), max(ac_tables)) > 1 else 0xC0
    out.append(_segment(sof, bytes([8]) + struct.pack(">HH", h, w) + bytes([nc]) +
                        b"".join(bytes([c + 1, ((hs << 4) | vs) if c == 0 and nc == 3 else 0x11, tq[c]]) for c in range(nc))))
    out += [_segment(0xC4, b"".join(hbody))] if merged else [_segment(0xC4, b) for b in hbody]
    if restart:
        out.append(_segment(0xDD, struct.pack(">H", restart)))
    out.append(_segment(0xDA, bytes([nc]) + b"".join(bytes([c + 1, (td[c] << 4) | ta[c]]) for c in range(nc)) + bytes([0, 63, 0])))
    for t, data in enumerate(intervals):
        out.append(data.replace(b"\xff", b"\xff\x00"))
        out.append(b"\xff" * fill + (bytes([0xFF, 0xD0 + (t & 7)]) if t + 1 < len(intervals) else b"\xff\xd9"))
    quant = np.zeros((3, 64), np.uint16)
    for c in range(nc):
        quant[c] = np.asarray(quants[tq[c]])
    record = np.concatenate([quant.ravel().view(np.uint8), np.concatenate([c.ravel() for c in coefs]).astype(np.int16).view(np.uint8)])
    sizes = [len(d) for d in intervals]
    return CoefJpeg(b"".join(out), record, w, h, nc, hs if nc == 3 else 1, vs if nc == 3 else 1, sum(sizes), sizes, block_start,
                    symbol_start, block_symbol)


def pil_rgb(raw):
    """What PIL decodes, with every warning of its an error (a file libjpeg finds fault with is no fixture)."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------- contents
def flat(q):
    return np.full(64, q, np.int64)


def sparse_blocks(rng, shape, dc=60, ac=40, density=0.08, reach=64):
    """Blocks [rows, cols, 64] with DC values in [-dc, dc] and a share `density` of the first `reach` natural positions in
    [-ac, ac]: far inside the envelope for quantisers of a few units, and different in every block, the MCU padding included."""
    b = np.zeros(shape + (64,), np.int64)
    b[..., 0] = rng.integers(-dc, dc + 1, shape)
    on = rng.random(shape + (reach - 1,)) < density
    b[..., 1:reach] = np.where(on, rng.integers(-ac, ac + 1, shape + (reach - 1,)), 0)
    return b


def sparse_image(rng, w, h, sampling, **kw):
    return [sparse_blocks(rng, s, **kw) for s in grids(w, h, sampling)[0]]


def sized_blocks(sizes, restart=0):
    """Gray blocks [1, n, 64] that the all-8-bit tables (B_DC, B_AC) code in exactly sizes[i] bytes, each 2..5: a DC difference of
    0 (one byte) or of 200 in magnitude (two), no coefficient or one of 200 at position 1 (two bytes), end of block (one).
    restart: the restart interval the file is written with (the prediction starts over there)."""
    b = np.zeros((1, len(sizes), 64), np.int64)
    dc = 0
    for i, s in enumerate(sizes):
        assert 2 <= s <= 5, s
        if restart and i % restart == 0:
            dc = 0
        if s in (3, 5):
            dc = 200 - dc
        b[0, i, 0] = dc
        if s >= 4:
            b[0, i, 1] = 200 if i % 2 else -200
    return b


def sizes_to(rng, total, n=None):
    """Block sizes of 2..5 bytes that sum to `total`: n of them, or as many as a seeded draw gives."""
    if n is None:
        sizes = []
        while total - sum(sizes) > 5:
            sizes.append(int(rng.integers(2, 6)))
            if 0 < total - sum(sizes) < 2:
                sizes[-1] -= 1
        return sizes + [total - sum(sizes)]
    assert 2 * n <= total <= 5 * n, (total, n)
    sizes = [2] * n
    for k in rng.permutation(3 * n)[:total - 2 * n]:
        sizes[k % n] += 1
    return sizes


# ------------------------------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "name jpeg one_byte note", defaults=(False, None))
# one_byte: a long run of whole-byte symbols in one interval, where a lane that starts in the wrong state can stay wrong across
#           more workgroups than the rounds of the parallel pass carry the truth (LEMON_JPEG_SYNC at small lanes is legitimate)
Q1 = {0: flat(1)}
BYTES_T = dict(dc_tables={0: B_DC}, ac_tables={0: B_AC})
LONG_T = dict(dc_tables={0: L_DC}, ac_tables={0: L_AC})
ONE = dict(tq=(0, 0, 0), td=(0, 0, 0), ta=(0, 0, 0))          # every component on table 0


@functools.lru_cache(None)
def intervals_cases(seed=11):
    """More than 256 restart intervals: the chunk loops of the plan and of both segmented scans, and the upper half of the
    interval search."""
    rng = np.random.default_rng(seed)
    q = {0: flat(2), 1: flat(3)}
    out = []
    for n in (255, 256, 257, 513):
        out.append(Case(f"gray_{n}x1_r1", write(8 * n, 8, GRAY, sparse_image(rng, 8 * n, 8, GRAY), q, restart=1)))
    out.append(Case("420_257x1_r1", write(16 * 257, 16, S420, sparse_image(rng, 16 * 257, 16, S420), q, restart=1)))
    out.append(Case("420_150x2_r7", write(16 * 150, 32, S420, sparse_image(rng, 16 * 150, 32, S420), q, restart=7)))
    out.append(Case("422_130x3_r3", write(16 * 130, 24, S422, sparse_image(rng, 16 * 130, 24, S422), q, restart=3, fill=1)))
    return out


@functools.lru_cache(None)
def lanes_cases(seed=12):
    """One interval of sparse gray blocks, its size chosen to the byte: note = (scan bytes, lanes of 16 bytes)."""
    rng = np.random.default_rng(seed)
    out = []
    for total in (16 * 255 - 7, 16 * 256 - 15, 16 * 256 - 3, 16 * 256, 16 * 256 + 1, 16 * 257 - 5, 16 * 512 - 9, 16 * 512 + 1):
        sizes = sizes_to(rng, total)
        j = write(8 * len(sizes), 8, GRAY, [sized_blocks(sizes)], Q1, **BYTES_T)
        out.append(Case(f"lanes_{total}", j, note=(total, -(-total // 16))))
    return out


INTERVAL_SIZES = (15, 16, 17, 31, 32, 33)


@functools.lru_cache(None)
def interval_sizes_cases(seed=13):
    """Intervals of 7 blocks and of 15, 16, 17, 31, 32, 33 bytes: note = the sizes asked for.  `inside`: the 257th lane of 16
    bytes is the second of a 17-byte interval; `between`: one 15-byte interval in front moves it to an interval's start."""
    rng = np.random.default_rng(seed)
    out = []
    for name, want in (("inside", INTERVAL_SIZES * 40), ("between", (15,) + INTERVAL_SIZES * 40)):
        sizes = [s for t in want for s in sizes_to(rng, t, 7)]
        j = write(8 * len(sizes), 8, GRAY, [sized_blocks(sizes, 7)], Q1, restart=7, **BYTES_T)
        out.append(Case(name, j, note=list(want)))
    return out


BIG_W, BIG_H, BIG_RESTART = 5208, 1208, 32767          # 98301 = 3 * 32767 blocks


@functools.lru_cache(None)
def big_cases():
    """Three intervals of 32767 gray blocks: the first of 65534, 65535 or 65536 bytes, the second ordinary, the third of
    65537 -- entries of the packet's `big` table on both sides of its search.  note = the three sizes."""
    out = []
    for first in (65534, 65535, 65536):
        want = (first, 65534, 65537)
        sizes = []
        for t in want:
            extra = t - 2 * BIG_RESTART
            s = np.full(BIG_RESTART, 2)
            s[np.arange(extra) * 7919 % BIG_RESTART] += 1          # (7919 is prime to 32767: distinct blocks)
            sizes += list(s)
        b = sized_blocks(sizes, BIG_RESTART).reshape(BIG_H // 8, BIG_W // 8, 64)
        j = write(BIG_W, BIG_H, GRAY, [b], Q1, restart=BIG_RESTART, **BYTES_T)
        out.append(Case(f"big_{first}", j, one_byte=True, note=want))
    return out


def _fillers(target):
    """(a, b): a filler blocks of 17 bits (a DC difference of +-1 under L_DC) and b of 16 put the next block at bit `target`
    mod 128."""
    return next((a, b) for b in range(16) for a in range(16) if (17 * a + 16 * b) % 128 == target % 128)


@functools.lru_cache(None)
def symbols_cases(seed=14):
    """The longest symbols and the structural extremes of a block.  note = (kind, index of the block in its interval, bit
    of a 16-byte lane its long symbol must start on) for the placed ones."""
    rng = np.random.default_rng(seed)
    out = []
    for bit in (127, 120, 113):
        for kind in ("dc", "ac"):
            # dc: the category-11 symbol opens the block; ac: the block's 8-bit DC symbol comes first
            a, b = _fillers(bit if kind == "dc" else bit - 8)
            at = a + b
            diff = np.zeros(at + 3, np.int64)
            diff[:a] = np.where(np.arange(a) % 2 == 0, 1, -1)
            blocks = np.zeros((1, at + 3, 64), np.int64)
            if kind == "dc":
                diff[at], diff[at + 1] = 2047, -2047
            else:
                blocks[0, at, 1] = -1023
                blocks[0, at + 1, 63] = 1023                    # three ZRL, then run 14 / size 10 under a 16-bit code
            blocks[0, at + 2] = sparse_blocks(rng, (), dc=0, ac=100, density=0.2)
            blocks[0, :, 0] = np.cumsum(diff)
            j = write(8 * blocks.shape[1], 8, GRAY, [blocks], Q1, **LONG_T)
            out.append(Case(f"{kind}_at_bit_{bit}", j, note=(kind, at, bit)))
    # structural blocks under the Annex K tables and under the long ones, in every sampling
    for tname, tables in (("annex", {}), ("long", dict(LONG_T, **ONE))):
        for sampling in SAMPLINGS:
            w, h = 8 * 6 * sampling[1], 8 * 2 * sampling[2]
            comps = []
            for shape in grids(w, h, sampling)[0]:
                b = np.zeros(shape + (64,), np.int64).reshape(-1, 64)
                k = np.arange(len(b)) % 6
                b[k == 0, 63] = rng.choice([-1023, 1023, 1, -7], (k == 0).sum())                     # only zig-zag 63
                b[k == 1, 1:] = rng.choice([-2, -1, 1, 2], ((k == 1).sum(), 63))                     # all 63, no EOB
                b[k == 2, 0] = rng.integers(-500, 500, (k == 2).sum())                               # DC only
                b[k == 3, rng.integers(1, 64)] = np.where(np.arange((k == 3).sum()) % 2, 1023, -1023)      # +-1023 AC
                b[k == 4, 0] = 1023
                b[k == 5, 0] = -1024                                                                 # a DC step of -2047
                comps.append(b.reshape(shape + (64,)))
            q = {0: flat(1), 1: flat(1)} if not tables else Q1
            out.append(Case(f"structure_{tname}_{sampling[0]}{sampling[1]}{sampling[2]}", write(w, h, sampling, comps, q, **tables)))
    # an interval whose last data byte is FF, so that FF 00 stands straight in front of the marker; with fill bytes too
    blocks = np.zeros((1, 12, 64), np.int64)
    blocks[0, :, 9] = 255                                       # (3, 8) and eight one bits, then EOB ...
    blocks[0, 2::3, 63] = 255                                   # ... or no EOB: the interval ends in FF
    for fill in (0, 1, 3):
        j = write(96, 8, GRAY, [blocks], Q1, restart=3, fill=fill, merged=fill == 1, **BYTES_T)
        out.append(Case(f"ends_in_ff_fill{fill}", j, note=("ff",)))
    return out


SELECTORS = ((1, 0, 1), (0, 2, 3), (3, 3, 0))


@functools.lru_cache(None)
def selectors_cases(seed=15):
    """Quantisers under ids (2, 0, 3) and others, Huffman selectors no encoder from pixels picks, different contents under every
    id, and geometries whose planes begin inside a 32-block inverse-DCT workgroup or make 31, 32, 33 blocks in all."""
    rng = np.random.default_rng(seed)
    dct = {0: K_DC_LUMA, 1: K_DC_CHROMA, 2: B_DC, 3: L_DC}
    act = {0: K_AC_LUMA, 1: K_AC_CHROMA, 2: B_AC, 3: L_AC}
    qs = [rng.integers(1, 6, 64) for _ in range(4)]
    qs[1][0], qs[2][0], qs[3][0] = 2, 3, 5                      # (distinct in every position that matters most)
    geoms = [(40, 24, S420), (80, 48, S420), (8 * 31, 8, GRAY), (16 * 8, 8, S422), (88, 8, S444), (37, 21, S422), (23, 23, S444)]
    out = []
    for gi, (w, h, sampling) in enumerate(geoms):
        for si, td in enumerate(SELECTORS):
            tq = ((2, 0, 3), (3, 1, 0), (1, 3, 2))[(gi + si) % 3]
            ta = (td[1], td[2], td[0]) if (gi + si) % 2 else td
            ids = set(td + ta)
            sof1 = max(ids) > 1
            have = range(4) if sof1 else range(2)
            j = write(w, h, sampling, sparse_image(rng, w, h, sampling, dc=80, ac=25, density=0.1), {t: qs[t] for t in sorted(set(tq))},
                      tq=tq, td=td, ta=ta, dc_tables={t: dct[t] for t in have}, ac_tables={t: act[t] for t in have}, merged=bool(si % 2))
            digits = lambda v: "".join(map(str, v))
            out.append(Case(f"sel_{w}x{h}_{digits(sampling)}_q{digits(tq)}_d{digits(td)}_a{digits(ta)}", j))
    return out


PAD_SIDES = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)


def outside_blocks(w, h, sampling):
    """Luma blocks (row, col) that lie wholly outside a w x h image (chroma blocks never do: one spans its whole MCU)."""
    rows, cols = grids(w, h, sampling)[0][0]
    return [(r, c) for r in range(rows) for c in range(cols) if 8 * r >= h or 8 * c >= w]


@functools.lru_cache(None)
def padding_cases(seed=16):
    """Every width and height of PAD_SIDES under every sampling, random content in every block, the padding included; where
    luma blocks lie wholly outside the image a second file (`..._twin`) differs in exactly those blocks."""
    rng = np.random.default_rng(seed)
    q = {0: flat(2), 1: flat(3)}
    out = []
    for sampling in SAMPLINGS:
        for h in PAD_SIDES:
            for w in PAD_SIDES:
                comps = sparse_image(rng, w, h, sampling, dc=220, ac=70, density=0.12, reach=30)
                name = f"pad_{w}x{h}_{''.join(map(str, sampling))}"
                out.append(Case(name, write(w, h, sampling, comps, q)))
                outside = outside_blocks(w, h, sampling)
                if outside:
                    other = [c.copy() for c in comps]
                    for r, c in outside:
                        other[0][r, c] = sparse_blocks(rng, (), dc=220, ac=70, density=0.3, reach=30)
                        other[0][r, c, 0] += 7 if other[0][r, c, 0] == comps[0][r, c, 0] else 0
                    out.append(Case(name + "_twin", write(w, h, sampling, other, q)))
    return out


N_ENVELOPE_RANDOM = 400


def _single(pos, v, q=4):
    b = np.zeros((1, 1, 64), np.int64)
    b[0, 0, pos] = v
    return write(8, 8, GRAY, [b], {0: flat(q)})


@functools.lru_cache(None)
def envelope_cases(seed=17):
    """400 random files around the arithmetic envelope (sizes 1..39, every sampling, flat quantisers 1..39, amplitudes and
    densities drawn per file), then 128 one-block files with a single coefficient: every position and sign at the largest
    magnitude the host verdict accepts (bisection on decode_record's status; note = (position, value))."""
    from lemon_amd import jpeg_host
    rng = np.random.default_rng(seed)
    out = []
    for k in range(N_ENVELOPE_RANDOM):
        w, h = (int(v) for v in rng.integers(1, 40, 2))
        sampling = SAMPLINGS[int(rng.integers(0, 4))]
        qv = [int(v) for v in rng.integers(1, 40, 2)]
        budget = float(rng.choice([1500, 3000, 4500, 6000, 9000]))          # about D + 2 A of the largest blocks, dequantised
        density = float(rng.choice([0.03, 0.1, 0.3, 1.0]))
        comps = []
        for c, shape in enumerate(grids(w, h, sampling)[0]):
            qc = qv[min(c, 1)]
            n_ac = max(1.0, 63 * density)
            dc = int(min(1023, budget / 2 / qc))
            ac = int(min(1023, max(1, budget / 4 / n_ac / qc * 2)))
            comps.append(sparse_blocks(rng, shape, dc=dc, ac=ac, density=density))
        j = write(w, h, sampling, comps, {0: flat(qv[0]), 1: flat(qv[1])})
        out.append(Case(f"env_{k}_{w}x{h}_{''.join(map(str, sampling))}_q{qv[0]}_{qv[1]}", j))
    for pos in range(64):
        for sign in (1, -1):
            lo, hi = 0, 2047 if pos == 0 else 1023           # accepted at lo, declined at hi
            assert jpeg_host.decode_record(_single(pos, sign * hi).raw)[1].status == 12
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if jpeg_host.decode_record(_single(pos, sign * mid).raw)[1].status == 0:
                    lo = mid
                else:
                    hi = mid
            out.append(Case(f"single_{pos}_{'+' if sign > 0 else '-'}{lo}", _single(pos, sign * lo), note=(pos, sign * lo)))
    return out


@functools.lru_cache(None)
def dc_range_cases():
    """DC differences of 2047 in magnitude whose sums leave int16 (quantiser 1).  Long before that the blocks are outside the
    envelope, so every path declines these files; the criterion is that all give the same status."""
    out = []
    for n, step in ((17, 2047), (40, -2047)):
        b = np.zeros((1, n, 64), np.int64)
        b[0, :, 0] = np.cumsum(np.full(n, step))
        j = write(8 * n, 8, GRAY, [np.clip(b, -32768, 32767)], Q1)
        out.append(Case(f"dc_{n}_steps_of_{step}", j._replace(record=None)))          # (no record: the sums do not fit one)
    return out


LISTS = {"intervals": intervals_cases, "lanes": lanes_cases, "interval_sizes": interval_sizes_cases, "big": big_cases,
         "symbols": symbols_cases, "selectors": selectors_cases, "padding": padding_cases, "envelope": envelope_cases,
         "dc_range": dc_range_cases}
