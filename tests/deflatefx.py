"""A bit-level zlib / DEFLATE writer the tests control (tests/test_png_inflate_host.py, tests/test_gpu_png_inflate.py), as
tests/jpegcoeffx.py is for JPEG coefficients: zlib's own encoder never emits most of what RFC 1951 allows and nothing of what
it forbids, so streams that reach every edge of the decoder (csrc/png_inflate_core.hpp) have to be written here, token by token.

A block is written from an explicit token list:
    b (int 0 .. 255)             a literal
    (length, distance)           a match, 3 <= length <= 258, 1 <= distance <= 32768
    EOB                          the end-of-block code (never added for you)
    ("sym", s)                   literal/length symbol s as it is, no extra bits (286, 287; or any)
    ("dsym", length, d, n, v)    a match whose distance is symbol d followed by n extra bits of value v (30, 31; or any)
with the block type, the code lengths, HLIT / HDIST / HCLEN, the code-length code and its symbol sequence, and the LEN / NLEN
and bit offset of a stored block under the caller's control.  zstream() wraps blocks in the RFC 1950 header and trailer, each
of which can be corrupted.  expand() is the reference output of a token list."""
import zlib

EOB = "eob"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """LSB-first bit packing (RFC 1951 3.1.1); Huffman codes go in most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0, (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        self.bits(int(format(code, f"0{length}b")[::-1], 2), length)

    def align(self, fill=0):
        if self.n:
            self.bits(fill & ((1 << (8 - self.n)) - 1), 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    @property
    def bit_offset(self):
        return self.n

    def bytes(self):
        assert self.n == 0, "align() first"
        return bytes(self.out)


def canonical(lengths):
    """Code of every symbol of a canonical Huffman code (RFC 1951 3.2.2); None where the length is 0.  The set may be
    incomplete or over-subscribed: the codes are then whatever the algorithm yields, truncated to their lengths."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        if n:
            out.append(nxt[n] & ((1 << n) - 1))
            nxt[n] += 1
        else:
            out.append(None)
    return out


def flat_lengths(used, size):
    """A complete code over the symbols `used`: lengths L - 1 and L.  One symbol gets a partner so that the set is complete."""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used + [used[0] + 1 if used[0] + 1 < size else used[0] - 1]))
    lens = [0] * size
    n = len(used)
    top = max(1, (n - 1).bit_length())
    short = (1 << top) - n
    for i, s in enumerate(used):
        lens[s] = top - 1 if i < short else top
    return lens


def length_symbol(length):
    assert 3 <= length <= 258
    k = max(i for i, b in enumerate(LENGTH_BASE) if b <= length)
    if length == 258:
        k = 28
    return 257 + k, LENGTH_EXTRA[k], length - LENGTH_BASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    k = max(i for i, b in enumerate(DIST_BASE) if b <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


def symbols_of(tokens):
    """(literal/length symbols, distance symbols) a token list uses."""
    lit, dist = [], []
    for t in tokens:
        if t == EOB:
            lit.append(256)
        elif isinstance(t, int):
            lit.append(t)
        elif t[0] == "sym":
            lit.append(t[1])
        elif t[0] == "dsym":
            lit.append(length_symbol(t[1])[0])
            dist.append(t[2])
        else:
            lit.append(length_symbol(t[0])[0])
            dist.append(dist_symbol(t[1])[0])
    return lit, dist


def expand(tokens, history=b""):
    """What a correct decoder makes of the tokens (matches may reach into `history`, the output of earlier blocks)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, tuple) and isinstance(t[0], int):
            length, dist = t
            assert dist <= len(out), "distance beyond the output"
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(history):])


def write_tokens(w, tokens, lit_lens, dist_lens):
    lit, dist = canonical(lit_lens), canonical(dist_lens)

    def emit(table, lens, s):
        assert lens[s], f"symbol {s} has no code"
        w.code(table[s], lens[s])

    for t in tokens:
        if t == EOB:
            emit(lit, lit_lens, 256)
        elif isinstance(t, int):
            emit(lit, lit_lens, t)
        elif t[0] == "sym":
            emit(lit, lit_lens, t[1])
        else:
            length = t[1] if t[0] == "dsym" else t[0]
            s, n, v = length_symbol(length)
            emit(lit, lit_lens, s)
            w.bits(v, n)
            d, dn, dv = (t[2], t[3], t[4]) if t[0] == "dsym" else dist_symbol(t[1])
            emit(dist, dist_lens, d)
            w.bits(dv, dn)


def stored_block(w, data, final=False, nlen=None, pad=0):
    """A stored block from the writer's current bit offset; nlen overrides the complement of LEN; pad fills the skipped bits."""
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align(pad)
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.raw(data)


def fixed_block(w, tokens, final=False):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    write_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def reserved_block(w, final=False):
    w.bits(1 if final else 0, 1)
    w.bits(3, 2)


def plain_cl_sequence(lengths):
    """Every code length as its own symbol (no repeats)."""
    return [(n, 0) for n in lengths]


def rle_cl_sequence(lengths):
    """Greedy 16 / 17 / 18 run coding over the concatenated lengths (so runs cross the literal / distance boundary)."""
    seq, i = [], 0
    while i < len(lengths):
        n, run = lengths[i], 1
        while i + run < len(lengths) and lengths[i + run] == n:
            run += 1
        if n == 0 and run >= 11:
            r = min(run, 138)
            seq.append((18, r - 11))
        elif n == 0 and run >= 3:
            r = min(run, 10)
            seq.append((17, r - 3))
        elif run >= 4:
            seq.append((n, 0))
            r = min(run - 1, 6)
            seq.append((16, r - 3))
            r += 1
        else:
            seq.append((n, 0))
            r = 1
        i += r
    return seq


def dynamic_block(w, tokens, final=False, lit_lens=None, dist_lens=None, hlit=None, hdist=None, hclen=None, cl_lens=None,
                  cl_seq=None, rle=True):
    """A dynamic block.  lit_lens / dist_lens (default: a flat complete code over the symbols the tokens use; no distance code
    used = one distance length of 0) are cut or padded to hlit / hdist entries (default: up to the last non-zero, at least 257
    and 1).  cl_seq: the (symbol, extra value) sequence that transmits them (default: run-coded, or plain with rle=False); cl_lens:
    the 19 lengths of the code-length code (default: flat over the symbols cl_seq uses); hclen: how many of them are sent."""
    used_lit, used_dist = symbols_of(tokens)
    if lit_lens is None:
        lit_lens = flat_lengths(used_lit + [256], 288)
    if dist_lens is None:
        dist_lens = flat_lengths(used_dist, 32) if used_dist else [0] * 32
    lit_lens, dist_lens = list(lit_lens) + [0] * (288 - len(lit_lens)), list(dist_lens) + [0] * (32 - len(dist_lens))
    if hlit is None:
        hlit = max(257, max((i + 1 for i, n in enumerate(lit_lens) if n), default=0))
    if hdist is None:
        hdist = max(1, max((i + 1 for i, n in enumerate(dist_lens) if n), default=0))
    if cl_seq is None:
        both = lit_lens[:hlit] + dist_lens[:hdist]
        cl_seq = rle_cl_sequence(both) if rle else plain_cl_sequence(both)
    if cl_lens is None:
        cl_lens = flat_lengths([s for s, _ in cl_seq], 19)
    if hclen is None:
        hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lens[s], 3)
    codes = canonical(cl_lens)
    for s, extra in cl_seq:
        assert cl_lens[s], f"code-length symbol {s} has no code"
        w.code(codes[s], cl_lens[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    write_tokens(w, tokens, lit_lens, dist_lens)


def zstream(raw, data, cmf=0x78, flg=None, fdict=False, bad_fcheck=False, adler=None, flip_adler_bit=None, tail=b"", cut=0):
    """RFC 1950 around the raw DEFLATE bytes `raw` that decode to `data`.  flg None: FLEVEL 2 with a valid FCHECK; fdict sets
    the bit (FCHECK still valid); bad_fcheck spoils it; adler overrides the checksum, flip_adler_bit flips one of its 32 bits;
    tail: bytes behind the trailer; cut: bytes dropped from the end."""
    if flg is None:
        flg = 0x80 | (0x20 if fdict else 0)
        flg += (31 - ((cmf << 8) | flg) % 31) % 31
        if bad_fcheck:
            flg ^= 1
    a = zlib.adler32(data) if adler is None else adler
    if flip_adler_bit is not None:
        a ^= 1 << flip_adler_bit
    out = bytes([cmf, flg]) + raw + a.to_bytes(4, "big") + tail
    return out[:len(out) - cut] if cut else out


def zlib_verdict(stream, want):
    """The rule of lemon_amd/png_host.py::fill_record with zlib.decompressobj(): (True, rows) for a stream that yields exactly
    `want` bytes, ends there and leaves nothing over; (False, None) otherwise."""
    z = zlib.decompressobj()
    try:
        rows = z.decompress(stream, want + 1)
    except zlib.error:
        return False, None
    if len(rows) != want or not z.eof or z.unused_data or z.unconsumed_tail:
        return False, None
    return True, rows
