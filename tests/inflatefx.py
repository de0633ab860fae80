"""The zlib streams of the inflate tests (tests/test_png_inflate_host.py on the CPU, tests/test_gpu_png_inflate.py on the device),
built once per session: (a) streams zlib writes over its settings, (b) streams written token by token with tests/deflatefx.py at
every edge of csrc/png_inflate_core.hpp, (c) streams that must be declined.  Every case is (name, stream, want); the expected
bytes are zlib's own (deflatefx.zlib_verdict, the rule of png_host.fill_record)."""
import functools
import zlib

import numpy as np

from tests import deflatefx as fx
from tests.deflatefx import EOB

WANTS = (1, 2, 257, 258, 259, 32767, 32768, 32769, 66000)


def _data(kind, want, rng):
    if kind == "noise":
        return rng.integers(0, 256, want, dtype=np.uint8).tobytes()
    if kind == "zeros":
        return bytes(want)
    if kind == "runs":
        return np.repeat(rng.integers(0, 256, want // 7 + 1, dtype=np.uint8), 7)[:want].tobytes()
    # "rows": filtered image rows -- small differences behind a filter-type byte every 131 bytes
    a = (rng.integers(-3, 4, want) % 256).astype(np.uint8)
    a[::131] = rng.integers(0, 5, a[::131].size)
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def zlib_cases():
    """(a): noise, zeros, runs and filtered rows at every `want`, levels 0 / 1 / 6 / 9, the five strategies, wbits 9 / 15,
    memLevel 1 / 9, and no flush, a Z_SYNC_FLUSH or a Z_FULL_FLUSH in the middle (cycling).  2880 streams."""
    rng = np.random.default_rng(20261021)
    out, k = [], 0
    for want in WANTS:
        for kind in ("noise", "zeros", "runs", "rows"):
            d = _data(kind, want, rng)
            for level in (0, 1, 6, 9):
                for sname, strat in (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE),
                                     ("huffman", zlib.Z_HUFFMAN_ONLY), ("filtered", zlib.Z_FILTERED)):
                    for wbits in (9, 15):
                        for mem in (1, 9):
                            c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strat)
                            flush = (None, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)[k % 3]
                            k += 1
                            z = c.compress(d[:want // 2])
                            if flush is not None:
                                z += c.flush(flush)
                            z += c.compress(d[want // 2:]) + c.flush()
                            out.append((f"{kind}{want}_l{level}_{sname}_w{wbits}_m{mem}_f{flush}", z, want))
    return out


def _history(rng, n):
    """Stored blocks of n random bytes: cheap history for far distances.  -> (writer with the blocks, the bytes)"""
    w = fx.BitWriter()
    d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for i in range(0, n, 65535):
        fx.stored_block(w, d[i:i + 65535])
    return w, d


def _finish(name, w, data, **kw):
    w.align()
    return (name, fx.zstream(w.bytes(), data, **kw), len(data))


def _lits(rng, n, lo=0, hi=256):
    return [int(v) for v in rng.integers(lo, hi, n)]


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(b): hand-written streams, each valid (zlib accepts every one: checked by the tests)."""
    rng = np.random.default_rng(7)
    out = []

    def one_block(name, tokens, kind="fixed", history=0, **kw):
        if history:
            w, hist = _history(rng, history)
        else:
            w, hist = fx.BitWriter(), b""
        (fx.fixed_block if kind == "fixed" else fx.dynamic_block)(w, tokens + [EOB], True, **kw)
        out.append(_finish(name, w, hist + fx.expand(tokens, hist)))

    # every length base, with its extra bits at both ends
    lengths = sorted({3, 258} | {b + e for b, x in zip(fx.LENGTH_BASE, fx.LENGTH_EXTRA) for e in (0, (1 << x) - 1)})
    for kind in ("fixed", "dynamic"):
        toks = _lits(rng, 300)
        for i, n in enumerate(lengths):
            toks += [(n, (1, 7, 300)[i % 3]), int(rng.integers(0, 256))]
        one_block(f"lengths_{kind}", toks, kind)
    # distances 1, 2, 63, 64, 65, 32767, 32768 with a length below, equal to and above the distance
    toks = []
    for d in (1, 2, 63, 64, 65, 32767, 32768):
        for n in sorted({min(max(n, 3), 258) for n in (d - 1, d, d + 1, 3, 258)}):
            toks += [(n, d), int(rng.integers(0, 256))]
    one_block("distances_fixed", toks, "fixed", history=32768)
    one_block("distances_dynamic", toks, "dynamic", history=32768)
    # a far match whose first source byte is the ring slot of the literal that follows it, and its neighbours
    toks = []
    for n in (3, 4, 100, 258):
        for d in (32768 - n - 1, 32768 - n, 32768 - n + 1, 32768):
            toks += [(n, d), 1, 2, (n, d), (5, 32768)] + _lits(rng, 3)
    one_block("far_match_then_literals", toks, "fixed", history=32768 + 50)
    # a match crossing the window wrap, at the wrap, and just behind it
    for back in (300, 258, 257, 1, 0):
        one_block(f"wrap_minus_{back}", [(258, 5), 9, (258, 30000), (40, 1)], "fixed", history=32768 - back)
    one_block("wrap_twice", _lits(rng, 40) + [(258, 17)] * 260, "dynamic")
    # a match crossing a 16-byte piece; as the 64th token of a queue, as the first of the next; the last before end of block
    one_block("piece_crossing", _lits(rng, 10) + [(20, 3), 5, (13, 16), (3, 1)])
    for n in (62, 63, 64, 65):
        one_block(f"match_as_token_{n + 1}", _lits(rng, n) + [(258, n), 7] + _lits(rng, 70) + [(3, 2)])
    one_block("match_last_before_eob", _lits(rng, 5) + [(10, 2)], "dynamic")
    # end of block as the first token of a queue; empty final blocks of all three types
    one_block("eob_first_in_queue", _lits(rng, 64))
    one_block("eob_first_in_queue_dynamic", _lits(rng, 128), "dynamic")
    for kind in ("stored", "fixed", "dynamic"):
        w = fx.BitWriter()
        toks = _lits(rng, 30) + [(9, 4)]
        fx.fixed_block(w, toks + [EOB])
        if kind == "stored":
            fx.stored_block(w, b"", True)
        elif kind == "fixed":
            fx.fixed_block(w, [EOB], True)
        else:
            fx.dynamic_block(w, [EOB], True)
        out.append(_finish(f"empty_final_{kind}", w, fx.expand(toks)))
    # stored blocks: length 0, length 65535, starting at each of the eight bit offsets (the skipped bits set)
    w = fx.BitWriter()
    big = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    fx.stored_block(w, b"")
    fx.stored_block(w, big)
    fx.stored_block(w, b"")
    fx.stored_block(w, b"xyz", True)
    out.append(_finish("stored_0_65535", w, big + b"xyz"))
    offsets = set()
    for j in range(8):
        w = fx.BitWriter()
        lead = [200] * j + [3] * 5                       # j nine-bit codes: the block ends at bit (3 + 9 j + 8 * 5 + 7) mod 8
        fx.fixed_block(w, lead + [EOB])
        at = w.bit_offset
        offsets.add(at)
        fx.stored_block(w, b"stored after %d" % j, False, pad=0xFF)
        fx.fixed_block(w, [(6, 3), EOB], True)
        d = fx.expand(lead) + b"stored after %d" % j
        out.append(_finish(f"stored_at_bit_{at}", w, d + fx.expand([(6, 3)], d)))
    assert len(offsets) == 8
    # BFINAL on the first block; after 100 blocks of mixed types
    one_block("final_first_fixed", _lits(rng, 3))
    w = fx.BitWriter()
    fx.stored_block(w, b"only", True)
    out.append(_finish("final_first_stored", w, b"only"))
    w, d = fx.BitWriter(), b""
    for k in range(100):
        if k % 3 == 0:
            piece = rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
            fx.stored_block(w, piece, False, pad=k)
            d += piece
        else:
            toks = _lits(rng, int(rng.integers(1, 90))) + ([(int(rng.integers(3, 259)), int(rng.integers(1, min(len(d), 32768) + 1)))] if d else [])
            (fx.fixed_block if k % 3 == 1 else fx.dynamic_block)(w, toks + [EOB])
            d += fx.expand(toks, d)
    fx.fixed_block(w, [0, EOB], True)
    out.append(_finish("final_after_100_blocks", w, d + b"\0"))
    # dynamic tables: codes of 1 .. 15 bits in both alphabets (HCLEN 19: length 15 is the last of the order)
    lit15 = [0] * 288
    for s in range(14):
        lit15[s] = s + 1
    lit15[14] = lit15[256] = 15
    one_block("lit_code_15_bits", [int(v) for v in rng.integers(0, 15, 400)] + [14, 13, 12, 11, 10, 9], "dynamic", lit_lens=lit15)
    lit_m = fx.flat_lengths(list(range(16)) + [256] + [257 + k for k in range(29)], 288)
    dist15 = [0] * 32
    for s in range(14):
        dist15[s] = s + 1
    dist15[14] = dist15[15] = 15
    toks = _lits(rng, 300, 0, 16)
    for d_ in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 192, 193, 256):
        toks += [(int(rng.integers(3, 259)), d_), int(rng.integers(0, 16))]
    one_block("dist_code_15_bits", toks, "dynamic", lit_lens=lit_m, dist_lens=dist15)
    # HCLEN 5: the order's first five are 16 17 18 0 8, so every code is 8 bits (HCLEN 4 cannot name an end-of-block code:
    # with the declines); HCLEN 19 above
    lit8 = [8] * 255 + [0] + [8] + [0] * 31
    for rle in (False, True):
        one_block(f"hclen_5_rle{int(rle)}", _lits(rng, 100, 0, 255), "dynamic", lit_lens=lit8, dist_lens=[0] * 32, rle=rle)
    # repeats 16 / 17 / 18 crossing the literal / distance boundary
    # 16: four lengths of 4 end the literal set (253 .. 256, and the length symbol 257) and sixteen open the distance set
    lit = [1, 2] + [0] * 252 + [4, 4, 4, 4]             # 0, 1 and 254 .. 257: 1/2 + 1/4 + 4/16
    one_block("repeat16_crosses", [0, 1, 254, 255, 0, (3, 1), (3, 8)], "dynamic", lit_lens=lit, dist_lens=[4] * 16, hlit=258, hdist=16)
    # 17 and 18: zeros end the literal set (HLIT beyond the last code) and open the distance set
    lit = fx.flat_lengths([1, 2, 256, 257], 288)
    one_block("repeat17_crosses", [1, 2, 1, (3, 5)], "dynamic", lit_lens=lit, hlit=261, dist_lens=[0, 0, 0, 0, 1, 1], history=10)
    one_block("repeat18_crosses", [1, 2, 1, (3, 1100)], "dynamic", lit_lens=lit, hlit=286, dist_lens=[0] * 20 + [1, 1], history=2000)
    # a single distance code (incomplete, as zlib allows), as symbol 0 and as symbol 4; no distance code at all
    one_block("single_dist_code_0", _lits(rng, 9) + [(30, 1), 4, (3, 1)], "dynamic", dist_lens=[1])
    one_block("single_dist_code_4", _lits(rng, 9) + [(30, 5), 4, (3, 6)], "dynamic", dist_lens=[0, 0, 0, 0, 1])
    one_block("no_dist_code", _lits(rng, 200), "dynamic")
    # a code straddling every staging piece: 8- and 9-bit codes over 6 KiB of input, run at every input alignment by the tests
    one_block("straddle_pieces", _lits(rng, 6000))
    # the last code ends on the last bit of the last byte: 3 + 6 * 9 + 7 = 64 bits
    w = fx.BitWriter()
    fx.fixed_block(w, [200] * 6 + [EOB], True)
    assert w.bit_offset == 0
    out.append(_finish("ends_on_last_bit", w, bytes([200] * 6)))
    # 6000 bytes of 0xFF: the Adler modulus
    one_block("adler_ff_matches", [255] + [(258, 1)] * 23 + [(65, 1)])
    w = fx.BitWriter()
    fx.stored_block(w, b"\xff" * 6000, True)
    out.append(_finish("adler_ff_stored", w, b"\xff" * 6000))
    assert len(out[-2][1]) and out[-2][2] == 6000
    return out


@functools.lru_cache(maxsize=None)
def decline_cases():
    """(c): (name, stream, want, strict).  strict: zlib rejects it under the fill_record rule and the decoder must decline;
    not strict: zlib accepts it (its non-strict rules, or a set the decoder is allowed to decline) and either verdict is right,
    with equal bytes where the decoder accepts."""
    rng = np.random.default_rng(9)
    out = []
    base = _lits(rng, 40) + [(12, 7), 3, 4]
    data = fx.expand(base)

    def block(name, writer, want=None, strict=True, produced=b"", **zkw):
        w = fx.BitWriter()
        writer(w)
        w.align()
        out.append((name, fx.zstream(w.bytes(), produced, **zkw), len(produced) if want is None else want, strict))

    good = lambda w: fx.fixed_block(w, base + [EOB], True)
    block("block_type_3", lambda w: (fx.fixed_block(w, base + [EOB]), fx.reserved_block(w, True)), produced=data)
    block("stored_nlen_mismatch", lambda w: fx.stored_block(w, data, True, nlen=(len(data) ^ 0xFFFF) ^ 0x0100), produced=data)
    lit = fx.flat_lengths(symbols := sorted(set(fx.symbols_of(base + [EOB])[0])), 288)
    dist = fx.flat_lengths(fx.symbols_of(base)[1], 32)
    block("hlit_287", lambda w: fx.dynamic_block(w, base + [EOB], True, lit_lens=lit, dist_lens=dist, hlit=287), produced=data)
    block("hlit_288", lambda w: fx.dynamic_block(w, base + [EOB], True, lit_lens=lit, dist_lens=dist, hlit=288), produced=data)
    block("hdist_31", lambda w: fx.dynamic_block(w, base + [EOB], True, lit_lens=lit, dist_lens=dist, hdist=31), produced=data)
    block("hdist_32", lambda w: fx.dynamic_block(w, base + [EOB], True, lit_lens=lit, dist_lens=dist, hdist=32), produced=data)
    hl, hd = max(i + 1 for i, n in enumerate(lit) if n), max(i + 1 for i, n in enumerate(dist) if n)
    seq = fx.plain_cl_sequence(lit[:hl] + dist[:hd])
    cl_all = fx.flat_lengths([s for s, _ in seq] + [16, 17, 18], 19)
    dyn = lambda **kw: (lambda w: fx.dynamic_block(w, base + [EOB], True, **{**dict(lit_lens=lit, dist_lens=dist, hlit=hl, hdist=hd, cl_lens=cl_all), **kw}))
    block("dynamic_control", dyn(cl_seq=seq), produced=data, strict=None)
    block("repeat_nothing_to_repeat", dyn(cl_seq=[(16, 0)] + seq[3:]), produced=data)
    block("repeat16_past_the_end", dyn(cl_seq=seq[:-2] + [(seq[-3][0], 0), (16, 3)]), produced=data)
    block("repeat18_past_the_end", dyn(cl_seq=seq[:-2] + [(18, 127)]), produced=data)
    block("repeat17_past_the_end", dyn(cl_seq=seq[:-1] + [(17, 7)]), produced=data)
    over = list(lit)
    over[symbols[0]] = 1
    over[symbols[1]] = 1
    over[symbols[2]] = 1
    block("lit_oversubscribed", lambda w: fx.dynamic_block(w, [EOB], True, lit_lens=over, dist_lens=dist), want=0)
    block("dist_oversubscribed", lambda w: fx.dynamic_block(w, [EOB], True, lit_lens=lit, dist_lens=[1, 1, 1]), want=0)
    block("cl_oversubscribed", dyn(cl_seq=seq, cl_lens=[1 if s in (0, 16, 17) else n for s, n in enumerate(cl_all)]), produced=data)
    block("cl_incomplete", lambda w: fx.dynamic_block(w, [EOB], True, lit_lens=[0] * 256 + [1], dist_lens=[0], rle=False,
                                                        cl_lens=[2, 2] + [0] * 17, cl_seq=[(0, 0)] * 256 + [(1, 0), (0, 0)]), want=0)
    block("cl_all_zero", lambda w: fx.dynamic_block(w, [], True, lit_lens=[0] * 257, dist_lens=[0], cl_lens=[0] * 19, cl_seq=[], hclen=19), want=0)
    inc = [0] * 288
    inc[5] = inc[256] = 2
    block("lit_incomplete", lambda w: fx.dynamic_block(w, [5, EOB], True, lit_lens=inc), want=1, produced=b"\x05")
    block("dist_incomplete_two_codes", lambda w: fx.dynamic_block(w, [5, 5, 5, (3, 1), EOB], True, dist_lens=[2, 2]), produced=bytes([5] * 6))
    noeob = [0] * 288
    noeob[0] = noeob[1] = 1
    block("missing_end_of_block_code", lambda w: fx.dynamic_block(w, [0, 1, 1], True, lit_lens=noeob), want=3, produced=b"\0\1\1")
    block("hclen_4_names_no_code", lambda w: fx.dynamic_block(w, [], True, lit_lens=[0] * 257, dist_lens=[0], cl_lens=[1] + [0] * 15 + [0, 0, 1],
                                                                cl_seq=[(18, 127), (18, 108), (0, 0)], hclen=4), want=0)
    for s in (286, 287):
        block(f"literal_length_symbol_{s}", lambda w, s=s: fx.fixed_block(w, base + [("sym", s), EOB], True), produced=data)
    for s in (30, 31):
        block(f"distance_symbol_{s}", lambda w, s=s: fx.fixed_block(w, base + [("dsym", 3, s, 0, 0), EOB], True), produced=data, want=len(data) + 3)
    block("distance_beyond_output", lambda w: fx.fixed_block(w, [1, 2, ("dsym", 3, 2, 0, 0), EOB], True), produced=b"\1\2", want=5)
    block("distance_beyond_output_far", lambda w: fx.fixed_block(w, base + [("dsym", 3, 29, 13, 8191), EOB], True), produced=data, want=len(data) + 3)
    block("single_dist_code_other_bit", lambda w: (fx.dynamic_block(w, [5, 5, 5, ("sym", 257)], True, dist_lens=[1]), w.bits(1, 1)),
          produced=bytes([5] * 3), want=6)
    block("want_one_less", good, produced=data, want=len(data) - 1)
    block("want_one_less_match_last", lambda w: fx.fixed_block(w, base[:-2] + [EOB], True), produced=data[:-2], want=len(data) - 3)
    block("want_one_more", good, produced=data, want=len(data) + 1)
    block("stored_beyond_want", lambda w: fx.stored_block(w, data, True), produced=data, want=len(data) - 1)
    block("trailing_byte", good, produced=data, tail=b"\0")
    for cut in (1, 4, 5, 6, 20):
        block(f"truncated_{cut}", good, produced=data, cut=cut)
    block("truncated_stored", lambda w: fx.stored_block(w, data, True), produced=data, cut=10)
    block("no_final_block", lambda w: fx.fixed_block(w, base + [EOB], False), produced=data)
    for bit in (0, 15, 16, 31):
        block(f"adler_bit_{bit}", good, produced=data, flip_adler_bit=bit)
    block("fdict", good, produced=data, fdict=True)
    block("cm_7", good, produced=data, cmf=0x77)
    block("cinfo_8", good, produced=data, cmf=0x88)
    block("bad_fcheck", good, produced=data, bad_fcheck=True)
    block("empty", lambda w: None, produced=b"", cut=6)
    block("header_only", lambda w: None, produced=b"", cut=4)
    # zlib accepts these (checked): either verdict, equal bytes
    w, hist = _history(rng, 600)
    fx.fixed_block(w, [(20, 500), EOB], True)
    w.align()
    d = hist + fx.expand([(20, 500)], hist)
    out.append(("distance_above_header_window", fx.zstream(w.bytes(), d, cmf=0x08), len(d), False))
    block("lit_single_code", lambda w: (fx.stored_block(w, b"abc"), fx.dynamic_block(w, [EOB], True, lit_lens=[0] * 256 + [1])),
          produced=b"abc", strict=False)
    return out
