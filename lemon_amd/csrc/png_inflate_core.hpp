// png_inflate_core.hpp -- the inflate of the PNG path (lib/datasets/dataloader.py:177-184 opens a PNG with
// `Image.open(p).convert("RGB")`; with LEMON_PNG=device the file's IDAT payload arrives compressed): a complete zlib / DEFLATE
// decoder (RFC 1950, RFC 1951) for ONE stream of known output size want = h * (stride + 1), written as the schedule of one
// wave of 64 lanes over a block of shared state, so that the kernel (png_inflate.hip: the state in LDS, the lanes real) and
// the host loop (lemon_png_inflate_host: the state on the heap, the lanes a for loop) execute the same code and give the same
// bytes and the same verdict.  Plain C++17, header-only, no HIP: also compiled with g++ into liblemon_jpeg_host.so and under
// AddressSanitizer / UBSan for the fuzzer (tests/native/png_inflate_fuzz.cpp).
//
// Acceptance rule (the one png_host.fill_record applies with Python's zlib): the header is CM = 8, CINFO <= 7, FCHECK valid,
// FDICT clear; exactly `want` bytes come out; the final block ends the stream; the four Adler-32 bytes match; NO byte follows
// them.  Everything else is DECLINED (status LEMON_PNG_STREAM, the caller decodes the file with PIL), never guessed at: block
// type 3, LEN / NLEN mismatch, HLIT > 286, HDIST > 30, a repeat with nothing to repeat or past HLIT + HDIST, an over-subscribed
// or incomplete code-length set (except a distance set of at most one 1-bit code, as zlib), a missing end-of-block code,
// literal/length symbols 286 / 287, distance symbols 30 / 31, a distance beyond the bytes produced, output beyond `want`,
// input exhausted.  The decoder may decline what zlib accepts (an incomplete literal set of one code); it never accepts what
// zlib rejects and never produces other bytes.
//
// The schedule.  The symbol walk of a DEFLATE stream is serial (every code starts where the previous ended, back-references
// rule out resynchronising), so lane 0 walks and the wave does everything that is wide:
//   input     the compressed bytes are staged into a ring (PZ_ZIN bytes) in aligned 16-byte pieces by all lanes before every
//             serial phase; a phase consumes at most PZ_PHASE_BYTES, the ring always holds that much ahead (or the stream's end)
//   tables    a dynamic block's code lengths are read by lane 0 (the code-length code is 19 symbols); then a lane per symbol
//             counts the lengths, lane 0 checks the Kraft sum and scans the counts into offsets, a lane per length writes the
//             symbols in canonical order, and a lane per entry fills the root tables (10 bits literal/length, 8 bits distance)
//             by walking its own index down the canonical code; codes longer than the root take that walk at decode time
//             (first code + count per length, 16 words) where zlib would chain sub-tables: same symbols, less LDS, and the walk
//             that fills the table is the walk that backs it up.  A fixed block loads its constant lengths into the same builder.
//   tokens    lane 0 fills a queue of up to PZ_QUEUE tokens (literal, or length + distance) with the offset each starts at
//             (it needs the running total anyway: a distance must not exceed the bytes produced); the wave places them: all
//             literals in one step, then the matches in order, each copied by all lanes, byte j of a match being
//             window[start - dist + (j mod dist)] -- an overlapping match (dist < length) is as wide as any other
//   stored    a wave-wide copy from the staging ring, PZ_STORED_CHUNK bytes a round
//   window    the last 32 KiB of output live in a ring; matches read the ring, never global memory; after every round the
//             finished aligned 16-byte pieces are written through to the record (alignment by the record's ADDRESS: output byte p
//             sits at ring slot (p + skew) & 32767), ragged ends byte by byte
//   adler     s1 = 1 + sum d[i], s2 = want + sum (want - i) * d[i] (mod 65521) because exactly `want` bytes are accepted, so
//             every lane sums the pieces it flushes on its own, reduced mod 65521 after every piece (a piece adds < 2^29), and
//             lane 0 adds the 64 partial sums at the end
// Every loop consumes input bits or produces output bytes or ends with a status; bits read past the end of the input are zeros
// that are counted, and consuming one of them is "input exhausted".  Nothing is read outside [in, in + n), nothing written
// outside [rows, rows + want).
#pragma once
#include <stdint.h>
#include <string.h>

#include "png_core.hpp"

#define PZ_LANES 64
#define PZ_WIN 32768                   // the window ring: DEFLATE's maximum distance
#define PZ_ZIN 2048                    // the staging ring of compressed bytes
#define PZ_PHASE_BYTES 1024            // no serial phase consumes more: a dynamic header <= 17 + 57 + 316 * 14 bits = 563 bytes, a
                                       // queue <= 64 * 48 bits = 384 bytes, a stored round PZ_STORED_CHUNK, each + 8 of look-ahead
#define PZ_STORED_CHUNK 1008
#define PZ_QUEUE 64
#define PZ_LIT_ROOT 10
#define PZ_DST_ROOT 8
#define PZ_ADLER 65521u

#if defined(__HIP_DEVICE_COMPILE__)
#define PZ_EACH_LANE(l) for (int l = (int)threadIdx.x, pz_once_ = 1; pz_once_; pz_once_ = 0)
#define PZ_FIRST_LANE if (threadIdx.x == 0)
#define PZ_SYNC() __syncthreads()
#define PZ_COUNT(p) atomicAdd((p), 1u)
#else
#define PZ_EACH_LANE(l) for (int l = 0; l < PZ_LANES; ++l)
#define PZ_FIRST_LANE
#define PZ_SYNC() ((void)0)
#define PZ_COUNT(p) (++*(p))
#endif

enum PzState { PZ_HEADER = 0, PZ_BUILD = 1, PZ_TOKENS = 2, PZ_STORED = 3, PZ_TRAILER = 4, PZ_DONE = 5 };

struct PzCtl {                         // written by lane 0 between two barriers, read by all lanes after the second
    int64_t pos;                       // bytes produced
    int64_t flushed;                   // bytes written through to the record
    int64_t zpos;                      // input byte that holds the next unread bit
    int64_t zhi;                       // staged so far: input bytes below zhi - zskew
    int64_t stored;                    // bytes left of a stored block
    int32_t state, final, bad, ntok, nmatch, fixed_ready, nlit, ndist;
};

struct PzShared {
    alignas(16) uint8_t win[PZ_WIN];
    alignas(16) uint8_t zin[PZ_ZIN];
    uint16_t lit[1 << PZ_LIT_ROOT], dst[1 << PZ_DST_ROOT];       // symbol << 4 | code length; 0: no code within the root bits
    uint16_t lsorted[288], dsorted[32];                          // symbols in canonical order
    uint32_t lcnt[16], dcnt[16], loff[16], doff[16];             // codes per length; first index per length in *sorted
    uint8_t lens[320];                                           // HLIT literal/length lengths, then HDIST distance lengths
    uint32_t queue[PZ_QUEUE];                                    // literal: the byte; match: 1 << 31 | dist << 9 | length
    uint32_t qat[PZ_QUEUE];                                      // output offset of the token from the queue's start
    uint8_t mlist[PZ_QUEUE];                                     // the queue's matches, in order (and the 19 code-length lengths)
    uint32_t ad_a[PZ_LANES], ad_b[PZ_LANES];                     // Adler-32 partial sums of the lanes
    PzCtl c;
};

struct PzBits {                        // lane 0's bit reader over the staging ring
    uint64_t buf;
    int32_t cnt;                       // valid bits in buf
    int32_t phantom;                   // of which, at the top, zeros from beyond the input
    int64_t next;                      // input byte fetched next
};

// One code of a canonical Huffman code off `bits` (LSB first): symbol << 4 | length, or 0 when no code of at most maxlen bits
// matches (maxlen below 15: the root tables; an incomplete set).  cnt / sorted describe a set that is not over-subscribed.
LEMON_PNG_HD uint32_t pz_walk(uint32_t bits, const uint32_t *cnt, const uint16_t *sorted, int maxlen) {
    int32_t code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
        code |= (int32_t)(bits & 1u);
        bits >>= 1;
        const int32_t count = (int32_t)cnt[len];
        if (code >= first && code - first < count) return ((uint32_t)sorted[index + (code - first)] << 4) | (uint32_t)len;
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return 0;
}

LEMON_PNG_HD void pz_ensure(PzShared &S, PzBits &b, const int64_t n, const int zskew, const int bits) {
    while (b.cnt < bits) {                                       // (bits <= 56)
        uint64_t v = 0;
        if (b.next >= n) b.phantom += 8;
        else if (b.next + zskew < S.c.zhi) v = S.zin[(b.next + zskew) & (PZ_ZIN - 1)];
        else S.c.bad = 1;                                        // (a phase outran the staging ring: never, but then decline)
        b.buf |= v << b.cnt;
        b.cnt += 8;
        b.next += 1;
    }
}

LEMON_PNG_HD uint32_t pz_take(PzBits &b, const int bits) {       // bits <= 16, after pz_ensure
    const uint32_t v = (uint32_t)b.buf & ((1u << bits) - 1u);
    b.buf >>= bits;
    b.cnt -= bits;
    return v;
}

// Stage input pieces so that [zpos, zpos + PZ_PHASE_BYTES + 8) or the rest of the input is in the ring.  All lanes.
LEMON_PNG_HD void pz_stage(PzShared &S, const uint8_t *in, const int64_t n, const int zskew) {
    const int64_t a = (S.c.zpos + zskew) & ~(int64_t)15, end = (n + zskew + 15) & ~(int64_t)15;
    const int64_t lim = a + PZ_ZIN < end ? a + PZ_ZIN : end;
    const int64_t from = S.c.zhi > a ? S.c.zhi : a;
    for (int64_t k0 = from; k0 < lim; k0 += 16 * PZ_LANES) {
        PZ_EACH_LANE(l) {
            const int64_t k = k0 + 16 * l;                       // the piece: input bytes [k - zskew, k - zskew + 16)
            if (k < lim) {
                uint8_t *slot = &S.zin[k & (PZ_ZIN - 1)];
                const int64_t lo = k - zskew;
                if (lo >= 0 && lo + 16 <= n) {
#if defined(__HIP_DEVICE_COMPILE__)
                    *reinterpret_cast<uint4 *>(slot) = *reinterpret_cast<const uint4 *>(in + lo);
#else
                    memcpy(slot, in + lo, 16);
#endif
                } else {
                    for (int j = 0; j < 16; ++j) slot[j] = (lo + j >= 0 && lo + j < n) ? in[lo + j] : (uint8_t)0;
                }
            }
        }
    }
    PZ_SYNC();
    PZ_FIRST_LANE { if (lim > S.c.zhi) S.c.zhi = lim; }
    PZ_SYNC();
}

// Write the finished pieces of the window through to the record and add them to the lanes' Adler sums.  All lanes.
LEMON_PNG_HD void pz_flush(PzShared &S, uint8_t *rows, const int64_t want, const int wskew, const bool last) {
    const int64_t q0 = S.c.flushed + wskew;
    const int64_t q1 = last ? S.c.pos + wskew : ((S.c.pos + wskew) & ~(int64_t)15);
    PZ_SYNC();
    if (q1 <= q0) return;
    const int64_t k1 = (q1 + 15) & ~(int64_t)15;
    for (int64_t k0 = q0 & ~(int64_t)15; k0 < k1; k0 += 16 * PZ_LANES) {
        PZ_EACH_LANE(l) {
            const int64_t k = k0 + 16 * l;
            if (k < k1) {
                const int64_t lo = k > q0 ? k : q0, hi = k + 16 < q1 ? k + 16 : q1;      // output bytes [lo - wskew, hi - wskew)
                const uint8_t *src = &S.win[k & (PZ_WIN - 1)];
                uint8_t *dst = rows + (k - wskew);
                uint32_t s = 0, t = 0;
                for (int64_t j = lo; j < hi; ++j) { s += src[j - k]; t += (uint32_t)(j - lo) * src[j - k]; }
                if (hi - lo == 16) {
#if defined(__HIP_DEVICE_COMPILE__)
                    *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
#else
                    memcpy(dst, src, 16);
#endif
                } else {
                    for (int64_t j = lo; j < hi; ++j) dst[j - k] = src[j - k];
                }
                // byte i weighs want - i in s2: (want - i0) * s - t, t <= 120 * 255 < 65521
                const uint32_t wm = (uint32_t)((uint64_t)(want - (lo - wskew)) % PZ_ADLER);
                S.ad_a[l] = (S.ad_a[l] + s) % PZ_ADLER;
                S.ad_b[l] = (S.ad_b[l] + (wm * s + PZ_ADLER - t) % PZ_ADLER) % PZ_ADLER;
            }
        }
    }
    PZ_SYNC();
    PZ_FIRST_LANE { S.c.flushed = q1 - wskew; }
    PZ_SYNC();
}

// The tables of one code from lens[0, n): counts, canonical order, root table.  All lanes.  Sets c.bad for an over-subscribed
// or incomplete set (incomplete_ok: a set of no code, or of one 1-bit code, passes -- zlib's rule for distances).
LEMON_PNG_HD void pz_build(PzShared &S, const uint8_t *lens, const int n, uint32_t *cnt, uint32_t *off, uint16_t *sorted,
                           uint16_t *table, const int root, const bool incomplete_ok) {
    PZ_EACH_LANE(l) { if (l < 16) cnt[l] = 0; }
    PZ_SYNC();
    for (int s0 = 0; s0 < n; s0 += PZ_LANES) {
        PZ_EACH_LANE(l) { if (s0 + l < n && lens[s0 + l]) PZ_COUNT(&cnt[lens[s0 + l]]); }
    }
    PZ_SYNC();
    PZ_FIRST_LANE {
        int32_t left = 1, most = 0;
        uint32_t at = 0;
        for (int len = 1; len <= 15; ++len) {
            left = 2 * left - (int32_t)cnt[len];
            if (left < 0) break;
            off[len] = at;
            at += cnt[len];
            if (cnt[len]) most = len;
        }
        if (left < 0 || (left > 0 && !(incomplete_ok && most <= 1))) S.c.bad = 1;
    }
    PZ_SYNC();
    if (S.c.bad) return;
    PZ_EACH_LANE(l) {
        if (l >= 1 && l < 16 && cnt[l]) {
            uint32_t at = off[l];
            for (int s = 0; s < n; ++s)
                if (lens[s] == l) sorted[at++] = (uint16_t)s;
        }
    }
    PZ_SYNC();
    for (int e0 = 0; e0 < (1 << root); e0 += PZ_LANES) {
        PZ_EACH_LANE(l) { table[e0 + l] = (uint16_t)pz_walk((uint32_t)(e0 + l), cnt, sorted, root); }
    }
    PZ_SYNC();
}

// ---- lane 0's serial phases.  Each leaves c.state, c.zpos and, on any violation, c.bad.

LEMON_PNG_HD void pz_sync_zpos(PzShared &S, PzBits &b) {
    if (b.cnt < b.phantom) S.c.bad = 1;                          // a bit from beyond the input was consumed: input exhausted
    S.c.zpos = b.next - ((b.cnt + 7) >> 3);
}

LEMON_PNG_HD int pz_cl_order(int i) {                            // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, 5 bits each
    const uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45;
    const uint64_t c = 11ull | 4ull << 5 | 12ull << 10 | 3ull << 15 | 13ull << 20 | 2ull << 25 | 14ull << 30 | 1ull << 35 | 15ull << 40;
    return (int)((i < 10 ? a >> (5 * i) : c >> (5 * (i - 10))) & 31);
}

LEMON_PNG_HD void pz_block_header(PzShared &S, PzBits &b, const int64_t n, const int zskew, const int64_t want) {
    pz_ensure(S, b, n, zskew, 3);
    S.c.final = (int32_t)pz_take(b, 1);
    const uint32_t type = pz_take(b, 2);
    if (type == 3) { S.c.bad = 1; return; }
    if (type == 0) {
        pz_take(b, b.cnt & 7);
        pz_ensure(S, b, n, zskew, 32);
        const uint32_t len = pz_take(b, 16), nlen = pz_take(b, 16);
        pz_sync_zpos(S, b);                                      // (cnt is a multiple of 8: zpos is the block's first byte)
        if ((len ^ 0xFFFFu) != nlen || (int64_t)len > want - S.c.pos || (int64_t)len > n - S.c.zpos) { S.c.bad = 1; return; }
        b.buf = 0; b.cnt = 0; b.phantom = 0; b.next = S.c.zpos;
        S.c.stored = len;
        S.c.state = len ? PZ_STORED : (S.c.final ? PZ_TRAILER : PZ_HEADER);
        return;
    }
    if (type == 1) {
        if (!S.c.fixed_ready) {
            for (int s = 0; s < 288; ++s) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (int s = 0; s < 32; ++s) S.lens[288 + s] = 5;
            S.c.nlit = 288; S.c.ndist = 32;
        }
        S.c.state = S.c.fixed_ready ? PZ_TOKENS : PZ_BUILD;
        S.c.fixed_ready = S.c.fixed_ready ? 1 : 2;               // 2: the tables being built are the fixed ones
        pz_sync_zpos(S, b);
        return;
    }
    S.c.fixed_ready = 0;
    pz_ensure(S, b, n, zskew, 14);
    const int nlit = 257 + (int)pz_take(b, 5), ndist = 1 + (int)pz_take(b, 5), ncode = 4 + (int)pz_take(b, 4);
    if (nlit > 286 || ndist > 30) { S.c.bad = 1; return; }
    // the code-length code, serial (19 symbols): its lengths in mlist, its counts and order in the distance arrays
    uint8_t *cl = S.mlist;
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        pz_ensure(S, b, n, zskew, 3);
        cl[pz_cl_order(i)] = (uint8_t)pz_take(b, 3);
    }
    for (int len = 0; len < 16; ++len) S.dcnt[len] = 0;
    for (int i = 0; i < 19; ++i) S.dcnt[cl[i]] += 1;
    S.dcnt[0] = 0;
    int32_t left = 1;
    uint32_t at = 0;
    for (int len = 1; len <= 7; ++len) {
        left = 2 * left - (int32_t)S.dcnt[len];
        if (left < 0) break;
        S.doff[len] = at;
        at += S.dcnt[len];
    }
    if (left != 0) { S.c.bad = 1; return; }                      // over-subscribed or incomplete (zlib: both rejected for this code)
    for (int i = 0; i < 19; ++i)
        if (cl[i]) S.dsorted[S.doff[cl[i]]++] = (uint16_t)i;
    const int total = nlit + ndist;
    for (int i = 0; i < total;) {
        pz_ensure(S, b, n, zskew, 14);
        const uint32_t e = pz_walk((uint32_t)b.buf, S.dcnt, S.dsorted, 7);
        if (!e) { S.c.bad = 1; return; }
        pz_take(b, (int)(e & 15));
        const int sym = (int)(e >> 4);
        if (sym < 16) { S.lens[i++] = (uint8_t)sym; continue; }
        int rep;
        uint8_t prev = 0;
        if (sym == 16) {
            if (i == 0) { S.c.bad = 1; return; }
            prev = S.lens[i - 1];
            rep = 3 + (int)pz_take(b, 2);
        } else if (sym == 17) {
            rep = 3 + (int)pz_take(b, 3);
        } else {
            rep = 11 + (int)pz_take(b, 7);
        }
        if (rep > total - i) { S.c.bad = 1; return; }
        for (int k = 0; k < rep; ++k) S.lens[i++] = prev;
    }
    if (S.lens[256] == 0) { S.c.bad = 1; return; }               // no end-of-block code
    S.c.nlit = nlit; S.c.ndist = ndist;
    S.c.state = PZ_BUILD;
    pz_sync_zpos(S, b);
}

// Up to PZ_QUEUE tokens of a fixed or dynamic block, or up to its end-of-block code.
LEMON_PNG_HD void pz_tokens(PzShared &S, PzBits &b, const int64_t n, const int zskew, const int64_t want) {
    int ntok = 0, nmatch = 0;
    int64_t at = S.c.pos;                                        // bytes produced once the queue is placed
    int64_t oldest = INT64_MAX;                                  // the oldest byte a match of this queue reads
    bool end = false;
    while (ntok < PZ_QUEUE) {
        // literals are placed before the queue's matches: one at `at` lands on the ring slot of byte at - 32768, which no
        // earlier match of the queue may still have to read, so the queue closes here and the token opens the next one
        if (at - PZ_WIN >= oldest) break;
        pz_ensure(S, b, n, zskew, 48);                           // 15 + 5 + 15 + 13: a whole token
        uint32_t e = S.lit[(uint32_t)b.buf & ((1u << PZ_LIT_ROOT) - 1u)];
        if (!(e & 15)) e = pz_walk((uint32_t)b.buf, S.lcnt, S.lsorted, 15);
        if (!e) { S.c.bad = 1; break; }
        pz_take(b, (int)(e & 15));
        const int sym = (int)(e >> 4);
        if (sym == 256) { end = true; break; }
        if (sym < 256) {
            if (at >= want) { S.c.bad = 1; break; }
            S.queue[ntok] = (uint32_t)sym;
            S.qat[ntok] = (uint32_t)(at - S.c.pos);
            at += 1;
        } else {
            if (sym > 285) { S.c.bad = 1; break; }
            int len;
            if (sym < 265) len = sym - 254;
            else if (sym == 285) len = 258;
            else {
                const int eb = (sym - 261) >> 2;
                len = 3 + ((4 + ((sym - 261) & 3)) << eb) + (int)pz_take(b, eb);
            }
            uint32_t d = S.dst[(uint32_t)b.buf & ((1u << PZ_DST_ROOT) - 1u)];
            if (!(d & 15)) d = pz_walk((uint32_t)b.buf, S.dcnt, S.dsorted, 15);
            if (!d) { S.c.bad = 1; break; }
            pz_take(b, (int)(d & 15));
            const int dsym = (int)(d >> 4);
            if (dsym > 29) { S.c.bad = 1; break; }
            int32_t dist;
            if (dsym < 4) dist = dsym + 1;
            else {
                const int eb = (dsym >> 1) - 1;
                dist = 1 + ((2 + (dsym & 1)) << eb) + (int32_t)pz_take(b, eb);
            }
            if (dist > at || len > want - at) { S.c.bad = 1; break; }
            S.queue[ntok] = 0x80000000u | ((uint32_t)dist << 9) | (uint32_t)len;
            S.qat[ntok] = (uint32_t)(at - S.c.pos);
            S.mlist[nmatch++] = (uint8_t)ntok;
            if (at - dist < oldest) oldest = at - dist;
            at += len;
        }
        ntok += 1;
        if (b.cnt < b.phantom) { S.c.bad = 1; break; }
    }
    S.c.ntok = ntok;
    S.c.nmatch = nmatch;
    if (end) S.c.state = S.c.final ? PZ_TRAILER : PZ_HEADER;
    pz_sync_zpos(S, b);
}

// The whole stream.  All lanes call it with the same arguments; returns LEMON_PNG_OK or LEMON_PNG_STREAM (to all lanes).
LEMON_PNG_HD int pz_inflate(PzShared &S, const uint8_t *in, const int64_t n, uint8_t *rows, const int64_t want) {
    const int zskew = (int)(reinterpret_cast<uintptr_t>(in) & 15), wskew = (int)(reinterpret_cast<uintptr_t>(rows) & 15);
    PzBits b;
    b.buf = 0; b.cnt = 0; b.phantom = 0; b.next = 0;
    PZ_EACH_LANE(l) { S.ad_a[l] = 0; S.ad_b[l] = 0; }
    PZ_FIRST_LANE {
        S.c.pos = S.c.flushed = S.c.zpos = S.c.zhi = S.c.stored = 0;
        S.c.state = PZ_HEADER; S.c.final = S.c.bad = S.c.ntok = S.c.nmatch = S.c.fixed_ready = S.c.nlit = S.c.ndist = 0;
    }
    PZ_SYNC();
    pz_stage(S, in, n, zskew);
    PZ_FIRST_LANE {                                              // RFC 1950: CMF, FLG
        pz_ensure(S, b, n, zskew, 16);
        const uint32_t cmf = pz_take(b, 8), flg = pz_take(b, 8);
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) S.c.bad = 1;
        pz_sync_zpos(S, b);
    }
    PZ_SYNC();
    while (!S.c.bad && S.c.state != PZ_DONE) {
        pz_stage(S, in, n, zskew);
        const int state = S.c.state;
        PZ_SYNC();
        if (state == PZ_HEADER) {
            PZ_FIRST_LANE { pz_block_header(S, b, n, zskew, want); }
            PZ_SYNC();
        } else if (state == PZ_BUILD) {
            pz_build(S, S.lens, S.c.nlit, S.lcnt, S.loff, S.lsorted, S.lit, PZ_LIT_ROOT, false);
            if (!S.c.bad) pz_build(S, S.lens + S.c.nlit, S.c.ndist, S.dcnt, S.doff, S.dsorted, S.dst, PZ_DST_ROOT, true);
            PZ_SYNC();
            PZ_FIRST_LANE { S.c.state = PZ_TOKENS; S.c.fixed_ready = S.c.fixed_ready == 2 ? 1 : 0; }
            PZ_SYNC();
        } else if (state == PZ_TOKENS) {
            PZ_FIRST_LANE { pz_tokens(S, b, n, zskew, want); }
            PZ_SYNC();
            // (a queue cut short by a violation is not placed: what it would add is never accepted)
            if (!S.c.bad) {
                const int ntok = S.c.ntok, nmatch = S.c.nmatch;
                const int64_t pos = S.c.pos + wskew;
                PZ_EACH_LANE(l) {
                    if (l < ntok && !(S.queue[l] >> 31)) S.win[(pos + S.qat[l]) & (PZ_WIN - 1)] = (uint8_t)S.queue[l];
                }
                PZ_SYNC();
                for (int m = 0; m < nmatch; ++m) {
                    const int t = S.mlist[m];
                    const uint32_t q = S.queue[t];
                    const int len = (int)(q & 511u), dist = (int)((q >> 9) & 0xFFFFu);
                    const int64_t start = pos + S.qat[t];
                    for (int j0 = 0; j0 < len; j0 += PZ_LANES) {
                        PZ_EACH_LANE(l) {
                            const int j = j0 + l;
                            if (j < len)
                                S.win[(start + j) & (PZ_WIN - 1)] = S.win[(start - dist + (dist >= len ? j : j % dist)) & (PZ_WIN - 1)];
                        }
                    }
                    PZ_SYNC();
                }
                PZ_FIRST_LANE {
                    if (ntok) S.c.pos += S.qat[ntok - 1] + ((S.queue[ntok - 1] >> 31) ? (S.queue[ntok - 1] & 511u) : 1u);
                }
                PZ_SYNC();
                pz_flush(S, rows, want, wskew, false);
            }
        } else if (state == PZ_STORED) {
            const int chunk = (int)(S.c.stored < PZ_STORED_CHUNK ? S.c.stored : PZ_STORED_CHUNK);
            const int64_t pos = S.c.pos + wskew, zp = S.c.zpos + zskew;
            for (int j0 = 0; j0 < chunk; j0 += PZ_LANES) {
                PZ_EACH_LANE(l) {
                    if (j0 + l < chunk) S.win[(pos + j0 + l) & (PZ_WIN - 1)] = S.zin[(zp + j0 + l) & (PZ_ZIN - 1)];
                }
            }
            PZ_SYNC();
            PZ_FIRST_LANE {
                S.c.pos += chunk; S.c.zpos += chunk; S.c.stored -= chunk;
                b.next = S.c.zpos;
                if (!S.c.stored) S.c.state = S.c.final ? PZ_TRAILER : PZ_HEADER;
            }
            PZ_SYNC();
            pz_flush(S, rows, want, wskew, false);
        } else {                                                 // PZ_TRAILER
            pz_flush(S, rows, want, wskew, true);
            PZ_FIRST_LANE {
                pz_take(b, b.cnt & 7);
                pz_sync_zpos(S, b);
                if (S.c.pos != want || S.c.zpos != n - 4) S.c.bad = 1;
                if (!S.c.bad) {
                    uint32_t s1 = 1, s2 = (uint32_t)((uint64_t)want % PZ_ADLER);
                    for (int l = 0; l < PZ_LANES; ++l) { s1 = (s1 + S.ad_a[l]) % PZ_ADLER; s2 = (s2 + S.ad_b[l]) % PZ_ADLER; }
                    const uint8_t *t = in + (n - 4);
                    const uint32_t adler = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
                    if (adler != ((s2 << 16) | s1)) S.c.bad = 1;
                }
                S.c.state = PZ_DONE;
            }
            PZ_SYNC();
        }
    }
    const int verdict = S.c.bad ? LEMON_PNG_STREAM : LEMON_PNG_OK;
    PZ_SYNC();
    return verdict;
}

// The host twin: the same schedule with the lanes looped.  Returns 0 unless an argument is invalid (then nothing is read or
// written); *status = 0 or LEMON_PNG_STREAM.  rows[0, want) holds the scanlines of an accepted stream.
static inline int lemon_png_inflate_host_impl(const uint8_t *z, int64_t n, uint8_t *rows, int64_t want, int32_t *status) {
    if (!z || !rows || !status || n < 0 || want < 0) return 1;
    PzShared *S = new PzShared;
    *status = pz_inflate(*S, z, n, rows, want);
    delete S;
    return 0;
}
