// jpeg_prog_par.hpp -- the device form of the Huffman pass of a PROGRESSIVE JPEG (SOF2): the packet a decode worker writes
// (lemon_jpeg_prog_pack, jpeg_prog.hpp) and the step functions that the kernels (jpeg_prog.hip) and the host loop
// (lemon_jpeg_prog_entropy_par_host) share.  Plain C++17, no HIP needed.  Bit window, Huffman step, the head's geometry, the
// interval-to-MCU map, the envelope loop and the record initialisation are jpeg_par.hpp's; the table builder is
// jpeg_entropy.hpp's (jpeg_build_huff).
//
// Packet (little endian, the whole a multiple of 16 bytes):
//   int32  head[32]           kH* below: magic "LJP2", geometry, scans, pool entries, wave items, levels, section offsets (at 0)
//   uint16 quant[3][64]       per component, natural order, as in effect at the component's first scan (at 128)
//   int32  scan[scans][16]    kS* below, one row per SOS in file order (at 512): component (or -1: all three interleaved),
//                             Ss, Se, Ah, Al, level, ITS OWN restart interval, its interval count, offset (within `data`) and
//                             byte count of its destuffed bytes, packet offset of its interval-end list (0 with one interval),
//                             pool indices of its tables (DC first scan: one per component; AC scans: one; DC refinement: none)
//   uint32 pool[entries]      packet offset of every Huffman specification that a scan uses
//   uint8  spec[...]          the specifications as in the file: 16 counts, then sum(counts) values; unaligned, back to back
//   uint32 ends[...]          per scan with more than one restart interval: the END offset of every interval within the scan's
//                             bytes (interval t is [ends[t-1], ends[t]); running sums of the interval lengths)
//   uint8  data[data_bytes]   every scan's entropy-coded bytes with FF 00 -> FF and restart markers and fill bytes removed
// Level of a scan = 1 + the highest level of an earlier scan that touches the same component and an overlapping band (0 when
// there is none): scans of one level write disjoint coefficients.  Pillow's script has levels 0, 1, 2.
// Capacity: n + 2 * (n / 3) + LEMON_JPEG_PROG_PACKET_BOUND bytes hold the packet of every n-byte file.  Fixed part: head 128 +
// quantisers 384 + 64 scan rows of 64 + 192 pool offsets of 4 + three paddings to 16 = 5424.  Variable part: a specification
// takes 16 + values bytes here and one more (Tc/Th) in the file; data bytes are the file's or fewer; an interval end takes 4
// bytes where the file spends 2 on the restart marker that closes the interval and at least 1 on its data, so the ends add at
// most 2 bytes per 3 of the file.
//
// Device pass.  A work ITEM is (image, scan, group of LEMON_JPEG_PROG_GROUP consecutive restart intervals) and is decoded by one
// wave; the items of one level are one launch, so no wave waits for another inside a launch.  Lane k of the wave holds zig-zag
// coefficient k of the current block.  The Huffman step is wave-uniform; what a symbol does to the block is done by all lanes:
//   AC refinement  H = the band's lanes whose coefficient is non-zero.  A symbol (r, s) targets the (r+1)-th clear lane of H at
//                  or after k; the correction bits of the H lanes passed on the way are one contiguous field, bit j for the
//                  lane of rank j, applied at once by libjpeg's rule ((coef & p1) == 0 -> +-p1).  The tail of a block inside
//                  an EOB run is the same with the rest of the band.
//   AC first       the lane of the decoded index takes extend(bits, s) << Al; a block inside an EOB run is not touched.
//   DC refinement  bit i of an interval belongs to block i: 64 blocks per step.
//   DC first       the difference chain of the interval.
// Status of an image: LEMON_JPEG_BUFFER when the plan rejects the packet; else the largest code raised by the items of the FIRST
// level at which any item raised one (an item stops at its first error; later levels of that image do not run, so no item ever
// decodes on top of another's wreck and the verdict does not depend on the order waves run in); else the envelope's.
#pragma once
#include "jpeg_par.hpp"

#define LEMON_JPEG_PROG_GROUP LEMON_JPEG_PROG_ITEM          // restart intervals per wave item (include/lemon_hip.h)

namespace lemon_jpeg_prog {

using lemon_jpeg_par::ParBits;
using lemon_jpeg_par::ParHuff;
using lemon_jpeg_par::par_extend;
using lemon_jpeg_par::par_peek32;
using lemon_jpeg_par::par_symbol;

enum { kHMagic = 0, kHWidth, kHHeight, kHComponents, kHHs, kHVs, kHScans, kHPool, kHItems, kHLevels, kHPoolOff, kHDataOff,
       kHDataBytes, kHTotal, kHeadInts = 32 };
enum { kSComp = 0, kSSs, kSSe, kSAh, kSAl, kSLevel, kSRestart, kSIntervals, kSData, kSBytes, kSEnds, kSTab0, kSTab1, kSTab2,
       kScanInts = 16 };
static const int32_t kMagic = 0x32504A4C;          // "LJP2"
static const int32_t kQuantOff = 128, kScanOff = 512;

struct ProgImage : lemon_jpeg_par::PacketGeom {          // a validated packet head
    int32_t scans, pool, items, levels;
    int64_t bytes, pool_off, data_off, data_bytes;
    const uint8_t *pkt;
};

struct ProgScan {                     // a validated scan row
    int32_t comp, ss, se, ah, al, level, restart, nivl, items;
    int32_t t0, t1, t2;               // pool indices (see the packet)
    int32_t bw, spm;                  // blocks per row of a single-component scan; blocks per MCU
    int64_t mcus, bytes;
    const uint8_t *data;
    const uint32_t *ends;
};

LEMON_JPEG_HD uint64_t prog_range(int a, int b) {                    // bits a .. b - 1, 0 <= a, b <= 64
    if (a >= b) return 0;
    const uint64_t hi = b >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << b) - 1);
    return hi & ~(((uint64_t)1 << a) - 1);
}

// Reads the head of the packet in pkt[0, bytes) and checks every section against `bytes`, the record against `rec_room`.
LEMON_JPEG_HD bool prog_open(const uint8_t *pkt, int64_t bytes, int64_t rec_room, ProgImage &im) {
    if (!pkt || bytes < kScanOff + 4 * kScanInts || (((uintptr_t)pkt) & 15) != 0) return false;
    const int32_t *hd = reinterpret_cast<const int32_t *>(pkt);
    if (hd[kHMagic] != kMagic) return false;
    if (!lemon_jpeg_par::packet_geometry(hd, rec_room, im)) return false;
    im.scans = hd[kHScans]; im.pool = hd[kHPool]; im.items = hd[kHItems]; im.levels = hd[kHLevels];
    if (im.scans < 1 || im.scans > 64 || im.pool < 0 || im.pool > 192 || im.levels < 1 || im.levels > im.scans || im.items < im.scans)
        return false;
    im.bytes = bytes; im.pool_off = hd[kHPoolOff]; im.data_off = hd[kHDataOff]; im.data_bytes = hd[kHDataBytes];
    if (im.pool_off != kScanOff + 4 * kScanInts * (int64_t)im.scans || im.pool_off + 4 * (int64_t)im.pool > bytes) return false;
    if (im.data_bytes < 0 || im.data_off < im.pool_off + 4 * (int64_t)im.pool || im.data_off > bytes || im.data_bytes > bytes - im.data_off)
        return false;
    im.pkt = pkt;
    return true;
}

// Row s (0 <= s < im.scans) of the scan table, every field checked: nothing of it is trusted.
LEMON_JPEG_HD bool prog_scan(const ProgImage &im, int s, ProgScan &sc) {
    const int32_t *r = reinterpret_cast<const int32_t *>(im.pkt + kScanOff) + kScanInts * s;
    sc.comp = r[kSComp]; sc.ss = r[kSSs]; sc.se = r[kSSe]; sc.ah = r[kSAh]; sc.al = r[kSAl]; sc.level = r[kSLevel];
    sc.restart = r[kSRestart]; sc.nivl = r[kSIntervals]; sc.t0 = r[kSTab0]; sc.t1 = r[kSTab1]; sc.t2 = r[kSTab2];
    if (sc.comp < -1 || sc.comp >= im.nc || (sc.comp < 0 && im.nc != 3)) return false;
    if (sc.ss < 0 || sc.se < sc.ss || sc.se > 63 || (sc.ss == 0 && sc.se != 0) || (sc.ss > 0 && sc.comp < 0)) return false;
    if (sc.al < 0 || sc.al > 13 || sc.ah < 0 || sc.ah > 14 || (sc.ah != 0 && sc.al != sc.ah - 1)) return false;
    if (sc.level < 0 || sc.level >= im.levels || sc.restart < 0 || sc.restart > 65535) return false;
    if (sc.comp < 0) {
        sc.bw = im.mx; sc.spm = im.spm; sc.mcus = im.mcus;
    } else {
        const int32_t cw = sc.comp == 0 || im.nc == 1 ? im.w : im.g.dwc, ch = sc.comp == 0 || im.nc == 1 ? im.h : im.g.dhc;
        sc.bw = (cw + 7) / 8; sc.spm = 1; sc.mcus = (int64_t)sc.bw * ((ch + 7) / 8);
    }
    const int64_t nivl = sc.restart ? (sc.mcus + sc.restart - 1) / sc.restart : 1;
    if (sc.nivl != nivl) return false;
    sc.items = (int32_t)((nivl + LEMON_JPEG_PROG_GROUP - 1) / LEMON_JPEG_PROG_GROUP);
    const int64_t off = r[kSData], nb = r[kSBytes], ends = r[kSEnds];
    if (off < 0 || nb < 0 || off > im.data_bytes || nb > im.data_bytes - off) return false;
    sc.bytes = nb; sc.data = im.pkt + im.data_off + off;
    sc.ends = nullptr;
    if (nivl > 1) {
        if (ends < im.pool_off || (ends & 3) != 0 || ends > im.bytes || 4 * nivl > im.bytes - ends) return false;
        sc.ends = reinterpret_cast<const uint32_t *>(im.pkt + ends);
    }
    const bool dc = sc.ss == 0;
    if (dc && sc.ah == 0) {
        if (sc.comp >= 0) { if (sc.t0 < 0 || sc.t0 >= im.pool) return false; }
        else if (sc.t0 < 0 || sc.t0 >= im.pool || sc.t1 < 0 || sc.t1 >= im.pool || sc.t2 < 0 || sc.t2 >= im.pool) return false;
    } else if (!dc && (sc.t0 < 0 || sc.t0 >= im.pool)) {
        return false;
    }
    return true;
}

// whether scans a and b write a common coefficient
LEMON_JPEG_HD bool prog_overlap(const ProgScan &a, const ProgScan &b) {
    return (a.comp < 0 || b.comp < 0 || a.comp == b.comp) && a.ss <= b.se && b.ss <= a.se;
}

// Pool entry idx (0 <= idx < im.pool) -> the table; false when the entry leaves the packet or describes no prefix code.
LEMON_JPEG_HD bool prog_build_huff(const ProgImage &im, int idx, ParHuff &h) {
    const int64_t off = reinterpret_cast<const uint32_t *>(im.pkt + im.pool_off)[idx];
    const bool inside = off >= im.pool_off && off <= im.bytes && 16 <= im.bytes - off;
    const uint8_t *spec = im.pkt + (inside ? off : 0);              // (outside: room -1 holds no table, and `h` is initialised)
    return lemon_jpeg::jpeg_build_huff(spec, spec + 16, inside ? im.bytes - off - 16 : -1, h);
}

// record block (planar, jpeg_entropy.hpp) of block q of the scan's own order
LEMON_JPEG_HD int64_t prog_block_addr(const ProgImage &im, const ProgScan &sc, int64_t q) {
    if (sc.comp >= 0) {
        const int64_t row = q / sc.bw, col = q - row * sc.bw;
        if (sc.comp == 0) return row * im.g.bw0 + col;
        return (sc.comp == 1 ? im.g.n0 : im.g.n0 + im.g.nc) + row * im.g.bwc + col;
    }
    const int64_t m = q / im.spm;
    return jpeg_mcu_block_addr(im.g, im.mx, im.hs, im.vs, im.luma, m, (int)(q - m * im.spm));
}

LEMON_JPEG_HD int prog_bit_at(const uint8_t *d, int64_t len, int64_t pos) {
    const int64_t at = pos >> 3;
    return at >= 0 && at < len ? (d[at] >> (7 - (int)(pos & 7))) & 1 : 0;
}

// what one lane does in an AC refinement step: lane j of the field F (the non-zero lanes passed) reads correction bit
// popcount(F below j) of the field that starts at bit `fb`
LEMON_JPEG_HD int16_t prog_refine_lane(int16_t c, int j, uint64_t F, int64_t fb, const uint8_t *d, int64_t len, int32_t p1) {
    if (!((F >> j) & 1)) return c;
    const int rank = __builtin_popcountll(F & (((uint64_t)1 << j) - 1));
    if (prog_bit_at(d, len, fb + rank) && (c & p1) == 0) return (int16_t)(c >= 0 ? c + p1 : c - p1);
    return c;
}

// The wave, with its lanes looped: lane k holds zig-zag coefficient k of the current block.  (jpeg_prog.hip has the device form.)
struct HostWave {
    int16_t c[64];
    inline void load(const int16_t *blk, const int16_t *) { for (int k = 0; k < 64; ++k) c[k] = blk[lemon_jpeg::kZigzag[k]]; }
    inline void clear() { for (int k = 0; k < 64; ++k) c[k] = 0; }
    inline uint64_t nonzero() const {
        uint64_t m = 0;
        for (int k = 0; k < 64; ++k) m |= (uint64_t)(c[k] != 0) << k;
        return m;
    }
    inline void set(int k, int32_t v) { c[k] = (int16_t)v; }
    inline void refine(uint64_t F, int64_t fb, const uint8_t *d, int64_t len, int32_t p1) {
        for (int k = 0; k < 64; ++k) c[k] = prog_refine_lane(c[k], k, F, fb, d, len, p1);
    }
    inline void store(int16_t *blk, uint64_t lanes) const {
        for (int k = 0; k < 64; ++k) if ((lanes >> k) & 1) blk[lemon_jpeg::kZigzag[k]] = c[k];
    }
    inline void store_dc(int16_t *blk, int32_t v) const { blk[0] = (int16_t)v; }
    inline void dc_refine(const ProgImage &im, const ProgScan &sc, int16_t *coef, int64_t q0, int64_t nblk, const uint8_t *d, int64_t len,
                          int32_t p1) const {
        for (int64_t i = 0; i < nblk; ++i)
            if (prog_bit_at(d, len, i)) coef[64 * prog_block_addr(im, sc, q0 + i)] |= (int16_t)p1;
    }
};

// The run of an EOBn symbol: 2^r blocks plus the r bits that follow its l-bit code in w.  Callers: prog_interval (AC first, AC
// refinement), lemon_jpeg_prog::seq_interval (jpeg_prog.hpp, the same two).
LEMON_JPEG_HD int32_t prog_eob_run(uint32_t w, int l, int r) { return (1 << r) + (r ? (int32_t)((w << l) >> (32 - r)) : 0); }

// the interval ends inside its last byte
LEMON_JPEG_HD int prog_interval_end(int64_t total_bits, int64_t bit) {
    const int64_t left = total_bits - bit;
    return left >= 0 && left < 8 ? LEMON_JPEG_OK : LEMON_JPEG_STREAM;
}

// One restart interval of a scan: the blocks q0 .. q0 + nblk - 1 of the scan's order from the bytes d[0, len).  huff: the
// scan's tables (DC first: by component, or [0] for a single-component scan; AC: [0]).  Returns the first error.
template <class Wave>
LEMON_JPEG_HD int prog_interval(const ProgImage &im, const ProgScan &sc, const ParHuff *huff, const uint8_t *d, int64_t len, int64_t q0,
                                int64_t nblk, int16_t *coef, Wave &wv) {
    const int64_t total = len * 8;
    const int32_t p1 = 1 << sc.al;
    ParBits bits = {d, len, -1, 0};
    int64_t bit = 0;
    if (sc.ss == 0 && sc.ah != 0) {                                  // ---- DC refinement: one bit per block
        if (nblk > total) return LEMON_JPEG_STREAM;
        wv.dc_refine(im, sc, coef, q0, nblk, d, len, p1);
        return prog_interval_end(total, nblk);
    }
    if (sc.ss == 0) {                                                // ---- DC first
        int32_t pred0 = 0, pred1 = 0, pred2 = 0;
        for (int64_t b = 0; b < nblk; ++b) {
            int c = 0;
            if (sc.comp < 0) {
                const int slot = (int)((q0 + b) % im.spm);
                c = slot < im.luma ? 0 : slot - im.luma + 1;
            }
            const uint32_t w = par_peek32(bits, bit);
            const int32_t e = par_symbol(w, huff[c]);
            const int l = e >> 8, s = e & 255;
            if (e < 0 || s > 11) return LEMON_JPEG_CODE;
            bit += l + s;
            if (bit > total) return LEMON_JPEG_STREAM;
            const int32_t diff = s ? par_extend(w, l, s) : 0;
            int32_t pred = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + diff;
            if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
            if (pred < -32768 || pred > 32767) return LEMON_JPEG_CODE;
            const int32_t v = pred * p1;
            if (v < -32768 || v > 32767) return LEMON_JPEG_CODE;
            wv.store_dc(coef + 64 * prog_block_addr(im, sc, q0 + b), v);
        }
        return prog_interval_end(total, bit);
    }
    const ParHuff &hf = huff[0];
    int32_t eobrun = 0;
    if (sc.ah == 0) {                                                // ---- AC first
        for (int64_t b = 0; b < nblk; ++b) {
            if (eobrun > 0) { --eobrun; continue; }
            uint64_t put = 0;
            wv.clear();
            for (int k = sc.ss; k <= sc.se;) {
                const uint32_t w = par_peek32(bits, bit);
                const int32_t e = par_symbol(w, hf);
                if (e < 0) return LEMON_JPEG_CODE;
                const int l = e >> 8, r = (e >> 4) & 15, s = e & 15;
                if (s) {
                    k += r;
                    if (k > sc.se) return LEMON_JPEG_CODE;
                    bit += l + s;
                    if (bit > total) return LEMON_JPEG_STREAM;
                    const int32_t v = par_extend(w, l, s) * p1;
                    if (v < -32768 || v > 32767) return LEMON_JPEG_CODE;
                    wv.set(k, v);
                    put |= (uint64_t)1 << k;
                    ++k;
                } else if (r == 15) {
                    k += 16;
                    if (k > sc.se + 1) return LEMON_JPEG_CODE;
                    bit += l;
                    if (bit > total) return LEMON_JPEG_STREAM;
                } else {
                    eobrun = prog_eob_run(w, l, r);
                    bit += l + r;
                    if (bit > total || eobrun > nblk - b) return LEMON_JPEG_STREAM;
                    --eobrun;
                    break;
                }
            }
            if (put) wv.store(coef + 64 * prog_block_addr(im, sc, q0 + b), put);
        }
        return prog_interval_end(total, bit);
    }
    const uint64_t band = prog_range(sc.ss, sc.se + 1);               // ---- AC refinement
    for (int64_t b = 0; b < nblk; ++b) {
        int16_t *blk = coef + 64 * prog_block_addr(im, sc, q0 + b);
        wv.load(blk, b + 1 < nblk ? coef + 64 * prog_block_addr(im, sc, q0 + b + 1) : nullptr);
        const uint64_t H = wv.nonzero() & band;
        uint64_t dirty = 0;
        int k = sc.ss;
        if (eobrun == 0) {
            while (k <= sc.se) {
                const uint32_t w = par_peek32(bits, bit);
                const int32_t e = par_symbol(w, hf);
                if (e < 0) return LEMON_JPEG_CODE;
                const int l = e >> 8, r = (e >> 4) & 15, s = e & 15;
                int32_t val = 0;
                if (s) {
                    if (s != 1) return LEMON_JPEG_CODE;
                    val = ((w << l) >> 31) ? p1 : -p1;
                    bit += l + 1;
                } else if (r != 15) {
                    eobrun = prog_eob_run(w, l, r);
                    bit += l + r;
                    if (bit > total || eobrun > nblk - b) return LEMON_JPEG_STREAM;
                    break;
                } else {
                    bit += l;
                }
                if (bit > total) return LEMON_JPEG_STREAM;
                uint64_t Z = ~H & prog_range(k, sc.se + 1);          // the (r+1)-th clear lane at or after k
                for (int i = 0; i < r; ++i) Z &= Z - 1;
                const int target = Z ? __builtin_ctzll(Z) : sc.se + 1;
                const uint64_t F = H & prog_range(k, target);
                const int nf = __builtin_popcountll(F);
                if (bit + nf > total) return LEMON_JPEG_STREAM;
                if (!Z) return LEMON_JPEG_CODE;                      // the band ends before the target
                if (F) wv.refine(F, bit, d, len, p1);
                bit += nf;
                if (s) { wv.set(target, val); dirty |= (uint64_t)1 << target; }
                dirty |= F;
                k = target + 1;
            }
        }
        if (eobrun > 0) {
            const uint64_t F = H & prog_range(k, sc.se + 1);
            const int nf = __builtin_popcountll(F);
            if (bit + nf > total) return LEMON_JPEG_STREAM;
            if (F) wv.refine(F, bit, d, len, p1);
            bit += nf;
            dirty |= F;
            --eobrun;
        }
        if (dirty) wv.store(blk, dirty);
    }
    return prog_interval_end(total, bit);
}

// One work item: intervals group * LEMON_JPEG_PROG_GROUP .. of the scan, until the first error.
template <class Wave>
LEMON_JPEG_HD int prog_item(const ProgImage &im, const ProgScan &sc, const ParHuff *huff, int32_t group, int16_t *coef, Wave &wv) {
    const int64_t t0 = (int64_t)group * LEMON_JPEG_PROG_GROUP;
    for (int64_t t = t0; t < t0 + LEMON_JPEG_PROG_GROUP && t < sc.nivl; ++t) {
        const int64_t lo = t ? sc.ends[t - 1] : 0, hi = sc.nivl > 1 ? (int64_t)sc.ends[t] : sc.bytes;
        if (lo > hi || hi > sc.bytes || (t + 1 == sc.nivl && hi != sc.bytes)) return LEMON_JPEG_STREAM;
        const lemon_jpeg_par::McuRange r = lemon_jpeg_par::interval_mcus(sc.restart, sc.mcus, t);
        const int rc = prog_interval(im, sc, huff, sc.data + lo, hi - lo, r.first * sc.spm, r.count * sc.spm, coef, wv);
        if (rc != LEMON_JPEG_OK) return rc;
    }
    return LEMON_JPEG_OK;
}

// the tables of a scan into huff[0..2]; false when one is no table
LEMON_JPEG_HD bool prog_scan_tables(const ProgImage &im, const ProgScan &sc, ParHuff *huff) {
    if (sc.ss == 0 && sc.ah != 0) return true;
    bool ok = prog_build_huff(im, sc.t0, huff[0]);
    if (sc.ss == 0 && sc.comp < 0) {
        ok = prog_build_huff(im, sc.t1, huff[1]) && ok;
        ok = prog_build_huff(im, sc.t2, huff[2]) && ok;
    }
    return ok;
}

// The plan's checks of scan row s: the row itself and its level (recomputed).  Returns the row's items, -1 when it is refused.
LEMON_JPEG_HD int32_t prog_plan_row(const ProgImage &im, int s) {
    ProgScan a, b;
    if (!prog_scan(im, s, a)) return -1;
    int lvl = 0;
    for (int e = 0; e < s; ++e) {
        if (!prog_scan(im, e, b)) return -1;
        if (prog_overlap(a, b) && b.level + 1 > lvl) lvl = b.level + 1;
    }
    return lvl == a.level ? a.items : -1;
}

// the whole-packet checks: every row, and the item count of the head
static inline bool prog_plan(const ProgImage &im) {
    int64_t items = 0;
    for (int s = 0; s < im.scans; ++s) {
        const int32_t n = prog_plan_row(im, s);
        if (n < 0) return false;
        items += n;
    }
    return items == im.items;
}

}  // namespace lemon_jpeg_prog

// The kernels' algorithm with the waves looped: the same items, level by level, the same step functions, the same verdict.
static inline int lemon_jpeg_prog_entropy_par_host_impl(const uint8_t *packet, int64_t bytes, uint8_t *record, int64_t record_cap,
                                                        int32_t *status) {
    using namespace lemon_jpeg_prog;
    if (!status) return 1;
    *status = LEMON_JPEG_BUFFER;
    ProgImage im;
    if (!record || !prog_open(packet, bytes, record_cap, im) || !prog_plan(im)) return 0;
    int16_t *coef = lemon_jpeg_par::par_new_record(record, packet, im.g);
    ParHuff *huff = new ParHuff[3];
    HostWave wv;
    int st = LEMON_JPEG_OK;
    for (int level = 0; level < im.levels && st == LEMON_JPEG_OK; ++level)
        for (int s = 0; s < im.scans; ++s) {
            ProgScan sc;
            prog_scan(im, s, sc);
            if (sc.level != level) continue;
            const bool tables = prog_scan_tables(im, sc, huff);
            for (int32_t g = 0; g < sc.items; ++g) {
                const int rc = tables ? prog_item(im, sc, huff, g, coef, wv) : (int)LEMON_JPEG_TABLE;
                if (rc > st) st = rc;
            }
        }
    delete[] huff;
    if (st == LEMON_JPEG_OK && !lemon_jpeg_par::par_envelope_blocks(record, im.g, 0, 1)) st = LEMON_JPEG_ENVELOPE;
    *status = st;
    return 0;
}
