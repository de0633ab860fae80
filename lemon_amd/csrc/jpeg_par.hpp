// jpeg_par.hpp -- the parallel form of the JPEG Huffman pass: the scan packet a decode worker writes (lemon_jpeg_pack) and the
// per-symbol decode step that the device kernels (jpeg_entropy.hip) and the host loop (lemon_jpeg_entropy_par_host) share.
// `LEMON_JPEG_HD` functions compile for both; the host loop below runs the lanes one after another with the same workgroup
// and round structure as the kernels, so both give the same record AND the same status.  Plain C++17, no HIP needed.
// Also here, for the progressive path too (jpeg_prog.hpp, jpeg_prog_par.hpp, jpeg_prog.hip): the scan walker of both packers
// (walk_scan), the geometry both packets open with (packet_geometry), interval_mcus, the envelope loop and the record
// initialisation of both passes.  The Huffman table builder is jpeg_entropy.hpp's (jpeg_build_huff), the parsers' own.
//
// Packet (little endian, every section at a multiple of 16, the whole a multiple of 16 bytes):
//   int32  head[32]          kPk* indices below: magic, geometry, restart interval, interval count, scan bytes, section offsets,
//                            the components' DC / AC table selectors
//   uint16 quant[3][64]      per component, natural order (at byte 128)
//   uint8  huff[8][272]      DC tables 0..3 then AC tables 0..3 as in the file: 16 counts, 256 values (unused: zeros) (at 512)
//   uint16 len16[nivl]       (only when nivl > 1) destuffed bytes of every restart interval; 0xFFFF = look it up in `big`
//   uint8  scan[scan_bytes]  the entropy-coded segment, FF 00 -> FF, restart markers and fill bytes removed, intervals back to back
//   uint32 big[nbig][2]      (interval index, bytes) of the intervals of 65535 bytes or more, ascending
// Capacity: n + LEMON_JPEG_PACKET_BOUND bytes hold the packet of every n-byte file whose restart intervals are shorter than
// 65535 bytes (every file without restart markers included: one interval, no table); a longer interval of a file WITH restart
// markers costs 6 bytes more, at most n / 8192 in all.  lemon_jpeg_pack declines with LEMON_JPEG_BUFFER rather than overrun.
//
// Parallel decode.  Every restart interval is cut into lanes of `subseq` bytes.  A lane's state is (bit position in its interval,
// block slot within the MCU, zig-zag index; index 0 = the DC symbol comes next), packed into 64 bits.  A lane decodes the symbols
// that START inside its bytes and hands its exit state to the lane on its right.  Lanes are grouped in workgroups of 256:
//   round 0      every lane decodes from a guess (its first bit, slot 0, index 0); then, inside the workgroup, a lane whose left
//                neighbour's exit differs from the entry it used decodes again, until nothing changes (at most 256 times: the
//                first lane of an interval starts from the truth and every iteration settles one more lane)
//   round 1..R-1 the first lane of a workgroup takes the previous workgroup's last exit of the round before (double-buffered, so
//                the outcome does not depend on the order workgroups run in), and the change ripples as far as it goes
//   final        a lane whose stored entry is not its left neighbour's stored exit reports LEMON_JPEG_SYNC: the rounds ended
//                before the states had settled.  When no lane reports that, every stored (entry, exit, block count) comes from
//                one decode that started where the lane on the left stopped, so by induction from lane 0 they are the
//                sequential decoder's -- the states AND the block counts, hence every lane's first block.  (Comparing exits
//                alone is not enough: two entries can reach the same exit inside one lane after a different number of
//                blocks.)  Every lane then decodes once more from that entry, writing coefficients (DC as differences), and
//                the errors it raises are real.  The status of an image is the largest code any lane or block raised.
// Then the DC differences are summed per component inside each interval (64-bit), and every block gets decode_scan's checks.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jpeg_entropy.hpp"

// (include/lemon_hip.h: LEMON_JPEG_SYNC, LEMON_JPEG_PACKET_BOUND = header 128 + quantisers 384 + tables 2176 + section padding,
// LEMON_JPEG_SUBSEQ_MIN = 16: a lane holds the longest symbol, a 16-bit code + 11 bits, with room; LEMON_JPEG_PAR_GROUP)
#define LEMON_JPEG_SUBSEQ_MAX 4096
#define LEMON_JPEG_SUBSEQ_DEFAULT 256          // measured: tools/jpeg_entropy_time.py, DESIGN.md section 5
#define LEMON_JPEG_PAR_ROUNDS 3            // rounds before the final pass

namespace lemon_jpeg_par {

enum { kPkMagic = 0, kPkWidth, kPkHeight, kPkComponents, kPkHs, kPkVs, kPkRestart, kPkIntervals, kPkScanBytes, kPkLenOff,
       kPkScanOff, kPkBigOff, kPkBig, kPkTotal, kPkTd0, kPkTa0 = kPkTd0 + 3, kPkHeadInts = 32 };
static const int32_t kMagic = 0x31504A4C;          // "LJP1"
static const int32_t kQuantOff = 128, kHuffOff = 512, kHuffSpec = 272, kLenOff = 2688;

// ------------------------------------------------------------------------------------------------ packet writer (host)
static inline void huff_spec(const lemon_jpeg::Huff &h, uint8_t *spec) {
    memset(spec, 0, kHuffSpec);
    if (!h.defined) return;
    int32_t k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t c = h.maxcode[l] >= 0 ? h.maxcode[l] - (k - h.valptr[l]) + 1 : 0;
        spec[l - 1] = (uint8_t)c;
        k += c;
    }
    if (k > 256) k = 256;
    memcpy(spec + 16, h.vals, (size_t)k);
}

// The ONE walk over the entropy-coded bytes of a scan, from d[p] to the marker that ends it (p is left at that marker's FF, fill
// bytes skipped; the caller decides which marker it accepts).  It destuffs FF 00, sequences RSTn modulo 8 over `nivl` intervals
// and declines (LEMON_JPEG_STREAM) an empty interval, a fill byte before data, a wrong or surplus RSTn, and an end before the
// last interval.  COPY writes the destuffed bytes to out[0, cap) (LEMON_JPEG_BUFFER when they do not fit); with several
// intervals on_end(ivl, o) receives the destuffed offset o at which interval ivl ends.  Callers: pack below (baseline: one
// scan, must end at EOI), lemon_jpeg_prog::parse (COPY = false: sizes only) and lemon_jpeg_prog::pack (jpeg_prog.hpp).
template <bool COPY, class OnEnd>
static inline int walk_scan(const uint8_t *d, size_t n, size_t &p, int32_t restart, int64_t nivl, uint8_t *out, int64_t cap, OnEnd on_end,
                            int64_t &bytes) {
    int64_t o = 0, ivl = 0, start = 0;
    bool fill = false;
    for (;;) {
        if (p >= n) return LEMON_JPEG_STREAM;
        if (d[p] != 0xFF) {                                          // the run of plain bytes up to the next FF, at once
            if (fill) return LEMON_JPEG_STREAM;
            const void *ff = memchr(d + p, 0xFF, n - p);
            const int64_t run = ff ? (int64_t)(static_cast<const uint8_t *>(ff) - (d + p)) : (int64_t)(n - p);
            if (COPY) {
                if (run > cap - o) return LEMON_JPEG_BUFFER;
                memcpy(out + o, d + p, (size_t)run);
            }
            o += run; p += (size_t)run;
            continue;
        }
        if (p + 1 >= n) return LEMON_JPEG_STREAM;
        const uint8_t m = d[p + 1];
        if (m == 0xFF) { fill = true; ++p; continue; }               // a fill byte: only a marker may follow
        if (m == 0) {
            if (fill) return LEMON_JPEG_STREAM;
            if (COPY) {
                if (o >= cap) return LEMON_JPEG_BUFFER;
                out[o] = 0xFF;
            }
            ++o; p += 2;
            continue;
        }
        if (o == start) return LEMON_JPEG_STREAM;                    // an interval without a byte
        const bool rst = m >= 0xD0 && m <= 0xD7;
        if (rst ? (!restart || ivl + 1 >= nivl || m != (uint8_t)(0xD0 + (ivl & 7))) : ivl != nivl - 1) return LEMON_JPEG_STREAM;
        if (nivl > 1) on_end(ivl, o);
        if (!rst) { bytes = o; return LEMON_JPEG_OK; }
        ++ivl; start = o; p += 2; fill = false;
    }
}

static inline int pack(const uint8_t *d, size_t n, uint8_t *pkt, int64_t cap, LemonJpegInfo *info, int64_t *packet_bytes,
                       lemon_jpeg::BaseFile &bf) {
    using namespace lemon_jpeg;
    const Frame &f = bf.f;
    int rc = parse_header(d, n, bf, info);
    if (rc != LEMON_JPEG_OK) return rc;
    if (!pkt || n >= ((size_t)1 << 31)) return LEMON_JPEG_BUFFER;
    const int64_t mcus = (int64_t)info->mcus_x * info->mcus_y;
    const int64_t nivl = f.restart ? (mcus + f.restart - 1) / f.restart : 1;
    const int64_t scan_off = kLenOff + (nivl > 1 ? ((2 * nivl + 15) & ~(int64_t)15) : 0);
    if (scan_off > cap) return nivl * 3 > (int64_t)n ? LEMON_JPEG_STREAM : LEMON_JPEG_BUFFER;   // (more intervals than bytes)
    memset(pkt, 0, (size_t)scan_off);
    uint16_t *len16 = reinterpret_cast<uint16_t *>(pkt + kLenOff);
    // the intervals of 65535 bytes or more are appended after the scan (8 bytes each, found at most once per 64 KB of input)
    std::vector<uint32_t> big;
    size_t p = f.scan;
    int64_t scan_bytes = 0, start = 0;
    rc = walk_scan<true>(d, n, p, f.restart, nivl, pkt + scan_off, cap - scan_off, [&](int64_t ivl, int64_t o) {
        const int64_t len = o - start;
        start = o;
        len16[ivl] = (uint16_t)(len < 0xFFFF ? len : 0xFFFF);
        if (len >= 0xFFFF) { big.push_back((uint32_t)ivl); big.push_back((uint32_t)len); }
    }, scan_bytes);
    if (rc != LEMON_JPEG_OK) return rc;
    if (d[p + 1] != 0xD9) return LEMON_JPEG_STREAM;                  // one scan: nothing but EOI may end it
    const int64_t nbig = (int64_t)big.size() / 2, o = scan_off + scan_bytes;
    const int64_t big_off = (o + 15) & ~(int64_t)15;
    const int64_t total = (big_off + 8 * nbig + 15) & ~(int64_t)15;
    if (total > cap) return LEMON_JPEG_BUFFER;
    memset(pkt + o, 0, (size_t)(total - o));
    if (nbig) memcpy(pkt + big_off, big.data(), (size_t)nbig * 8);
    int32_t head[kPkHeadInts];
    memset(head, 0, sizeof(head));
    head[kPkMagic] = kMagic; head[kPkWidth] = info->width; head[kPkHeight] = info->height;
    head[kPkComponents] = info->components; head[kPkHs] = info->hs; head[kPkVs] = info->vs; head[kPkRestart] = f.restart;
    head[kPkIntervals] = (int32_t)nivl; head[kPkScanBytes] = (int32_t)scan_bytes; head[kPkLenOff] = kLenOff;
    head[kPkScanOff] = (int32_t)scan_off; head[kPkBigOff] = (int32_t)big_off; head[kPkBig] = (int32_t)nbig;
    head[kPkTotal] = (int32_t)total;
    for (int c = 0; c < info->components; ++c) { head[kPkTd0 + c] = f.td[c]; head[kPkTa0 + c] = f.ta[c]; }
    memcpy(pkt, head, sizeof(head));
    memcpy(pkt + kQuantOff, info->quant, LEMON_JPEG_QUANT_BYTES);
    for (int s = 0; s < 4; ++s) {
        huff_spec(bf.dc[s], pkt + kHuffOff + s * kHuffSpec);
        huff_spec(bf.ac[s], pkt + kHuffOff + (4 + s) * kHuffSpec);
    }
    if (packet_bytes) *packet_bytes = total;
    return LEMON_JPEG_OK;
}

// ------------------------------------------------------------------------------------------- shared decode step (host + device)
using lemon_jpeg::ParHuff;

// spec: 16 counts, 256 values (a specification of the packet)
LEMON_JPEG_HD bool par_build_huff(const uint8_t *spec, ParHuff &h) { return lemon_jpeg::jpeg_build_huff(spec, spec + 16, 256, h); }

// 32 bits of the interval d[0, len) from bit position `bit` on, MSB first; zeros past the end.  A window of 8 bytes is kept and
// reloaded (one 8-byte load while 8 bytes remain, else byte by byte) when `bit` leaves its first 32 bits.
struct ParBits {
    const uint8_t *d;
    int64_t len;
    int64_t base;                     // bit position of the window's first bit (a multiple of 8); < 0: nothing loaded
    uint64_t acc;
};

LEMON_JPEG_HD uint32_t par_peek32(ParBits &b, int64_t bit) {
    if (b.base < 0 || bit < b.base || bit - b.base > 32) {
        const int64_t at = bit >> 3;
        uint64_t v = 0;
        if (at >= 0 && at + 8 <= b.len) {
            uint8_t raw[8];
            memcpy(raw, b.d + at, 8);
            for (int i = 0; i < 8; ++i) v = (v << 8) | raw[i];
        } else {
            for (int i = 0; i < 8; ++i) v = (v << 8) | (uint64_t)(at + i >= 0 && at + i < b.len ? b.d[at + i] : 0);
        }
        b.acc = v;
        b.base = at * 8;
    }
    return (uint32_t)((b.acc << (bit - b.base)) >> 32);
}

// one Huffman symbol from the top 16 bits of w: (length << 8 | value), or -1 when they are no code of the table
LEMON_JPEG_HD int32_t par_symbol(uint32_t w, const ParHuff &h) {
    const uint32_t x = w >> 16;
    const uint32_t e = h.look[x >> 7];
    if (e) return (int32_t)e;
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)(x >> (16 - l));
        if (code <= h.maxcode[l]) {
            const int32_t idx = h.valptr[l] + code;
            if (idx < 0 || idx > 255) return -1;
            return (l << 8) | h.vals[idx];
        }
    }
    return -1;
}

LEMON_JPEG_HD int32_t par_extend(uint32_t w, int l, int s) {         // s >= 1 magnitude bits after an l-bit code
    const int32_t v = (int32_t)((w << l) >> (32 - s));
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The geometry both packet formats open with: head ints 1..5 are width, height, components, hs, vs (int 0 is the magic).
struct PacketGeom {
    int32_t w, h, nc, hs, vs;
    int32_t spm, luma;                // blocks per interleaved MCU, of which luma
    int32_t mx, my;                   // the MCU grid
    int64_t mcus;
    JpegGeom g;
};

// false when the head describes no accepted geometry or the record it needs exceeds `rec_room`.  Callers: par_open below,
// lemon_jpeg_prog::prog_open (jpeg_prog_par.hpp).
LEMON_JPEG_HD bool packet_geometry(const int32_t *hd, int64_t rec_room, PacketGeom &im) {
    im.w = hd[1]; im.h = hd[2]; im.nc = hd[3]; im.hs = hd[4]; im.vs = hd[5];
    if (!jpeg_geometry(im.w, im.h, im.nc, im.hs, im.vs, im.g)) return false;
    if (rec_room < LEMON_JPEG_QUANT_BYTES + 128 * im.g.blocks) return false;
    im.luma = im.nc == 3 ? im.hs * im.vs : 1;
    im.spm = im.nc == 3 ? im.luma + 2 : 1;
    im.mx = im.nc == 3 ? im.g.bwc : im.g.bw0; im.my = im.nc == 3 ? im.g.bhc : im.g.bh0;
    im.mcus = (int64_t)im.mx * im.my;
    return true;
}

// Restart interval t of a scan of `mcus` MCUs -> its first MCU and its MCU count (restart 0: one interval).  Callers: the lanes
// of lemon_jpeg_entropy_par_host_impl and jent_lane (jpeg_entropy.hip), prog_item (jpeg_prog_par.hpp), seq_decode (jpeg_prog.hpp).
struct McuRange { int64_t first, count; };
LEMON_JPEG_HD McuRange interval_mcus(int32_t restart, int64_t mcus, int64_t t) {
    const int64_t mcu0 = restart ? t * restart : 0;
    return {mcu0, restart && mcus - mcu0 > restart ? restart : mcus - mcu0};
}

struct ParImage : PacketGeom {        // a validated packet
    int32_t restart, nivl, nbig;
    int64_t scan_bytes;
    const uint8_t *pkt, *scan;
    const uint16_t *len16;
    const uint32_t *big;
    int32_t tables;                   // table selectors, two bits each: DC of components 0..2, then AC (a packed word, not arrays:
                                      // a struct without indexed members stays in registers on the device)
};

// Reads the header of the packet in pkt[0, bytes) and checks every section against `bytes`, and the record the image needs
// against `rec_room`.  Nothing of the packet is trusted: the sizes come from the host, the contents from a file.
LEMON_JPEG_HD bool par_open(const uint8_t *pkt, int64_t bytes, int64_t rec_room, ParImage &im) {
    if (!pkt || bytes < kLenOff || (((uintptr_t)pkt) & 15) != 0) return false;
    const int32_t *hd = reinterpret_cast<const int32_t *>(pkt);
    if (hd[kPkMagic] != kMagic) return false;
    if (!packet_geometry(hd, rec_room, im)) return false;
    im.restart = hd[kPkRestart]; im.nivl = hd[kPkIntervals]; im.nbig = hd[kPkBig]; im.scan_bytes = hd[kPkScanBytes];
    if (im.restart < 0 || im.restart > 65535) return false;
    const int64_t nivl = im.restart ? (im.mcus + im.restart - 1) / im.restart : 1;
    if (im.nivl != nivl || im.scan_bytes < 0 || im.nbig < 0 || im.nbig > im.nivl) return false;
    const int64_t len_off = hd[kPkLenOff], scan_off = hd[kPkScanOff], big_off = hd[kPkBigOff];
    if (len_off != kLenOff || scan_off < len_off + (nivl > 1 ? 2 * nivl : 0) || scan_off > bytes || im.scan_bytes > bytes - scan_off)
        return false;
    if (big_off < scan_off + im.scan_bytes || (big_off & 3) != 0 || big_off > bytes || 8 * (int64_t)im.nbig > bytes - big_off) return false;
    im.tables = 0;
    for (int c = 0; c < 3; ++c) {
        const int32_t td = hd[kPkTd0 + c], ta = hd[kPkTa0 + c];
        if (td < 0 || td > 3 || ta < 0 || ta > 3) return false;
        im.tables |= (td << (2 * c)) | (ta << (6 + 2 * c));
    }
    im.pkt = pkt; im.scan = pkt + scan_off;
    im.len16 = reinterpret_cast<const uint16_t *>(pkt + len_off);
    im.big = reinterpret_cast<const uint32_t *>(pkt + big_off);
    return true;
}

// the table specification (16 counts, 256 values) component c decodes its DC (ac = 0) or AC (ac = 1) symbols with
LEMON_JPEG_HD const uint8_t *par_spec(const ParImage &im, int c, int ac) {
    return im.pkt + kHuffOff + (4 * ac + ((im.tables >> (6 * ac + 2 * c)) & 3)) * kHuffSpec;
}

// destuffed bytes of interval t
LEMON_JPEG_HD int64_t par_interval_bytes(const ParImage &im, int64_t t) {
    if (im.nivl == 1) return im.scan_bytes;
    const uint32_t e = im.len16[t];
    if (e != 0xFFFF) return e;
    int32_t lo = 0, hi = im.nbig;                            // first entry with index >= t
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if ((int64_t)im.big[2 * mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo < im.nbig && (int64_t)im.big[2 * lo] == t ? (int64_t)im.big[2 * lo + 1] : 0xFFFF;
}

LEMON_JPEG_HD int64_t par_lanes_of(int64_t bytes, int32_t subseq) { return bytes > 0 ? (bytes + subseq - 1) / subseq : 1; }

LEMON_JPEG_HD int par_comp_of_slot(const ParImage &im, int slot) { return slot < im.luma ? 0 : slot - im.luma + 1; }

// record block (planar, jpeg_entropy.hpp) of block b of the scan order, counted from MCU mcu0
LEMON_JPEG_HD int64_t par_block_addr(const ParImage &im, int64_t mcu0, int64_t b) {
    return jpeg_mcu_block_addr(im.g, im.mx, im.hs, im.vs, im.luma, mcu0 + b / im.spm, (int)(b % im.spm));
}

// record block of block q of component c in scan order, and whether a restart interval begins with it
LEMON_JPEG_HD int64_t par_comp_block_addr(const ParImage &im, int c, int64_t q, bool &head) {
    const int per = c == 0 ? im.luma : 1;
    const int64_t m = q / per;
    const int sub = (int)(q - m * per);
    head = sub == 0 && (im.restart ? m % im.restart == 0 : m == 0);
    return par_block_addr(im, m, c == 0 ? sub : im.luma + c - 1);
}

LEMON_JPEG_HD uint64_t par_state(int64_t bit, int slot, int k) { return ((uint64_t)bit << 16) | ((uint64_t)slot << 8) | (uint64_t)k; }

struct ParLane {                      // one lane's share of its interval
    const uint8_t *d;                 // the interval's bytes
    int64_t len;                      // of the interval
    int64_t end_bit;                  // of the lane
    int64_t mcu0, total;              // first MCU and block count of the interval
    uint64_t guess;                   // the lane's first bit, slot 0, DC next; the truth for the first lane of an interval
    bool first, last;                 // of its interval
};

// Decodes the symbols that start before lane.end_bit, from `state` on.  `cnt` counts the blocks completed.
// FINAL = false (speculation): what is no valid symbol costs one bit and the block starts over; nothing is written or raised.
// FINAL = true: coefficients go to `coef` (the record's blocks; DC as the decoded difference) from block `blk` of the interval
// on, the lane stops after block lane.total - 1 (`done`), and the return value is a LemonJpegStatus.
template <bool FINAL>
LEMON_JPEG_HD int par_run(const ParHuff *huff, const ParImage &im, const ParLane &lane, uint64_t &state, int64_t &cnt, int16_t *coef,
                          int64_t blk, bool &done) {
    int64_t bit = (int64_t)(state >> 16);
    int slot = (int)((state >> 8) & 255), k = (int)(state & 255);
    const int64_t total_bits = lane.len * 8;
    done = false;
    if (slot >= im.spm || k > 63 || bit < 0) { slot = 0; k = 0; }
    int16_t *cur = nullptr;
    if (FINAL) cur = coef + 64 * par_block_addr(im, lane.mcu0, blk);
    int64_t guard = lane.end_bit - bit;                     // every step consumes at least one bit
    ParBits bits = {lane.d, lane.len, -1, 0};
    while (bit < lane.end_bit && guard-- > 0) {
        const uint32_t w = par_peek32(bits, bit);
        const int c = par_comp_of_slot(im, slot);
        bool block_done = false;
        int nbits = 0;
        bool bad = false;
        if (k == 0) {
            const int32_t e = par_symbol(w, huff[c]);
            const int l = e >> 8, s = e & 255;
            if (e < 0 || s > 11) bad = true;
            else {
                nbits = l + s;
                if (FINAL) {
                    if (bit + nbits > total_bits) return LEMON_JPEG_STREAM;
                    cur[0] = (int16_t)(s ? par_extend(w, l, s) : 0);
                }
                k = 1;
            }
        } else {
            const int32_t e = par_symbol(w, huff[3 + c]);
            const int l = e >> 8, r = (e >> 4) & 15, s = e & 15;
            if (e < 0) bad = true;
            else if (s == 0) {
                if (r == 15) { k += 16; if (k > 64) bad = true; else { nbits = l; block_done = k == 64; } }
                else if (r != 0) bad = true;
                else { nbits = l; block_done = true; }
            } else {
                k += r;
                if (k > 63 || s > 10) bad = true;
                else {
                    nbits = l + s;
                    if (FINAL) {
                        if (bit + nbits > total_bits) return LEMON_JPEG_STREAM;
                        cur[lemon_jpeg::kZigzag[k]] = (int16_t)par_extend(w, l, s);
                    }
                    ++k;
                    block_done = k == 64;
                }
            }
        }
        if (bad) {
            if (FINAL) return LEMON_JPEG_CODE;
            bit += 1; k = 0;
            continue;
        }
        if (FINAL && bit + nbits > total_bits) return LEMON_JPEG_STREAM;
        bit += nbits;
        if (block_done) {
            ++cnt; ++blk; k = 0;
            slot = slot + 1 == im.spm ? 0 : slot + 1;
            if (FINAL) {
                if (blk >= lane.total) { done = true; break; }
                cur = coef + 64 * par_block_addr(im, lane.mcu0, blk);
            }
        }
    }
    state = par_state(bit, slot, k);
    return LEMON_JPEG_OK;
}

// The final pass of one lane: `entry` its left neighbour's stored exit (or the truth), `stored_entry` / `stored_exit` / the
// stored block count what the lane's last decode of the rounds started from and gave, `blk` the blocks of the interval decoded
// before it (summed from the stored counts).  Returns the status this lane raises (0: none).
LEMON_JPEG_HD int par_final_lane(const ParHuff *huff, const ParImage &im, const ParLane &lane, uint64_t entry, uint64_t stored_entry,
                                 uint64_t stored_exit, int64_t blk, int16_t *coef) {
    if (entry != stored_entry) return LEMON_JPEG_SYNC;               // the stored exit and block count belong to another entry
    if (blk < 0 || blk >= lane.total) return LEMON_JPEG_OK;          // (the lane that completed the interval has judged it)
    uint64_t st = entry;
    int64_t cnt = 0;
    bool done;
    const int rc = par_run<true>(huff, im, lane, st, cnt, coef, blk, done);
    if (rc != LEMON_JPEG_OK) return rc;
    if (done) {
        const int64_t left = lane.len * 8 - (int64_t)(st >> 16);     // the interval ends inside its last byte
        return left >= 0 && left < 8 ? LEMON_JPEG_OK : LEMON_JPEG_STREAM;
    }
    if (lane.last) return LEMON_JPEG_STREAM;                         // the bytes end before the interval's MCUs do
    return st == stored_exit ? LEMON_JPEG_OK : LEMON_JPEG_SYNC;
}

// decode_scan's envelope check on the finished blocks first, first + stride, ... of a record (quantisers at its head, DC
// values summed): false when one lies outside.  Callers: both host loops (every block: 0, 1) and, one thread each with a grid
// stride, k_jent_check (jpeg_entropy.hip) and k_jprog_check (jpeg_prog.hip).
LEMON_JPEG_HD bool par_envelope_blocks(const uint8_t *rec, const JpegGeom &g, int64_t first, int64_t stride) {
    const uint16_t *quant = reinterpret_cast<const uint16_t *>(rec);
    const int16_t *coef = reinterpret_cast<const int16_t *>(rec + LEMON_JPEG_QUANT_BYTES);
    bool ok = true;
    int32_t max_abs = 0, exact = 0;
    for (int64_t b = first; b < g.blocks; b += stride) {
        const int c = b < g.n0 ? 0 : (b < g.n0 + g.nc ? 1 : 2);
        if (!lemon_jpeg::block_in_envelope(coef + 64 * b, quant + 64 * c, max_abs, exact)) ok = false;
    }
    return ok;
}

// A record before its first coefficient: zeros behind the packet's quantisers (both packets keep them at byte 128).  Returns
// the coefficients.  Callers: both host loops below and in jpeg_prog_par.hpp, lemon_jpeg_prog::seq_decode (jpeg_prog.hpp).
static inline int16_t *par_new_record(uint8_t *record, const uint8_t *pkt, const JpegGeom &g) {
    memset(record, 0, (size_t)(LEMON_JPEG_QUANT_BYTES + 128 * g.blocks));
    memcpy(record, pkt + kQuantOff, LEMON_JPEG_QUANT_BYTES);
    return reinterpret_cast<int16_t *>(record + LEMON_JPEG_QUANT_BYTES);
}

#if defined(__HIPCC__)
// ---- what the kernels of jpeg_entropy.hip and jpeg_prog.hip share beyond the step functions (their grids differ)
// an image's descriptor (packet offset, packet bytes, record offset, ...) against the extents of the two buffers (jent_open,
// jprog_open)
__device__ __forceinline__ bool jpeg_dev_extents(const int64_t *d, int64_t pk_bytes, int64_t rec_bytes) {
    if (d[0] < 0 || (d[0] & 15) != 0 || d[1] < 0 || d[0] > pk_bytes || d[1] > pk_bytes - d[0]) return false;
    return d[2] >= 0 && (d[2] & 15) == 0 && d[2] <= rec_bytes;
}

// par_new_record, 16 bytes per thread: units first, first + stride, ... of the record (k_jent_zero, k_jprog_zero)
__device__ __forceinline__ void jpeg_dev_new_record(uint8_t *rec, const uint8_t *pkt, const JpegGeom &g, int64_t first, int64_t stride) {
    const int64_t n16 = (LEMON_JPEG_QUANT_BYTES + 128 * g.blocks) / 16;
    const uint4 *q = reinterpret_cast<const uint4 *>(pkt + kQuantOff);
    for (int64_t k = first; k < n16; k += stride)
        reinterpret_cast<uint4 *>(rec)[k] = k < LEMON_JPEG_QUANT_BYTES / 16 ? q[k] : make_uint4(0, 0, 0, 0);
}
#endif

LEMON_JPEG_HD int32_t par_subseq(int32_t subseq) { return subseq == 0 ? LEMON_JPEG_SUBSEQ_DEFAULT : subseq; }
LEMON_JPEG_HD bool par_subseq_ok(int32_t subseq) {
    return subseq == 0 || (subseq >= LEMON_JPEG_SUBSEQ_MIN && subseq <= LEMON_JPEG_SUBSEQ_MAX && (subseq & 3) == 0);
}

}  // namespace lemon_jpeg_par

// ------------------------------------------------------------------------------------------------------- host entry points
static inline int lemon_jpeg_pack_impl(const uint8_t *data, int64_t n, uint8_t *packet, int64_t cap, LemonJpegInfo *info,
                                       int64_t *packet_bytes) {
    memset(info, 0, sizeof(*info));
    if (packet_bytes) *packet_bytes = 0;
    if (!data || n < 0) return info->status = LEMON_JPEG_NOT_JPEG;
    lemon_jpeg::BaseFile *f = new lemon_jpeg::BaseFile();
    const int rc = lemon_jpeg_par::pack(data, (size_t)n, packet, cap, info, packet_bytes, *f);
    delete f;
    return info->status = rc;
}

// The kernels' algorithm with the lanes looped: the same workgroups of 256 lanes, the same rounds, the same final pass.
static inline int lemon_jpeg_entropy_par_host_impl(const uint8_t *packet, int64_t bytes, int32_t subseq, uint8_t *record,
                                                   int64_t record_cap, int32_t *status) {
    using namespace lemon_jpeg_par;
    if (!status) return 1;
    *status = LEMON_JPEG_BUFFER;
    if (!par_subseq_ok(subseq)) return 1;
    const int32_t S = par_subseq(subseq);
    ParImage im;
    if (!record || !par_open(packet, bytes, record_cap, im)) return 0;
    ParHuff *huff = new ParHuff[6];
    bool ok = true;
    for (int c = 0; c < im.nc; ++c) {
        ok = par_build_huff(par_spec(im, c, 0), huff[c]) && ok;
        ok = par_build_huff(par_spec(im, c, 1), huff[3 + c]) && ok;
    }
    // the intervals' first bytes and first lanes
    const int64_t nivl = im.nivl;
    int64_t *ivl_start = new int64_t[nivl + 1], *ivl_lane0 = new int64_t[nivl + 1];
    ivl_start[0] = ivl_lane0[0] = 0;
    for (int64_t t = 0; t < nivl; ++t) {
        const int64_t len = par_interval_bytes(im, t);
        ivl_start[t + 1] = ivl_start[t] + len;
        ivl_lane0[t + 1] = ivl_lane0[t] + par_lanes_of(len, S);
    }
    if (ivl_start[nivl] != im.scan_bytes) ok = false;
    int st = LEMON_JPEG_OK;
    if (!ok) {
        delete[] huff; delete[] ivl_start; delete[] ivl_lane0;
        return 0;                                                    // (*status = LEMON_JPEG_BUFFER: no packet of lemon_jpeg_pack)
    }
    const int64_t lanes = ivl_lane0[nivl];
    ParLane *L = new ParLane[lanes];
    for (int64_t t = 0; t < nivl; ++t)
        for (int64_t j = ivl_lane0[t]; j < ivl_lane0[t + 1]; ++j) {
            ParLane &l = L[j];
            const int64_t i = j - ivl_lane0[t];
            l.d = im.scan + ivl_start[t]; l.len = ivl_start[t + 1] - ivl_start[t];
            l.end_bit = 8 * (l.len < (i + 1) * S ? l.len : (i + 1) * S);
            const McuRange r = interval_mcus(im.restart, im.mcus, t);
            l.mcu0 = r.first; l.total = r.count * im.spm;
            l.guess = par_state(8 * i * S, 0, 0);
            l.first = i == 0; l.last = j + 1 == ivl_lane0[t + 1];
        }
    uint64_t *entry = new uint64_t[lanes], *exitst = new uint64_t[lanes];
    int64_t *cnt = new int64_t[lanes], *first_blk = new int64_t[lanes];
    const int64_t nwg = (lanes + LEMON_JPEG_PAR_GROUP - 1) / LEMON_JPEG_PAR_GROUP;
    uint64_t *wgexit = new uint64_t[2 * nwg];
    for (int r = 0; r < LEMON_JPEG_PAR_ROUNDS; ++r)
        for (int64_t w = 0; w < nwg; ++w) {
            const int64_t j0 = w * LEMON_JPEG_PAR_GROUP, j1 = j0 + LEMON_JPEG_PAR_GROUP < lanes ? j0 + LEMON_JPEG_PAR_GROUP : lanes;
            for (int64_t j = j0; j < j1; ++j) {
                // (the fixed point the workgroup's iterations reach: every lane decoded from its left neighbour's exit)
                const uint64_t e = L[j].first ? L[j].guess : (j > j0 ? exitst[j - 1] : (r == 0 ? L[j].guess : wgexit[((r - 1) & 1) * nwg + w - 1]));
                if (r > 0 && e == entry[j]) continue;
                entry[j] = e;
                uint64_t s = e;
                int64_t n = 0;
                bool done;
                par_run<false>(huff, im, L[j], s, n, nullptr, 0, done);
                exitst[j] = s; cnt[j] = n;
            }
            wgexit[(r & 1) * nwg + w] = exitst[j1 - 1];
        }
    for (int64_t j = 0, run = 0; j < lanes; ++j) {                   // exclusive sums of the block counts inside each interval
        if (L[j].first) run = 0;
        first_blk[j] = run;
        run += cnt[j];
    }
    int16_t *coef = par_new_record(record, packet, im.g);
    for (int64_t j = 0; j < lanes; ++j) {
        const int rc = par_final_lane(huff, im, L[j], L[j].first ? L[j].guess : exitst[j - 1], entry[j], exitst[j], first_blk[j], coef);
        if (rc > st) st = rc;
    }
    for (int c = 0; c < im.nc; ++c) {
        const int64_t nb = c == 0 ? im.g.n0 : im.g.nc;
        int64_t run = 0;
        for (int64_t q = 0; q < nb; ++q) {
            bool head;
            int16_t *b = coef + 64 * par_comp_block_addr(im, c, q, head);
            run = (head ? 0 : run) + b[0];
            if (run < -32768 || run > 32767) { if (LEMON_JPEG_CODE > st) st = LEMON_JPEG_CODE; }
            b[0] = (int16_t)run;
        }
    }
    if (!par_envelope_blocks(record, im.g, 0, 1) && LEMON_JPEG_ENVELOPE > st) st = LEMON_JPEG_ENVELOPE;
    *status = st;
    delete[] huff; delete[] ivl_start; delete[] ivl_lane0; delete[] L; delete[] entry; delete[] exitst; delete[] cnt;
    delete[] first_blk; delete[] wgexit;
    return 0;
}
