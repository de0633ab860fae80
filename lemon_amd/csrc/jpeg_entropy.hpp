// jpeg_entropy.hpp -- the host half of the JPEG decode: marker parsing and Huffman decoding of a baseline file into dense
// quantised coefficient blocks (the serial part; dequantisation, inverse DCT, upsampling and colour conversion run on the GPU,
// jpeg.hip).  Plain C++17, header-only, no HIP, so that it is also compiled with g++ into liblemon_jpeg_host.so (loaded by the
// decode workers) and under AddressSanitizer / UBSan for the fuzzer (tests/native/jpeg_fuzz.cpp).
//
// The input is untrusted: every read is checked against the end of the buffer, every table index is validated, and anything
// the decoder does not fully support is DECLINED with a status code (the caller then decodes with PIL), never guessed at.
// Four pieces here serve every JPEG path, the progressive and the device ones included, so that a check exists once:
// jpeg_build_huff (a Huffman table from counts and values), read_to_sos (the marker-segment loop), frame_checks (sampling,
// colour ids, geometry) and envelope_verdict / block_in_envelope (the arithmetic envelope of a finished block).
//
// Record written for an accepted file (LemonJpegInfo::record_bytes = 384 + 128 * blocks):
//   uint16 quant[3][64]      the quantisation table of each component, natural order (unused components: zeros)
//   int16  coef[blocks][64]  component 0 [block row][block col][64], then components 1 and 2, natural order, over the
//                            MCU-padded block grid (jpeg_core.hpp::jpeg_geometry)
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/lemon_hip.h"
#include "jpeg_core.hpp"

enum LemonJpegStatus {
    LEMON_JPEG_OK = 0,
    LEMON_JPEG_NOT_JPEG = 1,          // no SOI
    LEMON_JPEG_TRUNCATED = 2,         // a segment or the header runs past the end of the file
    LEMON_JPEG_PROCESS = 3,           // progressive, arithmetic, lossless, hierarchical, DNL
    LEMON_JPEG_PRECISION = 4,         // not 8-bit samples
    LEMON_JPEG_COMPONENTS = 5,        // not 1 or 3 components
    LEMON_JPEG_SAMPLING = 6,          // sampling factors other than 1x1 / 2x1 / 2x2 luma over 1x1 chroma
    LEMON_JPEG_COLOUR = 7,            // Adobe marker, or component ids that libjpeg would not read as YCbCr
    LEMON_JPEG_TABLE = 8,             // malformed, 16-bit or missing quantisation / Huffman table
    LEMON_JPEG_SCAN = 9,              // not one interleaved sequential scan over all components
    LEMON_JPEG_CODE = 10,             // a code that is not in its table, a coefficient index or value out of range
    LEMON_JPEG_STREAM = 11,           // the bit stream ends early, runs past its last MCU, or a restart marker is wrong
    LEMON_JPEG_ENVELOPE = 12,         // a block outside the arithmetic envelope (below)
    LEMON_JPEG_BUFFER = 13,           // the caller's record buffer is too small
    LEMON_JPEG_DIMENSION = 14,        // a dimension of 0
    LEMON_JPEG_MARKER = 15,           // a marker that may not appear where it does
};

namespace lemon_jpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- Huffman tables.  The ONE construction and validation of a table from (16 counts, values); every path that reads a DHT
// segment or a packet's specification goes through it.  Callers: read_to_sos below (both parsers), par_build_huff
// (jpeg_par.hpp: the baseline kernels and their host loop), prog_build_huff (jpeg_prog_par.hpp: the progressive ones).
struct ParHuff {                      // what the device decodes with
    uint16_t look[512];               // 9-bit prefix -> (length << 8 | value), 0 when the code is longer
    int32_t maxcode[18];              // largest code of each length, -1 when none
    int32_t valptr[17];               // index of the first value of each length, minus its first code
    uint8_t vals[256];
};

// counts[0..15]: codes of length 1..16; vals[0, avail): their values.  Always initialises all of `h`; false when the counts ask
// for more than 256 values or for values past `avail`, or describe no prefix code (`h` then holds the lengths before the fault).
LEMON_JPEG_HD bool jpeg_build_huff(const uint8_t *counts, const uint8_t *vals, int64_t avail, ParHuff &h) {
    for (int i = 0; i < 512; ++i) h.look[i] = 0;
    for (int i = 0; i < 256; ++i) h.vals[i] = 0;
    for (int l = 0; l < 17; ++l) { h.maxcode[l] = -1; h.valptr[l] = 0; }
    h.maxcode[17] = 0x7fffffff;
    int32_t total = 0;
    for (int l = 0; l < 16; ++l) total += counts[l];
    if (total > 256 || total > avail) return false;
    for (int i = 0; i < total; ++i) h.vals[i] = vals[i];
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        if (code + c > (1 << l)) return false;
        h.valptr[l] = k - code;
        h.maxcode[l] = c ? code + c - 1 : -1;
        if (l <= 9)
            for (int i = 0; i < c; ++i) {
                const int32_t first = (code + i) << (9 - l);
                for (int32_t j = 0; j < (1 << (9 - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
            }
        code += c; k += c;
        code <<= 1;
    }
    return true;
}

struct Huff : ParHuff {               // the sequential pass's table: ParHuff plus
    bool defined = false;
    // AC tables: 10-bit prefix -> a whole (run, size) symbol WITH its magnitude bits when both fit the prefix:
    // value << 16 | is_coefficient << 12 | run << 8 | bits consumed; 0 when they do not fit
    int32_t fast[1024];
};

static inline void build_fast(Huff &h) {
    for (int32_t i = 0; i < 1024; ++i) {
        h.fast[i] = 0;
        const uint32_t e = h.look[i >> 1];
        if (!e) continue;
        const int l = (int)(e >> 8), r = (int)(e & 255) >> 4, sz = (int)(e & 15);
        if (sz == 0) {                                        // EOB / ZRL (any other run with size 0 is left to the slow path)
            if (r == 0 || r == 15) h.fast[i] = (r << 8) | l;
            continue;
        }
        if (l + sz > 10 || sz > 10) continue;
        int32_t v = (i >> (10 - l - sz)) & ((1 << sz) - 1);
        if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
        h.fast[i] = (int32_t)((uint32_t)v << 16) | (1 << 12) | (r << 8) | (l + sz);
    }
}

struct Frame {
    int32_t w = 0, h = 0, nc = 0;
    int32_t id[3], hs[3], vs[3], tq[3], td[3], ta[3];
    bool have_sof = false, jfif = false, sof1 = false;
    int32_t restart = 0;
    bool q_defined[4] = {false, false, false, false};
    uint16_t q[4][64];                // natural order
    size_t scan = 0;                  // first byte of the entropy-coded segment
};

static inline int rd16(const uint8_t *d, size_t p) { return (d[p] << 8) | d[p + 1]; }

// The ONE marker-segment loop.  From the marker at d[p] on it applies DQT, DHT, DRI, SOFn, APP0 "JFIF" and APP14 "Adobe" to `f`
// and skips the other APPn and COM, up to the next SOS: LEMON_JPEG_OK with its payload in s[0, sl) and p behind the segment.
// sof2: the frame must be SOF2 (progressive), else SOF0 / SOF1; every other process is LEMON_JPEG_PROCESS.  after_scan (a
// progressive file past its first scan): EOI ends the loop too (`eoi`), and a JFIF marker no longer counts.  A DHT table that
// is a prefix code of at most 256 values inside its segment (and, for DC, of categories <= 11) is handed to
// on_table(tc, th, table, offset of its 16 counts in d).  Callers: parse_header below, lemon_jpeg_prog::parse (jpeg_prog.hpp).
template <class OnTable>
static inline int read_to_sos(const uint8_t *d, size_t n, size_t &p, Frame &f, bool sof2, bool after_scan, OnTable on_table,
                              const uint8_t *&s, size_t &sl, bool &eoi) {
    eoi = false;
    for (;;) {
        if (p + 2 > n) return LEMON_JPEG_TRUNCATED;
        if (d[p] != 0xFF) return LEMON_JPEG_MARKER;
        while (p + 1 < n && d[p + 1] == 0xFF) ++p;        // fill bytes
        if (p + 2 > n) return LEMON_JPEG_TRUNCATED;
        const int m = d[p + 1];
        p += 2;
        if (m == 0xD9 && after_scan) { eoi = true; return LEMON_JPEG_OK; }
        const bool sof = sof2 ? m == 0xC2 : (m == 0xC0 || m == 0xC1);
        if (!sof && ((m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8) || m == 0xDC || m == 0xDE || m == 0xDF))
            return LEMON_JPEG_PROCESS;                  // another SOFn, DAC, DNL, DHP, EXP
        const bool segment = sof || m == 0xC4 || m == 0xDA || m == 0xDB || m == 0xDD || (m >= 0xE0 && m <= 0xEF) || m == 0xFE;
        if (!segment) return LEMON_JPEG_MARKER;         // SOI again, EOI, RSTn, TEM, reserved: none belongs between segments
        if (p + 2 > n) return LEMON_JPEG_TRUNCATED;
        const size_t len = (size_t)rd16(d, p);
        if (len < 2 || len > n - p) return LEMON_JPEG_TRUNCATED;
        s = d + p + 2;
        sl = len - 2;
        p += len;
        if (m == 0xE0) {
            if (!after_scan && sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) f.jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 5 && memcmp(s, "Adobe", 5) == 0) return LEMON_JPEG_COLOUR;
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq != 0 || tq > 3) return LEMON_JPEG_TABLE;
                if (sl - o < 65) return LEMON_JPEG_TABLE;
                for (int k = 0; k < 64; ++k) f.q[tq][kZigzag[k]] = s[o + 1 + k];
                f.q_defined[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < sl) {
                if (sl - o < 17) return LEMON_JPEG_TABLE;
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return LEMON_JPEG_TABLE;
                ParHuff t;
                if (!jpeg_build_huff(s + o + 1, s + o + 17, (int64_t)(sl - o - 17), t)) return LEMON_JPEG_TABLE;
                int total = 0;
                for (int l = 1; l <= 16; ++l) total += s[o + l];
                for (int i = 0; i < total; ++i)
                    if (tc == 0 && t.vals[i] > 11) return LEMON_JPEG_TABLE;         // a DC category beyond 8-bit samples
                on_table(tc, th, t, (size_t)(s + o + 1 - d));
                o += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return LEMON_JPEG_TABLE;
            f.restart = rd16(s, 0);
        } else if (sof) {
            if (f.have_sof) return LEMON_JPEG_MARKER;
            if (sl < 6) return LEMON_JPEG_TRUNCATED;
            if (s[0] != 8) return LEMON_JPEG_PRECISION;
            f.h = rd16(s, 1); f.w = rd16(s, 3); f.nc = s[5];
            if (f.h == 0 || f.w == 0) return LEMON_JPEG_DIMENSION;
            if (f.nc != 1 && f.nc != 3) return LEMON_JPEG_COMPONENTS;
            if (sl != (size_t)(6 + 3 * f.nc)) return LEMON_JPEG_TRUNCATED;
            for (int c = 0; c < f.nc; ++c) {
                f.id[c] = s[6 + 3 * c]; f.hs[c] = s[7 + 3 * c] >> 4; f.vs[c] = s[7 + 3 * c] & 15; f.tq[c] = s[8 + 3 * c];
                if (f.tq[c] > 3) return LEMON_JPEG_TABLE;
            }
            f.have_sof = true; f.sof1 = m == 0xC1;
        } else if (m == 0xDA) {
            return f.have_sof ? LEMON_JPEG_OK : LEMON_JPEG_MARKER;
        }
        // APPn other than the two above, COM: skipped
    }
}

// What a frame must satisfy beyond its segments' own syntax: sampling, colour ids, geometry; fills the geometry fields of
// `info` (not the quantisers).  Callers: parse_header (after its SOS), lemon_jpeg_prog::parse (at its first SOS).
static inline int frame_checks(const Frame &f, LemonJpegInfo *info) {
    int hs = 1, vs = 1;
    if (f.nc == 3) {
        hs = f.hs[0]; vs = f.vs[0];
        if (f.hs[1] != 1 || f.vs[1] != 1 || f.hs[2] != 1 || f.vs[2] != 1) return LEMON_JPEG_SAMPLING;
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return LEMON_JPEG_SAMPLING;
        // without a JFIF marker libjpeg assumes YCbCr only for the ids 1, 2, 3
        if (!f.jfif && !(f.id[0] == 1 && f.id[1] == 2 && f.id[2] == 3)) return LEMON_JPEG_COLOUR;
    } else if (f.hs[0] < 1 || f.hs[0] > 4 || f.vs[0] < 1 || f.vs[0] > 4) {
        return LEMON_JPEG_SAMPLING;       // (a single component is never interleaved: valid factors do not matter)
    }
    JpegGeom g;
    if (!jpeg_geometry(f.w, f.h, f.nc, hs, vs, g)) return LEMON_JPEG_DIMENSION;
    info->width = f.w; info->height = f.h; info->components = f.nc; info->hs = hs; info->vs = vs;
    info->mcus_x = f.nc == 3 ? g.bwc : g.bw0; info->mcus_y = f.nc == 3 ? g.bhc : g.bh0;
    info->blocks = g.blocks;
    info->record_bytes = LEMON_JPEG_QUANT_BYTES + 128 * g.blocks;
    return LEMON_JPEG_OK;
}

struct BaseFile {                     // a baseline file's frame and the tables its one scan decodes with
    Frame f;
    Huff dc[4], ac[4];
};

// Markers from SOI up to and including SOS.  Fills `info` (geometry, quantisers, record size) when it returns LEMON_JPEG_OK.
static inline int parse_header(const uint8_t *d, size_t n, BaseFile &bf, LemonJpegInfo *info) {
    Frame &f = bf.f;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return LEMON_JPEG_NOT_JPEG;
    size_t p = 2, sl = 0;
    const uint8_t *s = nullptr;
    bool eoi;
    const int rc = read_to_sos(d, n, p, f, false, false, [&bf](int tc, int th, const ParHuff &t, size_t) {
        Huff &h = tc ? bf.ac[th] : bf.dc[th];
        static_cast<ParHuff &>(h) = t;
        h.defined = true;
        build_fast(h);
    }, s, sl, eoi);
    if (rc != LEMON_JPEG_OK) return rc;
    if (sl < 1 || s[0] != f.nc || sl != (size_t)(4 + 2 * f.nc)) return LEMON_JPEG_SCAN;
    for (int c = 0; c < f.nc; ++c) {
        if (s[1 + 2 * c] != f.id[c]) return LEMON_JPEG_SCAN;
        f.td[c] = s[2 + 2 * c] >> 4; f.ta[c] = s[2 + 2 * c] & 15;
        const int lim = f.sof1 ? 3 : 1;
        if (f.td[c] > lim || f.ta[c] > lim || !bf.dc[f.td[c]].defined || !bf.ac[f.ta[c]].defined) return LEMON_JPEG_TABLE;
        if (!f.q_defined[f.tq[c]]) return LEMON_JPEG_TABLE;
    }
    if (s[1 + 2 * f.nc] != 0 || s[2 + 2 * f.nc] != 63 || s[3 + 2 * f.nc] != 0) return LEMON_JPEG_SCAN;
    f.scan = p;
    const int fc = frame_checks(f, info);
    if (fc != LEMON_JPEG_OK) return fc;
    memset(info->quant, 0, sizeof(info->quant));
    for (int c = 0; c < f.nc; ++c) memcpy(info->quant[c], f.q[f.tq[c]], 128);
    return LEMON_JPEG_OK;
}

// MSB-first bit reader over the entropy-coded segment: FF 00 is a data byte FF, any other FF xx is a marker, at which the
// reader stops and supplies zero bits (`pad` counts those still in the accumulator, so a consumer that was handed one is found
// out by `overrun()`).
struct Bits {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int32_t bits = 0, pad = 0;
    bool at_marker = false;

    inline void fill() {
        if (bits >= 32) return;
        if (!at_marker && end - p >= 4) {                      // four plain bytes at once
            const uint32_t v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            if ((((~v) - 0x01010101u) & v & 0x80808080u) == 0) {       // no byte is FF
                acc = (acc << 32) | v;
                bits += 32;
                p += 4;
                return;
            }
        }
        while (bits <= 56) {
            uint32_t c = 0;
            if (!at_marker && p < end) {
                c = *p;
                if (c == 0xFF) {
                    if (p + 1 < end && p[1] == 0) p += 2;
                    else { at_marker = true; c = 0; pad += 8; }
                } else {
                    ++p;
                }
            } else {
                at_marker = true;
                pad += 8;
            }
            acc = (acc << 8) | c;
            bits += 8;
        }
    }
    inline uint32_t peek(int nb) const { return (uint32_t)(acc >> (bits - nb)) & ((1u << nb) - 1u); }
    inline void skip(int nb) { bits -= nb; }
    inline bool overrun() const { return bits < pad; }
    inline int real_bits() const { return bits - pad; }
    inline void reset() { acc = 0; bits = 0; pad = 0; at_marker = false; }
};

// one Huffman symbol, -1 when the next bits are no code of the table
static inline int decode_symbol(Bits &b, const Huff &h) {
    const uint32_t e = h.look[b.peek(9)];
    if (e) { b.skip((int)(e >> 8)); return (int)(e & 255); }
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)b.peek(l);
        if (code <= h.maxcode[l]) {
            const int32_t idx = h.valptr[l] + code;
            if (idx < 0 || idx > 255) return -1;
            b.skip(l);
            return h.vals[idx];
        }
    }
    return -1;
}

static inline int32_t receive_extend(Bits &b, int s) {
    const int32_t v = (int32_t)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Envelope.  The result must equal libjpeg-turbo's whichever inverse DCT it runs: the C form (jidctint.c, 32-bit) or a SIMD
// form, which keeps the dequantised coefficients and the pass-1 results in 16-bit lanes, forms sums of two of them in 16 bits
// before its widening multiplies, and narrows the final value with SATURATION where the C form masks it to 10 bits
// (jpeg_core.hpp::jpeg_range_limit).  The device arithmetic is the C form.  All three coincide for a block when
//   (E1) every dequantised coefficient d and every pass-1 result ws has |.| <= 16383: each fits a 16-bit lane and so does the
//        sum or difference of any two; and with inputs of that size every term of jpeg_idct_1d stays below 2^31 (largest:
//        |t10| + |a3| <= 2*16383*8192 + 16383*(4433 + 4433 + 6270) + 16383*(12299 + 2*7373 + 2*3196 + 4*9633) < 1.8e9);
//   (E2) every pass-2 result x lies in [-512, 511]: masking to 10 signed bits is then the identity, so mask-then-clamp
//        (C) equals saturate (SIMD).
// No norm of the coefficients can decide (E2) for every block an encoder writes (a flat block and a noise block of equal
// norm differ eightfold in their largest sample), so the check has two forms:
//   quick   D + 2 A <= 4000 with D = |d[0]| and A the sum of |d| over the 63 other coefficients.  Every weight with which a
//           1-D step combines its inputs is at most c = 11363/8192 < 1.3875 in magnitude (1 for index 0), so
//           |ws| <= 4 (D + c A) + 1 <= 16001 (E1), and |x| <= D/8 + c^2 A/8 + (1 + 7c)/32 + 1 < (D + 2 A)/8 + 2 <= 502 (E2).
//   exact   otherwise jpeg_block_in_envelope() evaluates the block's inverse DCT and tests (E1) and (E2) themselves.
// A block from 8-bit pixels has pass-1 results 4 sqrt(8) times a 1-D DCT of pixel rows in [-128, 127] (<= 4096 in magnitude)
// plus the spread of the quantisation error, and pass-2 results within a few quantisation steps of [-128, 127]: inside both.
// An image with a block outside is declined (LEMON_JPEG_ENVELOPE).
static const int32_t kEnvelopeQuick = 4000;

// The ONE verdict on a finished block: D = |d[0]|, A = the sum of |d| over the other 63 dequantised coefficients.  `exact`
// counts the blocks that needed the exact form.  Callers: decode_scan (which sums D and A while it decodes), block_in_envelope.
LEMON_JPEG_HD bool envelope_verdict(int64_t D, int64_t A, const int16_t *blk, const uint16_t *qt, int32_t &exact) {
    if (D + 2 * A <= kEnvelopeQuick) return true;
    ++exact;
    return jpeg_block_in_envelope(blk, qt);
}

// ... of a block in memory; `max_abs` takes the largest |d| seen (|d| <= 32768 * 65535 < 2^31).  Callers: par_envelope_blocks
// (jpeg_par.hpp: the host loops and the kernels of both parallel passes), lemon_jpeg_prog::seq_decode (jpeg_prog.hpp).
LEMON_JPEG_HD bool block_in_envelope(const int16_t *blk, const uint16_t *qt, int32_t &max_abs, int32_t &exact) {
    int64_t A = 0;
    int32_t D = 0;
    for (int i = 0; i < 64; ++i) {
        const int32_t v = blk[i], a = (v < 0 ? -v : v) * (int32_t)qt[i];
        if (a > max_abs) max_abs = a;
        if (i) A += a; else D = a;
    }
    return envelope_verdict(D, A, blk, qt, exact);
}

static inline int decode_scan(const uint8_t *d, size_t n, const BaseFile &bf, LemonJpegInfo *info, uint8_t *record) {
    const Frame &f = bf.f;
    JpegGeom g;
    if (!jpeg_geometry(info->width, info->height, info->components, info->hs, info->vs, g)) return LEMON_JPEG_DIMENSION;
    memcpy(record, info->quant, LEMON_JPEG_QUANT_BYTES);
    int16_t *coef = reinterpret_cast<int16_t *>(record + LEMON_JPEG_QUANT_BYTES);
    const int nc = info->components, hs = info->hs, vs = info->vs;
    const int64_t base[3] = {0, g.n0, g.n0 + g.nc};
    const int32_t bw[3] = {g.bw0, g.bwc, g.bwc};
    const int32_t mx = info->mcus_x, my = info->mcus_y;
    const int cw[3] = {nc == 3 ? hs : 1, 1, 1}, ch[3] = {nc == 3 ? vs : 1, 1, 1};
    Bits b;
    b.p = d + f.scan; b.end = d + n;
    int32_t pred[3] = {0, 0, 0};
    int32_t max_abs = 0, exact = 0;
    int64_t todo = f.restart, mcu = 0;
    for (int32_t yy = 0; yy < my; ++yy)
        for (int32_t xx = 0; xx < mx; ++xx, ++mcu) {
            if (f.restart && todo == 0) {
                // the interval's last byte is padding only; then (fill bytes and) RSTn with n counting modulo 8
                if (b.overrun() || b.real_bits() >= 8) return LEMON_JPEG_STREAM;
                b.fill();
                if (!b.at_marker || b.real_bits() >= 8) return LEMON_JPEG_STREAM;
                const uint8_t *q = b.p;
                while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
                if (q + 2 > b.end || q[0] != 0xFF || q[1] != (uint8_t)(0xD0 + ((mcu / f.restart - 1) & 7))) return LEMON_JPEG_STREAM;
                b.p = q + 2;
                b.reset();
                pred[0] = pred[1] = pred[2] = 0;
                todo = f.restart;
            }
            for (int c = 0; c < nc; ++c) {
                const Huff &hd = bf.dc[f.td[c]], &ha = bf.ac[f.ta[c]];
                const uint16_t *qt = info->quant[c];
                for (int by = 0; by < ch[c]; ++by)
                    for (int bx = 0; bx < cw[c]; ++bx) {
                        int16_t *blk = coef + 64 * (base[c] + (int64_t)(yy * ch[c] + by) * bw[c] + (xx * cw[c] + bx));
                        memset(blk, 0, 128);
                        b.fill();
                        int s = decode_symbol(b, hd);
                        if (s < 0 || s > 11) return LEMON_JPEG_CODE;
                        if (s) pred[c] += receive_extend(b, s);
                        if (pred[c] < -32768 || pred[c] > 32767) return LEMON_JPEG_CODE;
                        blk[0] = (int16_t)pred[c];
                        const int32_t D = (pred[c] < 0 ? -pred[c] : pred[c]) * (int32_t)qt[0];
                        int64_t A = 0;
                        if (D > max_abs) max_abs = D;
                        for (int k = 1; k < 64;) {
                            b.fill();
                            const int32_t e = ha.fast[b.peek(10)];
                            int r;
                            int32_t v;
                            if (e) {
                                b.skip(e & 255);
                                r = (e >> 8) & 15;
                                if (!(e & (1 << 12))) {
                                    if (r == 0) break;
                                    k += 16;
                                    if (k > 64) return LEMON_JPEG_CODE;
                                    continue;
                                }
                                v = e >> 16;
                                k += r;
                                if (k > 63) return LEMON_JPEG_CODE;
                            } else {
                                const int rs = decode_symbol(b, ha);
                                if (rs < 0) return LEMON_JPEG_CODE;
                                r = rs >> 4;
                                s = rs & 15;
                                if (s == 0) {
                                    if (r == 15) { k += 16; if (k > 64) return LEMON_JPEG_CODE; continue; }
                                    if (r != 0) return LEMON_JPEG_CODE;
                                    break;
                                }
                                k += r;
                                if (k > 63 || s > 10) return LEMON_JPEG_CODE;
                                v = receive_extend(b, s);
                            }
                            const int nat = kZigzag[k];
                            blk[nat] = (int16_t)v;
                            const int32_t a = (v < 0 ? -v : v) * (int32_t)qt[nat];
                            A += a;
                            if (a > max_abs) max_abs = a;
                            ++k;
                        }
                        if (b.overrun()) return LEMON_JPEG_STREAM;
                        if (!envelope_verdict(D, A, blk, qt, exact)) return LEMON_JPEG_ENVELOPE;
                    }
            }
            if (f.restart) --todo;
        }
    // after the last MCU: padding only, then (fill bytes and) EOI
    if (b.overrun() || b.real_bits() >= 8) return LEMON_JPEG_STREAM;
    b.fill();
    if (!b.at_marker || b.real_bits() >= 8) return LEMON_JPEG_STREAM;
    const uint8_t *q = b.p;
    while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
    if (q + 2 > b.end || q[0] != 0xFF || q[1] != 0xD9) return LEMON_JPEG_STREAM;
    info->max_abs = max_abs;
    info->exact_blocks = exact;
    return LEMON_JPEG_OK;
}

}  // namespace lemon_jpeg

// Header only: geometry, quantisers and the record size of a file (status LEMON_JPEG_OK), or why it is declined.
static inline int lemon_jpeg_info_impl(const uint8_t *data, int64_t n, LemonJpegInfo *info) {
    memset(info, 0, sizeof(*info));
    if (!data || n < 0) return info->status = LEMON_JPEG_NOT_JPEG;
    lemon_jpeg::BaseFile *f = new lemon_jpeg::BaseFile();
    const int rc = lemon_jpeg::parse_header(data, (size_t)n, *f, info);
    delete f;
    return info->status = rc;
}

// The whole host pass: `record` receives info->record_bytes bytes (at most `record_cap`).  A declined file leaves the record's
// contents unspecified (within `record_cap`).
static inline int lemon_jpeg_entropy_impl(const uint8_t *data, int64_t n, uint8_t *record, int64_t record_cap, LemonJpegInfo *info) {
    memset(info, 0, sizeof(*info));
    if (!data || n < 0) return info->status = LEMON_JPEG_NOT_JPEG;
    lemon_jpeg::BaseFile *f = new lemon_jpeg::BaseFile();
    int rc = lemon_jpeg::parse_header(data, (size_t)n, *f, info);
    if (rc == LEMON_JPEG_OK && (!record || info->record_bytes > record_cap)) rc = LEMON_JPEG_BUFFER;
    if (rc == LEMON_JPEG_OK) rc = lemon_jpeg::decode_scan(data, (size_t)n, *f, info, record);
    delete f;
    return info->status = rc;
}
