// jpeg_prog.hpp -- the host half of the decode of a PROGRESSIVE JPEG (SOF2): marker parsing over all scans, the packer
// (lemon_jpeg_prog_pack: file -> the packet of jpeg_prog_par.hpp) and the sequential Huffman pass (lemon_jpeg_prog_entropy: file ->
// the coefficient record of jpeg_entropy.hpp, which lemon_jpeg_decode and lemon_jpeg_reconstruct_host read unchanged).  Plain
// C++17, header-only, no HIP; compiled into both libraries like jpeg_entropy.hpp and under ASan / UBSan by
// tests/native/jpeg_prog_fuzz.cpp.
//
// Accepted: 8-bit Huffman SOF2 files of 1 or 3 components under parse_header's sampling and colour rules, DQT / DHT / DRI between
// scans (quantisers as in effect at a component's first scan, tables and restart interval as in effect at each SOS), restart
// intervals, at most 64 scans; a scan holds one component or all of them in frame order.  The input is untrusted: every read is
// checked against the end of the buffer, and a file is DECLINED with a status, never guessed at, whenever libjpeg would warn or
// its result would not be the plain inverse DCT of the decoded coefficients:
//   LEMON_JPEG_SCAN         a scan libjpeg refuses or warns about (Ss = 0 with Se != 0, an AC scan of several components,
//                           Se < Ss, Se > 63, Al > 13, Ah != 0 with Al != Ah - 1, an AC scan before the component's DC scan, a
//                           first scan (Ah = 0) of a coefficient sent before, a refinement whose Ah is not the coefficient's last
//                           Al), two components, more than 64 scans
//   LEMON_JPEG_PROGRESSION  at EOI some coefficient of some component has not been sent down to bit 0: libjpeg would smooth
//   LEMON_JPEG_STREAM       marker structure of a scan's bytes (an empty interval, RSTn out of sequence, too few or too many
//                           intervals, a fill byte before data), data that ends before the scan's blocks do, bytes left over, an
//                           EOB run past the interval's last block
//   LEMON_JPEG_CODE         no code of the table, a coefficient index past Se, a refinement symbol of size != 1, a value that
//                           an int16 does not hold after the shift by Al
// The Huffman pass itself reads the packet (so the packer's checks ARE the host pass's marker checks) and walks the work items of
// jpeg_prog_par.hpp level by level with the verdict rule stated there, but decodes every block the way libjpeg's jdphuff.c does:
// coefficient by coefficient in place.  Of the decode, only the bit window and the Huffman step are shared with the device form.
// The marker segments between the scans are read by jpeg_entropy.hpp's read_to_sos and judged by its frame_checks, the scans'
// bytes are walked by jpeg_par.hpp's walk_scan: the baseline path's own functions.
#pragma once
#include <stdlib.h>

#include "jpeg_prog_par.hpp"

namespace lemon_jpeg_prog {

struct FileTable { bool defined = false; size_t at = 0; int32_t pool = -1; };       // `at`: the 16 counts in the file

struct FileScan {
    int32_t comp, ss, se, ah, al, level, restart, t[3];
    int64_t nivl, bytes;
    size_t start;                     // first entropy-coded byte
};

struct ProgFile {
    lemon_jpeg::Frame f;              // SOF fields, quantisers as last defined, restart interval as last defined
    FileTable dc[4], ac[4];
    bool latched[3] = {false, false, false};
    uint16_t quant[3][64];
    int8_t sent[3][64];               // the Al each coefficient was last sent with, -1 = never
    FileScan scan[64];
    int32_t scans = 0, pool = 0, levels = 0;
    size_t pool_at[192];
    int64_t items = 0, spec_bytes = 0, ends_bytes = 0, data_bytes = 0;
};

// All markers from SOI to EOI (first_only: to the first SOS, for lemon_jpeg_prog_info).  The segments between the scans are
// lemon_jpeg::read_to_sos's (jpeg_entropy.hpp); a DHT table it found valid is remembered by its offset in the file.
static inline int parse(const uint8_t *d, size_t n, ProgFile &pf, LemonJpegInfo *info, bool first_only) {
    lemon_jpeg::Frame &f = pf.f;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return LEMON_JPEG_NOT_JPEG;
    if (n >= ((size_t)1 << 31)) return LEMON_JPEG_BUFFER;
    memset(pf.sent, -1, sizeof(pf.sent));
    memset(pf.quant, 0, sizeof(pf.quant));
    size_t p = 2;
    for (;;) {
        const uint8_t *s = nullptr;
        size_t sl = 0;
        bool eoi;
        const int hrc = lemon_jpeg::read_to_sos(d, n, p, f, true, pf.scans > 0, [&pf](int tc, int th, const ParHuff &, size_t at) {
            FileTable &t = tc ? pf.ac[th] : pf.dc[th];
            t.defined = true; t.at = at; t.pool = -1;
        }, s, sl, eoi);
        if (hrc != LEMON_JPEG_OK) return hrc;
        if (eoi) break;
        if (pf.scans == 0) {
            const int rc = lemon_jpeg::frame_checks(f, info);
            if (rc != LEMON_JPEG_OK) return rc;
        }
        if (pf.scans == 64) return LEMON_JPEG_SCAN;
        const int ns = sl >= 1 ? s[0] : 0;
        if ((ns != 1 && ns != f.nc) || sl != (size_t)(4 + 2 * ns)) return LEMON_JPEG_SCAN;
        FileScan &sc = pf.scan[pf.scans];
        int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
        if (ns == 1) {
            sc.comp = -1;
            for (int c = 0; c < f.nc; ++c)
                if (s[1] == f.id[c]) { sc.comp = c; break; }
            if (sc.comp < 0) return LEMON_JPEG_SCAN;
            td[0] = s[2] >> 4; ta[0] = s[2] & 15;
        } else {
            sc.comp = -1;
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != f.id[c]) return LEMON_JPEG_SCAN;
                td[c] = s[2 + 2 * c] >> 4; ta[c] = s[2 + 2 * c] & 15;
            }
        }
        for (int c = 0; c < ns; ++c)
            if (td[c] > 3 || ta[c] > 3) return LEMON_JPEG_TABLE;
        sc.ss = s[1 + 2 * ns]; sc.se = s[2 + 2 * ns]; sc.ah = s[3 + 2 * ns] >> 4; sc.al = s[3 + 2 * ns] & 15;
        if (sc.ss == 0 ? sc.se != 0 : (sc.se < sc.ss || sc.se > 63 || ns != 1)) return LEMON_JPEG_SCAN;
        if ((sc.ah != 0 && sc.al != sc.ah - 1) || sc.al > 13) return LEMON_JPEG_SCAN;
        for (int j = 0; j < ns; ++j) {
            const int c = ns == 1 ? sc.comp : j;
            if (sc.ss > 0 && pf.sent[c][0] < 0) return LEMON_JPEG_SCAN;
            for (int k = sc.ss; k <= sc.se; ++k) {
                if (sc.ah == 0 ? pf.sent[c][k] >= 0 : pf.sent[c][k] != sc.ah) return LEMON_JPEG_SCAN;
                pf.sent[c][k] = (int8_t)sc.al;
            }
            if (!pf.latched[c]) {
                if (!f.q_defined[f.tq[c]]) return LEMON_JPEG_TABLE;
                memcpy(pf.quant[c], f.q[f.tq[c]], 128);
                pf.latched[c] = true;
            }
        }
        sc.t[0] = sc.t[1] = sc.t[2] = -1;
        if (!(sc.ss == 0 && sc.ah != 0))
            for (int j = 0; j < ns; ++j) {
                FileTable &t = sc.ss == 0 ? pf.dc[td[j]] : pf.ac[ta[j]];
                if (!t.defined) return LEMON_JPEG_TABLE;
                if (t.pool < 0) {
                    if (pf.pool == 192) return LEMON_JPEG_TABLE;
                    int total = 0;
                    for (int l = 0; l < 16; ++l) total += d[t.at + l];
                    pf.spec_bytes += 16 + total;
                    pf.pool_at[pf.pool] = t.at;
                    t.pool = pf.pool++;
                }
                sc.t[j] = t.pool;
            }
        if (ns == 1 && f.nc == 1) sc.comp = 0;
        sc.level = 0;
        for (int e = 0; e < pf.scans; ++e) {
            const FileScan &b = pf.scan[e];
            if ((sc.comp < 0 || b.comp < 0 || sc.comp == b.comp) && sc.ss <= b.se && b.ss <= sc.se && b.level + 1 > sc.level)
                sc.level = b.level + 1;
        }
        if (sc.level + 1 > pf.levels) pf.levels = sc.level + 1;
        int64_t mcus = (int64_t)info->mcus_x * info->mcus_y;
        if (sc.comp >= 0 && f.nc == 3) {
            const int32_t cw = sc.comp == 0 ? f.w : (f.w + info->hs - 1) / info->hs, ch = sc.comp == 0 ? f.h : (f.h + info->vs - 1) / info->vs;
            mcus = (int64_t)((cw + 7) / 8) * ((ch + 7) / 8);
        } else if (f.nc == 1) {
            mcus = (int64_t)((f.w + 7) / 8) * ((f.h + 7) / 8);
        }
        sc.restart = f.restart;
        sc.nivl = sc.restart ? (mcus + sc.restart - 1) / sc.restart : 1;
        sc.start = p;
        ++pf.scans;
        if (first_only) {
            memcpy(info->quant, pf.quant, sizeof(pf.quant));
            return LEMON_JPEG_OK;
        }
        const int rc = lemon_jpeg_par::walk_scan<false>(d, n, p, sc.restart, sc.nivl, nullptr, 0, [](int64_t, int64_t) {}, sc.bytes);
        if (rc != LEMON_JPEG_OK) return rc;
        pf.items += (sc.nivl + LEMON_JPEG_PROG_GROUP - 1) / LEMON_JPEG_PROG_GROUP;
        pf.data_bytes += sc.bytes;
        if (sc.nivl > 1) pf.ends_bytes += 4 * sc.nivl;
    }
    for (int c = 0; c < f.nc; ++c)
        for (int k = 0; k < 64; ++k)
            if (pf.sent[c][k] != 0) return LEMON_JPEG_PROGRESSION;
    memcpy(info->quant, pf.quant, sizeof(pf.quant));
    return LEMON_JPEG_OK;
}

// The packet of a parsed file.
static inline int pack(const uint8_t *d, size_t n, const ProgFile &pf, const LemonJpegInfo *info, uint8_t *pkt, int64_t cap, int64_t *packet_bytes) {
    auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
    const int64_t pool_off = kScanOff + 4 * kScanInts * (int64_t)pf.scans;
    const int64_t spec_off = pool_off + 4 * (int64_t)pf.pool;
    const int64_t ends_off = up(spec_off + pf.spec_bytes);
    const int64_t data_off = up(ends_off + pf.ends_bytes);
    const int64_t total = up(data_off + pf.data_bytes);
    if (!pkt || total > cap) return LEMON_JPEG_BUFFER;
    memset(pkt, 0, (size_t)data_off);
    memset(pkt + data_off + pf.data_bytes, 0, (size_t)(total - data_off - pf.data_bytes));
    int32_t head[kHeadInts];
    memset(head, 0, sizeof(head));
    head[kHMagic] = kMagic; head[kHWidth] = info->width; head[kHHeight] = info->height; head[kHComponents] = info->components;
    head[kHHs] = info->hs; head[kHVs] = info->vs; head[kHScans] = pf.scans; head[kHPool] = pf.pool; head[kHItems] = (int32_t)pf.items;
    head[kHLevels] = pf.levels; head[kHPoolOff] = (int32_t)pool_off; head[kHDataOff] = (int32_t)data_off;
    head[kHDataBytes] = (int32_t)pf.data_bytes; head[kHTotal] = (int32_t)total;
    memcpy(pkt, head, sizeof(head));
    memcpy(pkt + kQuantOff, pf.quant, LEMON_JPEG_QUANT_BYTES);
    uint32_t *pool = reinterpret_cast<uint32_t *>(pkt + pool_off);
    int64_t so = spec_off;
    for (int i = 0; i < pf.pool; ++i) {
        int total_vals = 0;
        for (int l = 0; l < 16; ++l) total_vals += d[pf.pool_at[i] + l];
        memcpy(pkt + so, d + pf.pool_at[i], (size_t)(16 + total_vals));
        pool[i] = (uint32_t)so;
        so += 16 + total_vals;
    }
    int64_t eo = ends_off, dof = 0;
    for (int s = 0; s < pf.scans; ++s) {
        const FileScan &sc = pf.scan[s];
        int32_t row[kScanInts];
        memset(row, 0, sizeof(row));
        row[kSComp] = sc.comp; row[kSSs] = sc.ss; row[kSSe] = sc.se; row[kSAh] = sc.ah; row[kSAl] = sc.al; row[kSLevel] = sc.level;
        row[kSRestart] = sc.restart; row[kSIntervals] = (int32_t)sc.nivl; row[kSData] = (int32_t)dof; row[kSBytes] = (int32_t)sc.bytes;
        row[kSEnds] = sc.nivl > 1 ? (int32_t)eo : 0;
        row[kSTab0] = sc.t[0]; row[kSTab1] = sc.t[1]; row[kSTab2] = sc.t[2];
        memcpy(pkt + kScanOff + 4 * kScanInts * s, row, sizeof(row));
        size_t p = sc.start;
        int64_t bytes = 0;
        uint32_t *ends = reinterpret_cast<uint32_t *>(pkt + eo);
        const int rc = lemon_jpeg_par::walk_scan<true>(d, n, p, sc.restart, sc.nivl, pkt + data_off + dof, sc.bytes,
                                                       [ends](int64_t ivl, int64_t o) { ends[ivl] = (uint32_t)o; }, bytes);
        if (rc != LEMON_JPEG_OK || bytes != sc.bytes) return rc != LEMON_JPEG_OK ? rc : (int)LEMON_JPEG_STREAM;
        dof += sc.bytes;
        if (sc.nivl > 1) eo += 4 * sc.nivl;
    }
    if (packet_bytes) *packet_bytes = total;
    return LEMON_JPEG_OK;
}

// ---- the sequential decode of one restart interval, libjpeg's way: in place, coefficient by coefficient (natural order)
static inline int seq_interval(const ProgImage &im, const ProgScan &sc, const ParHuff *huff, const uint8_t *d, int64_t len, int64_t q0,
                               int64_t nblk, int16_t *coef) {
    using lemon_jpeg::kZigzag;
    const int64_t total = len * 8;
    const int32_t p1 = 1 << sc.al, m1 = -(1 << sc.al);
    ParBits bits = {d, len, -1, 0};
    int64_t bit = 0;
    if (sc.ss == 0 && sc.ah != 0) {
        if (nblk > total) return LEMON_JPEG_STREAM;
        for (int64_t b = 0; b < nblk; ++b, ++bit)
            if (prog_bit_at(d, len, bit)) coef[64 * prog_block_addr(im, sc, q0 + b)] |= (int16_t)p1;
        return prog_interval_end(total, bit);
    }
    if (sc.ss == 0) {
        int32_t last_dc[3] = {0, 0, 0};
        for (int64_t b = 0; b < nblk; ++b) {
            int c = 0;
            if (sc.comp < 0) {
                const int slot = (int)((q0 + b) % im.spm);
                c = slot < im.luma ? 0 : slot - im.luma + 1;
            }
            const uint32_t w = par_peek32(bits, bit);
            const int32_t e = par_symbol(w, huff[c]);
            if (e < 0 || (e & 255) > 11) return LEMON_JPEG_CODE;
            const int l = e >> 8, s = e & 255;
            bit += l + s;
            if (bit > total) return LEMON_JPEG_STREAM;
            if (s) last_dc[c] += par_extend(w, l, s);
            if (last_dc[c] < -32768 || last_dc[c] > 32767) return LEMON_JPEG_CODE;
            const int32_t v = last_dc[c] * p1;
            if (v < -32768 || v > 32767) return LEMON_JPEG_CODE;
            coef[64 * prog_block_addr(im, sc, q0 + b)] = (int16_t)v;
        }
        return prog_interval_end(total, bit);
    }
    const ParHuff &hf = huff[0];
    int32_t eobrun = 0;
    for (int64_t b = 0; b < nblk; ++b) {
        int16_t *blk = coef + 64 * prog_block_addr(im, sc, q0 + b);
        int k = sc.ss;
        if (sc.ah == 0) {                                            // decode_mcu_AC_first
            if (eobrun > 0) { --eobrun; continue; }
            for (; k <= sc.se; ++k) {
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
                    blk[kZigzag[k]] = (int16_t)v;
                } else if (r == 15) {
                    if (k + 16 > sc.se + 1) return LEMON_JPEG_CODE;
                    k += 15;
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
            continue;
        }
        if (eobrun == 0) {                                           // decode_mcu_AC_refine
            for (; k <= sc.se; ++k) {
                const uint32_t w = par_peek32(bits, bit);
                const int32_t e = par_symbol(w, hf);
                if (e < 0) return LEMON_JPEG_CODE;
                const int l = e >> 8;
                int r = (e >> 4) & 15, s = e & 15;
                if (s) {
                    if (s != 1) return LEMON_JPEG_CODE;
                    s = ((w << l) >> 31) ? p1 : m1;
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
                do {
                    int16_t *c = blk + kZigzag[k];
                    if (*c != 0) {
                        if (bit >= total) return LEMON_JPEG_STREAM;
                        if (prog_bit_at(d, len, bit) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c + m1);
                        ++bit;
                    } else if (--r < 0) {
                        break;
                    }
                    ++k;
                } while (k <= sc.se);
                if (k > sc.se) return LEMON_JPEG_CODE;               // (libjpeg would write past the band)
                if (s) blk[kZigzag[k]] = (int16_t)s;
            }
        }
        if (eobrun > 0) {
            for (; k <= sc.se; ++k) {
                int16_t *c = blk + kZigzag[k];
                if (*c == 0) continue;
                if (bit >= total) return LEMON_JPEG_STREAM;
                if (prog_bit_at(d, len, bit) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c + m1);
                ++bit;
            }
            --eobrun;
        }
    }
    return prog_interval_end(total, bit);
}

// packet -> record, sequentially; fills info->max_abs and info->exact_blocks
static inline int seq_decode(const uint8_t *pkt, int64_t bytes, uint8_t *record, int64_t record_cap, LemonJpegInfo *info) {
    ProgImage im;
    if (!prog_open(pkt, bytes, record_cap, im) || !prog_plan(im)) return LEMON_JPEG_BUFFER;
    int16_t *coef = lemon_jpeg_par::par_new_record(record, pkt, im.g);
    ParHuff *huff = new ParHuff[3];
    int st = LEMON_JPEG_OK;
    for (int level = 0; level < im.levels && st == LEMON_JPEG_OK; ++level)
        for (int s = 0; s < im.scans; ++s) {
            ProgScan sc;
            prog_scan(im, s, sc);
            if (sc.level != level) continue;
            if (!prog_scan_tables(im, sc, huff)) { if (LEMON_JPEG_TABLE > st) st = LEMON_JPEG_TABLE; continue; }
            for (int64_t t = 0; t < sc.nivl; ++t) {
                const int64_t lo = t ? sc.ends[t - 1] : 0, hi = sc.nivl > 1 ? (int64_t)sc.ends[t] : sc.bytes;
                int rc = LEMON_JPEG_STREAM;
                if (lo <= hi && hi <= sc.bytes && (t + 1 < sc.nivl || hi == sc.bytes)) {
                    const lemon_jpeg_par::McuRange r = lemon_jpeg_par::interval_mcus(sc.restart, sc.mcus, t);
                    rc = seq_interval(im, sc, huff, sc.data + lo, hi - lo, r.first * sc.spm, r.count * sc.spm, coef);
                }
                if (rc != LEMON_JPEG_OK) {                           // the rest of this work item is not decoded
                    if (rc > st) st = rc;
                    t |= LEMON_JPEG_PROG_GROUP - 1;
                }
            }
        }
    delete[] huff;
    if (st != LEMON_JPEG_OK) return st;
    int32_t max_abs = 0, exact = 0;
    const uint16_t *quant = reinterpret_cast<const uint16_t *>(record);
    for (int64_t b = 0; b < im.g.blocks; ++b) {
        const uint16_t *qt = quant + 64 * (b < im.g.n0 ? 0 : (b < im.g.n0 + im.g.nc ? 1 : 2));
        if (!lemon_jpeg::block_in_envelope(coef + 64 * b, qt, max_abs, exact)) return LEMON_JPEG_ENVELOPE;
    }
    info->max_abs = max_abs;
    info->exact_blocks = exact;
    return LEMON_JPEG_OK;
}

static inline int64_t packet_cap(int64_t n) { return n + 2 * (n / 3) + LEMON_JPEG_PROG_PACKET_BOUND; }

}  // namespace lemon_jpeg_prog

// ------------------------------------------------------------------------------------------------------- host entry points
static inline int lemon_jpeg_prog_info_impl(const uint8_t *data, int64_t n, LemonJpegInfo *info) {
    memset(info, 0, sizeof(*info));
    if (!data || n < 0) return info->status = LEMON_JPEG_NOT_JPEG;
    lemon_jpeg_prog::ProgFile *pf = new lemon_jpeg_prog::ProgFile();
    const int rc = lemon_jpeg_prog::parse(data, (size_t)n, *pf, info, true);
    delete pf;
    return info->status = rc;
}

static inline int lemon_jpeg_prog_pack_impl(const uint8_t *data, int64_t n, uint8_t *packet, int64_t cap, LemonJpegInfo *info,
                                            int64_t *packet_bytes) {
    memset(info, 0, sizeof(*info));
    if (packet_bytes) *packet_bytes = 0;
    if (!data || n < 0) return info->status = LEMON_JPEG_NOT_JPEG;
    lemon_jpeg_prog::ProgFile *pf = new lemon_jpeg_prog::ProgFile();
    int rc = lemon_jpeg_prog::parse(data, (size_t)n, *pf, info, false);
    if (rc == LEMON_JPEG_OK) rc = lemon_jpeg_prog::pack(data, (size_t)n, *pf, info, packet, cap, packet_bytes);
    delete pf;
    return info->status = rc;
}

// The whole host pass: `record` receives info->record_bytes bytes (at most `record_cap`); a declined file leaves it unspecified.
static inline int lemon_jpeg_prog_entropy_impl(const uint8_t *data, int64_t n, uint8_t *record, int64_t record_cap, LemonJpegInfo *info) {
    memset(info, 0, sizeof(*info));
    if (!data || n < 0) return info->status = LEMON_JPEG_NOT_JPEG;
    lemon_jpeg_prog::ProgFile *pf = new lemon_jpeg_prog::ProgFile();
    int rc = lemon_jpeg_prog::parse(data, (size_t)n, *pf, info, false);
    if (rc == LEMON_JPEG_OK && (!record || info->record_bytes > record_cap)) rc = LEMON_JPEG_BUFFER;
    if (rc == LEMON_JPEG_OK) {
        const int64_t cap = (lemon_jpeg_prog::packet_cap(n) + 15) & ~(int64_t)15;
        uint8_t *pkt = static_cast<uint8_t *>(aligned_alloc(16, (size_t)cap));
        int64_t bytes = 0;
        rc = pkt ? lemon_jpeg_prog::pack(data, (size_t)n, *pf, info, pkt, cap, &bytes) : (int)LEMON_JPEG_BUFFER;
        if (rc == LEMON_JPEG_OK) rc = lemon_jpeg_prog::seq_decode(pkt, bytes, record, record_cap, info);
        free(pkt);
    }
    delete pf;
    return info->status = rc;
}
