// png_core.hpp -- the PNG path (lib/datasets/dataloader.py:177-184 opens a PNG with `Image.open(p).convert("RGB")`): the chunk
// parser the decode workers run, and the arithmetic of the device half (png.hip): scanline reconstruction and the expansion to
// RGB, as functions of one lane's state, so that the kernel and the host loop (lemon_png_decode_host) execute the same code.
// Plain C++17, header-only, no HIP: also compiled with g++ into liblemon_jpeg_host.so (loaded by the decode workers) and
// under AddressSanitizer / UBSan for the fuzzer (tests/native/png_fuzz.cpp).
//
// The input is untrusted: every read is checked against the end of the buffer, the CRC-32 of every chunk is verified (table
// below: no libz dependency; the workers inflate with Python's zlib), and anything outside the envelope is DECLINED with a
// status (the caller then decodes with PIL), never guessed at.  Envelope: 8-bit samples; colour type 0, 2, 3 (PLTE of 1 .. 256
// entries before IDAT), 4 or 6; not interlaced; compression and filter method 0; consecutive IDAT chunks; IEND present; no
// acTL; at most 65535 x 65535 and PIL's own pixel limit.  tRNS, gAMA, iCCP and every other ancillary chunk are skipped (their
// CRC still checked), as convert("RGB") ignores them.
//
// Record of an accepted file (LemonPngInfo::record_bytes = 1024 + h * (stride + 1), stride = w * channels):
//   uint8 palette[256][4]           R, G, B, 0 of each PLTE entry; zeros beyond the PLTE count and for non-palette files
//   uint8 rows[h][1 + stride]       the filtered scanlines exactly as inflated, each row behind its filter-type byte
// This is the interface a device inflate would write to.
//
// Reconstruction order (png.hip): byte (r, x) needs (r, x - bpp), (r - 1, x) and (r - 1, x - bpp); Average and Paeth are not
// linear, so the rows of a band of 64 run as a diagonal wavefront: lane = row, each lane one PIXEL behind the lane above.  At
// step t lane l reconstructs pixel x = t - l; the pixel above it is what lane l - 1 produced at step t - 1 (one lane shift),
// the pixel above-left what it received the step before.  Lane 0 reads the row above from the previous band's last row, which
// lane 63 wrote to the work buffer as one uint32 per pixel.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/lemon_hip.h"

#if defined(__HIPCC__)
#define LEMON_PNG_HD __host__ __device__ __forceinline__
#else
#define LEMON_PNG_HD static inline
#endif

enum LemonPngStatus {
    LEMON_PNG_OK = 0,
    LEMON_PNG_NOT_PNG = 1,            // no PNG signature
    LEMON_PNG_TRUNCATED = 2,          // a chunk runs past the end of the file, or the file ends before IEND
    LEMON_PNG_CRC = 3,                // a chunk's CRC-32 does not match
    LEMON_PNG_HEADER = 4,             // IHDR missing, malformed or with values the standard does not allow; unknown critical chunk
    LEMON_PNG_DEPTH = 5,              // a valid bit depth other than 8 (1, 2, 4, 16)
    LEMON_PNG_INTERLACE = 6,          // Adam7
    LEMON_PNG_PALETTE = 7,            // colour type 3 without PLTE; a PLTE of no, too many or a fractional number of entries
    LEMON_PNG_CHUNK_ORDER = 8,        // PLTE after IDAT, IDAT chunks not consecutive, no IDAT, a second IHDR
    LEMON_PNG_ANIMATED = 9,           // acTL
    LEMON_PNG_DIMENSION = 10,         // a dimension of 0, above 65535, or more pixels than PIL opens without complaint
    LEMON_PNG_BUFFER = 11,            // the caller's buffer is too small; device: a descriptor leaves its buffer (nothing read or written)
    LEMON_PNG_STREAM = 12,            // the zlib stream does not yield exactly h * (stride + 1) bytes and end there (png_host.py)
    // 13 = LEMON_PNG_FILTER, 14 = LEMON_PNG_INDEX: the device verdicts (include/lemon_hip.h)
};

#define LEMON_PNG_MAX_DIM 65535
#define LEMON_PNG_MAX_PIXELS 89478485      // PIL's Image.MAX_IMAGE_PIXELS: above it PIL warns or raises, so PIL decides

namespace lemon_png {

struct CrcTable {                     // slicing by 8: t[k][i] = the CRC of byte i followed by k zero bytes
    uint32_t t[8][256];
    constexpr CrcTable() : t() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (int k = 1; k < 8; ++k)
            for (uint32_t i = 0; i < 256; ++i) t[k][i] = t[0][t[k - 1][i] & 255] ^ (t[k - 1][i] >> 8);
    }
};
static constexpr CrcTable kCrc{};

static inline uint32_t crc32(const uint8_t *p, int64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (; n >= 8; n -= 8, p += 8) {
        const uint32_t a = c ^ ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
        const uint32_t b = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
        c = kCrc.t[7][a & 255] ^ kCrc.t[6][(a >> 8) & 255] ^ kCrc.t[5][(a >> 16) & 255] ^ kCrc.t[4][a >> 24] ^
            kCrc.t[3][b & 255] ^ kCrc.t[2][(b >> 8) & 255] ^ kCrc.t[1][(b >> 16) & 255] ^ kCrc.t[0][b >> 24];
    }
    for (int64_t i = 0; i < n; ++i) c = kCrc.t[0][(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

static inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

static inline bool is_type(const uint8_t *p, const char *name) { return memcmp(p, name, 4) == 0; }

// The chunk walk.  `idat_out` (may be null): receives the concatenated IDAT payload, up to idat_cap bytes.
static inline int walk(const uint8_t *d, int64_t n, LemonPngInfo *info, uint8_t *idat_out, int64_t idat_cap) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    memset(info, 0, sizeof(*info));
    info->plte_offset = info->idat_offset = -1;
    if (!d || n <= 0) return info->status = LEMON_PNG_NOT_PNG;
    if (n < 8) return info->status = memcmp(d, sig, (size_t)n) == 0 ? LEMON_PNG_TRUNCATED : LEMON_PNG_NOT_PNG;
    if (memcmp(d, sig, 8) != 0) return info->status = LEMON_PNG_NOT_PNG;
    int64_t pos = 8, copied = 0;
    bool have_ihdr = false, in_idat = false, idat_done = false, have_plte = false;
    for (;;) {
        if (n - pos < 12) return info->status = LEMON_PNG_TRUNCATED;          // (length, type, CRC; also: no IEND)
        const int64_t len = be32(d + pos);
        const uint8_t *type = d + pos + 4;
        if (len > n - pos - 12) return info->status = LEMON_PNG_TRUNCATED;
        const uint8_t *body = d + pos + 8;
        if (crc32(type, 4 + len) != be32(body + len)) return info->status = LEMON_PNG_CRC;
        pos += 12 + len;
        if (!have_ihdr) {
            if (!is_type(type, "IHDR") || len != 13) return info->status = LEMON_PNG_HEADER;
            have_ihdr = true;
            const uint32_t w = be32(body), h = be32(body + 4);
            const int depth = body[8], ct = body[9];
            if (w == 0 || h == 0 || w > LEMON_PNG_MAX_DIM || h > LEMON_PNG_MAX_DIM || (int64_t)w * h > LEMON_PNG_MAX_PIXELS)
                return info->status = LEMON_PNG_DIMENSION;
            const bool pow2 = depth == 1 || depth == 2 || depth == 4 || depth == 8;
            const bool allowed = ct == 0 ? (pow2 || depth == 16) : ct == 3 ? pow2 : (ct == 2 || ct == 4 || ct == 6) ? (depth == 8 || depth == 16) : false;
            if (!allowed) return info->status = LEMON_PNG_HEADER;
            if (depth != 8) return info->status = LEMON_PNG_DEPTH;
            if (body[10] != 0 || body[11] != 0 || body[12] > 1) return info->status = LEMON_PNG_HEADER;
            if (body[12] == 1) return info->status = LEMON_PNG_INTERLACE;
            info->width = (int32_t)w; info->height = (int32_t)h; info->colour_type = ct;
            info->channels = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : 4;
            info->stride = (int64_t)w * info->channels;
            info->record_bytes = 1024 + (int64_t)h * (info->stride + 1);
            continue;
        }
        const bool idat = is_type(type, "IDAT");
        if (in_idat && !idat) { in_idat = false; idat_done = true; }
        if (idat) {
            if (idat_done) return info->status = LEMON_PNG_CHUNK_ORDER;
            if (!in_idat) info->idat_offset = body - d;
            in_idat = true;
            if (idat_out) {
                if (len > idat_cap - copied) return info->status = LEMON_PNG_BUFFER;
                if (len) memcpy(idat_out + copied, body, (size_t)len);
                copied += len;
            }
            info->idat_spans += 1;
            info->idat_bytes += len;
        } else if (is_type(type, "IEND")) {
            if (!info->idat_spans) return info->status = LEMON_PNG_CHUNK_ORDER;
            if (info->colour_type == 3 && !have_plte) return info->status = LEMON_PNG_PALETTE;     // (a PLTE behind IDAT: CHUNK_ORDER above)
            return info->status = LEMON_PNG_OK;
        } else if (is_type(type, "IHDR")) {
            return info->status = LEMON_PNG_CHUNK_ORDER;
        } else if (is_type(type, "PLTE")) {
            if (info->idat_spans) return info->status = LEMON_PNG_CHUNK_ORDER;
            if (have_plte || len == 0 || len % 3 != 0 || len > 768 || info->colour_type == 0 || info->colour_type == 4)
                return info->status = LEMON_PNG_PALETTE;
            have_plte = true;
            if (info->colour_type == 3) { info->plte_count = (int32_t)(len / 3); info->plte_offset = body - d; }
        } else if (is_type(type, "acTL")) {
            return info->status = LEMON_PNG_ANIMATED;
        } else if (!(type[0] & 0x20)) {
            return info->status = LEMON_PNG_HEADER;                              // a critical chunk this parser does not know
        }
    }
}

}  // namespace lemon_png

static inline int lemon_png_info_impl(const uint8_t *data, int64_t n, LemonPngInfo *info) {
    return lemon_png::walk(data, n, info, nullptr, 0);
}

// -> bytes copied (the file's idat_bytes), or -status
static inline int64_t lemon_png_idat_impl(const uint8_t *data, int64_t n, uint8_t *out, int64_t cap) {
    LemonPngInfo info;
    if (!out || cap < 0) return -(int64_t)LEMON_PNG_BUFFER;
    const int st = lemon_png::walk(data, n, &info, out, cap);
    return st == LEMON_PNG_OK ? info.idat_bytes : -(int64_t)st;
}

// ---- the device half's arithmetic.  A pixel is one uint32: byte k = channel k (bytes at and above `bpp` are zero).

#define LEMON_PNG_BAND 64              // rows of a band = lanes of a wave

LEMON_PNG_HD int png_channels(int64_t colour_type) {
    return colour_type == 0 ? 1 : colour_type == 2 ? 3 : colour_type == 3 ? 1 : colour_type == 4 ? 2 : colour_type == 6 ? 4 : 0;
}

LEMON_PNG_HD int32_t png_paeth(int32_t a, int32_t b, int32_t c) {
    const int32_t p = a + b - c;
    const int32_t pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

struct PngLane {
    uint32_t cur;                      // the pixel this lane reconstructed last (left of the next one)
    uint32_t above;                    // the pixel above `cur` (above-left of the next one)
};

// One step of one lane: filtered pixel `raw` of a row of filter type ft (0 .. 4), `up` the reconstructed pixel above it (0 in
// the first row), first = the row's first pixel.  Arithmetic mod 256 per byte, bpp = channels.
template <int BPP>
LEMON_PNG_HD uint32_t png_lane_step(PngLane &s, int ft, uint32_t raw, uint32_t up, bool first) {
    const uint32_t left = first ? 0u : s.cur, upleft = first ? 0u : s.above;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < BPP; ++k) {
        const int32_t a = (left >> (8 * k)) & 255, b = (up >> (8 * k)) & 255, c = (upleft >> (8 * k)) & 255;
        const int32_t pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : ft == 4 ? png_paeth(a, b, c) : 0;
        out |= ((((raw >> (8 * k)) & 255) + (uint32_t)pred) & 255u) << (8 * k);
    }
    s.cur = out;
    s.above = up;
    return out;
}

// convert("RGB") of one reconstructed pixel -> R | G << 8 | B << 16.  `pal`: the record's 256 palette words.
LEMON_PNG_HD uint32_t png_rgb(uint32_t px, int colour_type, const uint32_t *pal, int plte_count, bool &index_bad) {
    if (colour_type == 2 || colour_type == 6) return px & 0xFFFFFFu;
    const uint32_t g = px & 255u;
    if (colour_type == 3) {
        if ((int)g >= plte_count) { index_bad = true; return 0; }
        return pal[g] & 0xFFFFFFu;
    }
    return g * 0x010101u;
}

// The kernel's schedule with the lanes looped on the host: bands in order, steps t = 0 .. w + rows - 2, lane l at pixel t - l.
// Lanes run from the last to the first so that lane l still sees what lane l - 1 held after step t - 1 (the kernel's shift).
template <int BPP>
static inline int png_decode_host_t(const uint8_t *rec, int32_t h, int32_t w, int ct, int plte, uint8_t *rgb, uint32_t *work) {
    uint32_t pal[256];
    memcpy(pal, rec, 1024);
    const int64_t pitch = (int64_t)w * BPP + 1;
    bool index_bad = false;
    for (int32_t r0 = 0; r0 < h; r0 += LEMON_PNG_BAND) {
        const int rows = h - r0 < LEMON_PNG_BAND ? h - r0 : LEMON_PNG_BAND;
        PngLane lane[LEMON_PNG_BAND];
        int ft[LEMON_PNG_BAND];
        for (int l = 0; l < rows; ++l) {
            lane[l].cur = lane[l].above = 0;
            ft[l] = rec[1024 + (r0 + l) * pitch];
            if (ft[l] > 4) return LEMON_PNG_FILTER;
        }
        for (int64_t t = 0; t < (int64_t)w + rows - 1; ++t)
            for (int l = rows - 1; l >= 0; --l) {
                const int64_t x = t - l;
                if (x < 0 || x >= w) continue;
                const uint8_t *p = rec + 1024 + (r0 + l) * pitch + 1 + x * BPP;
                uint32_t raw = 0;
                for (int k = 0; k < BPP; ++k) raw |= (uint32_t)p[k] << (8 * k);
                const uint32_t up = l > 0 ? lane[l - 1].cur : (r0 > 0 ? work[x] : 0u);
                const uint32_t px = png_lane_step<BPP>(lane[l], ft[l], raw, up, x == 0);
                if (l == LEMON_PNG_BAND - 1) work[x] = px;
                const uint32_t c = png_rgb(px, ct, pal, plte, index_bad);
                uint8_t *o = rgb + ((int64_t)(r0 + l) * w + x) * 3;
                o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
            }
    }
    return index_bad ? LEMON_PNG_INDEX : LEMON_PNG_OK;
}

// record -> uint8 RGB [h, w, 3] and a status (0, LEMON_PNG_FILTER: rgb unspecified, LEMON_PNG_INDEX).  `work`: w uint32.
// Returns 0 unless an argument is invalid (then nothing is read or written).
static inline int lemon_png_decode_host_impl(const uint8_t *rec, int64_t rec_bytes, int32_t h, int32_t w, int32_t ct, int32_t plte,
                                             uint8_t *rgb, uint32_t *work, int32_t *status) {
    const int bpp = png_channels(ct);
    if (!rec || !rgb || !work || !status || !bpp || w < 1 || h < 1 || w > LEMON_PNG_MAX_DIM || h > LEMON_PNG_MAX_DIM) return 1;
    if (plte < 0 || plte > 256 || rec_bytes < 1024 + (int64_t)h * ((int64_t)w * bpp + 1)) return 1;
    *status = bpp == 1 ? png_decode_host_t<1>(rec, h, w, ct, plte, rgb, work)
            : bpp == 2 ? png_decode_host_t<2>(rec, h, w, ct, plte, rgb, work)
            : bpp == 3 ? png_decode_host_t<3>(rec, h, w, ct, plte, rgb, work)
                       : png_decode_host_t<4>(rec, h, w, ct, plte, rgb, work);
    return 0;
}
