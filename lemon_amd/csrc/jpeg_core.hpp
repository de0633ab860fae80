// jpeg_core.hpp -- the integer arithmetic that turns quantised DCT coefficients of a baseline JPEG into RGB pixels, exactly as
// libjpeg-turbo's defaults do it (JDCT_ISLOW, fancy upsampling, the fixed-point YCbCr tables): what PIL's
// `Image.open(p).convert("RGB")` returns.  `__host__ __device__`: jpeg.hip runs these functions per block / per pixel on the
// GPU, and the host build (lemon_jpeg_reconstruct_host, liblemon_jpeg_host.so) pins the same functions against PIL on a machine
// without a GPU.  All arithmetic is 32-bit integer; `>>` is an arithmetic shift.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LEMON_JPEG_HD __host__ __device__ __forceinline__
#else
#define LEMON_JPEG_HD static inline
#endif

// ---- geometry of an accepted image: component 0 sampled hs x vs (1x1, 2x1 or 2x2), components 1 and 2 sampled 1x1
struct JpegGeom {
    int32_t bw0, bh0;        // luma block grid (MCU-padded)
    int32_t bwc, bhc;        // chroma block grid (= the MCU grid); 0 with one component
    int32_t dwc, dhc;        // chroma samples that exist: ceil(w / hs), ceil(h / vs)
    int64_t n0, nc;          // blocks of the luma plane, of one chroma plane
    int64_t blocks;          // n0 + 2 nc
};

#define LEMON_JPEG_QUANT_BYTES 384       // three tables of 64 uint16, natural order, at the head of every record
#define LEMON_JPEG_MAX_DIM 65535

LEMON_JPEG_HD bool jpeg_geometry(int64_t w, int64_t h, int64_t ncomp, int64_t hs, int64_t vs, JpegGeom &g) {
    if (w < 1 || h < 1 || w > LEMON_JPEG_MAX_DIM || h > LEMON_JPEG_MAX_DIM) return false;
    if (ncomp != 1 && ncomp != 3) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    if (ncomp == 1 && (hs != 1 || vs != 1)) return false;
    const int32_t mx = (int32_t)((w + 8 * hs - 1) / (8 * hs)), my = (int32_t)((h + 8 * vs - 1) / (8 * vs));
    g.bw0 = mx * (int32_t)hs; g.bh0 = my * (int32_t)vs;
    g.bwc = ncomp == 3 ? mx : 0; g.bhc = ncomp == 3 ? my : 0;
    g.dwc = (int32_t)((w + hs - 1) / hs); g.dhc = (int32_t)((h + vs - 1) / vs);
    g.n0 = (int64_t)g.bw0 * g.bh0; g.nc = (int64_t)g.bwc * g.bhc;
    g.blocks = g.n0 + 2 * g.nc;
    return true;
}

// Record block (planar: luma plane, then the two chroma planes) of block `slot` of interleaved MCU m: the luma blocks of the
// MCU row by row (hs x vs of them, `luma` in all), then Cb, then Cr; mx MCUs per row.  With one component hs = vs = luma = 1.
// Callers: lemon_jpeg_par::par_block_addr (jpeg_par.hpp), lemon_jpeg_prog::prog_block_addr (jpeg_prog_par.hpp).
LEMON_JPEG_HD int64_t jpeg_mcu_block_addr(const JpegGeom &g, int32_t mx, int hs, int vs, int luma, int64_t m, int slot) {
    const int64_t yy = m / mx, xx = m - yy * mx;
    if (slot >= luma) return (slot == luma ? g.n0 : g.n0 + g.nc) + yy * g.bwc + xx;
    const int by = slot / hs, bx = slot - by * hs;
    return (yy * vs + by) * g.bw0 + xx * hs + bx;
}

// ---- jidctint: CONST_BITS = 13, PASS1_BITS = 2.  One 1-D step, outputs before the rounding shift.
LEMON_JPEG_HD void jpeg_idct_1d(int32_t in0, int32_t in1, int32_t in2, int32_t in3, int32_t in4, int32_t in5, int32_t in6, int32_t in7,
                                int32_t out[8]) {
    int32_t z1 = (in2 + in6) * 4433;
    const int32_t t2 = z1 - in6 * 15137;
    const int32_t t3 = z1 + in2 * 6270;
    const int32_t t0 = (int32_t)((uint32_t)(in0 + in4) << 13);
    const int32_t t1 = (int32_t)((uint32_t)(in0 - in4) << 13);
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int32_t a0 = in7, a1 = in5, a2 = in3, a3 = in1;
    z1 = a0 + a3;
    int32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int32_t z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 = -z1 * 7373;
    z2 = -z2 * 20995;
    z3 = -z3 * 16069 + z5;
    z4 = -z4 * 3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    out[0] = t10 + a3; out[7] = t10 - a3;
    out[1] = t11 + a2; out[6] = t11 - a2;
    out[2] = t12 + a1; out[5] = t12 - a1;
    out[3] = t13 + a0; out[4] = t13 - a0;
}

// pass 1 on one column of dequantised coefficients -> 8 workspace values (rows 0..7 of that column)
LEMON_JPEG_HD void jpeg_idct_col(const int32_t d[8], int32_t ws[8]) {
    jpeg_idct_1d(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], ws);
    for (int k = 0; k < 8; ++k) ws[k] = (ws[k] + (1 << 10)) >> 11;
}

// pass 2 on one row of the workspace -> 8 values before the range limit
LEMON_JPEG_HD void jpeg_idct_row(const int32_t ws[8], int32_t x[8]) {
    jpeg_idct_1d(ws[0], ws[1], ws[2], ws[3], ws[4], ws[5], ws[6], ws[7], x);
    for (int k = 0; k < 8; ++k) x[k] = (x[k] + (1 << 17)) >> 18;
}

// libjpeg's masked range-limit table: the low 10 bits read as a signed number, plus 128, clamped to a byte
LEMON_JPEG_HD uint8_t jpeg_range_limit(int32_t x) {
    x &= 1023;
    if (x >= 512) x -= 1024;
    x += 128;
    return (uint8_t)(x < 0 ? 0 : (x > 255 ? 255 : x));
}

// one block: quantised coefficients (natural order) and its quantiser -> 64 samples, row stride `stride`
LEMON_JPEG_HD void jpeg_idct_block(const int16_t *coef, const uint16_t *quant, uint8_t *out, int64_t stride) {
    int32_t ws[64];
    for (int c = 0; c < 8; ++c) {
        int32_t d[8], o[8];
        for (int k = 0; k < 8; ++k) d[k] = (int32_t)coef[k * 8 + c] * (int32_t)quant[k * 8 + c];
        jpeg_idct_col(d, o);
        for (int k = 0; k < 8; ++k) ws[k * 8 + c] = o[k];
    }
    for (int r = 0; r < 8; ++r) {
        int32_t x[8];
        jpeg_idct_row(ws + r * 8, x);
        for (int k = 0; k < 8; ++k) out[r * stride + k] = jpeg_range_limit(x[k]);
    }
}

// The exact form of the envelope check (jpeg_entropy.hpp, "Envelope"): true when every dequantised coefficient and every pass-1
// result of the block is at most 16383 in magnitude and every pass-2 result lies in [-512, 511].
LEMON_JPEG_HD bool jpeg_block_in_envelope(const int16_t *coef, const uint16_t *quant) {
    int32_t ws[64];
    for (int c = 0; c < 8; ++c) {
        int32_t d[8], o[8];
        for (int k = 0; k < 8; ++k) {
            d[k] = (int32_t)coef[k * 8 + c] * (int32_t)quant[k * 8 + c];
            if (d[k] > 16383 || d[k] < -16383) return false;
        }
        jpeg_idct_col(d, o);
        for (int k = 0; k < 8; ++k) {
            if (o[k] > 16383 || o[k] < -16383) return false;
            ws[k * 8 + c] = o[k];
        }
    }
    for (int r = 0; r < 8; ++r) {
        int32_t x[8];
        jpeg_idct_row(ws + r * 8, x);
        for (int k = 0; k < 8; ++k)
            if (x[k] < -512 || x[k] > 511) return false;
    }
    return true;
}

// ---- fancy upsampling: chroma sample of output pixel (x, y) from a plane of dw x dh real samples
LEMON_JPEG_HD int32_t jpeg_chroma_at(const uint8_t *p, int64_t stride, int32_t dw, int32_t dh, int hs, int vs, int32_t x, int32_t y) {
    if (hs == 1) return p[(int64_t)y * stride + x];
    const int32_t cx = x >> 1;
    if (vs == 1) {
        const uint8_t *row = p + (int64_t)y * stride;
        if (dw <= 2) return row[cx];
        if (x & 1) return cx == dw - 1 ? row[cx] : (3 * row[cx] + row[cx + 1] + 2) >> 2;
        return cx == 0 ? row[cx] : (3 * row[cx] + row[cx - 1] + 1) >> 2;
    }
    const int32_t cy = y >> 1;
    const uint8_t *r0 = p + (int64_t)cy * stride;
    if (dw <= 2) return r0[cx];
    int32_t ny = (y & 1) ? cy + 1 : cy - 1;
    ny = ny < 0 ? 0 : (ny > dh - 1 ? dh - 1 : ny);
    const uint8_t *r1 = p + (int64_t)ny * stride;
    const int32_t cs = 3 * r0[cx] + r1[cx];
    if (x & 1) {
        if (cx == dw - 1) return (4 * cs + 7) >> 4;
        return (3 * cs + (3 * r0[cx + 1] + r1[cx + 1]) + 7) >> 4;
    }
    if (cx == 0) return (4 * cs + 8) >> 4;
    return (3 * cs + (3 * r0[cx - 1] + r1[cx - 1]) + 8) >> 4;
}

LEMON_JPEG_HD uint8_t jpeg_clamp8(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// YCbCr -> RGB with libjpeg's 16-bit fixed-point tables
LEMON_JPEG_HD void jpeg_ycc_rgb(int32_t y, int32_t cb, int32_t cr, uint8_t rgb[3]) {
    cb -= 128; cr -= 128;
    rgb[0] = jpeg_clamp8(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = jpeg_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = jpeg_clamp8(y + ((116130 * cb + 32768) >> 16));
}
