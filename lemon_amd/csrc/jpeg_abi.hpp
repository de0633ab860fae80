// jpeg_abi.hpp -- the host-only C entry points of the JPEG path (include/lemon_hip.h).  Included by exactly one translation
// unit of each library: jpeg.hip (liblemon_hip.so) and jpeg_host.cpp (liblemon_jpeg_host.so, no HIP runtime).
#pragma once
#include <vector>

#include "jpeg_entropy.hpp"
#include "jpeg_par.hpp"
#include "jpeg_prog.hpp"

extern "C" int lemon_jpeg_info(const uint8_t *data, int64_t n, LemonJpegInfo *info) {
    if (!info) return LEMON_JPEG_BUFFER;
    return lemon_jpeg_info_impl(data, n, info);
}

extern "C" int lemon_jpeg_entropy(const uint8_t *data, int64_t n, uint8_t *record, int64_t record_cap, LemonJpegInfo *info) {
    if (!info) return LEMON_JPEG_BUFFER;
    return lemon_jpeg_entropy_impl(data, n, record, record_cap, info);
}

// The workers' share of the device Huffman pass: header + the scan packet of jpeg_par.hpp.
extern "C" int lemon_jpeg_pack(const uint8_t *data, int64_t n, uint8_t *packet, int64_t packet_cap, LemonJpegInfo *info,
                               int64_t *packet_bytes) {
    if (!info) return LEMON_JPEG_BUFFER;
    return lemon_jpeg_pack_impl(data, n, packet, packet_cap, info, packet_bytes);
}

// The device's Huffman kernels (jpeg_entropy.hip) with the lanes looped on the host: packet -> record + status.  For tests and
// the sanitizer fuzzer; no product path calls it.
extern "C" int lemon_jpeg_entropy_par_host(const uint8_t *packet, int64_t packet_bytes, int32_t subseq_bytes, uint8_t *record,
                                           int64_t record_cap, int32_t *status) {
    return lemon_jpeg_entropy_par_host_impl(packet, packet_bytes, subseq_bytes, record, record_cap, status);
}

// The device's arithmetic (jpeg_core.hpp) on the host: a record -> packed uint8 RGB [h, w, 3].  For tests and for pinning the
// arithmetic against PIL where there is no GPU; no product path calls it.
extern "C" int lemon_jpeg_reconstruct_host(const uint8_t *record, int64_t record_bytes, int32_t w, int32_t h, int32_t ncomp,
                                           int32_t hs, int32_t vs, uint8_t *rgb) {
    JpegGeom g;
    if (!record || !rgb || !jpeg_geometry(w, h, ncomp, hs, vs, g)) return 1;
    if (record_bytes < LEMON_JPEG_QUANT_BYTES + 128 * g.blocks) return 1;
    const uint16_t *quant = reinterpret_cast<const uint16_t *>(record);
    const int16_t *coef = reinterpret_cast<const int16_t *>(record + LEMON_JPEG_QUANT_BYTES);
    std::vector<uint8_t> work((size_t)g.blocks * 64);
    const int64_t base[3] = {0, g.n0, g.n0 + g.nc};
    const int32_t bw[3] = {g.bw0, g.bwc, g.bwc}, bh[3] = {g.bh0, g.bhc, g.bhc};
    for (int c = 0; c < ncomp; ++c)
        for (int32_t by = 0; by < bh[c]; ++by)
            for (int32_t bx = 0; bx < bw[c]; ++bx)
                jpeg_idct_block(coef + 64 * (base[c] + (int64_t)by * bw[c] + bx), quant + 64 * c,
                                work.data() + 64 * base[c] + ((int64_t)by * 8 * bw[c] + bx) * 8, (int64_t)bw[c] * 8);
    const uint8_t *Y = work.data(), *Cb = work.data() + 64 * base[1], *Cr = work.data() + 64 * base[2];
    for (int32_t y = 0; y < h; ++y)
        for (int32_t x = 0; x < w; ++x) {
            uint8_t *o = rgb + ((int64_t)y * w + x) * 3;
            const int32_t l = Y[(int64_t)y * g.bw0 * 8 + x];
            if (ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)l; continue; }
            jpeg_ycc_rgb(l, jpeg_chroma_at(Cb, (int64_t)g.bwc * 8, g.dwc, g.dhc, hs, vs, x, y),
                         jpeg_chroma_at(Cr, (int64_t)g.bwc * 8, g.dwc, g.dhc, hs, vs, x, y), o);
        }
    return 0;
}

// The progressive forms (jpeg_prog.hpp, jpeg_prog_par.hpp): SOF2 only.
extern "C" int lemon_jpeg_prog_info(const uint8_t *data, int64_t n, LemonJpegInfo *info) {
    if (!info) return LEMON_JPEG_BUFFER;
    return lemon_jpeg_prog_info_impl(data, n, info);
}

extern "C" int lemon_jpeg_prog_entropy(const uint8_t *data, int64_t n, uint8_t *record, int64_t record_cap, LemonJpegInfo *info) {
    if (!info) return LEMON_JPEG_BUFFER;
    return lemon_jpeg_prog_entropy_impl(data, n, record, record_cap, info);
}

extern "C" int lemon_jpeg_prog_pack(const uint8_t *data, int64_t n, uint8_t *packet, int64_t packet_cap, LemonJpegInfo *info,
                                    int64_t *packet_bytes) {
    if (!info) return LEMON_JPEG_BUFFER;
    return lemon_jpeg_prog_pack_impl(data, n, packet, packet_cap, info, packet_bytes);
}

extern "C" int lemon_jpeg_prog_entropy_par_host(const uint8_t *packet, int64_t packet_bytes, uint8_t *record, int64_t record_cap,
                                                int32_t *status) {
    return lemon_jpeg_prog_entropy_par_host_impl(packet, packet_bytes, record, record_cap, status);
}
