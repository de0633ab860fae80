// png_abi.hpp -- the host-only C entry points of the PNG path (include/lemon_hip.h).  Included by exactly one translation unit
// of each library: png.hip (liblemon_hip.so) and jpeg_host.cpp (liblemon_jpeg_host.so, no HIP runtime).
#pragma once
#include <vector>

#include "png_core.hpp"
#include "png_inflate_core.hpp"

// The device inflate's schedule (png_inflate_core.hpp) with the lanes looped on the host: a zlib stream -> the `want` bytes of
// filtered scanlines + status.  For tests, the fuzzer's cross-check and tools; no product path calls it.
extern "C" int lemon_png_inflate_host(const uint8_t *z, int64_t n, uint8_t *rows, int64_t want, int32_t *status) {
    return lemon_png_inflate_host_impl(z, n, rows, want, status);
}

extern "C" int lemon_png_info(const uint8_t *data, int64_t n, LemonPngInfo *info) {
    if (!info) return LEMON_PNG_BUFFER;
    return lemon_png_info_impl(data, n, info);
}

extern "C" int64_t lemon_png_idat(const uint8_t *data, int64_t n, uint8_t *out, int64_t cap) {
    return lemon_png_idat_impl(data, n, out, cap);
}

// The device's schedule and arithmetic (png_core.hpp) on the host: a record -> packed uint8 RGB [h, w, 3] + status.  For tests
// and for pinning the arithmetic against PIL where there is no GPU; no product path calls it.
extern "C" int lemon_png_decode_host(const uint8_t *record, int64_t record_bytes, int32_t h, int32_t w, int32_t colour_type,
                                     int32_t plte_count, uint8_t *rgb, int32_t *status) {
    if (w < 1 || w > LEMON_PNG_MAX_DIM) return 1;
    std::vector<uint32_t> work((size_t)w);
    return lemon_png_decode_host_impl(record, record_bytes, h, w, colour_type, plte_count, rgb, work.data(), status);
}
