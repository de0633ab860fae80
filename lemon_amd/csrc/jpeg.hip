// jpeg.hip -- the device half of the baseline JPEG decode (lemon_jpeg_decode, include/lemon_hip.h): the host's entropy pass
// (jpeg_entropy.hpp) delivers quantised coefficient blocks, and two kernels turn a batch of them into packed uint8 RGB images,
// the layout RaggedImages / lemon_preprocess_ragged read.  The arithmetic is jpeg_core.hpp (libjpeg-turbo's JDCT_ISLOW, fancy
// upsampling and YCbCr tables, bit for bit what PIL returns).
//   k_jpeg_idct   dequantise + 8x8 inverse DCT: 32 consecutive blocks of one image per workgroup.  Their 4 KB of coefficients
//                 are read as one coalesced 16-byte-per-lane load into LDS; pass 1 runs one (block, column) per lane, pass 2
//                 one (block, row) per lane with the 32 blocks across the lanes, so that 32 lanes store 256 contiguous bytes
//                 of a component plane row.
//   k_jpeg_rgb    chroma upsampling + colour conversion + crop: four pixels of a row per lane, 12 bytes out.
// Workgroup -> image as in the ragged transform: per-image block prefixes and a binary search.
#include "common.hpp"
#include "jpeg_abi.hpp"

namespace {

#define JPEG_GROUP 32            // blocks per k_jpeg_idct workgroup (Python: lemon_amd/jpeg.py::IDCT_GROUP)
#define JPEG_PIX 4               // pixels per k_jpeg_rgb lane (Python: RGB_PIXELS)
#define JPEG_LDS_PITCH 72        // elements between blocks in LDS: 8 blocks of a wave start 4 (int16) / 8 (int32) banks apart

struct JpegParams {
    const uint8_t *rec;
    const int64_t *desc;         // [n, 8] record offset, output offset, w, h, components, hs, vs, work offset
    const int64_t *apre, *bpre;  // [n + 1] first k_jpeg_idct / k_jpeg_rgb workgroup of each image
    uint8_t *work, *out;
    int64_t n, rec_bytes, work_bytes, out_bytes;
};

__device__ __forceinline__ int64_t jpeg_owner(const int64_t *pre, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;                      // largest i with pre[i] <= g (pre[0] = 0, pre[n] > g)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pre[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// an image whose record, planes or pixels would not lie inside their buffers: the host never builds one (lemon_amd/jpeg.py), but
// should it happen nothing of it is read or written
__device__ __forceinline__ bool jpeg_desc_ok(const JpegParams &p, const int64_t *d, JpegGeom &g) {
    if (!jpeg_geometry(d[2], d[3], d[4], d[5], d[6], g)) return false;
    return d[0] >= 0 && (d[0] & 15) == 0 && d[0] <= p.rec_bytes && LEMON_JPEG_QUANT_BYTES + 128 * g.blocks <= p.rec_bytes - d[0] &&
           d[1] >= 0 && d[1] <= p.out_bytes && d[2] * d[3] * 3 <= p.out_bytes - d[1] &&
           d[7] >= 0 && (d[7] & 15) == 0 && d[7] <= p.work_bytes && 64 * g.blocks <= p.work_bytes - d[7];
}

__global__ __launch_bounds__(256) void k_jpeg_idct(JpegParams p) {
    __shared__ __attribute__((aligned(16))) int16_t s_coef[JPEG_GROUP * JPEG_LDS_PITCH];
    __shared__ __attribute__((aligned(16))) int32_t s_ws[JPEG_GROUP * JPEG_LDS_PITCH];
    __shared__ uint16_t s_q[192];
    const int64_t gidx = blockIdx.x;
    const int64_t i = jpeg_owner(p.apre, p.n, gidx);
    const int64_t *d = p.desc + 8 * i;
    JpegGeom g;
    if (!jpeg_desc_ok(p, d, g)) return;
    const int64_t b0 = (gidx - p.apre[i]) * JPEG_GROUP;
    if (b0 >= g.blocks) return;
    const int nb = (int)min((int64_t)JPEG_GROUP, g.blocks - b0);
    const int t = threadIdx.x;
    const uint8_t *rec = p.rec + d[0];
    if (t < 192) s_q[t] = reinterpret_cast<const uint16_t *>(rec)[t];
    if ((t >> 3) < nb) {
        const uint4 v = *reinterpret_cast<const uint4 *>(rec + LEMON_JPEG_QUANT_BYTES + (b0 + (t >> 3)) * 128 + (t & 7) * 16);
        *reinterpret_cast<uint4 *>(&s_coef[(t >> 3) * JPEG_LDS_PITCH + (t & 7) * 8]) = v;
    }
    __syncthreads();
    {
        const int blk = t >> 3, col = t & 7;
        if (blk < nb) {
            const int64_t b = b0 + blk;
            const int c = b < g.n0 ? 0 : (b < g.n0 + g.nc ? 1 : 2);
            int32_t din[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                din[k] = (int32_t)s_coef[blk * JPEG_LDS_PITCH + k * 8 + col] * (int32_t)s_q[c * 64 + k * 8 + col];
            jpeg_idct_col(din, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) s_ws[blk * JPEG_LDS_PITCH + k * 8 + col] = o[k];
        }
    }
    __syncthreads();
    {
        const int r = t >> 5, blk = t & 31;
        if (blk < nb) {
            const int64_t b = b0 + blk;
            const int c = b < g.n0 ? 0 : (b < g.n0 + g.nc ? 1 : 2);
            const int64_t base = c == 0 ? 0 : (c == 1 ? g.n0 : g.n0 + g.nc);
            const int32_t bw = c == 0 ? g.bw0 : g.bwc;
            const int64_t lb = b - base;
            const int64_t by = lb / bw, bx = lb - by * bw;
            const int4 w0 = *reinterpret_cast<const int4 *>(&s_ws[blk * JPEG_LDS_PITCH + r * 8]);
            const int4 w1 = *reinterpret_cast<const int4 *>(&s_ws[blk * JPEG_LDS_PITCH + r * 8 + 4]);
            const int32_t ws[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            int32_t x[8];
            jpeg_idct_row(ws, x);
            uint2 o;
            o.x = (uint32_t)jpeg_range_limit(x[0]) | ((uint32_t)jpeg_range_limit(x[1]) << 8) | ((uint32_t)jpeg_range_limit(x[2]) << 16) |
                  ((uint32_t)jpeg_range_limit(x[3]) << 24);
            o.y = (uint32_t)jpeg_range_limit(x[4]) | ((uint32_t)jpeg_range_limit(x[5]) << 8) | ((uint32_t)jpeg_range_limit(x[6]) << 16) |
                  ((uint32_t)jpeg_range_limit(x[7]) << 24);
            // plane of component c: [8 bh][8 bw] bytes at 64 * base; every row and block start is a multiple of 8
            *reinterpret_cast<uint2 *>(p.work + d[7] + 64 * base + (by * 8 + r) * ((int64_t)bw * 8) + bx * 8) = o;
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_rgb(JpegParams p) {
    const int64_t gidx = blockIdx.x;
    const int64_t i = jpeg_owner(p.bpre, p.n, gidx);
    const int64_t *d = p.desc + 8 * i;
    JpegGeom g;
    if (!jpeg_desc_ok(p, d, g)) return;
    const int32_t w = (int32_t)d[2], h = (int32_t)d[3], hs = (int)d[5], vs = (int)d[6];
    const int32_t w4 = (w + JPEG_PIX - 1) / JPEG_PIX;
    const int64_t idx = (gidx - p.bpre[i]) * 256 + threadIdx.x;
    if (idx >= (int64_t)h * w4) return;
    const int32_t y = (int32_t)(idx / w4), x0 = (int32_t)(idx - (int64_t)y * w4) * JPEG_PIX;
    const uint8_t *Y = p.work + d[7];
    const int64_t ystride = (int64_t)g.bw0 * 8, cstride = (int64_t)g.bwc * 8;
    const uint8_t *Cb = Y + 64 * g.n0, *Cr = Cb + 64 * g.nc;
    const uint32_t luma = *reinterpret_cast<const uint32_t *>(Y + y * ystride + x0);    // (the padded plane holds x0 .. x0 + 3)
    const int np = min(JPEG_PIX, w - x0);
    uint8_t px[3 * JPEG_PIX];
#pragma unroll
    for (int j = 0; j < JPEG_PIX; ++j) {
        const int32_t l = (luma >> (8 * j)) & 255;
        if (d[4] == 1 || j >= np) {
            px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = (uint8_t)l;
        } else {
            jpeg_ycc_rgb(l, jpeg_chroma_at(Cb, cstride, g.dwc, g.dhc, hs, vs, x0 + j, y),
                         jpeg_chroma_at(Cr, cstride, g.dwc, g.dhc, hs, vs, x0 + j, y), px + 3 * j);
        }
    }
    uint8_t *o = p.out + d[1] + ((int64_t)y * w + x0) * 3;
    if (np == JPEG_PIX && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * np; ++k) o[k] = px[k];
    }
}

}  // namespace

extern "C" int lemon_jpeg_decode(const uint8_t *rec_dev, int64_t rec_bytes, int64_t batch, const int64_t *aux_dev, int64_t idct_blocks,
                                 int64_t rgb_blocks, uint8_t *work_dev, int64_t work_bytes, uint8_t *out_dev, int64_t out_bytes,
                                 void *stream) {
    LEMON_REQUIRE(batch >= 0 && rec_bytes >= 0 && work_bytes >= 0 && out_bytes >= 0 && idct_blocks >= 0 && rgb_blocks >= 0,
                  "batch, byte counts, block counts >= 0");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(rec_dev && aux_dev && work_dev && out_dev, "null pointer");
    LEMON_REQUIRE(idct_blocks < ((int64_t)1 << 31) && rgb_blocks < ((int64_t)1 << 31), "block counts < 2^31");
    LEMON_REQUIRE((((uintptr_t)rec_dev) & 15) == 0 && (((uintptr_t)work_dev) & 15) == 0, "rec_dev, work_dev 16-byte aligned");
    JpegParams p;
    p.rec = rec_dev; p.desc = aux_dev; p.apre = aux_dev + 8 * batch; p.bpre = p.apre + batch + 1;
    p.work = work_dev; p.out = out_dev; p.n = batch; p.rec_bytes = rec_bytes; p.work_bytes = work_bytes; p.out_bytes = out_bytes;
    if (idct_blocks) {
        hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)idct_blocks), dim3(256), 0, (hipStream_t)stream, p);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    if (rgb_blocks) {
        hipLaunchKernelGGL(k_jpeg_rgb, dim3((unsigned)rgb_blocks), dim3(256), 0, (hipStream_t)stream, p);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    return LEMON_OK;
}
