// png.hip -- the device half of the PNG decode (lemon_png_decode, include/lemon_hip.h; lib/datasets/dataloader.py:184 decodes
// the file with `Image.open(p).convert("RGB")`): the workers parse the chunks and inflate, and this kernel turns a batch of
// records -- palette + filtered scanlines, png_core.hpp -- into packed uint8 RGB images, the layout RaggedImages /
// lemon_preprocess_ragged read.
//   k_png_decode   one workgroup of ONE wave per image, so a loader batch of several hundred images fills the chip.  Bands of 64
//                  rows run in order; inside a band the rows form a diagonal wavefront: lane = row, at step t lane l
//                  reconstructs pixel t - l, the pixel above arrives from lane l - 1 by one lane shift (png_lane_step).  The
//                  band's last row goes to the work buffer (one uint32 per pixel) and comes back as lane 0's row above.
//                  Steps run in blocks of 64.  Before a block every lane copies the <= 64 * bpp filtered bytes it is about to
//                  consume from its row into its own LDS row, as aligned 16-byte pieces (placed at the same offset mod 16 as in
//                  memory); after it the lane's 192 RGB bytes leave its LDS row as aligned 16-byte pieces, the ragged ends byte
//                  by byte.  Nothing is read outside the record, nothing written outside the image's h * w * 3 bytes.  LDS rows
//                  are lane-private (pitches of an odd number of dwords: distinct banks), so only the 64 words of lane 0's row
//                  above need a barrier.
#include "common.hpp"
#include "png_abi.hpp"

namespace {

#define PNG_STEPS 64                               // steps per staging block
#define PNG_IN_PIECES(bpp) (4 * (bpp) + 1)         // 64 * bpp bytes + up to 15 bytes of alignment, in 16-byte pieces
#define PNG_IN_PITCH(bpp) (16 * PNG_IN_PIECES(bpp) + 4)
#define PNG_OUT_PIECES 13                          // 192 RGB bytes + up to 15 bytes of alignment
#define PNG_OUT_PITCH (16 * PNG_OUT_PIECES + 4)

struct PngParams {
    const uint8_t *rec;
    const int64_t *desc;         // [n, 8] record offset, h, w, colour type, PLTE count, output offset, work offset, 0
    uint8_t *work, *out;
    int32_t *status;
    int64_t n, rec_bytes, work_bytes, out_bytes;
};

// an image whose record, pixels or work share would not lie inside their buffers: the host never builds one
// (lemon_amd/jpeg_host.py::BatchLayout), but should it happen nothing of it is read or written
__device__ __forceinline__ bool png_desc_ok(const PngParams &p, const int64_t *d) {
    const int64_t h = d[1], w = d[2];
    const int bpp = png_channels(d[3]);
    if (!bpp || h < 1 || w < 1 || h > LEMON_PNG_MAX_DIM || w > LEMON_PNG_MAX_DIM || d[4] < 0 || d[4] > 256) return false;
    return d[0] >= 0 && (d[0] & 15) == 0 && d[0] <= p.rec_bytes && 1024 + h * (w * bpp + 1) <= p.rec_bytes - d[0] &&
           d[5] >= 0 && d[5] <= p.out_bytes && h * w * 3 <= p.out_bytes - d[5] &&
           d[6] >= 0 && (d[6] & 15) == 0 && d[6] <= p.work_bytes && ((4 * w + 15) & ~(int64_t)15) <= p.work_bytes - d[6];
}

template <int BPP>
__device__ __forceinline__ int png_image(const PngParams &p, const int64_t *d, uint32_t *s_in, uint32_t *s_out, uint32_t *s_up,
                                         const uint32_t *s_pal) {
    const int lane = threadIdx.x;
    const int32_t h = (int32_t)d[1], w = (int32_t)d[2];
    const int ct = (int)d[3], plte = (int)d[4];
    const uint8_t *rec = p.rec + d[0];
    const int64_t pitch = (int64_t)w * BPP + 1;
    const uint8_t *rec_end = rec + 1024 + (int64_t)h * pitch;
    uint8_t *out = p.out + d[5];
    uint32_t *work = reinterpret_cast<uint32_t *>(p.work + d[6]);
    uint32_t *in_row = s_in + lane * (PNG_IN_PITCH(BPP) / 4), *out_row = s_out + lane * (PNG_OUT_PITCH / 4);
    const uint8_t *in_b = reinterpret_cast<const uint8_t *>(in_row);
    uint8_t *out_b = reinterpret_cast<uint8_t *>(out_row);
    bool index_bad = false;
    for (int32_t r0 = 0; r0 < h; r0 += LEMON_PNG_BAND) {
        const int rows = min(LEMON_PNG_BAND, h - r0);
        const bool row_on = lane < rows;
        const int32_t row = r0 + lane;
        const uint8_t *rowp = rec + 1024 + (int64_t)(row_on ? row : r0) * pitch;      // (an idle lane points at a valid row, reads nothing)
        const int ft = row_on ? rowp[0] : 0;
        if (__any(ft > 4)) return LEMON_PNG_FILTER;                                  // (uniform)
        uint8_t *orow = out + (int64_t)(row_on ? row : r0) * w * 3;
        PngLane s;
        s.cur = s.above = 0;
        const int32_t nsteps = w + rows - 1;
        for (int32_t t0 = 0; t0 < nsteps; t0 += PNG_STEPS) {
            const int32_t xs = max(t0 - lane, 0), xe = min(t0 + PNG_STEPS - lane, w);
            const bool has = row_on && xe > xs;
            // ---- lane 0's row above: the previous band's last row, 64 pixels, one per lane
            __syncthreads();
            if (r0 > 0 && t0 + lane < w) s_up[lane] = work[t0 + lane];
            // ---- this lane's filtered bytes -> its LDS row, aligned 16-byte pieces
            const uintptr_t gin = reinterpret_cast<uintptr_t>(rowp + 1 + (int64_t)xs * BPP);
            const int in_skew = (int)(gin & 15);
            if (has) {
                const int pieces = (in_skew + (xe - xs) * BPP + 15) >> 4;             // <= PNG_IN_PIECES(BPP)
#pragma unroll
                for (int k = 0; k < PNG_IN_PIECES(BPP); ++k) {
                    if (k >= pieces) continue;
                    const uint8_t *src = reinterpret_cast<const uint8_t *>((gin & ~(uintptr_t)15) + 16 * k);   // (>= rec: rec is 16-byte aligned)
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (src + 16 <= rec_end) {
                        v = *reinterpret_cast<const uint4 *>(src);
                    } else {                                                         // the record's last, partial piece
                        uint32_t q[4] = {0, 0, 0, 0};
                        for (int j = 0; j < 16 && src + j < rec_end; ++j) q[j >> 2] |= (uint32_t)src[j] << (8 * (j & 3));
                        v = make_uint4(q[0], q[1], q[2], q[3]);
                    }
                    in_row[4 * k] = v.x; in_row[4 * k + 1] = v.y; in_row[4 * k + 2] = v.z; in_row[4 * k + 3] = v.w;
                }
            }
            const uintptr_t gout = reinterpret_cast<uintptr_t>(orow + (int64_t)xs * 3);
            const int out_skew = (int)(gout & 15);
            __syncthreads();
            // ---- the block's steps
            const int32_t jn = min(PNG_STEPS, nsteps - t0);
            for (int32_t j = 0; j < jn; ++j) {
                const uint32_t shifted = __shfl_up(s.cur, 1);                        // lane l - 1's pixel of step t - 1: the pixel above
                const int32_t x = t0 + j - lane;
                if (row_on && x >= 0 && x < w) {
                    const uint32_t up = lane > 0 ? shifted : (r0 > 0 ? s_up[j] : 0u);
                    const int at = in_skew + (x - xs) * BPP;
                    uint32_t raw = 0;
#pragma unroll
                    for (int k = 0; k < BPP; ++k) raw |= (uint32_t)in_b[at + k] << (8 * k);
                    const uint32_t px = png_lane_step<BPP>(s, ft, raw, up, x == 0);
                    if (lane == LEMON_PNG_BAND - 1 && r0 + LEMON_PNG_BAND < h) work[x] = px;
                    const uint32_t c = png_rgb(px, ct, s_pal, plte, index_bad);
                    const int ob = out_skew + (x - xs) * 3;
                    out_b[ob] = (uint8_t)c; out_b[ob + 1] = (uint8_t)(c >> 8); out_b[ob + 2] = (uint8_t)(c >> 16);
                }
            }
            // ---- this lane's RGB bytes [gout, gout + nb): whole aligned pieces as 16 bytes, the ragged ends byte by byte
            if (has) {
                const int end = out_skew + (xe - xs) * 3;                            // <= 15 + 192
#pragma unroll
                for (int k = 0; k < PNG_OUT_PIECES; ++k) {
                    if (16 * k >= end) continue;
                    uint8_t *dst = reinterpret_cast<uint8_t *>((gout & ~(uintptr_t)15) + 16 * k);
                    if (16 * k >= out_skew && 16 * k + 16 <= end) {
                        *reinterpret_cast<uint4 *>(dst) = make_uint4(out_row[4 * k], out_row[4 * k + 1], out_row[4 * k + 2], out_row[4 * k + 3]);
                    } else {
                        for (int j = max(16 * k, out_skew); j < min(16 * k + 16, end); ++j) dst[j - 16 * k] = out_b[j];
                    }
                }
            }
        }
        // the band's last row is in the work buffer before the next band's lanes read it
        __threadfence();
        __syncthreads();
    }
    return __any(index_bad) ? LEMON_PNG_INDEX : LEMON_PNG_OK;
}

__global__ __launch_bounds__(LEMON_PNG_BAND) void k_png_decode(PngParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t s_in[LEMON_PNG_BAND * PNG_IN_PITCH(4) / 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_out[LEMON_PNG_BAND * PNG_OUT_PITCH / 4];
    __shared__ uint32_t s_up[PNG_STEPS];
    __shared__ __attribute__((aligned(16))) uint32_t s_pal[256];
    const int64_t i = blockIdx.x;
    const int64_t *d = p.desc + 8 * i;
    const int lane = threadIdx.x;
    if (!png_desc_ok(p, d)) {
        if (lane == 0) p.status[i] = LEMON_PNG_BUFFER;
        return;
    }
    {   // the palette: 64 lanes x 16 bytes (the record starts at a multiple of 16)
        const uint4 v = *reinterpret_cast<const uint4 *>(p.rec + d[0] + 16 * lane);
        s_pal[4 * lane] = v.x; s_pal[4 * lane + 1] = v.y; s_pal[4 * lane + 2] = v.z; s_pal[4 * lane + 3] = v.w;
    }
    __syncthreads();
    const int bpp = png_channels(d[3]);
    const int verdict = bpp == 1 ? png_image<1>(p, d, s_in, s_out, s_up, s_pal)
                      : bpp == 2 ? png_image<2>(p, d, s_in, s_out, s_up, s_pal)
                      : bpp == 3 ? png_image<3>(p, d, s_in, s_out, s_up, s_pal)
                                 : png_image<4>(p, d, s_in, s_out, s_up, s_pal);
    if (lane == 0) p.status[i] = verdict;
}

}  // namespace

extern "C" int64_t lemon_png_decode_workspace_bytes(int64_t batch, int64_t total_width) {
    if (batch < 0 || total_width < 0 || batch > ((int64_t)1 << 31) || total_width > ((int64_t)1 << 48)) return LEMON_E_INVALID;
    return 16 * batch + 4 * total_width + 16;
}

extern "C" int lemon_png_decode(const uint8_t *rec_dev, int64_t rec_bytes, int64_t batch, const int64_t *aux_dev, uint8_t *work_dev,
                                int64_t work_bytes, uint8_t *out_dev, int64_t out_bytes, int32_t *status_dev, void *stream) {
    LEMON_REQUIRE(batch >= 0 && rec_bytes >= 0 && work_bytes >= 0 && out_bytes >= 0, "batch, byte counts >= 0");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(rec_dev && aux_dev && work_dev && out_dev && status_dev, "null pointer");
    LEMON_REQUIRE(batch < ((int64_t)1 << 31), "batch < 2^31");
    LEMON_REQUIRE((((uintptr_t)rec_dev) & 15) == 0 && (((uintptr_t)work_dev) & 15) == 0, "rec_dev, work_dev 16-byte aligned");
    PngParams p;
    p.rec = rec_dev; p.desc = aux_dev; p.work = work_dev; p.out = out_dev; p.status = status_dev;
    p.n = batch; p.rec_bytes = rec_bytes; p.work_bytes = work_bytes; p.out_bytes = out_bytes;
    hipLaunchKernelGGL(k_png_decode, dim3((unsigned)batch), dim3(LEMON_PNG_BAND), 0, (hipStream_t)stream, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
