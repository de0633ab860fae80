// png_inflate.hip -- the inflate of the PNG path on the device (lemon_png_inflate, include/lemon_hip.h; lib/datasets/dataloader.py:
// 177-184 decodes the file with `Image.open(p).convert("RGB")`): with LEMON_PNG=device the workers only walk the chunks and
// hand over the concatenated IDAT payload, and this kernel writes the filtered scanlines into the record that k_png_decode
// (png.hip) reads next on the same stream.
//   k_png_inflate   one workgroup of ONE wave per image, as k_png_decode: the symbol walk of a DEFLATE stream is serial, so the
//                   parallelism is across the images of a batch plus everything inside a stream that is wide -- staging the
//                   input, building a dynamic block's tables, placing a queue of tokens, copying matches and stored blocks,
//                   writing the window through, the Adler-32.  The whole schedule is png_inflate_core.hpp, shared with the host
//                   twin; here its state (32 KiB window, 2 KiB staging ring, tables, token queue: PzShared) is LDS and its
//                   lanes are the wave's.  A malformed stream ends with a status; nothing is read outside the stream's bytes,
//                   nothing written outside the image's `want` bytes.
#include "common.hpp"
#include "png_inflate_core.hpp"

namespace {

struct PzParams {
    const uint8_t *z;
    const int64_t *aux;          // [n, 4] stream offset, stream bytes, offset of the scanlines in rec, want
    uint8_t *rec;
    int32_t *status;
    int64_t z_bytes, rec_bytes;
};

__global__ __launch_bounds__(PZ_LANES) void k_png_inflate(PzParams p) {
    __shared__ PzShared S;
    const int64_t i = blockIdx.x;
    const int64_t *d = p.aux + 4 * i;
    const int64_t zoff = d[0], zn = d[1], roff = d[2], want = d[3];
    // an image whose stream or rows would not lie inside their buffers: nothing of it is read or written
    if (zoff < 0 || zn < 0 || zoff > p.z_bytes || zn > p.z_bytes - zoff || roff < 0 || want < 0 || roff > p.rec_bytes ||
        want > p.rec_bytes - roff) {
        if (threadIdx.x == 0) p.status[i] = LEMON_PNG_BUFFER;
        return;
    }
    const int verdict = pz_inflate(S, p.z + zoff, zn, p.rec + roff, want);
    if (threadIdx.x == 0) p.status[i] = verdict;
}

}  // namespace

extern "C" int lemon_png_inflate(const uint8_t *z_dev, int64_t z_bytes, int64_t batch, const int64_t *aux_dev, uint8_t *rec_dev,
                                 int64_t rec_bytes, int32_t *status_dev, void *stream) {
    LEMON_REQUIRE(batch >= 0 && z_bytes >= 0 && rec_bytes >= 0, "batch, byte counts >= 0");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(z_dev && aux_dev && rec_dev && status_dev, "null pointer");
    LEMON_REQUIRE(batch < ((int64_t)1 << 31), "batch < 2^31");
    PzParams p;
    p.z = z_dev; p.aux = aux_dev; p.rec = rec_dev; p.status = status_dev; p.z_bytes = z_bytes; p.rec_bytes = rec_bytes;
    hipLaunchKernelGGL(k_png_inflate, dim3((unsigned)batch), dim3(PZ_LANES), 0, (hipStream_t)stream, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
