// Image preprocessing of the embedding stage on the GPU (gfx950 only):
//   generic_transform = Resize(224, BICUBIC on the uint8 PIL image) -> CenterCrop(224) -> ToTensor ->
//   Normalize(CLIP mean/std)                                lib/datasets/utils.py:159-170
// for batches of equally sized uint8 HWC images (CIFAR: 32x32 -> 224x224, the x49 up-sampling the
// reference spends 8 DataLoader workers on, run_lemon.py:129-131).  PIL's resampler is integer
// arithmetic: per output pixel a window of <= ksize taps with 22-bit fixed-point coefficients,
// accumulator 1<<21 + sum(u8 * k), result clip8(acc >> 22), horizontal pass first, then vertical on the
// uint8 intermediate.  The coefficient tables are built on the host by the same double-precision
// recipe (lemon_amd/data.py::pil_bicubic_tables, pinned against PIL itself in the tests) and already
// cropped to the S output rows/columns; this kernel is the two integer passes + the float epilogue
// (v/255 - mean)/std, bit-identical to the PIL + torch pipeline.
//
// One workgroup per (image, block of R output rows): horizontal pass for the input rows that block
// needs into an LDS uint8 tile, vertical pass from LDS (four pixels x three channels per work item: three
// aligned LDS words per tap, the float epilogue from a 768-entry table, 16-byte stores).  Traffic: the
// uint8 image in (3 KB for CIFAR), 12*S*S bytes out (602 KB): HBM-write bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "split3.hpp"

namespace {

constexpr int PIL_PRECISION_BITS = 22;   // 32 - 8 - 2 (Pillow Resample.c)

struct PreParams {
    const uint8_t *img;      // [B, H, W, 3]
    const int32_t *kk_h, *bnd_h, *kk_v, *bnd_v;   // [S, ks_h], [S, 2] (xmin, count), [S, ks_v], [S, 2]
    float *out;              // [B, 3, S, S]
    int H, W, S, ks_h, ks_v, R, blocks_per_img;
    int patch;               // 0: NCHW; P > 0: patch-major [B, (S/P)^2, 3*P*P] (what the patch-embedding GEMM reads)
    unsigned short *out_t;   // non-null (with P > 0): the same patch rows as the TILE-MAJOR fp16 split operand of lemon_linear_f16x3t
    float mean[3], stdv[3];
};

__device__ __forceinline__ uint8_t pil_clip8(int acc) {
    const int v = acc >> PIL_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

constexpr int LUT_BYTES = 3 * 256 * 4;     // (v/255 - mean[c]) / std[c] for every uint8 value and channel
constexpr int VTAB_MAX_INTS = 512;         // the block's vertical windows: R x (ymin, count, ks_v taps)

// ---- the per-block bodies, shared by the same-shape kernel (k_preprocess_u8: horizontal rows in LDS) and the ragged pair
// (k_ragged_h / k_ragged_v: horizontal rows in a global uint8 intermediate) -----------------------------------------------

// the float epilogue of a uint8 value is one of 768 numbers: ToTensor's division and Normalize's, done once per value with
// exactly the arithmetic of the per-pixel form (two IEEE divisions per output pixel were most of this kernel's time)
__device__ __forceinline__ void fill_lut(float *s_lut, float m0, float m1, float m2, float s0, float s1, float s2) {
    for (int i = threadIdx.x; i < 768; i += blockDim.x) {
        const int c = i >> 8;
        const float f = (float)(i & 255) / 255.0f;                       // ToTensor
        s_lut[i] = (f - (c == 0 ? m0 : c == 1 ? m1 : m2)) / (c == 0 ? s0 : c == 1 ? s1 : s2);    // Normalize
    }
}

// the vertical windows of output rows [y0, y1): per row (ymin, count, ks_v taps)
__device__ __forceinline__ void fill_vtab(int *s_vt, const int32_t *bnd_v, const int32_t *kk_v, int ks_v, int y0, int y1) {
    const int vstride = 2 + ks_v;
    for (int i = threadIdx.x; i < (y1 - y0) * vstride; i += blockDim.x) {
        const int yy = i / vstride, j = i - yy * vstride;
        s_vt[i] = j < 2 ? bnd_v[2 * (y0 + yy) + j] : kk_v[(y0 + yy) * ks_v + (j - 2)];
    }
}

// horizontal pass: `rows` input rows (the first at `src`, row stride src_stride bytes) -> `rows` rows of S*3 uint8 at dst.  One
// output pixel per lane and iteration, its three channels together: each tap weight is loaded once and the window's bytes are
// contiguous for the lane (the same integer sums as one channel per lane, so the same bits)
__device__ __forceinline__ void hpass_rows(const uint8_t *src0, int64_t src_stride, uint8_t *dst, int rows, int S,
                                           const int32_t *bnd_h, const int32_t *kk_h, int ks_h) {
    for (int it = threadIdx.x; it < rows * S; it += blockDim.x) {
        const int r = it / S, x = it - r * S;
        const int xmin = bnd_h[2 * x], n = bnd_h[2 * x + 1];
        const int32_t *k = kk_h + x * ks_h;
        const uint8_t *src = src0 + (int64_t)r * src_stride + xmin * 3;
        int a0 = 1 << (PIL_PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
            a0 += (int)src[3 * t] * kt;
            a1 += (int)src[3 * t + 1] * kt;
            a2 += (int)src[3 * t + 2] * kt;
        }
        uint8_t *o = dst + (int64_t)r * 3 * S + 3 * x;
        o[0] = pil_clip8(a0); o[1] = pil_clip8(a1); o[2] = pil_clip8(a2);
    }
}

// vertical pass + epilogue of output rows [y0, y1) of batch position b, from horizontally resampled rows `tmp` (tmp row 0 = input
// row vmin, row stride 3S bytes, 4-byte aligned) and the block's windows s_vt; writes NCHW (P == 0), patch-major (P > 0) or,
// with out_t, the tile-major fp16 split operand
__device__ __forceinline__ void vpass_rows(const uint8_t *tmp, int vmin, const int *s_vt, int ks_v, const float *s_lut,
                                           int y0, int y1, int S, int P, int64_t b, float *out, unsigned short *out_t) {
    const int tid = threadIdx.x, S3 = 3 * S, vstride = 2 + ks_v;
    const int nP = P ? S / P : 0;
    if ((S & 3) == 0 && (P & 3) == 0) {
        // four output pixels x three channels per work item: 12 bytes (3 aligned words) of the tile per tap, three 16-byte stores
        const int q4 = S >> 2;
        for (int it = tid; it < (y1 - y0) * q4; it += blockDim.x) {
            const int yy = it / q4, x = 4 * (it - yy * q4), y = y0 + yy;
            const int *vt = s_vt + yy * vstride;
            const int ymin = vt[0], n = vt[1];
            int acc[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] = 1 << (PIL_PRECISION_BITS - 1);
            const uint8_t *src = tmp + (int64_t)(ymin - vmin) * S3 + 3 * x;
            for (int t = 0; t < n; ++t) {
                const int kt = vt[2 + t];
                const uint32_t *w = reinterpret_cast<const uint32_t *>(src + (int64_t)t * S3);
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i] += (int)((w0 >> (8 * i)) & 255u) * kt;
                    acc[4 + i] += (int)((w1 >> (8 * i)) & 255u) * kt;
                    acc[8 + i] += (int)((w2 >> (8 * i)) & 255u) * kt;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *lut = s_lut + 256 * c;
                const float4 v = make_float4(lut[pil_clip8(acc[c])], lut[pil_clip8(acc[3 + c])], lut[pil_clip8(acc[6 + c])], lut[pil_clip8(acc[9 + c])]);
                if (out_t) {
                    // the patch-embedding GEMM's activation operand (split3.hpp: tiled_off): four consecutive k of one patch row = 8 bytes
                    // of its hi plane and 8 of its lo plane; no fp32 pixel tensor, no split pass
                    const float x4[4] = {v.x, v.y, v.z, v.w};
                    lemon_split::us4 hi, lo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        unsigned short a_, b_, c_;
                        lemon_split::split2h<false>(x4[e], a_, b_, c_);
                        hi[e] = a_; lo[e] = c_;
                    }
                    const int64_t o = lemon_split::tiled_off(lemon_split::TILE_A_ROWS, b * nP * nP + (int64_t)(y / P) * nP + x / P,
                                                             c * P * P + (y % P) * P + (x % P), 0, 3 * P * P);
                    *reinterpret_cast<lemon_split::us4 *>(out_t + o) = hi;
                    *reinterpret_cast<lemon_split::us4 *>(out_t + o + lemon_split::TILE_A_ROWS * 16) = lo;
                    continue;
                }
                // NCHW row, or the row's place inside its patches: out[b][py*nP+px][c*P*P + (y%P)*P + (x%P)]
                float *dst = P ? out + (b * nP * nP + (int64_t)(y / P) * nP + x / P) * (3 * P * P) + c * P * P + (y % P) * P + (x % P)
                               : out + ((b * 3 + c) * S + y) * (int64_t)S + x;
                *reinterpret_cast<float4 *>(dst) = v;
            }
        }
        return;
    }
    for (int c = 0; c < 3; ++c) {
        const float *lut = s_lut + 256 * c;
        for (int y = y0; y < y1; ++y) {
            const int *vt = s_vt + (y - y0) * vstride;
            const int ymin = vt[0], n = vt[1];
            float *dst = P ? out + (b * nP * nP + (int64_t)(y / P) * nP) * (3 * P * P) + c * P * P + (y % P) * P
                           : out + ((b * 3 + c) * S + y) * (int64_t)S;
            for (int x = tid; x < S; x += blockDim.x) {
                const uint8_t *src = tmp + (int64_t)(ymin - vmin) * S3 + 3 * x + c;
                int acc = 1 << (PIL_PRECISION_BITS - 1);
                for (int t = 0; t < n; ++t) acc += (int)src[(int64_t)t * S3] * vt[2 + t];
                const float v = lut[pil_clip8(acc)];
                if (P) dst[(int64_t)(x / P) * (3 * P * P) + (x % P)] = v; else dst[x] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_preprocess_u8(PreParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    float *s_lut = reinterpret_cast<float *>(s_dyn);                     // [3][256]
    int *s_vt = reinterpret_cast<int *>(s_dyn + LUT_BYTES);              // [R][2 + ks_v]
    uint8_t *s_tmp = s_dyn + LUT_BYTES + VTAB_MAX_INTS * 4;              // [rows][S*3] horizontally resampled input rows
    const int64_t b = blockIdx.x / p.blocks_per_img;
    const int yb = blockIdx.x % p.blocks_per_img;
    const int y0 = yb * p.R;
    const int y1 = y0 + p.R < p.S ? y0 + p.R : p.S;
    const int vmin = p.bnd_v[2 * y0];            // windows are monotone in y
    const int vmax = p.bnd_v[2 * (y1 - 1)] + p.bnd_v[2 * (y1 - 1) + 1];
    const uint8_t *img = p.img + b * (int64_t)p.H * p.W * 3;

    fill_lut(s_lut, p.mean[0], p.mean[1], p.mean[2], p.stdv[0], p.stdv[1], p.stdv[2]);
    fill_vtab(s_vt, p.bnd_v, p.kk_v, p.ks_v, y0, y1);
    hpass_rows(img + (int64_t)vmin * p.W * 3, (int64_t)p.W * 3, s_tmp, vmax - vmin, p.S, p.bnd_h, p.kk_h, p.ks_h);
    __syncthreads();
    vpass_rows(s_tmp, vmin, s_vt, p.ks_v, s_lut, y0, y1, p.S, p.patch, b, p.out, p.out_t);
}

// ---- ragged batches: images of different (H, W) in one packed buffer -----------------------------------------------------
// Two launches.  k_ragged_h: one workgroup per (image, RAGGED_HROWS input rows of the rows its crop window needs), horizontal
// pass into a global uint8 intermediate (every input row resampled once, whatever the image size -- no LDS bound on the
// vertical window).  k_ragged_v: one workgroup per (image, R output rows of its plan), vertical pass + epilogue from that
// intermediate.  The workgroup -> image map is a binary search of per-image first-block prefixes (built on the host per call,
// one int per image): a sub-batch is just a subset of descriptors over the same packed buffer.
constexpr int RAGGED_HROWS = 16;           // input rows per horizontal workgroup: 16 x 224 pixels = 14 per lane
constexpr int RAGGED_VTAB_INTS = 4096;     // the vertical windows of one block, R (2 + ks_v) ints: R = 1 holds 4 094 taps (a 30 000 px
                                           // short side down to 30 px, 229 000 px down to 224); 19 KB of LDS keep 8 workgroups per CU
// plan table: RAGGED_PLAN_INTS int32 per distinct (H, W); offsets index the concatenated int32 tap buffer
enum { PL_H, PL_W, PL_KKH, PL_BH, PL_KKV, PL_BV, PL_KSH, PL_KSV, PL_R, PL_NVBLK, PL_VMIN, PL_ROWS, PL_NHBLK, RAGGED_PLAN_INTS = 16 };
// descriptors: 4 int64 per image (byte offset into the packed buffer, H, W, plan index)

struct RaggedParams {
    const uint8_t *data;
    const int64_t *desc;      // [n, 4]
    const int64_t *hpre;      // [n + 1] first horizontal block of each image
    const int64_t *vpre;      // [n + 1] first vertical block
    const int64_t *ioff;      // [n] byte offset of each image's rows in the intermediate
    const int32_t *plans, *taps;
    uint8_t *work;
    float *out;
    unsigned short *out_t;
    int64_t n, data_bytes;
    int S, patch;
    float mean[3], stdv[3];
};

__device__ __forceinline__ int64_t block_owner(const int64_t *pre, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;                      // largest i with pre[i] <= g (pre[0] = 0, pre[n] > g)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pre[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// a plan that does not belong to its descriptor, or an image that does not lie inside the packed buffer: the host never builds
// one (data.py::gpu_transform_ragged), but should it happen nothing is read and the image's outputs become NaN (loud, not wrong)
__device__ __forceinline__ bool ragged_ok(const RaggedParams &p, const int64_t *d, const int32_t *pl) {
    return pl[PL_H] == d[1] && pl[PL_W] == d[2] && d[0] >= 0 && d[0] + d[1] * d[2] * 3 <= p.data_bytes && pl[PL_R] >= 1 &&
           pl[PL_KSV] >= 1 && pl[PL_R] * (2 + pl[PL_KSV]) <= RAGGED_VTAB_INTS && pl[PL_VMIN] >= 0 && pl[PL_VMIN] + pl[PL_ROWS] <= d[1];
}

__global__ __launch_bounds__(256) void k_ragged_h(RaggedParams p) {
    const int64_t g = blockIdx.x;
    const int64_t i = block_owner(p.hpre, p.n, g);
    const int64_t *d = p.desc + 4 * i;
    const int32_t *pl = p.plans + RAGGED_PLAN_INTS * d[3];
    if (!ragged_ok(p, d, pl)) return;
    const int r0 = (int)(g - p.hpre[i]) * RAGGED_HROWS;
    const int r1 = min(r0 + RAGGED_HROWS, pl[PL_ROWS]);
    const int W3 = 3 * pl[PL_W];
    hpass_rows(p.data + d[0] + (int64_t)(pl[PL_VMIN] + r0) * W3, W3, p.work + p.ioff[i] + (int64_t)r0 * 3 * p.S, r1 - r0, p.S,
               p.taps + pl[PL_BH], p.taps + pl[PL_KKH], pl[PL_KSH]);
}

__global__ __launch_bounds__(256) void k_ragged_v(RaggedParams p) {
    __shared__ __attribute__((aligned(16))) float s_lut[768];
    __shared__ int s_vt[RAGGED_VTAB_INTS];
    const int64_t g = blockIdx.x;
    const int64_t i = block_owner(p.vpre, p.n, g);
    const int64_t *d = p.desc + 4 * i;
    const int32_t *pl = p.plans + RAGGED_PLAN_INTS * d[3];
    const int vb = (int)(g - p.vpre[i]);
    if (!ragged_ok(p, d, pl)) {
        // every output of this block's rows NaN: a LUT of NaN and windows of no taps (nothing is read)
        const int nb = (int)(p.vpre[i + 1] - p.vpre[i]);
        const int R = (p.S + nb - 1) / nb;
        const int y0 = vb * R, y1 = min(y0 + R, p.S);
        if (y0 >= p.S || R > RAGGED_VTAB_INTS / 2) return;
        for (int j = threadIdx.x; j < 768; j += blockDim.x) s_lut[j] = __builtin_nanf("");
        for (int j = threadIdx.x; j < 2 * (y1 - y0); j += blockDim.x) s_vt[j] = 0;
        __syncthreads();
        vpass_rows(p.work, 0, s_vt, 0, s_lut, y0, y1, p.S, p.patch, i, p.out, p.out_t);
        return;
    }
    const int y0 = vb * pl[PL_R];
    const int y1 = min(y0 + pl[PL_R], p.S);
    fill_lut(s_lut, p.mean[0], p.mean[1], p.mean[2], p.stdv[0], p.stdv[1], p.stdv[2]);
    fill_vtab(s_vt, p.taps + pl[PL_BV], p.taps + pl[PL_KKV], pl[PL_KSV], y0, y1);
    __syncthreads();
    vpass_rows(p.work + p.ioff[i], pl[PL_VMIN], s_vt, pl[PL_KSV], s_lut, y0, y1, p.S, p.patch, i, p.out, p.out_t);
}

}  // namespace

static int preprocess_impl(const uint8_t *img_dev, int64_t batch, int in_h, int in_w, const int32_t *kk_h_dev,
                           const int32_t *bnd_h_dev, int ks_h, const int32_t *kk_v_dev, const int32_t *bnd_v_dev,
                           int ks_v, int out_size, int max_rows_per_block, int rows_per_block,
                           const float *mean3_host, const float *std3_host, int patch, float *out_dev, unsigned short *out_t,
                           void *stream) {
    LEMON_REQUIRE(batch >= 0 && in_h > 0 && in_w > 0 && out_size > 0, "batch >= 0, sizes > 0");
    LEMON_REQUIRE(ks_h > 0 && ks_v > 0 && rows_per_block > 0 && max_rows_per_block > 0, "table geometry");
    LEMON_REQUIRE(patch >= 0 && (patch == 0 || out_size % patch == 0), "patch must divide out_size");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(img_dev && kk_h_dev && bnd_h_dev && kk_v_dev && bnd_v_dev && mean3_host && std3_host && out_dev, "null pointer");
    LEMON_REQUIRE((int64_t)rows_per_block * (2 + ks_v) <= VTAB_MAX_INTS, "rows_per_block * (2 + ks_v) <= 512");
    LEMON_REQUIRE((((uintptr_t)out_dev) & 15) == 0, "out_dev must be 16-byte aligned");
    const size_t lds = LUT_BYTES + VTAB_MAX_INTS * 4 + (((size_t)max_rows_per_block * out_size * 3 + 15) & ~(size_t)15);
    LEMON_REQUIRE((size_t)max_rows_per_block * out_size * 3 <= 56 * 1024, "rows_per_block too large: the horizontal tile must fit 56 KB of LDS");
    PreParams p;
    p.img = img_dev; p.kk_h = kk_h_dev; p.bnd_h = bnd_h_dev; p.kk_v = kk_v_dev; p.bnd_v = bnd_v_dev; p.out = out_dev;
    p.patch = patch; p.out_t = out_t;
    p.H = in_h; p.W = in_w; p.S = out_size; p.ks_h = ks_h; p.ks_v = ks_v; p.R = rows_per_block;
    p.blocks_per_img = (out_size + rows_per_block - 1) / rows_per_block;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean3_host[c]; p.stdv[c] = std3_host[c]; }
    const int64_t grid = batch * p.blocks_per_img;
    LEMON_REQUIRE(grid < (int64_t)1 << 31, "batch * row blocks < 2^31");
    hipLaunchKernelGGL(k_preprocess_u8, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

extern "C" int lemon_preprocess_u8(const uint8_t *img_dev, int64_t batch, int in_h, int in_w, const int32_t *kk_h_dev,
                                   const int32_t *bnd_h_dev, int ks_h, const int32_t *kk_v_dev, const int32_t *bnd_v_dev,
                                   int ks_v, int out_size, int max_rows_per_block, int rows_per_block,
                                   const float *mean3_host, const float *std3_host, int patch, float *out_dev,
                                   void *stream) {
    return preprocess_impl(img_dev, batch, in_h, in_w, kk_h_dev, bnd_h_dev, ks_h, kk_v_dev, bnd_v_dev, ks_v, out_size, max_rows_per_block,
                           rows_per_block, mean3_host, std3_host, patch, out_dev, nullptr, stream);
}

// ... with the patch rows written as the tile-major fp16 split operand of lemon_linear_f16x3t (rows = batch * (out_size / patch)^2,
// k = 3 patch^2): the patch embedding then runs in the hand-written GEMM straight from this kernel's output
extern "C" int lemon_preprocess_u8_f16x3t(const uint8_t *img_dev, int64_t batch, int in_h, int in_w, const int32_t *kk_h_dev,
                                          const int32_t *bnd_h_dev, int ks_h, const int32_t *kk_v_dev, const int32_t *bnd_v_dev,
                                          int ks_v, int out_size, int max_rows_per_block, int rows_per_block,
                                          const float *mean3_host, const float *std3_host, int patch, uint16_t *outt_dev,
                                          void *stream) {
    LEMON_REQUIRE(patch > 0 && patch % 4 == 0 && out_size % 4 == 0 && (3 * patch * patch) % 16 == 0,
                  "patch a positive multiple of 4 with 3 patch^2 a multiple of 16 (the operand's k16 steps)");
    LEMON_REQUIRE(outt_dev != nullptr, "null pointer");
    return preprocess_impl(img_dev, batch, in_h, in_w, kk_h_dev, bnd_h_dev, ks_h, kk_v_dev, bnd_v_dev, ks_v, out_size, max_rows_per_block,
                           rows_per_block, mean3_host, std3_host, patch, reinterpret_cast<float *>(outt_dev), outt_dev, stream);
}

// generic_transform for a ragged batch (images of different sizes in one packed uint8 HWC buffer): see include/lemon_hip.h
extern "C" int lemon_preprocess_ragged(const uint8_t *data_dev, int64_t data_bytes, int64_t batch, const int64_t *aux_dev, int64_t h_blocks,
                                       int64_t v_blocks, const int32_t *plans_dev, const int32_t *taps_dev, uint8_t *work_dev,
                                       int out_size, const float *mean3_host, const float *std3_host, int patch, int operand,
                                       void *out_dev, void *stream) {
    LEMON_REQUIRE(batch >= 0 && data_bytes >= 0 && out_size > 0 && h_blocks >= 0 && v_blocks >= 0,
                  "batch, data_bytes, block counts >= 0, out_size > 0");
    LEMON_REQUIRE(patch >= 0 && (patch == 0 || out_size % patch == 0), "patch must divide out_size");
    if (operand)
        LEMON_REQUIRE(patch > 0 && patch % 4 == 0 && out_size % 4 == 0 && (3 * patch * patch) % 16 == 0,
                      "operand form: patch a positive multiple of 4 with 3 patch^2 a multiple of 16 (the operand's k16 steps)");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(data_dev && aux_dev && plans_dev && taps_dev && work_dev && mean3_host && std3_host && out_dev, "null pointer");
    LEMON_REQUIRE(v_blocks >= batch && h_blocks < ((int64_t)1 << 31) && v_blocks < ((int64_t)1 << 31), "block counts");
    LEMON_REQUIRE((((uintptr_t)out_dev) & 15) == 0 && (((uintptr_t)work_dev) & 3) == 0, "out_dev 16-byte, work_dev 4-byte aligned");
    RaggedParams p;
    p.data = data_dev; p.desc = aux_dev; p.hpre = aux_dev + 4 * batch; p.vpre = p.hpre + batch + 1; p.ioff = p.vpre + batch + 1;
    p.plans = plans_dev; p.taps = taps_dev; p.work = work_dev;
    p.out = operand ? nullptr : reinterpret_cast<float *>(out_dev);
    p.out_t = operand ? reinterpret_cast<unsigned short *>(out_dev) : nullptr;
    p.n = batch; p.data_bytes = data_bytes; p.S = out_size; p.patch = patch;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean3_host[c]; p.stdv[c] = std3_host[c]; }
    if (h_blocks) {
        hipLaunchKernelGGL(k_ragged_h, dim3((unsigned)h_blocks), dim3(256), 0, (hipStream_t)stream, p);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ragged_v, dim3((unsigned)v_blocks), dim3(256), 0, (hipStream_t)stream, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
