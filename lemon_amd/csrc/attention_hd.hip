// Self-attention at head dims 72 .. 128 (ViT-H/14: 80, g/14: 88, bigG/14: 104; gfx950 only), behind
// lemon_attention_set_head_dims (attention.hip, off by default).
//
// k_attention_hdx_stream<HDP, SPLIT> is the body of k_attention_hd64_stream<SPLIT> (attention.hip: fp32 arithmetic,
// v_mfma_f32_32x32x2_f32, four waves, 64 keys per block, grid (batch * heads, query blocks)) with the head dimension `hd`
// (a multiple of 8) as a run-time argument and the padded size HDP (96 or 128) as a template argument:
//   S^T = K Q^T      hd / 2 MFMA steps: lane half h holds dims h * hd / 2 + i of its query row (registers) and reads the
//                    same dims of its key row from LDS -- no padding, the k-steps simply stop at hd / 2
//   O^T += V^T P^T   ceil(hd / 32) output tiles of 32 dims.  Output row d of a tile depends on V's column d alone: whatever
//                    LDS holds in columns [hd, 32 ceil(hd / 32)) ends in output columns >= hd, which are never stored
// LDS rows have pitch HDP + 4 floats (100 / 132: 16-byte aligned, 4 mod 32 banks as the 68 of the base kernel).
// With hd = 64 the operations per key tile and their order are those of k_attention_hd64_stream (the test forces this kernel
// onto head_dim 64 with mode 2 and compares all four output forms for equality).
// One kernel for every 1 <= L <= LEMON_ATTENTION_MAX_SEQ and for both selections of lemon_attention_set_f16.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "common.hpp"
#include "split3.hpp"
#include "attention_hd64.hpp"   // f32x16, store_row8

namespace {

constexpr int X_WMAX = 4, X_TB = 2, X_KB = 32 * X_TB;      // waves per workgroup, key tiles and keys per block
static_assert(2 * X_TB >= X_WMAX, "the output image (32 rows per wave) must fit the K and V regions");

// the query tiles [tile0, tile0 + ntiles) of query block qb out of nqb (even deal; ntiles <= blockDim.x / 64)
__device__ __forceinline__ void stream_tiles(int TJ, int qb, int nqb, int &tile0, int &ntiles) {
    tile0 = (int)(((long long)qb * TJ) / nqb);
    ntiles = (int)(((long long)(qb + 1) * TJ) / nqb) - tile0;
}

// LDS: 2 x 64 rows x (HDP + 4) floats = 51.2 KB (HDP 96: three workgroups per CU, hence a budget of 168 registers, 147 used) or
// 67.6 KB (HDP 128: two workgroups, budget 256, 179 used -- the query half row and the output tiles alone are 128)
template <int HDP, int SPLIT>
__global__ __launch_bounds__(64 * X_WMAX, HDP == 96 ? 3 : 2) void k_attention_hdx_stream(const float *__restrict__ qkv, int L, int H, int hd,
                                                                                           int causal, float c_exp, float *__restrict__ out) {
    constexpr int PITCH = HDP + 4;                 // LDS row pitch in floats
    constexpr int NC = HDP / 4;                    // 16-byte chunk slots per staged row (hd / 4 of them hold data)
    constexpr int NQ = HDP / 8;                    // float4 steps of a query half row at most
    constexpr int NT = HDP / 32;                   // output tiles at most
    // the host sends 64 <= hd <= 96 to HDP 96 and 96 < hd <= 128 to HDP 128: these steps and tiles run at every hd
    constexpr int NQ_MIN = HDP == 96 ? 8 : 13, NT_MIN = HDP == 96 ? 2 : 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // K rows, then V rows
    float *sK = smem, *sV = smem + X_KB * PITCH;
    const int TJ = (L + 31) >> 5;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int nthr = blockDim.x;
    const int64_t b = blockIdx.x / H;
    const int head = blockIdx.x % H;
    const int hd2 = hd >> 1, nc4 = hd >> 2, nc8 = hd >> 3;
    int tile0, ntiles;
    stream_tiles(TJ, blockIdx.y, gridDim.y, tile0, ntiles);
    const bool active = wave < ntiles;             // (a block of the even deal may hold one tile less than there are waves)
    const int gt = tile0 + wave;                   // this wave's query tile
    const int64_t tok_stride = (int64_t)3 * H * hd;
    const float *base = qkv + b * L * tok_stride + head * hd;
    const unsigned tok_bytes = (unsigned)(3 * H * hd * 4);     // (offsets inside one key block: 64 tokens x tok_bytes < 2^32, host-checked)

    const int qi = 32 * gt + l31;
    const int qrow = qi < L ? qi : L - 1;
    float q[4 * NQ];
    {
        const float *src = base + (int64_t)qrow * tok_stride + h * hd2;
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (u < NQ_MIN || 4 * u < hd2) t = *reinterpret_cast<const float4 *>(src + 4 * u);
            q[4 * u] = t.x; q[4 * u + 1] = t.y; q[4 * u + 2] = t.z; q[4 * u + 3] = t.w;
        }
    }
    f32x16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[t][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int kt_end = causal ? (tile0 + ntiles < TJ ? tile0 + ntiles : TJ) : TJ;   // key tiles the workgroup needs
    const int tj_end = !active ? 0 : causal ? (gt + 1 < TJ ? gt + 1 : TJ) : TJ;       // ... and this wave
    constexpr int CH = 4;
    for (int kb = 0; kb * X_TB < kt_end; ++kb) {
        if (kb > 0) __syncthreads();               // all waves are past their last read of the previous block
        const int nrows = 32 * ((kt_end - kb * X_TB) < X_TB ? (kt_end - kb * X_TB) : X_TB);
        const char *kbase = reinterpret_cast<const char *>(base + (int64_t)kb * X_KB * tok_stride + H * hd);
        for (int p0 = 0; p0 < nrows * NC; p0 += CH * nthr) {
#pragma unroll
            for (int kv = 0; kv < 2; ++kv) {
                float4 reg[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id / NC, c = id % NC;
                    reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (id < nrows * NC && c < nc4 && kb * X_KB + r < L)
                        reg[i] = *reinterpret_cast<const float4 *>(kbase + (size_t)kv * H * hd * 4 + ((unsigned)r * tok_bytes + 16u * (unsigned)c));
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id / NC, c = id % NC;
                    if (id < nrows * NC && c < nc4) *reinterpret_cast<float4 *>(&(kv == 0 ? sK : sV)[r * PITCH + 4 * c]) = reg[i];
                }
            }
        }
        __syncthreads();
        const int t_hi = (kb + 1) * X_TB < tj_end ? (kb + 1) * X_TB : tj_end;
        for (int tj = kb * X_TB; tj < t_hi; ++tj) {
            const int tl = tj - kb * X_TB;
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            const float *krow = &sK[(32 * tl + l31) * PITCH + h * hd2];
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                if (u < NQ_MIN || 4 * u < hd2) {   // (uniform: hd / 2 is a multiple of 4)
                    const float4 k4 = *reinterpret_cast<const float4 *>(krow + 4 * u);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, q[4 * u], s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, q[4 * u + 1], s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, q[4 * u + 2], s, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, q[4 * u + 3], s, 0, 0, 0);
                }
            }
            // masks only where a tile can hold a masked key (the last tile, the wave's diagonal tile): elsewhere the select
            // keeps every score, and multiplying the accumulators by alpha = 1 keeps every bit -- both are skipped
            if (32 * tj + 32 > L || (causal && tj == gt)) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = 32 * tj + (e & 3) + 8 * (e >> 2) + 4 * h;
                    const bool ok = j < L && (!causal || j <= qi);
                    s[e] = ok ? s[e] : -INFINITY;
                }
            }
            float mt = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) mt = fmaxf(mt, s[e]);
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            const float alpha = exp2f((m_run - m_new) * c_exp);
            float lt = 0.f;
            const float pbias = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = exp2f((s[e] - m_new) * c_exp + pbias);
                lt += s[e];
            }
            lt += __shfl_xor(lt, 32);
            l_run = l_run * alpha + lt;
            m_run = m_new;
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[t][e] *= alpha;
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float *vrow = &sV[(32 * tl + (m & 3) + 8 * (m >> 2) + 4 * h) * PITCH + l31];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < NT_MIN || 32 * t < hd) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * t], s[m], o[t], 0, 0, 0);
            }
        }
    }
    // the output tile goes through LDS (fp32 rows at the K / V pitch over both regions: 4 waves x 32 rows = their 128 rows)
    // and leaves as whole rows, hd / 8 lanes per token
    __syncthreads();
    {
        const float inv = 1.0f / l_run;
        float *dstl = &sK[(32 * wave + l31) * PITCH];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4 *>(dstl + 32 * t + 8 * g + 4 * h) =
                    make_float4(o[t][4 * g] * inv, o[t][4 * g + 1] * inv, o[t][4 * g + 2] * inv, o[t][4 * g + 3] * inv);
    }
    __syncthreads();
    const int rows_l = nthr >> 1;                   // 32 rows per wave
    for (int id = tid; id < rows_l * nc8; id += nthr) {
        // (tile-major operand: the 16-byte slots of consecutive ROWS are adjacent, so consecutive lanes take consecutive rows)
        const int rl = SPLIT == 3 ? id % rows_l : id / nc8, c8 = SPLIT == 3 ? id / rows_l : id % nc8;
        const int r = 32 * tile0 + rl;
        if (rl < 32 * ntiles && r < L) {
            const float4 v0 = *reinterpret_cast<const float4 *>(&sK[rl * PITCH + 8 * c8]);
            const float4 v1 = *reinterpret_cast<const float4 *>(&sK[rl * PITCH + 8 * c8 + 4]);
            store_row8<SPLIT>(out, b * L + r, H, hd, nc8, head, c8, v0, v1);
        }
    }
}

namespace plan = lemon_attn_plan;
static_assert(plan::X_WMAX == X_WMAX && plan::X_TB == X_TB && plan::X_KB == X_KB && plan::HD == HD && plan::HDX_NARROW == 96 && plan::HDX_MAX == 128 &&
              plan::hdx_lds(96) == 2 * X_KB * (96 + 4) * (int)sizeof(float), "attention_plan.hpp mirrors the kernel's geometry, LDS pitch and the HDP each hd takes");

// the instantiations, four output forms (SPLIT 0 .. 3) per plan::Form of this unit, in the order of plan::FACTS[].slot
typedef void (*HdxKernel)(const float *, int, int, int, int, float, float *);
constexpr HdxKernel KERNELS[] = {
    k_attention_hdx_stream<96, 0>, k_attention_hdx_stream<96, 1>, k_attention_hdx_stream<96, 2>, k_attention_hdx_stream<96, 3>,
    k_attention_hdx_stream<128, 0>, k_attention_hdx_stream<128, 1>, k_attention_hdx_stream<128, 2>, k_attention_hdx_stream<128, 3>,
};
constexpr int N_KERNELS = sizeof(KERNELS) / sizeof(KERNELS[0]);
static_assert(N_KERNELS == 4 * (plan::FACTS[plan::HDX_128].slot + 1) && plan::FACTS[plan::HDX_96].slot == 0, "four kernels per plan::Form of this unit");
LemonLdsAttr g_attr[N_KERNELS];

}  // namespace

int lemon_attention_hdx(const plan::Plan &p, int split, const float *qkv_dev, int seq_len, int heads, int causal, float *out_dev, hipStream_t stream) {
    const float c_exp = (float)(1.44269504088896340736 / sqrt((double)p.hd));       // log2(e) / sqrt(hd)
    return lemon_attention_launch(KERNELS, g_attr, p, split, stream, qkv_dev, seq_len, heads, p.hd, causal, c_exp, out_dev);
}
