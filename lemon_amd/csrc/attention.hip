// Fused multi-head self-attention for the CLIP towers of the embedding stage (gfx950 only).
//
// Replaces, inside encode_image / encode_text (lib/models/downstream_models.py:30-41 -> HF CLIPAttention;
// in-tree twin lib/models/chexzero_clip.py:191-212 nn.MultiheadAttention), the chain
//   view/permute(qkv) -> softmax(q k^T / sqrt(hd) [+ causal mask]) v -> transpose -> reshape
// with ONE pass: reads the packed projection output qkv[B, L, 3, H, 64] (what the fused QKV GEMM
// writes) and writes out[B, L, H*64] (what the output projection reads).  No [B,H,L,L] matrix, no
// permute copies: algorithmic HBM traffic 16*H*64 B per token (3 reads + 1 write).
//
// (Up to 288 tokens; longer sequences, to LEMON_ATTENTION_MAX_SEQ: the streaming kernels at the end of the namespace.)
// One workgroup per (batch, head); wave t owns queries 32t..32t+31.  K and V of the head are staged in
// LDS (row pitch 68 floats: 16-B aligned, conflict-free 128-bit reads).  Per 32-key tile:
//   S^T = K Q^T      32 x v_mfma_f32_32x32x2_f32   A = K rows from LDS, B = the wave's Q rows (registers)
//                    -> lane (i = lane&31, h) holds its OWN query's 16 scores: softmax statistics are
//                       in-lane reductions plus one cross-half shuffle (flash-style running max / sum)
//   O^T += V^T P^T   2 x 16 MFMAs: B = the score registers as they are, A = V columns from LDS
// fp32 throughout (the reference runs the encoders in fp32).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.hpp"
#include "split3.hpp"
#include "attention_hd64.hpp"

namespace {

// The kernels of seq_len <= 288: the bodies (layout, scheduling and what the template arguments select) are in
// attention_hd64.hpp, shared with attention_varlen.hip
template <int SPLIT, bool F16>
__global__ __launch_bounds__(576) void k_attention_hd64(const float *__restrict__ qkv, int L, int H, int causal,
                                                        float *__restrict__ out) {
    attention_general<SPLIT, F16, false>(qkv, L, H, causal, nullptr, out);
}

template <int SPLIT>
__global__ __launch_bounds__(576, 4) void k_attention_hd64_f16(const float *__restrict__ qkv, int L, int H, int causal,
                                                            float *__restrict__ out) {
    attention_staged<SPLIT, false>(qkv, L, H, causal, nullptr, out);
}

template <int TJ, int SPLIT, bool F16>
__global__ __launch_bounds__(64 * TJ, 3) void k_attention_hd64_short(const float *__restrict__ qkv, int L, int H, int causal,
                                                                  float *__restrict__ out) {
    attention_short<TJ, SPLIT, F16, false>(qkv, L, H, causal, nullptr, out);
}


// ---- streaming kernels: any L up to LEMON_ATTENTION_MAX_SEQ (the 577 tokens of ViT-L/14@336, 1025 at 448 px, long text contexts) ----
// The kernels above put one workgroup on a (batch, head) and keep all keys of the head in LDS: nine waves and 288 keys are
// their limit.  Here the grid is (batch * heads, query blocks): the TJ query tiles (32 queries = one wave, as above) are dealt
// evenly to ceil(TJ / WMAX) workgroups of ceil(TJ / blocks) waves (split-fp16 form, 577 tokens: 19 tiles -> 3 blocks of 6 / 6 / 7
// tiles, seven waves each), and the keys pass through LDS in blocks of TB tiles (split-fp16 form: 128 keys = 64 KB of fp16
// planes), so that two workgroups share a CU and one's staging runs under the other's MFMA loop -- the place the 197-token
// kernel above lives at.  K and V of a head are re-read once per query block (L2 traffic: 577 x 512 B per head).
// Causal: a workgroup stops at the key block of its last query tile, a wave at its own diagonal tile.
// Per key tile the operations, their order and therefore the bits are those of the kernels above (tests force these kernels
// onto 64 < L <= 288 with lemon_attention_set_stream_min and compare for equality).
constexpr int STREAM_WMAX = 8;    // waves per workgroup at most: two workgroups = four waves per SIMD at <= 128 registers
constexpr int STREAM_TB = 4;      // key tiles per block (the largest of the two forms: the host's offset guard is written for it)
constexpr int STREAM_KB = 32 * STREAM_TB;

// the query tiles [tile0, tile0 + ntiles) of query block qb out of nqb (even deal; ntiles <= blockDim.x / 64)
__device__ __forceinline__ void stream_tiles(int TJ, int qb, int nqb, int &tile0, int &ntiles) {
    tile0 = (int)(((long long)qb * TJ) / nqb);
    ntiles = (int)(((long long)(qb + 1) * TJ) / nqb) - tile0;
}

// fp32 arithmetic: the body of k_attention_hd64<SPLIT, false> (fp32 K / V rows at pitch 68, v_mfma_f32_32x32x2_f32)
// Four waves and 64 keys per block here (17 KB of K rows + 17 KB of V rows: FOUR workgroups per CU): this form is bound by the
// fp32 matrix pipe, and with eight waves and 128 keys -- two workgroups of seven waves at 577 / 1025 tokens, a SIMD holding
// four waves while its neighbour holds three, every barrier stalling half the CU -- it took 1.13-1.24 ms where this takes
// 0.88-1.03 ms (64 x 577 x 16 and 32 x 1025 x 12; six waves / 96 keys and two waves / 32 keys were slower than either).
constexpr int S32_WMAX = 4, S32_TB = 2, S32_KB = 32 * S32_TB;
static_assert(2 * S32_TB >= S32_WMAX, "the output image (32 rows per wave) must fit the K and V regions");
template <int SPLIT>
__global__ __launch_bounds__(64 * S32_WMAX, 4) void k_attention_hd64_stream(const float *__restrict__ qkv, int L, int H, int causal,
                                                                              float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];      // K rows, then V rows: 2 x 64 x 68 floats = 34 KB
    float *sK = smem, *sV = smem + S32_KB * PITCH;
    const int TJ = (L + 31) >> 5;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int nthr = blockDim.x;
    const int64_t b = blockIdx.x / H;
    const int head = blockIdx.x % H;
    int tile0, ntiles;
    stream_tiles(TJ, blockIdx.y, gridDim.y, tile0, ntiles);
    const bool active = wave < ntiles;             // (a block of the even deal may hold one tile less than there are waves)
    const int gt = tile0 + wave;                   // this wave's query tile
    const int64_t tok_stride = (int64_t)3 * H * HD;
    const float *base = qkv + b * L * tok_stride + head * HD;
    const unsigned tok_bytes = (unsigned)(3 * H * HD * 4);     // (offsets inside one key block: <= 128 tokens x tok_bytes < 2^32, host-checked)

    const int qi = 32 * gt + l31;
    const int qrow = qi < L ? qi : L - 1;
    float q[32];
    {
        const float *src = base + (int64_t)qrow * tok_stride + 32 * h;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 t = *reinterpret_cast<const float4 *>(src + 4 * u);
            q[4 * u] = t.x; q[4 * u + 1] = t.y; q[4 * u + 2] = t.z; q[4 * u + 3] = t.w;
        }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    const float c_exp = 0.125f * 1.44269504088896340736f;   // 1/sqrt(64) * log2(e)

    const int kt_end = causal ? (tile0 + ntiles < TJ ? tile0 + ntiles : TJ) : TJ;   // key tiles the workgroup needs
    const int tj_end = !active ? 0 : causal ? (gt + 1 < TJ ? gt + 1 : TJ) : TJ;       // ... and this wave
    constexpr int CH = 4;
    for (int kb = 0; kb * S32_TB < kt_end; ++kb) {
        if (kb > 0) __syncthreads();               // all waves are past their last read of the previous block
        const int nrows = 32 * ((kt_end - kb * S32_TB) < S32_TB ? (kt_end - kb * S32_TB) : S32_TB);
        const char *kbase = reinterpret_cast<const char *>(base + (int64_t)kb * S32_KB * tok_stride + H * HD);
        for (int p0 = 0; p0 < nrows * 16; p0 += CH * nthr) {
#pragma unroll
            for (int kv = 0; kv < 2; ++kv) {
                float4 reg[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id >> 4, c = id & 15;
                    reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (id < nrows * 16 && kb * S32_KB + r < L)
                        reg[i] = *reinterpret_cast<const float4 *>(kbase + (size_t)kv * H * HD * 4 + ((unsigned)r * tok_bytes + 16u * (unsigned)c));
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id >> 4, c = id & 15;
                    if (id < nrows * 16) *reinterpret_cast<float4 *>(&(kv == 0 ? sK : sV)[r * PITCH + 4 * c]) = reg[i];
                }
            }
        }
        __syncthreads();
        const int t_hi = (kb + 1) * S32_TB < tj_end ? (kb + 1) * S32_TB : tj_end;
        for (int tj = kb * S32_TB; tj < t_hi; ++tj) {
            const int tl = tj - kb * S32_TB;
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            const float *krow = &sK[(32 * tl + l31) * PITCH + 32 * h];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 k4 = *reinterpret_cast<const float4 *>(krow + 4 * u);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, q[4 * u], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, q[4 * u + 1], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, q[4 * u + 2], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, q[4 * u + 3], s, 0, 0, 0);
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
                for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float *vrow = &sV[(32 * tl + (m & 3) + 8 * (m >> 2) + 4 * h) * PITCH + l31];
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], s[m], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32], s[m], o1, 0, 0, 0);
            }
        }
    }
    // the output tile goes through LDS (fp32 rows at pitch 68 over the K and V regions: 4 waves x 32 rows = their 128 rows)
    // and leaves as whole rows, 8 lanes per token
    __syncthreads();
    {
        const float inv = 1.0f / l_run;
        float *dstl = &sK[(32 * wave + l31) * PITCH];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * h;
            *reinterpret_cast<float4 *>(dstl + c0) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4 *>(dstl + 32 + c0) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        }
    }
    __syncthreads();
    const int rows_l = nthr >> 1;                   // 32 rows per wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + i * nthr;
        const int rl = SPLIT == 3 ? id % rows_l : id >> 3, c8 = SPLIT == 3 ? id / rows_l : id & 7;
        const int r = 32 * tile0 + rl;
        if (rl < 32 * ntiles && r < L) {
            const float4 v0 = *reinterpret_cast<const float4 *>(&sK[rl * PITCH + 8 * c8]);
            const float4 v1 = *reinterpret_cast<const float4 *>(&sK[rl * PITCH + 8 * c8 + 4]);
            store_row8<SPLIT>(out, b * L + r, H, HD, HD / 8, head, c8, v0, v1);
        }
    }
}

// split-fp16 arithmetic: the body of k_attention_hd64_f16 (K and V split once at staging into fp16 hi / lo planes with the same
// XOR layouts, V read transposed by ds_read_b64_tr_b16, Q and the output through an fp32 staging image in the same 64 KB)
// (eight waves / 128 keys; four waves / 64 keys measured the same within 2 % at the non-causal shapes and 10 % slower at the causal one, two
// waves / 32 keys 25-45 % slower: this form waits for its vector ALU work, not for its barriers)
constexpr int S16_WMAX = STREAM_WMAX, S16_TB = STREAM_TB, S16_KB = 32 * S16_TB;
static_assert(2 * S16_TB >= S16_WMAX, "the fp32 staging image (32 rows of 256 B per wave) must fit the four planes");
template <int SPLIT>
__global__ __launch_bounds__(64 * S16_WMAX, 4) void k_attention_hd64_stream_f16(const float *__restrict__ qkv, int L, int H, int causal,
                                                                                  float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_c[];     // 64 KB: four planes of 128 keys = the fp32 [256][64] staging image
    constexpr int KB = S16_KB, TB = S16_TB;
    const int TJ = (L + 31) >> 5;
    char *sKh = smem_c, *sKl = smem_c + KB * 128, *sVh = smem_c + 2 * KB * 128, *sVl = smem_c + 3 * KB * 128;
    float *sQ = reinterpret_cast<float *>(smem_c);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int nthr = blockDim.x;
    const int64_t b = blockIdx.x / H;
    const int head = blockIdx.x % H;
    int tile0, ntiles;
    stream_tiles(TJ, blockIdx.y, gridDim.y, tile0, ntiles);
    const bool active = wave < ntiles;
    const int gt = tile0 + wave;                              // this wave's query tile
    const int64_t tok_stride = (int64_t)3 * H * HD;
    const float *base = qkv + b * L * tok_stride + head * HD;
    const unsigned tok_bytes = (unsigned)(3 * H * HD * 4);     // (offsets inside one key block: <= 128 tokens x tok_bytes < 2^32, host-checked)
    constexpr int CH = 5;
    const int kt_end = causal ? (tile0 + ntiles < TJ ? tile0 + ntiles : TJ) : TJ;   // key tiles the workgroup needs
    // key block kb -> fp16 hi / lo planes: K and V rows [kb KB, kb KB + nrows) of the head (zero beyond L), rows local to the block
    auto stage_block = [&](int kb) {
        const int nrows = 32 * ((kt_end - kb * TB) < TB ? (kt_end - kb * TB) : TB);
        const float *bbase = base + (int64_t)kb * KB * tok_stride;   // wave-uniform 64-bit base + 32-bit byte offset
        for (int p0 = 0; p0 < nrows * 16; p0 += CH * nthr) {
#pragma unroll
            for (int kv = 0; kv < 2; ++kv) {
                float4 reg[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id >> 4, c = id & 15;
                    reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (id < nrows * 16 && kb * KB + r < L)
                        reg[i] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(bbase + (kv + 1) * H * HD) + ((unsigned)r * tok_bytes + 16u * (unsigned)c));
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id >> 4, c = id & 15;
                    if (id < nrows * 16) {
                        h16x4 hi, lo;
                        split4u(reg[i], hi, lo);
                        const int o = kv == 0 ? r * 128 + ((((c >> 1) ^ ((r >> 1) & 7))) << 4) + (c & 1) * 8
                                              : r * 128 + ((c * 8) ^ (((r >> 1) & 1) << 6));
                        *reinterpret_cast<h16x4 *>((kv == 0 ? sKh : sVh) + o) = hi;
                        *reinterpret_cast<h16x4 *>((kv == 0 ? sKl : sVl) + o) = lo;
                    }
                }
            }
        }
    };
    // ---- the workgroup's Q rows through LDS (local row = 32 wave + l31; zero beyond its tiles and beyond L) ----
    {
        float4 qreg[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int id = tid + i * nthr, rl = id >> 4, c = id & 15, r = 32 * tile0 + rl;
            qreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rl < 32 * ntiles && r < L) qreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int id = tid + i * nthr, rl = id >> 4, c = id & 15;
            *reinterpret_cast<float4 *>(&sQ[stage_off(rl, c)]) = qreg[i];
        }
    }
    __syncthreads();
    const int ql_row = 32 * wave + l31;                       // local row of this lane's query
    const int qi = 32 * gt + l31;
    h16x8 qh[4], ql[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float4 a = *reinterpret_cast<const float4 *>(&sQ[stage_off(ql_row, 8 * h + 2 * u)]);
        const float4 c4 = *reinterpret_cast<const float4 *>(&sQ[stage_off(ql_row, 8 * h + 2 * u + 1)]);
        const float qv[8] = {a.x, a.y, a.z, a.w, c4.x, c4.y, c4.z, c4.w};
        split8u(qv, qh[u], ql[u]);
    }

    int koff[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) koff[u] = l31 * 128 + (((4 * h + u) ^ ((l31 >> 1) & 7)) << 4);
    const int g16 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int voff0 = (4 * (g16 >> 1) + q4) * 128 + (((16 * (g16 & 1) + 4 * p4) * 2) ^ ((q4 >> 1) << 6));
    const int voff1 = voff0 ^ 64;

    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    const float c_exp = 0.125f * 1.44269504088896340736f;     // 1/sqrt(64) * log2(e)
    const int tj_end = !active ? 0 : causal ? (gt + 1 < TJ ? gt + 1 : TJ) : TJ;
    for (int kb = 0; kb * TB < kt_end; ++kb) {
        __syncthreads();                                      // every lane has its query / all waves are past the previous block
        stage_block(kb);
        __syncthreads();
        const int t_hi = (kb + 1) * TB < tj_end ? (kb + 1) * TB : tj_end;
        for (int tj = kb * TB; tj < t_hi; ++tj) {
            const int tl = tj - kb * TB;                      // tile inside the block
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            const char *kh_t = sKh + tl * 4096, *kl_t = sKl + tl * 4096;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const h16x8 kh = *reinterpret_cast<const h16x8 *>(kh_t + koff[u]);
                const h16x8 kl = *reinterpret_cast<const h16x8 *>(kl_t + koff[u]);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[u], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[u], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[u], s, 0, 0, 0);
            }
            // masks only where a tile can hold a masked key: the last tile (keys >= L) and, causal, the wave's diagonal tile
            if (32 * tj + 32 > L || (causal && tj == gt)) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = 32 * tj + (e & 3) + 8 * (e >> 2) + 4 * h;
                    const bool ok = j < L && (!causal || j <= qi);
                    s[e] = ok ? s[e] : -INFINITY;
                }
            }
            float mt = s[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mt = fmaxf(mt, s[e]);
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            const float alpha = exp2f((m_run - m_new) * c_exp);
            float lt = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = __builtin_amdgcn_exp2f((s[e] - m_new) * c_exp + 10.0f);     // probabilities x 2^10 (l_run carries the factor, 1 / l_run removes it)
                lt += s[e];
            }
            lt += __shfl_xor(lt, 32);
            l_run = l_run * alpha + lt;
            m_run = m_new;
            if (!__all(alpha == 1.0f)) {                      // the running maximum moved for some query of the wave
#pragma unroll
                for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
            }
            const char *vh_t = sVh + tl * 4096, *vl_t = sVl + tl * 4096;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float pv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) pv[i] = s[8 * t + i];
                h16x8 ph, pl;
                split8u(pv, ph, pl);
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int vo = (half ? voff1 : voff0) + t * 2048;
                    const fp16x4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4v *)(vh_t + vo));
                    const fp16x4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4v *)(vh_t + vo + 1024));
                    const fp16x4v b0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4v *)(vl_t + vo));
                    const fp16x4v b1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4v *)(vl_t + vo + 1024));
                    h16x8 vh, vl;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        vh[e] = (_Float16)a0[e]; vh[4 + e] = (_Float16)a1[e];
                        vl[e] = (_Float16)b0[e]; vl[4 + e] = (_Float16)b1[e];
                    }
                    if (half == 0) {
                        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o0, 0, 0, 0);
                        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o0, 0, 0, 0);
                        o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o0, 0, 0, 0);
                    } else {
                        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o1, 0, 0, 0);
                        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o1, 0, 0, 0);
                        o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o1, 0, 0, 0);
                    }
                }
            }
        }
    }
    // the output tile goes through the buffer (every wave is past its last key tile)
    float *sO = sQ;
    __syncthreads();
    {
        const float inv = 1.0f / l_run;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * h;                     // columns c0 .. c0+3 (and 32 + c0 ..) of query qi
            *reinterpret_cast<float4 *>(&sO[stage_off(ql_row, c0 >> 2)]) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4 *>(&sO[stage_off(ql_row, 8 + (c0 >> 2))]) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        }
    }
    __syncthreads();
    const int rows_l = nthr >> 1;                             // 32 rows per wave
#pragma unroll
    for (int i = 0; i < 4; ++i) {                             // 8 lanes per token row, 8 values each: 16-byte stores in every form
        const int id = tid + i * nthr;
        const int rl = SPLIT == 3 ? id % rows_l : id >> 3, c8 = SPLIT == 3 ? id / rows_l : id & 7;
        const int r = 32 * tile0 + rl;
        if (rl < 32 * ntiles && r < L) {
            const float4 v0 = *reinterpret_cast<const float4 *>(&sO[stage_off(rl, 2 * c8)]);
            const float4 v1 = *reinterpret_cast<const float4 *>(&sO[stage_off(rl, 2 * c8 + 1)]);
            store_row8<SPLIT>(out, b * L + r, H, HD, HD / 8, head, c8, v0, v1);
        }
    }
}

}  // namespace

// ---- host side: attention_plan.hpp decides, lemon_attention_launch (common.hpp) launches from the unit's one table ----
namespace plan = lemon_attn_plan;
static_assert(plan::HD == HD && plan::PITCH == PITCH && plan::MAX_SEQ == LEMON_ATTENTION_MAX_SEQ && plan::E_INVALID == LEMON_E_INVALID &&
              plan::STREAM_WMAX == STREAM_WMAX && plan::STREAM_TB == STREAM_TB && plan::STREAM_KB == STREAM_KB && plan::S32_WMAX == S32_WMAX &&
              plan::S32_TB == S32_TB && plan::S32_KB == S32_KB && plan::S16_WMAX == S16_WMAX && plan::S16_TB == S16_TB && plan::S16_KB == S16_KB,
              "attention_plan.hpp mirrors attention_hd64.hpp, lemon_hip.h and the streaming kernels' geometry");
static_assert(S32_KB <= STREAM_KB && S16_KB <= STREAM_KB, "the plan's 32-bit-offset guard is written for the larger key block");

// the instantiations, four output forms (SPLIT 0 .. 3) per plan::Form of this unit, in the order of plan::FACTS[].slot
typedef void (*AttnKernel)(const float *, int, int, int, float *);
static constexpr AttnKernel KERNELS[] = {
    k_attention_hd64_short<1, 0, false>, k_attention_hd64_short<1, 1, false>, k_attention_hd64_short<1, 2, false>, k_attention_hd64_short<1, 3, false>,
    k_attention_hd64_short<1, 0, true>, k_attention_hd64_short<1, 1, true>, k_attention_hd64_short<1, 2, true>, k_attention_hd64_short<1, 3, true>,
    k_attention_hd64_short<2, 0, false>, k_attention_hd64_short<2, 1, false>, k_attention_hd64_short<2, 2, false>, k_attention_hd64_short<2, 3, false>,
    k_attention_hd64_short<2, 0, true>, k_attention_hd64_short<2, 1, true>, k_attention_hd64_short<2, 2, true>, k_attention_hd64_short<2, 3, true>,
    k_attention_hd64<0, false>, k_attention_hd64<1, false>, k_attention_hd64<2, false>, k_attention_hd64<3, false>,
    k_attention_hd64<0, true>, k_attention_hd64<1, true>, k_attention_hd64<2, true>, k_attention_hd64<3, true>,
    k_attention_hd64_f16<0>, k_attention_hd64_f16<1>, k_attention_hd64_f16<2>, k_attention_hd64_f16<3>,
    k_attention_hd64_stream<0>, k_attention_hd64_stream<1>, k_attention_hd64_stream<2>, k_attention_hd64_stream<3>,
    k_attention_hd64_stream_f16<0>, k_attention_hd64_stream_f16<1>, k_attention_hd64_stream_f16<2>, k_attention_hd64_stream_f16<3>,
};
constexpr int N_KERNELS = sizeof(KERNELS) / sizeof(KERNELS[0]);
static_assert(N_KERNELS == 4 * (plan::FACTS[plan::STREAM_F16].slot + 1) && plan::FACTS[plan::HDX_96].unit == plan::UNIT_HD, "four kernels per plan::Form of this unit");
static LemonLdsAttr g_attr[N_KERNELS];

// The calling thread's knobs (plan::Knobs says what they select) and the kernel it launched last.  Per calling THREAD (round 5:
// the arithmetic was one unsynchronised process-wide int, so two embedders in different GEMM modes -- or a bf16x6 re-embedding next
// to an f16x3 pass -- could pick each other's kernel): the host mirror calls lemon_attention_set_f16 in front of every tower pass.
// Every thread starts with $LEMON_ATTN_F16 (0: fp32 arithmetic), $LEMON_ATTN_HEAD_DIMS (1 or 2) and the two tuning knobs.
LemonAttnThread &lemon_attention_thread() {
    static const plan::Knobs start = [] {
        const char *f16 = getenv("LEMON_ATTN_F16"), *hd = getenv("LEMON_ATTN_HEAD_DIMS"), *sh = getenv("LEMON_ATTN_SHORT"), *ge = getenv("LEMON_ATTN_GENERAL");
        return plan::Knobs{(f16 && f16[0] == '0') ? 0 : 1, plan::ONE_WG_MAX_SEQ, (hd && (hd[0] == '1' || hd[0] == '2') && !hd[1]) ? hd[0] - '0' : 0,
                           sh && sh[0] == '0', ge && !strcmp(ge, "old")};
    }();
    thread_local LemonAttnThread t = {start, ""};
    return t;
}

extern "C" int lemon_attention_set_f16(int on) {
    return std::exchange(lemon_attention_thread().knobs.arithmetic, on == 2 ? 2 : on ? 1 : 0) != 0;
}

extern "C" int lemon_attention_set_stream_min(int seq_len) {
    if (seq_len < 64 || seq_len > plan::ONE_WG_MAX_SEQ) {
        lemon_set_error("lemon_attention_set_stream_min: seq_len must be in 64 .. 288");
        return LEMON_E_INVALID;
    }
    return std::exchange(lemon_attention_thread().knobs.stream_min, seq_len);
}

extern "C" int lemon_attention_set_head_dims(int mode) {
    if (mode < 0 || mode > 2) {
        lemon_set_error("lemon_attention_set_head_dims: mode must be 0, 1 or 2");
        return LEMON_E_INVALID;
    }
    return std::exchange(lemon_attention_thread().knobs.head_dims, mode);
}

extern "C" int lemon_attention_get_head_dims(void) { return lemon_attention_thread().knobs.head_dims; }
extern "C" const char *lemon_attention_last_kernel(void) { return lemon_attention_thread().last_kernel; }

// split = the output form 0 .. 3 (out_dev: see the entries)
static int attention_entry(int split, const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim, int causal, float *out_dev,
                           void *stream) {
    const plan::Plan p = plan::plan(lemon_attention_thread().knobs, batch, seq_len, heads, head_dim, split, false);
    if (p.early) return lemon_attention_refuse(p.early);
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(qkv_dev && out_dev, "null pointer");
    LEMON_REQUIRE((((uintptr_t)qkv_dev) & 15) == 0 && (((uintptr_t)out_dev) & 15) == 0, "16-byte alignment");
    if (p.late) return lemon_attention_refuse(p.late);
    if (plan::FACTS[p.form].unit == plan::UNIT_HD) return lemon_attention_hdx(p, split, qkv_dev, seq_len, heads, causal, out_dev, (hipStream_t)stream);
    return lemon_attention_launch(KERNELS, g_attr, p, split, (hipStream_t)stream, qkv_dev, seq_len, heads, causal, out_dev);
}

extern "C" int lemon_attention_f32(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                   int causal, float *out_dev, void *stream) {
    return attention_entry(0, qkv_dev, batch, seq_len, heads, head_dim, causal, out_dev, stream);
}

// lemon_attention_f32 whose output is the split activation operand of lemon_linear_bf16x6: out6_dev [batch*seq_len, 6*heads*64] bf16
extern "C" int lemon_attention_split3(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                      int causal, uint16_t *out6_dev, void *stream) {
    return attention_entry(1, qkv_dev, batch, seq_len, heads, head_dim, causal, reinterpret_cast<float *>(out6_dev), stream);
}

// ... of lemon_linear_f16x3: out3_dev [batch*seq_len, 3*heads*64] fp16
extern "C" int lemon_attention_f16x3(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                     int causal, uint16_t *out3_dev, void *stream) {
    return attention_entry(2, qkv_dev, batch, seq_len, heads, head_dim, causal, reinterpret_cast<float *>(out3_dev), stream);
}

// ... as the tile-major fp16 activation operand of lemon_linear_f16x3t (the output projection in the hand-written GEMM):
// outt_dev holds ceil(batch*seq_len / 128) * 128 x heads*64 x 2 halves, 16-byte aligned
extern "C" int lemon_attention_f16x3t(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                      int causal, uint16_t *outt_dev, void *stream) {
    return attention_entry(3, qkv_dev, batch, seq_len, heads, head_dim, causal, reinterpret_cast<float *>(outt_dev), stream);
}
