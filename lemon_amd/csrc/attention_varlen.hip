// Bidirectional self-attention with a key length PER SEQUENCE (gfx950 only): the padding mask of a BERT text tower.
//
// Replaces, inside encode_text of the `biomed_clip` branch (lib/models/utils.py:72-78 -> open_clip HFTextEncoder -> HF
// BertSelfAttention called with attention_mask = ids != pad), the chain
//   view/permute(qkv) -> softmax(q k^T / sqrt(64) + (1 - mask) * min) v -> transpose -> reshape
// for captions padded BEHIND their last token: sequence b of qkv[B, L, 3, H, 64] holds n_b = clamp(lengths[b], 1, L) tokens.
//   * rows t <  n_b of out[B, L, H*64] (any output form of attention.hip): attention of query t over keys 0 .. n_b - 1;
//   * rows t >= n_b: zeros (selected at the store, whatever the query row holds);
//   * K, V and Q rows t >= n_b are never LOADED: the r < L guards of the sibling kernels' loads are r < n_b here, so that
//     NaN, Inf or values beyond the fp16 range in a padded row cannot reach a product (0 * NaN) -- the mask j < n_b on the
//     scores alone would not give that.
// One workgroup per (sequence, head) as in attention.hip (seq_len <= 288), so n_b is a workgroup-uniform scalar.  The three
// kernels restate k_attention_hd64_short, k_attention_hd64<SPLIT, false> and k_attention_hd64_f16 of attention.hip without
// their causal branches: LDS layout, tile walk, arithmetic and summation order are those of the sibling at the same seq_len, a
// masked key adds exact zeros, and so a row t < n_b carries the bits of the plain kernel run on qkv[b, :n_b] wherever both have
// the same number of key tiles (tests/test_gpu_attention_varlen.py).  The comments on layout and scheduling live with the
// siblings; what is said here is what differs.
//   * a key tile entirely beyond n_b is skipped (its probabilities are exact zeros: the running maximum, sum and accumulators
//     would not move), a wave whose 32 queries all lie beyond n_b skips every product; both still take part in staging and
//     in every barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <mutex>
#include <algorithm>

#include "common.hpp"
#include "split3.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 fp16x4v __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) fp16x4v lds_fp16x4v;

constexpr int HD = 64;        // head dimension
constexpr int PITCH = 68;     // LDS row pitch in floats (fp32 K / V rows)

// (attention.hip: split8 -- lo scaled by 2^11, the short kernels; split8u / split4u -- lo unscaled, the staged kernel)
__device__ __forceinline__ void split8(const float *v, h16x8 &hi, h16x8 &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 hh = (_Float16)v[e];
        hi[e] = hh; lo[e] = (_Float16)((v[e] - (float)hh) * 2048.0f);
    }
}
__device__ __forceinline__ void split8u(const float *v, h16x8 &hi, h16x8 &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 hh = (_Float16)v[e];
        hi[e] = hh; lo[e] = (_Float16)(v[e] - (float)hh);
    }
}
__device__ __forceinline__ void split4u(const float4 v, h16x4 &hi, h16x4 &lo) {
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const _Float16 hh = (_Float16)x[e];
        hi[e] = hh; lo[e] = (_Float16)(x[e] - (float)hh);
    }
}

// the sequence's key count, clamped on the device (the host cannot read the values): a scalar of the workgroup
__device__ __forceinline__ int seq_keys(const int *__restrict__ lengths, int64_t b, int L) {
    const int n = lengths[b];
    return __builtin_amdgcn_readfirstlane(n < 1 ? 1 : (n > L ? L : n));
}

// rows of eight values leave in every output form with 16-byte stores (the tail of the sibling kernels' store loops)
template <int SPLIT>
__device__ __forceinline__ void store_row8(float *__restrict__ out, int64_t row, int H, int head, int c8, const float4 v0, const float4 v1) {
    if (SPLIT == 3)
        lemon_split::store_tiled8<lemon_split::TILE_A_ROWS, false>(reinterpret_cast<unsigned short *>(out), row, H * HD, head * (HD / 8) + c8, v0, v1);
    else if (SPLIT)
        lemon_split::store_split8<(SPLIT == 1 || SPLIT == 2) ? SPLIT : 1, false>(reinterpret_cast<unsigned short *>(out) + row * lemon_split::split_segments(SPLIT == 3 ? 2 : SPLIT) * (int64_t)(H * HD), H * HD,
                                         head * (HD / 8) + c8, v0, v1);
    else {
        float *dst = out + (row * H + head) * HD + 8 * c8;
        *reinterpret_cast<float4 *>(dst) = v0;
        *reinterpret_cast<float4 *>(dst + 4) = v1;
    }
}

// ---- seq_len <= 64: k_attention_hd64_short with keys [0, n) ------------------------------------------------------------------
template <int TJ, int SPLIT, bool F16>
__global__ __launch_bounds__(64 * TJ, 3) void k_attnvl_short(const float *__restrict__ qkv, int L, int H, const int *__restrict__ lengths,
                                                            float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float sKV[32 * TJ * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int64_t b = blockIdx.x / H;
    const int head = blockIdx.x % H;
    const int n = seq_keys(lengths, b, L);
    const bool wave_on = 32 * wave < n;             // (wave-uniform) some query of this wave is inside the sequence
    const int64_t tok_stride = (int64_t)3 * H * HD;
    const float *base = qkv + b * L * tok_stride + head * HD;
    float4 kreg[8], vreg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * 64 * TJ, r = id >> 4, c = id & 15;
        kreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) kreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c + H * HD);
    }
    const int qi = 32 * wave + l31;
    {
        float4 qreg[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int id = tid + i * 64 * TJ, r = id >> 4, c = id & 15;
            qreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < n) qreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int id = tid + i * 64 * TJ, r = id >> 4, c = id & 15;
            *reinterpret_cast<float4 *>(&sKV[r * PITCH + 4 * c]) = qreg[i];
        }
    }
    __syncthreads();
    float q[32];
    {
        const float *src = &sKV[qi * PITCH + 32 * h];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 t = *reinterpret_cast<const float4 *>(src + 4 * u);
            q[4 * u] = t.x; q[4 * u + 1] = t.y; q[4 * u + 2] = t.z; q[4 * u + 3] = t.w;
        }
    }
    __syncthreads();                                // every lane has its query row: the buffer now takes K
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * 64 * TJ, r = id >> 4, c = id & 15;
        *reinterpret_cast<float4 *>(&sKV[r * PITCH + 4 * c]) = kreg[i];
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * 64 * TJ, r = id >> 4, c = id & 15;
        vreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) vreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c + 2 * H * HD);
    }
    f32x16 s[TJ];
    h16x8 qh[4], ql[4];
    if (F16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) split8(q + 8 * u, qh[u], ql[u]);
    }
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
        f32x16 sa, sb;
#pragma unroll
        for (int e = 0; e < 16; ++e) { sa[e] = 0.f; sb[e] = 0.f; }
        if (wave_on && 32 * tj < n) {               // (a tile beyond n: every score is masked below)
            const float *krow = &sKV[(32 * tj + l31) * PITCH + 32 * h];
            if (F16) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 k0 = *reinterpret_cast<const float4 *>(krow + 8 * u), k1 = *reinterpret_cast<const float4 *>(krow + 8 * u + 4);
                    const float kv[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
                    h16x8 kh, kl;
                    split8(kv, kh, kl);
                    sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[u], sa, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[u], sb, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[u], sb, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float4 k4 = *reinterpret_cast<const float4 *>(krow + 4 * u);
                    sa = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, q[4 * u], sa, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, q[4 * u + 1], sb, 0, 0, 0);
                    sa = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, q[4 * u + 2], sa, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, q[4 * u + 3], sb, 0, 0, 0);
                }
            }
        }
        if (F16) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[tj][e] = sa[e] + sb[e] * 0.00048828125f;
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[tj][e] = sa[e] + sb[e];
        }
    }
    // mask (keys beyond the sequence), row maximum, exponentials, row sum
    const float c_exp = 0.125f * 1.44269504088896340736f;   // 1/sqrt(64) * log2(e)
    float mx = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = 32 * tj + (e & 3) + 8 * (e >> 2) + 4 * h;
            s[tj][e] = j < n ? s[tj][e] : -INFINITY;
            mx = fmaxf(mx, s[tj][e]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32));           // finite: key 0 is inside every sequence (n >= 1)
    float lsum = 0.f;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[tj][e] = exp2f((s[tj][e] - mx) * c_exp);
            lsum += s[tj][e];
        }
    lsum += __shfl_xor(lsum, 32);

    __syncthreads();                                // every wave is done with K
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * 64 * TJ, r = id >> 4, c = id & 15;
        *reinterpret_cast<float4 *>(&sKV[r * PITCH + 4 * c]) = vreg[i];
    }
    __syncthreads();

    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    if (F16) {
        f32x16 c0, c1;                                // the 2^11-scaled cross terms
#pragma unroll
        for (int e = 0; e < 16; ++e) { c0[e] = 0.f; c1[e] = 0.f; }
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
            if (!(wave_on && 32 * tj < n)) continue;  // (p = 0 for every key of the tile)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float pv[8], v0[8], v1[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    pv[i] = s[tj][8 * t + i];
                    const float *vrow = &sKV[(32 * tj + 16 * t + 8 * (i >> 2) + 4 * h + (i & 3)) * PITCH + l31];
                    v0[i] = vrow[0]; v1[i] = vrow[32];
                }
                h16x8 ph, pl, vh, vl;
                split8(pv, ph, pl);
                split8(v0, vh, vl);
                o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o0, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, c0, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, c0, 0, 0, 0);
                split8(v1, vh, vl);
                o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o1, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, c1, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, c1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) { o0[e] += c0[e] * 0.00048828125f; o1[e] += c1[e] * 0.00048828125f; }
    } else {
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
            if (!(wave_on && 32 * tj < n)) continue;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float *vrow = &sKV[(32 * tj + (m & 3) + 8 * (m >> 2) + 4 * h) * PITCH + l31];
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], s[tj][m], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32], s[tj][m], o1, 0, 0, 0);
            }
        }
    }
    __syncthreads();
    {
        const float inv = 1.0f / lsum;
        float *dst = &sKV[qi * PITCH];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * h;
            *reinterpret_cast<float4 *>(dst + c0) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4 *>(dst + 32 + c0) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + i * 64 * TJ;
        const int r = SPLIT == 3 ? id % (32 * TJ) : id >> 3, c8 = SPLIT == 3 ? id / (32 * TJ) : id & 7;
        if (r < L) {
            float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;   // rows beyond the sequence: zeros in every form
            if (r < n) {
                v0 = *reinterpret_cast<const float4 *>(&sKV[r * PITCH + 8 * c8]);
                v1 = *reinterpret_cast<const float4 *>(&sKV[r * PITCH + 8 * c8 + 4]);
            }
            store_row8<SPLIT>(out, b * L + r, H, head, c8, v0, v1);
        }
    }
}


// ---- fp32 arithmetic, 64 < seq_len <= 288: k_attention_hd64<SPLIT, false> with keys [0, n) -----------------------------------
template <int SPLIT>
__global__ __launch_bounds__(576) void k_attnvl_f32(const float *__restrict__ qkv, int L, int H, const int *__restrict__ lengths,
                                                    float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int TJ = (L + 31) >> 5;                 // key tiles the buffers are laid out for (= waves)
    float *sK = smem;                             // [32*TJ][PITCH]
    float *sV = smem + (size_t)32 * TJ * PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int64_t b = blockIdx.x / H;
    const int head = blockIdx.x % H;
    const int n = seq_keys(lengths, b, L);
    const int tj_n = (n + 31) >> 5;               // key tiles that hold a key of the sequence (>= 1)
    const bool wave_on = 32 * wave < n;
    const int64_t tok_stride = (int64_t)3 * H * HD;
    const float *base = qkv + b * L * tok_stride + head * HD;

    float4 kreg[8], vreg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * blockDim.x, r = id >> 4, c = id & 15;
        kreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) kreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c + H * HD);
    }
    const int qi = 32 * wave + l31;
    const int qrow = qi < n ? qi : n - 1;         // (a query beyond the sequence computes on a row inside it and stores zeros)
    float q[32];
    {
        const float *src = base + (int64_t)qrow * tok_stride + 32 * h;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 t = *reinterpret_cast<const float4 *>(src + 4 * u);
            q[4 * u] = t.x; q[4 * u + 1] = t.y; q[4 * u + 2] = t.z; q[4 * u + 3] = t.w;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * blockDim.x, r = id >> 4, c = id & 15;
        vreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) vreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c + 2 * H * HD);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + i * blockDim.x, r = id >> 4, c = id & 15;
        *reinterpret_cast<float4 *>(&sK[r * PITCH + 4 * c]) = kreg[i];
    }
    __syncthreads();

    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    const float c_exp = 0.125f * 1.44269504088896340736f;   // 1/sqrt(64) * log2(e)

    for (int tj = 0; tj < tj_n; ++tj) {           // (workgroup-uniform bound: every wave reaches the barrier of tile 0)
        f32x16 s;
        float alpha = 1.0f;
        if (wave_on) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            const float *krow = &sK[(32 * tj + l31) * PITCH + 32 * h];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 k4 = *reinterpret_cast<const float4 *>(krow + 4 * u);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, q[4 * u], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, q[4 * u + 1], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, q[4 * u + 2], s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, q[4 * u + 3], s, 0, 0, 0);
            }
            float mt = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = 32 * tj + (e & 3) + 8 * (e >> 2) + 4 * h;
                s[e] = j < n ? s[e] : -INFINITY;
                mt = fmaxf(mt, s[e]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            alpha = exp2f((m_run - m_new) * c_exp);
            float lt = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = exp2f((s[e] - m_new) * c_exp + 0.0f);
                lt += s[e];
            }
            lt += __shfl_xor(lt, 32);
            l_run = l_run * alpha + lt;
            m_run = m_new;
        }
        if (tj == 0) {                                // every wave passes here exactly once (tj_n >= 1): V into LDS
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int id = tid + i * blockDim.x, r = id >> 4, c = id & 15;
                *reinterpret_cast<float4 *>(&sV[r * PITCH + 4 * c]) = vreg[i];
            }
            __syncthreads();
        }
        if (wave_on) {
#pragma unroll
            for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float *vrow = &sV[(32 * tj + (m & 3) + 8 * (m >> 2) + 4 * h) * PITCH + l31];
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], s[m], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32], s[m], o1, 0, 0, 0);
            }
        }
    }

    if (qi < L) {
        const float inv = qi < n ? 1.0f / l_run : 0.0f;
        const bool in = qi < n;
        float *dst = out + ((b * L + qi) * H + head) * HD;
        unsigned short *row6 = reinterpret_cast<unsigned short *>(out) + (b * L + qi) * lemon_split::split_segments(SPLIT == 3 ? 2 : SPLIT) * (int64_t)(H * HD);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * h;
            float4 v0 = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            float4 v1 = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
            if (!in) { v0 = make_float4(0.f, 0.f, 0.f, 0.f); v1 = v0; }   // rows beyond the sequence: zeros in every form
            if (SPLIT == 3) {
                unsigned short *ot = reinterpret_cast<unsigned short *>(out);
                const float vv[2][4] = {{v0.x, v0.y, v0.z, v0.w}, {v1.x, v1.y, v1.z, v1.w}};
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    lemon_split::us4 hi, lo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        unsigned short a_, b_, c_;
                        lemon_split::split2h<false>(vv[u][e], a_, b_, c_);
                        hi[e] = a_; lo[e] = c_;
                    }
                    const int64_t o = lemon_split::tiled_off(lemon_split::TILE_A_ROWS, b * L + qi, head * HD + 32 * u + c0, 0, H * HD);
                    *reinterpret_cast<lemon_split::us4 *>(ot + o) = hi;
                    *reinterpret_cast<lemon_split::us4 *>(ot + o + lemon_split::TILE_A_ROWS * 16) = lo;
                }
            } else if (SPLIT) {
                lemon_split::store_split4<(SPLIT == 1 || SPLIT == 2) ? SPLIT : 1, false>(row6, H * HD, (head * HD + c0) >> 2, v0);
                lemon_split::store_split4<(SPLIT == 1 || SPLIT == 2) ? SPLIT : 1, false>(row6, H * HD, (head * HD + 32 + c0) >> 2, v1);
            } else {
                *reinterpret_cast<float4 *>(dst + c0) = v0;
                *reinterpret_cast<float4 *>(dst + 32 + c0) = v1;
            }
        }
    }
}


// ---- split-fp16 arithmetic, 64 < seq_len <= 288: k_attention_hd64_f16 with keys [0, n) ---------------------------------------
// (also what lemon_attention_set_f16(2) runs here: the first general kernel with fp16 arithmetic gives the same bits)
template <int SPLIT>
__global__ __launch_bounds__(576, 4) void k_attnvl_f16(const float *__restrict__ qkv, int L, int H, const int *__restrict__ lengths,
                                                     float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    const int TJ = (L + 31) >> 5, Lp = 32 * TJ;
    const int TB = (TJ <= 5 || TJ > 8) ? TJ : (TJ + 1) >> 1; // key tiles per block: laid out by seq_len, as the sibling at this seq_len
    const int KB = 32 * TB;
    char *sKh = smem_c, *sKl = smem_c + KB * 128, *sVh = smem_c + 2 * KB * 128, *sVl = smem_c + 3 * KB * 128;
    float *sQ = reinterpret_cast<float *>(smem_c);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int64_t b = blockIdx.x / H;
    const int head = blockIdx.x % H;
    const int n = seq_keys(lengths, b, L);
    const int tj_n = (n + 31) >> 5;                          // key tiles that hold a key of the sequence (>= 1)
    const bool wave_on = 32 * wave < n;
    const int64_t tok_stride = (int64_t)3 * H * HD;
    const float *base = qkv + b * L * tok_stride + head * HD;
    const int nthr = 64 * TJ;                                // = blockDim.x
    auto stage_off = [](int r, int c) { return r * 64 + 4 * (c ^ (r & 15)); };
    const unsigned tok_bytes = (unsigned)(3 * H * HD * 4);
    constexpr int CH = 5;
    auto stage_block = [&](int kb) {
        for (int p0 = 0; p0 < KB * 16; p0 += CH * nthr) {
#pragma unroll
            for (int kv = 0; kv < 2; ++kv) {
                float4 reg[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = kb * KB + (id >> 4), c = id & 15;
                    reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (id < KB * 16 && r < n)
                        reg[i] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(base + (kv + 1) * H * HD) + ((unsigned)r * tok_bytes + 16u * (unsigned)c));
                }
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int id = p0 + tid + i * nthr, r = id >> 4, c = id & 15;
                    if (id < KB * 16) {
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
    {
        float4 qreg[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int id = tid + i * nthr, r = id >> 4, c = id & 15;
            qreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < n) qreg[i] = *reinterpret_cast<const float4 *>(base + (int64_t)r * tok_stride + 4 * c);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int id = tid + i * nthr, r = id >> 4, c = id & 15;
            *reinterpret_cast<float4 *>(&sQ[stage_off(r, c)]) = qreg[i];
        }
    }
    __syncthreads();
    const int qi = 32 * wave + l31;
    h16x8 qh[4], ql[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float4 a = *reinterpret_cast<const float4 *>(&sQ[stage_off(qi, 8 * h + 2 * u)]);
        const float4 c4 = *reinterpret_cast<const float4 *>(&sQ[stage_off(qi, 8 * h + 2 * u + 1)]);
        const float qv[8] = {a.x, a.y, a.z, a.w, c4.x, c4.y, c4.z, c4.w};
        split8u(qv, qh[u], ql[u]);
    }
    __syncthreads();
    stage_block(0);
    __syncthreads();

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
    for (int kb = 0; kb * TB < tj_n; ++kb) {                  // (workgroup-uniform: a key block entirely beyond n is not staged)
        if (kb > 0) {
            __syncthreads();
            stage_block(kb);
            __syncthreads();
        }
        const int t_end = (kb + 1) * TB < tj_n ? (kb + 1) * TB : tj_n;
        const int t_hi = wave_on ? t_end : kb * TB;           // a wave beyond the sequence stages and waits, nothing else
        for (int tj = kb * TB; tj < t_hi; ++tj) {
            const int tl = tj - kb * TB;
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
            if (32 * tj + 32 > n) {                           // the sequence's last tile (wave-uniform branch)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int j = 32 * tj + (e & 3) + 8 * (e >> 2) + 4 * h;
                    s[e] = j < n ? s[e] : -INFINITY;
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
                s[e] = __builtin_amdgcn_exp2f((s[e] - m_new) * c_exp + 10.0f);
                lt += s[e];
            }
            lt += __shfl_xor(lt, 32);
            l_run = l_run * alpha + lt;
            m_run = m_new;
            if (!__all(alpha == 1.0f)) {
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
    float *sO = sQ;
    __syncthreads();
    {
        const float inv = 1.0f / l_run;                       // (a wave beyond the sequence: its rows are not read back below)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * h;
            *reinterpret_cast<float4 *>(&sO[stage_off(qi, c0 >> 2)]) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
            *reinterpret_cast<float4 *>(&sO[stage_off(qi, 8 + (c0 >> 2))]) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + i * nthr;
        const int r = SPLIT == 3 ? id % Lp : id >> 3, c8 = SPLIT == 3 ? id / Lp : id & 7;
        if (r < L) {
            float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;   // rows beyond the sequence: zeros in every form
            if (r < n) {
                v0 = *reinterpret_cast<const float4 *>(&sO[stage_off(r, 2 * c8)]);
                v1 = *reinterpret_cast<const float4 *>(&sO[stage_off(r, 2 * c8 + 1)]);
            }
            store_row8<SPLIT>(out, b * L + r, H, head, c8, v0, v1);
        }
    }
}

template <int SPLIT>
int attention_varlen_impl(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim, const int32_t *lengths_dev,
                          float *out_dev, void *stream) {
    LEMON_REQUIRE(batch >= 0 && seq_len > 0 && heads > 0, "batch >= 0, seq_len > 0, heads > 0");
    LEMON_REQUIRE(head_dim == HD, "per-sequence lengths: head_dim must be 64 (in every lemon_attention_set_head_dims mode)");
    LEMON_REQUIRE(seq_len <= 288, "per-sequence lengths: seq_len <= 288 (the streaming kernels take no lengths)");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(qkv_dev && out_dev, "null pointer");
    LEMON_REQUIRE((((uintptr_t)qkv_dev) & 15) == 0 && (((uintptr_t)out_dev) & 15) == 0, "16-byte alignment");
    LEMON_REQUIRE((((uintptr_t)lengths_dev) & 3) == 0, "lengths: 4-byte alignment");
    LEMON_REQUIRE(batch * heads < (int64_t)1 << 31, "batch * heads < 2^31");
    LEMON_REQUIRE((int64_t)288 * 3 * heads * HD * 4 < (int64_t)1 << 32, "heads < 19 418 (32-bit offsets inside a head's slice)");
    const int tj = (seq_len + 31) / 32;
    const bool f16 = lemon_attention_f16_mode() != 0;
    const dim3 grid((unsigned)(batch * heads));
    hipStream_t st = (hipStream_t)stream;
    if (tj <= 2) {
        if (f16) {
            if (tj == 1) hipLaunchKernelGGL((k_attnvl_short<1, SPLIT, true>), grid, dim3(64), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
            else         hipLaunchKernelGGL((k_attnvl_short<2, SPLIT, true>), grid, dim3(128), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
        } else {
            if (tj == 1) hipLaunchKernelGGL((k_attnvl_short<1, SPLIT, false>), grid, dim3(64), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
            else         hipLaunchKernelGGL((k_attnvl_short<2, SPLIT, false>), grid, dim3(128), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
        }
        LEMON_HIP_CHECK(hipGetLastError());
        return LEMON_OK;
    }
    const int tb = (tj <= 5 || tj > 8) ? tj : (tj + 1) / 2;
    const size_t lds = f16 ? std::max((size_t)4 * 32 * tb * 128, (size_t)32 * tj * 256) : (size_t)2 * 32 * tj * PITCH * sizeof(float);
    {   // the attribute is per DEVICE (and per instantiation): one flag per device index, under a lock
        static std::mutex mu;
        static bool attr_set[64] = {};
        int dev = 0;
        LEMON_HIP_CHECK(hipGetDevice(&dev));
        LEMON_REQUIRE(dev >= 0 && dev < 64, "device index");
        std::lock_guard<std::mutex> lock(mu);
        if (!attr_set[dev]) {
            LEMON_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_attnvl_f32<SPLIT>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            LEMON_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_attnvl_f16<SPLIT>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            attr_set[dev] = true;
        }
    }
    if (f16) hipLaunchKernelGGL((k_attnvl_f16<SPLIT>), grid, dim3(64 * tj), lds, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
    else hipLaunchKernelGGL((k_attnvl_f32<SPLIT>), grid, dim3(64 * tj), lds, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

}  // namespace

// lengths_dev == NULL: the plain entry point, bidirectional (identical bits; it applies its own argument checks)
extern "C" int lemon_attention_f32_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                          const int32_t *lengths_dev, float *out_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f32(qkv_dev, batch, seq_len, heads, head_dim, 0, out_dev, stream);
    return attention_varlen_impl<0>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, out_dev, stream);
}

extern "C" int lemon_attention_split3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                             const int32_t *lengths_dev, uint16_t *out6_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_split3(qkv_dev, batch, seq_len, heads, head_dim, 0, out6_dev, stream);
    return attention_varlen_impl<1>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(out6_dev), stream);
}

extern "C" int lemon_attention_f16x3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                            const int32_t *lengths_dev, uint16_t *out3_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f16x3(qkv_dev, batch, seq_len, heads, head_dim, 0, out3_dev, stream);
    return attention_varlen_impl<2>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(out3_dev), stream);
}

extern "C" int lemon_attention_f16x3t_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                             const int32_t *lengths_dev, uint16_t *outt_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f16x3t(qkv_dev, batch, seq_len, heads, head_dim, 0, outt_dev, stream);
    return attention_varlen_impl<3>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(outt_dev), stream);
}
