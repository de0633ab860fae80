// chain_dist.hpp -- the chain contract's pair distance on gathered rows: ONE fmaf chain over ascending columns.
// Shared by the kernels that gather rows by neighbour id (api.hip: k_neighbors_finalize, k_discrepancy;
// discrepancy_ks.hip: k_discrepancy_ks), so that the arithmetic exists once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <bool L2>
__device__ __forceinline__ float chain_dist(const float *__restrict__ a, const float *__restrict__ b, int d) {
    float acc = 0.0f;
    if ((d & 3) == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0) {
        const float4 *a4 = reinterpret_cast<const float4 *>(a);
        const float4 *b4 = reinterpret_cast<const float4 *>(b);
        for (int c = 0; c < d / 4; ++c) {
            const float4 u = a4[c], v = b4[c];
            if (L2) {
                float t;
                t = u.x - v.x; acc = __builtin_fmaf(t, t, acc);
                t = u.y - v.y; acc = __builtin_fmaf(t, t, acc);
                t = u.z - v.z; acc = __builtin_fmaf(t, t, acc);
                t = u.w - v.w; acc = __builtin_fmaf(t, t, acc);
            } else {
                acc = __builtin_fmaf(u.x, v.x, acc);
                acc = __builtin_fmaf(u.y, v.y, acc);
                acc = __builtin_fmaf(u.z, v.z, acc);
                acc = __builtin_fmaf(u.w, v.w, acc);
            }
        }
    } else {
        for (int c = 0; c < d; ++c) {
            if (L2) { float t = a[c] - b[c]; acc = __builtin_fmaf(t, t, acc); }
            else acc = __builtin_fmaf(a[c], b[c], acc);
        }
    }
    return L2 ? acc : 1.0f - acc;
}

// Wave-cooperative chained distance.  Lane l owns the row pair (a_l, b_l) and must walk it in ascending
// k with ONE fmaf chain (the numeric contract), but 64 lanes reading 64 different rows 16 B at a time
// touch 64 cache lines per instruction and thrash the 32 KB L1.  So rows are fetched 128 B (one line) at
// a time with full-line loads -- lane (r8, c) fetches chunk c of rows r8, r8+8, ... of the wave -- and
// transposed through LDS (row pitch 36 floats: conflict-free 128-bit reads); the next 128 B are in
// flight while the current ones are consumed.  Needs d % 4 == 0 and 16-byte aligned rows.
constexpr int NB_PITCH = 36;
template <bool L2>
__device__ __forceinline__ float chain_dist_wave(const float *a_row, const float *b_row, int d,
                                                 float *__restrict__ lds /* [2][64][NB_PITCH] */, int lane) {
    const int r8 = lane >> 3, c = lane & 7;
    // named registers, not arrays (hipcc keeps arrays that are filled under a condition in scratch)
#define NB_PTR(i) \
    const float *pa##i = reinterpret_cast<const float *>(__shfl((unsigned long long)(uintptr_t)a_row, r8 + 8 * i)) + 4 * c; \
    const float *pb##i = reinterpret_cast<const float *>(__shfl((unsigned long long)(uintptr_t)b_row, r8 + 8 * i)) + 4 * c;
    NB_PTR(0) NB_PTR(1) NB_PTR(2) NB_PTR(3) NB_PTR(4) NB_PTR(5) NB_PTR(6) NB_PTR(7)
#undef NB_PTR
    float4 va0, va1, va2, va3, va4, va5, va6, va7, vb0, vb1, vb2, vb3, vb4, vb5, vb6, vb7;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#define NB_LOAD(i, koff) \
    va##i = *reinterpret_cast<const float4 *>(pa##i + (koff)); vb##i = *reinterpret_cast<const float4 *>(pb##i + (koff));
#define NB_ZERO(i) va##i = zero; vb##i = zero;
#define NB_FETCH(koff)                                                                              \
    do {                                                                                            \
        if ((koff) + 4 * c < d) {                                                                   \
            NB_LOAD(0, koff) NB_LOAD(1, koff) NB_LOAD(2, koff) NB_LOAD(3, koff)                     \
            NB_LOAD(4, koff) NB_LOAD(5, koff) NB_LOAD(6, koff) NB_LOAD(7, koff)                     \
        } else {                                                                                    \
            NB_ZERO(0) NB_ZERO(1) NB_ZERO(2) NB_ZERO(3) NB_ZERO(4) NB_ZERO(5) NB_ZERO(6) NB_ZERO(7) \
        }                                                                                           \
    } while (0)
#define NB_STORE(i)                                                                    \
    *reinterpret_cast<float4 *>(&la[(r8 + 8 * i) * NB_PITCH + 4 * c]) = va##i;         \
    *reinterpret_cast<float4 *>(&lb[(r8 + 8 * i) * NB_PITCH + 4 * c]) = vb##i;
    NB_FETCH(0);
    float acc = 0.0f;
    float *la = lds, *lb = lds + 64 * NB_PITCH;
    for (int k0 = 0; k0 < d; k0 += 32) {
        NB_STORE(0) NB_STORE(1) NB_STORE(2) NB_STORE(3) NB_STORE(4) NB_STORE(5) NB_STORE(6) NB_STORE(7)
        const int kn = k0 + 32;
        if (kn < d) NB_FETCH(kn);                        // wave-uniform: next 128 B of every row
        __builtin_amdgcn_wave_barrier();
        const int lim = d - k0 < 32 ? d - k0 : 32;       // wave-uniform; multiple of 4
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (4 * u < lim) {
                const float4 x = *reinterpret_cast<const float4 *>(&la[lane * NB_PITCH + 4 * u]);
                const float4 y = *reinterpret_cast<const float4 *>(&lb[lane * NB_PITCH + 4 * u]);
                if (L2) {
                    float t;
                    t = x.x - y.x; acc = __builtin_fmaf(t, t, acc);
                    t = x.y - y.y; acc = __builtin_fmaf(t, t, acc);
                    t = x.z - y.z; acc = __builtin_fmaf(t, t, acc);
                    t = x.w - y.w; acc = __builtin_fmaf(t, t, acc);
                } else {
                    acc = __builtin_fmaf(x.x, y.x, acc);
                    acc = __builtin_fmaf(x.y, y.y, acc);
                    acc = __builtin_fmaf(x.z, y.z, acc);
                    acc = __builtin_fmaf(x.w, y.w, acc);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#undef NB_STORE
#undef NB_FETCH
#undef NB_ZERO
#undef NB_LOAD
    return L2 ? acc : 1.0f - acc;
}
