// kmeans.hip -- Lloyd's k-means on the device and the deep-kNN label score (gfx950).
//
// Stands in for lib/datasets/clustering.py:13-75 (FaissKMeans: faiss.Kmeans(d, k, niter=300, nredo=5, seed=42).train(x),
// predict = index.search(x, 1)) as used by get_dataset(..., cluster_text=True) (lib/datasets/utils.py:312-316,396-400), and
// for the neighbour-label vote of lib/baselines/run_deepknn.py.
//
//   assign   nearest centroid of every point, bit for bit IndexFlatL2(d).add(c).search(x, 1) of this library: the products
//            run on v_mfma_f32_32x32x2_f32 in ascending k (the chain of the numeric contract), the norms are the same chain
//            (what lemon_rowdot_chain computes), the key is max(0, fma(-2, <x,c>, |x|^2 + |c|^2)), ties go to the lower index.
//            A workgroup owns a panel of 128 points and streams the centroid matrix through LDS in 128-row tiles; the
//            reduction is a running arg-min in registers (no candidate lists, no merge pass, no workspace).
//   update   new centroid = float64 mean of its points in ASCENDING POINT ORDER: the point ids are bucketed by cluster with
//            hipcub's stable radix sort, then one thread per (cluster, coordinate) walks its bucket.  No floating-point
//            atomics; the result depends on the input only, not on launch geometry or timing.
//   split    empty clusters, in ascending index, take half of the currently largest cluster (ties: lower index): the
//            donor's centroid is copied and the pair is perturbed symmetrically by eps = 1/1024.  This is faiss's
//            split_clusters rule EXCEPT that faiss draws the donor at random in proportion to its size; faiss cannot be
//            imported where this project is built and the reference holds no vectors of it, so its RNG stream and tie order
//            stay unpinned here exactly as for the flat index.
//   train    niter x (assign, update, split) and a last assign, enqueued without any host synchronisation; a device flag
//            turns the iterations behind the fixed point into no-ops.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "knn_common.hpp"

namespace {

using lemon_knn::swz;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KM_P = 128;    // points per workgroup
constexpr int KM_C = 128;    // centroids per LDS tile
constexpr int KM_K = 32;     // k-slice per LDS stage
constexpr int KM_NT = 256;   // 4 wavefronts; wave w owns points 32w .. 32w+31 against all 128 centroids of the tile
constexpr int KM_MAX_C = 16384;
constexpr int KM_MAX_D = 1024;

// one staged item: 8 consecutive k of one row (two 16-B loads), zero beyond the matrix
struct Item { float4 lo, hi; };

__device__ __forceinline__ Item km_load(const float *__restrict__ m, int64_t row, int64_t rows, int d, int k) {
    Item it;
    it.lo = make_float4(0.f, 0.f, 0.f, 0.f);
    it.hi = it.lo;
    if (row < rows) {
        const float *r = m + row * (int64_t)d;
        if (k < d) it.lo = *reinterpret_cast<const float4 *>(r + k);
        if (k + 4 < d) it.hi = *reinterpret_cast<const float4 *>(r + k + 4);
    }
    return it;
}

// LDS layout of the scan (knn_common.hpp swz): every group of 8 k is stored [k0 k2 k4 k6 | k1 k3 k5 k7] so that one 16-B read
// feeds four MFMA steps in ascending k (lanes 0-31 supply the even k of a pair, lanes 32-63 the odd one)
__device__ __forceinline__ void km_store(float *__restrict__ t, int r, int g, const Item &it) {
    *reinterpret_cast<float4 *>(&t[swz(r, 2 * g)]) = make_float4(it.lo.x, it.lo.z, it.hi.x, it.hi.z);
    *reinterpret_cast<float4 *>(&t[swz(r, 2 * g + 1)]) = make_float4(it.lo.y, it.lo.w, it.hi.y, it.hi.w);
}

__global__ __launch_bounds__(KM_NT, 2) void k_kmeans_assign(const float *__restrict__ x, int64_t n, int d,
                                                            const float *__restrict__ c, int C, int *__restrict__ assign,
                                                            float *__restrict__ dist, const int *__restrict__ done) {
    if (done && *done) return;               // train loop at its fixed point (lemon_kmeans_train): nothing can change any more
    __shared__ __attribute__((aligned(16))) float s_tile[2][2][KM_P * KM_K];   // [buf][points | centroids] 64 KiB
    __shared__ float s_xn[KM_P];
    __shared__ float s_cn[2][KM_C];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int64_t p0 = (int64_t)blockIdx.x * KM_P;
    const int KT = (d + KM_K - 1) / KM_K;
    const int n_ct = (C + KM_C - 1) / KM_C;
    const int total = n_ct * KT;

    // staging: item id = tid + 256 i -> row id >> 2, 8-group id & 3
    const int r0 = tid >> 2, r1 = (tid + KM_NT) >> 2, g = tid & 3;
    Item px0, px1, pc0, pc1;
#define KM_ISSUE(S)                                                                                   \
    do {                                                                                              \
        const int ct_ = (S) / KT, k_ = ((S) - ct_ * KT) * KM_K + 8 * g;                               \
        px0 = km_load(x, p0 + r0, n, d, k_); px1 = km_load(x, p0 + r1, n, d, k_);                     \
        pc0 = km_load(c, (int64_t)ct_ * KM_C + r0, C, d, k_); pc1 = km_load(c, (int64_t)ct_ * KM_C + r1, C, d, k_); \
    } while (0)
#define KM_COMMIT(BUF)                                                                                \
    do {                                                                                              \
        km_store(s_tile[BUF][0], r0, g, px0); km_store(s_tile[BUF][0], r1, g, px1);                   \
        km_store(s_tile[BUF][1], r0, g, pc0); km_store(s_tile[BUF][1], r1, g, pc1);                   \
    } while (0)

    f32x16 acc0, acc1, acc2, acc3;
    float nacc = 0.0f;                       // chain norm of row (tid & 127) of operand (tid >> 7)
    const int nrow = tid & 127, nop = tid >> 7;   // waves 0,1: points; waves 2,3: centroids (wave-uniform)
    float best_d = INFINITY;
    int best_i = -1;
    const int prow = 32 * wave + l31;

    KM_ISSUE(0);
    KM_COMMIT(0);
    __syncthreads();
    for (int s = 0; s < total; ++s) {
        const int buf = s & 1;
        const int ct = s / KT, ks = s - ct * KT;
        if (ks == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc0[e] = 0.0f; acc1[e] = 0.0f; acc2[e] = 0.0f; acc3[e] = 0.0f; }
            if (nop == 1) nacc = 0.0f;
        }
        if (s + 1 < total) KM_ISSUE(s + 1);
        const float *tq = s_tile[buf][0], *tx = s_tile[buf][1];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(&tq[swz(prow, 2 * u + h)]);
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(&tx[swz(l31, 2 * u + h)]);
            const f32x4 a1 = *reinterpret_cast<const f32x4 *>(&tx[swz(32 + l31, 2 * u + h)]);
            const f32x4 a2 = *reinterpret_cast<const f32x4 *>(&tx[swz(64 + l31, 2 * u + h)]);
            const f32x4 a3 = *reinterpret_cast<const f32x4 *>(&tx[swz(96 + l31, 2 * u + h)]);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m], b[m], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m], b[m], acc1, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[m], b[m], acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a3[m], b[m], acc3, 0, 0, 0);
            }
        }
        // the norms ride along: one thread per row walks the slice in ascending k (points on the first centroid tile only)
        if (nop == 1 || ct == 0) {
            const float *tn = s_tile[buf][nop];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 ev = *reinterpret_cast<const f32x4 *>(&tn[swz(nrow, 2 * u)]);
                const f32x4 od = *reinterpret_cast<const f32x4 *>(&tn[swz(nrow, 2 * u + 1)]);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    nacc = __builtin_fmaf(ev[m], ev[m], nacc);
                    nacc = __builtin_fmaf(od[m], od[m], nacc);
                }
            }
        }
        if (ks == KT - 1) {
            if (nop == 1) s_cn[ct & 1][nrow] = nacc;
            else if (ct == 0) s_xn[nrow] = nacc;
        }
        if (s + 1 < total) KM_COMMIT(buf ^ 1);
        __syncthreads();
        if (ks == KT - 1) {
            // ---- tile epilogue: exact L2 key, running arg-min (rows arrive in ascending index: strict '<' keeps the lower) ----
            const float xn = s_xn[prow];
            const float *cn = s_cn[ct & 1];
            const int cb = ct * KM_C + 4 * h;
#define KM_MIN(ACC, OFF)                                                                              \
            _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                          \
                const int lr = (OFF) + (e & 3) + 8 * (e >> 2);                                        \
                const int j = cb + lr;                                                                \
                const float dd = __builtin_fmaf(-2.0f, ACC[e], xn + cn[lr + 4 * h]);                  \
                const float dv = dd > 0.0f ? dd : 0.0f;                                               \
                if (j < C && dv < best_d) { best_d = dv; best_i = j; }                                \
            }
            KM_MIN(acc0, 0) KM_MIN(acc1, 32) KM_MIN(acc2, 64) KM_MIN(acc3, 96)
#undef KM_MIN
        }
    }
#undef KM_ISSUE
#undef KM_COMMIT
    // the two lanes of a point (l, l + 32) hold interleaved centroid rows: merge them
    const float od = __shfl_xor(best_d, 32);
    const int oi = __shfl_xor(best_i, 32);
    if (od < best_d || (od == best_d && (unsigned)oi < (unsigned)best_i)) { best_d = od; best_i = oi; }
    const int64_t p = p0 + prow;
    if (h == 0 && p < n) {
        assign[p] = best_i;
        if (dist) dist[p] = best_i >= 0 ? best_d : FLT_MAX;
    }
}

// ---- update ---------------------------------------------------------------------------------------------------------
// (train loop: also notes in flags[KM_CHANGED] whether any assignment differs from the previous iteration's, kept in prev)
constexpr int KM_CHANGED = 0, KM_DONE = 1;
__global__ void k_km_keys(const int *__restrict__ assign, int64_t n, int C, u32 *__restrict__ keys, u32 *__restrict__ ids,
                          int *__restrict__ prev, int *__restrict__ flags, int first) {
    if (flags && flags[KM_DONE]) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int a = assign[i];
    if (prev) {
        if (first || prev[i] != a) flags[KM_CHANGED] = 1;      // every writer stores the same value
        prev[i] = a;
    }
    keys[i] = (a >= 0 && a < C) ? (u32)a : (u32)C;     // bucket C: points without a cluster (never averaged)
    ids[i] = (u32)i;
}

// start[c] = first sorted position whose key is >= c, for c = 0 .. C
__global__ void k_km_bounds(const u32 *__restrict__ keys_s, int64_t n, int C, int *__restrict__ start, const int *__restrict__ done) {
    if (done && *done) return;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > C) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys_s[mid] < (u32)c) lo = mid + 1; else hi = mid;
    }
    start[c] = (int)lo;
}

// one thread per (cluster, coordinate): float64 sum over the cluster's points in ascending point id, one rounding to float32
__global__ __launch_bounds__(128) void k_km_means(const float *__restrict__ x, int d, const u32 *__restrict__ ids_s,
                                                  const int *__restrict__ start, float *__restrict__ c,
                                                  int64_t *__restrict__ count, const int *__restrict__ done) {
    if (done && *done) return;
    const int cl = blockIdx.x;
    const int j = blockIdx.y * 128 + threadIdx.x;
    const int s = start[cl], e = start[cl + 1];
    if (j == 0) count[cl] = (int64_t)(e - s);
    if (j >= d || e == s) return;                      // an empty cluster keeps its centroid
    double sum = 0.0;
    int p = s;
    for (; p + 4 <= e; p += 4) {
        const u32 i0 = ids_s[p], i1 = ids_s[p + 1], i2 = ids_s[p + 2], i3 = ids_s[p + 3];
        const float v0 = x[(int64_t)i0 * d + j], v1 = x[(int64_t)i1 * d + j], v2 = x[(int64_t)i2 * d + j],
                    v3 = x[(int64_t)i3 * d + j];
        sum += (double)v0; sum += (double)v1; sum += (double)v2; sum += (double)v3;
    }
    for (; p < e; ++p) sum += (double)x[(int64_t)ids_s[p] * d + j];
    c[(int64_t)cl * d + j] = (float)(sum / (double)(e - s));
}

// obj = sum of dist in float64: ONE block of 1024 threads whatever n is (thread t sums elements t, t + 1024, ... in ascending
// order, then a fixed tree), so the order of additions is a function of n alone
// (train loop at its fixed point: the objective of the previous iteration is carried forward instead)
__global__ __launch_bounds__(1024) void k_km_obj(const float *__restrict__ dist, int64_t n, double *__restrict__ obj,
                                                 const int *__restrict__ done) {
    __shared__ double s[1024];
    if (done && *done) {
        if (threadIdx.x == 0) obj[0] = obj[-1];          // done is only ever set after an iteration: obj[-1] exists
        return;
    }
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) a += (double)dist[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) obj[0] = s[0];
}

// ---- split ----------------------------------------------------------------------------------------------------------
// one block; dynamic LDS: int cnt[C], then u64 red[16]
// flags (train loop only): the last kernel of an iteration decides whether the loop has reached its fixed point -- no
// assignment changed and no cluster is empty.  Then mean(a_t) = mean(a_t-1) bit for bit (the update is a function of its
// input alone), an empty cluster at t-1 would still be empty at t, so the centroids, hence every later assignment, repeat:
// the remaining iterations cannot change the result and their kernels return at once.
__global__ __launch_bounds__(1024) void k_km_split(float *__restrict__ c, int d, int C, int64_t *__restrict__ count,
                                                   int *__restrict__ flags) {
    if (flags && flags[KM_DONE]) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    int *s_cnt = reinterpret_cast<int *>(s_raw);
    u64 *s_red = reinterpret_cast<u64 *>(s_raw + (((size_t)C * 4 + 15) & ~(size_t)15));
    __shared__ int s_empty;
    const int tid = threadIdx.x;
    if (tid == 0) s_empty = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < C; i += 1024) { const int v = (int)count[i]; s_cnt[i] = v; mine += (v == 0); }
    if (mine) atomicAdd(&s_empty, mine);
    __syncthreads();
    if (flags && tid == 0) {
        if (flags[KM_CHANGED] == 0 && s_empty == 0) flags[KM_DONE] = 1;
        flags[KM_CHANGED] = 0;
    }
    if (s_empty == 0) return;
    const float up = 1.0f + 1.0f / 1024.0f, dn = 1.0f - 1.0f / 1024.0f;
    for (int e = 0; e < C; ++e) {
        if (s_cnt[e] != 0) continue;                    // block-uniform
        u64 best = 0;
        for (int i = tid; i < C; i += 1024) {
            const u64 key = ((u64)(u32)s_cnt[i] << 32) | (u64)(0xffffffffu - (u32)i);
            best = key > best ? key : best;
        }
        for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(best, off); best = o > best ? o : best; }
        if ((tid & 63) == 0) s_red[tid >> 6] = best;
        __syncthreads();
        best = 0;
        for (int w = 0; w < 16; ++w) best = s_red[w] > best ? s_red[w] : best;
        const int dc = (int)(best >> 32);
        const int donor = (int)(0xffffffffu - (u32)(best & 0xffffffffull));
        const int half = dc / 2;
        if (half == 0) break;                           // block-uniform: nothing left to split
        for (int j = tid; j < d; j += 1024) {
            const float v = c[(int64_t)donor * d + j];
            const bool even = (j & 1) == 0;
            c[(int64_t)e * d + j] = v * (even ? up : dn);
            c[(int64_t)donor * d + j] = v * (even ? dn : up);
        }
        __syncthreads();                                // every read of s_red / s_cnt above precedes the update
        if (tid == 0) { s_cnt[e] = half; s_cnt[donor] = dc - half; }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < C; i += 1024) count[i] = (int64_t)s_cnt[i];
}

// ---- deep-kNN label disagreement ------------------------------------------------------------------------------------
__global__ void k_label_disagreement(const int64_t *__restrict__ I, int64_t nq, int kk, int k, int drop_self,
                                     const uint8_t *__restrict__ in_db, const int32_t *__restrict__ db_label, int64_t ntotal,
                                     const int32_t *__restrict__ q_label, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int first = (drop_self && (!in_db || in_db[i])) ? 1 : 0;   // run_lemon.py:257-263: drop result[0], else result[-1]
    const int32_t ql = q_label[i];
    int bad = 0;
    for (int s = 0; s < k; ++s) {
        const int64_t id = I[i * kk + first + s];
        bool same = false;
        if (id >= 0 && id < ntotal && ql >= 0) same = db_label[id] == ql;
        bad += !same;
    }
    out[i] = (float)bad / (float)k;
}

inline size_t km_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline int km_key_bits(int C) { int b = 1; while ((1 << b) <= C) ++b; return b; }   // values 0 .. C

struct KmWs {
    u32 *keys, *keys_s, *ids, *ids_s;
    int *start, *prev, *flags;
    float *dist;
    void *cub;
    size_t cub_bytes, total;
};

int km_carve(int64_t n, int C, void *ws, KmWs *w) {
    size_t t = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const u32 *)nullptr, (u32 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr,
                                           (int)n, 0, km_key_bits(C), (hipStream_t)0) != hipSuccess) {
        lemon_set_error("hipcub radix sort size query failed");
        return LEMON_E_HIP;
    }
    const size_t n4 = km_align((size_t)n * 4), cs = km_align((size_t)(C + 2) * 4);
    char *p = (char *)ws;
    w->keys = (u32 *)p; p += n4;
    w->keys_s = (u32 *)p; p += n4;
    w->ids = (u32 *)p; p += n4;
    w->ids_s = (u32 *)p; p += n4;
    w->dist = (float *)p; p += n4;
    w->prev = (int *)p; p += n4;
    w->flags = (int *)p; p += 256;
    w->start = (int *)p; p += cs;
    w->cub = p;
    w->cub_bytes = km_align(t);
    w->total = 6 * n4 + cs + w->cub_bytes + 512;
    return LEMON_OK;
}

int km_check_shape(int64_t n, int d, int C) {
    LEMON_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n must lie in [0, 2^31)");
    LEMON_REQUIRE(C >= 1 && C <= KM_MAX_C, "1 <= C <= 16384");
    LEMON_REQUIRE(d >= 4 && d <= KM_MAX_D && (d & 3) == 0, "d must be a multiple of 4 in [4, 1024]");
    return LEMON_OK;
}

// the three steps with the train loop's fixed-point state (flags / prev: nullptr outside the loop)
int km_assign(const float *x_dev, int64_t n, int d, const float *c_dev, int C, int32_t *assign_dev, float *dist_dev,
              const int *done, hipStream_t s) {
    int rc = km_check_shape(n, d, C);
    if (rc) return rc;
    LEMON_REQUIRE(c_dev && assign_dev && (x_dev || n == 0), "null pointer");
    LEMON_REQUIRE((((uintptr_t)x_dev | (uintptr_t)c_dev) & 15) == 0, "x_dev and c_dev must be 16-byte aligned");
    if (n == 0) return LEMON_OK;
    const unsigned grid = (unsigned)((n + KM_P - 1) / KM_P);
    hipLaunchKernelGGL(k_kmeans_assign, dim3(grid), dim3(KM_NT), 0, s, x_dev, n, d, c_dev, C, assign_dev, dist_dev, done);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

int km_update(const float *x_dev, int64_t n, int d, const int32_t *assign_dev, const float *dist_dev, int C, float *c_dev,
              int64_t *count_dev, double *obj_dev, void *ws_dev, int64_t ws_bytes, bool loop, bool first, hipStream_t s) {
    int rc = km_check_shape(n, d, C);
    if (rc) return rc;
    LEMON_REQUIRE(n >= 1, "n >= 1");
    LEMON_REQUIRE(x_dev && assign_dev && c_dev && count_dev && ws_dev, "null pointer");
    LEMON_REQUIRE(((uintptr_t)ws_dev & 255) == 0, "ws_dev must be 256-byte aligned");
    KmWs w;
    rc = km_carve(n, C, ws_dev, &w);
    if (rc) return rc;
    LEMON_REQUIRE((size_t)ws_bytes >= w.total, "workspace smaller than lemon_kmeans_workspace_bytes(n, d, C)");
    int *flags = loop ? w.flags : nullptr;
    const int *done = loop ? w.flags + KM_DONE : nullptr;
    hipLaunchKernelGGL(k_km_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, assign_dev, n, C, w.keys, w.ids,
                       loop ? w.prev : nullptr, flags, first ? 1 : 0);
    LEMON_HIP_CHECK(hipGetLastError());
    size_t tb = w.cub_bytes;      // (the sort cannot look at the flag: at the fixed point it re-sorts the last keys, which nothing reads)
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, tb, w.keys, w.keys_s, w.ids, w.ids_s, (int)n, 0, km_key_bits(C), s) != hipSuccess) {
        lemon_set_error("hipcub radix sort failed");
        return LEMON_E_HIP;
    }
    hipLaunchKernelGGL(k_km_bounds, dim3((unsigned)((C + 1 + 255) / 256)), dim3(256), 0, s, w.keys_s, n, C, w.start, done);
    LEMON_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_km_means, dim3((unsigned)C, (unsigned)((d + 127) / 128)), dim3(128), 0, s, x_dev, d, w.ids_s, w.start, c_dev,
                       count_dev, done);
    LEMON_HIP_CHECK(hipGetLastError());
    if (obj_dev) {
        LEMON_REQUIRE(dist_dev != nullptr, "obj_dev needs dist_dev");
        hipLaunchKernelGGL(k_km_obj, dim3(1), dim3(1024), 0, s, dist_dev, n, obj_dev, done);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    return LEMON_OK;
}

int km_split(float *c_dev, int d, int C, int64_t *count_dev, int *flags, hipStream_t s) {
    int rc = km_check_shape(1, d, C);
    if (rc) return rc;
    LEMON_REQUIRE(c_dev && count_dev, "null pointer");
    const size_t lds = (((size_t)C * 4 + 15) & ~(size_t)15) + 16 * sizeof(u64);
    if (lds > 48 * 1024)
        LEMON_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_km_split), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_km_split, dim3(1), dim3(1024), lds, s, c_dev, d, C, count_dev, flags);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

}  // namespace

extern "C" {

int lemon_kmeans_assign(const float *x_dev, int64_t n, int d, const float *c_dev, int C, int32_t *assign_dev, float *dist_dev,
                        void *stream) {
    return km_assign(x_dev, n, d, c_dev, C, assign_dev, dist_dev, nullptr, (hipStream_t)stream);
}

int64_t lemon_kmeans_workspace_bytes(int64_t n, int d, int C) {
    if (km_check_shape(n, d, C)) return LEMON_E_INVALID;
    KmWs w;
    const int rc = km_carve(n > 0 ? n : 1, C, nullptr, &w);
    return rc ? (int64_t)rc : (int64_t)w.total;
}

int lemon_kmeans_update(const float *x_dev, int64_t n, int d, const int32_t *assign_dev, const float *dist_dev, int C,
                        float *c_dev, int64_t *count_dev, double *obj_dev, void *ws_dev, int64_t ws_bytes, void *stream) {
    return km_update(x_dev, n, d, assign_dev, dist_dev, C, c_dev, count_dev, obj_dev, ws_dev, ws_bytes, false, false,
                     (hipStream_t)stream);
}

int lemon_kmeans_split(float *c_dev, int d, int C, int64_t *count_dev, void *stream) {
    return km_split(c_dev, d, C, count_dev, nullptr, (hipStream_t)stream);
}

int lemon_kmeans_train(const float *x_dev, int64_t n, int d, int C, int niter, float *c_dev, double *obj_hist_dev,
                       int64_t *count_dev, int32_t *assign_dev, void *ws_dev, int64_t ws_bytes, void *stream) {
    int rc = km_check_shape(n, d, C);
    if (rc) return rc;
    LEMON_REQUIRE(n >= C, "fewer points than clusters");
    LEMON_REQUIRE(niter >= 0, "niter >= 0");
    LEMON_REQUIRE(x_dev && c_dev && count_dev && assign_dev && ws_dev && (obj_hist_dev || niter == 0), "null pointer");
    LEMON_REQUIRE(((uintptr_t)ws_dev & 255) == 0, "ws_dev must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    KmWs w;
    rc = km_carve(n, C, ws_dev, &w);
    if (rc) return rc;
    LEMON_REQUIRE((size_t)ws_bytes >= w.total, "workspace smaller than lemon_kmeans_workspace_bytes(n, d, C)");
    // Early stop without the host: once an iteration changes no assignment and leaves no cluster empty the loop is at a fixed
    // point (k_km_split), a device flag is raised and the kernels of the remaining iterations return at once; the objective
    // is carried forward.  LEMON_KMEANS_EARLY_STOP=0 runs every iteration in full (same bits: tests).
    const char *env = getenv("LEMON_KMEANS_EARLY_STOP");
    const bool early = !(env && env[0] == '0');
    if (early) LEMON_HIP_CHECK(hipMemsetAsync(w.flags, 0, 256, s));
    const int *done = early ? w.flags + KM_DONE : nullptr;
    for (int it = 0; it < niter; ++it) {
        rc = km_assign(x_dev, n, d, c_dev, C, assign_dev, w.dist, done, s);
        if (rc) return rc;
        rc = km_update(x_dev, n, d, assign_dev, w.dist, C, c_dev, count_dev, obj_hist_dev + it, ws_dev, ws_bytes, early, it == 0, s);
        if (rc) return rc;
        rc = km_split(c_dev, d, C, count_dev, early ? w.flags : nullptr, s);
        if (rc) return rc;
    }
    return km_assign(x_dev, n, d, c_dev, C, assign_dev, nullptr, nullptr, s);
}

int lemon_knn_label_disagreement(const int64_t *I_dev, int64_t nq, int kk, int k, int drop_self, const uint8_t *in_db_dev,
                                 const int32_t *db_label_dev, int64_t ntotal, const int32_t *q_label_dev, float *out_dev,
                                 void *stream) {
    LEMON_REQUIRE(nq >= 0 && k >= 1 && ntotal >= 0, "nq >= 0, k >= 1, ntotal >= 0");
    LEMON_REQUIRE(kk >= k + (drop_self ? 1 : 0), "kk must hold k (+ 1 with drop_self) neighbours");
    LEMON_REQUIRE(I_dev && db_label_dev && q_label_dev && out_dev, "null pointer");
    if (nq == 0) return LEMON_OK;
    hipLaunchKernelGGL(k_label_disagreement, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, I_dev, nq, kk, k,
                       drop_self ? 1 : 0, in_db_dev, db_label_dev, ntotal, q_label_dev, out_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

}  // extern "C"
