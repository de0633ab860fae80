// discrepancy_ks.hip -- the discrepancy baselines for every method and a list of knn_k from one search
// (lib/baselines/discrepancy_baseline.py:164-242 on the grid of experiments.py:141-177).
// One wavefront per (query, method): the pair matrix at the largest k is computed once into LDS (each pair a chain distance on
// gathered rows, as in k_discrepancy), then every k of the list replays k_discrepancy's lane-strided float64 sum over its
// prefix of the matrix (discrepancy_core.hpp).  lemon_discrepancy (api.hip) is the definition the results equal bit for bit.
#include "common.hpp"
#include <math.h>
#include <vector>
#include "chain_dist.hpp"
#include "discrepancy_core.hpp"

#define DSC_MAX_KS (LEMON_MAX_K - 1)     // strictly ascending ks in 1 .. LEMON_MAX_K - 1

struct DiscKsParams {
    const float *E[2], *q[2];            // [0] image, [1] text: database rows [ntotal, d], query rows [nq, d]
    const int64_t *Im, *Ic;              // [nq, kqmax] text neighbours of the queries; [ntotal, kc] of the database rows
    float *out;                          // [4][n_ks][nq]
    int64_t nq;
    int d, kc, kmax, kqmax, n_ks, is_train;
    int mat[4];                          // blockIdx.y -> 0 dis_x, 1 dis_y, 2 div_x, 3 div_y
    int ks[DSC_MAX_KS];
};

// STAGED: wave-cooperative row fetches (d % 4 == 0, aligned rows); otherwise every lane walks its rows from global.
// Dynamic LDS: the pair matrix, kqmax * max(kmax + 1, kqmax) floats (at most 64 x 64 x 4 B = 16 KB).
template <bool STAGED>
__global__ __launch_bounds__(64) void k_discrepancy_ks(DiscKsParams p) {
    __shared__ __attribute__((aligned(16))) float s_rows[STAGED ? 2 * 64 * NB_PITCH : 4];
    __shared__ unsigned long long s_act[dsc::MAX_W];
    extern __shared__ float s_M[];
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int m = p.mat[blockIdx.y];
    const int method = m >> 1, mod = m & 1;
    const float *E = p.E[mod];
    const float *qrow = p.q[mod] + i * (int64_t)p.d;     // read by dis only
    const int64_t *im = p.Im + i * p.kqmax;
    const int W = dsc::width(method, p.kmax, p.kqmax);
    if (lane < p.kqmax) s_act[lane] = dsc::row_mask(method, im, p.Ic, p.kc, lane, W);
    const int pairs = p.kqmax * W;
    for (int tb = 0; tb < pairs; tb += 64) {
        const int t = tb + lane;
        bool active = t < pairs;
        const float *ra = E, *rb = E;                    // idle lanes read row 0 (always present: ntotal >= 1)
        if (active) {
            const int a = t / W, b = t - a * W;
            int64_t r0, r1;
            active = dsc::pair_rows(method, im, p.Ic, p.kc, a, b, &r0, &r1);
            if (active) { ra = E + r0 * (int64_t)p.d; rb = r1 < 0 ? qrow : E + r1 * (int64_t)p.d; }
        }
        const float dist = STAGED ? chain_dist_wave<false>(ra, rb, p.d, s_rows, lane)
                                  : (active ? chain_dist<false>(ra, rb, p.d) : 0.0f);
        if (t < pairs) s_M[t] = dist;
    }
    __syncthreads();
    for (int ti = 0; ti < p.n_ks; ++ti) {
        const int k = p.ks[ti], rows = k + p.is_train, cols = method == 0 ? k + 1 : rows;
        double total;
        int count;
        dsc::lane_sum(s_M, (const uint64_t *)s_act, W, rows, cols, lane, &total, &count);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { total += __shfl_xor(total, off); count += __shfl_xor(count, off); }
        if (lane == 0) p.out[((int64_t)m * p.n_ks + ti) * p.nq + i] = dsc::finish(method, total, count, k);
    }
}

extern "C" int lemon_discrepancy_cache(lemon_index_t *idx_txt, int kc, int64_t *Ic_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LEMON_REQUIRE(idx_txt && idx_txt->metric == LEMON_METRIC_IP, "text index must be an IndexFlatIP");
    LEMON_REQUIRE(kc >= 2 && kc <= LEMON_MAX_K, "2 <= kc <= LEMON_MAX_K");
    const int64_t n = idx_txt->n;
    if (n == 0) return LEMON_OK;
    LEMON_REQUIRE(Ic_dev, "null pointer");
    if (int rc = lemon_reserve_nb(idx_txt, n * kc, stream)) return rc;   // the distances the search returns beside the lists
    return lemon_search_internal(idx_txt, idx_txt->x, n, kc, idx_txt->at<float>(lemon_index::WS_D), Ic_dev, stream);   // discrepancy_baseline.py:166
}

static int check_ks(const int32_t *ks, int n_ks) {
    LEMON_REQUIRE(ks && n_ks >= 1 && n_ks <= DSC_MAX_KS, "ks: 1 .. LEMON_MAX_K - 1 values");
    LEMON_REQUIRE(ks[0] >= 1, "1 <= ks[0]");
    for (int t = 1; t < n_ks; ++t) LEMON_REQUIRE(ks[t] > ks[t - 1], "ks strictly ascending");
    LEMON_REQUIRE(ks[n_ks - 1] + 1 <= LEMON_MAX_K, "ks[n_ks - 1] + 1 <= LEMON_MAX_K");
    return LEMON_OK;
}

extern "C" int lemon_discrepancy_ks(lemon_index_t *idx_txt, const float *E_img_tr_dev, const float *E_txt_tr_dev,
                                    const float *q_img_dev, const float *q_txt_dev, int64_t nq, const int32_t *ks, int n_ks,
                                    int is_train, int methods, const int64_t *Ic_dev, int64_t cache_rows, int kc,
                                    float *out_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LEMON_REQUIRE(methods >= 1 && methods <= 15, "methods: bits 0 dis_x, 1 dis_y, 2 div_x, 3 div_y, at least one");
    LEMON_REQUIRE(idx_txt && idx_txt->metric == LEMON_METRIC_IP, "text index must be an IndexFlatIP");
    LEMON_REQUIRE(nq >= 0 && nq <= 0x7fffffff, "0 <= nq < 2^31");
    if (int rc = check_ks(ks, n_ks)) return rc;
    const int kmax = ks[n_ks - 1], kqmax = kmax + (is_train ? 1 : 0);
    const bool dis = (methods & 3) != 0, use_x = (methods & 5) != 0, use_y = (methods & 10) != 0;
    if (dis) {
        LEMON_REQUIRE(cache_rows == idx_txt->n, "the cache was built for another row count of the index (cache_rows == ntotal)");
        LEMON_REQUIRE(kc >= kmax + 1 && kc <= LEMON_MAX_K, "ks[n_ks - 1] + 1 <= kc <= LEMON_MAX_K");
    }
    if (nq == 0) return LEMON_OK;
    LEMON_REQUIRE(idx_txt->n >= 1, "empty index");
    LEMON_REQUIRE(q_txt_dev && out_dev && (!use_x || E_img_tr_dev) && (!use_y || E_txt_tr_dev) &&
                      (!(methods & 1) || q_img_dev) && (!dis || Ic_dev), "null pointer");
    const int d = idx_txt->d;
    LEMON_REQUIRE(rows_vector_safe(E_img_tr_dev, d) && rows_vector_safe(E_txt_tr_dev, d) && rows_vector_safe(q_img_dev, d) &&
                      rows_vector_safe(q_txt_dev, d),
                  "E_img_tr_dev, E_txt_tr_dev, q_img_dev and q_txt_dev must be 16-byte aligned when d % 4 == 0");
    if (int rc = lemon_reserve_nb(idx_txt, nq * kqmax, stream)) return rc;
    int64_t *Im = idx_txt->at<int64_t>(lemon_index::WS_I);
    if (int rc = lemon_search_internal(idx_txt, q_txt_dev, nq, kqmax, idx_txt->at<float>(lemon_index::WS_D), Im, stream)) return rc;   // :209
    DiscKsParams p;
    p.E[0] = E_img_tr_dev; p.E[1] = E_txt_tr_dev; p.q[0] = q_img_dev; p.q[1] = q_txt_dev;
    p.Im = Im; p.Ic = Ic_dev; p.out = out_dev; p.nq = nq;
    p.d = d; p.kc = kc; p.kmax = kmax; p.kqmax = kqmax; p.n_ks = n_ks; p.is_train = is_train ? 1 : 0;
    int nmat = 0;
    for (int m = 0; m < 4; ++m) {
        p.mat[m] = 0;
        if (methods & (1 << m)) p.mat[nmat++] = m;
    }
    for (int t = 0; t < DSC_MAX_KS; ++t) p.ks[t] = t < n_ks ? ks[t] : 0;
    const int wmax = dis ? (kmax + 1 > kqmax ? kmax + 1 : kqmax) : kqmax;
    const size_t lds = (size_t)kqmax * wmax * sizeof(float);
    const bool staged = rows_staged(d, {E_img_tr_dev, E_txt_tr_dev, q_img_dev, q_txt_dev});
    const dim3 grid((unsigned)nq, (unsigned)nmat), block(64);
    if (staged) hipLaunchKernelGGL(k_discrepancy_ks<true>, grid, block, lds, stream, p);
    else hipLaunchKernelGGL(k_discrepancy_ks<false>, grid, block, lds, stream, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

// The host twin: the same header with the 64 lanes looped, on neighbour lists the caller brings (no index).  The pair distance
// is the chain contract restated for the host: one fmaf chain over ascending columns, 1 - dot.
static float chain_dist_host(const float *a, const float *b, int d) {
    float acc = 0.0f;
    for (int c = 0; c < d; ++c) acc = fmaf(a[c], b[c], acc);
    return 1.0f - acc;
}

extern "C" int lemon_discrepancy_ks_host(int method, const float *E, int64_t n, int d, const float *qv, const int64_t *Im,
                                         int64_t nq, const int64_t *Ic, int kc, const int32_t *ks, int n_ks, int is_train,
                                         float *out) {
    LEMON_REQUIRE(method == 0 || method == 1, "method: 0 dis, 1 div");
    LEMON_REQUIRE(n >= 1 && d >= 1 && nq >= 0, "n >= 1, d >= 1, nq >= 0");
    if (int rc = check_ks(ks, n_ks)) return rc;
    const int kmax = ks[n_ks - 1], kqmax = kmax + (is_train ? 1 : 0);
    if (method == 0) LEMON_REQUIRE(kc >= kmax + 1 && kc <= LEMON_MAX_K, "ks[n_ks - 1] + 1 <= kc <= LEMON_MAX_K");
    if (nq == 0) return LEMON_OK;
    LEMON_REQUIRE(E && Im && out && (method == 1 || (qv && Ic)), "null pointer");
    const int W = dsc::width(method, kmax, kqmax);
    // the kernel trusts the lists it made itself; these come from the caller
    for (int64_t t = 0; t < nq * kqmax; ++t) {
        LEMON_REQUIRE(Im[t] < n, "Im: row id < n");
        if (method == 0 && Im[t] >= 0)
            for (int b = 0; b < W; ++b) LEMON_REQUIRE(Ic[Im[t] * kc + b] < n, "Ic: row id < n");
    }
    std::vector<float> M((size_t)kqmax * W);
    uint64_t act[dsc::MAX_W];
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t *im = Im + i * kqmax;
        for (int a = 0; a < kqmax; ++a) {
            act[a] = dsc::row_mask(method, im, Ic, kc, a, W);
            for (int b = 0; b < W; ++b) {
                int64_t r0, r1;
                float dist = 0.0f;
                if (dsc::pair_rows(method, im, Ic, kc, a, b, &r0, &r1))
                    dist = chain_dist_host(E + r0 * (int64_t)d, r1 < 0 ? qv + i * (int64_t)d : E + r1 * (int64_t)d, d);
                M[(size_t)a * W + b] = dist;
            }
        }
        for (int ti = 0; ti < n_ks; ++ti) {
            const int k = ks[ti], rows = k + (is_train ? 1 : 0), cols = method == 0 ? k + 1 : rows;
            double total[dsc::LANES];
            int count[dsc::LANES];
            for (int lane = 0; lane < dsc::LANES; ++lane)
                dsc::lane_sum(M.data(), act, W, rows, cols, lane, &total[lane], &count[lane]);
            dsc::butterfly_host(total, count);
            out[(int64_t)ti * nq + i] = dsc::finish(method, total[0], count[0], k);
        }
    }
    return LEMON_OK;
}
