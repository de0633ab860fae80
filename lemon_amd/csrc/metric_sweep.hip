// metric_sweep.hip -- both dist_type values of the reference's grid from ONE scan (gfx950 only): the exact squared-L2 lists of
// an IndexFlatL2 derived from the lists of an IndexFlatIP over the same rows ("Metric sweep").
//
//   lemon_index_l2_from_ip   k_l2_from_ip on the lists of a finished IP search: one wave per query, one lane per candidate
//   lemon_l2_from_ip_host    the same header (l2_from_ip_core.hpp) with the lanes looped on the host, for the tests
//   lemon_neighbors_metrics  lemon_neighbors for both metrics: each side searched once at k + drop_self + margin, the cosine
//                            record from the first k + drop_self columns, the euclidean one from the derived lists, both through
//                            k_neighbors_finalize (api.hip)
// The derivation, its certificate and why the certificate is sound: l2_from_ip_core.hpp.  A row that is not certified is the
// caller's to search again with an IndexFlatL2 (neighbors.LemonDB.neighbors_metrics does).
#include "common.hpp"
#include "l2_from_ip_core.hpp"

namespace {

// min and max of the stored norms as float bits.  Norms are sums of squares: >= +0 or NaN, so the unsigned order of the bits is
// the order of the values, with every infinity and NaN (either sign bit) above FLT_MAX.  out[0] starts at FLT_MAX, out[1] at 0.
__global__ __launch_bounds__(256) void k_norm_range(const float *__restrict__ v, int64_t n, unsigned *__restrict__ out) {
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned b = __float_as_uint(v[i]);
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(out, lo); atomicMax(out + 1, hi); }
}

struct L2ipParams {
    const float *s;          // [nq, kd] IP scores, best first
    const int64_t *ids;      // [nq, kd]
    const float *qq;         // [nq]
    const float *xx;         // [n]
    const unsigned *xrange;  // k_norm_range's two scalars
    int64_t n, nq;
    int kd, k;
    float *D;                // [nq, k]
    int64_t *I;              // [nq, k]
    uint8_t *cert;           // [nq]
};

constexpr int L2IP_WAVES = 4;

// One wave per query, lane j holds slot j of the IP list (kd <= 64).  Every lane computes its D, the wave publishes (D, id,
// real) in LDS once, and every lane counts the slots that precede its own: that count is its place in the L2 list.
__global__ __launch_bounds__(64 * L2IP_WAVES) void k_l2_from_ip(L2ipParams p) {
    __shared__ float s_D[L2IP_WAVES][64];
    __shared__ int64_t s_id[L2IP_WAVES][64];
    __shared__ unsigned char s_real[L2IP_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * L2IP_WAVES + wave;
    const bool valid = q0 < p.nq;                       // wave-uniform; idle waves shadow the last query and write nothing
    const int64_t q = valid ? q0 : p.nq - 1;
    const float *s = p.s + q * p.kd;
    const int64_t *ids = p.ids + q * p.kd;
    const bool active = lane < p.kd;
    const int64_t id = active ? ids[lane] : -1;
    const bool real = id >= 0 && id < p.n;
    const float sj = active ? s[lane] : 0.0f;
    const float qq = p.qq[q];
    const float D = real ? l2ip::dist(sj, qq, p.xx[id]) : 0.0f;
    const bool bad = id >= p.n || (real && !l2ip::is_finite(sj));
    s_D[wave][lane] = D;
    s_id[wave][lane] = id;
    s_real[wave][lane] = real ? 1 : 0;
    __syncthreads();
    if (!valid) return;
    const int n_real = __popcll(__ballot(real));
    const int rank = real ? l2ip::rank_of(s_D[wave], s_id[wave], s_real[wave], p.kd, lane) : 64;
    const unsigned lo = p.xrange[0], hi = p.xrange[1];
    const float xx_min = hi < 0x7f800000u ? __uint_as_float(lo) : __builtin_nanf("");   // a norm that is not finite: nothing certified
    const bool whole_db = ids[p.kd - 1] < 0;
    const float B = l2ip::bound(s[p.kd - 1], qq, xx_min);
    const bool below = real && rank == p.k - 1 && D < B;
    const bool ok = l2ip::is_finite(qq) && l2ip::is_finite(xx_min) && !__any(bad);
    const bool cert = ok && (whole_db || __any(below));
    float *Do = p.D + q * p.k;
    int64_t *Io = p.I + q * p.k;
    if (rank < p.k) { Do[rank] = D; Io[rank] = id; }                       // rank < n_real: a permutation of the real slots
    if (lane < p.k && lane >= n_real) { Do[lane] = FLT_MAX; Io[lane] = -1; }
    if (lane == 0) p.cert[q] = cert ? 1 : 0;
}

// the stored norms' range, reduced once per index content (every add changes n)
int norm_range(lemon_index_t *idx, hipStream_t stream) {
    if (idx->xnrange_rows == idx->n + 1) return LEMON_OK;
    int rc = lemon_reserve(idx, lemon_index::XNRANGE, 8, stream, "norm range");
    if (rc) return rc;
    unsigned *range = idx->at<unsigned>(lemon_index::XNRANGE);
    // FLT_MAX, +0: what an empty index keeps
    LEMON_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)range, 0x7f7fffff, 1, stream));
    LEMON_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(range + 1), 0, 1, stream));
    if (idx->n > 0) {
        const int64_t blocks = (idx->n + 255) / 256;
        hipLaunchKernelGGL(k_norm_range, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, stream, idx->xnorm, idx->n, range);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    idx->xnrange_rows = idx->n + 1;
    return LEMON_OK;
}

// the lists of `nq` queries; every pointer is a device pointer and checked by the caller
int derive(lemon_index_t *idx, const float *qq, int64_t nq, const float *D_ip, const int64_t *I_ip, int kd, int k, float *D_l2,
           int64_t *I_l2, uint8_t *cert, hipStream_t stream) {
    int rc = norm_range(idx, stream);
    if (rc) return rc;
    L2ipParams p;
    p.s = D_ip; p.ids = I_ip; p.qq = qq; p.xx = idx->xnorm; p.xrange = idx->at<unsigned>(lemon_index::XNRANGE);
    p.n = idx->n; p.nq = nq; p.kd = kd; p.k = k; p.D = D_l2; p.I = I_l2; p.cert = cert;
    const int64_t blocks = (nq + L2IP_WAVES - 1) / L2IP_WAVES;
    LEMON_REQUIRE(blocks <= 0x7fffffff, "nq < 2^33");
    hipLaunchKernelGGL(k_l2_from_ip, dim3((unsigned)blocks), dim3(64 * L2IP_WAVES), 0, stream, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

}  // namespace

extern "C" int lemon_index_l2_from_ip(lemon_index_t *idx, const float *q_dev, int64_t nq, const float *D_ip_dev,
                                      const int64_t *I_ip_dev, int kd, int k, float *D_l2_dev, int64_t *I_l2_dev,
                                      uint8_t *cert_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LEMON_REQUIRE(idx != nullptr, "index handle");
    LEMON_REQUIRE(idx->metric == LEMON_METRIC_IP, "the index must be an IndexFlatIP");
    LEMON_REQUIRE(nq >= 0, "nq >= 0");
    LEMON_REQUIRE(k >= 1 && k <= kd && kd <= LEMON_MAX_K, "1 <= k <= kd <= LEMON_MAX_K");
    LEMON_REQUIRE(q_dev && D_ip_dev && I_ip_dev && D_l2_dev && I_l2_dev && cert_dev, "null pointer");
    LEMON_REQUIRE(rows_vector_safe(q_dev, idx->d), "q_dev must be 16-byte aligned when d % 4 == 0");
    if (nq == 0) return LEMON_OK;
    int rc = lemon_reserve_nb(idx, nq, stream);          // qq [nq] lives at the front of the neighbour workspace
    if (rc) return rc;
    float *qq = idx->at<float>(lemon_index::WS_D);
    rc = lemon_rowdot_chain(q_dev, q_dev, nq, idx->d, qq, stream);
    if (rc) return rc;
    return derive(idx, qq, nq, D_ip_dev, I_ip_dev, kd, k, D_l2_dev, I_l2_dev, cert_dev, stream);
}

extern "C" int lemon_l2_from_ip_host(const float *qq, const float *xx, int64_t n, float xx_min, const float *D_ip,
                                     const int64_t *I_ip, int64_t nq, int kd, int k, float *D_l2, int64_t *I_l2, uint8_t *cert) {
    LEMON_REQUIRE(n >= 0 && nq >= 0, "n >= 0, nq >= 0");
    LEMON_REQUIRE(k >= 1 && k <= kd && kd <= LEMON_MAX_K, "1 <= k <= kd <= LEMON_MAX_K");
    LEMON_REQUIRE(qq && (xx || n == 0) && D_ip && I_ip && D_l2 && I_l2 && cert, "null pointer");
    for (int64_t i = 0; i < nq; ++i)
        cert[i] = l2ip::derive_row(D_ip + i * kd, I_ip + i * kd, kd, k, qq[i], xx, n, xx_min, D_l2 + i * k, I_l2 + i * k);
    return LEMON_OK;
}

extern "C" int lemon_neighbors_metrics(lemon_index_t *idx_img, lemon_index_t *idx_txt, const float *dists_tr_ip_dev,
                                       const float *dists_tr_l2_dev, const float *q_img_dev, const float *q_txt_dev, int64_t nq,
                                       int k, int drop_self, const uint8_t *in_db_dev, int discrete,
                                       const int32_t *tr_label_id_dev, const int32_t *q_label_id_dev, int margin,
                                       float *d1_dev, float *D_n_dev, float *dists_n_dev, float *dists_tr_n_dev,
                                       int64_t *I_n_dev, float *D_m_dev, float *dists_m_dev, float *dists_tr_m_dev,
                                       int64_t *I_m_dev, float *d1_l2_dev, float *D_n_l2_dev, float *dists_n_l2_dev,
                                       float *dists_tr_n_l2_dev, int64_t *I_n_l2_dev, float *D_m_l2_dev, float *dists_m_l2_dev,
                                       float *dists_tr_m_l2_dev, int64_t *I_m_l2_dev, uint8_t *cert_n_dev, uint8_t *cert_m_dev,
                                       void *stream_) {
    float *const ip_f32[7] = {d1_dev, D_n_dev, dists_n_dev, dists_tr_n_dev, D_m_dev, dists_m_dev, dists_tr_m_dev};
    float *const l2_f32[7] = {d1_l2_dev, D_n_l2_dev, dists_n_l2_dev, dists_tr_n_l2_dev, D_m_l2_dev, dists_m_l2_dev, dists_tr_m_l2_dev};
    int64_t *const ip_i64[2] = {I_n_dev, I_m_dev}, *const l2_i64[2] = {I_n_l2_dev, I_m_l2_dev};
    hipStream_t stream = (hipStream_t)stream_;
    const TwoSided c = {idx_img, idx_txt, q_img_dev, q_txt_dev, nq, k, drop_self, discrete, in_db_dev, tr_label_id_dev, q_label_id_dev};
    LEMON_REQUIRE(!idx_img || !idx_txt || (idx_img->metric == LEMON_METRIC_IP && idx_txt->metric == LEMON_METRIC_IP),
                  "both indices must be IndexFlatIP");
    int rc = lemon_two_sided_check(c);
    if (rc) return rc;
    LEMON_REQUIRE(margin >= 0, "margin >= 0");
    LEMON_REQUIRE(cert_n_dev && cert_m_dev && dists_tr_ip_dev && dists_tr_l2_dev, "null pointer");
    for (int t = 0; t < 7; ++t) LEMON_REQUIRE(ip_f32[t] && l2_f32[t], "null pointer");
    const int ks = k + (drop_self ? 1 : 0), kd = ks + margin < LEMON_MAX_K ? ks + margin : LEMON_MAX_K;
    // the image index's neighbour workspace: IP lists [2][nq, kd] | L2 lists [2][nq, ks] | qq [2][nq] (WS_D only)
    rc = lemon_two_sided_search(c, kd, 2 * nq * (kd + ks) + 2 * nq, stream);
    if (rc || nq == 0) return rc;
    float *Dn = idx_img->at<float>(lemon_index::WS_D), *Dm = Dn + nq * kd, *Ln = Dm + nq * kd, *Lm = Ln + nq * ks, *qqv = Lm + nq * ks, *qqt = qqv + nq;
    int64_t *In = idx_img->at<int64_t>(lemon_index::WS_I), *Im = In + nq * kd, *Jn = Im + nq * kd, *Jm = Jn + nq * ks;
    const int d = idx_img->d;
    if ((rc = lemon_rowdot_chain(q_img_dev, q_img_dev, nq, d, qqv, stream))) return rc;
    if ((rc = lemon_rowdot_chain(q_txt_dev, q_txt_dev, nq, d, qqt, stream))) return rc;
    if ((rc = derive(idx_img, qqv, nq, Dn, In, kd, ks, Ln, Jn, cert_n_dev, stream))) return rc;
    if ((rc = derive(idx_txt, qqt, nq, Dm, Im, kd, ks, Lm, Jm, cert_m_dev, stream))) return rc;
    for (int m = 0; m < 2; ++m) {                        // 0: cosine from the IP lists' prefix, 1: euclidean from the derived lists
        float *const *f = m ? l2_f32 : ip_f32;
        int64_t *const *ix = m ? l2_i64 : ip_i64;
        NbParams p = lemon_nb_params(c);
        p.metric = m ? LEMON_METRIC_L2 : LEMON_METRIC_IP;
        if ((rc = lemon_paired_distance(p.metric, q_img_dev, q_txt_dev, nq, d, f[0], stream))) return rc;
        p.dists_tr = m ? dists_tr_l2_dev : dists_tr_ip_dev; p.ks = m ? ks : kd;
        p.Dn = m ? Ln : Dn; p.Dm = m ? Lm : Dm; p.In = m ? Jn : In; p.Im = m ? Jm : Im;
        p.D_n = f[1]; p.dists_n = f[2]; p.dists_tr_n = f[3]; p.D_m = f[4]; p.dists_m = f[5]; p.dists_tr_m = f[6];
        p.I_n = ix[0]; p.I_m = ix[1];
        if ((rc = lemon_neighbors_finalize(p, stream))) return rc;
    }
    return LEMON_OK;
}
