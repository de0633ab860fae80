// The hyper-parameter grid of the LEMoN score for SEVERAL knn_k at once (gfx950 only): lemon_grid_f1_ks.
//
// The record of a k' search is the first k' columns of the record of a deeper search ("k sweep"), and the
// score sum of k_score / k_grid_scores runs j = 0 .. k-1 in order in float64, so the sum after k' terms IS the k' run's sum.
// One walk over the [n, kmax] record therefore yields the neighbour terms of every k in `ks`.  Within a grid the terms depend on
// (tau_1, tau_2) of their side only -- 16 distinct pairs a side on the 21x21x4x4 grid, against 7 056 rows -- so they are
// computed once per distinct pair:
//   stage 1 (host)  distinct (tau_1_n, tau_2_n) and (tau_1_m, tau_2_m) pairs among the G rows, by bit pattern, in order of
//                   first appearance, and per row the index of its pair on each side;
//   stage 2         k_ks_terms: one thread per (sample, pair): the walk over j with k_score's expression and order; at each
//                   j + 1 in ks the running sum / k goes to terms[pair][k index][sample];
//   stage 3         k_ks_combine: score = d1 + beta a + gamma b, the expression of k_grid_scores, for every (k, row, sample);
//                   then k_grid_brent (gridf1_brent.hpp, shared with lemon_grid_f1) over the K * G score rows.
// For every k in ks the outputs equal lemon_grid_f1's on the contiguous [n, k] prefix bit for bit (tests/test_gpu_ksweep.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>

#include <map>
#include <utility>
#include <vector>

#include "common.hpp"
#include "gridf1_brent.hpp"

namespace {

struct KsList { int K; int k[LEMON_KSWEEP_MAX_KS]; };

// pairs [P, 2] = (tau_1, tau_2); the first Pn pairs read the n arrays, the others the m arrays.  terms [P, K, n].
__global__ __launch_bounds__(256) void k_ks_terms(const float *__restrict__ Dn, const float *__restrict__ trn,
                                                  const float *__restrict__ dn, const float *__restrict__ Dm,
                                                  const float *__restrict__ trm, const float *__restrict__ dm, int64_t n,
                                                  int kmax, KsList ks, const double *__restrict__ pairs, int Pn,
                                                  double *__restrict__ terms) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = blockIdx.y;
    const bool nside = p < Pn;                           // block-uniform
    const float *__restrict__ D = nside ? Dn : Dm;
    const float *__restrict__ tr = nside ? trn : trm;
    const float *__restrict__ d = nside ? dn : dm;
    const double t1 = pairs[2 * p], t2 = pairs[2 * p + 1];
    double *__restrict__ out = terms + (int64_t)p * ks.K * n + i;
    double sn = 0.0;
    int next = 0;
    const int last = ks.k[ks.K - 1];                     // nothing deeper is ever read
    for (int j = 0; j < last; ++j) {                     // identical to k_score (rowwise.hip) and k_grid_scores (gridf1.hip)
        const int64_t o = i * (int64_t)kmax + j;
        sn += exp(-t1 * (double)D[o]) * exp(-t2 * (double)tr[o]) * (double)d[o];
        if (j + 1 == ks.k[next]) {
            out[(int64_t)next * n] = sn / (double)(j + 1);
            ++next;
        }
    }
}

// rows [G, 2] = (beta, gamma); pidx [G, 2] = (pair of the n side, pair of the m side, both indices into terms); score [K, G, n]
__global__ __launch_bounds__(256) void k_ks_combine(const float *__restrict__ d1, const double *__restrict__ terms,
                                                    const double *__restrict__ rows, const int32_t *__restrict__ pidx,
                                                    int64_t n, int K, int G, double *__restrict__ score) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = blockIdx.y, kk = blockIdx.z;
    const double beta = rows[2 * g], gamma = rows[2 * g + 1];
    const double a = terms[((int64_t)pidx[2 * g] * K + kk) * n + i];
    const double b = terms[((int64_t)pidx[2 * g + 1] * K + kk) * n + i];
    score[((int64_t)kk * G + g) * n + i] = (double)d1[i] + beta * a + gamma * b;
}

struct KsPlan {
    std::vector<double> pairs;      // [P, 2]
    std::vector<double> rows;       // [G, 2]
    std::vector<int32_t> pidx;      // [G, 2]
    int Pn = 0, P = 0;
};

uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

// stage 1: bit patterns are compared, so 0.0 and -0.0 (and two NaNs of different payload) stay apart
void ks_plan(const double *hp, int G, KsPlan &pl) {
    typedef std::pair<uint64_t, uint64_t> Key;
    std::map<Key, int> seen_n, seen_m;
    std::vector<double> pn, pm;
    pl.rows.resize((size_t)2 * G);
    pl.pidx.resize((size_t)2 * G);
    for (int g = 0; g < G; ++g) {
        const double *r = hp + 6 * (size_t)g;
        pl.rows[2 * (size_t)g] = r[0]; pl.rows[2 * (size_t)g + 1] = r[1];
        auto in = seen_n.insert(std::make_pair(Key(bits_of(r[2]), bits_of(r[3])), (int)seen_n.size()));
        if (in.second) { pn.push_back(r[2]); pn.push_back(r[3]); }
        auto im = seen_m.insert(std::make_pair(Key(bits_of(r[4]), bits_of(r[5])), (int)seen_m.size()));
        if (im.second) { pm.push_back(r[4]); pm.push_back(r[5]); }
        pl.pidx[2 * (size_t)g] = in.first->second;
        pl.pidx[2 * (size_t)g + 1] = im.first->second;
    }
    pl.Pn = (int)seen_n.size();
    pl.P = pl.Pn + (int)seen_m.size();
    for (int g = 0; g < G; ++g) pl.pidx[2 * (size_t)g + 1] += pl.Pn;
    pl.pairs = pn;
    pl.pairs.insert(pl.pairs.end(), pm.begin(), pm.end());
}

// workspace layout, every region a multiple of 8 bytes: terms [P, K, n] f64 | scores [K, G, n] f64 | pairs [P, 2] f64 |
// rows [G, 2] f64 | pidx [G, 2] i32
struct KsLayout { int64_t terms, scores, pairs, rows, pidx, total; };

KsLayout ks_layout(int64_t n, int K, int G, int P) {
    KsLayout L;
    L.terms = 0;
    L.scores = L.terms + (int64_t)P * K * n * 8;
    L.pairs = L.scores + (int64_t)K * G * n * 8;
    L.rows = L.pairs + (int64_t)P * 16;
    L.pidx = L.rows + (int64_t)G * 16;
    L.total = L.pidx + (int64_t)G * 8;
    return L;
}

}  // namespace

extern "C" int64_t lemon_grid_f1_ks_workspace_bytes(int64_t n, int K, int G, const double *hp) {
    if (!(n > 0 && K >= 1 && K <= LEMON_KSWEEP_MAX_KS && G >= 0 && G <= 65535 && (hp || G == 0))) {
        lemon_set_error("invalid argument: n > 0, 1 <= K <= 16, 0 <= G <= 65535, hp != NULL");
        return -1;
    }
    KsPlan pl;
    ks_plan(hp, G, pl);
    return ks_layout(n, K, G, pl.P).total;
}

extern "C" int lemon_grid_f1_ks(const float *d1_dev, const float *D_n_dev, const float *dists_tr_n_dev, const float *dists_n_dev,
                                const float *D_m_dev, const float *dists_tr_m_dev, const float *dists_m_dev,
                                const uint8_t *y_dev, int64_t n, int kmax, const int *ks, int K, const double *hp, int G,
                                double xtol, int maxfun, void *ws_dev, int64_t ws_bytes, double *scores_dev, double *f1_dev,
                                double *thres_dev, void *stream_) {
    LEMON_REQUIRE(n > 0 && kmax >= 1 && kmax <= LEMON_MAX_K && G >= 0 && maxfun >= 1,
                  "n > 0, 1 <= kmax <= LEMON_MAX_K, G >= 0, maxfun >= 1");
    LEMON_REQUIRE(K >= 1 && K <= LEMON_KSWEEP_MAX_KS && ks, "1 <= K <= 16 values of k");
    LEMON_REQUIRE(ks[0] >= 1 && ks[K - 1] <= kmax, "1 <= ks[0], ks[K-1] <= kmax");
    for (int t = 1; t < K; ++t) LEMON_REQUIRE(ks[t - 1] < ks[t], "ks strictly ascending");
    if (G == 0) return LEMON_OK;
    LEMON_REQUIRE(G <= 65535, "at most 65535 grid points per call");
    LEMON_REQUIRE(d1_dev && D_n_dev && dists_tr_n_dev && dists_n_dev && D_m_dev && dists_tr_m_dev && dists_m_dev && y_dev && hp &&
                      ws_dev && f1_dev && thres_dev, "null pointer");
    LEMON_REQUIRE(((uintptr_t)ws_dev & 7) == 0, "workspace aligned to 8 bytes");
    KsPlan pl;
    ks_plan(hp, G, pl);
    const KsLayout L = ks_layout(n, K, G, pl.P);
    LEMON_REQUIRE(ws_bytes >= L.total, "workspace smaller than lemon_grid_f1_ks_workspace_bytes(n, K, G, hp)");
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)ws_dev;
    double *terms = (double *)(ws + L.terms), *pairs = (double *)(ws + L.pairs), *rows = (double *)(ws + L.rows);
    double *score = scores_dev ? scores_dev : (double *)(ws + L.scores);
    int32_t *pidx = (int32_t *)(ws + L.pidx);
    // the three tables are contiguous in the workspace; the plan's vectors live until the copies have left the host
    LEMON_HIP_CHECK(hipMemcpyAsync(pairs, pl.pairs.data(), (size_t)pl.P * 16, hipMemcpyHostToDevice, stream));
    LEMON_HIP_CHECK(hipMemcpyAsync(rows, pl.rows.data(), (size_t)G * 16, hipMemcpyHostToDevice, stream));
    LEMON_HIP_CHECK(hipMemcpyAsync(pidx, pl.pidx.data(), (size_t)G * 8, hipMemcpyHostToDevice, stream));
    LEMON_HIP_CHECK(hipStreamSynchronize(stream));
    KsList kl;
    kl.K = K;
    for (int t = 0; t < LEMON_KSWEEP_MAX_KS; ++t) kl.k[t] = t < K ? ks[t] : 0;
    const unsigned bx = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_ks_terms, dim3(bx, (unsigned)pl.P), dim3(256), 0, stream, D_n_dev, dists_tr_n_dev, dists_n_dev, D_m_dev,
                       dists_tr_m_dev, dists_m_dev, n, kmax, kl, pairs, pl.Pn, terms);
    LEMON_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ks_combine, dim3(bx, (unsigned)G, (unsigned)K), dim3(256), 0, stream, d1_dev, terms, rows, pidx, n, K, G,
                       score);
    LEMON_HIP_CHECK(hipGetLastError());
    const double sqrt_eps = sqrt(2.2e-16), golden_mean = 0.5 * (3.0 - sqrt(5.0));
    const int rows_total = K * G;                        // <= 16 * 65535
    hipLaunchKernelGGL(k_grid_brent, dim3((unsigned)((rows_total + 3) / 4)), dim3(256), 0, stream, score, y_dev, n, rows_total, xtol,
                       maxfun, sqrt_eps, golden_mean, f1_dev, thres_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
