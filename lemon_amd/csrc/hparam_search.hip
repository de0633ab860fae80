// The local searches of the hyper-parameter search on the device (gfx950 only, opt-in): lemon_hparam_search.
//
// maximize_metric (lib/metrics/utils.py:151-158) runs scipy.optimize.minimize from four start points with Powell and
// Nelder-Mead in front of the grid.  On the host every objective evaluation of those searches is one lemon_score launch, a
// device -> host copy and a fminbound in numpy: 23 .. 1 276 evaluations a search, all serial ("Local
// searches on the device").  Here a whole search is one workgroup of k_hparam_search and S searches are one launch:
//   * the optimiser (hparam_search_core.hpp, a restatement of scipy 1.15 in IEEE double) runs in every thread of the
//     workgroup on the same values, so its control flow is uniform and a barrier inside the objective is met by all;
//   * the objective is evaluated by all threads: thread t scores the samples t, t + 512, ... with the expression of k_score
//     (same order over j, default contraction, rows of pitch kmax so that k < kmax is the prefix record of a k sweep) and
//     counts its own samples against a threshold; the counts are summed over the workgroup as integers;
//   * the score row lives in LDS beside the labels while 9 n bytes fit into 48 KB, else in the search's slice of the workspace.
//     A thread only ever reads the scores it wrote.
// Recorded on an MI355X (tools/hparam_search_time.py, profiles/hparam_search/): the 64 searches of an eight-k sweep take 0.064 s
// at n = 250 and 0.42 s at n = 5 000, against 4.06 s and 7.03 s on the host path; same bits.
// The host twin (lemon_hparam_search_host, lemon_hparam_objective_host) compiles the same header with the threads looped on the
// host and libm's exp; it exists for the tests, no product path calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <vector>

#include "common.hpp"
#include "hparam_search_core.hpp"

static_assert(sizeof(LemonSearchResult) == sizeof(hps::Result) && sizeof(hps::Result) == 72, "LemonSearchResult layout");
static_assert(LEMON_SEARCH_NELDER_MEAD == hps::NELDER_MEAD && LEMON_SEARCH_POWELL == hps::POWELL, "method ids");

namespace {

constexpr int HPS_THREADS = 512, HPS_WAVES = HPS_THREADS / 64;
constexpr int64_t HPS_LDS_BYTES = 48 * 1024;             // dynamic LDS of a workgroup: scores [n] f64 | labels [n] u8

struct Record {
    const float *d1, *Dn, *trn, *dn, *Dm, *trm, *dm;
    const uint8_t *y;
    int64_t n;
    int kmax;
};

// score[i] at depth k: identical to k_score (rowwise.hip) and k_grid_scores (gridf1.hip), default contraction
__host__ __device__ inline double score_row(const Record &r, int64_t i, int k, const double *hp) {
    const double beta = hp[0], gamma = hp[1], t1n = hp[2], t2n = hp[3], t1m = hp[4], t2m = hp[5];
    double sn = 0.0, sm = 0.0;
    for (int j = 0; j < k; ++j) {
        const int64_t o = i * (int64_t)r.kmax + j;
        sn += exp(-t1n * (double)r.Dn[o]) * exp(-t2n * (double)r.trn[o]) * (double)r.dn[o];
        sm += exp(-t1m * (double)r.Dm[o]) * exp(-t2m * (double)r.trm[o]) * (double)r.dm[o];
    }
    const double a = sn / (double)k, b = sm / (double)k;
    return (double)r.d1[i] + beta * a + gamma * b;
}

// sklearn's binary F1 from integer counts, negated; 0 when nothing is counted
__host__ __device__ inline double neg_f1_of(long long pred, long long tp, long long pos) {
#pragma clang fp contract(off)
    const long long denom = 2 * tp + (pred - tp) + (pos - tp);
    return denom ? -(2.0 * (double)tp / (double)denom) : -0.0;
}

// Reduction slots of the workgroup.  Two sets used in turn: a thread can write set b again only behind the barrier of the
// reduction in between, which every thread reaches after its reads of set b, so one barrier a reduction is enough.
struct Slots {
    long long cnt[2][HPS_WAVES][2];
    double lohi[2][HPS_WAVES][2];
    int bad[2][HPS_WAVES];
};

struct DevBackend {
    Record r;
    int k;
    double *s;               // the score row: LDS or the workspace slice
    const uint8_t *yl;       // the labels: LDS or global
    Slots *sl;
    long long pos;
    int flip;

    __device__ void sum2(long long &a, long long &b) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
        const int set = flip, w = threadIdx.x >> 6;
        flip ^= 1;
        if ((threadIdx.x & 63) == 0) { sl->cnt[set][w][0] = a; sl->cnt[set][w][1] = b; }
        __syncthreads();
        a = b = 0;
        for (int v = 0; v < HPS_WAVES; ++v) { a += sl->cnt[set][v][0]; b += sl->cnt[set][v][1]; }
    }

    __device__ bool scores(const double *hp, double &lo_out, double &hi_out) {
        double lo = INFINITY, hi = -INFINITY;
        int bad = 0;
        for (int64_t i = threadIdx.x; i < r.n; i += HPS_THREADS) {
            const double v = score_row(r, i, k, hp);
            s[i] = v;
            bad |= !hps::is_finite(v);
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
            lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
            bad |= __shfl_xor(bad, off);
        }
        const int set = flip, w = threadIdx.x >> 6;
        flip ^= 1;
        if ((threadIdx.x & 63) == 0) { sl->lohi[set][w][0] = lo; sl->lohi[set][w][1] = hi; sl->bad[set][w] = bad; }
        __syncthreads();
        lo = INFINITY; hi = -INFINITY; bad = 0;
        for (int v = 0; v < HPS_WAVES; ++v) {
            const double l2 = sl->lohi[set][v][0], h2 = sl->lohi[set][v][1];
            lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
            bad |= sl->bad[set][v];
        }
        lo_out = lo; hi_out = hi;
        return !bad;
    }

    __device__ double neg_f1(double t) {
        long long pred = 0, tp = 0;
        for (int64_t i = threadIdx.x; i < r.n; i += HPS_THREADS) {
            const bool p = s[i] >= t;
            pred += p;
            tp += p && yl[i];
        }
        sum2(pred, tp);
        return neg_f1_of(pred, tp, pos);
    }
};

struct SearchArgs {
    Record r;
    const double *x0;        // [S, 6]
    const int32_t *spec;     // [S, 4]
    double *ws;              // [S, n] when the score rows do not live in LDS
    int use_lds;
    hps::Caps caps;
    double sqrt_eps, golden_mean;
    hps::Result *out;        // [S]
};

// one workgroup per search; every thread runs the optimiser on the same values (uniform control flow)
__global__ __launch_bounds__(HPS_THREADS) void k_hparam_search(SearchArgs a) {
    extern __shared__ double smem[];
    __shared__ Slots slots;
    const int sidx = blockIdx.x;
    const int32_t *sp = a.spec + 4 * (int64_t)sidx;
    DevBackend b;
    b.r = a.r; b.k = sp[1]; b.sl = &slots; b.flip = 0; b.pos = 0;
    if (a.use_lds) {
        uint8_t *yl = (uint8_t *)(smem + a.r.n);
        for (int64_t i = threadIdx.x; i < a.r.n; i += HPS_THREADS) yl[i] = a.r.y[i];   // read back by the same thread only
        b.s = smem; b.yl = yl;
    } else {
        b.s = a.ws + (int64_t)sidx * a.r.n; b.yl = a.r.y;
    }
    long long pos = 0, none = 0;
    for (int64_t i = threadIdx.x; i < a.r.n; i += HPS_THREADS) pos += b.yl[i] != 0;
    b.sum2(pos, none);
    b.pos = pos;
    hps::Objective<DevBackend> obj{b, (uint32_t)sp[2], (uint32_t)sp[3], a.sqrt_eps, a.golden_mean};
    double x0[hps::N];
    for (int c = 0; c < hps::N; ++c) x0[c] = a.x0[hps::N * (int64_t)sidx + c];
    hps::Result res;
    hps::search(obj, sp[0], x0, a.caps, res);
    if (threadIdx.x == 0) a.out[sidx] = res;
}

// the threads of the workgroup looped on the host
struct HostBackend {
    Record r;
    int k;
    std::vector<double> s;
    long long pos;
    bool scores(const double *hp, double &lo, double &hi) {
        lo = INFINITY; hi = -INFINITY;
        bool bad = false;
        for (int64_t i = 0; i < r.n; ++i) {
            const double v = score_row(r, i, k, hp);
            s[i] = v;
            bad |= !hps::is_finite(v);
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
        return !bad;
    }
    double neg_f1(double t) {
        long long pred = 0, tp = 0;
        for (int64_t i = 0; i < r.n; ++i) {
            const bool p = s[i] >= t;
            pred += p;
            tp += p && r.y[i];
        }
        return neg_f1_of(pred, tp, pos);
    }
};

HostBackend host_backend(const Record &r, int k) {
    HostBackend b;
    b.r = r; b.k = k; b.s.resize((size_t)r.n); b.pos = 0;
    for (int64_t i = 0; i < r.n; ++i) b.pos += r.y[i] != 0;
    return b;
}

// test-only knobs (lemon_hparam_search_set_test_knobs)
int g_force_workspace = 0;
hps::Caps g_caps = hps::DEFAULT_CAPS;

double sqrt_eps() { return sqrt(2.2e-16); }
double golden_mean() { return 0.5 * (3.0 - sqrt(5.0)); }

int check_spec(const int32_t *spec, int S, int kmax) {
    for (int s = 0; s < S; ++s) {
        const int32_t *sp = spec + 4 * (size_t)s;
        LEMON_REQUIRE(sp[0] == LEMON_SEARCH_NELDER_MEAD || sp[0] == LEMON_SEARCH_POWELL, "spec: unknown method");
        LEMON_REQUIRE(sp[1] >= 1 && sp[1] <= kmax, "spec: 1 <= k <= kmax");
        LEMON_REQUIRE((sp[2] & ~63) == 0 && (sp[3] & ~63) == 0, "spec: the force masks have six bits");
    }
    return LEMON_OK;
}

}  // namespace

extern "C" int lemon_hparam_search_set_test_knobs(int force_workspace, int nm_maxiter, int nm_maxfun, int powell_maxiter,
                                                  int powell_maxfun) {
    g_force_workspace = force_workspace != 0;
    g_caps.nm_maxiter = nm_maxiter > 0 ? nm_maxiter : hps::DEFAULT_CAPS.nm_maxiter;
    g_caps.nm_maxfun = nm_maxfun > 0 ? nm_maxfun : hps::DEFAULT_CAPS.nm_maxfun;
    g_caps.pw_maxiter = powell_maxiter > 0 ? powell_maxiter : hps::DEFAULT_CAPS.pw_maxiter;
    g_caps.pw_maxfun = powell_maxfun > 0 ? powell_maxfun : hps::DEFAULT_CAPS.pw_maxfun;
    return LEMON_OK;
}

extern "C" int64_t lemon_hparam_search_workspace_bytes(int64_t n, int S) {
    if (!(n > 0 && S >= 0 && S <= 65535 && n <= (int64_t)1 << 40)) {
        lemon_set_error("invalid argument: n > 0, 0 <= S <= 65535");
        return LEMON_E_INVALID;
    }
    return S > 0 ? (int64_t)S * n * 8 : 8;
}

#define HPS_RECORD_NONNULL                                                                                                   \
    (d1 && D_n && dists_tr_n && dists_n && D_m && dists_tr_m && dists_m && y && x0 && spec && out)

extern "C" int lemon_hparam_search(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                   const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y, int64_t n,
                                   int kmax, int S, const double *x0, const int32_t *spec, void *ws, int64_t ws_bytes,
                                   LemonSearchResult *out, void *stream_) {
    LEMON_REQUIRE(n > 0 && n <= (int64_t)1 << 40 && kmax >= 1 && S >= 0 && S <= 65535, "n > 0, kmax >= 1, 0 <= S <= 65535");
    if (S == 0) return LEMON_OK;
    LEMON_REQUIRE(HPS_RECORD_NONNULL && ws, "null pointer");
    LEMON_REQUIRE(((uintptr_t)ws & 7) == 0, "workspace aligned to 8 bytes");
    LEMON_REQUIRE(ws_bytes >= (int64_t)S * n * 8, "workspace smaller than lemon_hparam_search_workspace_bytes(n, S)");
    hipStream_t stream = (hipStream_t)stream_;
    // the kernel indexes the record with k and branches on the method: both are checked here, before anything is launched
    std::vector<int32_t> spec_h((size_t)4 * S);
    LEMON_HIP_CHECK(hipMemcpyAsync(spec_h.data(), spec, spec_h.size() * 4, hipMemcpyDeviceToHost, stream));
    LEMON_HIP_CHECK(hipStreamSynchronize(stream));
    if (int rc = check_spec(spec_h.data(), S, kmax)) return rc;
    SearchArgs a;
    a.r = Record{d1, D_n, dists_tr_n, dists_n, D_m, dists_tr_m, dists_m, y, n, kmax};
    a.x0 = x0; a.spec = spec; a.ws = (double *)ws;
    const int64_t lds = 8 * n + ((n + 7) & ~(int64_t)7);
    a.use_lds = !g_force_workspace && lds <= HPS_LDS_BYTES;
    a.caps = g_caps;
    a.sqrt_eps = sqrt_eps(); a.golden_mean = golden_mean();
    a.out = (hps::Result *)out;
    hipLaunchKernelGGL(k_hparam_search, dim3((unsigned)S), dim3(HPS_THREADS), a.use_lds ? (size_t)lds : 0, stream, a);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

extern "C" int lemon_hparam_search_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                        const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                                        int64_t n, int kmax, int S, const double *x0, const int32_t *spec, void *ws,
                                        int64_t ws_bytes, LemonSearchResult *out) {
    LEMON_REQUIRE(n > 0 && n <= (int64_t)1 << 40 && kmax >= 1 && S >= 0 && S <= 65535, "n > 0, kmax >= 1, 0 <= S <= 65535");
    if (S == 0) return LEMON_OK;
    LEMON_REQUIRE(HPS_RECORD_NONNULL && ws, "null pointer");
    LEMON_REQUIRE(ws_bytes >= (int64_t)S * n * 8, "workspace smaller than lemon_hparam_search_workspace_bytes(n, S)");
    if (int rc = check_spec(spec, S, kmax)) return rc;
    const Record r{d1, D_n, dists_tr_n, dists_n, D_m, dists_tr_m, dists_m, y, n, kmax};
    for (int s = 0; s < S; ++s) {
        const int32_t *sp = spec + 4 * (size_t)s;
        HostBackend b = host_backend(r, sp[1]);
        hps::Objective<HostBackend> obj{b, (uint32_t)sp[2], (uint32_t)sp[3], sqrt_eps(), golden_mean()};
        hps::search(obj, sp[0], x0 + hps::N * (size_t)s, g_caps, *(hps::Result *)(out + s));
    }
    return LEMON_OK;
}

extern "C" double lemon_hparam_objective_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                              const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                                              int64_t n, int kmax, int k, int force_zero, int force_one, const double *x) {
    if (!(d1 && D_n && dists_tr_n && dists_n && D_m && dists_tr_m && dists_m && y && x && n > 0 && k >= 1 && k <= kmax &&
          (force_zero & ~63) == 0 && (force_one & ~63) == 0)) {
        lemon_set_error("invalid argument: null pointer, n > 0, 1 <= k <= kmax, six-bit force masks");
        return NAN;
    }
    const Record r{d1, D_n, dists_tr_n, dists_n, D_m, dists_tr_m, dists_m, y, n, kmax};
    HostBackend b = host_backend(r, k);
    hps::Objective<HostBackend> obj{b, (uint32_t)force_zero, (uint32_t)force_one, sqrt_eps(), golden_mean()};
    return obj(x);
}
