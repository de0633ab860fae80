// The LBFGS polish of the hyper-parameter search on the device (gfx950 only, opt-in): lemon_lbfgs_polish.
//
// maximize_metric (lib/metrics/utils.py:160-176) polishes four start points on a SoftMargin proxy of the score with
// torch.optim.LBFGS: 4 starts x 20 optimizer.step calls x up to 25 closure evaluations, each a handful of tiny torch kernels plus
// autograd, all serial and launch-bound (about 3 s a knn_k on the device, whatever n: DESIGN.md section 5, "The polish on the
// device").  Here a whole polish is one workgroup of k_lbfgs_polish and the S polishes of a run (four starts for every k of a
// sweep) are one launch, laid out like k_hparam_search:
//   * the optimiser (lbfgs_core.hpp, a restatement of torch 2.10's LBFGS in IEEE double) runs in every thread of the workgroup
//     on the same values, so its control flow is uniform and the barrier inside the objective is met by all;
//   * the objective is evaluated by all threads: thread t sums the proxy's value and gradient terms over the rows t, t + 256, ...
//     (2 n k float64 exp an evaluation), the sums go through a 64-lane xor butterfly and then the waves are added in index order;
//   * the history (100 x 2 x 6 doubles, ro and al beside it: 11.2 KB) lives in LDS, written by every thread with the same values.
// The workgroup is 256 threads, one wave a SIMD: a polish is a serial chain of evaluations and a launch holds at most a few
// dozen polishes on 256 CUs, so what counts is the latency of one evaluation, and the two exp chains of a row (n and m side)
// are independent; a single wave a SIMD keeps the whole register file for the optimiser's state (215 VGPRs, none spilled).
// Recorded on an MI355X (tools/lbfgs_polish_time.py, profiles/hparam_search/lbfgs_polish.json): the 32 polishes of an eight-k
// sweep take 0.015 s at n = 250 and 0.30 s at n = 5 000, against 30.8 s and 27.4 s of torch.optim.LBFGS on the device.
// The host twin (lemon_lbfgs_polish_host, lemon_lbfgs_proxy_host) compiles the same header with the threads looped on the host
// in the same reduction order; same bits.  It exists for the tests, no product path calls it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <vector>

#include "common.hpp"
#include "lbfgs_core.hpp"

static_assert(sizeof(LemonPolishResult) == sizeof(lbp::Result) && sizeof(lbp::Result) == 72, "LemonPolishResult layout");

namespace {

// Reduction slots of the workgroup.  Two sets used in turn: a thread can write set b again only behind the barrier of the
// reduction in between, which every thread reaches after its reads of set b, so one barrier a reduction is enough.
struct Slots { double sum[2][lbp::WAVES][lbp::NSUM]; };

struct DevBackend {
    lbp::Record r;
    int k;
    Slots *sl;
    int flip;

    __device__ void reduce(const double *hp, double *sum) {
#pragma clang fp contract(off)
        for (int c = 0; c < lbp::NSUM; ++c) sum[c] = 0.0;
        for (int64_t i = threadIdx.x; i < r.n; i += lbp::THREADS) lbp::proxy_row(r, i, k, hp, sum);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            for (int c = 0; c < lbp::NSUM; ++c) sum[c] = sum[c] + __shfl_xor(sum[c], off);
        const int set = flip, w = threadIdx.x >> 6;
        flip ^= 1;
        if ((threadIdx.x & 63) == 0)
            for (int c = 0; c < lbp::NSUM; ++c) sl->sum[set][w][c] = sum[c];
        __syncthreads();
        for (int c = 0; c < lbp::NSUM; ++c) {
            double a = 0.0;
            for (int v = 0; v < lbp::WAVES; ++v) a += sl->sum[set][v][c];
            sum[c] = a;
        }
    }
};

struct PolishArgs {
    lbp::Record r;
    const double *x0;        // [S, 6]
    const int32_t *spec;     // [S, 3]: k, force_zero, force_one
    int outer_steps;
    lbp::Result *out;        // [S]
};

// one workgroup per polish; every thread runs the optimiser on the same values (uniform control flow)
__global__ __launch_bounds__(lbp::THREADS) void k_lbfgs_polish(PolishArgs a) {
    __shared__ Slots slots;
    __shared__ double dirs[lbp::HISTORY][lbp::N], stps[lbp::HISTORY][lbp::N], ro[lbp::HISTORY], al[lbp::HISTORY];
    const int sidx = blockIdx.x;
    const int32_t *sp = a.spec + 3 * (int64_t)sidx;
    DevBackend b{a.r, sp[0], &slots, 0};
    lbp::Proxy<DevBackend> f{b, (uint32_t)sp[1], (uint32_t)sp[2], a.r.n};
    const lbp::History h{dirs, stps, ro, al};
    double x0[lbp::N];
    for (int c = 0; c < lbp::N; ++c) x0[c] = a.x0[lbp::N * (int64_t)sidx + c];
    lbp::Result res;
    lbp::polish(f, x0, a.outer_steps, h, res);
    if (threadIdx.x == 0) a.out[sidx] = res;
}

// the threads of the workgroup looped on the host
struct HostBackend {
    lbp::Record r;
    int k;
    void reduce(const double *hp, double *sum) {
        double part[lbp::THREADS][lbp::NSUM];
        for (int t = 0; t < lbp::THREADS; ++t) {
            for (int c = 0; c < lbp::NSUM; ++c) part[t][c] = 0.0;
            for (int64_t i = t; i < r.n; i += lbp::THREADS) lbp::proxy_row(r, i, k, hp, part[t]);
        }
        lbp::reduce_threads_host(part, sum);
    }
};

struct HostHistory {
    std::vector<double> buf;
    lbp::History h;
    HostHistory() : buf((size_t)lbp::HISTORY * (2 * lbp::N + 2)) {
        h.dirs = (double (*)[lbp::N])buf.data();
        h.stps = (double (*)[lbp::N])(buf.data() + lbp::HISTORY * lbp::N);
        h.ro = buf.data() + 2 * lbp::HISTORY * lbp::N;
        h.al = h.ro + lbp::HISTORY;
    }
};

int check_spec(const int32_t *spec, int S, int kmax) {
    for (int s = 0; s < S; ++s) {
        const int32_t *sp = spec + 3 * (size_t)s;
        LEMON_REQUIRE(sp[0] >= 1 && sp[0] <= kmax, "spec: 1 <= k <= kmax");
        LEMON_REQUIRE((sp[1] & ~63) == 0 && (sp[2] & ~63) == 0, "spec: the force masks have six bits");
    }
    return LEMON_OK;
}

}  // namespace

#define LBP_RECORD_NONNULL (d1 && D_n && dists_tr_n && dists_n && D_m && dists_tr_m && dists_m && y)
#define LBP_SHAPE_OK (n > 0 && n <= (int64_t)1 << 40 && kmax >= 1 && S >= 0 && S <= 65535 && outer_steps >= 1 && outer_steps <= lbp::MAX_OUTER)
#define LBP_SHAPE_MSG "n > 0, kmax >= 1, 0 <= S <= 65535, 1 <= outer_steps <= 20"

extern "C" int lemon_lbfgs_polish(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                  const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y, int64_t n,
                                  int kmax, int S, const double *x0, const int32_t *spec, int outer_steps, LemonPolishResult *out,
                                  void *stream_) {
    LEMON_REQUIRE(LBP_SHAPE_OK, LBP_SHAPE_MSG);
    LEMON_REQUIRE(LBP_RECORD_NONNULL && x0 && spec && out, "null pointer");
    if (S == 0) return LEMON_OK;
    hipStream_t stream = (hipStream_t)stream_;
    // the kernel indexes the record with k: checked here, before anything is launched
    std::vector<int32_t> spec_h((size_t)3 * S);
    LEMON_HIP_CHECK(hipMemcpyAsync(spec_h.data(), spec, spec_h.size() * 4, hipMemcpyDeviceToHost, stream));
    LEMON_HIP_CHECK(hipStreamSynchronize(stream));
    if (int rc = check_spec(spec_h.data(), S, kmax)) return rc;
    PolishArgs a;
    a.r = lbp::Record{d1, D_n, dists_tr_n, dists_n, D_m, dists_tr_m, dists_m, y, n, kmax};
    a.x0 = x0; a.spec = spec; a.outer_steps = outer_steps;
    a.out = (lbp::Result *)out;
    hipLaunchKernelGGL(k_lbfgs_polish, dim3((unsigned)S), dim3(lbp::THREADS), 0, stream, a);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

extern "C" int lemon_lbfgs_polish_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                       const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                                       int64_t n, int kmax, int S, const double *x0, const int32_t *spec, int outer_steps,
                                       LemonPolishResult *out) {
    LEMON_REQUIRE(LBP_SHAPE_OK, LBP_SHAPE_MSG);
    LEMON_REQUIRE(LBP_RECORD_NONNULL && x0 && spec && out, "null pointer");
    if (int rc = check_spec(spec, S, kmax)) return rc;
    const lbp::Record r{d1, D_n, dists_tr_n, dists_n, D_m, dists_tr_m, dists_m, y, n, kmax};
    HostHistory hist;
    for (int s = 0; s < S; ++s) {
        const int32_t *sp = spec + 3 * (size_t)s;
        HostBackend b{r, sp[0]};
        lbp::Proxy<HostBackend> f{b, (uint32_t)sp[1], (uint32_t)sp[2], n};
        lbp::polish(f, x0 + lbp::N * (size_t)s, outer_steps, hist.h, *(lbp::Result *)(out + s));
    }
    return LEMON_OK;
}

extern "C" double lemon_lbfgs_proxy_host(const float *d1, const float *D_n, const float *dists_tr_n, const float *dists_n,
                                         const float *D_m, const float *dists_tr_m, const float *dists_m, const uint8_t *y,
                                         int64_t n, int kmax, int k, int force_zero, int force_one, const double *x, double *grad) {
    if (!(LBP_RECORD_NONNULL && x && grad && n > 0 && k >= 1 && k <= kmax && (force_zero & ~63) == 0 && (force_one & ~63) == 0)) {
        lemon_set_error("invalid argument: null pointer, n > 0, 1 <= k <= kmax, six-bit force masks");
        return NAN;
    }
    const lbp::Record r{d1, D_n, dists_tr_n, dists_n, D_m, dists_tr_m, dists_m, y, n, kmax};
    HostBackend b{r, k};
    lbp::Proxy<HostBackend> f{b, (uint32_t)force_zero, (uint32_t)force_one, n};
    double loss;
    f(x, loss, grad);
    return loss;
}

// the restated exp (fn 0) / log1p (fn 1) of the header on count host values, for the tests (against libm)
extern "C" int lemon_lbfgs_math_host(int fn, const double *x, int64_t count, double *out) {
    LEMON_REQUIRE((fn == 0 || fn == 1) && count >= 0 && (count == 0 || (x && out)), "fn is 0 (exp) or 1 (log1p), count >= 0, no null pointer");
    for (int64_t i = 0; i < count; ++i) out[i] = fn == 0 ? lbp::exp_r(x[i]) : lbp::log1p_r(x[i]);
    return LEMON_OK;
}
