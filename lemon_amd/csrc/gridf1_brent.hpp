// The bounded-Brent threshold search of the hyper-parameter grid, shared by lemon_grid_f1 (gridf1.hip) and lemon_grid_f1_ks
// (ksweep.hip): one wavefront per score row, a faithful restatement of scipy's _minimize_scalar_bounded in IEEE double (no FMA
// contraction inside the search; hps::fminbound of hparam_search_core.hpp, shared with lemon_hparam_search), F1 from integer counts.  A non-finite score row yields F1 = 0, thres = NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "hparam_search_core.hpp"

namespace {

struct F1Ctx { const double *s; const uint8_t *y; int64_t n; int64_t pos; int lane; };

// -F1(y, s >= t): sklearn's binary F1 from integer counts, 0 when nothing is counted
__device__ __forceinline__ double neg_f1(const F1Ctx &c, double t) {
#pragma clang fp contract(off)
    long long pred = 0, tp = 0;
    for (int64_t i = c.lane; i < c.n; i += 64) {
        const bool p = c.s[i] >= t;
        pred += p;
        tp += p && c.y[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { pred += __shfl_xor(pred, off); tp += __shfl_xor(tp, off); }
    const long long denom = 2 * tp + (pred - tp) + (c.pos - tp);
    return denom ? -(2.0 * (double)tp / (double)denom) : -0.0;
}

__global__ __launch_bounds__(256) void k_grid_brent(const double *__restrict__ score, const uint8_t *__restrict__ y,
                                                    int64_t n, int G, double xatol, int maxfun, double sqrt_eps,
                                                    double golden_mean, double *__restrict__ out_f1,
                                                    double *__restrict__ out_thres) {
#pragma clang fp contract(off)       // the Brent iteration must round like the interpreter: one operation at a time
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;                                  // wave-uniform
    F1Ctx c;
    c.s = score + (int64_t)g * n; c.y = y; c.n = n; c.lane = lane;
    // bounds = (min, max) of the row; positives; finiteness
    double lo = INFINITY, hi = -INFINITY;
    long long pos = 0; int bad = 0;
    for (int64_t i = lane; i < n; i += 64) {
        const double v = c.s[i];
        bad |= !(fabs(v) <= 1.7976931348623157e308);
        lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        pos += y[i] != 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
        pos += __shfl_xor(pos, off); bad |= __shfl_xor(bad, off);
    }
    c.pos = pos;
    if (bad) { if (lane == 0) { out_f1[g] = 0.0; out_thres[g] = __builtin_nan(""); } return; }

    // scipy.optimize._optimize._minimize_scalar_bounded (scipy 1.15), every wave-uniform value in double
    struct NegF1 { const F1Ctx &c; __device__ double operator()(double t) { return neg_f1(c, t); } } f{c};
    const double xf = hps::fminbound(f, lo, hi, xatol, maxfun, sqrt_eps, golden_mean);
    const double best = -neg_f1(c, xf);                  // optimize_f1_efficient re-evaluates at the returned x
    if (lane == 0) { out_f1[g] = best; out_thres[g] = xf; }
}

}  // namespace
