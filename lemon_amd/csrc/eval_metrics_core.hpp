// metrics.eval_metrics (lib/metrics/utils.py:273-441) restated so that all splits of a run are served without the interpreter:
// optimize_f1 (:273-284), f1_with_pred_prev_constraint and its fminbound fall-back (:298-322), f1_with_local_minima_finder
// (:327-349), the counts behind binary_metrics (:351-405) and the two curve areas of prob_metrics (:408-412).  Plain C++ for
// host and device: IEEE double, one rounding per written operation (no FMA contraction in any function of this file; the fma()
// calls of lbp::exp_r / lbp::log1p_r are written out), the comparisons of the sources including their < / <= choices.
//
// Everything is a function of ONE descending sort of a segment's (score, label) pairs -- Sorted: the scores and the inclusive
// prefix counts of positives -- beside the segment in its original order for the two sums that numpy / scipy take in that order:
//   * count(score >= t) and tp(t) are a binary search and one prefix lookup; a count always lands on the edge of a group of
//     equal scores, so the order of tied rows inside the sort never reaches a result;
//   * np.linspace(lo, hi, num): step = (hi - lo) / (num - 1), c_i = i * step + lo, c_{num-1} = hi; where step == 0 numpy
//     takes (i / (num - 1)) * (hi - lo) + lo;
//   * scipy.optimize.bisect is scipy's C routine (xtol 2e-12, rtol 4 eps, 100 iterations): f(xa) == 0 or f(xb) == 0 returns
//     that end, equal signs are its ValueError (-> false), each iteration dm *= .5; xm = xa + dm; if (fm * fa >= 0) xa = xm;
//   * np.mean(score) = np.add.reduce / n, numpy's order: consecutive chunks of NP_CHUNK = 8192 elements, each summed by the
//     pairwise rule (below 8: a loop from 0.0; up to 128: eight running sums, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
//     remainder in order; above: split at n / 2 rounded down to a multiple of 8), the chunk sums accumulated left to right;
//   * the KDE of gaussian_kde(score).evaluate: Scott factor n^(-1/5) = exp_r(-0.2 log1p_r(n - 1)), h = sqrt(var factor^2) with
//     the sample variance var = SUMSQ * (1 / (n - 1)) around np.mean, density_j = sum_i (1/n) (exp_r(-(r r)/2) norm) with
//     r = s_i / h - x_j / h and norm = (2 pi)^(-1/2) / h, i in the segment's ORIGINAL order from 0 (scipy's own order), one
//     grid point a lane;
//   * SUMSQ and the AUPRC terms are summed in the order of a workgroup of THREADS lanes: lane t owns the rows t, t + THREADS,
//     ... in index order (SUMSQ: rows of the original order; AUPRC: rows of the sorted order, a row that ends a group carries
//     the group's term), then the 64-lane xor butterfly of every wave (offsets 32, 16, .. 1), then the waves in index order
//     from wave 0.  LaneSums / reduce_lanes replay that on the host;
//   * AUROC is exact: over groups of equal scores (==, so -0.0 and +0.0 are one group) 2U' = sum_g pos_g (2 neg_above_g +
//     neg_g) in int64, 2U = 2 P N - 2U', AUROC = (double)2U / (2.0 P N);
//   * AUPRC = sum_g (pos_g / P) (tp_g / (tp_g + fp_g)) over the groups in descending score.
// A segment that cannot be served gets a status, never an exception; the first that applies in the order the host path
// raises: a non-finite score, then for a free segment fewer than two rows and zero variance (gaussian_kde), then one class.
// lemon_eval_metrics (eval_metrics.hip) and its host twin run this file; tests/native/eval_metrics_fuzz.cpp drives it alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hparam_search_core.hpp"
#include "lbfgs_core.hpp"

#if defined(__HIPCC__)
#define EVM_HD __host__ __device__ inline
#else
#define EVM_HD inline
#endif

namespace evm {

constexpr int THREADS = 1024, WAVES = THREADS / 64;   // the workgroup whose summation order LaneSums replays
constexpr int N_CAND = 100, N_GRID = 1000;            // optimize_f1's candidates, the KDE's grid points
constexpr int64_t NP_CHUNK = 8192;                    // numpy's reduction buffer, in elements
constexpr int ST_OK = 0, ST_NONFINITE = 1, ST_ONE_CLASS = 2, ST_FEW_ROWS = 3, ST_ZERO_VAR = 4, ST_SOURCE = 5;
constexpr int KDE_MINIMA = 1, KDE_ONE_MINIMUM = 2, KDE_MAXIMA = 3, KDE_MEAN = 4;     // Record::kde_branch (0: not taken)

struct Segment { int64_t offset, n; double prevalence; int32_t thres_from, pad; };   // = LemonEvalSegment
struct Record {                                                                      // = LemonEvalRecord
    double auroc, auprc, thres[3];       // thres: F1_optimal, F1_prev, F1_heuristic
    int64_t counts[3][4];                // (TP, FP, FN, TN) at each of the three
    int32_t status, kde_branch, bisect_fallback, pad;
};

// a segment sorted by descending score: cp[i] = positives among s[0 .. i]
struct Sorted { const double *s; const int32_t *cp; int64_t n; };

EVM_HD bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
EVM_HD bool sign_bit(double v) { return (lbp::to_bits(v) >> 63) != 0; }

// (score >= t).sum(): the first index whose score is below t
EVM_HD int64_t count_ge(const Sorted &v, double t) {
    int64_t lo = 0, hi = v.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v.s[mid] >= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}
EVM_HD int64_t tp_at(const Sorted &v, int64_t cnt) { return cnt > 0 ? (int64_t)v.cp[cnt - 1] : 0; }
EVM_HD int64_t positives(const Sorted &v) { return tp_at(v, v.n); }

// f1_binary from counts: 2 tp / (2 tp + fp + fn), 0 when there is nothing to count
EVM_HD double f1_counts(int64_t tp, int64_t cnt, int64_t pos) {
#pragma clang fp contract(off)
    const int64_t denom = 2 * tp + (cnt - tp) + (pos - tp);
    return denom ? 2.0 * (double)tp / (double)denom : 0.0;
}

EVM_HD double linspace_at(double lo, double hi, int num, int i) {
#pragma clang fp contract(off)
    if (i == num - 1) return hi;
    const double div = (double)(num - 1), delta = hi - lo, step = delta / div;
    if (step == 0.0) return ((double)i / div) * delta + lo;
    return (double)i * step + lo;
}

// ---------------------------------------------------------------------------------------------------------- optimize_f1
EVM_HD double candidate_f1(const Sorted &v, int i) {
    const int64_t cnt = count_ge(v, linspace_at(v.s[v.n - 1], v.s[0], N_CAND, i));
    return f1_counts(tp_at(v, cnt), cnt, positives(v));
}
// the loop's `if f1 >= best_f1` with best_f1 = 0 in front: the LAST candidate that reaches the maximum
EVM_HD int pick_candidate(const double *f1) {
    double best = 0.0;
    int at = 0;
    for (int i = 0; i < N_CAND; ++i)
        if (f1[i] >= best) { best = f1[i]; at = i; }
    return at;
}

// -------------------------------------------------------------------------------------------- scipy.optimize.bisect (C)
template <class F> EVM_HD bool bisect(F &f, double xa, double xb, double &root) {
#pragma clang fp contract(off)
    const double xtol = 2e-12, rtol = 8.881784197001252e-16;
    const double fa = f(xa), fb = f(xb);
    if (fa == 0.0) { root = xa; return true; }
    if (fb == 0.0) { root = xb; return true; }
    if (sign_bit(fa) == sign_bit(fb)) return false;      // SIGNERR: the wrapper's ValueError
    double dm = xb - xa, xm = xa;
    for (int i = 0; i < 100; ++i) {
        dm *= .5;
        xm = xa + dm;
        const double fm = f(xm);
        if (fm * fa >= 0.0) xa = xm;
        if (fm == 0.0 || fabs(dm) < xtol + rtol * fabs(xm)) { root = xm; return true; }
    }
    root = xa;                                           // CONVERR: unreachable for finite scores below 2e18 in range
    return true;
}

// f1_with_pred_prev_constraint -> its threshold; fallback = 1 where f1_with_pred_prev_constraint2 served it
EVM_HD double prev_threshold(const Sorted &v, double prevalence, double sqrt_eps, double golden_mean, int &fallback) {
#pragma clang fp contract(off)
    struct Gap {
        const Sorted &v; double prev;
        EVM_HD double operator()(double t) { return (double)count_ge(v, t) / (double)v.n - prev; }
    } gap{v, prevalence};
    const double lo = v.s[v.n - 1], hi = v.s[0];
    double root = 0.0;
    fallback = 0;
    if (bisect(gap, lo, hi, root) && root == root) return root;
    fallback = 1;
    struct Gap2 {
        Gap &g;
        EVM_HD double operator()(double t) { const double d = g(t); return d * d; }
    } gap2{gap};
    return hps::fminbound(gap2, lo, hi, 1e-5, 500, sqrt_eps, golden_mean);
}

// ----------------------------------------------------------------------------------------------- np.sum / np.mean's order
EVM_HD double pairwise_leaf(const double *a, int64_t n) {      // n <= 128
#pragma clang fp contract(off)
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
// numpy's pairwise sum of one reduction chunk: n <= NP_CHUNK (seven levels; the stack would hold 128 * 2^15 elements)
EVM_HD double pairwise_sum(const double *a, int64_t n) {
#pragma clang fp contract(off)
    int64_t off[16], len[16];
    int phase[16];
    double left[16];
    int sp = 0;
    double ret = 0.0;
    off[0] = 0; len[0] = n; phase[0] = 0;
    while (sp >= 0) {
        if (phase[sp] == 0) {
            if (len[sp] <= 128) { ret = pairwise_leaf(a + off[sp], len[sp]); --sp; continue; }
            int64_t n2 = len[sp] / 2;
            n2 -= n2 % 8;
            phase[sp] = 1;
            off[sp + 1] = off[sp]; len[sp + 1] = n2; phase[sp + 1] = 0;
            ++sp;
        } else if (phase[sp] == 1) {
            int64_t n2 = len[sp] / 2;
            n2 -= n2 % 8;
            left[sp] = ret;
            phase[sp] = 2;
            off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; phase[sp + 1] = 0;
            ++sp;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}
EVM_HD int64_t np_chunks(int64_t n) { return (n + NP_CHUNK - 1) / NP_CHUNK; }
EVM_HD double np_chunk_sum(const double *a, int64_t n, int64_t c) {
    const int64_t lo = c * NP_CHUNK;
    return pairwise_sum(a + lo, n - lo < NP_CHUNK ? n - lo : NP_CHUNK);
}
EVM_HD double np_mean(const double *a, int64_t n) {            // the sequential form: host twin and fuzz program
#pragma clang fp contract(off)
    double tot = 0.0;
    for (int64_t c = 0; c < np_chunks(n); ++c) tot += np_chunk_sum(a, n, c);
    return tot / (double)n;
}

// --------------------------------------------------------------------------------------- the workgroup's summation order
// wave_total[w] after the butterfly of wave w's 64 lane sums; the total from wave 0 on
EVM_HD double reduce_waves(const double *wave_total) {
#pragma clang fp contract(off)
    double tot = wave_total[0];
    for (int w = 1; w < WAVES; ++w) tot += wave_total[w];
    return tot;
}
// the lanes looped on the host (host code only): add(i, term) in index order, total() = the butterflies, then the waves
struct LaneSums {
    double lane[THREADS];
    LaneSums() { for (int t = 0; t < THREADS; ++t) lane[t] = 0.0; }
    void add(int64_t i, double term) { lane[i % THREADS] += term; }
    double total() {
        double wt[WAVES];
        for (int w = 0; w < WAVES; ++w) {
            double v[64], u[64];
            for (int l = 0; l < 64; ++l) v[l] = lane[64 * w + l];
            for (int off = 32; off > 0; off >>= 1) {
                for (int l = 0; l < 64; ++l) u[l] = v[l] + v[l ^ off];
                for (int l = 0; l < 64; ++l) v[l] = u[l];
            }
            wt[w] = v[0];
        }
        return reduce_waves(wt);
    }
};

// ------------------------------------------------------------------------------------------------ curve terms of a row
// Row i of the sorted segment ends a group when it is the last row or s[i] != s[i + 1].  With prev_end = (rows, positives)
// at the end of the group before (0, 0 in front of the first): the group's AUPRC term and its share of 2U'.
EVM_HD double auprc_term(int64_t rows, int64_t tp, int64_t prev_tp, int64_t pos) {
#pragma clang fp contract(off)
    return ((double)(tp - prev_tp) / (double)pos) * ((double)tp / (double)rows);
}
EVM_HD int64_t auroc_term(int64_t rows, int64_t tp, int64_t prev_rows, int64_t prev_tp) {
    const int64_t pos_g = tp - prev_tp, neg_above = prev_rows - prev_tp, neg_g = (rows - tp) - neg_above;
    return pos_g * (2 * neg_above + neg_g);
}
EVM_HD double auroc_from(int64_t u2_above, int64_t pos, int64_t n) {
#pragma clang fp contract(off)
    const int64_t neg = n - pos;
    return (double)(2 * pos * neg - u2_above) / (2.0 * (double)pos * (double)neg);
}

// ------------------------------------------------------------------------------------------------------------- the KDE
struct Kde { double lo, hi, mean, h, norm, w; };         // grid ends, np.mean, bandwidth, (2 pi)^(-1/2) / h, 1 / n

EVM_HD double sq_dev(double s, double mean) {
#pragma clang fp contract(off)
    const double d = s - mean;
    return d * d;
}
// false: the covariance is zero where scipy's Cholesky raises (or not positive / not finite, where it raises as well)
EVM_HD bool kde_setup(double lo, double hi, double mean, double sumsq, int64_t n, Kde &k) {
#pragma clang fp contract(off)
    const double var = sumsq * (1.0 / (double)(n - 1));
    const double factor = lbp::exp_r(-0.2 * lbp::log1p_r((double)(n - 1)));
    const double cov = var * (factor * factor);
    k.lo = lo; k.hi = hi; k.mean = mean;
    k.h = sqrt(cov);
    k.norm = 0.3989422804014327 / k.h;
    k.w = 1.0 / (double)n;
    return cov > 0.0 && is_finite(cov) && k.h > 0.0;
}
EVM_HD double kde_point(const Kde &k, int j) {
#pragma clang fp contract(off)
    return linspace_at(k.lo, k.hi, N_GRID, j) / k.h;
}
// one row's share of one grid point: u = s_i / h, xj = kde_point
EVM_HD double kde_term(const Kde &k, double u, double xj) {
#pragma clang fp contract(off)
    const double r = u - xj;
    return k.w * (lbp::exp_r(-(r * r) / 2.0) * k.norm);
}
// argrelextrema(dens, less / greater, order 1, mode clip) on the grid, then the median rule of f1_with_local_minima_finder
EVM_HD double kde_threshold(const Kde &k, const double *dens, int &branch) {
#pragma clang fp contract(off)
    int n_min = 0, n_max = 0;
    for (int j = 1; j + 1 < N_GRID; ++j) {
        n_min += dens[j] < dens[j - 1] && dens[j] < dens[j + 1];
        n_max += dens[j] > dens[j - 1] && dens[j] > dens[j + 1];
    }
    const bool minima = n_min > 0;
    const int m = minima ? n_min : n_max;
    if (!minima && n_max < 2) { branch = KDE_MEAN; return k.mean; }
    branch = !minima ? KDE_MAXIMA : n_min > 1 ? KDE_MINIMA : KDE_ONE_MINIMUM;
    // np.median of m ascending grid points: the middle one, or the mean of the middle two
    const int want_hi = m / 2, want_lo = (m & 1) ? m / 2 : m / 2 - 1;
    double a = 0.0, b = 0.0;
    int seen = 0;
    for (int j = 1; j + 1 < N_GRID; ++j) {
        const bool hit = minima ? (dens[j] < dens[j - 1] && dens[j] < dens[j + 1]) : (dens[j] > dens[j - 1] && dens[j] > dens[j + 1]);
        if (!hit) continue;
        if (seen == want_lo) a = linspace_at(k.lo, k.hi, N_GRID, j);
        if (seen == want_hi) b = linspace_at(k.lo, k.hi, N_GRID, j);
        ++seen;
    }
    if (m == 1) return a;
    return (m & 1) ? a : (a + b) / 2.0;
}

// ---------------------------------------------------------------------------------------------------------- the counts
EVM_HD void counts_at(const Sorted &v, double t, int64_t *c) {
    const int64_t cnt = count_ge(v, t), tp = tp_at(v, cnt), pos = positives(v);
    c[0] = tp; c[1] = cnt - tp; c[2] = pos - tp; c[3] = (v.n - cnt) - (pos - tp);
}

// the status of a segment from what one pass over it finds
EVM_HD int segment_status(bool free_seg, bool nonfinite, int64_t n, int64_t pos, bool kde_ok) {
    if (nonfinite) return ST_NONFINITE;
    if (free_seg && n < 2) return ST_FEW_ROWS;
    if (free_seg && !kde_ok) return ST_ZERO_VAR;
    if (pos == 0 || pos == n) return ST_ONE_CLASS;
    return ST_OK;
}

}  // namespace evm
