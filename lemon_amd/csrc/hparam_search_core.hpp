// The local searches of the hyper-parameter search (lib/metrics/utils.py:151-158), restated from scipy 1.15
// optimize/_optimize.py so that a whole search runs without the interpreter: _minimize_neldermead and _minimize_powell (with
// _linesearch_powell, bracket, _recover_from_bracket_error and Brent.optimize) as minimize(..., options={}) runs them, and
// _minimize_scalar_bounded, the threshold search inside the objective.  Plain C++ for host and device: IEEE double
// throughout, one rounding per Python operation (no FMA contraction in any function of this file), the comparisons of the
// source including their < / <= choices.  The dimension is fixed at N = 6.
//
// Where scipy raises _MaxFuncCallError a call returns false and the callers unwind as the except clauses do.  lemon_grid_f1
// and lemon_grid_f1_ks run fminbound() through gridf1_brent.hpp; lemon_hparam_search (hparam_search.hip) and its host twin
// run search().  tests/native/hparam_search_fuzz.cpp drives this file alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HPS_HD __host__ __device__ inline
#else
#define HPS_HD inline
#endif

namespace hps {

constexpr int N = 6;
constexpr int NELDER_MEAD = 0, POWELL = 1;
// status: scipy's warnflag (0 ok, 1 maxfev, 2 maxiter, 3 NaN) and, beyond scipy, 5 where bracket() raises its RuntimeError
constexpr int STATUS_BRACKET_ITER = 5;

struct Caps { int nm_maxiter, nm_maxfun, pw_maxiter, pw_maxfun; };      // N * 200 and N * 1000 in scipy
constexpr Caps DEFAULT_CAPS = {1200, 1200, 6000, 6000};

struct Result { double x[N]; double fun; int32_t nfev, nit, status, pad; };   // = LemonSearchResult

HPS_HD bool is_nan(double v) { return v != v; }
HPS_HD bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// _wrap_scalar_function_maxfun_validation: false = _MaxFuncCallError
template <class F> struct Counted {
    F &f;
    int ncalls, maxfun;
    HPS_HD bool operator()(const double *x, double &out) {
        if (ncalls >= maxfun) return false;
        ++ncalls;
        out = f(x);
        return true;
    }
};

// ---------------------------------------------------------------------------------------------- _minimize_scalar_bounded
HPS_HD double sgn1(double v) { return v < 0.0 ? -1.0 : 1.0; }   // np.sign(v) + (v == 0)

// fminbound(f, a, b, xtol=xatol, maxfun) -> x.  sqrt_eps = sqrt(2.2e-16) and golden_mean = 0.5 (3 - sqrt 5) come from the host.
template <class F1D>
HPS_HD double fminbound(F1D &f, double a, double b, double xatol, int maxfun, double sqrt_eps, double golden_mean) {
#pragma clang fp contract(off)       // the iteration must round like the interpreter: one operation at a time
    double fulc = a + golden_mean * (b - a);
    double nfc = fulc, xf = fulc;
    double rat = 0.0, e = 0.0;
    double x = xf;
    double fx = f(x);
    int num = 1;
    double fu = INFINITY;
    double ffulc = fx, fnfc = fx;
    double xm = 0.5 * (a + b);
    double tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
    double tol2 = 2.0 * tol1;
    while (fabs(xf - xm) > (tol2 - 0.5 * (b - a))) {
        int golden = 1;
        if (fabs(e) > tol1) {                            // parabolic fit
            golden = 0;
            double r = (xf - nfc) * (fx - ffulc);
            double q = (xf - fulc) * (fx - fnfc);
            double p = (xf - fulc) * q - (xf - nfc) * r;
            q = 2.0 * (q - r);
            if (q > 0.0) p = -p;
            q = fabs(q);
            r = e;
            e = rat;
            if ((fabs(p) < fabs(0.5 * q * r)) && (p > q * (a - xf)) && (p < q * (b - xf))) {
                rat = (p + 0.0) / q;
                x = xf + rat;
                if (((x - a) < tol2) || ((b - x) < tol2)) rat = tol1 * sgn1(xm - xf);
            } else {
                golden = 1;
            }
        }
        if (golden) {
            e = (xf >= xm) ? a - xf : b - xf;
            rat = golden_mean * e;
        }
        const double ar = fabs(rat);
        x = xf + sgn1(rat) * (ar > tol1 ? ar : tol1);    // np.maximum(abs(rat), tol1); neither is NaN here
        fu = f(x);
        num += 1;
        if (fu <= fx) {
            if (x >= xf) a = xf; else b = xf;
            fulc = nfc; ffulc = fnfc;
            nfc = xf; fnfc = fx;
            xf = x; fx = fu;
        } else {
            if (x < xf) a = x; else b = x;
            if ((fu <= fnfc) || (nfc == xf)) {
                fulc = nfc; ffulc = fnfc;
                nfc = x; fnfc = fu;
            } else if ((fu <= ffulc) || (fulc == xf) || (fulc == nfc)) {
                fulc = x; ffulc = fu;
            }
        }
        xm = 0.5 * (a + b);
        tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
        tol2 = 2.0 * tol1;
        if (num >= maxfun) break;
    }
    return xf;
}

// ----------------------------------------------------------------------------------------------------- the objective
// maximize_metric.objective over a backend B that holds the record of one search:
//   bool B::scores(const double hp[6], double &lo, double &hi)   fills the score row; false when a score is not finite
//   double B::neg_f1(double t)                                   -F1(y, score >= t) from integer counts
// fz / fo: bit i set = HP_NAMES[i] forced to 0.0 / 1.0 (metrics.unpack_vector: zeros first, then ones).
template <class B> struct Objective {
    B &b;
    uint32_t fz, fo;
    double sqrt_eps, golden_mean;
    HPS_HD double operator()(const double *x) {
        double hp[N];
        for (int i = 0; i < N; ++i) hp[i] = (fo >> i & 1) ? 1.0 : (fz >> i & 1) ? 0.0 : x[i];
        double lo, hi;
        if (!b.scores(hp, lo, hi)) return 0.0;           // overflowing hyper-parameters: worst objective
        struct T { B &b; HPS_HD double operator()(double t) { return b.neg_f1(t); } } f{b};
        const double thres = fminbound(f, lo, hi, 1e-8, 500, sqrt_eps, golden_mean);
        return b.neg_f1(thres);                          // optimize_f1_efficient re-evaluates at the returned threshold
    }
};

// ------------------------------------------------------------------------------------------------ _minimize_neldermead
// np.argsort of the N + 1 values and np.take of the rows.  Ties are the normal case (F1 is piecewise constant) and their
// order decides the trajectory, so the order is numpy's: on x86-64 with AVX-512 (numpy >= 1.25) np.argsort of float64 does
// NOT sort seven values by insertion, it runs an 8-lane bitonic network on (key, index) pairs, lane 7 padded with +inf, and is
// not stable.  A lane keeps its index when the key it ends up with compares equal to the key it held, else it takes the
// partner's.  This is that network, checked against np.argsort on random tie patterns (tests/test_hparam_search_host.py).
// Keys that are not finite (numpy leaves the network for NaN; +inf would tie with the pad) are sorted by stable insertion.
HPS_HD void sort_simplex(double (*sim)[N], double *fsim) {
    bool finite = true;
    for (int i = 0; i <= N; ++i) finite &= is_finite(fsim[i]);
    if (finite) {
        double k[8];
        int idx[8];
        for (int l = 0; l < 8; ++l) { k[l] = l <= N ? fsim[l] : INFINITY; idx[l] = l; }
        // (lane ^ x, lanes that keep the larger key) of the six compare-exchange stages
        const int stage_xor[6] = {1, 3, 1, 7, 2, 1};
        const int stage_max[6] = {0xAA, 0xCC, 0xAA, 0xF0, 0xCC, 0xAA};
        for (int s = 0; s < 6; ++s) {
            double k2[8];
            int i2[8];
            for (int l = 0; l < 8; ++l) {
                const int p = l ^ stage_xor[s];
                const double a = k[l], b = k[p];
                const double t = (stage_max[s] >> l & 1) ? (b > a ? b : a) : (b < a ? b : a);
                k2[l] = t;
                i2[l] = t == a ? idx[l] : idx[p];
            }
            for (int l = 0; l < 8; ++l) { k[l] = k2[l]; idx[l] = i2[l]; }
        }
        double rows[N + 1][N], vals[N + 1];
        for (int i = 0; i <= N; ++i) {
            vals[i] = fsim[i];
            for (int c = 0; c < N; ++c) rows[i][c] = sim[i][c];
        }
        for (int i = 0; i <= N; ++i) {
            const int from = idx[i] <= N ? idx[i] : N;   // finite keys sort below the pad, so idx[i] <= N
            fsim[i] = vals[from];
            for (int c = 0; c < N; ++c) sim[i][c] = rows[from][c];
        }
        return;
    }
    for (int i = 1; i <= N; ++i) {
        const double v = fsim[i];
        double row[N];
        for (int c = 0; c < N; ++c) row[c] = sim[i][c];
        int j = i;
        while (j > 0 && (v < fsim[j - 1] || (is_nan(fsim[j - 1]) && !is_nan(v)))) {
            fsim[j] = fsim[j - 1];
            for (int c = 0; c < N; ++c) sim[j][c] = sim[j - 1][c];
            --j;
        }
        fsim[j] = v;
        for (int c = 0; c < N; ++c) sim[j][c] = row[c];
    }
}

template <class F> HPS_HD void nelder_mead(F &f, const double *x0, int maxiter, int maxfun, Result &res) {
#pragma clang fp contract(off)
    const double xatol = 1e-4, fatol = 1e-4;
    Counted<F> func{f, 0, maxfun};
    double sim[N + 1][N], fsim[N + 1];
    for (int c = 0; c < N; ++c) sim[0][c] = x0[c];
    for (int k = 0; k < N; ++k) {
        for (int c = 0; c < N; ++c) sim[k + 1][c] = x0[c];
        sim[k + 1][k] = x0[k] != 0.0 ? (1.0 + 0.05) * x0[k] : 0.00025;
    }
    for (int k = 0; k <= N; ++k) fsim[k] = INFINITY;
    for (int k = 0; k <= N; ++k) {
        double v;
        if (!func(sim[k], v)) break;
        fsim[k] = v;
    }
    sort_simplex(sim, fsim);
    int iterations = 1;
    while (func.ncalls < maxfun && iterations < maxiter) {
        bool converged = false;
        do {                                             // the try block: `break` is _MaxFuncCallError (or convergence)
            bool small = true;
            for (int j = 1; j <= N; ++j) {
                for (int c = 0; c < N; ++c) small &= fabs(sim[j][c] - sim[0][c]) <= xatol;   // a NaN keeps the search going
                small &= fabs(fsim[0] - fsim[j]) <= fatol;
            }
            if (small) { converged = true; break; }
            double xbar[N], xt[N], ft;
            for (int c = 0; c < N; ++c)
                xbar[c] = (((((sim[0][c] + sim[1][c]) + sim[2][c]) + sim[3][c]) + sim[4][c]) + sim[5][c]) / 6.0;
            double xr[N], fxr;
            for (int c = 0; c < N; ++c) xr[c] = 2.0 * xbar[c] - 1.0 * sim[N][c];
            if (!func(xr, fxr)) break;
            bool doshrink = false;
            if (fxr < fsim[0]) {
                for (int c = 0; c < N; ++c) xt[c] = 3.0 * xbar[c] - 2.0 * sim[N][c];         // expansion
                if (!func(xt, ft)) break;
                if (ft < fxr) {
                    for (int c = 0; c < N; ++c) sim[N][c] = xt[c];
                    fsim[N] = ft;
                } else {
                    for (int c = 0; c < N; ++c) sim[N][c] = xr[c];
                    fsim[N] = fxr;
                }
            } else if (fxr < fsim[N - 1]) {
                for (int c = 0; c < N; ++c) sim[N][c] = xr[c];
                fsim[N] = fxr;
            } else {
                if (fxr < fsim[N]) {                                                         // contraction
                    for (int c = 0; c < N; ++c) xt[c] = 1.5 * xbar[c] - 0.5 * sim[N][c];
                    if (!func(xt, ft)) break;
                    if (ft <= fxr) {
                        for (int c = 0; c < N; ++c) sim[N][c] = xt[c];
                        fsim[N] = ft;
                    } else {
                        doshrink = true;
                    }
                } else {                                                                     // inside contraction
                    for (int c = 0; c < N; ++c) xt[c] = 0.5 * xbar[c] + 0.5 * sim[N][c];
                    if (!func(xt, ft)) break;
                    if (ft < fsim[N]) {
                        for (int c = 0; c < N; ++c) sim[N][c] = xt[c];
                        fsim[N] = ft;
                    } else {
                        doshrink = true;
                    }
                }
                if (doshrink) {
                    bool over = false;
                    for (int j = 1; j <= N && !over; ++j) {
                        for (int c = 0; c < N; ++c) sim[j][c] = sim[0][c] + 0.5 * (sim[j][c] - sim[0][c]);
                        if (!func(sim[j], ft)) over = true; else fsim[j] = ft;               // the row stays moved
                    }
                    if (over) break;
                }
            }
            iterations += 1;
        } while (0);
        sort_simplex(sim, fsim);                         // the finally clause
        if (converged) break;
    }
    for (int c = 0; c < N; ++c) res.x[c] = sim[0][c];
    double m = fsim[0];                                  // np.min: a NaN wins
    for (int j = 1; j <= N && !is_nan(m); ++j)
        if (fsim[j] < m || is_nan(fsim[j])) m = fsim[j];
    res.fun = m;
    res.nfev = func.ncalls;
    res.nit = iterations;
    res.status = func.ncalls >= maxfun ? 1 : iterations >= maxiter ? 2 : 0;
    res.pad = 0;
}

// ---------------------------------------------------------------------------------------------------- _minimize_powell
enum Flow { FLOW_OK = 0, FLOW_MAXFUN = 1, FLOW_BRACKET_ITER = 2 };

// func(p + alpha * xi)
template <class F> struct Line {
    Counted<F> &func;
    const double *p, *xi;
    HPS_HD bool operator()(double alpha, double &out) {
#pragma clang fp contract(off)
        double x[N];
        for (int c = 0; c < N; ++c) x[c] = p[c] + alpha * xi[c];
        return func(x, out);
    }
};

struct Bracket { double xa, xb, xc, fa, fb, fc; bool valid; };

// bracket(func) with xa = 0, xb = 1, grow_limit = 110, maxiter = 1000
template <class L> HPS_HD Flow bracket(L &f, Bracket &o) {
#pragma clang fp contract(off)
    const double gold = 1.618034, verysmall = 1e-21, grow_limit = 110.0;
    const int maxiter = 1000;
    double xa = 0.0, xb = 1.0, fa, fb, fc, fw;
    if (!f(xa, fa)) return FLOW_MAXFUN;
    if (!f(xb, fb)) return FLOW_MAXFUN;
    if (fa < fb) {
        double t = xa; xa = xb; xb = t;
        t = fa; fa = fb; fb = t;
    }
    double xc = xb + gold * (xb - xa);
    if (!f(xc, fc)) return FLOW_MAXFUN;
    int iter = 0;
    while (fc < fb) {
        const double tmp1 = (xb - xa) * (fb - fc);
        const double tmp2 = (xb - xc) * (fb - fa);
        const double val = tmp2 - tmp1;
        const double denom = fabs(val) < verysmall ? 2.0 * verysmall : 2.0 * val;
        double w = xb - ((xb - xc) * tmp2 - (xb - xa) * tmp1) / denom;
        const double wlim = xb + grow_limit * (xc - xb);
        if (iter > maxiter) return FLOW_BRACKET_ITER;
        iter += 1;
        if ((w - xc) * (xb - w) > 0.0) {
            if (!f(w, fw)) return FLOW_MAXFUN;
            if (fw < fc) {
                xa = xb; xb = w; fa = fb; fb = fw;
                break;
            } else if (fw > fb) {
                xc = w; fc = fw;
                break;
            }
            w = xc + gold * (xc - xb);
            if (!f(w, fw)) return FLOW_MAXFUN;
        } else if ((w - wlim) * (wlim - xc) >= 0.0) {
            w = wlim;
            if (!f(w, fw)) return FLOW_MAXFUN;
        } else if ((w - wlim) * (xc - w) > 0.0) {
            if (!f(w, fw)) return FLOW_MAXFUN;
            if (fw < fc) {
                xb = xc; xc = w;
                w = xc + gold * (xc - xb);
                fb = fc; fc = fw;
                if (!f(w, fw)) return FLOW_MAXFUN;
            }
        } else {
            w = xc + gold * (xc - xb);
            if (!f(w, fw)) return FLOW_MAXFUN;
        }
        xa = xb; xb = xc; xc = w;
        fa = fb; fb = fc; fc = fw;
    }
    const bool cond1 = (fb < fc && fb <= fa) || (fb < fa && fb <= fc);
    const bool cond2 = (xa < xb && xb < xc) || (xc < xb && xb < xa);
    const bool cond3 = is_finite(xa) && is_finite(xb) && is_finite(xc);
    o.xa = xa; o.xb = xb; o.xc = xc; o.fa = fa; o.fb = fb; o.fc = fc;
    o.valid = cond1 && cond2 && cond3;
    return FLOW_OK;
}

// _recover_from_bracket_error(_minimize_scalar_brent, f, None, (), xtol=tol) -> (x, fun)
template <class L> HPS_HD Flow brent_line(L &f, double tol, double &xmin, double &fmin) {
#pragma clang fp contract(off)
    const double mintol = 1.0e-11, cg = 0.3819660;
    const int maxiter = 500;
    Bracket br;
    const Flow fl = bracket(f, br);
    if (fl != FLOW_OK) return fl;
    if (!br.valid) {                                     // BracketError: the best of the three points
        if (is_nan(br.xa) || is_nan(br.xb) || is_nan(br.xc) || is_nan(br.fa) || is_nan(br.fb) || is_nan(br.fc)) {
            xmin = fmin = NAN;
            return FLOW_OK;
        }
        xmin = br.xa; fmin = br.fa;                      // np.argmin: the first of equal values
        if (br.fb < fmin) { xmin = br.xb; fmin = br.fb; }
        if (br.fc < fmin) { xmin = br.xc; fmin = br.fc; }
        return FLOW_OK;
    }
    // Brent.optimize
    double x = br.xb, w = br.xb, v = br.xb;
    double fx = br.fb, fw = br.fb, fv = br.fb;
    double a, b;
    if (br.xa < br.xc) { a = br.xa; b = br.xc; } else { a = br.xc; b = br.xa; }
    double deltax = 0.0, rat = 0.0, u, fu;
    int iter = 0;
    while (iter < maxiter) {
        const double tol1 = tol * fabs(x) + mintol;
        const double tol2 = 2.0 * tol1;
        const double xmid = 0.5 * (a + b);
        if (fabs(x - xmid) < (tol2 - 0.5 * (b - a))) break;
        if (fabs(deltax) <= tol1) {
            deltax = (x >= xmid) ? a - x : b - x;        // golden section step
            rat = cg * deltax;
        } else {                                         // parabolic step
            const double tmp1 = (x - w) * (fx - fv);
            double tmp2 = (x - v) * (fx - fw);
            double p = (x - v) * tmp2 - (x - w) * tmp1;
            tmp2 = 2.0 * (tmp2 - tmp1);
            if (tmp2 > 0.0) p = -p;
            tmp2 = fabs(tmp2);
            const double dx_temp = deltax;
            deltax = rat;
            if ((p > tmp2 * (a - x)) && (p < tmp2 * (b - x)) && (fabs(p) < fabs(0.5 * tmp2 * dx_temp))) {
                rat = p * 1.0 / tmp2;
                u = x + rat;
                if ((u - a) < tol2 || (b - u) < tol2) rat = (xmid - x >= 0) ? tol1 : -tol1;
            } else {
                deltax = (x >= xmid) ? a - x : b - x;
                rat = cg * deltax;
            }
        }
        if (fabs(rat) < tol1) u = (rat >= 0) ? x + tol1 : x - tol1;
        else u = x + rat;
        if (!f(u, fu)) return FLOW_MAXFUN;
        if (fu > fx) {
            if (u < x) a = u; else b = u;
            if ((fu <= fw) || (w == x)) {
                v = w; w = u; fv = fw; fw = fu;
            } else if ((fu <= fv) || (v == x) || (v == w)) {
                v = u; fv = fu;
            }
        } else {
            if (u >= x) a = x; else b = x;
            v = w; w = x; x = u;
            fv = fw; fw = fx; fx = fu;
        }
        iter += 1;
    }
    xmin = x; fmin = fx;
    return FLOW_OK;
}

// _linesearch_powell without bounds: (fval, p, xi) -> (fret, p + alpha xi, alpha xi), in place
template <class F> HPS_HD Flow linesearch_powell(Counted<F> &func, double *p, double *xi, double tol, double &fval) {
#pragma clang fp contract(off)
    bool any = false;
    for (int c = 0; c < N; ++c) any |= xi[c] != 0.0;
    if (!any) return FLOW_OK;                            // xi is zero: fval is reused
    Line<F> line{func, p, xi};
    double alpha, fret;
    const Flow fl = brent_line(line, tol, alpha, fret);
    if (fl != FLOW_OK) return fl;
    for (int c = 0; c < N; ++c) {
        xi[c] = alpha * xi[c];
        p[c] = p[c] + xi[c];
    }
    fval = fret;
    return FLOW_OK;
}

template <class F> HPS_HD void powell(F &f, const double *x0, int maxiter, int maxfun, Result &res) {
#pragma clang fp contract(off)
    const double xtol = 1e-4, ftol = 1e-4;
    const double tol = xtol * 100;
    Counted<F> func{f, 0, maxfun};
    double direc[N][N], x[N], x1[N], x2[N], direc1[N];
    for (int i = 0; i < N; ++i)
        for (int c = 0; c < N; ++c) direc[i][c] = i == c ? 1.0 : 0.0;
    for (int c = 0; c < N; ++c) x[c] = x1[c] = x0[c];
    double fval = 0.0;
    func(x, fval);
    int iter = 0;
    Flow fl = FLOW_OK;
    while (true) {
        const double fx = fval;
        int bigind = 0;
        double delta = 0.0, fx2;
        for (int i = 0; i < N; ++i) {
            for (int c = 0; c < N; ++c) direc1[c] = direc[i][c];
            fx2 = fval;
            fl = linesearch_powell(func, x, direc1, tol, fval);
            if (fl != FLOW_OK) break;
            if ((fx2 - fval) > delta) {
                delta = fx2 - fval;
                bigind = i;
            }
        }
        if (fl != FLOW_OK) break;
        iter += 1;
        const double bnd = ftol * (fabs(fx) + fabs(fval)) + 1e-20;
        if (2.0 * (fx - fval) <= bnd) break;
        if (func.ncalls >= maxfun) break;
        if (iter >= maxiter) break;
        if (is_nan(fx) && is_nan(fval)) break;
        for (int c = 0; c < N; ++c) {                    // the extrapolated point
            direc1[c] = x[c] - x1[c];
            x1[c] = x[c];
            x2[c] = x[c] + 1.0 * direc1[c];
        }
        if (!func(x2, fx2)) break;
        if (fx > fx2) {
            double t = 2.0 * (fx + fx2 - 2.0 * fval);
            double temp = fx - fval - delta;
            t *= temp * temp;
            temp = fx - fx2;
            t -= delta * temp * temp;
            if (t < 0.0) {
                fl = linesearch_powell(func, x, direc1, tol, fval);
                if (fl != FLOW_OK) break;
                bool any = false;
                for (int c = 0; c < N; ++c) any |= direc1[c] != 0.0;
                if (any)
                    for (int c = 0; c < N; ++c) {
                        direc[bigind][c] = direc[N - 1][c];
                        direc[N - 1][c] = direc1[c];
                    }
            }
        }
    }
    bool xnan = false;
    for (int c = 0; c < N; ++c) {
        res.x[c] = x[c];
        xnan |= is_nan(x[c]);
    }
    res.fun = fval;
    res.nfev = func.ncalls;
    res.nit = iter;
    res.status = fl == FLOW_BRACKET_ITER ? STATUS_BRACKET_ITER
                 : func.ncalls >= maxfun ? 1 : iter >= maxiter ? 2 : (is_nan(fval) || xnan) ? 3 : 0;
    res.pad = 0;
}

template <class F> HPS_HD void search(F &f, int method, const double *x0, const Caps &caps, Result &res) {
    if (method == POWELL) powell(f, x0, caps.pw_maxiter, caps.pw_maxfun, res);
    else nelder_mead(f, x0, caps.nm_maxiter, caps.nm_maxfun, res);
}

}  // namespace hps
