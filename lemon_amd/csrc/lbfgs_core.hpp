// The LBFGS polish of the hyper-parameter search (lib/metrics/utils.py:121-149), restated so that a whole polish runs without
// the interpreter and without autograd:
//   * the SoftMargin proxy, value and gradient in one pass over the record, float64 on the float32 record;
//   * exp and log1p restated with explicit fma(), so that the host and the device round alike (ocml's and glibc's differ in the
//     last place, which is enough to separate two LBFGS trajectories on this flat landscape);
//   * one reduction order for both backends: thread t owns the rows t, t + THREADS, ..., then a 64-lane xor butterfly, then the
//     waves in index order (ThreadSums is what a backend reduces);
//   * torch.optim.LBFGS (torch 2.10, optim/lbfgs.py) as torch_minimize drives it: lr 0.1, max_iter 20, max_eval 25,
//     tolerance_grad 1e-7, tolerance_change 1e-9, history_size 100, strong_wolfe with c1 1e-4, c2 0.9; _cubic_interpolate and
//     both phases of _strong_wolfe, the two-loop recursion, the state that persists over the outer step() calls.
// Plain C++ for host and device: IEEE double, one rounding per written operation (no FMA contraction anywhere in this file; the
// fma() calls of exp_r / log1p_r are written out), the comparisons of the source including their < / <= choices and what
// Python's min / max do with a NaN.  Every loop is bounded by torch's own counters, so a NaN flows through to the result.
// lemon_lbfgs_polish (lbfgs_polish.hip) and its host twin run polish(); tests/native/lbfgs_fuzz.cpp drives this file alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LBP_HD __host__ __device__ inline
#else
#define LBP_HD inline
#endif

namespace lbp {

constexpr int N = 6;
constexpr int THREADS = 256, WAVES = THREADS / 64;   // the workgroup of a polish; the host twin replays its reduction order
constexpr int HISTORY = 100, MAX_ITER = 20, MAX_EVAL = 25;
constexpr int MAX_OUTER = 20;                        // torch_minimize calls optimizer.step 20 times
constexpr double LR = 0.1, TOL_GRAD = 1e-7, TOL_CHANGE = 1e-9, C1 = 1e-4, C2 = 0.9;

struct Result { double x[N]; double loss; int32_t nfev, nit, status, pad; };   // = LemonPolishResult

LBP_HD bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
LBP_HD double from_bits(uint64_t b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
LBP_HD uint64_t to_bits(double d) { uint64_t b; __builtin_memcpy(&b, &d, 8); return b; }

// ------------------------------------------------------------------------------------------------------ exp and log1p
// exp(x) = 2^k exp(r), k = round(x / ln 2), r = x - k ln 2 in two fma steps (|r| <= 0.3466), exp(r) = 1 + r + r^2 q(r) with
// the Taylor coefficients 1/2! .. 1/13! (the first term left out is below 2^-57), scaled by 2^k in two exact halves so that a
// subnormal result rounds once.  libm's special cases: NaN -> NaN, +inf -> +inf, -inf -> 0, overflow -> +inf, underflow -> 0.
LBP_HD double exp_r(double x) {
#pragma clang fp contract(off)
    if (x != x) return x + x;
    if (x > 710.0) return INFINITY;                      // 709.78.. .. 710 overflows in the scaling below
    if (x < -746.0) return 0.0;                          // -745.13.. .. -746 rounds to 0 in the scaling below
    const double shift = 6755399441055744.0;             // 1.5 * 2^52: adding it rounds to the nearest integer
    const double kd = fma(x, 1.4426950408889634074, shift) - shift;
    double r = fma(-kd, 6.93147180369123816490e-01, x);  // ln 2, high part (32 trailing zero bits)
    r = fma(-kd, 1.90821492927058770002e-10, r);         // ln 2, low part
    double q = 1.6059043836821613e-10;                   // 1/13!
    q = fma(q, r, 2.08767569878681e-09);                 // 1/12!
    q = fma(q, r, 2.505210838544172e-08);                // 1/11!
    q = fma(q, r, 2.755731922398589e-07);                // 1/10!
    q = fma(q, r, 2.7557319223985893e-06);               // 1/9!
    q = fma(q, r, 2.48015873015873e-05);                 // 1/8!
    q = fma(q, r, 0.0001984126984126984);                // 1/7!
    q = fma(q, r, 0.001388888888888889);                 // 1/6!
    q = fma(q, r, 0.008333333333333333);                 // 1/5!
    q = fma(q, r, 0.041666666666666664);                 // 1/4!
    q = fma(q, r, 0.16666666666666666);                  // 1/3!
    q = fma(q, r, 0.5);                                  // 1/2!
    const double p = 1.0 + fma(r * r, q, r);
    const int k = (int)kd, k1 = k >> 1, k2 = k - k1;     // both halves within [-538, 512]: normal powers of two
    return p * from_bits((uint64_t)(1023 + k1) << 52) * from_bits((uint64_t)(1023 + k2) << 52);
}

// log1p(x): u = 1 + x = 2^k m with m in [sqrt(1/2), sqrt 2), f = m - 1, s = f / (2 + f), log m = f - (f^2/2 - s (f^2/2 + R))
// where R = sum_{i>=1} 2 s^(2i) / (2i + 1) (eleven Taylor terms: s^2 <= 0.0295, the first left out is below 2^-60); c / u, c the
// rounding error of 1 + x, is added with the low part of k ln 2.  libm's special cases: NaN, x < -1 -> NaN, -1 -> -inf,
// +inf -> +inf, +-0 and tiny x -> x.
LBP_HD double log1p_r(double x) {
#pragma clang fp contract(off)
    if (x != x) return x + x;
    if (x < -1.0) return NAN;
    if (x == -1.0) return -INFINITY;
    if (x == INFINITY) return x;
    if (fabs(x) < 5.551115123125783e-17) return x;       // 2^-54: log1p(x) rounds to x; keeps -0 and subnormals
    double f = x, c = 0.0;
    int k = 0;
    if (!(x > -0.2928 && x < 0.4142)) {                  // outside, 1 + x leaves [sqrt(1/2), sqrt 2)
        const double u = 1.0 + x;
        c = (x >= 1.0 ? 1.0 - (u - x) : x - (u - 1.0)) / u;
        uint64_t b = to_bits(u);
        k = (int)(b >> 52 & 0x7ff) - 1023;
        b &= 0x000fffffffffffffull;
        if (b < 0x0006a09e667f3bcdull) {                 // mantissa below sqrt 2: m in [1, sqrt 2)
            b |= 0x3ff0000000000000ull;
        } else {                                         // m in [sqrt(1/2), 1)
            b |= 0x3fe0000000000000ull;
            k += 1;
        }
        f = from_bits(b) - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double R = 2.0 / 23.0;
    R = fma(R, z, 2.0 / 21.0);
    R = fma(R, z, 2.0 / 19.0);
    R = fma(R, z, 2.0 / 17.0);
    R = fma(R, z, 2.0 / 15.0);
    R = fma(R, z, 2.0 / 13.0);
    R = fma(R, z, 2.0 / 11.0);
    R = fma(R, z, 2.0 / 9.0);
    R = fma(R, z, 2.0 / 7.0);
    R = fma(R, z, 2.0 / 5.0);
    R = fma(R, z, 2.0 / 3.0);
    R = R * z;
    if (k == 0) return f - (hfsq - fma(s, hfsq + R, c));
    const double kd = (double)k;
    return fma(kd, 6.93147180369123816490e-01, -((hfsq - (fma(s, hfsq + R, fma(kd, 1.90821492927058770002e-10, c)))) - f));
}

// ----------------------------------------------------------------------------------------------------------- the proxy
// The record of a polish: rows of pitch kmax, read to depth k (the prefix record of a k sweep), as score_row reads it.
struct Record {
    const float *d1, *Dn, *trn, *dn, *Dm, *trm, *dm;
    const uint8_t *y;
    int64_t n;
    int kmax;
};

// What a thread sums over its rows and a backend reduces: log1p(z_i) | g_i A_n/k | g_i A_m/k | g_i B_n/k | g_i C_n/k |
// g_i B_m/k | g_i C_m/k, with e_j = exp(-(tau_1 D_ij + tau_2 tr_ij)), A = sum_j e_j dist_ij, B = sum_j e_j dist_ij D_ij,
// C = sum_j e_j dist_ij tr_ij, s_i = d1_i + beta A_n/k + gamma A_m/k, t_i = 2 y_i - 1, z_i = exp(-t_i s_i),
// g_i = -t_i z_i / (1 + z_i) / n.  Nothing is clamped: inf / inf = NaN propagates as it does in torch.
constexpr int NSUM = 7;

LBP_HD void proxy_row(const Record &r, int64_t i, int k, const double *hp, double *sum) {
#pragma clang fp contract(off)
    const double beta = hp[0], gamma = hp[1], t1n = hp[2], t2n = hp[3], t1m = hp[4], t2m = hp[5];
    double An = 0.0, Bn = 0.0, Cn = 0.0, Am = 0.0, Bm = 0.0, Cm = 0.0;
    for (int j = 0; j < k; ++j) {
        const int64_t o = i * (int64_t)r.kmax + j;
        const double Dn = (double)r.Dn[o], trn = (double)r.trn[o], Dm = (double)r.Dm[o], trm = (double)r.trm[o];
        const double wn = exp_r(-(t1n * Dn + t2n * trn)) * (double)r.dn[o];
        const double wm = exp_r(-(t1m * Dm + t2m * trm)) * (double)r.dm[o];
        An += wn; Bn += wn * Dn; Cn += wn * trn;
        Am += wm; Bm += wm * Dm; Cm += wm * trm;
    }
    const double kd = (double)k;
    const double an = An / kd, am = Am / kd;
    const double s = (double)r.d1[i] + beta * an + gamma * am;
    const double t = r.y[i] ? 1.0 : -1.0;
    const double z = exp_r(-(t * s));
    const double g = -t * z / (1.0 + z) / (double)r.n;
    sum[0] += log1p_r(z);
    sum[1] += g * an;
    sum[2] += g * am;
    sum[3] += g * (Bn / kd);
    sum[4] += g * (Cn / kd);
    sum[5] += g * (Bm / kd);
    sum[6] += g * (Cm / kd);
}

// The proxy over a backend B that holds the record of one polish:
//   void B::reduce(const double hp[6], double sum[NSUM])   the sums of proxy_row over all rows, in the fixed order
// fz / fo: bit i set = HP_NAMES[i] forced to 0.0 / 1.0 (metrics.unpack_vector: zeros first, then ones).  A forced coordinate
// enters as the constant and its gradient is 0: what autograd gives an x[i] that the loss never reads.
template <class B> struct Proxy {
    B &b;
    uint32_t fz, fo;
    int64_t n;
    LBP_HD void operator()(const double *x, double &loss, double *grad) {
#pragma clang fp contract(off)
        double hp[N], sum[NSUM];
        for (int i = 0; i < N; ++i) hp[i] = (fo >> i & 1) ? 1.0 : (fz >> i & 1) ? 0.0 : x[i];
        b.reduce(hp, sum);
        loss = sum[0] / (double)n;
        grad[0] = sum[1];
        grad[1] = sum[2];
        grad[2] = -hp[0] * sum[3];
        grad[3] = -hp[0] * sum[4];
        grad[4] = -hp[1] * sum[5];
        grad[5] = -hp[1] * sum[6];
        for (int i = 0; i < N; ++i)
            if ((fz | fo) >> i & 1) grad[i] = 0.0;
    }
};

// The reduction order of a workgroup, replayed on values held in memory: part[t][c] is thread t's sum c.  Lanes l and l ^ off
// add the same two values, so every lane of a wave ends with the same bits; the waves are then added in index order to 0.
inline void reduce_threads_host(double (*part)[NSUM], double *sum) {
#pragma clang fp contract(off)
    for (int c = 0; c < NSUM; ++c) sum[c] = 0.0;
    for (int w = 0; w < WAVES; ++w)
        for (int c = 0; c < NSUM; ++c) {
            double v[64], v2[64];
            for (int l = 0; l < 64; ++l) v[l] = part[64 * w + l][c];
            for (int off = 32; off > 0; off >>= 1) {
                for (int l = 0; l < 64; ++l) v2[l] = v[l] + v[l ^ off];
                for (int l = 0; l < 64; ++l) v[l] = v2[l];
            }
            sum[c] += v[0];
        }
}

// ------------------------------------------------------------------------------------------------------- torch.optim.LBFGS
LBP_HD double py_max(double a, double b) { return b > a ? b : a; }       // Python's max(a, b): the first unless the second is larger
LBP_HD double py_min(double a, double b) { return b < a ? b : a; }

LBP_HD double dot(const double *a, const double *b) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += a[i] * b[i];
    return s;
}

LBP_HD double abs_max(const double *v) {                                   // tensor.abs().max(): a NaN wins
    double m = fabs(v[0]);
    for (int i = 1; i < N; ++i) {
        const double a = fabs(v[i]);
        if (m == m && (a > m || a != a)) m = a;
    }
    return m;
}

// _cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds): bounded = false is bounds=None
LBP_HD double cubic_interpolate(double x1, double f1, double g1, double x2, double f2, double g2, bool bounded, double lo,
                                double hi) {
#pragma clang fp contract(off)
    if (!bounded) {
        if (x1 <= x2) { lo = x1; hi = x2; } else { lo = x2; hi = x1; }
    }
    const double d1 = g1 + g2 - 3.0 * (f1 - f2) / (x1 - x2);
    const double d2_square = d1 * d1 - g1 * g2;
    if (d2_square >= 0.0) {
        const double d2 = sqrt(d2_square);
        double min_pos;
        if (x1 <= x2) min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2.0 * d2));
        else min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2.0 * d2));
        return py_min(py_max(min_pos, lo), hi);
    }
    return (lo + hi) / 2.0;
}

// The two ends of a line-search bracket.  A one-point bracket (the Wolfe point met in the first phase) fills both ends.
struct Bracket {
    double t[2], f[2], g[2][N], gtd[2];
    LBP_HD void set(int e, double t_, double f_, const double *g_, double gtd_) {
        t[e] = t_; f[e] = f_; gtd[e] = gtd_;
        for (int i = 0; i < N; ++i) g[e][i] = g_[i];
    }
};

// obj_func(x, t, d) = closure at x + t d
template <class F> LBP_HD void directional(F &f, const double *x, double t, const double *d, double &loss, double *g) {
#pragma clang fp contract(off)
    double xt[N];
    for (int i = 0; i < N; ++i) xt[i] = x[i] + t * d[i];
    f(xt, loss, g);
}

// _strong_wolfe(obj_func, x, t, d, f, g, gtd, c1, c2, tolerance_change, max_ls) -> (f_new, g_new, t, ls_func_evals), in place
template <class F>
LBP_HD int strong_wolfe(F &func, const double *x, double &t, const double *d, double &f, double *g, double gtd, int max_ls) {
#pragma clang fp contract(off)
    const double d_norm = abs_max(d);
    double f_new, g_new[N], g_prev[N];
    directional(func, x, t, d, f_new, g_new);
    int ls_func_evals = 1;
    double gtd_new = dot(g_new, d);
    double t_prev = 0.0, f_prev = f, gtd_prev = gtd;
    for (int i = 0; i < N; ++i) g_prev[i] = g[i];
    Bracket br;
    bool done = false;
    int ls_iter = 0;
    while (ls_iter < max_ls) {
        if (f_new > (f + C1 * t * gtd) || (ls_iter > 1 && f_new >= f_prev)) {
            br.set(0, t_prev, f_prev, g_prev, gtd_prev);
            br.set(1, t, f_new, g_new, gtd_new);
            break;
        }
        if (fabs(gtd_new) <= -C2 * gtd) {
            br.set(0, t, f_new, g_new, gtd_new);
            br.set(1, t, f_new, g_new, gtd_new);
            done = true;
            break;
        }
        if (gtd_new >= 0.0) {
            br.set(0, t_prev, f_prev, g_prev, gtd_prev);
            br.set(1, t, f_new, g_new, gtd_new);
            break;
        }
        const double min_step = t + 0.01 * (t - t_prev);
        const double max_step = t * 10.0;
        const double tmp = t;
        t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, true, min_step, max_step);
        t_prev = tmp;
        f_prev = f_new;
        for (int i = 0; i < N; ++i) g_prev[i] = g_new[i];
        gtd_prev = gtd_new;
        directional(func, x, t, d, f_new, g_new);
        ls_func_evals += 1;
        gtd_new = dot(g_new, d);
        ls_iter += 1;
    }
    if (ls_iter == max_ls) {                             // the zoom below does not run: the slopes of this bracket are never read
        br.set(0, 0.0, f, g, gtd);
        br.set(1, t, f_new, g_new, gtd_new);
    }
    bool insuf_progress = false;
    int low_pos = br.f[0] <= br.f[1] ? 0 : 1, high_pos = 1 - low_pos;
    while (!done && ls_iter < max_ls) {
        if (fabs(br.t[1] - br.t[0]) * d_norm < TOL_CHANGE) break;
        t = cubic_interpolate(br.t[0], br.f[0], br.gtd[0], br.t[1], br.f[1], br.gtd[1], false, 0.0, 0.0);
        const double bmax = py_max(br.t[0], br.t[1]), bmin = py_min(br.t[0], br.t[1]);
        const double eps = 0.1 * (bmax - bmin);
        if (py_min(bmax - t, t - bmin) < eps) {
            if (insuf_progress || t >= bmax || t <= bmin) {
                if (fabs(t - bmax) < fabs(t - bmin)) t = bmax - eps;
                else t = bmin + eps;
                insuf_progress = false;
            } else {
                insuf_progress = true;
            }
        } else {
            insuf_progress = false;
        }
        directional(func, x, t, d, f_new, g_new);
        ls_func_evals += 1;
        gtd_new = dot(g_new, d);
        ls_iter += 1;
        if (f_new > (f + C1 * t * gtd) || f_new >= br.f[low_pos]) {
            br.set(high_pos, t, f_new, g_new, gtd_new);
            low_pos = br.f[0] <= br.f[1] ? 0 : 1;
            high_pos = 1 - low_pos;
        } else {
            if (fabs(gtd_new) <= -C2 * gtd) done = true;
            else if (gtd_new * (br.t[high_pos] - br.t[low_pos]) >= 0.0) br.set(high_pos, br.t[low_pos], br.f[low_pos], br.g[low_pos], br.gtd[low_pos]);
            br.set(low_pos, t, f_new, g_new, gtd_new);
        }
    }
    t = br.t[low_pos];
    f = br.f[low_pos];
    for (int i = 0; i < N; ++i) g[i] = br.g[low_pos][i];
    return ls_func_evals;
}

// old_dirs / old_stps / ro / al of the optimiser's state: HISTORY pairs as a ring (pop(0) = the head moves on).  On the device
// the four arrays live in LDS and every thread of the workgroup writes the same values to them; a thread reads a slot only
// after having written it itself, and between two writes of a slot lies the barrier of an objective evaluation.
struct History {
    double (*dirs)[N];      // y
    double (*stps)[N];      // s
    double *ro, *al;
};

struct State {              // what optimizer.state keeps between two step() calls
    int n_iter, num_old, head;
    double d[N], t, H_diag, prev_flat_grad[N], prev_loss;
};

LBP_HD void state_init(State &st) {
    st.n_iter = st.num_old = st.head = 0;
    st.t = 0.0; st.H_diag = 1.0; st.prev_loss = 0.0;
    for (int i = 0; i < N; ++i) st.d[i] = st.prev_flat_grad[i] = 0.0;
}

// LBFGS.step(closure): x moves in place; loss = the closure at the x the call leaves; nfev counts the closure's calls
template <class F> LBP_HD void step(F &func, double *x, State &st, const History &h, double &loss, int &nfev) {
#pragma clang fp contract(off)
    double flat_grad[N];
    func(x, loss, flat_grad);
    int current_evals = 1;
    nfev += 1;
    if (abs_max(flat_grad) <= TOL_GRAD) return;          // opt_cond: the step returns at once
    int n_iter = 0;
    while (n_iter < MAX_ITER) {
        n_iter += 1;
        st.n_iter += 1;
        if (st.n_iter == 1) {
            for (int i = 0; i < N; ++i) st.d[i] = -flat_grad[i];
            st.num_old = 0; st.head = 0;
            st.H_diag = 1.0;
        } else {
            double y[N], s[N], q[N];
            for (int i = 0; i < N; ++i) {
                y[i] = flat_grad[i] - st.prev_flat_grad[i];
                s[i] = st.d[i] * st.t;
            }
            const double ys = dot(y, s);
            if (ys > 1e-10) {
                if (st.num_old == HISTORY) {
                    st.head = (st.head + 1) % HISTORY;
                    st.num_old -= 1;
                }
                const int slot = (st.head + st.num_old) % HISTORY;
                for (int i = 0; i < N; ++i) { h.dirs[slot][i] = y[i]; h.stps[slot][i] = s[i]; }
                h.ro[slot] = 1.0 / ys;
                st.num_old += 1;
                st.H_diag = ys / dot(y, y);
            }
            for (int i = 0; i < N; ++i) q[i] = -flat_grad[i];
            for (int j = st.num_old - 1; j >= 0; --j) {
                const int slot = (st.head + j) % HISTORY;
                const double al = dot(h.stps[slot], q) * h.ro[slot];
                h.al[slot] = al;
                for (int i = 0; i < N; ++i) q[i] = q[i] + -al * h.dirs[slot][i];
            }
            for (int i = 0; i < N; ++i) st.d[i] = q[i] * st.H_diag;
            for (int j = 0; j < st.num_old; ++j) {
                const int slot = (st.head + j) % HISTORY;
                const double be_i = dot(h.dirs[slot], st.d) * h.ro[slot];
                const double a = h.al[slot] - be_i;
                for (int i = 0; i < N; ++i) st.d[i] = st.d[i] + a * h.stps[slot][i];
            }
        }
        for (int i = 0; i < N; ++i) st.prev_flat_grad[i] = flat_grad[i];
        st.prev_loss = loss;
        if (st.n_iter == 1) {
            double l1 = 0.0;
            for (int i = 0; i < N; ++i) l1 += fabs(flat_grad[i]);
            st.t = py_min(1.0, 1.0 / l1) * LR;
        } else {
            st.t = LR;
        }
        const double gtd = dot(flat_grad, st.d);
        if (gtd > -TOL_CHANGE) break;
        const int ls_func_evals = strong_wolfe(func, x, st.t, st.d, loss, flat_grad, gtd, MAX_EVAL - current_evals);
        for (int i = 0; i < N; ++i) x[i] = x[i] + st.t * st.d[i];
        const bool opt_cond = abs_max(flat_grad) <= TOL_GRAD;
        current_evals += ls_func_evals;
        nfev += ls_func_evals;
        if (n_iter == MAX_ITER) break;
        if (current_evals >= MAX_EVAL) break;
        if (opt_cond) break;
        double dt[N];
        for (int i = 0; i < N; ++i) dt[i] = st.d[i] * st.t;
        if (abs_max(dt) <= TOL_CHANGE) break;
        if (fabs(loss - st.prev_loss) < TOL_CHANGE) break;
    }
}

// torch_minimize (lib/metrics/utils.py:129-141): outer_steps calls of optimizer.step(closure); status 1 = x or loss not finite
template <class F> LBP_HD void polish(F &func, const double *x0, int outer_steps, const History &h, Result &res) {
    State st;
    state_init(st);
    double x[N], loss = NAN;
    for (int i = 0; i < N; ++i) x[i] = x0[i];
    int nfev = 0;
    for (int s = 0; s < outer_steps; ++s) step(func, x, st, h, loss, nfev);
    bool finite = is_finite(loss);
    for (int i = 0; i < N; ++i) {
        res.x[i] = x[i];
        finite &= is_finite(x[i]);
    }
    res.loss = loss;
    res.nfev = nfev;
    res.nit = st.n_iter;
    res.status = finite ? 0 : 1;
    res.pad = 0;
}

}  // namespace lbp
