// Drives lemon_amd/csrc/lbfgs_core.hpp alone (no HIP, no Python), also under -fsanitize=address,undefined.
//   lbfgs_fuzz trace                the optimiser on two functions with benign dynamics, x after every outer step as hex floats:
//                                   "quadratic <step> <nfev> <nit> x0 .. x5" for 1/2 sum c_i (x_i - a_i)^2, c from 1 to 100, from
//                                   (1, .., 1) -- its later steps return at once on opt_cond -- and
//                                   "rosenbrock ..." for the six-variable Rosenbrock function from (-1.2, 1, -1.2, 1, -1.2, 1);
//                                   tests/test_lbfgs_polish_host.py runs torch.optim.LBFGS on the same functions and compares
//   lbfgs_fuzz [cases] [seed]       random starts on a quadratic, a constant, objectives that return NaN or infinities now and
//                                   then or from a point on, and a long Rosenbrock run that evicts history pairs; checks what must
//                                   hold on ANY objective: the polish ends, nfev and nit stay within torch's counters, the status
//                                   says whether the result is finite; exp_r / log1p_r on special and random arguments
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all lbfgs_fuzz.cpp
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../lemon_amd/csrc/lbfgs_core.hpp"

static uint64_t g_state = 1;
static uint64_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}
static double unit() { return (double)(rnd() % 1000001) / 1000000.0; }

static const double QUAD_C[lbp::N] = {1.0, 20.8, 40.6, 60.4, 80.2, 100.0};
static const double QUAD_A[lbp::N] = {1.0, -2.0, 0.5, 3.0, -1.5, 0.25};

struct Objective {
    int kind;
    double c[lbp::N];
    long calls;
    double scale = 1.0;                                               // of Rosenbrock's value and slope
    void operator()(const double *x, double &loss, double *g) {
        ++calls;
        switch (kind) {
        case 0:                                                       // the test's quadratic
        case 2: {                                                     // a quadratic around c
            double q = 0.0;
            for (int i = 0; i < lbp::N; ++i) {
                const double w = kind == 0 ? QUAD_C[i] : (double)(i + 1), a = kind == 0 ? QUAD_A[i] : c[i];
                q += 0.5 * w * (x[i] - a) * (x[i] - a);
                g[i] = w * (x[i] - a);
            }
            loss = q;
            return;
        }
        case 1: {                                                     // Rosenbrock: sum 100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2
            double f = 0.0;
            for (int i = 0; i < lbp::N; ++i) g[i] = 0.0;
            for (int i = 0; i + 1 < lbp::N; ++i) {
                const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
                f += 100.0 * a * a + b * b;
                g[i] += -400.0 * a * x[i] - 2.0 * b;
                g[i + 1] += 200.0 * a;
            }
            loss = scale * f;
            for (int i = 0; i < lbp::N; ++i) g[i] *= scale;
            return;
        }
        case 3:                                                       // constant: the gradient is zero
            loss = 0.25;
            for (int i = 0; i < lbp::N; ++i) g[i] = 0.0;
            return;
        case 4:                                                       // NaN now and then
        case 5:                                                       // infinities beyond a plane, a NaN slope with them
        default: {
            double q = 0.0;
            for (int i = 0; i < lbp::N; ++i) { q += (x[i] - c[i]) * (x[i] - c[i]); g[i] = 2.0 * (x[i] - c[i]); }
            loss = q;
            if (kind == 4 && calls % 7 == 3) { loss = NAN; g[calls % lbp::N] = NAN; }
            if (kind == 5 && x[0] > c[0]) { loss = INFINITY; g[0] = NAN; }
            if (kind == 6) { loss = NAN; }                            // a NaN value over a finite slope
            return;
        }
        }
    }
};

struct Hist {
    double dirs[lbp::HISTORY][lbp::N], stps[lbp::HISTORY][lbp::N], ro[lbp::HISTORY], al[lbp::HISTORY];
    lbp::History view() { return lbp::History{dirs, stps, ro, al}; }
};

static int trace(const char *name, int kind, const double *x0) {
    Objective f;
    f.kind = kind; f.calls = 0;
    static Hist trace_hist;
    Hist *hist = &trace_hist;
    lbp::State st;
    lbp::state_init(st);
    double x[lbp::N], loss = NAN;
    memcpy(x, x0, sizeof x);
    int nfev = 0;
    for (int s = 0; s < lbp::MAX_OUTER; ++s) {
        lbp::step(f, x, st, hist->view(), loss, nfev);
        printf("%s %d %d %d", name, s, nfev, st.n_iter);
        for (int i = 0; i < lbp::N; ++i) printf(" %a", x[i]);
        printf("\n");
    }
    return 0;
}

#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            printf("lbfgs_fuzz: FAILED %s (line %d, case %ld, kind %d)\n", #cond, __LINE__, t, kind); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "trace")) {
        const double q0[lbp::N] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, r0[lbp::N] = {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0};
        return trace("quadratic", 0, q0) || trace("rosenbrock", 1, r0);
    }
    const long cases = argc > 1 ? atol(argv[1]) : 300;
    g_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
    static Hist main_hist;
    Hist *hist = &main_hist;
    for (long t = 0; t < cases; ++t) {
        const int kind = 1 + (int)(rnd() % 6);
        Objective f;
        f.kind = kind; f.calls = 0;
        double x0[lbp::N];
        const int start = (int)(rnd() % 4);
        for (int i = 0; i < lbp::N; ++i) {
            f.c[i] = 4.0 * unit() - 2.0;
            x0[i] = start == 0 ? 0.0 : start == 1 ? 20.0 * unit() - 10.0 : start == 2 ? 800.0 : (i % 2 ? -0.0 : 1e-300);
        }
        const int outer = 1 + (int)(rnd() % lbp::MAX_OUTER);
        lbp::Result r;
        lbp::polish(f, x0, outer, hist->view(), r);
        CHECK(r.nfev == f.calls && r.nfev >= outer && r.nfev <= outer * (lbp::MAX_EVAL + 1));
        CHECK(r.nit >= 0 && r.nit <= outer * lbp::MAX_ITER);
        bool finite = lbp::is_finite(r.loss);
        for (int i = 0; i < lbp::N; ++i) finite &= lbp::is_finite(r.x[i]);
        CHECK(r.status == (finite ? 0 : 1) && r.pad == 0);
        if (kind == 3) {                                              // opt_cond at once, in every step: x does not move
            CHECK(r.nfev == outer && r.nit == 0 && r.loss == 0.25);
            for (int i = 0; i < lbp::N; ++i) CHECK(r.x[i] == x0[i] || (r.x[i] == 0.0 && x0[i] == 0.0));
        }
        if (kind == 2 && outer == lbp::MAX_OUTER && start < 2) {      // the bowl's minimum, as far as torch's own rule goes: a
            for (int i = 0; i < lbp::N; ++i) CHECK(fabs(r.x[i] - f.c[i]) < 1e-3);   // step ends where g . d > -1e-9, |g| ~ 1e-4
        }
    }
    {   // a long run in the valley of Rosenbrock's function times 1e4 (the absolute tolerances bite later): more than HISTORY
        // curvature pairs, so the ring evicts
        const long t = -1;
        const int kind = 1;
        Objective f;
        f.kind = kind; f.calls = 0; f.scale = 1e4;
        lbp::State st;
        lbp::state_init(st);
        double x[lbp::N] = {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, loss = NAN;
        int nfev = 0, evicted = 0;
        for (int s = 0; s < 100; ++s) {
            const int head = st.head;
            lbp::step(f, x, st, hist->view(), loss, nfev);
            evicted |= st.head != head;
            CHECK(st.num_old >= 0 && st.num_old <= lbp::HISTORY && st.head >= 0 && st.head < lbp::HISTORY);
        }
        printf("lbfgs_fuzz: long rosenbrock run: loss %g, nit %d, pairs %d, evicted %d\n", loss, st.n_iter, st.num_old, evicted);
        CHECK(lbp::is_finite(loss) && loss < 1e-6 && evicted);
        for (int i = 0; i < lbp::N; ++i) CHECK(fabs(x[i] - 1.0) < 1e-3);
    }
    for (long t = 0; t < cases * 50; ++t) {                           // exp_r / log1p_r: specials and the shape of the result
        const int kind = -1;
        const double specials[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, 709.782712893384, 709.7827128933841, 710.0, 710.1, -745.2,
                                   -746.0, -746.1, 5e-324, -1.0, -1.0000000000000002, -0.9999999999999999, 1.7976931348623157e308};
        const int ns = (int)(sizeof specials / sizeof specials[0]);
        const double x = t < ns ? specials[t] : (rnd() % 2 ? 1500.0 * unit() - 760.0 : exp(40.0 * unit() - 20.0) - (rnd() % 2));
        const double e = lbp::exp_r(x), l = lbp::log1p_r(x);
        if (x != x) { CHECK(e != e && l != l); continue; }
        CHECK(e >= 0.0 && (x <= 709.78 ? lbp::is_finite(e) : true) && (x > 709.79 ? e == INFINITY : true));
        CHECK(x < -746.0 ? e == 0.0 : true);
        CHECK(fabs(e - exp(x)) <= 1e-15 * exp(x) || e == exp(x) || exp(x) < 1e-300);
        if (x < -1.0) CHECK(l != l);
        else if (x == -1.0) CHECK(l == -INFINITY);
        else CHECK(fabs(l - log1p(x)) <= 1e-15 * fabs(log1p(x)) || l == log1p(x));
    }
    printf("lbfgs_fuzz: ok (%ld cases)\n", cases);
    return 0;
}
