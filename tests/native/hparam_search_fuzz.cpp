// Drives lemon_amd/csrc/hparam_search_core.hpp alone (no HIP, no Python) under -fsanitize=address,undefined: Nelder-Mead and
// Powell on a quadratic, on plateaus (constant and staircase), on an objective that returns NaN or infinities, from random
// starts and under random caps; the simplex sort on random tie patterns.  Checks what must hold on ANY objective: the search
// ends, nfev stays within the cap, the status is one of the known ones, the sort permutes rows and orders the values.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all hparam_search_fuzz.cpp && ./a.out [cases] [seed]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../lemon_amd/csrc/hparam_search_core.hpp"

static uint64_t g_state = 1;
static uint64_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}
static double unit() { return (double)(rnd() % 1000001) / 1000000.0; }

struct Objective {
    int kind;
    double c[hps::N];
    long calls;
    double operator()(const double *x) {
        ++calls;
        double q = 0.0;
        for (int i = 0; i < hps::N; ++i) q += (i + 1) * (x[i] - c[i]) * (x[i] - c[i]);
        switch (kind) {
        case 0: return q;                                         // quadratic
        case 1: return -0.0;                                      // flat
        case 2: return -floor(8.0 / (1.0 + q)) / 8.0;             // staircase: piecewise constant like F1
        case 3: return q > 2.0 ? NAN : q;                         // NaN outside a ball
        case 4: return x[0] > c[0] ? INFINITY : -INFINITY;        // infinities
        default: return (calls % 7 == 3) ? NAN : floor(q);        // NaN now and then
        }
    }
};

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            printf("hparam_search_fuzz: FAILED %s (line %d, case %ld, kind %d, method %d)\n", #cond, __LINE__, t, kind, method); \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 300;
    g_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
    for (long t = 0; t < cases; ++t) {
        const int kind = (int)(rnd() % 6), method = (int)(rnd() % 2);
        Objective f;
        f.kind = kind; f.calls = 0;
        double x0[hps::N];
        const int start = (int)(rnd() % 4);
        for (int i = 0; i < hps::N; ++i) {
            f.c[i] = 4.0 * unit() - 2.0;
            x0[i] = start == 0 ? 0.0 : start == 1 ? 20.0 * unit() - 10.0 : start == 2 ? 800.0 : (i % 2 ? -0.0 : 1e-300);
        }
        hps::Caps caps = hps::DEFAULT_CAPS;
        if (rnd() % 3 == 0) {
            caps.nm_maxfun = 1 + (int)(rnd() % 40); caps.nm_maxiter = 1 + (int)(rnd() % 40);
            caps.pw_maxfun = 1 + (int)(rnd() % 200); caps.pw_maxiter = 1 + (int)(rnd() % 3);
        }
        hps::Result r;
        hps::search(f, method, x0, caps, r);
        const int maxfun = method == hps::POWELL ? caps.pw_maxfun : caps.nm_maxfun;
        CHECK(r.nfev == f.calls && r.nfev <= maxfun && r.nfev >= 1);
        CHECK(r.status == 0 || r.status == 1 || r.status == 2 || r.status == 3 || r.status == hps::STATUS_BRACKET_ITER);
        CHECK(r.nit >= 0 && r.nit <= (method == hps::POWELL ? caps.pw_maxiter : caps.nm_maxiter));
        if (kind == 0) {
            Objective g = f;
            CHECK(r.fun <= g(x0));                                                  // never worse than the start
            if (method == hps::POWELL && r.status == 0) {                           // Powell finds the bowl's minimum
                for (int i = 0; i < hps::N; ++i) CHECK(fabs(r.x[i] - f.c[i]) < 1e-2);
                CHECK(r.fun < 1e-3);
            }
        }
        if (kind == 1 && caps.nm_maxfun == hps::DEFAULT_CAPS.nm_maxfun) CHECK(r.fun == 0.0 && r.status == 0);
    }
    // the simplex sort: a permutation of the rows, values in ascending order, equal to a plain sort of the values
    for (long t = 0; t < cases * 20; ++t) {
        const int kind = -1, method = -1;
        double sim[hps::N + 1][hps::N], fsim[hps::N + 1];
        const int levels = 1 + (int)(rnd() % 5);
        for (int i = 0; i <= hps::N; ++i) {
            fsim[i] = -(double)(rnd() % levels) / 4.0;
            if (rnd() % 50 == 0) fsim[i] = rnd() % 2 ? INFINITY : NAN;
            for (int c = 0; c < hps::N; ++c) sim[i][c] = (double)i;      // a row carries its index
        }
        double before[hps::N + 1];
        for (int i = 0; i <= hps::N; ++i) before[i] = fsim[i];
        hps::sort_simplex(sim, fsim);
        int seen = 0;
        for (int i = 0; i <= hps::N; ++i) {
            const int from = (int)sim[i][0];
            CHECK(from >= 0 && from <= hps::N);
            for (int c = 0; c < hps::N; ++c) CHECK(sim[i][c] == (double)from);
            seen |= 1 << from;
            CHECK((fsim[i] == before[from]) || (fsim[i] != fsim[i] && before[from] != before[from]));
            if (i) CHECK(!(fsim[i] < fsim[i - 1]) && !(fsim[i - 1] != fsim[i - 1] && fsim[i] == fsim[i]));
        }
        CHECK(seen == (1 << (hps::N + 1)) - 1);
    }
    printf("hparam_search_fuzz: ok (%ld cases)\n", cases);
    return 0;
}
