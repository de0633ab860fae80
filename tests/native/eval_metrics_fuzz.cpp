// Drives lemon_amd/csrc/eval_metrics_core.hpp alone (no HIP, no Python) under -fsanitize=address,undefined: random segments
// with ties, signed zeros, a single row, one class, sizes around the pairwise blocks and numpy's 8 192-row chunk.  Checks what
// must hold on ANY segment: the binary search equals a plain count for every threshold (infinities and NaN included), the four
// counts add up, every threshold search ends inside [min, max], the pair count behind AUROC equals the count over all pairs,
// AUPRC lies in [0, 1], the pairwise and the lane-ordered sums stay within n eps sum|a| of a plain loop, linspace keeps its ends,
// the extrema rule returns a grid point, a mid-point of two or the mean on arbitrary densities (plateaus and zeros included).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all eval_metrics_fuzz.cpp && ./a.out [cases] [seed]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../lemon_amd/csrc/eval_metrics_core.hpp"

static uint64_t g_state = 1;
static uint64_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}
static double unit() { return (double)(rnd() % 1000001) / 1000000.0; }

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            printf("eval_metrics_fuzz: FAILED %s (line %d, case %ld, n %ld, kind %d)\n", #cond, __LINE__, t, (long)n, kind); \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 200;
    g_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
    const double sqrt_eps = sqrt(2.2e-16), golden_mean = 0.5 * (3.0 - sqrt(5.0));
    const int64_t edges[] = {1, 2, 7, 8, 9, 127, 128, 129, 136, 255, 257, 1000, 8191, 8192, 8193, 16385};
    for (long t = 0; t < cases; ++t) {
        const int kind = (int)(rnd() % 6);
        int64_t n = (rnd() % 4 == 0) ? edges[rnd() % (sizeof(edges) / sizeof(edges[0]))] : 1 + (int64_t)(rnd() % 400);
        std::vector<double> orig((size_t)n);
        std::vector<uint8_t> y((size_t)n);
        const double scale = kind == 4 ? 1e-300 : kind == 5 ? 1e150 : 3.0;
        for (int64_t i = 0; i < n; ++i) {
            double v = (unit() - 0.5) * scale;
            if (kind == 1) v = floor(v * 4.0) / 4.0;                  // heavy ties
            if (kind == 2) v = (rnd() & 1) ? 0.0 : -0.0;              // signed zeros only
            if (kind == 3 && i % 3 == 0) v = 1.0;                     // many rows tied at the maximum
            orig[i] = v;
            y[i] = (uint8_t)((rnd() % 10) < 3 ? 1 + rnd() % 200 : 0);
        }
        if (rnd() % 8 == 0) for (int64_t i = 0; i < n; ++i) y[i] = 0;  // one class
        // the descending sort and the prefix counts
        std::vector<int64_t> order((size_t)n);
        for (int64_t i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return orig[a] > orig[b]; });
        std::vector<double> ss((size_t)n);
        std::vector<int32_t> cp((size_t)n);
        int64_t run = 0;
        for (int64_t i = 0; i < n; ++i) { ss[i] = orig[order[i]]; run += y[order[i]] != 0; cp[i] = (int32_t)run; }
        const evm::Sorted v{ss.data(), cp.data(), n};
        const int64_t pos = evm::positives(v);
        CHECK(pos == run);
        const double lo = ss[n - 1], hi = ss[0];

        // counts against a plain loop
        for (int q = 0; q < 24; ++q) {
            double thr = q == 0 ? INFINITY : q == 1 ? -INFINITY : q == 2 ? NAN : q == 3 ? lo : q == 4 ? hi : q == 5 ? 0.0
                       : (q & 1) ? orig[rnd() % n] : (unit() - 0.5) * scale * 1.2;
            int64_t cnt = 0, tp = 0;
            for (int64_t i = 0; i < n; ++i) { const bool p = orig[i] >= thr; cnt += p; tp += p && y[i]; }
            CHECK(evm::count_ge(v, thr) == cnt && evm::tp_at(v, cnt) == tp);
            int64_t c[4];
            evm::counts_at(v, thr, c);
            CHECK(c[0] == tp && c[1] == cnt - tp && c[2] == pos - tp && c[0] + c[1] + c[2] + c[3] == n && c[3] >= 0);
            const double f1 = evm::f1_counts(tp, cnt, pos);
            CHECK(f1 >= 0.0 && f1 <= 1.0);
        }

        // linspace and optimize_f1
        for (int num : {evm::N_CAND, evm::N_GRID}) {
            CHECK(evm::linspace_at(lo, hi, num, num - 1) == hi && evm::linspace_at(lo, hi, num, 0) == lo);
            double before = lo;
            for (int i = 0; i < num; ++i) {
                const double c = evm::linspace_at(lo, hi, num, i);
                CHECK(c >= before && c <= hi + fabs(hi) * 1e-15);
                before = c;
            }
        }
        double f1[evm::N_CAND];
        for (int i = 0; i < evm::N_CAND; ++i) { f1[i] = evm::candidate_f1(v, i); CHECK(f1[i] >= 0.0 && f1[i] <= 1.0); }
        const int at = evm::pick_candidate(f1);
        CHECK(at >= 0 && at < evm::N_CAND);
        for (int i = 0; i < evm::N_CAND; ++i) CHECK(f1[i] < f1[at] || (f1[i] == f1[at] && i <= at));

        // bisect and its fall-back
        for (double prev : {0.0, 0.3, (double)pos / (double)n, 1.0, 1.5, -0.5}) {
            int fallback = -1;
            const double thr = evm::prev_threshold(v, prev, sqrt_eps, golden_mean, fallback);
            CHECK((fallback == 0 || fallback == 1) && thr >= lo && thr <= hi);
        }

        // the curve: pair counts against all pairs, AUPRC in [0, 1]
        if (pos > 0 && pos < n) {
            evm::LaneSums ap;
            int64_t u2 = 0, prev_rows = 0, prev_tp = 0;
            for (int64_t i = 0; i < n; ++i) {
                if (!(i == n - 1 || ss[i] != ss[i + 1])) continue;
                ap.add(i, evm::auprc_term(i + 1, cp[i], prev_tp, pos));
                u2 += evm::auroc_term(i + 1, cp[i], prev_rows, prev_tp);
                prev_rows = i + 1; prev_tp = cp[i];
            }
            const double auprc = ap.total(), auroc = evm::auroc_from(u2, pos, n);
            CHECK(auprc >= 0.0 && auprc <= 1.0 + 1e-12 && auroc >= 0.0 && auroc <= 1.0);
            if (n <= 300) {
                int64_t twice = 0;                                   // 2 for a pair in order, 1 for a tied pair
                for (int64_t i = 0; i < n; ++i)
                    for (int64_t j = 0; j < n; ++j)
                        if (y[i] && !y[j]) twice += orig[i] > orig[j] ? 2 : orig[i] == orig[j] ? 1 : 0;
                CHECK(auroc == (double)twice / (2.0 * (double)pos * (double)(n - pos)));
            }
        }

        // numpy's order and the lanes' order against a plain loop
        double plain = 0.0, mag = 0.0;
        evm::LaneSums lanes;
        for (int64_t i = 0; i < n; ++i) { plain += orig[i]; mag += fabs(orig[i]); lanes.add(i, orig[i]); }
        const double slack = (double)n * 2.3e-16 * mag;
        const double mean = evm::np_mean(orig.data(), n);
        CHECK(fabs(mean * (double)n - plain) <= slack + fabs(plain) * 4.5e-16 && fabs(lanes.total() - plain) <= slack);
        if (n <= evm::NP_CHUNK) CHECK(fabs(evm::pairwise_sum(orig.data(), n) - plain) <= slack);

        // the KDE set-up and the extrema rule
        if (n >= 2) {
            evm::LaneSums sq;
            for (int64_t i = 0; i < n; ++i) sq.add(i, evm::sq_dev(orig[i], mean));
            evm::Kde k;
            const bool ok = evm::kde_setup(lo, hi, mean, sq.total(), n, k);
            if (lo == hi) CHECK(!ok || sq.total() > 0.0);
            if (ok) {
                CHECK(k.h > 0.0 && k.norm > 0.0 && k.w > 0.0);
                std::vector<double> dens((size_t)evm::N_GRID);
                const int shape = (int)(rnd() % 4);
                for (int j = 0; j < evm::N_GRID; ++j) {
                    if (shape == 0) {                                 // the real density, a few rows of it
                        double acc = 0.0;
                        const double xj = evm::kde_point(k, j);
                        for (int64_t i = 0; i < n && i < 40; ++i) acc += evm::kde_term(k, orig[i] / k.h, xj);
                        dens[j] = acc;
                        CHECK(acc >= 0.0 && acc == acc);
                    } else {
                        dens[j] = shape == 1 ? 0.0 : shape == 2 ? floor(unit() * 3.0) : unit();
                    }
                }
                int branch = 0;
                const double thr = evm::kde_threshold(k, dens.data(), branch);
                CHECK(branch >= evm::KDE_MINIMA && branch <= evm::KDE_MEAN);
                CHECK(branch == evm::KDE_MEAN ? thr == mean : (thr >= lo && thr <= hi));
                if (shape == 1) CHECK(branch == evm::KDE_MEAN);
            }
        }
        for (int st = 0; st < 32; ++st) {
            const int s = evm::segment_status(st & 1, st & 2, (st & 4) ? 1 : n, (st & 8) ? 0 : pos, !(st & 16));
            CHECK(s >= evm::ST_OK && s <= evm::ST_ZERO_VAR && ((st & 2) ? s == evm::ST_NONFINITE : true));
        }
    }
    printf("eval_metrics_fuzz: ok (%ld cases)\n", cases);
    return 0;
}
