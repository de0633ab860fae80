// Drives lemon_amd/csrc/l2_from_ip_core.hpp alone (no HIP, no Python): random databases of (score, norm) pairs drawn from small
// value sets -- so that scores, norms and distances tie -- with +0 / -0, denormals and huge values among them, an exact IP list
// of random depth (padded when the database is shorter), and now and then a query norm or a score that is not finite or an id
// that is no row.  Checks, against a sort of the WHOLE database by the same expression:
//   * the output is always the first k of the list's own real slots by (D, id), padded with (-1, FLT_MAX);
//   * cert == 1 implies the output IS the first k of the whole database: the certificate is sound;
//   * a list that holds the whole database is certified, anything that is not finite never is.
//   g++ -std=c++17 -O1 -g -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] l2_from_ip_fuzz.cpp && ./a.out [cases] [seed]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../lemon_amd/csrc/l2_from_ip_core.hpp"

static uint64_t g_state = 1;
static uint64_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}

static float pick_score(int flavour) {
    static const float small[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 1e-39f, 0.5f, 0.5f, 0.49999997f, 0.50000006f, 1.0f, -1.0f, 0.25f};
    if (flavour == 0) return small[rnd() % (sizeof(small) / sizeof(small[0]))];
    if (flavour == 1) return (float)(rnd() % 9) * 0.125f;                          // nine values: ties everywhere
    if (flavour == 2) return 1.0f - (float)(rnd() % 64) * 5.9604645e-8f;           // neighbours of 1 in the last bits
    return ((float)(rnd() % 2000001) / 1000000.0f - 1.0f) * (rnd() % 16 == 0 ? 1e30f : 1.0f);
}
static float pick_norm(int flavour) {
    static const float small[] = {0.0f, 1e-45f, 1e-39f, 1.0f, 1.0f, 0.99999994f, 1.0000001f, 2.0f, 4.0f};
    if (flavour == 0) return small[rnd() % (sizeof(small) / sizeof(small[0]))];
    if (flavour == 1) return 1.0f;
    if (flavour == 2) return 1.0f + (float)((int)(rnd() % 5) - 2) * 5.9604645e-8f;
    return (float)(rnd() % 4000001) / 1000000.0f * (rnd() % 16 == 0 ? 1e30f : 1.0f);
}

static bool same(float a, float b) { return memcmp(&a, &b, 4) == 0; }

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            printf("l2_from_ip_fuzz: FAILED %s (line %d, case %ld, n %d, kd %d, k %d)\n", #cond, __LINE__, t, n, kd, k); \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 1000;
    g_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
    long certified = 0, uncertified = 0;
    for (long t = 0; t < cases; ++t) {
        const int n = (int)(rnd() % 4 == 0 ? rnd() % 70 : 1 + rnd() % 300);
        const int kd = 1 + (int)(rnd() % l2ip::MAX_KD), k = 1 + (int)(rnd() % kd);
        const int fs = (int)(rnd() % 4), fn = (int)(rnd() % 4);
        std::vector<float> s(n), xx(n);
        for (int i = 0; i < n; ++i) { s[i] = pick_score(fs); xx[i] = pick_norm(fn); }
        float qq = pick_norm((int)(rnd() % 4));
        const int poison = (int)(rnd() % 12);                 // 0: qq, 1: a score, 2: an id, 3: xx_min; else nothing
        if (poison == 0) qq = rnd() % 2 ? INFINITY : NAN;
        if (poison == 1 && n) s[rnd() % n] = INFINITY;        // +inf stands at the head of every IP list
        float xx_min = FLT_MAX;
        for (int i = 0; i < n; ++i) xx_min = xx[i] < xx_min ? xx[i] : xx_min;
        if (poison == 3) xx_min = NAN;
        // the exact IP list: (s descending, id ascending), padded with (-1, -FLT_MAX)
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return s[a] > s[b] || (s[a] == s[b] && a < b); });
        float ls[l2ip::MAX_KD];
        int64_t li[l2ip::MAX_KD];
        for (int j = 0; j < kd; ++j) {
            ls[j] = j < n ? s[order[j]] : -FLT_MAX;
            li[j] = j < n ? order[j] : -1;
        }
        bool bad_id = false;
        if (poison == 2 && n) { li[rnd() % (kd < n ? kd : n)] = n + (int64_t)(rnd() % 3); bad_id = true; }
        // references: the first k of the list's real slots, and of the whole database
        struct Ent { float D; int64_t id; };
        auto by_D = [](const Ent &a, const Ent &b) { return a.D < b.D || (a.D == b.D && a.id < b.id); };
        std::vector<Ent> of_list, of_db;
        for (int j = 0; j < kd; ++j)
            if (li[j] >= 0 && li[j] < n) of_list.push_back({l2ip::dist(ls[j], qq, xx[li[j]]), li[j]});
        for (int i = 0; i < n; ++i) of_db.push_back({l2ip::dist(s[i], qq, xx[i]), i});
        std::sort(of_list.begin(), of_list.end(), by_D);
        std::sort(of_db.begin(), of_db.end(), by_D);
        // guard slots around the outputs
        float Dg[l2ip::MAX_KD + 2];
        int64_t Ig[l2ip::MAX_KD + 2];
        for (int j = 0; j < l2ip::MAX_KD + 2; ++j) { Dg[j] = -7.0f; Ig[j] = -7; }
        const unsigned char cert = l2ip::derive_row(ls, li, kd, k, qq, xx.data(), n, xx_min, Dg + 1, Ig + 1);
        CHECK(cert == 0 || cert == 1);
        CHECK(Dg[0] == -7.0f && Ig[0] == -7);
        for (int j = k + 1; j < l2ip::MAX_KD + 2; ++j) CHECK(Dg[j] == -7.0f && Ig[j] == -7);
        for (int j = 0; j < k; ++j) {
            if (bad_id) break;                                // (two slots may then name one row: no order to check)
            if (j < (int)of_list.size()) CHECK(same(Dg[1 + j], of_list[j].D) && Ig[1 + j] == of_list[j].id);
            else CHECK(same(Dg[1 + j], FLT_MAX) && Ig[1 + j] == -1);
        }
        if (cert) {
            ++certified;
            CHECK(poison > 3 || (poison == 1 && n == 0) || (poison == 2 && n == 0));
            for (int j = 0; j < k; ++j) {
                if (j < n) CHECK(same(Dg[1 + j], of_db[j].D) && Ig[1 + j] == of_db[j].id);
                else CHECK(same(Dg[1 + j], FLT_MAX) && Ig[1 + j] == -1);
            }
        } else {
            ++uncertified;
            if (poison > 3 && n < kd) CHECK(cert == 1);       // the whole database, all finite: must be certified
        }
    }
    if (cases >= 1000 && (certified * 10 < cases || uncertified * 10 < cases)) {
        printf("l2_from_ip_fuzz: FAILED one-sided run (%ld certified, %ld not)\n", certified, uncertified);
        return 1;
    }
    printf("l2_from_ip_fuzz: ok (%ld cases, %ld certified)\n", cases, certified);
    return 0;
}
