// l2_from_ip_core.hpp -- the exact squared-L2 neighbour list of a query, derived from a deeper inner-product list (plain C++,
// host and device; no HIP, no library).  Run by k_l2_from_ip (metric_sweep.hip, one lane per candidate), by the host twin
// lemon_l2_from_ip_host (the lanes looped) and by tests/native/l2_from_ip_fuzz.cpp.
//
// The numeric contract (oracle/lemon_oracle.c lo_l2_from_ip) defines the L2 result as
//     D_l2(q, x) = max(0, fmaf(-2, dot(q,x), dot(q,q) + dot(x,x)))
// where dot(q,x) is the fp32 chain the IP search returns as its D, dot(x,x) is the row norm every index stores at add and
// dot(q,q) is one more chain.  So the L2 distance of every row of an IP list is known without touching the row again.
//
// Input per query: the IP list at depth kd, s_0 >= ... >= s_{kd-1} with ids, ordered (s descending, id ascending); padding slots
// (the DB has fewer than kd rows, or a NaN score that is never selected) carry id < 0 and stand at the end.  qq, xx[id] and
// xx_min, the smallest stored row norm of the whole index.
// Output: the first k of the real slots by (D ascending, id ascending); slots beyond them get I = -1, D = +FLT_MAX.
//
// Certificate.  cert = 1 says "this IS the k list IndexFlatL2.search returns, bit for bit":
//   * slot kd-1 is padding: the list holds every row of the DB that a search can select, so the ranking is over the whole DB;
//   * otherwise D_(k-1) < B STRICTLY, with B = max(0, fmaf(-2, s_{kd-1}, qq + xx_min)).
// Why that is sound: a row outside the list has s <= s_{kd-1} (the IP list is exact) and xx >= xx_min.  fp32 addition, fmaf in
// each argument and max are monotone (rounding is monotone), so with c = -2 < 0
//     qq + xx >= qq + xx_min,   fmaf(-2, s, qq + xx) >= fmaf(-2, s_{kd-1}, qq + xx_min),   D >= B.
// Every unseen row is therefore at distance >= B > D_(k-1): none of them enters the first k, and because the inequality is
// strict the tie rule (lower id first) never has to be applied to a row nobody has seen.  With D_(k-1) == B an unseen row
// could tie and win on its id, so equality is NOT certified.
//   * cert = 0 whenever qq, xx_min or the s of a real slot is not finite (the monotonicity argument needs ordered numbers), or
//     an id is not a row of the index.  The caller passes xx_min = NaN when ANY stored norm is not finite: a row with a NaN or
//     an infinity in it can score NaN, which the IP search never selects while the L2 expression maps it to distance 0, so with
//     such a row in the DB nothing is certified.  With every norm and qq finite no chain of fmaf yields NaN (a finite product
//     added to an infinity keeps it), so every row the list does not show really has s <= s_{kd-1}.
// An uncertified query goes through the ordinary L2 search (the caller's job); its derived row is still written.
//
// D is never NaN (v > 0 ? v : 0 maps NaN to +0) and never -0, so (D, id) with distinct ids is a strict total order and the
// rank of a slot -- the number of slots that precede it -- is a permutation of 0 .. real-1: no sort, every slot finds its own
// place with one pass over the others.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define L2IP_HD __host__ __device__
#else
#define L2IP_HD
#endif

namespace l2ip {

constexpr int MAX_KD = 64;          // == LEMON_MAX_K: a list is at most one wavefront

// the oracle's expression, no contraction, no reassociation (lo_l2_from_ip)
L2IP_HD inline float dist(float s, float qq, float xx) {
    const float v = fmaf(-2.0f, s, qq + xx);
    return v > 0.0f ? v : 0.0f;
}

L2IP_HD inline bool is_finite(float v) { return v - v == 0.0f; }       // false for NaN and both infinities

// (D ascending, id ascending)
L2IP_HD inline bool before(float Da, int64_t ia, float Db, int64_t ib) { return Da < Db || (Da == Db && ia < ib); }

// rank of slot j among the real slots of a list: D / id / real are the kd slots of ONE query (LDS on the device)
L2IP_HD inline int rank_of(const float *D, const int64_t *id, const unsigned char *real, int kd, int j) {
    int r = 0;
    const float Dj = D[j];
    const int64_t ij = id[j];
    for (int t = 0; t < kd; ++t) r += (real[t] && before(D[t], id[t], Dj, ij)) ? 1 : 0;
    return r;
}

// the bound every row outside the list stays above
L2IP_HD inline float bound(float s_last, float qq, float xx_min) { return dist(s_last, qq, xx_min); }

// one query on the host: the device kernel makes the same calls with a lane per j.  xx [n]; the outputs are rows of k.
inline unsigned char derive_row(const float *s, const int64_t *ids, int kd, int k, float qq, const float *xx, int64_t n,
                                float xx_min, float *D_out, int64_t *I_out) {
    float D[MAX_KD];
    unsigned char real[MAX_KD];
    bool ok = is_finite(qq) && is_finite(xx_min);
    int n_real = 0;
    for (int j = 0; j < kd; ++j) {
        const int64_t id = ids[j];
        real[j] = (id >= 0 && id < n) ? 1 : 0;
        if (id >= n) ok = false;
        D[j] = 0.0f;
        if (real[j]) {
            D[j] = dist(s[j], qq, xx[id]);
            if (!is_finite(s[j])) ok = false;
            ++n_real;
        }
    }
    const bool whole_db = ids[kd - 1] < 0;
    const float B = bound(s[kd - 1], qq, xx_min);
    bool below = false;
    for (int j = 0; j < kd; ++j) {
        if (j < k && j >= n_real) { D_out[j] = FLT_MAX; I_out[j] = -1; }
        if (!real[j]) continue;
        const int r = rank_of(D, ids, real, kd, j);
        if (r < k) { D_out[r] = D[j]; I_out[r] = ids[j]; }
        if (r == k - 1) below = D[j] < B;
    }
    return (ok && (whole_db || below)) ? 1 : 0;
}

}  // namespace l2ip
