// The discrepancy baselines (lib/baselines/discrepancy_baseline.py:164-242) for a list of knn_k from ONE pair matrix per query.
// k_discrepancy (api.hip) is the definition for a single k:
//   kq = k + is_train, kc_k = k + 1; the pairs are t = a * kc_k + b (dis) or t = a * kq + b (div); a pair is skipped by its
//   indices alone (Im[a] < 0; dis: the cache entry < 0 or == Im[a]; div: Im[b] < 0); lane L adds its pairs L, L + 64, ... in
//   ascending order in float64; total and count go through the xor butterfly 32 .. 1; dis = total / count (NaN when count is
//   0), div = total / (k k), cast to float32.
// An exact top-k list is a prefix of every deeper one (the index's tie rule is total: distance, then row id) and a pair's
// distance is a pure function of its two rows, so the matrix at the largest k holds every smaller k's pairs with the same bits.
// This file is what the sweep adds to that: which rows a pair (a, b) reads, the lane-strided sum over a prefix of the matrix,
// and the final division.  Plain C++ for host and device: k_discrepancy_ks and lemon_discrepancy_ks_host (discrepancy_ks.hip)
// both run it, the host twin with the 64 lanes looped.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DSC_HD __host__ __device__ inline
#else
#define DSC_HD inline
#endif

namespace dsc {

constexpr int LANES = 64;
constexpr int MAX_W = 64;                                // rows and columns of a pair matrix: kmax + 1 <= LEMON_MAX_K

// matrix width: dis kqmax x (kmax + 1), div kqmax x kqmax
DSC_HD int width(int method, int kmax, int kqmax) { return method == 0 ? kmax + 1 : kqmax; }

// The rows of pair (a, b) of the query whose text neighbours are im[0 .. kqmax).  Returns whether the pair counts; then *r0 is
// a database row and *r1 a database row (div) or -1 for the query's own row (dis).  Ic: the database's own text neighbours,
// row pitch kc (dis only).
DSC_HD bool pair_rows(int method, const int64_t *im, const int64_t *Ic, int kc, int a, int b, int64_t *r0, int64_t *r1) {
    const int64_t j = im[a];
    if (j < 0) return false;
    if (method == 0) {
        const int64_t l = Ic[j * kc + b];
        if (l < 0 || l == j) return false;
        *r0 = l; *r1 = -1;
    } else {
        const int64_t l = im[b];
        if (l < 0) return false;
        *r0 = j; *r1 = l;
    }
    return true;
}

// activity of row a of the matrix, bit b = pair (a, b) counts
DSC_HD uint64_t row_mask(int method, const int64_t *im, const int64_t *Ic, int kc, int a, int W) {
    uint64_t bits = 0;
    int64_t r0, r1;
    for (int b = 0; b < W; ++b)
        if (pair_rows(method, im, Ic, kc, a, b, &r0, &r1)) bits |= (uint64_t)1 << b;
    return bits;
}

// What lane `lane` of k_discrepancy adds up for one k: the pairs t = lane, lane + 64, ... of the rows x cols prefix of the
// matrix M (row pitch W), ascending, in float64.
DSC_HD void lane_sum(const float *M, const uint64_t *act, int W, int rows, int cols, int lane, double *total, int *count) {
    double s = 0.0;
    int c = 0;
    const int pairs = rows * cols;
    for (int t = lane; t < pairs; t += LANES) {
        const int a = t / cols, b = t - a * cols;
        if ((act[a] >> b) & 1) { s += (double)M[a * W + b]; ++c; }
    }
    *total = s; *count = c;
}

DSC_HD float finish(int method, double total, int count, int k) {
    return method == 0 ? (float)(count ? total / (double)count : (double)__builtin_nanf(""))
                       : (float)(total / ((double)k * (double)k));
}

// the xor butterfly 32 .. 1 over 64 looped lanes; lane 0 holds what the wave's lane 0 holds
inline void butterfly_host(double *total, int *count) {
    for (int off = 32; off > 0; off >>= 1) {
        double t2[LANES];
        int c2[LANES];
        for (int l = 0; l < LANES; ++l) { t2[l] = total[l] + total[l ^ off]; c2[l] = count[l] + count[l ^ off]; }
        for (int l = 0; l < LANES; ++l) { total[l] = t2[l]; count[l] = c2[l]; }
    }
}

}  // namespace dsc
