// Hyper-parameter grid of the LEMoN score, evaluated as ONE batch on the GPU (gfx950 only).
//
// run_lemon.py:319-384 -> maximize_metric (lib/metrics/utils.py:151-196) evaluates, for each of the
// 21*21*4*4 = 7056 grid points, scores = calc_scores_given_hparams_vectorized(val, hp) (:47-82) and
// optimize_f1_efficient(y, scores) (:286-296) = scipy.optimize.fminbound on t -> -F1(y, scores >= t)
// with xtol = 1e-8.  On the host that is one K5 launch + one device->host copy + ~35 numpy F1
// evaluations per grid point.  Here: kernel 1 fills scores[G, N] with exactly K5's arithmetic
// (float64, same expression order), kernel 2 runs one bounded-Brent search per grid point -- one
// wavefront each, a faithful restatement of scipy's _minimize_scalar_bounded in IEEE double (no FMA
// contraction inside the search; the score kernel keeps the default so that it matches k_score), F1 from integer counts -- and returns (F1, threshold) per grid point,
// bit-identical to the host path (tests/test_gpu_parity.py).  A non-finite score row yields F1 = 0, as the
// host objective does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "common.hpp"
#include "gridf1_brent.hpp"

namespace {

__global__ __launch_bounds__(256) void k_grid_scores(const float *__restrict__ d1, const float *__restrict__ Dn,
                                                     const float *__restrict__ trn, const float *__restrict__ dn,
                                                     const float *__restrict__ Dm, const float *__restrict__ trm,
                                                     const float *__restrict__ dm, int64_t n, int k,
                                                     const double *__restrict__ hp /* [G,6] */, double *__restrict__ score) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = blockIdx.y;
    const double beta = hp[6 * g], gamma = hp[6 * g + 1], t1n = hp[6 * g + 2], t2n = hp[6 * g + 3], t1m = hp[6 * g + 4],
                 t2m = hp[6 * g + 5];
    double sn = 0.0, sm = 0.0;
    for (int j = 0; j < k; ++j) {                        // identical to k_score (rowwise.hip)
        const int64_t o = i * (int64_t)k + j;
        sn += exp(-t1n * (double)Dn[o]) * exp(-t2n * (double)trn[o]) * (double)dn[o];
        sm += exp(-t1m * (double)Dm[o]) * exp(-t2m * (double)trm[o]) * (double)dm[o];
    }
    const double a = sn / (double)k, b = sm / (double)k;
    score[(int64_t)g * n + i] = (double)d1[i] + beta * a + gamma * b;
}

}  // namespace

extern "C" int lemon_grid_f1(const float *d1_dev, const float *D_n_dev, const float *dists_tr_n_dev, const float *dists_n_dev,
                             const float *D_m_dev, const float *dists_tr_m_dev, const float *dists_m_dev,
                             const uint8_t *y_dev, int64_t n, int k, const double *hp_dev, int G, double xtol, int maxfun,
                             double *scores_ws_dev, double *f1_dev, double *thres_dev, void *stream_) {
    LEMON_REQUIRE(n > 0 && k > 0 && G >= 0 && maxfun >= 1, "n > 0, k > 0, G >= 0, maxfun >= 1");
    if (G == 0) return LEMON_OK;
    LEMON_REQUIRE(G <= 65535, "at most 65535 grid points per call");
    LEMON_REQUIRE(d1_dev && D_n_dev && dists_tr_n_dev && dists_n_dev && D_m_dev && dists_tr_m_dev && dists_m_dev && y_dev &&
                      hp_dev && scores_ws_dev && f1_dev && thres_dev, "null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_grid_scores, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, stream, d1_dev, D_n_dev,
                       dists_tr_n_dev, dists_n_dev, D_m_dev, dists_tr_m_dev, dists_m_dev, n, k, hp_dev, scores_ws_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    const double sqrt_eps = sqrt(2.2e-16), golden_mean = 0.5 * (3.0 - sqrt(5.0));
    hipLaunchKernelGGL(k_grid_brent, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, stream, scores_ws_dev, y_dev, n, G, xtol,
                       maxfun, sqrt_eps, golden_mean, f1_dev, thres_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
