// metrics.eval_metrics on the device (gfx950 only, opt-in): lemon_eval_metrics.
//
// Behind the hyper-parameter search a run evaluates its score once on the free validation rows and once more on every split, in
// scipy and sklearn on the host (lib/metrics/utils.py:414-441): 68 ms a cell at the headline sizes, most of it gaussian_kde.
// Everything those calls return is a function of one descending sort of (score, label) plus 1 000 x n Gaussian kernel
// evaluations, so S segments of one score array are served by one launch sequence on the caller's stream:
//   k_eval_offsets     segment bounds for the sort, the density slot of every free segment
//   hipcub             segmented descending radix sort of (score, label); one plain radix sort when S == 1
//   k_eval_curve       one workgroup of 1 024 lanes a segment: positives, finiteness, then a walk over the sorted rows 1 024
//                      at a time -- prefix counts of positives into the workspace (one block scan), the end of the group in
//                      front of every row (one block max-scan), the AUPRC term and the integer pair count of every group --
//                      and for a free segment np.mean in numpy's order (a lane per 8 192-row chunk), the variance and the
//                      KDE's bandwidth
//   k_eval_density     free segments: a lane per grid point, four workgroups of 256 a segment; the rows stream through LDS
//                      1 024 at a time, already divided by the bandwidth, in the segment's original order from row 0
//   k_eval_thresholds  free segments: the 100 candidates of optimize_f1 on 100 lanes (binary search + one prefix lookup each);
//                      bisect / fminbound on one lane of the second wave, the extrema and their median on one lane of the third
//   k_eval_counts      a lane per (segment, threshold): one binary search, four counts
// Recorded on an MI355X (tools/eval_metrics_time.py, profiles/eval_metrics/): a cell of 5 000 / 40 000 / 5 000 rows (four
// segments) takes 3.5 ms through ops.eval_metrics against 68 ms of scipy / sklearn on the same box; 250 / 2 000 / 250: 0.43 ms
// against 19 ms; one fixed segment of 3 M rows 0.14 s against 2.1 s.
// The arithmetic and every summation order are csrc/eval_metrics_core.hpp's; the host twin (lemon_eval_metrics_host) runs the
// same header with the lanes looped and std::stable_sort; it exists for the tests, no product path calls it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <math.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "eval_metrics_core.hpp"

static_assert(sizeof(LemonEvalSegment) == sizeof(evm::Segment) && sizeof(evm::Segment) == 32, "LemonEvalSegment layout");
static_assert(sizeof(LemonEvalRecord) == sizeof(evm::Record) && sizeof(evm::Record) == 152, "LemonEvalRecord layout");
static_assert(LEMON_EVAL_NONFINITE == evm::ST_NONFINITE && LEMON_EVAL_ONE_CLASS == evm::ST_ONE_CLASS &&
              LEMON_EVAL_FEW_ROWS == evm::ST_FEW_ROWS && LEMON_EVAL_ZERO_VARIANCE == evm::ST_ZERO_VAR &&
              LEMON_EVAL_SOURCE == evm::ST_SOURCE, "status ids");

namespace {

constexpr int EVM_T = evm::THREADS, EVM_W = evm::WAVES;
constexpr int DENS_T = 256, DENS_TILE = 1024;
constexpr int DENS_BLOCKS = (evm::N_GRID + DENS_T - 1) / DENS_T;

struct SegState { evm::Kde kde; int64_t pos; int32_t status, slot; };      // what the later kernels need of k_eval_curve

struct EvalWs {
    double *ss;          // [total] scores, every segment sorted descending in place of its rows
    uint8_t *ys;         // [total] the labels beside them
    int32_t *cp;         // [total] positives among the sorted rows of the segment up to and including this one
    int32_t *begin, *end;   // [S] segment bounds for the sort
    SegState *state;     // [S]
    double *dens;        // [S_free, N_GRID]
    void *cub;
    size_t cub_bytes, total;
};

inline size_t ev_align(size_t v) { return (v + 255) & ~(size_t)255; }

int ev_carve(int64_t total, int S, int S_free, void *ws, EvalWs *w) {
    // the temporary storage of the one sort the call makes; the segmented query needs a HIP device, the plain one does not
    size_t t = 0;
    const hipError_t asked = S == 1
        ? hipcub::DeviceRadixSort::SortPairsDescending(nullptr, t, (const double *)nullptr, (double *)nullptr, (const uint8_t *)nullptr,
                                                       (uint8_t *)nullptr, (int)total, 0, 64, (hipStream_t)0)
        : hipcub::DeviceSegmentedRadixSort::SortPairsDescending(nullptr, t, (const double *)nullptr, (double *)nullptr,
                                                                (const uint8_t *)nullptr, (uint8_t *)nullptr, (int)total, S,
                                                                (const int32_t *)nullptr, (const int32_t *)nullptr, 0, 64, (hipStream_t)0);
    if (asked != hipSuccess) {
        lemon_set_error("hipcub radix sort size query failed: %s", hipGetErrorString(asked));
        return LEMON_E_HIP;
    }
    char *p = (char *)ws;
    w->ss = (double *)p; p += ev_align((size_t)total * 8);
    w->ys = (uint8_t *)p; p += ev_align((size_t)total);
    w->cp = (int32_t *)p; p += ev_align((size_t)total * 4);
    w->begin = (int32_t *)p; p += ev_align((size_t)S * 4);
    w->end = (int32_t *)p; p += ev_align((size_t)S * 4);
    w->state = (SegState *)p; p += ev_align((size_t)S * sizeof(SegState));
    w->dens = (double *)p; p += ev_align((size_t)S_free * evm::N_GRID * 8);
    w->cub = p;
    w->cub_bytes = ev_align(t);
    w->total = (size_t)(p - (char *)ws) + w->cub_bytes;
    return LEMON_OK;
}

int ev_check_shape(int64_t total, int S) {
    LEMON_REQUIRE(S >= 1 && S <= 65535, "1 <= S <= 65535");
    LEMON_REQUIRE(total >= 1 && total < ((int64_t)1 << 31), "total must lie in [1, 2^31)");
    return LEMON_OK;
}

// segs on the host; *n_free = the number of free segments
int ev_check_segments(const evm::Segment *segs, int S, int64_t total, int *n_free) {
    std::vector<int> order((size_t)S);
    std::iota(order.begin(), order.end(), 0);
    int free_segs = 0;
    for (int s = 0; s < S; ++s) {
        const evm::Segment &g = segs[s];
        LEMON_REQUIRE(g.offset >= 0 && g.n >= 1, "segment: offset >= 0, n >= 1");
        LEMON_REQUIRE(g.offset <= total && g.n <= total - g.offset, "segment: passes the end of score");
        LEMON_REQUIRE(g.thres_from == -1 || (g.thres_from >= 0 && g.thres_from < S && segs[g.thres_from].thres_from == -1),
                      "segment: thres_from is -1 or the index of a free segment");
        free_segs += g.thres_from == -1;
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return segs[a].offset < segs[b].offset; });
    for (int i = 0; i + 1 < S; ++i)
        LEMON_REQUIRE(segs[order[i]].offset + segs[order[i]].n <= segs[order[i + 1]].offset, "segments overlap");
    *n_free = free_segs;
    return LEMON_OK;
}

// ------------------------------------------------------------------------------------------------ workgroup primitives
// every thread of the workgroup calls these; `slots` is reused behind the trailing barrier
template <class T> __device__ T block_sum(T v, T *slots) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) slots[w] = v;
    __syncthreads();
    T tot = slots[0];
    for (int x = 1; x < nw; ++x) tot += slots[x];
    __syncthreads();
    return tot;
}
// the double sum in the order of eval_metrics_core.hpp: butterfly, then the waves from wave 0 (blockDim.x == evm::THREADS)
__device__ double block_sum_ordered(double v, double *slots) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    const double tot = evm::reduce_waves(slots);
    __syncthreads();
    return tot;
}
// inclusive scan over the workgroup in thread order; *total = the scan's last value
template <class T, class Op> __device__ T block_scan(T v, Op op, T *slots, T *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    if (lane == 63) slots[w] = v;
    __syncthreads();
    T tot = slots[0];
    for (int x = 1; x < nw; ++x) {
        if (x == w) v = op(tot, v);
        tot = op(tot, slots[x]);
    }
    __syncthreads();
    *total = tot;
    return v;
}

struct EvalArgs {
    const double *score;
    const uint8_t *y;
    const evm::Segment *segs;
    int S;
    EvalWs w;
    double sqrt_eps, golden_mean;
    evm::Record *out;
};

__global__ __launch_bounds__(256) void k_eval_offsets(EvalArgs a) {
    for (int s = threadIdx.x; s < a.S; s += blockDim.x) {
        a.w.begin[s] = (int32_t)a.segs[s].offset;
        a.w.end[s] = (int32_t)(a.segs[s].offset + a.segs[s].n);
    }
    if (threadIdx.x == 0) {
        int slot = 0;
        for (int s = 0; s < a.S; ++s) a.w.state[s].slot = a.segs[s].thres_from == -1 ? slot++ : -1;
    }
}

__global__ __launch_bounds__(EVM_T) void k_eval_curve(EvalArgs a) {
#pragma clang fp contract(off)
    __shared__ double sm_d[EVM_T];
    __shared__ long long sm_i[EVM_W];
    __shared__ unsigned long long sm_k[EVM_W], sm_last[EVM_W];
    __shared__ double sm_w[EVM_W];
    const int sidx = blockIdx.x, tid = threadIdx.x;
    const evm::Segment g = a.segs[sidx];
    const int64_t n = g.n;
    const bool free_seg = g.thres_from == -1;
    const double *orig = a.score + g.offset, *ss = a.w.ss + g.offset;
    const uint8_t *yo = a.y + g.offset, *ys = a.w.ys + g.offset;
    int32_t *cp = a.w.cp + g.offset;

    long long pos = 0, bad = 0;
    for (int64_t i = tid; i < n; i += EVM_T) {
        bad += !evm::is_finite(orig[i]);
        pos += yo[i] != 0;
    }
    pos = block_sum(pos, sm_i);
    bad = block_sum(bad, sm_i);

    double auprc = 0.0;
    long long u2 = 0;
    const bool both = pos > 0 && pos < n;
    if (!bad) {                                          // workgroup-uniform
        long long carry_cp = 0;
        unsigned long long carry_key = 0;                // (rows << 32 | positives) at the last group end so far
        double ap = 0.0;
        for (int64_t base = 0; base < n; base += EVM_T) {
            const int64_t i = base + tid;
            const bool active = i < n;
            long long tot_cp;
            const long long cpi = carry_cp + block_scan<long long>(active && ys[i] != 0 ? 1 : 0,
                                                                    [](long long x, long long y) { return x + y; }, sm_i, &tot_cp);
            if (active) cp[i] = (int32_t)cpi;
            const bool is_end = active && (i == n - 1 || ss[i] != ss[i + 1]);
            const unsigned long long key = is_end ? ((unsigned long long)(i + 1) << 32 | (unsigned long long)cpi) : 0ull;
            unsigned long long tot_key;
            const unsigned long long incl = block_scan<unsigned long long>(
                key, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; }, sm_k, &tot_key);
            // the key in front of this lane: the inclusive maximum of the lane before, or the carry
            unsigned long long before = __shfl_up(incl, 1);
            if ((tid & 63) == 0) before = 0;
            if ((tid & 63) == 63) sm_last[tid >> 6] = incl;
            __syncthreads();
            if ((tid & 63) == 0 && tid > 0) before = sm_last[(tid >> 6) - 1];
            __syncthreads();
            if (before < carry_key) before = carry_key;
            if (is_end && both) {
                const int64_t prev_rows = (int64_t)(before >> 32), prev_tp = (int64_t)(before & 0xffffffffull);
                ap = ap + evm::auprc_term(i + 1, cpi, prev_tp, pos);
                u2 += evm::auroc_term(i + 1, cpi, prev_rows, prev_tp);
            }
            carry_cp += tot_cp;
            if (tot_key > carry_key) carry_key = tot_key;
        }
        auprc = block_sum_ordered(ap, sm_w);
        u2 = block_sum(u2, sm_i);
    }

    // a free segment: np.mean in numpy's order, the variance around it, the bandwidth
    evm::Kde kde{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool kde_ok = true;
    if (!bad && free_seg && n >= 2) {
        double tot = 0.0;                                // thread 0's
        const int64_t chunks = evm::np_chunks(n);
        for (int64_t cb = 0; cb < chunks; cb += EVM_T) {
            if (cb + tid < chunks) sm_d[tid] = evm::np_chunk_sum(orig, n, cb + tid);
            __syncthreads();
            if (tid == 0)
                for (int64_t c = 0; c < EVM_T && cb + c < chunks; ++c) tot = tot + sm_d[c];
            __syncthreads();
        }
        if (tid == 0) sm_w[0] = tot / (double)n;
        __syncthreads();
        const double mean = sm_w[0];
        __syncthreads();
        double sq = 0.0;
        for (int64_t i = tid; i < n; i += EVM_T) sq = sq + evm::sq_dev(orig[i], mean);
        const double sumsq = block_sum_ordered(sq, sm_w);
        kde_ok = evm::kde_setup(ss[n - 1], ss[0], mean, sumsq, n, kde);
    }
    if (tid == 0) {
        const int status = evm::segment_status(free_seg, bad != 0, n, pos, kde_ok);
        evm::Record r;
        const double nan = __builtin_nan("");
        r.auroc = status == evm::ST_OK ? evm::auroc_from(u2, pos, n) : nan;
        r.auprc = status == evm::ST_OK ? auprc : nan;
        for (int k = 0; k < 3; ++k) {
            r.thres[k] = nan;
            for (int c = 0; c < 4; ++c) r.counts[k][c] = 0;
        }
        r.status = status; r.kde_branch = 0; r.bisect_fallback = 0; r.pad = 0;
        a.out[sidx] = r;
        a.w.state[sidx].kde = kde;
        a.w.state[sidx].pos = pos;
        a.w.state[sidx].status = status;
    }
}

__global__ __launch_bounds__(DENS_T) void k_eval_density(EvalArgs a) {
#pragma clang fp contract(off)
    __shared__ double u[DENS_TILE];
    const int sidx = blockIdx.y, tid = threadIdx.x;
    const evm::Segment g = a.segs[sidx];
    const SegState st = a.w.state[sidx];
    if (g.thres_from != -1 || st.status != evm::ST_OK) return;      // workgroup-uniform
    const double *orig = a.score + g.offset;
    const int j = blockIdx.x * DENS_T + tid;
    const bool mine = j < evm::N_GRID;
    const double xj = mine ? evm::kde_point(st.kde, j) : 0.0;
    double acc = 0.0;
    for (int64_t base = 0; base < g.n; base += DENS_TILE) {
        const int cnt = (int)(g.n - base < DENS_TILE ? g.n - base : DENS_TILE);
        for (int k = tid; k < cnt; k += DENS_T) u[k] = orig[base + k] / st.kde.h;
        __syncthreads();
        if (mine)
            for (int k = 0; k < cnt; ++k) acc = acc + evm::kde_term(st.kde, u[k], xj);
        __syncthreads();
    }
    if (mine) a.w.dens[(int64_t)st.slot * evm::N_GRID + j] = acc;
}

__global__ __launch_bounds__(256) void k_eval_thresholds(EvalArgs a) {
    __shared__ double f1[evm::N_CAND];
    const int sidx = blockIdx.x, tid = threadIdx.x;
    const evm::Segment g = a.segs[sidx];
    const SegState st = a.w.state[sidx];
    if (g.thres_from != -1 || st.status != evm::ST_OK) return;      // workgroup-uniform
    const evm::Sorted v{a.w.ss + g.offset, a.w.cp + g.offset, g.n};
    if (tid < evm::N_CAND) f1[tid] = evm::candidate_f1(v, tid);
    __syncthreads();
    evm::Record *r = a.out + sidx;
    if (tid == 0) r->thres[0] = evm::linspace_at(v.s[v.n - 1], v.s[0], evm::N_CAND, evm::pick_candidate(f1));
    if (tid == 64) {
        int fallback = 0;
        r->thres[1] = evm::prev_threshold(v, g.prevalence, a.sqrt_eps, a.golden_mean, fallback);
        r->bisect_fallback = fallback;
    }
    if (tid == 128) {
        int branch = 0;
        r->thres[2] = evm::kde_threshold(st.kde, a.w.dens + (int64_t)st.slot * evm::N_GRID, branch);
        r->kde_branch = branch;
    }
}

__global__ __launch_bounds__(256) void k_eval_counts(EvalArgs a) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= 3 * a.S) return;
    const int sidx = gid / 3, k = gid % 3;
    const evm::Segment g = a.segs[sidx];
    if (a.w.state[sidx].status != evm::ST_OK) return;
    evm::Record *r = a.out + sidx;
    double t;
    if (g.thres_from == -1) {
        t = r->thres[k];
    } else {
        if (a.w.state[g.thres_from].status != evm::ST_OK) {          // three lanes write the same values
            r->status = evm::ST_SOURCE;
            r->auroc = r->auprc = __builtin_nan("");
            return;
        }
        t = a.out[g.thres_from].thres[k];
        r->thres[k] = t;
    }
    const evm::Sorted v{a.w.ss + g.offset, a.w.cp + g.offset, g.n};
    int64_t c[4];
    evm::counts_at(v, t, c);
    for (int x = 0; x < 4; ++x) r->counts[k][x] = c[x];
}

// the free-segment set-up and the density of the host twin: np.mean, the variance in the lanes' order, one grid point at a time
bool ev_host_kde(const double *orig, int64_t n, double lo, double hi, evm::Kde &kde) {
    const double mean = evm::np_mean(orig, n);
    evm::LaneSums sq;
    for (int64_t i = 0; i < n; ++i) sq.add(i, evm::sq_dev(orig[i], mean));
    return evm::kde_setup(lo, hi, mean, sq.total(), n, kde);
}
void ev_host_density(const double *orig, int64_t n, const evm::Kde &kde, double *dens) {
#pragma clang fp contract(off)
    std::vector<double> u((size_t)n);
    for (int64_t i = 0; i < n; ++i) u[i] = orig[i] / kde.h;
    for (int j = 0; j < evm::N_GRID; ++j) {
        const double xj = evm::kde_point(kde, j);
        double acc = 0.0;
        for (int64_t i = 0; i < n; ++i) acc = acc + evm::kde_term(kde, u[i], xj);
        dens[j] = acc;
    }
}

double ev_sqrt_eps() { return sqrt(2.2e-16); }
double ev_golden_mean() { return 0.5 * (3.0 - sqrt(5.0)); }

}  // namespace

extern "C" int64_t lemon_eval_metrics_workspace_bytes(int64_t total, int S, int S_free) {
    if (int rc = ev_check_shape(total, S)) return rc;
    if (!(S_free >= 0 && S_free <= S)) {
        lemon_set_error("invalid argument: 0 <= S_free <= S");
        return LEMON_E_INVALID;
    }
    EvalWs w;
    if (int rc = ev_carve(total, S, S_free, nullptr, &w)) return rc;
    return (int64_t)w.total;
}

extern "C" int lemon_eval_metrics(const double *score, const uint8_t *y, int64_t total, const LemonEvalSegment *segs, int S,
                                  void *ws, int64_t ws_bytes, LemonEvalRecord *out, void *stream_) {
    if (int rc = ev_check_shape(total, S)) return rc;
    LEMON_REQUIRE(score && y && segs && ws && out, "null pointer");
    LEMON_REQUIRE(((uintptr_t)ws & 255) == 0, "workspace aligned to 256 bytes");
    hipStream_t stream = (hipStream_t)stream_;
    // the kernels index score, y and the workspace with the segments: they are checked here, before anything is launched
    std::vector<evm::Segment> segs_h((size_t)S);
    LEMON_HIP_CHECK(hipMemcpyAsync(segs_h.data(), segs, segs_h.size() * sizeof(evm::Segment), hipMemcpyDeviceToHost, stream));
    LEMON_HIP_CHECK(hipStreamSynchronize(stream));
    int n_free = 0;
    if (int rc = ev_check_segments(segs_h.data(), S, total, &n_free)) return rc;
    EvalArgs a;
    if (int rc = ev_carve(total, S, n_free, ws, &a.w)) return rc;
    LEMON_REQUIRE(ws_bytes >= (int64_t)a.w.total, "workspace smaller than lemon_eval_metrics_workspace_bytes(total, S, S_free)");
    a.score = score; a.y = y; a.segs = (const evm::Segment *)segs; a.S = S;
    a.sqrt_eps = ev_sqrt_eps(); a.golden_mean = ev_golden_mean();
    a.out = (evm::Record *)out;
    hipLaunchKernelGGL(k_eval_offsets, dim3(1), dim3(256), 0, stream, a);
    LEMON_HIP_CHECK(hipGetLastError());
    size_t tb = a.w.cub_bytes;
    const hipError_t sorted = S == 1
        ? hipcub::DeviceRadixSort::SortPairsDescending(a.w.cub, tb, score + segs_h[0].offset, a.w.ss + segs_h[0].offset,
                                                       y + segs_h[0].offset, a.w.ys + segs_h[0].offset, (int)segs_h[0].n, 0, 64,
                                                       stream)
        : hipcub::DeviceSegmentedRadixSort::SortPairsDescending(a.w.cub, tb, score, a.w.ss, y, a.w.ys, (int)total, S,
                                                                (const int32_t *)a.w.begin, (const int32_t *)a.w.end, 0, 64, stream);
    if (sorted != hipSuccess) {
        lemon_set_error("hipcub radix sort failed: %s", hipGetErrorString(sorted));
        return LEMON_E_HIP;
    }
    hipLaunchKernelGGL(k_eval_curve, dim3((unsigned)S), dim3(EVM_T), 0, stream, a);
    LEMON_HIP_CHECK(hipGetLastError());
    if (n_free > 0) {
        hipLaunchKernelGGL(k_eval_density, dim3(DENS_BLOCKS, (unsigned)S), dim3(DENS_T), 0, stream, a);
        LEMON_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_eval_thresholds, dim3((unsigned)S), dim3(256), 0, stream, a);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_eval_counts, dim3((unsigned)((3 * S + 255) / 256)), dim3(256), 0, stream, a);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

extern "C" int lemon_eval_metrics_host(const double *score, const uint8_t *y, int64_t total, const LemonEvalSegment *segs_, int S,
                                       LemonEvalRecord *out_) {
#pragma clang fp contract(off)
    if (int rc = ev_check_shape(total, S)) return rc;
    LEMON_REQUIRE(score && y && segs_ && out_, "null pointer");
    const evm::Segment *segs = (const evm::Segment *)segs_;
    evm::Record *out = (evm::Record *)out_;
    int n_free = 0;
    if (int rc = ev_check_segments(segs, S, total, &n_free)) return rc;
    std::vector<std::vector<double>> ss((size_t)S);
    std::vector<std::vector<int32_t>> cp((size_t)S);
    std::vector<int> status((size_t)S);
    const double nan = __builtin_nan("");
    for (int s = 0; s < S; ++s) {
        const evm::Segment &g = segs[s];
        const int64_t n = g.n;
        const double *orig = score + g.offset;
        const uint8_t *yo = y + g.offset;
        const bool free_seg = g.thres_from == -1;
        int64_t pos = 0;
        bool bad = false;
        for (int64_t i = 0; i < n; ++i) { bad |= !evm::is_finite(orig[i]); pos += yo[i] != 0; }
        evm::Record r;
        r.auroc = r.auprc = nan;
        for (int k = 0; k < 3; ++k) {
            r.thres[k] = nan;
            for (int c = 0; c < 4; ++c) r.counts[k][c] = 0;
        }
        r.kde_branch = r.bisect_fallback = r.pad = 0;
        double auprc = 0.0;
        int64_t u2 = 0;
        evm::Kde kde{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool kde_ok = true;
        if (!bad) {
            std::vector<int64_t> order((size_t)n);
            std::iota(order.begin(), order.end(), (int64_t)0);
            std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t z) { return orig[x] > orig[z]; });
            ss[s].resize((size_t)n); cp[s].resize((size_t)n);
            int64_t run = 0;
            for (int64_t i = 0; i < n; ++i) {
                ss[s][i] = orig[order[i]];
                run += yo[order[i]] != 0;
                cp[s][i] = (int32_t)run;
            }
            if (pos > 0 && pos < n) {
                evm::LaneSums ap;
                int64_t prev_rows = 0, prev_tp = 0;
                for (int64_t i = 0; i < n; ++i) {
                    if (!(i == n - 1 || ss[s][i] != ss[s][i + 1])) continue;
                    ap.add(i, evm::auprc_term(i + 1, cp[s][i], prev_tp, pos));
                    u2 += evm::auroc_term(i + 1, cp[s][i], prev_rows, prev_tp);
                    prev_rows = i + 1; prev_tp = cp[s][i];
                }
                auprc = ap.total();
            }
            if (free_seg && n >= 2) kde_ok = ev_host_kde(orig, n, ss[s][n - 1], ss[s][0], kde);
        }
        r.status = status[s] = evm::segment_status(free_seg, bad, n, pos, kde_ok);
        if (r.status == evm::ST_OK) {
            r.auroc = evm::auroc_from(u2, pos, n);
            r.auprc = auprc;
            if (free_seg) {
                const evm::Sorted v{ss[s].data(), cp[s].data(), n};
                double f1[evm::N_CAND];
                for (int i = 0; i < evm::N_CAND; ++i) f1[i] = evm::candidate_f1(v, i);
                r.thres[0] = evm::linspace_at(v.s[n - 1], v.s[0], evm::N_CAND, evm::pick_candidate(f1));
                int fallback = 0, branch = 0;
                r.thres[1] = evm::prev_threshold(v, g.prevalence, ev_sqrt_eps(), ev_golden_mean(), fallback);
                r.bisect_fallback = fallback;
                std::vector<double> dens((size_t)evm::N_GRID, 0.0);
                ev_host_density(orig, n, kde, dens.data());
                r.thres[2] = evm::kde_threshold(kde, dens.data(), branch);
                r.kde_branch = branch;
            }
        }
        out[s] = r;
    }
    for (int s = 0; s < S; ++s) {
        if (status[s] != evm::ST_OK) continue;
        const evm::Segment &g = segs[s];
        evm::Record &r = out[s];
        if (g.thres_from != -1) {
            if (status[g.thres_from] != evm::ST_OK) { r.status = evm::ST_SOURCE; r.auroc = r.auprc = nan; continue; }
            for (int k = 0; k < 3; ++k) r.thres[k] = out[g.thres_from].thres[k];
        }
        const evm::Sorted v{ss[s].data(), cp[s].data(), g.n};
        for (int k = 0; k < 3; ++k) evm::counts_at(v, r.thres[k], r.counts[k]);
    }
    return LEMON_OK;
}

extern "C" int lemon_eval_metrics_kde_host(const double *score, int64_t n, double *grid, double *dens) {
    LEMON_REQUIRE(score && grid && dens && n >= 2 && n < ((int64_t)1 << 31), "null pointer, 2 <= n < 2^31");
    double lo = score[0], hi = score[0];
    bool bad = false;
    for (int64_t i = 0; i < n; ++i) {
        bad |= !evm::is_finite(score[i]);
        lo = score[i] < lo ? score[i] : lo; hi = score[i] > hi ? score[i] : hi;
    }
    evm::Kde kde;
    LEMON_REQUIRE(!bad && ev_host_kde(score, n, lo, hi, kde), "finite scores of non-zero variance");
    for (int j = 0; j < evm::N_GRID; ++j) grid[j] = evm::linspace_at(lo, hi, evm::N_GRID, j);
    ev_host_density(score, n, kde, dens);
    return LEMON_OK;
}
