// common.hpp -- shared host/device helpers of liblemon_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <float.h>
#include "../../include/lemon_hip.h"
#include "attention_plan.hpp"
#include "index_ws.hpp"
#include <initializer_list>
#include <vector>
#include <utility>
#include <mutex>

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- error plumbing -------------------------------------------------------------
void lemon_set_error(const char *fmt, ...);

#define LEMON_HIP_CHECK(expr)                                                              \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            lemon_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LEMON_E_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define LEMON_REQUIRE(cond, msg)                                                           \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            lemon_set_error("invalid argument: %s (%s)", msg, #cond);                      \
            return LEMON_E_INVALID;                                                        \
        }                                                                                  \
    } while (0)

// Caller-owned embedding / query rows: with d % 4 == 0 some kernels behind the search read them 16 bytes at a time on the
// strength of d alone (exact_score and the staged k_bf16_final in knn_bf16.hip), so such rows must start on a 16-byte
// boundary.  With d % 4 != 0 every kernel walks rows one float at a time and any float pointer will do.
static inline bool rows_vector_safe(const float *p, int d) { return (d & 3) != 0 || (((uintptr_t)p) & 15) == 0; }
// The STAGED forms of the pair-distance kernels (chain_dist_wave) fetch rows 16 bytes at a time: d % 4 == 0 and every row
// array the kernel reads (a null one is not read) on a 16-byte boundary; otherwise every lane walks its rows from global.
static inline bool rows_staged(int d, std::initializer_list<const float *> rows) {
    uintptr_t bits = 0;
    for (const float *p : rows) bits |= (uintptr_t)p;
    return (d & 3) == 0 && (bits & 15) == 0;
}

// ---- index object ---------------------------------------------------------------
// Data layout in HBM (DESIGN.md "Data layout"):
//   x     [cap, d]        row-major copy of what the caller added (gathers, exact re-rank)
//   xp    [cap_pad, dpad] same rows, zero padded to dpad = ceil64(d) columns and with every
//                         group of 8 consecutive k stored as [k0 k2 k4 k6 | k1 k3 k5 k7] so
//                         that one 16-B LDS read feeds four v_mfma_f32_32x32x2_f32 steps in
//                         ascending-k order (cap_pad = ceil128(cap), pad rows are zero)
//   xnorm [cap_pad]       dot(x,x) (chain numerics), used by the L2 epilogue
struct lemon_index {
    int metric;
    int d, dpad;
    int device;
    int algo;
    int64_t n, cap;       // rows stored / rows allocated (cap is a multiple of 128)
    float *x, *xp, *xnorm;
    // every device buffer that is grown on demand, under the rule of index_ws.hpp (DESIGN.md "Index buffers"):
    //   XH, XH_STATS, XN2MAX  one group, built lazily by the filter scan (knn_bf16.hip): [cap, dpad_h] 16-bit (RNE) copy of x;
    //             [2, cap] measured ||x-xh||^2 and ||xh||^2 per row; float bits of max dot(x,x), max ||x-xh||^2, max ||xh||^2
    //   XNRANGE   float bits: min and max of xnorm[0 .. n) for the metric sweep (metric_sweep.hip)
    //   WS_QP, WS_QNORM  one group: [ws_q] staged query rows of ws_qp_row_bytes each; [3, ws_q] norms + two spare columns
    //   WS_CAND   [rows, CAND_CAP] candidates (one 128-row region per scan workgroup)
    //   WS_PART   [splits, ws_q, LEMON_MAX_K] lists to merge
    //   WS_STATE  per-lane scan state carried across database chunks + the list counts of k_bf16_final
    //   WS_D, WS_I  one group of equal element counts: the neighbour workspace of the two-sided search and the discrepancy baselines
    //   WS_DD, WS_DDQ  query de-duplication (dedup.hip): its arrays; the gathered representative queries + their results
    //   PLAN0 ..  the device side of plan_slots[0 .. 3]
    enum Buf { XH, XH_STATS, XN2MAX, XNRANGE, WS_QP, WS_QNORM, WS_CAND, WS_PART, WS_STATE, WS_D, WS_I, WS_DD, WS_DDQ, PLAN0,
               N_BUFS = PLAN0 + 4 };
    LemonBuf buf[N_BUFS];
    template <typename T> T *at(int which) const { return reinterpret_cast<T *>(buf[which].p); }
    int64_t xh_rows;      // rows of XH that are up to date
    int dpad_h;           // column pitch of XH (0 until the 16-bit copy exists)
    int64_t xnrange_rows; // 1 + the n XNRANGE was reduced at (0: never), so every add makes it stale
    int64_t ws_q;         // query rows WS_QP / WS_QNORM are sized for (the stride of WS_QNORM's three columns)
    int64_t ws_qp_row_bytes;  // bytes per staged query row WS_QP is sized for
    // fp32 scan: segment plans on the device (knn_f32.hip), a few recent ones -- a pipeline alternates between its train /
    // val / test query counts -- under all the segment planner reads: the (panels, tiles) shape, the resident slots and
    // the two knobs.  `host` keeps the upload's source alive (stream-ordered copy).
    struct PlanSlot {
        int panels, tiles, slots, xcds, seg_cost, grid, splits, pieces_off, segs_off;
        unsigned long long stamp; std::vector<int> *host;
    } plan_slots[4];
    unsigned long long plan_clock;
    lemon_search_info_t last;
    const char *last_kernel;  // family name of the last search's dominant scan kernel (static string; null before any search)
    int wide_filter;      // 1: widths 769..1280 take the register-resident pitches 1024 / 1280 (k_scan_f16_qsw, knn_bf16.hip)
    // LEMON_ALGO_AUTO decision cache (valid while auto_n == n)
    int auto_algo;
    int64_t auto_n;
    // query de-duplication (dedup.hip): 0 off, 1 auto.  Written by lemon_index_create and lemon_index_set_query_dedup only:
    // a call that must not fold says so in its arguments (lemon_search_internal)
    int qdedup;
    // optional scan-kernel timing (lemon_index_set_profiling)
    int profiling;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> *prof_events;
    double prof_flops, prof_bytes;
};

// the rule of index_ws.hpp on the device: growth synchronises `s`, the stream of the call that grows
struct LemonHipDev {
    hipStream_t s;
    bool sync() { return hipStreamSynchronize(s) == hipSuccess; }
    bool alloc(void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }
    void free(void *p) { (void)hipFree(p); }
};
// every member of an all-or-nothing group of (which, bytes) at its size or more; `what` names the workspace in lemon_last_error
inline int lemon_reserve_group(lemon_index *idx, std::initializer_list<std::pair<int, size_t>> want, hipStream_t stream, const char *what) {
    LemonBuf *bufs[lemon_ws::MAX_GROUP];
    size_t bytes[lemon_ws::MAX_GROUP], total = 0;
    int n = 0;
    for (const auto &w : want) { bufs[n] = &idx->buf[w.first]; bytes[n++] = w.second; total += w.second; }
    LemonHipDev dev{stream};
    const lemon_ws::Result r = lemon_ws::reserve_group(dev, bufs, bytes, n);
    if (r == lemon_ws::OK) return LEMON_OK;
    const bool nomem = r == lemon_ws::NO_MEMORY;
    lemon_set_error("%s: %s (%zu bytes)", what, nomem ? "allocation failed" : "stream synchronisation failed", total);
    return nomem ? LEMON_E_NOMEM : LEMON_E_HIP;
}
inline int lemon_reserve(lemon_index *idx, int which, size_t bytes, hipStream_t stream, const char *what) {
    return lemon_reserve_group(idx, {{which, bytes}}, stream, what);
}
// free and empty; the caller has synchronised whatever may still read the buffer
inline void lemon_release(lemon_index *idx, int which) {
    LemonHipDev dev{nullptr};
    lemon_ws::release(dev, idx->buf[which]);
}
// WS_D / WS_I at `elems` elements each
inline int lemon_reserve_nb(lemon_index *idx, int64_t elems, hipStream_t stream) {
    return lemon_reserve_group(idx, {{lemon_index::WS_D, (size_t)elems * sizeof(float)}, {lemon_index::WS_I, (size_t)elems * sizeof(int64_t)}},
                               stream, "neighbour workspace");
}

// bracket a kernel launch with events when profiling is on
struct LemonProfScope {
    lemon_index *idx; hipStream_t s; hipEvent_t a, b; bool on;
    LemonProfScope(lemon_index *i, hipStream_t st, double flops, double bytes) : idx(i), s(st), on(false) {
        if (!i->profiling) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        on = true;
        (void)hipEventRecord(a, s);
        i->prof_flops += flops; i->prof_bytes += bytes;
    }
    ~LemonProfScope() {
        if (!on) return;
        (void)hipEventRecord(b, s);
        idx->prof_events->push_back(std::make_pair(a, b));
    }
};

// ---- key packing: bigger key == better candidate ----------------------------------
// hi 32 bits: order-preserving map of the float score (to MAXIMISE), lo 32 bits: ~index so
// that, at equal score, the LOWER database index wins.  key 0 is "no candidate".
__host__ __device__ inline u32 lemon_f2ord(float f) {
    u32 u;
#ifdef __HIP_DEVICE_COMPILE__
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float lemon_ord2f(u32 o) {
    u32 u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
#ifdef __HIP_DEVICE_COMPILE__
    f = __uint_as_float(u);
#else
    memcpy(&f, &u, 4);
#endif
    return f;
}
__host__ __device__ inline u64 lemon_make_key(float score, u32 idx) {
    return ((u64)lemon_f2ord(score) << 32) | (u64)(0xffffffffu - idx);
}
__host__ __device__ inline float lemon_key_score(u64 key) { return lemon_ord2f((u32)(key >> 32)); }
__host__ __device__ inline u32 lemon_key_index(u64 key) { return 0xffffffffu - (u32)(key & 0xffffffffu); }

#define LEMON_CAND_CAP 256 // candidate slots per query in the scan workspace
// LayerNorm fold (lemon_linear_f16x3t_ln): the folded GEMM's rounding error grows with sqrt(1 + mean^2 / var) of a row; rows
// beyond |mean| rstd = this get a NaN row affine -> a non-finite output row -> the caller's range fallback re-embeds the
// micro-batch with LayerNorm kernels (pipeline.Embedder), so the fold never silently loses accuracy
#define LEMON_LN_FOLD_MAX_SHIFT 8.0f
#define LEMON_DEDUP_MIN_NQ 1024 // query de-duplication is attempted from this many queries on

// internal entry points shared between translation units
// may_dedup: this call may fold identical query rows, if the handle's setting says so too (idx->qdedup && may_dedup)
int lemon_search_internal(lemon_index_t *idx, const float *q_dev, int64_t nq, int k,
                          float *D_dev, int64_t *I_dev, hipStream_t stream, bool may_dedup = true);
int lemon_rowdot_chain(const float *a, const float *b, int64_t n, int d, float *out, hipStream_t s);
// K4, the neighbour finalisation of lemon_neighbors (api.hip), shared with lemon_neighbors_metrics (metric_sweep.hip)
struct NbParams {
    const float *img_tr, *txt_tr, *dists_tr, *q_img, *q_txt;
    const float *Dn, *Dm;       // [nq, ks] raw search output (ks: the pitch of a row; k + off <= ks columns are read)
    const int64_t *In, *Im;
    const uint8_t *in_db;
    const int32_t *tr_lab, *q_lab;
    float *D_n, *dists_n, *dists_tr_n, *D_m, *dists_m, *dists_tr_m;
    int64_t *I_n, *I_m;
    int64_t nq;
    int d, k, ks, metric, drop_self, discrete;
};
int lemon_neighbors_finalize(const NbParams &p, hipStream_t stream);
// The two-sided search behind lemon_neighbors and lemon_neighbors_metrics (api.hip).  TwoSided: the arguments both are given.
// _check: the handles and counts (the entry's own checks follow it).  _search: checks the query rows and labels, reserves the
// image handle's neighbour workspace at `elems` elements and searches both sides at kd into its front, [2][nq, kd], image side
// first: the image side never de-duplicated, the text side as its handle says (nq == 0: checks only).  lemon_nb_params: the
// fields of NbParams that do not depend on the metric or on where the lists and the outputs are.
struct TwoSided {
    lemon_index_t *img, *txt;
    const float *q_img, *q_txt;
    int64_t nq;
    int k, drop_self, discrete;
    const uint8_t *in_db; const int32_t *tr_lab, *q_lab;
};
int lemon_two_sided_check(const TwoSided &c);
int lemon_two_sided_search(const TwoSided &c, int kd, int64_t elems, hipStream_t stream);
NbParams lemon_nb_params(const TwoSided &c);
int lemon_dedup_queries(lemon_index_t *idx, const float *q_dev, int64_t nq, hipStream_t stream, int64_t *U_host,
                        const int **rep_dev, const int **group_dev);
int lemon_gather_query_rows(const float *q_dev, const int *rep_dev, int64_t U, int d, float *out_dev, hipStream_t stream);
int lemon_expand_results(const float *Dr, const int64_t *Ir, const int *group_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                         hipStream_t stream);
// ---- attention: what its three units share (attention_plan.hpp decides, each unit launches from its own table) ----
// the calling thread's knobs and the reported name of the kernel it launched last ("" before any launch): attention.hip
struct LemonAttnThread { lemon_attn_plan::Knobs knobs; const char *last_kernel; };
LemonAttnThread &lemon_attention_thread();
inline int lemon_attention_refuse(lemon_attn_plan::Refusal why) {
    lemon_set_error("%s", lemon_attn_plan::MESSAGES[why]);
    return lemon_attn_plan::E_INVALID;
}
// Launch a unit's kernels[4 * slot + split] as the plan says.  Dynamic LDS beyond 64 KB needs
// hipFuncAttributeMaxDynamicSharedMemorySize per DEVICE and per kernel: attr_set holds one row of flags (a flag per device index)
// per kernel of the table, set under one lock in front of the kernel's first launch on the current device.
struct LemonLdsAttr { bool set[64]; };
inline std::mutex g_lemon_lds_attr_mu;
template <typename Kernel, typename... Args>
int lemon_attention_launch(const Kernel *kernels, LemonLdsAttr *attr_set, const lemon_attn_plan::Plan &p, int split, hipStream_t stream, Args... args) {
    const lemon_attn_plan::FormFacts &f = lemon_attn_plan::FACTS[p.form];
    const int i = 4 * f.slot + split;
    if (f.attr) {
        int dev = 0;
        LEMON_HIP_CHECK(hipGetDevice(&dev));
        LEMON_REQUIRE(dev >= 0 && dev < 64, "device index");
        std::lock_guard<std::mutex> lock(g_lemon_lds_attr_mu);
        if (!attr_set[i].set[dev]) {
            LEMON_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernels[i]), hipFuncAttributeMaxDynamicSharedMemorySize, f.attr));
            attr_set[i].set[dev] = true;
        }
    }
    hipLaunchKernelGGL(kernels[i], dim3(p.grid_x, p.grid_y), dim3(p.threads), p.lds, stream, args...);
    lemon_attention_thread().last_kernel = f.name[split];
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
// the launch of a plan whose form belongs to attention_hd.hip, for the entries of attention.hip (after their checks)
int lemon_attention_hdx(const lemon_attn_plan::Plan &p, int split, const float *qkv_dev, int seq_len, int heads, int causal, float *out_dev,
                        hipStream_t stream);
