// scan_plan.hpp -- the host-side plan of the exact scan (lemon_search_f32, knn_f32.hip): how a query chunk is cut, whether its
// workgroups follow a segment plan or (panel, split) rectangles, the segment planner itself, and the per-launch settings.
// Plain C++: no HIP, no getenv, no function-local statics, so that the host compiler builds it -- with gcc under
// AddressSanitizer / UBSan for the fuzzer (tests/native/plan_fuzz.cpp, tests/test_sanitizers.py) -- and
// tests/test_knn_f32_plan_host.py checks it on the CPU against a table of recorded decisions.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "knn_bf16_plan.hpp"

struct LemonPlan {
    std::vector<int> seg_begin;      // [grid + 1]
    std::vector<int> pieces;         // [panels]
    std::vector<int> segs;           // 4 ints per segment
    int grid = 0, splits = 1;
};

// `c` = what a segment costs on top of its tiles (pipeline refill, the cold start of its candidate lists, the final
// selection), in tile times: shares are equal in COST, not in tiles -- a workgroup that collects four tails would
// otherwise finish 5 % after one that walks a single head (measured: lives 16.9 ms against 16.0-16.3 ms).
static inline void plan_group(const std::vector<int> &wgs, const std::vector<int> &pnls, int T, int c, std::vector<std::vector<int>> &wg_segs,
                       std::vector<int> &pieces) {
    const int m = (int)wgs.size(), n = (int)pnls.size();
    if (m == 0 || n == 0) return;
    const int64_t total = (int64_t)n * T;
    const int64_t u = (total + m - 1) / m;
    // budget per workgroup: tiles + c per segment; about one segment per panel and one more per workgroup boundary
    int64_t budget;
    std::vector<int64_t> room;
    auto put = [&](int w, int panel, int t0, int nt) {
        std::vector<int> &v = wg_segs[wgs[w]];
        v.push_back(panel); v.push_back(t0); v.push_back(nt); v.push_back(pieces[panel]++);
        room[w] -= nt + c;
    };
    std::vector<std::pair<int, int>> pool;   // (panel, first tile) of what the aligned part leaves, panel-major
    if ((int64_t)T >= u) {                   // heads [0, h) of one panel per workgroup, tails to the pool
        int64_t h = (total + (int64_t)c * n + m - 1) / m;      // h + c = (n (T - h) + c m) / (m - n)
        if (h > T || n == m) h = T;
        budget = h + c;
        room.assign(m, budget);
        for (int i = 0; i < n; ++i) {
            put(i, pnls[i], 0, (int)h);      // n <= m here (n T <= m u and T >= u)
            if ((int64_t)T > h) pool.push_back(std::make_pair(pnls[i], (int)h));
        }
    } else {                                 // whole panels per workgroup while they fit the budget, the rest to the pool
        budget = ((int64_t)n * (T + c) + m - 1) / m + c;
        room.assign(m, budget);
        const int a = (int)(budget / (T + c)) > 0 ? (int)(budget / (T + c)) : 1;
        int next = 0;
        for (int w = 0; w < m; ++w)
            for (int j = 0; j < a && next < n; ++j) put(w, pnls[next++], 0, T);
        for (; next < n; ++next) pool.push_back(std::make_pair(pnls[next], 0));
    }
    int w = 0;
    for (auto &pt : pool) {                  // share the pool out in order: every workgroup is filled up to its budget
        int t0 = pt.second;
        while (t0 < T) {
            while (w < m - 1 && room[w] <= c) ++w;
            int64_t fit = room[w] - c;
            if (fit < 1 || w == m - 1) fit = T;              // the last workgroup takes whatever is left
            const int nt = (int)std::min<int64_t>(fit, T - t0);
            put(w, pt.first, t0, nt);
            t0 += nt;
        }
    }
}

// Planned ("stream-K", XCD-aware) decomposition of the fp32 scan.
//
// Balance.  One workgroup alone on a CU reaches well under the MFMA rate of two co-resident ones, so a grid that is not
// a multiple of 2 x CUs pays a whole extra round (391 panels ran as slowly as 512).  Instead the panels x tiles unit
// space is cut into equal shares, one per resident slot; a share that touches several panels yields one partial list per
// panel touched and k_merge combines the pieces of a panel.
//
// Locality.  A workgroup re-streams its query panel (128 x d x 4 B) and streams a database tile of the same size per
// unit; the 64 workgroups of an XCD move 32 MB per unit time through a 4 MB L2, so NOTHING hits unless workgroups read
// the same tile at the same time.  With plain contiguous shares (round 1) the shares start at arbitrary tiles: at the
// headline shape PMC FETCH_SIZE was 2.0 x the scan-model bytes and the launch ran at 0.80 of the MFMA peak, against
// 0.89 at 262 144^2 where every share happens to be four whole panels walked from tile 0 in step.  So the shares are
// built per XCD (workgroup b runs on XCD b % 8: round-robin dispatch; panel p belongs to XCD p % 8) and ALIGNED: with
// u units per workgroup and T tiles per panel, T >= u: as many workgroups as the XCD has panels take tiles [0, u) of
// one panel each -- they walk the same tiles in step -- and the other workgroups share the tails [u, T); T < u: every
// workgroup first takes floor(u / T) whole panels (again from tile 0, in step), the rest is shared out.  A segment is
// (panel, first tile, tiles, piece number in the panel); workgroup b owns segments seg_begin[b] .. seg_begin[b+1].
//
// the plan for `slots` resident workgroup slots (2 per CU), `xcds` XCD groups (1 = not XCD-aware) and `seg_cost` tile times per segment
static inline void lemon_plan_segments_host(int panels, int n_tiles, int slots, int xcds, int seg_cost, LemonPlan &plan) {
    const int64_t units = (int64_t)panels * n_tiles;
    int64_t g = units / 8;                               // every workgroup keeps >= 8 tiles
    if (g < 1) g = 1;
    if (g > slots) g = slots;
    const int X = (panels >= 8 * xcds && g >= 8 * xcds) ? xcds : 1;   // few panels: one group, still aligned
    std::vector<std::vector<int>> wg_segs((size_t)g);
    plan.pieces.assign((size_t)panels, 0);
    for (int x = 0; x < X; ++x) {
        std::vector<int> wgs, pnls;
        for (int b = x; b < (int)g; b += X) wgs.push_back(b);
        for (int q = x; q < panels; q += X) pnls.push_back(q);
        plan_group(wgs, pnls, n_tiles, seg_cost, wg_segs, plan.pieces);
    }
    plan.grid = (int)g;
    plan.seg_begin.assign((size_t)g + 1, 0);
    plan.segs.clear();
    for (int b = 0; b < (int)g; ++b) {
        plan.seg_begin[b] = (int)(plan.segs.size() / 4);
        plan.segs.insert(plan.segs.end(), wg_segs[b].begin(), wg_segs[b].end());
    }
    plan.seg_begin[g] = (int)(plan.segs.size() / 4);
    plan.splits = 1;
    for (int c : plan.pieces) plan.splits = c > plan.splits ? c : plan.splits;
}

namespace lemon_f32_plan {

constexpr int BQ = 128, BX = 128;       // query rows per panel, database rows per tile (mirror knn_common.hpp: static_asserts in knn_f32.hip)
constexpr int64_t QCHUNK = 1 << 19;     // queries per chunk at the most: the workspace stays bounded (1 GiB of candidates)
constexpr int CUS = 256;                // CUs a plan assumes where no device says otherwise (MI355X)

// tuning knobs of the fp32 scan (read_scan_knobs() in knn_f32.hip fills them per call)
struct Knobs {
    bool splits_set = false;            // LEMON_SPLITS set at all: (panel, split) rectangles, no segment plan
    int splits = 0;                     //   its value: > 0 fixes the split count
    int xcds = 8;                       // LEMON_XCDS: XCD groups of the segment plan, 1 = not XCD-aware
    int seg_cost = 3;                   // LEMON_SEG_COST: what a segment costs on top of its tiles, in tile times
    bool share_bounds = true;           // LEMON_SHARE_BOUNDS=0: the pieces of a panel keep their admission bounds to themselves
    int stale = 96;                     // LEMON_STALE: new entries per query that trigger a re-selection
    int fair = -1;                      // LEMON_FAIR: log2(fair-share turn in 10 ns ticks), 0 = no turns, -1 = derive it
};

struct Chunk {
    int64_t cn, nq_pad;                 // queries of this chunk, padded to whole panels
    int panels, n_tiles;
    bool planned;                       // its workgroups follow the segment plan of (panels, n_tiles, slots, xcds, seg_cost)
    int slots, xcds, seg_cost;
    int grid, splits, tiles_per_split;  // planned: grid and splits are the segment plan's (set_geometry), 0 until then
    int fair;                           // ScanParams::fair
    bool share;                         // a panel is scanned by several workgroups, which share their admission bounds
                                        // (planned: the knob alone until set_geometry)
    int stale;
};

inline void set_geometry(Chunk &c, int grid, int splits) {
    c.grid = grid; c.splits = splits;
    c.share = c.share && splits > 1;
}

inline void plan_segments(const Chunk &c, LemonPlan &plan) {
    lemon_plan_segments_host(c.panels, c.n_tiles, c.slots, c.xcds, c.seg_cost, plan);
}

// Plans one query chunk of a search over n rows of width d on `cus` CUs (two resident workgroups each): `left` queries remain.
// A unit space of fewer than 2 units has no segment plan: one workgroup, no merge.
inline Chunk plan_chunk(int64_t left, int64_t n, int d, int cus, const Knobs &kn) {
    Chunk c;
    c.cn = left < QCHUNK ? left : QCHUNK;
    c.nq_pad = (c.cn + BQ - 1) / BQ * BQ;
    c.panels = (int)(c.nq_pad / BQ);
    c.n_tiles = (int)((n + BX - 1) / BX);
    c.planned = !kn.splits_set && (int64_t)c.panels * c.n_tiles >= 2;
    c.slots = 2 * (cus > 0 ? cus : CUS); c.xcds = kn.xcds; c.seg_cost = kn.seg_cost;
    c.tiles_per_split = c.n_tiles;
    c.share = kn.share_bounds;
    if (c.planned) c.grid = c.splits = 0;
    else {
        int splits;
        lemon_bf16_plan::plan_splits(c.panels, c.n_tiles, kn.splits, &splits, &c.tiles_per_split);
        set_geometry(c, c.panels * splits, splits);
    }
    c.stale = kn.stale;
    // fair-share turns (see k_scan_f32): about eight turns per launch, between 82 us and 5.2 ms each -- longer turns
    // measured better (16.9 / 16.7 / 16.4 / 16.3 ms at the headline shape for no turns / 5 us / 82 us / 2.6 ms), a
    // turn longer than the launch is no turn at all.
    c.fair = kn.fair;
    if (kn.fair < 0) {
        const double ticks = 2.0 * (double)c.cn * (double)n * (double)d / 1.25e14 * 1e8 / 8.0;   // launch / 8, in ticks
        int bit = 13;
        while (bit < 19 && (double)(2u << bit) <= ticks) ++bit;
        c.fair = bit;
    }
    return c;
}

}  // namespace lemon_f32_plan

