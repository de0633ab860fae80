// knn_bf16_plan.hpp -- the host-side plan of the 16-bit filter scan (lemon_search_bf16, knn_bf16.hip): which of the five scan
// kernels serves a query chunk, where the chunk is cut, how the database is split between workgroups and into Infinity-Cache
// chunks, and how much carried state that takes.  Plain C++: no HIP, no getenv, no statics, so that the host compiler builds it
// and tests/test_knn_bf16_plan_host.py checks it on the CPU against a table of recorded decisions.
#pragma once
#include <stdint.h>

namespace lemon_bf16_plan {

// geometry (BQ, BX, NT mirror knn_common.hpp: static_asserts in knn_bf16.hip)
constexpr int BQ = 128;        // queries per workgroup of the streaming and the one-block kernel
constexpr int BX = 128;        // database rows per tile of those two; lemon_plan_splits counts in these
constexpr int NT = 256;        // threads per workgroup
constexpr int BKH = 64;        // 16-bit k-slice per LDS stage (128 B rows, like fp32 BK = 32)
constexpr int RT2 = 64;        // database rows per tile of QS2 / QS4 / QSW
constexpr int BQ2 = 256;       // queries per workgroup of QS2 / QS4 (64 per wave)
constexpr int BQW = 128;       // queries per workgroup of QSW (32 per wave)
constexpr int64_t QCHUNK_H = 1 << 19;   // queries per chunk at the most

enum Kernel { SCAN_BF16 = 0, QS, QS2, QS4, QSW, N_KERNELS };

// what the host has to know about a kernel: its reported name, queries per workgroup, database rows per tile, floats of
// per-lane state carried between database chunks (0: streaming, no lane lists, no k_bf16_final), count segments per query
struct KernelFacts { const char *name; int panel, tile, state_floats, segs; };
constexpr KernelFacts FACTS[N_KERNELS] = {
    {"scan_bf16", BQ,  BX,  0,  2},     // k_scan_bf16: any pitch, streams both operands
    {"qs",        BQ,  BX,  4,  2},     // k_scan_bf16_qs: one query block per wave, pitches 256 / 512 / 768
    {"qs2",       BQ2, RT2, 8,  2},     // k_scan_bf16_qs2: two blocks per wave, pitches 512 / 768
    {"qs4",       BQ2, RT2, 16, 4},     // k_scan_f16_qs4: the same on the 16x16x32 MFMA, pitch 512 and inner product at 768
    {"qsw",       BQW, RT2, 8,  4},     // k_scan_f16_qsw: pitches 1024 / 1280 with the wide filter on
};

// runtime knobs that choose between production kernels or size them (read_knobs() in knn_bf16.hip fills them per call)
struct Knobs {
    bool qs2 = true;               // LEMON_QS2=0: the one-block kernel instead of QS2 / QS4 (A/B aid)
    bool qs4 = true;               // LEMON_QS4=0: QS2 instead of QS4 (A/B aid)
    int qs2_min_panels = 768;      // LEMON_QS2_MIN_PANELS: panels from which QS2 / QS4 / QSW are used (the tests force them with 0)
    bool rest_split = true;        // LEMON_QS4_REST=0: the ragged rest goes through the small kernel (A/B aid)
    double chunk_mb = 64.0;        // LEMON_CHUNK_MB: database chunk of a launch; <= 0: the whole database
    int forced_splits = 0;         // LEMON_SPLITS: > 0 fixes the split count
};

struct Plan {
    Kernel kernel;
    const char *name;
    int64_t cn;                    // queries of this chunk
    int panel, tile;               // queries per workgroup, database rows per tile
    int n_tiles, panels, splits, tiles_per_split, chunk_tiles;
    int64_t state_elems, cnt_elems;
    int segs;
};

// enough workgroups to fill 256 CUs x 2 resident 1.5 times; every split keeps >= 8 tiles so the
// per-split warm-up (first-tile selection, final sort, merge) amortises
inline void plan_splits(int panels, int n_tiles, int forced, int *splits_out, int *tiles_per_split_out) {
    int splits = 1;
    if (forced > 0) {
        splits = forced;
        if (splits > n_tiles) splits = n_tiles;
    } else if (panels < 768) {
        splits = (768 + panels - 1) / panels;
        int max_splits = n_tiles / 8;
        if (max_splits < 1) max_splits = 1;
        if (splits > max_splits) splits = max_splits;
    }
    const int tiles_per_split = (n_tiles + splits - 1) / splits;
    *splits_out = (n_tiles + tiles_per_split - 1) / tiles_per_split;
    *tiles_per_split_out = tiles_per_split;
}

// Whole rounds first.  The chunked scan runs ONE workgroup per CU, all of equal length: 1 859 workgroups take eight rounds of
// 256 like 2 048 do (1 M queries = 2 048 + 1 859 panels: 4.6 % of the scan spent in a quarter-full last round).  So a final
// stretch that does not fill its last round to 80 % is cut at the last whole round; the ragged rest comes back as a chunk of
// its own (rest_splits).
inline int64_t whole_round_cut(int64_t cn, int panel, int cus) {
    const int64_t panels_c = (cn + panel - 1) / panel, full = panels_c / cus * cus;
    return (full > 0 && panels_c != full && (panels_c - full) * 5 < (int64_t)cus * 4) ? full * panel : cn;
}

// The ragged rest behind whole-round chunks (1 M queries: 16 960 = 67 panels of 256): the same kernel with the database split
// between a few workgroups per panel -- the smallest split count that fills at least three quarters of the rounds it takes
// (67 panels x 3 = 201 of 256 slots) and leaves every split 64 tiles -- instead of 133 one-block panels x 6 splits (39 ms per
// modality at 1 M x 768).  0: no such count.
inline int rest_splits(int64_t cn, int panel, int n_tiles128, int cus) {
    const int panels_r = (int)((cn + panel - 1) / panel);
    for (int sp = 1; sp <= 16; ++sp) {
        const int64_t wgs = (int64_t)panels_r * sp, rounds = (wgs + cus - 1) / cus;
        if (wgs * 4 >= rounds * cus * 3 && n_tiles128 / sp >= 64) return sp;
    }
    return 0;
}

// Plans one query chunk: `left` queries remain, `prev` served the chunk before (ignored for the first).
//
// A pitch and a metric have a small kernel (one-block QS up to pitch 768, streaming beyond) and possibly a large one with
// wider panels or tiles.  QS2 halves the panel count.  When 256-query panels alone do not fill the chip the database would be
// split between more workgroups, and every split pays its own cold start (k ln(n/k) appends per query): measured 13.0 -> 20.1 ms
// at 50 000 x 40 000 x 512 and 17.3 -> 21.8 ms at 131 072^2 x 256 (k = 11), against 1 648 -> 1 501 ms at 1 M x 768,
// 142.1 -> 129.9 ms at 262 144^2 x 768 and 103.9 -> 97.8 ms at 262 144^2 x 512.  So the large kernel runs from 768 of its
// panels on (the splits == 1 regime of plan_splits), and on the ragged rest behind such a chunk.
// (QS4: the L2 epilogue's |x|^2 loads and |q|^2 registers do not fit next to d = 768's fragments -- 14 spilled registers with
// 20 parked steps, and 21 is what the LDS holds --, so squared-L2 at pitch 768 stays on QS2.  Pitches 1024 / 1280 exist only
// with the wide filter on: lemon_bf16_pitch.)
inline Plan plan_chunk(int64_t left, bool first, Kernel prev, int64_t n, int d, int pitch, bool l2, bool wide_on, int cus,
                       const Knobs &kn) {
    Kernel small = SCAN_BF16, large = SCAN_BF16;
    if (pitch <= 768) {
        small = large = QS;
        if (kn.qs2 && pitch >= 512) large = (kn.qs4 && (pitch / BKH == 8 || !l2)) ? QS4 : QS2;
    } else if (wide_on && d > 768 && (pitch == 1024 || pitch == 1280)) {
        large = QSW;
    }
    const int n_tiles128 = (int)((n + BX - 1) / BX);
    Plan p;
    p.cn = left < QCHUNK_H ? left : QCHUNK_H;
    p.kernel = small;
    int rest = 0;
    if (large != small) {
        const int panel = FACTS[large].panel;
        if (p.cn >= (int64_t)kn.qs2_min_panels * panel) p.kernel = large;
        else if (!first && prev == large && large != QS2 && kn.rest_split && (rest = rest_splits(p.cn, panel, n_tiles128, cus)) != 0)
            p.kernel = large;
        if (p.kernel == large && p.cn < QCHUNK_H) p.cn = whole_round_cut(p.cn, panel, cus);
    }
    const KernelFacts &f = FACTS[p.kernel];
    p.name = f.name; p.panel = f.panel; p.tile = f.tile; p.segs = f.segs;
    p.n_tiles = (int)((n + f.tile - 1) / f.tile);
    p.panels = (int)((p.cn + f.panel - 1) / f.panel);
    plan_splits(p.panels, n_tiles128, kn.forced_splits, &p.splits, &p.tiles_per_split);
    if (rest) {
        p.tiles_per_split = (n_tiles128 + rest - 1) / rest;
        p.splits = (n_tiles128 + p.tiles_per_split - 1) / p.tiles_per_split;
    }
    p.tiles_per_split *= BX / f.tile;                // (plan_splits counts 128-row tiles)
    const bool stationary = f.state_floats > 0;      // lane lists, chunked launches, k_bf16_final
    const int64_t grid = (int64_t)p.panels * p.splits;
    // database chunks sized for the Infinity Cache (the chunk is re-read by every query panel)
    p.chunk_tiles = p.n_tiles;
    if (stationary && p.splits == 1) {
        if (kn.chunk_mb > 0) {
            p.chunk_tiles = (int)(kn.chunk_mb * 1048576.0 / ((double)f.tile * pitch * 2));
            if (p.chunk_tiles < 8) p.chunk_tiles = 8;
        }
        if (p.chunk_tiles > p.n_tiles) p.chunk_tiles = p.n_tiles;
    }
    // per-lane state carried between chunk launches (splits == 1) + the list counts handed to k_bf16_final
    p.state_elems = p.splits == 1 ? grid * NT * f.state_floats : 0;
    p.cnt_elems = stationary ? grid * f.panel * f.segs : 0;
    return p;
}

}  // namespace lemon_bf16_plan
