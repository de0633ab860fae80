// gemm_f16x3_plan.hpp -- the host-side plan of the hand-written split-fp16 GEMM (linear_f16x3t_impl, gemm_f16x3.hip): which of
// the 13 kernel instantiations serves a call and how its tiles are walked.  Plain C++: no HIP, no getenv, no statics, so that the
// host compiler builds it and tests/test_gemm_f16x3_plan_host.py checks it on the CPU against a table of recorded decisions.
#pragma once
#include <stdint.h>

#ifndef LEMON_GEMM_GM
#define LEMON_GEMM_GM 32
#endif

namespace lemon_gemm_plan {

// geometry and codes (mirror split3.hpp, gemm_f16x3.hip and lemon_hip.h: static_asserts in gemm_f16x3.hip)
constexpr int TM = 128, TN = 256;      // rows of an activation tile, of a weight tile
constexpr int GM = LEMON_GEMM_GM;      // m-tiles per super-block where a super-block is one n-tile wide
constexpr int ACT_GELU = 2;            // LEMON_ACT_GELU

// The launch forms, in the order of FACTS and of KERNELS[] in gemm_f16x3.hip: three that consume a folded LayerNorm (row_aff +
// colsum), four that leave the operand + row statistics of the next one, three plain on each MFMA shape.
enum Form { T16_GELU_FOLD = 0, T16_SILU_FOLD, T16_F32_FOLD, T16_EMIT, T16_EMIT_LEAN1, T16_EMIT_LEAN2, T16_EMIT_LEAN3,
            T16_GELU, T16_SILU, T16_F32, T32_GELU, T32_SILU, T32_F32, N_FORMS };

// a form's reported name (the instantiation), its MFMA shape (16: 16x16x32, 32: 32x32x16) and template arguments: EPI 0 fp32
// out / 1 SiLU operand / 2 GELU operand, FOLD, EMIT, LEAN (bit 0: no fp32 result, bit 1: the residual is a tile-major operand)
struct FormFacts { const char *name; int mfma, epi; bool fold, emit; int lean; };
constexpr FormFacts FACTS[N_FORMS] = {
    {"k_gemm_f16x3t16<2, true, false>",    16, 2, true,  false, 0},
    {"k_gemm_f16x3t16<1, true, false>",    16, 1, true,  false, 0},
    {"k_gemm_f16x3t16<0, true, false>",    16, 0, true,  false, 0},
    {"k_gemm_f16x3t16<0, false, true>",    16, 0, false, true,  0},
    {"k_gemm_f16x3t16<0, false, true, 1>", 16, 0, false, true,  1},
    {"k_gemm_f16x3t16<0, false, true, 2>", 16, 0, false, true,  2},
    {"k_gemm_f16x3t16<0, false, true, 3>", 16, 0, false, true,  3},
    {"k_gemm_f16x3t16<2, false, false>",   16, 2, false, false, 0},
    {"k_gemm_f16x3t16<1, false, false>",   16, 1, false, false, 0},
    {"k_gemm_f16x3t16<0, false, false>",   16, 0, false, false, 0},
    {"k_gemm_f16x3t<2>",                   32, 2, false, false, 0},
    {"k_gemm_f16x3t<1>",                   32, 1, false, false, 0},
    {"k_gemm_f16x3t<0>",                   32, 0, false, false, 0},
};

// Matrix instruction: 16x16x32 where the k extent allows whole k32 steps (ks = k / 16 even: every tower width), else 32x32x16;
// mfma_shape = 32 forces the latter (LEMON_GEMM_MFMA: A/B runs).  The fold and emit forms exist in the 16x16x32 kernel only and
// take it whatever mfma_shape says (their entries refuse k % 32 != 0).  An operand output that is not GELU is SiLU.
inline Form select_form(int mfma_shape, int ks, int act, bool out_operand, bool fold, bool emit, bool has_out, bool has_residual_t) {
    const int epi = !out_operand ? 0 : act == ACT_GELU ? 2 : 1;
    if (fold) return epi == 2 ? T16_GELU_FOLD : epi == 1 ? T16_SILU_FOLD : T16_F32_FOLD;
    if (emit) return has_residual_t ? (has_out ? T16_EMIT_LEAN2 : T16_EMIT_LEAN3) : (has_out ? T16_EMIT : T16_EMIT_LEAN1);
    if (mfma_shape == 16 && ks % 2 == 0) return epi == 2 ? T16_GELU : epi == 1 ? T16_SILU : T16_F32;
    return epi == 2 ? T32_GELU : epi == 1 ? T32_SILU : T32_F32;
}

// gm x gn: the super-block an XCD works through at a time; vblocks: the grid (>= tiles: ragged super-blocks leave holes)
struct Walk { int m_tiles, n_tiles, ks, gm, gn; int64_t vblocks; };

// Super-block of the tile walk: gn = the largest divisor of the n-tile count up to 4 (a gn that does not divide it leaves
// every other XCD with half-empty super-blocks: +25 % time measured), gm so that an XCD's 64 resident workgroups cover one
// or two super-blocks.  Measured against 32 x 1 at the tower shapes (tools/micro/gemm_ab.hip walk): -1 ... -3 %; the
// operand re-fetches this saves (FETCH_SIZE 5.0 GB for fc1 at 32 x 1: the activations once per weight tile column) are
// served by the Infinity Cache either way.  gm_override > 0 (LEMON_GEMM_WALK=gm,gn) replaces both.  The super-block count is
// padded to the 8 XCDs the workgroup ids go round.
inline Walk plan_walk(int64_t m, int n, int k, int gm_override, int gn_override) {
    Walk w;
    w.ks = k / 16; w.m_tiles = (int)((m + TM - 1) / TM); w.n_tiles = n / TN;
    if (gm_override > 0) { w.gm = gm_override; w.gn = gn_override > 0 ? gn_override : 1; }
    else {
        w.gn = w.n_tiles % 4 == 0 ? 4 : w.n_tiles % 3 == 0 ? 3 : w.n_tiles % 2 == 0 ? 2 : 1;
        w.gm = w.gn == 1 ? GM : w.gn == 3 ? 8 : 16;
    }
    if (w.gn > w.n_tiles) w.gn = w.n_tiles;
    const int64_t blocks = (int64_t)((w.m_tiles + w.gm - 1) / w.gm) * ((w.n_tiles + w.gn - 1) / w.gn);
    w.vblocks = ((blocks + 7) / 8) * w.gm * w.gn * 8;
    return w;
}

}  // namespace lemon_gemm_plan
