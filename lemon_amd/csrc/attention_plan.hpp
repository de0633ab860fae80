// attention_plan.hpp -- the host-side plan of the attention family (attention.hip, attention_hd.hip, attention_varlen.hip): which of
// the 68 kernel instantiations serves a call, its grid, block and dynamic LDS, or why the call is refused.  Plain C++: no HIP, no
// getenv, no statics, so that the host compiler builds it and tests/test_attention_plan_host.py checks it on the CPU against a
// table of recorded decisions.
#pragma once
#include <stdint.h>

namespace lemon_attn_plan {

// geometry (the kernels' own constants: static_asserts in the three units tie them to these)
constexpr int HD = 64, PITCH = 68;            // head dimension of every family but hdx; LDS row pitch of the fp32 forms, in floats
constexpr int MAX_SEQ = 4096;                 // LEMON_ATTENTION_MAX_SEQ
constexpr int ONE_WG_MAX_SEQ = 288;           // one workgroup of nine waves per (sequence, head): also the most lemon_attention_set_stream_min takes
constexpr int STREAM_WMAX = 8, STREAM_TB = 4, STREAM_KB = 32 * STREAM_TB;     // streaming forms: waves, key tiles and keys per block at most
constexpr int S32_WMAX = 4, S32_TB = 2, S32_KB = 32 * S32_TB;                 // ... of the fp32 form
constexpr int S16_WMAX = STREAM_WMAX, S16_TB = STREAM_TB, S16_KB = 32 * S16_TB;   // ... of the split-fp16 form
constexpr int X_WMAX = 4, X_TB = 2, X_KB = 32 * X_TB;                         // ... of k_attention_hdx_stream
constexpr int HD_MIN_STEP = 8, HDX_MAX = 128, HDX_NARROW = 96;                // hdx: multiples of 8 up to 128; up to 96 in the HDP 96 kernel
constexpr int E_INVALID = -1;                 // LEMON_E_INVALID

// What may influence the choice, per calling thread.  arithmetic, as lemon_attention_set_f16 took it: 0 = v_mfma_f32_32x32x2_f32 (no
// range limit), 1 = split products on the fp16 matrix cores (q, k, v and the probabilities carried as fp16 pairs: inputs must stay
// inside +-65 504), 2 = that with the FIRST general kernel (fp32 K / V in LDS, re-split by every wave: the equality test).
// stream_min (lemon_attention_set_stream_min): longer sequences take the streaming kernels.  head_dims
// (lemon_attention_set_head_dims): 0 = head_dim must be 64, 1 = multiples of 8 in 72 .. 128 go to k_attention_hdx_stream, 2 = 64
// goes there as well (the equality test, A/B timing).  short_off (LEMON_ATTN_SHORT=0): seq_len <= 64 goes to the general kernels;
// old_general (LEMON_ATTN_GENERAL=old): arithmetic 1 behaves as 2 (A/B runs).
struct Knobs { int arithmetic, stream_min, head_dims; bool short_off, old_general; };

// The launch families, in the order of FACTS; a family's four output forms (SPLIT 0 .. 3) are consecutive in each unit's KERNELS[]
enum Form { SHORT1_F32 = 0, SHORT1_F16, SHORT2_F32, SHORT2_F16, GENERAL_F32, GENERAL_F16, STAGED, STREAM_F32, STREAM_F16,
            HDX_96, HDX_128,
            VL_SHORT1_F32, VL_SHORT1_F16, VL_SHORT2_F32, VL_SHORT2_F16, VL_F32, VL_F16, N_FORMS };
enum Unit { UNIT_ATTENTION = 0, UNIT_HD, UNIT_VARLEN };      // attention.hip, attention_hd.hip, attention_varlen.hip

constexpr int hdx_lds(int hdp) { return 2 * X_KB * (hdp + 4) * 4; }      // K rows, then V rows, at pitch HDP + 4 floats

// a form's reported names (the instantiation, one per output form), its unit and place in the unit's KERNELS[], its template
// arguments (tj: TJ of the short forms, f16: F16, hdp: HDP; 0 where the kernel has none), the threads its launch bound allows and the
// hipFuncAttributeMaxDynamicSharedMemorySize it needs before its first launch on a device (0: none).  The attribute is a fixed
// value per family, not the call's LDS size: 160 KB for the one-workgroup families, 80 KB for the streaming ones, and the
// kernel's own (fixed) LDS size for hdx where that exceeds 64 KB.
#define LEMON_ATTN_NAMES(pre, post) {pre "0" post, pre "1" post, pre "2" post, pre "3" post}
struct FormFacts { const char *name[4]; Unit unit; int slot, tj; bool f16; int hdp, max_threads, attr; };
constexpr FormFacts FACTS[N_FORMS] = {
    {LEMON_ATTN_NAMES("k_attention_hd64_short<1, ", ", false>"), UNIT_ATTENTION, 0, 1, false, 0, 64, 0},
    {LEMON_ATTN_NAMES("k_attention_hd64_short<1, ", ", true>"),  UNIT_ATTENTION, 1, 1, true,  0, 64, 0},
    {LEMON_ATTN_NAMES("k_attention_hd64_short<2, ", ", false>"), UNIT_ATTENTION, 2, 2, false, 0, 128, 0},
    {LEMON_ATTN_NAMES("k_attention_hd64_short<2, ", ", true>"),  UNIT_ATTENTION, 3, 2, true,  0, 128, 0},
    {LEMON_ATTN_NAMES("k_attention_hd64<", ", false>"),          UNIT_ATTENTION, 4, 0, false, 0, 576, 160 * 1024},
    {LEMON_ATTN_NAMES("k_attention_hd64<", ", true>"),           UNIT_ATTENTION, 5, 0, true,  0, 576, 160 * 1024},
    {LEMON_ATTN_NAMES("k_attention_hd64_f16<", ">"),             UNIT_ATTENTION, 6, 0, true,  0, 576, 160 * 1024},
    {LEMON_ATTN_NAMES("k_attention_hd64_stream<", ">"),          UNIT_ATTENTION, 7, 0, false, 0, 64 * S32_WMAX, 80 * 1024},
    {LEMON_ATTN_NAMES("k_attention_hd64_stream_f16<", ">"),      UNIT_ATTENTION, 8, 0, true,  0, 64 * S16_WMAX, 80 * 1024},
    {LEMON_ATTN_NAMES("k_attention_hdx_stream<96, ", ">"),       UNIT_HD, 0, 0, false, 96,  64 * X_WMAX, hdx_lds(96) > 64 * 1024 ? hdx_lds(96) : 0},
    {LEMON_ATTN_NAMES("k_attention_hdx_stream<128, ", ">"),      UNIT_HD, 1, 0, false, 128, 64 * X_WMAX, hdx_lds(128) > 64 * 1024 ? hdx_lds(128) : 0},
    {LEMON_ATTN_NAMES("k_attnvl_short<1, ", ", false>"),         UNIT_VARLEN, 0, 1, false, 0, 64, 0},
    {LEMON_ATTN_NAMES("k_attnvl_short<1, ", ", true>"),          UNIT_VARLEN, 1, 1, true,  0, 64, 0},
    {LEMON_ATTN_NAMES("k_attnvl_short<2, ", ", false>"),         UNIT_VARLEN, 2, 2, false, 0, 128, 0},
    {LEMON_ATTN_NAMES("k_attnvl_short<2, ", ", true>"),          UNIT_VARLEN, 3, 2, true,  0, 128, 0},
    {LEMON_ATTN_NAMES("k_attnvl_f32<", ">"),                     UNIT_VARLEN, 4, 0, false, 0, 576, 160 * 1024},
    {LEMON_ATTN_NAMES("k_attnvl_f16<", ">"),                     UNIT_VARLEN, 5, 0, true,  0, 576, 160 * 1024},
};

// Why a call is refused: the text lemon_last_error() then holds.  The entries test the EARLY ones (shape arguments) first, return
// LEMON_OK for batch == 0, check their pointers, and only then the LATE ones (32-bit offsets, the tile-major operand).
enum Refusal { ACCEPTED = 0, R_SHAPE, R_HEAD_DIM, R_MAX_SEQ, R_VL_HEAD_DIM, R_VL_SEQ, R_GRID, R_STREAM_HEADS, R_VL_HEADS, R_HDX_HEADS,
               R_HDX_TILED, N_REFUSALS };
constexpr const char *MESSAGES[N_REFUSALS] = {
    "",
    "invalid argument: batch >= 0, seq_len > 0, heads > 0 (batch >= 0 && seq_len > 0 && heads > 0)",
    "invalid argument: head_dim must be 64 (head_dim == HD || hdx)",
    "invalid argument: seq_len <= LEMON_ATTENTION_MAX_SEQ = 4096 (seq_len <= LEMON_ATTENTION_MAX_SEQ)",
    "invalid argument: per-sequence lengths: head_dim must be 64 (in every lemon_attention_set_head_dims mode) (head_dim == HD)",
    "invalid argument: per-sequence lengths: seq_len <= 288 (the streaming kernels take no lengths) (seq_len <= 288)",
    "invalid argument: batch * heads < 2^31 (batch * heads < (int64_t)1 << 31)",
    "invalid argument: heads < 43 690 (32-bit offsets inside a key block) ((int64_t)STREAM_KB * 3 * heads * HD * 4 < (int64_t)1 << 32)",
    "invalid argument: heads < 19 418 (32-bit offsets inside a head's slice) ((int64_t)288 * 3 * heads * HD * 4 < (int64_t)1 << 32)",
    "invalid argument: 64 * 3 * heads * head_dim * 4 < 2^32 (32-bit offsets inside a key block) "
    "((int64_t)X_KB * 3 * heads * hd * 4 < (int64_t)1 << 32)",
    "invalid argument: tile-major output: heads * head_dim a multiple of 16 (split != 3 || (heads * hd) % 16 == 0)",
};

// Neither refusal and batch == 0: nothing to do (form and geometry are not set).  hd: what k_attention_hdx_stream takes as its
// head dimension and its launch derives c_exp = log2(e) / sqrt(hd) from (HD elsewhere: those kernels hold the constant).
struct Plan { Refusal early, late; Form form; int tj, hd; unsigned grid_x, grid_y; int threads, lds; };

// the tokens of one key / query block are addressed with 32-bit byte offsets: `tokens` of them, 3 * heads * hd floats each
inline bool offsets_fit(int tokens, int heads, int hd) { return (int64_t)tokens * 3 * heads * hd * 4 < (int64_t)1 << 32; }

// One-workgroup families (seq_len <= 288): tj waves; fp32 K and V rows at PITCH, or the staged form's four fp16 planes of one key
// block (ceil(tj / 2) tiles when 5 < tj <= 8), but never less than the fp32 [32 tj][64] image Q and the output pass through
inline int one_wg_lds(bool staged, int tj) {
    if (!staged) return 2 * 32 * tj * PITCH * 4;
    const int tb = (tj <= 5 || tj > 8) ? tj : (tj + 1) / 2;
    const int planes = 4 * 32 * tb * 128, image = 32 * tj * 256;
    return planes > image ? planes : image;
}

// Streaming families: the tj query tiles are dealt evenly to ceil(tj / wmax) workgroups of ceil(tj / blocks) waves
inline void deal_tiles(Plan &p, int wmax) {
    const int nqb = (p.tj + wmax - 1) / wmax;
    p.grid_y = (unsigned)nqb;
    p.threads = 64 * ((p.tj + nqb - 1) / nqb);
}

// split: the output form 0 .. 3; varlen: the lemon_attention_*_varlen entries with lengths (without: the plain entry, as they call it)
inline Plan plan(const Knobs &k, int64_t batch, int seq_len, int heads, int head_dim, int split, bool varlen) {
    Plan p = {ACCEPTED, ACCEPTED, N_FORMS, 0, HD, 0, 1, 0, 0};
    const bool hdx = !varlen && k.head_dims != 0 && head_dim % HD_MIN_STEP == 0 && head_dim <= HDX_MAX &&
                     (head_dim > HD || (head_dim == HD && k.head_dims == 2));
    if (!(batch >= 0 && seq_len > 0 && heads > 0)) p.early = R_SHAPE;
    else if (varlen && head_dim != HD) p.early = R_VL_HEAD_DIM;
    else if (varlen && seq_len > ONE_WG_MAX_SEQ) p.early = R_VL_SEQ;
    else if (!varlen && !(head_dim == HD || hdx)) p.early = R_HEAD_DIM;
    else if (!varlen && seq_len > MAX_SEQ) p.early = R_MAX_SEQ;
    if (p.early != ACCEPTED || batch == 0) return p;

    p.tj = (seq_len + 31) / 32;
    p.grid_x = (unsigned)(batch * heads);
    const bool f16 = k.arithmetic != 0;
    if (batch * heads >= (int64_t)1 << 31) p.late = R_GRID;
    else if (varlen) {
        // (the varlen entries know neither short_off nor old_general, and arithmetic 2 runs the staged form here)
        if (!offsets_fit(ONE_WG_MAX_SEQ, heads, HD)) p.late = R_VL_HEADS;
        p.form = p.tj <= 2 ? (Form)(VL_SHORT1_F32 + 2 * (p.tj - 1) + f16) : f16 ? VL_F16 : VL_F32;
        p.threads = 64 * p.tj;
        p.lds = p.tj <= 2 ? 0 : one_wg_lds(f16, p.tj);
    } else if (hdx) {
        // (one fp32 kernel for every seq_len and both arithmetic selections)
        if (!offsets_fit(X_KB, heads, head_dim)) p.late = R_HDX_HEADS;
        else if (split == 3 && (heads * head_dim) % 16 != 0) p.late = R_HDX_TILED;
        p.form = head_dim > HDX_NARROW ? HDX_128 : HDX_96;
        p.hd = head_dim;
        deal_tiles(p, X_WMAX);
        p.lds = hdx_lds(FACTS[p.form].hdp);
    } else if (p.tj <= 2 && !k.short_off) {
        p.form = (Form)(SHORT1_F32 + 2 * (p.tj - 1) + f16);
        p.threads = 64 * p.tj;
    } else if (seq_len > k.stream_min) {
        // (the guard is written for the larger key block of the two forms)
        if (!offsets_fit(STREAM_KB, heads, HD)) p.late = R_STREAM_HEADS;
        p.form = f16 ? STREAM_F16 : STREAM_F32;
        deal_tiles(p, f16 ? S16_WMAX : S32_WMAX);
        p.lds = f16 ? 4 * S16_KB * 128 : 2 * S32_KB * PITCH * 4;
    } else {
        const bool staged = k.arithmetic == 1 && !k.old_general;
        p.form = staged ? STAGED : f16 ? GENERAL_F16 : GENERAL_F32;
        p.threads = 64 * p.tj;
        p.lds = one_wg_lds(staged, p.tj);
    }
    return p;
}

}  // namespace lemon_attn_plan
