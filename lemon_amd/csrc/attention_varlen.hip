// Bidirectional self-attention with a key length PER SEQUENCE (gfx950 only): the padding mask of a BERT text tower.
//
// Replaces, inside encode_text of the `biomed_clip` branch (lib/models/utils.py:72-78 -> open_clip HFTextEncoder -> HF
// BertSelfAttention called with attention_mask = ids != pad), the chain
//   view/permute(qkv) -> softmax(q k^T / sqrt(64) + (1 - mask) * min) v -> transpose -> reshape
// for captions padded BEHIND their last token: sequence b of qkv[B, L, 3, H, 64] holds n_b = clamp(lengths[b], 1, L) tokens.
//   * rows t <  n_b of out[B, L, H*64] (any output form of attention.hip): attention of query t over keys 0 .. n_b - 1;
//   * rows t >= n_b: zeros;
//   * K, V and Q rows t >= n_b are never loaded.
// One workgroup per (sequence, head) as in attention.hip (seq_len <= 288).  The three kernels are the VL = true instantiations
// of the bodies in attention_hd64.hpp, whose VL = false instantiations are k_attention_hd64_short, k_attention_hd64<SPLIT, false>
// and k_attention_hd64_f16 of attention.hip: what per-sequence lengths change is said there.  This unit holds the kernels'
// entry points and their dispatch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "attention_hd64.hpp"

namespace {

template <int TJ, int SPLIT, bool F16>
__global__ __launch_bounds__(64 * TJ, 3) void k_attnvl_short(const float *__restrict__ qkv, int L, int H, const int *__restrict__ lengths,
                                                            float *__restrict__ out) {
    attention_short<TJ, SPLIT, F16, true>(qkv, L, H, 0, lengths, out);
}

template <int SPLIT>
__global__ __launch_bounds__(576) void k_attnvl_f32(const float *__restrict__ qkv, int L, int H, const int *__restrict__ lengths,
                                                    float *__restrict__ out) {
    attention_general<SPLIT, false, true>(qkv, L, H, 0, lengths, out);
}

// (also what lemon_attention_set_f16(2) runs here: the first general kernel with fp16 arithmetic gives the same bits)
template <int SPLIT>
__global__ __launch_bounds__(576, 4) void k_attnvl_f16(const float *__restrict__ qkv, int L, int H, const int *__restrict__ lengths,
                                                     float *__restrict__ out) {
    attention_staged<SPLIT, true>(qkv, L, H, 0, lengths, out);
}

namespace plan = lemon_attn_plan;
static_assert(plan::HD == HD && plan::PITCH == PITCH, "attention_plan.hpp mirrors attention_hd64.hpp");

// the instantiations, four output forms (SPLIT 0 .. 3) per plan::Form of this unit, in the order of plan::FACTS[].slot
typedef void (*VarlenKernel)(const float *, int, int, const int *, float *);
constexpr VarlenKernel KERNELS[] = {
    k_attnvl_short<1, 0, false>, k_attnvl_short<1, 1, false>, k_attnvl_short<1, 2, false>, k_attnvl_short<1, 3, false>,
    k_attnvl_short<1, 0, true>, k_attnvl_short<1, 1, true>, k_attnvl_short<1, 2, true>, k_attnvl_short<1, 3, true>,
    k_attnvl_short<2, 0, false>, k_attnvl_short<2, 1, false>, k_attnvl_short<2, 2, false>, k_attnvl_short<2, 3, false>,
    k_attnvl_short<2, 0, true>, k_attnvl_short<2, 1, true>, k_attnvl_short<2, 2, true>, k_attnvl_short<2, 3, true>,
    k_attnvl_f32<0>, k_attnvl_f32<1>, k_attnvl_f32<2>, k_attnvl_f32<3>,
    k_attnvl_f16<0>, k_attnvl_f16<1>, k_attnvl_f16<2>, k_attnvl_f16<3>,
};
constexpr int N_KERNELS = sizeof(KERNELS) / sizeof(KERNELS[0]);
static_assert(N_KERNELS == 4 * (plan::FACTS[plan::VL_F16].slot + 1) && plan::FACTS[plan::VL_SHORT1_F32].slot == 0, "four kernels per plan::Form of this unit");
LemonLdsAttr g_attr[N_KERNELS];


// split = the output form 0 .. 3 (out_dev: see the entries)
int varlen_entry(int split, const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim, const int32_t *lengths_dev, float *out_dev,
                 void *stream) {
    const plan::Plan p = plan::plan(lemon_attention_thread().knobs, batch, seq_len, heads, head_dim, split, true);
    if (p.early) return lemon_attention_refuse(p.early);
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(qkv_dev && out_dev, "null pointer");
    LEMON_REQUIRE((((uintptr_t)qkv_dev) & 15) == 0 && (((uintptr_t)out_dev) & 15) == 0, "16-byte alignment");
    LEMON_REQUIRE((((uintptr_t)lengths_dev) & 3) == 0, "lengths: 4-byte alignment");
    if (p.late) return lemon_attention_refuse(p.late);
    return lemon_attention_launch(KERNELS, g_attr, p, split, (hipStream_t)stream, qkv_dev, seq_len, heads, lengths_dev, out_dev);
}

}  // namespace

// lengths_dev == NULL: the plain entry point, bidirectional (identical bits; it applies its own argument checks)
extern "C" int lemon_attention_f32_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                          const int32_t *lengths_dev, float *out_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f32(qkv_dev, batch, seq_len, heads, head_dim, 0, out_dev, stream);
    return varlen_entry(0, qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, out_dev, stream);
}

extern "C" int lemon_attention_split3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                             const int32_t *lengths_dev, uint16_t *out6_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_split3(qkv_dev, batch, seq_len, heads, head_dim, 0, out6_dev, stream);
    return varlen_entry(1, qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(out6_dev), stream);
}

extern "C" int lemon_attention_f16x3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                            const int32_t *lengths_dev, uint16_t *out3_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f16x3(qkv_dev, batch, seq_len, heads, head_dim, 0, out3_dev, stream);
    return varlen_entry(2, qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(out3_dev), stream);
}

extern "C" int lemon_attention_f16x3t_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                             const int32_t *lengths_dev, uint16_t *outt_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f16x3t(qkv_dev, batch, seq_len, heads, head_dim, 0, outt_dev, stream);
    return varlen_entry(3, qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(outt_dev), stream);
}
