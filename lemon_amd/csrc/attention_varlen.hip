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
#include <mutex>
#include <algorithm>

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

template <int SPLIT>
int attention_varlen_impl(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim, const int32_t *lengths_dev,
                          float *out_dev, void *stream) {
    LEMON_REQUIRE(batch >= 0 && seq_len > 0 && heads > 0, "batch >= 0, seq_len > 0, heads > 0");
    LEMON_REQUIRE(head_dim == HD, "per-sequence lengths: head_dim must be 64 (in every lemon_attention_set_head_dims mode)");
    LEMON_REQUIRE(seq_len <= 288, "per-sequence lengths: seq_len <= 288 (the streaming kernels take no lengths)");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(qkv_dev && out_dev, "null pointer");
    LEMON_REQUIRE((((uintptr_t)qkv_dev) & 15) == 0 && (((uintptr_t)out_dev) & 15) == 0, "16-byte alignment");
    LEMON_REQUIRE((((uintptr_t)lengths_dev) & 3) == 0, "lengths: 4-byte alignment");
    LEMON_REQUIRE(batch * heads < (int64_t)1 << 31, "batch * heads < 2^31");
    LEMON_REQUIRE((int64_t)288 * 3 * heads * HD * 4 < (int64_t)1 << 32, "heads < 19 418 (32-bit offsets inside a head's slice)");
    const int tj = (seq_len + 31) / 32;
    const bool f16 = lemon_attention_f16_mode() != 0;
    const dim3 grid((unsigned)(batch * heads));
    hipStream_t st = (hipStream_t)stream;
    if (tj <= 2) {
        if (f16) {
            if (tj == 1) hipLaunchKernelGGL((k_attnvl_short<1, SPLIT, true>), grid, dim3(64), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
            else         hipLaunchKernelGGL((k_attnvl_short<2, SPLIT, true>), grid, dim3(128), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
        } else {
            if (tj == 1) hipLaunchKernelGGL((k_attnvl_short<1, SPLIT, false>), grid, dim3(64), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
            else         hipLaunchKernelGGL((k_attnvl_short<2, SPLIT, false>), grid, dim3(128), 0, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
        }
        LEMON_HIP_CHECK(hipGetLastError());
        return LEMON_OK;
    }
    const int tb = (tj <= 5 || tj > 8) ? tj : (tj + 1) / 2;
    const size_t lds = f16 ? std::max((size_t)4 * 32 * tb * 128, (size_t)32 * tj * 256) : (size_t)2 * 32 * tj * PITCH * sizeof(float);
    {   // the attribute is per DEVICE (and per instantiation): one flag per device index, under a lock
        static std::mutex mu;
        static bool attr_set[64] = {};
        int dev = 0;
        LEMON_HIP_CHECK(hipGetDevice(&dev));
        LEMON_REQUIRE(dev >= 0 && dev < 64, "device index");
        std::lock_guard<std::mutex> lock(mu);
        if (!attr_set[dev]) {
            LEMON_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_attnvl_f32<SPLIT>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            LEMON_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_attnvl_f16<SPLIT>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            attr_set[dev] = true;
        }
    }
    if (f16) hipLaunchKernelGGL((k_attnvl_f16<SPLIT>), grid, dim3(64 * tj), lds, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
    else hipLaunchKernelGGL((k_attnvl_f32<SPLIT>), grid, dim3(64 * tj), lds, st, qkv_dev, seq_len, heads, lengths_dev, out_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

}  // namespace

// lengths_dev == NULL: the plain entry point, bidirectional (identical bits; it applies its own argument checks)
extern "C" int lemon_attention_f32_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                          const int32_t *lengths_dev, float *out_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f32(qkv_dev, batch, seq_len, heads, head_dim, 0, out_dev, stream);
    return attention_varlen_impl<0>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, out_dev, stream);
}

extern "C" int lemon_attention_split3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                             const int32_t *lengths_dev, uint16_t *out6_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_split3(qkv_dev, batch, seq_len, heads, head_dim, 0, out6_dev, stream);
    return attention_varlen_impl<1>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(out6_dev), stream);
}

extern "C" int lemon_attention_f16x3_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                            const int32_t *lengths_dev, uint16_t *out3_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f16x3(qkv_dev, batch, seq_len, heads, head_dim, 0, out3_dev, stream);
    return attention_varlen_impl<2>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(out3_dev), stream);
}

extern "C" int lemon_attention_f16x3t_varlen(const float *qkv_dev, int64_t batch, int seq_len, int heads, int head_dim,
                                             const int32_t *lengths_dev, uint16_t *outt_dev, void *stream) {
    if (!lengths_dev) return lemon_attention_f16x3t(qkv_dev, batch, seq_len, heads, head_dim, 0, outt_dev, stream);
    return attention_varlen_impl<3>(qkv_dev, batch, seq_len, heads, head_dim, lengths_dev, reinterpret_cast<float *>(outt_dev), stream);
}
