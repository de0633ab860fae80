// tokenize.hip -- caption tokenizers on gfx950 (include/lemon_hip.h: lemon_tokenize): CLIP BPE and BERT WordPiece.
//
// One wave64 per caption (a workgroup is one wave; rows are strided over the grid).  All per-byte and per-word rules are the
// functions of tokenize_core.hpp; this file only spreads them over the lanes:
//   1. envelope: lane l checks bytes l, l + 64, ...; the reason bits are OR-ed across the wave.
//   2. token list: 64 bytes at a time, every lane flags "opens a token" / "closes a token" for its byte (look-backs and
//      look-aheads read the text, so a token or a contraction across a chunk edge is nothing special); two ballots, and the
//      lane's rank among the set bits below it (popcount) plus the running count is the token's slot in the LDS lists.  Only
//      the first ctx - 1 tokens can reach the row: the sweep stops there.
//   3. words: 64 tokens at a time, a lane per word.  Its symbols live in LDS, column `lane` of a [64][64] uint16 array (lane-
//      consecutive, so the wave's accesses of one step fall into 32 banks); the pair / piece probes are global loads of 16-byte
//      slots that stay in L2 (the tables are a few MB at most).  The merge loop, the prefix match and the probes are bounded by
//      the word's symbols and the table's longest probe sequence; no lane reads what another lane writes.
//   4. an inclusive shuffle scan of the words' id counts gives every word its offset in the row, staged in LDS; the loop over
//      groups ends once ctx - 1 ids exist.  Then the row is written once, coalesced: first token, ids, last token, padding.
// A declined row is written as padding with length 0 and its status.
#include "common.hpp"
#include "tokenize_core.hpp"

#include <mutex>
#include <new>

struct lemon_tokenizer {
    TokHostTable host;
    std::mutex lock;
    int device = -1;              // where the table was uploaded (-1: nowhere yet)
    void *dev_slots = nullptr;
    uint8_t *dev_blob = nullptr;
    TokTable dev{};
};

__global__ __launch_bounds__(64) void k_tokenize(TokTable T, const uint8_t *__restrict__ text, int64_t text_bytes,
                                                 const int64_t *__restrict__ offsets, int64_t rows, int ctx, int pad,
                                                 int64_t *__restrict__ ids, int32_t *__restrict__ length, uint8_t *__restrict__ status) {
    __shared__ uint16_t s_start[LEMON_TOKENIZE_MAX_CTX], s_end[LEMON_TOKENIZE_MAX_CTX], s_row[LEMON_TOKENIZE_MAX_CTX];
    __shared__ uint16_t s_sym[LEMON_TOKENIZE_MAX_WORD * 64];
    const int lane = threadIdx.x, need = ctx - 1;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t o0 = offsets[r], o1 = offsets[r + 1];
        int st = 0, total = 0;
        if (o0 < 0 || o1 < o0 || o1 > text_bytes) st = LEMON_TOK_BUFFER;
        else if (o1 - o0 > LEMON_TOKENIZE_MAX_BYTES) st = LEMON_TOK_TOO_LONG;
        else {
            const uint8_t *t = text + o0;
            const int n = (int)(o1 - o0);
            uint32_t bits = 0;
            for (int i = lane; i < n; i += 64) bits |= tok_env_bits(T.kind, t, n, i);
            for (int d = 32; d > 0; d >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, d);
            st = tok_status_of(bits);
            int ntok = 0, nend = 0;
            for (int base = 0; st == 0 && base < n && nend < need; base += 64) {
                const int i = base + lane;
                const bool fs = i < n && tok_is_start(T.kind, t, n, i), fe = i < n && tok_is_end(T.kind, t, n, i);
                const unsigned long long ms = __ballot(fs), me = __ballot(fe);
                if (fs) { const int k = ntok + __popcll(ms & below); if (k < need) s_start[k] = (uint16_t)i; }
                if (fe) { const int k = nend + __popcll(me & below); if (k < need) s_end[k] = (uint16_t)(i + 1); }
                ntok += __popcll(ms);
                nend += __popcll(me);
            }
            ntok = nend < need ? nend : need;
            __syncthreads();
            for (int g = 0; st == 0 && g < ntok && total < ctx - 1; g += 64) {
                int cnt = 0;
                if (g + lane < ntok) {
                    const int a = s_start[g + lane];
                    cnt = tok_word(T, t + a, (int)s_end[g + lane] - a, s_sym + lane, 64);
                }
                if (__ballot(cnt < 0)) { st = LEMON_TOK_WORD; break; }
                int incl = cnt;
                for (int d = 1; d < 64; d <<= 1) {
                    const int up = __shfl_up(incl, d);
                    if (lane >= d) incl += up;
                }
                const int at = total + incl - cnt;
                for (int j = 0; j < cnt; ++j)
                    if (at + j < ctx - 2) s_row[1 + at + j] = s_sym[j * 64 + lane];
                total += __shfl(incl, 63);
            }
        }
        __syncthreads();
        const int kept = total < ctx - 2 ? total : ctx - 2;
        int64_t *out = ids + r * (int64_t)ctx;
        for (int p = lane; p < ctx; p += 64) out[p] = st ? (int64_t)pad : tok_row_slot(T, s_row, kept, pad, p);
        if (lane == 0) { length[r] = st ? 0 : kept + 2; status[r] = (uint8_t)st; }
        __syncthreads();
    }
}

static int tok_new(lemon_tokenizer_t **out, lemon_tokenizer **made) {
    LEMON_REQUIRE(out != nullptr, "out is null");
    *out = nullptr;
    *made = new (std::nothrow) lemon_tokenizer();
    if (!*made) { lemon_set_error("host allocation failed"); return LEMON_E_NOMEM; }
    return LEMON_OK;
}

extern "C" int lemon_tokenizer_create_bpe(const int32_t *left, const int32_t *right, const int32_t *rank, const int32_t *merged,
                                          int64_t n_merges, int32_t sot_id, int32_t eot_id, lemon_tokenizer_t **out) {
    LEMON_REQUIRE(n_merges == 0 || (left && right && rank && merged), "a merges array is null");
    lemon_tokenizer *t;
    const int rc = tok_new(out, &t);
    if (rc) return rc;
    if (!tok_build_bpe(t->host, left, right, rank, merged, n_merges, sot_id, eot_id)) {
        delete t;
        lemon_set_error("invalid argument: merges table (an id outside [0, 65535), a pair with two meanings, or no hash table within %d probes)", TOK_MAX_PROBE);
        return LEMON_E_INVALID;
    }
    *out = t;
    return LEMON_OK;
}

extern "C" int lemon_tokenizer_create_wordpiece(const uint8_t *blob, const int64_t *offsets, const int32_t *ids, int64_t n_tokens,
                                                int32_t cls_id, int32_t sep_id, int32_t unk_id, int lower_case, int max_chars,
                                                int home_buckets, lemon_tokenizer_t **out) {
    LEMON_REQUIRE(blob && offsets && ids, "a vocabulary array is null");
    lemon_tokenizer *t;
    const int rc = tok_new(out, &t);
    if (rc) return rc;
    if (!tok_build_wordpiece(t->host, blob, offsets, ids, n_tokens, cls_id, sep_id, unk_id, lower_case, max_chars, home_buckets)) {
        delete t;
        lemon_set_error("invalid argument: vocabulary (an id outside [0, 65535), unordered offsets, an empty or repeated token, or no hash table within %d probes)", TOK_MAX_PROBE);
        return LEMON_E_INVALID;
    }
    *out = t;
    return LEMON_OK;
}

extern "C" int lemon_tokenizer_free(lemon_tokenizer_t *tok) {
    if (!tok) return LEMON_OK;
    if (tok->dev_slots) (void)hipFree(tok->dev_slots);
    if (tok->dev_blob) (void)hipFree(tok->dev_blob);
    delete tok;
    return LEMON_OK;
}

extern "C" int lemon_tokenizer_table_info(const lemon_tokenizer_t *tok, int64_t *slots, int64_t *entries, int *max_probe) {
    LEMON_REQUIRE(tok && slots && entries && max_probe, "null argument");
    *slots = (int64_t)tok->host.T.mask + 1;
    *entries = tok->host.entries;
    *max_probe = tok->host.T.max_probe;
    return LEMON_OK;
}

static int tok_check_call(const void *tok, const void *text, int64_t text_bytes, const void *offsets, int64_t n, int ctx, int32_t pad_id,
                          const void *ids, const void *length, const void *status) {
    LEMON_REQUIRE(tok != nullptr, "tokenizer is null");
    LEMON_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "n out of range");
    LEMON_REQUIRE(text_bytes >= 0 && (text || text_bytes == 0), "text is null");
    LEMON_REQUIRE(ctx >= 2 && ctx <= LEMON_TOKENIZE_MAX_CTX, "ctx outside [2, LEMON_TOKENIZE_MAX_CTX]");
    LEMON_REQUIRE(pad_id >= 0, "pad_id is negative");
    LEMON_REQUIRE(n == 0 || (offsets && ids && length && status), "null argument");
    return LEMON_OK;
}

// the table in HBM, uploaded once per tokenizer
static int tok_upload(lemon_tokenizer *tok) {
    std::lock_guard<std::mutex> hold(tok->lock);
    int device = 0;
    LEMON_HIP_CHECK(hipGetDevice(&device));
    if (tok->device == device) return LEMON_OK;
    LEMON_REQUIRE(tok->device < 0, "the tokenizer's table lives on another device");
    const TokHostTable &H = tok->host;
    const size_t slot_bytes = ((size_t)H.T.mask + 1) * 16, blob_bytes = H.blob.size();
    const void *slots = H.T.kind ? (const void *)H.pieces.data() : (const void *)H.pairs.data();
    if (hipMalloc(&tok->dev_slots, slot_bytes) != hipSuccess) { tok->dev_slots = nullptr; lemon_set_error("tokenizer table allocation failed"); return LEMON_E_NOMEM; }
    LEMON_HIP_CHECK(hipMemcpy(tok->dev_slots, slots, slot_bytes, hipMemcpyHostToDevice));
    if (blob_bytes) {
        if (hipMalloc((void **)&tok->dev_blob, blob_bytes) != hipSuccess) { tok->dev_blob = nullptr; lemon_set_error("tokenizer vocabulary allocation failed"); return LEMON_E_NOMEM; }
        LEMON_HIP_CHECK(hipMemcpy(tok->dev_blob, H.blob.data(), blob_bytes, hipMemcpyHostToDevice));
    }
    tok->dev = H.T;
    tok->dev.pairs = (const TokPair *)tok->dev_slots;
    tok->dev.pieces = (const TokPiece *)tok->dev_slots;
    tok->dev.blob = tok->dev_blob;
    tok->device = device;
    return LEMON_OK;
}

extern "C" int lemon_tokenize(lemon_tokenizer_t *tok, const uint8_t *text_dev, int64_t text_bytes, const int64_t *offsets_dev, int64_t n,
                              int ctx, int32_t pad_id, int64_t *ids_dev, int32_t *length_dev, uint8_t *status_dev, void *stream) {
    int rc = tok_check_call(tok, text_dev, text_bytes, offsets_dev, n, ctx, pad_id, ids_dev, length_dev, status_dev);
    if (rc) return rc;
    if (n == 0) return LEMON_OK;
    rc = tok_upload(tok);
    if (rc) return rc;
    const int64_t grid = n < (1 << 20) ? n : (1 << 20);
    hipLaunchKernelGGL(k_tokenize, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, tok->dev, text_dev, text_bytes, offsets_dev, n, ctx,
                       (int)pad_id, ids_dev, length_dev, status_dev);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}

extern "C" int lemon_tokenize_host(const lemon_tokenizer_t *tok, const uint8_t *text, int64_t text_bytes, const int64_t *offsets, int64_t n,
                                   int ctx, int32_t pad_id, int64_t *ids, int32_t *length, uint8_t *status) {
    const int rc = tok_check_call(tok, text, text_bytes, offsets, n, ctx, pad_id, ids, length, status);
    if (rc) return rc;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t o0 = offsets[r], o1 = offsets[r + 1];
        int64_t *row = ids + r * (int64_t)ctx;
        if (o0 < 0 || o1 < o0 || o1 > text_bytes) {
            for (int p = 0; p < ctx; ++p) row[p] = pad_id;
            length[r] = 0;
            status[r] = LEMON_TOK_BUFFER;
        } else
            status[r] = (uint8_t)tok_row_host(tok->host.T, text + o0, o1 - o0, ctx, pad_id, row, &length[r]);
    }
    return LEMON_OK;
}
