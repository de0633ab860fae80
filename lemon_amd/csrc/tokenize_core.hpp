// tokenize_core.hpp -- the caption tokenizers of the text towers (CLIP byte-pair encoding: lib/models/simple_tokenizer.py:86-156
// framed by lib/models/chexzero_clip.py:481-493 and run_lemon.py:140-154; BERT WordPiece: lib/models/utils.py:72-78), restated so
// that one set of functions serves the device kernel (tokenize.hip: a wave per caption, a lane per byte and then per word), the
// host loop lemon_tokenize_host (the same functions with the lanes looped) and the sanitizer fuzz (tests/native/tokenize_fuzz.cpp).
// Plain C++: no HIP type appears here, TOK_HD is empty under a host compiler.
//
// The envelope.  A row is served when every byte is one of {9, 10, 13, 32 .. 126} and it holds no '&' and no "<|" (WordPiece:
// also no whitespace-delimited word equal to [PAD] [UNK] [CLS] [SEP] [MASK]).  On such a row html.unescape, Unicode normal forms,
// accent stripping, CJK spacing and control-character removal are the identity, the only whitespace is the four bytes above and
// lower-casing is ASCII's.  Every other row gets a LEMON_TOK_* status and is left to the caller (lemon_amd/tokenizer.py fills it
// from the Python tokenizer).  Whitespace never reaches a token, so "collapse and strip" needs no pass of its own.
//
// CLIP pattern  's|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+  on lower-cased text, as a per-byte rule: whether byte i
// opens a token depends on bytes i-4 .. i+2 only (tok_bpe_is_start), whether it closes one on whether i+1 opens one.  So a wave
// flags 64 bytes at a time and ballots the flags; every look-back reads the text itself, so a chunk edge needs no special case.
//   other byte (the apostrophe included)   opens iff the byte before it is not of the other class (else it continues that run)
//   apostrophe that opens                  is a contraction of 2 or 3 bytes when the letters after it say so (tok_bpe_contraction)
//   digit                                  always opens (and closes) a token
//   letter                                 inside a contraction: never; right after one: always; else iff the byte before is no letter
// WordPiece words: whitespace-delimited, every ASCII punctuation byte a word of its own.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/lemon_hip.h"

#if defined(__HIPCC__)
#define TOK_HD __host__ __device__ inline
#else
#define TOK_HD inline
#endif

#define TOK_MAX_PROBE 64          // longest probe sequence a table may need (the builders grow the table or refuse)
#define TOK_EMPTY 0xffffffffu
#define TOK_HASH_P 0x01000193u    // rolling string hash h' = h * P + byte + 1 (mod 2^32); P is odd, so a byte can be taken off the end again
#define TOK_HASH_PINV 0x359c449bu // P * PINV == 1 (mod 2^32)
#define TOK_HASH_CONT 0x240038d0u // the hash of "##"

struct TokPair { uint32_t key, rank, id, pad; };   // key = left id << 16 | right id, compared exactly; empty slot: key == TOK_EMPTY
struct TokPiece { uint32_t off, len, id, pad; };   // the piece is blob[off, off + len), compared byte for byte; empty slot: len == TOK_EMPTY
struct TokTable {
    int32_t kind;                 // 0 CLIP BPE, 1 WordPiece
    uint32_t mask;                // slots - 1 (a power of two, at least twice the entries)
    uint32_t home_mask;           // bits of the mixed hash that choose the home slot (all ones; the collision test hook narrows it)
    int32_t max_probe;            // 1 + the largest displacement in the table, <= TOK_MAX_PROBE
    const TokPair *pairs;
    const TokPiece *pieces;
    const uint8_t *blob;
    int32_t first, last;          // <|startoftext|>, <|endoftext|>  /  [CLS], [SEP]
    int32_t unk, lower, max_chars;
};

TOK_HD uint32_t tok_mix(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
// 0 whitespace, 1 letter, 2 digit, 3 other printable, 4 outside the envelope
TOK_HD int tok_class(uint32_t b) {
    if (b == 32 || b == 9 || b == 10 || b == 13) return 0;
    if (b < 33 || b > 126) return 4;
    if ((b | 32) >= 97 && (b | 32) <= 122) return 1;
    if (b >= 48 && b <= 57) return 2;
    return 3;
}
TOK_HD uint32_t tok_lower(uint32_t b) { return (b >= 65 && b <= 90) ? b + 32 : b; }
TOK_HD bool tok_punct(uint32_t b) { return (b >= 33 && b <= 47) || (b >= 58 && b <= 64) || (b >= 91 && b <= 96) || (b >= 123 && b <= 126); }

// [PAD] [UNK] [CLS] [SEP] [MASK] as a whole whitespace-delimited word starting at byte i (BasicTokenizer's never_split)
TOK_HD bool tok_wp_reserved_at(const uint8_t *t, int n, int i) {
    if (t[i] != '[' || (i > 0 && tok_class(t[i - 1]) != 0)) return false;
    int len = 0;
    if (i + 4 < n && t[i + 4] == ']') {
        const uint32_t a = t[i + 1], b = t[i + 2], c = t[i + 3];
        if ((a == 'P' && b == 'A' && c == 'D') || (a == 'U' && b == 'N' && c == 'K') || (a == 'C' && b == 'L' && c == 'S') ||
            (a == 'S' && b == 'E' && c == 'P')) len = 5;
    }
    if (!len && i + 5 < n && t[i + 5] == ']' && t[i + 1] == 'M' && t[i + 2] == 'A' && t[i + 3] == 'S' && t[i + 4] == 'K') len = 6;
    return len && (i + len == n || tok_class(t[i + len]) == 0);
}
// the reasons byte i puts its row outside the envelope, one bit per LEMON_TOK_* code
TOK_HD uint32_t tok_env_bits(int kind, const uint8_t *t, int n, int i) {
    const uint32_t b = t[i];
    uint32_t bits = 0;
    if (tok_class(b) == 4) bits |= 1u << LEMON_TOK_NON_ASCII;
    if (b == '&') bits |= 1u << LEMON_TOK_AMPERSAND;
    if (b == '<' && i + 1 < n && t[i + 1] == '|') bits |= 1u << LEMON_TOK_SPECIAL;
    if (kind == 1 && b == '[' && tok_wp_reserved_at(t, n, i)) bits |= 1u << LEMON_TOK_SPECIAL;
    return bits;
}
TOK_HD int tok_status_of(uint32_t bits) {        // the lowest code present
    for (int c = 1; c < 8; ++c)
        if (bits >> c & 1) return c;
    return 0;
}

// length (2 or 3 bytes) of the contraction that the apostrophe at byte j opens, 0 when there is none
TOK_HD int tok_bpe_contraction(const uint8_t *t, int n, int j) {
    if (j < 0 || j + 1 >= n || t[j] != '\'') return 0;
    if (j > 0 && tok_class(t[j - 1]) == 3) return 0;          // the apostrophe continues a run of other bytes
    const uint32_t a = tok_lower(t[j + 1]);
    if (a == 's' || a == 't' || a == 'm' || a == 'd') return 2;
    if (j + 2 < n) {
        const uint32_t b = tok_lower(t[j + 2]);
        if ((a == 'r' && b == 'e') || (a == 'v' && b == 'e') || (a == 'l' && b == 'l')) return 3;
    }
    return 0;
}
TOK_HD bool tok_bpe_is_start(const uint8_t *t, int n, int i) {
    const int c = tok_class(t[i]);
    if (c == 0) return false;
    if (c == 2) return true;
    const int before = i > 0 ? tok_class(t[i - 1]) : 0;
    if (c != 1) return before != 3;
    if (tok_bpe_contraction(t, n, i - 1)) return false;
    const int two = tok_bpe_contraction(t, n, i - 2);
    if (two) return two == 2;
    if (tok_bpe_contraction(t, n, i - 3) == 3) return true;
    return before != 1;
}
TOK_HD bool tok_wp_is_start(const uint8_t *t, int n, int i) {
    if (tok_class(t[i]) == 0) return false;
    return tok_punct(t[i]) || i == 0 || tok_class(t[i - 1]) == 0 || tok_punct(t[i - 1]);
}
TOK_HD bool tok_is_start(int kind, const uint8_t *t, int n, int i) { return kind ? tok_wp_is_start(t, n, i) : tok_bpe_is_start(t, n, i); }
TOK_HD bool tok_is_end(int kind, const uint8_t *t, int n, int i) {
    if (tok_class(t[i]) == 0) return false;
    if (i + 1 >= n || tok_class(t[i + 1]) == 0) return true;
    return tok_is_start(kind, t, n, i + 1);
}

TOK_HD bool tok_pair_probe(const TokTable &T, uint32_t key, uint32_t &rank, uint32_t &id) {
    const uint32_t home = tok_mix(key) & T.home_mask;
    for (int p = 0; p < T.max_probe; ++p) {
        const TokPair e = T.pairs[(home + p) & T.mask];
        if (e.key == key) { rank = e.rank; id = e.id; return true; }
        if (e.key == TOK_EMPTY) return false;
    }
    return false;
}
// One CLIP word: s[0], s[stride], ... hold its n symbols (byte-alphabet ids, the last one + 256).  Each round finds the adjacent
// pair of the lowest rank and merges all its non-overlapping occurrences from the left; at most n - 1 rounds.  Returns the count.
TOK_HD int tok_bpe_merge(const TokTable &T, uint16_t *s, int stride, int n) {
    for (int round = n - 1; round > 0 && n > 1; --round) {
        uint32_t best = TOK_EMPTY, bl = 0, br = 0, bid = 0, left = s[0];
        for (int i = 1; i < n; ++i) {
            const uint32_t right = s[i * stride];
            uint32_t rank, id;
            if (tok_pair_probe(T, left << 16 | right, rank, id) && rank < best) { best = rank; bl = left; br = right; bid = id; }
            left = right;
        }
        if (best == TOK_EMPTY) break;
        int o = 0;
        for (int i = 0; i < n; ++o) {
            const uint32_t a = s[i * stride];
            if (i + 1 < n && a == bl && s[(i + 1) * stride] == br) { s[o * stride] = (uint16_t)bid; i += 2; }
            else { s[o * stride] = (uint16_t)a; i += 1; }
        }
        n = o;
    }
    return n;
}
TOK_HD int tok_bpe_word(const TokTable &T, const uint8_t *w, int len, uint16_t *s, int stride) {
    for (int j = 0; j < len; ++j) s[j * stride] = (uint16_t)(tok_lower(w[j]) - 33 + (j == len - 1 ? 256 : 0));
    return tok_bpe_merge(T, s, stride, len);
}

// the piece ("##" when cont) + lower(w[0, len)) in the vocabulary: hash to a home slot, then the stored bytes decide
TOK_HD bool tok_piece_probe(const TokTable &T, uint32_t hash, const uint8_t *w, int len, bool cont, uint32_t &id) {
    const uint32_t home = tok_mix(hash) & T.home_mask, total = (uint32_t)len + (cont ? 2u : 0u);
    for (int p = 0; p < T.max_probe; ++p) {
        const TokPiece e = T.pieces[(home + p) & T.mask];
        if (e.len == TOK_EMPTY) return false;
        if (e.len != total) continue;
        const uint8_t *s = T.blob + e.off;
        bool same = !cont || (s[0] == '#' && s[1] == '#');
        if (cont) s += 2;
        for (int k = 0; same && k < len; ++k) same = s[k] == (T.lower ? tok_lower(w[k]) : w[k]);
        if (same) { id = e.id; return true; }
    }
    return false;
}
// One WordPiece word: longest prefix first, "##" continuations, any miss -> [UNK].  Pieces go to out[0], out[stride], ...;
// returns their count, or -1 when the word has more than cap pieces.
TOK_HD int tok_wp_word(const TokTable &T, const uint8_t *w, int len, uint16_t *out, int stride, int cap) {
    if (len > T.max_chars) { out[0] = (uint16_t)T.unk; return 1; }
    int start = 0, cnt = 0;
    while (start < len) {
        uint32_t h = start ? TOK_HASH_CONT : 0u, id = 0;
        for (int k = start; k < len; ++k) h = h * TOK_HASH_P + (T.lower ? tok_lower(w[k]) : w[k]) + 1u;
        int end = len;
        bool hit = false;
        while (end > start) {
            hit = tok_piece_probe(T, h, w + start, end - start, start > 0, id);
            if (hit) break;
            --end;
            h = (h - ((T.lower ? tok_lower(w[end]) : w[end]) + 1u)) * TOK_HASH_PINV;
        }
        if (!hit) { out[0] = (uint16_t)T.unk; return 1; }
        if (cnt >= cap) return -1;
        out[cnt * stride] = (uint16_t)id;
        ++cnt;
        start = end;
    }
    return cnt;
}
TOK_HD int tok_word(const TokTable &T, const uint8_t *w, int len, uint16_t *s, int stride) {
    if (T.kind) return tok_wp_word(T, w, len, s, stride, LEMON_TOKENIZE_MAX_WORD);
    return len > LEMON_TOKENIZE_MAX_WORD ? -1 : tok_bpe_word(T, w, len, s, stride);
}
// slot p of a served row that holds `kept` = min(ids, ctx - 2) word ids in row[1 .. kept]
TOK_HD int64_t tok_row_slot(const TokTable &T, const uint16_t *row, int kept, int pad, int p) {
    return p == 0 ? T.first : p <= kept ? (int64_t)row[p] : p == kept + 1 ? T.last : pad;
}

// ---- host only: the wave's walk with its 64 lanes looped, and the table builders ----------------------------------------------
#include <vector>

// One row on the host, step for step what k_tokenize does: flags per 64-byte chunk compacted into the token list, then groups of
// 64 words, an exclusive prefix sum of their id counts and the early exit once ctx - 1 ids exist.  Returns the status; a
// declined row is all pad_id with length 0.
inline int tok_row_host(const TokTable &T, const uint8_t *t, int64_t n64, int ctx, int pad, int64_t *ids, int32_t *length) {
    int st = 0;
    const int need = ctx - 1;
    std::vector<uint16_t> starts(need), ends(need), sym((size_t)64 * LEMON_TOKENIZE_MAX_WORD), row(ctx);
    int total = 0;
    if (n64 > LEMON_TOKENIZE_MAX_BYTES) st = LEMON_TOK_TOO_LONG;
    else {
        const int n = (int)n64;
        uint32_t bits = 0;
        for (int i = 0; i < n; ++i) bits |= tok_env_bits(T.kind, t, n, i);
        st = tok_status_of(bits);
        int ntok = 0, nend = 0;
        for (int base = 0; st == 0 && base < n && nend < need; base += 64) {
            int s_here = 0, e_here = 0;
            for (int lane = 0; lane < 64 && base + lane < n; ++lane) {
                const int i = base + lane;
                if (tok_is_start(T.kind, t, n, i)) { if (ntok + s_here < need) starts[ntok + s_here] = (uint16_t)i; ++s_here; }
                if (tok_is_end(T.kind, t, n, i)) { if (nend + e_here < need) ends[nend + e_here] = (uint16_t)(i + 1); ++e_here; }
            }
            ntok += s_here; nend += e_here;
        }
        ntok = nend < need ? nend : need;
        for (int g = 0; st == 0 && g < ntok && total < ctx - 1; g += 64) {
            int cnt[64];
            bool bad = false;
            for (int lane = 0; lane < 64; ++lane) {
                cnt[lane] = 0;
                if (g + lane >= ntok) continue;
                const int a = starts[g + lane], len = ends[g + lane] - a;
                cnt[lane] = tok_word(T, t + a, len, &sym[lane], 64);
                if (cnt[lane] < 0) { bad = true; cnt[lane] = 0; }
            }
            if (bad) { st = LEMON_TOK_WORD; break; }
            for (int lane = 0; lane < 64; ++lane) {
                for (int j = 0; j < cnt[lane]; ++j)
                    if (total + j < ctx - 2) row[1 + total + j] = sym[(size_t)j * 64 + lane];
                total += cnt[lane];
            }
        }
    }
    const int kept = total < ctx - 2 ? total : ctx - 2;
    for (int p = 0; p < ctx; ++p) ids[p] = st ? pad : tok_row_slot(T, row.data(), kept, pad, p);
    *length = st ? 0 : kept + 2;
    return st;
}

struct TokHostTable {
    std::vector<TokPair> pairs;
    std::vector<TokPiece> pieces;
    std::vector<uint8_t> blob;
    int64_t entries = 0;
    TokTable T{};
    void bind() { T.pairs = pairs.data(); T.pieces = pieces.data(); T.blob = blob.data(); }
};
inline uint32_t tok_slots_for(int64_t entries) {
    uint32_t slots = 4;
    while ((int64_t)slots < 2 * entries) slots <<= 1;
    return slots;
}
// Pair table of a CLIP vocabulary: merge m joins the symbols left[m], right[m] (ids, < 65535) at rank[m] into merged[m].  The
// caller drops merges whose parts or result have no id -- they can never fire.  Load factor <= 0.5; a key that would sit more
// than TOK_MAX_PROBE slots from home doubles the table (up to 8 times).  False: bad ids, a key with two meanings, or no table
// within the probe limit.
inline bool tok_build_bpe(TokHostTable &H, const int32_t *left, const int32_t *right, const int32_t *rank, const int32_t *merged,
                          int64_t n, int32_t sot, int32_t eot) {
    if (n < 0 || n > (1 << 24) || sot < 0 || sot >= 65535 || eot < 0 || eot >= 65535) return false;
    for (int64_t m = 0; m < n; ++m)
        if (left[m] < 0 || left[m] >= 65535 || right[m] < 0 || right[m] >= 65535 || merged[m] < 0 || merged[m] >= 65535 || rank[m] < 0) return false;
    uint32_t slots = tok_slots_for(n);
    for (int grow = 0; grow < 8; ++grow, slots <<= 1) {
        H.pairs.assign(slots, TokPair{TOK_EMPTY, 0, 0, 0});
        int worst = 0;
        int64_t entries = 0;
        bool ok = true;
        for (int64_t m = 0; ok && m < n; ++m) {
            const uint32_t key = (uint32_t)left[m] << 16 | (uint32_t)right[m], home = tok_mix(key);
            int p = 0;
            for (; p < TOK_MAX_PROBE; ++p) {
                TokPair &e = H.pairs[(home + p) & (slots - 1)];
                if (e.key == key) {
                    if (e.rank != (uint32_t)rank[m] || e.id != (uint32_t)merged[m]) return false;
                    break;
                }
                if (e.key == TOK_EMPTY) { e = TokPair{key, (uint32_t)rank[m], (uint32_t)merged[m], 0}; ++entries; break; }
            }
            if (p == TOK_MAX_PROBE) ok = false;
            else if (p + 1 > worst) worst = p + 1;
        }
        if (!ok) continue;
        H.entries = entries;
        H.T = TokTable{};
        H.T.kind = 0; H.T.mask = slots - 1; H.T.home_mask = 0xffffffffu; H.T.max_probe = worst > 0 ? worst : 1;
        H.T.first = sot; H.T.last = eot;
        H.bind();
        return true;
    }
    return false;
}
// Piece table of a WordPiece vocabulary: token v is blob[offsets[v], offsets[v + 1]) with id ids[v] (< 65535).  home_buckets: 0, or
// a power of two that limits the home slots (the tests force collisions with 2).  False: bad ids or offsets, an empty or
// repeated token, or no table within the probe limit.
inline bool tok_build_wordpiece(TokHostTable &H, const uint8_t *blob, const int64_t *offsets, const int32_t *ids, int64_t n, int32_t cls,
                                int32_t sep, int32_t unk, int lower, int max_chars, int home_buckets) {
    if (n < 1 || n > (1 << 24) || offsets[0] != 0 || max_chars < 1) return false;
    if (home_buckets < 0 || (home_buckets & (home_buckets - 1))) return false;
    for (int32_t v : {cls, sep, unk})
        if (v < 0 || v >= 65535) return false;
    for (int64_t v = 0; v < n; ++v)
        if (offsets[v + 1] <= offsets[v] || offsets[v + 1] > 0x7fffffff || ids[v] < 0 || ids[v] >= 65535) return false;
    H.blob.assign(blob, blob + offsets[n]);
    const uint32_t home_mask = home_buckets ? (uint32_t)home_buckets - 1 : 0xffffffffu;
    uint32_t slots = tok_slots_for(n);
    for (int grow = 0; grow < 8; ++grow, slots <<= 1) {
        H.pieces.assign(slots, TokPiece{0, TOK_EMPTY, 0, 0});
        int worst = 0;
        bool ok = true;
        for (int64_t v = 0; ok && v < n; ++v) {
            const uint32_t off = (uint32_t)offsets[v], len = (uint32_t)(offsets[v + 1] - offsets[v]);
            uint32_t h = 0;
            for (uint32_t k = 0; k < len; ++k) h = h * TOK_HASH_P + blob[off + k] + 1u;
            const uint32_t home = tok_mix(h) & home_mask;
            int p = 0;
            for (; p < TOK_MAX_PROBE; ++p) {
                TokPiece &e = H.pieces[(home + p) & (slots - 1)];
                if (e.len == TOK_EMPTY) { e = TokPiece{off, len, (uint32_t)ids[v], 0}; break; }
                if (e.len == len && memcmp(blob + e.off, blob + off, len) == 0) return false;
            }
            if (p == TOK_MAX_PROBE) ok = false;
            else if (p + 1 > worst) worst = p + 1;
        }
        if (!ok) continue;
        H.entries = n;
        H.T = TokTable{};
        H.T.kind = 1; H.T.mask = slots - 1; H.T.home_mask = home_mask; H.T.max_probe = worst;
        H.T.first = cls; H.T.last = sep; H.T.unk = unk; H.T.lower = lower ? 1 : 0; H.T.max_chars = max_chars;
        H.bind();
        return true;
    }
    return false;
}
