// tokenize_fuzz.cpp -- property fuzz of the device tokenizers' shared core (lemon_amd/csrc/tokenize_core.hpp) on the CPU, built
// with g++ under AddressSanitizer + UBSan by tests/test_tokenize_device_host.py (the kernel runs the same functions; GPU
// sanitizers are not available on the pool).  Random merges tables and WordPiece vocabularies, random rows of arbitrary bytes in
// heap buffers of exactly the row's size, random context lengths.  Checked: the status is the documented one for the row's
// bytes; a declined row is padding with length 0; a served row is framed (first, ids, last, padding), every id belongs to the
// vocabulary, and -- CLIP, rows that were not cut -- the ids' strings spell the row's non-space bytes, lower-cased.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/tokenize_fuzz.cpp -o tokenize_fuzz && ./tokenize_fuzz [cases] [seed]
#include "../../lemon_amd/csrc/tokenize_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

#define FAIL(...) do { fprintf(stderr, "FAIL case %d: ", c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

static std::string random_row(std::mt19937 &g, int kind_of_row) {
    static const char *pools[] = {"abcde'.-1 abcde  \t", "'''stmdrevl ' .1!?", " \t\n\r", "abc[]PADUNKCLSEPMASK [PAD] [MASK] "};
    std::string s;
    int len = (int)(g() % 120);
    if (kind_of_row == 7) len = 4000 + (int)(g() % 200);
    if (kind_of_row == 8) len = 60 + (int)(g() % 12);
    for (int i = 0; i < len; ++i) {
        if (kind_of_row == 8) s.push_back("ab"[g() % 2]);                        // one long word around the 64-symbol limit
        else if (kind_of_row < 4) { const char *p = pools[kind_of_row]; s.push_back(p[g() % strlen(p)]); }
        else if (kind_of_row == 4) s.push_back((char)(g() % 256));               // any byte
        else if (kind_of_row == 5) s.push_back("ab&<| '"[g() % 7]);
        else s.push_back((char)(32 + g() % 95));
    }
    return s;
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937 g(argc > 2 ? (unsigned)atoll(argv[2]) : 1u);
    for (int c = 0; c < cases; ++c) {
        const int kind = c & 1;
        TokHostTable H;
        std::vector<std::string> str_of(65536);            // id -> string, CLIP only
        int vocab = 0;
        if (kind == 0) {
            // ids: 0 .. 93 the printable bytes, 256 .. 349 the same as a word's last symbol, 512 + m the merges
            std::vector<int32_t> left, right, rank, merged;
            std::map<std::string, int> id_of;
            std::vector<std::string> inner, fin;
            for (int b = 33; b <= 126; ++b) {
                const std::string ch(1, (char)b);
                id_of[ch] = b - 33; str_of[b - 33] = ch; inner.push_back(ch);
                id_of[ch + "\n"] = b - 33 + 256; str_of[b - 33 + 256] = ch; fin.push_back(ch + "\n");      // "\n" marks </w>
            }
            const int want = (int)(g() % 300);
            std::map<std::pair<int, int>, int> seen;
            for (int m = 0; m < want; ++m) {
                const std::string a = inner[g() % inner.size()];
                const bool last = g() % 3 == 0;
                const std::string b = last ? fin[g() % fin.size()] : inner[g() % inner.size()];
                if (a.size() + b.size() > 10 || seen.count({id_of[a], id_of[b]}) || id_of.count(a + b)) continue;
                seen[{id_of[a], id_of[b]}] = 1;
                left.push_back(id_of[a]); right.push_back(id_of[b]); rank.push_back(m); merged.push_back(512 + m);
                id_of[a + b] = 512 + m;
                std::string plain = a + b;
                if (last) plain.pop_back();
                str_of[512 + m] = plain;
                (last ? fin : inner).push_back(a + b);
            }
            vocab = 512 + want + 2;
            if (!tok_build_bpe(H, left.data(), right.data(), rank.data(), merged.data(), (int64_t)left.size(), vocab - 2, vocab - 1)) FAIL("bpe table refused");
            if (2 * H.entries > (int64_t)H.T.mask + 1 || H.T.max_probe > TOK_MAX_PROBE) FAIL("bpe table shape");
        } else {
            std::vector<std::string> toks = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"};
            std::map<std::string, int> seen;
            for (auto &t : toks) seen[t] = 1;
            const int want = 5 + (int)(g() % 200);
            while ((int)toks.size() < want) {
                std::string t = g() % 2 ? "##" : "";
                const int len = 1 + (int)(g() % 4);
                for (int i = 0; i < len; ++i) t.push_back("abcde.-1A"[g() % 9]);
                if (!seen.count(t)) { seen[t] = 1; toks.push_back(t); }
            }
            std::vector<uint8_t> blob;
            std::vector<int64_t> off(1, 0);
            std::vector<int32_t> ids;
            for (size_t v = 0; v < toks.size(); ++v) { blob.insert(blob.end(), toks[v].begin(), toks[v].end()); off.push_back((int64_t)blob.size()); ids.push_back((int32_t)v); }
            vocab = (int)toks.size();
            const int buckets = toks.size() < 40 && g() % 2 ? 2 : 0;
            if (!tok_build_wordpiece(H, blob.data(), off.data(), ids.data(), (int64_t)toks.size(), 2, 3, 1, (int)(g() % 2), 1 + (int)(g() % 100), buckets)) FAIL("wordpiece table refused");
            if (2 * H.entries > (int64_t)H.T.mask + 1 || H.T.max_probe > TOK_MAX_PROBE) FAIL("wordpiece table shape");
        }
        const int ctx = 2 + (int)(g() % (c % 50 == 0 ? 1023 : 40)), pad = (int)(g() % 3 == 0 ? H.T.last : 0);
        for (int rowi = 0; rowi < 6; ++rowi) {
            const std::string s = random_row(g, (int)(g() % 9));
            const int n = (int)s.size();
            uint8_t *t = (uint8_t *)malloc(n ? n : 1);                 // exactly the row: a read past either end is a report
            memcpy(t, s.data(), n);
            int64_t *ids = (int64_t *)malloc(sizeof(int64_t) * ctx);
            int32_t length = -1;
            const int st = tok_row_host(H.T, t, n, ctx, pad, ids, &length);
            int want = 0;
            if (n > LEMON_TOKENIZE_MAX_BYTES) want = LEMON_TOK_TOO_LONG;
            else {
                bool non = false, amp = false, spec = false;
                for (int i = 0; i < n; ++i) {
                    const uint8_t b = t[i];
                    non = non || !(b == 9 || b == 10 || b == 13 || (b >= 32 && b <= 126));
                    amp = amp || b == '&';
                    spec = spec || (b == '<' && i + 1 < n && t[i + 1] == '|');
                }
                if (kind == 1) {
                    std::string w;
                    for (int i = 0; i <= n; ++i) {
                        if (i == n || s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r') {
                            spec = spec || w == "[PAD]" || w == "[UNK]" || w == "[CLS]" || w == "[SEP]" || w == "[MASK]";
                            w.clear();
                        } else w.push_back(s[i]);
                    }
                }
                want = non ? LEMON_TOK_NON_ASCII : amp ? LEMON_TOK_AMPERSAND : spec ? LEMON_TOK_SPECIAL : 0;
            }
            if (want ? st != want : (st != 0 && st != LEMON_TOK_WORD)) FAIL("status %d, expected %d (row of %d bytes)", st, want, n);
            if (st) {
                if (length != 0) FAIL("declined row with length %d", length);
                for (int p = 0; p < ctx; ++p) if (ids[p] != pad) FAIL("declined row is not padding");
            } else {
                if (length < 2 || length > ctx || ids[0] != H.T.first || ids[length - 1] != H.T.last) FAIL("framing, length %d of %d", length, ctx);
                for (int p = length; p < ctx; ++p) if (ids[p] != pad) FAIL("padding");
                std::string spelled, plain;
                for (int p = 1; p < length - 1; ++p) {
                    if (ids[p] < 0 || ids[p] >= vocab) FAIL("id %lld outside the vocabulary of %d", (long long)ids[p], vocab);
                    if (kind == 0) spelled += str_of[ids[p]];
                }
                for (int i = 0; i < n; ++i) if (tok_class(t[i]) != 0) plain.push_back((char)tok_lower(t[i]));
                if (kind == 0 && length < ctx && spelled != plain) FAIL("ids spell '%s', row is '%s'", spelled.c_str(), plain.c_str());
                if (kind == 0 && length == ctx && plain.compare(0, spelled.size(), spelled) != 0) FAIL("cut row does not spell a prefix");
            }
            free(t);
            free(ids);
        }
    }
    printf("tokenize_fuzz: ok (%d cases)\n", cases);
    return 0;
}
