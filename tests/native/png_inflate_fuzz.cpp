// png_inflate_fuzz.cpp -- mutation fuzz of the PNG path's inflate (lemon_amd/csrc/png_inflate_core.hpp: the device's schedule
// with the lanes looped) on the CPU, built with g++ under AddressSanitizer + UBSan by tests/test_png_inflate_fuzz.py.
//   seeds     files of an 8-byte little-endian `want` followed by a valid zlib stream that yields exactly that many bytes
//   mutants   bit flips, truncations, splices from another seed, edits of 16-bit fields (a stored block's LEN / NLEN, a dynamic
//             header's counts), trailing bytes, and `want` moved by a little
//   checks    every run returns (termination) with status 0 or LEMON_PNG_STREAM; the stream sits in a heap block of exactly its
//             size and the rows in a heap block of exactly `want` bytes, so one byte read or written outside either is a
//             sanitizer report; two runs over differently poisoned rows give the same status and, when accepted, the same
//             bytes (determinism); an unmutated seed is accepted.  With -DPZ_FUZZ_ZLIB (and -lz) an accepted stream must be
//             accepted by zlib's inflate() under the same rule -- exactly `want` bytes, Z_STREAM_END, no input left -- with the
//             same bytes; streams zlib accepts and the decoder declines are counted, not failed.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/png_inflate_fuzz.cpp -o fuzz [-DPZ_FUZZ_ZLIB -lz]
//   ./fuzz CASES SEED seed.bin [seed.bin ...]
#include "../../lemon_amd/csrc/png_inflate_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#ifdef PZ_FUZZ_ZLIB
#include <zlib.h>
#endif

typedef std::vector<uint8_t> Bytes;

struct Seed {
    int64_t want;
    Bytes z;
};

static bool read_seed(const char *path, Seed &s) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    Bytes all;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) all.insert(all.end(), buf, buf + n);
    fclose(f);
    if (all.size() < 8) return false;
    s.want = 0;
    for (int k = 0; k < 8; ++k) s.want |= (int64_t)all[k] << (8 * k);
    s.z.assign(all.begin() + 8, all.end());
    return s.want >= 0 && s.want < (1 << 24);
}

static long accepted = 0, declined = 0, stricter = 0;

// -> status, or -1 after a failed check
static int run(const Bytes &z, int64_t want) {
    uint8_t *in = (uint8_t *)malloc(z.size() ? z.size() : 1);
    if (!z.empty()) memcpy(in, z.data(), z.size());
    uint8_t *rows[2];
    int32_t st[2] = {-1, -1};
    int bad = 0;
    for (int k = 0; k < 2; ++k) {
        rows[k] = (uint8_t *)malloc(want ? (size_t)want : 1);
        memset(rows[k], k ? 0x5A : 0xA5, want ? (size_t)want : 1);
        if (lemon_png_inflate_host_impl(in, (int64_t)z.size(), rows[k], want, &st[k]) != 0) { fprintf(stderr, "FAIL: arguments refused\n"); bad = 1; }
    }
    if (!z.empty() && memcmp(in, z.data(), z.size()) != 0) { fprintf(stderr, "FAIL: the input was written\n"); bad = 1; }
    if (st[0] != st[1] || (st[0] != LEMON_PNG_OK && st[0] != LEMON_PNG_STREAM)) { fprintf(stderr, "FAIL: status %d then %d\n", st[0], st[1]); bad = 1; }
    if (!bad && st[0] == LEMON_PNG_OK && want && memcmp(rows[0], rows[1], (size_t)want) != 0) { fprintf(stderr, "FAIL: two runs, two results\n"); bad = 1; }
#ifdef PZ_FUZZ_ZLIB
    if (!bad) {
        Bytes ref((size_t)want + 1);
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        bool ok = inflateInit(&zs) == Z_OK;
        if (ok) {
            zs.next_in = in; zs.avail_in = (uInt)z.size();
            zs.next_out = ref.data(); zs.avail_out = (uInt)ref.size();
            const int rc = inflate(&zs, Z_FINISH);
            ok = rc == Z_STREAM_END && (int64_t)zs.total_out == want && zs.avail_in == 0;
            inflateEnd(&zs);
        }
        if (st[0] == LEMON_PNG_OK && !ok) { fprintf(stderr, "FAIL: accepted a stream zlib rejects\n"); bad = 1; }
        if (st[0] == LEMON_PNG_OK && ok && want && memcmp(rows[0], ref.data(), (size_t)want) != 0) { fprintf(stderr, "FAIL: bytes differ from zlib's\n"); bad = 1; }
        if (st[0] != LEMON_PNG_OK && ok) ++stricter;
    }
#endif
    free(rows[0]);
    free(rows[1]);
    free(in);
    if (bad) return -1;
    ++(st[0] == LEMON_PNG_OK ? accepted : declined);
    return st[0];
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s CASES SEED seed.bin [seed.bin ...]\n", argv[0]); return 2; }
    const long cases = atol(argv[1]);
    std::mt19937_64 rng((uint64_t)atoll(argv[2]));
    std::vector<Seed> seeds;
    for (int i = 3; i < argc; ++i) {
        Seed s;
        if (!read_seed(argv[i], s)) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        if (run(s.z, s.want) != LEMON_PNG_OK) { fprintf(stderr, "FAIL: seed %s is not accepted\n", argv[i]); return 1; }
        seeds.push_back(s);
    }
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    for (long c = 0; c < cases; ++c) {
        const Seed &s = seeds[below(seeds.size())];
        Bytes m = s.z;
        int64_t want = s.want;
        const int rounds = 1 + (int)below(3);
        for (int r = 0; r < rounds; ++r) {
            switch (below(8)) {
            case 0: case 1:                                          // bit flips
                for (int k = 1 + (int)below(4); k > 0 && !m.empty(); --k) m[below(m.size())] ^= (uint8_t)(1u << below(8));
                break;
            case 2:                                                  // truncation
                m.resize(below(m.size() + 1));
                break;
            case 3: {                                                // a span of another seed, over or into the stream
                const Bytes &o = seeds[below(seeds.size())].z;
                if (o.empty()) break;
                const size_t from = below(o.size()), len = 1 + below(o.size() - from), at = below(m.size() + 1);
                if (below(2)) m.insert(m.begin() + (long)at, o.begin() + (long)from, o.begin() + (long)(from + len));
                else for (size_t k = 0; k < len && at + k < m.size(); ++k) m[at + k] = o[from + k];
                break;
            }
            case 4:                                                  // a 16-bit field: extreme values, or off by one
                if (m.size() >= 2) {
                    const size_t at = below(m.size() - 1);
                    const uint64_t how = below(4);
                    if (how == 0) { m[at] = 0; m[at + 1] = 0; }
                    else if (how == 1) { m[at] = 0xFF; m[at + 1] = 0xFF; }
                    else if (how == 2) { m[at] = (uint8_t)(m[at] + 1); }
                    else { m[at] = (uint8_t)(m[at] - 1); m[at + 1] = (uint8_t)~m[at + 1]; }
                }
                break;
            case 5:                                                  // bytes behind the trailer
                for (int k = 1 + (int)below(5); k > 0; --k) m.push_back((uint8_t)below(256));
                break;
            case 6:                                                  // another size
                want += (int64_t)below(5) - 2;
                if (want < 0) want = 0;
                break;
            default:                                                 // the header's two bytes
                if (m.size() >= 2) m[below(2)] = (uint8_t)below(256);
                break;
            }
        }
        if (run(m, want) < 0) { fprintf(stderr, "case %ld\n", c); return 1; }
    }
    printf("png_inflate_fuzz: ok, %ld accepted, %ld declined, %ld declined that zlib accepts\n", accepted, declined, stricter);
    return 0;
}
