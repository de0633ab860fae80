// jpeg_fuzz.cpp -- mutation fuzz of the JPEG host pass (lemon_amd/csrc/jpeg_entropy.hpp) on the CPU, built with g++ under
// AddressSanitizer + UBSan by tests/test_jpeg_host.py.  Seed files are mutated (byte flips, truncations, length-field edits,
// duplicated segments, spliced tails); every mutant goes through the header pass and the full pass.  The parser must return
// (any status) without a sanitizer report; the input is copied to an exact-size heap block and an accepted file's record is
// written into a heap block of exactly its stated size, so that one byte read or written outside either is a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/jpeg_fuzz.cpp -o jpeg_fuzz
//   ./jpeg_fuzz CASES SEED file.jpg [file.jpg ...]
#include "../../lemon_amd/csrc/jpeg_entropy.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef std::vector<uint8_t> Bytes;

static bool read_file(const char *path, Bytes &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

// offsets of the marker segments that carry a length, up to SOS
static std::vector<size_t> segments(const Bytes &d) {
    std::vector<size_t> at;
    size_t p = 2;
    while (p + 4 <= d.size() && d[p] == 0xFF) {
        const int m = d[p + 1];
        const size_t len = ((size_t)d[p + 2] << 8) | d[p + 3];
        at.push_back(p);
        if (m == 0xDA || len < 2) break;
        p += 2 + len;
    }
    return at;
}

static long accepted = 0, declined = 0;

static int run_one(const Bytes &m) {
    // exact-size copies: the sanitizer sees any access outside the file or the record
    uint8_t *in = (uint8_t *)malloc(m.size() ? m.size() : 1);
    memcpy(in, m.data(), m.size());
    LemonJpegInfo head, full;
    const int rc0 = lemon_jpeg_info_impl(in, (int64_t)m.size(), &head);
    int bad = 0;
    if (rc0 == LEMON_JPEG_OK) {
        JpegGeom g;
        if (!jpeg_geometry(head.width, head.height, head.components, head.hs, head.vs, g) || g.blocks != head.blocks ||
            head.record_bytes != LEMON_JPEG_QUANT_BYTES + 128 * head.blocks) {
            fprintf(stderr, "FAIL: accepted header with inconsistent geometry\n");
            bad = 1;
        } else if (head.record_bytes > ((int64_t)64 << 20)) {
            uint8_t small[16];
            if (lemon_jpeg_entropy_impl(in, (int64_t)m.size(), small, sizeof(small), &full) != LEMON_JPEG_BUFFER) {
                fprintf(stderr, "FAIL: a record larger than the buffer was not refused\n");
                bad = 1;
            }
        } else {
            uint8_t *rec = (uint8_t *)malloc((size_t)head.record_bytes);
            const int rc = lemon_jpeg_entropy_impl(in, (int64_t)m.size(), rec, head.record_bytes, &full);
            if (rc == LEMON_JPEG_OK) {
                ++accepted;
                if (full.record_bytes != head.record_bytes || full.width != head.width || full.height != head.height) {
                    fprintf(stderr, "FAIL: the two passes disagree on an accepted file\n");
                    bad = 1;
                }
            } else {
                ++declined;
            }
            free(rec);
        }
    } else {
        ++declined;
        uint8_t small[16];
        if (lemon_jpeg_entropy_impl(in, (int64_t)m.size(), small, sizeof(small), &full) == LEMON_JPEG_OK) {
            fprintf(stderr, "FAIL: the full pass accepted what the header pass declined\n");
            bad = 1;
        }
    }
    free(in);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: jpeg_fuzz CASES SEED file.jpg [...]\n");
        return 2;
    }
    const long cases = atol(argv[1]);
    std::mt19937_64 rng((uint64_t)atoll(argv[2]));
    std::vector<Bytes> seeds;
    for (int i = 3; i < argc; ++i) {
        Bytes b;
        if (!read_file(argv[i], b) || b.size() < 4) {
            fprintf(stderr, "cannot read seed %s\n", argv[i]);
            return 2;
        }
        seeds.push_back(b);
    }
    auto pick = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    for (const Bytes &s : seeds)
        if (run_one(s)) return 1;
    if (accepted != (long)seeds.size()) {
        fprintf(stderr, "FAIL: %ld of %zu unmutated seeds accepted\n", accepted, seeds.size());
        return 1;
    }
    for (long c = 0; c < cases; ++c) {
        Bytes m = seeds[pick(seeds.size())];
        const int rounds = 1 + (int)pick(3);
        for (int r = 0; r < rounds && !m.empty(); ++r) {
            const std::vector<size_t> segs = segments(m);
            switch (pick(7)) {
            case 0:                                  // flip one byte anywhere
                m[pick(m.size())] ^= (uint8_t)(1u << pick(8));
                break;
            case 1: {                                // overwrite a byte in the header part
                const size_t hdr = segs.empty() ? m.size() : std::min(m.size(), segs.back() + 16);
                m[pick(hdr)] = (uint8_t)rng();
                break;
            }
            case 2:                                  // truncate
                m.resize(pick(m.size() + 1));
                break;
            case 3:                                  // edit a length field
                if (!segs.empty()) {
                    const size_t at = segs[pick(segs.size())];
                    if (at + 3 < m.size()) {
                        const uint16_t v = (uint16_t)(pick(4) == 0 ? rng() : (((m[at + 2] << 8) | m[at + 3]) + (int)pick(9) - 4));
                        m[at + 2] = (uint8_t)(v >> 8);
                        m[at + 3] = (uint8_t)v;
                    }
                }
                break;
            case 4:                                  // duplicate a segment
                if (!segs.empty()) {
                    const size_t at = segs[pick(segs.size())];
                    if (at + 4 <= m.size()) {
                        const size_t len = std::min(m.size() - at, (size_t)2 + (((size_t)m[at + 2] << 8) | m[at + 3]));
                        const Bytes seg(m.begin() + at, m.begin() + at + len);
                        m.insert(m.begin() + segs[pick(segs.size())], seg.begin(), seg.end());
                    }
                }
                break;
            case 5: {                                // put a marker byte pair somewhere
                const size_t at = pick(m.size());
                m[at] = 0xFF;
                if (at + 1 < m.size()) m[at + 1] = (uint8_t)(0xC0 + pick(0x40));
                break;
            }
            default: {                               // splice: the tail of another seed
                const Bytes &o = seeds[pick(seeds.size())];
                m.resize(pick(m.size() + 1));
                const size_t from = pick(o.size());
                m.insert(m.end(), o.begin() + from, o.end());
                break;
            }
            }
        }
        if (run_one(m)) {
            fprintf(stderr, "case %ld\n", c);
            return 1;
        }
    }
    printf("jpeg_fuzz: ok (%ld cases, %ld accepted, %ld declined)\n", cases, accepted, declined);
    return 0;
}
