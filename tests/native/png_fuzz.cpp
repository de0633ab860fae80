// png_fuzz.cpp -- mutation fuzz of the PNG chunk parser and of the device schedule looped on the host
// (lemon_amd/csrc/png_core.hpp) on the CPU, built with g++ under AddressSanitizer + UBSan by tests/test_png_fuzz.py.
//   files    seed files are mutated (byte flips, truncations, length-field edits, duplicated chunks, spliced tails; a mutant's
//            CRCs are repaired half of the time so that the walk gets past them); every mutant goes through lemon_png_info
//            and lemon_png_idat.  The parser must return (any status) without a sanitizer report; the input is copied to an
//            exact-size heap block and the IDAT payload is written into a heap block of exactly its stated size, so that one
//            byte read or written outside either is a report.
//   records  random records of random geometry (filter bytes mostly 0 .. 4, sometimes above; palette indices sometimes beyond
//            the PLTE count) in exact-size heap blocks go through lemon_png_decode_host; the pixels must equal a row-by-row
//            reference written here, the status the expected verdict, and a record one byte short must be refused.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/png_fuzz.cpp -o png_fuzz
//   ./png_fuzz CASES SEED file.png [file.png ...]
#include "../../lemon_amd/csrc/png_core.hpp"

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

// offsets of the chunks of a well-formed prefix
static std::vector<size_t> chunks(const Bytes &d) {
    std::vector<size_t> at;
    size_t p = 8;
    while (p + 12 <= d.size()) {
        const size_t len = lemon_png::be32(d.data() + p);
        if (len > d.size() - p - 12) break;
        at.push_back(p);
        p += 12 + len;
    }
    return at;
}

static void repair_crcs(Bytes &d) {
    for (size_t p : chunks(d)) {
        const size_t len = lemon_png::be32(d.data() + p);
        const uint32_t c = lemon_png::crc32(d.data() + p + 4, (int64_t)(4 + len));
        uint8_t *o = d.data() + p + 8 + len;
        o[0] = (uint8_t)(c >> 24); o[1] = (uint8_t)(c >> 16); o[2] = (uint8_t)(c >> 8); o[3] = (uint8_t)c;
    }
}

static long accepted = 0, declined = 0, records = 0, verdicts = 0;

static int run_file(const Bytes &m) {
    uint8_t *in = (uint8_t *)malloc(m.size() ? m.size() : 1);
    memcpy(in, m.data(), m.size());
    LemonPngInfo head;
    const int rc = lemon_png_info_impl(in, (int64_t)m.size(), &head);
    int bad = 0;
    if (rc == LEMON_PNG_OK) {
        ++accepted;
        const int ch = png_channels(head.colour_type);
        if (!ch || ch != head.channels || head.stride != (int64_t)head.width * ch ||
            head.record_bytes != 1024 + (int64_t)head.height * (head.stride + 1) || head.idat_spans < 1 || head.idat_bytes < 0 ||
            head.idat_offset < 0 || head.idat_offset > (int64_t)m.size() || (head.colour_type == 3) != (head.plte_count > 0) ||
            head.plte_count > 256 || (head.plte_count && (head.plte_offset < 0 || head.plte_offset + 3 * head.plte_count > (int64_t)m.size()))) {
            fprintf(stderr, "FAIL: accepted file with inconsistent info\n");
            bad = 1;
        }
        uint8_t *out = (uint8_t *)malloc(head.idat_bytes ? (size_t)head.idat_bytes : 1);
        if (lemon_png_idat_impl(in, (int64_t)m.size(), out, head.idat_bytes) != head.idat_bytes) {
            fprintf(stderr, "FAIL: the IDAT copy disagrees with the header pass\n");
            bad = 1;
        }
        if (head.idat_bytes > 0 && lemon_png_idat_impl(in, (int64_t)m.size(), out, head.idat_bytes - 1) != -(int64_t)LEMON_PNG_BUFFER) {
            fprintf(stderr, "FAIL: an IDAT buffer one byte short was not refused\n");
            bad = 1;
        }
        free(out);
    } else {
        ++declined;
        uint8_t small[16];
        if (lemon_png_idat_impl(in, (int64_t)m.size(), small, sizeof(small)) >= 0) {
            fprintf(stderr, "FAIL: the IDAT copy accepted what the header pass declined\n");
            bad = 1;
        }
    }
    free(in);
    return bad;
}

static int paeth_ref(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

template <class Rng>
static int run_record(Rng &rng) {
    static const int cts[5] = {0, 2, 3, 4, 6};
    const int ct = cts[rng() % 5], bpp = png_channels(ct);
    const int h = 1 + (int)(rng() % (rng() % 4 ? 70 : 200)), w = 1 + (int)(rng() % (rng() % 4 ? 70 : 200));
    const int plte = ct == 3 ? 1 + (int)(rng() % 256) : 0;
    const bool spoil_filter = rng() % 8 == 0, spoil_index = ct == 3 && plte < 256 && rng() % 4 == 0;
    const int64_t stride = (int64_t)w * bpp, n = 1024 + h * (stride + 1);
    uint8_t *rec = (uint8_t *)malloc((size_t)n), *rgb = (uint8_t *)malloc((size_t)h * w * 3);
    uint32_t *work = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)w);
    for (int64_t i = 0; i < n; ++i) rec[i] = (uint8_t)rng();
    for (int i = plte; i < 256; ++i) memset(rec + 4 * i, 0, 4);
    for (int r = 0; r < h; ++r) rec[1024 + r * (stride + 1)] = (uint8_t)(rng() % 5);
    if (spoil_filter) rec[1024 + (rng() % h) * (stride + 1)] = (uint8_t)(5 + rng() % 251);
    // the reference: row by row, byte by byte
    std::vector<uint8_t> img((size_t)h * stride);
    bool filter_bad = false, index_bad = false;
    for (int r = 0; r < h && !filter_bad; ++r) {
        const uint8_t *src = rec + 1024 + r * (stride + 1);
        if (src[0] > 4) { filter_bad = true; break; }
        for (int64_t x = 0; x < stride; ++x) {
            const int a = x >= bpp ? img[r * stride + x - bpp] : 0, b = r ? img[(r - 1) * stride + x] : 0;
            const int c = (r && x >= bpp) ? img[(r - 1) * stride + x - bpp] : 0;
            const int pred = src[0] == 0 ? 0 : src[0] == 1 ? a : src[0] == 2 ? b : src[0] == 3 ? (a + b) / 2 : paeth_ref(a, b, c);
            img[r * stride + x] = (uint8_t)(src[1 + x] + pred);
        }
    }
    if (ct == 3 && !filter_bad) {
        if (!spoil_index)                        // every index valid: the rows become filter None over indices below the PLTE count
            for (int r = 0; r < h; ++r)
                for (int64_t x = 0; x < stride; ++x) {
                    rec[1024 + r * (stride + 1)] = 0;
                    rec[1024 + r * (stride + 1) + 1 + x] = img[r * stride + x] = (uint8_t)(img[r * stride + x] % plte);
                }
        for (size_t i = 0; i < img.size(); ++i) index_bad |= img[i] >= plte;
    }
    int32_t status = -1;
    int bad = 0;
    if (lemon_png_decode_host_impl(rec, n - 1, h, w, ct, plte, rgb, work, &status) != 1 || status != -1) {
        fprintf(stderr, "FAIL: a record one byte short was not refused\n");
        bad = 1;
    }
    if (lemon_png_decode_host_impl(rec, n, h, w, ct, plte, rgb, work, &status) != 0) {
        fprintf(stderr, "FAIL: a valid record was refused\n");
        bad = 1;
    }
    const int want = filter_bad ? LEMON_PNG_FILTER : index_bad ? LEMON_PNG_INDEX : LEMON_PNG_OK;
    if (status != want) {
        fprintf(stderr, "FAIL: status %d, expected %d (h %d w %d ct %d)\n", status, want, h, w, ct);
        bad = 1;
    }
    if (!filter_bad)
        for (int r = 0; r < h && !bad; ++r)
            for (int x = 0; x < w && !bad; ++x) {
                const uint8_t *p = &img[r * stride + (int64_t)x * bpp], *o = rgb + ((int64_t)r * w + x) * 3;
                uint8_t e[3];
                if (ct == 0 || ct == 4) e[0] = e[1] = e[2] = p[0];
                else if (ct == 3) { const bool in = p[0] < plte; e[0] = in ? rec[4 * p[0]] : 0; e[1] = in ? rec[4 * p[0] + 1] : 0; e[2] = in ? rec[4 * p[0] + 2] : 0; }
                else { e[0] = p[0]; e[1] = p[1]; e[2] = p[2]; }
                if (status == LEMON_PNG_OK && memcmp(e, o, 3) != 0) {
                    fprintf(stderr, "FAIL: pixel (%d, %d) of h %d w %d ct %d differs from the row-by-row reference\n", r, x, h, w, ct);
                    bad = 1;
                }
            }
    ++records;
    verdicts += want != LEMON_PNG_OK;
    free(rec); free(rgb); free(work);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: png_fuzz CASES SEED file.png [...]\n");
        return 2;
    }
    const long cases = atol(argv[1]);
    std::mt19937_64 rng((uint64_t)atoll(argv[2]));
    std::vector<Bytes> seeds;
    for (int i = 3; i < argc; ++i) {
        Bytes b;
        if (!read_file(argv[i], b) || b.size() < 8) {
            fprintf(stderr, "cannot read seed %s\n", argv[i]);
            return 2;
        }
        seeds.push_back(b);
    }
    auto pick = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    for (const Bytes &s : seeds)
        if (run_file(s)) return 1;
    if (accepted != (long)seeds.size()) {
        fprintf(stderr, "FAIL: %ld of %zu unmutated seeds accepted\n", accepted, seeds.size());
        return 1;
    }
    for (long c = 0; c < cases; ++c) {
        Bytes m = seeds[pick(seeds.size())];
        const int rounds = 1 + (int)pick(3);
        for (int r = 0; r < rounds && !m.empty(); ++r) {
            const std::vector<size_t> cs = chunks(m);
            switch (pick(7)) {
            case 0:                                  // flip one bit anywhere
                m[pick(m.size())] ^= (uint8_t)(1u << pick(8));
                break;
            case 1: {                                // overwrite a byte of IHDR or of a chunk's header
                const size_t at = cs.empty() || pick(2) ? 8 + pick(std::min<size_t>(m.size() - 8 ? m.size() - 8 : 1, 25)) : cs[pick(cs.size())] + pick(8);
                if (at < m.size()) m[at] = (uint8_t)(pick(3) ? rng() : pick(17));
                break;
            }
            case 2:                                  // truncate
                m.resize(pick(m.size() + 1));
                break;
            case 3:                                  // edit a length field
                if (!cs.empty()) {
                    const size_t at = cs[pick(cs.size())];
                    const uint32_t v = pick(4) == 0 ? (uint32_t)rng() : lemon_png::be32(m.data() + at) + (uint32_t)pick(9) - 4;
                    m[at] = (uint8_t)(v >> 24); m[at + 1] = (uint8_t)(v >> 16); m[at + 2] = (uint8_t)(v >> 8); m[at + 3] = (uint8_t)v;
                }
                break;
            case 4:                                  // duplicate or move a chunk
                if (!cs.empty()) {
                    const size_t at = cs[pick(cs.size())];
                    const size_t len = 12 + (size_t)lemon_png::be32(m.data() + at);
                    const Bytes seg(m.begin() + at, m.begin() + at + len);
                    m.insert(m.begin() + cs[pick(cs.size())], seg.begin(), seg.end());
                }
                break;
            case 5:                                  // rename a chunk
                if (!cs.empty()) {
                    static const char *names[] = {"IDAT", "PLTE", "IEND", "IHDR", "acTL", "tRNS", "zzZz", "ZZZZ"};
                    memcpy(m.data() + cs[pick(cs.size())] + 4, names[pick(8)], 4);
                }
                break;
            default: {                               // splice: the tail of another seed
                const Bytes &o = seeds[pick(seeds.size())];
                m.resize(pick(m.size() + 1));
                const size_t from = pick(o.size());
                m.insert(m.end(), o.begin() + from, o.end());
                break;
            }
            }
        }
        if (m.size() >= 8 && pick(2)) repair_crcs(m);
        if (run_file(m)) {
            fprintf(stderr, "file case %ld\n", c);
            return 1;
        }
        if (c % 8 == 0 && run_record(rng)) {
            fprintf(stderr, "record case %ld\n", c);
            return 1;
        }
    }
    printf("png_fuzz: ok (%ld cases, %ld accepted, %ld declined, %ld records, %ld verdicts)\n", cases, accepted, declined, records, verdicts);
    return 0;
}
