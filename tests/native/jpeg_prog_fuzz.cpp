// jpeg_prog_fuzz.cpp -- mutation fuzz of the progressive JPEG host code (lemon_amd/csrc/jpeg_prog.hpp, jpeg_prog_par.hpp): the
// sequential host pass, the packer and the device algorithm with its waves looped on the CPU, built with g++ under
// AddressSanitizer + UBSan by tests/test_jpeg_progressive.py.  Seed files are mutated in their scans (bit flips, deleted bytes,
// truncations, inserted markers), in their headers and tables, and in the SOS headers; every mutant is packed into a heap block
// of exactly the stated capacity, the packet copied to a block of exactly its size and decoded into a record block of exactly
// its size.  Checked besides the sanitizers: the stated capacity holds every packet, the packer declines exactly what the host
// pass's header and marker checks decline, the looped device algorithm returns the host pass's status, and accepted records are
// equal.  A share of the PACKETS is mutated too (the device trusts nothing in a packet): those only have to come back without
// a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/jpeg_prog_fuzz.cpp -o jpeg_prog_fuzz
//   ./jpeg_prog_fuzz CASES SEED file.jpg [file.jpg ...]
#include "../../lemon_amd/csrc/jpeg_prog.hpp"

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

// offsets of the SOS markers (segment walk; inside entropy-coded bytes only FF 00 and RSTn are passed over)
static std::vector<size_t> sos_offsets(const Bytes &d) {
    std::vector<size_t> out;
    size_t p = 2;
    while (p + 4 <= d.size() && d[p] == 0xFF) {
        const size_t len = ((size_t)d[p + 2] << 8) | d[p + 3];
        if (d[p + 1] == 0xD9) break;
        if (d[p + 1] == 0xDA) {
            out.push_back(p);
            p += 2 + len;
            while (p + 1 < d.size() && !(d[p] == 0xFF && d[p + 1] != 0 && !(d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7))) ++p;
        } else {
            p += 2 + len;
        }
    }
    return out;
}

static long accepted = 0, declined = 0, packets_mutated = 0;
static std::mt19937_64 rng;
static size_t pick(size_t n) { return (size_t)(rng() % (n ? n : 1)); }

static int run_one(const Bytes &m, bool mutate_packet) {
    const int64_t n = (int64_t)m.size();
    uint8_t *in = (uint8_t *)malloc(m.size() ? m.size() : 1);
    memcpy(in, m.data(), m.size());
    LemonJpegInfo full, head, first;
    int bad = 0;
    uint8_t *ref = nullptr;
    int rc_host = lemon_jpeg_prog_info_impl(in, n, &first);
    int64_t rec_bytes = first.record_bytes;
    if (rc_host == LEMON_JPEG_OK && rec_bytes <= ((int64_t)64 << 20)) {
        ref = (uint8_t *)malloc((size_t)rec_bytes);
        rc_host = lemon_jpeg_prog_entropy_impl(in, n, ref, rec_bytes, &full);
    } else if (rc_host == LEMON_JPEG_OK) {
        rc_host = -1;                                // (too large to decode here: only the packer runs)
    }
    const int64_t cap = lemon_jpeg_prog::packet_cap(n);
    uint8_t *pk = (uint8_t *)aligned_alloc(16, (size_t)((cap + 15) & ~(int64_t)15));
    int64_t pk_bytes = -1;
    const int rc_pack = lemon_jpeg_prog_pack_impl(in, n, pk, cap, &head, &pk_bytes);
    if (rc_pack == LEMON_JPEG_BUFFER && n < ((int64_t)1 << 31)) {
        fprintf(stderr, "FAIL: the stated capacity did not hold the packet\n");
        bad = 1;
    }
    if (rc_pack == LEMON_JPEG_OK && (pk_bytes <= 0 || pk_bytes > cap || (pk_bytes & 15))) {
        fprintf(stderr, "FAIL: packet size %lld of capacity %lld\n", (long long)pk_bytes, (long long)cap);
        bad = 1;
    }
    if (rc_host != -1 && rc_pack != LEMON_JPEG_OK && rc_pack != rc_host) {
        fprintf(stderr, "FAIL: header and marker verdicts differ: host %d, packer %d\n", rc_host, rc_pack);
        bad = 1;
    }
    if (rc_host != -1 && rc_pack == LEMON_JPEG_OK && rc_host != LEMON_JPEG_OK && rc_host != LEMON_JPEG_CODE && rc_host != LEMON_JPEG_STREAM &&
        rc_host != LEMON_JPEG_ENVELOPE) {
        fprintf(stderr, "FAIL: the packer accepted what the host pass's header checks decline (%d)\n", rc_host);
        bad = 1;
    }
    if (!bad && rc_pack == LEMON_JPEG_OK && rc_host != -1) {
        uint8_t *exact = (uint8_t *)aligned_alloc(16, (size_t)pk_bytes);
        memcpy(exact, pk, (size_t)pk_bytes);
        if (mutate_packet) {
            ++packets_mutated;
            const int edits = 1 + (int)pick(3);
            for (int e = 0; e < edits; ++e) {
                const size_t r = pick(4);
                const size_t at = r == 0 ? pick(128) : (r == 1 ? 512 + pick(64 * 12) % (size_t)(pk_bytes - 512) : pick((size_t)pk_bytes));
                if (pick(2)) exact[at] ^= (uint8_t)(1u << pick(8)); else exact[at] = (uint8_t)rng();
            }
        }
        uint8_t *rec = (uint8_t *)malloc((size_t)head.record_bytes);
        int32_t st = -1;
        if (lemon_jpeg_prog_entropy_par_host_impl(exact, pk_bytes, rec, head.record_bytes, &st) != 0 || st < 0) {
            fprintf(stderr, "FAIL: the looped device algorithm refused its arguments\n");
            bad = 1;
        } else if (!mutate_packet && st != rc_host) {
            fprintf(stderr, "FAIL: statuses differ: host pass %d, looped device algorithm %d\n", rc_host, st);
            bad = 1;
        } else if (!mutate_packet && st == LEMON_JPEG_OK && memcmp(rec, ref, (size_t)rec_bytes) != 0) {
            fprintf(stderr, "FAIL: the record differs from the host pass's\n");
            bad = 1;
        }
        free(rec);
        free(exact);
    }
    if (rc_host == LEMON_JPEG_OK) ++accepted; else ++declined;
    free(pk);
    free(ref);
    free(in);
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: jpeg_prog_fuzz CASES SEED file.jpg [...]\n");
        return 2;
    }
    const long cases = atol(argv[1]);
    rng.seed((uint64_t)atoll(argv[2]));
    std::vector<Bytes> seeds;
    for (int i = 3; i < argc; ++i) {
        Bytes b;
        if (!read_file(argv[i], b) || b.size() < 4) {
            fprintf(stderr, "cannot read seed %s\n", argv[i]);
            return 2;
        }
        seeds.push_back(b);
    }
    for (const Bytes &s : seeds)
        if (run_one(s, false)) return 1;
    if (accepted != (long)seeds.size()) {
        fprintf(stderr, "FAIL: %ld of %zu unmutated seeds accepted\n", accepted, seeds.size());
        return 1;
    }
    for (long c = 0; c < cases; ++c) {
        Bytes m = seeds[pick(seeds.size())];
        const int rounds = 1 + (int)pick(3);
        for (int r = 0; r < rounds && m.size() > 4; ++r) {
            const std::vector<size_t> sos = sos_offsets(m);
            const size_t s0 = sos.empty() ? m.size() / 2 : sos[0];
            const size_t in_scan = s0 + pick(m.size() - s0);
            switch (pick(10)) {
            case 0: case 1:                          // flip one bit at or after the first scan
                m[in_scan < m.size() ? in_scan : m.size() - 1] ^= (uint8_t)(1u << pick(8));
                break;
            case 2:                                  // delete a byte there
                if (in_scan < m.size()) m.erase(m.begin() + in_scan);
                break;
            case 3:                                  // truncate there
                m.resize(in_scan);
                break;
            case 4: {                                // insert a marker: restart, EOI, fill bytes or any other
                static const uint8_t kinds[6] = {0xD0, 0xD1, 0xD9, 0xFF, 0x00, 0xC4};
                const uint8_t mk[2] = {0xFF, pick(2) ? kinds[pick(6)] : (uint8_t)(0xD0 + pick(8))};
                m.insert(m.begin() + (in_scan < m.size() ? in_scan : m.size()), mk, mk + 2);
                break;
            }
            case 5:                                  // overwrite a byte there
                if (in_scan < m.size()) m[in_scan] = (uint8_t)(pick(4) ? rng() : 0xFF);
                break;
            case 6:                                  // overwrite a byte of the header
                m[pick(s0 ? s0 : 1)] = (uint8_t)rng();
                break;
            case 7: case 8:                          // overwrite a byte of an SOS header (components, tables, Ss, Se, Ah/Al)
                if (!sos.empty()) {
                    const size_t at = sos[pick(sos.size())] + 4 + pick(10);
                    if (at < m.size()) m[at] = (uint8_t)(pick(2) ? rng() : pick(16));
                }
                break;
            default:                                 // flip a bit anywhere
                m[pick(m.size())] ^= (uint8_t)(1u << pick(8));
                break;
            }
        }
        if (run_one(m, pick(5) == 0)) {
            fprintf(stderr, "case %ld\n", c);
            return 1;
        }
    }
    printf("jpeg_prog_fuzz: ok (%ld cases, %ld accepted, %ld declined, %ld packets mutated)\n", cases, accepted, declined, packets_mutated);
    return 0;
}
