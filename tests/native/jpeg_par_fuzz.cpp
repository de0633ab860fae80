// jpeg_par_fuzz.cpp -- mutation fuzz of the scan packer and of the parallel Huffman decode's shared host/device functions
// (lemon_amd/csrc/jpeg_par.hpp) with the lanes looped on the CPU, built with g++ under AddressSanitizer + UBSan by
// tests/test_jpeg_entropy_par.py.  Seed files are mutated mostly inside the scan (bit flips, deleted bytes, truncations, inserted
// markers) and sometimes in the header; every mutant is packed into a heap block of exactly the stated capacity, the packet is
// copied to a block of exactly its size and decoded into a record block of exactly its size, at the smallest lane size and at
// the default.  Checked besides the sanitizers: whatever the host pass declines is declined, an accepted file gives the host
// pass's record, and only LEMON_JPEG_SYNC may decline what the host pass accepts.  A share of the PACKETS is mutated too (the
// device trusts nothing in a packet): those only have to come back without a report.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/native/jpeg_par_fuzz.cpp -o jpeg_par_fuzz
//   ./jpeg_par_fuzz CASES SEED file.jpg [file.jpg ...]
#include "../../lemon_amd/csrc/jpeg_par.hpp"

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

static size_t scan_start(const Bytes &d) {
    size_t p = 2;
    while (p + 4 <= d.size() && d[p] == 0xFF) {
        const size_t len = ((size_t)d[p + 2] << 8) | d[p + 3];
        if (d[p + 1] == 0xDA) return p + 2 + len < d.size() ? p + 2 + len : d.size();
        p += 2 + len;
    }
    return d.size() / 2;
}

static long accepted = 0, declined = 0, sync_only = 0, packets_mutated = 0;
static std::mt19937_64 rng;
static size_t pick(size_t n) { return (size_t)(rng() % (n ? n : 1)); }

static int run_one(const Bytes &m, bool mutate_packet) {
    const int64_t n = (int64_t)m.size();
    uint8_t *in = (uint8_t *)malloc(m.size() ? m.size() : 1);
    memcpy(in, m.data(), m.size());
    LemonJpegInfo full, head;
    int bad = 0;
    // the host pass
    uint8_t *ref = nullptr;
    int rc_host = lemon_jpeg_info_impl(in, n, &full);
    const int rc_info = rc_host;
    int64_t rec_bytes = full.record_bytes;
    if (rc_host == LEMON_JPEG_OK && rec_bytes <= ((int64_t)64 << 20)) {
        ref = (uint8_t *)malloc((size_t)rec_bytes);
        rc_host = lemon_jpeg_entropy_impl(in, n, ref, rec_bytes, &full);
    } else if (rc_host == LEMON_JPEG_OK) {
        rc_host = -1;                                // (too large to decode here: only the packer runs)
    }
    const int64_t cap = n + n / 8192 + LEMON_JPEG_PACKET_BOUND + 16;
    uint8_t *pk = (uint8_t *)aligned_alloc(16, (size_t)((cap + 15) & ~(int64_t)15));
    int64_t pk_bytes = -1;
    const int rc_pack = lemon_jpeg_pack_impl(in, n, pk, cap, &head, &pk_bytes);
    if (rc_pack == LEMON_JPEG_BUFFER) {
        fprintf(stderr, "FAIL: the stated capacity did not hold the packet\n");
        bad = 1;
    }
    if (rc_pack == LEMON_JPEG_OK && (pk_bytes <= 0 || pk_bytes > cap || (pk_bytes & 15))) {
        fprintf(stderr, "FAIL: packet size %lld of capacity %lld\n", (long long)pk_bytes, (long long)cap);
        bad = 1;
    }
    if (rc_host == LEMON_JPEG_OK && rc_pack != LEMON_JPEG_OK) {
        fprintf(stderr, "FAIL: the packer declined (%d) what the host pass accepts\n", rc_pack);
        bad = 1;
    }
    if (rc_info != LEMON_JPEG_OK && rc_pack != rc_info) {
        fprintf(stderr, "FAIL: header verdicts differ: host %d, packer %d\n", rc_info, rc_pack);
        bad = 1;
    }
    if (!bad && rc_pack == LEMON_JPEG_OK && rc_host != -1) {
        uint8_t *exact = (uint8_t *)aligned_alloc(16, (size_t)pk_bytes);
        memcpy(exact, pk, (size_t)pk_bytes);
        if (mutate_packet) {
            ++packets_mutated;
            const int edits = 1 + (int)pick(3);
            for (int e = 0; e < edits; ++e) {
                const size_t at = pick(3) == 0 ? pick(128) : pick((size_t)pk_bytes);
                if (pick(2)) exact[at] ^= (uint8_t)(1u << pick(8)); else exact[at] = (uint8_t)rng();
            }
        }
        uint8_t *rec = (uint8_t *)malloc((size_t)head.record_bytes);
        const int32_t sizes[2] = {LEMON_JPEG_SUBSEQ_MIN, 0};
        for (int k = 0; k < 2 && !bad; ++k) {
            int32_t st = -1;
            if (lemon_jpeg_entropy_par_host_impl(exact, pk_bytes, sizes[k], rec, head.record_bytes, &st) != 0 || st < 0) {
                fprintf(stderr, "FAIL: the parallel decode refused its arguments\n");
                bad = 1;
            } else if (mutate_packet) {
                continue;
            } else if (rc_host != LEMON_JPEG_OK && st == LEMON_JPEG_OK) {
                fprintf(stderr, "FAIL: subseq %d accepted what the host pass declines (%d)\n", sizes[k], rc_host);
                bad = 1;
            } else if (rc_host == LEMON_JPEG_OK && st != LEMON_JPEG_OK && st != LEMON_JPEG_SYNC) {
                fprintf(stderr, "FAIL: subseq %d declined (%d) what the host pass accepts\n", sizes[k], st);
                bad = 1;
            } else if (rc_host == LEMON_JPEG_OK && st == LEMON_JPEG_OK && memcmp(rec, ref, (size_t)rec_bytes) != 0) {
                fprintf(stderr, "FAIL: subseq %d: the record differs from the host pass's\n", sizes[k]);
                bad = 1;
            } else if (rc_host == LEMON_JPEG_OK && st == LEMON_JPEG_SYNC) {
                ++sync_only;
            }
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
        fprintf(stderr, "usage: jpeg_par_fuzz CASES SEED file.jpg [...]\n");
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
    if (accepted != (long)seeds.size() || sync_only) {
        fprintf(stderr, "FAIL: %ld of %zu unmutated seeds accepted, %ld not settled\n", accepted, seeds.size(), sync_only);
        return 1;
    }
    for (long c = 0; c < cases; ++c) {
        Bytes m = seeds[pick(seeds.size())];
        const int rounds = 1 + (int)pick(3);
        for (int r = 0; r < rounds && m.size() > 4; ++r) {
            const size_t s0 = scan_start(m);
            const size_t in_scan = s0 + pick(m.size() - s0);
            switch (pick(8)) {
            case 0: case 1:                          // flip one bit of the scan
                m[in_scan < m.size() ? in_scan : m.size() - 1] ^= (uint8_t)(1u << pick(8));
                break;
            case 2:                                  // delete a byte of the scan
                if (in_scan < m.size()) m.erase(m.begin() + in_scan);
                break;
            case 3:                                  // truncate inside the scan
                m.resize(in_scan);
                break;
            case 4: {                                // insert a marker: restart, EOI, fill bytes or any other
                static const uint8_t kinds[6] = {0xD0, 0xD1, 0xD9, 0xFF, 0x00, 0xC4};
                const uint8_t mk[2] = {0xFF, pick(2) ? kinds[pick(6)] : (uint8_t)(0xD0 + pick(8))};
                m.insert(m.begin() + (in_scan < m.size() ? in_scan : m.size()), mk, mk + 2);
                break;
            }
            case 5:                                  // overwrite a byte of the scan
                if (in_scan < m.size()) m[in_scan] = (uint8_t)(pick(4) ? rng() : 0xFF);
                break;
            case 6:                                  // overwrite a byte of the header
                m[pick(s0 ? s0 : 1)] = (uint8_t)rng();
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
    printf("jpeg_par_fuzz: ok (%ld cases, %ld accepted, %ld declined, %ld left to the fallback, %ld packets mutated)\n", cases, accepted,
           declined, sync_only, packets_mutated);
    return 0;
}
