// Drives lemon_amd/csrc/index_ws.hpp alone (no HIP, no Python) with a fake device that counts live allocations, logs every
// synchronise / free / alloc in order, poisons and tracks what it frees, and fails the allocation (or the synchronise) it is
// told to.  Seeded random sequences of reserve, group reserve and release over a pool of buffers, every growing step run with a
// failed synchronise, then once per position at which an allocation can fail, then once without a failure.  After every step:
//   * p == nullptr exactly when bytes == 0, for every buffer;
//   * a request that fits changes nothing: same pointers, same sizes, nothing logged (no synchronise);
//   * a growth synchronises exactly once, before its first free and its first alloc, and allocates exactly the request;
//   * a member of a group that fits is not touched, whatever happens to the others;
//   * after a failed group reserve every member that was being grown is empty;
//   * a failed synchronise changes nothing;
//   * the live allocations are exactly the non-empty buffers: nothing leaks, nothing is freed twice;
//   * the same request without a failure then succeeds and fills every member.
// named_half_copy() is the sequence that used to leave an index with a 16-bit copy and no statistics.
//   g++ -std=c++17 -O1 -g [-fsanitize=address,undefined -fno-sanitize-recover=all] index_ws_fuzz.cpp && ./a.out [steps] [seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../lemon_amd/csrc/index_ws.hpp"

static uint64_t g_state = 1;
static uint64_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 17;
}

struct FakeDev {
    std::map<void *, size_t> live;
    std::string log;            // 'S' synchronise, 'F' free, 'A' alloc (also a failed one)
    int fail_alloc = -1;        // the alloc of this step, counted from 0, that fails (-1: none)
    bool fail_sync = false;
    int allocs = 0, bad_frees = 0;
    bool sync() { log += 'S'; return !fail_sync; }
    bool alloc(void **p, size_t bytes) {
        log += 'A';
        if (allocs++ == fail_alloc) return false;
        *p = malloc(bytes);
        memset(*p, 0xa5, bytes);
        live[*p] = bytes;
        return true;
    }
    void free(void *p) {
        log += 'F';
        auto it = live.find(p);
        if (it == live.end()) { ++bad_frees; return; }      // never allocated here, or freed twice
        memset(p, 0xdd, it->second);
        ::free(p);
        live.erase(it);
    }
    void begin_step(int fail_at, bool sync_fails) { log.clear(); allocs = 0; fail_alloc = fail_at; fail_sync = sync_fails; }
};

static long g_step = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            printf("index_ws_fuzz: FAILED %s (line %d, step %ld)\n", #cond, __LINE__, g_step);   \
            return false;                                                                        \
        }                                                                                        \
    } while (0)

// what must hold between any two steps
static bool consistent(const FakeDev &dev, const LemonBuf *pool, int n_pool) {
    size_t holding = 0;
    for (int i = 0; i < n_pool; ++i) {
        CHECK((pool[i].p == nullptr) == (pool[i].bytes == 0));
        if (!pool[i].p) continue;
        ++holding;
        auto it = dev.live.find(pool[i].p);
        CHECK(it != dev.live.end() && it->second == pool[i].bytes);
        memset(pool[i].p, 0x5a, pool[i].bytes);              // all of it is the buffer's to write (the sanitizer checks)
    }
    CHECK(holding == dev.live.size() && dev.bad_frees == 0);
    return true;
}

// one reserve of members[0 .. count) of the pool at want[]: with `fail_at` / `sync_fails`, then checked against the rules
static bool reserve_step(FakeDev &dev, LemonBuf *pool, int n_pool, const int *members, const size_t *want, int count, int fail_at,
                         bool sync_fails, bool single) {
    ++g_step;
    std::vector<LemonBuf> before(pool, pool + n_pool);
    LemonBuf *bufs[lemon_ws::MAX_GROUP];
    int growing = 0;
    for (int i = 0; i < count; ++i) { bufs[i] = &pool[members[i]]; growing += want[i] > bufs[i]->bytes; }
    dev.begin_step(fail_at, sync_fails);
    const lemon_ws::Result r = single ? lemon_ws::reserve(dev, *bufs[0], want[0]) : lemon_ws::reserve_group(dev, bufs, want, count);
    CHECK(consistent(dev, pool, n_pool));
    std::vector<bool> member(n_pool, false);
    for (int i = 0; i < count; ++i) member[members[i]] = true;
    for (int i = 0; i < n_pool; ++i)
        if (!member[i]) CHECK(pool[i].p == before[i].p && pool[i].bytes == before[i].bytes);
    for (int i = 0; i < count; ++i)                          // a member that fits is never touched
        if (want[i] <= before[members[i]].bytes) CHECK(bufs[i]->p == before[members[i]].p && bufs[i]->bytes == before[members[i]].bytes);
    if (!growing) {
        CHECK(r == lemon_ws::OK && dev.log.empty());
        return true;
    }
    CHECK(dev.log[0] == 'S' && dev.log.find('S', 1) == std::string::npos);      // once, and first
    if (sync_fails) {
        CHECK(r == lemon_ws::SYNC_FAILED && dev.log == "S");
        for (int i = 0; i < count; ++i) CHECK(bufs[i]->p == before[members[i]].p && bufs[i]->bytes == before[members[i]].bytes);
        return true;
    }
    const bool failed = fail_at >= 0 && fail_at < growing;
    CHECK(r == (failed ? lemon_ws::NO_MEMORY : lemon_ws::OK));
    for (int i = 0; i < count; ++i) {
        if (want[i] <= before[members[i]].bytes) continue;
        if (failed) CHECK(bufs[i]->p == nullptr && bufs[i]->bytes == 0);
        else CHECK(bufs[i]->p != nullptr && bufs[i]->bytes == want[i]);         // exactly the request: no geometric growth
    }
    return true;
}

// the step with a failed synchronise, then at every failure position, then for real: the retry succeeds and fills every member
static bool reserve_everywhere(FakeDev &dev, LemonBuf *pool, int n_pool, const int *members, const size_t *want, int count, bool single) {
    int growing = 0;
    for (int i = 0; i < count; ++i) growing += want[i] > pool[members[i]].bytes;
    if (growing) CHECK(reserve_step(dev, pool, n_pool, members, want, count, -1, true, single));
    // (a failure empties the growing members, so later positions are tried from that state: still `growing` allocations)
    for (int f = 0; f < growing; ++f) CHECK(reserve_step(dev, pool, n_pool, members, want, count, f, false, single));
    CHECK(reserve_step(dev, pool, n_pool, members, want, count, -1, false, single));
    for (int i = 0; i < count; ++i) CHECK(pool[members[i]].p != nullptr || want[i] == 0);
    for (int i = 0; i < count; ++i) CHECK(pool[members[i]].bytes >= want[i]);
    return true;
}

static bool release_all(FakeDev &dev, LemonBuf *pool, int n_pool) {
    for (int i = 0; i < n_pool; ++i) lemon_ws::release(dev, pool[i]);
    CHECK(dev.live.empty() && consistent(dev, pool, n_pool));
    return true;
}

// xh, xh_stats, xn2max_dev of an index: the copy's allocation succeeds, the statistics' fails.  The handle must not keep a
// copy without statistics: every member empty, and the next search's reserve builds all three.
static bool named_half_copy() {
    FakeDev dev;
    LemonBuf pool[3] = {};
    const int members[3] = {0, 1, 2};
    const size_t want[3] = {4096 * 64 * 2 + 16, 4096 * 2 * 4, 16};
    for (int f = 0; f < 3; ++f) {
        CHECK(reserve_step(dev, pool, 3, members, want, 3, f, false, false));
        for (int i = 0; i < 3; ++i) CHECK(pool[i].p == nullptr && pool[i].bytes == 0);
        CHECK(dev.live.empty());
    }
    CHECK(reserve_step(dev, pool, 3, members, want, 3, -1, false, false));
    for (int i = 0; i < 3; ++i) CHECK(pool[i].p != nullptr && pool[i].bytes == want[i]);
    // an add beyond the capacity releases the copy and its statistics and keeps the maxima; the rebuild at the new capacity
    // fails on the statistics: the maxima, which fit, stay, the other two end empty, and the retry fills them
    lemon_ws::release(dev, pool[0]);
    lemon_ws::release(dev, pool[1]);
    const size_t more[3] = {2 * want[0], 2 * want[1], 16};
    void *const maxima = pool[2].p;
    CHECK(reserve_step(dev, pool, 3, members, more, 3, 1, false, false));
    CHECK(!pool[0].p && !pool[1].p && pool[2].p == maxima && dev.live.size() == 1);
    CHECK(reserve_step(dev, pool, 3, members, more, 3, -1, false, false));
    CHECK(pool[0].bytes == more[0] && pool[1].bytes == more[1] && pool[2].p == maxima);
    return release_all(dev, pool, 3);
}

int main(int argc, char **argv) {
    const long steps = argc > 1 ? atol(argv[1]) : 20000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    if (!named_half_copy()) return 1;
    const int N = 6;
    static_assert(N <= lemon_ws::MAX_GROUP, "a group of the whole pool");
    FakeDev dev;
    LemonBuf pool[N] = {};                                     // all-zero is empty, as calloc of the handle leaves it
    for (long t = 0; t < steps; ++t) {
        const int op = (int)(rnd() % 8);
        if (op == 0) {
            ++g_step;
            const int i = (int)(rnd() % N);
            dev.begin_step(-1, false);
            lemon_ws::release(dev, pool[i]);
            if (!(pool[i].p == nullptr && pool[i].bytes == 0 && dev.log.find('S') == std::string::npos && consistent(dev, pool, N))) {
                printf("index_ws_fuzz: FAILED release (step %ld)\n", g_step);
                return 1;
            }
            continue;
        }
        const bool single = op <= 3;
        const int count = single ? 1 : 2 + (int)(rnd() % (N - 1));        // groups of 2 .. N <= MAX_GROUP
        int members[N];
        size_t want[N];
        int order[N];
        for (int i = 0; i < N; ++i) order[i] = i;
        for (int i = 0; i < count; ++i) {                      // distinct members
            const int j = i + (int)(rnd() % (N - i));
            const int tmp = order[i]; order[i] = order[j]; order[j] = tmp;
            members[i] = order[i];
            const size_t have = pool[members[i]].bytes;
            switch (rnd() % 6) {                               // zero, what it has, one byte either side, anything
                case 0: want[i] = 0; break;
                case 1: want[i] = have; break;
                case 2: want[i] = have + 1; break;
                case 3: want[i] = have ? have - 1 : 0; break;
                default: want[i] = (size_t)(rnd() % 5000);
            }
        }
        if (!reserve_everywhere(dev, pool, N, members, want, count, single)) return 1;
    }
    if (!release_all(dev, pool, N)) return 1;
    printf("index_ws_fuzz: ok (%ld steps)\n", g_step);
    return 0;
}
