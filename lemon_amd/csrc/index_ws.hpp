// index_ws.hpp -- the device buffers an index handle keeps between calls, and the one rule by which they grow.
// Plain C++: no device runtime, no globals, no environment, so tests/native/index_ws_fuzz.cpp drives it with a fake allocator.
//
// A LemonBuf is empty (p == nullptr, bytes == 0: what calloc of the handle gives) or holds exactly `bytes` bytes.  Buffers
// only grow: a request that fits does nothing at all, a larger one synchronises ONCE (work queued earlier may still read the
// old memory), frees, and allocates exactly what was asked -- no geometric growth, the callers' sizes are exact.  A failed
// growth leaves the buffer empty, never half made, so the caller's next attempt allocates again.
//
// Dev is the device policy: bool sync(), bool alloc(void **, size_t), void free(void *) (common.hpp has the real one).
#pragma once
#include <stddef.h>

struct LemonBuf {
    void *p;
    size_t bytes;
};

namespace lemon_ws {

enum Result { OK = 0, SYNC_FAILED, NO_MEMORY };
constexpr int MAX_GROUP = 8;

// Free and empty.  The CALLER has synchronised whatever may still read the buffer.
template <typename Dev>
void release(Dev &dev, LemonBuf &buf) {
    if (buf.p) dev.free(buf.p);
    buf.p = nullptr;
    buf.bytes = 0;
}

// Grow every member of a group (count <= MAX_GROUP) that is smaller than its request; members that fit are not touched.
// All or nothing: if one allocation fails, every member that was being grown ends empty, so nothing ever runs on half a
// group (the 16-bit copy without its statistics).  A failed synchronisation changes nothing.
template <typename Dev>
Result reserve_group(Dev &dev, LemonBuf *const *bufs, const size_t *bytes, int count) {
    bool grows[MAX_GROUP] = {};
    bool any = false;
    for (int i = 0; i < count; ++i) any |= grows[i] = bytes[i] > bufs[i]->bytes;
    if (!any) return OK;
    if (!dev.sync()) return SYNC_FAILED;
    for (int i = 0; i < count; ++i)
        if (grows[i]) release(dev, *bufs[i]);
    for (int i = 0; i < count; ++i) {
        if (!grows[i]) continue;
        if (!dev.alloc(&bufs[i]->p, bytes[i]) || !bufs[i]->p) {
            bufs[i]->p = nullptr;
            for (int j = 0; j < i; ++j)
                if (grows[j]) release(dev, *bufs[j]);
            return NO_MEMORY;
        }
        bufs[i]->bytes = bytes[i];
    }
    return OK;
}

template <typename Dev>
Result reserve(Dev &dev, LemonBuf &buf, size_t bytes) {
    LemonBuf *one = &buf;
    return reserve_group(dev, &one, &bytes, 1);
}

}  // namespace lemon_ws
