// jpeg_prog.hip -- the Huffman pass of a progressive JPEG on the device (lemon_jpeg_prog_entropy_device, include/lemon_hip.h): a
// batch of packets (lemon_jpeg_prog_pack) -> the coefficient records lemon_jpeg_decode reads, bit for bit what
// lemon_jpeg_prog_entropy writes, and one status per image.  The packet, the work items, the verdict rule and every step function
// are in jpeg_prog_par.hpp; this file holds the wave (lane k = zig-zag coefficient k of the current block) and the launches.
// Nothing is exchanged between waves inside a launch:
//   k_jprog_plan   one wave per image: validates the packet and every scan row against the extents, recomputes the levels,
//                  writes the image's work items, initialises its status
//   k_jprog_zero   clears the accepted images' records and writes their quantisers
//   k_jprog_level  one wave per work item, launched once per level; an image that raised a code at a lower level is skipped
//   k_jprog_check  the status of the first level that raised one, else the envelope of every block
// Every loop is bounded by a size of the packet, by 64 or by a block count; every symbol consumes at least one bit.
#include "common.hpp"
#include "jpeg_prog_par.hpp"

namespace {

using namespace lemon_jpeg_prog;

#define JPROG_T 64
#define JPROG_ZT 256
#define JPROG_ZY 32              // workgroups per image of k_jprog_zero and k_jprog_check (grid-stride)

struct JprogWs {
    int32_t *img;                // [batch] 1 = the plan accepted the image
    int32_t *err;                // [levels][batch] the largest code the items of a level raised
    int32_t *item;               // [total_items][4] image, scan, group, level; image < 0: none
};

struct JprogParams {
    const uint8_t *pk;
    const int64_t *desc;         // [batch][8] packet offset, packet bytes, record offset, first item slot, items, 0, 0, 0
    uint8_t *rec;
    int32_t *status;
    JprogWs ws;
    int64_t batch, pk_bytes, rec_bytes, total_items;
    int32_t levels;
};

inline int64_t jprog_carve(char *base, int64_t batch, int64_t items, int32_t levels, JprogWs *ws) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *p = base + o; o += (bytes + 15) & ~(int64_t)15; return p; };
    JprogWs w;
    w.img = (int32_t *)take(batch * 4);
    w.err = (int32_t *)take(batch * 4 * levels);
    w.item = (int32_t *)take(items * 16);
    if (ws) *ws = w;
    return o + 16;
}

// the image's descriptor against the buffers' extents, then its packet head (jpeg_prog_par.hpp::prog_open)
__device__ __forceinline__ bool jprog_open(const JprogParams &p, int64_t i, ProgImage &im) {
    const int64_t *d = p.desc + 8 * i;
    if (!lemon_jpeg_par::jpeg_dev_extents(d, p.pk_bytes, p.rec_bytes)) return false;
    if (d[3] < 0 || d[4] < 1 || d[3] > p.total_items || d[4] > p.total_items - d[3]) return false;
    if (!prog_open(p.pk + d[0], d[1], p.rec_bytes - d[2], im)) return false;
    return im.items == d[4] && im.levels <= p.levels;
}

// the wave: lane k holds zig-zag coefficient k of the current block (jpeg_prog_par.hpp::HostWave is the looped form)
struct DevWave {
    int lane, nat;               // nat: the lane's coefficient in natural order
    int16_t c, pre;
    const int16_t *pre_of;       // the block `pre` was fetched from
    __device__ __forceinline__ void load(const int16_t *blk, const int16_t *nxt) {
        c = blk == pre_of ? pre : blk[nat];                          // one 128-byte line per block
        pre_of = nxt;
        if (nxt) pre = nxt[nat];                                     // in flight while this block is decoded
    }
    __device__ __forceinline__ void clear() { c = 0; }
    __device__ __forceinline__ uint64_t nonzero() const { return __ballot(c != 0); }
    __device__ __forceinline__ void set(int k, int32_t v) { if (lane == k) c = (int16_t)v; }
    __device__ __forceinline__ void refine(uint64_t F, int64_t fb, const uint8_t *d, int64_t len, int32_t p1) {
        c = prog_refine_lane(c, lane, F, fb, d, len, p1);
    }
    __device__ __forceinline__ void store(int16_t *blk, uint64_t lanes) const { if ((lanes >> lane) & 1) blk[nat] = c; }
    __device__ __forceinline__ void store_dc(int16_t *blk, int32_t v) const { if (lane == 0) blk[0] = (int16_t)v; }
    __device__ __forceinline__ void dc_refine(const ProgImage &im, const ProgScan &sc, int16_t *coef, int64_t q0, int64_t nblk,
                                              const uint8_t *d, int64_t len, int32_t p1) const {
        for (int64_t i = lane; i < nblk; i += JPROG_T)
            if (prog_bit_at(d, len, i)) coef[64 * prog_block_addr(im, sc, q0 + i)] |= (int16_t)p1;
    }
};

__global__ __launch_bounds__(JPROG_T) void k_jprog_plan(JprogParams p) {
    __shared__ int32_t s_items[64];
    __shared__ int32_t s_first[65];
    __shared__ int s_ok;
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    ProgImage im;
    bool ok = jprog_open(p, i, im);                                  // (uniform: every thread opened the same packet)
    int32_t mine = 0;
    if (ok && t < im.scans) mine = prog_plan_row(im, t);
    s_items[t] = mine;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        bool good = ok;
        for (int s = 0; good && s < im.scans; ++s) {
            if (s_items[s] < 0) good = false;
            s_first[s] = (int32_t)run;
            run += s_items[s] < 0 ? 0 : s_items[s];
        }
        s_ok = good && run == im.items;
    }
    __syncthreads();
    ok = ok && s_ok;
    if (ok && t < im.scans) {
        ProgScan sc;
        prog_scan(im, t, sc);
        int32_t *it = p.ws.item + 4 * (p.desc[8 * i + 3] + s_first[t]);
        for (int32_t g = 0; g < mine; ++g) { it[4 * g] = (int32_t)i; it[4 * g + 1] = t; it[4 * g + 2] = g; it[4 * g + 3] = sc.level; }
    }
    if (t < p.levels) p.ws.err[(int64_t)t * p.batch + i] = 0;
    if (t == 0) {
        p.ws.img[i] = ok ? 1 : 0;
        p.status[i] = ok ? LEMON_JPEG_OK : LEMON_JPEG_BUFFER;
    }
}

__global__ __launch_bounds__(JPROG_ZT) void k_jprog_zero(JprogParams p) {
    const int64_t i = blockIdx.x;
    ProgImage im;
    if (!p.ws.img[i] || !jprog_open(p, i, im)) return;
    lemon_jpeg_par::jpeg_dev_new_record(p.rec + p.desc[8 * i + 2], im.pkt, im.g, (int64_t)blockIdx.y * JPROG_ZT + threadIdx.x,
                                        (int64_t)JPROG_ZY * JPROG_ZT);
}

__global__ __launch_bounds__(JPROG_T) void k_jprog_level(JprogParams p, int level) {
    __shared__ ParHuff s_huff[3];
    __shared__ int s_ok;
    const int t = threadIdx.x;
    const int32_t *it = p.ws.item + 4 * (int64_t)blockIdx.x;
    const int64_t i = it[0];
    if (i < 0 || i >= p.batch || it[3] != level || !p.ws.img[i]) return;
    for (int l = 0; l < level; ++l)
        if (p.ws.err[(int64_t)l * p.batch + i] != 0) return;         // (written by earlier launches only)
    ProgImage im;
    ProgScan sc;
    if (!jprog_open(p, i, im)) return;
    const int64_t slot = (int64_t)blockIdx.x - p.desc[8 * i + 3];
    if (slot < 0 || slot >= p.desc[8 * i + 4] || it[1] < 0 || it[1] >= im.scans || !prog_scan(im, it[1], sc)) return;
    if (sc.level != level || it[2] < 0 || it[2] >= sc.items) return;
    if (t == 0) s_ok = prog_scan_tables(im, sc, s_huff);
    __syncthreads();
    int rc = LEMON_JPEG_TABLE;
    if (s_ok) {
        DevWave wv;
        wv.lane = t; wv.nat = lemon_jpeg::kZigzag[t]; wv.c = 0; wv.pre = 0; wv.pre_of = nullptr;
        int16_t *coef = reinterpret_cast<int16_t *>(p.rec + p.desc[8 * i + 2] + LEMON_JPEG_QUANT_BYTES);
        rc = prog_item(im, sc, s_huff, it[2], coef, wv);
    }
    if (rc != LEMON_JPEG_OK && t == 0) atomicMax(p.ws.err + (int64_t)level * p.batch + i, rc);
}

__global__ __launch_bounds__(JPROG_ZT) void k_jprog_check(JprogParams p) {
    const int64_t i = blockIdx.x;
    ProgImage im;
    if (!p.ws.img[i] || !jprog_open(p, i, im)) return;
    for (int l = 0; l < p.levels; ++l) {
        const int32_t e = p.ws.err[(int64_t)l * p.batch + i];
        if (e != 0) {
            if (blockIdx.y == 0 && threadIdx.x == 0) p.status[i] = e;
            return;
        }
    }
    if (!lemon_jpeg_par::par_envelope_blocks(p.rec + p.desc[8 * i + 2], im.g, (int64_t)blockIdx.y * JPROG_ZT + threadIdx.x,
                                             (int64_t)JPROG_ZY * JPROG_ZT))
        atomicMax(p.status + i, (int)LEMON_JPEG_ENVELOPE);
}

}  // namespace

extern "C" int64_t lemon_jpeg_prog_entropy_workspace_bytes(int64_t batch, int64_t total_items, int32_t levels) {
    if (batch < 0 || total_items < 0 || levels < 0 || levels > 64 || batch >= ((int64_t)1 << 31) || total_items >= ((int64_t)1 << 31))
        return LEMON_E_INVALID;
    return jprog_carve(nullptr, batch, total_items, levels, nullptr);
}

extern "C" int lemon_jpeg_prog_entropy_device(const uint8_t *packets_dev, int64_t packets_bytes, int64_t batch, const int64_t *desc_dev,
                                              int64_t total_items, int32_t levels, uint8_t *rec_dev, int64_t rec_bytes,
                                              int32_t *status_dev, void *ws_dev, int64_t ws_bytes, void *stream) {
    LEMON_REQUIRE(batch >= 0 && packets_bytes >= 0 && rec_bytes >= 0 && total_items >= 0 && ws_bytes >= 0,
                  "batch, byte counts and item count >= 0");
    LEMON_REQUIRE(levels >= 0 && levels <= 64, "levels in [0, 64]");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(packets_dev && desc_dev && rec_dev && status_dev && ws_dev, "null pointer");
    LEMON_REQUIRE(batch < ((int64_t)1 << 31) && total_items < ((int64_t)1 << 31), "batch, total_items < 2^31");
    LEMON_REQUIRE((((uintptr_t)packets_dev) & 15) == 0 && (((uintptr_t)rec_dev) & 15) == 0 && (((uintptr_t)ws_dev) & 15) == 0,
                  "packets_dev, rec_dev, ws_dev 16-byte aligned");
    JprogParams p;
    LEMON_REQUIRE(jprog_carve((char *)ws_dev, batch, total_items, levels, &p.ws) <= ws_bytes,
                  "ws_bytes < lemon_jpeg_prog_entropy_workspace_bytes()");
    p.pk = packets_dev; p.desc = desc_dev; p.rec = rec_dev; p.status = status_dev;
    p.batch = batch; p.pk_bytes = packets_bytes; p.rec_bytes = rec_bytes; p.total_items = total_items; p.levels = levels;
    hipStream_t s = (hipStream_t)stream;
    if (total_items) LEMON_HIP_CHECK(hipMemsetAsync(p.ws.item, 0xFF, (size_t)total_items * 16, s));     // image -1: no item
    hipLaunchKernelGGL(k_jprog_plan, dim3((unsigned)batch), dim3(JPROG_T), 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jprog_zero, dim3((unsigned)batch, JPROG_ZY), dim3(JPROG_ZT), 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    for (int level = 0; total_items && level < levels; ++level) {
        hipLaunchKernelGGL(k_jprog_level, dim3((unsigned)total_items), dim3(JPROG_T), 0, s, p, level);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_jprog_check, dim3((unsigned)batch, JPROG_ZY), dim3(JPROG_ZT), 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
