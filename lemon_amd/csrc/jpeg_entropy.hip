// jpeg_entropy.hip -- the Huffman pass of a baseline JPEG on the device (lemon_jpeg_entropy_device, include/lemon_hip.h): a batch
// of scan packets (lemon_jpeg_pack) -> the coefficient records lemon_jpeg_decode reads, bit for bit what lemon_jpeg_entropy writes,
// and one status per image.  The scheme, the packet and every per-symbol function are in jpeg_par.hpp; this file holds the
// kernels that run its lanes in parallel.  Nothing is exchanged between workgroups inside a launch: every step that needs another
// workgroup's result is a launch of its own.
//   k_jent_plan   one workgroup per image: validates the packet against its extents, sums the interval lengths into first
//                 bytes and first lanes, initialises the status
//   k_jent_zero   clears the accepted images' records and writes their quantisers
//   k_jent_sync   one lane per thread, 256 per workgroup, tables built in LDS; launched LEMON_JPEG_PAR_ROUNDS times
//   k_jent_scan   one workgroup per image: exclusive sums of the lanes' block counts inside each interval
//   k_jent_final  the final pass: coefficients, DC differences, the lanes' verdicts
//   k_jent_dc     one workgroup per (image, component): DC differences -> DC values, segmented by interval, 64-bit
//   k_jent_check  one thread per block: the envelope
// Every loop is bounded by a size of the packet or by LEMON_JPEG_PAR_GROUP; an image whose packet, record or workspace share
// would leave its buffer gets LEMON_JPEG_BUFFER from k_jent_plan and is not touched by any other kernel.
#include "common.hpp"
#include "jpeg_par.hpp"

namespace {

using namespace lemon_jpeg_par;

#define JENT_T LEMON_JPEG_PAR_GROUP
#define JENT_ZY 32               // workgroups per image of k_jent_zero and k_jent_check (grid-stride)
#define JENT_FIRST 0x80000000u   // in a lane's stored block count: the lane is the first of its interval

struct JentWs {                  // the workspace, carved by jent_carve()
    int32_t *img;                // [batch][4] ok, lanes, the most iterations a workgroup of the image ran in k_jent_sync (a
                                 //            diagnostic: tools/jpeg_entropy_time.py reads it), 0
    uint32_t *ivl_start, *ivl_len, *ivl_lane0;       // [total_intervals]
    uint64_t *entry, *exit_;     // [total_groups * 256]
    int64_t *first_blk;          // [total_groups * 256]
    uint32_t *cnt;               // [total_groups * 256]
    uint64_t *wgexit;            // [2][total_groups]
};

struct JentParams {
    const uint8_t *pk;
    const int64_t *desc;         // [batch][8] packet offset, packet bytes, record offset, intervals, first workgroup, first interval
                                 //            slot, workgroups, 0
    uint8_t *rec;
    int32_t *status;
    JentWs ws;
    int64_t batch, pk_bytes, rec_bytes, total_groups, total_intervals;
    int32_t subseq;
};

inline int64_t jent_carve(char *base, int64_t batch, int64_t groups, int64_t intervals, JentWs *ws) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *p = base + o; o += (bytes + 15) & ~(int64_t)15; return p; };
    const int64_t lanes = groups * JENT_T;
    JentWs w;
    w.img = (int32_t *)take(batch * 16);
    w.ivl_start = (uint32_t *)take(intervals * 4); w.ivl_len = (uint32_t *)take(intervals * 4); w.ivl_lane0 = (uint32_t *)take(intervals * 4);
    w.entry = (uint64_t *)take(lanes * 8); w.exit_ = (uint64_t *)take(lanes * 8); w.first_blk = (int64_t *)take(lanes * 8);
    w.cnt = (uint32_t *)take(lanes * 4);
    w.wgexit = (uint64_t *)take(2 * groups * 8);
    if (ws) *ws = w;
    return o + 16;
}

// the image's descriptor against the buffers' extents, then its packet (jpeg_par.hpp::par_open)
__device__ __forceinline__ bool jent_open(const JentParams &p, int64_t i, ParImage &im) {
    const int64_t *d = p.desc + 8 * i;
    if (!jpeg_dev_extents(d, p.pk_bytes, p.rec_bytes)) return false;
    if (d[4] < 0 || d[6] < 0 || d[4] > p.total_groups || d[6] > p.total_groups - d[4]) return false;
    if (d[5] < 0 || d[3] < 1 || d[5] > p.total_intervals || d[3] > p.total_intervals - d[5]) return false;
    if (!par_open(p.pk + d[0], d[1], p.rec_bytes - d[2], im)) return false;
    return im.nivl == d[3];
}

__device__ __forceinline__ int64_t jent_owner(const JentParams &p, int64_t wg) {
    int64_t lo = 0, hi = p.batch;                // largest i with first workgroup <= wg
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (p.desc[8 * mid + 4] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t jent_scan(uint64_t v, uint64_t *s, int t) {          // inclusive, 256 threads
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < JENT_T; d <<= 1) {
        const uint64_t x = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const uint64_t r = s[t];
    __syncthreads();
    return r;
}

// inclusive sums that start over at every head; f returns whether a head lies at or before the thread in the chunk
__device__ __forceinline__ void jent_seg_scan(int64_t &v, int &f, int64_t *sv, int *sf, int t) {
    sv[t] = v; sf[t] = f;
    __syncthreads();
    for (int d = 1; d < JENT_T; d <<= 1) {
        int64_t xv = 0;
        int xf = 0;
        if (t >= d) { xv = sv[t - d]; xf = sf[t - d]; }
        __syncthreads();
        if (t >= d) {
            if (!sf[t]) sv[t] += xv;
            sf[t] |= xf;
        }
        __syncthreads();
    }
    v = sv[t]; f = sf[t];
    __syncthreads();
}

__device__ __forceinline__ void jent_tables(const ParImage &im, ParHuff *huff, int t) {
    if (t < 6 && (t % 3) < im.nc) {
        par_build_huff(par_spec(im, t % 3, t / 3), huff[t]);
    }
    __syncthreads();
}

// lane jl of image i (jl < the image's lanes)
__device__ __forceinline__ void jent_lane(const JentParams &p, const ParImage &im, int64_t ivl0, int64_t jl, ParLane &l) {
    const uint32_t *lane0 = p.ws.ivl_lane0 + ivl0;
    int64_t lo = 0, hi = im.nivl;                // largest t with lane0[t] <= jl
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)lane0[mid] <= jl) lo = mid; else hi = mid;
    }
    const int64_t t = lo, i = jl - lane0[t], S = p.subseq;
    l.len = p.ws.ivl_len[ivl0 + t];
    l.d = im.scan + p.ws.ivl_start[ivl0 + t];
    l.end_bit = 8 * (l.len < (i + 1) * S ? l.len : (i + 1) * S);
    const McuRange r = interval_mcus(im.restart, im.mcus, t);
    l.mcu0 = r.first; l.total = r.count * im.spm;
    l.guess = par_state(8 * i * S, 0, 0);
    l.first = i == 0;
    l.last = i + 1 == par_lanes_of(l.len, (int32_t)S);
}

__global__ __launch_bounds__(JENT_T) void k_jent_plan(JentParams p) {
    __shared__ uint64_t s_scan[JENT_T];
    __shared__ ParHuff s_huff;
    __shared__ int s_ok;
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    ParImage im;
    bool ok = jent_open(p, i, im);
    if (t == 0) s_ok = 1;
    __syncthreads();
    if (ok && t == 0)
        for (int c = 0; c < im.nc; ++c)
            if (!par_build_huff(par_spec(im, c, 0), s_huff) || !par_build_huff(par_spec(im, c, 1), s_huff)) s_ok = 0;
    __syncthreads();
    ok = ok && s_ok;
    uint64_t bytes = 0, lanes = 0;
    if (ok) {                                   // (uniform: every thread opened the same packet)
        const int64_t ivl0 = p.desc[8 * i + 5];
        for (int64_t base = 0; base < im.nivl; base += JENT_T) {
            const int64_t k = base + t;
            const uint64_t len = k < im.nivl ? (uint64_t)par_interval_bytes(im, k) : 0;
            const uint64_t ln = k < im.nivl ? (uint64_t)par_lanes_of((int64_t)len, p.subseq) : 0;
            const uint64_t a = jent_scan(len, s_scan, t), b = jent_scan(ln, s_scan, t);
            if (k < im.nivl && bytes + a <= (uint64_t)im.scan_bytes && lanes + b <= 0xFFFFFFFFull) {
                p.ws.ivl_start[ivl0 + k] = (uint32_t)(bytes + a - len);
                p.ws.ivl_len[ivl0 + k] = (uint32_t)len;
                p.ws.ivl_lane0[ivl0 + k] = (uint32_t)(lanes + b - ln);
            }
            s_scan[t] = a;
            __syncthreads();
            bytes += s_scan[JENT_T - 1];
            __syncthreads();
            s_scan[t] = b;
            __syncthreads();
            lanes += s_scan[JENT_T - 1];
            __syncthreads();
            if (bytes > (uint64_t)im.scan_bytes) break;          // (uniform)
        }
        ok = bytes == (uint64_t)im.scan_bytes && lanes <= (uint64_t)p.desc[8 * i + 6] * JENT_T;
    }
    if (t == 0) {
        p.ws.img[4 * i] = ok ? 1 : 0;
        p.ws.img[4 * i + 1] = ok ? (int32_t)lanes : 0;
        p.ws.img[4 * i + 2] = p.ws.img[4 * i + 3] = 0;
        p.status[i] = ok ? LEMON_JPEG_OK : LEMON_JPEG_BUFFER;
    }
}

__global__ __launch_bounds__(JENT_T) void k_jent_zero(JentParams p) {
    const int64_t i = blockIdx.x;
    ParImage im;
    if (!p.ws.img[4 * i] || !jent_open(p, i, im)) return;
    jpeg_dev_new_record(p.rec + p.desc[8 * i + 2], im.pkt, im.g, (int64_t)blockIdx.y * JENT_T + threadIdx.x, (int64_t)JENT_ZY * JENT_T);
}

__global__ __launch_bounds__(JENT_T) void k_jent_sync(JentParams p, int round) {
    __shared__ ParHuff s_huff[6];
    __shared__ uint64_t s_exit[JENT_T];
    const int64_t wg = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t i = jent_owner(p, wg);
    ParImage im;
    if (!p.ws.img[4 * i] || !jent_open(p, i, im)) return;
    const int64_t wg0 = p.desc[8 * i + 4], ivl0 = p.desc[8 * i + 5];
    if (wg < wg0 || wg - wg0 >= p.desc[8 * i + 6]) return;
    const int64_t jl = (wg - wg0) * JENT_T + t, g = wg * JENT_T + t;
    const bool active = jl < p.ws.img[4 * i + 1];
    ParLane lane;
    lane.first = false; lane.guess = 0;
    if (active) jent_lane(p, im, ivl0, jl, lane);
    uint64_t entry = 0, exit_ = 0;
    int64_t cnt = 0;
    bool done;
    const uint64_t wg_entry = round > 0 && wg > wg0 ? p.ws.wgexit[((round - 1) & 1) * p.total_groups + wg - 1] : lane.guess;
    if (round > 0) {
        entry = p.ws.entry[g]; exit_ = p.ws.exit_[g]; cnt = p.ws.cnt[g] & ~JENT_FIRST;
        // nothing to do when the one entry that can have changed, the first lane's, has not
        const bool moved = active && t == 0 && !lane.first && wg_entry != entry;
        if (!__syncthreads_or(moved)) {
            if (t == JENT_T - 1) p.ws.wgexit[(round & 1) * p.total_groups + wg] = exit_;
            return;
        }
    }
    jent_tables(im, s_huff, t);
    if (round == 0 && active) {
        entry = exit_ = lane.guess;
        par_run<false>(s_huff, im, lane, exit_, cnt, nullptr, 0, done);
    }
    s_exit[t] = exit_;
    __syncthreads();
    int it = 0;
    for (; it <= JENT_T; ++it) {                 // (iteration k settles lane k at the latest)
        const uint64_t left = lane.first ? lane.guess : (t == 0 ? wg_entry : s_exit[t - 1]);
        const bool changed = active && left != entry;
        if (changed) {
            entry = exit_ = left;
            cnt = 0;
            par_run<false>(s_huff, im, lane, exit_, cnt, nullptr, 0, done);
        }
        __syncthreads();
        if (changed) s_exit[t] = exit_;
        if (!__syncthreads_or(changed)) break;
    }
    p.ws.entry[g] = entry; p.ws.exit_[g] = exit_;
    p.ws.cnt[g] = (uint32_t)cnt | (active && lane.first ? JENT_FIRST : 0u);
    if (t == JENT_T - 1) p.ws.wgexit[(round & 1) * p.total_groups + wg] = exit_;
    if (t == 0) atomicMax(p.ws.img + 4 * i + 2, it + (round == 0));
}

__global__ __launch_bounds__(JENT_T) void k_jent_scan(JentParams p) {
    __shared__ int64_t s_v[JENT_T];
    __shared__ int s_f[JENT_T];
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    if (!p.ws.img[4 * i]) return;
    const int64_t lanes = p.ws.img[4 * i + 1], g0 = p.desc[8 * i + 4] * JENT_T;
    if (lanes > p.desc[8 * i + 6] * JENT_T || g0 < 0 || g0 > (p.total_groups - p.desc[8 * i + 6]) * JENT_T) return;
    int64_t carry = 0;
    for (int64_t base = 0; base < lanes; base += JENT_T) {
        const int64_t j = base + t;
        const uint32_t c = j < lanes ? p.ws.cnt[g0 + j] : 0;
        int64_t v = c & ~JENT_FIRST;
        const int64_t own = v;
        int f = (c & JENT_FIRST) != 0;
        jent_seg_scan(v, f, s_v, s_f, t);
        if (!f) v += carry;
        if (j < lanes) p.ws.first_blk[g0 + j] = v - own;
        s_v[t] = v;
        __syncthreads();
        carry = s_v[JENT_T - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(JENT_T) void k_jent_final(JentParams p) {
    __shared__ ParHuff s_huff[6];
    const int64_t wg = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t i = jent_owner(p, wg);
    ParImage im;
    if (!p.ws.img[4 * i] || !jent_open(p, i, im)) return;
    const int64_t wg0 = p.desc[8 * i + 4], ivl0 = p.desc[8 * i + 5];
    if (wg < wg0 || wg - wg0 >= p.desc[8 * i + 6]) return;
    const int64_t jl = (wg - wg0) * JENT_T + t, g = wg * JENT_T + t;
    jent_tables(im, s_huff, t);
    if (jl >= p.ws.img[4 * i + 1]) return;
    ParLane lane;
    jent_lane(p, im, ivl0, jl, lane);
    int16_t *coef = reinterpret_cast<int16_t *>(p.rec + p.desc[8 * i + 2] + LEMON_JPEG_QUANT_BYTES);
    const int rc = par_final_lane(s_huff, im, lane, lane.first ? lane.guess : p.ws.exit_[g - 1], p.ws.entry[g],
                                  p.ws.exit_[g], p.ws.first_blk[g], coef);
    if (rc != LEMON_JPEG_OK) atomicMax(p.status + i, rc);
}

__global__ __launch_bounds__(JENT_T) void k_jent_dc(JentParams p) {
    __shared__ int64_t s_v[JENT_T];
    __shared__ int s_f[JENT_T];
    const int64_t i = blockIdx.x;
    const int c = blockIdx.y, t = threadIdx.x;
    ParImage im;
    if (!p.ws.img[4 * i] || !jent_open(p, i, im) || c >= im.nc) return;
    int16_t *coef = reinterpret_cast<int16_t *>(p.rec + p.desc[8 * i + 2] + LEMON_JPEG_QUANT_BYTES);
    const int64_t nb = c == 0 ? im.g.n0 : im.g.nc;
    int64_t carry = 0;
    bool bad = false;
    for (int64_t base = 0; base < nb; base += JENT_T) {
        const int64_t q = base + t;
        bool head = false;
        int16_t *b = nullptr;
        int64_t v = 0;
        if (q < nb) {
            b = coef + 64 * par_comp_block_addr(im, c, q, head);
            v = b[0];
        }
        int f = head;
        jent_seg_scan(v, f, s_v, s_f, t);
        if (!f) v += carry;
        if (q < nb) {
            if (v < -32768 || v > 32767) bad = true;
            b[0] = (int16_t)v;
        }
        s_v[t] = v;
        __syncthreads();
        carry = s_v[JENT_T - 1];
        __syncthreads();
    }
    if (bad) atomicMax(p.status + i, (int)LEMON_JPEG_CODE);
}

__global__ __launch_bounds__(JENT_T) void k_jent_check(JentParams p) {
    const int64_t i = blockIdx.x;
    ParImage im;
    if (!p.ws.img[4 * i] || !jent_open(p, i, im)) return;
    if (!par_envelope_blocks(p.rec + p.desc[8 * i + 2], im.g, (int64_t)blockIdx.y * JENT_T + threadIdx.x, (int64_t)JENT_ZY * JENT_T))
        atomicMax(p.status + i, (int)LEMON_JPEG_ENVELOPE);
}

}  // namespace

extern "C" int64_t lemon_jpeg_entropy_workspace_bytes(int64_t batch, int64_t total_groups, int64_t total_intervals) {
    if (batch < 0 || total_groups < 0 || total_intervals < 0 || total_groups > ((int64_t)1 << 22) || total_intervals > ((int64_t)1 << 31))
        return LEMON_E_INVALID;
    return jent_carve(nullptr, batch, total_groups, total_intervals, nullptr);
}

extern "C" int lemon_jpeg_entropy_device(const uint8_t *packets_dev, int64_t packets_bytes, int64_t batch, const int64_t *desc_dev,
                                         int64_t total_groups, int64_t total_intervals, int32_t subseq_bytes, uint8_t *rec_dev,
                                         int64_t rec_bytes, int32_t *status_dev, void *ws_dev, int64_t ws_bytes, void *stream) {
    LEMON_REQUIRE(batch >= 0 && packets_bytes >= 0 && rec_bytes >= 0 && total_groups >= 0 && total_intervals >= 0 && ws_bytes >= 0,
                  "batch, byte counts, group and interval counts >= 0");
    LEMON_REQUIRE(par_subseq_ok(subseq_bytes), "subseq_bytes: 0 or a multiple of 4 in [16, 4096]");
    if (batch == 0) return LEMON_OK;
    LEMON_REQUIRE(packets_dev && desc_dev && rec_dev && status_dev && ws_dev, "null pointer");
    LEMON_REQUIRE(batch < ((int64_t)1 << 31) && total_groups <= ((int64_t)1 << 22) && total_intervals <= ((int64_t)1 << 31),
                  "batch < 2^31, total_groups <= 2^22, total_intervals <= 2^31");
    LEMON_REQUIRE((((uintptr_t)packets_dev) & 15) == 0 && (((uintptr_t)rec_dev) & 15) == 0 && (((uintptr_t)ws_dev) & 15) == 0,
                  "packets_dev, rec_dev, ws_dev 16-byte aligned");
    JentParams p;
    LEMON_REQUIRE(jent_carve((char *)ws_dev, batch, total_groups, total_intervals, &p.ws) <= ws_bytes,
                  "ws_bytes < lemon_jpeg_entropy_workspace_bytes()");
    p.pk = packets_dev; p.desc = desc_dev; p.rec = rec_dev; p.status = status_dev;
    p.batch = batch; p.pk_bytes = packets_bytes; p.rec_bytes = rec_bytes; p.total_groups = total_groups;
    p.total_intervals = total_intervals; p.subseq = par_subseq(subseq_bytes);
    hipStream_t s = (hipStream_t)stream;
    const dim3 T(JENT_T);
    hipLaunchKernelGGL(k_jent_plan, dim3((unsigned)batch), T, 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jent_zero, dim3((unsigned)batch, JENT_ZY), T, 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    if (total_groups) {
        for (int r = 0; r < LEMON_JPEG_PAR_ROUNDS; ++r) {
            hipLaunchKernelGGL(k_jent_sync, dim3((unsigned)total_groups), T, 0, s, p, r);
            LEMON_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_jent_scan, dim3((unsigned)batch), T, 0, s, p);
        LEMON_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_jent_final, dim3((unsigned)total_groups), T, 0, s, p);
        LEMON_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_jent_dc, dim3((unsigned)batch, 3), T, 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_jent_check, dim3((unsigned)batch, JENT_ZY), T, 0, s, p);
    LEMON_HIP_CHECK(hipGetLastError());
    return LEMON_OK;
}
