// dpq_flat_ivf_device.h -- the key sink the list scans over raw rows share (dpq_flat_ivf.hip: fp32 rows, dpq_flat_ivf_u8.hip:
// byte rows).  Per (query, probed list) pair of a stretch a buffer of cap = 2 P2 keys in LDS, P2 the
// power of two >= max(top_k, 256); a count and a threshold per pair.  A key below its pair's threshold is appended by an
// LDS atomic on the count; when a buffer could overflow on the next tile of kFlatIvfTileRows rows, the buffers of the
// stretch are sorted side by side (one bitonic network, the same barriers for all), cut to top_k, and the thresholds
// become the k-th keys.  Included by the two .hip files only; every function is called by all 256 threads of a workgroup
// with arguments that are the same in every thread.
#pragma once
#include "dpq_flat.h"
#include "dpq_flat_ivf.h"

namespace dpq {
namespace {

constexpr uint32_t kNoRow = 0xffffffffu;  // a slot of the row tile beyond the list's end

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

int scan_cap(int top_k) { return 2 * pow2_at_least(std::max(top_k, 256)); }

// Sorts nb buffers of n keys each (n a power of two >= 2), `stride` keys apart, ascending: ivf_bitonic's network over
// every buffer at once.  Every thread of the workgroup calls it.  Ends behind a barrier.
__device__ __forceinline__ void sort_buffers(uint64_t* buf, int nb, int n, int stride, int tid) {
    const int half = n >> 1, hs = __ffs(half) - 1, total = nb * half;
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < total; t += 256) {
                const int u = t & (half - 1);
                uint64_t* b = buf + (size_t)(t >> hs) * stride;
                const int i = ((u & ~(j - 1)) << 1) | (u & (j - 1));
                const int l = i | j;
                const uint64_t x = b[i], y = b[l];
                const bool up = (i & k) == 0;
                if ((x > y) == up) {
                    b[i] = y;
                    b[l] = x;
                }
            }
            __syncthreads();
        }
}

// The buffers of the stretch's nqs pairs, each padded to the power of two >= the largest count mx, sorted.  Behind a
// barrier that closed the appends; ends behind a barrier.
__device__ __forceinline__ void sink_sort_to(uint64_t* buf, const uint32_t* s_cnt, int nqs, int cap, uint32_t mx, int tid) {
    int n = 2;
    while ((uint32_t)n < mx) n <<= 1;
    for (int p = 0; p < nqs; ++p)
        for (int i = (int)s_cnt[p] + tid; i < n; i += 256) buf[(size_t)p * cap + i] = kFlatNoKey;
    __syncthreads();
    sort_buffers(buf, nqs, n, cap, tid);
}

// ... with the largest count found here.
__device__ __forceinline__ void sink_sort(uint64_t* buf, const uint32_t* s_cnt, int nqs, int cap, int tid) {
    uint32_t mx = 0u;
    for (int p = 0; p < nqs; ++p) mx = max(mx, s_cnt[p]);
    sink_sort_to(buf, s_cnt, nqs, cap, mx, tid);
}

// Between two tiles, behind the barrier that closed the first one's appends: when a buffer has no room for the next
// tile, sort, keep top_k, lower the thresholds.  The caller's next barrier publishes the counts and thresholds.
__device__ __forceinline__ void sink_make_room(uint64_t* buf, uint32_t* s_cnt, uint64_t* s_thr, int nqs, int cap, int top_k,
                                               int tid) {
    uint32_t mx = 0u;
    for (int p = 0; p < nqs; ++p) mx = max(mx, s_cnt[p]);
    if (mx + kFlatIvfTileRows > (uint32_t)cap) {
        sink_sort_to(buf, s_cnt, nqs, cap, mx, tid);
        if (tid < nqs) {
            const uint32_t c = s_cnt[tid];
            if (c >= (uint32_t)top_k) s_thr[tid] = buf[(size_t)tid * cap + top_k - 1];  // ids are unique in a list: the
            s_cnt[tid] = min(c, (uint32_t)top_k);                                      // strict test loses nothing
        }
    }
}

// The answer of one pair: the first min(cnt, top_k) keys of its sorted buffer, padded with -1 / +inf.
__device__ __forceinline__ void sink_emit(const uint64_t* b, uint32_t cnt, int top_k, int32_t* out_i, float* out_d, int tid) {
    for (int r = tid; r < top_k; r += 256) {
        const uint64_t key = (uint32_t)r < cnt ? b[r] : kFlatNoKey;
        out_i[r] = key != kFlatNoKey ? (int32_t)(key & 0xffffffffu) : -1;
        out_d[r] = key != kFlatNoKey ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
    }
}

}  // namespace
}  // namespace dpq
