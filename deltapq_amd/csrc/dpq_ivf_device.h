// dpq_ivf_device.h -- the device helpers the list scans share (dpq_ivf.hip, dpq_ivf_residual.hip): the sort of a
// workgroup's key buffer, the key of a list entry under a table in LDS, a filter's test of an entry.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dpq_flat.h"
#include "dpq_ivf.h"

namespace dpq {

// Sorts buf[0, n) ascending, n a power of two >= 2; every thread of the workgroup calls it.  Ends behind a barrier.
__device__ __forceinline__ void ivf_bitonic(uint64_t* buf, int n, int tid) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t a = buf[i], b = buf[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
}

// The cnt keys of buf sorted, the rest of the next power of two filled with padding.  Ends behind a barrier.
__device__ __forceinline__ void ivf_sort_keys(uint64_t* buf, uint32_t cnt, int tid) {
    int n = 2;
    while ((uint32_t)n < cnt) n <<= 1;
    for (int i = (int)cnt + tid; i < n; i += 256) buf[i] = kFlatNoKey;
    __syncthreads();
    ivf_bitonic(buf, n, tid);
}

// The key of list entry `at` under the table in LDS: ivf_scan_kernel's arithmetic, to the bit.
template <int M, bool PLAIN_RULE>
__device__ __forceinline__ uint64_t ivf_entry_key(const float* T, const uint8_t* __restrict__ codes, int64_t at, int32_t id) {
    uint32_t w[M / 4];
    if constexpr (M == 8) {
        const uint2 v = reinterpret_cast<const uint2*>(codes)[at];
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = reinterpret_cast<const uint4*>(codes)[at];
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    [[maybe_unused]] double acc64 = 0.0;
    [[maybe_unused]] float acc32 = 0.0f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float e = T[m * 256 + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)];
        if constexpr (PLAIN_RULE)
            acc32 = __fadd_rn(acc32, e);
        else
            acc64 = __dadd_rn(acc64, (double)e);
    }
    const float d = PLAIN_RULE ? acc32 : (float)acc64;
    return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)id;
}

// Whether the filter lets the entry of reported id `id` pass: the id back to its local node (the even-N renaming undone,
// id_base subtracted), then that node's bit.  A list holds ids of the handle's own nodes only; the range test keeps a
// foreign id from reading past the bitmap all the same.
__device__ __forceinline__ bool ivf_eligible(const IvfFilter& f, int32_t id) {
    const int64_t pos = (f.even && (int64_t)id == f.N) ? f.N - 1 : (int64_t)id;
    const int64_t l = pos - f.base;
    if (l < 0 || l >= f.n_local) return false;
    return (f.bits[l >> 5] >> (l & 31)) & 1u;
}

}  // namespace dpq
