// dpq_filter.hip -- filter construction on the GPU (gfx950, wave64): a dpq_filter's bitmap from a bitmap over reported
// ids, an id list, an id range, a bitmap over original vector ids, or other filters; and two packing helpers.  See
// dpq_filter.h for the bitmap's layout and DESIGN.md 5.8.1 for what each path moves.
//
// Every kernel is a grid-stride loop over 64-bit indices whose trip count is the same for all threads of a workgroup
// (blocks are whole wavefronts and start at multiples of 256), so the ballots, the wavefront sums and the barrier below
// see every lane.  A build's popcount is summed per lane, once across the wavefront and once across the workgroup's
// four wavefronts, and added with one atomic per workgroup: atomics on the one count word serialise, and with one per
// wavefront (8192 of them) the vector-id build of 1 M nodes took 0.140 ms instead of 0.053.
#include "dpq_filter.h"

#include <algorithm>

namespace dpq {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxBlocks = 2048;  // 8 workgroups of 4 wavefronts per CU: enough to cover the memory latency
constexpr int64_t kMinPerThread = 4;  // items a thread takes before the grid grows: fewer workgroups, fewer atomics

inline int blocks_for(int64_t work) {
    const int64_t per_block = kThreads * kMinPerThread;
    return (int)std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (work + per_block - 1) / per_block));
}

__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t low_bits(int64_t k) {  // the k lowest bits set; k <= 0: none, k >= 32: all
    return k <= 0 ? 0u : k >= 32 ? 0xffffffffu : (1u << k) - 1u;
}

// Bits of word w that stand for nodes of the handle.
__device__ __forceinline__ uint32_t local_mask(const FilterGeom& g, int64_t w) { return low_bits(g.n_local - 32 * w); }

// Every thread of the workgroup calls it once, after its loop: the workgroup's sum goes to *count in one atomic.
__device__ __forceinline__ void block_add(unsigned long long* count, uint32_t c) {
    __shared__ uint32_t wave_sum[kThreads / 64];
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < kThreads / 64; ++i) total += wave_sum[i];
        if (total) atomicAdd(count, total);
    }
}

__device__ __forceinline__ uint32_t source_bit(const uint32_t* __restrict__ words, int64_t n_bits, int64_t r) {
    return r < n_bits ? (words[r >> 5] >> (r & 31)) & 1u : 0u;
}

// One thread per output word: a funnel shift of two source words by (base + 32 w) & 31.
__global__ __launch_bounds__(kThreads) void filter_reindex_kernel(const uint32_t* __restrict__ words, int64_t n_bits,
                                                                  FilterGeom g, uint32_t* __restrict__ bits,
                                                                  unsigned long long* count) {
    const int64_t user_words = (n_bits + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    uint32_t c = 0;
    for (int64_t w0 = (int64_t)blockIdx.x * kThreads; w0 < g.n_words; w0 += stride) {
        const int64_t w = w0 + threadIdx.x;
        if (w >= g.n_words) continue;
        uint32_t v = 0;
        const int64_t g0 = g.base + 32 * w;  // global position of local bit 32 w
        if (32 * w < g.n_local && g0 < n_bits) {
            const int64_t lo = g0 >> 5;
            const int sh = (int)(g0 & 31);
            const uint32_t a = words[lo];
            const uint32_t b = (sh && lo + 1 < user_words) ? words[lo + 1] : 0u;
            v = (uint32_t)((((uint64_t)b << 32) | a) >> sh);
            v &= low_bits(imin(n_bits - g0, g.n_local - 32 * w));
        }
        if (g.tail_l >= 0 && (g.tail_l >> 5) == w) {  // the even-N rule: source bit N governs position N - 1
            const int s = (int)(g.tail_l & 31);
            v = (v & ~(1u << s)) | (source_bit(words, n_bits, g.N) << s);
        }
        bits[w] = v;
        c += (uint32_t)__popc(v);
    }
    block_add(count, c);
}

// One thread per id, into cleared bits.
__global__ __launch_bounds__(kThreads) void filter_scatter_ids_kernel(const int32_t* __restrict__ ids, int64_t n,
                                                                      FilterGeom g, uint32_t* __restrict__ bits) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        int64_t pos = ids[i];
        if (pos < 0) continue;  // padding
        if (g.even) {           // the inverse of report_id
            if (pos == g.N)
                pos = g.N - 1;
            else if (pos == g.N - 1)
                continue;
        }
        const int64_t l = pos - g.base;
        if (l < 0 || l >= g.n_local) continue;  // a node of another handle
        atomicOr(&bits[l >> 5], 1u << (l & 31));
    }
}

// After the scatter: complement within n_local where asked, and count.
__global__ __launch_bounds__(kThreads) void filter_finish_kernel(FilterGeom g, int invert, uint32_t* __restrict__ bits,
                                                                 unsigned long long* count) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    uint32_t c = 0;
    for (int64_t w0 = (int64_t)blockIdx.x * kThreads; w0 < g.n_words; w0 += stride) {
        const int64_t w = w0 + threadIdx.x;
        if (w >= g.n_words) continue;
        uint32_t v = bits[w];
        if (invert) {
            v = ~v & local_mask(g, w);
            bits[w] = v;
        }
        c += (uint32_t)__popc(v);
    }
    block_add(count, c);
}

// Reported ids [lo, hi), 0 <= lo <= hi: local positions [lo - base, hi - base) cut to the handle, and the even-N node
// by whether N lies in the range.
__global__ __launch_bounds__(kThreads) void filter_range_kernel(int64_t lo, int64_t hi, FilterGeom g,
                                                                uint32_t* __restrict__ bits, unsigned long long* count) {
    const int64_t lo_l = imin(imax(lo - g.base, 0), g.n_local), hi_l = imin(imax(hi - g.base, 0), g.n_local);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    uint32_t c = 0;
    for (int64_t w0 = (int64_t)blockIdx.x * kThreads; w0 < g.n_words; w0 += stride) {
        const int64_t w = w0 + threadIdx.x;
        if (w >= g.n_words) continue;
        uint32_t v = low_bits(hi_l - 32 * w) & ~low_bits(lo_l - 32 * w);
        if (g.tail_l >= 0 && (g.tail_l >> 5) == w) {
            const int s = (int)(g.tail_l & 31);
            v = (v & ~(1u << s)) | ((lo <= g.N && g.N < hi ? 1u : 0u) << s);
        }
        bits[w] = v;
        c += (uint32_t)__popc(v);
    }
    block_add(count, c);
}

// One lane per local node: its vector id's bit of the source; a wavefront's ballot is two words of the filter.
__global__ __launch_bounds__(kThreads) void filter_gather_kernel(const uint32_t* __restrict__ words, int64_t n_bits,
                                                                 const uint32_t* __restrict__ vec_id, FilterGeom g,
                                                                 uint32_t* __restrict__ bits, unsigned long long* count) {
    const int64_t n_lanes = ((g.n_words + 1) >> 1) << 6;  // whole wavefronts over every word of the bitmap
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    uint32_t c = 0;  // (lane 0 of a wavefront counts for all its lanes)
    for (int64_t l0 = (int64_t)blockIdx.x * kThreads; l0 < n_lanes; l0 += stride) {
        const int64_t l = l0 + threadIdx.x;  // (n_lanes is a multiple of 64: a wavefront lies wholly inside it or outside)
        bool set = false;
        if (l < g.n_local) {
            const int64_t v = vec_id[l];
            set = v < n_bits && ((words[v >> 5] >> (v & 31)) & 1u);
        }
        const uint64_t b = __ballot(set);
        if ((threadIdx.x & 63) == 0 && l < n_lanes) {
            const int64_t w = l >> 5;
            bits[w] = (uint32_t)b;
            if (w + 1 < g.n_words) bits[w + 1] = (uint32_t)(b >> 32);
            c += (uint32_t)__popcll(b);
        }
    }
    block_add(count, c);
}

__global__ __launch_bounds__(kThreads) void filter_combine_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                                  int op, FilterGeom g, uint32_t* __restrict__ out,
                                                                  unsigned long long* count) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    uint32_t c = 0;
    for (int64_t w0 = (int64_t)blockIdx.x * kThreads; w0 < g.n_words; w0 += stride) {
        const int64_t w = w0 + threadIdx.x;
        if (w >= g.n_words) continue;
        const uint32_t x = a[w], y = op == kFilterNot ? 0u : b[w];
        uint32_t v;
        switch (op) {
            case kFilterAnd: v = x & y; break;
            case kFilterOr: v = x | y; break;
            case kFilterAndNot: v = x & ~y; break;
            case kFilterXor: v = x ^ y; break;
            default: v = ~x; break;
        }
        v &= local_mask(g, w);
        out[w] = v;
        c += (uint32_t)__popc(v);
    }
    block_add(count, c);
}

// One lane per byte of the mask; a wavefront's ballot is two words of the bitmap.
__global__ __launch_bounds__(kThreads) void bitmap_from_mask_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                                    uint32_t* __restrict__ words_out) {
    const int64_t n_words = (n + 31) >> 5, n_lanes = ((n_words + 1) >> 1) << 6;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i0 = (int64_t)blockIdx.x * kThreads; i0 < n_lanes; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        const uint64_t b = __ballot(i < n && mask[i] != 0);
        if ((threadIdx.x & 63) == 0 && i < n_lanes) {
            const int64_t w = i >> 5;
            words_out[w] = (uint32_t)b;
            if (w + 1 < n_words) words_out[w + 1] = (uint32_t)(b >> 32);
        }
    }
}

__global__ __launch_bounds__(kThreads) void bitmap_from_ids_kernel(const int32_t* __restrict__ ids, int64_t n, int64_t n_bits,
                                                                   uint32_t* __restrict__ words_out) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const int64_t id = ids[i];
        if (id < 0 || id >= n_bits) continue;
        atomicOr(&words_out[id >> 5], 1u << (id & 31));
    }
}

}  // namespace

hipError_t launch_filter_reindex(const uint32_t* words, int64_t n_bits, const FilterGeom& g, uint32_t* bits,
                                 unsigned long long* count, hipStream_t stream) {
    hipLaunchKernelGGL(filter_reindex_kernel, dim3(blocks_for(g.n_words)), dim3(kThreads), 0, stream, words, n_bits, g, bits,
                       count);
    return hipGetLastError();
}

hipError_t launch_filter_ids_build(const int32_t* ids, int64_t n, int invert, const FilterGeom& g, uint32_t* bits,
                                   unsigned long long* count, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(bits, 0, (size_t)g.n_words * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (n > 0) {
        hipLaunchKernelGGL(filter_scatter_ids_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, ids, n, g, bits);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(filter_finish_kernel, dim3(blocks_for(g.n_words)), dim3(kThreads), 0, stream, g, invert, bits, count);
    return hipGetLastError();
}

hipError_t launch_filter_range(int64_t lo, int64_t hi, const FilterGeom& g, uint32_t* bits, unsigned long long* count,
                               hipStream_t stream) {
    hipLaunchKernelGGL(filter_range_kernel, dim3(blocks_for(g.n_words)), dim3(kThreads), 0, stream, lo, hi, g, bits, count);
    return hipGetLastError();
}

hipError_t launch_filter_gather(const uint32_t* words, int64_t n_bits, const uint32_t* vec_id, const FilterGeom& g,
                                uint32_t* bits, unsigned long long* count, hipStream_t stream) {
    hipLaunchKernelGGL(filter_gather_kernel, dim3(blocks_for(g.n_words * 32)), dim3(kThreads), 0, stream, words, n_bits, vec_id,
                       g, bits, count);
    return hipGetLastError();
}

hipError_t launch_filter_combine(const uint32_t* a, const uint32_t* b, FilterOp op, const FilterGeom& g, uint32_t* out,
                                 unsigned long long* count, hipStream_t stream) {
    hipLaunchKernelGGL(filter_combine_kernel, dim3(blocks_for(g.n_words)), dim3(kThreads), 0, stream, a, b, (int)op, g, out,
                       count);
    return hipGetLastError();
}

hipError_t launch_bitmap_from_mask(const uint8_t* mask, int64_t n, uint32_t* words_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bitmap_from_mask_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, mask, n, words_out);
    return hipGetLastError();
}

hipError_t launch_bitmap_from_ids(const int32_t* ids, int64_t n, int64_t n_bits, uint32_t* words_out, hipStream_t stream) {
    if (n_bits <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(words_out, 0, (size_t)((n_bits + 31) >> 5) * sizeof(uint32_t), stream);
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(bitmap_from_ids_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, ids, n, n_bits, words_out);
    return hipGetLastError();
}

}  // namespace dpq
