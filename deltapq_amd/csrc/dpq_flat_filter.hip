// dpq_flat_filter.hip -- what filtered and range search over raw vectors need besides distances, on gfx950
// (DESIGN.md 5.10.2): the row list of a filter, the state a range pass starts from, and the sort of its lists.
// The distances themselves are flat_dist_kernel<LIST, MODE> (dpq_flat.hip) and flat_dist_u8_kernel<LIST, MODE>
// (dpq_flat_u8.hip), the same kernels the unfiltered search runs; no distance code lives here.
//
// A filter is an ascending list of the eligible rows of a handle.
//
//   flat_filter_count_kernel   popcount of every 32-row word of the handle's slice of the bitmap
//   (hipcub ExclusiveSum)      where each word's rows start in the list; the total is n_allowed
//   flat_filter_emit_kernel    a thread per word writes its set bits as row numbers, each position checked against the
//                              list's capacity
//   flat_range_state_kernel    per query: count = overflow = 0, threshold = its radius key
//   (hipcub segmented radix sort) every list of the pool by key = (distance, id)
// No kernel waits for another workgroup.
#include "dpq_flat.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace dpq {
namespace {

__global__ void flat_filter_count_kernel(const uint32_t* __restrict__ words, int64_t n_words, uint32_t* __restrict__ cnt) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n_words) cnt[w] = (uint32_t)__popc(words[w]);
}

__global__ void flat_filter_emit_kernel(const uint32_t* __restrict__ words, int64_t n_words,
                                        const uint32_t* __restrict__ off, uint32_t* __restrict__ list, int64_t cap,
                                        uint32_t* flag) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint32_t bits = words[w];
    int64_t o = off[w];
    while (bits) {
        const int b = __ffs((int)bits) - 1;
        bits &= bits - 1;
        if (o < cap)
            list[o] = (uint32_t)(w * 32 + b);
        else
            *flag = 1;
        ++o;
    }
}

// count = 0, overflow = 0, thr = the radius key of the query
__global__ void flat_range_state_kernel(FlatQueryState* state, const uint64_t* __restrict__ thr, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) {
        state[q].count = 0;
        state[q].overflow = 0;
        state[q].thr = thr[q];
    }
}

}  // namespace

hipError_t flat_filter_count(const uint32_t* d_words, int64_t n_words, uint32_t* d_cnt, uint32_t* d_off, int64_t* n_allowed,
                             hipStream_t stream) {
    *n_allowed = 0;
    if (n_words <= 0) return hipSuccess;
    flat_filter_count_kernel<<<dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream>>>(d_words, n_words, d_cnt);
    size_t tb = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_cnt, d_off, (int)n_words, stream);
    if (e != hipSuccess) return e;
    void* d_temp = nullptr;
    if ((e = hipMalloc(&d_temp, std::max<size_t>(tb, 1))) != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(d_temp, tb, d_cnt, d_off, (int)n_words, stream);
    uint32_t last[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&last[0], d_off + n_words - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], d_cnt + n_words - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    hipFree(d_temp);
    *n_allowed = (int64_t)last[0] + last[1];
    return e;
}

hipError_t launch_flat_filter_emit(const uint32_t* d_words, int64_t n_words, const uint32_t* d_off, uint32_t* d_list,
                                   int64_t cap, uint32_t* d_flag, hipStream_t stream) {
    if (n_words <= 0) return hipSuccess;
    flat_filter_emit_kernel<<<dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream>>>(d_words, n_words, d_off, d_list,
                                                                                               cap, d_flag);
    return hipGetLastError();
}

hipError_t launch_flat_range_state(FlatQueryState* d_state, const uint64_t* d_thr, int nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    flat_range_state_kernel<<<dim3((nq + 255) / 256), dim3(256), 0, stream>>>(d_state, d_thr, nq);
    return hipGetLastError();
}

hipError_t flat_range_sort(void* d_temp, size_t* temp_bytes, const uint64_t* d_in, uint64_t* d_out, int64_t n_keys,
                           int n_lists, const int64_t* d_offs, hipStream_t stream) {
    return hipcub::DeviceSegmentedRadixSort::SortKeys(d_temp, *temp_bytes, d_in, d_out, (int)n_keys, n_lists, d_offs,
                                                      d_offs + 1, 0, 64, stream);
}

}  // namespace dpq
