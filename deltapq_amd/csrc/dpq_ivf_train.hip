// dpq_ivf_train.hip -- training a coarse quantiser on gfx950: the nearest centroid of every row, and the
// update, repair and distortion of a Lloyd round.  The distance is the exact search's (dpq_flat.hip): per dimension, in
// ascending order, t = c[d] - v[d] and s = t * t in fp32, each rounded on its own (the build passes -ffp-contract=off),
// then acc += (double)s on an fp64 accumulator that starts at +0.0; the distance is (float)acc.
//
//   ivf_argmin_kernel
//                      flat_dist_kernel's fp32 L2 body with a running minimum where its key sink stands.  A workgroup of
//                      256 owns 64 rows and walks every tile of 64 centroids; both tiles go through LDS in slices of 32
//                      dimensions, transposed, read back as 16-byte LDS loads; thread (tx, ty) owns rows ty*4.. x centroids
//                      tx*4.. on 16 fp64 accumulators, one lane one distance from the first dimension to the last.  No
//                      matrix instruction: their accumulation order is not the contract's.  After a tile's last slice a
//                      lane folds its keys `distance bits << 32 | list` into four running minima, one per row: min on the
//                      key is the tie rule.  After the last tile the 16 lanes of a row, neighbours in one wavefront,
//                      reduce by lane exchange; lane tx = 0 writes the label and the distance and counts a changed
//                      label, one integer atomic per wavefront.  The row tile is staged again for every centroid tile: a
//                      variant that kept it in LDS across the tiles measured within 1 % of this one at 16 to 160
//                      dimensions (the loop is bound by its fp64 adds and conversions), so there is one
//                      kernel with 17 KB of static LDS for every D.
//   ivf_means_kernel   a workgroup per list, a thread per dimension: the members' values in list order, eight loads ahead
//                      of eight dependent fp64 adds -- one add after the other is the contract, so no tree.
//   ivf_dist_leaf_kernel, ivf_round_stats_kernel
//                      the distortion as a fixed reduction: a workgroup per leaf of 1024 distances (a thread's four in
//                      ascending order, then a tree over the 256 threads), then one workgroup over the leaves' sums in the
//                      same shape; it also counts the empty lists.  No floating-point atomics.
//   ivf_repair_keys_kernel, ivf_repair_copy_kernel
//                      ~bits(winning distance) << 32 | row for hipCUB's sort; the first E ranked rows into the empty lists.
#include "dpq_ivf_train.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "dpq_flat.h"

namespace dpq {
namespace {

constexpr int TR = kIvfArgminRows, TC = 64;  // rows and centroids of a workgroup's tile
constexpr int DC = 32;                       // dimensions staged at a time
constexpr int LD = TC + 4;                   // LDS row stride in floats (16-byte aligned; spreads the transposed writes)
static_assert(TR == 64 && TC == 64, "thread (tx, ty) owns 4 x 4 of a 64 x 64 tile");

// grid (tiles of 64 rows), 256 threads.  Rows past n and centroids past nlist are staged as zeros and masked: a centroid
// past nlist never enters a minimum, a row past n is never written.  nlist >= 1, so every row of the tile ends with a key.
__global__ __launch_bounds__(256) void ivf_argmin_kernel(const float* __restrict__ rows, int64_t n, int Dp,
                                                         const float* __restrict__ cent, int nlist, const int32_t* prev,
                                                         int32_t* labels, float* __restrict__ win, uint32_t* changed) {
    __shared__ float qs[DC][LD];
    __shared__ float vs[DC][LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int sr = tid >> 3, sj = (tid & 7) * 4;  // staging: tile entry sr (and sr + 32), dimensions sj .. sj + 3 of a slice
    const int64_t r0 = (int64_t)blockIdx.x * TR;

    uint64_t best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    for (int c0 = 0; c0 < nlist; c0 += TC) {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int d0 = 0; d0 < Dp; d0 += DC) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = sr + 32 * h, d = d0 + sj;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f), q = v;  // both loads ahead of both sets of LDS writes
                if (c0 + r < nlist && d < Dp) v = *reinterpret_cast<const float4*>(cent + (size_t)(c0 + r) * Dp + d);
                if (r0 + r < n && d < Dp) q = *reinterpret_cast<const float4*>(rows + (size_t)(r0 + r) * Dp + d);
                vs[sj + 0][r] = v.x; vs[sj + 1][r] = v.y; vs[sj + 2][r] = v.z; vs[sj + 3][r] = v.w;
                qs[sj + 0][r] = q.x; qs[sj + 1][r] = q.y; qs[sj + 2][r] = q.z; qs[sj + 3][r] = q.w;
            }
            __syncthreads();
            const int dc = min(DC, Dp - d0);
#pragma unroll 4
            for (int d = 0; d < dc; ++d) {
                const float4 q4 = *reinterpret_cast<const float4*>(&qs[d][ty * 4]);
                const float4 v4 = *reinterpret_cast<const float4*>(&vs[d][tx * 4]);
                const float qa[4] = {q4.x, q4.y, q4.z, q4.w}, va[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) accumulate<kFlatL2>(acc[i][j], va[j], qa[i]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int list = c0 + tx * 4 + j;
                const uint64_t key = make_key<kFlatL2>(acc[i][j], (uint32_t)list);
                if (list < nlist && key < best[i]) best[i] = key;
            }
    }

    // the 16 lanes of a row are lanes ty*16 .. ty*16 + 15 of the workgroup: neighbours in one wavefront
    uint32_t moved = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint64_t k = best[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)k, o), hi = __shfl_xor((uint32_t)(k >> 32), o);
            const uint64_t other = ((uint64_t)hi << 32) | lo;
            if (other < k) k = other;
        }
        const int64_t row = r0 + ty * 4 + i;
        if (tx == 0 && row < n) {
            const int32_t label = (int32_t)(uint32_t)k;
            if (prev && prev[row] != label) ++moved;  // prev may be labels: read before the write below, by the same lane
            labels[row] = label;
            if (win) win[row] = __uint_as_float((uint32_t)(k >> 32));
        }
    }
    if (changed) {  // uniform
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) moved += __shfl_xor(moved, o);
        if ((tid & 63) == 0 && moved) atomicAdd(changed, moved);
    }
}

__global__ __launch_bounds__(256) void ivf_means_kernel(const float* __restrict__ rows, int Dp,
                                                        const uint32_t* __restrict__ members,
                                                        const int64_t* __restrict__ offsets, float* __restrict__ cent) {
    const int l = blockIdx.x;
    const int64_t b = offsets[l], e = offsets[l + 1];
    if (b >= e) return;
    const double count = (double)(e - b);
    for (int d = threadIdx.x; d < Dp; d += blockDim.x) {
        double s = 0.0;
        int64_t i = b;
        for (; i + 8 <= e; i += 8) {
            float x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = rows[(size_t)members[i + k] * Dp + d];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += (double)x[k];
        }
        for (; i < e; ++i) s += (double)rows[(size_t)members[i] * Dp + d];
        cent[(size_t)l * Dp + d] = (float)(s / count);
    }
}

// The sum of the 256 threads' values in a fixed tree; valid in thread 0.  buf: 256 doubles of LDS.
__device__ __forceinline__ double block_sum_256(double v, double* buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) buf[threadIdx.x] = buf[threadIdx.x] + buf[threadIdx.x + o];
        __syncthreads();
    }
    return buf[0];
}

__global__ __launch_bounds__(256) void ivf_dist_leaf_kernel(const float* __restrict__ win, int64_t n, double* __restrict__ partial) {
    __shared__ double buf[256];
    const int64_t base = (int64_t)blockIdx.x * kIvfDistLeaf;
    double s = 0.0;
    for (int k = 0; k < kIvfDistLeaf / 256; ++k) {
        const int64_t i = base + threadIdx.x + 256 * k;
        if (i < n) s += (double)win[i];
    }
    s = block_sum_256(s, buf);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void ivf_round_stats_kernel(const double* __restrict__ partial, int64_t n_partial,
                                                              const unsigned long long* __restrict__ counts, int nlist,
                                                              IvfRoundStats* out) {
    __shared__ double buf[256];
    __shared__ uint32_t empties;
    if (threadIdx.x == 0) empties = 0;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_partial; i += 256) s += partial[i];
    s = block_sum_256(s, buf);  // its first barrier publishes `empties`
    uint32_t e = 0;
    for (int l = threadIdx.x; l < nlist; l += 256) e += counts[l] == 0 ? 1u : 0u;
    if (e) atomicAdd(&empties, e);
    __syncthreads();
    if (threadIdx.x == 0) {
        out->distortion = s;
        out->n_empty = empties;
    }
}

__global__ __launch_bounds__(256) void ivf_repair_keys_kernel(const float* __restrict__ win, int64_t n, uint64_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = ((uint64_t)(~__float_as_uint(win[i])) << 32) | (uint32_t)i;
}

// grid (E): the j-th empty list takes the j-th ranked row
__global__ __launch_bounds__(256) void ivf_repair_copy_kernel(const uint64_t* __restrict__ sorted, const int32_t* __restrict__ empty,
                                                              const float* __restrict__ rows, int Dp, float* __restrict__ cent) {
    const uint32_t row = (uint32_t)sorted[blockIdx.x];
    const int l = empty[blockIdx.x];
    for (int d = threadIdx.x; d < Dp; d += blockDim.x) cent[(size_t)l * Dp + d] = rows[(size_t)row * Dp + d];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_ivf_argmin(const float* d_rows, int64_t n, int Dp, const float* d_cent, int nlist, const int32_t* d_prev,
                             int32_t* d_labels, float* d_win, uint32_t* d_changed, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_rows || !d_cent || !d_labels || n > 0x7fffffff || Dp < 4 || Dp % 4 != 0 || Dp > kFlatMaxD || nlist < 1 ||
        nlist > 65536 || !aligned16(d_rows) || !aligned16(d_cent))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + TR - 1) / TR));
    ivf_argmin_kernel<<<grid, dim3(256), 0, stream>>>(d_rows, n, Dp, d_cent, nlist, d_prev, d_labels, d_win, d_changed);
    return hipGetLastError();
}

hipError_t launch_ivf_means(const float* d_rows, int Dp, const uint32_t* d_members, const int64_t* d_offsets, int nlist,
                            float* d_cent, hipStream_t stream) {
    if (!d_rows || !d_members || !d_offsets || !d_cent || Dp < 1 || nlist < 1 || nlist > 65536) return hipErrorInvalidValue;
    const int threads = std::min(256, (Dp + 63) / 64 * 64);
    ivf_means_kernel<<<dim3(nlist), dim3(threads), 0, stream>>>(d_rows, Dp, d_members, d_offsets, d_cent);
    return hipGetLastError();
}

hipError_t launch_ivf_round_stats(const float* d_win, int64_t n, const unsigned long long* d_counts, int nlist,
                                  double* d_partial, IvfRoundStats* d_out, hipStream_t stream) {
    if (!d_win || !d_counts || !d_partial || !d_out || n < 1 || n > 0x7fffffff || nlist < 1) return hipErrorInvalidValue;
    const size_t leaves = ivf_dist_partials(n);
    ivf_dist_leaf_kernel<<<dim3((unsigned)leaves), dim3(256), 0, stream>>>(d_win, n, d_partial);
    ivf_round_stats_kernel<<<dim3(1), dim3(256), 0, stream>>>(d_partial, (int64_t)leaves, d_counts, nlist, d_out);
    return hipGetLastError();
}

hipError_t ivf_train_repair(void* d_temp, size_t* temp_bytes, const float* d_win, int64_t n, uint64_t* d_keys,
                            uint64_t* d_sorted, const int32_t* d_empty, int E, const float* d_rows, int Dp, float* d_cent,
                            hipStream_t stream) {
    if (n < 1 || n > 0x7fffffff) return hipErrorInvalidValue;
    size_t need = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, need, d_keys, d_sorted, (int)n, 0, 64, stream);
    if (e != hipSuccess) return e;
    if (!d_temp) {
        *temp_bytes = need;
        return hipSuccess;
    }
    if (*temp_bytes < need || !d_win || !d_keys || !d_sorted || !d_empty || !d_rows || !d_cent || E < 1 || E > n || Dp < 1)
        return hipErrorInvalidValue;
    ivf_repair_keys_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(d_win, n, d_keys);
    size_t tb = *temp_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(d_temp, tb, d_keys, d_sorted, (int)n, 0, 64, stream);
    if (e != hipSuccess) return e;
    const int threads = std::min(256, (Dp + 63) / 64 * 64);
    ivf_repair_copy_kernel<<<dim3(E), dim3(threads), 0, stream>>>(d_sorted, d_empty, d_rows, Dp, d_cent);
    return hipGetLastError();
}

}  // namespace dpq
