// dpq_flat_filter.hip -- exact search over the rows an id bitmap allows, and exact range search, on gfx950
// (DESIGN.md 5.10.2).  The kernels of dpq_flat.hip / dpq_flat_u8.hip stay as they are; these sit beside them.
//
// A filter is an ascending list of the eligible rows of a handle.  The distance kernels below are the two of the
// unfiltered search with one change: the 64 (fp32) or 256 (byte) vectors of a workgroup's tile are list entries
// l0 + v0 .. instead of rows row0 + v0 ..; their row numbers go through LDS once per tile.  The per-lane arithmetic and
// its order are flat_dist_kernel's and flat_dist_u8_kernel's, so the distance bits are too.  Without a list (a range
// search over all rows) entry e is row e.
//
//   flat_filter_count_kernel   popcount of every 32-row word of the handle's slice of the bitmap
//   (hipcub ExclusiveSum)      where each word's rows start in the list; the total is n_allowed
//   flat_filter_emit_kernel    a thread per word writes its set bits as row numbers
//   flat_dist_sel_kernel       fp32 distances; MODE says what becomes of a key:
//   flat_dist_sel_u8_kernel    the same on the int8 matrix cores
//       kTopK    key <= threshold: appended to the query's buffer (flat_dist_kernel's threshold / counter protocol;
//                selection and the final sort are dpq_flat.hip's kernels, which pad short lists with -1 / +inf)
//       kCount   key <  radius key: counted
//       kEmit    key <  radius key: appended to the query's list in the pool, whose length the count pass gave
//   (hipcub segmented radix sort) every list of the pool by key = (distance, id)
// No kernel waits for another workgroup.  Every append checks its position against the capacity of its buffer and
// raises FlatQueryState::overflow instead of storing outside it.
#include "dpq_flat.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace dpq {
namespace {

constexpr int TQ = 64, TV = 64;  // flat_dist_kernel's tile
constexpr int DC = 32;
constexpr int LD = TV + 4;
constexpr int UQ = 64, UV = 256;  // flat_dist_u8_kernel's tile
constexpr int KS = 32;

enum { kTopK = 0, kCount = 1, kEmit = 2 };

static_assert(KS == kFlatU8KStep, "rows are padded to the K step of the MFMA");

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

__device__ __forceinline__ uint64_t make_key(double acc, uint32_t id) {
    return ((uint64_t)__float_as_uint((float)acc) << 32) | id;
}

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

// Where the keys of query q go and how many fit.
template <int MODE>
__device__ __forceinline__ uint64_t* sink_of(uint64_t* keys, int cap, const int64_t* offs, int q, uint32_t* room) {
    if (MODE == kEmit) {
        *room = (uint32_t)(offs[q + 1] - offs[q]);
        return keys + offs[q];
    }
    *room = (uint32_t)cap;
    return keys + (size_t)q * cap;
}

// grid (tiles of the stripe's `rows` entries, query tiles), 256 threads: thread (tx, ty) owns queries ty*4.. x entries
// tx*4..; entry e of the stripe is row list[l0 + e] (LIST) or row l0 + e.
template <bool LIST, int MODE>
__global__ __launch_bounds__(256) void flat_dist_sel_kernel(const float* __restrict__ base, const uint32_t* __restrict__ list,
                                                            int64_t l0, int rows, int Dp, const float* __restrict__ queries,
                                                            int nq, int64_t id_offset, uint64_t* __restrict__ keys, int cap,
                                                            const int64_t* __restrict__ offs, FlatQueryState* state) {
    __shared__ float qs[DC][LD];
    __shared__ float vs[DC][LD];
    __shared__ uint32_t lrow[TV];
    __shared__ uint32_t cnt[TQ];
    __shared__ uint32_t pos0[TQ];
    __shared__ uint64_t thr[TQ];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int v0 = blockIdx.x * TV, q0 = blockIdx.y * TQ;
    const int sr = tid >> 3, sj = (tid & 7) * 4;
    if (tid < TV) {
        uint32_t row = 0;  // entries past the stripe read row 0 and are masked below
        if (v0 + tid < rows) row = LIST ? list[l0 + v0 + tid] : (uint32_t)(l0 + v0 + tid);
        lrow[tid] = row;
    }
    __syncthreads();

    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

    for (int d0 = 0; d0 < Dp; d0 += DC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = sr + 32 * h, d = d0 + sj;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), q = v;
            if (v0 + r < rows && d < Dp) v = *reinterpret_cast<const float4*>(base + (size_t)lrow[r] * Dp + d);
            if (q0 + r < nq && d < Dp) q = *reinterpret_cast<const float4*>(queries + (size_t)(q0 + r) * Dp + d);
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
                for (int j = 0; j < 4; ++j) {
                    const float t = va[j] - qa[i];
                    const float s = t * t;
                    acc[i][j] += (double)s;
                }
        }
        __syncthreads();
    }

    if (tid < TQ) {
        cnt[tid] = 0;
        thr[tid] = q0 + tid < nq ? state[q0 + tid].thr : 0;
    }
    __syncthreads();
    uint64_t key[4][4];
    uint32_t slot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ql = ty * 4 + i, vl = tx * 4 + j;
            key[i][j] = make_key(acc[i][j], (uint32_t)(id_offset + lrow[vl]));
            const bool below = MODE == kTopK ? key[i][j] <= thr[ql] : key[i][j] < thr[ql];
            const bool pass = q0 + ql < nq && v0 + vl < rows && below;
            slot[i][j] = pass ? atomicAdd(&cnt[ql], 1u) : 0xffffffffu;
        }
    __syncthreads();
    if (tid < TQ && cnt[tid]) pos0[tid] = atomicAdd(&state[q0 + tid].count, cnt[tid]);
    if (MODE == kCount) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (slot[i][j] == 0xffffffffu) continue;
            const int ql = ty * 4 + i;
            const uint32_t pos = pos0[ql] + slot[i][j];
            uint32_t room;
            uint64_t* out = sink_of<MODE>(keys, cap, offs, q0 + ql, &room);
            if (pos < room)
                out[pos] = key[i][j];
            else
                state[q0 + ql].overflow = 1;
        }
}

// flat_dist_u8_kernel over stripe entries: wavefront w owns entries 64 w .. 64 w + 63 of the workgroup's 256 and all 64
// queries; the accumulator layout is the one described there.
template <bool LIST, int MODE>
__global__ __launch_bounds__(256) void flat_dist_sel_u8_kernel(const int8_t* __restrict__ base,
                                                               const int32_t* __restrict__ vnorm,
                                                               const uint32_t* __restrict__ list, int64_t l0, int rows, int Dp,
                                                               const int8_t* __restrict__ queries,
                                                               const int32_t* __restrict__ qnorm, int nq, int64_t id_offset,
                                                               uint64_t* __restrict__ keys, int cap,
                                                               const int64_t* __restrict__ offs, FlatQueryState* state) {
    __shared__ uint32_t lrow[UV];
    __shared__ uint32_t cnt[UQ];
    __shared__ uint32_t pos0[UQ];
    __shared__ uint64_t thr[UQ];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int b0 = blockIdx.x * UV, lv0 = w * 64, q0 = blockIdx.y * UQ;  // lv0: the wavefront's first entry in the tile
    {
        uint32_t row = 0;  // entries past the stripe read row 0 and are masked below
        if (b0 + tid < rows) row = LIST ? list[l0 + b0 + tid] : (uint32_t)(l0 + b0 + tid);
        lrow[tid] = row;
    }
    if (tid < UQ) {
        cnt[tid] = 0;
        thr[tid] = q0 + tid < nq ? state[q0 + tid].thr : 0;
    }
    __syncthreads();

    const int8_t* ap[2];
    const int8_t* bp[2];
    bool aok[2], bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int lv = lv0 + 32 * i + r, q = q0 + 32 * i + r;
        aok[i] = b0 + lv < rows;
        bok[i] = q < nq;
        ap[i] = base + (size_t)lrow[lv] * Dp + 16 * h;
        bp[i] = queries + (size_t)(bok[i] ? q : 0) * Dp + 16 * h;
    }
    i32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;

    const i32x4 zero = {0, 0, 0, 0};
    for (int k0 = 0; k0 < Dp; k0 += KS) {
        i32x4 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = aok[i] ? *reinterpret_cast<const i32x4*>(ap[i] + k0) : zero;
            b[i] = bok[i] ? *reinterpret_cast<const i32x4*>(bp[i] + k0) : zero;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }

    // dot products -> the fp32 bit patterns of the distances, in place (flat_dist_u8_kernel's epilogue, the norm of
    // every entry fetched by its row number)
    uint32_t thi[2], tlo[2];
    bool qok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ql = 32 * j + r;
        qok[j] = q0 + ql < nq;
        thi[j] = (uint32_t)(thr[ql] >> 32);
        tlo[j] = (uint32_t)thr[ql];
        const int qn = qok[j] ? qnorm[q0 + ql] : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int lv = lv0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                const int vn = vnorm[lrow[lv]];
                acc[i][j][e] = __float_as_int(__int2float_rn(vn + qn - 2 * acc[i][j][e]));
            }
    }
    const uint32_t id0 = (uint32_t)id_offset;
    auto passes = [&](int i, int j, int e, int lv) {
        const uint32_t b = (uint32_t)acc[i][j][e];
        if (b0 + lv >= rows) return false;
        if (MODE != kTopK) return b < thi[j];  // the radius key's id half is zero
        return b < thi[j] || (b == thi[j] && id0 + lrow[lv] <= tlo[j]);
    };

    uint32_t run[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t np = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) np += passes(i, j, e, lv0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h);
        if (!qok[j]) np = 0;
        run[j] = np ? atomicAdd(&cnt[32 * j + r], np) : 0u;
    }
    __syncthreads();
    if (tid < UQ && cnt[tid]) pos0[tid] = atomicAdd(&state[q0 + tid].count, cnt[tid]);
    if (MODE == kCount) return;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ql = 32 * j + r;
        if (!qok[j] || !cnt[ql]) continue;
        uint32_t pos = pos0[ql] + run[j];
        uint32_t room;
        uint64_t* out = sink_of<MODE>(keys, cap, offs, q0 + ql, &room);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int lv = lv0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (passes(i, j, e, lv)) {
                    if (pos < room)
                        out[pos] = ((uint64_t)(uint32_t)acc[i][j][e] << 32) | (id0 + lrow[lv]);
                    else
                        state[q0 + ql].overflow = 1;
                    ++pos;
                }
            }
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

template <int MODE>
void dist_fp32(const float* base, const uint32_t* list, int64_t l0, int rows, int Dp, const float* q, int nq,
               int64_t id_offset, uint64_t* keys, int cap, const int64_t* offs, FlatQueryState* state, hipStream_t stream) {
    const dim3 grid((rows + TV - 1) / TV, (nq + TQ - 1) / TQ), block(256);
    if (list)
        flat_dist_sel_kernel<true, MODE><<<grid, block, 0, stream>>>(base, list, l0, rows, Dp, q, nq, id_offset, keys, cap, offs, state);
    else
        flat_dist_sel_kernel<false, MODE><<<grid, block, 0, stream>>>(base, list, l0, rows, Dp, q, nq, id_offset, keys, cap, offs, state);
}

template <int MODE>
void dist_u8(const int8_t* base, const int32_t* vnorm, const uint32_t* list, int64_t l0, int rows, int Dp, const int8_t* q,
             const int32_t* qnorm, int nq, int64_t id_offset, uint64_t* keys, int cap, const int64_t* offs,
             FlatQueryState* state, hipStream_t stream) {
    const dim3 grid((rows + UV - 1) / UV, (nq + UQ - 1) / UQ), block(256);
    if (list)
        flat_dist_sel_u8_kernel<true, MODE><<<grid, block, 0, stream>>>(base, vnorm, list, l0, rows, Dp, q, qnorm, nq, id_offset, keys, cap, offs, state);
    else
        flat_dist_sel_u8_kernel<false, MODE><<<grid, block, 0, stream>>>(base, vnorm, list, l0, rows, Dp, q, qnorm, nq, id_offset, keys, cap, offs, state);
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

hipError_t launch_flat_search_list(const float* d_base, const uint32_t* d_list, int64_t n_list, int Dp, const float* d_queries,
                                   int nq, int top_k, int64_t id_offset, uint64_t* d_keys, FlatQueryState* d_state,
                                   int32_t* d_ids, float* d_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    // launch_flat_search's stripes, limit and selection, a stripe being cap / 2 list entries
    const int cap = flat_key_capacity(top_k);
    const int64_t stripe = cap / 2;
    const uint32_t limit = (uint32_t)std::max(top_k, cap / 4);
    hipError_t e = launch_flat_init_state(d_state, nq, stream);
    if (e != hipSuccess) return e;
    for (int64_t l0 = 0; l0 < n_list; l0 += stripe) {
        const int rows = (int)std::min<int64_t>(stripe, n_list - l0);
        if (l0 > 0 && (e = launch_flat_select(d_keys, cap, d_state, nq, top_k, limit, stream)) != hipSuccess) return e;
        dist_fp32<kTopK>(d_base, d_list, l0, rows, Dp, d_queries, nq, id_offset, d_keys, cap, nullptr, d_state, stream);
    }
    if ((e = launch_flat_select(d_keys, cap, d_state, nq, top_k, (uint32_t)top_k, stream)) != hipSuccess) return e;
    return launch_flat_sort_emit(d_keys, (size_t)cap, d_state, nq, top_k, top_k, d_ids, d_dists, stream);
}

hipError_t launch_flat_search_list_u8(const int8_t* d_base, const int32_t* d_vnorm, const uint32_t* d_list, int64_t n_list,
                                      int Dp, const int8_t* d_queries, const int32_t* d_qnorm, int nq, int top_k,
                                      int64_t id_offset, uint64_t* d_keys, FlatQueryState* d_state, int32_t* d_ids,
                                      float* d_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int cap = flat_key_capacity(top_k);
    const int64_t stripe = cap / 2;
    const uint32_t limit = (uint32_t)std::max(top_k, cap / 4);
    hipError_t e = launch_flat_init_state(d_state, nq, stream);
    if (e != hipSuccess) return e;
    for (int64_t l0 = 0; l0 < n_list; l0 += stripe) {
        const int rows = (int)std::min<int64_t>(stripe, n_list - l0);
        if (l0 > 0 && (e = launch_flat_select(d_keys, cap, d_state, nq, top_k, limit, stream)) != hipSuccess) return e;
        dist_u8<kTopK>(d_base, d_vnorm, d_list, l0, rows, Dp, d_queries, d_qnorm, nq, id_offset, d_keys, cap, nullptr, d_state,
                       stream);
    }
    if ((e = launch_flat_select(d_keys, cap, d_state, nq, top_k, (uint32_t)top_k, stream)) != hipSuccess) return e;
    return launch_flat_sort_emit(d_keys, (size_t)cap, d_state, nq, top_k, top_k, d_ids, d_dists, stream);
}

hipError_t launch_flat_range_state(FlatQueryState* d_state, const uint64_t* d_thr, int nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    flat_range_state_kernel<<<dim3((nq + 255) / 256), dim3(256), 0, stream>>>(d_state, d_thr, nq);
    return hipGetLastError();
}

hipError_t launch_flat_range_pass(const float* d_base, const uint32_t* d_list, int64_t n_entries, int Dp,
                                  const float* d_queries, int nq, int64_t id_offset, uint64_t* d_pool, const int64_t* d_offs,
                                  FlatQueryState* d_state, hipStream_t stream) {
    if (nq <= 0 || n_entries <= 0) return hipSuccess;
    if (d_pool)
        dist_fp32<kEmit>(d_base, d_list, 0, (int)n_entries, Dp, d_queries, nq, id_offset, d_pool, 0, d_offs, d_state, stream);
    else
        dist_fp32<kCount>(d_base, d_list, 0, (int)n_entries, Dp, d_queries, nq, id_offset, nullptr, 0, nullptr, d_state, stream);
    return hipGetLastError();
}

hipError_t launch_flat_range_pass_u8(const int8_t* d_base, const int32_t* d_vnorm, const uint32_t* d_list, int64_t n_entries,
                                     int Dp, const int8_t* d_queries, const int32_t* d_qnorm, int nq, int64_t id_offset,
                                     uint64_t* d_pool, const int64_t* d_offs, FlatQueryState* d_state, hipStream_t stream) {
    if (nq <= 0 || n_entries <= 0) return hipSuccess;
    if (d_pool)
        dist_u8<kEmit>(d_base, d_vnorm, d_list, 0, (int)n_entries, Dp, d_queries, d_qnorm, nq, id_offset, d_pool, 0, d_offs,
                       d_state, stream);
    else
        dist_u8<kCount>(d_base, d_vnorm, d_list, 0, (int)n_entries, Dp, d_queries, d_qnorm, nq, id_offset, nullptr, 0, nullptr,
                        d_state, stream);
    return hipGetLastError();
}

hipError_t flat_range_sort(void* d_temp, size_t* temp_bytes, const uint64_t* d_in, uint64_t* d_out, int64_t n_keys,
                           int n_lists, const int64_t* d_offs, hipStream_t stream) {
    return hipcub::DeviceSegmentedRadixSort::SortKeys(d_temp, *temp_bytes, d_in, d_out, (int)n_keys, n_lists, d_offs,
                                                      d_offs + 1, 0, 64, stream);
}

}  // namespace dpq
