// dpq_flat_half.hip -- exact L2 distances, or inner products, between fp32 queries and fp16 / bf16 base vectors on gfx950
// (DESIGN.md 5.10.4).
//
// A half base holds what the caller gave, 16 bits per value, at half the bytes of an fp32 base.  Widening a half to fp32
// is exact, so the contract needs no tolerance: every answer equals, bit for bit, the answer of the fp32 kernels
// (dpq_flat.hip) over the widened rows.  The kernels here get there by construction: they are the fp32 kernels with
// another staging step -- a lane loads 16 bytes, eight halves, widens them in registers and writes fp32 to LDS -- and the
// same inner loop (accumulate<METRIC>), key (make_key<METRIC>) and epilogue from there on.  bf16 widens with a shift,
// fp16 with v_cvt_f32_f16, which is exact and, under the build's 16-bit denormal mode, keeps subnormals.  No matrix
// instruction: the f16 / bf16 MFMAs accumulate in fp32 and in an order of their own, which the contract does not allow.
//
//   flat_dist_half_kernel<LIST, MODE, METRIC, FORMAT>   flat_dist_kernel's 64 x 64 tile, 32-dimension slices, 4 x 4 fp64
//                                                       accumulators per lane and epilogue
//   flat_rerank_half_kernel<METRIC, FORMAT>             flat_rerank_kernel with 16-byte gathers of eight halves per lane
//   flat_half_prepare_kernel, flat_half_narrow_kernel   pad 16-bit rows / narrow fp32 rows to padded 16-bit rows
#include "dpq_flat.h"

#include <algorithm>

namespace dpq {
namespace {

constexpr int TQ = 64, TV = 64;  // queries and vectors of a workgroup's tile
constexpr int DC = 32;           // dimensions staged at a time
constexpr int LD = TV + 4;       // LDS row stride in floats, as in dpq_flat.hip

// Eight halves as they lie in memory -> eight fp32 values.
template <int FORMAT>
__device__ __forceinline__ void widen8(const uint4& raw, float* out) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (FORMAT == kFlatBF16) {
            out[2 * i] = __uint_as_float(w[i] << 16);
            out[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        } else {
            union { uint16_t u; _Float16 h; } lo, hi;
            lo.u = (uint16_t)(w[i] & 0xffffu);
            hi.u = (uint16_t)(w[i] >> 16);
            out[2 * i] = (float)lo.h;
            out[2 * i + 1] = (float)hi.h;
        }
    }
}

// grid (tiles of the stripe's `rows` entries, query tiles), 256 threads: flat_dist_kernel (dpq_flat.hip) in every respect
// but the staging of the base tile.  The tile's 64 rows x 32 dimensions are 256 loads of 16 bytes, one per thread: thread
// t takes row vr = (t & 15) | (t >> 6) << 4 and dimensions vj = ((t >> 4) & 3) * 8 .. + 7 of the slice, so that the 32 lanes
// of a half wavefront write 16 consecutive rows of two slice rows that lie 8 * LD floats apart: two addresses per LDS
// bank of a ds_write_b32, which costs nothing extra.  The queries are fp32 and staged as there.
template <bool LIST, int MODE, int METRIC, int FORMAT>
__global__ __launch_bounds__(256) void flat_dist_half_kernel(const uint16_t* __restrict__ base,
                                                             const uint32_t* __restrict__ list, int64_t l0, int rows, int Dp,
                                                             const float* __restrict__ queries, int nq, int64_t id_offset,
                                                             uint64_t* __restrict__ keys, int cap,
                                                             const int64_t* __restrict__ offs, FlatQueryState* state) {
    __shared__ float qs[DC][LD];
    __shared__ float vs[DC][LD];
    __shared__ uint32_t lrow[TV];  // LIST only
    __shared__ uint32_t cnt[TQ];
    __shared__ uint32_t pos0[TQ];
    __shared__ uint64_t thr[TQ];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int v0 = blockIdx.x * TV, q0 = blockIdx.y * TQ;
    const int sr = tid >> 3, sj = (tid & 7) * 4;                           // queries: row sr (and sr + 32), four dimensions
    const int vr = (tid & 15) | ((tid >> 6) << 4), vj = ((tid >> 4) & 3) * 8;  // base: row vr, eight dimensions
    if constexpr (LIST) {
        if (tid < TV) lrow[tid] = v0 + tid < rows ? list[l0 + v0 + tid] : 0;  // past the stripe: row 0, masked below
        __syncthreads();
    }
    // the row of tile entry e; only called for, or masked to, e with v0 + e < rows
    auto row_of = [&](int e) -> int64_t {
        if constexpr (LIST) return lrow[e];
        else return l0 + (v0 + e);
    };

    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

    for (int d0 = 0; d0 < Dp; d0 += DC) {
        {
            uint4 raw = make_uint4(0u, 0u, 0u, 0u);  // the bits of eight zeros in either format
            if (v0 + vr < rows && d0 + vj < Dp) raw = *reinterpret_cast<const uint4*>(base + (size_t)row_of(vr) * Dp + d0 + vj);
            float v[8];
            widen8<FORMAT>(raw, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) vs[vj + k][vr] = v[k];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = sr + 32 * h, d = d0 + sj;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q0 + r < nq && d < Dp) q = *reinterpret_cast<const float4*>(queries + (size_t)(q0 + r) * Dp + d);
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
                for (int j = 0; j < 4; ++j) accumulate<METRIC>(acc[i][j], va[j], qa[i]);
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
            key[i][j] = make_key<METRIC>(acc[i][j], (uint32_t)(id_offset + row_of(vl)));
            const bool below = MODE == kFlatTopK ? key[i][j] <= thr[ql] : key[i][j] < thr[ql];
            const bool pass = q0 + ql < nq && v0 + vl < rows && below;
            slot[i][j] = pass ? atomicAdd(&cnt[ql], 1u) : 0xffffffffu;
        }
    __syncthreads();
    if (tid < TQ && cnt[tid]) pos0[tid] = atomicAdd(&state[q0 + tid].count, cnt[tid]);
    if (MODE == kFlatCount) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (slot[i][j] == 0xffffffffu) continue;
            const int ql = ty * 4 + i;
            const uint32_t pos = pos0[ql] + slot[i][j];
            uint32_t room;
            uint64_t* out = flat_sink_of<MODE>(keys, cap, offs, q0 + ql, &room);
            if (pos < room)
                out[pos] = key[i][j];
            else
                state[q0 + ql].overflow = 1;
        }
}

// grid (candidate groups of 256, queries), 256 threads: lane = candidate, as flat_rerank_kernel.  A wavefront fetches
// the 32-dimension slice of its 64 rows in four rounds of 16 rows, four lanes of 16 bytes per row.
template <int METRIC, int FORMAT>
__global__ __launch_bounds__(256) void flat_rerank_half_kernel(const uint16_t* __restrict__ base, int64_t n, int D, int Dp,
                                                               const float* __restrict__ queries,
                                                               const int32_t* __restrict__ cand, int n_cand, int n_pad,
                                                               int64_t id_offset, const uint32_t* __restrict__ map,
                                                               int64_t n_map, uint64_t* __restrict__ keys, uint32_t* flag) {
    __shared__ float qv[kFlatMaxD];
    __shared__ float tile[4][64][DC + 1];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int d = tid; d < Dp; d += 256) qv[d] = d < D ? queries[(size_t)q * D + d] : 0.0f;
    const int ci = blockIdx.x * 256 + tid;
    int row = -1;
    if (ci < n_cand) {
        const int32_t c = cand[(size_t)q * n_cand + ci];
        if (c >= 0) {  // a negative candidate is padding
            if (map) {
                int64_t p = c;
                if ((n_map & 1) == 0 && p == n_map) p = n_map - 1;  // the even-N id of the last DFS node
                if (p < n_map && (int64_t)map[p] < n) row = (int)map[p];
            } else {
                const int64_t r = (int64_t)c - id_offset;
                if (r >= 0 && r < n) row = (int)r;
            }
            if (row < 0) *flag = 1;  // names no row
        }
    }
    __syncthreads();
    double acc = 0.0;
    const int lj = (lane & 3) * 8;
    for (int d0 = 0; d0 < Dp; d0 += DC) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int cc = it * 16 + (lane >> 2);
            const int rr = __shfl(row, cc);
            uint4 raw = make_uint4(0u, 0u, 0u, 0u);
            if (rr >= 0 && d0 + lj < Dp) raw = *reinterpret_cast<const uint4*>(base + (size_t)rr * Dp + d0 + lj);
            float v[8];
            widen8<FORMAT>(raw, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) tile[w][cc][lj + k] = v[k];
        }
        __syncthreads();
        const int dc = min(DC, Dp - d0);
#pragma unroll 8
        for (int d = 0; d < dc; ++d) accumulate<METRIC>(acc, tile[w][lane][d], qv[d0 + d]);
        __syncthreads();
    }
    if (ci < n_pad)
        keys[(size_t)q * n_pad + ci] = row >= 0 ? make_key<METRIC>(acc, (uint32_t)((int64_t)row + id_offset)) : kFlatNoKey;
}

// Grid-stride over the rows * Dp values of the output.
__global__ __launch_bounds__(256) void flat_half_prepare_kernel(const uint16_t* __restrict__ in, int64_t rows, int D, int Dp,
                                                                uint16_t* __restrict__ out) {
    const int64_t total = rows * Dp, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / Dp;
        const int d = (int)(i - r * Dp);
        out[i] = d < D ? in[r * D + d] : (uint16_t)0;
    }
}

__global__ __launch_bounds__(256) void flat_half_narrow_kernel(const float* __restrict__ in, int64_t rows, int D, int Dp,
                                                               int format, uint16_t* __restrict__ out) {
    const int64_t total = rows * Dp, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / Dp;
        const int d = (int)(i - r * Dp);
        out[i] = d < D ? flat_half_narrow(__float_as_uint(in[r * D + d]), format) : (uint16_t)0;
    }
}

unsigned grid_for(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 8192); }

template <bool LIST, int MODE, int METRIC, int FORMAT>
void dist_half(const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys, int cap, const int64_t* offs,
               FlatQueryState* state, hipStream_t stream) {
    flat_dist_half_kernel<LIST, MODE, METRIC, FORMAT><<<dim3((rows + TV - 1) / TV, (q.nq + TQ - 1) / TQ), dim3(256), 0, stream>>>(
        b.h16, b.list, e0, rows, b.Dp, q.f32, q.nq, b.id_offset, keys, cap, offs, state);
}

template <int METRIC, int FORMAT>
auto* pick_dist_half(bool filtered, int mode) {
    return filtered ? (mode == kFlatTopK    ? dist_half<true, kFlatTopK, METRIC, FORMAT>
                       : mode == kFlatCount ? dist_half<true, kFlatCount, METRIC, FORMAT>
                                            : dist_half<true, kFlatEmit, METRIC, FORMAT>)
                    : (mode == kFlatTopK    ? dist_half<false, kFlatTopK, METRIC, FORMAT>
                       : mode == kFlatCount ? dist_half<false, kFlatCount, METRIC, FORMAT>
                                            : dist_half<false, kFlatEmit, METRIC, FORMAT>);
}

}  // namespace

hipError_t launch_flat_half_prepare(const uint16_t* d_in, int64_t rows, int D, int Dp, uint16_t* d_out, hipStream_t stream) {
    const int64_t total = rows * Dp;
    if (total <= 0) return hipSuccess;
    flat_half_prepare_kernel<<<dim3(grid_for(total)), dim3(256), 0, stream>>>(d_in, rows, D, Dp, d_out);
    return hipGetLastError();
}

hipError_t launch_flat_half_narrow(const float* d_in, int64_t rows, int D, int Dp, int format, uint16_t* d_out,
                                   hipStream_t stream) {
    const int64_t total = rows * Dp;
    if (total <= 0) return hipSuccess;
    flat_half_narrow_kernel<<<dim3(grid_for(total)), dim3(256), 0, stream>>>(d_in, rows, D, Dp, format, d_out);
    return hipGetLastError();
}

hipError_t launch_flat_dist_half(int mode, const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys,
                                 int cap, const int64_t* offs, FlatQueryState* state, hipStream_t stream) {
    auto* launch = b.half_format == kFlatBF16
                       ? (b.metric == kFlatIP ? pick_dist_half<kFlatIP, kFlatBF16>(b.filtered, mode)
                                              : pick_dist_half<kFlatL2, kFlatBF16>(b.filtered, mode))
                       : (b.metric == kFlatIP ? pick_dist_half<kFlatIP, kFlatF16>(b.filtered, mode)
                                              : pick_dist_half<kFlatL2, kFlatF16>(b.filtered, mode));
    launch(b, e0, rows, q, keys, cap, offs, state, stream);
    return hipGetLastError();
}

hipError_t launch_flat_rerank_half(int metric, int format, const uint16_t* d_base, int64_t n, int D, int Dp,
                                   const float* d_queries, int nq, const int32_t* d_cand, int n_cand, int top_k,
                                   int64_t id_offset, const uint32_t* d_map, int64_t n_map, uint64_t* d_keys, uint32_t* d_flag,
                                   int32_t* d_ids, float* d_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int n_pad = (int)flat_rerank_keys(n_cand);
    auto* kernel = format == kFlatBF16
                       ? (metric == kFlatIP ? flat_rerank_half_kernel<kFlatIP, kFlatBF16> : flat_rerank_half_kernel<kFlatL2, kFlatBF16>)
                       : (metric == kFlatIP ? flat_rerank_half_kernel<kFlatIP, kFlatF16> : flat_rerank_half_kernel<kFlatL2, kFlatF16>);
    for (int q0 = 0; q0 < nq; q0 += 65535) {  // the grid's y extent
        const int m = std::min(65535, nq - q0);
        kernel<<<dim3((n_pad + 255) / 256, m), dim3(256), 0, stream>>>(
            d_base, n, D, Dp, d_queries + (size_t)q0 * D, d_cand + (size_t)q0 * n_cand, n_cand, n_pad, id_offset, d_map, n_map,
            d_keys + (size_t)q0 * n_pad, d_flag);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_flat_sort_emit(d_keys, (size_t)n_pad, nullptr, nq, n_pad, top_k, d_ids, d_dists, stream, metric);
}

}  // namespace dpq
