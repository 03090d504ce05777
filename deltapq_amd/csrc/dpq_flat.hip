// dpq_flat.hip -- exact L2 distances, or inner products, between fp32 queries and fp32, fp16, bf16 or scalar-quantised
// (8-bit, 4-bit) base vectors on gfx950.
//
// The arithmetic (include/deltapq_amd.h, "exact search"): per dimension, in ascending order, t = v[d] - q[d] and
// s = t * t in fp32, each rounded on its own (the build passes -ffp-contract=off), then acc += (double)s on an fp64
// accumulator that starts at +0.0; the reported distance is (float)acc.  One lane owns one distance from the first
// dimension to the last, so the order of the sum is the reference's (main.cpp:150-156) and the bits are too.
// METRIC = kFlatIP ("exact inner-product search"): acc = acc + (double)v[d] * (double)q[d] instead, one rounding per
// step, and the score's bits go through flat_ip_word into the key, so that ascending keys are descending scores; the
// kernels below are otherwise the same source.
//
//   flat_dist_kernel<LIST, MODE, METRIC, FORMAT>
//                         the one fp32-query distance kernel, for every search.  A workgroup takes 64 queries x 64 entries
//                         of a stripe; both tiles go through LDS in slices of 32 dimensions, transposed so that a lane
//                         reads its four queries and four vectors as two 16-byte LDS loads; 16 fp64 accumulators per
//                         lane.  LIST: entry e is row l0 + e (false: every row, or a range search without a filter), or
//                         row list[l0 + e] (true: a filter's row list), the tile's row numbers staged in LDS.  MODE,
//                         what becomes of a key (distance bits, or the score's key word, << 32 | id):
//                           kFlatTopK   key <= the query's threshold: appended to the query's buffer
//                           kFlatCount  key <  the radius key: counted
//                           kFlatEmit   key <  the radius key: appended to the query's list in the pool, whose length
//                                       the count pass gave
//                         Every append checks its position against the capacity of its buffer and raises
//                         FlatQueryState::overflow instead of storing outside it.  FORMAT: the rows are fp32, or fp16 /
//                         bf16 at half the bytes, widened as the base tile is staged -- a lane loads
//                         16 bytes, eight halves, widens them in registers and writes fp32 to LDS; the staging is the
//                         only code the formats do not share.  Widening is exact, so every answer over a half base
//                         equals, bit for bit, the answer over the widened rows.  No matrix instruction: the f16 / bf16
//                         MFMAs accumulate in fp32 and in an order of their own, which the contract does not allow.
//                         kFlatSQ8 / kFlatSQ4: the rows are codes of a scalar quantiser, a byte or a
//                         nibble per dimension; a lane loads 16 bytes of one row, decodes them with the slice's
//                         (lo, step), read once per slice through scalar loads, and writes fp32 to LDS.
//   flat_select_kernel    when a buffer is filling up: radix select of the top_k-th key, compaction in place, the
//                         threshold lowered to that key.
//   flat_sort_emit_kernel<METRIC>
//                         bitonic sort of a query's keys in LDS, duplicates dropped, ids and distances (scores) written.
//   flat_rerank_kernel<METRIC, FORMAT>
//                         a lane per candidate; a wavefront fetches its 64 rows with 16-byte loads into LDS, 32
//                         dimensions at a time (halves widened, codes decoded on the way), and every lane then walks
//                         its own row in order.
//   flat_pad_rows_kernel, flat_half_prepare_kernel, flat_half_narrow_kernel
//                         pad fp32 rows / pad 16-bit rows / narrow fp32 rows to padded 16-bit rows, when a base is opened
//   flat_sq_minmax_kernel, flat_sq_encode_kernel, flat_sq_prepare_kernel
//                         a scalar quantiser's training reduction (per-dimension minima and maxima, integer atomics on
//                         order-mapped float bits), fp32 rows to codes, a caller's codes to a base's padded rows
// launch_flat_search is the one stripe driver (state, then per stripe a select and a distance launch, then the last
// select and the sort), launch_flat_range_pass the one range pass and launch_flat_rerank the one re-rank launcher (the
// chunks of the grid's y extent, then the sort), for every format, with and without a list; the byte kernels of
// dpq_flat_u8.hip come in through launch_flat_dist_u8 and launch_flat_rerank_chunk_u8, the Hamming kernels of
// dpq_flat_bits.hip through launch_flat_dist_bits and launch_flat_rerank_chunk_bits.  make_key<METRIC>,
// accumulate<METRIC> and flat_candidate_row live in dpq_flat.h.
#include "dpq_flat.h"

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace dpq {
namespace {

constexpr int TQ = 64, TV = 64;  // queries and vectors of a workgroup's tile
constexpr int DC = 32;           // dimensions staged at a time
constexpr int LD = TV + 4;       // LDS row stride in floats (16-byte aligned; spreads the transposed writes)
constexpr int kSelThreads = 1024;

__global__ void flat_init_state_kernel(FlatQueryState* state, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) {
        state[q].count = 0;
        state[q].overflow = 0;
        state[q].thr = kFlatNoKey;
    }
}

__global__ void flat_pad_rows_kernel(const float* in, int64_t rows, int D, int Dp, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * Dp) return;
    const int64_t r = i / Dp;
    const int d = (int)(i - r * Dp);
    out[i] = d < D ? in[r * D + d] : 0.0f;
}

// The stored type of a row's values, and eight halves as they lie in memory -> eight fp32 values (exact: bf16 widens
// with a shift, fp16 with v_cvt_f32_f16, which under the build's 16-bit denormal mode keeps subnormals).
template <int FORMAT> using flat_row_t =
    std::conditional_t<FORMAT == kFlatF32, float, std::conditional_t<FORMAT == kFlatSQ8 || FORMAT == kFlatSQ4, uint8_t, uint16_t>>;
template <int FORMAT> constexpr bool flat_is_sq = FORMAT == kFlatSQ8 || FORMAT == kFlatSQ4;
// Dimensions that 16 bytes of a quantised row hold, and the byte at which dimension d (a multiple of that) of a row starts.
template <int FORMAT> constexpr int flat_sq_dims16 = FORMAT == kFlatSQ8 ? 16 : 32;
template <int FORMAT>
__device__ __forceinline__ size_t flat_sq_offset(int64_t row, int Dp, int d) {
    return FORMAT == kFlatSQ8 ? (size_t)row * Dp + d : ((size_t)row * Dp + d) >> 1;
}

// 16 bytes of a quantised row as they lie in memory -> the 16 (kFlatSQ8) or 32 (kFlatSQ4: low nibble first) fp32 values
// of their dimensions; q: those dimensions' (lo, step), the same for every lane.
template <int FORMAT>
__device__ __forceinline__ void decode16(const uint4& raw, const float2* __restrict__ q, float* out) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t byte = (w[i] >> (8 * b)) & 0xffu;
            const int j = 4 * i + b;
            if constexpr (FORMAT == kFlatSQ8) {
                out[j] = flat_sq_decode(byte, q[j]);
            } else {
                out[2 * j] = flat_sq_decode(byte & 15u, q[2 * j]);
                out[2 * j + 1] = flat_sq_decode(byte >> 4, q[2 * j + 1]);
            }
        }
}

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

// grid (tiles of the stripe's `rows` entries, query tiles), 256 threads: thread (tx, ty) owns queries ty*4.. x entries
// tx*4.. of the tile.  Entry e of the stripe is row l0 + e, computed where it is needed (LIST false: no row numbers in
// LDS, no barrier before the first slice), or row list[l0 + e], staged once per tile in lrow.  Every instantiation is
// the straight-line kernel of its case; nothing is picked at run time.
// FORMAT decides one thing, how a slice of the base tile, 64 rows x 32 dimensions, gets into vs.  fp32: thread t loads
// 16 bytes of rows sr and sr + 32, as it does for the queries.  Halves: the slice is 256 loads of 16 bytes, one per
// thread; thread t takes row vr = (t & 15) | (t >> 6) << 4 and dimensions vj = ((t >> 4) & 3) * 8 .. + 7, so that the 32
// lanes of a half wavefront write 16 consecutive rows of two slice rows that lie 8 * LD floats apart: two addresses per
// LDS bank of a ds_write_b32, which costs nothing extra.  Quantised rows: the slice is 2 KB (kFlatSQ8) or 1 KB (kFlatSQ4),
// 128 or 64 loads of 16 bytes; thread t takes row t & 63 and, at 8 bits, dimensions (t >> 6) * 16 .. + 15 of the slice,
// at 4 bits all 32.  A wavefront's lanes so hold 64 consecutive rows of the same dimensions: every ds_write_b32 puts the
// 32 lanes of a half wavefront on 32 consecutive words, one address per bank, and the dimensions' (lo, step) are the
// same for the whole wavefront, fetched once per slice by scalar loads.  The quantiser lies in front of the rows
// (flat_sq_quant_of), so the kernel's arguments are those of every other format.
template <bool LIST, int MODE, int METRIC, int FORMAT>
__global__ __launch_bounds__(256) void flat_dist_kernel(const void* __restrict__ base_rows, const uint32_t* __restrict__ list,
                                                        int64_t l0, int rows, int Dp, const float* __restrict__ queries,
                                                        int nq, int64_t id_offset, uint64_t* __restrict__ keys, int cap,
                                                        const int64_t* __restrict__ offs, FlatQueryState* state) {
    const auto* base = static_cast<const flat_row_t<FORMAT>*>(base_rows);
    [[maybe_unused]] const float2* quant = flat_sq_quant_of(base_rows, Dp);  // quantised rows only
    __shared__ float qs[DC][LD];
    __shared__ float vs[DC][LD];
    __shared__ uint32_t lrow[TV];  // LIST only
    __shared__ uint32_t cnt[TQ];
    __shared__ uint32_t pos0[TQ];
    __shared__ uint64_t thr[TQ];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int v0 = blockIdx.x * TV, q0 = blockIdx.y * TQ;
    const int sr = tid >> 3, sj = (tid & 7) * 4;  // staging: row sr (and sr + 32), dimensions sj .. sj + 3 of the slice
    const int vr = (tid & 15) | ((tid >> 6) << 4), vj = ((tid >> 4) & 3) * 8;  // halves: row vr, eight dimensions
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
        if constexpr (flat_is_sq<FORMAT>) {
            constexpr int N16 = flat_sq_dims16<FORMAT>;
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wavefront: DC / N16 of the four stage
            const int cj = wv * N16;                                  // its first dimension of the slice
            if (wv < DC / N16 && d0 + cj < Dp) {                      // Dp is a multiple of N16
                const int cr = tid & 63;
                uint4 raw = make_uint4(0u, 0u, 0u, 0u);  // past the stripe: code 0, masked below
                if (v0 + cr < rows) raw = *reinterpret_cast<const uint4*>(base + flat_sq_offset<FORMAT>(row_of(cr), Dp, d0 + cj));
                float v[N16];
                decode16<FORMAT>(raw, quant + d0 + cj, v);
#pragma unroll
                for (int k = 0; k < N16; ++k) vs[cj + k][cr] = v[k];
            }
        } else if constexpr (FORMAT != kFlatF32) {
            uint4 raw = make_uint4(0u, 0u, 0u, 0u);  // the bits of eight zeros in either format
            if (v0 + vr < rows && d0 + vj < Dp) raw = *reinterpret_cast<const uint4*>(base + (size_t)row_of(vr) * Dp + d0 + vj);
            float v[8];
            widen8<FORMAT>(raw, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) vs[vj + k][vr] = v[k];
        }
        // the queries, and beside them the fp32 base tile: both loads ahead of both sets of LDS writes
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = sr + 32 * h, d = d0 + sj;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), q = v;
            if constexpr (FORMAT == kFlatF32)
                if (v0 + r < rows && d < Dp) v = *reinterpret_cast<const float4*>(base + (size_t)row_of(r) * Dp + d);
            if (q0 + r < nq && d < Dp) q = *reinterpret_cast<const float4*>(queries + (size_t)(q0 + r) * Dp + d);
            if constexpr (FORMAT == kFlatF32) {
                vs[sj + 0][r] = v.x; vs[sj + 1][r] = v.y; vs[sj + 2][r] = v.z; vs[sj + 3][r] = v.w;
            }
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

// exclusive prefix sum over the 1024 threads of a workgroup; *total = the sum.  wsum: 16 words of LDS.
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
    for (int k = 0; k < 16; ++k) {
        const uint32_t s = wsum[k];
        if (k < w) woff += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

// One workgroup per query.  With more than `limit` (>= top_k) keys in the buffer: keep the top_k smallest, in place,
// and lower the threshold to the top_k-th.  Keys of one query are distinct (distinct ids), so "<= the k-th" is k keys.
__global__ __launch_bounds__(kSelThreads) void flat_select_kernel(uint64_t* keys, int cap, FlatQueryState* state, int top_k,
                                                                  uint32_t limit) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[16];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_rem;
    const int q = blockIdx.x, tid = threadIdx.x;
    uint64_t* buf = keys + (size_t)q * cap;
    const uint32_t cnt = min(state[q].count, (uint32_t)cap);
    if (cnt <= limit) return;
    uint64_t prefix = 0, mask = 0;
    uint32_t rem = (uint32_t)top_k;  // rank, from 1, of the wanted key among those that match the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < cnt; i += kSelThreads) {
            const uint64_t k = buf[i];
            if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0;
            for (int b = 0; b < 256; ++b) {
                if (cum + hist[b] >= rem) {
                    s_prefix = prefix | ((uint64_t)b << shift);
                    s_rem = rem - cum;
                    break;
                }
                cum += hist[b];
            }
        }
        __syncthreads();
        prefix = s_prefix;
        rem = s_rem;
        mask |= 0xffull << shift;
        __syncthreads();
    }
    const uint64_t kth = prefix;
    uint32_t out = 0;
    for (uint32_t b = 0; b < cnt; b += kSelThreads) {
        // a round reads [b, b + 1024) before the barrier inside the scan and writes below b + 1024 after it
        const uint32_t i = b + tid;
        const uint64_t k = i < cnt ? buf[i] : kFlatNoKey;
        const uint32_t keep = i < cnt && k <= kth;
        uint32_t total;
        const uint32_t off = block_scan_1024(keep, wsum, &total);
        if (keep) buf[out + off] = k;
        out += total;
    }
    if (tid == 0) {
        state[q].count = out;  // == top_k
        state[q].thr = kth;
    }
}

// One workgroup per query: sort its keys (n_keys of them, or state[q].count) in LDS, drop repeats, write the first
// top_k as (id, distance); rows are padded with -1 / +inf.  kFlatNoKey entries are padding.  n_pad: a power of two.
// kFlatIP: the key's high word is unmade into the score's bits, and the padding is -1 / -inf.
template <int METRIC>
__global__ __launch_bounds__(kSelThreads) void flat_sort_emit_kernel(const uint64_t* __restrict__ keys, size_t stride,
                                                                     const FlatQueryState* state, int n_keys, int n_pad,
                                                                     int top_k, int32_t* __restrict__ ids,
                                                                     float* __restrict__ dists) {
    extern __shared__ uint64_t sk[];
    __shared__ uint32_t wsum[16];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int cnt = state ? (int)min(state[q].count, (uint32_t)n_keys) : n_keys;
    for (int i = tid; i < n_pad; i += kSelThreads) sk[i] = i < cnt ? keys[(size_t)q * stride + i] : kFlatNoKey;
    __syncthreads();
    for (int k = 2; k <= n_pad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n_pad; i += kSelThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t a = sk[i], b = sk[x];
                    if ((a > b) == ((i & k) == 0)) {
                        sk[i] = b;
                        sk[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    const int per = (n_pad + kSelThreads - 1) / kSelThreads;
    const int lo = min(n_pad, tid * per), hi = min(n_pad, lo + per);
    uint32_t u = 0;
    for (int i = lo; i < hi; ++i) u += sk[i] != kFlatNoKey && (i == 0 || sk[i] != sk[i - 1]);
    uint32_t total;
    uint32_t pos = block_scan_1024(u, wsum, &total);
    for (int i = lo; i < hi; ++i)
        if (sk[i] != kFlatNoKey && (i == 0 || sk[i] != sk[i - 1])) {
            if (pos < (uint32_t)top_k) {
                ids[(size_t)q * top_k + pos] = (int32_t)(uint32_t)(sk[i] & 0xffffffffu);
                const uint32_t w = (uint32_t)(sk[i] >> 32);
                dists[(size_t)q * top_k + pos] = __uint_as_float(METRIC == kFlatIP ? flat_ip_word(w) : w);
            }
            ++pos;
        }
    for (int r = (int)total + tid; r < top_k; r += kSelThreads) {
        ids[(size_t)q * top_k + r] = -1;
        dists[(size_t)q * top_k + r] = __uint_as_float(METRIC == kFlatIP ? 0xff800000u : 0x7f800000u);
    }
}

// grid (candidate groups of 256, queries), 256 threads: lane = candidate.  FORMAT decides how a wavefront fetches the
// 32-dimension slice of its 64 rows into its tile: eight rounds of 8 rows, eight lanes of 16 bytes (four floats) per row,
// or, for halves, four rounds of 16 rows, four lanes of 16 bytes (eight halves, widened) per row.  Quantised rows: a lane
// per row, 16 bytes of it per round -- two rounds of 16 dimensions at 8 bits, one of 32 at 4 -- so that a round's
// (lo, step) are the same for every lane (scalar loads) and a lane decodes into its own row of the tile.
template <int METRIC, int FORMAT>
__global__ __launch_bounds__(256) void flat_rerank_kernel(const void* __restrict__ base_rows, int64_t n, int D, int Dp,
                                                          const float* __restrict__ queries,
                                                          const int32_t* __restrict__ cand, int n_cand, int n_pad,
                                                          int64_t id_offset, const uint32_t* __restrict__ map,
                                                          int64_t n_map, uint64_t* __restrict__ keys, uint32_t* flag) {
    const auto* base = static_cast<const flat_row_t<FORMAT>*>(base_rows);
    [[maybe_unused]] const float2* quant = flat_sq_quant_of(base_rows, Dp);  // quantised rows only
    __shared__ float qv[kFlatMaxD];
    __shared__ float tile[4][64][DC + 1];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int d = tid; d < Dp; d += 256) qv[d] = d < D ? queries[(size_t)q * D + d] : 0.0f;
    const int ci = blockIdx.x * 256 + tid;
    int row = -1;
    if (ci < n_cand) row = flat_candidate_row(cand[(size_t)q * n_cand + ci], n, id_offset, map, n_map, flag);
    __syncthreads();
    double acc = 0.0;
    const int lj = FORMAT == kFlatF32 ? (lane & 7) * 4 : (lane & 3) * 8;  // the lane's first dimension of a fetched slice
    for (int d0 = 0; d0 < Dp; d0 += DC) {
        if constexpr (flat_is_sq<FORMAT>) {
            constexpr int N16 = flat_sq_dims16<FORMAT>;
#pragma unroll
            for (int cj = 0; cj < DC; cj += N16) {
                if (d0 + cj >= Dp) break;  // Dp is a multiple of N16
                uint4 raw = make_uint4(0u, 0u, 0u, 0u);
                if (row >= 0) raw = *reinterpret_cast<const uint4*>(base + flat_sq_offset<FORMAT>(row, Dp, d0 + cj));
                float v[N16];
                decode16<FORMAT>(raw, quant + d0 + cj, v);
#pragma unroll
                for (int k = 0; k < N16; ++k) tile[w][lane][cj + k] = v[k];
            }
        } else if constexpr (FORMAT == kFlatF32) {
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int cc = it * 8 + (lane >> 3);
                const int rr = __shfl(row, cc);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rr >= 0 && d0 + lj < Dp) v = *reinterpret_cast<const float4*>(base + (size_t)rr * Dp + d0 + lj);
                tile[w][cc][lj + 0] = v.x; tile[w][cc][lj + 1] = v.y; tile[w][cc][lj + 2] = v.z; tile[w][cc][lj + 3] = v.w;
            }
        } else {
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

// The two kernels that make a half base's rows.  Grid-stride over the rows * Dp values of the output.
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

// The kernels of a scalar quantiser.  Min / max: block (64, 4), thread (x, y) walks column blockIdx.y * 64 + x over rows
// y, y + 4, .. of the block's kSqRows and folds its minimum and maximum into the column's order words.
constexpr int kSqRows = 1024;
__global__ __launch_bounds__(256) void flat_sq_minmax_kernel(const float* __restrict__ in, int64_t rows, int D,
                                                             uint32_t* __restrict__ mn, uint32_t* __restrict__ mx) {
    const int d = blockIdx.y * 64 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kSqRows, r1 = min(rows, r0 + kSqRows);
    if (d >= D || r0 + threadIdx.y >= r1) return;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int64_t r = r0 + threadIdx.y; r < r1; r += 4) {
        const uint32_t w = flat_order_word(__float_as_uint(in[r * D + d]));
        lo = min(lo, w);
        hi = max(hi, w);
    }
    atomicMin(&mn[d], lo);
    atomicMax(&mx[d], hi);
}

// The code of v (include/deltapq_amd.h, "scalar-quantised vectors"): fp64 subtract, fp64 divide, ties to even, clamp.
__device__ __forceinline__ uint32_t flat_sq_code(float v, float2 q, double top) {
    if (q.y == 0.0f) return 0u;
    const double u = ((double)v - (double)q.x) / (double)q.y;
    return (uint32_t)(int)fmin(fmax(rint(u), 0.0), top);
}

// One byte of the output per step of the grid-stride loop.
__global__ __launch_bounds__(256) void flat_sq_encode_kernel(const float* __restrict__ in, int64_t rows, int D, int bits,
                                                             const float2* __restrict__ quant, uint8_t* __restrict__ out,
                                                             int out_stride) {
    const int64_t total = rows * out_stride, step = (int64_t)gridDim.x * blockDim.x;
    const double top = bits == 8 ? 255.0 : 15.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / out_stride;
        const int j = (int)(i - r * out_stride);
        uint32_t c = 0;
        if (bits == 8) {
            if (j < D) c = flat_sq_code(in[r * D + j], quant[j], top);
        } else {
            if (2 * j < D) c = flat_sq_code(in[r * D + 2 * j], quant[2 * j], top);
            if (2 * j + 1 < D) c |= flat_sq_code(in[r * D + 2 * j + 1], quant[2 * j + 1], top) << 4;
        }
        out[i] = (uint8_t)c;
    }
}

__global__ __launch_bounds__(256) void flat_sq_prepare_kernel(const uint8_t* __restrict__ in, int64_t rows, int D, int bits,
                                                              uint8_t* __restrict__ out, int out_stride) {
    const int64_t total = rows * out_stride, step = (int64_t)gridDim.x * blockDim.x;
    const int in_stride = flat_sq_row_bytes(D, bits);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / out_stride;
        const int j = (int)(i - r * out_stride);
        uint8_t c = j < in_stride ? in[r * in_stride + j] : (uint8_t)0;
        if (bits == 4 && 2 * j + 1 >= D) c &= 15u;  // the spare nibble of an odd D
        out[i] = c;
    }
}

unsigned grid_for(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 8192); }

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// hipFuncSetAttribute is per device
hipError_t ensure_sort_lds() {
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        for (const void* fn : {reinterpret_cast<const void*>(flat_sort_emit_kernel<kFlatL2>),
                               reinterpret_cast<const void*>(flat_sort_emit_kernel<kFlatIP>)}) {
            e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kFlatMaxTopK * (int)sizeof(uint64_t));
            if (e != hipSuccess) return e;
        }
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

int flat_key_capacity(int top_k) { return std::max(8192, pow2_at_least(4 * top_k)); }

int flat_query_batch(int top_k) { return (int)(((size_t)64 << 20) / ((size_t)flat_key_capacity(top_k) * sizeof(uint64_t))); }

size_t flat_rerank_keys(int n_cand) { return (size_t)pow2_at_least(n_cand); }

hipError_t launch_flat_pad_rows(const float* d_in, int64_t rows, int D, int Dp, float* d_out, hipStream_t stream) {
    const int64_t total = rows * Dp;
    if (total <= 0) return hipSuccess;
    flat_pad_rows_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(d_in, rows, D, Dp, d_out);
    return hipGetLastError();
}

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

hipError_t launch_flat_sq_minmax(const float* d_in, int64_t rows, int D, uint32_t* d_mn, uint32_t* d_mx, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    flat_sq_minmax_kernel<<<dim3((unsigned)((rows + kSqRows - 1) / kSqRows), (D + 63) / 64), dim3(64, 4), 0, stream>>>(
        d_in, rows, D, d_mn, d_mx);
    return hipGetLastError();
}

hipError_t launch_flat_sq_encode(const float* d_in, int64_t rows, int D, int bits, const float2* d_quant, uint8_t* d_out,
                                 int out_stride, hipStream_t stream) {
    const int64_t total = rows * out_stride;
    if (total <= 0) return hipSuccess;
    flat_sq_encode_kernel<<<dim3(grid_for(total)), dim3(256), 0, stream>>>(d_in, rows, D, bits, d_quant, d_out, out_stride);
    return hipGetLastError();
}

hipError_t launch_flat_sq_prepare(const uint8_t* d_in, int64_t rows, int D, int bits, uint8_t* d_out, int out_stride,
                                  hipStream_t stream) {
    const int64_t total = rows * out_stride;
    if (total <= 0) return hipSuccess;
    flat_sq_prepare_kernel<<<dim3(grid_for(total)), dim3(256), 0, stream>>>(d_in, rows, D, bits, d_out, out_stride);
    return hipGetLastError();
}

namespace {

template <bool LIST, int MODE, int METRIC, int FORMAT>
void dist(const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys, int cap, const int64_t* offs,
          FlatQueryState* state, hipStream_t stream) {
    flat_dist_kernel<LIST, MODE, METRIC, FORMAT><<<dim3((rows + TV - 1) / TV, (q.nq + TQ - 1) / TQ), dim3(256), 0, stream>>>(
        b.rows, b.list, e0, rows, b.Dp, q.f32, q.nq, b.id_offset, keys, cap, offs, state);
}

// The launch of an fp32-query base's instantiation: format x metric x row source x mode.
template <int METRIC, int FORMAT>
auto* pick_dist(bool filtered, int mode) {
    return filtered ? (mode == kFlatTopK    ? dist<true, kFlatTopK, METRIC, FORMAT>
                       : mode == kFlatCount ? dist<true, kFlatCount, METRIC, FORMAT>
                                            : dist<true, kFlatEmit, METRIC, FORMAT>)
                    : (mode == kFlatTopK    ? dist<false, kFlatTopK, METRIC, FORMAT>
                       : mode == kFlatCount ? dist<false, kFlatCount, METRIC, FORMAT>
                                            : dist<false, kFlatEmit, METRIC, FORMAT>);
}

template <int FORMAT>
auto* pick_dist(int metric, bool filtered, int mode) {
    return metric == kFlatIP ? pick_dist<kFlatIP, FORMAT>(filtered, mode) : pick_dist<kFlatL2, FORMAT>(filtered, mode);
}

// The sort stage of a search or a re-rank, by metric.
void sort_emit(int metric, const uint64_t* d_keys, size_t stride, const FlatQueryState* d_state, int nq, int n_keys,
               int n_pad, int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    auto* kernel = metric == kFlatIP ? flat_sort_emit_kernel<kFlatIP> : flat_sort_emit_kernel<kFlatL2>;
    kernel<<<dim3(nq), dim3(kSelThreads), (size_t)n_pad * sizeof(uint64_t), stream>>>(d_keys, stride, d_state, n_keys, n_pad,
                                                                                     top_k, d_ids, d_dists);
}

// A quantised base keeps its quantiser where the kernels look for it.
bool sq_layout_ok(const FlatBase& b) {
    return (b.format != kFlatSQ8 && b.format != kFlatSQ4) || (b.quant && b.quant == flat_sq_quant_of(b.rows, b.Dp));
}

// One distance launch over entries e0 .. e0 + rows - 1 of the base, by format, metric, row source and mode.
hipError_t launch_flat_dist(int mode, const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys, int cap,
                            const int64_t* offs, FlatQueryState* state, hipStream_t stream) {
    if (!sq_layout_ok(b)) return hipErrorInvalidValue;
    switch (b.format) {
        case kFlatU8:
        case kFlatI8: return launch_flat_dist_u8(mode, b, e0, rows, q, keys, cap, offs, state, stream);
        case kFlatBits: return launch_flat_dist_bits(mode, b, e0, rows, q, keys, cap, offs, state, stream);
        case kFlatF16: pick_dist<kFlatF16>(b.metric, b.filtered, mode)(b, e0, rows, q, keys, cap, offs, state, stream); break;
        case kFlatBF16: pick_dist<kFlatBF16>(b.metric, b.filtered, mode)(b, e0, rows, q, keys, cap, offs, state, stream); break;
        case kFlatSQ8: pick_dist<kFlatSQ8>(b.metric, b.filtered, mode)(b, e0, rows, q, keys, cap, offs, state, stream); break;
        case kFlatSQ4: pick_dist<kFlatSQ4>(b.metric, b.filtered, mode)(b, e0, rows, q, keys, cap, offs, state, stream); break;
        default: pick_dist<kFlatF32>(b.metric, b.filtered, mode)(b, e0, rows, q, keys, cap, offs, state, stream);
    }
    return hipGetLastError();
}

template <int FORMAT>
void rerank_chunk(const FlatBase& b, const FlatRerank& r, int n_pad, hipStream_t stream) {
    auto* kernel = b.metric == kFlatIP ? flat_rerank_kernel<kFlatIP, FORMAT> : flat_rerank_kernel<kFlatL2, FORMAT>;
    kernel<<<dim3((n_pad + 255) / 256, r.nq), dim3(256), 0, stream>>>(
        b.rows, b.n, b.D, b.Dp, static_cast<const float*>(r.queries), r.cand, r.n_cand, n_pad, b.id_offset, r.map, r.n_map,
        r.keys, r.flag);
}

}  // namespace

hipError_t launch_flat_search(const FlatBase& b, const FlatQueries& q, int top_k, uint64_t* d_keys, FlatQueryState* d_state,
                              int32_t* d_ids, float* d_dists, hipStream_t stream) {
    const int nq = q.nq;
    if (nq <= 0) return hipSuccess;
    hipError_t e = ensure_sort_lds();
    if (e != hipSuccess) return e;
    const int cap = flat_key_capacity(top_k);
    // A stripe appends at most cap / 2 keys to a buffer, and a buffer enters a stripe with at most cap / 2: the select
    // between two stripes cuts every buffer above cap / 4 (>= top_k) down to top_k.  The first stripe, with no
    // threshold yet, is the prefix the first thresholds come from.  A stripe is cap / 2 entries: rows, or list entries.
    const int64_t stripe = cap / 2;
    const uint32_t limit = (uint32_t)std::max(top_k, cap / 4);
    flat_init_state_kernel<<<dim3((nq + 255) / 256), dim3(256), 0, stream>>>(d_state, nq);
    for (int64_t e0 = 0; e0 < b.n_entries; e0 += stripe) {
        const int rows = (int)std::min<int64_t>(stripe, b.n_entries - e0);
        if (e0 > 0) flat_select_kernel<<<dim3(nq), dim3(kSelThreads), 0, stream>>>(d_keys, cap, d_state, top_k, limit);
        if ((e = launch_flat_dist(kFlatTopK, b, e0, rows, q, d_keys, cap, nullptr, d_state, stream)) != hipSuccess) return e;
    }
    flat_select_kernel<<<dim3(nq), dim3(kSelThreads), 0, stream>>>(d_keys, cap, d_state, top_k, (uint32_t)top_k);
    const int n_pad = pow2_at_least(top_k);
    sort_emit(b.metric, d_keys, (size_t)cap, d_state, nq, top_k, n_pad, top_k, d_ids, d_dists, stream);
    return hipGetLastError();
}

hipError_t launch_flat_range_pass(const FlatBase& b, const FlatQueries& q, uint64_t* d_pool, const int64_t* d_offs,
                                  FlatQueryState* d_state, hipStream_t stream) {
    if (q.nq <= 0 || b.n_entries <= 0) return hipSuccess;
    return launch_flat_dist(d_pool ? kFlatEmit : kFlatCount, b, 0, (int)b.n_entries, q, d_pool, 0, d_pool ? d_offs : nullptr,
                            d_state, stream);
}

hipError_t launch_flat_rerank(const FlatBase& b, const FlatRerank& r, hipStream_t stream) {
    if (r.nq <= 0) return hipSuccess;
    if (!sq_layout_ok(b)) return hipErrorInvalidValue;
    hipError_t e = ensure_sort_lds();
    if (e != hipSuccess) return e;
    const int n_pad = pow2_at_least(r.n_cand);
    const size_t q_bytes = b.format == kFlatBits ? (size_t)flat_bits_bytes(b.D)  // of one query
                                                 : (size_t)b.D * (flat_query_format(b.format) == kFlatF32 ? sizeof(float) : 1);
    for (int q0 = 0; q0 < r.nq; q0 += 65535) {  // the grid's y extent
        FlatRerank c = r;
        c.queries = static_cast<const char*>(r.queries) + (size_t)q0 * q_bytes;
        c.nq = std::min(65535, r.nq - q0);
        c.cand = r.cand + (size_t)q0 * r.n_cand;
        c.keys = r.keys + (size_t)q0 * n_pad;
        switch (b.format) {
            case kFlatU8:
            case kFlatI8: launch_flat_rerank_chunk_u8(b, c, n_pad, stream); break;
            case kFlatBits: launch_flat_rerank_chunk_bits(b, c, n_pad, stream); break;
            case kFlatF16: rerank_chunk<kFlatF16>(b, c, n_pad, stream); break;
            case kFlatBF16: rerank_chunk<kFlatBF16>(b, c, n_pad, stream); break;
            case kFlatSQ8: rerank_chunk<kFlatSQ8>(b, c, n_pad, stream); break;
            case kFlatSQ4: rerank_chunk<kFlatSQ4>(b, c, n_pad, stream); break;
            default: rerank_chunk<kFlatF32>(b, c, n_pad, stream);
        }
    }
    sort_emit(b.metric, r.keys, (size_t)n_pad, nullptr, r.nq, n_pad, n_pad, r.top_k, r.ids, r.dists, stream);
    return hipGetLastError();
}

hipError_t launch_flat_sort_emit(const uint64_t* d_keys, size_t stride, const FlatQueryState* d_state, int nq, int n_keys,
                                 int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream, int metric) {
    hipError_t e = ensure_sort_lds();
    if (e != hipSuccess) return e;
    const int n_pad = pow2_at_least(n_keys);
    sort_emit(metric, d_keys, stride, d_state, nq, n_keys, n_pad, top_k, d_ids, d_dists, stream);
    return hipGetLastError();
}

}  // namespace dpq
