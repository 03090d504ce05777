// dpq_flat_u8.hip -- exact L2 distances and inner products between byte queries and byte base vectors, unsigned
// (0..255) or signed (-128..127), on the int8 matrix cores of gfx950.
//
// With v, q in {0..255}^D and D <= 2048 every intermediate of the fp32 path's arithmetic (dpq_flat.hip) is an exactly
// representable integer: |t| <= 255, s <= 65025, acc <= 2048 * 65025 < 2^31.  The reported distance is therefore
// (float)(int32)sum (v[d] - q[d])^2, round to nearest even, whatever the order of the sum -- the same bits as
// flat_dist_kernel gives on the widened data.
//
// The MFMA operands are signed bytes, so a value x is stored as x ^ 0x80 (x - 128 as int8), rows padded with int8 zeros
// to a multiple of 32 bytes, with the int32 norm |v'|^2 beside them.  Differences are unchanged by the bias:
//     |v - q|^2 = |v'|^2 + |q'|^2 - 2 v'.q'      all in int32, |v'.q'| <= 2048 * 128^2 = 2^25.
// An int8 zero adds nothing to a dot product or a norm, so padding is invisible.
// A signed base (dpq_flat_open_i8) stores its rows as they are; its L2 is the same identity and the same kernel.
//
// Inner product (kFlatIP): the score is (float)(int32)S, its key word flat_ip_word of the bits.  Signed rows: S = v.q,
// the int8 dot product itself, |S| <= 2048 * 128^2 = 2^25.  Unsigned rows, v = v' + 128 and q = q' + 128:
//     S = v'.q' + rs[row] + qs[query],   rs = 128 sum v' + 16384 D (= 128 sum v, 0 .. 2048 * 32640 < 2^26),
//                                        qs = 128 sum q'           (within +-2^25),
// all in int32 (S <= 2048 * 65025 < 2^31).  The padding adds nothing to either sum.  The kernel takes rs / qs in the
// place of the norms; flat_u8_sums_kernel makes them.
//
//   flat_u8_bias_rows_kernel<BIAS>
//                              bytes [rows][D] -> int8 [rows][Dp], biased (unsigned data) or as they are, padded
//   flat_u8_norms_kernel       a lane per row: its int32 norm
//   flat_u8_sums_kernel        a lane per row: 128 * the sum of its int8 values + a constant (rs, qs above)
//   flat_dist_u8_kernel<LIST, MODE, METRIC, CORR>
//                              the one byte distance kernel, for every search.  A workgroup takes 64 queries x 256
//                              entries of a stripe, a wavefront 64 x 64 as 2 x 2 tiles of v_mfma_i32_32x32x32_i8 (A =
//                              vectors, B = queries); a lane's operand of a K step is 16 contiguous bytes of one row,
//                              loaded straight from global memory.  The epilogue forms the int32 distances and treats
//                              the keys as flat_dist_kernel<LIST, MODE> does: the same row sources (LIST), the same
//                              modes and threshold / counter protocol (dpq_flat.hip's header).  kFlatIP: the epilogue
//                              forms the scores instead, with (CORR, unsigned rows) or without (signed rows) the two
//                              correction terms, and the keys' high words are flat_ip_word of their bits.
//   flat_rerank_u8_kernel<METRIC, SIGNED>
//                              a lane per candidate; a wavefront fetches its 64 rows with 16-byte loads into LDS, 128
//                              bytes of a row at a time, and every lane then sums its own row in int32.
// State, selection, the final sort, the stripe driver and the re-rank launcher are dpq_flat.hip's; launch_flat_dist_u8 and
// launch_flat_rerank_chunk_u8 are the two ways in.
#include "dpq_flat.h"

namespace dpq {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

constexpr int UQ = 64;    // queries of a workgroup's tile
constexpr int UV = 256;   // vectors of a workgroup's tile: 64 per wavefront
constexpr int KS = 32;    // bytes of a row one MFMA consumes (kFlatU8KStep)
constexpr int RC = 128;   // bytes of a row the re-rank stages at a time

static_assert(KS == kFlatU8KStep, "rows are padded to the K step of the MFMA");

// The high word of a key: the fp32 bits of the integer distance, or the key word of the integer score's.
template <int METRIC>
__device__ __forceinline__ uint32_t key_word_i32(int x) {
    const uint32_t u = __float_as_uint(__int2float_rn(x));
    return METRIC == kFlatIP ? flat_ip_word(u) : u;
}

// one thread per four output bytes (Dp is a multiple of four)
template <bool BIAS>
__global__ void flat_u8_bias_rows_kernel(const uint8_t* __restrict__ in, int64_t rows, int D, int Dp,
                                         int8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = Dp >> 2;
    if (i >= rows * wpr) return;
    const int64_t r = i / wpr;
    const int d = (int)(i - r * wpr) * 4;
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (d + b < D) w |= (uint32_t)(in[r * D + d + b] ^ (BIAS ? 0x80u : 0u)) << (8 * b);
    *reinterpret_cast<uint32_t*>(out + r * Dp + d) = w;
}

__device__ __forceinline__ int sq_sum4(uint32_t a) {
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int x = (int)(int8_t)(a >> (8 * b));
        s += x * x;
    }
    return s;
}

__global__ void flat_u8_norms_kernel(const int8_t* __restrict__ rows8, int64_t rows, int Dp, int32_t* __restrict__ norms) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int s = 0;
    for (int d = 0; d < Dp; d += 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(rows8 + r * Dp + d);
        s += sq_sum4(v.x) + sq_sum4(v.y) + sq_sum4(v.z) + sq_sum4(v.w);
    }
    norms[r] = s;
}

__device__ __forceinline__ int sum4(uint32_t a) {
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) s += (int)(int8_t)(a >> (8 * b));
    return s;
}

// sums[r] = 128 * (the sum of row r's int8 values) + add: the correction terms of the unsigned inner product
__global__ void flat_u8_sums_kernel(const int8_t* __restrict__ rows8, int64_t rows, int Dp, int add, int32_t* __restrict__ sums) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int s = 0;
    for (int d = 0; d < Dp; d += 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(rows8 + r * Dp + d);
        s += sum4(v.x) + sum4(v.y) + sum4(v.z) + sum4(v.w);
    }
    sums[r] = 128 * s + add;
}

// grid (tiles of the stripe's `rows` entries, query tiles), 256 threads.  Wavefront w owns entries 64 w .. 64 w + 63 of
// the workgroup's 256 and all 64 queries.  acc[i][j] is the 32 x 32 tile of the wavefront's entries 32 i .. x queries
// 32 j ..: register e of lane l holds entry 32 i + (e & 3) + 8 (e >> 2) + 4 (l >> 5) against query 32 j + (l & 31)  (the
// C/D map of the 32x32 shapes).  Entry e of the stripe is row l0 + e, computed where it is needed (LIST false: no row
// numbers in LDS, no barrier before the MFMA loop, the norms of four adjacent registers one 16-byte load), or row
// list[l0 + e], staged once per tile in lrow, every norm fetched by its row number.  Every instantiation is the
// straight-line kernel of its case; nothing is picked at run time.
// kFlatIP: vnorm / qnorm are the correction terms rs / qs of an unsigned base (CORR), or are not read at all (a signed
// base); the MFMA loop is the same.  kFlatL2 has no CORR = false form.
template <bool LIST, int MODE, int METRIC, bool CORR>
__global__ __launch_bounds__(256) void flat_dist_u8_kernel(const int8_t* __restrict__ base, const int32_t* __restrict__ vnorm,
                                                           const uint32_t* __restrict__ list, int64_t l0, int rows, int Dp,
                                                           const int8_t* __restrict__ queries,
                                                           const int32_t* __restrict__ qnorm, int nq, int64_t id_offset,
                                                           uint64_t* __restrict__ keys, int cap,
                                                           const int64_t* __restrict__ offs, FlatQueryState* state) {
    __shared__ uint32_t lrow[UV];  // LIST only
    __shared__ uint32_t cnt[UQ];
    __shared__ uint32_t pos0[UQ];
    __shared__ uint64_t thr[UQ];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int b0 = blockIdx.x * UV, q0 = blockIdx.y * UQ;  // b0: the tile's first entry in the stripe
    // Below, an entry goes by the index v that finds its row: its place in the tile under LIST (lrow[v]), its place in
    // the stripe otherwise (row l0 + v).  v0: the wavefront's first entry.  inside(v): the stripe has that entry.
    const int v0 = (LIST ? 0 : b0) + w * 64;
    auto inside = [&](int v) { return (LIST ? b0 + v : v) < rows; };
    if constexpr (LIST) {
        lrow[tid] = b0 + tid < rows ? list[l0 + b0 + tid] : 0;  // past the stripe: row 0, masked below
    }
    if (tid < UQ) {
        cnt[tid] = 0;
        thr[tid] = q0 + tid < nq ? state[q0 + tid].thr : 0;
    }
    if constexpr (LIST) __syncthreads();
    // the row of entry v; past the stripe it is clamped to a row that exists, and the entry masked below
    auto row_of = [&](int v) -> int64_t {
        if constexpr (LIST) return lrow[v];
        else return l0 + (inside(v) ? v : 0);
    };

    // lane l feeds row (l & 31) of a tile with bytes 16 (l >> 5) .. + 15 of the K step, on both sides
    const int8_t* ap[2];
    const int8_t* bp[2];
    bool aok[2], bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int v = v0 + 32 * i + r, q = q0 + 32 * i + r;
        aok[i] = inside(v);
        bok[i] = q < nq;
        ap[i] = base + (size_t)row_of(v) * Dp + 16 * h;
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
    if constexpr (!LIST) __syncthreads();  // cnt and thr

    // dot products -> the fp32 bit patterns of the distances, in place.  A distance is a non-negative integer, so its
    // bits order as unsigned integers and key <= thr is (bits, id) <= (thr >> 32, thr & 0xffffffff).  kFlatIP: the key
    // words of the scores, which order as unsigned integers by construction.
    static_assert(METRIC == kFlatIP || CORR, "the L2 epilogue always reads the norms");
    uint32_t thi[2], tlo[2];
    bool qok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ql = 32 * j + r;
        qok[j] = q0 + ql < nq;
        thi[j] = (uint32_t)(thr[ql] >> 32);
        tlo[j] = (uint32_t)thr[ql];
        int qn = 0;
        if constexpr (CORR) qn = qok[j] ? qnorm[q0 + ql] : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int vg = v0 + 32 * i + 8 * g + 4 * h;  // four entries in a row: registers 4 g .. 4 g + 3
                // Their norms: one 16-byte load where the rows are adjacent (vnorm is padded to four rows), else a load
                // per row right before its conversion -- fetching the four first costs 4 % of a filtered search.
                i32x4 vn = zero;
                if constexpr (!LIST && CORR)
                    if (inside(vg)) vn = *reinterpret_cast<const i32x4*>(vnorm + l0 + vg);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if constexpr (LIST && CORR) vn[c] = vnorm[row_of(vg + c)];
                    if constexpr (METRIC == kFlatL2)
                        acc[i][j][4 * g + c] = __float_as_int(__int2float_rn(vn[c] + qn - 2 * acc[i][j][4 * g + c]));
                    else if constexpr (CORR)
                        acc[i][j][4 * g + c] = (int)key_word_i32<kFlatIP>(acc[i][j][4 * g + c] + vn[c] + qn);
                    else
                        acc[i][j][4 * g + c] = (int)key_word_i32<kFlatIP>(acc[i][j][4 * g + c]);
                }
            }
    }
    // the reported id of entry v
    const uint32_t id0 = LIST ? (uint32_t)id_offset : (uint32_t)(id_offset + l0);
    auto id_of = [&](int v) -> uint32_t {
        if constexpr (LIST) return id0 + lrow[v];
        else return id0 + (uint32_t)v;
    };
    auto passes = [&](int i, int j, int e, int v) {
        const uint32_t b = (uint32_t)acc[i][j][e];
        if (!inside(v)) return false;
        if (MODE != kFlatTopK) return b < thi[j];  // the radius key's id half is zero
        return b < thi[j] || (b == thi[j] && id_of(v) <= tlo[j]);
    };

    // first pass: how many of a lane's 32 entries per query pass, and where its run starts in the query's block
    uint32_t run[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        uint32_t np = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) np += passes(i, j, e, v0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h);
        if (!qok[j]) np = 0;
        run[j] = np ? atomicAdd(&cnt[32 * j + r], np) : 0u;
    }
    __syncthreads();
    if (tid < UQ && cnt[tid]) pos0[tid] = atomicAdd(&state[q0 + tid].count, cnt[tid]);
    if (MODE == kFlatCount) return;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ql = 32 * j + r;
        if (!qok[j] || !cnt[ql]) continue;
        uint32_t pos = pos0[ql] + run[j];
        uint32_t room;
        uint64_t* out = flat_sink_of<MODE>(keys, cap, offs, q0 + ql, &room);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int v = v0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (passes(i, j, e, v)) {
                    if (pos < room)
                        out[pos] = ((uint64_t)(uint32_t)acc[i][j][e] << 32) | id_of(v);
                    else
                        state[q0 + ql].overflow = 1;
                    ++pos;
                }
            }
    }
}

__device__ __forceinline__ int sq_diff4(uint32_t a, uint32_t b) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)(int8_t)(a >> (8 * k)) - (int)(int8_t)(b >> (8 * k));
        s += d * d;
    }
    return s;
}

// kFlatIP over signed rows: the int8 products as they are.
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (int)(int8_t)(a >> (8 * k)) * (int)(int8_t)(b >> (8 * k));
    return s;
}

// kFlatIP over unsigned rows stored biased: (v' + 128)(q' + 128), the products of the bytes themselves.
__device__ __forceinline__ int dot4_biased(uint32_t a, uint32_t b) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += ((int)(int8_t)(a >> (8 * k)) + 128) * ((int)(int8_t)(b >> (8 * k)) + 128);
    return s;
}

template <int METRIC, bool SIGNED>
__device__ __forceinline__ int pair4(uint32_t a, uint32_t b) {
    if constexpr (METRIC == kFlatL2) return sq_diff4(a, b);
    else if constexpr (SIGNED) return dot4(a, b);
    else return dot4_biased(a, b);
}

// grid (candidate groups of 256, queries), 256 threads: lane = candidate.  queries: the caller's bytes [nq][D], read as
// int8 when SIGNED.  The query is staged as the rows are stored; its padding is an int8 zero, except for the unsigned
// inner product, where a padded row byte stands for 128 and the query's padding must stand for 0: the int8 -128.
template <int METRIC, bool SIGNED>
__global__ __launch_bounds__(256) void flat_rerank_u8_kernel(const int8_t* __restrict__ base, int64_t n, int D, int Dp,
                                                             const uint8_t* __restrict__ queries,
                                                             const int32_t* __restrict__ cand, int n_cand, int n_pad,
                                                             int64_t id_offset, const uint32_t* __restrict__ map,
                                                             int64_t n_map, uint64_t* __restrict__ keys, uint32_t* flag) {
    __shared__ __align__(16) int8_t qv[kFlatMaxD];
    __shared__ __align__(16) int8_t tile[4][64][RC + 16];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr uint32_t flip = SIGNED ? 0u : 0x80u;
    constexpr int8_t qpad = (METRIC == kFlatIP && !SIGNED) ? (int8_t)-128 : (int8_t)0;
    for (int d = tid; d < Dp; d += 256) qv[d] = d < D ? (int8_t)(queries[(size_t)q * D + d] ^ flip) : qpad;
    const int ci = blockIdx.x * 256 + tid;
    int row = -1;
    if (ci < n_cand) row = flat_candidate_row(cand[(size_t)q * n_cand + ci], n, id_offset, map, n_map, flag);
    __syncthreads();
    int acc = 0;
    const int lj = (lane & 7) * 16;
    for (int d0 = 0; d0 < Dp; d0 += RC) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int cc = it * 8 + (lane >> 3);
            const int rr = __shfl(row, cc);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (rr >= 0 && d0 + lj < Dp) v = *reinterpret_cast<const uint4*>(base + (size_t)rr * Dp + d0 + lj);
            *reinterpret_cast<uint4*>(&tile[w][cc][lj]) = v;
        }
        __syncthreads();
        const int dc = min(RC, Dp - d0);
        for (int d = 0; d < dc; d += 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(&tile[w][lane][d]);
            const uint4 u = *reinterpret_cast<const uint4*>(&qv[d0 + d]);
            acc += pair4<METRIC, SIGNED>(v.x, u.x) + pair4<METRIC, SIGNED>(v.y, u.y) + pair4<METRIC, SIGNED>(v.z, u.z) +
                   pair4<METRIC, SIGNED>(v.w, u.w);
        }
        __syncthreads();
    }
    if (ci < n_pad)
        keys[(size_t)q * n_pad + ci] =
            row >= 0 ? ((uint64_t)key_word_i32<METRIC>(acc) << 32) | (uint32_t)((int64_t)row + id_offset) : kFlatNoKey;
}

}  // namespace

hipError_t launch_flat_u8_prepare(const uint8_t* d_in, int64_t rows, int D, int Dp, int8_t* d_out, int32_t* d_norms,
                                  hipStream_t stream, bool is_signed) {
    if (rows <= 0) return hipSuccess;
    const int64_t words = rows * (Dp >> 2);
    auto* pad = is_signed ? flat_u8_bias_rows_kernel<false> : flat_u8_bias_rows_kernel<true>;
    pad<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream>>>(d_in, rows, D, Dp, d_out);
    flat_u8_norms_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream>>>(d_out, rows, Dp, d_norms);
    return hipGetLastError();
}

hipError_t launch_flat_u8_sums(const int8_t* d_rows8, int64_t rows, int Dp, int add, int32_t* d_sums, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    flat_u8_sums_kernel<<<dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream>>>(d_rows8, rows, Dp, add, d_sums);
    return hipGetLastError();
}

namespace {

// b's per-row and q's per-query terms of the epilogue: the norms (L2), the correction sums (inner product, unsigned
// rows), or nothing (inner product, signed rows).
template <bool LIST, int MODE, int METRIC, bool CORR>
void dist_u8(const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys, int cap, const int64_t* offs,
             FlatQueryState* state, hipStream_t stream) {
    const int32_t* vterm = METRIC == kFlatL2 ? b.norm : CORR ? b.rsum : nullptr;
    const int32_t* qterm = METRIC == kFlatL2 ? q.norm : CORR ? q.sum : nullptr;
    flat_dist_u8_kernel<LIST, MODE, METRIC, CORR><<<dim3((rows + UV - 1) / UV, (q.nq + UQ - 1) / UQ), dim3(256), 0, stream>>>(
        static_cast<const int8_t*>(b.rows), vterm, b.list, e0, rows, b.Dp, q.i8, qterm, q.nq, b.id_offset, keys, cap, offs, state);
}

template <int METRIC, bool CORR>
auto pick_dist_u8(bool filtered, int mode) {
    return filtered ? (mode == kFlatTopK    ? dist_u8<true, kFlatTopK, METRIC, CORR>
                       : mode == kFlatCount ? dist_u8<true, kFlatCount, METRIC, CORR>
                                            : dist_u8<true, kFlatEmit, METRIC, CORR>)
                    : (mode == kFlatTopK    ? dist_u8<false, kFlatTopK, METRIC, CORR>
                       : mode == kFlatCount ? dist_u8<false, kFlatCount, METRIC, CORR>
                                            : dist_u8<false, kFlatEmit, METRIC, CORR>);
}

}  // namespace

hipError_t launch_flat_dist_u8(int mode, const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys,
                               int cap, const int64_t* offs, FlatQueryState* state, hipStream_t stream) {
    auto* launch = b.metric != kFlatIP   ? pick_dist_u8<kFlatL2, true>(b.filtered, mode)
                   : b.format == kFlatI8 ? pick_dist_u8<kFlatIP, false>(b.filtered, mode)
                                         : pick_dist_u8<kFlatIP, true>(b.filtered, mode);
    launch(b, e0, rows, q, keys, cap, offs, state, stream);
    return hipGetLastError();
}

void launch_flat_rerank_chunk_u8(const FlatBase& b, const FlatRerank& r, int n_pad, hipStream_t stream) {
    const bool is_signed = b.format == kFlatI8;
    auto* kernel = b.metric == kFlatIP ? (is_signed ? flat_rerank_u8_kernel<kFlatIP, true> : flat_rerank_u8_kernel<kFlatIP, false>)
                                       : (is_signed ? flat_rerank_u8_kernel<kFlatL2, true> : flat_rerank_u8_kernel<kFlatL2, false>);
    kernel<<<dim3((n_pad + 255) / 256, r.nq), dim3(256), 0, stream>>>(
        static_cast<const int8_t*>(b.rows), b.n, b.D, b.Dp, static_cast<const uint8_t*>(r.queries), r.cand, r.n_cand, n_pad,
        b.id_offset, r.map, r.n_map, r.keys, r.flag);
}

}  // namespace dpq
