// dpq_flat_bits.hip -- exact Hamming distances between packed binary queries and packed binary base vectors on gfx950
// (include/deltapq_amd.h, "binary vectors").
//
// A row is D bits, dimension d in bit d & 7 of byte d >> 3.  A stored row (and a prepared query) is the caller's
// (D + 7) / 8 bytes with the spare bits of the last byte cleared, padded with zero bytes to a multiple of 16 bytes
// (flat_bits_row_bytes): whole 16-byte loads, and zero against zero XORs to zero, so the padding adds nothing.  The
// distance is the population count of row XOR query, an integer of at most 4096; the key's high word is the fp32 bits of
// that integer, which order as unsigned integers, as in dpq_flat_u8.hip.  There are no norms.
//
//   flat_bits_prepare_kernel     the caller's bytes [rows][(D + 7) / 8] -> masked, padded rows; rows and queries alike
//   flat_bits_from_float_kernel  fp32 rows and thresholds -> packed bits, bit d = v[d] > t[d]: a wavefront takes 64
//                                dimensions of one row, one coalesced load per lane, and its ballot is the 64 bits; a
//                                lane then stores a whole output word (or, where the caller's row length is no multiple
//                                of four, whole bytes) built in registers: no byte is written twice or read back
//   flat_dist_bits_kernel<LIST, MODE, CW, BQ>
//                                the one Hamming distance kernel, for every search.  A workgroup takes BQ queries x 256
//                                entries of a stripe; a lane owns one entry and holds CW words of its row in VGPRs,
//                                loaded as 16-byte loads straight from the row, against BQ accumulators, one per query.
//                                The query tile is the same for every lane: its words are read through wavefront-uniform
//                                addresses (scalar loads into SGPRs), so a pair costs a v_xor_b32 with a scalar operand
//                                and a v_bcnt_u32_b32 that adds into the accumulator.  CW = 32 (rows of whole 128 bytes)
//                                or 4 (any other row length).  BQ = 32 where a launch has more than 256 tiles of 256
//                                entries x 64 queries, one per compute unit (a range pass over a large base): the rows
//                                are read once per 32 queries.  BQ = 16 otherwise, which is every stripe of a top-k
//                                search (the stripe driver sizes stripe x batch to 256 such tiles): four workgroups per
//                                compute unit, so that a SIMD has four wavefronts to hide the scalar loads behind.  (64
//                                accumulators made the compiler spill 130 - 270 SGPRs into VGPR lanes; 32 spill none.)
//                                Nothing else is picked at run time.  The keys are treated
//                                as flat_dist_kernel / flat_dist_u8_kernel treat them: the same row sources (LIST), the
//                                same modes, the same threshold / counter / overflow protocol (dpq_flat.hip's header);
//                                since a lane has one key per query, the places of a wavefront's keys come from a ballot
//                                instead of LDS atomics.
//   flat_rerank_bits_kernel      a lane per candidate: the query, masked and padded, is staged in LDS and read as
//                                broadcasts, the lane walks its own row with 16-byte loads.
// State, selection, the final sort, the stripe driver and the re-rank launcher are dpq_flat.hip's; launch_flat_dist_bits
// and launch_flat_rerank_chunk_bits are the two ways in.
#include "dpq_flat.h"

#include <algorithm>

namespace dpq {
namespace {

constexpr int BV = 256;  // entries of a workgroup's tile: one per lane

// one thread per four output bytes (out_stride is a multiple of four)
__global__ __launch_bounds__(256) void flat_bits_prepare_kernel(const uint8_t* __restrict__ in, int64_t rows, int D,
                                                                uint8_t* __restrict__ out, int out_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = out_stride >> 2, nb = (D + 7) >> 3;
    if (i >= rows * wpr) return;
    const int64_t r = i / wpr;
    const int j = (int)(i - r * wpr) * 4;
    const uint32_t last = (D & 7) ? (1u << (D & 7)) - 1u : 0xffu;  // the bits of the last byte that are dimensions
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (j + b < nb) w |= ((uint32_t)in[r * nb + j + b] & (j + b == nb - 1 ? last : 0xffu)) << (8 * b);
    *reinterpret_cast<uint32_t*>(out + r * out_stride + j) = w;
}

// 256 threads; a wavefront per unit of 64 dimensions (8 output bytes) of one row, grid-stride over rows * units.
// out_stride >= (D + 7) / 8; bytes past the row's last dimension are written as zero.
__global__ __launch_bounds__(256) void flat_bits_from_float_kernel(const float* __restrict__ in, int64_t rows, int D,
                                                                   const float* __restrict__ thr, uint8_t* __restrict__ out,
                                                                   int out_stride) {
    const int lane = threadIdx.x & 63;
    const int units = (out_stride + 7) >> 3;
    const int64_t total = rows * units, step = (int64_t)gridDim.x * 4;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < total; u += step) {
        const int64_t r = u / units;
        const int j = (int)(u - r * units);  // the unit of the row
        const int d = 64 * j + lane;
        bool bit = false;
        if (d < D) bit = in[r * D + d] > (thr ? thr[d] : 0.0f);  // false for a NaN on either side
        const uint64_t m = __ballot(bit);
        uint8_t* o = out + r * out_stride + 8 * j;
        if ((out_stride & 3) == 0) {
            if (lane < 2 && 8 * j + 4 * lane < out_stride) *reinterpret_cast<uint32_t*>(o + 4 * lane) = (uint32_t)(m >> (32 * lane));
        } else {
            if (lane < 8 && 8 * j + lane < out_stride) o[lane] = (uint8_t)(m >> (8 * lane));
        }
    }
}

// grid (tiles of the stripe's `rows` entries, query tiles), 256 threads.  Lane tid owns entry b0 + tid of the stripe: row
// l0 + entry (LIST false), or row list[l0 + entry] (LIST true) -- a register, not LDS, since no other lane needs it.
// Wp: 32-bit words of a stored row and of a prepared query, a multiple of CW.  BQ (16 or 32): queries of the workgroup's
// tile, an accumulator each; acc[j]: the distance to query q0 + j.
// The query buffer holds whole tiles: queries past nq are read, whatever they are, and masked in the epilogue, as entries
// past the stripe are, which read a row that exists.
template <bool LIST, int MODE, int CW, int BQ>
__global__ __launch_bounds__(256) void flat_dist_bits_kernel(const uint32_t* __restrict__ base, const uint32_t* __restrict__ list,
                                                             int64_t l0, int rows, int Wp, const uint32_t* __restrict__ queries,
                                                             int nq, int64_t id_offset, uint64_t* __restrict__ keys, int cap,
                                                             const int64_t* __restrict__ offs, FlatQueryState* state) {
    __shared__ uint32_t wcnt[4][BQ];  // keys of wavefront w that pass for query j; then where its run starts
    __shared__ uint64_t thr[BQ];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b0 = blockIdx.x * BV, q0 = blockIdx.y * BQ;
    const bool inside = b0 + tid < rows;
    int64_t row;
    if constexpr (LIST) row = inside ? list[l0 + b0 + tid] : list[l0];  // past the stripe: a row that exists, masked below
    else row = l0 + (inside ? b0 + tid : 0);
    if (tid < BQ) thr[tid] = q0 + tid < nq ? state[q0 + tid].thr : 0;

    uint32_t acc[BQ];
#pragma unroll
    for (int j = 0; j < BQ; ++j) acc[j] = 0;
    const uint32_t* rp = base + (size_t)row * Wp;
    const int q_last = nq - 1 - q0;  // tile queries above it do not exist
    // one copy of the BQ x CW body, which is most of the kernel's code: no unrolling, no interleaving of two chunks
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int c0 = 0; c0 < Wp; c0 += CW) {
        uint32_t v[CW];
#pragma unroll
        for (int i = 0; i < CW; i += 4) {
            const uint4 t = *reinterpret_cast<const uint4*>(rp + c0 + i);
            v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
        }
        // the same addresses in every lane; stepped from query to query, so that no BQ row offsets stay live over the loop
        const uint32_t* qp = queries + (size_t)q0 * Wp + c0;
#pragma unroll
        for (int j = 0; j < BQ; ++j) {
#pragma unroll
            for (int i = 0; i < CW; ++i) acc[j] += __builtin_popcount(v[i] ^ qp[i]);
            qp += Wp;
        }
    }
    __syncthreads();  // thr

    // A distance is a non-negative integer, so the fp32 bits of two distances order as the distances do and key <= thr
    // is (bits, id) <= (thr >> 32, thr & 0xffffffff).
    const uint32_t id = (uint32_t)(id_offset + row);
    auto passes = [&](int j) {
        const uint32_t thi = (uint32_t)(thr[j] >> 32), tlo = (uint32_t)thr[j];
        const uint32_t b = __float_as_uint(__int2float_rn((int)acc[j]));
        if (!inside || j > q_last) return false;
        if (MODE != kFlatTopK) return b < thi;  // the radius key's id half is zero
        return b < thi || (b == thi && id <= tlo);
    };
    // first pass: lane j of a wavefront keeps how many of the wavefront's 64 entries pass for query j
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < BQ; ++j) {
        const uint32_t np = (uint32_t)__popcll(__ballot(passes(j)));
        if (lane == j) mine = np;
    }
    if (lane < BQ) wcnt[w][lane] = mine;
    __syncthreads();
    if (tid < BQ) {
        const uint32_t c[4] = {wcnt[0][tid], wcnt[1][tid], wcnt[2][tid], wcnt[3][tid]};
        const uint32_t total = c[0] + c[1] + c[2] + c[3];
        uint32_t pos = total ? atomicAdd(&state[q0 + tid].count, total) : 0u;  // total is zero for a query past nq
        if (MODE != kFlatCount) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wcnt[k][tid] = pos;
                pos += c[k];
            }
        }
    }
    if (MODE == kFlatCount) return;
    __syncthreads();
    const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
    for (int j = 0; j < BQ; ++j) {
        const bool p = passes(j);
        const uint64_t m = __ballot(p);
        if (!p) continue;
        const uint32_t pos = wcnt[w][j] + (uint32_t)__popcll(m & below);
        uint32_t room;
        uint64_t* out = flat_sink_of<MODE>(keys, cap, offs, q0 + j, &room);
        if (pos < room)
            out[pos] = ((uint64_t)__float_as_uint(__int2float_rn((int)acc[j])) << 32) | id;
        else
            state[q0 + j].overflow = 1;
    }
}

// grid (candidate groups of 256, queries), 256 threads: lane = candidate.  queries: the caller's bytes [nq][(D + 7) / 8],
// staged as the rows are stored.  Wp: words of a stored row, a multiple of four.
__global__ __launch_bounds__(256) void flat_rerank_bits_kernel(const uint32_t* __restrict__ base, int64_t n, int D, int Wp,
                                                               const uint8_t* __restrict__ queries,
                                                               const int32_t* __restrict__ cand, int n_cand, int n_pad,
                                                               int64_t id_offset, const uint32_t* __restrict__ map,
                                                               int64_t n_map, uint64_t* __restrict__ keys, uint32_t* flag) {
    __shared__ __align__(16) uint32_t qv[kFlatBitsMaxD / 32];
    const int q = blockIdx.y, tid = threadIdx.x;
    const int nb = (D + 7) >> 3;
    const uint32_t last = (D & 7) ? (1u << (D & 7)) - 1u : 0xffu;
    if (tid < Wp) {
        uint32_t wd = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * tid + b;
            if (j < nb) wd |= ((uint32_t)queries[(size_t)q * nb + j] & (j == nb - 1 ? last : 0xffu)) << (8 * b);
        }
        qv[tid] = wd;
    }
    const int ci = blockIdx.x * 256 + tid;
    int row = -1;
    if (ci < n_cand) row = flat_candidate_row(cand[(size_t)q * n_cand + ci], n, id_offset, map, n_map, flag);
    __syncthreads();
    uint32_t acc = 0;
    if (row >= 0) {
        const uint32_t* rp = base + (size_t)row * Wp;
        for (int c = 0; c < Wp; c += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(rp + c);
            const uint4 u = *reinterpret_cast<const uint4*>(&qv[c]);
            acc += __builtin_popcount(v.x ^ u.x) + __builtin_popcount(v.y ^ u.y) + __builtin_popcount(v.z ^ u.z) +
                   __builtin_popcount(v.w ^ u.w);
        }
    }
    if (ci < n_pad)
        keys[(size_t)q * n_pad + ci] = row >= 0 ? ((uint64_t)__float_as_uint(__int2float_rn((int)acc)) << 32) |
                                                      (uint32_t)((int64_t)row + id_offset)
                                                : kFlatNoKey;
}

template <bool LIST, int MODE, int CW, int BQ>
void dist_bits(const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys, int cap, const int64_t* offs,
               FlatQueryState* state, hipStream_t stream) {
    flat_dist_bits_kernel<LIST, MODE, CW, BQ><<<dim3((rows + BV - 1) / BV, (q.nq + BQ - 1) / BQ), dim3(256), 0, stream>>>(
        static_cast<const uint32_t*>(b.rows), b.list, e0, rows, b.Dp >> 2, reinterpret_cast<const uint32_t*>(q.bits), q.nq,
        b.id_offset, keys, cap, offs, state);
}

// wide: the 32-query tile.  A top-k stripe never has the workgroups for it (above), so it has no such instantiation.
template <int CW>
auto* pick_dist_bits(bool filtered, int mode, bool wide) {
    if (wide && mode != kFlatTopK)
        return filtered ? (mode == kFlatCount ? dist_bits<true, kFlatCount, CW, 32> : dist_bits<true, kFlatEmit, CW, 32>)
                        : (mode == kFlatCount ? dist_bits<false, kFlatCount, CW, 32> : dist_bits<false, kFlatEmit, CW, 32>);
    return filtered ? (mode == kFlatTopK    ? dist_bits<true, kFlatTopK, CW, 16>
                       : mode == kFlatCount ? dist_bits<true, kFlatCount, CW, 16>
                                            : dist_bits<true, kFlatEmit, CW, 16>)
                    : (mode == kFlatTopK    ? dist_bits<false, kFlatTopK, CW, 16>
                       : mode == kFlatCount ? dist_bits<false, kFlatCount, CW, 16>
                                            : dist_bits<false, kFlatEmit, CW, 16>);
}

}  // namespace

hipError_t launch_flat_bits_prepare(const uint8_t* d_in, int64_t rows, int D, uint8_t* d_out, int out_stride,
                                    hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (out_stride != flat_bits_row_bytes(D)) return hipErrorInvalidValue;
    const int64_t words = rows * (out_stride >> 2);
    flat_bits_prepare_kernel<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream>>>(d_in, rows, D, d_out, out_stride);
    return hipGetLastError();
}

hipError_t launch_flat_bits_from_float(const float* d_in, int64_t rows, int D, const float* d_thr, uint8_t* d_out,
                                       int out_stride, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (out_stride < (D + 7) / 8) return hipErrorInvalidValue;
    const int64_t units = rows * ((out_stride + 7) >> 3);
    flat_bits_from_float_kernel<<<dim3((unsigned)std::min<int64_t>((units + 3) / 4, 16384)), dim3(256), 0, stream>>>(
        d_in, rows, D, d_thr, d_out, out_stride);
    return hipGetLastError();
}

hipError_t launch_flat_dist_bits(int mode, const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys,
                                 int cap, const int64_t* offs, FlatQueryState* state, hipStream_t stream) {
    if (b.Dp != flat_bits_row_bytes(b.D) || !q.bits || b.metric != kFlatL2) return hipErrorInvalidValue;
    // more than one tile of 256 entries x 64 queries per compute unit of an MI355X: the 32-query form
    const bool wide = (int64_t)((rows + BV - 1) / BV) * ((q.nq + 63) / 64) > 256;
    auto* launch = b.Dp % 128 == 0 ? pick_dist_bits<32>(b.filtered, mode, wide) : pick_dist_bits<4>(b.filtered, mode, wide);
    launch(b, e0, rows, q, keys, cap, offs, state, stream);
    return hipGetLastError();
}

void launch_flat_rerank_chunk_bits(const FlatBase& b, const FlatRerank& r, int n_pad, hipStream_t stream) {
    flat_rerank_bits_kernel<<<dim3((n_pad + 255) / 256, r.nq), dim3(256), 0, stream>>>(
        static_cast<const uint32_t*>(b.rows), b.n, b.D, b.Dp >> 2, static_cast<const uint8_t*>(r.queries), r.cand, r.n_cand,
        n_pad, b.id_offset, r.map, r.n_map, r.keys, r.flag);
}

}  // namespace dpq
