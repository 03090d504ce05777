// dpq_flat_ivf_bits.hip -- the inverted-list scan over packed binary rows on gfx950: exact Hamming
// distances of binary queries to the rows of the lists they probe, over a dpq_flat_open_bits handle's own rows.  The
// arithmetic is dpq_flat_bits.hip's: rows and queries are words of 32 dimensions, spare bits and padding zero, the
// distance is the population count of row XOR query, an integer of at most 4096, and the key's high word is the fp32 bits
// of that integer.  There are no norms and nothing is rounded.
//
//   flat_ivf_scan_bits_kernel<CW>
//       a workgroup of 256 per run of G consecutive SORTED pairs (dpq_flat_ivf.hip's outer shape: the same pairs, the
//       same stretches of equal list, the same tiles of 256 row numbers, the same key sink -- dpq_flat_ivf_device.h).
//       A lane owns ONE row of a tile.  Its row number is a register, not LDS: no other lane needs it, which also
//       spares the two barriers around a staged tile.  The row's words come CW at a time into VGPRs, 16-byte loads
//       straight from global memory through the row number; rows never pass through LDS.  CW = 32 for rows of whole
//       128 bytes, 4 for any other length, as in flat_dist_bits_kernel.  A slot beyond the list's end loads nothing
//       and appends nothing.
//       The stretch's queries (16 at most) are the same for every lane.  Their numbers come out of LDS, so each is
//       made provably uniform (readfirstlane) once per stretch and kept as a word offset in an SGPR; a query's words
//       are then read through wavefront-uniform addresses, scalar loads into SGPRs, and a (row, query) pair of words
//       costs one v_xor_b32 with a scalar operand and one v_bcnt_u32_b32 that adds into the accumulator.  One
//       accumulator per query of the stretch.  The inner product of the chunk with the queries exists in three
//       sizes, 4, 8 and 16 queries, picked per stretch by its length: a stretch of three queries pays for four, not
//       for sixteen.  The slots of the picked size beyond the stretch repeat its last query and are never appended.
//       A lane has at most one key per pair per tile, so the places of a wavefront's keys in the pair's buffer come
//       from a ballot and ONE LDS atomic per wavefront on the pair's count; the sink's invariants (cap, the counts,
//       the thresholds) are the ones the fp32 and the byte scan keep.
#include "dpq_flat_ivf.h"

#include <algorithm>
#include <atomic>

#include "dpq_flat.h"
#include "dpq_flat_ivf_device.h"
#include "dpq_ivf.h"

namespace dpq {
namespace {

constexpr int TR = kFlatIvfTileRows, GM = kFlatIvfGroupMax;
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kStaticBytes = 512;  // the run's words below, rounded up

static_assert(TR == 256 && GM == 16, "a tile is one row per lane; a stretch is at most 16 accumulators");

// acc[j] += the distance of the lane's CW-word chunks to query j, j < NQ.  rp: the lane's row (ok: it exists).  qoff[j]:
// the word offset of query j in `queries`, the same in every lane.  One copy of the NQ x CW body per size: no unrolling
// of the chunk loop, as in flat_dist_bits_kernel.
template <int CW, int NQ>
__device__ __forceinline__ void bits_tile(const uint32_t* __restrict__ rp, bool ok, int Wp, const uint32_t* __restrict__ queries,
                                          const uint32_t (&qoff)[GM], uint32_t (&acc)[GM]) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int c0 = 0; c0 < Wp; c0 += CW) {
        uint32_t v[CW];
#pragma unroll
        for (int i = 0; i < CW; ++i) v[i] = 0u;
        if (ok) {
#pragma unroll
            for (int i = 0; i < CW; i += 4) {
                const uint4 t = *reinterpret_cast<const uint4*>(rp + c0 + i);
                v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
            }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const uint32_t* qp = queries + qoff[j] + c0;  // a uniform address: scalar loads
#pragma unroll
            for (int i = 0; i < CW; ++i) acc[j] += __builtin_popcount(v[i] ^ qp[i]);
        }
    }
}

// grid: the runs; 256 threads; dynamic LDS: G buffers of cap = 2 P2 keys.  Wp: words of a stored row and of a prepared
// query, a multiple of CW.  nq * Wp < 2^32 (a slice holds at most kIvfSliceQueries queries of at most 128 words).
// FILTERED (fbits: the filter's bitmap over the rows): a tile is the next up to 256 eligible rows, compacted into 256
// row-number slots in front of the buffers (dpq_flat_ivf_device.h's fill_tile); a lane takes its row number from its slot.
template <int CW, bool FILTERED, int SINK>
__global__ __launch_bounds__(256) void flat_ivf_scan_bits_kernel(const uint32_t* __restrict__ rows, int Wp, int64_t id_offset,
                                                                 const int64_t* __restrict__ offsets,
                                                                 const uint32_t* __restrict__ list_rows, int nlist,
                                                                 const uint32_t* __restrict__ queries, int nq, int nprobe,
                                                                 const uint32_t* __restrict__ skeys,
                                                                 const uint32_t* __restrict__ svals, int64_t n_pairs, int G,
                                                                 int top_k, int cap, int32_t* __restrict__ part_ids,
                                                                 float* __restrict__ part_dists,
                                                                 const uint32_t* __restrict__ fbits,
                                                                 [[maybe_unused]] SinkArgs<SINK> sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned char flat_ivf_bits_smem[];
    [[maybe_unused]] uint32_t* s_rows = reinterpret_cast<uint32_t*>(flat_ivf_bits_smem);           // [TR], FILTERED only
    uint64_t* buf = reinterpret_cast<uint64_t*>(flat_ivf_bits_smem + (FILTERED ? TR * 4 : 0));  // [G][cap]
    __shared__ uint32_t s_key[GM], s_val[GM], s_q[GM], s_cnt[GM];
    __shared__ uint64_t s_thr[GM];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    [[maybe_unused]] RangeLds* rl = nullptr;
    const int64_t p0 = (int64_t)blockIdx.x * G;
    const int np = (int)min((int64_t)G, n_pairs - p0);
    if (tid < GM) {
        const uint32_t val = tid < np ? svals[p0 + tid] : 0u;
        s_key[tid] = tid < np ? skeys[p0 + tid] : (uint32_t)nlist;
        s_val[tid] = val;
        s_q[tid] = val / (uint32_t)nprobe;
    }
    __syncthreads();
    // Everything the workgroup branches on below is read from LDS behind a barrier, or from one global address: the
    // stretches, the list bounds and the buffer counts are the same in every thread.
    for (int s = 0; s < np;) {
        const uint32_t list = s_key[s];
        int e = s + 1;
        while (e < np && s_key[e] == list) ++e;
        int nqs = e - s;  // queries of the stretch: pairs s .. e - 1, at most GM
        if constexpr (SINK != kSinkTopK) {  // the thresholds; emit: only the pairs with hits stay -- maybe a smaller form
            __shared__ RangeLds s_range;
            rl = &s_range;
            nqs = range_begin<SINK>(sink.r, s_val, s_q, s_cnt, s_thr, s_range, s, nqs, tid);
            if (nqs == 0) {  // (emit only) nothing of the list is read
                s = e;
                continue;
            }
        }
        int64_t lo = 0, hi = 0;
        if (list < (uint32_t)nlist) {
            lo = offsets[list];
            hi = offsets[list + 1];
        }
        if constexpr (SINK == kSinkTopK)
            if (tid < nqs) {
                s_cnt[tid] = 0u;
                s_thr[tid] = kFlatNoKey;
            }
        [[maybe_unused]] uint32_t hits[GM];  // count: this lane's passing keys per query, over the stretch
#pragma unroll
        for (int j = 0; j < GM; ++j) hits[j] = 0u;
        uint32_t qoff[GM];  // SGPRs: slots beyond the stretch repeat its last query
#pragma unroll
        for (int j = 0; j < GM; ++j)
            qoff[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_q[s + min(j, nqs - 1)]) * (uint32_t)Wp;
        for (int64_t base = lo; base < hi; base += FILTERED ? 0 : TR) {
            __syncthreads();  // the counts and thresholds: the stretch's first, or what sink_make_room left
            bool ok;
            uint32_t row;
            if constexpr (FILTERED) {  // base moves to where the next tile starts; every lane has read its slot before
                const int got = fill_tile(s_rows, list_rows, base, hi, fbits, tid);  // the tile's closing barrier
                if (got == 0) break;  // the list ended on no eligible row
                ok = tid < got;
                row = ok ? s_rows[tid] : 0u;
            } else {
                ok = base + tid < hi;
                row = ok ? list_rows[base + tid] : 0u;
            }
            const uint32_t* rp = rows + (size_t)row * Wp;
            uint32_t acc[GM];
#pragma unroll
            for (int j = 0; j < GM; ++j) acc[j] = 0u;
            if (nqs <= 4) bits_tile<CW, 4>(rp, ok, Wp, queries, qoff, acc);
            else if (nqs <= 8) bits_tile<CW, 8>(rp, ok, Wp, queries, qoff, acc);
            else bits_tile<CW, 16>(rp, ok, Wp, queries, qoff, acc);
            const uint32_t id = (uint32_t)(id_offset + (int64_t)row);
#pragma unroll
            for (int j = 0; j < GM; ++j) {
                const uint64_t key = ((uint64_t)__float_as_uint(__int2float_rn((int)acc[j])) << 32) | id;
                const bool p = j < nqs && ok && key < s_thr[j];
                if constexpr (SINK == kSinkCount) {
                    hits[j] += p ? 1u : 0u;
                    continue;
                }
                const uint64_t m = __ballot(p);
                if (m != 0) {
                    const int first = __ffsll((unsigned long long)m) - 1;
                    uint32_t at = 0u;
                    if (lane == first) at = atomicAdd(&s_cnt[j], (uint32_t)__popcll(m));
                    at = (uint32_t)__shfl((int)at, first) + (uint32_t)__popcll(m & below);
                    if constexpr (SINK == kSinkTopK) {
                        if (p) buf[(size_t)j * cap + at] = key;  // < cap: the tile had room for its 256 rows
                    } else {
                        const int64_t to = rl->off[j] + (int64_t)at;
                        if (p && to >= 0 && to < sink.r.pool_n) sink.r.pool[to] = key;
                    }
                }
            }
            if constexpr (SINK == kSinkTopK) {  // (the range sinks need no barrier of their own between two tiles)
                __syncthreads();
                if (base + (FILTERED ? 0 : TR) < hi) sink_make_room(buf, s_cnt, s_thr, nqs, cap, top_k, tid);
            }
        }
        if constexpr (SINK != kSinkTopK) {
            if constexpr (SINK == kSinkCount) {
                if (hi > lo)
#pragma unroll
                    for (int j = 0; j < GM; ++j) {
                        const uint32_t c = wave_sum(hits[j]);
                        if (lane == 0 && j < nqs) atomicAdd(&s_cnt[j], c);
                    }
                range_counts_out(sink.r, s_val, s_cnt, s, nqs, hi > lo, tid);
            }
            __syncthreads();  // the next stretch starts the counts over
            s = e;
            continue;
        }
        if (hi > lo) sink_sort(buf, s_cnt, nqs, cap, tid);  // (behind the last tile's closing barrier)
        // the stretch's answers: pair i = q * nprobe + j goes to row j * nq + q.  A padding pair, or an empty list: padding
        for (int p = 0; p < nqs; ++p) {
            const uint32_t q = s_q[s + p], j = s_val[s + p] - q * (uint32_t)nprobe;
            int32_t* out_i = part_ids + ((size_t)j * nq + q) * top_k;
            float* out_d = part_dists + ((size_t)j * nq + q) * top_k;
            sink_emit(buf + (size_t)p * cap, hi > lo ? s_cnt[p] : 0u, top_k, out_i, out_d, tid);
        }
        __syncthreads();  // the next stretch starts the counts and the buffers over
        s = e;
    }
}

// hipFuncSetAttribute is per device
hipError_t ensure_scan_lds() {
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        for (const void* k : {reinterpret_cast<const void*>(&flat_ivf_scan_bits_kernel<32, false, kSinkTopK>),
                              reinterpret_cast<const void*>(&flat_ivf_scan_bits_kernel<4, false, kSinkTopK>),
                              reinterpret_cast<const void*>(&flat_ivf_scan_bits_kernel<32, true, kSinkTopK>),
                              reinterpret_cast<const void*>(&flat_ivf_scan_bits_kernel<4, true, kSinkTopK>)}) {
            e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBytes - kStaticBytes));
            if (e != hipSuccess) return e;
        }
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

int flat_ivf_group_bits(int top_k, int /*Wp*/, int group) {
    const size_t per = (size_t)scan_cap(top_k) * sizeof(uint64_t);
    int g = GM;
    while (g > 1 && (g > group || (size_t)g * per + kStaticBytes > kLdsBytes)) g >>= 1;
    return g;
}

hipError_t launch_flat_ivf_scan_bits(const FlatIvfListsBits& L, const uint32_t* d_queries, int nq, int nprobe,
                                     const uint32_t* d_skeys, const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids,
                                     float* d_part_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!L.rows || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !d_part_ids || !d_part_dists || L.Wp < 4 ||
        L.Wp % 4 != 0 || L.Wp * 4 > flat_bits_row_bytes(kFlatBitsMaxD) || L.nlist < 1 || L.nlist > kIvfMaxLists || nprobe < 1 ||
        nprobe > kIvfMaxProbe || top_k < 1 || top_k > kIvfMaxTopK || group < 1 || (int64_t)nq * nprobe > 0x7fffffff ||
        (int64_t)nq * L.Wp > 0xffffffffll ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    if (hipError_t e = ensure_scan_lds()) return e;
    const int cap = scan_cap(top_k), G = flat_ivf_group_bits(top_k, L.Wp, group);
    const int64_t n_pairs = (int64_t)nq * nprobe;
    // the filtered scan's 256 row-number slots never cost a pair: a group's buffers are a power of two of at most 128 KB
    const size_t lds = (L.filter ? (size_t)TR * 4 : 0) + (size_t)G * cap * sizeof(uint64_t);
    if (lds + kStaticBytes > kLdsBytes) return hipErrorInvalidValue;
    auto* kernel = L.Wp % 32 == 0 ? flat_ivf_scan_bits_kernel<32, false, kSinkTopK> : flat_ivf_scan_bits_kernel<4, false, kSinkTopK>;
    if (L.filter) kernel = L.Wp % 32 == 0 ? flat_ivf_scan_bits_kernel<32, true, kSinkTopK> : flat_ivf_scan_bits_kernel<4, true, kSinkTopK>;
    kernel<<<dim3((unsigned)((n_pairs + G - 1) / G)), dim3(256), lds, stream>>>(L.rows, L.Wp, L.id_offset, L.offsets, L.list_rows,
                                                                                 L.nlist, d_queries, nq, nprobe, d_skeys, d_svals,
                                                                                 n_pairs, G, top_k, cap, d_part_ids, d_part_dists,
                                                                                 L.filter, {});
    return hipGetLastError();
}

// The range sinks: the only dynamic LDS is a filtered scan's 256 row-number slots.
template <int SINK>
hipError_t launch_range(const FlatIvfListsBits& L, const uint32_t* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                        const uint32_t* d_svals, int G, const FlatIvfRange& r, hipStream_t stream) {
    const int64_t n_pairs = (int64_t)nq * nprobe;
    auto* kernel = L.Wp % 32 == 0 ? flat_ivf_scan_bits_kernel<32, false, SINK> : flat_ivf_scan_bits_kernel<4, false, SINK>;
    if (L.filter) kernel = L.Wp % 32 == 0 ? flat_ivf_scan_bits_kernel<32, true, SINK> : flat_ivf_scan_bits_kernel<4, true, SINK>;
    kernel<<<dim3((unsigned)((n_pairs + G - 1) / G)), dim3(256), L.filter ? (size_t)TR * 4 : 0, stream>>>(
        L.rows, L.Wp, L.id_offset, L.offsets, L.list_rows, L.nlist, d_queries, nq, nprobe, d_skeys, d_svals, n_pairs, G, 0, 0, nullptr,
        nullptr, L.filter, {r});
    return hipGetLastError();
}

hipError_t launch_flat_ivf_range_bits(const FlatIvfListsBits& L, const uint32_t* d_queries, int nq, int nprobe,
                                      const uint32_t* d_skeys, const uint32_t* d_svals, int group, const FlatIvfRange& r,
                                      hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!L.rows || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !r.thr || !r.counts ||
        (r.pool && (!r.offs || r.pool_n < 1 || r.qa < 0 || r.qa >= r.qb || r.qb > nq)) || L.Wp < 4 || L.Wp % 4 != 0 ||
        L.Wp * 4 > flat_bits_row_bytes(kFlatBitsMaxD) || L.nlist < 1 || L.nlist > kIvfMaxLists || nprobe < 1 ||
        nprobe > kIvfMaxProbe || group < 1 || (int64_t)nq * nprobe > 0x7fffffff || (int64_t)nq * L.Wp > 0xffffffffll ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const int G = flat_ivf_range_group(group);
    return r.pool ? launch_range<kSinkEmit>(L, d_queries, nq, nprobe, d_skeys, d_svals, G, r, stream)
                  : launch_range<kSinkCount>(L, d_queries, nq, nprobe, d_skeys, d_svals, G, r, stream);
}

}  // namespace dpq
