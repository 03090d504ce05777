// dpq_flat_ivf_u8.hip -- the inverted-list scan over byte rows on the int8 matrix cores of gfx950: exact
// squared L2 distances of byte queries to the rows of the lists they probe, over a dpq_flat_open_u8 / _i8 handle's own rows.
// The arithmetic is dpq_flat_u8.hip's: rows and queries are int8 (unsigned data biased by 128, which no difference sees),
// padded with int8 zeros, with their int32 norms beside them, and
//     |v - q|^2 = |v'|^2 + |q'|^2 - 2 v'.q'      all in int32, exact whatever the order of the sum,
// reported as (float)(int32), one round-to-nearest-even conversion.
//
//   flat_ivf_widen_kernel    bytes -> fp32 rows padded with zeros: the caller's values (0..255 or -128..127), from raw
//                            bytes or from a handle's stored (biased) rows.  Feeds the coarse step and the label build.
//   flat_ivf_scan_u8_kernel  a workgroup of 256 per run of G consecutive SORTED pairs (dpq_flat_ivf.hip's outer shape: the
//                            same pairs, the same stretches of equal list, the same tiles of 256 staged row numbers, the
//                            same key sink -- dpq_flat_ivf_device.h).  A stretch holds at most 16 queries: they are the
//                            N = 16 side of v_mfma_i32_16x16x64_i8, staged ONCE per stretch as Qs[16][Dp + 16] int8, slots
//                            beyond the stretch zero; the 16 spare bytes stagger the 16 query rows' 16-byte reads over the
//                            banks.  Wavefront w owns rows 64 w .. 64 w + 63 of a tile as four blocks of 16.  In K step
//                            k0 (64 bytes) lane l feeds, on the A side, bytes k0 + 16 (l >> 4) .. + 15 of row
//                            s_rows[64 w + 16 i + (l & 15)] of block i -- one 16-byte load straight from global memory
//                            through the row number, four lanes to a row's 64 contiguous bytes, the next step's four
//                            operands loaded before the current step's MFMAs issue -- and, on the B side, the same bytes
//                            of query row l & 15 from LDS, one read for the step's four MFMAs.  Both sides put the same
//                            bytes of K into the same lane positions, so a dot product does not depend on how the
//                            instruction numbers K.  Rows are padded to 32 bytes, not 64: in the last step of a
//                            Dp % 64 == 32 row the lanes with l >> 4 >= 2 feed zeros on both sides and load nothing.  A
//                            row slot beyond the list's end feeds zeros and loads nothing.  Register e of lane l in block
//                            i is row 16 i + 4 (l >> 4) + e against query l & 15 (the C/D map of the 16x16 shapes): the
//                            epilogue adds the norms, converts, and appends the key where it is below the pair's threshold.
#include "dpq_flat_ivf.h"

#include <algorithm>
#include <atomic>

#include "dpq_flat.h"
#include "dpq_flat_ivf_device.h"
#include "dpq_ivf.h"

namespace dpq {
namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int TR = kFlatIvfTileRows, GM = kFlatIvfGroupMax;
constexpr int KS = 64;   // bytes of a row one v_mfma_i32_16x16x64_i8 consumes
constexpr int QPAD = 16;  // spare bytes behind a staged query row
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kStaticBytes = 512;  // the run's words below, rounded up

static_assert(TR == 256 && GM == 16, "a tile is four wavefronts of four 16-row blocks; a stretch is the MFMA's N side");

size_t tile_bytes(int Dp) { return (size_t)GM * (Dp + QPAD) + (size_t)TR * 4; }  // queries, row numbers

// one thread per value of the output [rows][Dp].  in: [rows][in_stride] bytes, the first D of a row valid; a byte b
// stands for (int8)b when is_signed, else for (uint8)(b ^ flip) -- flip 0x80 undoes a stored unsigned row's bias.
__global__ __launch_bounds__(256) void flat_ivf_widen_kernel(const uint8_t* __restrict__ in, int64_t rows, int D, int in_stride,
                                                             int Dp, uint32_t flip, bool is_signed, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * Dp) return;
    const int64_t r = i / Dp;
    const int d = (int)(i - r * Dp);
    float v = 0.0f;
    if (d < D) {
        const uint8_t b = in[r * in_stride + d];
        v = is_signed ? (float)(int)(int8_t)b : (float)(int)(uint8_t)(b ^ flip);
    }
    out[i] = v;
}

// grid: the runs; 256 threads; dynamic LDS: the queries, the row numbers, then G buffers of cap = 2 P2 keys.
// METRIC kFlatIP: the score is the int32 S of dpq_flat_u8.hip's header -- the int8 dot product, plus, for unsigned rows (CORR),
// rs[row] + qs[query], which come in the place of the norms (vnorm, qnorm); without CORR neither array is read.  The key
// word is flat_ip_word of the converted score's bits.  kFlatL2 always has CORR: its norms.
template <bool FILTERED, int METRIC, bool CORR, int SINK>
__global__ __launch_bounds__(256) void flat_ivf_scan_u8_kernel(const int8_t* __restrict__ rows, const int32_t* __restrict__ vnorm,
                                                               int Dp, int64_t id_offset, const int64_t* __restrict__ offsets,
                                                               const uint32_t* __restrict__ list_rows, int nlist,
                                                               const int8_t* __restrict__ queries,
                                                               const int32_t* __restrict__ qnorm, int nq, int nprobe,
                                                               const uint32_t* __restrict__ skeys,
                                                               const uint32_t* __restrict__ svals, int64_t n_pairs, int G,
                                                               int top_k, int cap, int32_t* __restrict__ part_ids,
                                                               float* __restrict__ part_dists,
                                                               const uint32_t* __restrict__ fbits,
                                                               [[maybe_unused]] SinkArgs<SINK> sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned char flat_ivf_u8_smem[];
    const int QS = Dp + QPAD;                                                          // bytes between two query rows
    int8_t* Qs = reinterpret_cast<int8_t*>(flat_ivf_u8_smem);                          // [GM][QS]
    uint32_t* s_rows = reinterpret_cast<uint32_t*>(flat_ivf_u8_smem + (size_t)GM * QS);  // [TR]
    uint64_t* buf = reinterpret_cast<uint64_t*>(s_rows + TR);                          // [G][cap]
    __shared__ uint32_t s_key[GM], s_val[GM], s_q[GM], s_cnt[GM];
    __shared__ int32_t s_qn[GM];
    __shared__ uint64_t s_thr[GM];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, h = lane >> 4;
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
    const i32x4 zero = {0, 0, 0, 0};
    const int cpr = Dp >> 4;  // 16-byte chunks of a row
    // Everything the workgroup branches on below is read from LDS behind a barrier, or from one global address: the
    // stretches, the list bounds and the buffer counts are the same in every thread.
    for (int s = 0; s < np;) {
        const uint32_t list = s_key[s];
        int e = s + 1;
        while (e < np && s_key[e] == list) ++e;
        int nqs = e - s;  // queries of the stretch: pairs s .. e - 1, at most GM
        if constexpr (SINK != kSinkTopK) {  // the thresholds; emit: only the pairs with hits stay -- a shorter N side
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
        if (tid < nqs) {
            if constexpr (SINK == kSinkTopK) {
                s_cnt[tid] = 0u;
                s_thr[tid] = kFlatNoKey;
            }
            s_qn[tid] = CORR ? qnorm[s_q[s + tid]] : 0;
        }
        [[maybe_unused]] uint32_t hits = 0u;  // count: this lane's passing keys for query r, over the stretch
        if (hi > lo)  // the stretch's queries, once for all its tiles (the first tile's barriers publish them)
            for (int idx = tid; idx < GM * cpr; idx += 256) {
                const int slot = idx / cpr, c = idx - slot * cpr;
                i32x4 v = zero;
                if (slot < nqs) v = *reinterpret_cast<const i32x4*>(queries + (size_t)s_q[s + slot] * Dp + 16 * c);
                *reinterpret_cast<i32x4*>(Qs + slot * QS + 16 * c) = v;
            }
        for (int64_t base = lo; base < hi; base += FILTERED ? 0 : TR) {
            __syncthreads();  // the tile before is done with s_rows; the first tile: the counts and queries above are in place
            if constexpr (FILTERED) {  // the next up to 256 eligible rows; base moves to where the next tile starts
                if (fill_tile(s_rows, list_rows, base, hi, fbits, tid) == 0) break;  // the list ended on no eligible row
            } else {
                s_rows[tid] = base + tid < hi ? list_rows[base + tid] : kNoRow;
                __syncthreads();
            }
            const int8_t* ap[4];
            bool aok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t row = s_rows[64 * w + 16 * i + r];
                aok[i] = row != kNoRow;
                ap[i] = rows + (size_t)(aok[i] ? row : 0u) * Dp + 16 * h;
            }
            // the norms of the four rows of each block this lane's registers stand for: in flight under the K loop
            int vn[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t row = s_rows[64 * w + 16 * i + 4 * h + c];
                    vn[i][c] = CORR && row != kNoRow ? vnorm[row] : 0;
                }
            const int8_t* bp = Qs + r * QS + 16 * h;
            i32x4 acc[4], nxt[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i] = zero;
                nxt[i] = aok[i] && 16 * h < Dp ? *reinterpret_cast<const i32x4*>(ap[i]) : zero;
            }
            for (int k0 = 0; k0 < Dp; k0 += KS) {
                i32x4 a[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = nxt[i];
                const bool kn = k0 + KS + 16 * h < Dp;  // this lane's bytes of the next step exist
#pragma unroll
                for (int i = 0; i < 4; ++i) nxt[i] = aok[i] && kn ? *reinterpret_cast<const i32x4*>(ap[i] + k0 + KS) : zero;
                const i32x4 b = k0 + 16 * h < Dp ? *reinterpret_cast<const i32x4*>(bp + k0) : zero;
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b, acc[i], 0, 0, 0);
            }
            if (r < nqs) {
                const uint64_t thr = s_thr[r];
                const int qn = s_qn[r];
                uint64_t* b = buf + (size_t)r * cap;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const uint32_t row = s_rows[64 * w + 16 * i + 4 * h + c];
                        if (row == kNoRow) continue;
                        const int d = METRIC == kFlatIP ? acc[i][c] + vn[i][c] + qn : vn[i][c] + qn - 2 * acc[i][c];
                        const uint32_t u = __float_as_uint(__int2float_rn(d));
                        const uint64_t key = ((uint64_t)(METRIC == kFlatIP ? flat_ip_word(u) : u) << 32) | (uint32_t)(id_offset + (int64_t)row);
                        if (key >= thr) continue;
                        if constexpr (SINK == kSinkTopK) b[atomicAdd(&s_cnt[r], 1u)] = key;  // < cap: the tile had room for its 256 rows
                        else if constexpr (SINK == kSinkCount) ++hits;
                        else range_put(sink.r, *rl, s_cnt, r, key);
                    }
            }
            if constexpr (SINK == kSinkTopK) {  // (the range sinks need no barrier of their own between two tiles)
                __syncthreads();
                if (base + (FILTERED ? 0 : TR) < hi) sink_make_room(buf, s_cnt, s_thr, nqs, cap, top_k, tid);
            }
        }
        if constexpr (SINK != kSinkTopK) {
            if constexpr (SINK == kSinkCount) {  // the four lanes of a wavefront that share query r, then one atomic
                uint32_t c = hits;
                c += (uint32_t)__shfl_xor((int)c, 16);
                c += (uint32_t)__shfl_xor((int)c, 32);
                if (h == 0 && r < nqs && hi > lo) atomicAdd(&s_cnt[r], c);
                range_counts_out(sink.r, s_val, s_cnt, s, nqs, hi > lo, tid);
            }
            __syncthreads();  // the next stretch starts the counts and the queries over
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
        __syncthreads();  // the next stretch starts the counts, the queries and the buffers over
        s = e;
    }
}

// hipFuncSetAttribute is per device
template <bool FILTERED, int METRIC, bool CORR, int SINK>
hipError_t ensure_scan_lds() {
    if constexpr (SINK != kSinkTopK) return hipSuccess;  // the range sinks' tiles fit the default 64 KB
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flat_ivf_scan_u8_kernel<FILTERED, METRIC, CORR, SINK>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBytes - kStaticBytes));
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

struct ScanArgs {
    const int8_t* queries;
    const int32_t* qterm;
    int nq, nprobe;
    const uint32_t *skeys, *svals;
    int G, top_k;
    int32_t* part_ids;
    float* part_dists;
    hipStream_t stream;
    const FlatIvfRange* range = nullptr;  // the range sinks: top_k 0, no outputs
};

template <bool FILTERED, int METRIC, bool CORR, int SINK>
hipError_t launch_scan(const FlatIvfListsU8& L, const ScanArgs& a) {
    if (hipError_t e = ensure_scan_lds<FILTERED, METRIC, CORR, SINK>()) return e;
    const int cap = SINK == kSinkTopK ? scan_cap(a.top_k) : 0;
    const int64_t n_pairs = (int64_t)a.nq * a.nprobe;
    const size_t lds = tile_bytes(L.Dp) + (size_t)a.G * cap * sizeof(uint64_t);
    SinkArgs<SINK> sink;
    if constexpr (SINK != kSinkTopK) sink.r = *a.range;
    flat_ivf_scan_u8_kernel<FILTERED, METRIC, CORR, SINK><<<dim3((unsigned)((n_pairs + a.G - 1) / a.G)), dim3(256), lds, a.stream>>>(
        L.rows, L.norm, L.Dp, L.id_offset, L.offsets, L.list_rows, L.nlist, a.queries, a.qterm, a.nq, a.nprobe, a.skeys, a.svals,
        n_pairs, a.G, a.top_k, cap, a.part_ids, a.part_dists, L.filter, sink);
    return hipGetLastError();
}

template <int SINK>
hipError_t launch_scan_of(const FlatIvfListsU8& L, const ScanArgs& a) {
    if (L.metric == kFlatIP) {
        if (L.norm) return L.filter ? launch_scan<true, kFlatIP, true, SINK>(L, a) : launch_scan<false, kFlatIP, true, SINK>(L, a);
        return L.filter ? launch_scan<true, kFlatIP, false, SINK>(L, a) : launch_scan<false, kFlatIP, false, SINK>(L, a);
    }
    return L.filter ? launch_scan<true, kFlatL2, true, SINK>(L, a) : launch_scan<false, kFlatL2, true, SINK>(L, a);
}

}  // namespace

int flat_ivf_group_u8(int top_k, int Dp, int group) {
    const size_t per = (size_t)scan_cap(top_k) * sizeof(uint64_t);
    int g = GM;
    while (g > 1 && (g > group || tile_bytes(Dp) + (size_t)g * per + kStaticBytes > kLdsBytes)) g >>= 1;
    return g;
}

hipError_t launch_flat_ivf_widen(const void* d_in, int64_t rows, int D, int in_stride, int Dp, bool stored, bool is_signed,
                                 float* d_out, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!d_in || !d_out || D < 1 || D > in_stride || D > Dp) return hipErrorInvalidValue;
    const int64_t total = rows * Dp;
    flat_ivf_widen_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(
        static_cast<const uint8_t*>(d_in), rows, D, in_stride, Dp, stored && !is_signed ? 0x80u : 0u, is_signed, d_out);
    return hipGetLastError();
}

hipError_t launch_flat_ivf_scan_u8(const FlatIvfListsU8& L, const int8_t* d_queries, const int32_t* d_qnorm, int nq, int nprobe,
                                   const uint32_t* d_skeys, const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids,
                                   float* d_part_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const bool terms = L.metric != kFlatIP || L.norm || d_qnorm;  // signed rows under kFlatIP take neither array
    if (L.metric != kFlatL2 && L.metric != kFlatIP) return hipErrorInvalidValue;
    if (!L.rows || (terms && (!L.norm || !d_qnorm)) || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !d_part_ids ||
        !d_part_dists || L.Dp < kFlatU8KStep || L.Dp % kFlatU8KStep != 0 || L.Dp > kFlatMaxD || L.nlist < 1 ||
        L.nlist > kIvfMaxLists || nprobe < 1 || nprobe > kIvfMaxProbe || top_k < 1 || top_k > kIvfMaxTopK || group < 1 ||
        (int64_t)nq * nprobe > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const ScanArgs a{d_queries, d_qnorm, nq, nprobe, d_skeys, d_svals, flat_ivf_group_u8(top_k, L.Dp, group), top_k, d_part_ids,
                     d_part_dists, stream};
    return launch_scan_of<kSinkTopK>(L, a);
}

hipError_t launch_flat_ivf_range_u8(const FlatIvfListsU8& L, const int8_t* d_queries, const int32_t* d_qnorm, int nq, int nprobe,
                                    const uint32_t* d_skeys, const uint32_t* d_svals, int group, const FlatIvfRange& r,
                                    hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const bool terms = L.metric != kFlatIP || L.norm || d_qnorm;  // signed rows under kFlatIP take neither array
    if (L.metric != kFlatL2 && L.metric != kFlatIP) return hipErrorInvalidValue;
    if (!L.rows || (terms && (!L.norm || !d_qnorm)) || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !r.thr ||
        !r.counts || (r.pool && (!r.offs || r.pool_n < 1 || r.qa < 0 || r.qa >= r.qb || r.qb > nq)) || L.Dp < kFlatU8KStep ||
        L.Dp % kFlatU8KStep != 0 || L.Dp > kFlatMaxD || L.nlist < 1 || L.nlist > kIvfMaxLists || nprobe < 1 ||
        nprobe > kIvfMaxProbe || group < 1 || (int64_t)nq * nprobe > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const ScanArgs a{d_queries, d_qnorm, nq, nprobe, d_skeys, d_svals, flat_ivf_range_group(group), 0, nullptr, nullptr, stream, &r};
    return r.pool ? launch_scan_of<kSinkEmit>(L, a) : launch_scan_of<kSinkCount>(L, a);
}

}  // namespace dpq
