// dpq_flat_ivf.hip -- the inverted-list scan over raw fp32 rows on gfx950: exact distances of the
// queries to the rows of the lists they probe.  The arithmetic is the exact search's (dpq_flat.h): per dimension in
// ascending order t = v[d] - q[d] and s = t * t, each rounded in fp32, summed on one lane's fp64 accumulator from +0.0,
// rounded once.  The build passes -ffp-contract=off and keeps clear of the packed fp32 instructions.
//
//   flat_ivf_pairs_kernel  a thread per (query, probe): the pair's sort key, its list or nlist for padding.
//   flat_ivf_scan_kernel   a workgroup of 256 per run of G consecutive SORTED pairs.  The pairs of a list are neighbours, so
//                          a run is a few stretches of equal list; the workgroup takes them in turn and reads a list's rows
//                          once for all the queries of its stretch.  Per tile of 256 rows: the row numbers go to LDS
//                          once; then, in slices of 32 dimensions, the rows (gathered through the row numbers, eight
//                          lanes to a row's 128 bytes) and the stretch's queries go to LDS transposed -- Rs[d][row]
//                          with a stride of 260, Qs[d][query] -- while the next slice's rows are already on their way
//                          in registers.  Lane (tx, ty) owns rows 4 tx .. 4 tx + 3 and queries QPL ty .. QPL ty + QPL - 1
//                          (QPL = 4 at G = 16): its rows come as one 16-byte LDS read per dimension, its queries as a
//                          broadcast, and each of its 4 QPL fp64 accumulators runs from the first dimension to the
//                          last.  Behind the last slice a key below its pair's threshold is appended to the pair's
//                          buffer of 2 P2 keys by an LDS atomic on the pair's count.  When a buffer could overflow on
//                          the next tile, the buffers of the stretch are sorted side by side (one bitonic network, the
//                          same barriers for all), cut to top_k, and the thresholds become the k-th keys
//                          (dpq_flat_ivf_device.h: the sink is shared with the byte scan, dpq_flat_ivf_u8.hip).
#include "dpq_flat_ivf.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>

#include "dpq_flat.h"
#include "dpq_flat_ivf_device.h"
#include "dpq_ivf.h"

namespace dpq {
namespace {

constexpr int TR = kFlatIvfTileRows, SD = kFlatIvfSliceDims, GM = kFlatIvfGroupMax;
constexpr int RS = TR + 4;  // floats between two dimensions of the row tile: 16-byte reads stay aligned, and the eight
                            // 4-dimension columns a wavefront stores at once start 16 banks apart
constexpr size_t kTileBytes = (size_t)SD * RS * 4 + (size_t)SD * GM * 4 + (size_t)TR * 4;  // rows, queries, row numbers
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kStaticBytes = 512;  // the run's words below, rounded up

__global__ __launch_bounds__(256) void flat_ivf_pairs_kernel(const int32_t* __restrict__ probes, int64_t n, int nlist,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t l = probes[i];
    keys[i] = (l >= 0 && l < nlist) ? (uint32_t)l : (uint32_t)nlist;
    vals[i] = (uint32_t)i;
}

// The rows' part of slice d0 for this thread: float4 c of row r = idx >> 3, idx = tid + 256 i.  A row beyond the list's
// end and a column beyond the last dimension give zeros (neither is read by the sum).
__device__ __forceinline__ void load_slice(float4 (&pre)[8], const float* __restrict__ rows, int Dp, const uint32_t* s_rows,
                                           int d0, int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + 256 * i, r = idx >> 3, c = idx & 7;
        const uint32_t row = s_rows[r];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row != kNoRow && d0 + 4 * c < Dp) v = *reinterpret_cast<const float4*>(rows + (size_t)row * Dp + d0 + 4 * c);
        pre[i] = v;
    }
}

// grid: the runs; 256 threads; dynamic LDS: the tiles, then G buffers of cap = 2 P2 keys.
// SINK (dpq_flat_ivf_device.h): kSinkTopK as described above; kSinkCount / kSinkEmit, the passes of a range search, take
// `sink.r`, keep no buffers (top_k, cap and the outputs are unused) and share every line of the distance loop.
template <int QPL, bool FILTERED, int METRIC, int SINK>
__global__ __launch_bounds__(256) void flat_ivf_scan_kernel(const float* __restrict__ rows, int Dp, int64_t id_offset,
                                                            const int64_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ list_rows, int nlist,
                                                            const float* __restrict__ queries, int nq, int nprobe,
                                                            const uint32_t* __restrict__ skeys,
                                                            const uint32_t* __restrict__ svals, int64_t n_pairs, int G,
                                                            int top_k, int cap, int32_t* __restrict__ part_ids,
                                                            float* __restrict__ part_dists,
                                                            const uint32_t* __restrict__ fbits,
                                                            [[maybe_unused]] SinkArgs<SINK> sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned char flat_ivf_smem[];
    float* Rs = reinterpret_cast<float*>(flat_ivf_smem);          // [SD][RS]
    float* Qs = Rs + SD * RS;                                     // [SD][GM]
    uint32_t* s_rows = reinterpret_cast<uint32_t*>(Qs + SD * GM);  // [TR]
    uint64_t* buf = reinterpret_cast<uint64_t*>(s_rows + TR);      // [G][cap]
    __shared__ uint32_t s_key[GM], s_val[GM], s_q[GM], s_cnt[GM];
    __shared__ uint64_t s_thr[GM];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
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
        int nqs = e - s;  // queries of the stretch: pairs s .. e - 1
        if constexpr (SINK != kSinkTopK) {  // the thresholds; emit: only the pairs with hits stay, compacted
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
        [[maybe_unused]] uint32_t hits[QPL];  // count: this lane's passing keys per query it owns, over the stretch
#pragma unroll
        for (int i = 0; i < QPL; ++i) hits[i] = 0u;
        const bool active = QPL * ty < nqs;  // (a wavefront's lanes share ty)
        for (int64_t base = lo; base < hi; base += FILTERED ? 0 : TR) {
            __syncthreads();  // the tile before is done with s_rows; the first tile: the counts above are in place
            if constexpr (FILTERED) {  // the next up to 256 eligible rows; base moves to where the next tile starts
                if (fill_tile(s_rows, list_rows, base, hi, fbits, tid) == 0) break;  // the list ended on no eligible row
            } else {
                s_rows[tid] = base + tid < hi ? list_rows[base + tid] : kNoRow;
                __syncthreads();
            }
            double acc[QPL][4];
#pragma unroll
            for (int i = 0; i < QPL; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
            float4 pre[8];
            load_slice(pre, rows, Dp, s_rows, 0, tid);
            for (int d0 = 0; d0 < Dp; d0 += SD) {
                const int dlen = min(SD, Dp - d0);  // a multiple of four
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int idx = tid + 256 * i, r = idx >> 3, c = idx & 7;
                    if (4 * c < dlen) {
                        Rs[(4 * c + 0) * RS + r] = pre[i].x;
                        Rs[(4 * c + 1) * RS + r] = pre[i].y;
                        Rs[(4 * c + 2) * RS + r] = pre[i].z;
                        Rs[(4 * c + 3) * RS + r] = pre[i].w;
                    }
                }
#pragma unroll
                for (int i = 0; i < SD * GM / 256; ++i) {
                    const int idx = tid + 256 * i, qs = idx >> 5, d = idx & 31;
                    float v = 0.f;
                    if (qs < nqs && d < dlen) v = queries[(size_t)s_q[s + qs] * Dp + d0 + d];
                    Qs[d * GM + qs] = v;
                }
                __syncthreads();
                if (d0 + SD < Dp) load_slice(pre, rows, Dp, s_rows, d0 + SD, tid);  // in flight under the sums below
                if (active) {
#pragma unroll 4
                    for (int d = 0; d < dlen; ++d) {
                        const float4 v = *reinterpret_cast<const float4*>(&Rs[d * RS + 4 * tx]);
                        float q[QPL];
                        if constexpr (QPL == 4) {
                            const float4 w = *reinterpret_cast<const float4*>(&Qs[d * GM + 4 * ty]);
                            q[0] = w.x; q[1] = w.y; q[2] = w.z; q[3] = w.w;
                        } else if constexpr (QPL == 2) {
                            const float2 w = *reinterpret_cast<const float2*>(&Qs[d * GM + 2 * ty]);
                            q[0] = w.x; q[1] = w.y;
                        } else {
                            q[0] = Qs[d * GM + ty];
                        }
#pragma unroll
                        for (int i = 0; i < QPL; ++i) {
                            accumulate<METRIC>(acc[i][0], v.x, q[i]);
                            accumulate<METRIC>(acc[i][1], v.y, q[i]);
                            accumulate<METRIC>(acc[i][2], v.z, q[i]);
                            accumulate<METRIC>(acc[i][3], v.w, q[i]);
                        }
                    }
                }
                __syncthreads();
            }
            if (active) {
#pragma unroll
                for (int i = 0; i < QPL; ++i) {
                    const int qs = QPL * ty + i;
                    if (qs >= nqs) continue;
                    const uint64_t thr = s_thr[qs];
                    uint64_t* b = buf + (size_t)qs * cap;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t row = s_rows[4 * tx + j];
                        if (row == kNoRow) continue;
                        const uint64_t key = make_key<METRIC>(acc[i][j], (uint32_t)(id_offset + (int64_t)row));
                        if (key >= thr) continue;
                        if constexpr (SINK == kSinkTopK) b[atomicAdd(&s_cnt[qs], 1u)] = key;  // < cap: the tile had room for its 256 rows
                        else if constexpr (SINK == kSinkCount) ++hits[i];
                        else range_put(sink.r, *rl, s_cnt, qs, key);
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
                if (active && hi > lo)  // (a wavefront's lanes share their queries)
#pragma unroll
                    for (int i = 0; i < QPL; ++i) {
                        const uint32_t c = wave_sum(hits[i]);
                        if (tx == 0 && QPL * ty + i < nqs) atomicAdd(&s_cnt[QPL * ty + i], c);
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
template <int QPL, bool FILTERED, int METRIC, int SINK>
hipError_t ensure_scan_lds() {
    if constexpr (SINK != kSinkTopK) return hipSuccess;  // the range sinks' tiles fit the default 64 KB
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flat_ivf_scan_kernel<QPL, FILTERED, METRIC, SINK>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBytes - kStaticBytes));
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

// The range sinks (sink.r) take no buffers: top_k, cap and the outputs are 0 / NULL.
template <int QPL, bool FILTERED, int METRIC, int SINK>
hipError_t launch_scan(const FlatIvfLists& L, const float* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                       const uint32_t* d_svals, int64_t n_pairs, int G, int top_k, int cap, int32_t* d_part_ids,
                       float* d_part_dists, const SinkArgs<SINK>& sink, hipStream_t stream) {
    if (hipError_t e = ensure_scan_lds<QPL, FILTERED, METRIC, SINK>()) return e;
    const size_t lds = kTileBytes + (SINK == kSinkTopK ? (size_t)G * cap * sizeof(uint64_t) : 0);
    const dim3 grid((unsigned)((n_pairs + G - 1) / G)), block(256);
    flat_ivf_scan_kernel<QPL, FILTERED, METRIC, SINK><<<grid, block, lds, stream>>>(
        L.rows, L.Dp, L.id_offset, L.offsets, L.list_rows, L.nlist, d_queries, nq, nprobe, d_skeys, d_svals, n_pairs, G, top_k, cap,
        d_part_ids, d_part_dists, L.filter, sink);
    return hipGetLastError();
}

// The instantiation for a group, a filter and a metric.
template <int SINK>
auto* scan_of(const FlatIvfLists& L, int G) {
    auto* launch = G == 16 ? launch_scan<4, false, kFlatL2, SINK> : G == 8 ? launch_scan<2, false, kFlatL2, SINK> : launch_scan<1, false, kFlatL2, SINK>;
    if (L.filter) launch = G == 16 ? launch_scan<4, true, kFlatL2, SINK> : G == 8 ? launch_scan<2, true, kFlatL2, SINK> : launch_scan<1, true, kFlatL2, SINK>;
    if (L.metric == kFlatIP) {
        launch = G == 16 ? launch_scan<4, false, kFlatIP, SINK> : G == 8 ? launch_scan<2, false, kFlatIP, SINK> : launch_scan<1, false, kFlatIP, SINK>;
        if (L.filter) launch = G == 16 ? launch_scan<4, true, kFlatIP, SINK> : G == 8 ? launch_scan<2, true, kFlatIP, SINK> : launch_scan<1, true, kFlatIP, SINK>;
    }
    return launch;
}

bool range_ok(const FlatIvfRange& r, int nq) {
    return r.thr && r.counts && (!r.pool || (r.offs && r.pool_n > 0 && r.qa >= 0 && r.qa < r.qb && r.qb <= nq));
}

// a thread per entry of the merged answer: the key word back to the score's bits, padding to -inf
__global__ __launch_bounds__(256) void flat_ivf_ip_scores_kernel(const int32_t* __restrict__ ids, float* __restrict__ vals, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    vals[i] = ids[i] < 0 ? -INFINITY : __uint_as_float(flat_ip_word(__float_as_uint(vals[i])));
}

int key_bits(int nlist) {
    int bits = 1;  // keys are 0 .. nlist
    while ((1u << bits) <= (uint32_t)nlist) ++bits;
    return bits;
}

}  // namespace

int flat_ivf_group(int top_k, int group) {
    const size_t per = (size_t)scan_cap(top_k) * sizeof(uint64_t);
    int g = GM;
    while (g > 1 && (g > group || kTileBytes + (size_t)g * per + kStaticBytes > kLdsBytes)) g >>= 1;
    return g;
}

hipError_t launch_flat_ivf_pairs(const int32_t* d_probes, int64_t n_pairs, int nlist, uint32_t* d_keys, uint32_t* d_vals,
                                 hipStream_t stream) {
    if (n_pairs <= 0) return hipSuccess;
    if (!d_probes || !d_keys || !d_vals || nlist < 1 || nlist > kIvfMaxLists || n_pairs > 0x7fffffff) return hipErrorInvalidValue;
    flat_ivf_pairs_kernel<<<dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream>>>(d_probes, n_pairs, nlist, d_keys,
                                                                                               d_vals);
    return hipGetLastError();
}

hipError_t flat_ivf_sort_pairs(void* d_temp, size_t* temp_bytes, const uint32_t* d_keys, uint32_t* d_keys_out,
                               const uint32_t* d_vals, uint32_t* d_vals_out, int64_t n_pairs, int nlist, hipStream_t stream) {
    if (!temp_bytes || nlist < 1 || nlist > kIvfMaxLists || n_pairs < 1 || n_pairs > 0x7fffffff) return hipErrorInvalidValue;
    size_t need = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, d_keys, d_keys_out, d_vals, d_vals_out, (int)n_pairs, 0,
                                                      key_bits(nlist), stream);
    if (e != hipSuccess) return e;
    if (!d_temp) {
        *temp_bytes = need;
        return hipSuccess;
    }
    if (*temp_bytes < need) return hipErrorInvalidValue;
    size_t tb = *temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(d_temp, tb, d_keys, d_keys_out, d_vals, d_vals_out, (int)n_pairs, 0, key_bits(nlist),
                                              stream);
}

hipError_t launch_flat_ivf_ip_scores(const int32_t* d_ids, float* d_vals, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_ids || !d_vals) return hipErrorInvalidValue;
    flat_ivf_ip_scores_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(d_ids, d_vals, n);
    return hipGetLastError();
}

hipError_t launch_flat_ivf_scan(const FlatIvfLists& L, const float* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                                const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids, float* d_part_dists,
                                hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!L.rows || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !d_part_ids || !d_part_dists ||
        L.Dp < 4 || L.Dp % 4 != 0 || L.Dp > kFlatMaxD || L.nlist < 1 || L.nlist > kIvfMaxLists || nprobe < 1 ||
        nprobe > kIvfMaxProbe || top_k < 1 || top_k > kIvfMaxTopK || group < 1 || (int64_t)nq * nprobe > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const int cap = scan_cap(top_k), G = flat_ivf_group(top_k, group);
    const int64_t n_pairs = (int64_t)nq * nprobe;
    return scan_of<kSinkTopK>(L, G)(L, d_queries, nq, nprobe, d_skeys, d_svals, n_pairs, G, top_k, cap, d_part_ids, d_part_dists, {},
                                    stream);
}

int flat_ivf_range_group(int group) {
    int g = GM;
    while (g > 1 && g > group) g >>= 1;
    return g;
}

hipError_t launch_flat_ivf_range(const FlatIvfLists& L, const float* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                                 const uint32_t* d_svals, int group, const FlatIvfRange& range, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!L.rows || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !range_ok(range, nq) || L.Dp < 4 ||
        L.Dp % 4 != 0 || L.Dp > kFlatMaxD || L.nlist < 1 || L.nlist > kIvfMaxLists || nprobe < 1 || nprobe > kIvfMaxProbe ||
        group < 1 || (int64_t)nq * nprobe > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const int G = flat_ivf_range_group(group);
    const int64_t n_pairs = (int64_t)nq * nprobe;
    if (!range.pool)
        return scan_of<kSinkCount>(L, G)(L, d_queries, nq, nprobe, d_skeys, d_svals, n_pairs, G, 0, 0, nullptr, nullptr, {range}, stream);
    return scan_of<kSinkEmit>(L, G)(L, d_queries, nq, nprobe, d_skeys, d_svals, n_pairs, G, 0, 0, nullptr, nullptr, {range}, stream);
}

}  // namespace dpq
