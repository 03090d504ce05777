// dpq_flat_ivf_narrow.hip -- the inverted-list scan over narrow rows on gfx950: fp16 and bf16 rows and 8-bit
// and 4-bit scalar-quantised rows under fp32 queries, over a dpq_flat_open_half / _narrowed / _sq / _quantised handle's own
// rows.  The answer is, bit for bit, dpq_flat_ivf.hip's over the rows widened (flat_half_widen) or decoded (flat_sq_decode)
// to fp32: per dimension in ascending order t = v[d] - q[d] and s = t * t, each rounded in fp32, summed on one lane's fp64
// accumulator from +0.0, rounded once.  The build passes -ffp-contract=off and keeps clear of the packed fp32 instructions.
//
//   flat_ivf_narrow_widen_kernel  a thread per stored word: the fp32 values of its dimensions, [rows][Dp].  Feeds the label
//                                 build (the arg-min over the centroids reads fp32 rows).
//   flat_ivf_scan_narrow_kernel   a workgroup of 256 per run of G consecutive SORTED pairs: dpq_flat_ivf.hip's outer shape --
//                                 the same pairs, the same stretches of equal list, the same tiles of 256 staged row
//                                 numbers, the same key sink (dpq_flat_ivf_device.h).  The rows stay NARROW in LDS: the
//                                 tile is Rw[w][row], words of four stored bytes (2 halves, 4 or 8 codes of one row) with
//                                 a stride of 260 words, and a slice is 16 words -- 64 stored bytes, 32 / 64 / 128
//                                 dimensions -- of every row: 16.6 KB where the fp32 scan keeps 33 KB, and at D = 128 four,
//                                 two or one barrier pairs a tile.  A lane's global load is 16 bytes through the staged
//                                 row number, four lanes to a row's 64 bytes, four loads per thread and slice, written as
//                                 four words to Rw[4 c + k][r]: a wavefront's store covers 16 consecutive rows of four
//                                 column groups that start 16 banks apart.  The next slice's loads are issued before the
//                                 current slice is summed.  The stretch's queries go to LDS transposed per slice,
//                                 Qs[d][query], in fp32, and for quantised rows the slice's (lo, step) pairs beside them.
//                                 Lane (tx, ty) owns rows 4 tx .. 4 tx + 3 and queries QPL ty .. QPL ty + QPL - 1; per
//                                 word it reads ONE 16-byte group, that word of its four rows, and turns it into 2, 4 or 8
//                                 dimensions x 4 rows of fp32 in registers (decode_word), which it runs in ascending
//                                 dimension over its queries: each of its 4 QPL fp64 accumulators goes from the first
//                                 dimension to the last.  Behind the last slice the keys go to the sink as in the fp32 scan.
#include "dpq_flat_ivf.h"

#include <algorithm>
#include <atomic>

#include "dpq_flat.h"
#include "dpq_flat_ivf_device.h"
#include "dpq_ivf.h"

namespace dpq {
namespace {

constexpr int TR = kFlatIvfTileRows, GM = kFlatIvfGroupMax;
constexpr int SW = kFlatIvfNarrowSliceWords;  // words of a row that are in LDS at a time
constexpr int RS = TR + 4;  // words between two columns of the row tile: 16-byte reads stay aligned, and the four 4-word
                            // columns a wavefront stores at once start 16 banks apart
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kStaticBytes = 512;  // the run's words below, rounded up

static_assert(TR == 256 && SW == 16, "a slice is 1024 loads of 16 bytes: four per thread, four lanes to a row");

template <int FORMAT> constexpr bool is_sq = FORMAT == kFlatSQ8 || FORMAT == kFlatSQ4;
// Dimensions a stored word holds.
template <int FORMAT> constexpr int word_dims = FORMAT == kFlatSQ4 ? 8 : FORMAT == kFlatSQ8 ? 4 : 2;
int word_dims_of(int format) { return format == kFlatSQ4 ? 8 : format == kFlatSQ8 ? 4 : 2; }

// LDS beside the buffers: the row tile, the queries of a slice, a quantised format's (lo, step) of a slice, the row numbers.
size_t tile_bytes(int format) {
    const size_t sd = (size_t)SW * word_dims_of(format);
    const bool sq = format == kFlatSQ8 || format == kFlatSQ4;
    return (size_t)SW * RS * 4 + sd * GM * 4 + (sq ? sd * sizeof(float2) : 0) + (size_t)TR * 4;
}

// One stored word -> the fp32 values of its dimensions, ascending: the low half first, byte 0 first, the low nibble of
// byte 0 first.  The arithmetic of dpq_flat.hip's widen8 / decode16: bf16 widens with a shift or a mask, fp16 with
// v_cvt_f32_f16 (the build's 16-bit denormal mode keeps subnormals), a code is converted by v_cvt_f32_ubyteN and decoded
// by flat_sq_decode under q[dimension], the word's own (lo, step).
template <int FORMAT>
__device__ __forceinline__ void decode_word(uint32_t w, [[maybe_unused]] const float2* q, float* out) {
    if constexpr (FORMAT == kFlatBF16) {
        out[0] = __uint_as_float(w << 16);
        out[1] = __uint_as_float(w & 0xffff0000u);
    } else if constexpr (FORMAT == kFlatF16) {
        union { uint16_t u; _Float16 h; } lo, hi;
        lo.u = (uint16_t)(w & 0xffffu);
        hi.u = (uint16_t)(w >> 16);
        out[0] = (float)lo.h;
        out[1] = (float)hi.h;
    } else if constexpr (FORMAT == kFlatSQ8) {
#pragma unroll
        for (int b = 0; b < 4; ++b) out[b] = flat_sq_decode((w >> (8 * b)) & 0xffu, q[b]);
    } else {
        const uint32_t even = w & 0x0f0f0f0fu, odd = (w >> 4) & 0x0f0f0f0fu;  // dimensions 0, 2, 4, 6 and 1, 3, 5, 7 as bytes
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            out[2 * b] = flat_sq_decode((even >> (8 * b)) & 0xffu, q[2 * b]);
            out[2 * b + 1] = flat_sq_decode((odd >> (8 * b)) & 0xffu, q[2 * b + 1]);
        }
    }
}

// a thread per stored word of rows r0 .. r0 + m - 1; out [m][Wr * word_dims].
template <int FORMAT>
__global__ __launch_bounds__(256) void flat_ivf_narrow_widen_kernel(const uint32_t* __restrict__ rows, int Wr, int64_t r0, int64_t m,
                                                                    float* __restrict__ out) {
    constexpr int DW = word_dims<FORMAT>;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m * Wr) return;
    const int w = (int)(i % Wr);
    float v[DW];
    decode_word<FORMAT>(rows[(size_t)r0 * Wr + i], flat_sq_quant_of(rows, Wr * DW) + w * DW, v);
#pragma unroll
    for (int k = 0; k < DW; ++k) out[i * DW + k] = v[k];
}

// The rows' part of the slice at word w0 for this thread: 16-byte group c of row r = idx >> 2, idx = tid + 256 i.  A row
// slot beyond the list's end and a column beyond the row's last word load nothing and give zeros (neither is read by the sum).
__device__ __forceinline__ void load_slice(uint4 (&pre)[4], const uint32_t* __restrict__ rows, int Wr, const uint32_t* s_rows,
                                           int w0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 2, c = idx & 3;
        const uint32_t row = s_rows[r];
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row != kNoRow && w0 + 4 * c < Wr) v = *reinterpret_cast<const uint4*>(rows + (size_t)row * Wr + w0 + 4 * c);
        pre[i] = v;
    }
}

// grid: the runs; 256 threads; dynamic LDS: the tiles, then G buffers of cap = 2 P2 keys.  Wr: the words of a stored row,
// a multiple of four.
template <int FORMAT, int QPL, bool FILTERED, int METRIC, int SINK>
__global__ __launch_bounds__(256) void flat_ivf_scan_narrow_kernel(const uint32_t* __restrict__ rows, int Wr, int64_t id_offset,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const uint32_t* __restrict__ list_rows, int nlist,
                                                                   const float* __restrict__ queries, int nq, int nprobe,
                                                                   const uint32_t* __restrict__ skeys,
                                                                   const uint32_t* __restrict__ svals, int64_t n_pairs, int G,
                                                                   int top_k, int cap, int32_t* __restrict__ part_ids,
                                                                   float* __restrict__ part_dists,
                                                                   const uint32_t* __restrict__ fbits,
                                                                   [[maybe_unused]] SinkArgs<SINK> sink) {
    constexpr int DW = word_dims<FORMAT>, SD = SW * DW;  // dimensions of a word and of a slice
    constexpr int UNR = 8 / DW;                          // words the sum is unrolled by: eight dimensions
    extern __shared__ __attribute__((aligned(16))) unsigned char flat_ivf_narrow_smem[];
    uint32_t* Rw = reinterpret_cast<uint32_t*>(flat_ivf_narrow_smem);  // [SW][RS]
    float* Qs = reinterpret_cast<float*>(Rw + SW * RS);                // [SD][GM]
    float2* Qn = reinterpret_cast<float2*>(Qs + SD * GM);              // [SD], quantised rows only
    uint32_t* s_rows = reinterpret_cast<uint32_t*>(Qn + (is_sq<FORMAT> ? SD : 0));  // [TR]
    uint64_t* buf = reinterpret_cast<uint64_t*>(s_rows + TR);                       // [G][cap]
    __shared__ uint32_t s_key[GM], s_val[GM], s_q[GM], s_cnt[GM];
    __shared__ uint64_t s_thr[GM];
    const int Dp = Wr * DW;
    [[maybe_unused]] const float2* quant = flat_sq_quant_of(rows, Dp);  // quantised rows only
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
            uint4 pre[4];
            load_slice(pre, rows, Wr, s_rows, 0, tid);
            for (int w0 = 0; w0 < Wr; w0 += SW) {
                const int wlen = min(SW, Wr - w0);  // a multiple of four
                const int d0 = w0 * DW, dlen = wlen * DW;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = tid + 256 * i, r = idx >> 2, c = idx & 3;
                    Rw[(4 * c + 0) * RS + r] = pre[i].x;
                    Rw[(4 * c + 1) * RS + r] = pre[i].y;
                    Rw[(4 * c + 2) * RS + r] = pre[i].z;
                    Rw[(4 * c + 3) * RS + r] = pre[i].w;
                }
#pragma unroll
                for (int i = 0; i < SD * GM / 256; ++i) {
                    const int idx = tid + 256 * i, qs = idx / SD, d = idx % SD;
                    float v = 0.f;
                    if (qs < nqs && d < dlen) v = queries[(size_t)s_q[s + qs] * Dp + d0 + d];
                    Qs[d * GM + qs] = v;
                }
                if constexpr (is_sq<FORMAT>)
                    if (tid < SD) Qn[tid] = tid < dlen ? quant[d0 + tid] : make_float2(0.f, 0.f);
                __syncthreads();
                if (w0 + SW < Wr) load_slice(pre, rows, Wr, s_rows, w0 + SW, tid);  // in flight under the sums below
                if (active) {
#pragma unroll UNR
                    for (int w = 0; w < wlen; ++w) {
                        const uint4 g = *reinterpret_cast<const uint4*>(&Rw[w * RS + 4 * tx]);
                        float v[4][DW];
                        decode_word<FORMAT>(g.x, Qn + w * DW, v[0]);
                        decode_word<FORMAT>(g.y, Qn + w * DW, v[1]);
                        decode_word<FORMAT>(g.z, Qn + w * DW, v[2]);
                        decode_word<FORMAT>(g.w, Qn + w * DW, v[3]);
#pragma unroll
                        for (int k = 0; k < DW; ++k) {
                            const int d = w * DW + k;
                            float q[QPL];
                            if constexpr (QPL == 4) {
                                const float4 t = *reinterpret_cast<const float4*>(&Qs[d * GM + 4 * ty]);
                                q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
                            } else if constexpr (QPL == 2) {
                                const float2 t = *reinterpret_cast<const float2*>(&Qs[d * GM + 2 * ty]);
                                q[0] = t.x; q[1] = t.y;
                            } else {
                                q[0] = Qs[d * GM + ty];
                            }
#pragma unroll
                            for (int i = 0; i < QPL; ++i) {
                                accumulate<METRIC>(acc[i][0], v[0][k], q[i]);
                                accumulate<METRIC>(acc[i][1], v[1][k], q[i]);
                                accumulate<METRIC>(acc[i][2], v[2][k], q[i]);
                                accumulate<METRIC>(acc[i][3], v[3][k], q[i]);
                            }
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
template <int FORMAT, int QPL, bool FILTERED, int METRIC, int SINK>
hipError_t ensure_scan_lds() {
    if constexpr (SINK != kSinkTopK) return hipSuccess;  // the range sinks' tiles fit the default 64 KB
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flat_ivf_scan_narrow_kernel<FORMAT, QPL, FILTERED, METRIC, SINK>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsBytes - kStaticBytes));
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

struct ScanArgs {
    const float* queries;
    int nq, nprobe;
    const uint32_t *skeys, *svals;
    int G, top_k;
    int32_t* part_ids;
    float* part_dists;
    hipStream_t stream;
    const FlatIvfRange* range = nullptr;  // the range sinks: top_k 0, no outputs
};

template <int FORMAT, int QPL, bool FILTERED, int METRIC, int SINK>
hipError_t launch_scan(const FlatIvfListsNarrow& L, const ScanArgs& a) {
    if (hipError_t e = ensure_scan_lds<FORMAT, QPL, FILTERED, METRIC, SINK>()) return e;
    const int cap = SINK == kSinkTopK ? scan_cap(a.top_k) : 0;
    const int64_t n_pairs = (int64_t)a.nq * a.nprobe;
    const size_t lds = tile_bytes(FORMAT) + (size_t)a.G * cap * sizeof(uint64_t);
    const dim3 grid((unsigned)((n_pairs + a.G - 1) / a.G)), block(256);
    SinkArgs<SINK> sink;
    if constexpr (SINK != kSinkTopK) sink.r = *a.range;
    flat_ivf_scan_narrow_kernel<FORMAT, QPL, FILTERED, METRIC, SINK><<<grid, block, lds, a.stream>>>(
        static_cast<const uint32_t*>(L.rows), L.Dp / word_dims<FORMAT>, L.id_offset, L.offsets, L.list_rows, L.nlist, a.queries,
        a.nq, a.nprobe, a.skeys, a.svals, n_pairs, a.G, a.top_k, cap, a.part_ids, a.part_dists, L.filter, sink);
    return hipGetLastError();
}

template <int FORMAT, int METRIC, int SINK>
hipError_t launch_scan_by(const FlatIvfListsNarrow& L, const ScanArgs& a) {
    if (L.filter) return a.G == 16 ? launch_scan<FORMAT, 4, true, METRIC, SINK>(L, a) : a.G == 8 ? launch_scan<FORMAT, 2, true, METRIC, SINK>(L, a)
                                                                                                : launch_scan<FORMAT, 1, true, METRIC, SINK>(L, a);
    if (a.G == 16) return launch_scan<FORMAT, 4, false, METRIC, SINK>(L, a);
    if (a.G == 8) return launch_scan<FORMAT, 2, false, METRIC, SINK>(L, a);
    return launch_scan<FORMAT, 1, false, METRIC, SINK>(L, a);
}

template <int FORMAT, int SINK>
hipError_t launch_scan_of(const FlatIvfListsNarrow& L, const ScanArgs& a) {
    return L.metric == kFlatIP ? launch_scan_by<FORMAT, kFlatIP, SINK>(L, a) : launch_scan_by<FORMAT, kFlatL2, SINK>(L, a);
}

template <int SINK>
hipError_t launch_scan_format(const FlatIvfListsNarrow& L, const ScanArgs& a) {
    if (L.format == kFlatF16) return launch_scan_of<kFlatF16, SINK>(L, a);
    if (L.format == kFlatBF16) return launch_scan_of<kFlatBF16, SINK>(L, a);
    if (L.format == kFlatSQ8) return launch_scan_of<kFlatSQ8, SINK>(L, a);
    return launch_scan_of<kFlatSQ4, SINK>(L, a);
}

bool is_narrow(int format) { return format == kFlatF16 || format == kFlatBF16 || format == kFlatSQ8 || format == kFlatSQ4; }

// Dimensions a stored row of the format is padded to a multiple of.
int pad_of(int format) { return format == kFlatSQ4 ? 32 : format == kFlatSQ8 ? 16 : 8; }

}  // namespace

int flat_ivf_group_narrow(int format, int top_k, int group) {
    const size_t per = (size_t)scan_cap(top_k) * sizeof(uint64_t);
    int g = GM;
    while (g > 1 && (g > group || tile_bytes(format) + (size_t)g * per + kStaticBytes > kLdsBytes)) g >>= 1;
    return g;
}

hipError_t launch_flat_ivf_narrow_widen(int format, const void* d_rows, int Dp, int64_t r0, int64_t rows, float* d_out,
                                        hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!is_narrow(format) || !d_rows || !d_out || r0 < 0 || Dp < pad_of(format) || Dp % pad_of(format) != 0 || Dp > kFlatMaxD)
        return hipErrorInvalidValue;
    const int Wr = Dp / word_dims_of(format);
    const uint32_t* w = static_cast<const uint32_t*>(d_rows);
    const dim3 grid((unsigned)((rows * Wr + 255) / 256)), block(256);
    if (format == kFlatF16) flat_ivf_narrow_widen_kernel<kFlatF16><<<grid, block, 0, stream>>>(w, Wr, r0, rows, d_out);
    else if (format == kFlatBF16) flat_ivf_narrow_widen_kernel<kFlatBF16><<<grid, block, 0, stream>>>(w, Wr, r0, rows, d_out);
    else if (format == kFlatSQ8) flat_ivf_narrow_widen_kernel<kFlatSQ8><<<grid, block, 0, stream>>>(w, Wr, r0, rows, d_out);
    else flat_ivf_narrow_widen_kernel<kFlatSQ4><<<grid, block, 0, stream>>>(w, Wr, r0, rows, d_out);
    return hipGetLastError();
}

hipError_t launch_flat_ivf_scan_narrow(const FlatIvfListsNarrow& L, const float* d_queries, int nq, int nprobe,
                                       const uint32_t* d_skeys, const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids,
                                       float* d_part_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!is_narrow(L.format) || !L.rows || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !d_part_ids ||
        !d_part_dists || L.Dp < pad_of(L.format) || L.Dp % pad_of(L.format) != 0 || L.Dp > kFlatMaxD || L.nlist < 1 ||
        L.nlist > kIvfMaxLists || nprobe < 1 || nprobe > kIvfMaxProbe || top_k < 1 || top_k > kIvfMaxTopK || group < 1 ||
        (int64_t)nq * nprobe > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const ScanArgs a{d_queries, nq, nprobe, d_skeys, d_svals, flat_ivf_group_narrow(L.format, top_k, group), top_k, d_part_ids,
                     d_part_dists, stream};
    return launch_scan_format<kSinkTopK>(L, a);
}

hipError_t launch_flat_ivf_range_narrow(const FlatIvfListsNarrow& L, const float* d_queries, int nq, int nprobe,
                                        const uint32_t* d_skeys, const uint32_t* d_svals, int group, const FlatIvfRange& r,
                                        hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!is_narrow(L.format) || !L.rows || !L.offsets || !L.list_rows || !d_queries || !d_skeys || !d_svals || !r.thr || !r.counts ||
        (r.pool && (!r.offs || r.pool_n < 1 || r.qa < 0 || r.qa >= r.qb || r.qb > nq)) || L.Dp < pad_of(L.format) ||
        L.Dp % pad_of(L.format) != 0 || L.Dp > kFlatMaxD || L.nlist < 1 || L.nlist > kIvfMaxLists || nprobe < 1 ||
        nprobe > kIvfMaxProbe || group < 1 || (int64_t)nq * nprobe > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(L.rows) | reinterpret_cast<uintptr_t>(d_queries)) & 15u))
        return hipErrorInvalidValue;
    const ScanArgs a{d_queries, nq, nprobe, d_skeys, d_svals, flat_ivf_range_group(group), 0, nullptr, nullptr, stream, &r};
    return r.pool ? launch_scan_format<kSinkEmit>(L, a) : launch_scan_format<kSinkCount>(L, a);
}

}  // namespace dpq
