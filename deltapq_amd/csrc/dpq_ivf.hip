// dpq_ivf.hip -- inverted lists over a handle's nodes on gfx950: their construction from labels, and
// the list scan.  The distance of an entry is what the scans give the same node: the M entries T[m][code[m]] of the
// query's exact table, summed in ascending m -- in fp64 and rounded once (a DTC handle), or in fp32 with M roundings (a
// dpq_open_plain_* handle).  The build passes -ffp-contract=off; a sum has no product to fuse anyway.
//
//   ivf_label_keys_kernel  a thread per node: the sort key of its label, its position, the count of its list.
//   ivf_ids_kernel         a thread per list entry: the id a search reports for its node.
//   ivf_gather_codes_kernel  a thread per list entry: its code from a tile of decoded codes, where its node is in it.
//   ivf_reconstruct_kernel a thread per float: the codebook's row of a decoded code (the assignment by centroids).
//   ivf_probes_kernel      a workgroup per query: its probe row with repeats and padding as -1; a flag word for an
//                          entry that names no list.
//   ivf_scan_kernel        a workgroup of 256 per (probe, query).  The query's table (M x 256 fp32) goes to LDS once with
//                          16-byte loads.  Per stride of 256 entries a lane loads its code as one 8- or 16-byte word (the
//                          stride is one coalesced access), gathers its M entries with one 4-byte LDS read each, forms the
//                          key and appends it to an LDS buffer of 2 P keys (P the power of two >= max(top_k, 256)) only
//                          if it lies below the workgroup's threshold: one ballot and one LDS count word per
//                          wavefront, one barrier per stride, no atomics.  When the buffer cannot take another stride a bitonic sort in LDS keeps the best
//                          top_k and the threshold becomes the k-th key; ids are unique inside a list, so the strict
//                          comparison loses nothing.  A last sort emits the list's top_k.
//   ivf_scan_filtered_kernel  the same scan over the entries a dpq_filter allows: the entry's bit is
//                          tested before its code is loaded.
//   ivf_range_kernel       the same grid and table load for a radius: a count pass, then an emit pass that writes every
//                          passing key at its rank inside the region the count reserved.
#include "dpq_ivf.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <type_traits>

#include "dpq_flat.h"

namespace dpq {
namespace {

__global__ __launch_bounds__(256) void ivf_label_keys_kernel(const int32_t* __restrict__ labels, int64_t n, int nlist,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ pos,
                                                             unsigned long long* counts, uint32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    uint32_t key = (uint32_t)nlist;
    if (l >= nlist)
        *flag = 1u;  // every thread that finds one stores the same word
    else if (l >= 0)
        key = (uint32_t)l;
    keys[i] = key;
    pos[i] = (uint32_t)i;
    atomicAdd(&counts[key], 1ull);
}

__global__ __launch_bounds__(256) void ivf_ids_kernel(const uint32_t* __restrict__ pos, int64_t n, const RefineIds rid,
                                                      int32_t* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ids[i] = ivf_report_id(rid.id_base + (int64_t)pos[i], rid);
}

// A thread per list entry: the entry's M code bytes from a tile of decoded codes, where its node lies in the tile.
template <int M>
__global__ __launch_bounds__(256) void ivf_gather_codes_kernel(const uint32_t* __restrict__ pos, int64_t n, int64_t l0,
                                                               int64_t l1, const uint8_t* __restrict__ tile,
                                                               uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = pos[i];
    if (l < l0 || l >= l1) return;
    if constexpr (M == 8)
        reinterpret_cast<uint2*>(out)[i] = reinterpret_cast<const uint2*>(tile)[l - l0];
    else
        reinterpret_cast<uint4*>(out)[i] = reinterpret_cast<const uint4*>(tile)[l - l0];
}

// A thread per float of a reconstructed row: codebook[m][code[m]][d]; a code byte >= K has no codeword and gives NaN.
__global__ __launch_bounds__(256) void ivf_reconstruct_kernel(const uint8_t* __restrict__ codes, int64_t n, int M, int K,
                                                              int Ds, const float* __restrict__ codebook,
                                                              float* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int D = M * Ds;
    if (at >= n * D) return;
    const int64_t i = at / D;
    const int j = (int)(at % D), m = j / Ds, d = j % Ds;
    const int c = codes[i * M + m];
    out[at] = c < K ? codebook[((size_t)m * K + c) * Ds + d] : __uint_as_float(0x7FC00000u);
}

__global__ __launch_bounds__(256) void ivf_probes_kernel(const int32_t* __restrict__ probes, int nprobe, int nlist,
                                                         int32_t* __restrict__ out, uint32_t* flag) {
    __shared__ int32_t row[kIvfMaxProbe];
    const int q = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < nprobe; j += 256) row[j] = probes[(size_t)q * nprobe + j];
    __syncthreads();
    for (int j = tid; j < nprobe; j += 256) {
        int32_t v = row[j];
        if (v >= nlist) {
            *flag = 1u;
            v = -1;
        }
        for (int k = 0; v >= 0 && k < j; ++k)
            if (row[k] == v) v = -1;
        out[(size_t)q * nprobe + j] = v;
    }
}

// Sorts buf[0, n) ascending, n a power of two >= 2; every thread of the workgroup calls it.  Ends behind a barrier.
__device__ __forceinline__ void ivf_bitonic(uint64_t* buf, int n, int tid) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t a = buf[i], b = buf[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
}

// The cnt keys of buf sorted, the rest of the next power of two filled with padding.  Ends behind a barrier.
__device__ __forceinline__ void ivf_sort_keys(uint64_t* buf, uint32_t cnt, int tid) {
    int n = 2;
    while ((uint32_t)n < cnt) n <<= 1;
    for (int i = (int)cnt + tid; i < n; i += 256) buf[i] = kFlatNoKey;
    __syncthreads();
    ivf_bitonic(buf, n, tid);
}

// grid (probes, queries), 256 threads, dynamic LDS: 2 P keys.
template <int M, bool PLAIN_RULE>
__global__ __launch_bounds__(256) void ivf_scan_kernel(const float* __restrict__ lut32, const int32_t* __restrict__ probes,
                                                       int nprobe, const int64_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ ids, const uint8_t* __restrict__ codes,
                                                       int top_k, int cap, int32_t* __restrict__ part_ids,
                                                       float* __restrict__ part_dists) {
    __shared__ __attribute__((aligned(16))) float T[M * 256];
    __shared__ uint32_t s_wcnt[2][4];  // keys the four wavefronts append in a stride, by the stride's parity
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(ivf_smem);  // [cap = 2 P]
    const int p = blockIdx.x, q = blockIdx.y, nq = gridDim.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* out_i = part_ids + ((size_t)p * nq + q) * top_k;
    float* out_d = part_dists + ((size_t)p * nq + q) * top_k;
    const int32_t list = probes[(size_t)q * nprobe + p];
    int64_t lo = 0, hi = 0;
    if (list >= 0) {
        lo = offsets[list];
        hi = offsets[list + 1];
    }
    if (hi <= lo) {  // padding, a repeat or an empty list (uniform over the workgroup)
        for (int r = tid; r < top_k; r += 256) {
            out_i[r] = -1;
            out_d[r] = INFINITY;
        }
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(lut32 + (size_t)q * M * 256);
#pragma unroll
    for (int i = 0; i < M / 4; ++i) reinterpret_cast<float4*>(T)[i * 256 + tid] = src[i * 256 + tid];
    __syncthreads();
    // The number of keys in the buffer lives in a register and is the same in every thread: it starts at 0, grows by
    // the sum of the four words a stride's wavefronts stored BEFORE the stride's barrier and every thread reads behind
    // it, and is cut to min(cnt, top_k) by every thread alike.  The words alternate by the stride's parity, so a
    // wavefront that runs ahead stores the next stride's word beside the one a slower wavefront is still reading; the
    // stride after that lies behind the next barrier.  Nothing the workgroup branches on is read while it can change.
    uint32_t cnt = 0u;
    int par = 0;
    uint64_t thr = kFlatNoKey;
    for (int64_t base = lo; base < hi; base += 256, par ^= 1) {
        const int64_t at = base + tid;
        uint64_t key = kFlatNoKey;
        if (at < hi) {
            uint32_t w[M / 4];
            if constexpr (M == 8) {
                const uint2 v = reinterpret_cast<const uint2*>(codes)[at];
                w[0] = v.x; w[1] = v.y;
            } else {
                const uint4 v = reinterpret_cast<const uint4*>(codes)[at];
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            }
            [[maybe_unused]] double acc64 = 0.0;
            [[maybe_unused]] float acc32 = 0.0f;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float e = T[m * 256 + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)];
                if constexpr (PLAIN_RULE)
                    acc32 = __fadd_rn(acc32, e);
                else
                    acc64 = __dadd_rn(acc64, (double)e);
            }
            const float d = PLAIN_RULE ? acc32 : (float)acc64;
            key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)ids[at];
        }
        const bool pass = key < thr;  // (padding never passes: thr <= kFlatNoKey)
        const unsigned long long mask = __ballot(pass);
        if (lane == 0) s_wcnt[par][wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        const uint32_t c0 = s_wcnt[par][0], c1 = s_wcnt[par][1], c2 = s_wcnt[par][2], c3 = s_wcnt[par][3];
        const uint32_t wbase = cnt + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);
        if (pass) buf[wbase + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = key;  // < cap: the stride had room
        cnt += c0 + c1 + c2 + c3;
        if (cnt + 256u > (uint32_t)cap && base + 256 < hi) {  // no room for the next stride
            ivf_sort_keys(buf, cnt, tid);                      // (its first barrier is behind this stride's appends)
            if (cnt >= (uint32_t)top_k) thr = buf[top_k - 1];  // the next appends go to slots >= top_k
            cnt = min(cnt, (uint32_t)top_k);                   // <= P, and P + 256 <= 2 P
        }
    }
    ivf_sort_keys(buf, cnt, tid);
    for (int r = tid; r < top_k; r += 256) {
        const uint64_t key = (uint32_t)r < cnt ? buf[r] : kFlatNoKey;
        out_i[r] = key != kFlatNoKey ? (int32_t)(key & 0xffffffffu) : -1;
        out_d[r] = key != kFlatNoKey ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
    }
}

// ---- the list scans of DESIGN.md 5.18: a filter, a radius ----------------------------------------------------------------

// The key of list entry `at` under the table in LDS: ivf_scan_kernel's arithmetic, to the bit.
template <int M, bool PLAIN_RULE>
__device__ __forceinline__ uint64_t ivf_entry_key(const float* T, const uint8_t* __restrict__ codes, int64_t at, int32_t id) {
    uint32_t w[M / 4];
    if constexpr (M == 8) {
        const uint2 v = reinterpret_cast<const uint2*>(codes)[at];
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = reinterpret_cast<const uint4*>(codes)[at];
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    [[maybe_unused]] double acc64 = 0.0;
    [[maybe_unused]] float acc32 = 0.0f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float e = T[m * 256 + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)];
        if constexpr (PLAIN_RULE)
            acc32 = __fadd_rn(acc32, e);
        else
            acc64 = __dadd_rn(acc64, (double)e);
    }
    const float d = PLAIN_RULE ? acc32 : (float)acc64;
    return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)id;
}

// Whether the filter lets the entry of reported id `id` pass: the id back to its local node (the even-N renaming undone,
// id_base subtracted), then that node's bit.  A list holds ids of the handle's own nodes only; the range test keeps a
// foreign id from reading past the bitmap all the same.
__device__ __forceinline__ bool ivf_eligible(const IvfFilter& f, int32_t id) {
    const int64_t pos = (f.even && (int64_t)id == f.N) ? f.N - 1 : (int64_t)id;
    const int64_t l = pos - f.base;
    if (l < 0 || l >= f.n_local) return false;
    return (f.bits[l >> 5] >> (l & 31)) & 1u;
}

// ivf_scan_kernel with an eligibility test per entry, made before the code load and the M gathers: an entry the filter
// refuses forms no key.  Everything else -- the register count, the parity words, the uniform branches -- is the scan's.
template <int M, bool PLAIN_RULE>
__global__ __launch_bounds__(256) void ivf_scan_filtered_kernel(const float* __restrict__ lut32,
                                                                const int32_t* __restrict__ probes, int nprobe,
                                                                const int64_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ ids,
                                                                const uint8_t* __restrict__ codes, const IvfFilter filt,
                                                                int top_k, int cap, int32_t* __restrict__ part_ids,
                                                                float* __restrict__ part_dists) {
    __shared__ __attribute__((aligned(16))) float T[M * 256];
    __shared__ uint32_t s_wcnt[2][4];
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(ivf_smem);  // [cap = 2 P]
    const int p = blockIdx.x, q = blockIdx.y, nq = gridDim.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* out_i = part_ids + ((size_t)p * nq + q) * top_k;
    float* out_d = part_dists + ((size_t)p * nq + q) * top_k;
    const int32_t list = probes[(size_t)q * nprobe + p];
    int64_t lo = 0, hi = 0;
    if (list >= 0) {
        lo = offsets[list];
        hi = offsets[list + 1];
    }
    if (hi <= lo) {  // padding, a repeat or an empty list (uniform over the workgroup)
        for (int r = tid; r < top_k; r += 256) {
            out_i[r] = -1;
            out_d[r] = INFINITY;
        }
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(lut32 + (size_t)q * M * 256);
#pragma unroll
    for (int i = 0; i < M / 4; ++i) reinterpret_cast<float4*>(T)[i * 256 + tid] = src[i * 256 + tid];
    __syncthreads();
    uint32_t cnt = 0u;  // uniform over the workgroup, as in ivf_scan_kernel
    int par = 0;
    uint64_t thr = kFlatNoKey;
    for (int64_t base = lo; base < hi; base += 256, par ^= 1) {
        const int64_t at = base + tid;
        uint64_t key = kFlatNoKey;
        if (at < hi) {
            const int32_t id = ids[at];
            if (ivf_eligible(filt, id)) key = ivf_entry_key<M, PLAIN_RULE>(T, codes, at, id);
        }
        const bool pass = key < thr;
        const unsigned long long mask = __ballot(pass);
        if (lane == 0) s_wcnt[par][wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        const uint32_t c0 = s_wcnt[par][0], c1 = s_wcnt[par][1], c2 = s_wcnt[par][2], c3 = s_wcnt[par][3];
        const uint32_t wbase = cnt + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);
        if (pass) buf[wbase + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = key;  // < cap: the stride had room
        cnt += c0 + c1 + c2 + c3;
        if (cnt + 256u > (uint32_t)cap && base + 256 < hi) {
            ivf_sort_keys(buf, cnt, tid);
            if (cnt >= (uint32_t)top_k) thr = buf[top_k - 1];
            cnt = min(cnt, (uint32_t)top_k);
        }
    }
    ivf_sort_keys(buf, cnt, tid);
    for (int r = tid; r < top_k; r += 256) {
        const uint64_t key = (uint32_t)r < cnt ? buf[r] : kFlatNoKey;
        out_i[r] = key != kFlatNoKey ? (int32_t)(key & 0xffffffffu) : -1;
        out_d[r] = key != kFlatNoKey ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
    }
}

// The range scan, grid (probes, queries), 256 threads.  EMIT false: counts[q][p] = the eligible entries of the list whose
// key lies below thr[q].  EMIT true: the same walk again, every such key to pool[offs[q][p] - pool_base + its rank]; the
// rank of an entry is the number of passing entries before it in the list, from the ballot prefix of its wavefront, the
// counts of the wavefronts before it in the stride, and the running count of the strides before (a register, uniform
// over the workgroup, fed through the parity words exactly as the top-k scan's).  No atomics; both passes visit the same
// entries in the same order, so the ranks fill the region the count reserved.  A write at or past pool_n is dropped.
template <int M, bool PLAIN_RULE, bool EMIT>
__global__ __launch_bounds__(256) void ivf_range_kernel(const float* __restrict__ lut32, const int32_t* __restrict__ probes,
                                                        int nprobe, const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ ids, const uint8_t* __restrict__ codes,
                                                        const IvfFilter filt, const uint64_t* __restrict__ thr_key,
                                                        int64_t* __restrict__ counts, const int64_t* __restrict__ offs,
                                                        int64_t pool_base, uint64_t* __restrict__ pool, int64_t pool_n) {
    __shared__ __attribute__((aligned(16))) float T[M * 256];
    __shared__ uint32_t s_wcnt[2][4];
    const int p = blockIdx.x, q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slot = (size_t)q * nprobe + p;
    const int32_t list = probes[slot];
    const uint64_t thr = thr_key[q];
    int64_t lo = 0, hi = 0;
    if (list >= 0 && thr != 0ull) {
        lo = offsets[list];
        hi = offsets[list + 1];
    }
    if (hi <= lo) {  // padding, a repeat, an empty list or a radius <= 0 (uniform over the workgroup)
        if (!EMIT && tid == 0) counts[slot] = 0;
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(lut32 + (size_t)q * M * 256);
#pragma unroll
    for (int i = 0; i < M / 4; ++i) reinterpret_cast<float4*>(T)[i * 256 + tid] = src[i * 256 + tid];
    __syncthreads();
    [[maybe_unused]] const int64_t out0 = EMIT ? offs[slot] - pool_base : 0;
    uint32_t cnt = 0u;  // EMIT: uniform over the workgroup; else the wavefront's own total
    int par = 0;
    for (int64_t base = lo; base < hi; base += 256, par ^= 1) {
        const int64_t at = base + tid;
        uint64_t key = kFlatNoKey;
        if (at < hi) {
            const int32_t id = ids[at];
            if (!filt.bits || ivf_eligible(filt, id)) key = ivf_entry_key<M, PLAIN_RULE>(T, codes, at, id);
        }
        const bool pass = key < thr;  // (thr = kFlatNoKey, the radius +inf, passes every key and no padding)
        const unsigned long long mask = __ballot(pass);
        if constexpr (!EMIT) {
            cnt += (uint32_t)__popcll(mask);
        } else {
            if (lane == 0) s_wcnt[par][wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            const uint32_t c0 = s_wcnt[par][0], c1 = s_wcnt[par][1], c2 = s_wcnt[par][2], c3 = s_wcnt[par][3];
            const uint32_t wbase = cnt + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);
            const int64_t to = out0 + wbase + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (pass && to >= 0 && to < pool_n) pool[to] = key;
            cnt += c0 + c1 + c2 + c3;
        }
    }
    if constexpr (!EMIT) {
        if (lane == 0) s_wcnt[0][wave] = cnt;
        __syncthreads();
        if (tid == 0) counts[slot] = (int64_t)s_wcnt[0][0] + s_wcnt[0][1] + s_wcnt[0][2] + s_wcnt[0][3];
    }
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

unsigned grid_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_ivf_label_keys(const int32_t* d_labels, int64_t n, int nlist, uint32_t* d_keys, uint32_t* d_pos,
                                 unsigned long long* d_counts, uint32_t* d_flag, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_labels || !d_keys || !d_pos || !d_counts || !d_flag || nlist < 1 || nlist > kIvfMaxLists || n > 0x7fffffff)
        return hipErrorInvalidValue;
    ivf_label_keys_kernel<<<dim3(grid_of(n)), dim3(256), 0, stream>>>(d_labels, n, nlist, d_keys, d_pos, d_counts, d_flag);
    return hipGetLastError();
}

hipError_t ivf_scan_and_sort(void* d_temp, size_t* temp_bytes, const unsigned long long* d_counts, int64_t* d_offsets,
                             int nlist, const uint32_t* d_keys, uint32_t* d_keys_out, const uint32_t* d_pos,
                             uint32_t* d_pos_out, int64_t n, hipStream_t stream) {
    if (nlist < 1 || nlist > kIvfMaxLists || n < 0 || n > 0x7fffffff) return hipErrorInvalidValue;
    int bits = 1;  // keys are 0 .. nlist
    while ((1u << bits) <= (uint32_t)nlist) ++bits;
    // the counts are read as the offsets' own type: both are 64-bit and no count reaches the sign
    const int64_t* counts = reinterpret_cast<const int64_t*>(d_counts);
    size_t a = 0, b = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, a, counts, d_offsets, nlist + 1, stream);
    if (e != hipSuccess) return e;
    if (n > 0) {
        e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, d_keys, d_keys_out, d_pos, d_pos_out, (int)n, 0, bits, stream);
        if (e != hipSuccess) return e;
    }
    if (!d_temp) {
        *temp_bytes = std::max(a, b);
        return hipSuccess;
    }
    if (*temp_bytes < std::max(a, b)) return hipErrorInvalidValue;
    size_t tb = *temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(d_temp, tb, counts, d_offsets, nlist + 1, stream);
    if (e != hipSuccess || n == 0) return e;
    tb = *temp_bytes;
    return hipcub::DeviceRadixSort::SortPairs(d_temp, tb, d_keys, d_keys_out, d_pos, d_pos_out, (int)n, 0, bits, stream);
}

hipError_t launch_ivf_ids(const uint32_t* d_pos, int64_t n, const RefineIds& ids, int32_t* d_ids, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_pos || !d_ids || n > 0x7fffffff) return hipErrorInvalidValue;
    ivf_ids_kernel<<<dim3(grid_of(n)), dim3(256), 0, stream>>>(d_pos, n, ids, d_ids);
    return hipGetLastError();
}

hipError_t launch_ivf_gather_codes(const uint32_t* d_pos, int64_t n, int64_t l0, int64_t l1, const uint8_t* d_tile, int M,
                                   uint8_t* d_out, hipStream_t stream) {
    if (n <= 0 || l1 <= l0) return hipSuccess;
    if (!d_pos || !d_tile || !d_out || (M != 8 && M != 16) || l0 < 0 || n > 0x7fffffff ||
        ((reinterpret_cast<uintptr_t>(d_tile) | reinterpret_cast<uintptr_t>(d_out)) & (uintptr_t)(M - 1)))
        return hipErrorInvalidValue;
    if (M == 8)
        ivf_gather_codes_kernel<8><<<dim3(grid_of(n)), dim3(256), 0, stream>>>(d_pos, n, l0, l1, d_tile, d_out);
    else
        ivf_gather_codes_kernel<16><<<dim3(grid_of(n)), dim3(256), 0, stream>>>(d_pos, n, l0, l1, d_tile, d_out);
    return hipGetLastError();
}

hipError_t launch_ivf_reconstruct(const uint8_t* d_codes, int64_t n, int M, int K, int Ds, const float* d_codebook,
                                  float* d_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_codes || !d_codebook || !d_out || M < 1 || K < 1 || K > 256 || Ds < 1 || n * M * Ds > ((int64_t)1 << 38))
        return hipErrorInvalidValue;
    ivf_reconstruct_kernel<<<dim3(grid_of(n * M * Ds)), dim3(256), 0, stream>>>(d_codes, n, M, K, Ds, d_codebook, d_out);
    return hipGetLastError();
}

hipError_t launch_ivf_probes(const int32_t* d_probes, int nq, int nprobe, int nlist, int32_t* d_out, uint32_t* d_flag,
                             hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!d_probes || !d_out || !d_flag || nprobe < 1 || nprobe > kIvfMaxProbe || nlist < 1) return hipErrorInvalidValue;
    ivf_probes_kernel<<<dim3((unsigned)nq), dim3(256), 0, stream>>>(d_probes, nprobe, nlist, d_out, d_flag);
    return hipGetLastError();
}

hipError_t launch_ivf_scan(const float* d_lut32, int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets,
                           const int32_t* d_ids, const uint8_t* d_codes, int M, bool plain_rule, int top_k,
                           int32_t* d_part_ids, float* d_part_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!d_lut32 || !d_probes || !d_offsets || !d_ids || !d_codes || !d_part_ids || !d_part_dists || (M != 8 && M != 16) ||
        nprobe < 1 || nprobe > kIvfMaxProbe || top_k < 1 || top_k > kIvfMaxTopK || nq > 65535 ||
        (reinterpret_cast<uintptr_t>(d_codes) & (uintptr_t)(M - 1)) || (reinterpret_cast<uintptr_t>(d_lut32) & 15u))
        return hipErrorInvalidValue;
    const int cap = 2 * pow2_at_least(std::max(top_k, 256));
    const size_t lds = (size_t)cap * sizeof(uint64_t);  // at most 32 KB beside the table's 16
    const dim3 grid((unsigned)nprobe, (unsigned)nq), block(256);
    if (M == 8) {
        if (plain_rule)
            ivf_scan_kernel<8, true><<<grid, block, lds, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes, top_k,
                                                                   cap, d_part_ids, d_part_dists);
        else
            ivf_scan_kernel<8, false><<<grid, block, lds, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes, top_k,
                                                                    cap, d_part_ids, d_part_dists);
    } else {
        if (plain_rule)
            ivf_scan_kernel<16, true><<<grid, block, lds, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes, top_k,
                                                                    cap, d_part_ids, d_part_dists);
        else
            ivf_scan_kernel<16, false><<<grid, block, lds, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes,
                                                                     top_k, cap, d_part_ids, d_part_dists);
    }
    return hipGetLastError();
}

namespace {
bool ivf_filter_ok(const IvfFilter& f, bool required) {
    if (!f.bits) return !required;
    return f.n_local >= 0 && f.base >= 0 && f.N >= 0;
}
}  // namespace

hipError_t launch_ivf_scan_filtered(const float* d_lut32, int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets,
                                    const int32_t* d_ids, const uint8_t* d_codes, int M, bool plain_rule, const IvfFilter& filter,
                                    int top_k, int32_t* d_part_ids, float* d_part_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!d_lut32 || !d_probes || !d_offsets || !d_ids || !d_codes || !d_part_ids || !d_part_dists || (M != 8 && M != 16) ||
        nprobe < 1 || nprobe > kIvfMaxProbe || top_k < 1 || top_k > kIvfMaxTopK || nq > 65535 || !ivf_filter_ok(filter, true) ||
        (reinterpret_cast<uintptr_t>(d_codes) & (uintptr_t)(M - 1)) || (reinterpret_cast<uintptr_t>(d_lut32) & 15u))
        return hipErrorInvalidValue;
    const int cap = 2 * pow2_at_least(std::max(top_k, 256));
    const size_t lds = (size_t)cap * sizeof(uint64_t);
    const dim3 grid((unsigned)nprobe, (unsigned)nq), block(256);
    auto* kernel = M == 8 ? (plain_rule ? ivf_scan_filtered_kernel<8, true> : ivf_scan_filtered_kernel<8, false>)
                          : (plain_rule ? ivf_scan_filtered_kernel<16, true> : ivf_scan_filtered_kernel<16, false>);
    kernel<<<grid, block, lds, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes, filter, top_k, cap, d_part_ids,
                                         d_part_dists);
    return hipGetLastError();
}

hipError_t launch_ivf_range(const float* d_lut32, int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets,
                            const int32_t* d_ids, const uint8_t* d_codes, int M, bool plain_rule, const IvfFilter& filter,
                            const uint64_t* d_thr, int64_t* d_counts, const int64_t* d_offs, int64_t pool_base, uint64_t* d_pool,
                            int64_t pool_n, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const bool emit = d_pool != nullptr;
    if (!d_lut32 || !d_probes || !d_offsets || !d_ids || !d_codes || !d_thr || (M != 8 && M != 16) || nprobe < 1 ||
        nprobe > kIvfMaxProbe || nq > 65535 || !ivf_filter_ok(filter, false) || (emit ? (!d_offs || pool_n < 0) : !d_counts) ||
        (reinterpret_cast<uintptr_t>(d_codes) & (uintptr_t)(M - 1)) || (reinterpret_cast<uintptr_t>(d_lut32) & 15u))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nprobe, (unsigned)nq), block(256);
    auto pick = [&](auto m, auto plain) {
        constexpr int MM = decltype(m)::value;
        constexpr bool PL = decltype(plain)::value;
        if (emit)
            ivf_range_kernel<MM, PL, true><<<grid, block, 0, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes, filter,
                                                                       d_thr, d_counts, d_offs, pool_base, d_pool, pool_n);
        else
            ivf_range_kernel<MM, PL, false><<<grid, block, 0, stream>>>(d_lut32, d_probes, nprobe, d_offsets, d_ids, d_codes, filter,
                                                                        d_thr, d_counts, d_offs, pool_base, d_pool, pool_n);
    };
    if (M == 8) {
        if (plain_rule) pick(std::integral_constant<int, 8>{}, std::true_type{});
        else pick(std::integral_constant<int, 8>{}, std::false_type{});
    } else {
        if (plain_rule) pick(std::integral_constant<int, 16>{}, std::true_type{});
        else pick(std::integral_constant<int, 16>{}, std::false_type{});
    }
    return hipGetLastError();
}

hipError_t ivf_range_offsets(void* d_temp, size_t* temp_bytes, const int64_t* d_counts, int64_t* d_offs, int64_t n,
                             hipStream_t stream) {
    if (n < 1 || n > 0x7fffffff) return hipErrorInvalidValue;
    size_t tb = d_temp ? *temp_bytes : 0;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(d_temp, tb, d_counts, d_offs, (int)n, stream);
    if (!d_temp) *temp_bytes = tb;
    return e;
}

}  // namespace dpq
