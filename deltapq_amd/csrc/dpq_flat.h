// dpq_flat.h -- exact search over raw vectors on the GPU, by squared L2 or by inner product: fp32 rows, fp16 / bf16
// rows widened exactly to fp32 and 8-bit / 4-bit scalar-quantised rows decoded to fp32, all under fp32 queries
// (dpq_flat.hip), and bytes, unsigned or signed, on the int8 matrix cores (dpq_flat_u8.hip); top-k over a whole base or
// over the rows a filter lists, range search, re-ranking over a candidate list per query.  The arithmetic is the reference's brute force (main.cpp:150-156), restated in
// include/deltapq_amd.h and DESIGN.md 5.10.  A base says what its rows are once, in FlatBase::format.  The fp32-query
// formats share one distance kernel template <LIST, MODE, METRIC, FORMAT> and one re-rank kernel <METRIC, FORMAT>; the
// bytes have their own pair.  One stripe driver (launch_flat_search), one range pass (launch_flat_range_pass) and one
// re-rank launcher (launch_flat_rerank) serve every format, with and without a filter; the metric reaches the kernels
// through FlatBase::metric.  What the kernels of the two files share -- the modes, the key sink, the padding key, the
// row a candidate names, and for the fp32-query kernels the step of the sum and the key -- is defined here, once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kFlatMaxTopK = 16384;  // DPQ_FLAT_MAX_TOPK, and the most candidates a re-rank takes per query
constexpr int kFlatMaxD = 2048;
constexpr int kFlatBitsMaxD = 4096;  // DPQ_FLAT_BITS_MAX_D: the most dimensions of a binary row

// The metric of a kernel.  kFlatL2: the key's high word is the bits of the (non-negative) distance.  kFlatIP: the
// score's bits mapped so that ascending keys are descending scores (flat_ip_word below).
enum { kFlatL2 = 0, kFlatIP = 1 };
// What the rows of a base are stored as.  kFlatF16 / kFlatBF16 are DPQ_HALF_F16 / DPQ_HALF_BF16.
// kFlatSQ8 / kFlatSQ4: codes of a scalar quantiser, DPQ_SQ_8BIT / DPQ_SQ_4BIT ("scalar-quantised vectors" below).
// kFlatBits: one bit per dimension, compared by Hamming distance ("binary vectors" below).
enum { kFlatF32 = 0, kFlatF16 = 1, kFlatBF16 = 2, kFlatU8 = 3, kFlatI8 = 4, kFlatSQ8 = 5, kFlatSQ4 = 6, kFlatBits = 7 };
// The format of the queries a base of this format takes: fp32 for fp32, half and quantised rows, the rows' own for bytes
// and for bits.
inline int flat_query_format(int format) {
    return format == kFlatU8 || format == kFlatI8 || format == kFlatBits ? format : kFlatF32;
}
// Score bits <-> high word of an inner-product key; the map is its own inverse.  -0.0 is read as +0.0 first.  A
// non-negative score u becomes ~u & 0x7fffffff (larger scores, smaller words), a negative one keeps its bits (sign set,
// larger magnitudes later): +inf 0x007fffff < 1.0 < +0.0 0x7fffffff < -1e-40 < -1.0 < -inf 0xff800000 < kFlatNoKey's.
__host__ __device__ inline uint32_t flat_ip_word(uint32_t u) {
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? u : (~u & 0x7fffffffu);
}

#ifdef __HIPCC__
// The key of an fp32-query kernel: the accumulator rounded to fp32, its bits (kFlatIP: their key word) above the id.
template <int METRIC>
__device__ __forceinline__ uint64_t make_key(double acc, uint32_t id) {
    const uint32_t u = __float_as_uint((float)acc);
    return ((uint64_t)(METRIC == kFlatIP ? flat_ip_word(u) : u) << 32) | id;
}

// One dimension of one (vector, query) pair on the lane's fp64 accumulator.  L2: the difference and its square each
// rounded in fp32, then widened.  Inner product: both values widened first, so the product is exact and the step is one
// rounding, fused or not.
template <int METRIC>
__device__ __forceinline__ void accumulate(double& acc, float v, float q) {
    if constexpr (METRIC == kFlatIP) {
        acc = fma((double)v, (double)q, acc);
    } else {
        const float t = v - q;
        const float s = t * t;
        acc += (double)s;
    }
}

// The row a re-rank candidate c names, or -1.  A negative candidate is padding.  With a map (n_map entries) c is a DFS
// position and the row map[c]; without one the row is c - id_offset.  *flag is set when c >= 0 names no row of the n.
__device__ __forceinline__ int flat_candidate_row(int32_t c, int64_t n, int64_t id_offset, const uint32_t* map, int64_t n_map,
                                                  uint32_t* flag) {
    int row = -1;
    if (c >= 0) {
        if (map) {
            int64_t p = c;
            if ((n_map & 1) == 0 && p == n_map) p = n_map - 1;  // the even-N id of the last DFS node
            if (p < n_map && (int64_t)map[p] < n) row = (int)map[p];
        } else {
            const int64_t r = (int64_t)c - id_offset;
            if (r >= 0 && r < n) row = (int)r;
        }
        if (row < 0) *flag = 1;
    }
    return row;
}
#endif

// Per-query selection state of a search.  overflow: an append fell outside the key buffer (the launcher's striping
// rules that out; a set word is reported as an internal error instead of a wrong answer).
struct FlatQueryState {
    uint32_t count;     // keys in the query's buffer
    uint32_t overflow;
    uint64_t thr;       // keys above it are not appended
};

// Rows are stored padded with zeros to a multiple of four floats (16-byte loads; a zero dimension adds +0.0).
inline int flat_padded_d(int D) { return (D + 3) & ~3; }
// Keys a query's buffer holds for this top_k (a power of two, at least 4 * top_k).
int flat_key_capacity(int top_k);
// Queries one search pass takes (their key buffers together stay within 64 MB).
int flat_query_batch(int top_k);

// ---- what a search, a range pass or a re-rank runs over ----------------------------------------------------------------
// A prepared base: rows [n][Dp] of `format`, padded with zeros -- fp32 to a multiple of four values, halves to a multiple
// of eight, bytes (biased int8 for kFlatU8, see "byte vectors" below) to the K step of the MFMA, with their int32 norms,
// codes of a scalar quantiser to 16 (kFlatSQ8) or 32 (kFlatSQ4, two to a byte) with code 0, beside their quantiser.
// A kFlatBits base: D is the number of bits and Dp the bytes of a stored row (flat_bits_row_bytes), no norms.
// The entries a pass visits are rows 0 .. n_entries - 1, or, with `filtered`, rows list[0 .. n_entries - 1] (ascending).
// `filtered`, not the list pointer, says which: an empty filter has n_entries == 0 and may have a NULL list.
// Reported id = row + id_offset.
struct FlatBase {
    int format = kFlatF32;
    const void* rows = nullptr;
    int64_t n = 0;
    int D = 0, Dp = 0;
    int64_t id_offset = 0;
    int metric = kFlatL2;
    const int32_t* norm = nullptr;  // a byte base: the rows' norms, allocated rounded up to four rows
    const int32_t* rsum = nullptr;  // a kFlatU8 base under kFlatIP: the rows' correction terms, padded as norm is
    // a kFlatSQ8 / kFlatSQ4 base: (lo, step) per padded dimension, (+0, +0) in the padding.  It lies in the rows' own
    // allocation, directly in front of them (flat_sq_quant_of), where the kernels find it without an argument of its own
    const float2* quant = nullptr;
    bool filtered = false;
    const uint32_t* list = nullptr;
    int64_t n_entries = 0;
};
// Prepared queries of the base's kind: [nq][Dp] padded rows, with norms for bytes (and, for the inner product over an
// unsigned byte base, the queries' correction terms).
struct FlatQueries {
    const float* f32;
    const int8_t* i8;
    const int32_t* norm;
    int nq;
    const int32_t* sum = nullptr;
    const uint8_t* bits = nullptr;  // a kFlatBits base: [nq][Dp] prepared as the rows are
};

// What a distance kernel does with a key (its MODE): at or below the query's threshold it is appended to the query's
// buffer keys[q][cap]; below the radius key it is counted; below the radius key it is appended to the query's list
// keys[offs[q] .. offs[q + 1]).
enum { kFlatTopK = 0, kFlatCount = 1, kFlatEmit = 2 };
constexpr uint64_t kFlatNoKey = ~0ull;  // padding in a key buffer; the threshold that lets every key pass

// Where the keys of query q go and how many fit.
template <int MODE>
__device__ __forceinline__ uint64_t* flat_sink_of(uint64_t* keys, int cap, const int64_t* offs, int q, uint32_t* room) {
    if (MODE == kFlatEmit) {
        *room = (uint32_t)(offs[q + 1] - offs[q]);
        return keys + offs[q];
    }
    *room = (uint32_t)cap;
    return keys + (size_t)q * cap;
}

// Exact top_k of q.nq (<= flat_query_batch(top_k)) queries over the base's entries, all device pointers.
// d_keys [nq][flat_key_capacity(top_k)], d_state [nq].  Fewer than top_k entries (a filter): rows are padded with
// -1 / +inf (kFlatIP: -1 / -inf, and d_dists holds scores, descending).  Enqueues on `stream`; d_state[q].overflow and .count must be read back afterwards.
hipError_t launch_flat_search(const FlatBase& b, const FlatQueries& q, int top_k, uint64_t* d_keys, FlatQueryState* d_state,
                              int32_t* d_ids, float* d_dists, hipStream_t stream);

// A re-rank: exact distances of cand[nq][n_cand] only, best top_k by (distance, reported id), all device pointers.
// queries: the caller's [nq][D] (a bits base: [nq][(D + 7) / 8] bytes), unpadded, of flat_query_format(the base's format).  map (may be NULL) [n_map]: a
// candidate is a DFS position, row = map[c], with the even-N rule; without it row = c - id_offset.
// keys [nq][flat_rerank_keys(n_cand)].  *flag is set when a candidate names no row.  kFlatIP: exact scores, best top_k by
// (score descending, reported id).
struct FlatRerank {
    const void* queries = nullptr;
    int nq = 0;
    const int32_t* cand = nullptr;
    int n_cand = 0;
    int top_k = 0;
    const uint32_t* map = nullptr;
    int64_t n_map = 0;
    uint64_t* keys = nullptr;
    uint32_t* flag = nullptr;
    int32_t* ids = nullptr;
    float* dists = nullptr;
};
hipError_t launch_flat_rerank(const FlatBase& b, const FlatRerank& r, hipStream_t stream);
size_t flat_rerank_keys(int n_cand);  // keys per query launch_flat_rerank needs: n_cand rounded up to a power of two

// [rows][D] -> [rows][Dp] with zero padding, on the device.
hipError_t launch_flat_pad_rows(const float* d_in, int64_t rows, int D, int Dp, float* d_out, hipStream_t stream);

// The last stage of a search or a re-rank, for the other files: sorts n_keys keys per query (d_state[q].count of them
// when d_state is given), drops repeats, writes top_k.
hipError_t launch_flat_sort_emit(const uint64_t* d_keys, size_t stride, const FlatQueryState* d_state, int nq, int n_keys,
                                 int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream, int metric = kFlatL2);

// ---- byte vectors on the int8 matrix cores (dpq_flat_u8.hip) -------------------------------------------------------
// Unsigned rows (0..255) are stored as x ^ 0x80 (int8), signed rows (-128..127) as they are; both padded with int8 zeros
// to the K step of v_mfma_i32_32x32x32_i8, with an int32 norm per row; the norm array of a base is allocated rounded up
// to four rows (16-byte loads in the epilogue).  The inner product over unsigned rows adds a term per row and a term per
// query to the int8 dot product (dpq_flat_u8.hip's header); the rows' terms are padded as the norms are.
constexpr int kFlatU8KStep = 32;
inline int flat_u8_padded_d(int D) { return (D + kFlatU8KStep - 1) & ~(kFlatU8KStep - 1); }

// bytes [rows][D] -> int8 [rows][Dp] (biased unless is_signed: d_in then holds int8 values) and norms [rows], on the device.
hipError_t launch_flat_u8_prepare(const uint8_t* d_in, int64_t rows, int D, int Dp, int8_t* d_out, int32_t* d_norms,
                                  hipStream_t stream, bool is_signed = false);
// d_sums[r] = 128 * (the sum of prepared row r) + add: the rows' terms with add = 16384 * D, the queries' with add = 0.
hipError_t launch_flat_u8_sums(const int8_t* d_rows8, int64_t rows, int Dp, int add, int32_t* d_sums, hipStream_t stream);
// The distance stage of launch_flat_search / launch_flat_range_pass on a byte base: one launch of the byte kernel's
// (b.filtered, mode, b.metric, signed rows) instantiation over entries e0 .. e0 + rows - 1.  keys / cap / offs: the mode's
// sink, as above.  kFlatIP on an unsigned base needs b.rsum and q.sum.
hipError_t launch_flat_dist_u8(int mode, const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys,
                               int cap, const int64_t* offs, FlatQueryState* state, hipStream_t stream);
// The distance stage of launch_flat_rerank on a byte base: one launch of the byte re-rank kernel's (b.metric, signed)
// instantiation over r.nq <= 65535 queries (the grid's y extent); r.queries are the caller's bytes (int8 values on a
// kFlatI8 base).  n_pad: flat_rerank_keys(r.n_cand), the stride of r.keys.
void launch_flat_rerank_chunk_u8(const FlatBase& b, const FlatRerank& r, int n_pad, hipStream_t stream);

// ---- half-precision vectors, fp16 and bf16 (dpq_flat.hip: the fp32 kernels' FORMAT) ----------------------------------
// Rows are stored as they are given, 16 bits per value, padded with zeros to a multiple of eight values (16-byte loads).
// The kernels widen a value to fp32 as they stage it, which is exact, and are the fp32 kernels in everything else: an
// answer over a half base is, bit for bit, the answer over the widened rows.  Queries are fp32 throughout.
inline int flat_half_padded_d(int D) { return (D + 7) & ~7; }

// fp32 bits -> 16 bits, round to nearest, ties to even, in integer arithmetic: the same bits on the host and on the
// device, whatever the denormal mode.  fp16 underflows gradually and overflows to infinity from 65520 on; NaNs are out
// of scope (they stay NaNs).
__host__ __device__ inline uint16_t flat_half_narrow(uint32_t u, int format) {
    if (format == kFlatBF16) return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // 65520 and above
    if (a >= 0x38800000u) {                                   // 2^-14 and above: a normal half
        const uint32_t r = a - 0x38000000u;
        return (uint16_t)(sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13));
    }
    if (a < 0x33000000u) return (uint16_t)sign;               // below 2^-25: zero
    const uint32_t shift = 126u - (a >> 23), m = (a & 0x7fffffu) | 0x800000u;  // the half is m * 2^-shift, 14 <= shift <= 24
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1);
    if (rem > mid || (rem == mid && (h & 1u))) ++h;
    return (uint16_t)(sign | h);
}
// 16 bits -> the bits of the fp32 value they stand for, exactly.
__host__ __device__ inline uint32_t flat_half_widen(uint16_t h, int format) {
    if (format == kFlatBF16) return (uint32_t)h << 16;
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u;
    uint32_t m = h & 0x3ffu;
    if (e == 31u) return sign | 0x7f800000u | (m << 13);
    if (e) return sign | ((e + 112u) << 23) | (m << 13);
    if (!m) return sign;
    uint32_t s = 0;
    while (!(m & 0x400u)) m <<= 1, ++s;
    return sign | ((113u - s) << 23) | ((m & 0x3ffu) << 13);
}

// 16-bit rows [rows][D] -> [rows][Dp] with zero padding; fp32 rows [rows][D] -> narrowed, padded 16-bit rows.
hipError_t launch_flat_half_prepare(const uint16_t* d_in, int64_t rows, int D, int Dp, uint16_t* d_out, hipStream_t stream);
hipError_t launch_flat_half_narrow(const float* d_in, int64_t rows, int D, int Dp, int format, uint16_t* d_out,
                                   hipStream_t stream);

// ---- scalar-quantised vectors, 8 and 4 bits per dimension (dpq_flat.hip: the fp32 kernels' FORMAT) -------------------
// A quantiser over D dimensions is (lo[d], step[d]); a code c of `bits` bits stands for lo[d] + (float)c * step[d], the
// product and the sum each rounded in fp32 (include/deltapq_amd.h, "scalar-quantised vectors").  A base keeps one byte
// per dimension (kFlatSQ8), rows padded to a multiple of 16 dimensions, or one nibble (kFlatSQ4: dimension 2j in the low
// nibble of byte j), rows padded to a multiple of 32: a row is whole 16-byte loads.  The padding is code 0 under
// (lo, step) = (+0, +0), which decodes to +0.0.  The kernels decode a value as they stage it and are the fp32 kernels in
// everything else: an answer over a quantised base is, bit for bit, the answer over the decoded rows.
inline int flat_sq_padded_d(int D, int bits) { return bits == 8 ? (D + 15) & ~15 : (D + 31) & ~31; }
__host__ __device__ inline int flat_sq_row_bytes(int d, int bits) { return bits == 8 ? d : (d + 1) / 2; }  // of d dimensions' codes
// The quantiser array of a base: (lo, step) per dimension, allocated and zeroed up to a multiple of 32 dimensions (256
// bytes), and placed so that it ends where the rows begin: the distance and re-rank kernels keep one argument list for
// every format and reach a quantised base's quantiser from its rows.
__host__ __device__ inline int flat_sq_quant_len(int Dp) { return (Dp + 31) & ~31; }
__host__ __device__ inline const float2* flat_sq_quant_of(const void* rows, int Dp) {
    return static_cast<const float2*>(rows) - flat_sq_quant_len(Dp);
}

#ifdef __HIPCC__
// The value of code c.  Two roundings: the build passes -ffp-contract=off, and the intrinsics say it once more.
__device__ __forceinline__ float flat_sq_decode(uint32_t c, float2 q) { return __fadd_rn(q.x, __fmul_rn((float)c, q.y)); }
#endif

// Float bits <-> a word whose unsigned order is the order of the values (-0.0 below +0.0); the minima and maxima of
// launch_flat_sq_minmax are such words.
__host__ __device__ inline uint32_t flat_order_word(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline uint32_t flat_order_bits(uint32_t w) { return (w & 0x80000000u) ? (w & 0x7fffffffu) : ~w; }

// d_mn / d_mx [D] order words: lowered / raised to the minimum / maximum of every column of d_in [rows][D].  The caller
// starts them at 0xffffffff / 0.
hipError_t launch_flat_sq_minmax(const float* d_in, int64_t rows, int D, uint32_t* d_mn, uint32_t* d_mx, hipStream_t stream);
// fp32 rows [rows][D] -> codes, out_stride bytes per row: the codes of dimensions 0 .. D - 1 under d_quant [D], then
// code 0 (out_stride = flat_sq_row_bytes(D, bits): the caller's layout; flat_sq_row_bytes(Dp, bits): a base's rows).
hipError_t launch_flat_sq_encode(const float* d_in, int64_t rows, int D, int bits, const float2* d_quant, uint8_t* d_out,
                                 int out_stride, hipStream_t stream);
// The caller's codes [rows][flat_sq_row_bytes(D, bits)] -> a base's rows [rows][out_stride]; the spare nibble of an odd
// D and the padding become code 0.
hipError_t launch_flat_sq_prepare(const uint8_t* d_in, int64_t rows, int D, int bits, uint8_t* d_out, int out_stride,
                                  hipStream_t stream);

// ---- binary vectors, one bit per dimension, by Hamming distance (dpq_flat_bits.hip) ----------------------------------
// A row is D bits in (D + 7) / 8 bytes, dimension d in bit d & 7 of byte d >> 3.  A base (and a staged query batch) keeps
// the spare bits of the last byte cleared and pads a row with zero bytes to a multiple of 16 (16-byte loads); zero against
// zero XORs to zero, so the padding adds nothing to a distance.  FlatBase::D is the number of bits, FlatBase::Dp the bytes
// of a stored row; the metric stays kFlatL2: the key word is the fp32 bits of the integer distance.
inline int flat_bits_bytes(int D) { return (D + 7) / 8; }                         // of a row as the caller holds it
inline int flat_bits_row_bytes(int D) { return (flat_bits_bytes(D) + 15) & ~15; }  // of a stored row
// The caller's bytes [rows][flat_bits_bytes(D)] -> stored rows [rows][out_stride = flat_bits_row_bytes(D)]; a query batch
// takes the same path.
hipError_t launch_flat_bits_prepare(const uint8_t* d_in, int64_t rows, int D, uint8_t* d_out, int out_stride,
                                    hipStream_t stream);
// fp32 rows [rows][D] -> packed bits, bit d = in[d] > d_thr[d] in fp32 (d_thr NULL: > 0), out_stride bytes per row, zero
// from the row's last dimension on (out_stride = flat_bits_bytes(D): the caller's layout; flat_bits_row_bytes(D): a base's).
hipError_t launch_flat_bits_from_float(const float* d_in, int64_t rows, int D, const float* d_thr, uint8_t* d_out,
                                       int out_stride, hipStream_t stream);
// The distance stage of launch_flat_search / launch_flat_range_pass on a bits base (q.bits), as launch_flat_dist_u8 is
// the byte bases'.
hipError_t launch_flat_dist_bits(int mode, const FlatBase& b, int64_t e0, int rows, const FlatQueries& q, uint64_t* keys,
                                 int cap, const int64_t* offs, FlatQueryState* state, hipStream_t stream);
// The distance stage of launch_flat_rerank on a bits base; r.queries are the caller's bytes [nq][flat_bits_bytes(D)].
void launch_flat_rerank_chunk_bits(const FlatBase& b, const FlatRerank& r, int n_pad, hipStream_t stream);

// ---- filters and range search (dpq_flat_filter.hip: the row list, the range state, the sort; no distance code) -----
// A filter is the ascending list of a handle's eligible rows.  d_words [n_words]: bit b of word w = row 32 w + b.
// flat_filter_count fills d_cnt / d_off [n_words] (popcounts and their exclusive prefix sum) and waits for n_allowed;
// launch_flat_filter_emit then writes d_list [cap] (*d_flag is set if an entry would fall outside it).
hipError_t flat_filter_count(const uint32_t* d_words, int64_t n_words, uint32_t* d_cnt, uint32_t* d_off, int64_t* n_allowed,
                             hipStream_t stream);
hipError_t launch_flat_filter_emit(const uint32_t* d_words, int64_t n_words, const uint32_t* d_off, uint32_t* d_list,
                                   int64_t cap, uint32_t* d_flag, hipStream_t stream);
// Range search, count then emit.  launch_flat_range_state: count = overflow = 0, thr = d_thr[q] (distance bits of the
// radius << 32; 0 passes nothing).  launch_flat_range_pass (dpq_flat.hip, beside the distance kernels) forms the distances
// of the queries to every entry of the base in one launch and, for keys below thr, counts them (d_pool NULL) or appends
// them to the query's list d_pool[d_offs[q] .. d_offs[q + 1]).  flat_range_sort: hipcub's two-call protocol (d_temp NULL:
// *temp_bytes only); sorts every list of the pool by key into d_out.
hipError_t launch_flat_range_state(FlatQueryState* d_state, const uint64_t* d_thr, int nq, hipStream_t stream);
hipError_t launch_flat_range_pass(const FlatBase& b, const FlatQueries& q, uint64_t* d_pool, const int64_t* d_offs,
                                  FlatQueryState* d_state, hipStream_t stream);
hipError_t flat_range_sort(void* d_temp, size_t* temp_bytes, const uint64_t* d_in, uint64_t* d_out, int64_t n_keys,
                           int n_lists, const int64_t* d_offs, hipStream_t stream);

}  // namespace dpq
