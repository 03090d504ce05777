// dpq_flat_ivf.h -- launch interface of the inverted-list scan over raw fp32 rows (dpq_flat_ivf.hip): exact distances of
// the queries to the rows of the lists they probe, a running top-k per (query, probed list) (include/deltapq_amd.h "IVF
// search over raw vectors"), and of its sibling over byte rows on the int8 matrix cores
// (dpq_flat_ivf_u8.hip, "IVF search over byte vectors") and over binary rows by Hamming distance
// (dpq_flat_ivf_bits.hip, "IVF search over binary vectors"), and of the fp32 scan's form for half and
// scalar-quantised rows (dpq_flat_ivf_narrow.hip).  The lists are row numbers into a dpq_flat handle's own padded rows; they
// come from dpq_ivf.h's launch_ivf_label_keys and ivf_scan_and_sort, the probe rows from its launch_ivf_probes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kFlatIvfGroupMax = 16;  // pairs (query, probed list) one workgroup takes: 16, 8, 4, 2 or 1
constexpr int kFlatIvfGroup = 4;      // ... and the shipped choice: the fastest measured at nprobe 16
constexpr int kFlatIvfTileRows = 256;  // rows of a workgroup's tile
constexpr int kFlatIvfSliceDims = 32;  // dimensions of a tile that are in LDS at a time

// The group the scan runs with: the largest of 16, 8, 4, 2, 1 that is at most `group` and whose LDS -- the tiles beside
// group buffers of 2 P2 keys, P2 the power of two >= max(top_k, 256) -- fits a workgroup.
int flat_ivf_group(int top_k, int group);

// The pairs of a slice.  d_probes [n_pairs] is the pre-pass's output read as one row, entry i = q * nprobe + j:
// d_keys[i] = the list it names, nlist where it is -1; d_vals[i] = i.
hipError_t launch_flat_ivf_pairs(const int32_t* d_probes, int64_t n_pairs, int nlist, uint32_t* d_keys, uint32_t* d_vals,
                                 hipStream_t stream);

// hipCUB's two-call protocol (d_temp NULL: *temp_bytes only): a STABLE sort of (d_keys, d_vals) by key -- the pairs of
// a list stay in ascending (q, j) order, the padding pairs come last.
hipError_t flat_ivf_sort_pairs(void* d_temp, size_t* temp_bytes, const uint32_t* d_keys, uint32_t* d_keys_out,
                               const uint32_t* d_vals, uint32_t* d_vals_out, int64_t n_pairs, int nlist, hipStream_t stream);

// What the scan runs over: rows [n][Dp] fp32 padded with zeros (Dp % 4 == 0, 16-byte aligned); list l holds the row
// numbers d_list_rows[d_offsets[l] .. d_offsets[l + 1]), ascending.  Reported id = row + id_offset.
struct FlatIvfLists {
    const float* rows = nullptr;
    int Dp = 0;
    int64_t id_offset = 0;
    const int64_t* offsets = nullptr;
    const uint32_t* list_rows = nullptr;
    int nlist = 0;
    const uint32_t* filter = nullptr;  // NULL, or a bitmap over the rows, [(n + 31) / 32] words, bit r & 31 of word r >> 5:
                                       // only the rows whose bit is set are scanned (dpq_flat_ivf_device.h's fill_tile)
    int metric = 0;  // dpq_flat.h's kFlatL2, or kFlatIP: the scan forms scores and d_part_dists holds their KEY WORDS
                     // (flat_ip_word of the score's bits; padding -1 / +inf as ever), which launch_merge orders as it orders
                     // distance bits: score descending, id ascending.  launch_flat_ivf_ip_scores turns the merged answer back
};

// The list scan.  d_skeys / d_svals [n_pairs = nq * nprobe]: the sorted pairs.  A workgroup takes `group` consecutive
// pairs (see flat_ivf_group) and, for every stretch of equal list among them, reads the list's rows once for the
// stretch's queries.  d_queries [nq][Dp], padded as the rows are.  The distance of (row, query): per dimension in
// ascending order t = v[d] - q[d] and s = t * t, each rounded in fp32, summed on an fp64 accumulator from +0.0 and
// rounded once (dpq_flat.h's accumulate<kFlatL2> and make_key<kFlatL2>).  The best top_k of pair i = q * nprobe + j by
// key `distance bits << 32 | id` go to d_part_ids / d_part_dists [(j * nq + q)][top_k], padded with -1 / +inf:
// launch_ivf_scan's output contract.  The answer does not depend on the group.
hipError_t launch_flat_ivf_scan(const FlatIvfLists& lists, const float* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                                const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids, float* d_part_dists,
                                hipStream_t stream);

// After the last merge round of an inner-product search: d_vals[i], a key word, becomes the score's bits; an entry whose
// d_ids[i] is negative becomes -inf.  n entries.
hipError_t launch_flat_ivf_ip_scores(const int32_t* d_ids, float* d_vals, int64_t n, hipStream_t stream);

// ---- byte rows (dpq_flat_ivf_u8.hip) -------------------------------------------------------------------------------
constexpr int kFlatIvfGroupU8 = 8;  // the byte scan's shipped group: the fastest measured at nprobe 16

// flat_ivf_group for the byte scan, whose LDS beside the buffers is the stretch's queries [16][Dp + 16] bytes and the
// row numbers.
int flat_ivf_group_u8(int top_k, int Dp, int group);

// What the byte scan runs over: a byte base's rows [n][Dp] int8 (dpq_flat.h "byte vectors": biased where the data are
// unsigned, padded with zeros, Dp % 32 == 0, 16-byte aligned) and their int32 norms [n]; the lists as in FlatIvfLists.
struct FlatIvfListsU8 {
    const int8_t* rows = nullptr;
    const int32_t* norm = nullptr;
    int Dp = 0;
    int64_t id_offset = 0;
    const int64_t* offsets = nullptr;
    const uint32_t* list_rows = nullptr;
    int nlist = 0;
    const uint32_t* filter = nullptr;  // see FlatIvfLists
    int metric = 0;                    // see FlatIvfLists
};

// launch_flat_ivf_scan over byte rows.  d_queries [nq][Dp] int8 and d_qnorm [nq]: the queries as the rows are stored,
// launch_flat_u8_prepare's output.  The distance of (row, query) is norm[row] + qnorm[query] - 2 * (their int8 dot
// product) in int32 -- the exact sum of (v[d] - q[d])^2 -- converted once to fp32, round to nearest even.  The same pairs,
// the same output rows, the same order and padding; the answer does not depend on the group.  lists.metric kFlatIP: the score
// is the int32 S of dpq_flat_u8.hip's header, converted once: signed rows, the int8 dot product, lists.norm and d_qnorm both
// NULL; unsigned rows, dot + rs[row] + qs[query] with rs in lists.norm (launch_flat_u8_sums, add = 16384 D) and qs in
// d_qnorm (add = 0).
hipError_t launch_flat_ivf_scan_u8(const FlatIvfListsU8& lists, const int8_t* d_queries, const int32_t* d_qnorm, int nq,
                                   int nprobe, const uint32_t* d_skeys, const uint32_t* d_svals, int top_k, int group,
                                   int32_t* d_part_ids, float* d_part_dists, hipStream_t stream);

// Bytes -> the fp32 values they stand for, d_out [rows][Dp] padded with zeros.  d_in [rows][in_stride] bytes, the first D
// of a row read.  is_signed: int8 values.  stored: a byte base's rows, whose unsigned values are biased (undone here);
// otherwise the caller's bytes as they are.
hipError_t launch_flat_ivf_widen(const void* d_in, int64_t rows, int D, int in_stride, int Dp, bool stored, bool is_signed,
                                 float* d_out, hipStream_t stream);

// ---- binary rows (dpq_flat_ivf_bits.hip) -----------------------------------------------------------------------------
constexpr int kFlatIvfGroupBits = 4;  // the binary scan's shipped group: the fastest measured at nprobe 16

// flat_ivf_group for the binary scan, whose LDS is the buffers alone: a lane keeps its row number in a register and the
// queries are read as scalars (Wp, the words of a row, is part of the rule for a form that stages them).
int flat_ivf_group_bits(int top_k, int Wp, int group);

// What the binary scan runs over: a kFlatBits base's rows [n][Wp] uint32 (dpq_flat.h "binary vectors": Wp * 4 =
// flat_bits_row_bytes(D), spare bits and padding zero, 16-byte aligned); the lists as in FlatIvfLists.
struct FlatIvfListsBits {
    const uint32_t* rows = nullptr;
    int Wp = 0;
    int64_t id_offset = 0;
    const int64_t* offsets = nullptr;
    const uint32_t* list_rows = nullptr;
    int nlist = 0;
    const uint32_t* filter = nullptr;  // see FlatIvfLists
};

// launch_flat_ivf_scan over binary rows.  d_queries [nq][Wp]: the queries as the rows are stored,
// launch_flat_bits_prepare's output.  The distance of (row, query) is the population count of their XOR, an integer,
// converted to fp32 exactly; the key is flat_dist_bits_kernel's.  The same pairs, the same output rows, the same order and
// padding; the answer does not depend on the group.
hipError_t launch_flat_ivf_scan_bits(const FlatIvfListsBits& lists, const uint32_t* d_queries, int nq, int nprobe,
                                     const uint32_t* d_skeys, const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids,
                                     float* d_part_dists, hipStream_t stream);

// ---- narrow rows: fp16, bf16, 8-bit and 4-bit scalar-quantised (dpq_flat_ivf_narrow.hip) ----------------------------------
constexpr int kFlatIvfGroupNarrow = 4;  // the narrow scan's shipped group, every format: the fastest measured at nprobe 16
constexpr int kFlatIvfNarrowSliceWords = 16;  // 4-byte words of a stored row that are in LDS at a time: 32 / 64 / 128 dimensions

// flat_ivf_group for the narrow scan of `format`, whose LDS beside the buffers is the narrow row tile, a slice of the
// stretch's queries, a quantised format's (lo, step) of the slice, and the row numbers.
int flat_ivf_group_narrow(int format, int top_k, int group);

// What the narrow scan runs over: a kFlatF16 / kFlatBF16 / kFlatSQ8 / kFlatSQ4 base's rows [n][Dp] as dpq_flat.h stores
// them (Dp dimensions, a multiple of 8 / 8 / 16 / 32: a row is whole 16-byte loads; 16-byte aligned; a quantised base's
// quantiser in front of the rows, flat_sq_quant_of); the lists as in FlatIvfLists.
struct FlatIvfListsNarrow {
    int format = 0;  // dpq_flat.h's kFlatF16, kFlatBF16, kFlatSQ8 or kFlatSQ4
    const void* rows = nullptr;
    int Dp = 0;
    int64_t id_offset = 0;
    const int64_t* offsets = nullptr;
    const uint32_t* list_rows = nullptr;
    int nlist = 0;
    const uint32_t* filter = nullptr;  // see FlatIvfLists
    int metric = 0;                    // see FlatIvfLists
};

// launch_flat_ivf_scan over narrow rows.  d_queries [nq][Dp] fp32, padded with zeros.  The distance of (row, query) is
// launch_flat_ivf_scan's over the row widened (flat_half_widen) or decoded (flat_sq_decode) to fp32, bit for bit.  The
// same pairs, the same output rows, the same order and padding; the answer does not depend on the group.
hipError_t launch_flat_ivf_scan_narrow(const FlatIvfListsNarrow& lists, const float* d_queries, int nq, int nprobe,
                                       const uint32_t* d_skeys, const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids,
                                       float* d_part_dists, hipStream_t stream);

// Rows r0 .. r0 + rows - 1 of a narrow base (d_rows: the base's first row) -> the fp32 values they stand for,
// d_out [rows][Dp]; the padding comes out as +0.0.
hipError_t launch_flat_ivf_narrow_widen(int format, const void* d_rows, int Dp, int64_t r0, int64_t rows, float* d_out,
                                        hipStream_t stream);

// ---- range search: every row of the probed lists below a threshold ----------------------------------------
// The four scans above with a second sink in the place of the running top-k.  thr [nq]: a query's threshold as a key --
// distance bits << 32 (0 passes nothing, kFlatNoKey everything), or flat_ip_word of a score threshold << 32; a key passes
// when key < thr.  pool == NULL, the count pass: counts[q * nprobe + j] = the eligible rows of pair (q, j)'s list that pass
// (0 for padding, a repeat, an empty list); one workgroup writes a pair's count, once.  Else the emit pass: the pairs whose
// count is 0 or whose query lies outside [qa, qb) are dropped before anything of their list is read, the stretch's
// surviving queries are compacted, and the passing keys of pair i go to pool[offs[i] - pool_base ..) in no particular
// order (offs: ivf_range_offsets of the counts); nothing is written at or past pool_n.  No key buffers in LDS: the group
// is the largest of 16, 8, 4, 2, 1 that is at most `group`, whatever the format.
struct FlatIvfRange {
    const uint64_t* thr = nullptr;
    int64_t* counts = nullptr;  // written by the count pass, read by the emit pass
    const int64_t* offs = nullptr;
    int64_t pool_base = 0;
    uint64_t* pool = nullptr;
    int64_t pool_n = 0;
    int qa = 0, qb = 0;
};

int flat_ivf_range_group(int group);

// The arguments are those of the scan of the same row format; d_qnorm as in launch_flat_ivf_scan_u8.
hipError_t launch_flat_ivf_range(const FlatIvfLists& lists, const float* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                                 const uint32_t* d_svals, int group, const FlatIvfRange& range, hipStream_t stream);
hipError_t launch_flat_ivf_range_narrow(const FlatIvfListsNarrow& lists, const float* d_queries, int nq, int nprobe,
                                        const uint32_t* d_skeys, const uint32_t* d_svals, int group, const FlatIvfRange& range,
                                        hipStream_t stream);
hipError_t launch_flat_ivf_range_u8(const FlatIvfListsU8& lists, const int8_t* d_queries, const int32_t* d_qnorm, int nq, int nprobe,
                                    const uint32_t* d_skeys, const uint32_t* d_svals, int group, const FlatIvfRange& range,
                                    hipStream_t stream);
hipError_t launch_flat_ivf_range_bits(const FlatIvfListsBits& lists, const uint32_t* d_queries, int nq, int nprobe,
                                      const uint32_t* d_skeys, const uint32_t* d_svals, int group, const FlatIvfRange& range,
                                      hipStream_t stream);

}  // namespace dpq
