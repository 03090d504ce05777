// dpq_filter.h -- launch interface of the filter construction kernels (dpq_filter.hip): every way of producing a
// dpq_filter's device bitmap without a host pass.
//
// The bitmap they write (dpq_filter::bits, what dpq_filter_create uploads): bit l stands for local node id_base + l,
// n_words words cover max(n_local, segments x nodes per segment) nodes, and the bits of nodes at or past n_local are 0
// (the scan reads whole segments' words).  Every build adds the number of bits it set to *count, which the caller
// clears beforehand on the same stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dpq {

// What a kernel needs to know of the handle the filter is for.
struct FilterGeom {
    int64_t base;      // id_base: global DFS position of local node 0
    int64_t n_local;   // nodes of the handle
    int64_t n_words;   // words of the bitmap (>= (n_local + 31) / 32, >= 1)
    int64_t N;         // n_codes_total
    int32_t even;      // 1: DTC handle with even N -- position N - 1 is reported as N, id N - 1 names nothing
    int64_t tail_l;    // local position of that node where this handle holds it, else -1
};

enum FilterOp : int32_t { kFilterAnd = 0, kFilterOr = 1, kFilterAndNot = 2, kFilterXor = 3, kFilterNot = 4 };

// words[(n_bits + 31) / 32] over REPORTED ids -> bits.  No word beyond the source's end is read.
hipError_t launch_filter_reindex(const uint32_t* words, int64_t n_bits, const FilterGeom& g, uint32_t* bits,
                                 unsigned long long* count, hipStream_t stream);
// ids[n] reported ids (< 0: padding; an id that names no node of the handle is skipped) -> bits; invert != 0: every
// node of the handle except the listed ones.  Clears bits first.
hipError_t launch_filter_ids_build(const int32_t* ids, int64_t n, int invert, const FilterGeom& g, uint32_t* bits,
                                   unsigned long long* count, hipStream_t stream);
// reported ids in [lo, hi) (0 <= lo <= hi) -> bits.
hipError_t launch_filter_range(int64_t lo, int64_t hi, const FilterGeom& g, uint32_t* bits, unsigned long long* count,
                               hipStream_t stream);
// words[(n_bits + 31) / 32] over ORIGINAL vector ids, vec_id[n_local] (local node -> vector id) -> bits.
hipError_t launch_filter_gather(const uint32_t* words, int64_t n_bits, const uint32_t* vec_id, const FilterGeom& g,
                                uint32_t* bits, unsigned long long* count, hipStream_t stream);
// out = a op b (b unused for kFilterNot), masked to n_local.
hipError_t launch_filter_combine(const uint32_t* a, const uint32_t* b, FilterOp op, const FilterGeom& g, uint32_t* out,
                                 unsigned long long* count, hipStream_t stream);

// General helpers: a bitmap of (n_bits + 31) / 32 words in any id space.
// mask[n] bytes, non-zero = set -> words_out[(n + 31) / 32]; the tail word is zero-padded.
hipError_t launch_bitmap_from_mask(const uint8_t* mask, int64_t n, uint32_t* words_out, hipStream_t stream);
// ids[n] -> words_out[(n_bits + 31) / 32], cleared first; ids outside [0, n_bits) are skipped.
hipError_t launch_bitmap_from_ids(const int32_t* ids, int64_t n, int64_t n_bits, uint32_t* words_out, hipStream_t stream);

}  // namespace dpq
