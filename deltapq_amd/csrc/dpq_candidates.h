// dpq_candidates.h -- launch interface of the candidate search kernels (dpq_candidates.hip): the plain one-level ADC
// distance of every id of a per-query candidate list, from the query's exact table and the candidates' level-1 codes
// (include/deltapq_amd.h "candidate search").
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dpq_refine.h"

namespace dpq {

constexpr int kCandMaxCand = kRefineMaxCand;  // candidates per query: the bound of every re-ranker and of the LDS sort
constexpr int kCandSlice = (int)kRefineSlice; // candidates one pass takes
constexpr int kCandSliceQueries = 2048;       // ... and queries: their tables stay within 2048 * M KB

// What a candidate is to a handle.  kCandLocal: it names one of the handle's nodes.  kCandSkip: padding (negative), or a
// node of the index that another handle holds (its position lies in [0, n_total) outside the handle's range).
// kCandNone: it names no node of the whole index -- beyond n_total, n_total - 1 of an even-N DTC index, n_total of a
// plain one.  The rule is the code lookup's (dpq_refine.h, RefineIds), with the other shards' nodes told apart.
enum { kCandLocal = 1, kCandSkip = 0, kCandNone = -1 };
__host__ __device__ inline int cand_classify(int32_t id, const RefineIds& r) {
    if (id < 0) return kCandSkip;
    int64_t pos = id;
    if (r.even_rule && (r.n_total & 1) == 0) {
        if (pos == r.n_total)
            pos = r.n_total - 1;
        else if (pos == r.n_total - 1)
            return kCandNone;
    }
    if (pos >= r.n_total) return kCandNone;
    const int64_t l = pos - r.id_base;
    return l >= 0 && l < r.n_local ? kCandLocal : kCandSkip;
}

size_t cand_keys(int n_cand);  // keys per query launch_cand_adc writes in emit mode: n_cand rounded up to a power of two

// d_out[i] = d_cand[i] where it names a node of the handle, -1 where it is padding or another handle's node; *d_flag is
// set to 1 by every candidate that names no node of the index (its entry is -1 too).
hipError_t launch_cand_classify(const int32_t* d_cand, int64_t n, const RefineIds& ids, int32_t* d_out, uint32_t* d_flag,
                                hipStream_t stream);

// The distances of d_local[nq][n_cand] (launch_cand_classify's output) under d_lut32[nq][M][256], from the candidates'
// codes d_codes[nq][n_cand][M] (M = 8 or 16; 16-byte aligned).  plain_rule: M fp32 additions in ascending m; else the
// fp64 sum in ascending m, rounded once.  d_keys != NULL: keys `distance bits << 32 | id` to d_keys[q][cand_keys(n_cand)]
// (entries j < n_cand; kFlatNoKey for a -1), nothing else is written.  d_keys == NULL: floats to d_dists[nq][n_cand],
// a quiet NaN for a -1.
hipError_t launch_cand_adc(const float* d_lut32, int nq, const int32_t* d_local, int n_cand, const uint8_t* d_codes, int M,
                           bool plain_rule, uint64_t* d_keys, float* d_dists, hipStream_t stream);

}  // namespace dpq
