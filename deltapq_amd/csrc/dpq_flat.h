// dpq_flat.h -- exact L2 search over raw fp32 vectors on the GPU (dpq_flat.hip): ground truth over a whole base,
// re-ranking over a candidate list per query.  The arithmetic is the reference's brute force (main.cpp:150-156),
// restated in include/deltapq_amd.h and DESIGN.md 5.10.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kFlatMaxTopK = 16384;  // DPQ_FLAT_MAX_TOPK, and the most candidates a re-rank takes per query
constexpr int kFlatMaxD = 2048;

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

// Exact top_k of nq (<= flat_query_batch(top_k)) queries over n rows, all device pointers.  d_base [n][Dp],
// d_queries [nq][Dp] (padded rows), d_keys [nq][flat_key_capacity(top_k)], d_state [nq].  Reported id = row + id_offset.
// Enqueues on `stream`; d_state[q].overflow must be read back afterwards.
hipError_t launch_flat_search(const float* d_base, int64_t n, int Dp, const float* d_queries, int nq, int top_k,
                              int64_t id_offset, uint64_t* d_keys, FlatQueryState* d_state, int32_t* d_ids, float* d_dists,
                              hipStream_t stream);

// Exact distances of cand[nq][n_cand] only, best top_k by (distance, reported id).  d_map (may be NULL) [n_map]: a
// candidate is a DFS position, row = map[c], with the even-N rule; without it row = c - id_offset.  d_queries [nq][D]
// unpadded.  d_keys [nq][n_cand rounded up to a power of two].  *d_flag is set when a candidate names no row.
hipError_t launch_flat_rerank(const float* d_base, int64_t n, int D, int Dp, const float* d_queries, int nq,
                              const int32_t* d_cand, int n_cand, int top_k, int64_t id_offset, const uint32_t* d_map,
                              int64_t n_map, uint64_t* d_keys, uint32_t* d_flag, int32_t* d_ids, float* d_dists,
                              hipStream_t stream);
size_t flat_rerank_keys(int n_cand);  // keys per query launch_flat_rerank needs

// [rows][D] -> [rows][Dp] with zero padding, on the device.
hipError_t launch_flat_pad_rows(const float* d_in, int64_t rows, int D, int Dp, float* d_out, hipStream_t stream);

}  // namespace dpq
