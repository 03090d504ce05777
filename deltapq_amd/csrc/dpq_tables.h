// dpq_tables.h -- launch interface of the table kernels (dpq_tables.hip): a batch's distance tables from the caller
// instead of lut_build_kernel, and the inner-product tables built on that (include/deltapq_amd.h "Search by distance
// tables").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dpq {

constexpr int kIpQueries = 4;  // queries one block of ip_tables_kernel serves

// What launch_lut_build does to a workspace, from d_tables[nq][M][K] instead of queries and a codebook: lut32, its
// labelled copy (d_relabel != NULL), the four partial minima per (query, m), the cleared overflow words and tightening
// histograms of slots [0, n_slots).  An entry that is negative, -inf or a NaN becomes +inf and sets *d_bad to 1 (nothing
// clears it here); -0.0 becomes +0.0.  Columns K .. 255 are +inf.
hipError_t launch_tables_ingest(const float* d_tables, int nq, int n_slots, int M, int K, float* d_lut32, float* d_lut_min,
                                uint32_t* d_overflow, const uint8_t* d_relabel, float* d_lut_labels, uint32_t* d_tight_hist,
                                uint32_t* d_bad, hipStream_t stream);

// d_tables[nq][M][K] = top[m] - p[m][k] and d_bias[nq] of the inner-product rule (include/deltapq_amd.h).  No allocation.
hipError_t launch_ip_tables(const float* d_codebook, const float* d_queries, int nq, int M, int K, int Ds, float* d_tables,
                            float* d_bias, hipStream_t stream);

// d_scores[q][j] = (float)((double)d_bias[q] - (double)d_gaps[q][j]), -inf where d_ids[q][j] < 0.
hipError_t launch_ip_scores(const float* d_bias, const float* d_gaps, const int32_t* d_ids, int nq, int top_k,
                            float* d_scores, hipStream_t stream);

}  // namespace dpq
