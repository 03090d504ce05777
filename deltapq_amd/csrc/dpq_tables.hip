// dpq_tables.hip -- gfx950 kernels of the search by caller-supplied distance tables and of the inner-product search
// built on it (include/deltapq_amd.h "Search by distance tables").
//
//   tables_ingest_kernel   stands where lut_build_kernel stands for a batch whose tables the caller made: copies
//                          tables[q][m][0..K) into the workspace's [q][m][256] layout (and the labelled copy), writes the
//                          partial minima, clears the slots' overflow words and tightening histograms, and replaces an
//                          entry no kernel downstream may see (negative, -inf, NaN) by +inf, raising one flag word.
//   ip_tables_kernel       p[m][k] = <q_m, c[m][k]> in fp64, top[m] = max_k p, e = top - p >= 0, B = sum_m top[m].
//   ip_scores_kernel       score = B - gap.
#include "dpq_tables.h"

#include <algorithm>
#include <cmath>

#include "dpq_kernels.h"

namespace dpq {

// grid = (n_slots, M), block = 256: one thread per entry of the [slot][m][256] table.
__global__ __launch_bounds__(256) void tables_ingest_kernel(const float* __restrict__ tables, int nq, int n_slots, int M,
                                                             int K, float* __restrict__ lut, float* __restrict__ lut_min,
                                                             uint32_t* __restrict__ overflow,
                                                             const uint8_t* __restrict__ relabel,
                                                             float* __restrict__ lut_labels,
                                                             uint32_t* __restrict__ tight_hist, uint32_t* __restrict__ bad) {
    // the same place in a batch as lut_build_kernel, so the same wave priority and, for its reason, no LDS (see there)
    __builtin_amdgcn_s_setprio(DPQ_UNDER_SCAN_PRIO);
    const int q = blockIdx.x, m = blockIdx.y, k = threadIdx.x;
    if (m == 0) {  // (q < n_slots: the grid is n_slots wide)
        if (k == 0 && overflow) overflow[q] = 0;
        // the first filter level's tightening histogram of this slot (scan_kernel)
        if (tight_hist)
            for (int i = k; i < kTightWords; i += 256) tight_hist[(size_t)q * kTightWords + i] = 0;
    }
    if (q >= nq) return;  // a padding slot
    float v = INFINITY;   // centroids beyond K do not exist; no valid code points at them
    if (k < K) {
        v = tables[((size_t)q * M + m) * K + k];
        if (!(v >= 0.0f)) {  // negative, -inf or NaN: the scan orders distances as unsigned bit patterns
            v = INFINITY;
            *bad = 1u;  // every thread that finds one stores the same word
        }
    }
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;  // -0.0 is +0.0
    v = __uint_as_float(b);
    lut[((size_t)q * M + m) * 256 + k] = v;
    if (lut_labels) lut_labels[((size_t)q * M + m) * 256 + relabel[m * 256 + k]] = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = min(b, (uint32_t)__shfl_xor((int)b, o));  // v >= 0: uint order == float order
    if ((k & 63) == 0) lut_min[((size_t)q * M + m) * kLutMinParts + (k >> 6)] = __uint_as_float(b);
}

// grid = ceil(nq / kIpQueries), block = 256: thread k owns centroid k; the block walks the sub-spaces in ascending m, so
// that one thread adds the maxima into B in the order of the rule.  This kernel runs ahead of a batch, not under a scan,
// so its block-wide maximum goes through LDS (64 B).
__global__ __launch_bounds__(256) void ip_tables_kernel(const float* __restrict__ codebook, const float* __restrict__ queries,
                                                         int nq, int M, int K, int Ds, float* __restrict__ tables,
                                                         float* __restrict__ bias) {
    __shared__ float wave_top[4][kIpQueries];
    const int q0 = blockIdx.x * kIpQueries, k = threadIdx.x;
    const int nj = min(kIpQueries, nq - q0);
    const size_t qstride = (size_t)M * Ds;
    double B[kIpQueries];
#pragma unroll
    for (int j = 0; j < kIpQueries; ++j) B[j] = 0.0;
    for (int m = 0; m < M; ++m) {
        double acc[kIpQueries];
#pragma unroll
        for (int j = 0; j < kIpQueries; ++j) acc[j] = 0.0;
        if (k < K) {
            const float* c = codebook + ((size_t)m * K + k) * Ds;
            const float* qv = queries + (size_t)q0 * qstride + (size_t)m * Ds;  // query j: qv + j * qstride (clamped)
            for (int d = 0; d < Ds; ++d) {
                const double cv = (double)c[d];
#pragma unroll
                for (int j = 0; j < kIpQueries; ++j)  // wave-uniform address: a scalar load
                    acc[j] = __fma_rn((double)qv[(size_t)min(j, nj - 1) * qstride + d], cv, acc[j]);
            }
        }
        float p[kIpQueries];
#pragma unroll
        for (int j = 0; j < kIpQueries; ++j) {
            p[j] = k < K ? (float)acc[j] : -INFINITY;
            float t = p[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t = fmaxf(t, __shfl_xor(t, o));
            if ((k & 63) == 0) wave_top[k >> 6][j] = t;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kIpQueries; ++j) {
            const float top = fmaxf(fmaxf(wave_top[0][j], wave_top[1][j]), fmaxf(wave_top[2][j], wave_top[3][j]));
            B[j] = __dadd_rn(B[j], (double)top);
            if (k < K && j < nj) tables[((size_t)(q0 + j) * M + m) * K + k] = __fsub_rn(top, p[j]);
        }
        __syncthreads();  // wave_top is written again for the next sub-space
    }
    if (k == 0) {
#pragma unroll
        for (int j = 0; j < kIpQueries; ++j)
            if (j < nj) bias[q0 + j] = (float)B[j];
    }
}

__global__ __launch_bounds__(256) void ip_scores_kernel(const float* __restrict__ bias, const float* __restrict__ gaps,
                                                         const int32_t* __restrict__ ids, int top_k, int64_t n,
                                                         float* __restrict__ scores) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    scores[i] = ids[i] < 0 ? -INFINITY : (float)__dsub_rn((double)bias[i / top_k], (double)gaps[i]);
}

hipError_t launch_tables_ingest(const float* d_tables, int nq, int n_slots, int M, int K, float* d_lut32, float* d_lut_min,
                                uint32_t* d_overflow, const uint8_t* d_relabel, float* d_lut_labels, uint32_t* d_tight_hist,
                                uint32_t* d_bad, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    n_slots = std::max(n_slots, nq);
    hipLaunchKernelGGL(tables_ingest_kernel, dim3((unsigned)n_slots, (unsigned)M), dim3(256), 0, stream, d_tables, nq, n_slots,
                       M, K, d_lut32, d_lut_min, d_overflow, d_relabel, d_relabel ? d_lut_labels : nullptr, d_tight_hist,
                       d_bad);
    return hipGetLastError();
}

hipError_t launch_ip_tables(const float* d_codebook, const float* d_queries, int nq, int M, int K, int Ds, float* d_tables,
                            float* d_bias, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(ip_tables_kernel, dim3((unsigned)((nq + kIpQueries - 1) / kIpQueries)), dim3(256), 0, stream,
                       d_codebook, d_queries, nq, M, K, Ds, d_tables, d_bias);
    return hipGetLastError();
}

hipError_t launch_ip_scores(const float* d_bias, const float* d_gaps, const int32_t* d_ids, int nq, int top_k,
                            float* d_scores, hipStream_t stream) {
    const int64_t n = (int64_t)nq * top_k;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ip_scores_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_bias, d_gaps, d_ids,
                       top_k, n, d_scores);
    return hipGetLastError();
}

}  // namespace dpq
