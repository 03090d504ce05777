// dpq_opq.h -- launch interface of the OPQ kernels (dpq_opq.hip): the rotation out = x . R and the ordered
// cross-covariance of vectors with their PQ reconstruction (include/deltapq_amd.h "OPQ").
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kOpqMaxD = 1024;                     // dimensions of a rotation
constexpr int64_t kOpqSlice = (int64_t)1 << 20;    // rows one launch (and one host upload) takes
constexpr int kOpqLeaf = 1024;                     // rows of a cross-covariance leaf
constexpr size_t kOpqLeafBytesCap = (size_t)256 << 20;  // device bytes of the leaf sums S[l][D][D] held at once

// out[i][j] = (float)(fp64 sum over d ascending of (double)x[i][d] * (double)R[d][j]), acc from +0.0.  Any n >= 0
// (launched in slices of kOpqSlice rows), 1 <= D <= kOpqMaxD; d_out must not overlap d_x.  No allocation.
hipError_t launch_opq_rotate(const float* d_x, int64_t n, int D, const float* d_R, float* d_out, hipStream_t stream);

// Leaves of kOpqLeaf rows this many bytes of S can hold for dimension D (at least 1).
int64_t opq_cross_leaves_per_pass(int D);

// d_C[d][j] (double [D][D]) = the leaf-ordered sum over rows of (double)x[i][d] * (double)cw[j / Ds][codes[i][j / Ds]][j % Ds],
// D = M * Ds.  d_S: double [min(leaves, opq_cross_leaves_per_pass(D))][D][D] work array.  Every code byte must be < K
// (the caller checks).  n >= 1.
hipError_t launch_opq_cross(const float* d_x, int64_t n, int D, const uint8_t* d_codes, const float* d_cw, int M, int K,
                            int Ds, double* d_S, double* d_C, hipStream_t stream);

}  // namespace dpq
