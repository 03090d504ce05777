// dpq_procrustes.h -- the orthogonal Procrustes solve of OPQ (dpq_procrustes.cpp): host code in fp64, no HIP.
// The stated arithmetic is in include/deltapq_amd.h "OPQ / Procrustes".
#pragma once

namespace dpq {

constexpr int kProcrustesMaxD = 1024;
constexpr int kProcrustesMaxSweeps = 64;

// R_out (double [D][D], row-major) = the orthogonal polar factor U . V^T of C = U . S . V^T (double [D][D]).
// *degenerate = 1 and R_out untouched when the factor is not unique to working precision (smallest singular value at
// or below D * 2^-52 times the largest) or an entry of C is not finite.  The caller has checked the arguments
// (1 <= D <= kProcrustesMaxD, no NULL); sweeps_out may be NULL.
void procrustes(const double* C, int D, double* R_out, int* degenerate, int* sweeps_out);

// max |R^T R - I| over the entries, fp64: column sums in ascending row order.
double orthogonality_residual(const float* R, int D);

}  // namespace dpq
