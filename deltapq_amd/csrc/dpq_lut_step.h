// dpq_lut_step.h -- one dimension of an exact distance-table entry, for the kernels that build such tables
// (lut_build_kernel in dpq_kernels.hip, ivf_scan_residual_kernel in dpq_ivf_residual.hip): one body, so that a table made
// inside a list scan is the table the table build makes, to the bit.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace dpq {

// h:2845-2846: `float += pow(float - float, 2)`, d ascending
__device__ __forceinline__ void lut_step(float& a, float cv, float qd) {
    const float diff = __fsub_rn(cv, qd);                      // fp32 subtract
    const double sq = __dmul_rn((double)diff, (double)diff);   // pow(.,2): exact in fp64
    a = (float)__dadd_rn((double)a, sq);                       // float += double
}

}  // namespace dpq
