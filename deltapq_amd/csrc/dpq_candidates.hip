// dpq_candidates.hip -- candidate search on gfx950: the plain asymmetric distance of every id of a
// per-query candidate list.  The distance of a candidate is what the scans give the same node: the M entries
// T[m][code[m]] of the query's exact table, summed in ascending m -- in fp64 and rounded once (a DTC handle), or in
// fp32 with M roundings (a dpq_open_plain_* handle).  The build passes -ffp-contract=off; there is nothing to fuse
// here anyway, a sum has no product.
//
//   cand_classify_kernel  a thread per candidate of a slice: the id kept where it names one of the handle's nodes, -1
//                         where it is padding or another handle's node; a flag word where it names no node at all.
//   cand_adc_kernel       a lane per candidate, 256 candidates of one query per workgroup.  The query's table
//                         (M x 256 fp32: 8 KB at M = 8, 16 KB at M = 16) goes to LDS once with 16-byte loads; a lane
//                         loads its code as one 8- or 16-byte word and gathers its M entries with one 4-byte LDS read
//                         each.  The gathers are random by nature (64 lanes into 256 words of a sub-space on the LDS's
//                         banks); nothing is laid out around that.  Keys go to a buffer that flat_sort_emit_kernel
//                         sorts; the distance form writes the floats in place.
#include "dpq_candidates.h"

#include <algorithm>

#include "dpq_flat.h"

namespace dpq {
namespace {

constexpr uint32_t kNaNBits = 0x7FC00000u;

__global__ __launch_bounds__(256) void cand_classify_kernel(const int32_t* __restrict__ cand, int64_t n, const RefineIds rid,
                                                            int32_t* __restrict__ out, uint32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t c = cand[i];
    const int cls = cand_classify(c, rid);
    if (cls == kCandNone) *flag = 1u;  // every thread that finds one stores the same word
    out[i] = cls == kCandLocal ? c : -1;
}

// grid (candidate groups of 256, queries), 256 threads: lane = candidate.  local[q][ci] is the candidate's id (the
// caller's own, so the id the answer reports) or -1.
template <int M, bool PLAIN_RULE, bool EMIT>
__global__ __launch_bounds__(256) void cand_adc_kernel(const float* __restrict__ lut32, const int32_t* __restrict__ local,
                                                       int n_cand, int n_pad, const uint8_t* __restrict__ codes,
                                                       uint64_t* __restrict__ keys, float* __restrict__ dists) {
    __shared__ __attribute__((aligned(16))) float T[M * 256];
    const int q = blockIdx.y, tid = threadIdx.x;
    const int ci = blockIdx.x * 256 + tid;
    const float4* src = reinterpret_cast<const float4*>(lut32 + (size_t)q * M * 256);
#pragma unroll
    for (int i = 0; i < M / 4; ++i) reinterpret_cast<float4*>(T)[i * 256 + tid] = src[i * 256 + tid];
    int32_t c = -1;
    uint32_t w[M / 4];
#pragma unroll
    for (int k = 0; k < M / 4; ++k) w[k] = 0u;
    if (ci < n_cand) {
        const size_t at = (size_t)q * n_cand + ci;
        c = local[at];
        if (c >= 0) {  // (a row without a node: the lookup left zero bytes there; it is not read)
            if constexpr (M == 8) {
                const uint2 v = reinterpret_cast<const uint2*>(codes)[at];
                w[0] = v.x; w[1] = v.y;
            } else {
                const uint4 v = reinterpret_cast<const uint4*>(codes)[at];
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            }
        }
    }
    __syncthreads();
    if (ci >= n_cand) return;
    [[maybe_unused]] double acc64 = 0.0;
    [[maybe_unused]] float acc32 = 0.0f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float e = T[m * 256 + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)];
        if constexpr (PLAIN_RULE)
            acc32 = __fadd_rn(acc32, e);
        else
            acc64 = __dadd_rn(acc64, (double)e);
    }
    const float d = PLAIN_RULE ? acc32 : (float)acc64;
    if constexpr (EMIT)
        keys[(size_t)q * n_pad + ci] = c >= 0 ? ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)c : kFlatNoKey;
    else
        dists[(size_t)q * n_cand + ci] = c >= 0 ? d : __uint_as_float(kNaNBits);
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

template <int M, bool PLAIN_RULE>
void launch_adc(const dim3& grid, const float* lut32, const int32_t* local, int n_cand, int n_pad, const uint8_t* codes,
                uint64_t* keys, float* dists, hipStream_t stream) {
    if (keys)
        cand_adc_kernel<M, PLAIN_RULE, true><<<grid, dim3(256), 0, stream>>>(lut32, local, n_cand, n_pad, codes, keys, dists);
    else
        cand_adc_kernel<M, PLAIN_RULE, false><<<grid, dim3(256), 0, stream>>>(lut32, local, n_cand, n_pad, codes, keys, dists);
}

}  // namespace

size_t cand_keys(int n_cand) { return (size_t)pow2_at_least(n_cand); }

hipError_t launch_cand_classify(const int32_t* d_cand, int64_t n, const RefineIds& ids, int32_t* d_out, uint32_t* d_flag,
                                hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_cand || !d_out || !d_flag || n > ((int64_t)1 << 38)) return hipErrorInvalidValue;
    cand_classify_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(d_cand, n, ids, d_out, d_flag);
    return hipGetLastError();
}

hipError_t launch_cand_adc(const float* d_lut32, int nq, const int32_t* d_local, int n_cand, const uint8_t* d_codes, int M,
                           bool plain_rule, uint64_t* d_keys, float* d_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!d_lut32 || !d_local || !d_codes || (!d_keys && !d_dists) || (M != 8 && M != 16) || n_cand < 1 ||
        n_cand > kCandMaxCand || (reinterpret_cast<uintptr_t>(d_codes) & (uintptr_t)(M - 1)) ||
        (reinterpret_cast<uintptr_t>(d_lut32) & 15u))
        return hipErrorInvalidValue;
    const int n_pad = pow2_at_least(n_cand);
    for (int q0 = 0; q0 < nq; q0 += 65535) {  // the grid's y extent
        const int m = std::min(65535, nq - q0);
        const dim3 grid((n_cand + 255) / 256, m);
        const float* lp = d_lut32 + (size_t)q0 * M * 256;
        const int32_t* cp = d_local + (size_t)q0 * n_cand;
        const uint8_t* bp = d_codes + (size_t)q0 * n_cand * M;
        uint64_t* kp = d_keys ? d_keys + (size_t)q0 * n_pad : nullptr;
        float* dp = d_dists ? d_dists + (size_t)q0 * n_cand : nullptr;
        if (M == 8) {
            if (plain_rule)
                launch_adc<8, true>(grid, lp, cp, n_cand, n_pad, bp, kp, dp, stream);
            else
                launch_adc<8, false>(grid, lp, cp, n_cand, n_pad, bp, kp, dp, stream);
        } else {
            if (plain_rule)
                launch_adc<16, true>(grid, lp, cp, n_cand, n_pad, bp, kp, dp, stream);
            else
                launch_adc<16, false>(grid, lp, cp, n_cand, n_pad, bp, kp, dp, stream);
        }
    }
    return hipGetLastError();
}

}  // namespace dpq
