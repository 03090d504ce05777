// dpq_refine.hip -- residual re-ranking on gfx950: a second product quantizer over the residuals
// v - reconstruct(code(v)) of the first; a PQ shortlist is re-ranked by the distance to a + b, the sum of the two
// levels' codewords, without the raw vectors on the GPU.
//
// The arithmetic (include/deltapq_amd.h, "residual re-ranking"): x[j] = a[j] + b[j], one fp32 add; then the exact
// search's rule over the row x: per dimension, in ascending order, t = x[j] - q[j] and s = t * t in fp32, each rounded
// on its own (the build passes -ffp-contract=off), acc += (double)s from +0.0; the distance is (float)acc.  One lane
// owns one distance from the first dimension to the last.
//
//   refine_residual_kernel     a thread per output float: v[j] - a[j].
//   refine_reconstruct_kernel  a thread per output float: a[j] + b[j].
//   refine_rerank_kernel       a lane per candidate, 256 candidates of one query per workgroup.  A wavefront keeps its
//                              64 candidates' codes of both levels in LDS and builds their rows of x there, 32
//                              dimensions at a time: eight lanes fetch the eight 16-byte pieces of a row's slice from
//                              the two codebooks (they stay in L2: 2 x 128 KB at M = 8, K = 256, Ds = 16), add them and
//                              store them transposed; every lane then walks its own row in order against the query
//                              slice in LDS.  Keys go to a buffer that flat_sort_emit_kernel sorts.
#include "dpq_refine.h"

#include <algorithm>

#include "dpq_flat.h"

namespace dpq {
namespace {

constexpr int DC = 32;   // dimensions staged at a time
// Row stride of the transposed tile in floats.  A store instruction banks the 32 lanes of a half-wavefront by
// (address / 4) % 32; they hold 4 candidates x 8 pieces and write word (4 piece + k) * LD + candidate, which is
// 4 piece + candidate + const (mod 32) for LD = 65: 32 different banks.  The reads of the walk are consecutive words.
constexpr int LD = 65;
constexpr int C1W = 5;   // words of a candidate's level-1 code in LDS (M <= 16 bytes, one word of padding)
constexpr int C2S = 68;  // bytes of a candidate's level-2 code in LDS (M2 <= 64, padded by a word)
constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kNaNBits = 0x7FC00000u;

// Local position of the node a reported id names, -1 if it names none: global DFS positions, the opened prefix, the
// even-N rule -- the code lookup's rule.
__device__ __forceinline__ int64_t refine_local(int32_t id, const RefineIds& r) {
    if (id < 0) return -1;
    int64_t pos = id;
    if (r.even_rule && (r.n_total & 1) == 0) {
        if (pos == r.n_total)
            pos = r.n_total - 1;
        else if (pos == r.n_total - 1)
            return -1;
    }
    const int64_t l = pos - r.id_base;
    return l >= 0 && l < r.n_local ? l : -1;
}

__global__ __launch_bounds__(256) void refine_residual_kernel(const float* __restrict__ rows, int64_t n, int D,
                                                              const int32_t* __restrict__ ids,
                                                              const uint8_t* __restrict__ codes1, const RefineLevelArgs lv,
                                                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * lv.D1) return;
    const int64_t r = i / lv.D1;
    const int j = (int)(i - r * lv.D1);
    float f = __uint_as_float(kNaNBits);
    if (!ids || ids[r] >= 0) {
        const int m = j / lv.Ds, d = j - m * lv.Ds;
        const int c = codes1[(size_t)r * lv.M + m];
        if (c < lv.K) {
            const float v = j < D ? rows[(size_t)r * D + j] : 0.0f;
            f = v - lv.cw1[((size_t)m * lv.K + c) * lv.Ds + d];
        }
    }
    out[i] = f;
}

__global__ __launch_bounds__(256) void refine_reconstruct_kernel(const int32_t* __restrict__ ids, int64_t n,
                                                                 const uint8_t* __restrict__ codes1,
                                                                 const RefineLevelArgs lv, const RefineIds rid,
                                                                 float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * lv.D1) return;
    const int64_t r = i / lv.D1;
    const int j = (int)(i - r * lv.D1);
    float f = __uint_as_float(kNaNBits);
    const int64_t local = refine_local(ids[r], rid);
    if (local >= 0) {
        const int m = j / lv.Ds, d = j - m * lv.Ds;
        const int m2 = j / lv.Ds2, d2 = j - m2 * lv.Ds2;
        const int c = codes1[(size_t)r * lv.M + m];
        const int c2 = lv.codes2[(size_t)local * lv.M2 + m2];
        if (c < lv.K && c2 < lv.K2) {
            const float a = lv.cw1[((size_t)m * lv.K + c) * lv.Ds + d];
            const float b = lv.cw2[((size_t)m2 * lv.K2 + c2) * lv.Ds2 + d2];
            f = a + b;
        }
    }
    out[i] = f;
}

// grid (candidate groups of 256, queries), 256 threads: lane = candidate.  VEC: Ds and Ds2 are multiples of four, so a
// 16-byte piece of a row lies inside one codeword of either level and is 16-byte aligned in both codebooks.
template <bool VEC>
__global__ __launch_bounds__(256) void refine_rerank_kernel(const float* __restrict__ queries,
                                                            const int32_t* __restrict__ cand, int n_cand, int n_pad,
                                                            const uint8_t* __restrict__ codes1, const RefineLevelArgs lv,
                                                            const RefineIds rid, uint64_t* __restrict__ keys,
                                                            uint32_t* flag) {
    __shared__ float tile[4][DC][LD];
    __shared__ float qv[DC];
    __shared__ int32_t off1[DC], off2[DC];  // per dimension of the slice: where its float sits in codeword 0 of its sub-space
    __shared__ uint8_t sub1[DC], sub2[DC];  // and the sub-space
    __shared__ uint32_t c1w[4][64][C1W];
    __shared__ uint8_t c2s[4][64][C2S];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ci = blockIdx.x * 256 + tid;
    if (blockIdx.x * 256 >= n_cand) {  // (a whole workgroup) the padding of the key buffer
        if (ci < n_pad) keys[(size_t)q * n_pad + ci] = kNoKey;
        return;
    }
    int32_t c = -1;
    int64_t local = -1;
    if (ci < n_cand) {
        c = cand[(size_t)q * n_cand + ci];
        if (c >= 0) {  // a negative candidate is padding
            local = refine_local(c, rid);
            if (local < 0) *flag = 1;  // names no node
        }
    }
    // the candidate's codes; a row without a node stages code 0 everywhere and is dropped at the end
    const int W1 = lv.M >> 2;
    for (int k = 0; k < W1; ++k)
        c1w[w][lane][k] =
            local >= 0 ? reinterpret_cast<const uint32_t*>(codes1)[((size_t)q * n_cand + ci) * W1 + k] : 0u;
    for (int k = 0; k < lv.M2; ++k) c2s[w][lane][k] = local >= 0 ? lv.codes2[(size_t)local * lv.M2 + k] : (uint8_t)0;

    double acc = 0.0;
    const int D1 = lv.D1;
    const int lj = (lane & 7) * 4;
    for (int d0 = 0; d0 < D1; d0 += DC) {
        if (tid < DC) {
            const int j = d0 + tid;
            int m = 0, o1 = 0, m2 = 0, o2 = 0;
            float qf = 0.0f;
            if (j < D1) {
                m = j / lv.Ds;
                o1 = m * lv.K * lv.Ds + (j - m * lv.Ds);
                m2 = j / lv.Ds2;
                o2 = m2 * lv.K2 * lv.Ds2 + (j - m2 * lv.Ds2);
                qf = queries[(size_t)q * D1 + j];
            }
            sub1[tid] = (uint8_t)m;
            off1[tid] = o1;
            sub2[tid] = (uint8_t)m2;
            off2[tid] = o2;
            qv[tid] = qf;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int cc = it * 8 + (lane >> 3);
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {
                if (d0 + lj < D1) {
                    const int m = sub1[lj];
                    const int k1 = (int)((c1w[w][cc][m >> 2] >> (8 * (m & 3))) & 0xffu);
                    const int k2 = c2s[w][cc][sub2[lj]];
                    if (k1 < lv.K) {
                        const float4 a = *reinterpret_cast<const float4*>(lv.cw1 + off1[lj] + (size_t)k1 * lv.Ds);
                        const float4 b = *reinterpret_cast<const float4*>(lv.cw2 + off2[lj] + (size_t)k2 * lv.Ds2);
                        x[0] = a.x + b.x; x[1] = a.y + b.y; x[2] = a.z + b.z; x[3] = a.w + b.w;
                    } else {
                        x[0] = x[1] = x[2] = x[3] = __uint_as_float(kNaNBits);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int dl = lj + k;
                    if (d0 + dl < D1) {
                        const int m = sub1[dl];
                        const int k1 = (int)((c1w[w][cc][m >> 2] >> (8 * (m & 3))) & 0xffu);
                        const int k2 = c2s[w][cc][sub2[dl]];
                        if (k1 < lv.K) {
                            const float a = lv.cw1[off1[dl] + (size_t)k1 * lv.Ds];
                            const float b = lv.cw2[off2[dl] + (size_t)k2 * lv.Ds2];
                            x[k] = a + b;
                        } else {
                            x[k] = __uint_as_float(kNaNBits);
                        }
                    }
                }
            }
            tile[w][lj + 0][cc] = x[0]; tile[w][lj + 1][cc] = x[1]; tile[w][lj + 2][cc] = x[2]; tile[w][lj + 3][cc] = x[3];
        }
        __syncthreads();
        const int dc = min(DC, D1 - d0);
#pragma unroll 8
        for (int d = 0; d < dc; ++d) {
            const float t = tile[w][d][lane] - qv[d];
            const float s = t * t;
            acc += (double)s;
        }
        __syncthreads();
    }
    if (ci < n_pad)
        keys[(size_t)q * n_pad + ci] =
            local >= 0 ? ((uint64_t)__float_as_uint((float)acc) << 32) | (uint32_t)c : kNoKey;
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

bool level_ok(const RefineLevelArgs& lv) {
    return lv.cw1 && lv.M >= 4 && lv.M <= 16 && (lv.M & 3) == 0 && lv.K >= 1 && lv.K <= 256 && lv.Ds >= 1 &&
           lv.D1 == lv.M * lv.Ds;
}

}  // namespace

size_t refine_rerank_keys(int n_cand) { return (size_t)pow2_at_least(n_cand); }

hipError_t launch_refine_residual(const float* d_rows, int64_t n, int D, const int32_t* d_ids, const uint8_t* d_codes1,
                                  const RefineLevelArgs& lv, float* d_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t total = n * lv.D1;
    if (!level_ok(lv) || !d_rows || !d_codes1 || !d_out || D < 1 || D > lv.D1 || total > ((int64_t)1 << 38))
        return hipErrorInvalidValue;
    refine_residual_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(d_rows, n, D, d_ids, d_codes1,
                                                                                          lv, d_out);
    return hipGetLastError();
}

hipError_t launch_refine_reconstruct(const int32_t* d_ids, int64_t n, const uint8_t* d_codes1, const RefineLevelArgs& lv,
                                     const RefineIds& ids, float* d_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t total = n * lv.D1;
    if (!level_ok(lv) || !lv.cw2 || !lv.codes2 || !d_ids || !d_codes1 || !d_out || total > ((int64_t)1 << 38))
        return hipErrorInvalidValue;
    refine_reconstruct_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(d_ids, n, d_codes1, lv, ids,
                                                                                             d_out);
    return hipGetLastError();
}

hipError_t launch_refine_rerank(const float* d_queries, int nq, const int32_t* d_cand, int n_cand, int top_k,
                                const uint8_t* d_codes1, const RefineLevelArgs& lv, const RefineIds& ids, uint64_t* d_keys,
                                uint32_t* d_flag, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!level_ok(lv) || !lv.cw2 || !lv.codes2 || lv.M2 < 1 || lv.M2 > kRefineMaxM2 || lv.K2 < 1 || lv.K2 > 256 ||
        lv.Ds2 < 1 || (int64_t)lv.M2 * lv.Ds2 < lv.D1 || top_k < 1 || top_k > n_cand || n_cand > kRefineMaxCand ||
        (reinterpret_cast<uintptr_t>(d_codes1) & 3u))
        return hipErrorInvalidValue;
    const int n_pad = pow2_at_least(n_cand);
    const bool vec = (lv.Ds & 3) == 0 && (lv.Ds2 & 3) == 0;
    for (int q0 = 0; q0 < nq; q0 += 65535) {  // the grid's y extent
        const int m = std::min(65535, nq - q0);
        const dim3 grid((n_pad + 255) / 256, m), block(256);
        const float* qp = d_queries + (size_t)q0 * lv.D1;
        const int32_t* cp = d_cand + (size_t)q0 * n_cand;
        const uint8_t* c1 = d_codes1 + (size_t)q0 * n_cand * lv.M;
        uint64_t* kp = d_keys + (size_t)q0 * n_pad;
        if (vec)
            refine_rerank_kernel<true><<<grid, block, 0, stream>>>(qp, cp, n_cand, n_pad, c1, lv, ids, kp, d_flag);
        else
            refine_rerank_kernel<false><<<grid, block, 0, stream>>>(qp, cp, n_cand, n_pad, c1, lv, ids, kp, d_flag);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_flat_sort_emit(d_keys, (size_t)n_pad, nullptr, nq, n_pad, top_k, d_ids, d_dists, stream);
}

}  // namespace dpq
