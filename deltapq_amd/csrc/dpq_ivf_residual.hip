// dpq_ivf_residual.hip -- the list scan over an index of RESIDUAL codes on gfx950: every node's code is
// the PQ code of x - c_list, so the distance table of a query depends on the list it probes,
//     d(q, x^) = sum_m || (q_m - c_l,m) - cb[m][code_m] ||^2 ,
// and [nq][nprobe][M][256] tables in memory would be written and read once each.  They are made where they are used.
//
//   ivf_scan_residual_kernel  grid (ceil(nprobe / P), queries), 256 threads: a workgroup takes one query and P consecutive
//                          probe columns, P = 1, 2 or 4.  Build: thread k owns codeword k; per sub-space it streams its
//                          codebook row ONCE (16-byte loads where Ds % 4 == 0) and feeds up to P accumulators, one per
//                          live probe of the group -- the codebook (M K Ds floats, 128 KB at M = 8, Ds = 16) is read once
//                          per group, not once per list.  q[d] and c_p[d] are the same for the whole workgroup: scalar
//                          loads, subtracted (fp32, round to nearest) at the point of use, then lut_build_kernel's step
//                          (dpq_lut_step.h).  The P tables go to LDS, [P][M][256] fp32; a probe that is padding, a repeat
//                          or an empty list does no accumulator work and its rows are never written nor read.  Scan: behind
//                          ONE barrier the P lists in turn, each against its own table, by ivf_scan_kernel's stride loop
//                          (ballot, parity words, append below the threshold to 2 P2 keys, sort, threshold refresh); the
//                          count, the parity and the threshold restart per list, behind a barrier.  FILTERED: the entry's
//                          bit is tested before its code is loaded.  Results: the layout launch_merge takes.
//   residual_rows_kernel   a thread per float: out[i][d] = vectors[i][d] - centroids[labels[i]][d], the subtraction the scan
//                          undoes; a label that names no list raises a flag word.
//
// This file is compiled on its own, without the packed fp32 instructions (Makefile).
#include "dpq_ivf.h"

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "dpq_ivf_device.h"
#include "dpq_lut_step.h"

namespace dpq {
namespace {

constexpr int kLdsBytes = 160 * 1024;  // of a gfx950 workgroup

// dynamic LDS: P * M * 256 floats of tables, then `cap` keys.
template <int M, bool PLAIN_RULE, bool FILTERED>
__global__ __launch_bounds__(256) void ivf_scan_residual_kernel(
    const float* __restrict__ codebook, int K, int Ds, const float* __restrict__ queries, const float* __restrict__ centroids,
    const int32_t* __restrict__ probes, int nprobe, int P, const int64_t* __restrict__ offsets, const int32_t* __restrict__ ids,
    const uint8_t* __restrict__ codes, const IvfFilter filt, int top_k, int cap, int32_t* __restrict__ part_ids,
    float* __restrict__ part_dists) {
    __shared__ uint32_t s_wcnt[2][4];  // keys the four wavefronts append in a stride, by the stride's parity
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_smem[];
    float* T = reinterpret_cast<float*>(ivf_smem);                                      // [P][M][256]
    uint64_t* buf = reinterpret_cast<uint64_t*>(ivf_smem + (size_t)P * M * 256 * sizeof(float));  // [cap = 2 P2]
    const int col0 = blockIdx.x * P, q = blockIdx.y, nq = gridDim.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = M * Ds;
    const int ncol = min(P, nprobe - col0);  // columns of this group: the last group may be ragged

    // the group's probes: everything here is uniform over the workgroup
    const float* cen[kIvfResidualGroupMax];
    unsigned live = 0u;
#pragma unroll
    for (int p = 0; p < kIvfResidualGroupMax; ++p) {
        cen[p] = centroids;
        if (p < ncol) {
            const int32_t list = probes[(size_t)q * nprobe + col0 + p];
            if (list >= 0 && offsets[list + 1] > offsets[list]) {
                live |= 1u << p;
                cen[p] = centroids + (size_t)list * D;
            }
        }
    }
    if (live == 0u) {  // nothing but padding, repeats and empty lists
        for (int p = 0; p < ncol; ++p)
            for (int r = tid; r < top_k; r += 256) {
                part_ids[((size_t)(col0 + p) * nq + q) * top_k + r] = -1;
                part_dists[((size_t)(col0 + p) * nq + q) * top_k + r] = INFINITY;
            }
        return;
    }

    // ---- the tables: T[p][m][k] = sum_d (cb[m][k][d] - (q[d] - c_p[d]))^2 by lut_build_kernel's rule, k >= K: +inf ----
    {
        const int k = tid;
        const float* qv = queries + (size_t)q * D;
        for (int m = 0; m < M; ++m) {
            float acc[kIvfResidualGroupMax];
#pragma unroll
            for (int p = 0; p < kIvfResidualGroupMax; ++p) acc[p] = 0.0f;
            if (k < K) {
                const float* c = codebook + ((size_t)m * K + k) * Ds;
                const int o = m * Ds;
                if ((Ds & 3) == 0) {  // rows are 16-byte aligned: one dwordx4 load per 4 dimensions
                    const float4* c4 = reinterpret_cast<const float4*>(c);
                    for (int d = 0; d < Ds; d += 4) {
                        const float4 v = c4[d >> 2];
#pragma unroll
                        for (int p = 0; p < kIvfResidualGroupMax; ++p)
                            if (live & (1u << p)) {
                                const float* qq = qv + o + d;
                                const float* cc = cen[p] + o + d;
                                lut_step(acc[p], v.x, __fsub_rn(qq[0], cc[0]));
                                lut_step(acc[p], v.y, __fsub_rn(qq[1], cc[1]));
                                lut_step(acc[p], v.z, __fsub_rn(qq[2], cc[2]));
                                lut_step(acc[p], v.w, __fsub_rn(qq[3], cc[3]));
                            }
                    }
                } else {
                    for (int d = 0; d < Ds; ++d) {
                        const float cv = c[d];
#pragma unroll
                        for (int p = 0; p < kIvfResidualGroupMax; ++p)
                            if (live & (1u << p)) lut_step(acc[p], cv, __fsub_rn(qv[o + d], cen[p][o + d]));
                    }
                }
            } else {
#pragma unroll
                for (int p = 0; p < kIvfResidualGroupMax; ++p) acc[p] = INFINITY;  // no valid code points at a codeword beyond K
            }
#pragma unroll
            for (int p = 0; p < kIvfResidualGroupMax; ++p)
                if (live & (1u << p)) T[(p * M + m) * 256 + k] = acc[p];
        }
    }
    __syncthreads();

    // ---- the lists in turn: ivf_scan_kernel's stride loop against T[p] ----
    for (int p = 0; p < ncol; ++p) {
        int32_t* out_i = part_ids + ((size_t)(col0 + p) * nq + q) * top_k;
        float* out_d = part_dists + ((size_t)(col0 + p) * nq + q) * top_k;
        if (!(live & (1u << p))) {
            for (int r = tid; r < top_k; r += 256) {
                out_i[r] = -1;
                out_d[r] = INFINITY;
            }
            continue;
        }
        const int32_t list = probes[(size_t)q * nprobe + col0 + p];
        const int64_t lo = offsets[list], hi = offsets[list + 1];
        const float* Tp = T + (size_t)p * M * 256;
        // cnt is a register, the same in every thread (see ivf_scan_kernel); with par and thr it starts afresh per list
        uint32_t cnt = 0u;
        int par = 0;
        uint64_t thr = kFlatNoKey;
        for (int64_t base = lo; base < hi; base += 256, par ^= 1) {
            const int64_t at = base + tid;
            uint64_t key = kFlatNoKey;
            if (at < hi) {
                const int32_t id = ids[at];
                if (!FILTERED || ivf_eligible(filt, id)) key = ivf_entry_key<M, PLAIN_RULE>(Tp, codes, at, id);
            }
            const bool pass = key < thr;  // (padding never passes: thr <= kFlatNoKey)
            const unsigned long long mask = __ballot(pass);
            if (lane == 0) s_wcnt[par][wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            const uint32_t c0 = s_wcnt[par][0], c1 = s_wcnt[par][1], c2 = s_wcnt[par][2], c3 = s_wcnt[par][3];
            const uint32_t wbase = cnt + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);
            if (pass) buf[wbase + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = key;  // < cap: the stride had room
            cnt += c0 + c1 + c2 + c3;
            if (cnt + 256u > (uint32_t)cap && base + 256 < hi) {  // no room for the next stride
                ivf_sort_keys(buf, cnt, tid);
                if (cnt >= (uint32_t)top_k) thr = buf[top_k - 1];
                cnt = min(cnt, (uint32_t)top_k);
            }
        }
        ivf_sort_keys(buf, cnt, tid);
        for (int r = tid; r < top_k; r += 256) {
            const uint64_t key = (uint32_t)r < cnt ? buf[r] : kFlatNoKey;
            out_i[r] = key != kFlatNoKey ? (int32_t)(key & 0xffffffffu) : -1;
            out_d[r] = key != kFlatNoKey ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
        }
        __syncthreads();  // the next list writes the buffer and the parity words this one has just read
    }
}

// (`out` may be `vectors`: a thread reads the float it writes)
__global__ __launch_bounds__(256) void residual_rows_kernel(const float* vectors, const int32_t* __restrict__ labels, int64_t n,
                                                            int D, const float* __restrict__ centroids, int nlist, float* out,
                                                            uint32_t* flag) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n * D) return;
    const int64_t i = at / D;
    const int d = (int)(at % D);
    const int32_t l = labels[i];
    if (l < 0 || l >= nlist) {
        *flag = 1u;  // every thread that finds one stores the same word
        return;
    }
    out[at] = __fsub_rn(vectors[at], centroids[(size_t)l * D + d]);
}

int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

size_t residual_lds(int P, int M, int cap) { return (size_t)P * M * 256 * sizeof(float) + (size_t)cap * sizeof(uint64_t); }

// hipFuncSetAttribute is per device
template <int M, bool PLAIN_RULE, bool FILTERED>
hipError_t ensure_residual_lds() {
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ivf_scan_residual_kernel<M, PLAIN_RULE, FILTERED>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes - 64);  // (the static words)
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

}  // namespace

int ivf_residual_group(int M, int top_k, int group) {
    const int cap = 2 * pow2_at_least(std::max(top_k, 256));
    int P = kIvfResidualGroupMax;
    while (P > 1 && (P > group || residual_lds(P, M, cap) > (size_t)kLdsBytes - 64)) P >>= 1;
    return P;
}

hipError_t launch_ivf_scan_residual(const float* d_codebook, int K, int Ds, const float* d_queries, const float* d_centroids,
                                    int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets, const int32_t* d_ids,
                                    const uint8_t* d_codes, int M, bool plain_rule, const IvfFilter& filter, int top_k, int group,
                                    int32_t* d_part_ids, float* d_part_dists, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (!d_codebook || !d_queries || !d_centroids || !d_probes || !d_offsets || !d_ids || !d_codes || !d_part_ids ||
        !d_part_dists || (M != 8 && M != 16) || K < 1 || K > 256 || Ds < 1 || nprobe < 1 || nprobe > kIvfMaxProbe || top_k < 1 ||
        top_k > kIvfMaxTopK || nq > 65535 || group < 1 || (filter.bits && (filter.n_local < 0 || filter.base < 0 || filter.N < 0)) ||
        (reinterpret_cast<uintptr_t>(d_codes) & (uintptr_t)(M - 1)) ||
        ((Ds & 3) == 0 && (reinterpret_cast<uintptr_t>(d_codebook) & 15u)))
        return hipErrorInvalidValue;
    const int cap = 2 * pow2_at_least(std::max(top_k, 256));
    const int P = ivf_residual_group(M, top_k, group);
    const size_t lds = residual_lds(P, M, cap);
    if (lds > (size_t)kLdsBytes - 64) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nprobe + P - 1) / P), (unsigned)nq), block(256);
    auto run = [&](auto m, auto plain, auto filtered) -> hipError_t {
        constexpr int MM = decltype(m)::value;
        constexpr bool PL = decltype(plain)::value, FI = decltype(filtered)::value;
        if (hipError_t e = ensure_residual_lds<MM, PL, FI>()) return e;
        ivf_scan_residual_kernel<MM, PL, FI><<<grid, block, lds, stream>>>(d_codebook, K, Ds, d_queries, d_centroids, d_probes,
                                                                           nprobe, P, d_offsets, d_ids, d_codes, filter, top_k,
                                                                           cap, d_part_ids, d_part_dists);
        return hipGetLastError();
    };
    auto by_filter = [&](auto m, auto plain) -> hipError_t {
        return filter.bits ? run(m, plain, std::true_type{}) : run(m, plain, std::false_type{});
    };
    auto by_rule = [&](auto m) -> hipError_t { return plain_rule ? by_filter(m, std::true_type{}) : by_filter(m, std::false_type{}); };
    return M == 8 ? by_rule(std::integral_constant<int, 8>{}) : by_rule(std::integral_constant<int, 16>{});
}

hipError_t launch_ivf_residuals(const float* d_vectors, const int32_t* d_labels, int64_t n, int D, const float* d_centroids,
                                int nlist, float* d_out, uint32_t* d_flag, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!d_vectors || !d_labels || !d_centroids || !d_out || !d_flag || D < 1 || nlist < 1) return hipErrorInvalidValue;
    const int64_t rows = std::max<int64_t>(1, ((int64_t)1 << 30) / D);  // of one launch: its grid stays below 2^22 workgroups
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
        const int64_t m = std::min(rows, n - r0);
        residual_rows_kernel<<<dim3((unsigned)((m * D + 255) / 256)), dim3(256), 0, stream>>>(
            d_vectors + (size_t)r0 * D, d_labels + r0, m, D, d_centroids, nlist, d_out + (size_t)r0 * D, d_flag);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace dpq
