// dpq_train.hip -- codebook learning on the GPU (include/deltapq_amd.h: dpq_train_codebook).
//
// Replaces PQ::Learn (pq.cpp:112-157), which hands each sub-space to cv::kmeans.  NO REFERENCE SEMANTICS
// (cv::kmeans): OpenCV's k-means++ start, its three restarts and the parallel shuffle before it
// (main.cpp:262) are not reproducible, so this file defines Lloyd's algorithm, a k-means++ start and a restart
// rule with exact, stated arithmetic; tests/_kmeans_restatement.py and
// tests/_kmeanspp_restatement.py restate them on the CPU bit for bit.
//
// One round, all sub-spaces at once (a sub-space that has stopped is skipped by every kernel):
//   train_assign_kernel   label + winning distance per (vector, sub-space), label histogram, changed count,
//                         per-block distortion sums                                       -- the hot path
//   train_stats_kernel    per sub-space: cluster offsets, empty count, distortion, the stop rule; the host
//                         reads this record back -- the round's only synchronisation
//   hipcub radix sort     (sub-space, label) keys, stable: member lists in ascending vector index
//   train_update_kernel   one thread per (sub-space, cluster, dimension): the ordered fp64 sum and the mean
//   train_repair_kernel   one block per sub-space with empty clusters: top-E by (distance desc, index asc)
// The start is the caller's codebook, K rows drawn on the host, or k-means++ per sub-space on the device
// (train_pp_update_kernel + train_pp_choose_kernel per centre); train_leaf_sum_kernel and the choose kernel's
// chain give the leaf-ordered potential by which restarts are compared.
// The vectors stay on the device for the whole run as sub[m][n][DsP]: one sub-space's sub-vectors
// contiguous and zero padded to the kernel's width, so that a thread's sub-vector is a few 16-byte loads.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/deltapq_amd.h"
#include "dpq_train.h"

namespace dpq {

namespace {

constexpr int kAssignThreads = 256;
constexpr int kRepairThreads = 1024;
constexpr int kMaxK = 256;  // one byte per label; counts / offsets rows are kMaxK wide
constexpr int kLeaf = 256;  // vectors per leaf of the ordered sums: part of the contract (deltapq_amd.h)
constexpr int kChunk = 1024;  // leaf sums train_pp_choose_kernel holds in LDS at a time

struct RoundRec {  // what the host reads per round and sub-space
    int32_t changed, empty;
    double distortion;
};

// vectors: a tile [cnt][D] of the caller's array, its first vector being vector `base` of n.
__global__ __launch_bounds__(256) void train_split_kernel(const float* __restrict__ vectors, int64_t base, int64_t cnt,
                                                           int64_t n, int D, int M, int Ds, int DsP,
                                                           float* __restrict__ sub) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= cnt * M * DsP) return;
    const int d = (int)(gid % DsP), m = (int)((gid / DsP) % M);
    const int64_t v = gid / ((int64_t)DsP * M);
    const int col = m * Ds + d;
    // short vectors are zero padded exactly as encode_pq_kernel pads them (pq.cpp:114-123)
    sub[((size_t)m * n + base + v) * DsP + d] = (d < Ds && col < D) ? vectors[(size_t)v * D + col] : 0.0f;
}

__global__ __launch_bounds__(256) void train_iota_kernel(uint32_t* __restrict__ vals, int64_t n, int64_t total) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid < total) vals[gid] = (uint32_t)(gid % n);
}

// Assignment: encode_pq_kernel's arithmetic (`diff = v - c; dist += diff * diff`, separately rounded, dimensions
// in order, strict `<`), but the thread's V sub-vectors sit in VGPRs and the codewords, uniform across the
// wavefront, come from LDS as 16-byte broadcasts: three VALU operations per dimension and vector, one LDS read
// per four dimensions and V vectors.  grid = (ceil(n / (256 V)), M).
template <int DSP, int V>
__global__ __launch_bounds__(kAssignThreads) void train_assign_kernel(
    const float* __restrict__ sub, int64_t n, const float* __restrict__ cb, int K, const int32_t* __restrict__ active,
    uint16_t* __restrict__ keys, float* __restrict__ dist, uint32_t* __restrict__ counts, uint32_t* __restrict__ changed,
    double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int Q = DSP / 4;
    float4* cw = reinterpret_cast<float4*>(smem);                    // [K][Q]
    uint32_t* hist = reinterpret_cast<uint32_t*>(cw + (size_t)K * Q);  // [kMaxK]
    double* red = reinterpret_cast<double*>(hist + kMaxK);           // [4]
    uint32_t* redc = reinterpret_cast<uint32_t*>(red + 4);           // [4]
    const int m = blockIdx.y, tid = threadIdx.x;
    if (!active[m]) return;
    const float4* cb4 = reinterpret_cast<const float4*>(cb + (size_t)m * K * DSP);
    for (int i = tid; i < K * Q; i += kAssignThreads) cw[i] = cb4[i];
    hist[tid] = 0;
    float x[V][DSP];
    int64_t vi[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        vi[j] = ((int64_t)blockIdx.x * V + j) * kAssignThreads + tid;
        const int64_t vc = vi[j] < n ? vi[j] : n - 1;  // the tail reads a valid row and writes nothing
        const float4* p = reinterpret_cast<const float4*>(sub + ((size_t)m * n + vc) * DSP);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 t = p[q];
            x[j][4 * q] = t.x;
            x[j][4 * q + 1] = t.y;
            x[j][4 * q + 2] = t.z;
            x[j][4 * q + 3] = t.w;
        }
    }
    __syncthreads();
    float best[V];
    int best_k[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        best[j] = FLT_MAX;
        best_k[j] = 0;
    }
    for (int k = 0; k < K; ++k) {
        float d[V];
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 c = cw[k * Q + q];
            const float ce[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float diff = __fsub_rn(x[j][4 * q + e], ce[e]);
                    d[j] = __fadd_rn(d[j], __fmul_rn(diff, diff));
                }
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (d[j] < best[j]) {
                best[j] = d[j];
                best_k[j] = k;
            }
    }
    // Nothing was below FLT_MAX (every distance +inf, or FLT_MAX itself): the label stays 0, dpq_encode_pq's, and the
    // winning distance is the computed distance to that codeword, not the FLT_MAX the search started from.  Off
    // the hot loop: the sub-vector is still in registers, so this is one more codeword for the rare thread.
#pragma unroll
    for (int j = 0; j < V; ++j)
        if (!(best[j] < FLT_MAX)) {
            float d0 = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 c = cw[q];
                const float ce[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float diff = __fsub_rn(x[j][4 * q + e], ce[e]);
                    d0 = __fadd_rn(d0, __fmul_rn(diff, diff));
                }
            }
            best[j] = d0;
        }
    double ds = 0.0;
    uint32_t ch = 0;
#pragma unroll
    for (int j = 0; j < V; ++j)
        if (vi[j] < n) {
            const size_t e = (size_t)m * n + vi[j];
            const uint16_t key = (uint16_t)((m << 8) | best_k[j]);
            ch += keys[e] != key;
            keys[e] = key;
            dist[e] = best[j];
            atomicAdd(&hist[best_k[j]], 1u);
            ds += (double)best[j];
        }
    for (int o = 32; o > 0; o >>= 1) {
        ds += __shfl_down(ds, o);
        ch += __shfl_down(ch, o);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = ds;
        redc[tid >> 6] = ch;
    }
    __syncthreads();
    if (tid == 0) {
        partial[(size_t)m * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        const uint32_t c = redc[0] + redc[1] + redc[2] + redc[3];
        if (c) atomicAdd(&changed[m], c);
    }
    if (tid < K && hist[tid]) atomicAdd(&counts[m * kMaxK + tid], hist[tid]);
}

// One block of kMaxK threads per sub-space: cluster offsets into the sorted member list, the number of empty
// clusters, the round's distortion, and the stop rule (round > 0: the first assignment has nothing to compare with).
__global__ __launch_bounds__(kMaxK) void train_stats_kernel(int64_t n, int K, int n_blocks, int round,
                                                             int32_t* __restrict__ active,
                                                             const uint32_t* __restrict__ counts,
                                                             const uint32_t* __restrict__ changed,
                                                             const double* __restrict__ partial,
                                                             uint32_t* __restrict__ offsets, RoundRec* __restrict__ rec) {
    __shared__ uint32_t scan[kMaxK];
    __shared__ uint32_t n_empty;
    __shared__ double sums[kMaxK];
    const int m = blockIdx.x, tid = threadIdx.x;
    if (!active[m]) return;
    if (tid == 0) n_empty = 0;
    const uint32_t c = tid < K ? counts[m * kMaxK + tid] : 0;
    scan[tid] = c;
    double s = 0.0;
    for (int b = tid; b < n_blocks; b += kMaxK) s += partial[(size_t)m * n_blocks + b];
    sums[tid] = s;
    __syncthreads();
    if (tid < K && c == 0) atomicAdd(&n_empty, 1u);
    for (int o = 1; o < kMaxK; o <<= 1) {
        const uint32_t add = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    offsets[m * kMaxK + tid] = (uint32_t)((int64_t)m * n) + scan[tid] - c;
    for (int o = kMaxK / 2; o > 0; o >>= 1) {
        if (tid < o) sums[tid] += sums[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        rec[m].changed = (int32_t)changed[m];
        rec[m].empty = (int32_t)n_empty;
        rec[m].distortion = sums[0];
        if (round > 0 && changed[m] == 0 && n_empty == 0) active[m] = 0;
    }
}

// Update: one thread per (sub-space, cluster, dimension).  The fp64 sum of the members' fp32 values in ascending
// vector index, one add after the other (the sort is stable, so the member list is in that order), divided in
// fp64 by the count, rounded once to fp32.  A chain-latency kernel: the loads of four members are in flight
// while the adds of the previous four retire.
__global__ __launch_bounds__(256) void train_update_kernel(const float* __restrict__ sub, int64_t n, int M, int K, int DsP,
                                                            const int32_t* __restrict__ active,
                                                            const uint32_t* __restrict__ counts,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ members, float* __restrict__ cb) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)M * K * DsP) return;
    const int d = (int)(gid % DsP), k = (int)((gid / DsP) % K), m = (int)(gid / ((int64_t)DsP * K));
    if (!active[m]) return;
    const uint32_t cnt = counts[m * kMaxK + k];
    if (cnt == 0) return;  // train_repair_kernel fills it
    const uint32_t* list = members + offsets[m * kMaxK + k];
    const float* col = sub + (size_t)m * n * DsP + d;
    double s = 0.0;
    uint32_t i = 0;
    for (; i + 4 <= cnt; i += 4) {
        const float x0 = col[(size_t)list[i] * DsP], x1 = col[(size_t)list[i + 1] * DsP];
        const float x2 = col[(size_t)list[i + 2] * DsP], x3 = col[(size_t)list[i + 3] * DsP];
        s = __dadd_rn(s, (double)x0);
        s = __dadd_rn(s, (double)x1);
        s = __dadd_rn(s, (double)x2);
        s = __dadd_rn(s, (double)x3);
    }
    for (; i < cnt; ++i) s = __dadd_rn(s, (double)col[(size_t)list[i] * DsP]);
    cb[gid] = __double2float_rn(__ddiv_rn(s, (double)cnt));
}

// Empty clusters: rank the sub-space's vectors by (winning distance descending, vector index ascending); the j-th
// empty cluster in ascending k takes the j-th ranked vector's sub-vector.  The key packs both (distances are
// non-negative, so their bit patterns order like the values); pass j finds the largest key below pass j - 1's.
__global__ __launch_bounds__(kRepairThreads) void train_repair_kernel(const float* __restrict__ sub, int64_t n, int K,
                                                                       int DsP, const int32_t* __restrict__ active,
                                                                       const uint32_t* __restrict__ counts,
                                                                       const float* __restrict__ dist,
                                                                       float* __restrict__ cb) {
    __shared__ int empty_k[kMaxK];
    __shared__ int n_empty;
    __shared__ unsigned long long wave_max[kRepairThreads / 64];
    __shared__ unsigned long long found;
    const int m = blockIdx.x, tid = threadIdx.x;
    if (!active[m]) return;
    if (tid == 0) {
        int e = 0;
        for (int k = 0; k < K; ++k)
            if (counts[m * kMaxK + k] == 0) empty_k[e++] = k;
        n_empty = e;
    }
    __syncthreads();
    const int E = n_empty;
    const float* dm = dist + (size_t)m * n;
    unsigned long long prev = ~0ull;
    for (int j = 0; j < E; ++j) {
        unsigned long long best = 0;
        for (int64_t v = tid; v < n; v += kRepairThreads) {
            const unsigned long long key =
                ((unsigned long long)__float_as_uint(dm[v]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)v);
            if (key < prev && key > best) best = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_down(best, o);
            if (other > best) best = other;
        }
        if ((tid & 63) == 0) wave_max[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long b = 0;
            for (int w = 0; w < kRepairThreads / 64; ++w)
                if (wave_max[w] > b) b = wave_max[w];
            found = b;
        }
        __syncthreads();
        prev = found;
        const uint32_t donor = 0xffffffffu - (uint32_t)(prev & 0xffffffffu);
        if (tid < DsP && (int64_t)donor < n)  // E < K <= n: a donor always exists
            cb[((size_t)m * K + empty_k[j]) * DsP + tid] = sub[((size_t)m * n + donor) * DsP + tid];
        __syncthreads();
    }
}

// ---- k-means++ start and the leaf-ordered potential (include/deltapq_amd.h) -----------------------
// A leaf is kLeaf consecutive vectors.  Every sum here is ordered by contract: the leaf sum S_l is one lane's chain
// of fp64 adds over the leaf's fp32 weights in ascending index, the running totals T_l are one lane's chain over
// the leaves.  No floating point atomics.  One step of the seeding is train_pp_update_kernel followed by
// train_pp_choose_kernel, all sub-spaces in each launch; the steps are queued back to back and the chosen index
// never leaves the device.

// Lane 0's ordered chain over a leaf's weights in LDS (16-byte aligned): the adds are one after the other by
// contract, so the next eight values are read while the current eight are added.
__device__ __forceinline__ double leaf_chain(const float* wl, int cnt) {
    const float4* w4 = reinterpret_cast<const float4*>(wl);
    const int groups = cnt >> 3;
    double s = 0.0;
    float4 a = {}, b = {};
    if (groups) {
        a = w4[0];
        b = w4[1];
    }
    for (int g = 0; g < groups; ++g) {
        float4 na = a, nb = b;
        if (g + 1 < groups) {
            na = w4[2 * g + 2];
            nb = w4[2 * g + 3];
        }
        s = __dadd_rn(s, (double)a.x);
        s = __dadd_rn(s, (double)a.y);
        s = __dadd_rn(s, (double)a.z);
        s = __dadd_rn(s, (double)a.w);
        s = __dadd_rn(s, (double)b.x);
        s = __dadd_rn(s, (double)b.y);
        s = __dadd_rn(s, (double)b.z);
        s = __dadd_rn(s, (double)b.w);
        a = na;
        b = nb;
    }
    for (int t = groups << 3; t < cnt; ++t) s = __dadd_rn(s, (double)wl[t]);
    return s;
}

// grid = (leaves, M), step j: the distance of every sub-vector to centre j = sub-vector chosen[m][j] in
// train_assign_kernel's arithmetic, w = (d < w ? d : w) (step 0: w = d), and the leaf's ordered fp64 sum.  The
// leaf-0 block also files the centre in the codebook.  Dynamic LDS: DsP floats of centre, kLeaf floats of weights.
__global__ __launch_bounds__(kLeaf) void train_pp_update_kernel(const float* __restrict__ sub, int64_t n, int K, int DsP,
                                                                 int j, const int32_t* __restrict__ chosen,
                                                                 float* __restrict__ w, double* __restrict__ S,
                                                                 float* __restrict__ cb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Q = DsP / 4;
    float4* c4 = reinterpret_cast<float4*>(smem);      // [Q]
    float* wl = reinterpret_cast<float*>(c4 + Q);      // [kLeaf]
    const int m = blockIdx.y, tid = threadIdx.x;
    const int64_t leaf = blockIdx.x;
    const int64_t c = chosen[m * K + j];
    if (tid < Q) {
        const float4 t = reinterpret_cast<const float4*>(sub + ((size_t)m * n + c) * DsP)[tid];
        c4[tid] = t;
        if (leaf == 0) reinterpret_cast<float4*>(cb + ((size_t)m * K + j) * DsP)[tid] = t;
    }
    __syncthreads();
    const int64_t i = leaf * kLeaf + tid;
    if (i < n) {
        const float4* p = reinterpret_cast<const float4*>(sub + ((size_t)m * n + i) * DsP);
        float d = 0.0f;
        for (int q = 0; q < Q; ++q) {
            const float4 x = p[q], y = c4[q];
            float diff = __fsub_rn(x.x, y.x);
            d = __fadd_rn(d, __fmul_rn(diff, diff));
            diff = __fsub_rn(x.y, y.y);
            d = __fadd_rn(d, __fmul_rn(diff, diff));
            diff = __fsub_rn(x.z, y.z);
            d = __fadd_rn(d, __fmul_rn(diff, diff));
            diff = __fsub_rn(x.w, y.w);
            d = __fadd_rn(d, __fmul_rn(diff, diff));
        }
        const size_t e = (size_t)m * n + i;
        if (j > 0) {
            const float old = w[e];
            d = d < old ? d : old;
        }
        w[e] = d;
        wl[tid] = d;
    }
    __syncthreads();
    if (tid == 0) {
        const int cnt = (int)(n - leaf * kLeaf < kLeaf ? n - leaf * kLeaf : kLeaf);
        S[(size_t)m * gridDim.x + leaf] = leaf_chain(wl, cnt);
    }
}

// grid = (leaves, M): the ordered leaf sums of any weights [M][n] (the potential of a codebook sums the winning
// distances train_assign_kernel left).
__global__ __launch_bounds__(kLeaf) void train_leaf_sum_kernel(const float* __restrict__ w, int64_t n,
                                                                double* __restrict__ S) {
    __shared__ __attribute__((aligned(16))) float wl[kLeaf];
    const int m = blockIdx.y, tid = threadIdx.x;
    const int64_t leaf = blockIdx.x, i = leaf * kLeaf + tid;
    if (i < n) wl[tid] = w[(size_t)m * n + i];
    __syncthreads();
    if (tid == 0) {
        const int cnt = (int)(n - leaf * kLeaf < kLeaf ? n - leaf * kLeaf : kLeaf);
        S[(size_t)m * gridDim.x + leaf] = leaf_chain(wl, cnt);
    }
}

// One block per sub-space.  Lane 0 chains the running totals T over the leaf sums, kChunk leaves at a time through
// LDS, and the block keeps them.  j < 0: the total is the potential, nothing else.  Otherwise centre j is drawn
// with z = zs[m][j]: total == 0 takes the smallest index that is no centre yet; else r = u * total, the first leaf
// with T_l > r (none: the last with S_l > 0), and in it the first i whose running sum exceeds r - T_{l-1} (none:
// the last with w_i > 0).  The searches over the leaves are minima and maxima of indices, the same in any order.
__global__ __launch_bounds__(kLeaf) void train_pp_choose_kernel(const float* __restrict__ w, int64_t n, int L, int K, int j,
                                                                 const uint64_t* __restrict__ zs,
                                                                 const double* __restrict__ S, double* __restrict__ T,
                                                                 int32_t* __restrict__ chosen,
                                                                 double* __restrict__ potential) {
    __shared__ __attribute__((aligned(16))) double chunk[kChunk];
    __shared__ float wl[kLeaf];
    __shared__ int taken[kLeaf];
    __shared__ double s_total;
    __shared__ int s_first, s_last;
    const int m = blockIdx.x, tid = threadIdx.x;
    const double* Sm = S + (size_t)m * L;
    double* Tm = T + (size_t)m * L;
    double run = 0.0;  // lane 0's
    for (int base = 0; base < L; base += kChunk) {
        const int cnt = L - base < kChunk ? L - base : kChunk;
        for (int i = tid; i < cnt; i += kLeaf) chunk[i] = Sm[base + i];
        __syncthreads();
        if (tid == 0) {
            // T_0 = +0.0 + S_0 = S_0: a leaf sum is never -0.0.  Eight sums at a time, the next eight in flight.
            double2* c2 = reinterpret_cast<double2*>(chunk);
            const int groups = cnt >> 3;
            double2 v[4] = {}, nv[4] = {};
            if (groups)
                for (int q = 0; q < 4; ++q) v[q] = c2[q];
            for (int g = 0; g < groups; ++g) {
                if (g + 1 < groups)
                    for (int q = 0; q < 4; ++q) nv[q] = c2[4 * g + 4 + q];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    run = __dadd_rn(run, v[q].x);
                    v[q].x = run;
                    run = __dadd_rn(run, v[q].y);
                    v[q].y = run;
                    c2[4 * g + q] = v[q];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = nv[q];
            }
            for (int i = groups << 3; i < cnt; ++i) {
                run = __dadd_rn(run, chunk[i]);
                chunk[i] = run;
            }
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += kLeaf) Tm[base + i] = chunk[i];
        __syncthreads();
    }
    if (tid == 0) {
        s_total = run;
        s_first = 0x7fffffff;
        s_last = -1;
    }
    taken[tid] = 0;
    __syncthreads();  // also makes the block's own T stores visible to all of its lanes
    const double total = s_total;
    if (j < 0) {
        if (tid == 0) potential[m] = total;
        return;
    }
    int32_t* mine = chosen + m * K;
    int leaf = -1;
    double r = 0.0;
    if (total != 0.0) {
        const double u = __dmul_rn((double)(zs[m * K + j] >> 11), 0x1p-53);
        r = __dmul_rn(u, total);
        int first = 0x7fffffff, last = -1;
        for (int l = tid; l < L; l += kLeaf) {
            if (Tm[l] > r && l < first) first = l;
            if (Sm[l] > 0.0) last = l;  // ascending l: the lane's largest
        }
        if (first != 0x7fffffff) atomicMin(&s_first, first);
        if (last >= 0) atomicMax(&s_last, last);
        __syncthreads();
        leaf = s_first != 0x7fffffff ? s_first : s_last;  // total > 0: some S_l > 0
    }
    if (leaf < 0) {
        // total == 0 (or a NaN total, which has no leaf either: the same rule keeps every index in range).
        // j centres so far, so one of the indices 0 .. j is free (j < K <= n)
        if (tid < j && mine[tid] >= 0 && mine[tid] <= j) taken[mine[tid]] = 1;
        __syncthreads();
        if (tid == 0) {
            int pick = 0;
            while (pick < j && taken[pick]) ++pick;
            mine[j] = pick;
        }
        return;
    }
    const int64_t at = (int64_t)leaf * kLeaf;
    const int cnt = (int)(n - at < kLeaf ? n - at : kLeaf);
    if (tid < cnt) wl[tid] = w[(size_t)m * n + at + tid];
    __syncthreads();
    if (tid == 0) {
        const double rp = __dsub_rn(r, leaf ? Tm[leaf - 1] : 0.0);
        double t = 0.0;
        int pick = -1, positive = -1;
        for (int i = 0; i < cnt; ++i) {
            t = __dadd_rn(t, (double)wl[i]);
            if (wl[i] > 0.0f) positive = i;
            if (t > rp) {
                pick = i;
                break;
            }
        }
        if (pick < 0) pick = positive >= 0 ? positive : 0;  // S_leaf > 0: a positive weight exists
        mine[j] = (int32_t)(at + pick);
    }
}

// hipFuncSetAttribute is per device
hipError_t ensure_lds(const void* fn, std::atomic<bool>* done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

struct AssignArgs {
    const float* sub;
    int64_t n;
    const float* cb;
    int M, K;
    const int32_t* active;
    uint16_t* keys;
    float* dist;
    uint32_t* counts;
    uint32_t* changed;
    double* partial;
};

template <int DSP, int V>
hipError_t launch_assign_as(const AssignArgs& a, size_t lds) {
    static std::atomic<bool> done[64] = {};
    hipError_t e = ensure_lds(reinterpret_cast<const void*>(&train_assign_kernel<DSP, V>), done);
    if (e != hipSuccess) return e;
    const unsigned blocks = (unsigned)((a.n + kAssignThreads * V - 1) / (kAssignThreads * V));
    hipLaunchKernelGGL((train_assign_kernel<DSP, V>), dim3(blocks, (unsigned)a.M), dim3(kAssignThreads), lds, nullptr, a.sub,
                       a.n, a.cb, a.K, a.active, a.keys, a.dist, a.counts, a.changed, a.partial);
    return hipGetLastError();
}

// vectors per thread of the width's instance: two while 2 x DsP registers leave four waves per SIMD
int assign_vectors_per_thread(int DsP) { return DsP <= 32 ? 2 : 1; }

hipError_t launch_assign(const AssignArgs& a, int DsP, size_t lds) {
    switch (DsP) {
        case 4: return launch_assign_as<4, 2>(a, lds);
        case 8: return launch_assign_as<8, 2>(a, lds);
        case 12: return launch_assign_as<12, 2>(a, lds);
        case 16: return launch_assign_as<16, 2>(a, lds);
        case 24: return launch_assign_as<24, 2>(a, lds);
        case 32: return launch_assign_as<32, 2>(a, lds);
        case 64: return launch_assign_as<64, 1>(a, lds);
        case 96: return launch_assign_as<96, 1>(a, lds);
        case 128: return launch_assign_as<128, 1>(a, lds);
        case 160: return launch_assign_as<160, 1>(a, lds);
    }
    return hipErrorInvalidValue;
}

template <class T>
struct Dev {  // an owned device array
    T* p = nullptr;
    ~Dev() {
        if (p) hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)); }
    operator T*() const { return p; }
};

struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() {
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
};

}  // namespace

int train_padded_ds(int Ds) {
    static const int widths[] = {4, 8, 12, 16, 24, 32, 64, 96, 128, 160};
    for (int w : widths)
        if (Ds <= w) return w;
    return 0;
}

size_t train_lds_bytes(int K, int Ds) {
    const int DsP = train_padded_ds(Ds);
    if (DsP == 0) return 0;
    return (size_t)K * DsP * sizeof(float) + kMaxK * sizeof(uint32_t) + 4 * sizeof(double) + 4 * sizeof(uint32_t);
}

#define TR_HIP(expr)                                                                   \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            if (err) *err = std::string(#expr) + ": " + hipGetErrorString(_e);         \
            return _e == hipErrorOutOfMemory ? DPQ_ERR_NOMEM : DPQ_ERR_HIP;            \
        }                                                                              \
    } while (0)

struct Trainer::Impl {
    int64_t n = 0, total = 0;
    int D = 0, M = 0, K = 0, Ds = 0, DsP = 0, V = 0, n_blocks = 0, n_leaves = 0, key_bits = 8;
    size_t lds = 0, temp_bytes = 0;
    Dev<float> d_sub, d_cb, d_dist;
    Dev<uint16_t> d_keys, d_keys_sorted;
    Dev<uint32_t> d_iota, d_members, d_counts, d_changed, d_offsets;
    Dev<int32_t> d_active, d_chosen;
    Dev<double> d_partial, d_leaf_sums, d_leaf_totals, d_potential;
    Dev<uint64_t> d_zs;
    Dev<RoundRec> d_rec;
    Dev<unsigned char> d_temp;

    AssignArgs assign_args() const {
        return {d_sub, n, d_cb, M, K, d_active, d_keys, d_dist, d_counts, d_changed, d_partial};
    }
    int activate_all(std::string* err) {
        std::vector<int32_t> act((size_t)M, 1);
        TR_HIP(hipMemcpy(d_active, act.data(), act.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return DPQ_OK;
    }
};

Trainer::Trainer() : p_(new Impl) {}
Trainer::~Trainer() { delete p_; }

int Trainer::open(const float* vectors, int64_t n, int D, int M, int K, int Ds, std::string* err) {
    Impl& s = *p_;
    s.n = n, s.D = D, s.M = M, s.K = K, s.Ds = Ds;
    s.DsP = train_padded_ds(Ds);
    s.lds = train_lds_bytes(K, Ds);
    s.total = n * M;
    s.V = assign_vectors_per_thread(s.DsP);
    s.n_blocks = (int)((n + kAssignThreads * s.V - 1) / (kAssignThreads * s.V));
    s.n_leaves = (int)((n + kLeaf - 1) / kLeaf);
    const int64_t total = s.total;
    const int DsP = s.DsP;

    Dev<float> d_tile;
    const int64_t tile = std::min<int64_t>(n, 1 << 18);  // vectors per upload
    TR_HIP(s.d_sub.alloc((size_t)total * DsP));
    TR_HIP(d_tile.alloc((size_t)tile * D));
    TR_HIP(s.d_cb.alloc((size_t)M * K * DsP));
    TR_HIP(s.d_dist.alloc((size_t)total));
    TR_HIP(s.d_keys.alloc((size_t)total));
    TR_HIP(s.d_keys_sorted.alloc((size_t)total));
    TR_HIP(s.d_iota.alloc((size_t)total));
    TR_HIP(s.d_members.alloc((size_t)total));
    TR_HIP(s.d_counts.alloc((size_t)M * kMaxK));
    TR_HIP(s.d_changed.alloc((size_t)M));
    TR_HIP(s.d_offsets.alloc((size_t)M * kMaxK));
    TR_HIP(s.d_active.alloc((size_t)M));
    TR_HIP(s.d_partial.alloc((size_t)M * s.n_blocks));
    TR_HIP(s.d_rec.alloc((size_t)M));
    TR_HIP(s.d_leaf_sums.alloc((size_t)M * s.n_leaves));
    TR_HIP(s.d_leaf_totals.alloc((size_t)M * s.n_leaves));
    TR_HIP(s.d_potential.alloc((size_t)M));
    TR_HIP(s.d_chosen.alloc((size_t)M * K));
    TR_HIP(s.d_zs.alloc((size_t)M * K));
    while ((1 << s.key_bits) < M * 256) ++s.key_bits;
    TR_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, s.temp_bytes, s.d_keys.p, s.d_keys_sorted.p, s.d_iota.p,
                                              s.d_members.p, (int)total, 0, s.key_bits, nullptr));
    TR_HIP(s.d_temp.alloc(s.temp_bytes));

    for (int64_t base = 0; base < n; base += tile) {
        const int64_t cnt = std::min(tile, n - base);
        TR_HIP(hipMemcpy(d_tile, vectors + (size_t)base * D, (size_t)cnt * D * sizeof(float), hipMemcpyHostToDevice));
        const int64_t work = cnt * M * DsP;
        hipLaunchKernelGGL(train_split_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, nullptr, d_tile.p, base,
                           cnt, n, D, M, Ds, DsP, s.d_sub.p);
        TR_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(train_iota_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, s.d_iota.p, n, total);
    TR_HIP(hipGetLastError());
    TR_HIP(hipDeviceSynchronize());  // d_tile goes out of scope
    return DPQ_OK;
}

int Trainer::set_codebook(const float* codewords, std::string* err) {
    Impl& s = *p_;
    std::vector<float> cbp((size_t)s.M * s.K * s.DsP, 0.0f);
    for (size_t r = 0; r < (size_t)s.M * s.K; ++r)
        for (int d = 0; d < s.Ds; ++d) cbp[r * s.DsP + d] = codewords[r * s.Ds + d];
    TR_HIP(hipMemcpy(s.d_cb, cbp.data(), cbp.size() * sizeof(float), hipMemcpyHostToDevice));
    return DPQ_OK;
}

int Trainer::get_codebook(float* codewords, std::string* err) {
    Impl& s = *p_;
    std::vector<float> cbp((size_t)s.M * s.K * s.DsP);
    TR_HIP(hipMemcpy(cbp.data(), s.d_cb, cbp.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < (size_t)s.M * s.K; ++r)
        for (int d = 0; d < s.Ds; ++d) codewords[r * s.Ds + d] = cbp[r * s.DsP + d];
    return DPQ_OK;
}

int Trainer::seed_kmeanspp(uint64_t seed, double* potential, double* ms, std::string* err) {
    Impl& s = *p_;
    const int M = s.M, K = s.K;
    // every draw of every sub-space, from the host: s = seed + m * 0xD6E8FEB86659FD93, splitmix64 from there
    std::vector<uint64_t> zs((size_t)M * K);
    std::vector<int32_t> chosen((size_t)M * K, 0);
    for (int m = 0; m < M; ++m) {
        uint64_t st = seed + (uint64_t)m * 0xD6E8FEB86659FD93ull;
        for (int j = 0; j < K; ++j) {
            st += 0x9E3779B97F4A7C15ull;
            uint64_t z = st;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            zs[(size_t)m * K + j] = z;
        }
        chosen[(size_t)m * K] = (int32_t)(zs[(size_t)m * K] % (uint64_t)s.n);  // centre 0
    }
    TR_HIP(hipMemcpy(s.d_zs, zs.data(), zs.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    TR_HIP(hipMemcpy(s.d_chosen, chosen.data(), chosen.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    Events events;
    events.ev.resize(2);
    for (hipEvent_t& e : events.ev) TR_HIP(hipEventCreate(&e));
    TR_HIP(hipEventRecord(events.ev[0], nullptr));
    const dim3 leaves((unsigned)s.n_leaves, (unsigned)M);
    const size_t lds = (size_t)s.DsP * sizeof(float) + kLeaf * sizeof(float);
    for (int j = 0; j < K; ++j) {
        if (j > 0) {
            hipLaunchKernelGGL(train_pp_choose_kernel, dim3((unsigned)M), dim3(kLeaf), 0, nullptr, s.d_dist.p, s.n, s.n_leaves,
                               K, j, s.d_zs.p, s.d_leaf_sums.p, s.d_leaf_totals.p, s.d_chosen.p, s.d_potential.p);
            TR_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(train_pp_update_kernel, leaves, dim3(kLeaf), lds, nullptr, s.d_sub.p, s.n, K, s.DsP, j,
                           s.d_chosen.p, s.d_dist.p, s.d_leaf_sums.p, s.d_cb.p);
        TR_HIP(hipGetLastError());
    }
    if (potential) {
        hipLaunchKernelGGL(train_pp_choose_kernel, dim3((unsigned)M), dim3(kLeaf), 0, nullptr, s.d_dist.p, s.n, s.n_leaves, K,
                           -1, s.d_zs.p, s.d_leaf_sums.p, s.d_leaf_totals.p, s.d_chosen.p, s.d_potential.p);
        TR_HIP(hipGetLastError());
    }
    TR_HIP(hipEventRecord(events.ev[1], nullptr));
    TR_HIP(hipDeviceSynchronize());
    if (potential) TR_HIP(hipMemcpy(potential, s.d_potential, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
    if (ms) {
        float f = 0.f;
        TR_HIP(hipEventElapsedTime(&f, events.ev[0], events.ev[1]));
        *ms = f;
    }
    return DPQ_OK;
}

int Trainer::potential(double* out, std::string* err) {
    Impl& s = *p_;
    const int M = s.M;
    int rc = s.activate_all(err);
    if (rc) return rc;
    TR_HIP(hipMemsetAsync(s.d_counts, 0, (size_t)M * kMaxK * sizeof(uint32_t), nullptr));
    TR_HIP(hipMemsetAsync(s.d_changed, 0, (size_t)M * sizeof(uint32_t), nullptr));
    TR_HIP(launch_assign(s.assign_args(), s.DsP, s.lds));
    hipLaunchKernelGGL(train_leaf_sum_kernel, dim3((unsigned)s.n_leaves, (unsigned)M), dim3(kLeaf), 0, nullptr, s.d_dist.p,
                       s.n, s.d_leaf_sums.p);
    TR_HIP(hipGetLastError());
    hipLaunchKernelGGL(train_pp_choose_kernel, dim3((unsigned)M), dim3(kLeaf), 0, nullptr, s.d_dist.p, s.n, s.n_leaves, s.K, -1,
                       s.d_zs.p, s.d_leaf_sums.p, s.d_leaf_totals.p, s.d_chosen.p, s.d_potential.p);
    TR_HIP(hipGetLastError());
    TR_HIP(hipMemcpy(out, s.d_potential, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

int Trainer::lloyd(int max_iters, TrainStats* st, std::string* err) {
    Impl& s = *p_;
    const int64_t n = s.n, total = s.total;
    const int M = s.M, K = s.K, DsP = s.DsP, n_blocks = s.n_blocks;
    int rc = s.activate_all(err);
    if (rc) return rc;
    TR_HIP(hipMemset(s.d_keys, 0xff, (size_t)total * sizeof(uint16_t)));
    TR_HIP(hipMemset(s.d_rec, 0, (size_t)M * sizeof(RoundRec)));

    Events events;
    events.ev.resize((size_t)max_iters * 5);
    for (hipEvent_t& e : events.ev) TR_HIP(hipEventCreate(&e));
    std::vector<int> ran((size_t)max_iters, 0);  // 1: assignment only, 2: the update ran, 3: the repair too
    std::vector<RoundRec> rec((size_t)M);
    std::vector<char> active((size_t)M, 1);
    const AssignArgs aa = s.assign_args();
    *st = TrainStats();
    TR_HIP(hipDeviceSynchronize());
    const auto rounds0 = std::chrono::steady_clock::now();
    for (int r = 0; r < max_iters; ++r) {
        hipEvent_t* ev = &events.ev[(size_t)r * 5];
        TR_HIP(hipEventRecord(ev[0], nullptr));
        TR_HIP(hipMemsetAsync(s.d_counts, 0, (size_t)M * kMaxK * sizeof(uint32_t), nullptr));
        TR_HIP(hipMemsetAsync(s.d_changed, 0, (size_t)M * sizeof(uint32_t), nullptr));
        TR_HIP(launch_assign(aa, DsP, s.lds));
        hipLaunchKernelGGL(train_stats_kernel, dim3((unsigned)M), dim3(kMaxK), 0, nullptr, n, K, n_blocks, r, s.d_active.p,
                           s.d_counts.p, s.d_changed.p, s.d_partial.p, s.d_offsets.p, s.d_rec.p);
        TR_HIP(hipGetLastError());
        TR_HIP(hipEventRecord(ev[1], nullptr));
        TR_HIP(hipMemcpy(rec.data(), s.d_rec, (size_t)M * sizeof(RoundRec), hipMemcpyDeviceToHost));  // the round's only sync
        st->iters_run = r + 1;
        ran[(size_t)r] = 1;
        double distortion = 0.0;
        int64_t n_empty = 0;
        bool any = false;
        for (int m = 0; m < M; ++m) {
            distortion += rec[(size_t)m].distortion;  // a stopped sub-space keeps its last round's sum
            if (!active[(size_t)m]) continue;
            if (r > 0 && rec[(size_t)m].changed == 0 && rec[(size_t)m].empty == 0) {
                active[(size_t)m] = 0;  // train_stats_kernel cleared its device flag by the same rule
                continue;
            }
            any = true;
            n_empty += rec[(size_t)m].empty;
        }
        st->distortion[r] = distortion;
        if (!any) {
            st->converged = 1;
            break;
        }
        TR_HIP(hipEventRecord(ev[2], nullptr));  // between ev[1] and ev[2] the device waits for the host
        TR_HIP(hipcub::DeviceRadixSort::SortPairs(s.d_temp.p, s.temp_bytes, s.d_keys.p, s.d_keys_sorted.p, s.d_iota.p,
                                                  s.d_members.p, (int)total, 0, s.key_bits, nullptr));
        const int64_t chains = (int64_t)M * K * DsP;
        hipLaunchKernelGGL(train_update_kernel, dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, nullptr, s.d_sub.p, n, M,
                           K, DsP, s.d_active.p, s.d_counts.p, s.d_offsets.p, s.d_members.p, s.d_cb.p);
        TR_HIP(hipGetLastError());
        TR_HIP(hipEventRecord(ev[3], nullptr));
        ran[(size_t)r] = 2;
        if (n_empty > 0) {
            hipLaunchKernelGGL(train_repair_kernel, dim3((unsigned)M), dim3(kRepairThreads), 0, nullptr, s.d_sub.p, n, K, DsP,
                               s.d_active.p, s.d_counts.p, s.d_dist.p, s.d_cb.p);
            TR_HIP(hipGetLastError());
            TR_HIP(hipEventRecord(ev[4], nullptr));
            ran[(size_t)r] = 3;
            st->reseeded += n_empty;
        }
    }
    TR_HIP(hipDeviceSynchronize());
    st->rounds_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - rounds0).count();
    for (int r = 0; r < st->iters_run; ++r) {
        hipEvent_t* ev = &events.ev[(size_t)r * 5];
        float ms = 0.f;
        TR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        st->assign_ms += ms;
        if (ran[(size_t)r] >= 2) {
            TR_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
            st->update_ms += ms;
        }
        if (ran[(size_t)r] >= 3) {
            TR_HIP(hipEventElapsedTime(&ms, ev[3], ev[4]));
            st->repair_ms += ms;
        }
    }
    st->gpu_ms = st->assign_ms + st->update_ms + st->repair_ms;
    return DPQ_OK;
}

}  // namespace dpq
