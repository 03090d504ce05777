// dpq_opq.hip -- the OPQ kernels for gfx950: the rotation out = x . R in stated fp64 arithmetic, and the ordered
// cross-covariance of the vectors with their PQ reconstruction.  Contract: include/deltapq_amd.h "OPQ"; resource
// table and bounds: DESIGN.md 5.13.  No floating-point atomics anywhere: every sum has one owner and one order.
#include "dpq_opq.h"

#include <algorithm>

namespace dpq {

namespace {

// ---- rotation ---------------------------------------------------------------------------------------------------
// A workgroup of 8 waves owns 64 * RT rows x 64 output columns and walks d in tiles of 32.  Lane l of every wave
// owns rows l, l + 64, ... (RT of them); wave w owns the strip of 8 columns [8 w, 8 w + 8).  A thread keeps RT x 8
// fp64 accumulators; each is one chain acc = fma((double)x[i][d], (double)R[d][j], acc) over d ascending, which is
// the contract's order: no sum is split across lanes or tiles (a tile boundary only pauses the chain).  Zero filled
// tile edges (d >= D) add fma(+0, +0, acc) = acc: acc starts at +0.0 and a sum that starts there is never -0.0, so
// the bits do not change.
//
// LDS: the R tile as fp64 [32][64] (16 KB; converted once when staged, so the inner loop has no per-use conversion)
// and the x tile as fp32 [64 RT][36].
//   R reads   every lane of a wave reads the same 64 bytes R[d][8 w ..] as four ds_read_b128: one address per
//             instruction, a broadcast, which cannot conflict whatever the lane groups are.
//   x reads   lane l reads 16 bytes at row l, stride 36 floats = 9 sixteen-byte slots.  9 is odd and a bank row has 16
//             slots, so 16 lanes with distinct l mod 16 hit 16 distinct slots; each of ds_read_b128's four lane groups
//             ({0-3,12-15,20-27}, ...) has distinct l mod 16: no conflict.
//   out       the accumulators go back through LDS ([64][68] floats, stride 17 slots, odd as well) so that the stores
//             to memory are 256 contiguous bytes per 16 lanes instead of 32 bytes per lane at stride D.
// Per d and wave: 8 RT v_fma_f64 against 4 + RT / 4 ds_read_b128, so the fp64 pipe is the bound from RT = 2 on; RT = 1
// (small n: more workgroups, a shorter critical path) leans on the LDS instead.
constexpr int kRotThreads = 512;
constexpr int kRotKT = 32;       // d per tile
constexpr int kRotCT = 64;       // output columns per workgroup
constexpr int kRotXStride = 36;  // floats; 9 slots
constexpr int kRotOStride = 68;  // floats; 17 slots

template <int RT>
__global__ __launch_bounds__(kRotThreads) void opq_rotate_kernel(const float* __restrict__ x, int64_t n, int D,
                                                                  const float* __restrict__ R, float* __restrict__ out,
                                                                  int vec_in, int vec_out) {
    constexpr int BR = 64 * RT;
    constexpr int kXFloats = BR * kRotXStride > 64 * kRotOStride ? BR * kRotXStride : 64 * kRotOStride;
    __shared__ __attribute__((aligned(16))) double rs[kRotKT][kRotCT];
    __shared__ __attribute__((aligned(16))) float xs[kXFloats];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * BR;
    const int c0 = blockIdx.y * kRotCT;

    double acc[RT][8];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = 0.0;

    // The next tile's global loads are issued before the current tile's arithmetic and parked in registers (4 RT floats
    // of x and 4 of R a thread), so their latency hides under the fma chain; they reach LDS between the two barriers.
    float xr[4 * RT], rr[4];
    auto fetch = [&](int k0) {
        if (vec_in) {
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                const int idx = tid + i * kRotThreads, r = idx >> 3, c4 = idx & 7;
                const int64_t row = row0 + r;
                const int k = k0 + c4 * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < n && k < D) v = *reinterpret_cast<const float4*>(x + (size_t)row * D + k);
                xr[4 * i] = v.x; xr[4 * i + 1] = v.y; xr[4 * i + 2] = v.z; xr[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4 * RT; ++i) {
                const int idx = tid + i * kRotThreads, r = idx >> 5, c = idx & 31;
                const int64_t row = row0 + r;
                const int k = k0 + c;
                xr[i] = (row < n && k < D) ? x[(size_t)row * D + k] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * kRotThreads, k = idx >> 6, c = idx & 63;
            rr[i] = (k0 + k < D && c0 + c < D) ? R[(size_t)(k0 + k) * D + c0 + c] : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < D; k0 += kRotKT) {
        __syncthreads();  // the previous tile's readers are done
        if (vec_in) {
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                const int idx = tid + i * kRotThreads, r = idx >> 3, c4 = idx & 7;
                *reinterpret_cast<float4*>(&xs[r * kRotXStride + c4 * 4]) =
                    make_float4(xr[4 * i], xr[4 * i + 1], xr[4 * i + 2], xr[4 * i + 3]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4 * RT; ++i) {
                const int idx = tid + i * kRotThreads, r = idx >> 5, c = idx & 31;
                xs[r * kRotXStride + c] = xr[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * kRotThreads, k = idx >> 6, c = idx & 63;
            rs[k][c] = (double)rr[i];
        }
        __syncthreads();
        if (k0 + kRotKT < D) fetch(k0 + kRotKT);
#pragma unroll 2
        for (int k4 = 0; k4 < kRotKT / 4; ++k4) {
            float4 xv[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r)
                xv[r] = *reinterpret_cast<const float4*>(&xs[(lane + 64 * r) * kRotXStride + k4 * 4]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const double2* rp = reinterpret_cast<const double2*>(&rs[k4 * 4 + kk][w * 8]);
                const double2 r01 = rp[0], r23 = rp[1], r45 = rp[2], r67 = rp[3];
                const double rv[8] = {r01.x, r01.y, r23.x, r23.y, r45.x, r45.y, r67.x, r67.y};
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const float xf = kk == 0 ? xv[r].x : kk == 1 ? xv[r].y : kk == 2 ? xv[r].z : xv[r].w;
                    const double xd = (double)xf;
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[r][c] = __builtin_fma(xd, rv[c], acc[r][c]);
                }
            }
        }
    }

    // out through LDS, 64 rows at a time
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        __syncthreads();
        float4 lo, hi;
        lo.x = (float)acc[r][0]; lo.y = (float)acc[r][1]; lo.z = (float)acc[r][2]; lo.w = (float)acc[r][3];
        hi.x = (float)acc[r][4]; hi.y = (float)acc[r][5]; hi.z = (float)acc[r][6]; hi.w = (float)acc[r][7];
        *reinterpret_cast<float4*>(&xs[lane * kRotOStride + w * 8]) = lo;
        *reinterpret_cast<float4*>(&xs[lane * kRotOStride + w * 8 + 4]) = hi;
        __syncthreads();
        const int64_t rbase = row0 + 64 * r;
        if (vec_out) {
            for (int idx = tid; idx < 64 * (kRotCT / 4); idx += kRotThreads) {
                const int rr = idx >> 4, c4 = idx & 15;
                const int64_t row = rbase + rr;
                const int col = c0 + c4 * 4;
                if (row < n && col < D)
                    *reinterpret_cast<float4*>(out + (size_t)row * D + col) =
                        *reinterpret_cast<const float4*>(&xs[rr * kRotOStride + c4 * 4]);
            }
        } else {
            for (int idx = tid; idx < 64 * kRotCT; idx += kRotThreads) {
                const int rr = idx >> 6, c = idx & 63;
                const int64_t row = rbase + rr;
                if (row < n && c0 + c < D) out[(size_t)row * D + c0 + c] = xs[rr * kRotOStride + c];
            }
        }
    }
}

// ---- cross-covariance -------------------------------------------------------------------------------------------
// opq_cross_leaf_kernel: a thread per (leaf, d, j) walks the leaf's rows in ascending order, one fp64 chain.  Rows go
// 64 at a time: the codes of those rows (only the sub-spaces this workgroup's j touch) are loaded once per workgroup
// into LDS; then four rows' x and gathered y are loaded before their four adds retire, train_update_kernel's pattern.
// The product of two fp32 values is exact in fp64, so fma and multiply-then-add give the same bits.
constexpr int kCrossThreads = 256;
constexpr int kCrossChunk = 64;

__global__ __launch_bounds__(kCrossThreads) void opq_cross_leaf_kernel(const float* __restrict__ x, int64_t n, int D,
                                                                        const uint8_t* __restrict__ codes,
                                                                        const float* __restrict__ cw, int M, int K, int Ds,
                                                                        int64_t leaf0, double* __restrict__ S) {
    __shared__ uint8_t codes_s[kCrossChunk * 256];
    const int tid = threadIdx.x;
    const int64_t DD = (int64_t)D * D;
    const int64_t e_lo = (int64_t)blockIdx.x * kCrossThreads;
    const int64_t e = e_lo + tid;
    const bool valid = e < DD;
    // the sub-spaces this workgroup needs: those of its j range when it stays inside one d, else all of them
    int m_lo = 0, m_cnt = M;
    const int j_lo = (int)(e_lo % D);
    if (j_lo + kCrossThreads - 1 < D) {
        m_lo = j_lo / Ds;
        m_cnt = (j_lo + kCrossThreads - 1) / Ds - m_lo + 1;
    }
    // (a thread past D * D walks along with entry (0, m_lo * Ds) and writes nothing)
    const int d = valid ? (int)(e / D) : 0, j = valid ? (int)(e % D) : m_lo * Ds;
    const int m = j / Ds, jj = j % Ds;
    const int64_t leaf = leaf0 + blockIdx.y;
    const int64_t lo = leaf * kOpqLeaf, hi = lo + kOpqLeaf < n ? lo + kOpqLeaf : n;
    const float* cwm = cw + (size_t)m * K * Ds + jj;

    double acc = 0.0;
    for (int64_t base = lo; base < hi; base += kCrossChunk) {
        const int cnt = (int)(hi - base < kCrossChunk ? hi - base : kCrossChunk);
        __syncthreads();
        for (int idx = tid; idx < cnt * m_cnt; idx += kCrossThreads) {
            const int r = idx / m_cnt, mm = idx - r * m_cnt;
            codes_s[idx] = codes[(size_t)(base + r) * M + m_lo + mm];
        }
        __syncthreads();
        for (int r = 0; r < cnt; r += 4) {
            float xv[4], yv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = r + u < cnt;
                const int rr = in ? r + u : r;
                xv[u] = x[(size_t)(base + rr) * D + d];
                yv[u] = cwm[(size_t)codes_s[rr * m_cnt + (m - m_lo)] * Ds];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + u < cnt) acc = __builtin_fma((double)xv[u], (double)yv[u], acc);
        }
    }
    if (valid) S[(size_t)blockIdx.y * DD + e] = acc;
}

// T over the leaves of one pass, one add after the other; the first pass starts at S_0 itself.
__global__ __launch_bounds__(256) void opq_cross_chain_kernel(const double* __restrict__ S, int n_leaves, int64_t DD, int first,
                                                               double* __restrict__ C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= DD) return;
    double T = first ? S[e] : C[e] + S[e];
    for (int l = 1; l < n_leaves; ++l) T = T + S[(size_t)l * DD + e];
    C[e] = T;
}

}  // namespace

hipError_t launch_opq_rotate(const float* d_x, int64_t n, int D, const float* d_R, float* d_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int vec_in = D % 4 == 0 && (reinterpret_cast<uintptr_t>(d_x) & 15) == 0;
    const int vec_out = D % 4 == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    const bool wide = n >= 2048;  // four rows a lane once there are rows enough to fill the machine anyway
    for (int64_t base = 0; base < n; base += kOpqSlice) {
        const int64_t m = std::min(kOpqSlice, n - base);
        const float* xs = d_x + (size_t)base * D;
        float* os = d_out + (size_t)base * D;
        const int br = wide ? 256 : 64;
        const dim3 grid((unsigned)((m + br - 1) / br), (unsigned)((D + kRotCT - 1) / kRotCT));
        if (wide)
            opq_rotate_kernel<4><<<grid, kRotThreads, 0, stream>>>(xs, m, D, d_R, os, vec_in, vec_out);
        else
            opq_rotate_kernel<1><<<grid, kRotThreads, 0, stream>>>(xs, m, D, d_R, os, vec_in, vec_out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int64_t opq_cross_leaves_per_pass(int D) {
    const size_t per_leaf = (size_t)D * D * sizeof(double);
    return (int64_t)std::min<size_t>(65535, std::max<size_t>(1, kOpqLeafBytesCap / per_leaf));
}

hipError_t launch_opq_cross(const float* d_x, int64_t n, int D, const uint8_t* d_codes, const float* d_cw, int M, int K,
                            int Ds, double* d_S, double* d_C, hipStream_t stream) {
    const int64_t DD = (int64_t)D * D;
    const int64_t leaves = (n + kOpqLeaf - 1) / kOpqLeaf, per_pass = opq_cross_leaves_per_pass(D);
    const unsigned gx = (unsigned)((DD + kCrossThreads - 1) / kCrossThreads);
    for (int64_t l0 = 0; l0 < leaves; l0 += per_pass) {
        const int nl = (int)std::min(per_pass, leaves - l0);
        opq_cross_leaf_kernel<<<dim3(gx, (unsigned)nl), kCrossThreads, 0, stream>>>(d_x, n, D, d_codes, d_cw, M, K, Ds, l0, d_S);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        opq_cross_chain_kernel<<<(unsigned)((DD + 255) / 256), 256, 0, stream>>>(d_S, nl, DD, l0 == 0 ? 1 : 0, d_C);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dpq
