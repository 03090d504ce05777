// dpq_ivf_train.h -- launch interface of the coarse-quantiser kernels (dpq_ivf_train.hip): the nearest centroid of every
// row under the exact search's arithmetic, and the pieces of a Lloyd round around it (include/deltapq_amd.h "IVF
// training").  The lists of a round come from dpq_ivf.h's launch_ivf_label_keys and ivf_scan_and_sort.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kIvfArgminRows = 64;       // rows of a workgroup's tile
constexpr int kIvfDistLeaf = 1024;       // winning distances one partial sum of the distortion covers

// What the host reads back once per round.
struct IvfRoundStats {
    double distortion;   // the fp64 sum of the winning distances
    uint32_t changed;    // rows whose label differs from the previous round's
    uint32_t n_empty;    // lists without a member
};

// Partial sums launch_ivf_round_stats needs for n winning distances.
inline size_t ivf_dist_partials(int64_t n) { return (size_t)((n + kIvfDistLeaf - 1) / kIvfDistLeaf); }

// d_labels[i] = the list with the smallest key `distance bits << 32 | list` of row i, d_win[i] (may be NULL) the distance
// to it: per dimension in ascending order t = c[d] - v[d] and s = t * t in fp32, each rounded, summed on an fp64
// accumulator from +0.0 and rounded once to fp32.  d_rows [n][Dp] and d_cent [nlist][Dp], Dp a multiple of 4 (padding
// zeros), both 16-byte aligned.  d_prev (may be NULL, may be d_labels itself): *d_changed += the rows i with d_prev[i] !=
// the new label.
hipError_t launch_ivf_argmin(const float* d_rows, int64_t n, int Dp, const float* d_cent, int nlist, const int32_t* d_prev,
                             int32_t* d_labels, float* d_win, uint32_t* d_changed, hipStream_t stream);

// d_cent[l][d], d < Dp, of every list l with members: the fp64 sum from +0.0 of d_rows[m][d] over its members m =
// d_members[d_offsets[l] .. d_offsets[l + 1]) in that order, one add after the other, divided in fp64 by the count and
// rounded once.  Lists without members are left alone.
hipError_t launch_ivf_means(const float* d_rows, int Dp, const uint32_t* d_members, const int64_t* d_offsets, int nlist,
                            float* d_cent, hipStream_t stream);

// d_out->distortion = the sum of (double)d_win[i] in a fixed order (leaves of kIvfDistLeaf, then the leaves' sums);
// d_out->n_empty = the lists l < nlist with d_counts[l] == 0.  d_partial [ivf_dist_partials(n)].  changed is not written.
hipError_t launch_ivf_round_stats(const float* d_win, int64_t n, const unsigned long long* d_counts, int nlist,
                                  double* d_partial, IvfRoundStats* d_out, hipStream_t stream);

// The repair of a round with E empty lists.  hipCUB's two-call protocol (d_temp NULL: *temp_bytes only): d_keys[i] =
// ~bits(d_win[i]) << 32 | i, sorted ascending into d_sorted (winning distance descending, then index ascending); then
// d_cent[d_empty[j]] = d_rows[row of d_sorted[j]], j < E.  d_empty: the empty lists in ascending order.
hipError_t ivf_train_repair(void* d_temp, size_t* temp_bytes, const float* d_win, int64_t n, uint64_t* d_keys,
                            uint64_t* d_sorted, const int32_t* d_empty, int E, const float* d_rows, int Dp, float* d_cent,
                            hipStream_t stream);

}  // namespace dpq
