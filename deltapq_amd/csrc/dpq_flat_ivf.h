// dpq_flat_ivf.h -- launch interface of the inverted-list scan over raw fp32 rows (dpq_flat_ivf.hip): exact distances of
// the queries to the rows of the lists they probe, a running top-k per (query, probed list) (include/deltapq_amd.h "IVF
// search over raw vectors").  The lists are row numbers into a dpq_flat handle's own padded rows; they
// come from dpq_ivf.h's launch_ivf_label_keys and ivf_scan_and_sort, the probe rows from its launch_ivf_probes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kFlatIvfGroupMax = 16;  // pairs (query, probed list) one workgroup takes: 16, 8, 4, 2 or 1
constexpr int kFlatIvfGroup = 4;      // ... and the shipped choice: the fastest measured at nprobe 16
constexpr int kFlatIvfTileRows = 256;  // rows of a workgroup's tile
constexpr int kFlatIvfSliceDims = 32;  // dimensions of a tile that are in LDS at a time

// The group the scan runs with: the largest of 16, 8, 4, 2, 1 that is at most `group` and whose LDS -- the tiles beside
// group buffers of 2 P2 keys, P2 the power of two >= max(top_k, 256) -- fits a workgroup.
int flat_ivf_group(int top_k, int group);

// The pairs of a slice.  d_probes [n_pairs] is the pre-pass's output read as one row, entry i = q * nprobe + j:
// d_keys[i] = the list it names, nlist where it is -1; d_vals[i] = i.
hipError_t launch_flat_ivf_pairs(const int32_t* d_probes, int64_t n_pairs, int nlist, uint32_t* d_keys, uint32_t* d_vals,
                                 hipStream_t stream);

// hipCUB's two-call protocol (d_temp NULL: *temp_bytes only): a STABLE sort of (d_keys, d_vals) by key -- the pairs of
// a list stay in ascending (q, j) order, the padding pairs come last.
hipError_t flat_ivf_sort_pairs(void* d_temp, size_t* temp_bytes, const uint32_t* d_keys, uint32_t* d_keys_out,
                               const uint32_t* d_vals, uint32_t* d_vals_out, int64_t n_pairs, int nlist, hipStream_t stream);

// What the scan runs over: rows [n][Dp] fp32 padded with zeros (Dp % 4 == 0, 16-byte aligned); list l holds the row
// numbers d_list_rows[d_offsets[l] .. d_offsets[l + 1]), ascending.  Reported id = row + id_offset.
struct FlatIvfLists {
    const float* rows = nullptr;
    int Dp = 0;
    int64_t id_offset = 0;
    const int64_t* offsets = nullptr;
    const uint32_t* list_rows = nullptr;
    int nlist = 0;
};

// The list scan.  d_skeys / d_svals [n_pairs = nq * nprobe]: the sorted pairs.  A workgroup takes `group` consecutive
// pairs (see flat_ivf_group) and, for every stretch of equal list among them, reads the list's rows once for the
// stretch's queries.  d_queries [nq][Dp], padded as the rows are.  The distance of (row, query): per dimension in
// ascending order t = v[d] - q[d] and s = t * t, each rounded in fp32, summed on an fp64 accumulator from +0.0 and
// rounded once (dpq_flat.h's accumulate<kFlatL2> and make_key<kFlatL2>).  The best top_k of pair i = q * nprobe + j by
// key `distance bits << 32 | id` go to d_part_ids / d_part_dists [(j * nq + q)][top_k], padded with -1 / +inf:
// launch_ivf_scan's output contract.  The answer does not depend on the group.
hipError_t launch_flat_ivf_scan(const FlatIvfLists& lists, const float* d_queries, int nq, int nprobe, const uint32_t* d_skeys,
                                const uint32_t* d_svals, int top_k, int group, int32_t* d_part_ids, float* d_part_dists,
                                hipStream_t stream);

}  // namespace dpq
