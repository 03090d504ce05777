// dpq_ivf.h -- launch interface of the inverted-file kernels (dpq_ivf.hip): lists of a handle's nodes built from labels
// on the device, and the list scan that keeps a running top-k per probed list (include/deltapq_amd.h "IVF search",
// DESIGN.md 5.16).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dpq_refine.h"

namespace dpq {

constexpr int kIvfMaxLists = 65536;    // nlist
constexpr int kIvfMaxProbe = 1024;     // nprobe (and min(nlist, .))
constexpr int kIvfMaxTopK = 2048;      // top_k: 2 * 2048 keys of the scan's LDS buffer are 32 KB
constexpr int kIvfSliceQueries = 2048; // queries one pass takes: their tables stay within 2048 * M KB
constexpr size_t kIvfPartialBytes = (size_t)256 << 20;  // ... and their partial lists [nprobe][queries][top_k] within this
constexpr int kIvfMergeKeys = 16384;   // keys one launch_merge holds (128 KB of LDS)

// The id a search reports for global DFS position `pos`: the position, except for the last node of an even-N DTC index.
__host__ __device__ inline int32_t ivf_report_id(int64_t pos, const RefineIds& r) {
    return (int32_t)((r.even_rule && (r.n_total & 1) == 0 && pos == r.n_total - 1) ? r.n_total : pos);
}

// Labels -> sort keys.  d_keys[l] = labels[l] where 0 <= label < nlist, nlist where the label is negative (the node is in
// no list) or >= nlist (*d_flag is raised too); d_pos[l] = l; d_counts[key] += 1 (d_counts [nlist + 1], zero at launch).
hipError_t launch_ivf_label_keys(const int32_t* d_labels, int64_t n, int nlist, uint32_t* d_keys, uint32_t* d_pos,
                                 unsigned long long* d_counts, uint32_t* d_flag, hipStream_t stream);

// hipCUB's two-call protocol (d_temp NULL: *temp_bytes only).  d_offsets [nlist + 1] = exclusive prefix of d_counts
// (d_offsets[nlist] = nodes in a list), and a STABLE sort of (d_keys, d_pos) by key into (d_keys_out, d_pos_out): the
// positions of a list ascend.
hipError_t ivf_scan_and_sort(void* d_temp, size_t* temp_bytes, const unsigned long long* d_counts, int64_t* d_offsets,
                             int nlist, const uint32_t* d_keys, uint32_t* d_keys_out, const uint32_t* d_pos,
                             uint32_t* d_pos_out, int64_t n, hipStream_t stream);

// d_ids[i] = the reported id of local node d_pos[i], i < n.
hipError_t launch_ivf_ids(const uint32_t* d_pos, int64_t n, const RefineIds& ids, int32_t* d_ids, hipStream_t stream);

// d_out[i] = the M code bytes of local node d_pos[i], for every i < n whose node lies in [l0, l1): d_tile holds the plain
// codes of nodes l0 .. l1 - 1, [l1 - l0][M].  Other entries are left alone.  M = 8 or 16; both arrays M-byte aligned.
hipError_t launch_ivf_gather_codes(const uint32_t* d_pos, int64_t n, int64_t l0, int64_t l1, const uint8_t* d_tile, int M,
                                   uint8_t* d_out, hipStream_t stream);

// d_out[i][m * Ds + d] = d_codebook[m][d_codes[i][m]][d], i < n: dpq_reconstruct's row of every code of a tile (a code
// byte >= K: quiet NaNs).
hipError_t launch_ivf_reconstruct(const uint8_t* d_codes, int64_t n, int M, int K, int Ds, const float* d_codebook,
                                  float* d_out, hipStream_t stream);

// The probe pre-pass.  d_out[q][j] = d_probes[q][j] where it names a list for the first time in its row, -1 where it is
// negative or a repeat; an entry >= nlist raises *d_flag (its entry is -1 too).  nprobe <= kIvfMaxProbe.
hipError_t launch_ivf_probes(const int32_t* d_probes, int nq, int nprobe, int nlist, int32_t* d_out, uint32_t* d_flag,
                             hipStream_t stream);

// The list scan: a workgroup per (probe, query).  d_probes [nq][nprobe] is the pre-pass's output; list l holds entries
// d_offsets[l] .. d_offsets[l + 1] of d_ids (reported ids) and d_codes ([entry][M], M = 8 or 16, 16-byte aligned).  The
// distance of an entry under d_lut32[q][M][256]: plain_rule -- M fp32 additions in ascending m; else the fp64 sum in
// ascending m, rounded once.  The list's best top_k by key `distance bits << 32 | id` go to d_part_ids / d_part_dists
// [(probe * nq + q)][top_k], padded with -1 / +inf: what launch_merge takes as nprobe lists of nq queries.
hipError_t launch_ivf_scan(const float* d_lut32, int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets,
                           const int32_t* d_ids, const uint8_t* d_codes, int M, bool plain_rule, int top_k,
                           int32_t* d_part_ids, float* d_part_dists, hipStream_t stream);

// ---- filters and range search over lists --------------------------------------------------------------
constexpr int64_t kIvfRangePoolKeys = (int64_t)8 << 20;  // keys of a range slice: 64 MB unsorted beside 64 MB sorted

// A dpq_filter as the list scans read it: bit l of `bits` is local node l of the handle (what dpq_filter::bits holds);
// an entry's reported id goes back to its node by undoing the even-N renaming (`even`: id N is position N - 1) and
// subtracting `base` (id_base).  bits == NULL: no filter (launch_ivf_range only).
struct IvfFilter {
    const uint32_t* bits = nullptr;
    int64_t base = 0, n_local = 0, N = 0;
    int32_t even = 0;
};

// launch_ivf_scan over the entries the filter allows: an entry it refuses forms no key (its bit is tested before its
// code is loaded).  A list without an eligible entry gives a row of padding.
hipError_t launch_ivf_scan_filtered(const float* d_lut32, int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets,
                                    const int32_t* d_ids, const uint8_t* d_codes, int M, bool plain_rule, const IvfFilter& filter,
                                    int top_k, int32_t* d_part_ids, float* d_part_dists, hipStream_t stream);

// The range scan, the same grid and table load.  d_thr[nq]: the radius keys -- distance bits << 32; 0 passes nothing
// (r <= 0), ~0 passes every entry (r = +inf).  d_pool == NULL, the count pass: d_counts[q][p] = the eligible entries of
// probe p's list with key < d_thr[q] (0 for padding, a repeat, an empty list).  Else the emit pass: those keys to
// d_pool[d_offs[q][p] - pool_base ..), in list order (d_offs: the exclusive scan of the counts; pool_base: the offset of
// the first query of this launch); nothing is written at or past pool_n.
hipError_t launch_ivf_range(const float* d_lut32, int nq, const int32_t* d_probes, int nprobe, const int64_t* d_offsets,
                            const int32_t* d_ids, const uint8_t* d_codes, int M, bool plain_rule, const IvfFilter& filter,
                            const uint64_t* d_thr, int64_t* d_counts, const int64_t* d_offs, int64_t pool_base, uint64_t* d_pool,
                            int64_t pool_n, hipStream_t stream);

// hipCUB's two-call protocol (d_temp NULL: *temp_bytes only): d_offs[n] = the exclusive prefix sum of d_counts[n].
hipError_t ivf_range_offsets(void* d_temp, size_t* temp_bytes, const int64_t* d_counts, int64_t* d_offs, int64_t n,
                             hipStream_t stream);

}  // namespace dpq
