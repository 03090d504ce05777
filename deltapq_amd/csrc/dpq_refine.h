// dpq_refine.h -- launch interface of the residual re-ranking kernels (dpq_refine.hip): a second product quantizer
// over the residuals of the first (include/deltapq_amd.h "residual re-ranking").
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dpq {

constexpr int kRefineMaxM2 = 64;              // sub-spaces of a level (its codes are staged in LDS, 64 bytes a candidate)
constexpr int kRefineMaxCand = 16384;         // candidates per query (the sort's LDS list, kFlatMaxTopK)
constexpr int64_t kRefineSlice = (int64_t)1 << 20;  // candidates, ids or nodes one pass takes

// Which reported ids name a node of the handle, and where: the code lookup's rule (dpq_lookup.hip).
struct RefineIds {
    int64_t id_base;    // global DFS position of local node 0
    int64_t n_local;    // nodes of the handle
    int64_t n_total;    // N of the whole index (or of the opened prefix)
    int32_t even_rule;  // 1: DTC index -- for even N the id N names position N - 1 and N - 1 names nothing
};

// Both codebooks of a level and its codes.
struct RefineLevelArgs {
    const float* cw1;       // [M][K][Ds]
    const float* cw2;       // [M2][K2][Ds2]
    const uint8_t* codes2;  // [n_local][M2]
    int32_t M, K, Ds, D1;   // D1 = M * Ds
    int32_t M2, K2, Ds2;
};

// out[i][j] = (j < D ? rows[i][j] : 0) - cw1[j / Ds][codes1[i][j / Ds]][j % Ds], j < D1.  d_ids (may be NULL: every row
// is a node): a negative id gives D1 quiet NaNs.  A code byte >= K has no codeword: its Ds floats are NaN.
hipError_t launch_refine_residual(const float* d_rows, int64_t n, int D, const int32_t* d_ids, const uint8_t* d_codes1,
                                  const RefineLevelArgs& lv, float* d_out, hipStream_t stream);

// out[i][j] = cw1[..codes1[i]..][j] + cw2[j / Ds2][codes2[local(ids[i])][j / Ds2]][j % Ds2].  An id that is negative
// or names no node gives D1 quiet NaNs (the caller's lookup of codes1 has raised the flag for the latter).
hipError_t launch_refine_reconstruct(const int32_t* d_ids, int64_t n, const uint8_t* d_codes1, const RefineLevelArgs& lv,
                                     const RefineIds& ids, float* d_out, hipStream_t stream);

// Refined distances of cand[nq][n_cand] (d_codes1 [nq][n_cand][M]: the candidates' level-1 codes) to queries [nq][D1],
// the best top_k by (distance bits, candidate id).  d_keys [nq][refine_rerank_keys(n_cand)].  *d_flag is set when a
// non-negative candidate names no node.
hipError_t launch_refine_rerank(const float* d_queries, int nq, const int32_t* d_cand, int n_cand, int top_k,
                                const uint8_t* d_codes1, const RefineLevelArgs& lv, const RefineIds& ids, uint64_t* d_keys,
                                uint32_t* d_flag, int32_t* d_ids, float* d_dists, hipStream_t stream);
size_t refine_rerank_keys(int n_cand);  // keys per query launch_refine_rerank needs

}  // namespace dpq
