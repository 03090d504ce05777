// dpq_train.h -- codebook learning on the GPU (dpq_train.hip): Lloyd's k-means per sub-space with exact,
// stated arithmetic.  No reference semantics (cv::kmeans): the rules are this build's own, see DESIGN.md 5.9
// and include/deltapq_amd.h.
#pragma once
#include <cstdint>
#include <string>

namespace dpq {

struct TrainStats {
    int iters_run = 0;       // rounds in which an assignment ran
    int converged = 0;       // 1: every sub-space stopped by the rule before max_iters ran out
    int64_t reseeded = 0;    // empty clusters repaired, all rounds and sub-spaces
    double distortion[64] = {};
    double gpu_ms = 0;     // assign_ms + update_ms + repair_ms (device events)
    double wall_ms = 0;    // the whole call: upload, rounds, download
    double rounds_ms = 0;  // host clock around the rounds; minus gpu_ms = the host round trips
    double assign_ms = 0, update_ms = 0, repair_ms = 0;  // update_ms: label sort + means
};

// Ds rounded up to a width the assignment kernel is built for (zero padding adds exact zeros to a distance);
// 0 when Ds is above the widest one.
int train_padded_ds(int Ds);
// Dynamic LDS of the assignment kernel: the sub-space's padded codewords, the label histogram, the block sums.
// 0 when train_padded_ds(Ds) is.
size_t train_lds_bytes(int K, int Ds);

// Runs on the current device.  codewords [M][K][Ds]: the start on entry, the trained codebook on return.
// Returns a dpq_status; *err gets the detail.
int train_codebook(const float* vectors, int64_t n, int D, int M, int K, int Ds, int max_iters, float* codewords,
                   TrainStats* stats, std::string* err);

}  // namespace dpq
