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

// One training problem on the current device: the vectors as the split image sub[m][n][DsP] and every work array,
// uploaded once and shared by the start, the Lloyd rounds, the potential and any number of restarts.  Every member
// returns a dpq_status; *err gets the detail.  codewords are host arrays [M][K][Ds].
class Trainer {
public:
    Trainer();
    ~Trainer();
    Trainer(const Trainer&) = delete;
    Trainer& operator=(const Trainer&) = delete;

    int open(const float* vectors, int64_t n, int D, int M, int K, int Ds, std::string* err);
    int set_codebook(const float* codewords, std::string* err);
    int get_codebook(float* codewords, std::string* err);
    // The k-means++ start of `seed` into the device codebook.  potential: double [M] or NULL; ms: device time or NULL.
    int seed_kmeanspp(uint64_t seed, double* potential, double* ms, std::string* err);
    // Lloyd's rounds from the device codebook.  stats->wall_ms stays 0: the caller owns the whole call's clock.
    int lloyd(int max_iters, TrainStats* stats, std::string* err);
    // The leaf-ordered potential, double [M], of the device codebook: one more assignment, then the ordered sums.
    int potential(double* out, std::string* err);

private:
    struct Impl;
    Impl* p_;
};

}  // namespace dpq
