// dpq_capi_ivf_train.cpp -- the coarse-quantiser entry points of include/deltapq_amd.h "IVF training" (kernels in
// dpq_ivf_train.hip, the lists of a round from dpq_ivf.hip): dpq_ivf_train, dpq_ivf_assign[_device], dpq_write_vecs.
#include "dpq_capi_internal.h"
#include "dpq_ivf_train.h"

namespace {

constexpr int64_t kAssignTileBytes = (int64_t)256 << 20;  // rows dpq_ivf_assign holds on the device at a time

int ivf_train_shape(const std::string& who, int D, int nlist) {
    if (D < 1 || D > dpq::kFlatMaxD) return fail(DPQ_ERR_ARG, who + ": needs 1 <= D <= 2048");
    if (nlist < 1 || nlist > dpq::kIvfMaxLists) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nlist <= 65536");
    return DPQ_OK;
}

int ivf_train_device(const std::string& who, int device) {
    if (int rc = flat_device_present(who)) return rc;
    int ndev = 0;
    hipGetDeviceCount(&ndev);
    if (device < 0 || device >= ndev) return fail(DPQ_ERR_NO_DEVICE, who + ": device ordinal out of range");
    DPQ_HIP(hipSetDevice(device));
    return DPQ_OK;
}

// rows[n][D] of host memory -> d_out[n][Dp], the padding zeros; `stage` holds the rows of one upload when D < Dp.
int upload_rows(const float* rows, int64_t n, int D, int Dp, float* d_out, DevBuf<float>& stage, int64_t stage_rows) {
    if (D == Dp) {
        DPQ_HIP(hipMemcpy(d_out, rows, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice));
        return DPQ_OK;
    }
    for (int64_t r0 = 0; r0 < n; r0 += stage_rows) {
        const int64_t m = std::min(stage_rows, n - r0);
        DPQ_HIP(hipMemcpy(stage, rows + (size_t)r0 * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice));
        DPQ_HIP(dpq::launch_flat_pad_rows(stage, m, D, Dp, d_out + (size_t)r0 * Dp, nullptr));
        DPQ_HIP(hipStreamSynchronize(nullptr));  // the next upload overwrites the staging rows
    }
    return DPQ_OK;
}

std::vector<float> padded(const float* rows, int64_t n, int D, int Dp) {
    std::vector<float> out((size_t)n * Dp, 0.0f);
    for (int64_t i = 0; i < n; ++i) memcpy(out.data() + (size_t)i * Dp, rows + (size_t)i * D, (size_t)D * sizeof(float));
    return out;
}

// Timing events of a call, destroyed with it.
struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() {
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
    hipError_t mark(hipStream_t stream) {
        hipEvent_t e = nullptr;
        if (hipError_t rc = hipEventCreate(&e)) return rc;
        ev.push_back(e);
        return hipEventRecord(e, stream);
    }
};

// "Start" without use_initial: dpq_train_codebook's rows start with K = nlist; centroid i is vector p[i].
void seeded_start(const float* vectors, int64_t n, int D, int nlist, uint64_t seed, float* centroids) {
    std::vector<int32_t> p((size_t)n);
    std::iota(p.begin(), p.end(), 0);
    uint64_t s = seed;
    for (int i = 0; i < nlist; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        std::swap(p[(size_t)i], p[(size_t)i + (size_t)(z % (uint64_t)(n - i))]);
        memcpy(centroids + (size_t)i * D, vectors + (size_t)p[(size_t)i] * D, (size_t)D * sizeof(float));
    }
}

}  // namespace

extern "C" {

int dpq_ivf_train(const float* vectors, int64_t n, int D, int nlist, const dpq_ivf_train_opts* opts, float* centroids,
                  dpq_ivf_train_stats* stats) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_train";
    const int device = opts ? opts->device : 0, max_iters = opts ? opts->max_iters : 25;
    const uint64_t seed = opts ? opts->seed : 0;
    const bool use_initial = opts && opts->use_initial;
    if (!vectors || !centroids) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = ivf_train_shape(who, D, nlist)) return rc;
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(DPQ_ERR_ARG, who + ": needs 1 <= n < 2^31");
    if (nlist > n) return fail(DPQ_ERR_ARG, who + ": fewer vectors than lists (nlist > n)");
    if (max_iters < 1 || max_iters > 64) return fail(DPQ_ERR_ARG, who + ": max_iters outside 1..64");
    if (opts && (opts->reserved[0] || opts->reserved[1] || opts->reserved[2])) return fail(DPQ_ERR_ARG, who + ": reserved is not 0");
    if (int rc = ivf_train_device(who, device)) return rc;
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    const auto wall0 = clock::now();
    const int Dp = (D + 3) & ~3;
    const int64_t stage_rows = std::max<int64_t>(1, std::min(n, kAssignTileBytes / ((int64_t)D * 4)));

    // one array of 4 n words serves the label sort (keys, positions, both sorted) and, behind a round's means, the
    // repair's 64-bit keys and their sorted copy
    DevBuf<float> d_rows, d_cent, d_win, stage;
    DevBuf<int32_t> d_labels, d_empty;
    DevBuf<uint32_t> sortbuf, flag;
    DevBuf<unsigned long long> counts;
    DevBuf<int64_t> offsets;
    DevBuf<double> partial;
    DevBuf<dpq::IvfRoundStats> d_stats;
    DevBuf<uint8_t> temp;
    int rc = d_rows.alloc((size_t)n * Dp);
    if (!rc) rc = d_cent.alloc((size_t)nlist * Dp);
    if (!rc) rc = d_win.alloc((size_t)n);
    if (!rc) rc = d_labels.alloc((size_t)n);
    if (!rc) rc = d_empty.alloc((size_t)nlist);
    if (!rc) rc = sortbuf.alloc((size_t)n * 4);
    if (!rc) rc = flag.alloc(1);
    if (!rc) rc = counts.alloc((size_t)nlist + 1);
    if (!rc) rc = offsets.alloc((size_t)nlist + 1);
    if (!rc) rc = partial.alloc(dpq::ivf_dist_partials(n));
    if (!rc) rc = d_stats.alloc(1);
    if (!rc && D != Dp) rc = stage.alloc((size_t)stage_rows * D);
    if (rc) return rc;
    uint32_t* keys = sortbuf.get();
    uint32_t *pos = keys + n, *keys_out = keys + 2 * n, *members = keys + 3 * n;
    uint64_t* rkeys = reinterpret_cast<uint64_t*>(keys);
    uint64_t* rsorted = reinterpret_cast<uint64_t*>(keys_out);
    size_t sort_bytes = 0, repair_bytes = 0;
    DPQ_HIP(dpq::ivf_scan_and_sort(nullptr, &sort_bytes, counts, offsets, nlist, keys, keys_out, pos, members, n, nullptr));
    DPQ_HIP(dpq::ivf_train_repair(nullptr, &repair_bytes, d_win, n, rkeys, rsorted, d_empty, 1, d_rows, Dp, d_cent, nullptr));
    size_t temp_bytes = std::max(sort_bytes, repair_bytes);
    if ((rc = temp.alloc(temp_bytes))) return rc;

    if (!use_initial) seeded_start(vectors, n, D, nlist, seed, centroids);
    if ((rc = upload_rows(vectors, n, D, Dp, d_rows, stage, stage_rows))) return rc;
    if (D == Dp) {
        DPQ_HIP(hipMemcpy(d_cent, centroids, (size_t)nlist * D * sizeof(float), hipMemcpyHostToDevice));
    } else {
        const std::vector<float> c = padded(centroids, nlist, D, Dp);
        DPQ_HIP(hipMemcpy(d_cent, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
    }

    hipStream_t stream = nullptr;
    Events ev;  // per round: 0 assign 1 lists 2 [host] 3 means 4 repair 5; a round that stops records the first three
    std::vector<int> ev_round;  // events a round recorded
    dpq_ivf_train_stats st{};
    std::vector<int64_t> h_offsets;
    std::vector<int32_t> h_empty;
    const auto rounds0 = clock::now();
    for (int r = 0; r < max_iters; ++r) {
        DPQ_HIP(hipMemsetAsync(d_stats, 0, sizeof(dpq::IvfRoundStats), stream));
        DPQ_HIP(hipMemsetAsync(counts, 0, ((size_t)nlist + 1) * sizeof(unsigned long long), stream));
        DPQ_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), stream));
        DPQ_HIP(ev.mark(stream));
        DPQ_HIP(dpq::launch_ivf_argmin(d_rows, n, Dp, d_cent, nlist, r ? d_labels.get() : nullptr, d_labels, d_win,
                                       &d_stats.get()->changed, stream));
        DPQ_HIP(ev.mark(stream));
        DPQ_HIP(dpq::launch_ivf_label_keys(d_labels, n, nlist, keys, pos, counts, flag, stream));
        DPQ_HIP(dpq::ivf_scan_and_sort(temp, &temp_bytes, counts, offsets, nlist, keys, keys_out, pos, members, n, stream));
        DPQ_HIP(dpq::launch_ivf_round_stats(d_win, n, counts, nlist, partial, d_stats, stream));
        DPQ_HIP(ev.mark(stream));
        dpq::IvfRoundStats h{};
        DPQ_HIP(hipMemcpyAsync(&h, d_stats, sizeof h, hipMemcpyDeviceToHost, stream));
        DPQ_HIP(hipStreamSynchronize(stream));
        st.distortion[r] = h.distortion;
        st.iters_run = r + 1;
        if (r > 0 && h.changed == 0 && h.n_empty == 0) {
            st.converged = 1;
            ev_round.push_back(3);
            break;
        }
        DPQ_HIP(ev.mark(stream));
        DPQ_HIP(dpq::launch_ivf_means(d_rows, Dp, members, offsets, nlist, d_cent, stream));
        DPQ_HIP(ev.mark(stream));
        if (h.n_empty) {
            // rare: the empty lists are found on the host, in ascending order
            h_offsets.resize((size_t)nlist + 1);
            DPQ_HIP(hipMemcpyAsync(h_offsets.data(), offsets, h_offsets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
            DPQ_HIP(hipStreamSynchronize(stream));
            h_empty.clear();
            for (int l = 0; l < nlist; ++l)
                if (h_offsets[(size_t)l + 1] == h_offsets[(size_t)l]) h_empty.push_back(l);
            if ((int64_t)h_empty.size() != (int64_t)h.n_empty)
                return fail(DPQ_ERR_STATE, who + ": internal error: the empty lists do not add up");
            DPQ_HIP(hipMemcpyAsync(d_empty, h_empty.data(), h_empty.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            DPQ_HIP(dpq::ivf_train_repair(temp, &temp_bytes, d_win, n, rkeys, rsorted, d_empty, (int)h_empty.size(), d_rows, Dp,
                                          d_cent, stream));
            DPQ_HIP(hipStreamSynchronize(stream));  // h_empty is read by the copy until here
            st.reseeded += (int64_t)h_empty.size();
        }
        DPQ_HIP(ev.mark(stream));
        ev_round.push_back(6);
    }
    DPQ_HIP(hipStreamSynchronize(stream));
    st.rounds_ms = ms_since(rounds0);
    size_t at = 0;
    for (int cnt : ev_round) {
        float a = 0, b = 0, c = 0, d = 0;
        DPQ_HIP(hipEventElapsedTime(&a, ev.ev[at], ev.ev[at + 1]));
        DPQ_HIP(hipEventElapsedTime(&b, ev.ev[at + 1], ev.ev[at + 2]));
        if (cnt == 6) {
            DPQ_HIP(hipEventElapsedTime(&c, ev.ev[at + 3], ev.ev[at + 4]));
            DPQ_HIP(hipEventElapsedTime(&d, ev.ev[at + 4], ev.ev[at + 5]));
        }
        st.assign_ms += a;
        st.update_ms += (double)b + c;
        st.repair_ms += d;
        at += (size_t)cnt;
    }
    st.gpu_ms = st.assign_ms + st.update_ms + st.repair_ms;

    if (D == Dp) {
        DPQ_HIP(hipMemcpy(centroids, d_cent, (size_t)nlist * D * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        std::vector<float> c((size_t)nlist * Dp);
        DPQ_HIP(hipMemcpy(c.data(), d_cent, c.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int l = 0; l < nlist; ++l) memcpy(centroids + (size_t)l * D, c.data() + (size_t)l * Dp, (size_t)D * sizeof(float));
    }
    st.wall_ms = ms_since(wall0);
    if (stats) *stats = st;
    return DPQ_OK;
    });
}

int dpq_ivf_assign(const float* centroids, int nlist, int D, const float* vectors, int64_t n, int device, int32_t* labels_out,
                   float* dists_out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_assign";
    if (!centroids || !vectors || !labels_out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = ivf_train_shape(who, D, nlist)) return rc;
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(DPQ_ERR_ARG, who + ": needs 0 <= n < 2^31");
    if (int rc = ivf_train_device(who, device)) return rc;
    if (n == 0) return DPQ_OK;
    const int Dp = (D + 3) & ~3;
    const int64_t tile = std::max<int64_t>(1, std::min(n, kAssignTileBytes / ((int64_t)Dp * 4)));
    DevBuf<float> d_rows, d_cent, d_win, stage;
    DevBuf<int32_t> d_labels;
    int rc = d_rows.alloc((size_t)tile * Dp);
    if (!rc) rc = d_cent.alloc((size_t)nlist * Dp);
    if (!rc) rc = d_win.alloc((size_t)tile);
    if (!rc) rc = d_labels.alloc((size_t)tile);
    if (!rc && D != Dp) rc = stage.alloc((size_t)tile * D);
    if (rc) return rc;
    if (D == Dp) {
        DPQ_HIP(hipMemcpy(d_cent, centroids, (size_t)nlist * D * sizeof(float), hipMemcpyHostToDevice));
    } else {
        const std::vector<float> c = padded(centroids, nlist, D, Dp);
        DPQ_HIP(hipMemcpy(d_cent, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    for (int64_t r0 = 0; r0 < n; r0 += tile) {
        const int64_t m = std::min(tile, n - r0);
        if ((rc = upload_rows(vectors + (size_t)r0 * D, m, D, Dp, d_rows, stage, tile))) return rc;
        DPQ_HIP(dpq::launch_ivf_argmin(d_rows, m, Dp, d_cent, nlist, nullptr, d_labels, d_win, nullptr, nullptr));
        DPQ_HIP(hipMemcpy(labels_out + r0, d_labels, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (dists_out) DPQ_HIP(hipMemcpy(dists_out + r0, d_win, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
    }
    return DPQ_OK;
    });
}

int dpq_ivf_assign_device(const float* d_centroids, int nlist, int D, const float* d_vectors, int64_t n, int32_t* d_labels,
                          float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_assign_device";
    if (!d_centroids || !d_vectors || !d_labels) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = ivf_train_shape(who, D, nlist)) return rc;
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(DPQ_ERR_ARG, who + ": needs 0 <= n < 2^31");
    if (D % 4 != 0) return fail(DPQ_ERR_ARG, who + ": needs D % 4 == 0 (pad the rows with zeros)");
    if ((reinterpret_cast<uintptr_t>(d_centroids) | reinterpret_cast<uintptr_t>(d_vectors)) & 15u)
        return fail(DPQ_ERR_ARG, who + ": the rows must be 16-byte aligned");
    if (int rc = flat_device_present(who)) return rc;
    if (n == 0) return DPQ_OK;
    const hipError_t e = dpq::launch_ivf_argmin(d_vectors, n, D, d_centroids, nlist, nullptr, d_labels, d_dists, nullptr,
                                                (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(DPQ_ERR_HIP, who + ": " + hipGetErrorString(e));
    return DPQ_OK;
    });
}

int dpq_write_vecs(const char* path, const float* vectors, int64_t n, int D) {
    return guarded([&]() -> int {
    const std::string who = "dpq_write_vecs";
    if (!path || !vectors) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 0 || D < 1) return fail(DPQ_ERR_ARG, who + ": n < 0 or D < 1");
    FILE* f = fopen(path, "wb");
    if (!f) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    const int32_t d32 = D;
    bool ok = true;
    for (int64_t i = 0; i < n && ok; ++i)
        ok = fwrite(&d32, 4, 1, f) == 1 && fwrite(vectors + (size_t)i * D, sizeof(float), (size_t)D, f) == (size_t)D;
    if (fclose(f) != 0 || !ok) return fail(DPQ_ERR_IO, std::string("short write on ") + path);
    return DPQ_OK;
    });
}

}  // extern "C"
