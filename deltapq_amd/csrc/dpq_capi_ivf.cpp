// dpq_capi_ivf.cpp -- the IVF entry points of include/deltapq_amd.h (kernels in dpq_ivf.hip): inverted lists over a
// handle's nodes, built on the device from labels or from centroids, and the search that scans the lists a query probes.
#include "dpq_capi_internal.h"

namespace {

constexpr int64_t kIvfTileNodes = (int64_t)4 << 20;      // nodes decoded per tile (dpq_decode_range's bound)
constexpr int64_t kIvfAssignTile = 65536;                // nodes reconstructed per step of dpq_ivf_build
constexpr size_t kIvfAssignVecBytes = (size_t)64 << 20;  // ... and the bytes of their rows

dpq::RefineIds ivf_ids_of(const dpq_index* x) {
    dpq::RefineIds r{};
    r.id_base = (int64_t)x->img.id_base;
    r.n_local = x->img.n_local;
    r.n_total = x->img.n_codes_total;
    r.even_rule = x->plain ? 0 : 1;
    return r;
}

// A device and a handle whose codes the lookup decodes; settles what is in flight.
int ivf_enter_index(const std::string& who, dpq_index* x) {
    if (int rc = flat_device_present(who)) return rc;
    if (x->M != 8 && x->M != 16) return fail(DPQ_ERR_ARG, who + ": needs a handle of M = 8 or M = 16");
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    return DPQ_OK;
}

int ivf_nlist_ok(const std::string& who, int nlist) {
    if (nlist < 1 || nlist > dpq::kIvfMaxLists) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nlist <= 65536");
    return DPQ_OK;
}

// The handle's plain code values, a tile at a time, each node decoded once: fn(d_codes, l0, l1) sees the codes of local
// nodes l0 .. l1 - 1, [l1 - l0][M], and enqueues its work on `stream`, on which the next tile's decode overwrites them.  A
// plain handle is one tile, its own codes; a DTC handle goes through the bulk decode (decode_list_kernel, no
// relabelling) in tiles of whole segments, at most 4 Mi nodes, into a scratch that lives for the call.
template <class F>
int ivf_code_tiles(dpq_index* x, hipStream_t stream, F&& fn) {
    const int64_t n = x->img.n_local;
    if (x->plain) return fn(static_cast<const uint8_t*>(x->d_raw.get()), (int64_t)0, n);
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment, n_seg = x->img.n_segments;
    if (n_seg < 1 || n_seg * S < n) return fail(DPQ_ERR_STATE, "internal error: the handle's segments do not cover its nodes");
    int64_t tile_nodes = kIvfTileNodes;
    if (dev_mode())
        if (const char* e = getenv("DPQ_IVF_TILE_NODES")) tile_nodes = std::max<int64_t>(1, atoll(e));  // tests: several tiles of a small handle
    const int64_t tile = std::min(std::max<int64_t>(1, tile_nodes / S), n_seg);
    DevBuf<uint8_t> codes;
    DevBuf<uint32_t> segs;
    int rc = codes.alloc((size_t)(tile * S * x->M));
    if (!rc) rc = segs.alloc((size_t)n_seg);
    if (rc) return rc;
    std::vector<uint32_t> h_segs((size_t)n_seg);
    std::iota(h_segs.begin(), h_segs.end(), 0u);
    DPQ_HIP(hipMemcpy(segs, h_segs.data(), (size_t)n_seg * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (int64_t t0 = 0; t0 < n_seg && !rc; t0 += tile) {
        const int64_t nt = std::min(tile, n_seg - t0);
        DPQ_HIP(dpq::launch_decode_list(x->img, segs.get() + t0, (int)nt, nullptr, reinterpret_cast<uint32_t*>(codes.get()), stream));
        const int64_t l0 = t0 * S, l1 = std::min(n, (t0 + nt) * S);
        if (l1 > l0) rc = fn(static_cast<const uint8_t*>(codes.get()), l0, l1);
    }
    hipStreamSynchronize(stream);  // nothing may still read the scratch when it is freed
    return rc;
}

// The lists of d_labels[n] (n = the handle's nodes), all on `stream`; *out is a structure without centroids.
int ivf_from_device_labels(const std::string& who, dpq_index* x, const int32_t* d_labels, int64_t n, int nlist,
                           hipStream_t stream, std::unique_ptr<dpq_ivf>* out) {
    if (n != x->info.node_hi - x->info.node_lo || n != x->img.n_local)
        return fail(DPQ_ERR_ARG, who + ": n must be the handle's node_hi - node_lo");
    std::unique_ptr<dpq_ivf> v(new dpq_ivf());
    v->idx = x;
    v->device = x->device;
    v->nlist = nlist;
    v->M = x->M;
    DevBuf<uint32_t> keys, pos, keys_out, pos_out, flag;
    DevBuf<unsigned long long> counts;
    DevBuf<uint8_t> temp;
    int rc = keys.alloc((size_t)n);
    if (!rc) rc = pos.alloc((size_t)n);
    if (!rc) rc = keys_out.alloc((size_t)n);
    if (!rc) rc = pos_out.alloc((size_t)n);
    if (!rc) rc = counts.alloc((size_t)nlist + 1);
    if (!rc) rc = flag.alloc(1);
    if (!rc) rc = v->offsets.alloc((size_t)nlist + 1);
    if (rc) return rc;
    DPQ_HIP(hipMemsetAsync(counts, 0, ((size_t)nlist + 1) * sizeof(unsigned long long), stream));
    DPQ_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), stream));
    DPQ_HIP(dpq::launch_ivf_label_keys(d_labels, n, nlist, keys, pos, counts, flag, stream));
    size_t temp_bytes = 0;
    DPQ_HIP(dpq::ivf_scan_and_sort(nullptr, &temp_bytes, counts, v->offsets, nlist, keys, keys_out, pos, pos_out, n, stream));
    if ((rc = temp.alloc(temp_bytes))) return rc;
    DPQ_HIP(dpq::ivf_scan_and_sort(temp, &temp_bytes, counts, v->offsets, nlist, keys, keys_out, pos, pos_out, n, stream));
    v->h_offsets.resize((size_t)nlist + 1);
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(v->h_offsets.data(), v->offsets, ((size_t)nlist + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, who + ": a label is >= nlist");
    v->n_assigned = v->h_offsets[(size_t)nlist];
    v->n_unassigned = n - v->n_assigned;
    if (v->h_offsets[0] != 0 || v->n_assigned < 0 || v->n_assigned > n)
        return fail(DPQ_ERR_STATE, who + ": internal error: the list offsets do not add up");
    for (int l = 0; l < nlist; ++l) {
        const int64_t len = v->h_offsets[(size_t)l + 1] - v->h_offsets[(size_t)l];
        if (len < 0) return fail(DPQ_ERR_STATE, who + ": internal error: the list offsets do not ascend");
        v->max_list_len = std::max(v->max_list_len, len);
    }
    if ((rc = v->ids.alloc((size_t)v->n_assigned))) return rc;
    if ((rc = v->codes.alloc((size_t)v->n_assigned * x->M))) return rc;
    if (v->n_assigned > 0) {
        DPQ_HIP(dpq::launch_ivf_ids(pos_out, v->n_assigned, ivf_ids_of(x), v->ids, stream));
        // the nodes' plain code values in list order: every tile of decoded codes hands its nodes' codes to their entries
        const int64_t n_assigned = v->n_assigned;
        uint8_t* d_codes = v->codes;
        const uint32_t* d_pos = pos_out;
        rc = ivf_code_tiles(x, stream, [&](const uint8_t* d_tile, int64_t l0, int64_t l1) -> int {
            DPQ_HIP(dpq::launch_ivf_gather_codes(d_pos, n_assigned, l0, l1, d_tile, x->M, d_codes, stream));
            return DPQ_OK;
        });
        if (rc) return rc;
    }
    DPQ_HIP(hipStreamSynchronize(stream));
    v->device_bytes = ((int64_t)nlist + 1) * 8 + v->n_assigned * (4 + (int64_t)x->M);
    *out = std::move(v);
    return DPQ_OK;
}

// centroids[nlist][D] in host memory -> the device.  D = M * Ds is a multiple of 8 (M is 8 or 16), so the rows are
// already what the exact search takes: whole 16-byte loads, no padding.
int ivf_upload_centroids(dpq_index* x, const float* centroids, int nlist, DevBuf<float>* d_out, int* D_out) {
    const int D = x->M * x->Ds;
    if (int rc = d_out->alloc((size_t)nlist * D)) return rc;
    DPQ_HIP(hipMemcpy(d_out->get(), centroids, (size_t)nlist * D * sizeof(float), hipMemcpyHostToDevice));
    *D_out = D;
    return DPQ_OK;
}

dpq::FlatBase ivf_centroid_base(const float* d_centroids, int nlist, int D) {
    dpq::FlatBase b;
    b.format = dpq::kFlatF32;
    b.rows = d_centroids;
    b.n = nlist;
    b.D = D;
    b.Dp = D;
    b.n_entries = nlist;
    return b;
}

// d_labels[l] = the nearest centroid of local node l's reconstruction (the lowest list at a tie): per tile of decoded
// codes, in steps, the codebook's rows of the codes (dpq_reconstruct's rows), then the exact search with k = 1 over the
// centroids.
int ivf_assign(dpq_index* x, const float* d_centroids, int nlist, int D, int32_t* d_labels,
               int64_t n) {
    const int64_t tile = std::max<int64_t>(1, std::min(std::min(n, kIvfAssignTile), (int64_t)(kIvfAssignVecBytes / ((size_t)D * 4))));
    const int qb = (int)std::min<int64_t>(tile, dpq::flat_query_batch(1));
    DevBuf<float> vecs, dists;
    DevBuf<uint64_t> keys;
    DevBuf<dpq::FlatQueryState> state;
    int rc = vecs.alloc((size_t)tile * D);
    if (!rc) rc = dists.alloc((size_t)qb);
    if (!rc) rc = keys.alloc((size_t)qb * dpq::flat_key_capacity(1));
    if (!rc) rc = state.alloc((size_t)qb);
    if (rc) return rc;
    const dpq::FlatBase base = ivf_centroid_base(d_centroids, nlist, D);
    rc = ivf_code_tiles(x, nullptr, [&](const uint8_t* d_tile, int64_t l0, int64_t l1) -> int {
        for (int64_t t0 = l0; t0 < l1; t0 += tile) {
            const int64_t t = std::min(tile, l1 - t0);
            DPQ_HIP(dpq::launch_ivf_reconstruct(d_tile + (size_t)(t0 - l0) * x->M, t, x->M, x->K, x->Ds, x->d_codebook, vecs, nullptr));
            for (int64_t s0 = 0; s0 < t; s0 += qb) {
                const int m = (int)std::min<int64_t>(qb, t - s0);
                const dpq::FlatQueries q{vecs.get() + (size_t)s0 * D, nullptr, nullptr, m};
                DPQ_HIP(dpq::launch_flat_search(base, q, 1, keys, state, d_labels + t0 + s0, dists, nullptr));
            }
        }
        return DPQ_OK;
    });
    if (rc) return rc;
    DPQ_HIP(hipDeviceSynchronize());
    return DPQ_OK;
}

// ---- search ----------------------------------------------------------------------------------------------------------

int ivf_search_args(const std::string& who, const void* ivf, const void* queries, int nq, bool with_probes, const void* probes,
                    int nprobe, int top_k, const void* ids, const void* dists) {
    if (!ivf || !queries || (with_probes && !probes) || !ids || !dists || nq < 0)
        return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (top_k < 1 || top_k > dpq::kIvfMaxTopK) return fail(DPQ_ERR_ARG, who + ": needs 1 <= top_k <= 2048");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    return DPQ_OK;
}

// What needs the structure's fields; then a device and the handle's state.
int ivf_enter(const std::string& who, dpq_ivf* v, int nprobe, bool coarse) {
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (coarse && !v->centroids.get())
        return fail(DPQ_ERR_STATE, who + ": the structure has no centroids (dpq_ivf_build / dpq_ivf_set_centroids)");
    dpq_index* x = v->idx;
    if (int rc = ivf_enter_index(who, x)) return rc;
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (coarse && x->M * x->Ds != v->D) return fail(DPQ_ERR_STATE, who + ": the codebook's dimension is not the centroids'");
    return DPQ_OK;
}

// The coarse step, all device pointers: d_lists[nq][nprobe] the nearest centroids by (distance, list number),
// d_cdists[nq][nprobe] their distances.  Enqueues on `stream`.
int ivf_probe_on_device(dpq_ivf* v, const float* d_queries, int nq, int nprobe, int32_t* d_lists, float* d_cdists,
                        hipStream_t stream) {
    const int qb = std::min(nq, dpq::flat_query_batch(nprobe));
    int rc = grow(v->keys, &v->keys_n, (size_t)qb * dpq::flat_key_capacity(nprobe));
    if (!rc) rc = grow(v->state, &v->state_n, (size_t)qb);
    if (rc) return rc;
    const dpq::FlatBase base = ivf_centroid_base(v->centroids, v->nlist, v->D);
    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        const dpq::FlatQueries q{d_queries + (size_t)q0 * v->D, nullptr, nullptr, m};
        DPQ_HIP(dpq::launch_flat_search(base, q, nprobe, v->keys, v->state, d_lists + (size_t)q0 * nprobe,
                                        d_cdists + (size_t)q0 * nprobe, stream));
    }
    return DPQ_OK;
}

// The search behind its checks, all device pointers.  Slices of queries: per slice the tables, the probe pre-pass, the
// list scan, the merge of the lists' answers in rounds of what one merge holds.  Ends with the flag word read back.
int ivf_search_on_device(dpq_ivf* v, const std::string& who, const float* d_queries, int nq, const int32_t* d_probes,
                         int nprobe, int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    dpq_index* x = v->idx;
    const int M = x->M, K = x->K;
    const size_t row = (size_t)nprobe * top_k;
    const int per = (int)std::max<size_t>(1, std::min<size_t>(std::min(nq, dpq::kIvfSliceQueries), dpq::kIvfPartialBytes / (row * 8)));
    const int round = dpq::kIvfMergeKeys / top_k;  // lists one merge takes: at least 8
    int rc = grow(v->lut32, &v->lut_n, (size_t)per * M * 256);
    if (!rc) rc = grow(v->lut_min, &v->min_n, (size_t)per * M * dpq::kLutMinParts);
    if (!rc) rc = grow(v->probes, &v->probes_n, (size_t)per * nprobe);
    if (!rc) rc = grow(v->part_ids, &v->part_ids_n, (size_t)per * row);
    if (!rc) rc = grow(v->part_dists, &v->part_dists_n, (size_t)per * row);
    if (!rc && nprobe > round) rc = grow(v->tmp_ids, &v->tmp_ids_n, (size_t)per * top_k);
    if (!rc && nprobe > round) rc = grow(v->tmp_dists, &v->tmp_dists_n, (size_t)per * top_k);
    if (!rc && !v->flag.get()) rc = v->flag.alloc(1);
    if (rc) return rc;
    DPQ_HIP(hipMemsetAsync(v->flag, 0, sizeof(uint32_t), stream));
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const size_t list = (size_t)m * top_k;  // elements of one list's answers for the slice
        DPQ_HIP(dpq::launch_lut_build(x->d_codebook, d_queries + (size_t)q0 * M * x->Ds, m, m, M, K, x->Ds, v->lut32, v->lut_min,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, stream));
        DPQ_HIP(dpq::launch_ivf_probes(d_probes + (size_t)q0 * nprobe, m, nprobe, v->nlist, v->probes, v->flag, stream));
        DPQ_HIP(dpq::launch_ivf_scan(v->lut32, m, v->probes, nprobe, v->offsets, v->ids, v->codes, M, x->plain, top_k,
                                     v->part_ids, v->part_dists, stream));
        int32_t* out_i = d_ids + (size_t)q0 * top_k;
        float* out_d = d_dists + (size_t)q0 * top_k;
        // the lists are disjoint and the merge keeps every key, so a merge of merges is the merge of all: a round's
        // answer takes the place of the last list it consumed and opens the next round
        for (int l0 = 0;;) {
            const int l1 = std::min(l0 + round, nprobe);
            const bool last = l1 == nprobe;
            DPQ_HIP(dpq::launch_merge(v->part_ids.get() + (size_t)l0 * list, v->part_dists.get() + (size_t)l0 * list, l1 - l0, m,
                                      top_k, top_k, last ? out_i : v->tmp_ids.get(), last ? out_d : v->tmp_dists.get(), stream));
            if (last) break;
            l0 = l1 - 1;
            DPQ_HIP(hipMemcpyAsync(v->part_ids.get() + (size_t)l0 * list, v->tmp_ids, list * sizeof(int32_t),
                                   hipMemcpyDeviceToDevice, stream));
            DPQ_HIP(hipMemcpyAsync(v->part_dists.get() + (size_t)l0 * list, v->tmp_dists, list * sizeof(float),
                                   hipMemcpyDeviceToDevice, stream));
        }
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(&bad, v->flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, who + ": a probe names no list (an entry >= nlist)");
    return DPQ_OK;
}

// Staging of the host forms: the queries up; room for probes and results.
int ivf_stage(dpq_ivf* v, const float* queries, int nq, int nprobe, int top_k) {
    const size_t n_in = (size_t)nq * v->idx->M * v->idx->Ds;
    int rc = grow(v->d_in, &v->in_n, n_in);
    if (!rc) rc = grow(v->d_probes, &v->dprobes_n, (size_t)nq * nprobe);
    if (!rc) rc = grow(v->d_cdists, &v->cdists_n, (size_t)nq * nprobe);
    if (!rc && top_k > 0) rc = grow(v->d_ids, &v->ids_n, (size_t)nq * top_k);
    if (!rc && top_k > 0) rc = grow(v->d_dists, &v->dists_n, (size_t)nq * top_k);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(v->d_in, queries, n_in * sizeof(float), hipMemcpyHostToDevice));
    return DPQ_OK;
}

int ivf_results_down(dpq_ivf* v, int nq, int top_k, int32_t* ids, float* dists) {
    DPQ_HIP(hipMemcpy(ids, v->d_ids, (size_t)nq * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, v->d_dists, (size_t)nq * top_k * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_ivf_create_device(dpq_index* x, const int32_t* d_labels, int64_t n, int nlist, void* hip_stream, dpq_ivf** out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_create_device";
    if (out) *out = nullptr;
    if (!x || !d_labels || !out || n < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or n < 0");
    if (int rc = ivf_nlist_ok(who, nlist)) return rc;
    if (int rc = ivf_enter_index(who, x)) return rc;
    std::unique_ptr<dpq_ivf> v;
    if (int rc = ivf_from_device_labels(who, x, d_labels, n, nlist, (hipStream_t)hip_stream, &v)) return rc;
    *out = v.release();
    return DPQ_OK;
    });
}

int dpq_ivf_create(dpq_index* x, const int32_t* labels, int64_t n, int nlist, dpq_ivf** out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_create";
    if (out) *out = nullptr;
    if (!x || !labels || !out || n < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or n < 0");
    if (int rc = ivf_nlist_ok(who, nlist)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] >= nlist) {
            char msg[96];
            snprintf(msg, sizeof msg, ": labels[%lld] = %d is >= nlist", (long long)i, (int)labels[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    if (int rc = ivf_enter_index(who, x)) return rc;
    DevBuf<int32_t> d_labels;
    if (int rc = d_labels.alloc((size_t)n)) return rc;
    DPQ_HIP(hipMemcpy(d_labels, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    std::unique_ptr<dpq_ivf> v;
    if (int rc = ivf_from_device_labels(who, x, d_labels, n, nlist, nullptr, &v)) return rc;
    *out = v.release();
    return DPQ_OK;
    });
}

int dpq_ivf_build(dpq_index* x, const float* centroids, int nlist, dpq_ivf** out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_build";
    if (out) *out = nullptr;
    if (!x || !centroids || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = ivf_nlist_ok(who, nlist)) return rc;
    if (int rc = ivf_enter_index(who, x)) return rc;
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (x->M * x->Ds > dpq::kFlatMaxD) return fail(DPQ_ERR_ARG, who + ": M * Ds exceeds 2048");
    DevBuf<float> d_cent;
    int D = 0;
    if (int rc = ivf_upload_centroids(x, centroids, nlist, &d_cent, &D)) return rc;
    const int64_t n = x->img.n_local;
    DevBuf<int32_t> d_labels;
    if (int rc = d_labels.alloc((size_t)n)) return rc;
    if (int rc = ivf_assign(x, d_cent, nlist, D, d_labels, n)) return rc;
    std::unique_ptr<dpq_ivf> v;
    if (int rc = ivf_from_device_labels(who, x, d_labels, n, nlist, nullptr, &v)) return rc;
    v->centroids = std::move(d_cent);
    v->D = D;
    v->device_bytes += (int64_t)nlist * D * 4;
    *out = v.release();
    return DPQ_OK;
    });
}

int dpq_ivf_set_centroids(dpq_ivf* v, const float* centroids, int nlist) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_set_centroids";
    if (!v || !centroids) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (nlist != v->nlist) return fail(DPQ_ERR_ARG, who + ": nlist is not the structure's");
    dpq_index* x = v->idx;
    if (int rc = ivf_enter_index(who, x)) return rc;
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (x->M * x->Ds > dpq::kFlatMaxD) return fail(DPQ_ERR_ARG, who + ": M * Ds exceeds 2048");
    DevBuf<float> d_cent;
    int D = 0;
    if (int rc = ivf_upload_centroids(x, centroids, nlist, &d_cent, &D)) return rc;
    if (v->centroids.get()) v->device_bytes -= (int64_t)nlist * v->D * 4;
    v->centroids = std::move(d_cent);
    v->D = D;
    v->device_bytes += (int64_t)nlist * D * 4;
    return DPQ_OK;
    });
}

void dpq_ivf_free(dpq_ivf* v) {
    if (!v) return;
    hipSetDevice(v->device);
    delete v;
}

int dpq_ivf_get_info(const dpq_ivf* v, dpq_ivf_stats* out) {
    return guarded([&]() -> int {
    if (!v || !out) return fail(DPQ_ERR_ARG, "dpq_ivf_get_info: NULL argument");
    out->n_assigned = v->n_assigned;
    out->n_unassigned = v->n_unassigned;
    out->max_list_len = v->max_list_len;
    out->device_bytes = v->device_bytes;
    out->nlist = v->nlist;
    out->has_centroids = v->centroids.get() ? 1 : 0;
    return DPQ_OK;
    });
}

int dpq_ivf_get(const dpq_ivf* v, int64_t* offsets_out, int32_t* ids_out) {
    return guarded([&]() -> int {
    if (!v || !offsets_out) return fail(DPQ_ERR_ARG, "dpq_ivf_get: NULL argument");
    std::copy(v->h_offsets.begin(), v->h_offsets.end(), offsets_out);
    if (ids_out && v->n_assigned > 0) {
        DPQ_HIP(hipSetDevice(v->device));
        DPQ_HIP(hipMemcpy(ids_out, v->ids, (size_t)v->n_assigned * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return DPQ_OK;
    });
}

int dpq_ivf_search_probes_device(dpq_ivf* v, const float* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
                                 int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_search_probes_device";
    if (int rc = ivf_search_args(who, v, d_queries, nq, true, d_probes, nprobe, top_k, d_ids, d_dists)) return rc;
    if (int rc = ivf_enter(who, v, nprobe, false)) return rc;
    if (nq == 0) return DPQ_OK;
    return ivf_search_on_device(v, who, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, (hipStream_t)hip_stream);
    });
}

int dpq_ivf_search_probes(dpq_ivf* v, const float* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
                          float* dists) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_search_probes";
    if (int rc = ivf_search_args(who, v, queries, nq, true, probes, nprobe, top_k, ids, dists)) return rc;
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    for (size_t i = 0; i < (size_t)nq * nprobe; ++i)
        if (probes[i] >= v->nlist) {
            char msg[96];
            snprintf(msg, sizeof msg, ": entry %lld = %d names no list", (long long)i, (int)probes[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    if (int rc = ivf_enter(who, v, nprobe, false)) return rc;
    if (nq == 0) return DPQ_OK;
    if (int rc = ivf_stage(v, queries, nq, nprobe, top_k)) return rc;
    DPQ_HIP(hipMemcpy(v->d_probes, probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyHostToDevice));
    if (int rc = ivf_search_on_device(v, who, v->d_in, nq, v->d_probes, nprobe, top_k, v->d_ids, v->d_dists, nullptr)) return rc;
    return ivf_results_down(v, nq, top_k, ids, dists);
    });
}

int dpq_ivf_probe(dpq_ivf* v, const float* queries, int nq, int nprobe, int32_t* lists_out, float* dists_out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_probe";
    if (!v || !queries || !lists_out || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (int rc = ivf_enter(who, v, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    if (int rc = ivf_stage(v, queries, nq, nprobe, 0)) return rc;
    if (int rc = ivf_probe_on_device(v, v->d_in, nq, nprobe, v->d_probes, v->d_cdists, nullptr)) return rc;
    DPQ_HIP(hipMemcpy(lists_out, v->d_probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (dists_out) DPQ_HIP(hipMemcpy(dists_out, v->d_cdists, (size_t)nq * nprobe * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_ivf_search_device(dpq_ivf* v, const float* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
                          void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_search_device";
    if (int rc = ivf_search_args(who, v, d_queries, nq, false, nullptr, nprobe, top_k, d_ids, d_dists)) return rc;
    if (int rc = ivf_enter(who, v, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    int rc = grow(v->d_probes, &v->dprobes_n, (size_t)nq * nprobe);
    if (!rc) rc = grow(v->d_cdists, &v->cdists_n, (size_t)nq * nprobe);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if ((rc = ivf_probe_on_device(v, d_queries, nq, nprobe, v->d_probes, v->d_cdists, stream))) return rc;
    return ivf_search_on_device(v, who, d_queries, nq, v->d_probes, nprobe, top_k, d_ids, d_dists, stream);
    });
}

int dpq_ivf_search(dpq_ivf* v, const float* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_search";
    if (int rc = ivf_search_args(who, v, queries, nq, false, nullptr, nprobe, top_k, ids, dists)) return rc;
    if (int rc = ivf_enter(who, v, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    if (int rc = ivf_stage(v, queries, nq, nprobe, top_k)) return rc;
    if (int rc = ivf_probe_on_device(v, v->d_in, nq, nprobe, v->d_probes, v->d_cdists, nullptr)) return rc;
    if (int rc = ivf_search_on_device(v, who, v->d_in, nq, v->d_probes, nprobe, top_k, v->d_ids, v->d_dists, nullptr)) return rc;
    return ivf_results_down(v, nq, top_k, ids, dists);
    });
}

}  // extern "C"
