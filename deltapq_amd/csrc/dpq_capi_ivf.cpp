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
int ivf_enter(const std::string& who, dpq_ivf* v, int nprobe, bool coarse, bool codebook = true) {
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (coarse && !v->centroids.get())
        return fail(DPQ_ERR_STATE, who + ": the structure has no centroids (dpq_ivf_build / dpq_ivf_set_centroids)");
    dpq_index* x = v->idx;
    if (int rc = ivf_enter_index(who, x)) return rc;
    if (codebook && !x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (coarse && x->M * x->Ds != v->D) return fail(DPQ_ERR_STATE, who + ": the codebook's dimension is not the centroids'");
    return DPQ_OK;
}

// The coarse step, all device pointers: d_lists[nq][nprobe] the nearest centroids by (distance, list number),
// d_cdists[nq][nprobe] their distances -- metric dpq::kFlatIP: the centroids of largest exact inner product by (score
// descending, list number), and their scores.  Enqueues on `stream`.
int ivf_probe_on_device(dpq_ivf* v, const float* d_queries, int nq, int nprobe, int32_t* d_lists, float* d_cdists,
                        hipStream_t stream, int metric = dpq::kFlatL2) {
    const int qb = std::min(nq, dpq::flat_query_batch(nprobe));
    int rc = grow(v->keys, &v->keys_n, (size_t)qb * dpq::flat_key_capacity(nprobe));
    if (!rc) rc = grow(v->state, &v->state_n, (size_t)qb);
    if (rc) return rc;
    dpq::FlatBase base = ivf_centroid_base(v->centroids, v->nlist, v->D);
    base.metric = metric;
    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        const dpq::FlatQueries q{d_queries + (size_t)q0 * v->D, nullptr, nullptr, m};
        DPQ_HIP(dpq::launch_flat_search(base, q, nprobe, v->keys, v->state, d_lists + (size_t)q0 * nprobe,
                                        d_cdists + (size_t)q0 * nprobe, stream));
    }
    return DPQ_OK;
}

// Where a slice's exact tables come from, and who may be scanned.
enum { kIvfQueries = 0, kIvfTables = 1, kIvfIp = 2 };
struct IvfSource {
    int kind = kIvfQueries;
    const float* d_in = nullptr;         // queries [nq][M * Ds] (kIvfQueries, kIvfIp) or tables [nq][M][K] (kIvfTables)
    const dpq_filter* filter = nullptr;  // NULL: every entry of a list
    float* d_bias = nullptr;             // kIvfIp: [nq] dpq_ip_tables' bias, and d_scores[nq][top_k] the scores made of
    float* d_scores = nullptr;           // it and the gaps (the search's distances) behind the last slice
};

dpq::IvfFilter ivf_filter_of(const dpq_filter* f) {
    dpq::IvfFilter g;
    if (!f) return g;
    g.bits = f->bits;
    g.base = f->base;
    g.n_local = f->n_local;
    g.N = f->N;
    g.even = (!f->plain && (f->N & 1) == 0) ? 1 : 0;
    return g;
}

// The exact tables of queries q0 .. q0 + m - 1 into v->lut32: from the queries and the codebook, from the caller's tables,
// or from the inner-product tables of the queries (into v->tab first, their bias to the caller).
int ivf_slice_tables(dpq_ivf* v, const IvfSource& s, int q0, int m, hipStream_t stream) {
    dpq_index* x = v->idx;
    const int M = x->M, K = x->K;
    if (s.kind == kIvfQueries) {
        DPQ_HIP(dpq::launch_lut_build(x->d_codebook, s.d_in + (size_t)q0 * M * x->Ds, m, m, M, K, x->Ds, v->lut32, v->lut_min,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, stream));
        return DPQ_OK;
    }
    const float* tab = s.d_in + (size_t)q0 * M * K;
    if (s.kind == kIvfIp) {
        DPQ_HIP(dpq::launch_ip_tables(x->d_codebook, s.d_in + (size_t)q0 * M * x->Ds, m, M, K, x->Ds, v->tab, s.d_bias + q0, stream));
        tab = v->tab;
    }
    DPQ_HIP(dpq::launch_tables_ingest(tab, m, m, M, K, v->lut32, v->lut_min, nullptr, nullptr, nullptr, nullptr,
                                      v->flag.get() + 1, stream));
    return DPQ_OK;
}

// The two flag words behind a call's last launch: the closing synchronisation.
int ivf_read_flags(dpq_ivf* v, const std::string& who, int kind, hipStream_t stream) {
    uint32_t bad[2] = {0, 0};
    DPQ_HIP(hipMemcpyAsync(bad, v->flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad[0]) return fail(DPQ_ERR_ARG, who + ": a probe names no list (an entry >= nlist)");
    if (bad[1])
        return fail(DPQ_ERR_ARG, who + (kind == kIvfIp ? ": a query or codeword is not finite (or a dot product is not); the outputs are unspecified"
                                                       : ": a table entry is negative or a NaN; the outputs are unspecified"));
    return DPQ_OK;
}

// The search behind its checks, all device pointers.  Slices of queries: per slice the tables, the probe pre-pass, the
// list scan, the merge of the lists' answers in rounds of what one merge holds.  Ends with the flag words read back.
int ivf_search_on_device(dpq_ivf* v, const std::string& who, const IvfSource& src, int nq, const int32_t* d_probes,
                         int nprobe, int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    dpq_index* x = v->idx;
    const int M = x->M, K = x->K;
    const dpq::IvfFilter filt = ivf_filter_of(src.filter);
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
    if (!rc && src.kind == kIvfIp) rc = grow(v->tab, &v->tab_n, (size_t)per * M * K);
    if (!rc && !v->flag.get()) rc = v->flag.alloc(2);
    if (rc) return rc;
    DPQ_HIP(hipMemsetAsync(v->flag, 0, 2 * sizeof(uint32_t), stream));
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const size_t list = (size_t)m * top_k;  // elements of one list's answers for the slice
        if ((rc = ivf_slice_tables(v, src, q0, m, stream))) return rc;
        DPQ_HIP(dpq::launch_ivf_probes(d_probes + (size_t)q0 * nprobe, m, nprobe, v->nlist, v->probes, v->flag, stream));
        if (filt.bits)
            DPQ_HIP(dpq::launch_ivf_scan_filtered(v->lut32, m, v->probes, nprobe, v->offsets, v->ids, v->codes, M, x->plain, filt,
                                                  top_k, v->part_ids, v->part_dists, stream));
        else
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
    if (src.d_scores) DPQ_HIP(dpq::launch_ip_scores(src.d_bias, d_dists, d_ids, nq, top_k, src.d_scores, stream));
    return ivf_read_flags(v, who, src.kind, stream);
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

// ---- filters, caller tables, inner product ------------------------------------------------------------

// One top-k call of the forms that came after the unfiltered L2 search.  `in`: queries, or tables (kIvfTables).
struct IvfCall {
    const char* fn;
    int kind;          // kIvfQueries / kIvfTables / kIvfIp
    bool need_filter;  // the _filtered forms: a NULL filter is an error
    bool coarse;       // the probes come from the centroids (kIvfIp: by inner product)
    bool device;       // device pointers, results complete on return
    const dpq_filter* filter;
    const float* in;
    int nq;
    const int32_t* probes;
    int nprobe, top_k;
    int32_t* ids;
    float* dists;  // kIvfIp: the scores
    float* gaps;   // kIvfIp, may be NULL
    float* bias;
    hipStream_t stream;
};

int ivf_probe_rows_ok(const std::string& who, const dpq_ivf* v, const int32_t* probes, int nq, int nprobe) {
    for (size_t i = 0; i < (size_t)nq * nprobe; ++i)
        if (probes[i] >= v->nlist) {
            char msg[96];
            snprintf(msg, sizeof msg, ": entry %lld = %d names no list", (long long)i, (int)probes[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    return DPQ_OK;
}

int ivf_call(dpq_ivf* v, const IvfCall& c) {
    const std::string who = c.fn;
    if (int rc = ivf_search_args(who, v, c.in, c.nq, !c.coarse, c.probes, c.nprobe, c.top_k, c.ids, c.dists)) return rc;
    if (c.need_filter && !c.filter) return fail(DPQ_ERR_ARG, who + ": filter is NULL");
    if (c.nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    dpq_index* x = v->idx;
    if (c.filter && c.filter->owner != x->serial)
        return fail(DPQ_ERR_ARG, who + ": the filter was made for another index handle");
    const bool tables = c.kind == kIvfTables;
    const size_t n_in = (size_t)c.nq * x->M * (tables ? x->K : x->Ds), n_out = (size_t)c.nq * c.top_k;
    if (!c.device) {
        if (!c.coarse)
            if (int rc = ivf_probe_rows_ok(who, v, c.probes, c.nq, c.nprobe)) return rc;
        if (tables)
            for (size_t i = 0; i < n_in; ++i)
                if (!(c.in[i] >= 0.0f)) return fail(DPQ_ERR_ARG, who + ": table entry " + std::to_string(i) + " is negative or a NaN");
    }
    if (int rc = ivf_enter(who, v, c.nprobe, c.coarse, !tables)) return rc;
    if (c.nq == 0) return DPQ_OK;
    const bool ip = c.kind == kIvfIp;
    IvfSource src;
    src.kind = c.kind;
    src.filter = c.filter;
    const int32_t* d_probes = c.probes;
    int32_t* d_ids = c.ids;
    float *d_out = c.dists, *d_gaps = c.gaps, *d_bias = c.bias;
    int rc = DPQ_OK;
    if (c.device) {
        src.d_in = c.in;
        if (c.coarse) {
            rc = grow(v->d_probes, &v->dprobes_n, (size_t)c.nq * c.nprobe);
            if (!rc) rc = grow(v->d_cdists, &v->cdists_n, (size_t)c.nq * c.nprobe);
        }
    } else {
        // ivf_stage brings queries up; tables take the same staging buffer
        rc = grow(v->d_in, &v->in_n, n_in);
        if (!rc) rc = grow(v->d_probes, &v->dprobes_n, (size_t)c.nq * c.nprobe);
        if (!rc) rc = grow(v->d_cdists, &v->cdists_n, (size_t)c.nq * c.nprobe);
        if (!rc) rc = grow(v->d_ids, &v->ids_n, n_out);
        if (!rc) rc = grow(v->d_dists, &v->dists_n, n_out);
        if (rc) return rc;
        DPQ_HIP(hipMemcpy(v->d_in, c.in, n_in * sizeof(float), hipMemcpyHostToDevice));
        if (!c.coarse) DPQ_HIP(hipMemcpy(v->d_probes, c.probes, (size_t)c.nq * c.nprobe * sizeof(int32_t), hipMemcpyHostToDevice));
        src.d_in = v->d_in;
        d_ids = v->d_ids;
        d_out = v->d_dists;
        d_gaps = d_bias = nullptr;
    }
    if (!rc && ip && !d_gaps) {
        rc = grow(v->d_gaps, &v->gaps_n, n_out);
        d_gaps = v->d_gaps;
    }
    if (!rc && ip && !d_bias) {
        rc = grow(v->d_bias, &v->bias_n, (size_t)c.nq);
        d_bias = v->d_bias;
    }
    if (rc) return rc;
    if (c.coarse) {
        if ((rc = ivf_probe_on_device(v, src.d_in, c.nq, c.nprobe, v->d_probes, v->d_cdists, c.stream,
                                      ip ? dpq::kFlatIP : dpq::kFlatL2)))
            return rc;
        d_probes = v->d_probes;
    } else if (!c.device) {
        d_probes = v->d_probes;
    }
    if (ip) {
        src.d_bias = d_bias;
        src.d_scores = d_out;
    }
    if ((rc = ivf_search_on_device(v, who, src, c.nq, d_probes, c.nprobe, c.top_k, d_ids, ip ? d_gaps : d_out, c.stream))) return rc;
    if (c.device) return DPQ_OK;
    DPQ_HIP(hipMemcpy(c.ids, d_ids, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(c.dists, d_out, n_out * sizeof(float), hipMemcpyDeviceToHost));
    if (ip && c.gaps) DPQ_HIP(hipMemcpy(c.gaps, d_gaps, n_out * sizeof(float), hipMemcpyDeviceToHost));
    if (ip && c.bias) DPQ_HIP(hipMemcpy(c.bias, d_bias, (size_t)c.nq * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

// ---- range search over lists ---------------------------------------------------------------------------------------

// Keys a group of queries may lay out in the structure's pool (a longer single list works in buffers of the call).
int64_t ivf_range_pool_keys() {
    int64_t keys = dpq::kIvfRangePoolKeys;
    if (dev_mode())
        if (const char* e = getenv("DPQ_IVF_RANGE_POOL_KEYS"))  // tests: several groups, and a call-local pool, at a small size
            keys = std::min(keys, std::max<int64_t>(1, atoll(e)));
    return keys;
}

// dpq_ivf_range_search[_probes].  probes == NULL: the coarse step.  Slices of at most 2048 queries: their tables, the probe
// pre-pass, the count pass and its exclusive scan, and ONE host round trip for the queries' totals; then groups of queries
// whose lists fit the pool: the emit pass, the segmented sort, the keys down and split on the host.
int ivf_range_call(const char* fn, dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, const int32_t* probes,
                   bool coarse, int nprobe, const float* radii, dpq_range_result** out) {
    const std::string who = fn;
    if (!out) return fail(DPQ_ERR_ARG, who + ": out is NULL");
    *out = nullptr;
    if (!v || nq < 0 || (nq > 0 && (!queries || !radii || (!coarse && !probes))))
        return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    for (int q = 0; q < nq; ++q)
        if (std::isnan(radii[q])) return fail(DPQ_ERR_ARG, who + ": radius of query " + std::to_string(q) + " is NaN");
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    dpq_index* x = v->idx;
    if (filter && filter->owner != x->serial) return fail(DPQ_ERR_ARG, who + ": the filter was made for another index handle");
    if (!coarse)
        if (int rc = ivf_probe_rows_ok(who, v, probes, nq, nprobe)) return rc;
    if (int rc = ivf_enter(who, v, nprobe, coarse)) return rc;
    std::unique_ptr<dpq_range_result> res(new dpq_range_result());
    res->nq = nq;
    res->lims.assign((size_t)nq + 1, 0);
    if (nq == 0) {
        *out = res.release();
        return DPQ_OK;
    }
    const int M = x->M;
    const int per = std::min(nq, dpq::kIvfSliceQueries);
    const size_t slots = (size_t)per * nprobe + 1;
    const int64_t budget = ivf_range_pool_keys();
    int rc = ivf_stage(v, queries, nq, nprobe, 0);
    if (!rc) rc = grow(v->lut32, &v->lut_n, (size_t)per * M * 256);
    if (!rc) rc = grow(v->lut_min, &v->min_n, (size_t)per * M * dpq::kLutMinParts);
    if (!rc) rc = grow(v->probes, &v->probes_n, (size_t)per * nprobe);
    if (!rc) rc = grow(v->r_thr, &v->r_thr_n, (size_t)nq);
    if (!rc) rc = grow(v->r_counts, &v->r_counts_n, slots);
    if (!rc) rc = grow(v->r_offs, &v->r_offs_n, slots);
    if (!rc) rc = grow(v->r_qoffs, &v->r_qoffs_n, (size_t)per + 1);
    if (!rc) rc = grow(v->r_pool, &v->r_pool_n, (size_t)budget);
    if (!rc) rc = grow(v->r_sorted, &v->r_sorted_n, (size_t)budget);
    if (!rc && !v->flag.get()) rc = v->flag.alloc(2);
    if (rc) return rc;
    std::vector<uint64_t> thr((size_t)nq), sorted;
    for (int q = 0; q < nq; ++q) {  // d < r on non-negative floats is bits(d) < bits(r); key 0 lets nothing pass, ~0 everything
        const float r = radii[q];
        uint32_t bits = 0;
        if (r > 0.0f) memcpy(&bits, &r, sizeof bits);
        thr[(size_t)q] = std::isinf(r) && r > 0.0f ? dpq::kFlatNoKey : (uint64_t)bits << 32;
    }
    DPQ_HIP(hipMemcpy(v->r_thr, thr.data(), (size_t)nq * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (coarse) {
        if ((rc = ivf_probe_on_device(v, v->d_in, nq, nprobe, v->d_probes, v->d_cdists, nullptr))) return rc;
    } else {
        DPQ_HIP(hipMemcpy(v->d_probes, probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    DPQ_HIP(hipMemsetAsync(v->flag, 0, 2 * sizeof(uint32_t), nullptr));
    const dpq::IvfFilter filt = ivf_filter_of(filter);
    const IvfSource src{kIvfQueries, v->d_in};
    size_t scan_bytes = 0;
    DPQ_HIP(dpq::ivf_range_offsets(nullptr, &scan_bytes, v->r_counts, v->r_offs, (int64_t)slots, nullptr));
    DevBuf<uint8_t> scan_temp;
    if ((rc = scan_temp.alloc(scan_bytes))) return rc;
    std::vector<int64_t> tot((size_t)per + 1), qoffs;
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const int64_t n_slots = (int64_t)m * nprobe + 1;
        if ((rc = ivf_slice_tables(v, src, q0, m, nullptr))) return rc;
        DPQ_HIP(dpq::launch_ivf_probes(v->d_probes.get() + (size_t)q0 * nprobe, m, nprobe, v->nlist, v->probes, v->flag, nullptr));
        DPQ_HIP(hipMemsetAsync(v->r_counts.get() + (n_slots - 1), 0, sizeof(int64_t), nullptr));
        DPQ_HIP(dpq::launch_ivf_range(v->lut32, m, v->probes, nprobe, v->offsets, v->ids, v->codes, M, x->plain, filt,
                                      v->r_thr.get() + q0, v->r_counts, nullptr, 0, nullptr, 0, nullptr));
        size_t tb = scan_bytes;
        DPQ_HIP(dpq::ivf_range_offsets(scan_temp, &tb, v->r_counts, v->r_offs, n_slots, nullptr));
        // the queries' list starts: every nprobe-th offset, and the slice's total behind them
        DPQ_HIP(hipMemcpy2D(tot.data(), sizeof(int64_t), v->r_offs, (size_t)nprobe * sizeof(int64_t), sizeof(int64_t),
                            (size_t)m + 1, hipMemcpyDeviceToHost));
        const int64_t at0 = res->lims[(size_t)q0];
        for (int q = 0; q <= m; ++q) {
            if (tot[(size_t)q] < 0 || (q > 0 && tot[(size_t)q] < tot[(size_t)q - 1]))
                return fail(DPQ_ERR_STATE, who + ": internal error: the list offsets do not ascend");
            res->lims[(size_t)q0 + q] = at0 + tot[(size_t)q];
        }
        res->ids.resize((size_t)res->lims[(size_t)q0 + m]);
        res->dists.resize((size_t)res->lims[(size_t)q0 + m]);
        for (int a = 0; a < m;) {
            int b = a + 1;
            while (b < m && tot[(size_t)b + 1] - tot[(size_t)a] <= budget) ++b;
            const int64_t sum = tot[(size_t)b] - tot[(size_t)a];
            if (sum > 0) {
                DevBuf<uint64_t> own_pool, own_sorted;  // one query's list beyond the pool: buffers of this call
                uint64_t *pool = v->r_pool, *spool = v->r_sorted;
                if (sum > budget) {
                    if ((rc = own_pool.alloc((size_t)sum))) return rc;
                    if ((rc = own_sorted.alloc((size_t)sum))) return rc;
                    pool = own_pool;
                    spool = own_sorted;
                }
                qoffs.assign((size_t)(b - a) + 1, 0);
                for (int q = a; q <= b; ++q) qoffs[(size_t)(q - a)] = tot[(size_t)q] - tot[(size_t)a];
                DPQ_HIP(hipMemcpy(v->r_qoffs, qoffs.data(), qoffs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
                DPQ_HIP(dpq::launch_ivf_range(v->lut32.get() + (size_t)a * M * 256, b - a, v->probes.get() + (size_t)a * nprobe, nprobe,
                                              v->offsets, v->ids, v->codes, M, x->plain, filt, v->r_thr.get() + q0 + a, nullptr,
                                              v->r_offs.get() + (size_t)a * nprobe, tot[(size_t)a], pool, sum, nullptr));
                size_t sb = 0;
                DPQ_HIP(dpq::flat_range_sort(nullptr, &sb, pool, spool, sum, b - a, v->r_qoffs, nullptr));
                DevBuf<uint8_t> temp;  // the segmented sort's workspace
                if ((rc = temp.alloc(sb))) return rc;
                DPQ_HIP(dpq::flat_range_sort(temp, &sb, pool, spool, sum, b - a, v->r_qoffs, nullptr));
                sorted.resize((size_t)sum);
                DPQ_HIP(hipMemcpy(sorted.data(), spool, (size_t)sum * sizeof(uint64_t), hipMemcpyDeviceToHost));
                const size_t at = (size_t)(at0 + tot[(size_t)a]);
                for (size_t i = 0; i < (size_t)sum; ++i) {
                    const uint32_t bits = (uint32_t)(sorted[i] >> 32);
                    res->ids[at + i] = (int32_t)(uint32_t)sorted[i];
                    memcpy(&res->dists[at + i], &bits, sizeof bits);
                }
            }
            a = b;
        }
    }
    if ((rc = ivf_read_flags(v, who, kIvfQueries, nullptr))) return rc;
    *out = res.release();
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
    return ivf_search_on_device(v, who, IvfSource{kIvfQueries, d_queries}, nq, d_probes, nprobe, top_k, d_ids, d_dists, (hipStream_t)hip_stream);
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
    if (int rc = ivf_search_on_device(v, who, IvfSource{kIvfQueries, v->d_in}, nq, v->d_probes, nprobe, top_k, v->d_ids, v->d_dists, nullptr)) return rc;
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
    return ivf_search_on_device(v, who, IvfSource{kIvfQueries, d_queries}, nq, v->d_probes, nprobe, top_k, d_ids, d_dists, stream);
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
    if (int rc = ivf_search_on_device(v, who, IvfSource{kIvfQueries, v->d_in}, nq, v->d_probes, nprobe, top_k, v->d_ids, v->d_dists, nullptr)) return rc;
    return ivf_results_down(v, nq, top_k, ids, dists);
    });
}

// ---- filters, caller tables, inner product, range ----

int dpq_ivf_search_filtered(dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, int nprobe, int top_k,
                            int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_filtered", kIvfQueries, true, true, false, filter, queries, nq, nullptr, nprobe,
                               top_k, ids, dists, nullptr, nullptr, nullptr});
    });
}

int dpq_ivf_search_device_filtered(dpq_ivf* v, const dpq_filter* filter, const float* d_queries, int nq, int nprobe, int top_k,
                                   int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_device_filtered", kIvfQueries, true, true, true, filter, d_queries, nq, nullptr,
                               nprobe, top_k, d_ids, d_dists, nullptr, nullptr, (hipStream_t)hip_stream});
    });
}

int dpq_ivf_search_probes_filtered(dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, const int32_t* probes,
                                   int nprobe, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_probes_filtered", kIvfQueries, true, false, false, filter, queries, nq, probes,
                               nprobe, top_k, ids, dists, nullptr, nullptr, nullptr});
    });
}

int dpq_ivf_search_probes_device_filtered(dpq_ivf* v, const dpq_filter* filter, const float* d_queries, int nq,
                                          const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
                                          void* hip_stream) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_probes_device_filtered", kIvfQueries, true, false, true, filter, d_queries, nq,
                               d_probes, nprobe, top_k, d_ids, d_dists, nullptr, nullptr, (hipStream_t)hip_stream});
    });
}

int dpq_ivf_search_probes_tables(dpq_ivf* v, const dpq_filter* filter, const float* tables, int nq, const int32_t* probes,
                                 int nprobe, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_probes_tables", kIvfTables, false, false, false, filter, tables, nq, probes, nprobe,
                               top_k, ids, dists, nullptr, nullptr, nullptr});
    });
}

int dpq_ivf_search_probes_device_tables(dpq_ivf* v, const dpq_filter* filter, const float* d_tables, int nq,
                                        const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
                                        void* hip_stream) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_probes_device_tables", kIvfTables, false, false, true, filter, d_tables, nq,
                               d_probes, nprobe, top_k, d_ids, d_dists, nullptr, nullptr, (hipStream_t)hip_stream});
    });
}

int dpq_ivf_probe_ip(dpq_ivf* v, const float* queries, int nq, int nprobe, int32_t* lists_out, float* scores_out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ivf_probe_ip";
    if (!v || !queries || !lists_out || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (int rc = ivf_enter(who, v, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    if (int rc = ivf_stage(v, queries, nq, nprobe, 0)) return rc;
    if (int rc = ivf_probe_on_device(v, v->d_in, nq, nprobe, v->d_probes, v->d_cdists, nullptr, dpq::kFlatIP)) return rc;
    DPQ_HIP(hipMemcpy(lists_out, v->d_probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (scores_out) DPQ_HIP(hipMemcpy(scores_out, v->d_cdists, (size_t)nq * nprobe * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_ivf_search_ip(dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, int nprobe, int top_k, int32_t* ids,
                      float* scores, float* gaps_out, float* bias_out) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_ip", kIvfIp, false, true, false, filter, queries, nq, nullptr, nprobe, top_k, ids,
                               scores, gaps_out, bias_out, nullptr});
    });
}

int dpq_ivf_search_device_ip(dpq_ivf* v, const dpq_filter* filter, const float* d_queries, int nq, int nprobe, int top_k,
                             int32_t* d_ids, float* d_scores, float* d_gaps, float* d_bias, void* hip_stream) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_device_ip", kIvfIp, false, true, true, filter, d_queries, nq, nullptr, nprobe, top_k,
                               d_ids, d_scores, d_gaps, d_bias, (hipStream_t)hip_stream});
    });
}

int dpq_ivf_search_probes_ip(dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, const int32_t* probes,
                             int nprobe, int top_k, int32_t* ids, float* scores, float* gaps_out, float* bias_out) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_probes_ip", kIvfIp, false, false, false, filter, queries, nq, probes, nprobe, top_k,
                               ids, scores, gaps_out, bias_out, nullptr});
    });
}

int dpq_ivf_search_probes_device_ip(dpq_ivf* v, const dpq_filter* filter, const float* d_queries, int nq,
                                    const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_scores,
                                    float* d_gaps, float* d_bias, void* hip_stream) {
    return guarded([&]() -> int {
    return ivf_call(v, IvfCall{"dpq_ivf_search_probes_device_ip", kIvfIp, false, false, true, filter, d_queries, nq, d_probes,
                               nprobe, top_k, d_ids, d_scores, d_gaps, d_bias, (hipStream_t)hip_stream});
    });
}

int dpq_ivf_range_search(dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, int nprobe, const float* radii,
                         dpq_range_result** out) {
    return guarded([&]() -> int {
    return ivf_range_call("dpq_ivf_range_search", v, filter, queries, nq, nullptr, true, nprobe, radii, out);
    });
}

int dpq_ivf_range_search_probes(dpq_ivf* v, const dpq_filter* filter, const float* queries, int nq, const int32_t* probes,
                                int nprobe, const float* radii, dpq_range_result** out) {
    return guarded([&]() -> int {
    return ivf_range_call("dpq_ivf_range_search_probes", v, filter, queries, nq, probes, false, nprobe, radii, out);
    });
}

}  // extern "C"
