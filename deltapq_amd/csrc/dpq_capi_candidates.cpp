// dpq_capi_candidates.cpp -- the candidate search entry points of include/deltapq_amd.h (kernels in dpq_candidates.hip):
// PQ distances, and the best top_k, over each query's own list of ids.
#include "dpq_capi_internal.h"

namespace {

// One call behind its checks, all device pointers.  top_k == 0: the distance form (d_ids unused, d_dists [nq][n_cand]).
struct CandCall {
    const char* fn;
    const float* d_in;  // queries [nq][M * Ds], or tables [nq][M][K]
    bool tables;
    int nq;
    const int32_t* d_cand;
    int n_cand, top_k;
    int32_t* d_ids;
    float* d_dists;
    hipStream_t stream;
};

dpq::RefineIds cand_ids_of(const dpq_index* x) {
    dpq::RefineIds r{};
    r.id_base = (int64_t)x->img.id_base;
    r.n_local = x->img.n_local;
    r.n_total = x->img.n_codes_total;
    r.even_rule = x->plain ? 0 : 1;
    return r;
}

// Slices of at most 2^20 candidates and 2048 queries: per slice the tables of its queries, the id pre-pass, the code
// lookup, the distances, the sort.  Ends with the two flag words read back.
int cand_on_device(dpq_index* x, const CandCall& c) {
    CandWs& w = x->cand;
    const int M = x->M, K = x->K;
    const bool emit = c.top_k > 0;
    const size_t n_pad = dpq::cand_keys(c.n_cand);
    const int per = std::max(1, std::min(std::min(c.nq, dpq::kCandSliceQueries), dpq::kCandSlice / c.n_cand));
    int rc = grow(w.lut32, &w.lut_n, (size_t)per * M * 256);
    if (!rc) rc = grow(w.lut_min, &w.min_n, (size_t)per * M * dpq::kLutMinParts);
    if (!rc) rc = grow(w.local, &w.local_n, (size_t)per * c.n_cand);
    if (!rc) rc = grow(w.codes, &w.codes_n, (size_t)per * c.n_cand * M);
    if (!rc && emit) rc = grow(w.keys, &w.keys_n, (size_t)per * n_pad);
    if (!rc && !w.flag.get()) rc = w.flag.alloc(2);
    if (rc) return rc;
    DPQ_HIP(hipMemsetAsync(w.flag, 0, 2 * sizeof(uint32_t), c.stream));
    const dpq::RefineIds rid = cand_ids_of(x);
    const size_t in_stride = c.tables ? (size_t)M * K : (size_t)M * x->Ds;
    for (int q0 = 0; q0 < c.nq; q0 += per) {
        const int m = std::min(per, c.nq - q0);
        const float* in = c.d_in + (size_t)q0 * in_stride;
        const int32_t* cand = c.d_cand + (size_t)q0 * c.n_cand;
        if (c.tables)
            DPQ_HIP(dpq::launch_tables_ingest(in, m, m, M, K, w.lut32, w.lut_min, nullptr, nullptr, nullptr, nullptr,
                                              w.flag.get() + 1, c.stream));
        else
            DPQ_HIP(dpq::launch_lut_build(x->d_codebook, in, m, m, M, K, x->Ds, w.lut32, w.lut_min, nullptr, nullptr, nullptr,
                                          nullptr, nullptr, c.stream));
        DPQ_HIP(dpq::launch_cand_classify(cand, (int64_t)m * c.n_cand, rid, w.local, w.flag, c.stream));
        // (the pre-pass has taken out every id the lookup would refuse)
        if ((rc = lookup_on_device(x, w.local, (int64_t)m * c.n_cand, w.codes, nullptr, c.stream, c.fn))) return rc;
        DPQ_HIP(dpq::launch_cand_adc(w.lut32, m, w.local, c.n_cand, w.codes, M, x->plain, emit ? w.keys.get() : nullptr,
                                     emit ? nullptr : c.d_dists + (size_t)q0 * c.n_cand, c.stream));
        if (emit)
            DPQ_HIP(dpq::launch_flat_sort_emit(w.keys, n_pad, nullptr, m, c.n_cand, c.top_k, c.d_ids + (size_t)q0 * c.top_k,
                                               c.d_dists + (size_t)q0 * c.top_k, c.stream));
    }
    uint32_t bad[2] = {0, 0};
    DPQ_HIP(hipMemcpyAsync(bad, w.flag, sizeof bad, hipMemcpyDeviceToHost, c.stream));
    DPQ_HIP(hipStreamSynchronize(c.stream));
    if (bad[0]) return fail(DPQ_ERR_ARG, std::string(c.fn) + ": a candidate names no node of the index");
    if (bad[1])
        return fail(DPQ_ERR_ARG, std::string(c.fn) + ": a table entry is negative or a NaN; the outputs are unspecified");
    return DPQ_OK;
}

// The checks that need neither the handle's fields nor a device.  top_k == 0 with ids == NULL: the distance form.
int cand_args(const std::string& who, const void* x, const void* in, int nq, const void* cand, int n_cand, bool search,
              int top_k, const void* ids, const void* dists) {
    if (!x || !in || !cand || !dists || (search && !ids) || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (search && (top_k < 1 || top_k > n_cand || n_cand > dpq::kCandMaxCand))
        return fail(DPQ_ERR_ARG, who + ": needs 1 <= top_k <= n_cand <= 16384");
    if (!search && (n_cand < 1 || n_cand > dpq::kCandMaxCand)) return fail(DPQ_ERR_ARG, who + ": needs 1 <= n_cand <= 16384");
    return DPQ_OK;
}

// A device, a handle the code lookup decodes, a codebook for the query forms; settles what is in flight.
int cand_enter(const std::string& who, dpq_index* x, bool tables) {
    if (int rc = flat_device_present(who)) return rc;
    if (x->M != 8 && x->M != 16) return fail(DPQ_ERR_ARG, who + ": needs a handle of M = 8 or M = 16");
    if (!tables && !x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    return DPQ_OK;
}

int cand_device_form(const char* fn, dpq_index* x, const float* d_in, bool tables, int nq, const int32_t* d_cand, int n_cand,
                     bool search, int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    const std::string who = fn;
    if (int rc = cand_args(who, x, d_in, nq, d_cand, n_cand, search, top_k, d_ids, d_dists)) return rc;
    if (int rc = cand_enter(who, x, tables)) return rc;
    if (nq == 0) return DPQ_OK;
    return cand_on_device(x, CandCall{fn, d_in, tables, nq, d_cand, n_cand, search ? top_k : 0, d_ids, d_dists,
                                      (hipStream_t)hip_stream});
}

// Host buffers: every candidate, and every table entry, is checked before any device work; then up, the device form's
// body on the default stream, down.
int cand_host_form(const char* fn, dpq_index* x, const float* in, bool tables, int nq, const int32_t* cand, int n_cand,
                   bool search, int top_k, int32_t* ids, float* dists) {
    const std::string who = fn;
    if (int rc = cand_args(who, x, in, nq, cand, n_cand, search, top_k, ids, dists)) return rc;
    if (int rc = cand_enter(who, x, tables)) return rc;
    if (nq == 0) return DPQ_OK;
    const dpq::RefineIds rid = cand_ids_of(x);
    const size_t n_in = (size_t)nq * x->M * (tables ? x->K : x->Ds), n_c = (size_t)nq * n_cand;
    const size_t n_out = search ? (size_t)nq * top_k : n_c;
    for (size_t i = 0; i < n_c; ++i)
        if (dpq::cand_classify(cand[i], rid) == dpq::kCandNone) {
            char msg[96];
            snprintf(msg, sizeof msg, ": entry %lld = %d names no node of the index", (long long)i, (int)cand[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    if (tables)
        for (size_t i = 0; i < n_in; ++i)
            if (!(in[i] >= 0.0f)) return fail(DPQ_ERR_ARG, who + ": table entry " + std::to_string(i) + " is negative or a NaN");
    CandWs& w = x->cand;
    int rc = grow(w.d_in, &w.in_n, n_in);
    if (!rc) rc = grow(w.d_cand, &w.cand_n, n_c);
    if (!rc) rc = grow(w.d_dists, &w.dists_n, n_out);
    if (!rc && search) rc = grow(w.d_ids, &w.ids_n, n_out);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(w.d_in, in, n_in * sizeof(float), hipMemcpyHostToDevice));
    DPQ_HIP(hipMemcpy(w.d_cand, cand, n_c * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = cand_on_device(x, CandCall{fn, w.d_in, tables, nq, w.d_cand, n_cand, search ? top_k : 0, w.d_ids, w.d_dists, nullptr});
    if (rc) return rc;
    if (search) DPQ_HIP(hipMemcpy(ids, w.d_ids, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, w.d_dists, n_out * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_candidate_search(dpq_index* x, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                         int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return cand_host_form("dpq_candidate_search", x, queries, false, nq, cand_ids, n_cand, true, top_k, ids, dists);
    });
}

int dpq_candidate_search_device(dpq_index* x, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand, int top_k,
                                int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return cand_device_form("dpq_candidate_search_device", x, d_queries, false, nq, d_cand_ids, n_cand, true, top_k, d_ids,
                            d_dists, hip_stream);
    });
}

int dpq_candidate_search_tables(dpq_index* x, const float* tables, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                                int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return cand_host_form("dpq_candidate_search_tables", x, tables, true, nq, cand_ids, n_cand, true, top_k, ids, dists);
    });
}

int dpq_candidate_search_device_tables(dpq_index* x, const float* d_tables, int nq, const int32_t* d_cand_ids, int n_cand,
                                       int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return cand_device_form("dpq_candidate_search_device_tables", x, d_tables, true, nq, d_cand_ids, n_cand, true, top_k, d_ids,
                            d_dists, hip_stream);
    });
}

int dpq_candidate_distances(dpq_index* x, const float* queries, int nq, const int32_t* cand_ids, int n_cand, float* dists) {
    return guarded([&]() -> int {
    return cand_host_form("dpq_candidate_distances", x, queries, false, nq, cand_ids, n_cand, false, 0, nullptr, dists);
    });
}

int dpq_candidate_distances_device(dpq_index* x, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                   float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return cand_device_form("dpq_candidate_distances_device", x, d_queries, false, nq, d_cand_ids, n_cand, false, 0, nullptr,
                            d_dists, hip_stream);
    });
}

}  // extern "C"
