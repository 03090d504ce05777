// dpq_capi_tables.cpp -- search by caller-supplied distance tables, and the inner-product search built on it
// (include/deltapq_amd.h "Search by distance tables"; kernels in dpq_tables.hip).  The batches themselves are
// run_batch / range_batch of dpq_capi.cpp with a TableSource that names tables instead of queries.
#include "dpq_capi_internal.h"

namespace {

// What the table forms check of a top-k call: everything check_batch_args does but the codebook.
int check_tables_args(const std::string& who, const dpq_index* x, const void* in, int nq, int top_k, const void* ids,
                      const void* dists) {
    if (!x || !in || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (top_k < 1 || top_k > dpq::kMaxTopK) return fail(DPQ_ERR_ARG, who + ": top_k must be in 1..2048");
    if ((int64_t)top_k > x->img.n_codes_total)
        return fail(DPQ_ERR_TOPK, who + ": top_k exceeds the number of codes in the index");
    return DPQ_OK;
}

// An entry is a distance: finite and >= 0 (-0.0 included: it is read as +0.0), or +inf.
int check_entries(const std::string& who, const float* tables, size_t per_query, int nq) {
    for (int q = 0; q < nq; ++q)
        for (size_t i = 0; i < per_query; ++i)
            if (!(tables[(size_t)q * per_query + i] >= 0.0f))
                return fail(DPQ_ERR_ARG, who + ": entry " + std::to_string(i) + " of query " + std::to_string(q) +
                                             " is negative or a NaN");
    return DPQ_OK;
}

int finish_pending(dpq_index* x) { return x->pending.empty() ? DPQ_OK : dpq_finish(x); }

// The word tables_ingest_kernel raises, cleared: the batches before this call are finished, nothing else writes it.
int arm_bad_word(dpq_index* x) {
    if (!x->h_tables_bad) {
        DPQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&x->h_tables_bad), sizeof(uint32_t), hipHostMallocMapped));
        DPQ_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&x->d_tables_bad), x->h_tables_bad, 0));
    }
    *x->h_tables_bad = 0;
    return DPQ_OK;
}

// The call's closing synchronisation, and the word with it.
int read_bad_word(const std::string& who, dpq_index* x, hipStream_t stream, const char* what) {
    DPQ_HIP(hipStreamSynchronize(stream));
    if (*reinterpret_cast<volatile uint32_t*>(x->h_tables_bad) != 0) return fail(DPQ_ERR_ARG, who + ": " + what);
    return DPQ_OK;
}

constexpr const char* kBadEntry = "a table entry is negative or a NaN; the outputs are unspecified";
constexpr const char* kBadDot = "a query or codeword is not finite (or a dot product is not); the outputs are unspecified";

int stage_tables(dpq_index* x, int nq) {
    return grow(x->d_tab_stage, &x->tab_stage_n, (size_t)std::min(nq, kMaxBatchQueries) * x->M * x->K);
}

// dpq_query_batch_device_ip behind its checks; also the body of the host form (on its staging buffers).  One sub-batch
// at a time: its tables into the handle's buffer, the table search over them (synchronous, so the buffer is free
// again), then every score at once.
int ip_search(const std::string& who, dpq_index* x, const dpq_filter* filt, const float* d_queries, int nq, int top_k,
              int32_t* d_ids, float* d_scores, float* d_gaps, float* d_bias, hipStream_t stream) {
    int rc;
    if ((rc = finish_pending(x))) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    if ((rc = stage_tables(x, nq))) return rc;
    if (!d_bias) {
        if ((rc = grow(x->d_ip_bias, &x->ip_bias_n, (size_t)nq))) return rc;
        d_bias = x->d_ip_bias;
    }
    if (!d_gaps) {
        if ((rc = grow(x->d_ip_gaps, &x->ip_gaps_n, (size_t)nq * top_k))) return rc;
        d_gaps = x->d_ip_gaps;
    }
    if ((rc = arm_bad_word(x))) return rc;
    const size_t D = (size_t)x->M * x->Ds;
    for (int base = 0; base < nq; base += kMaxBatchQueries) {
        const int n = std::min(kMaxBatchQueries, nq - base);
        DPQ_HIP(dpq::launch_ip_tables(x->d_codebook, d_queries + (size_t)base * D, n, x->M, x->K, x->Ds, x->d_tab_stage,
                                      d_bias + base, stream));
        TableSource src;
        src.d_tables = x->d_tab_stage;
        src.d_bad = x->d_tables_bad;
        if ((rc = query_device_src(x, filt, src, n, top_k, d_ids + (size_t)base * top_k, d_gaps + (size_t)base * top_k, stream)))
            return rc;
    }
    DPQ_HIP(dpq::launch_ip_scores(d_bias, d_gaps, d_ids, nq, top_k, d_scores, stream));
    return read_bad_word(who, x, stream, kBadDot);
}

int check_ip_args(const std::string& who, const dpq_index* x, const dpq_filter* filter, const float* queries, int nq,
                  int top_k, const int32_t* ids, const float* scores) {
    int rc = check_tables_args(who, x, queries, nq, top_k, ids, scores);
    if (rc) return rc;
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    return filter ? check_filter(x, filter) : DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_query_batch_device_tables(dpq_index* x, const dpq_filter* filter, const float* d_tables, int nq, int top_k,
                                  int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_query_batch_device_tables";
    int rc = check_tables_args(who, x, d_tables, nq, top_k, d_ids, d_dists);
    if (rc || nq == 0) return rc;
    if (filter && (rc = check_filter(x, filter))) return rc;
    if ((rc = finish_pending(x))) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    if ((rc = arm_bad_word(x))) return rc;
    TableSource src;
    src.d_tables = d_tables;
    src.d_bad = x->d_tables_bad;
    if ((rc = query_device_src(x, filter, src, nq, top_k, d_ids, d_dists, hip_stream))) return rc;
    return read_bad_word(who, x, (hipStream_t)hip_stream, kBadEntry);
    });
}

int dpq_query_batch_tables(dpq_index* x, const dpq_filter* filter, const float* tables, int nq, int top_k, int32_t* ids,
                           float* dists) {
    return guarded([&]() -> int {
    const std::string who = "dpq_query_batch_tables";
    int rc = check_tables_args(who, x, tables, nq, top_k, ids, dists);
    if (rc || nq == 0) return rc;
    if ((rc = check_entries(who, tables, (size_t)x->M * x->K, nq))) return rc;
    if (filter && (rc = check_filter(x, filter))) return rc;
    if ((rc = finish_pending(x))) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    const size_t oe = (size_t)nq * top_k;
    if ((rc = stage_tables(x, nq))) return rc;
    if ((rc = ensure_out_stage(x, oe))) return rc;
    if ((rc = arm_bad_word(x))) return rc;
    TableSource src;
    src.h_tables = tables;
    src.d_bad = x->d_tables_bad;
    if ((rc = query_device_src(x, filter, src, nq, top_k, x->d_ids_stage, x->d_dists_stage, nullptr))) return rc;
    DPQ_HIP(hipDeviceSynchronize());
    DPQ_HIP(hipMemcpy(ids, x->d_ids_stage, oe * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, x->d_dists_stage, oe * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_range_search_tables(dpq_index* x, const float* tables, int nq, const float* radii, dpq_range_result** out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_range_search_tables";
    if (!out) return fail(DPQ_ERR_ARG, who + ": out is NULL");
    *out = nullptr;
    if (!x || nq < 0 || (nq > 0 && (!tables || !radii))) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    for (int q = 0; q < nq; ++q)
        if (std::isnan(radii[q])) return fail(DPQ_ERR_ARG, who + ": radius of query " + std::to_string(q) + " is NaN");
    int rc;
    if ((rc = check_entries(who, tables, (size_t)x->M * x->K, nq))) return rc;
    if ((rc = finish_pending(x))) return rc;
    TableSource src;
    if (nq > 0) {
        DPQ_HIP(hipSetDevice(x->device));
        if ((rc = stage_tables(x, nq))) return rc;
        if ((rc = arm_bad_word(x))) return rc;
        src.h_tables = tables;
        src.d_bad = x->d_tables_bad;
    }
    return range_search_src(x, src, nq, radii, out);
    });
}

int dpq_ip_tables_device(dpq_index* x, const float* d_queries, int nq, float* d_tables, float* d_bias, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ip_tables_device";
    if (!x || !d_queries || !d_tables || !d_bias || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (nq == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(x->device));
    DPQ_HIP(dpq::launch_ip_tables(x->d_codebook, d_queries, nq, x->M, x->K, x->Ds, d_tables, d_bias, (hipStream_t)hip_stream));
    return DPQ_OK;
    });
}

int dpq_ip_tables(dpq_index* x, const float* queries, int nq, float* tables_out, float* bias_out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_ip_tables";
    if (!x || !queries || !tables_out || !bias_out || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (nq == 0) return DPQ_OK;
    int rc;
    if ((rc = finish_pending(x))) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    const size_t D = (size_t)x->M * x->Ds, T = (size_t)x->M * x->K;
    if ((rc = grow(x->d_q_stage, &x->q_stage_floats, (size_t)nq * D))) return rc;
    if ((rc = stage_tables(x, nq))) return rc;
    if ((rc = grow(x->d_ip_bias, &x->ip_bias_n, (size_t)nq))) return rc;
    DPQ_HIP(hipMemcpy(x->d_q_stage, queries, (size_t)nq * D * sizeof(float), hipMemcpyHostToDevice));
    for (int base = 0; base < nq; base += kMaxBatchQueries) {
        const int n = std::min(kMaxBatchQueries, nq - base);
        DPQ_HIP(dpq::launch_ip_tables(x->d_codebook, x->d_q_stage + (size_t)base * D, n, x->M, x->K, x->Ds, x->d_tab_stage,
                                      x->d_ip_bias + base, nullptr));
        DPQ_HIP(hipMemcpy(tables_out + (size_t)base * T, x->d_tab_stage, (size_t)n * T * sizeof(float), hipMemcpyDeviceToHost));
    }
    DPQ_HIP(hipMemcpy(bias_out, x->d_ip_bias, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_query_batch_device_ip(dpq_index* x, const dpq_filter* filter, const float* d_queries, int nq, int top_k,
                              int32_t* d_ids, float* d_scores, float* d_gaps, float* d_bias, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_query_batch_device_ip";
    int rc = check_ip_args(who, x, filter, d_queries, nq, top_k, d_ids, d_scores);
    if (rc || nq == 0) return rc;
    return ip_search(who, x, filter, d_queries, nq, top_k, d_ids, d_scores, d_gaps, d_bias, (hipStream_t)hip_stream);
    });
}

int dpq_query_batch_ip(dpq_index* x, const dpq_filter* filter, const float* queries, int nq, int top_k, int32_t* ids,
                       float* scores, float* gaps_out, float* bias_out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_query_batch_ip";
    int rc = check_ip_args(who, x, filter, queries, nq, top_k, ids, scores);
    if (rc || nq == 0) return rc;
    if ((rc = finish_pending(x))) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    const size_t qf = (size_t)nq * x->M * x->Ds, oe = (size_t)nq * top_k;
    if ((rc = grow(x->d_q_stage, &x->q_stage_floats, qf))) return rc;
    if ((rc = ensure_out_stage(x, oe))) return rc;
    if ((rc = grow(x->d_ip_bias, &x->ip_bias_n, (size_t)nq))) return rc;
    if ((rc = grow(x->d_ip_gaps, &x->ip_gaps_n, oe))) return rc;
    DPQ_HIP(hipMemcpy(x->d_q_stage, queries, qf * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = ip_search(who, x, filter, x->d_q_stage, nq, top_k, x->d_ids_stage, x->d_dists_stage, x->d_ip_gaps, x->d_ip_bias,
                        nullptr)))
        return rc;
    DPQ_HIP(hipMemcpy(ids, x->d_ids_stage, oe * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(scores, x->d_dists_stage, oe * sizeof(float), hipMemcpyDeviceToHost));
    if (gaps_out) DPQ_HIP(hipMemcpy(gaps_out, x->d_ip_gaps, oe * sizeof(float), hipMemcpyDeviceToHost));
    if (bias_out) DPQ_HIP(hipMemcpy(bias_out, x->d_ip_bias, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_ip_scores(const float* bias, const float* gaps, const int32_t* ids, int nq, int top_k, float* scores_out) {
    return guarded([&]() -> int {
    if (!bias || !gaps || !ids || !scores_out || nq < 0 || top_k < 1)
        return fail(DPQ_ERR_ARG, "dpq_ip_scores: NULL argument, nq < 0 or top_k < 1");
    for (int q = 0; q < nq; ++q)
        for (int j = 0; j < top_k; ++j) {
            const size_t i = (size_t)q * top_k + j;
            scores_out[i] = ids[i] < 0 ? -INFINITY : (float)((double)bias[q] - (double)gaps[i]);
        }
    return DPQ_OK;
    });
}

}  // extern "C"
