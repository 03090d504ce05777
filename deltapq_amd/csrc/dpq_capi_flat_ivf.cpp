// dpq_capi_flat_ivf.cpp -- the dpq_flat_ivf_* entry points of include/deltapq_amd.h (kernels in dpq_flat_ivf.hip,
// dpq_flat_ivf_narrow.hip, dpq_flat_ivf_u8.hip and dpq_flat_ivf_bits.hip): inverted lists over the rows of an fp32 (or half, or
// scalar-quantised: the formats that take fp32 queries, one kind), a byte or a binary dpq_flat handle,
// built on the device from labels or from centroids, and the search that forms exact distances to the rows of the lists a
// query probes.  The fp32 entry points, the *_bytes and the *_bits ones run the same code; `kind` (kFivfF32, kFivfBytes,
// kFivfBits) says which kind of handle, of queries and of centroids a call is about.
#include "dpq_capi_internal.h"
#include "dpq_ivf_train.h"

namespace {

int fivf_nlist_ok(const std::string& who, int nlist) {
    if (nlist < 1 || nlist > dpq::kIvfMaxLists) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nlist <= 65536");
    return DPQ_OK;
}

// A handle of the call's kind on a present device.  (The launchers that make the lists take at most 2^31 - 1 rows.)
int fivf_enter_flat(const std::string& who, dpq_flat* f, int kind) {
    if (kind == kFivfBits && f->format != dpq::kFlatBits)
        return fail(DPQ_ERR_ARG, who + ": needs a handle of binary rows (dpq_flat_open_bits / dpq_flat_open_binarised)");
    if (kind == kFivfBytes && f->format != dpq::kFlatU8 && f->format != dpq::kFlatI8)
        return fail(DPQ_ERR_ARG, who + ": needs a handle of byte rows (dpq_flat_open_u8 / dpq_flat_open_i8)");
    if (kind == kFivfF32 && dpq::flat_query_format(f->format) != dpq::kFlatF32)
        return fail(DPQ_ERR_ARG, who + ": needs a handle that takes fp32 queries (fp32, half or scalar-quantised rows); byte handles have the *_bytes calls, binary handles the *_bits calls");
    if (f->map.get()) return fail(DPQ_ERR_ARG, who + ": a handle with an id map (dpq_flat_set_id_map) is not supported");
    if (f->n > 0x7fffffff) return fail(DPQ_ERR_ARG, who + ": the handle has too many rows");
    if (int rc = flat_device_present(who)) return rc;
    DPQ_HIP(hipSetDevice(f->device));
    return DPQ_OK;
}

// The lists of d_labels[n] (n = the handle's rows), all on `stream`; *out is a structure without centroids.
int fivf_from_device_labels(const std::string& who, dpq_flat* f, const int32_t* d_labels, int64_t n, int nlist,
                            hipStream_t stream, std::unique_ptr<dpq_flat_ivf>* out) {
    if (n != f->n) return fail(DPQ_ERR_ARG, who + ": n must be the handle's row count");
    std::unique_ptr<dpq_flat_ivf> v(new dpq_flat_ivf());
    v->flat = f;
    v->kind = f->format == dpq::kFlatBits ? kFivfBits : f->format == dpq::kFlatU8 || f->format == dpq::kFlatI8 ? kFivfBytes : kFivfF32;
    v->device = f->device;
    v->nlist = nlist;
    DevBuf<uint32_t> keys, pos, keys_out, flag;
    DevBuf<unsigned long long> counts;
    DevBuf<uint8_t> temp;
    int rc = keys.alloc((size_t)n);
    if (!rc) rc = pos.alloc((size_t)n);
    if (!rc) rc = keys_out.alloc((size_t)n);
    if (!rc) rc = v->rows.alloc((size_t)n);  // the sorted positions ARE the lists: rows [0, n_assigned), then the unassigned
    if (!rc) rc = counts.alloc((size_t)nlist + 1);
    if (!rc) rc = flag.alloc(1);
    if (!rc) rc = v->offsets.alloc((size_t)nlist + 1);
    if (rc) return rc;
    DPQ_HIP(hipMemsetAsync(counts, 0, ((size_t)nlist + 1) * sizeof(unsigned long long), stream));
    DPQ_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), stream));
    DPQ_HIP(dpq::launch_ivf_label_keys(d_labels, n, nlist, keys, pos, counts, flag, stream));
    size_t temp_bytes = 0;
    DPQ_HIP(dpq::ivf_scan_and_sort(nullptr, &temp_bytes, counts, v->offsets, nlist, keys, keys_out, pos, v->rows, n, stream));
    if ((rc = temp.alloc(temp_bytes))) return rc;
    DPQ_HIP(dpq::ivf_scan_and_sort(temp, &temp_bytes, counts, v->offsets, nlist, keys, keys_out, pos, v->rows, n, stream));
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
    v->device_bytes = ((int64_t)nlist + 1) * 8 + n * 4;
    *out = std::move(v);
    return DPQ_OK;
}

// centroids[nlist][D] in host memory -> the device, padded with zeros to the handle's Dp.
int fivf_upload_centroids(const dpq_flat* f, const float* centroids, int nlist, DevBuf<float>* d_out) {
    const int D = f->D, Dp = f->Dp;
    if (int rc = d_out->alloc((size_t)nlist * Dp)) return rc;
    if (D == Dp) {
        DPQ_HIP(hipMemcpy(d_out->get(), centroids, (size_t)nlist * D * sizeof(float), hipMemcpyHostToDevice));
        return DPQ_OK;
    }
    std::vector<float> padded((size_t)nlist * Dp, 0.0f);
    for (int l = 0; l < nlist; ++l) memcpy(&padded[(size_t)l * Dp], centroids + (size_t)l * D, (size_t)D * sizeof(float));
    DPQ_HIP(hipMemcpy(d_out->get(), padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
    return DPQ_OK;
}

void fivf_keep_centroids(dpq_flat_ivf* v, DevBuf<float>&& d_cent) {
    const int64_t bytes = (int64_t)v->nlist * v->flat->Dp * 4;
    if (v->centroids.get()) v->device_bytes -= bytes;
    v->centroids = std::move(d_cent);
    v->device_bytes += bytes;
}

int fivf_search_args(const std::string& who, const void* ivf, const void* queries, int nq, bool with_probes, const void* probes,
                     int nprobe, int top_k, const void* ids, const void* dists) {
    if (!ivf || !queries || (with_probes && !probes) || !ids || !dists || nq < 0)
        return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (top_k < 1 || top_k > dpq::kIvfMaxTopK) return fail(DPQ_ERR_ARG, who + ": needs 1 <= top_k <= 2048");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    return DPQ_OK;
}

// A call of one kind on a structure of another names the structure's own set.
int fivf_kind_ok(const std::string& who, const dpq_flat_ivf* v, int kind) {
    if (v->kind == kind) return DPQ_OK;
    static const char* const sets[] = {": the structure is over fp32 rows: its calls are the ones without _bytes or _bits",
                                       ": the structure is over byte rows: its calls are the *_bytes ones",
                                       ": the structure is over binary rows: its calls are the *_bits ones"};
    return fail(DPQ_ERR_ARG, who + sets[v->kind]);
}

// A filter of the *_filtered calls (NULL: none) was made for the structure's own handle, which puts it on its device:
// dpq_flat_search_filtered's checks.
int fivf_filter_ok(const std::string& who, const dpq_flat_ivf* v, const dpq_flat_filter* ff) {
    if (!ff) return DPQ_OK;
    if (ff->owner != v->flat->serial) return fail(DPQ_ERR_ARG, who + ": the filter was made for another handle");
    if (ff->device != v->device)  // defensive: a filter of the structure's handle lives on the handle's device
        return fail(DPQ_ERR_ARG, who + ": the filter is on another device");
    return DPQ_OK;
}

// What needs the structure's fields; then a device.
int fivf_enter(const std::string& who, dpq_flat_ivf* v, int kind, int nprobe, bool coarse) {
    if (int rc = fivf_kind_ok(who, v, kind)) return rc;
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (coarse && !(kind == kFivfBits ? (const void*)v->bcent.get() : (const void*)v->centroids.get()))
        return fail(DPQ_ERR_STATE, who + (kind == kFivfBits
                                              ? ": the structure has no centroids (dpq_flat_ivf_build_bits / dpq_flat_ivf_set_centroids_bits)"
                                              : ": the structure has no centroids (dpq_flat_ivf_build / dpq_flat_ivf_set_centroids)"));
    if (int rc = flat_device_present(who)) return rc;
    DPQ_HIP(hipSetDevice(v->device));
    return DPQ_OK;
}

int fivf_probe_rows_ok(const std::string& who, const dpq_flat_ivf* v, const int32_t* probes, int nq, int nprobe) {
    for (size_t i = 0; i < (size_t)nq * nprobe; ++i)
        if (probes[i] >= v->nlist) {
            char msg[96];
            snprintf(msg, sizeof msg, ": entry %lld = %d names no list", (long long)i, (int)probes[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    return DPQ_OK;
}

// A call's queries as the kernels read them.  f32 [nq][Dp] with zero padding: what the coarse step ranks the centroids by,
// and what the fp32 scan reads.  A byte structure: i8 [nq][Dp] and norm [nq], the queries as the handle stores rows.
// A binary structure: bits [nq][Dp] bytes, the queries as the handle stores rows, for the coarse step and the scan alike.
struct FivfQueries {
    const float* f32 = nullptr;
    const int8_t* i8 = nullptr;
    const int32_t* norm = nullptr;
    const uint8_t* bits = nullptr;
};

// Packed binary queries [nq][(D + 7) / 8] in the caller's layout: prepared as dpq_flat_search_bits prepares them
// (launch_flat_bits_prepare over the batch).  Host form: through v->q_raw.  The buffer has room for 64 more queries: the
// Hamming kernel of the coarse step reads whole query tiles and masks what lies past nq.
int fivf_queries_bits(dpq_flat_ivf* v, const void* queries, int nq, bool device, hipStream_t stream, FivfQueries* out) {
    const int D = v->flat->D, Dp = v->flat->Dp;
    const size_t nb = (size_t)dpq::flat_bits_bytes(D);
    const uint8_t* raw = static_cast<const uint8_t*>(queries);
    int rc = grow(v->q8, &v->q8_n, ((size_t)nq + 64) * Dp);
    if (!rc && !device) rc = grow(v->q_raw, &v->q_raw_n, (size_t)nq * nb);
    if (rc) return rc;
    if (!device) {
        DPQ_HIP(hipMemcpy(v->q_raw, queries, (size_t)nq * nb, hipMemcpyHostToDevice));
        raw = v->q_raw;
    }
    uint8_t* q = reinterpret_cast<uint8_t*>(v->q8.get());
    DPQ_HIP(dpq::launch_flat_bits_prepare(raw, nq, D, q, Dp, stream));
    out->bits = q;
    return DPQ_OK;
}

// Byte queries [nq][D] of the handle's kind: prepared as the rows are (launch_flat_u8_prepare over the batch) and, for a
// call with a coarse step, widened exactly to fp32 -- the caller's values, not the biased storage.  Host form: through
// v->q_raw.
// metric kFlatIP: out->norm is, in the place of the norms, the queries' terms qs of the unsigned inner product
// (launch_flat_u8_sums, add = 0), or NULL on a signed handle, whose score is the int8 dot product alone.
int fivf_queries_bytes(dpq_flat_ivf* v, const void* queries, int nq, bool device, bool coarse, hipStream_t stream,
                       FivfQueries* out, int metric) {
    const int D = v->flat->D, Dp = v->flat->Dp;
    const bool is_signed = v->flat->format == dpq::kFlatI8;
    const uint8_t* raw = static_cast<const uint8_t*>(queries);
    int rc = grow(v->q8, &v->q8_n, (size_t)nq * Dp);
    if (!rc) rc = grow(v->qnorm, &v->qnorm_n, (size_t)nq);
    if (!rc && !device) rc = grow(v->q_raw, &v->q_raw_n, (size_t)nq * D);
    if (!rc && coarse) rc = grow(v->d_q, &v->q_n, (size_t)nq * Dp);
    if (rc) return rc;
    if (!device) {
        DPQ_HIP(hipMemcpy(v->q_raw, queries, (size_t)nq * D, hipMemcpyHostToDevice));
        raw = v->q_raw;
    }
    DPQ_HIP(dpq::launch_flat_u8_prepare(raw, nq, D, Dp, v->q8, v->qnorm, stream, is_signed));
    if (coarse) {
        DPQ_HIP(dpq::launch_flat_ivf_widen(raw, nq, D, D, Dp, false, is_signed, v->d_q, stream));
        out->f32 = v->d_q;
    }
    out->i8 = v->q8;
    out->norm = v->qnorm;
    if (metric == dpq::kFlatIP) {
        if (is_signed) out->norm = nullptr;
        else DPQ_HIP(dpq::launch_flat_u8_sums(v->q8, nq, Dp, 0, v->qnorm, stream));
    }
    return DPQ_OK;
}

// fp32 queries [nq][D].  Host form: into v->d_q.  Device form: the caller's rows where they already are [nq][Dp] (D a
// multiple of four, 16-byte aligned), else padded into v->d_q on `stream`.
int fivf_queries(dpq_flat_ivf* v, const void* queries_, int nq, bool device, bool coarse, hipStream_t stream, FivfQueries* q,
                 int metric = dpq::kFlatL2) {
    if (v->kind == kFivfBits) return fivf_queries_bits(v, queries_, nq, device, stream, q);
    if (v->kind == kFivfBytes) return fivf_queries_bytes(v, queries_, nq, device, coarse, stream, q, metric);
    const float* queries = static_cast<const float*>(queries_);
    const float** out = &q->f32;
    const int D = v->flat->D, Dp = v->flat->Dp;
    if (device && D == Dp && (reinterpret_cast<uintptr_t>(queries) & 15u) == 0) {
        *out = queries;
        return DPQ_OK;
    }
    if (int rc = grow(v->d_q, &v->q_n, (size_t)nq * Dp)) return rc;
    if (device) {
        DPQ_HIP(dpq::launch_flat_pad_rows(queries, nq, D, Dp, v->d_q, stream));
    } else if (D == Dp) {
        DPQ_HIP(hipMemcpy(v->d_q, queries, (size_t)nq * D * sizeof(float), hipMemcpyHostToDevice));
    } else {
        std::vector<float> padded((size_t)nq * Dp, 0.0f);
        for (int q = 0; q < nq; ++q) memcpy(&padded[(size_t)q * Dp], queries + (size_t)q * D, (size_t)D * sizeof(float));
        DPQ_HIP(hipMemcpy(v->d_q, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = v->d_q;
    return DPQ_OK;
}

// Room for the host forms' probes and results on the device.
int fivf_stage(dpq_flat_ivf* v, int nq, int nprobe, int top_k) {
    int rc = grow(v->d_probes, &v->dprobes_n, (size_t)nq * nprobe);
    if (!rc) rc = grow(v->d_cdists, &v->cdists_n, (size_t)nq * nprobe);
    if (!rc && top_k > 0) rc = grow(v->d_ids, &v->ids_n, (size_t)nq * top_k);
    if (!rc && top_k > 0) rc = grow(v->d_dists, &v->dists_n, (size_t)nq * top_k);
    return rc;
}

// The coarse step, all device pointers: d_lists[nq][nprobe] the nearest centroids by (distance, list number),
// d_cdists[nq][nprobe] their distances: the exact search over the centroids as a base.  Enqueues on `stream`.
// A binary structure: the centroids are a kFlatBits base and the distance is Hamming's, so ties are the rule and the key
// order settles them.  The query pointer of a batch may stand anywhere in a buffer with 64 spare rows behind its last.
// metric kFlatIP (fp32 centroids only): the nprobe centroids of largest exact inner product, ties to the lower list number,
// d_cdists their scores.
int fivf_probe_on_device(dpq_flat_ivf* v, const FivfQueries& qs, int nq, int nprobe, int32_t* d_lists, float* d_cdists,
                         hipStream_t stream, int metric = dpq::kFlatL2) {
    const int qb = std::min(nq, dpq::flat_query_batch(nprobe));
    int rc = grow(v->keys, &v->keys_n, (size_t)qb * dpq::flat_key_capacity(nprobe));
    if (!rc) rc = grow(v->state, &v->state_n, (size_t)qb);
    if (rc) return rc;
    const bool bits = v->kind == kFivfBits;
    dpq::FlatBase base;
    base.format = bits ? dpq::kFlatBits : dpq::kFlatF32;
    base.rows = bits ? (const void*)v->bcent.get() : (const void*)v->centroids.get();
    base.n = v->nlist;
    base.D = v->flat->D;
    base.Dp = v->flat->Dp;
    base.n_entries = v->nlist;
    base.metric = metric;
    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        const dpq::FlatQueries q{bits ? nullptr : qs.f32 + (size_t)q0 * base.Dp, nullptr, nullptr, m, nullptr,
                                 bits ? qs.bits + (size_t)q0 * base.Dp : nullptr};
        DPQ_HIP(dpq::launch_flat_search(base, q, nprobe, v->keys, v->state, d_lists + (size_t)q0 * nprobe,
                                        d_cdists + (size_t)q0 * nprobe, stream));
    }
    return DPQ_OK;
}

// Pairs a workgroup of the scan takes.
int fivf_group_cfg(int kind, int format) {
    int group = kind == kFivfBits ? dpq::kFlatIvfGroupBits : kind == kFivfBytes ? dpq::kFlatIvfGroupU8
              : format != dpq::kFlatF32 ? dpq::kFlatIvfGroupNarrow : dpq::kFlatIvfGroup;
    if (dev_mode())
        if (const char* e = getenv("DPQ_FLAT_IVF_GROUP")) group = std::max(1, atoi(e));  // tests and the probe script: a cap on G
    return group;
}

// What the scans of the four row formats run over: the handle's rows and the structure's lists, under a filter's bitmap
// (ff NULL: none) and a metric.  The scan of the structure's kind and the handle's format reads its own member.
struct FivfLists {
    dpq::FlatIvfLists f32;
    dpq::FlatIvfListsU8 u8;
    dpq::FlatIvfListsBits bits;
    dpq::FlatIvfListsNarrow narrow;  // a half or a quantised handle
};

int fivf_lists(dpq_flat_ivf* v, const dpq_flat_filter* ff, int metric, FivfLists* L) {
    const dpq_flat* f = v->flat;
    L->f32.rows = reinterpret_cast<const float*>(f->rows.get() + f->rows_at);
    L->f32.Dp = f->Dp;
    L->f32.id_offset = f->id_offset;
    L->f32.offsets = v->offsets;
    L->f32.list_rows = v->rows;
    L->f32.nlist = v->nlist;
    L->u8.rows = reinterpret_cast<const int8_t*>(f->rows.get() + f->rows_at);
    L->u8.norm = f->norm8;
    L->u8.Dp = f->Dp;
    L->u8.id_offset = f->id_offset;
    L->u8.offsets = v->offsets;
    L->u8.list_rows = v->rows;
    L->u8.nlist = v->nlist;
    L->bits.rows = reinterpret_cast<const uint32_t*>(f->rows.get() + f->rows_at);
    L->bits.Wp = f->Dp >> 2;
    L->bits.id_offset = f->id_offset;
    L->bits.offsets = v->offsets;
    L->bits.list_rows = v->rows;
    L->bits.nlist = v->nlist;
    L->narrow.format = f->format;
    L->narrow.rows = f->rows.get() + f->rows_at;
    L->narrow.Dp = f->Dp;
    L->narrow.id_offset = f->id_offset;
    L->narrow.offsets = v->offsets;
    L->narrow.list_rows = v->rows;
    L->narrow.nlist = v->nlist;
    L->f32.filter = L->u8.filter = L->bits.filter = L->narrow.filter = ff ? ff->words.get() : nullptr;
    L->f32.metric = L->u8.metric = L->narrow.metric = metric;
    if (metric == dpq::kFlatIP && v->kind == kFivfBytes) {  // the rows' terms in the place of the norms; none for signed rows
        if (f->format == dpq::kFlatU8)
            if (int rc = flat_ensure_rsum(v->flat)) return rc;
        L->u8.norm = f->format == dpq::kFlatU8 ? f->rsum8.get() : nullptr;
    }
    return DPQ_OK;
}

// The search behind its checks, all device pointers; qs: the prepared queries.  Slices of queries: per slice the probe
// pre-pass, the pairs sorted by list, the list scan of the structure's kind, the merge of the pairs' answers in rounds.
// Ends with the flag word read back.  ff (NULL: none): the scans take the rows its bitmap allows only.
int fivf_search_on_device(dpq_flat_ivf* v, const std::string& who, const FivfQueries& qs, int nq, const int32_t* d_probes,
                          int nprobe, int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream, const dpq_flat_filter* ff,
                          int metric = dpq::kFlatL2) {
    const dpq_flat* f = v->flat;
    const size_t row = (size_t)nprobe * top_k;
    const int per = (int)std::max<size_t>(1, std::min<size_t>(std::min(nq, dpq::kIvfSliceQueries), dpq::kIvfPartialBytes / (row * 8)));
    const int round = dpq::kIvfMergeKeys / top_k;
    const size_t pairs = (size_t)per * nprobe;
    size_t sort_bytes = 0, last_bytes = 0;  // of a full slice's sort, and of the last slice's
    DPQ_HIP(dpq::flat_ivf_sort_pairs(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, (int64_t)pairs, v->nlist, stream));
    if (nq % per)
        DPQ_HIP(dpq::flat_ivf_sort_pairs(nullptr, &last_bytes, nullptr, nullptr, nullptr, nullptr, (int64_t)(nq % per) * nprobe,
                                         v->nlist, stream));
    sort_bytes = std::max(sort_bytes, last_bytes);
    int rc = grow(v->probes, &v->probes_n, pairs);
    if (!rc && v->pairs_n < pairs) {
        v->pairs_n = 0;
        rc = v->pkeys.alloc(pairs);
        if (!rc) rc = v->pvals.alloc(pairs);
        if (!rc) rc = v->skeys.alloc(pairs);
        if (!rc) rc = v->svals.alloc(pairs);
        if (!rc) v->pairs_n = pairs;
    }
    if (!rc) rc = grow(v->sort_temp, &v->sort_n, sort_bytes);
    if (!rc) rc = grow(v->part_ids, &v->part_ids_n, (size_t)per * row);
    if (!rc) rc = grow(v->part_dists, &v->part_dists_n, (size_t)per * row);
    if (!rc && nprobe > round) rc = grow(v->tmp_ids, &v->tmp_ids_n, (size_t)per * top_k);
    if (!rc && nprobe > round) rc = grow(v->tmp_dists, &v->tmp_dists_n, (size_t)per * top_k);
    if (!rc && !v->flag.get()) rc = v->flag.alloc(1);
    if (rc) return rc;
    FivfLists L;
    if ((rc = fivf_lists(v, ff, metric, &L))) return rc;
    const dpq::FlatIvfLists& lists = L.f32;
    const dpq::FlatIvfListsU8& lists8 = L.u8;
    const dpq::FlatIvfListsBits& listsb = L.bits;
    const dpq::FlatIvfListsNarrow& listsn = L.narrow;
    const int group = fivf_group_cfg(v->kind, f->format);
    DPQ_HIP(hipMemsetAsync(v->flag, 0, sizeof(uint32_t), stream));
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const int64_t n_pairs = (int64_t)m * nprobe;
        DPQ_HIP(dpq::launch_ivf_probes(d_probes + (size_t)q0 * nprobe, m, nprobe, v->nlist, v->probes, v->flag, stream));
        DPQ_HIP(dpq::launch_flat_ivf_pairs(v->probes, n_pairs, v->nlist, v->pkeys, v->pvals, stream));
        size_t tb = v->sort_n;
        DPQ_HIP(dpq::flat_ivf_sort_pairs(v->sort_temp, &tb, v->pkeys, v->skeys, v->pvals, v->svals, n_pairs, v->nlist, stream));
        if (v->kind == kFivfBits)
            DPQ_HIP(dpq::launch_flat_ivf_scan_bits(listsb, reinterpret_cast<const uint32_t*>(qs.bits + (size_t)q0 * f->Dp), m, nprobe,
                                                   v->skeys, v->svals, top_k, group, v->part_ids, v->part_dists, stream));
        else if (v->kind == kFivfBytes)
            DPQ_HIP(dpq::launch_flat_ivf_scan_u8(lists8, qs.i8 + (size_t)q0 * f->Dp, qs.norm ? qs.norm + q0 : nullptr, m, nprobe, v->skeys, v->svals,
                                                 top_k, group, v->part_ids, v->part_dists, stream));
        else if (f->format != dpq::kFlatF32)
            DPQ_HIP(dpq::launch_flat_ivf_scan_narrow(listsn, qs.f32 + (size_t)q0 * f->Dp, m, nprobe, v->skeys, v->svals, top_k,
                                                     group, v->part_ids, v->part_dists, stream));
        else
            DPQ_HIP(dpq::launch_flat_ivf_scan(lists, qs.f32 + (size_t)q0 * f->Dp, m, nprobe, v->skeys, v->svals, top_k, group,
                                              v->part_ids, v->part_dists, stream));
        if ((rc = ivf_merge_rounds(v->part_ids, v->part_dists, v->tmp_ids, v->tmp_dists, nprobe, m, top_k,
                                   d_ids + (size_t)q0 * top_k, d_dists + (size_t)q0 * top_k, stream)))
            return rc;
        if (metric == dpq::kFlatIP)  // the merge ordered key words: now the scores, and -inf for padding
            DPQ_HIP(dpq::launch_flat_ivf_ip_scores(d_ids + (size_t)q0 * top_k, d_dists + (size_t)q0 * top_k, (int64_t)m * top_k, stream));
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(&bad, v->flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, who + ": a probe names no list (an entry >= nlist)");
    return DPQ_OK;
}

int fivf_results_down(dpq_flat_ivf* v, int nq, int top_k, int32_t* ids, float* dists) {
    DPQ_HIP(hipMemcpy(ids, v->d_ids, (size_t)nq * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, v->d_dists, (size_t)nq * top_k * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

// ---- the entry points' bodies, for either kind of handle ----------------------------------------------------------------

int fivf_create_device(const std::string& who, int kind, dpq_flat* f, const int32_t* d_labels, int64_t n, int nlist,
                       void* hip_stream, dpq_flat_ivf** out) {
    if (out) *out = nullptr;
    if (!f || !d_labels || !out || n < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or n < 0");
    if (int rc = fivf_nlist_ok(who, nlist)) return rc;
    if (int rc = fivf_enter_flat(who, f, kind)) return rc;
    std::unique_ptr<dpq_flat_ivf> v;
    if (int rc = fivf_from_device_labels(who, f, d_labels, n, nlist, (hipStream_t)hip_stream, &v)) return rc;
    *out = v.release();
    return DPQ_OK;
}

int fivf_create(const std::string& who, int kind, dpq_flat* f, const int32_t* labels, int64_t n, int nlist, dpq_flat_ivf** out) {
    if (out) *out = nullptr;
    if (!f || !labels || !out || n < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or n < 0");
    if (int rc = fivf_nlist_ok(who, nlist)) return rc;
    if (n != f->n) return fail(DPQ_ERR_ARG, who + ": n must be the handle's row count");
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] >= nlist) {
            char msg[96];
            snprintf(msg, sizeof msg, ": labels[%lld] = %d is >= nlist", (long long)i, (int)labels[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    if (int rc = fivf_enter_flat(who, f, kind)) return rc;
    DevBuf<int32_t> d_labels;
    if (int rc = d_labels.alloc((size_t)n)) return rc;
    DPQ_HIP(hipMemcpy(d_labels, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    std::unique_ptr<dpq_flat_ivf> v;
    if (int rc = fivf_from_device_labels(who, f, d_labels, n, nlist, nullptr, &v)) return rc;
    *out = v.release();
    return DPQ_OK;
}

// dpq_ivf_assign's arg-min over the handle's rows.  fp32: over its own padded rows, whose zero padding adds +0.0 to every
// distance.  Bytes: over its rows widened to fp32 (the bias of unsigned rows undone) a chunk at a time, the scratch
// bounded at 256 MB.  Half and quantised rows: likewise, widened or decoded by launch_flat_ivf_narrow_widen.
int fivf_labels_by_centroids(dpq_flat* f, const float* d_cent, int nlist, int32_t* d_labels) {
    if (f->format == dpq::kFlatF32) {
        DPQ_HIP(dpq::launch_ivf_argmin(reinterpret_cast<const float*>(f->rows.get() + f->rows_at), f->n, f->Dp, d_cent, nlist, nullptr,
                                       d_labels, nullptr, nullptr, nullptr));
        return DPQ_OK;
    }
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)f->Dp * (int64_t)sizeof(float)));
    DevBuf<float> wide;
    if (int rc = wide.alloc((size_t)std::min(chunk, f->n) * f->Dp)) return rc;
    const bool bytes = f->format == dpq::kFlatU8 || f->format == dpq::kFlatI8;
    for (int64_t r0 = 0; r0 < f->n; r0 += chunk) {
        const int64_t m = std::min(chunk, f->n - r0);
        if (bytes)
            DPQ_HIP(dpq::launch_flat_ivf_widen(f->rows.get() + (size_t)r0 * f->Dp, m, f->D, f->Dp, f->Dp, true,
                                               f->format == dpq::kFlatI8, wide, nullptr));
        else
            DPQ_HIP(dpq::launch_flat_ivf_narrow_widen(f->format, f->rows.get() + f->rows_at, f->Dp, r0, m, wide, nullptr));
        DPQ_HIP(dpq::launch_ivf_argmin(wide, m, f->Dp, d_cent, nlist, nullptr, d_labels + r0, nullptr, nullptr, nullptr));
    }
    DPQ_HIP(hipDeviceSynchronize());  // `wide` is freed on return
    return DPQ_OK;
}

int fivf_build(const std::string& who, int kind, dpq_flat* f, const float* centroids, int nlist, dpq_flat_ivf** out) {
    if (out) *out = nullptr;
    if (!f || !centroids || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = fivf_nlist_ok(who, nlist)) return rc;
    if (int rc = fivf_enter_flat(who, f, kind)) return rc;
    DevBuf<float> d_cent;
    if (int rc = fivf_upload_centroids(f, centroids, nlist, &d_cent)) return rc;
    DevBuf<int32_t> d_labels;
    if (int rc = d_labels.alloc((size_t)f->n)) return rc;
    if (int rc = fivf_labels_by_centroids(f, d_cent, nlist, d_labels)) return rc;
    std::unique_ptr<dpq_flat_ivf> v;
    if (int rc = fivf_from_device_labels(who, f, d_labels, f->n, nlist, nullptr, &v)) return rc;
    fivf_keep_centroids(v.get(), std::move(d_cent));
    *out = v.release();
    return DPQ_OK;
}

// ---- binary centroids: packed rows [nlist][(D + 7) / 8] in the caller's layout, ranked by Hamming distance ------------------

// ... in host memory -> the device, prepared as the handle's rows are (spare bits cleared, padded to Dp bytes).
int fivf_upload_centroids_bits(const dpq_flat* f, const uint8_t* centroids, int nlist, DevBuf<uint8_t>* d_out) {
    const size_t nb = (size_t)dpq::flat_bits_bytes(f->D);
    DevBuf<uint8_t> raw;
    if (int rc = raw.alloc((size_t)nlist * nb)) return rc;
    if (int rc = d_out->alloc((size_t)nlist * f->Dp)) return rc;
    DPQ_HIP(hipMemcpy(raw, centroids, (size_t)nlist * nb, hipMemcpyHostToDevice));
    DPQ_HIP(dpq::launch_flat_bits_prepare(raw, nlist, f->D, d_out->get(), f->Dp, nullptr));
    DPQ_HIP(hipDeviceSynchronize());  // `raw` is freed on return
    return DPQ_OK;
}

void fivf_keep_centroids_bits(dpq_flat_ivf* v, DevBuf<uint8_t>&& d_cent) {
    const int64_t bytes = (int64_t)v->nlist * v->flat->Dp;
    if (v->bcent.get()) v->device_bytes -= bytes;
    v->bcent = std::move(d_cent);
    v->device_bytes += bytes;
}

// The label of a row is its nearest centroid by (Hamming distance, list number): the exact top-1 search over the
// centroids as a kFlatBits base with the handle's own stored rows -- which have the prepared-query layout -- as the
// queries, a batch at a time.  The Hamming kernel reads whole tiles of up to 64 queries and masks those past the batch:
// the last batch of a handle whose row count is no multiple of 64 is searched from a copy with room behind it.
int fivf_labels_by_centroids_bits(dpq_flat* f, const uint8_t* d_cent, int nlist, int32_t* d_labels) {
    if (f->n == 0) return DPQ_OK;
    const int qb = (int)std::min<int64_t>(f->n, dpq::flat_query_batch(1));
    DevBuf<uint64_t> keys;
    DevBuf<dpq::FlatQueryState> state;
    DevBuf<float> dists;
    DevBuf<uint8_t> tail;
    int rc = keys.alloc((size_t)qb * dpq::flat_key_capacity(1));
    if (!rc) rc = state.alloc((size_t)qb);
    if (!rc) rc = dists.alloc((size_t)qb);
    if (rc) return rc;
    dpq::FlatBase base;
    base.format = dpq::kFlatBits;
    base.rows = d_cent;
    base.n = nlist;
    base.D = f->D;
    base.Dp = f->Dp;
    base.n_entries = nlist;
    const uint8_t* rows = f->rows.get() + f->rows_at;
    for (int64_t r0 = 0; r0 < f->n; r0 += qb) {
        const int m = (int)std::min<int64_t>(qb, f->n - r0);
        const uint8_t* q = rows + (size_t)r0 * f->Dp;
        if (r0 + m == f->n && f->n % 64 != 0) {
            if ((rc = tail.alloc(((size_t)m + 64) * f->Dp))) return rc;
            DPQ_HIP(hipMemcpyAsync(tail, q, (size_t)m * f->Dp, hipMemcpyDeviceToDevice, nullptr));
            q = tail;
        }
        DPQ_HIP(dpq::launch_flat_search(base, dpq::FlatQueries{nullptr, nullptr, nullptr, m, nullptr, q}, 1, keys, state,
                                        d_labels + r0, dists, nullptr));
    }
    DPQ_HIP(hipDeviceSynchronize());  // the scratch is freed on return
    return DPQ_OK;
}

int fivf_build_bits(const std::string& who, dpq_flat* f, const uint8_t* centroids, int nlist, dpq_flat_ivf** out) {
    if (out) *out = nullptr;
    if (!f || !centroids || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = fivf_nlist_ok(who, nlist)) return rc;
    if (int rc = fivf_enter_flat(who, f, kFivfBits)) return rc;
    DevBuf<uint8_t> d_cent;
    if (int rc = fivf_upload_centroids_bits(f, centroids, nlist, &d_cent)) return rc;
    DevBuf<int32_t> d_labels;
    if (int rc = d_labels.alloc((size_t)f->n)) return rc;
    if (int rc = fivf_labels_by_centroids_bits(f, d_cent, nlist, d_labels)) return rc;
    std::unique_ptr<dpq_flat_ivf> v;
    if (int rc = fivf_from_device_labels(who, f, d_labels, f->n, nlist, nullptr, &v)) return rc;
    fivf_keep_centroids_bits(v.get(), std::move(d_cent));
    *out = v.release();
    return DPQ_OK;
}

int fivf_probe(const std::string& who, int kind, dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int32_t* lists_out,
               float* dists_out, int metric = dpq::kFlatL2) {
    if (!v || !queries || !lists_out || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (int rc = fivf_enter(who, v, kind, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    FivfQueries q;
    if (int rc = fivf_queries(v, queries, nq, false, true, nullptr, &q)) return rc;  // (the coarse step reads no query terms)
    if (int rc = fivf_stage(v, nq, nprobe, 0)) return rc;
    if (int rc = fivf_probe_on_device(v, q, nq, nprobe, v->d_probes, v->d_cdists, nullptr, metric)) return rc;
    DPQ_HIP(hipMemcpy(lists_out, v->d_probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (dists_out) DPQ_HIP(hipMemcpy(dists_out, v->d_cdists, (size_t)nq * nprobe * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

int fivf_search_probes_device(const std::string& who, int kind, dpq_flat_ivf* v, const void* d_queries, int nq,
                              const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_dists, void* hip_stream,
                              const dpq_flat_filter* ff = nullptr, int metric = dpq::kFlatL2) {
    if (int rc = fivf_search_args(who, v, d_queries, nq, true, d_probes, nprobe, top_k, d_ids, d_dists)) return rc;
    if (int rc = fivf_filter_ok(who, v, ff)) return rc;
    if (int rc = fivf_enter(who, v, kind, nprobe, false)) return rc;
    if (nq == 0) return DPQ_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    FivfQueries q;
    if (int rc = fivf_queries(v, d_queries, nq, true, false, stream, &q, metric)) return rc;
    return fivf_search_on_device(v, who, q, nq, d_probes, nprobe, top_k, d_ids, d_dists, stream, ff, metric);
}

int fivf_search_probes(const std::string& who, int kind, dpq_flat_ivf* v, const void* queries, int nq, const int32_t* probes,
                       int nprobe, int top_k, int32_t* ids, float* dists, const dpq_flat_filter* ff = nullptr, int metric = dpq::kFlatL2) {
    if (int rc = fivf_search_args(who, v, queries, nq, true, probes, nprobe, top_k, ids, dists)) return rc;
    if (int rc = fivf_filter_ok(who, v, ff)) return rc;
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (int rc = fivf_probe_rows_ok(who, v, probes, nq, nprobe)) return rc;
    if (int rc = fivf_enter(who, v, kind, nprobe, false)) return rc;
    if (nq == 0) return DPQ_OK;
    FivfQueries q;
    if (int rc = fivf_queries(v, queries, nq, false, false, nullptr, &q, metric)) return rc;
    if (int rc = fivf_stage(v, nq, nprobe, top_k)) return rc;
    DPQ_HIP(hipMemcpy(v->d_probes, probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyHostToDevice));
    if (int rc = fivf_search_on_device(v, who, q, nq, v->d_probes, nprobe, top_k, v->d_ids, v->d_dists, nullptr, ff, metric)) return rc;
    return fivf_results_down(v, nq, top_k, ids, dists);
}

int fivf_search_device(const std::string& who, int kind, dpq_flat_ivf* v, const void* d_queries, int nq, int nprobe, int top_k,
                       int32_t* d_ids, float* d_dists, void* hip_stream, const dpq_flat_filter* ff = nullptr, int metric = dpq::kFlatL2) {
    if (int rc = fivf_search_args(who, v, d_queries, nq, false, nullptr, nprobe, top_k, d_ids, d_dists)) return rc;
    if (int rc = fivf_filter_ok(who, v, ff)) return rc;
    if (int rc = fivf_enter(who, v, kind, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    FivfQueries q;
    if (int rc = fivf_queries(v, d_queries, nq, true, true, stream, &q, metric)) return rc;
    if (int rc = fivf_stage(v, nq, nprobe, 0)) return rc;
    if (int rc = fivf_probe_on_device(v, q, nq, nprobe, v->d_probes, v->d_cdists, stream, metric)) return rc;
    return fivf_search_on_device(v, who, q, nq, v->d_probes, nprobe, top_k, d_ids, d_dists, stream, ff, metric);
}

int fivf_search(const std::string& who, int kind, dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int top_k,
                int32_t* ids, float* dists, const dpq_flat_filter* ff = nullptr, int metric = dpq::kFlatL2) {
    if (int rc = fivf_search_args(who, v, queries, nq, false, nullptr, nprobe, top_k, ids, dists)) return rc;
    if (int rc = fivf_filter_ok(who, v, ff)) return rc;
    if (int rc = fivf_enter(who, v, kind, nprobe, true)) return rc;
    if (nq == 0) return DPQ_OK;
    FivfQueries q;
    if (int rc = fivf_queries(v, queries, nq, false, true, nullptr, &q, metric)) return rc;
    if (int rc = fivf_stage(v, nq, nprobe, top_k)) return rc;
    if (int rc = fivf_probe_on_device(v, q, nq, nprobe, v->d_probes, v->d_cdists, nullptr, metric)) return rc;
    if (int rc = fivf_search_on_device(v, who, q, nq, v->d_probes, nprobe, top_k, v->d_ids, v->d_dists, nullptr, ff, metric)) return rc;
    return fivf_results_down(v, nq, top_k, ids, dists);
}

// ---- range search over the probed lists ------------------------------------------------------------------

// One pass of the range scan of the structure's kind over queries q0 .. q0 + m - 1 and their sorted pairs: counting
// (r.pool NULL) or emitting.
int fivf_range_pass(dpq_flat_ivf* v, const FivfLists& L, const FivfQueries& qs, int q0, int m, int nprobe, int group,
                    const dpq::FlatIvfRange& r) {
    const dpq_flat* f = v->flat;
    if (v->kind == kFivfBits)
        DPQ_HIP(dpq::launch_flat_ivf_range_bits(L.bits, reinterpret_cast<const uint32_t*>(qs.bits + (size_t)q0 * f->Dp), m, nprobe,
                                                v->skeys, v->svals, group, r, nullptr));
    else if (v->kind == kFivfBytes)
        DPQ_HIP(dpq::launch_flat_ivf_range_u8(L.u8, qs.i8 + (size_t)q0 * f->Dp, qs.norm ? qs.norm + q0 : nullptr, m, nprobe, v->skeys,
                                              v->svals, group, r, nullptr));
    else if (f->format != dpq::kFlatF32)
        DPQ_HIP(dpq::launch_flat_ivf_range_narrow(L.narrow, qs.f32 + (size_t)q0 * f->Dp, m, nprobe, v->skeys, v->svals, group, r, nullptr));
    else
        DPQ_HIP(dpq::launch_flat_ivf_range(L.f32, qs.f32 + (size_t)q0 * f->Dp, m, nprobe, v->skeys, v->svals, group, r, nullptr));
    return DPQ_OK;
}

// dpq_flat_ivf_range_search[_probes][_ip][_bytes | _bits].  probes == NULL: the coarse step.  Slices of at most 2048
// queries: the probe pre-pass, the pairs sorted by list, the count pass and its exclusive scan, and ONE host round trip for
// the queries' totals; then sub-batches of queries whose lists fit the pool: the emit pass, the segmented sort, the keys
// down and split on the host (inner product: the key words back to scores).
int fivf_range_call(const char* fn, int kind, int metric, dpq_flat_ivf* v, const dpq_flat_filter* ff, const void* queries, int nq,
                    const int32_t* probes, bool coarse, int nprobe, const float* radii, dpq_range_result** out) {
    const std::string who = fn;
    const bool ip = metric == dpq::kFlatIP;
    if (!out) return fail(DPQ_ERR_ARG, who + ": out is NULL");
    *out = nullptr;
    if (!v || nq < 0 || (nq > 0 && (!queries || !radii || (!coarse && !probes))))
        return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (nprobe < 1 || nprobe > dpq::kIvfMaxProbe) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    for (int q = 0; q < nq; ++q)
        if (std::isnan(radii[q]))
            return fail(DPQ_ERR_ARG, who + (ip ? ": threshold of query " : ": radius of query ") + std::to_string(q) + " is NaN");
    if (int rc = fivf_filter_ok(who, v, ff)) return rc;
    if (nprobe > v->nlist) return fail(DPQ_ERR_ARG, who + ": needs 1 <= nprobe <= min(nlist, 1024)");
    if (!coarse)
        if (int rc = fivf_probe_rows_ok(who, v, probes, nq, nprobe)) return rc;
    if (int rc = fivf_enter(who, v, kind, nprobe, coarse)) return rc;
    std::unique_ptr<dpq_range_result> res(new dpq_range_result());
    res->nq = nq;
    res->lims.assign((size_t)nq + 1, 0);
    if (nq == 0) {
        *out = res.release();
        return DPQ_OK;
    }
    FivfQueries qs;
    if (int rc = fivf_queries(v, queries, nq, false, coarse, nullptr, &qs, metric)) return rc;
    const int per = std::min(nq, dpq::kIvfSliceQueries);
    const size_t pairs = (size_t)per * nprobe, slots = pairs + 1;
    const int64_t budget = ivf_range_pool_keys();
    size_t sort_bytes = 0, last_bytes = 0, scan_bytes = 0;  // of a full slice's pair sort, of the last slice's, of the offsets' scan
    DPQ_HIP(dpq::flat_ivf_sort_pairs(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, (int64_t)pairs, v->nlist, nullptr));
    if (nq % per)
        DPQ_HIP(dpq::flat_ivf_sort_pairs(nullptr, &last_bytes, nullptr, nullptr, nullptr, nullptr, (int64_t)(nq % per) * nprobe,
                                         v->nlist, nullptr));
    sort_bytes = std::max(sort_bytes, last_bytes);
    int rc = fivf_stage(v, nq, nprobe, 0);
    if (!rc) rc = grow(v->probes, &v->probes_n, pairs);
    if (!rc && v->pairs_n < pairs) {
        v->pairs_n = 0;
        rc = v->pkeys.alloc(pairs);
        if (!rc) rc = v->pvals.alloc(pairs);
        if (!rc) rc = v->skeys.alloc(pairs);
        if (!rc) rc = v->svals.alloc(pairs);
        if (!rc) v->pairs_n = pairs;
    }
    if (!rc) rc = grow(v->sort_temp, &v->sort_n, sort_bytes);
    if (!rc) rc = grow(v->r_thr, &v->r_thr_n, (size_t)nq);
    if (!rc) rc = grow(v->r_counts, &v->r_counts_n, slots);
    if (!rc) rc = grow(v->r_offs, &v->r_offs_n, slots);
    if (!rc) rc = grow(v->r_qoffs, &v->r_qoffs_n, (size_t)per + 1);
    if (!rc) rc = grow(v->r_pool, &v->r_pool_n, (size_t)budget);
    if (!rc) rc = grow(v->r_sorted, &v->r_sorted_n, (size_t)budget);
    if (!rc && !v->flag.get()) rc = v->flag.alloc(1);
    if (rc) return rc;
    std::vector<uint64_t> thr((size_t)nq), sorted;
    for (int q = 0; q < nq; ++q) {
        const float r = radii[q];
        uint32_t bits = 0;
        if (ip) {  // s > t is word(s) < word(t): dpq_flat_range_search_ip's rule
            memcpy(&bits, &r, sizeof bits);
            thr[(size_t)q] = (uint64_t)dpq::flat_ip_word(bits) << 32;
        } else {  // d < r on non-negative floats is bits(d) < bits(r); key 0 lets nothing pass, ~0 everything
            if (r > 0.0f) memcpy(&bits, &r, sizeof bits);
            thr[(size_t)q] = std::isinf(r) && r > 0.0f ? dpq::kFlatNoKey : (uint64_t)bits << 32;
        }
    }
    DPQ_HIP(hipMemcpy(v->r_thr, thr.data(), (size_t)nq * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (coarse) {
        if ((rc = fivf_probe_on_device(v, qs, nq, nprobe, v->d_probes, v->d_cdists, nullptr, metric))) return rc;
    } else {
        DPQ_HIP(hipMemcpy(v->d_probes, probes, (size_t)nq * nprobe * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    FivfLists L;
    if ((rc = fivf_lists(v, ff, metric, &L))) return rc;
    const int group = fivf_group_cfg(v->kind, v->flat->format);
    DPQ_HIP(hipMemsetAsync(v->flag, 0, sizeof(uint32_t), nullptr));
    DPQ_HIP(dpq::ivf_range_offsets(nullptr, &scan_bytes, v->r_counts, v->r_offs, (int64_t)slots, nullptr));
    DevBuf<uint8_t> scan_temp;
    if ((rc = scan_temp.alloc(scan_bytes))) return rc;
    std::vector<int64_t> tot((size_t)per + 1), qoffs, offs_h;
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const int64_t n_pairs = (int64_t)m * nprobe;
        DPQ_HIP(dpq::launch_ivf_probes(v->d_probes.get() + (size_t)q0 * nprobe, m, nprobe, v->nlist, v->probes, v->flag, nullptr));
        DPQ_HIP(dpq::launch_flat_ivf_pairs(v->probes, n_pairs, v->nlist, v->pkeys, v->pvals, nullptr));
        size_t tb = v->sort_n;
        DPQ_HIP(dpq::flat_ivf_sort_pairs(v->sort_temp, &tb, v->pkeys, v->skeys, v->pvals, v->svals, n_pairs, v->nlist, nullptr));
        DPQ_HIP(hipMemsetAsync(v->r_counts.get() + n_pairs, 0, sizeof(int64_t), nullptr));  // the slot behind the last pair
        dpq::FlatIvfRange r;
        r.thr = v->r_thr.get() + q0;
        r.counts = v->r_counts;
        if ((rc = fivf_range_pass(v, L, qs, q0, m, nprobe, group, r))) return rc;
        tb = scan_bytes;
        DPQ_HIP(dpq::ivf_range_offsets(scan_temp, &tb, v->r_counts, v->r_offs, n_pairs + 1, nullptr));
        // the queries' list starts: every nprobe-th offset, and the slice's total behind them (one contiguous copy: a
        // strided one to pageable memory goes row by row)
        offs_h.resize((size_t)n_pairs + 1);
        DPQ_HIP(hipMemcpy(offs_h.data(), v->r_offs, offs_h.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int q = 0; q <= m; ++q) tot[(size_t)q] = offs_h[(size_t)q * nprobe];
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
                r.offs = v->r_offs;
                r.pool_base = tot[(size_t)a];
                r.pool = pool;
                r.pool_n = sum;
                r.qa = a;
                r.qb = b;
                if ((rc = fivf_range_pass(v, L, qs, q0, m, nprobe, group, r))) return rc;
                size_t sb = 0;
                DPQ_HIP(dpq::flat_range_sort(nullptr, &sb, pool, spool, sum, b - a, v->r_qoffs, nullptr));
                DevBuf<uint8_t> temp;  // the segmented sort's workspace
                if ((rc = temp.alloc(sb))) return rc;
                DPQ_HIP(dpq::flat_range_sort(temp, &sb, pool, spool, sum, b - a, v->r_qoffs, nullptr));
                sorted.resize((size_t)sum);
                DPQ_HIP(hipMemcpy(sorted.data(), spool, (size_t)sum * sizeof(uint64_t), hipMemcpyDeviceToHost));
                const size_t at = (size_t)(at0 + tot[(size_t)a]);
                for (size_t i = 0; i < (size_t)sum; ++i) {
                    uint32_t bits = (uint32_t)(sorted[i] >> 32);
                    if (ip) bits = dpq::flat_ip_word(bits);
                    res->ids[at + i] = (int32_t)(uint32_t)sorted[i];
                    memcpy(&res->dists[at + i], &bits, sizeof bits);
                }
            }
            a = b;
        }
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpy(&bad, v->flag, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) return fail(DPQ_ERR_ARG, who + ": a probe names no list (an entry >= nlist)");
    *out = res.release();
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_flat_ivf_create_device(dpq_flat* f, const int32_t* d_labels, int64_t n, int nlist, void* hip_stream, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_create_device("dpq_flat_ivf_create_device", kFivfF32, f, d_labels, n, nlist, hip_stream, out); });
}

int dpq_flat_ivf_create_bytes_device(dpq_flat* f, const int32_t* d_labels, int64_t n, int nlist, void* hip_stream, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_create_device("dpq_flat_ivf_create_bytes_device", kFivfBytes, f, d_labels, n, nlist, hip_stream, out); });
}

int dpq_flat_ivf_create(dpq_flat* f, const int32_t* labels, int64_t n, int nlist, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_create("dpq_flat_ivf_create", kFivfF32, f, labels, n, nlist, out); });
}

int dpq_flat_ivf_create_bytes(dpq_flat* f, const int32_t* labels, int64_t n, int nlist, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_create("dpq_flat_ivf_create_bytes", kFivfBytes, f, labels, n, nlist, out); });
}

int dpq_flat_ivf_build(dpq_flat* f, const float* centroids, int nlist, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_build("dpq_flat_ivf_build", kFivfF32, f, centroids, nlist, out); });
}

int dpq_flat_ivf_build_bytes(dpq_flat* f, const float* centroids, int nlist, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_build("dpq_flat_ivf_build_bytes", kFivfBytes, f, centroids, nlist, out); });
}

int dpq_flat_ivf_set_centroids(dpq_flat_ivf* v, const float* centroids, int nlist) {
    return guarded([&]() -> int {
    const std::string who = "dpq_flat_ivf_set_centroids";
    if (!v || !centroids) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (v->kind == kFivfBits)
        return fail(DPQ_ERR_ARG, who + ": the structure is over binary rows: its centroids are packed bits (dpq_flat_ivf_set_centroids_bits)");
    if (nlist != v->nlist) return fail(DPQ_ERR_ARG, who + ": nlist is not the structure's");
    if (int rc = flat_device_present(who)) return rc;
    DPQ_HIP(hipSetDevice(v->device));
    DevBuf<float> d_cent;
    if (int rc = fivf_upload_centroids(v->flat, centroids, nlist, &d_cent)) return rc;
    fivf_keep_centroids(v, std::move(d_cent));
    return DPQ_OK;
    });
}

int dpq_flat_ivf_set_centroids_bits(dpq_flat_ivf* v, const uint8_t* centroids, int nlist) {
    return guarded([&]() -> int {
    const std::string who = "dpq_flat_ivf_set_centroids_bits";
    if (!v || !centroids) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = fivf_kind_ok(who, v, kFivfBits)) return rc;
    if (nlist != v->nlist) return fail(DPQ_ERR_ARG, who + ": nlist is not the structure's");
    if (int rc = flat_device_present(who)) return rc;
    DPQ_HIP(hipSetDevice(v->device));
    DevBuf<uint8_t> d_cent;
    if (int rc = fivf_upload_centroids_bits(v->flat, centroids, nlist, &d_cent)) return rc;
    fivf_keep_centroids_bits(v, std::move(d_cent));
    return DPQ_OK;
    });
}

// ---- the *_bits set: a dpq_flat_open_bits handle, packed queries [nq][(D + 7) / 8] -----------------------------------------

int dpq_flat_ivf_create_bits(dpq_flat* f, const int32_t* labels, int64_t n, int nlist, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_create("dpq_flat_ivf_create_bits", kFivfBits, f, labels, n, nlist, out); });
}

int dpq_flat_ivf_create_bits_device(dpq_flat* f, const int32_t* d_labels, int64_t n, int nlist, void* hip_stream, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_create_device("dpq_flat_ivf_create_bits_device", kFivfBits, f, d_labels, n, nlist, hip_stream, out); });
}

int dpq_flat_ivf_build_bits(dpq_flat* f, const uint8_t* centroids, int nlist, dpq_flat_ivf** out) {
    return guarded([&]() -> int { return fivf_build_bits("dpq_flat_ivf_build_bits", f, centroids, nlist, out); });
}

int dpq_flat_ivf_probe_bits(dpq_flat_ivf* v, const uint8_t* queries, int nq, int nprobe, int32_t* lists_out, float* dists_out) {
    return guarded([&]() -> int { return fivf_probe("dpq_flat_ivf_probe_bits", kFivfBits, v, queries, nq, nprobe, lists_out, dists_out); });
}

int dpq_flat_ivf_search_probes_bits_device(dpq_flat_ivf* v, const uint8_t* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
        int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_bits_device", kFivfBits, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_flat_ivf_search_probes_bits(dpq_flat_ivf* v, const uint8_t* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* dists) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_bits", kFivfBits, v, queries, nq, probes, nprobe, top_k, ids, dists); });
}

int dpq_flat_ivf_search_bits_device(dpq_flat_ivf* v, const uint8_t* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
        void* hip_stream) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_bits_device", kFivfBits, v, d_queries, nq, nprobe, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_flat_ivf_search_bits(dpq_flat_ivf* v, const uint8_t* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_bits", kFivfBits, v, queries, nq, nprobe, top_k, ids, dists); });
}

void dpq_flat_ivf_free(dpq_flat_ivf* v) {
    if (!v) return;
    hipSetDevice(v->device);
    delete v;
}

int dpq_flat_ivf_get_info(const dpq_flat_ivf* v, dpq_ivf_stats* out) {
    return guarded([&]() -> int {
    if (!v || !out) return fail(DPQ_ERR_ARG, "dpq_flat_ivf_get_info: NULL argument");
    out->n_assigned = v->n_assigned;
    out->n_unassigned = v->n_unassigned;
    out->max_list_len = v->max_list_len;
    out->device_bytes = v->device_bytes;
    out->nlist = v->nlist;
    out->has_centroids = v->centroids.get() || v->bcent.get() ? 1 : 0;
    return DPQ_OK;
    });
}

int dpq_flat_ivf_get(const dpq_flat_ivf* v, int64_t* offsets_out, int32_t* ids_out) {
    return guarded([&]() -> int {
    if (!v || !offsets_out) return fail(DPQ_ERR_ARG, "dpq_flat_ivf_get: NULL argument");
    std::copy(v->h_offsets.begin(), v->h_offsets.end(), offsets_out);
    if (ids_out && v->n_assigned > 0) {
        DPQ_HIP(hipSetDevice(v->device));
        std::vector<uint32_t> rows((size_t)v->n_assigned);
        DPQ_HIP(hipMemcpy(rows.data(), v->rows, rows.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rows.size(); ++i) ids_out[i] = (int32_t)(uint32_t)((int64_t)rows[i] + v->flat->id_offset);
    }
    return DPQ_OK;
    });
}

int dpq_flat_ivf_probe(dpq_flat_ivf* v, const float* queries, int nq, int nprobe, int32_t* lists_out, float* dists_out) {
    return guarded([&]() -> int { return fivf_probe("dpq_flat_ivf_probe", kFivfF32, v, queries, nq, nprobe, lists_out, dists_out); });
}

int dpq_flat_ivf_probe_bytes(dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int32_t* lists_out, float* dists_out) {
    return guarded([&]() -> int { return fivf_probe("dpq_flat_ivf_probe_bytes", kFivfBytes, v, queries, nq, nprobe, lists_out, dists_out); });
}

int dpq_flat_ivf_search_probes_device(dpq_flat_ivf* v, const float* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids,
        float* d_dists, void* hip_stream) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_device", kFivfF32, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_flat_ivf_search_probes_bytes_device(dpq_flat_ivf* v, const void* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids,
        float* d_dists, void* hip_stream) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_bytes_device", kFivfBytes, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_flat_ivf_search_probes(dpq_flat_ivf* v, const float* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* dists) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes", kFivfF32, v, queries, nq, probes, nprobe, top_k, ids, dists); });
}

int dpq_flat_ivf_search_probes_bytes(dpq_flat_ivf* v, const void* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* dists) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_bytes", kFivfBytes, v, queries, nq, probes, nprobe, top_k, ids, dists); });
}

int dpq_flat_ivf_search_device(dpq_flat_ivf* v, const float* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
        void* hip_stream) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_device", kFivfF32, v, d_queries, nq, nprobe, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_flat_ivf_search_bytes_device(dpq_flat_ivf* v, const void* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
        void* hip_stream) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_bytes_device", kFivfBytes, v, d_queries, nq, nprobe, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_flat_ivf_search(dpq_flat_ivf* v, const float* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search", kFivfF32, v, queries, nq, nprobe, top_k, ids, dists); });
}

int dpq_flat_ivf_search_bytes(dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_bytes", kFivfBytes, v, queries, nq, nprobe, top_k, ids, dists); });
}

// ---- the *_filtered set: the search of each kind under a dpq_flat_filter of the structure's handle (NULL: no filter) ----------

int dpq_flat_ivf_search_probes_filtered_device(dpq_flat_ivf* v, const float* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
        int32_t* d_ids, float* d_dists, void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_filtered_device", kFivfF32, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, hip_stream, filter); });
}

int dpq_flat_ivf_search_probes_filtered(dpq_flat_ivf* v, const float* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* dists, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_filtered", kFivfF32, v, queries, nq, probes, nprobe, top_k, ids, dists, filter); });
}

int dpq_flat_ivf_search_filtered_device(dpq_flat_ivf* v, const float* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
        void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_filtered_device", kFivfF32, v, d_queries, nq, nprobe, top_k, d_ids, d_dists, hip_stream, filter); });
}

int dpq_flat_ivf_search_filtered(dpq_flat_ivf* v, const float* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists,
        const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_filtered", kFivfF32, v, queries, nq, nprobe, top_k, ids, dists, filter); });
}

int dpq_flat_ivf_search_probes_filtered_bytes_device(dpq_flat_ivf* v, const void* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
        int32_t* d_ids, float* d_dists, void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_filtered_bytes_device", kFivfBytes, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, hip_stream, filter); });
}

int dpq_flat_ivf_search_probes_filtered_bytes(dpq_flat_ivf* v, const void* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* dists, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_filtered_bytes", kFivfBytes, v, queries, nq, probes, nprobe, top_k, ids, dists, filter); });
}

int dpq_flat_ivf_search_filtered_bytes_device(dpq_flat_ivf* v, const void* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
        void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_filtered_bytes_device", kFivfBytes, v, d_queries, nq, nprobe, top_k, d_ids, d_dists, hip_stream, filter); });
}

int dpq_flat_ivf_search_filtered_bytes(dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists,
        const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_filtered_bytes", kFivfBytes, v, queries, nq, nprobe, top_k, ids, dists, filter); });
}

int dpq_flat_ivf_search_probes_filtered_bits_device(dpq_flat_ivf* v, const uint8_t* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
        int32_t* d_ids, float* d_dists, void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_filtered_bits_device", kFivfBits, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_dists, hip_stream, filter); });
}

int dpq_flat_ivf_search_probes_filtered_bits(dpq_flat_ivf* v, const uint8_t* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* dists, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_filtered_bits", kFivfBits, v, queries, nq, probes, nprobe, top_k, ids, dists, filter); });
}

int dpq_flat_ivf_search_filtered_bits_device(dpq_flat_ivf* v, const uint8_t* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
        void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_filtered_bits_device", kFivfBits, v, d_queries, nq, nprobe, top_k, d_ids, d_dists, hip_stream, filter); });
}

int dpq_flat_ivf_search_filtered_bits(dpq_flat_ivf* v, const uint8_t* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists,
        const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_filtered_bits", kFivfBits, v, queries, nq, nprobe, top_k, ids, dists, filter); });
}

// ---- inner product: the plain and the *_bytes set (a structure over binary rows is refused by its kind) --------------------

int dpq_flat_ivf_probe_ip(dpq_flat_ivf* v, const float* queries, int nq, int nprobe, int32_t* lists_out, float* scores_out) {
    return guarded([&]() -> int { return fivf_probe("dpq_flat_ivf_probe_ip", kFivfF32, v, queries, nq, nprobe, lists_out, scores_out, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_probes_ip_device(dpq_flat_ivf* v, const float* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
        int32_t* d_ids, float* d_scores, void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_ip_device", kFivfF32, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_scores, hip_stream, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_probes_ip(dpq_flat_ivf* v, const float* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* scores, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_ip", kFivfF32, v, queries, nq, probes, nprobe, top_k, ids, scores, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_ip_device(dpq_flat_ivf* v, const float* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_scores,
        void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_ip_device", kFivfF32, v, d_queries, nq, nprobe, top_k, d_ids, d_scores, hip_stream, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_ip(dpq_flat_ivf* v, const float* queries, int nq, int nprobe, int top_k, int32_t* ids, float* scores,
        const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_ip", kFivfF32, v, queries, nq, nprobe, top_k, ids, scores, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_probe_ip_bytes(dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int32_t* lists_out, float* scores_out) {
    return guarded([&]() -> int { return fivf_probe("dpq_flat_ivf_probe_ip_bytes", kFivfBytes, v, queries, nq, nprobe, lists_out, scores_out, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_probes_ip_bytes_device(dpq_flat_ivf* v, const void* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
        int32_t* d_ids, float* d_scores, void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes_device("dpq_flat_ivf_search_probes_ip_bytes_device", kFivfBytes, v, d_queries, nq, d_probes, nprobe, top_k, d_ids, d_scores, hip_stream, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_probes_ip_bytes(dpq_flat_ivf* v, const void* queries, int nq, const int32_t* probes, int nprobe, int top_k, int32_t* ids,
        float* scores, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_probes("dpq_flat_ivf_search_probes_ip_bytes", kFivfBytes, v, queries, nq, probes, nprobe, top_k, ids, scores, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_ip_bytes_device(dpq_flat_ivf* v, const void* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_scores,
        void* hip_stream, const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search_device("dpq_flat_ivf_search_ip_bytes_device", kFivfBytes, v, d_queries, nq, nprobe, top_k, d_ids, d_scores, hip_stream, filter, dpq::kFlatIP); });
}

int dpq_flat_ivf_search_ip_bytes(dpq_flat_ivf* v, const void* queries, int nq, int nprobe, int top_k, int32_t* ids, float* scores,
        const dpq_flat_filter* filter) {
    return guarded([&]() -> int { return fivf_search("dpq_flat_ivf_search_ip_bytes", kFivfBytes, v, queries, nq, nprobe, top_k, ids, scores, filter, dpq::kFlatIP); });
}

// ---- range search: host forms; the answer is freed by dpq_range_result_free ------------------------------------------------

int dpq_flat_ivf_range_search(dpq_flat_ivf* v, const dpq_flat_filter* filter, const float* queries, int nq, int nprobe, const float* radii,
        dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search", kFivfF32, dpq::kFlatL2, v, filter, queries, nq, nullptr, true, nprobe, radii, out); });
}

int dpq_flat_ivf_range_search_probes(dpq_flat_ivf* v, const dpq_flat_filter* filter, const float* queries, int nq, const int32_t* probes,
        int nprobe, const float* radii, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_probes", kFivfF32, dpq::kFlatL2, v, filter, queries, nq, probes, false, nprobe, radii, out); });
}

int dpq_flat_ivf_range_search_ip(dpq_flat_ivf* v, const dpq_flat_filter* filter, const float* queries, int nq, int nprobe,
        const float* thresholds, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_ip", kFivfF32, dpq::kFlatIP, v, filter, queries, nq, nullptr, true, nprobe, thresholds, out); });
}

int dpq_flat_ivf_range_search_probes_ip(dpq_flat_ivf* v, const dpq_flat_filter* filter, const float* queries, int nq, const int32_t* probes,
        int nprobe, const float* thresholds, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_probes_ip", kFivfF32, dpq::kFlatIP, v, filter, queries, nq, probes, false, nprobe, thresholds, out); });
}

int dpq_flat_ivf_range_search_bytes(dpq_flat_ivf* v, const dpq_flat_filter* filter, const void* queries, int nq, int nprobe, const float* radii,
        dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_bytes", kFivfBytes, dpq::kFlatL2, v, filter, queries, nq, nullptr, true, nprobe, radii, out); });
}

int dpq_flat_ivf_range_search_probes_bytes(dpq_flat_ivf* v, const dpq_flat_filter* filter, const void* queries, int nq, const int32_t* probes,
        int nprobe, const float* radii, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_probes_bytes", kFivfBytes, dpq::kFlatL2, v, filter, queries, nq, probes, false, nprobe, radii, out); });
}

int dpq_flat_ivf_range_search_ip_bytes(dpq_flat_ivf* v, const dpq_flat_filter* filter, const void* queries, int nq, int nprobe,
        const float* thresholds, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_ip_bytes", kFivfBytes, dpq::kFlatIP, v, filter, queries, nq, nullptr, true, nprobe, thresholds, out); });
}

int dpq_flat_ivf_range_search_probes_ip_bytes(dpq_flat_ivf* v, const dpq_flat_filter* filter, const void* queries, int nq, const int32_t* probes,
        int nprobe, const float* thresholds, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_probes_ip_bytes", kFivfBytes, dpq::kFlatIP, v, filter, queries, nq, probes, false, nprobe, thresholds, out); });
}

int dpq_flat_ivf_range_search_bits(dpq_flat_ivf* v, const dpq_flat_filter* filter, const uint8_t* queries, int nq, int nprobe, const float* radii,
        dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_bits", kFivfBits, dpq::kFlatL2, v, filter, queries, nq, nullptr, true, nprobe, radii, out); });
}

int dpq_flat_ivf_range_search_probes_bits(dpq_flat_ivf* v, const dpq_flat_filter* filter, const uint8_t* queries, int nq, const int32_t* probes,
        int nprobe, const float* radii, dpq_range_result** out) {
    return guarded([&]() -> int { return fivf_range_call("dpq_flat_ivf_range_search_probes_bits", kFivfBits, dpq::kFlatL2, v, filter, queries, nq, probes, false, nprobe, radii, out); });
}

}  // extern "C"
