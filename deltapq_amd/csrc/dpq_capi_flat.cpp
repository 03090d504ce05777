// dpq_capi_flat.cpp -- the exact-search entry points of include/deltapq_amd.h: dpq_flat_* and dpq_flat_filter_*.
#include "dpq_capi_internal.h"

// ---- exact search over raw vectors (dpq_flat.hip, dpq_flat_u8.hip) ---------------------------------------------------

namespace {

// The format of queries of type Q.  A call takes the handles whose rows go with it (dpq::flat_query_format): float -- an
// fp32, a half or a quantised handle, uint8_t -- a handle of dpq_flat_open_u8, int8_t -- a handle of dpq_flat_open_i8.
// The _bits calls take uint8_t as well, eight dimensions to a byte: their entry points hand the bytes on as bits_t.
enum class bits_t : uint8_t {};
template <class Q> constexpr int format_of = dpq::kFlatF32;
template <> constexpr int format_of<uint8_t> = dpq::kFlatU8;
template <> constexpr int format_of<int8_t> = dpq::kFlatI8;
template <> constexpr int format_of<bits_t> = dpq::kFlatBits;
const bits_t* as_bits(const uint8_t* p) { return reinterpret_cast<const bits_t*>(p); }

// Elements of type Q in one query as the caller holds it: D values, or the (D + 7) / 8 bytes of D bits.
size_t flat_query_elems(const dpq_flat* f) {
    return f->format == dpq::kFlatBits ? (size_t)dpq::flat_bits_bytes(f->D) : (size_t)f->D;
}

// A search call's name: its shape ("dpq_flat_search", "dpq_flat_rerank", ...), its metric, the format of its queries
// (`kind`), the device form.  The same pieces name the call of the same shape for queries of any other format.
struct FlatCall {
    const char* stem;
    int metric;
    int kind;
    bool device = false;
    std::string name(int k) const {
        if (k == dpq::kFlatBits) return std::string(stem) + "_bits" + (device ? "_device" : "");  // no inner product over bits
        return std::string(stem) + (metric == dpq::kFlatIP ? "_ip" : "") + (k == dpq::kFlatU8 ? "_u8" : k == dpq::kFlatI8 ? "_i8" : "") +
               (device ? "_device" : "");
    }
    std::string name() const { return name(kind); }
};

// The handle's rows, all of them or those a filter lists, as the launchers of dpq_flat.h take them.
dpq::FlatBase flat_base(const dpq_flat* f, const dpq_flat_filter* ff, int metric) {
    dpq::FlatBase b;
    b.format = f->format;
    b.rows = f->rows.get() + f->rows_at;
    b.n = f->n;
    b.D = f->D;
    b.Dp = f->Dp;
    b.id_offset = f->id_offset;
    b.metric = metric;
    b.norm = f->norm8;
    b.rsum = f->rsum8;
    if (f->rows_at) b.quant = reinterpret_cast<const float2*>(f->rows.get());
    b.filtered = ff != nullptr;
    b.list = ff ? ff->list.get() : nullptr;
    b.n_entries = ff ? ff->n_allowed : f->n;
    return b;
}

// Candidates of dpq_flat_rerank*, all device pointers; ends with one flag word read back.
template <class Q>
int flat_rerank_on_device(const char* fn, int metric, dpq_flat* f, const Q* d_queries, int nq, const int32_t* d_cand,
                          int n_cand, int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    const size_t n_pad = dpq::flat_rerank_keys(n_cand);
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)nq, ((size_t)64 << 20) / (n_pad * sizeof(uint64_t))));
    int rc = grow(f->keys, &f->keys_n, (size_t)per * n_pad);
    if (rc) return rc;
    if (!f->flag.get() && (rc = f->flag.alloc(1))) return rc;
    DPQ_HIP(hipMemsetAsync(f->flag, 0, sizeof(uint32_t), stream));
    const dpq::FlatBase base = flat_base(f, nullptr, metric);
    dpq::FlatRerank r;
    r.n_cand = n_cand;
    r.top_k = top_k;
    r.map = f->h_map.empty() ? nullptr : f->map.get();
    r.n_map = (int64_t)f->h_map.size();
    r.keys = f->keys;
    r.flag = f->flag;
    for (int q0 = 0; q0 < nq; q0 += per) {
        r.queries = d_queries + (size_t)q0 * flat_query_elems(f);
        r.nq = std::min(per, nq - q0);
        r.cand = d_cand + (size_t)q0 * n_cand;
        r.ids = d_ids + (size_t)q0 * top_k;
        r.dists = d_dists + (size_t)q0 * top_k;
        DPQ_HIP(dpq::launch_flat_rerank(base, r, stream));
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(&bad, f->flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, std::string(fn) + ": a candidate names no row of this handle");
    return DPQ_OK;
}

// A handle takes the calls of its own kind only: the fp32-query functions an fp32, a half or a quantised handle, the
// _u8 functions a handle of dpq_flat_open_u8, the _i8 functions one of dpq_flat_open_i8, the _bits functions one of
// dpq_flat_open_bits / dpq_flat_open_binarised.  The message names the call of the same shape that the handle does take.
int flat_kind(const dpq_flat* f, const FlatCall& c) {
    const int kind = dpq::flat_query_format(f->format);
    if (kind == c.kind) return DPQ_OK;
    const std::string fn = c.name(), right = c.name(kind);
    switch (f->format) {
        case dpq::kFlatF16:
        case dpq::kFlatBF16:
            return fail(DPQ_ERR_ARG, fn + ": the handle holds half-precision vectors (dpq_flat_open_half, "
                                          "dpq_flat_open_narrowed), searched with fp32 queries; call " + right);
        case dpq::kFlatSQ8:
        case dpq::kFlatSQ4:
            return fail(DPQ_ERR_ARG, fn + ": the handle holds scalar-quantised vectors (dpq_flat_open_sq, "
                                          "dpq_flat_open_quantised), searched with fp32 queries; call " + right);
        case dpq::kFlatF32: return fail(DPQ_ERR_ARG, fn + ": the handle holds fp32 vectors (dpq_flat_open); call " + right);
        case dpq::kFlatI8:
            return fail(DPQ_ERR_ARG, fn + ": the handle holds signed byte vectors (dpq_flat_open_i8); call " + right);
        case dpq::kFlatBits:
            return fail(DPQ_ERR_ARG, fn + ": the handle holds binary vectors (dpq_flat_open_bits, dpq_flat_open_binarised), "
                                          "compared by Hamming distance only; call " + right);
    }
    if (c.kind == dpq::kFlatF32 && c.metric == dpq::kFlatIP)
        return fail(DPQ_ERR_ARG, fn + ": the handle holds byte vectors (dpq_flat_open_u8), which have no inner-product search "
                                      "with fp32 queries; call " + right);
    return fail(DPQ_ERR_ARG, fn + ": the handle holds byte vectors (dpq_flat_open_u8); call " + right);
}

int flat_rerank_args(const FlatCall& c, const dpq_flat* f, const void* queries, int nq, const void* cand, int n_cand,
                     int top_k, const void* ids, const void* dists) {
    if (!f || !queries || !cand || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, c.name() + ": NULL argument or nq < 0");
    if (int rc = flat_kind(f, c)) return rc;
    if (top_k < 1 || top_k > n_cand || n_cand > dpq::kFlatMaxTopK)
        return fail(DPQ_ERR_ARG, c.name() + ": needs 1 <= top_k <= n_cand <= 16384");
    return DPQ_OK;
}

// After the arguments: the device a call works on.
int flat_use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(DPQ_ERR_NO_DEVICE, "device ordinal out of range");
    DPQ_HIP(hipSetDevice(device));
    return DPQ_OK;
}

// The checks of every dpq_flat_open*: the arguments (the half format too, where there is one) before any device call,
// then the device.
int flat_open_args(const char* fn, const void* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out,
                   const int* half_format = nullptr, int max_d = dpq::kFlatMaxD) {
    const std::string who(fn);
    if (out) *out = nullptr;
    if (!vectors || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 1) return fail(DPQ_ERR_ARG, who + ": n < 1");
    if (D < 1 || D > max_d) return fail(DPQ_ERR_ARG, who + ": D outside 1.." + std::to_string(max_d));
    if (id_offset < 0 || n + id_offset >= ((int64_t)1 << 31))
        return fail(DPQ_ERR_ARG, who + ": id_offset < 0 or n + id_offset >= 2^31 (ids are int32)");
    if (half_format && *half_format != DPQ_HALF_F16 && *half_format != DPQ_HALF_BF16)
        return fail(DPQ_ERR_ARG, who + ": format is neither DPQ_HALF_F16 nor DPQ_HALF_BF16");
    return flat_use_device(device);
}

// Every dpq_flat_open*: n rows of D values, fp32 (from_fp32: dpq_flat_open, and dpq_flat_open_narrowed, which narrows
// them) or already of `format`, become the handle's rows of `format`.  callers_format: `format` is an argument of the
// call and is checked with the others.  The rows go up in slices of at most 128 MB through one staging buffer and are
// padded (narrowed, biased) by the format's prepare kernel on the device; fp32 and 16-bit rows that need no padding go
// straight to their place.
int flat_open(const char* fn, int format, bool from_fp32, bool callers_format, const void* vectors, int64_t n, int D,
              int device, int64_t id_offset, dpq_flat** out) {
    if (int rc = flat_open_args(fn, vectors, n, D, device, id_offset, out, callers_format ? &format : nullptr)) return rc;
    const bool bytes = dpq::flat_query_format(format) != dpq::kFlatF32;
    const size_t elem = bytes ? 1 : format == dpq::kFlatF32 ? sizeof(float) : sizeof(uint16_t);  // of a stored value
    const size_t in_elem = from_fp32 ? sizeof(float) : elem;                                     // of a value as given
    std::unique_ptr<dpq_flat> f(new dpq_flat);
    f->device = device;
    f->n = n;
    f->id_offset = id_offset;
    f->D = D;
    f->Dp = bytes ? dpq::flat_u8_padded_d(D) : format == dpq::kFlatF32 ? dpq::flat_padded_d(D) : dpq::flat_half_padded_d(D);
    f->format = format;
    int rc = f->rows.alloc((size_t)n * f->Dp * elem);
    if (!rc && bytes) rc = f->norm8.alloc((size_t)((n + 3) & ~(int64_t)3));
    if (rc) return fail(rc, std::string(fn) + ": the vectors do not fit into device memory (" + dpq_last_error() + ")");
    // the norm array's padding is read by the last stripe's 16-byte loads (and masked afterwards): keep it defined
    if (bytes) DPQ_HIP(hipMemset(f->norm8.get() + ((n - 1) & ~(int64_t)3), 0, 4 * sizeof(int32_t)));
    if (!bytes && in_elem == elem && f->Dp == D) {
        DPQ_HIP(hipMemcpy(f->rows, vectors, (size_t)n * D * elem, hipMemcpyHostToDevice));
    } else {
        const int64_t tile = std::max<int64_t>(1, ((int64_t)128 << 20) / ((int64_t)D * (int64_t)in_elem));  // rows per upload
        DevBuf<uint8_t> tmp;
        if ((rc = tmp.alloc((size_t)std::min(n, tile) * D * in_elem))) return rc;
        for (int64_t r0 = 0; r0 < n; r0 += tile) {
            const int64_t m = std::min(tile, n - r0);
            const void* src = tmp.get();
            void* dst = f->rows.get() + (size_t)r0 * f->Dp * elem;
            DPQ_HIP(hipMemcpy(tmp, static_cast<const uint8_t*>(vectors) + (size_t)r0 * D * in_elem, (size_t)m * D * in_elem,
                              hipMemcpyHostToDevice));
            if (bytes)
                DPQ_HIP(dpq::launch_flat_u8_prepare(tmp, m, D, f->Dp, static_cast<int8_t*>(dst), f->norm8.get() + r0, nullptr,
                                                    format == dpq::kFlatI8));
            else if (format == dpq::kFlatF32)
                DPQ_HIP(dpq::launch_flat_pad_rows(static_cast<const float*>(src), m, D, f->Dp, static_cast<float*>(dst), nullptr));
            else if (from_fp32)
                DPQ_HIP(dpq::launch_flat_half_narrow(static_cast<const float*>(src), m, D, f->Dp, format,
                                                     static_cast<uint16_t*>(dst), nullptr));
            else
                DPQ_HIP(dpq::launch_flat_half_prepare(static_cast<const uint16_t*>(src), m, D, f->Dp, static_cast<uint16_t*>(dst),
                                                      nullptr));
            DPQ_HIP(hipDeviceSynchronize());
        }
    }
    *out = f.release();
    return DPQ_OK;
}

// ---- scalar-quantised vectors: the quantiser's calls and the two ways of opening a quantised handle -----------------

// The arguments every dpq_sq_* / dpq_flat_open_sq / dpq_flat_open_quantised call checks, in the header's order, before
// any device call.  null_arg: one of the call's required pointers is NULL.  id_offset: of the open calls only.  lo and
// step are checked where both are given; `optional` (dpq_flat_open_quantised) allows both to be NULL, never one.
int sq_args(const std::string& who, bool null_arg, int64_t n, int D, int bits, const int64_t* id_offset, const float* lo,
            const float* step, bool optional = false) {
    if (null_arg || (!optional && (!lo || !step))) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 1) return fail(DPQ_ERR_ARG, who + ": n < 1");
    if (D < 1 || D > dpq::kFlatMaxD) return fail(DPQ_ERR_ARG, who + ": D outside 1..2048");
    if (bits != DPQ_SQ_8BIT && bits != DPQ_SQ_4BIT) return fail(DPQ_ERR_ARG, who + ": bits is neither DPQ_SQ_8BIT nor DPQ_SQ_4BIT");
    if (id_offset && (*id_offset < 0 || n + *id_offset >= ((int64_t)1 << 31)))
        return fail(DPQ_ERR_ARG, who + ": id_offset < 0 or n + id_offset >= 2^31 (ids are int32)");
    if (lo && step) {
        for (int d = 0; d < D; ++d) {
            if (!std::isfinite(lo[d])) return fail(DPQ_ERR_ARG, who + ": lo of dimension " + std::to_string(d) + " is not finite");
            if (!(step[d] >= 0.0f) || std::isinf(step[d]))
                return fail(DPQ_ERR_ARG, who + ": step of dimension " + std::to_string(d) + " is negative, NaN or infinite");
        }
    } else if (lo || step) {
        return fail(DPQ_ERR_ARG, who + ": lo and step are both NULL (train on these rows) or both given");
    }
    return DPQ_OK;
}

// Host rows [n][row_bytes] go up in slices of at most 128 MB through one staging buffer; use(d_slice, r0, m) works on
// rows r0 .. r0 + m - 1 and the device is idle when it returns.
template <class F>
int sq_slices(const void* host, int64_t n, size_t row_bytes, F&& use) {
    const int64_t tile = std::max<int64_t>(1, ((int64_t)128 << 20) / (int64_t)row_bytes);
    DevBuf<uint8_t> tmp;
    if (int rc = tmp.alloc((size_t)std::min(n, tile) * row_bytes)) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += tile) {
        const int64_t m = std::min(tile, n - r0);
        DPQ_HIP(hipMemcpy(tmp, static_cast<const uint8_t*>(host) + (size_t)r0 * row_bytes, (size_t)m * row_bytes, hipMemcpyHostToDevice));
        if (int rc = use(tmp.get(), r0, m)) return rc;
        DPQ_HIP(hipDeviceSynchronize());
    }
    return DPQ_OK;
}

// dpq_sq_train once the arguments are checked and the device is chosen.
int sq_train(const float* vectors, int64_t n, int D, int bits, float* lo_out, float* step_out) {
    std::vector<uint32_t> mm((size_t)2 * D, 0u);
    std::fill(mm.begin(), mm.begin() + D, 0xffffffffu);
    DevBuf<uint32_t> d_mm;
    if (int rc = d_mm.alloc(mm.size())) return rc;
    DPQ_HIP(hipMemcpy(d_mm, mm.data(), mm.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    int rc = sq_slices(vectors, n, (size_t)D * sizeof(float), [&](const uint8_t* d_slice, int64_t, int64_t m) -> int {
        DPQ_HIP(dpq::launch_flat_sq_minmax(reinterpret_cast<const float*>(d_slice), m, D, d_mm, d_mm.get() + D, nullptr));
        return DPQ_OK;
    });
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(mm.data(), d_mm, mm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const double levels = bits == DPQ_SQ_8BIT ? 255.0 : 15.0;
    for (int d = 0; d < D; ++d) {
        const uint32_t lb = dpq::flat_order_bits(mm[(size_t)d]), hb = dpq::flat_order_bits(mm[(size_t)D + d]);
        float lo, hi;
        memcpy(&lo, &lb, sizeof lo);
        memcpy(&hi, &hb, sizeof hi);
        if (lo == 0.0f) lo = 0.0f;  // -0.0 is stored as +0.0
        if (hi == 0.0f) hi = 0.0f;
        lo_out[d] = lo;
        step_out[d] = (float)(((double)hi - (double)lo) / levels);
    }
    return DPQ_OK;
}

// (lo, step) [D] -> the device array the kernels read, len >= D entries, (+0, +0) beyond D.
int sq_upload_quant(const float* lo, const float* step, int D, int len, float2* d_quant) {
    std::vector<float2> q((size_t)len, make_float2(0.0f, 0.0f));
    for (int d = 0; d < D; ++d) q[(size_t)d] = make_float2(lo[d], step[d]);
    DPQ_HIP(hipMemcpy(d_quant, q.data(), q.size() * sizeof(float2), hipMemcpyHostToDevice));
    return DPQ_OK;
}

// A quantised handle with its quantiser in place and its rows allocated, not yet filled.
int sq_new_handle(const char* fn, int64_t n, int D, int bits, const float* lo, const float* step, int device, int64_t id_offset,
                  std::unique_ptr<dpq_flat>* out) {
    std::unique_ptr<dpq_flat> f(new dpq_flat);
    f->device = device;
    f->n = n;
    f->id_offset = id_offset;
    f->D = D;
    f->Dp = dpq::flat_sq_padded_d(D, bits);
    f->format = bits == DPQ_SQ_8BIT ? dpq::kFlatSQ8 : dpq::kFlatSQ4;
    f->sq_lo.assign(lo, lo + D);
    f->sq_step.assign(step, step + D);
    const int qlen = dpq::flat_sq_quant_len(f->Dp);
    f->rows_at = (size_t)qlen * sizeof(float2);
    if (int rc = f->rows.alloc(f->rows_at + (size_t)n * dpq::flat_sq_row_bytes(f->Dp, bits)))
        return fail(rc, std::string(fn) + ": the vectors do not fit into device memory (" + dpq_last_error() + ")");
    if (int rc = sq_upload_quant(lo, step, D, qlen, reinterpret_cast<float2*>(f->rows.get()))) return rc;
    *out = std::move(f);
    return DPQ_OK;
}

// ---- binary vectors: a handle with its rows allocated, not yet filled ------------------------------------------------
int bits_new_handle(const char* fn, int64_t n, int D, int device, int64_t id_offset, std::unique_ptr<dpq_flat>* out) {
    std::unique_ptr<dpq_flat> f(new dpq_flat);
    f->device = device;
    f->n = n;
    f->id_offset = id_offset;
    f->D = D;
    f->Dp = dpq::flat_bits_row_bytes(D);  // bytes of a stored row
    f->format = dpq::kFlatBits;
    if (int rc = f->rows.alloc((size_t)n * f->Dp))
        return fail(rc, std::string(fn) + ": the vectors do not fit into device memory (" + dpq_last_error() + ")");
    *out = std::move(f);
    return DPQ_OK;
}

// thresholds [D] on the device, or nothing for NULL
int bits_upload_thresholds(const float* thresholds, int D, DevBuf<float>* d_thr) {
    if (!thresholds) return DPQ_OK;
    if (int rc = d_thr->alloc((size_t)D)) return rc;
    DPQ_HIP(hipMemcpy(*d_thr, thresholds, (size_t)D * sizeof(float), hipMemcpyHostToDevice));
    return DPQ_OK;
}

int grow_outputs(dpq_flat* f, size_t want) {
    if (f->out_n >= want) return DPQ_OK;
    f->out_n = 0;
    int rc = f->d_ids.alloc(want);
    if (!rc) rc = f->d_dists.alloc(want);
    if (!rc) f->out_n = want;
    return rc;
}

// Uploads m queries as the distance kernels read them: fp32 rows padded to Dp, or bytes (biased, on a u8 handle) padded
// with norms -- and, for the inner product on a u8 handle, with the queries' correction terms.
template <class Q>
int flat_stage_queries(dpq_flat* f, int metric, const Q* src, int m, std::vector<float>* padded) {
    const int D = f->D, Dp = f->Dp;
    if constexpr (format_of<Q> == dpq::kFlatBits) {
        DPQ_HIP(hipMemcpy(f->q_raw, src, (size_t)m * flat_query_elems(f), hipMemcpyHostToDevice));
        DPQ_HIP(dpq::launch_flat_bits_prepare(f->q_raw, m, D, reinterpret_cast<uint8_t*>(f->q8.get()), Dp, nullptr));
    } else if constexpr (format_of<Q> != dpq::kFlatF32) {
        DPQ_HIP(hipMemcpy(f->q_raw, src, (size_t)m * D, hipMemcpyHostToDevice));
        DPQ_HIP(dpq::launch_flat_u8_prepare(f->q_raw, m, D, Dp, f->q8, f->qnorm, nullptr, format_of<Q> == dpq::kFlatI8));
        if (format_of<Q> == dpq::kFlatU8 && metric == dpq::kFlatIP)
            DPQ_HIP(dpq::launch_flat_u8_sums(f->q8, m, Dp, 0, f->qsum, nullptr));
    } else {
        if (Dp != D) {
            padded->assign((size_t)m * Dp, 0.0f);
            for (int q = 0; q < m; ++q) memcpy(&(*padded)[(size_t)q * Dp], src + (size_t)q * D, (size_t)D * sizeof(float));
            src = padded->data();
        }
        DPQ_HIP(hipMemcpy(f->d_q, src, (size_t)m * Dp * sizeof(float), hipMemcpyHostToDevice));
    }
    return DPQ_OK;
}

// The query buffers of a search or a range call.  The first inner-product call on a u8 handle also makes the rows'
// correction terms, in one pass over the stored rows: 4 * n bytes, kept until dpq_flat_close.
template <class Q>
int flat_grow_queries(dpq_flat* f, int metric, size_t qb) {
    if constexpr (format_of<Q> == dpq::kFlatBits) {
        // the distance kernel reads whole tiles of up to 64 queries from wherever a sub-batch starts, and masks the rest
        int rc = grow(f->q_raw, &f->q_raw_n, qb * flat_query_elems(f));
        if (!rc) rc = grow(f->q8, &f->q8_n, (qb + 64) * f->Dp);
        return rc;
    } else if constexpr (format_of<Q> != dpq::kFlatF32) {
        int rc = grow(f->q_raw, &f->q_raw_n, qb * f->D);
        if (!rc) rc = grow(f->q8, &f->q8_n, qb * f->Dp);
        if (!rc) rc = grow(f->qnorm, &f->qnorm_n, qb);
        if (format_of<Q> == dpq::kFlatU8 && metric == dpq::kFlatIP) {
            if (!rc) rc = grow(f->qsum, &f->qsum_n, qb);
            if (!rc && !f->rsum8.get()) {
                DevBuf<int32_t> sums;
                if ((rc = sums.alloc((size_t)((f->n + 3) & ~(int64_t)3)))) return rc;
                // the padding is read by the last stripe's 16-byte loads (and masked afterwards): keep it defined
                DPQ_HIP(hipMemset(sums.get() + ((f->n - 1) & ~(int64_t)3), 0, 4 * sizeof(int32_t)));
                DPQ_HIP(dpq::launch_flat_u8_sums(reinterpret_cast<const int8_t*>(f->rows.get()), f->n, f->Dp, 16384 * f->D, sums, nullptr));
                DPQ_HIP(hipDeviceSynchronize());
                f->rsum8 = std::move(sums);
            }
        }
        return rc;
    } else {
        return grow(f->d_q, &f->q_n, qb * f->Dp);
    }
}

// Queries [a, a + m) of the staged batch, as the launchers of dpq_flat.h take them.
dpq::FlatQueries flat_queries(const dpq_flat* f, int a, int m) {
    if (f->format == dpq::kFlatBits)
        return {nullptr, nullptr, nullptr, m, nullptr, reinterpret_cast<const uint8_t*>(f->q8.get()) + (size_t)a * f->Dp};
    if (dpq::flat_query_format(f->format) != dpq::kFlatF32)
        return {nullptr, f->q8.get() + (size_t)a * f->Dp, f->qnorm.get() + a, m, f->qsum.get() ? f->qsum.get() + a : nullptr};
    return {f->d_q.get() + (size_t)a * f->Dp, nullptr, nullptr, m};
}

// What dpq_flat_search[_u8] and dpq_flat_search_filtered[_u8] share once their arguments are checked: the buffers, the
// batches of staged queries, the copies down and the check of every query's state.  ff NULL: all rows, top_k <= n.
// metric: dpq::kFlatL2, or dpq::kFlatIP (dists then holds scores).
template <class Q>
int flat_search_run(const std::string& who, int metric, dpq_flat* f, const dpq_flat_filter* ff, const Q* queries, int nq,
                    int top_k, int32_t* ids, float* dists) {
    if (nq == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(f->device));
    const int qb = std::min(nq, dpq::flat_query_batch(top_k));
    int rc = grow(f->keys, &f->keys_n, (size_t)qb * dpq::flat_key_capacity(top_k));
    if (!rc) rc = grow(f->state, &f->state_n, (size_t)qb);
    if (!rc) rc = flat_grow_queries<Q>(f, metric, (size_t)qb);
    if (!rc) rc = grow_outputs(f, (size_t)qb * top_k);
    if (rc) return rc;
    const dpq::FlatBase base = flat_base(f, ff, metric);
    const uint32_t expect = (uint32_t)std::min<int64_t>(top_k, base.n_entries);
    std::vector<float> padded;
    std::vector<dpq::FlatQueryState> st((size_t)qb);
    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        if ((rc = flat_stage_queries(f, metric, queries + (size_t)q0 * flat_query_elems(f), m, &padded))) return rc;
        DPQ_HIP(dpq::launch_flat_search(base, flat_queries(f, 0, m), top_k, f->keys, f->state, f->d_ids, f->d_dists, nullptr));
        DPQ_HIP(hipMemcpy(ids + (size_t)q0 * top_k, f->d_ids, (size_t)m * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
        DPQ_HIP(hipMemcpy(dists + (size_t)q0 * top_k, f->d_dists, (size_t)m * top_k * sizeof(float), hipMemcpyDeviceToHost));
        DPQ_HIP(hipMemcpy(st.data(), f->state, (size_t)m * sizeof(dpq::FlatQueryState), hipMemcpyDeviceToHost));
        for (int q = 0; q < m; ++q)
            if (st[(size_t)q].overflow || st[(size_t)q].count != expect)
                return fail(DPQ_ERR_STATE, who + ": internal error: a key buffer overflowed");
    }
    return DPQ_OK;
}

// dpq_flat_search and its _ip / _u8 / _i8 forms: Q is the query type of the call's kind.
template <class Q>
int flat_search_call(const FlatCall& c, dpq_flat* f, const Q* queries, int nq, int top_k, int32_t* ids, float* dists) {
    const std::string who = c.name();
    if (!f || !queries || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (top_k < 1 || top_k > DPQ_FLAT_MAX_TOPK) return fail(DPQ_ERR_ARG, who + ": top_k outside 1..DPQ_FLAT_MAX_TOPK");
    if (int rc = flat_kind(f, c)) return rc;
    if (top_k > f->n) return fail(DPQ_ERR_TOPK, who + ": top_k exceeds the number of vectors");
    return flat_search_run(who, c.metric, f, nullptr, queries, nq, top_k, ids, dists);
}

}  // namespace

extern "C" {

int dpq_flat_open(const float* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    return flat_open("dpq_flat_open", dpq::kFlatF32, true, false, vectors, n, D, device, id_offset, out);
    });
}

int dpq_flat_open_u8(const uint8_t* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    return flat_open("dpq_flat_open_u8", dpq::kFlatU8, false, false, vectors, n, D, device, id_offset, out);
    });
}

int dpq_flat_open_i8(const int8_t* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    return flat_open("dpq_flat_open_i8", dpq::kFlatI8, false, false, vectors, n, D, device, id_offset, out);
    });
}

int dpq_half_from_float(const float* in, int64_t count, int format, uint16_t* out) {
    return guarded([&]() -> int {
    if (count < 0 || (count > 0 && (!in || !out))) return fail(DPQ_ERR_ARG, "dpq_half_from_float: NULL argument or count < 0");
    if (format != DPQ_HALF_F16 && format != DPQ_HALF_BF16)
        return fail(DPQ_ERR_ARG, "dpq_half_from_float: format is neither DPQ_HALF_F16 nor DPQ_HALF_BF16");
    for (int64_t i = 0; i < count; ++i) {
        uint32_t u;
        memcpy(&u, in + i, sizeof u);
        out[i] = dpq::flat_half_narrow(u, format);
    }
    return DPQ_OK;
    });
}

int dpq_half_to_float(const uint16_t* in, int64_t count, int format, float* out) {
    return guarded([&]() -> int {
    if (count < 0 || (count > 0 && (!in || !out))) return fail(DPQ_ERR_ARG, "dpq_half_to_float: NULL argument or count < 0");
    if (format != DPQ_HALF_F16 && format != DPQ_HALF_BF16)
        return fail(DPQ_ERR_ARG, "dpq_half_to_float: format is neither DPQ_HALF_F16 nor DPQ_HALF_BF16");
    for (int64_t i = 0; i < count; ++i) {
        const uint32_t u = dpq::flat_half_widen(in[i], format);
        memcpy(out + i, &u, sizeof u);
    }
    return DPQ_OK;
    });
}

int dpq_flat_open_half(const uint16_t* vectors, int64_t n, int D, int format, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    return flat_open("dpq_flat_open_half", format, false, true, vectors, n, D, device, id_offset, out);
    });
}

int dpq_flat_open_narrowed(const float* vectors, int64_t n, int D, int format, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    return flat_open("dpq_flat_open_narrowed", format, true, true, vectors, n, D, device, id_offset, out);
    });
}

int dpq_sq_train(const float* vectors, int64_t n, int D, int bits, int device, float* lo_out, float* step_out) {
    return guarded([&]() -> int {
    if (int rc = sq_args("dpq_sq_train", !vectors || !lo_out || !step_out, n, D, bits, nullptr, nullptr, nullptr, true)) return rc;
    if (int rc = flat_use_device(device)) return rc;
    return sq_train(vectors, n, D, bits, lo_out, step_out);
    });
}

int dpq_sq_encode(const float* vectors, int64_t n, int D, int bits, const float* lo, const float* step, int device,
                  uint8_t* codes_out) {
    return guarded([&]() -> int {
    if (int rc = sq_args("dpq_sq_encode", !vectors || !codes_out, n, D, bits, nullptr, lo, step)) return rc;
    if (int rc = flat_use_device(device)) return rc;
    const int stride = dpq::flat_sq_row_bytes(D, bits);
    const int64_t tile = std::max<int64_t>(1, ((int64_t)128 << 20) / ((int64_t)D * (int64_t)sizeof(float)));
    DevBuf<float2> d_quant;
    DevBuf<uint8_t> d_codes;
    int rc = d_quant.alloc((size_t)D);
    if (!rc) rc = d_codes.alloc((size_t)std::min(n, tile) * stride);
    if (!rc) rc = sq_upload_quant(lo, step, D, D, d_quant);
    if (rc) return rc;
    return sq_slices(vectors, n, (size_t)D * sizeof(float), [&](const uint8_t* d_slice, int64_t r0, int64_t m) -> int {
        DPQ_HIP(dpq::launch_flat_sq_encode(reinterpret_cast<const float*>(d_slice), m, D, bits, d_quant, d_codes, stride, nullptr));
        DPQ_HIP(hipMemcpy(codes_out + (size_t)r0 * stride, d_codes, (size_t)m * stride, hipMemcpyDeviceToHost));
        return DPQ_OK;
    });
    });
}

int dpq_sq_decode(const uint8_t* codes, int64_t n, int D, int bits, const float* lo, const float* step, float* out) {
    return guarded([&]() -> int {
    if (int rc = sq_args("dpq_sq_decode", !codes || !out, n, D, bits, nullptr, lo, step)) return rc;
    const size_t stride = (size_t)dpq::flat_sq_row_bytes(D, bits);
    for (int64_t r = 0; r < n; ++r)
        for (int d = 0; d < D; ++d) {
            const uint8_t b = codes[(size_t)r * stride + (bits == DPQ_SQ_8BIT ? d : d >> 1)];
            const uint32_t c = bits == DPQ_SQ_8BIT ? b : (d & 1) ? b >> 4 : b & 15u;
            const float scaled = (float)c * step[d];  // the product and the sum each rounded: the build passes -ffp-contract=off
            out[(size_t)r * D + d] = lo[d] + scaled;
        }
    return DPQ_OK;
    });
}

int dpq_flat_open_sq(const uint8_t* codes, int64_t n, int D, int bits, const float* lo, const float* step, int device,
                     int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    const char* fn = "dpq_flat_open_sq";
    if (out) *out = nullptr;
    if (int rc = sq_args(fn, !codes || !out, n, D, bits, &id_offset, lo, step)) return rc;
    if (int rc = flat_use_device(device)) return rc;
    std::unique_ptr<dpq_flat> f;
    if (int rc = sq_new_handle(fn, n, D, bits, lo, step, device, id_offset, &f)) return rc;
    const int in_stride = dpq::flat_sq_row_bytes(D, bits), stride = dpq::flat_sq_row_bytes(f->Dp, bits);
    uint8_t* rows = f->rows.get() + f->rows_at;
    if (f->Dp == D) {
        DPQ_HIP(hipMemcpy(rows, codes, (size_t)n * stride, hipMemcpyHostToDevice));
    } else {
        int rc = sq_slices(codes, n, (size_t)in_stride, [&](const uint8_t* d_slice, int64_t r0, int64_t m) -> int {
            DPQ_HIP(dpq::launch_flat_sq_prepare(d_slice, m, D, bits, rows + (size_t)r0 * stride, stride, nullptr));
            return DPQ_OK;
        });
        if (rc) return rc;
    }
    *out = f.release();
    return DPQ_OK;
    });
}

int dpq_flat_open_quantised(const float* vectors, int64_t n, int D, int bits, const float* lo, const float* step, int device,
                            int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    const char* fn = "dpq_flat_open_quantised";
    if (out) *out = nullptr;
    if (int rc = sq_args(fn, !vectors || !out, n, D, bits, &id_offset, lo, step, true)) return rc;
    if (int rc = flat_use_device(device)) return rc;
    std::vector<float> trained;
    if (!lo) {  // dpq_sq_train on these very rows
        trained.resize((size_t)2 * D);
        if (int rc = sq_train(vectors, n, D, bits, trained.data(), trained.data() + D)) return rc;
        lo = trained.data();
        step = trained.data() + D;
    }
    std::unique_ptr<dpq_flat> f;
    if (int rc = sq_new_handle(fn, n, D, bits, lo, step, device, id_offset, &f)) return rc;
    const int stride = dpq::flat_sq_row_bytes(f->Dp, bits);
    uint8_t* rows = f->rows.get() + f->rows_at;
    const float2* d_quant = reinterpret_cast<const float2*>(f->rows.get());
    int rc = sq_slices(vectors, n, (size_t)D * sizeof(float), [&](const uint8_t* d_slice, int64_t r0, int64_t m) -> int {
        DPQ_HIP(dpq::launch_flat_sq_encode(reinterpret_cast<const float*>(d_slice), m, D, bits, d_quant, rows + (size_t)r0 * stride,
                                           stride, nullptr));
        return DPQ_OK;
    });
    if (rc) return rc;
    *out = f.release();
    return DPQ_OK;
    });
}

int dpq_flat_sq_get(const dpq_flat* f, int* bits, float* lo_out, float* step_out) {
    return guarded([&]() -> int {
    if (!f || !bits || !lo_out || !step_out) return fail(DPQ_ERR_ARG, "dpq_flat_sq_get: NULL argument");
    if (f->format != dpq::kFlatSQ8 && f->format != dpq::kFlatSQ4)
        return fail(DPQ_ERR_ARG, "dpq_flat_sq_get: the handle holds no scalar-quantised vectors (dpq_flat_open_sq, "
                                 "dpq_flat_open_quantised)");
    *bits = f->format == dpq::kFlatSQ8 ? DPQ_SQ_8BIT : DPQ_SQ_4BIT;
    memcpy(lo_out, f->sq_lo.data(), (size_t)f->D * sizeof(float));
    memcpy(step_out, f->sq_step.data(), (size_t)f->D * sizeof(float));
    return DPQ_OK;
    });
}

int dpq_flat_open_bits(const uint8_t* rows, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    const char* fn = "dpq_flat_open_bits";
    if (int rc = flat_open_args(fn, rows, n, D, device, id_offset, out, nullptr, DPQ_FLAT_BITS_MAX_D)) return rc;
    std::unique_ptr<dpq_flat> f;
    if (int rc = bits_new_handle(fn, n, D, device, id_offset, &f)) return rc;
    int rc = sq_slices(rows, n, (size_t)dpq::flat_bits_bytes(D), [&](const uint8_t* d_slice, int64_t r0, int64_t m) -> int {
        DPQ_HIP(dpq::launch_flat_bits_prepare(d_slice, m, D, f->rows.get() + (size_t)r0 * f->Dp, f->Dp, nullptr));
        return DPQ_OK;
    });
    if (rc) return rc;
    *out = f.release();
    return DPQ_OK;
    });
}

int dpq_bits_from_float(const float* vectors, int64_t n, int D, const float* thresholds, int device, uint8_t* bits_out) {
    return guarded([&]() -> int {
    const std::string who("dpq_bits_from_float");
    if (!vectors || !bits_out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 1) return fail(DPQ_ERR_ARG, who + ": n < 1");
    if (D < 1 || D > DPQ_FLAT_BITS_MAX_D) return fail(DPQ_ERR_ARG, who + ": D outside 1.." + std::to_string(DPQ_FLAT_BITS_MAX_D));
    if (int rc = flat_use_device(device)) return rc;
    const int stride = dpq::flat_bits_bytes(D);
    const int64_t tile = std::max<int64_t>(1, ((int64_t)128 << 20) / ((int64_t)D * (int64_t)sizeof(float)));
    DevBuf<float> d_thr;
    DevBuf<uint8_t> d_bits;
    int rc = bits_upload_thresholds(thresholds, D, &d_thr);
    if (!rc) rc = d_bits.alloc((size_t)std::min(n, tile) * stride);
    if (rc) return rc;
    return sq_slices(vectors, n, (size_t)D * sizeof(float), [&](const uint8_t* d_slice, int64_t r0, int64_t m) -> int {
        DPQ_HIP(dpq::launch_flat_bits_from_float(reinterpret_cast<const float*>(d_slice), m, D, d_thr.get(), d_bits, stride, nullptr));
        DPQ_HIP(hipMemcpy(bits_out + (size_t)r0 * stride, d_bits, (size_t)m * stride, hipMemcpyDeviceToHost));
        return DPQ_OK;
    });
    });
}

int dpq_flat_open_binarised(const float* vectors, int64_t n, int D, const float* thresholds, int device, int64_t id_offset,
                            dpq_flat** out) {
    return guarded([&]() -> int {
    const char* fn = "dpq_flat_open_binarised";
    if (int rc = flat_open_args(fn, vectors, n, D, device, id_offset, out, nullptr, DPQ_FLAT_BITS_MAX_D)) return rc;
    std::unique_ptr<dpq_flat> f;
    if (int rc = bits_new_handle(fn, n, D, device, id_offset, &f)) return rc;
    DevBuf<float> d_thr;
    if (int rc = bits_upload_thresholds(thresholds, D, &d_thr)) return rc;
    int rc = sq_slices(vectors, n, (size_t)D * sizeof(float), [&](const uint8_t* d_slice, int64_t r0, int64_t m) -> int {
        DPQ_HIP(dpq::launch_flat_bits_from_float(reinterpret_cast<const float*>(d_slice), m, D, d_thr.get(),
                                                 f->rows.get() + (size_t)r0 * f->Dp, f->Dp, nullptr));
        return DPQ_OK;
    });
    if (rc) return rc;
    *out = f.release();
    return DPQ_OK;
    });
}

int dpq_flat_close(dpq_flat* f) {
    return guarded([&]() -> int {
    if (!f) return DPQ_OK;
    hipSetDevice(f->device);
    delete f;
    return DPQ_OK;
    });
}

int dpq_flat_search(dpq_flat* f, const float* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatL2, dpq::kFlatF32}, f, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_ip(dpq_flat* f, const float* queries, int nq, int top_k, int32_t* ids, float* scores) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatIP, dpq::kFlatF32}, f, queries, nq, top_k, ids, scores);
    });
}

int dpq_flat_search_u8(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatL2, dpq::kFlatU8}, f, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_ip_u8(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* scores) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatIP, dpq::kFlatU8}, f, queries, nq, top_k, ids, scores);
    });
}

int dpq_flat_search_i8(dpq_flat* f, const int8_t* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatL2, dpq::kFlatI8}, f, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_ip_i8(dpq_flat* f, const int8_t* queries, int nq, int top_k, int32_t* ids, float* scores) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatIP, dpq::kFlatI8}, f, queries, nq, top_k, ids, scores);
    });
}

int dpq_flat_search_bits(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_search_call({"dpq_flat_search", dpq::kFlatL2, dpq::kFlatBits}, f, as_bits(queries), nq, top_k, ids, dists);
    });
}

int dpq_flat_set_id_map(dpq_flat* f, const uint32_t* map, int64_t n_map) {
    return guarded([&]() -> int {
    if (!f || !map || n_map < 1 || n_map >= ((int64_t)1 << 31)) return fail(DPQ_ERR_ARG, "dpq_flat_set_id_map: bad argument");
    for (int64_t i = 0; i < n_map; ++i)
        if ((int64_t)map[i] >= f->n) return fail(DPQ_ERR_ARG, "dpq_flat_set_id_map: an entry names no row of this handle");
    DPQ_HIP(hipSetDevice(f->device));
    DevBuf<uint32_t> d;
    int rc = d.alloc((size_t)n_map);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(d, map, (size_t)n_map * sizeof(uint32_t), hipMemcpyHostToDevice));
    f->map = std::move(d);
    f->h_map.assign(map, map + n_map);
    return DPQ_OK;
    });
}

}  // extern "C"

// ---- exact filtered and range search (dpq_flat_filter.hip) -----------------------------------------------------------
namespace {

constexpr int64_t kFlatRangePoolKeys = (int64_t)1 << 19;  // keys of a range sub-batch's lists: 4 MB, and as much sorted
constexpr int kFlatRangeQueries = 1024;                   // queries whose lists one pass counts

// 32 bits of the caller's bitmap from bit `start` on; bits at or beyond n_bits read as 0.
uint32_t bitmap_bits32(const uint32_t* words, int64_t n_bits, int64_t start) {
    if (start >= n_bits) return 0;
    const int64_t lo = start >> 5, n_words = (n_bits + 31) / 32;
    const int sh = (int)(start & 31);
    uint32_t v = words[lo] >> sh;
    if (sh && lo + 1 < n_words) v |= words[lo + 1] << (32 - sh);
    const int64_t valid = n_bits - start;
    if (valid < 32) v &= (1u << valid) - 1u;
    return v;
}

}  // namespace

// After the arguments that need no handle, before the handle is read.
int flat_device_present(const std::string& who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, who + ": no HIP device visible; this library has no CPU fallback");
    return DPQ_OK;
}

namespace {

int flat_filter_owner(const dpq_flat* f, const dpq_flat_filter* ff, const std::string& who) {
    if (ff->owner == f->serial) return DPQ_OK;
    return fail(DPQ_ERR_ARG, who + ": the filter was made for another handle");
}

// dpq_flat_search_filtered and its _ip / _u8 / _i8 forms: Q is the query type of the call's kind.
template <class Q>
int flat_search_filtered_call(const FlatCall& c, dpq_flat* f, const dpq_flat_filter* ff, const Q* queries, int nq, int top_k,
                              int32_t* ids, float* dists) {
    const std::string who = c.name();
    if (!f || !ff || !queries || !ids || !dists || nq < 0)
        return fail(DPQ_ERR_ARG, who + ": NULL argument (the filter included) or nq < 0");
    if (top_k < 1 || top_k > DPQ_FLAT_MAX_TOPK) return fail(DPQ_ERR_ARG, who + ": top_k outside 1..DPQ_FLAT_MAX_TOPK");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = flat_kind(f, c)) return rc;
    if (int rc = flat_filter_owner(f, ff, who)) return rc;
    return flat_search_run(who, c.metric, f, ff, queries, nq, top_k, ids, dists);
}

// One distance pass of a range search over queries [a, a + m) of the staged batch: counting (pool NULL) or emitting.
int flat_range_pass(dpq_flat* f, const dpq_flat_filter* ff, int metric, int a, int m, uint64_t* pool) {
    dpq::FlatQueryState* state = f->state.get() + a;
    DPQ_HIP(dpq::launch_flat_range_state(state, f->r_thr.get() + a, m, nullptr));
    DPQ_HIP(dpq::launch_flat_range_pass(flat_base(f, ff, metric), flat_queries(f, a, m), pool, f->r_offs, state, nullptr));
    return DPQ_OK;
}

// dpq_flat_range_search and its _ip / _u8 / _i8 forms (_ip: radii are score thresholds, a row is kept when its score is
// above).  Count, then emit: a pass over a batch of queries counts every list, the host lays the lists out, and
// sub-batches of at most kFlatRangePoolKeys keys (or one longer list) are formed again into the pool,
// sorted there and brought down.
template <class Q>
int flat_range_call(const FlatCall& c, dpq_flat* f, const dpq_flat_filter* ff, const Q* queries, int nq, const float* radii,
                    dpq_range_result** out) {
    const int metric = c.metric;
    const std::string who = c.name();
    if (!out) return fail(DPQ_ERR_ARG, who + ": out is NULL");
    *out = nullptr;
    if (!f || nq < 0 || (nq > 0 && (!queries || !radii))) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    for (int q = 0; q < nq; ++q)
        if (std::isnan(radii[q]))
            return fail(DPQ_ERR_ARG, who + (metric == dpq::kFlatIP ? ": threshold of query " : ": radius of query ") +
                                         std::to_string(q) + " is NaN");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = flat_kind(f, c)) return rc;
    if (ff)
        if (int rc = flat_filter_owner(f, ff, who)) return rc;
    std::unique_ptr<dpq_range_result> res(new dpq_range_result());
    res->nq = nq;
    res->lims.assign((size_t)nq + 1, 0);
    if (nq == 0) {
        *out = res.release();
        return DPQ_OK;
    }
    DPQ_HIP(hipSetDevice(f->device));
    const int qb = std::min(nq, kFlatRangeQueries);
    int rc = grow(f->state, &f->state_n, (size_t)qb);
    if (!rc) rc = flat_grow_queries<Q>(f, metric, (size_t)qb);
    if (!rc) rc = grow(f->r_thr, &f->r_thr_n, (size_t)qb);
    if (!rc) rc = grow(f->r_offs, &f->r_offs_n, (size_t)qb + 1);
    if (rc) return rc;
    std::vector<float> padded;
    std::vector<dpq::FlatQueryState> st((size_t)qb);
    std::vector<uint64_t> thr((size_t)qb), sorted;
    std::vector<int64_t> offs;
    for (int q0 = 0; q0 < nq && !rc; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        if ((rc = flat_stage_queries(f, metric, queries + (size_t)q0 * flat_query_elems(f), m, &padded))) break;
        for (int q = 0; q < m; ++q) {  // d < r on non-negative floats is bits(d) < bits(r); key 0 lets nothing pass
            const float r = radii[q0 + q];
            uint32_t bits = 0;
            if (metric == dpq::kFlatIP) {  // s > r is word(s) < word(r): the map descends, and -0.0 is read as +0.0
                memcpy(&bits, &r, sizeof bits);
                bits = dpq::flat_ip_word(bits);
            } else if (r > 0.0f) {
                memcpy(&bits, &r, sizeof bits);
            }
            thr[(size_t)q] = (uint64_t)bits << 32;
        }
        DPQ_HIP(hipMemcpy(f->r_thr, thr.data(), (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice));
        if ((rc = flat_range_pass(f, ff, metric, 0, m, nullptr))) break;
        DPQ_HIP(hipMemcpy(st.data(), f->state, (size_t)m * sizeof(dpq::FlatQueryState), hipMemcpyDeviceToHost));
        for (int q = 0; q < m; ++q) res->lims[(size_t)q0 + q + 1] = res->lims[(size_t)q0 + q] + st[(size_t)q].count;
        res->ids.resize((size_t)res->lims[(size_t)q0 + m]);
        res->dists.resize((size_t)res->lims[(size_t)q0 + m]);
        for (int a = 0; a < m && !rc;) {
            int b = a;
            int64_t sum = 0;
            while (b < m && (b == a || sum + st[(size_t)b].count <= kFlatRangePoolKeys)) sum += st[(size_t)b++].count;
            if (sum > 0) {
                offs.assign(1, 0);
                for (int q = a; q < b; ++q) offs.push_back(offs.back() + st[(size_t)q].count);
                if ((rc = grow(f->r_pool, &f->r_pool_n, (size_t)std::max(sum, kFlatRangePoolKeys)))) break;
                if ((rc = grow(f->r_sorted, &f->r_sorted_n, f->r_pool_n))) break;
                DPQ_HIP(hipMemcpy(f->r_offs, offs.data(), offs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
                if ((rc = flat_range_pass(f, ff, metric, a, b - a, f->r_pool))) break;
                size_t tb = 0;
                DPQ_HIP(dpq::flat_range_sort(nullptr, &tb, f->r_pool, f->r_sorted, sum, b - a, f->r_offs, nullptr));
                DevBuf<uint8_t> temp;  // the segmented sort's workspace
                if ((rc = temp.alloc(tb))) break;
                DPQ_HIP(dpq::flat_range_sort(temp, &tb, f->r_pool, f->r_sorted, sum, b - a, f->r_offs, nullptr));
                sorted.resize((size_t)sum);
                DPQ_HIP(hipMemcpy(sorted.data(), f->r_sorted, (size_t)sum * sizeof(uint64_t), hipMemcpyDeviceToHost));
                std::vector<dpq::FlatQueryState> st2((size_t)(b - a));
                DPQ_HIP(hipMemcpy(st2.data(), f->state.get() + a, st2.size() * sizeof(dpq::FlatQueryState), hipMemcpyDeviceToHost));
                for (int q = a; q < b; ++q)
                    if (st2[(size_t)(q - a)].overflow || st2[(size_t)(q - a)].count != st[(size_t)q].count)
                        rc = fail(DPQ_ERR_STATE, who + ": internal error: the two passes disagree on the length of a list");
                if (rc) break;
                const size_t at = (size_t)res->lims[(size_t)q0 + a];
                for (size_t i = 0; i < (size_t)sum; ++i) {
                    uint32_t bits = (uint32_t)(sorted[i] >> 32);
                    if (metric == dpq::kFlatIP) bits = dpq::flat_ip_word(bits);
                    res->ids[at + i] = (int32_t)(uint32_t)sorted[i];
                    memcpy(&res->dists[at + i], &bits, sizeof bits);
                }
            }
            a = b;
        }
    }
    if (f->r_pool_n > (size_t)kFlatRangePoolKeys) {  // a list longer than the pool: give the larger buffers back
        f->r_pool.reset();
        f->r_sorted.reset();
        f->r_pool_n = f->r_sorted_n = 0;
    }
    if (rc) return rc;
    *out = res.release();
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_flat_filter_create(dpq_flat* f, const uint32_t* words, int64_t n_bits, dpq_flat_filter** out) {
    return guarded([&]() -> int {
    const std::string who("dpq_flat_filter_create");
    if (!out) return fail(DPQ_ERR_ARG, who + ": out is NULL");
    *out = nullptr;
    if (!f || n_bits < 0 || (n_bits > 0 && !words)) return fail(DPQ_ERR_ARG, who + ": NULL argument or n_bits < 0");
    if (int rc = flat_device_present(who)) return rc;
    DPQ_HIP(hipSetDevice(f->device));
    // bit b of local word w = row 32 w + b = the caller's bit of the reported id row + id_offset
    const int64_t n_words = (f->n + 31) / 32;
    std::vector<uint32_t> h((size_t)n_words);
    for (int64_t w = 0; w < n_words; ++w) {
        uint32_t v = bitmap_bits32(words, n_bits, f->id_offset + 32 * w);
        if (f->n - 32 * w < 32) v &= (1u << (f->n - 32 * w)) - 1u;
        h[(size_t)w] = v;
    }
    std::unique_ptr<dpq_flat_filter> ff(new dpq_flat_filter());
    ff->owner = f->serial;
    ff->device = f->device;
    DevBuf<uint32_t> d_words, d_cnt, d_off, d_flag;
    int rc = d_words.alloc((size_t)n_words);
    if (!rc) rc = d_cnt.alloc((size_t)n_words);
    if (!rc) rc = d_off.alloc((size_t)n_words);
    if (!rc) rc = d_flag.alloc(1);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(d_words, h.data(), (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    DPQ_HIP(hipMemset(d_flag, 0, sizeof(uint32_t)));
    DPQ_HIP(dpq::flat_filter_count(d_words, n_words, d_cnt, d_off, &ff->n_allowed, nullptr));
    if (ff->n_allowed < 0 || ff->n_allowed > f->n) return fail(DPQ_ERR_STATE, who + ": internal error: bad row count");
    if ((rc = ff->list.alloc((size_t)ff->n_allowed))) return rc;
    DPQ_HIP(dpq::launch_flat_filter_emit(d_words, n_words, d_off, ff->list, ff->n_allowed, d_flag, nullptr));
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpy(&bad, d_flag, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) return fail(DPQ_ERR_STATE, who + ": internal error: the row list overflowed");
    *out = ff.release();
    return DPQ_OK;
    });
}

void dpq_flat_filter_free(dpq_flat_filter* ff) {
    if (!ff) return;
    hipSetDevice(ff->device);
    delete ff;
}

int dpq_flat_filter_count(const dpq_flat_filter* ff, int64_t* n_allowed) {
    if (!ff || !n_allowed) return fail(DPQ_ERR_ARG, "dpq_flat_filter_count: NULL argument");
    *n_allowed = ff->n_allowed;
    return DPQ_OK;
}

int dpq_flat_search_filtered(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, int top_k, int32_t* ids,
                             float* dists) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatL2, dpq::kFlatF32}, f, ff, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_filtered_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k, int32_t* ids,
                                float* dists) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatL2, dpq::kFlatU8}, f, ff, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_filtered_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, int top_k, int32_t* ids,
                                float* dists) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatL2, dpq::kFlatI8}, f, ff, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_filtered_bits(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k,
                                  int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatL2, dpq::kFlatBits}, f, ff, as_bits(queries), nq, top_k, ids,
                                     dists);
    });
}

int dpq_flat_range_search_bits(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, const float* radii,
                               dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatL2, dpq::kFlatBits}, f, ff, as_bits(queries), nq, radii, out);
    });
}

int dpq_flat_search_filtered_ip(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, int top_k, int32_t* ids,
                                float* scores) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatIP, dpq::kFlatF32}, f, ff, queries, nq, top_k, ids, scores);
    });
}

int dpq_flat_search_filtered_ip_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k, int32_t* ids,
                                   float* scores) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatIP, dpq::kFlatU8}, f, ff, queries, nq, top_k, ids, scores);
    });
}

int dpq_flat_search_filtered_ip_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, int top_k, int32_t* ids,
                                   float* scores) {
    return guarded([&]() -> int {
    return flat_search_filtered_call({"dpq_flat_search_filtered", dpq::kFlatIP, dpq::kFlatI8}, f, ff, queries, nq, top_k, ids, scores);
    });
}

int dpq_flat_range_search(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, const float* radii,
                          dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatL2, dpq::kFlatF32}, f, ff, queries, nq, radii, out);
    });
}

int dpq_flat_range_search_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, const float* radii,
                             dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatL2, dpq::kFlatU8}, f, ff, queries, nq, radii, out);
    });
}

int dpq_flat_range_search_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, const float* radii,
                             dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatL2, dpq::kFlatI8}, f, ff, queries, nq, radii, out);
    });
}

int dpq_flat_range_search_ip(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, const float* thresholds,
                             dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatIP, dpq::kFlatF32}, f, ff, queries, nq, thresholds, out);
    });
}

int dpq_flat_range_search_ip_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, const float* thresholds,
                                dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatIP, dpq::kFlatU8}, f, ff, queries, nq, thresholds, out);
    });
}

int dpq_flat_range_search_ip_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, const float* thresholds,
                                dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call({"dpq_flat_range_search", dpq::kFlatIP, dpq::kFlatI8}, f, ff, queries, nq, thresholds, out);
    });
}

}  // extern "C"

namespace {

// dpq_flat_rerank_device and its _ip / _u8 / _i8 forms: Q is the query type of the call's kind.
template <class Q>
int flat_rerank_device_call(const FlatCall& c, dpq_flat* f, const Q* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                            int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    int rc = flat_rerank_args(c, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids, d_dists);
    if (rc || nq == 0) return rc;
    DPQ_HIP(hipSetDevice(f->device));
    return flat_rerank_on_device(c.name().c_str(), c.metric, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids, d_dists,
                                 (hipStream_t)hip_stream);
}

// dpq_flat_rerank and its _ip / _u8 / _i8 forms: the candidates are checked on the host, then queries and candidates go
// up and the answer down.
template <class Q>
int flat_rerank_host_call(const FlatCall& c, dpq_flat* f, const Q* queries, int nq, const int32_t* cand_ids, int n_cand,
                          int top_k, int32_t* ids, float* dists) {
    constexpr bool bytes = format_of<Q> != dpq::kFlatF32;
    const std::string who = c.name();
    const char* fn = who.c_str();
    int rc = flat_rerank_args(c, f, queries, nq, cand_ids, n_cand, top_k, ids, dists);
    if (rc || nq == 0) return rc;
    const int64_t n_map = (int64_t)f->h_map.size();
    for (size_t i = 0; i < (size_t)nq * n_cand; ++i) {
        const int64_t c = cand_ids[i];
        if (c < 0) continue;
        bool ok;
        if (n_map)
            ok = c < n_map || (c == n_map && (n_map & 1) == 0);
        else
            ok = c - f->id_offset >= 0 && c - f->id_offset < f->n;
        if (!ok) return fail(DPQ_ERR_ARG, std::string(fn) + ": a candidate names no row of this handle");
    }
    DPQ_HIP(hipSetDevice(f->device));
    Q* d_q;
    if constexpr (bytes) {
        rc = grow(f->q_raw, &f->q_raw_n, (size_t)nq * flat_query_elems(f));
        d_q = reinterpret_cast<Q*>(f->q_raw.get());
    } else {
        rc = grow(f->d_q, &f->q_n, (size_t)nq * f->D);
        d_q = f->d_q;
    }
    if (!rc) rc = grow(f->d_cand, &f->cand_n, (size_t)nq * n_cand);
    if (!rc) rc = grow_outputs(f, (size_t)nq * top_k);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(d_q, queries, (size_t)nq * flat_query_elems(f) * sizeof(Q), hipMemcpyHostToDevice));
    DPQ_HIP(hipMemcpy(f->d_cand, cand_ids, (size_t)nq * n_cand * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = flat_rerank_on_device(fn, c.metric, f, d_q, nq, f->d_cand, n_cand, top_k, f->d_ids, f->d_dists, nullptr);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(ids, f->d_ids, (size_t)nq * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, f->d_dists, (size_t)nq * top_k * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_flat_rerank(dpq_flat* f, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                    int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatF32}, f, queries, nq, cand_ids, n_cand, top_k, ids, dists);
    });
}

int dpq_flat_rerank_device(dpq_flat* f, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                           int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatF32, true}, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                                   d_dists, hip_stream);
    });
}

int dpq_flat_rerank_u8(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                       int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatU8}, f, queries, nq, cand_ids, n_cand, top_k, ids, dists);
    });
}

int dpq_flat_rerank_u8_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                              int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatU8, true}, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                                   d_dists, hip_stream);
    });
}

int dpq_flat_rerank_i8(dpq_flat* f, const int8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                       int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatI8}, f, queries, nq, cand_ids, n_cand, top_k, ids, dists);
    });
}

int dpq_flat_rerank_i8_device(dpq_flat* f, const int8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                              int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatI8, true}, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                                   d_dists, hip_stream);
    });
}

int dpq_flat_rerank_bits(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                         int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatBits}, f, as_bits(queries), nq, cand_ids, n_cand, top_k, ids,
                                 dists);
    });
}

int dpq_flat_rerank_bits_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatL2, dpq::kFlatBits, true}, f, as_bits(d_queries), nq, d_cand_ids, n_cand,
                                   top_k, d_ids, d_dists, hip_stream);
    });
}

int dpq_flat_rerank_ip(dpq_flat* f, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                       int32_t* ids, float* scores) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatIP, dpq::kFlatF32}, f, queries, nq, cand_ids, n_cand, top_k, ids, scores);
    });
}

int dpq_flat_rerank_ip_device(dpq_flat* f, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                              int top_k, int32_t* d_ids, float* d_scores, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatIP, dpq::kFlatF32, true}, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                                   d_scores, hip_stream);
    });
}

int dpq_flat_rerank_ip_u8(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                          int32_t* ids, float* scores) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatIP, dpq::kFlatU8}, f, queries, nq, cand_ids, n_cand, top_k, ids, scores);
    });
}

int dpq_flat_rerank_ip_u8_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                 int top_k, int32_t* d_ids, float* d_scores, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatIP, dpq::kFlatU8, true}, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                                   d_scores, hip_stream);
    });
}

int dpq_flat_rerank_ip_i8(dpq_flat* f, const int8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                          int32_t* ids, float* scores) {
    return guarded([&]() -> int {
    return flat_rerank_host_call({"dpq_flat_rerank", dpq::kFlatIP, dpq::kFlatI8}, f, queries, nq, cand_ids, n_cand, top_k, ids, scores);
    });
}

int dpq_flat_rerank_ip_i8_device(dpq_flat* f, const int8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                 int top_k, int32_t* d_ids, float* d_scores, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call({"dpq_flat_rerank", dpq::kFlatIP, dpq::kFlatI8, true}, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                                   d_scores, hip_stream);
    });
}

int dpq_merge_topk_ip_host(const int32_t* ids, const float* scores, int n_lists, int nq, int top_k, int32_t* out_ids,
                           float* out_scores) {
    return guarded([&]() -> int {
    if (!ids || !scores || !out_ids || !out_scores || n_lists < 1 || nq < 0 || top_k < 1)
        return fail(DPQ_ERR_ARG, "dpq_merge_topk_ip_host: NULL argument, n_lists < 1, nq < 0 or top_k < 1");
    std::vector<uint64_t> keys;
    for (int q = 0; q < nq; ++q) {
        keys.clear();
        for (int l = 0; l < n_lists; ++l)
            for (int r = 0; r < top_k; ++r) {
                const size_t o = ((size_t)l * nq + q) * top_k + r;
                if (ids[o] < 0) continue;
                uint32_t bits;
                memcpy(&bits, &scores[o], 4);
                keys.push_back(((uint64_t)dpq::flat_ip_word(bits) << 32) | (uint32_t)ids[o]);
            }
        const size_t kk = std::min((size_t)top_k, keys.size());
        std::partial_sort(keys.begin(), keys.begin() + kk, keys.end());
        for (int r = 0; r < top_k; ++r) {
            const size_t o = (size_t)q * top_k + r;
            if ((size_t)r < kk) {
                out_ids[o] = (int32_t)(keys[r] & 0xffffffffu);
                const uint32_t bits = dpq::flat_ip_word((uint32_t)(keys[r] >> 32));
                memcpy(&out_scores[o], &bits, 4);
            } else {
                out_ids[o] = -1;
                out_scores[o] = -INFINITY;
            }
        }
    }
    return DPQ_OK;
    });
}

}  // extern "C"
