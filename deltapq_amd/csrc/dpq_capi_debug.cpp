// dpq_capi_debug.cpp -- the developer hooks of include/deltapq_amd.h (dpq_debug_*): timings, marks and dumps of what
// the last batch left in the handle.  Live only in a process started with DPQ_DEV=1; no query path calls them.
#include "dpq_capi_internal.h"

namespace {

// The full-index filter scan of the dpq_debug_scan_* hooks: nq slots of the active workspace with the thresholds and
// tables the last batch left behind (at most DPQ_DEBUG_NSEG segments); *splits <= 0 becomes splits_for's.
dpq::ScanArgs debug_scan_args(const dpq_index* x, int nq, int* splits) {
    const Workspace& w = x->ws();
    const int QG = dpq::queries_per_group(x->M);
    dpq::ScanArgs sa{};
    sa.img = x->img;
    sa.fp32_accum = x->plain ? 1 : 0;
    sa.lut32 = w.d_lut32;
    sa.lut_min = w.d_lut_min;
    sa.lut_stat = w.d_lut_stat;
    sa.thr_key = w.d_thr_key;
    sa.slot_query = nullptr;
    sa.n_queries = nq;
    sa.seg_list = nullptr;
    sa.n_seg_pass = x->img.n_segments;
    if (const char* e = getenv("DPQ_DEBUG_NSEG")) sa.n_seg_pass = std::min(x->img.n_segments, atoi(e));
    if (*splits <= 0) *splits = splits_for(sa.n_seg_pass, (nq + QG - 1) / QG);
    sa.cand_count = w.d_cand_count;
    sa.cand_key = w.d_cand_key;
    sa.cand_stride = w.cap;
    sa.region_off = 0;
    sa.region_cap = std::max(1, w.cap / *splits);
    sa.qtab = w.d_qtab;
    return sa;
}

}  // namespace

extern "C" {

// Developer hook: time `reps` full-index filter-scan
// launches for nq query slots with the filter pinned (pass_all == 0: nothing
// survives; 1: everything survives), to separate decode/ADC cost from
// candidate handling.  Needs a prior dpq_query_batch* call with >= nq queries.
int dpq_debug_scan_time(dpq_index* x, int nq, int pass_all, int reps, int splits, float* ms_out) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !ms_out || !x->ws().d_lut32) return fail(DPQ_ERR_STATE, "run a query batch first");
    DPQ_HIP(hipSetDevice(x->device));
    if (pass_all == 3) {
        // the last batch's first filter level exactly as it ran: its bootstrap again (thresholds + tables), then `reps`
        // timed launches of its scan
        if (x->dbg_groups <= 0 || x->dbg_boot_slots <= 0) return fail(DPQ_ERR_STATE, "the last batch ran no bootstrap + scan");
        hipEvent_t a, b;
        DPQ_HIP(hipEventCreate(&a));
        DPQ_HIP(hipEventCreate(&b));
        DPQ_HIP(dpq::launch_bootstrap(x->dbg_ba, x->M, x->dbg_boot_slots, nullptr));
        DPQ_HIP(dpq::launch_scan(x->dbg_sa, x->dbg_groups, x->dbg_splits, nullptr));
        DPQ_HIP(hipEventRecord(a, nullptr));
        for (int r = 0; r < reps; ++r) {
            // every launch starts its in-scan tightening from empty histograms, as a batch's first level does (the fill
            // is a 1-2 us kernel inside the timed region)
            if (x->dbg_sa.tight_hist)
                DPQ_HIP(hipMemsetAsync(x->dbg_sa.tight_hist, 0, sizeof(uint32_t) * dpq::kTightWords * (size_t)x->dbg_boot_slots, nullptr));
            DPQ_HIP(dpq::launch_scan(x->dbg_sa, x->dbg_groups, x->dbg_splits, nullptr));
        }
        DPQ_HIP(hipEventRecord(b, nullptr));
        DPQ_HIP(hipEventSynchronize(b));
        float ms = 0;
        DPQ_HIP(hipEventElapsedTime(&ms, a, b));
        *ms_out = ms / reps;
        hipEventDestroy(a);
        hipEventDestroy(b);
        return DPQ_OK;
    }
    const int QG = dpq::queries_per_group(x->M);
    const int nqp = (nq + QG - 1) / QG * QG;
    const Workspace& w = x->ws();
    if (nqp > w.slots) return fail(DPQ_ERR_ARG, "nq exceeds the workspace");
    dpq::ScanArgs sa = debug_scan_args(x, nq, &splits);
    sa.debug_pass = pass_all == 2 ? 0 : (pass_all ? 2 : 1);  // 2: the thresholds the last batch left behind
    // what the last batch ran: its plain-code scratch, if it decoded the whole shard into one
    if (!x->plain && x->image_state != 0 && !getenv("DPQ_DEBUG_FUSED")) {
        if (x->image_state == 1) {  // (this replay runs on the null stream: the image must be there)
            DPQ_HIP(hipEventSynchronize(x->image_done));
            x->image_state = 2;
        }
        sa.img.raw = x->d_plain_image;
        if (x->d_relabel) sa.lut32 = w.d_lut32r;
    }
    hipEvent_t a, b;
    DPQ_HIP(hipEventCreate(&a));
    DPQ_HIP(hipEventCreate(&b));
    DPQ_HIP(dpq::launch_quantise(sa, nqp / QG, nullptr));
    DPQ_HIP(dpq::launch_scan(sa, nqp / QG, splits, nullptr));
    DPQ_HIP(hipEventRecord(a, nullptr));
    for (int r = 0; r < reps; ++r) DPQ_HIP(dpq::launch_scan(sa, nqp / QG, splits, nullptr));
    DPQ_HIP(hipEventRecord(b, nullptr));
    DPQ_HIP(hipEventSynchronize(b));
    float ms = 0;
    DPQ_HIP(hipEventElapsedTime(&ms, a, b));
    *ms_out = ms / reps;
    hipEventDestroy(a);
    hipEventDestroy(b);
    if (getenv("DPQ_DEBUG_WG_TIMES")) {  // when do the workgroups of one launch start and end?
        const int nwg = splits * (nqp / QG);
        DevBuf<unsigned long long> d_t;
        int rc = d_t.alloc((size_t)nwg * 2);
        if (rc) return rc;
        sa.wg_times = d_t;
        DPQ_HIP(dpq::launch_scan(sa, nqp / QG, splits, nullptr));
        DPQ_HIP(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)nwg * 2);
        DPQ_HIP(hipMemcpy(h.data(), d_t, h.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0;
        for (int i = 0; i < nwg; ++i) t0 = std::min(t0, h[2 * (size_t)i]), t1 = std::max(t1, h[2 * (size_t)i + 1]);
        std::vector<double> st, en, life;
        for (int i = 0; i < nwg; ++i) {
            st.push_back((double)(h[2 * (size_t)i] - t0) / 100.0);
            en.push_back((double)(h[2 * (size_t)i + 1] - t0) / 100.0);
            life.push_back(en.back() - st.back());
        }
        std::sort(st.begin(), st.end()); std::sort(en.begin(), en.end()); std::sort(life.begin(), life.end());
        auto pct = [&](const std::vector<double>& v, double p) { return v[(size_t)(p * (v.size() - 1))]; };
        fprintf(stderr, "scan workgroups (%d, %s codes): span %.1f us; start p50 %.1f max %.1f; end min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f; "
                        "lifetime min %.1f p50 %.1f max %.1f us; busy %.1f %%\n", nwg, sa.img.raw ? "plain" : "compressed",
                (double)(t1 - t0) / 100.0, pct(st, 0.5), st.back(), en.front(), pct(en, 0.1), pct(en, 0.5), pct(en, 0.9), en.back(),
                life.front(), pct(life, 0.5), life.back(),
                100.0 * std::accumulate(life.begin(), life.end(), 0.0) / (nwg * (double)(t1 - t0) / 100.0));
    }
    return DPQ_OK;
    });
}

// Developer hook (not in the public header): one full-index filter-scan launch of the STAMPS build of the
// scan kernel (s_memtime brackets around the sections of the loop) with the thresholds the last batch
// left behind; out[0..n) = per-section cycle sums over all wavefronts (order: enum in dpq_kernels.hip).
int dpq_debug_scan_stamps(dpq_index* x, int nq, int splits, unsigned long long* out, int n_out, float* ms_out) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !out || !x->ws().d_lut32) return fail(DPQ_ERR_STATE, "run a query batch first");
    if (x->M != 8) return fail(DPQ_ERR_ARG, "the STAMPS build exists for M = 8");
    DPQ_HIP(hipSetDevice(x->device));
    const int QG = dpq::queries_per_group(x->M);
    const int nqp = (nq + QG - 1) / QG * QG;
    if (nqp > x->ws().slots) return fail(DPQ_ERR_ARG, "nq exceeds the workspace");
    const int n = std::min(n_out, dpq::scan_stamp_count());
    DevBuf<unsigned long long> d_st;
    int rc = d_st.alloc((size_t)dpq::scan_stamp_count());
    if (rc) return rc;
    DPQ_HIP(hipMemset(d_st, 0, sizeof(unsigned long long) * dpq::scan_stamp_count()));
    dpq::ScanArgs sa = debug_scan_args(x, nq, &splits);
    sa.stamps = d_st;
    hipEvent_t a, b;
    DPQ_HIP(hipEventCreate(&a));
    DPQ_HIP(hipEventCreate(&b));
    DPQ_HIP(dpq::launch_quantise(sa, nqp / QG, nullptr));
    DPQ_HIP(hipEventRecord(a, nullptr));
    DPQ_HIP(dpq::launch_scan(sa, nqp / QG, splits, nullptr));
    DPQ_HIP(hipEventRecord(b, nullptr));
    DPQ_HIP(hipEventSynchronize(b));
    float ms = 0;
    DPQ_HIP(hipEventElapsedTime(&ms, a, b));
    if (ms_out) *ms_out = ms;
    DPQ_HIP(hipMemcpy(out, d_st, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    hipEventDestroy(a);
    hipEventDestroy(b);
    return DPQ_OK;
    });
}

// Developer hook: per-wavefront marks of strand1_kernel (100 MHz clock): [256 workgroups][16 wavefronts][16 marks] =
// start, end of the prologue, end of each of the wavefront's first strips.  First call arms it; later calls copy out
// the marks of the last one-query call on a strand image.
int dpq_debug_strand1_stamps(dpq_index* x, unsigned long long* out, int n_words) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !out) return fail(DPQ_ERR_ARG, "NULL argument");
    DPQ_HIP(hipSetDevice(x->device));
    const size_t total = (size_t)256 * 16 * 16;
    if (!x->d_s1_stamps) {
        int rc = x->d_s1_stamps.alloc(total);
        if (rc) return rc;
        DPQ_HIP(hipMemset(x->d_s1_stamps, 0, total * 8));
        return DPQ_OK;
    }
    DPQ_HIP(hipDeviceSynchronize());
    DPQ_HIP(hipMemcpy(out, x->d_s1_stamps, std::min((size_t)std::max(n_words, 0), total) * 8, hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemset(x->d_s1_stamps, 0, total * 8));
    return DPQ_OK;
    });
}

// Developer hook: phase marks of the bootstrap kernel.  First call arms it
// (allocates [2048][8] marks); later calls return the mean cycles between consecutive marks over `nq` slots
// of the last batch: out[0] rank, [1] cell counts + prefix, [2] node evaluation, [3] k-th key select.
int dpq_debug_boot_stamps(dpq_index* x, int nq, double* out) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !out) return fail(DPQ_ERR_ARG, "NULL argument");
    DPQ_HIP(hipSetDevice(x->device));
    if (!x->d_boot_stamps) {
        int rc = x->d_boot_stamps.alloc((size_t)kMaxBatchQueries * 16);
        if (rc) return rc;
        DPQ_HIP(hipMemset(x->d_boot_stamps, 0, sizeof(unsigned long long) * kMaxBatchQueries * 16));
        for (int i = 0; i < 8; ++i) out[i] = 0;
        return DPQ_OK;
    }
    DPQ_HIP(hipDeviceSynchronize());
    std::vector<unsigned long long> h((size_t)kMaxBatchQueries * 16);
    DPQ_HIP(hipMemcpy(h.data(), x->d_boot_stamps, h.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out[i] = 0;
    nq = std::min(nq, kMaxBatchQueries);
    // out[0..3]: bootstrap (rank, cells, evaluate, select); out[4..7]: the last select launch (gather, k-th key,
    // winners, sort + output)
    for (int half = 0; half < 2; ++half) {
        // blocks on the 100 MHz chip-wide clock: first start -> last end, distribution of lifetimes and start offsets
        const size_t o = (size_t)half * kMaxBatchQueries * 8;
        unsigned long long t0 = ~0ull, t1 = 0;
        std::vector<double> life, start;
        for (int q = 0; q < nq; ++q) {
            t0 = std::min(t0, h[o + (size_t)q * 8 + 6]);
            t1 = std::max(t1, h[o + (size_t)q * 8 + 7]);
        }
        for (int q = 0; q < nq; ++q) {
            life.push_back((double)(h[o + (size_t)q * 8 + 7] - h[o + (size_t)q * 8 + 6]) / 100.0);
            start.push_back((double)(h[o + (size_t)q * 8 + 6] - t0) / 100.0);
        }
        std::sort(life.begin(), life.end());
        std::sort(start.begin(), start.end());
        auto pct = [&](const std::vector<double>& v, double p) { return v[(size_t)(p * (v.size() - 1))]; };
        fprintf(stderr, "%s blocks: span %.2f us; lifetime min %.2f median %.2f p90 %.2f max %.2f us; start offset median %.2f p90 %.2f max %.2f us\n",
                half ? "select" : "bootstrap", (double)(t1 - t0) / 100.0, life.front(), pct(life, 0.5), pct(life, 0.9), life.back(),
                pct(start, 0.5), pct(start, 0.9), start.back());
        if (!half) {  // bootstrap blocks by the rounds of cells they walked (slot 5 of a block's stamps)
            double sum[4] = {0, 0, 0, 0}, mx[4] = {0, 0, 0, 0};
            int cnt[4] = {0, 0, 0, 0};
            for (int q = 0; q < nq; ++q) {
                const int r = (int)std::min<unsigned long long>(h[o + (size_t)q * 8 + 5], 4) - 1;
                if (r < 0) continue;
                const double l = (double)(h[o + (size_t)q * 8 + 7] - h[o + (size_t)q * 8 + 6]) / 100.0;
                sum[r] += l, mx[r] = std::max(mx[r], l), cnt[r]++;
            }
            for (int r = 0; r < 4; ++r)
                if (cnt[r]) fprintf(stderr, "  %d%s round(s): %d blocks, lifetime mean %.2f max %.2f us\n", r + 1, r == 3 ? "+" : "", cnt[r], sum[r] / cnt[r], mx[r]);
        }
    }
    for (int half = 0; half < 2; ++half)
        for (int q = 0; q < nq; ++q)
            for (int i = 0; i < 4; ++i) {
                const size_t o = (size_t)half * kMaxBatchQueries * 8 + (size_t)q * 8;
                out[4 * half + i] += (double)(h[o + i + 1] - h[o + i]) / nq;
            }
    return DPQ_OK;
    });
}

// Developer hook: the first filter level's tables of the last batch answered on `lane`, as the scan copies them into
// LDS ([group][g][m][code] x 16 B), followed at M = 8 by one 16-byte record per slot (8 saturation bytes, the u64
// threshold key the fields were built from) -- recomputed here by saturation_debug_kernel from the thresholds the
// batch saved before its first level (a batch run with DPQ_DEV=1).  Waits for the device.
int dpq_debug_filter_tables(dpq_index* x, int lane, void* out, int64_t bytes) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !out || lane < 0 || lane > 1) return fail(DPQ_ERR_ARG, "bad argument");
    const Workspace& w = x->lane[lane];
    if (!w.d_qtab || w.dbg_qtab_groups <= 0 || w.dbg_qtab_levels != 1)
        return fail(DPQ_ERR_STATE, "the lane's last batch did not leave one filter level's tables");
    const int slots = w.dbg_qtab_groups * dpq::queries_per_group(x->M);
    const size_t tables = (size_t)w.dbg_qtab_groups * dpq::qtab_bytes_per_group(x->M);
    const size_t records = x->M == 8 ? (size_t)slots * 16 : 0;
    if (records && w.dbg_qtab_nq <= 0) return fail(DPQ_ERR_STATE, "the batch did not run with DPQ_DEV=1: no thresholds saved");
    if (bytes < (int64_t)(tables + records)) return fail(DPQ_ERR_ARG, "the buffer is smaller than the tables");
    DPQ_HIP(hipSetDevice(x->device));
    DPQ_HIP(hipDeviceSynchronize());
    DPQ_HIP(hipMemcpy(out, w.d_qtab.get(), tables, hipMemcpyDeviceToHost));
    if (records) {
        DevBuf<unsigned char> d_rec;
        int rc;
        if ((rc = d_rec.alloc(records))) return rc;
        dpq::ScanArgs sa{};
        sa.img.M = x->M;
        sa.lut_min = w.d_lut_min;
        sa.lut_stat = w.d_lut_stat;
        sa.thr_key = w.d_dbg_thr;
        sa.n_queries = w.dbg_qtab_nq;
        DPQ_HIP(dpq::launch_saturation_debug(sa, slots, d_rec, nullptr));
        DPQ_HIP(hipMemcpy(static_cast<char*>(out) + tables, d_rec.get(), records, hipMemcpyDeviceToHost));
    }
    return DPQ_OK;
    });
}

// Developer hook: the code value -> label map of the plain-code scratch ([M][256] bytes; the rows of a scratch batch's
// filter tables stand in label order).  DPQ_ERR_STATE: the handle has none (labels are code values).
int dpq_debug_relabel(dpq_index* x, unsigned char* out, int bytes) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !out || bytes < x->M * 256) return fail(DPQ_ERR_ARG, "bad argument");
    if (!x->d_relabel) return fail(DPQ_ERR_STATE, "the handle has no label map");
    DPQ_HIP(hipSetDevice(x->device));
    DPQ_HIP(hipDeviceSynchronize());
    DPQ_HIP(hipMemcpy(out, x->d_relabel.get(), (size_t)x->M * 256, hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

// Developer hook: candidate keys the largest scan launch of the last dpq_range_search laid out.
int dpq_debug_range_keys(dpq_index* x, int64_t* max_keys) {
    DPQ_DEV_ONLY();
    if (!x || !max_keys) return fail(DPQ_ERR_ARG, "NULL argument");
    *max_keys = x->range.last_max_keys;
    return DPQ_OK;
}

int dpq_debug_select_time(dpq_index* x, int nq, int top_k, int flags, int reps, float* ms_out) {
    return guarded([&]() -> int {
    DPQ_DEV_ONLY();
    if (!x || !ms_out || !x->ws().d_lut32 || !x->d_l0_id) return fail(DPQ_ERR_STATE, "run a query batch first");
    DPQ_HIP(hipSetDevice(x->device));
    const Workspace& w = x->ws();
    dpq::SelectArgs se{};
    se.shared_id = x->d_l0_id;
    se.shared_code = x->d_l0_code;
    se.shared_n = x->l0_segments * dpq::kChunk * x->img.chunks_per_segment;
    se.cand_count = w.d_cand_count;
    se.cand_key = w.d_cand_key;
    se.cand_stride = w.cap;
    se.region_off = top_k;
    se.scratch = w.d_scratch;
    se.lut32 = w.d_lut32;
    se.top_k = top_k;
    se.final_pass = 0;
    se.thr_key = w.d_thr_key;
    se.overflow = w.d_overflow;
    se.n_codes_total = x->img.n_codes_total;
    (void)flags;
    hipEvent_t a, b;
    DPQ_HIP(hipEventCreate(&a));
    DPQ_HIP(hipEventCreate(&b));
    DPQ_HIP(dpq::launch_select(se, x->M, nq, nullptr));
    DPQ_HIP(hipEventRecord(a, nullptr));
    for (int r = 0; r < reps; ++r) DPQ_HIP(dpq::launch_select(se, x->M, nq, nullptr));
    DPQ_HIP(hipEventRecord(b, nullptr));
    DPQ_HIP(hipEventSynchronize(b));
    float ms = 0;
    DPQ_HIP(hipEventElapsedTime(&ms, a, b));
    *ms_out = ms / reps;
    hipEventDestroy(a);
    hipEventDestroy(b);
    return DPQ_OK;
    });
}

}  // extern "C"
