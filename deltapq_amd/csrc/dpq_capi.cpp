// dpq_capi.cpp -- the core of the C-ABI of include/deltapq_amd.h: the error slot, index lifetime, the
// threshold-cascade driver around the scan/select kernels, range search and profiling.  The other entry points live by
// feature in dpq_capi_{io,train,flat,lookup,filter,refine,tables,debug}.cpp; dpq_capi_internal.h is what they share.
// Compiled with hipcc (HIP runtime calls only; kernels live in dpq_kernels.hip).
//
// There is no CPU implementation of the query in this library: every
// dpq_query_* call runs the HIP kernels or fails with an error code.
#include "dpq_capi_internal.h"

namespace {

thread_local std::string g_last_error;

}  // namespace

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

uint64_t next_index_serial() {
    static std::atomic<uint64_t> next{1};
    return next++;
}

bool dev_mode() {
    const char* dev = getenv("DPQ_DEV");
    return dev && atoi(dev) != 0;
}

namespace {

// dpq_open_opts -> Tuning.  The environment takes part only with DPQ_DEV=1 (developer sweeps: scripts/), and only
// here, once per dpq_open_*: a product process' plan never depends on its environment.
Tuning resolve_tuning(const dpq_open_opts& o) {
    Tuning t;
    if (o.stream_max_queries != 0) t.stream_max = std::min(16, std::max(0, o.stream_max_queries));  // (four queries per pass at most)
    if (o.coarse_below > 0) t.coarse_below = o.coarse_below;
    for (int i = 0; i < 3; ++i) t.plan_ratios[i] = o.plan_ratios[i];
    t.boot_cap = std::max(0, o.boot_cap);
    t.boot_target = std::max(0, o.boot_target);
    if (o.batch_tile_nodes > 0) t.batch_tile_nodes = o.batch_tile_nodes;
    t.relabel = !(o.flags & DPQ_OPT_NO_RELABEL);
    t.fuse_quantise = !(o.flags & DPQ_OPT_NO_FUSE_QUANTISE);
    t.async_overlap = !(o.flags & DPQ_OPT_NO_ASYNC_OVERLAP);
    t.boot_fullsort = (o.flags & DPQ_OPT_BOOT_FULLSORT) != 0;
    t.tighten = !(o.flags & DPQ_OPT_NO_TIGHTEN);
    t.strands = !(o.flags & DPQ_OPT_NO_STRANDS);
    t.force_strands = (o.flags & DPQ_OPT_FORCE_STRANDS) != 0;
    t.strand1 = !(o.flags & DPQ_OPT_NO_STRAND1);
    if (dev_mode()) {
        auto geti = [](const char* name, int* v) { if (const char* e = getenv(name)) *v = atoi(e); };
        geti("DPQ_STREAM_MAX_QUERIES", &t.stream_max);
        geti("DPQ_COARSE_BELOW", &t.coarse_below);
        if (const char* e = getenv("DPQ_PLAN_RATIOS")) sscanf(e, "%d,%d,%d", &t.plan_ratios[0], &t.plan_ratios[1], &t.plan_ratios[2]);
        geti("DPQ_BOOT_CAP", &t.boot_cap);
        geti("DPQ_BOOT_TARGET", &t.boot_target);
        geti("DPQ_BOOT_VARIANT", &t.boot_variant);
        if (const char* e = getenv("DPQ_BATCH_TILE_NODES")) t.batch_tile_nodes = std::max<int64_t>(1, atoll(e));
        int v = 1;
        geti("DPQ_RELABEL", &v); t.relabel = t.relabel && v != 0;
        v = 1; geti("DPQ_FUSE_QUANTISE", &v); t.fuse_quantise = t.fuse_quantise && v != 0;
        v = 1; geti("DPQ_ASYNC_OVERLAP", &v); t.async_overlap = t.async_overlap && v != 0;
        v = 0; geti("DPQ_BOOT_FULLSORT", &v); t.boot_fullsort = t.boot_fullsort || v != 0;
        v = 1; geti("DPQ_TIGHTEN", &v); t.tighten = t.tighten && v != 0;
        geti("DPQ_SELECT_THREADS", &t.select_threads);
        geti("DPQ_SELECT_FAST", &t.select_fast);
        v = 1; geti("DPQ_STRANDS", &v); t.strands = t.strands && v != 0;
        t.force_strands = t.force_strands || v == 2;
        v = 1; geti("DPQ_STRAND1", &v); t.strand1 = t.strand1 && v != 0;
        geti("DPQ_S1_DEBUG", &t.s1_debug);
    }
    return t;
}

// Makes `lane`'s workspace the active one.
void use_lane(dpq_index* x, int lane) {
    if (lane == x->active_lane) return;
    x->dbg_groups = x->dbg_boot_slots = 0;  // (dpq_debug_scan_time mode 3 replays launches of the ACTIVE workspace)
    x->active_lane = lane;
}

// Grows the active workspace to at least `slots` padded queries and `cap` candidates each (its plain-code scratch stays).
int ensure_workspace(dpq_index* x, int slots, int cap) {
    Workspace& w = x->ws();
    if (slots <= w.slots && cap <= w.cap) return DPQ_OK;
    slots = std::max(slots, w.slots);
    cap = std::max(cap, w.cap);
    x->dbg_groups = x->dbg_boot_slots = 0;  // the recorded launch arguments point into what is freed here
    DevBuf<uint8_t> batch_raw = std::move(w.d_batch_raw);
    w = Workspace();  // the old buffers go before the new ones are allocated
    w.d_batch_raw = std::move(batch_raw);
    int rc;
    if ((rc = w.d_lut32.alloc((size_t)slots * x->M * 256))) return rc;
    if (x->d_relabel && (rc = w.d_lut32r.alloc((size_t)slots * x->M * 256))) return rc;
    if ((rc = w.d_lut_min.alloc((size_t)slots * x->M * 4))) return rc;  // four partial minima per (query, m)
    if ((rc = w.d_lut_stat.alloc((size_t)slots * x->M))) return rc;
    if ((rc = w.d_qtab.alloc((size_t)(slots / dpq::queries_per_group(x->M) + 1) *
                             (dpq::qtab_bytes_per_group(x->M) / sizeof(uint4)))))
        return rc;
    if ((rc = w.d_cand_count.alloc((size_t)slots * dpq::kRegionStride))) return rc;
    if ((rc = w.d_cand_key.alloc((size_t)slots * cap))) return rc;
    if ((rc = w.d_scratch.alloc((size_t)slots * cap))) return rc;
    if ((rc = w.d_overflow.alloc((size_t)slots))) return rc;
    if ((rc = w.d_tight.alloc((size_t)slots * dpq::kTightWords))) return rc;
    if ((rc = w.d_thr_key.alloc((size_t)slots))) return rc;
    if ((rc = w.d_dbg_thr.alloc((size_t)slots))) return rc;
    if (!x->h_overflow) DPQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&x->h_overflow), sizeof(uint32_t) * 4096));
    if (!x->d_counters) {
        if ((rc = x->d_counters.alloc(2))) return rc;
        DPQ_HIP(hipMemset(x->d_counters, 0, 16));
    }
    if (!x->h_any) {
        DPQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&x->h_any), sizeof(uint32_t) * dpq_index::kFlagSlots,
                              hipHostMallocMapped));
        DPQ_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&x->d_any), x->h_any, 0));
    }
    w.slots = slots;
    w.cap = cap;
    return DPQ_OK;
}

// order[j] = j * P mod n with P ~ n / golden ratio and gcd(P, n) = 1: a low-discrepancy visiting order of 0 .. n - 1
// (every prefix is a spread-out sample)
std::vector<uint32_t> golden_order(int64_t n) {
    std::vector<uint32_t> order((size_t)n);
    int64_t P = std::max<int64_t>(1, (int64_t)((double)n * 0.6180339887498949));
    auto gcd = [](int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; };
    while (gcd(P, n) != 1) ++P;
    for (int64_t j = 0; j < n; ++j) order[(size_t)j] = (uint32_t)((j * P) % n);
    return order;
}

// x->d_order: the segments' low-discrepancy visiting order (the cascade's levels are slices of it)
int ensure_order(dpq_index* x) {
    const int64_t nseg = x->img.n_segments;
    if (x->d_order || nseg <= 0) return DPQ_OK;
    const std::vector<uint32_t> order = golden_order(nseg);
    int rc = x->d_order.alloc((size_t)nseg);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(x->d_order, order.data(), (size_t)nseg * sizeof(uint32_t), hipMemcpyHostToDevice));
    return DPQ_OK;
}

int auto_cap(int top_k) { return std::max(4096, 32 * top_k); }

// Progressive cascade plan.  Segments are visited in a low-discrepancy order
// (so every prefix is a spread-out sample of the DFS stream); level l covers
// order[bound[l-1] : bound[l]] -- every segment exactly once over the whole
// cascade.  Level 0 (<= 4096 nodes) is query independent: its segments are
// decoded once here and every query evaluates that list exactly.  Later levels
// are filter scans; expected survivors of level l = top_k * (bound[l]/bound[l-1] - 1).
// Small batches (coarse == 1) are bound by the fixed cost per level (a launch + a select), not by survivor
// handling, so they use steps of 16 and end up with three levels instead of five.
int ensure_plan(dpq_index* x, int top_k, int cap, int shape) {
    if (x->plan_top_k == top_k && x->plan_cap == cap && x->plan_coarse == shape) return DPQ_OK;
    const int coarse = shape & 1;
    const bool tight = (shape & 2) != 0;  // the scan tightens its thresholds as it goes (run_batch)
    const bool one_level = (shape & 4) != 0;  // one query per pass on the strand image: strand1_kernel tightens in the kernel
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    const int64_t nseg = x->img.n_segments;
    const int64_t s0 = std::min<int64_t>(nseg, std::max<int64_t>(1, dpq::kLevel0Nodes / S));
    std::vector<int64_t> bounds;
    if (x->boot) {
        // The bootstrap kernel delivers the first threshold (no segments consumed: level 0 is empty), as tight
        // as the k-th of a spread sample of a quarter of a 1 M-node index; the filter levels then cover ALL
        // segments.  One level up to 2 M nodes; beyond, levels growing by 8 (a larger shard's first threshold
        // admits more nodes in absolute terms); top_k > 512: see below.  dpq_open_opts.plan_ratios forces levels.
        bounds.push_back(nseg);
        std::vector<int> ratios;
        const int* forced = x->tune.plan_ratios;
        if (forced[0] >= 2) {
            for (int i = 0; i < 3; ++i)
                if (forced[i] >= 2) ratios.push_back(forced[i]);
        } else if (forced[0] == 1 || one_level) {
            // one level whatever the shard size (experiments; the one-query strand pass)
        } else {
            for (int64_t b = nseg; b * S > ((int64_t)2 << 20); b /= 8) ratios.push_back(8);
            // A large top_k takes its first threshold from a worse quantile of the bootstrap sample (the 1000th of
            // 8 K nodes): two short levels in front tighten it before the bulk of the index is filtered.  Measured
            // on 1 M codes (scripts/gpu_sweep_plans.sh): top-1000 1.40 M q/s with 3,3 against 0.95 M with one level
            // (M = 16: 0.79 M against 0.40 M); top-300 and below are fastest with one level.
            // With in-scan tightening the scan does that itself and one level wins again: top-1000 2.27 M q/s
            // against 1.89 M with 3,3 (M = 16: 1.27 M against 1.21 M), top-2048 1.19 M against 0.97 M.
            if (top_k > 512 && ratios.size() < 2 && !(tight && ratios.empty())) ratios = {3, 3};
        }
        int64_t b = nseg;
        for (int r : ratios) {
            b /= r;
            if (b < 1) break;
            bounds.push_back(b);
        }
        bounds.push_back(0);
        std::reverse(bounds.begin(), bounds.end());
    } else if (s0 >= nseg) {
        bounds.push_back(nseg);
    } else {
        bounds.push_back(nseg);
        // large batches: level sizes shrink by 4, 8, 8 from the full index down at top-100 (three filter levels
        // at 1 M codes); measured best trade between per-level fixed cost and survivor handling.
        // dpq_open_opts.plan_ratios overrides it for experiments.
        // A level costs a fixed ~45 us (scan prologue, launch, select) plus ~top_k * (ratio - 1) candidates per
        // query to check and select: the best ratio falls with top_k (measured: 8 at top-100, 3 at top-1000).
        const int r = (int)std::lround(std::min(16.0, std::max(2.0, 8.0 * std::sqrt(100.0 / (double)top_k))));
        int fine[] = {r >= 16 ? r : std::max(2, r / 2), r, r};  // few candidates (small top_k): the fewest levels win
        for (int i = 0; i < 3; ++i)
            if (x->tune.plan_ratios[i] >= 2) fine[i] = x->tune.plan_ratios[i];
        for (int& f : fine) f = std::max(2, f);
        // expected survivors of a level = top_k * (ratio - 1) must stay well inside the candidate buffer
        const int wide = (int)std::max<int64_t>(2, std::min<int64_t>(16, cap / (2 * (int64_t)top_k)));
        int64_t b = nseg;
        for (int i = 0;; ++i) {
            const int64_t nb = b / (coarse ? wide : fine[std::min(i, 2)]);
            if (nb < 2 * s0) break;
            bounds.push_back(nb);
            b = nb;
        }
        bounds.push_back(s0);
        std::reverse(bounds.begin(), bounds.end());
    }
    x->level_off.clear();
    x->level_cnt.clear();
    int64_t prev = 0;
    for (int64_t bnd : bounds) {
        x->level_off.push_back((int)prev);
        x->level_cnt.push_back((int)(bnd - prev));
        prev = bnd;
    }
    int rc0 = ensure_order(x);
    if (rc0) return rc0;
    if (!x->boot && nseg > 0 && x->l0_segments != (int)s0) {
        x->d_l0_code.reset();
        int rc = x->d_l0_id.alloc((size_t)(s0 * S));
        if (!rc) rc = x->d_l0_code.alloc((size_t)(s0 * S * (x->M / 4)));
        if (rc) return rc;
        DPQ_HIP(dpq::launch_decode_segments(x->img, x->d_order, (int)s0, x->d_l0_id, x->d_l0_code, nullptr));
        DPQ_HIP(hipStreamSynchronize(nullptr));
        x->l0_segments = (int)s0;
    }
    x->plan_top_k = top_k;
    x->plan_cap = cap;
    x->plan_coarse = shape;
    return DPQ_OK;
}

struct Timer {
    dpq_index* x;
    hipStream_t s;
    int kind;
    bool on;
    EventPair ep{};
    Timer(dpq_index* x_, hipStream_t s_, int kind_)
        : x(x_), s(s_), kind(kind_), on(x_->prof && (kind_ == 1 || !x_->prof_scan_only)) {
        if (on) {
            ep.kind = kind;
            ep.a = x->get_event();
            ep.b = x->get_event();
            if (!ep.a || !ep.b || hipEventRecord(ep.a, s) != hipSuccess) {
                x->prof_failed = true;
                if (ep.a) x->ev_pool.push_back(ep.a);
                if (ep.b) x->ev_pool.push_back(ep.b);
                on = false;
            }
        }
    }
    ~Timer() {
        if (on) {
            if (hipEventRecord(ep.b, s) != hipSuccess) x->prof_failed = true;
            x->events.push_back(ep);
        }
    }
};

// Plain-code scratch of a batch (per pipeline lane; a shard of one tile: the handle's resident image instead): one TILE of a filter level's segment list at a time -- decode the
// tile, scan it with every query group, next tile -- so the scratch stays Infinity-Cache-sized whatever the shard
// (16 M nodes = 128 MB at M = 8; the 1 M-code headline and a 12.5 M-code shard are one tile, a 125 M-code shard's
// last level eight).  dpq_open_opts.batch_tile_nodes overrides; dpq_open_opts.batch_decode >= 2 = tile of that many segments.
int64_t batch_tile_segments(const dpq_index* x) {
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    int64_t t = x->batch_decode >= 2 ? x->batch_decode : std::max<int64_t>(1, x->tune.batch_tile_nodes / S);
    return std::min<int64_t>(t, std::max<int64_t>(1, x->img.n_segments));
}
int64_t batch_raw_bytes(const dpq_index* x) {
    return batch_tile_segments(x) * dpq::kChunk * x->img.chunks_per_segment * x->M;
}
bool batch_decode_possible(const dpq_index* x) { return !x->plain && x->batch_decode >= 0 && x->img.n_segments > 0; }
bool use_batch_decode(const dpq_index* x, int n_groups) {
    return batch_decode_possible(x) && (x->batch_decode > 0 || n_groups >= 3);
}
// one tile holds the shard: its batches scan the handle's resident image, not a workspace's tile scratch
bool one_tile_shard(const dpq_index* x) { return batch_tile_segments(x) >= x->img.n_segments; }
int ensure_batch_raw(dpq_index* x) {
    if (one_tile_shard(x)) return DPQ_OK;  // (ensure_plain_image allocates with the decode)
    if (x->ws().d_batch_raw) return DPQ_OK;
    return x->ws().d_batch_raw.alloc((size_t)batch_raw_bytes(x));
}

// The resident plain-code image, valid for what is enqueued on `stream` after this call.  The first call decodes it on
// `stream` (timed as decode) and records image_done behind the decode; until the host has seen that event complete, a
// batch on another stream (the other lane, a caller's ordered stream, range search) waits for it.
int ensure_plain_image(dpq_index* x, hipStream_t stream) {
    if (x->image_state == 2) return DPQ_OK;
    if (x->image_state == 1) {
        const hipError_t q = hipEventQuery(x->image_done);
        if (q == hipSuccess) {
            x->image_state = 2;
            return DPQ_OK;
        }
        if (q != hipErrorNotReady) DPQ_HIP(q);
        (void)hipGetLastError();  // ("not ready" is no error of this call: the launches' own checks must not see it)
        if (stream != x->image_stream) DPQ_HIP(hipStreamWaitEvent(stream, x->image_done, 0));
        return DPQ_OK;
    }
    int rc;
    if (!x->d_plain_image && (rc = x->d_plain_image.alloc((size_t)batch_raw_bytes(x)))) return rc;
    if (!x->image_done) DPQ_HIP(hipEventCreateWithFlags(&x->image_done, hipEventDisableTiming));
    {
        Timer t(x, stream, 4);
        DPQ_HIP(dpq::launch_decode_list(x->img, nullptr, x->img.n_segments, x->d_relabel,
                                        reinterpret_cast<uint32_t*>(x->d_plain_image.get()), stream));
    }
    DPQ_HIP(hipEventRecord(x->image_done, stream));
    x->image_stream = stream;
    x->image_state = 1;
    return DPQ_OK;
}

}  // namespace

int splits_for(int n_seg_pass, int n_groups) {
    // One workgroup per CU is resident (LDS), so aim at ONE chip-wave: <= 256 workgroups.  Small levels
    // still spread over as many CUs as they have segments: the exact checks of the filter survivors
    // are bound by each CU's vector-memory address rate, not by its wavefront count.
    const int want = std::max(1, dpq::kMaxSplits / std::max(1, n_groups));
    return std::max(1, std::min(n_seg_pass, want));
}

namespace {

// Candidate-buffer geometry of one scan launch: region 0 (top_k keys) carries the winners of the
// previous level, then one region per scan workgroup of a query group (no global atomics: a
// workgroup appends to its own region).
struct Regions {
    int splits;
    int region_cap;
    int64_t stride;  // keys per slot
};

Regions regions_for(const dpq_index* x, int n_seg_pass, int n_groups, int top_k, int cap) {
    Regions r;
    r.splits = splits_for(n_seg_pass, n_groups);
    r.region_cap = (cap - top_k) / r.splits;
    // automatic sizing: a query's candidates cluster in few segments (DFS neighbours are similar codes), so a
    // region must absorb a few dense segments; 16 K keys per slot, at least one segment's worth per region,
    // and four times a level's expected candidates (top_k x 16) spread over the regions
    if (x->cap_auto)
        r.region_cap = std::max(r.region_cap, std::max(std::max(256, 16384 / r.splits), 64 * top_k / r.splits));
    r.region_cap = std::max(r.region_cap, 1);
    r.stride = (int64_t)top_k + (int64_t)r.splits * r.region_cap;
    return r;
}

// What run_batch does with one sub-batch, decided up front from its size and the index.
struct Batch {
    int nq, top_k;
    int nqp, ngroups;  // slots, padded to whole query groups
    int cap;           // candidate capacity the plan is made for
    // In-scan tightening is live when the scan runs its plain-code instantiation with at most kTightSplits
    // workgroups per query group (8 groups or more): the plan then keeps one filter level also for a large top_k.
    bool tight_plan;
    // One or two queries (the reference's own call shape), up to dpq_open_opts.stream_max_queries (-1 = never): one
    // query per pass over the compressed image, every node evaluated against the exact table (stream_kernel) -- no
    // filter tables, no 64-query group machinery.
    bool direct;
    // Which stream pass: the strand image (a lane per run of 64 nodes) has 64 x fewer, 64 x longer work items than the
    // chunk-per-wavefront decode, so it wants a big shard (dpq::kStrandMinNodes).  ONE query per pass runs
    // strand1_kernel, which tightens its threshold while it runs: one level over the whole shard.
    bool strands, strand1, strand1_tight;
    // Where the decode happens (dpq_open_opts.batch_decode): a batch of several query groups decodes the shard
    // once into plain codes that every group's filter pass reads (through L2 / Infinity Cache at the headline
    // sizes) -- the scan kernel then runs its plain-code instantiation with the DTC distance rule; a batch of one or
    // two groups, or a shard whose plain codes exceed the scratch budget, decodes inside the scan, once per group.
    // Measured on 1 M codes x 1000 queries (16 groups): scan 0.166 -> 0.122 ms, step 0.212 -> 0.172 ms.
    bool scratch;
    int64_t tile_segs;  // segments per tile of the scratch
    bool one_tile;      // one tile holds the shard: decoded once, ahead of the table build
    // the scratch holds relabelled codes (bank-aware labels): the filter tables of this batch are laid
    // out by label, the scan maps a surviving node's code back before the exact check
    bool labelled;
    bool boot_tables;   // the bootstrap writes the first filter level's tables (DPQ_OPT_NO_FUSE_QUANTISE: quantise_kernel)
    int plan_shape;     // ensure_plan's shape bits
    int64_t stride;     // keys per slot of the candidate buffers (the workspace's cap; prepare_batch)
};

// filtered: a batch of dpq_query_batch_*_filtered -- never the stream pass (its kernels take no bitmap): a batch of up to
// stream_max_queries goes through the filter scan as one query group.
Batch batch_mode(const dpq_index* x, int nq, int top_k, bool filtered = false) {
    Batch b{};
    const int QG = dpq::queries_per_group(x->M);
    b.nq = nq;
    b.top_k = top_k;
    b.nqp = (nq + QG - 1) / QG * QG;
    b.ngroups = b.nqp / QG;
    b.cap = x->cap_auto ? auto_cap(top_k) : std::max(x->cap, top_k);
    b.tight_plan = x->tune.tighten && nq > x->tune.stream_max && b.ngroups * dpq::kTightSplits >= dpq::kMaxSplits &&
                   (x->plain || use_batch_decode(x, b.ngroups));
    b.direct = !x->plain && nq <= x->tune.stream_max && !filtered;
    b.strands = b.direct && x->img.st_ckpt != nullptr && (x->tune.force_strands || x->img.n_local >= dpq::kStrandMinNodes);
    b.strand1 = b.strands && x->tune.strand1 && dpq::stream_queries_per_pass(x->M, nq) == 1;
    b.strand1_tight = b.strand1 && x->tune.tighten && x->tune.plan_ratios[0] == 0;
    b.scratch = !b.direct && use_batch_decode(x, b.ngroups);
    b.tile_segs = b.scratch ? batch_tile_segments(x) : 0;
    b.one_tile = b.scratch && b.tile_segs >= x->img.n_segments;
    b.labelled = b.scratch && x->d_relabel.get() != nullptr;
    b.boot_tables = x->boot && x->tune.fuse_quantise && !b.direct;
    b.plan_shape = (nq <= x->tune.coarse_below ? 1 : 0) | (b.tight_plan ? 2 : 0) | (b.strand1_tight ? 4 : 0);
    return b;
}

// The batch's plan and the active workspace, sized for it; sets b->stride.
int prepare_batch(dpq_index* x, Batch* b) {
    int rc;
    if ((rc = ensure_plan(x, b->top_k, b->cap, b->plan_shape))) return rc;
    int64_t stride = b->top_k;
    for (size_t l = 1; l < x->level_cnt.size(); ++l)
        stride = std::max(stride, regions_for(x, x->level_cnt[l], b->ngroups, b->top_k, b->cap).stride);
    // strand1_kernel: a region per workgroup (no global atomics on the candidates' way): room for top_k keys each, 64..256
    const int s1_region_cap = std::min(std::max(64, b->top_k), 256);
    if (b->strand1) stride = std::max<int64_t>(stride, (int64_t)b->top_k + (int64_t)dpq::kStrand1Regions * s1_region_cap);
    if (stride > INT32_MAX) return fail(DPQ_ERR_NOMEM, "candidate buffer too large");
    if ((rc = ensure_workspace(x, b->nqp, (int)stride))) return rc;
    b->stride = x->ws().cap;
    if (b->scratch && (rc = ensure_batch_raw(x))) return rc;
    return DPQ_OK;
}

// The exact tables of the batch; also clears the overflow flags and tightening counters of its slots.  One tile covers
// the whole shard (the common case): the handle's resident plain-code image serves every batch (decoded by the first
// one, ahead of its table build) and every level scans its slice of it.  Otherwise each level decodes its own tiles
// in list order.
int build_tables(dpq_index* x, const Batch& b, const TableSource& src, hipStream_t stream, bool row_stats = true) {
    Workspace& w = x->ws();
    int rc;
    if (b.one_tile && (rc = ensure_plain_image(x, stream))) return rc;
    {
        Timer t(x, stream, 0);
        // batches that scan the plain-code scratch also get the tables in the scratch's label order
        const uint8_t* relabel = b.scratch ? x->d_relabel.get() : nullptr;
        uint32_t* tight = x->tune.tighten ? w.d_tight.get() : nullptr;
        if (src.d_tables)  // the caller's tables (dpq_query_batch_tables): the same workspace state, entries validated
            DPQ_HIP(dpq::launch_tables_ingest(src.d_tables, b.nq, b.nqp, x->M, x->K, w.d_lut32, w.d_lut_min, w.d_overflow,
                                              relabel, w.d_lut32r, tight, src.d_bad, stream));
        else
            DPQ_HIP(dpq::launch_lut_build(x->d_codebook, src.d_queries, b.nq, b.nqp, x->M, x->K, x->Ds, w.d_lut32,
                                          w.d_lut_min, nullptr, w.d_overflow, relabel, w.d_lut32r, tight, stream));
        // the rows' order statistics the filter's saturations are split by (M = 8): behind the tables, under the other
        // lane's scan like them.  row_stats false: a batch of the stream pass, which builds no filter tables
        if (row_stats) DPQ_HIP(dpq::launch_row_stats(w.d_lut32, b.nq, x->M, w.d_lut_stat, stream));
    }
    if (x->prof) x->prof_acc.lut_launches++;
    return DPQ_OK;
}

// What every scan launch of the batch starts from.
dpq::ScanArgs batch_scan_args(const dpq_index* x, const Batch& b) {
    const Workspace& w = x->ws();
    dpq::ScanArgs sa{};
    sa.img = x->img;
    if (b.one_tile) sa.img.raw = x->d_plain_image;
    sa.fp32_accum = x->plain ? 1 : 0;
    sa.lut32 = b.labelled ? w.d_lut32r.get() : w.d_lut32.get();
    sa.lut_min = w.d_lut_min;
    sa.lut_stat = w.d_lut_stat;
    sa.thr_key = w.d_thr_key;
    sa.slot_query = nullptr;
    sa.n_queries = b.nq;
    sa.cand_count = w.d_cand_count;
    sa.cand_key = w.d_cand_key;
    sa.cand_stride = b.stride;
    sa.region_off = b.top_k;
    sa.counters = x->prof && !x->prof_scan_only ? x->d_counters.get() : nullptr;
    sa.qtab = w.d_qtab;
    // in-scan threshold tightening (plain-code scans of this batch; scan_kernel): the workspace's tightening counters.
    // Measured (1 M codes x 1000 queries): top-100 +2 % queries/s (exact checks 3002 -> 1813 and candidates 802 -> 404 per
    // query, select 21 -> 16 us); top-300 +7 %, top-512 +22 %.  On top of the two short levels a large top_k used to get
    // it cost 2 % (M = 8) to 7 % (M = 16) -- but ONE level with the tightening beats those plans (top-1000 1.89 -> 2.27 M
    // q/s, M = 16 1.21 -> 1.27 M, top-2048 0.97 -> 1.19 M): ensure_plan gives top_k > 512 one level when the launch
    // tightens, and the tightening stays off only where such a top_k meets a plan of several levels (shards > 2 M codes).
    sa.tight_hist = x->tune.tighten && (b.top_k <= 512 || x->level_cnt.size() <= 2) ? w.d_tight.get() : nullptr;
    sa.tight_k = b.top_k;
    return sa;
}

// What every select launch of the batch starts from.
dpq::SelectArgs batch_select_args(const dpq_index* x, const Batch& b, int32_t* d_ids, float* d_dists, int flag_slot) {
    const Workspace& w = x->ws();
    dpq::SelectArgs se{};
    se.threads = x->tune.select_threads;
    se.fast_final = x->tune.select_fast;
    se.cand_count = w.d_cand_count;
    se.cand_key = w.d_cand_key;
    se.cand_stride = b.stride;
    se.region_off = b.top_k;
    se.scratch = w.d_scratch;
    se.lut32 = w.d_lut32;
    se.slot_query = nullptr;
    se.top_k = b.top_k;
    se.thr_key = w.d_thr_key;
    se.overflow = w.d_overflow;
    se.any_overflow = x->d_any + flag_slot;
    se.out_ids = d_ids;
    se.out_dists = d_dists;
    se.n_codes_total = x->plain ? -1 : x->img.n_codes_total;
    se.fp32_accum = x->plain ? 1 : 0;
    se.keep_thr = x->boot ? 1 : 0;
    se.stamps = x->d_boot_stamps ? x->d_boot_stamps + (size_t)kMaxBatchQueries * 8 : nullptr;
    return se;
}

// Level 0 with a multi-index: the nodes of the query's best cells, evaluated exactly -> first threshold.
int boot_level(dpq_index* x, const Batch& b, const dpq_filter* filt, hipStream_t stream) {
    const Workspace& w = x->ws();
    const int top_k = b.top_k;
    const int cap_env = x->tune.boot_cap;
    dpq::BootArgs ba{};
    ba.cell_start = x->d_mi_cell;
    const bool full_sort = x->tune.boot_fullsort;  // developer A/B
    ba.nbr = full_sort ? nullptr : x->d_nbr.get();
    ba.n_classes = x->boot_classes;
    ba.mi_code = x->d_mi_code;
    ba.mi_id = x->d_mi_id;
    ba.lut32 = w.d_lut32;
    ba.slot_query = nullptr;
    ba.top_k = top_k;
    // 4-byte keys: up to 6144 of them keep the block at 40 KB of LDS (four blocks per CU).  Measured at top-100,
    // M = 8 (scripts/gpu_boot_ab.sh): 3072 / 4096 / 6144 nodes -> 727 / 559 / 404 candidates per query and the
    // same step time within 1.5 % (what the scan saves the bootstrap spends); 3072 is the shortest critical path.
    // M = 16 (a class sees 2 of 16 sub-spaces: weaker cells; a check costs 16 gathers): 3072 / 6144 / 8192 ->
    // 3003 / 1373 / 1021 candidates, 1.77 / 1.99 / 2.00 M q/s (scripts/gpu_m16_boot.sh).  top_k > 256
    // (scripts/gpu_boot_cap1000.sh, top-1000): 8192 / 12288 / 16384 -> M = 8 1.81 / 1.83 / 1.81, M = 16
    // 1.05 / 1.10 / 1.00 M q/s.  Round 3, one level + in-scan tightening (scripts/gpu_boot_cap_large_k.sh),
    // 4096 / 6144 / 8192 / 12288: top-512 3.11 / 3.27 / 3.25 / 3.16, top-1000 1.76 / 1.96 / 2.10 / 2.28,
    // top-2048 0.74 / 0.97 / 1.06 / 1.20, M = 16 top-1000 1.04 / 1.17 / 1.22 / 1.27 M q/s.
    // (5888, not 6144, keys where the block is meant to stay at four per CU: 39 KB is what four blocks per CU take --
    // see select_list_keys; M = 16 holds 16 KB of tables and runs three per CU either way)
    const int cap_auto = top_k <= 256 ? (x->M <= 8 ? 3072 : 6144) : (top_k <= 640 && x->M <= 8) ? 5888 : 12288;
    ba.cap = std::max(std::min(cap_env > 0 ? cap_env : cap_auto, 16384), std::max(top_k, 2048));
    ba.cap = (ba.cap + 63) / 64 * 64;
    const int target_env = x->tune.boot_target;
    // Cells are walked in rounds until `target` nodes are evaluated.  At top_k <= 256 two thirds of the key list are
    // enough: the 1 % of the queries whose first round of cells brings fewer than `cap` nodes (sparse neighbourhoods:
    // 9 of 1000 on the bench index) then stop there instead of walking a second round -- they were the launch's
    // last blocks (dev_boot_stamps.py: span 25.4 -> 22.4 us), their thresholds come from >= 2048 nodes instead of
    // 3072 and the scan's own tightening does the rest (exact checks and candidates per query unchanged).
    const int target_auto = top_k <= 256 ? std::max(top_k, ba.cap * 2 / 3) : ba.cap;
    ba.target = target_env > 0 ? std::min(ba.cap, std::max(target_env, top_k)) : target_auto;
    ba.thr_key = w.d_thr_key;
    ba.cand_count = w.d_cand_count;
    ba.fp32_accum = x->plain ? 1 : 0;
    ba.stamps = x->d_boot_stamps;
    ba.variant = x->tune.boot_variant;
    ba.n_queries = b.nq;
    // DPQ_OPT_NO_FUSE_QUANTISE: the first level's tables from quantise_kernel, as for every later level
    ba.qtab = b.boot_tables ? w.d_qtab.get() : nullptr;
    ba.relabel = b.scratch ? x->d_relabel.get() : nullptr;
    ba.lut_min = w.d_lut_min;
    ba.lut_stat = w.d_lut_stat;
    if (filt) {
        // Filtered: the k-th key among allowed nodes, from at most 8 x cap evaluated nodes.  The bound keeps the launch
        // within 8 x the unfiltered one's evaluations; a filter that allows 1/8 of the nodes or more still fills the key
        // list, one that allows fewer gives a looser threshold (the k-th of fewer keys) or none (fewer than top_k keys:
        // the first level then lets every allowed node through, which the select and the rerun handle).
        ba.filter = filt->bits;
        ba.id_base = x->img.id_base;
        ba.eval_cap = 8 * ba.cap;
    }
    const int slots = b.boot_tables ? b.nqp : b.nq;
    {
        Timer t(x, stream, 5);
        DPQ_HIP(dpq::launch_bootstrap(ba, x->M, slots, stream));
    }
    if (x->prof) x->prof_acc.bootstrap_launches++;
    if (filt) return DPQ_OK;  // (the developer replay hooks keep unfiltered launches only: a filter may be freed)
    x->dbg_ba = ba;
    x->dbg_boot_slots = slots;
    return DPQ_OK;
}

// Level l >= 1 of a batch of the stream pass: every node of the level's segments (sa.seg_list / n_seg_pass), or of its
// share of the strips, against each query's exact table; one region per slot behind the carried winners.
int stream_level(dpq_index* x, const Batch& b, size_t l, const dpq::ScanArgs& sa, dpq::SelectArgs& se,
                 hipStream_t stream) {
    const Workspace& w = x->ws();
    const int nq = b.nq, top_k = b.top_k;
    dpq::ScanArgs st = sa;
    st.tight_hist = nullptr;
    // one region per slot behind the carried winners, filled through a global counter
    st.region_cap = se.region_cap = (int32_t)std::min<int64_t>(b.stride - top_k, INT32_MAX);
    se.n_regions = 2;
    DPQ_HIP(hipMemset2DAsync(w.d_cand_count + 1, sizeof(uint32_t) * dpq::kRegionStride, 0, sizeof(uint32_t), (size_t)nq,
                             stream));
    // Which stream pass: the strand image (a lane per run of 64 nodes) has 64 x fewer, 64 x longer work items than
    // the chunk-per-wavefront decode, so it wants a big shard.  Measured, us per call (strand / chunk), one query:
    // 1 M codes 35 / 37 pipelined but 89 / 59 as a single synchronous call, 4 M 50 / 49, 12.5 M 72 / 97, 32 M
    // 113 / 172, 125 M 343 / 619; four queries per pass: 1 M 55 / 47, 4 M 76 / 61, 12.5 M 103 / 121, 32 M
    // 195 / 230, 125 M 609 / 841.  From 8 M codes.
    if (!b.strands) {
        Timer t(x, stream, 1);
        DPQ_HIP(dpq::launch_stream(st, nq, stream));
        if (x->prof) x->prof_acc.stream_launches++;
    } else {
        // the pass over the strand image: the level's share of the strips (every strip exactly once over the levels,
        // like the segments; the bootstrap consumed none)
        const bool one_level = x->level_cnt.size() == 2;
        const int64_t nseg = x->img.n_segments, ns = x->img.n_strips;
        const int64_t lo = (int64_t)x->level_off[l] * ns / nseg;
        const int64_t hi = l + 1 == x->level_cnt.size() ? ns : ((int64_t)x->level_off[l] + x->level_cnt[l]) * ns / nseg;
        Timer t(x, stream, 1);
        if (b.strand1) {
            // one level: the strips in storage order (a workgroup sweeps a contiguous share)
            st.seg_list = one_level ? nullptr : x->d_strip_order + lo;
            st.n_seg_pass = (int32_t)(hi - lo);
            // the kernel's candidate histogram (kS1HistWords of the batch's one slot, cleared by the table build); one
            // launch per batch reads it (a later level would count in other units)
            st.tight_hist = b.strand1_tight && one_level && nq == 1 ? w.d_tight.get() : nullptr;
            st.debug_pass = x->tune.s1_debug ? 16 + x->tune.s1_debug : 0;
            st.stamps = x->d_s1_stamps;
            // a region per workgroup, counts written by the kernel
            st.region_cap = se.region_cap = (int32_t)((b.stride - top_k) / dpq::kStrand1Regions);
            se.n_regions = 1 + dpq::strand1_workgroups(st.n_seg_pass);
            DPQ_HIP(dpq::launch_strand1(st, nq, stream));
            if (x->prof) x->prof_acc.strand1_launches++;
        } else if (hi - lo < 1536 && x->d_strip_segs && !x->tune.force_strands) {
            // A level of few strips (one strip per wavefront: the launch takes a strip's 64 dependent steps however
            // few there are) goes through the chunk-per-wavefront pass over the same nodes: measured break-even at
            // about 1500 strips (6 M nodes).
            st.seg_list = x->d_strip_segs + x->strip_seg_off[(size_t)lo];
            st.n_seg_pass = (int32_t)(x->strip_seg_off[(size_t)hi] - x->strip_seg_off[(size_t)lo]);
            DPQ_HIP(dpq::launch_stream(st, nq, stream));
            if (x->prof) x->prof_acc.stream_launches++;
        } else {
            st.seg_list = x->d_strip_order + lo;
            st.n_seg_pass = (int32_t)(hi - lo);
            DPQ_HIP(dpq::launch_strand(st, nq, stream));
            if (x->prof) x->prof_acc.strand_launches++;
        }
    }
    if (x->prof) {
        x->prof_acc.scan_launches++;
        x->prof_acc.scan_stream_bytes +=
            (int64_t)nq * (int64_t)((double)x->info.device_bytes * sa.n_seg_pass / std::max(1, x->img.n_segments));
    }
    return DPQ_OK;
}

// The scan of sa.seg_list / n_seg_pass by every query group -- in tiles of the plain-code scratch (decode a tile in list
// order, scan it with all groups, next tile) where one tile does not hold the shard.  filter_level's and range_scan's.
int scan_level(dpq_index* x, const Batch& b, const dpq::ScanArgs& sa, int n_groups, int splits, hipStream_t stream) {
    if (!b.scratch || b.one_tile) {
        Timer t(x, stream, 1);
        DPQ_HIP(dpq::launch_scan(sa, n_groups, splits, stream));
        if (x->prof) x->prof_acc.scan_launches++;
        return DPQ_OK;
    }
    Workspace& w = x->ws();
    for (int t0 = 0; t0 < sa.n_seg_pass; t0 += (int)b.tile_segs) {
        const int cnt = std::min<int>((int)b.tile_segs, sa.n_seg_pass - t0);
        {
            Timer t(x, stream, 4);
            DPQ_HIP(dpq::launch_decode_list(x->img, sa.seg_list + t0, cnt, x->d_relabel,
                                            reinterpret_cast<uint32_t*>(w.d_batch_raw.get()), stream));
        }
        dpq::ScanArgs tile = sa;
        tile.img.raw = w.d_batch_raw;
        tile.raw_by_pos = 1;
        tile.append = t0 > 0 ? 1 : 0;
        tile.seg_list = sa.seg_list + t0;
        tile.n_seg_pass = cnt;
        Timer t(x, stream, 1);
        DPQ_HIP(dpq::launch_scan(tile, n_groups, splits, stream));
        if (x->prof) x->prof_acc.scan_launches++;
    }
    return DPQ_OK;
}

// Filter level l >= 1 (sa.seg_list / n_seg_pass): its tables, then its scan by every query group (scan_level).
int filter_level(dpq_index* x, const Batch& b, size_t l, dpq::ScanArgs sa, dpq::SelectArgs& se, hipStream_t stream) {
    Workspace& w = x->ws();
    if (l == 1) {
        // developer hook dpq_debug_filter_tables (DPQ_DEV=1 only): the thresholds the first level's tables are built from,
        // before the selects lower them
        w.dbg_qtab_groups = b.ngroups;
        w.dbg_qtab_nq = 0;
        if (dev_mode()) {
            DPQ_HIP(hipMemcpyAsync(w.d_dbg_thr.get(), sa.thr_key, sizeof(uint64_t) * (size_t)b.nqp, hipMemcpyDeviceToDevice, stream));
            w.dbg_qtab_nq = b.nq;
        }
    }
    w.dbg_qtab_levels++;
    const Regions rg = regions_for(x, sa.n_seg_pass, b.ngroups, b.top_k, b.cap);
    sa.region_cap = se.region_cap = rg.region_cap;
    se.n_regions = 1 + rg.splits;
    if (!(b.boot_tables && l == 1)) {  // the bootstrap kernel wrote the first level's tables itself
        Timer t(x, stream, 3);
        DPQ_HIP(dpq::launch_quantise(sa, b.ngroups, stream));
    }
    if (int rc = scan_level(x, b, sa, b.ngroups, rg.splits, stream)) return rc;
    if (l == 1 && !sa.filter && (!b.scratch || b.one_tile)) {  // (one launch: what dpq_debug_scan_time mode 3 replays)
        x->dbg_sa = sa;
        x->dbg_groups = b.ngroups;
        x->dbg_splits = rg.splits;
    }
    if (x->prof)
        x->prof_acc.scan_stream_bytes +=
            (int64_t)((double)x->info.device_bytes * sa.n_seg_pass / std::max(1, x->img.n_segments));
    return DPQ_OK;
}

// The only host synchronisation of a synchronous batch: did any query drop candidates at some level (buffer
// overflow)?  Then its list may miss entries: those queries are answered again.  sa / se: the batch's last launches.
int rerun_overflowed(dpq_index* x, const Batch& b, dpq::ScanArgs sa, dpq::SelectArgs se, hipStream_t stream) {
    const Workspace& w = x->ws();
    const int nq = b.nq, top_k = b.top_k;
    DPQ_HIP(hipStreamSynchronize(stream));
    if (*reinterpret_cast<volatile uint32_t*>(x->h_any) == 0) return DPQ_OK;
    std::vector<int> over;
    for (int base = 0; base < nq; base += 4096) {
        const int n = std::min(4096, nq - base);
        DPQ_HIP(hipMemcpyAsync(x->h_overflow, w.d_overflow.get() + base, sizeof(uint32_t) * n, hipMemcpyDeviceToHost,
                               stream));
        DPQ_HIP(hipStreamSynchronize(stream));
        for (int i = 0; i < n; ++i)
            if (x->h_overflow[i]) over.push_back(base + i);
    }
    if (over.empty()) return DPQ_OK;

    // Rerun the affected queries over the whole shard in ONE filter level.  The
    // k-th key of the incomplete list is still a valid upper bound (its entries
    // are real nodes) and it is tight, so the number of nodes under it is about
    // top_k; grow the buffer and repeat in the (pathological) case it is not.
    const int QG = dpq::queries_per_group(x->M);
    const int slots2 = ((int)over.size() + QG - 1) / QG * QG;
    const int ng2 = slots2 / QG;
    std::vector<int32_t> slot_query((size_t)slots2, -1);
    std::vector<uint64_t> h_key((size_t)b.nqp), k2((size_t)slots2, ~0ull);
    DPQ_HIP(hipMemcpy(h_key.data(), w.d_thr_key, sizeof(uint64_t) * b.nqp, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < over.size(); ++i) {
        slot_query[i] = over[i];
        k2[i] = h_key[(size_t)over[i]];
    }
    // few, large regions: with a tight threshold the candidates of a query may all sit in one workgroup's share
    const int splits2 = std::min(16, splits_for(x->img.n_segments, ng2));
    int64_t rcap2 = std::max<int64_t>(2 * (int64_t)top_k, 1024);
    for (int attempt = 0;; ++attempt) {
        const int64_t stride2 = (int64_t)top_k + (int64_t)splits2 * rcap2;
        if (stride2 > INT32_MAX) return fail(DPQ_ERR_NOMEM, "candidate buffer too large");
        DevBuf<int32_t> d_slot_query;
        DevBuf<uint32_t> c_count, c_over;
        DevBuf<uint64_t> c_keys, c_scratch, c_tk;
        DevBuf<uint4> c_qtab;
        int rc = d_slot_query.alloc((size_t)slots2);
        if (!rc) rc = c_count.alloc((size_t)slots2 * dpq::kRegionStride);
        if (!rc) rc = c_over.alloc((size_t)slots2);
        if (!rc) rc = c_keys.alloc((size_t)slots2 * stride2);
        if (!rc) rc = c_scratch.alloc((size_t)slots2 * stride2);
        if (!rc) rc = c_tk.alloc((size_t)slots2);
        if (!rc) rc = c_qtab.alloc((size_t)ng2 * (dpq::qtab_bytes_per_group(x->M) / sizeof(uint4)));
        if (rc) return rc;
        hipError_t e = hipSuccess;
        auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
        chk(hipMemcpy(d_slot_query, slot_query.data(), sizeof(int32_t) * slots2, hipMemcpyHostToDevice));
        chk(hipMemcpy(c_tk, k2.data(), sizeof(uint64_t) * slots2, hipMemcpyHostToDevice));
        chk(hipMemsetAsync(c_count, 0, sizeof(uint32_t) * slots2 * dpq::kRegionStride, stream));  // region 0: no carried winners
        chk(hipMemsetAsync(c_over, 0, sizeof(uint32_t) * slots2, stream));
        sa.seg_list = nullptr;
        sa.n_seg_pass = x->img.n_segments;
        sa.tight_hist = nullptr;  // the rerun starts from final thresholds
        if (!b.one_tile) {  // a tiled scratch holds the last tile only: the rerun decodes inside the scan, code values as labels
            sa.img.raw = x->img.raw;
            sa.lut32 = w.d_lut32;
        }
        sa.thr_key = c_tk;
        sa.slot_query = d_slot_query;
        sa.n_queries = slots2;
        sa.cand_count = c_count;
        sa.cand_key = c_keys;
        sa.cand_stride = stride2;
        sa.region_cap = (int32_t)rcap2;
        sa.qtab = c_qtab;
        if (b.direct && attempt == 0)  // a batch of the stream pass left no row statistics for the filter tables
            chk(dpq::launch_row_stats(w.d_lut32, b.nq, x->M, w.d_lut_stat, stream));
        chk(dpq::launch_quantise(sa, ng2, stream));
        chk(dpq::launch_scan(sa, ng2, splits2, stream));
        std::vector<uint32_t> h_cnt((size_t)slots2 * dpq::kRegionStride, 0);
        chk(hipMemcpyAsync(h_cnt.data(), c_count, sizeof(uint32_t) * h_cnt.size(), hipMemcpyDeviceToHost, stream));
        chk(hipStreamSynchronize(stream));
        uint32_t max_cnt = 0;
        for (uint32_t c : h_cnt) max_cnt = std::max(max_cnt, c);
        if (e == hipSuccess && (int64_t)max_cnt > rcap2 && attempt < 4) {
            rcap2 = (int64_t)max_cnt + 64;
            continue;
        }
        se.shared_id = nullptr;
        se.shared_code = nullptr;
        se.shared_n = 0;
        se.cand_count = c_count;
        se.cand_key = c_keys;
        se.cand_stride = stride2;
        se.region_cap = (int32_t)rcap2;
        se.n_regions = 1 + splits2;
        se.scratch = c_scratch;
        se.slot_query = d_slot_query;
        se.thr_key = c_tk;
        se.overflow = c_over;
        se.any_overflow = nullptr;
        se.final_pass = 1;
        chk(dpq::launch_select(se, x->M, slots2, stream));
        chk(hipStreamSynchronize(stream));
        if (e != hipSuccess) return fail(DPQ_ERR_HIP, std::string("overflow rerun: ") + hipGetErrorString(e));
        if ((int64_t)max_cnt > rcap2) return fail(DPQ_ERR_NOMEM, "candidate overflow persisted after reruns");
        break;
    }
    if (x->prof) x->prof_acc.overflow_reruns += (int64_t)over.size();
    return DPQ_OK;
}

// One sub-batch (nq <= kMaxBatchQueries) end to end on `stream`.
// flag_slot 0: synchronous (waits, checks the overflow word, reruns what overflowed); > 0: enqueue only,
// dpq_finish looks at the word later.
// filt (synchronous calls only): the batch of dpq_query_batch_*_filtered -- the bootstrap, the scans and level 0 see only
// the nodes it allows.
int run_batch(dpq_index* x, const TableSource& src, int nq, int top_k, int32_t* d_ids, float* d_dists,
              hipStream_t stream, int flag_slot = 0, const dpq_filter* filt = nullptr) {
    Batch b = batch_mode(x, nq, top_k, filt != nullptr);
    int rc;
    if ((rc = prepare_batch(x, &b))) return rc;
    if (filt && !x->boot && x->img.n_segments > 0) {
        // level 0 of this handle's plan, its nodes the filter does not allow turned into padding (once per filter: the
        // list of a handle does not change)
        const int n0 = (int)(x->level_cnt[0] * (int64_t)dpq::kChunk * x->img.chunks_per_segment);
        if (filt->l0_n != n0) {
            filt->l0_n = -1;
            if ((rc = filt->l0_id.alloc((size_t)n0))) return rc;
            DPQ_HIP(dpq::launch_filter_ids(x->d_l0_id, n0, filt->bits, x->img.id_base, filt->l0_id, stream));
            filt->l0_n = n0;
        }
    }
    if ((rc = build_tables(x, b, src, stream, !b.direct))) return rc;
    x->ws().dbg_qtab_levels = 0;
    x->h_any[flag_slot] = 0;  // the slot is free: its previous batch has been finished
    dpq::ScanArgs sa = batch_scan_args(x, b);
    sa.filter = filt ? filt->bits.get() : nullptr;
    dpq::SelectArgs se = batch_select_args(x, b, d_ids, d_dists, flag_slot);

    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    const size_t n_levels = x->img.n_segments > 0 ? x->level_cnt.size() : 0;
    if (n_levels == 0) {  // empty shard: every row is padding
        se.final_pass = 1;
        DPQ_HIP(dpq::launch_select(se, x->M, nq, stream));
        return DPQ_OK;
    }
    for (size_t l = 0; l < n_levels; ++l) {
        if (l == 0 && x->boot) {
            if ((rc = boot_level(x, b, filt, stream))) return rc;
            continue;
        }
        if (l == 0) {
            // level 0: the pre-decoded, query-independent list; every query evaluates it exactly
            se.shared_id = filt ? filt->l0_id.get() : x->d_l0_id.get();
            se.shared_code = x->d_l0_code;
            se.shared_n = (int)(x->level_cnt[0] * S);
        } else {
            se.shared_id = nullptr;
            se.shared_code = nullptr;
            se.shared_n = 0;
            // the next slice of segments; its candidates go behind the carried winners
            sa.seg_list = x->d_order + x->level_off[l];
            sa.n_seg_pass = x->level_cnt[l];
            if ((rc = b.direct ? stream_level(x, b, l, sa, se, stream) : filter_level(x, b, l, sa, se, stream))) return rc;
        }
        if (x->prof) x->prof_acc.scan_node_query_pairs += (int64_t)x->level_cnt[l] * S * nq;
        se.final_pass = l + 1 == n_levels ? 1 : 0;
        {
            Timer t(x, stream, 2);
            DPQ_HIP(dpq::launch_select(se, x->M, nq, stream));
        }
        if (x->prof) x->prof_acc.select_launches++;
    }
    if (flag_slot > 0) return DPQ_OK;  // asynchronous batch: dpq_finish checks the word
    return rerun_overflowed(x, b, sa, se, stream);
}

// ---- range search (dpq_range_search) ------------------------------------------------------------------------------
// One filter level over every segment at the caller's radius: no bootstrap, no tightening, no select.  The scan's
// region counts are exact past region_cap, so range_count_kernel knows every list's length after the one scan; the
// lists that did not fit their regions are scanned again with regions as large as their fullest one (segments go to
// the scan's workgroups by list position, so the counts come out the same), and range_emit_kernel sorts each list
// into the CSR output.  DESIGN.md 5.7.
constexpr int64_t kRangeChunkKeys = (int64_t)1 << 26;  // keys (or results) a launch's buffers may hold: 512 MB of keys

// The threshold key of radius r: the scan keeps key <= thr, so d < r is (dist bits << 32 | pos) <= (bits(r) << 32) - 1.
// false: the list is empty (r <= 0).  +inf keeps every code.
bool range_thr_key(float r, uint64_t* key) {
    if (!(r > 0.0f)) return false;
    if (std::isinf(r)) {
        *key = ~0ull;
        return true;
    }
    uint32_t bits;
    std::memcpy(&bits, &r, sizeof bits);
    *key = ((uint64_t)bits << 32) - 1ull;
    return true;
}

// The filter scan of one range launch: the slots' tables from their thresholds, then every segment (scan_level).
int range_scan(dpq_index* x, const Batch& b, dpq::ScanArgs sa, int n_groups, int splits, hipStream_t stream) {
    Workspace& w = x->ws();
    w.dbg_qtab_levels = 0;  // (not a batch's first filter level: dpq_debug_filter_tables)
    DPQ_HIP(hipMemsetAsync(sa.cand_count, 0, sizeof(uint32_t) * (size_t)n_groups * dpq::queries_per_group(x->M) *
                                                 dpq::kRegionStride, stream));
    if (sa.n_seg_pass <= 0) return DPQ_OK;
    {
        Timer t(x, stream, 3);
        DPQ_HIP(dpq::launch_quantise(sa, n_groups, stream));
    }
    return scan_level(x, b, sa, n_groups, splits, stream);
}

// Writes the lists of the launch's slots `emit` (their queries in ascending order) from the candidate buffers of `ea`
// into res at res_base + lims[query]: in chunks of at most kRangeChunkKeys results (a longer list is a chunk of its own).
int range_emit(dpq_index* x, dpq::RangeEmitArgs ea, int n_slots, const std::vector<int>& emit,
               const std::vector<int32_t>& slot_query, const std::vector<int64_t>& lims, int64_t res_base,
               dpq_range_result* res, hipStream_t stream) {
    RangeWs& R = x->range;
    std::vector<int64_t> off((size_t)n_slots);
    for (size_t i = 0; i < emit.size();) {
        std::fill(off.begin(), off.end(), -1);
        int64_t span = 0, max_n = 0;
        bool contiguous = true;
        size_t j = i;
        for (; j < emit.size(); ++j) {
            const int q = slot_query[(size_t)emit[j]];
            const int64_t n = lims[(size_t)q + 1] - lims[(size_t)q];
            if (j > i && span + n > kRangeChunkKeys) break;
            if (j > i && lims[(size_t)slot_query[(size_t)emit[j - 1]] + 1] != lims[(size_t)q]) contiguous = false;
            off[(size_t)emit[j]] = span;
            span += n;
            max_n = std::max(max_n, n);
        }
        if (span > 0) {
            int rc;
            if ((size_t)span > R.out_n) {
                R.out_n = 0;
                if ((rc = R.out_ids.alloc((size_t)span)) || (rc = R.out_dists.alloc((size_t)span))) return rc;
                R.out_n = (size_t)span;
            }
            if (max_n > dpq::kRangeLdsKeys && (rc = grow(R.scratch, &R.scratch_n, 2 * (size_t)span))) return rc;
            DPQ_HIP(hipMemcpyAsync(R.out_off, off.data(), sizeof(int64_t) * n_slots, hipMemcpyHostToDevice, stream));
            ea.out_off = R.out_off;
            ea.out_ids = R.out_ids;
            ea.out_dists = R.out_dists;
            ea.out_n = span;
            ea.scratch = max_n > dpq::kRangeLdsKeys ? R.scratch.get() : nullptr;
            int lk = 2;
            while (lk < std::min<int64_t>(max_n, dpq::kRangeLdsKeys)) lk <<= 1;
            ea.lds_keys = lk;
            {
                Timer t(x, stream, 2);
                DPQ_HIP(dpq::launch_range_emit(ea, n_slots, stream));
            }
            const int64_t first = res_base + lims[(size_t)slot_query[(size_t)emit[i]]];
            if (contiguous) {
                DPQ_HIP(hipMemcpyAsync(res->ids.data() + first, R.out_ids, sizeof(int32_t) * span, hipMemcpyDeviceToHost, stream));
                DPQ_HIP(hipMemcpyAsync(res->dists.data() + first, R.out_dists, sizeof(float) * span, hipMemcpyDeviceToHost,
                                       stream));
                DPQ_HIP(hipStreamSynchronize(stream));
            } else {
                std::vector<int32_t> h_ids((size_t)span);
                std::vector<float> h_d((size_t)span);
                DPQ_HIP(hipMemcpyAsync(h_ids.data(), R.out_ids, sizeof(int32_t) * span, hipMemcpyDeviceToHost, stream));
                DPQ_HIP(hipMemcpyAsync(h_d.data(), R.out_dists, sizeof(float) * span, hipMemcpyDeviceToHost, stream));
                DPQ_HIP(hipStreamSynchronize(stream));
                for (size_t k = i; k < j; ++k) {
                    const int q = slot_query[(size_t)emit[k]];
                    const int64_t o = off[(size_t)emit[k]], n = lims[(size_t)q + 1] - lims[(size_t)q];
                    std::copy(h_ids.begin() + o, h_ids.begin() + o + n, res->ids.begin() + res_base + lims[(size_t)q]);
                    std::copy(h_d.begin() + o, h_d.begin() + o + n, res->dists.begin() + res_base + lims[(size_t)q]);
                }
            }
        }
        i = j;
    }
    return DPQ_OK;
}

// One sub-batch (nq <= kMaxBatchQueries) of dpq_range_search: queries or tables on the device, radii on the host; appends
// its lists to res (res->lims[base .. base + nq] are filled, base = the number of queries before it).
int range_batch(dpq_index* x, const TableSource& src, int nq, const float* radii, int base, dpq_range_result* res,
                hipStream_t stream) {
    RangeWs& R = x->range;
    const int QG = dpq::queries_per_group(x->M);
    // the plain-code scratch as a top-k batch of this size would use it (tiles included); top_k only sizes what is unused here
    Batch b = batch_mode(x, nq, 1);
    std::vector<int32_t> slot_query;
    std::vector<uint64_t> thr;
    for (int q = 0; q < nq; ++q) {
        uint64_t key;
        if (!range_thr_key(radii[q], &key)) continue;
        slot_query.push_back(q);
        thr.push_back(key);
    }
    const int n_active = (int)slot_query.size();
    const int slots = (n_active + QG - 1) / QG * QG, n_groups = slots / QG;
    slot_query.resize((size_t)slots, -1);
    thr.resize((size_t)slots, 0ull);
    const int64_t res_base = res->lims[(size_t)base];
    std::vector<int64_t> lims((size_t)nq + 1, 0);
    if (n_active == 0) {
        for (int q = 0; q <= nq; ++q) res->lims[(size_t)base + q] = res_base;
        return DPQ_OK;
    }
    int rc;
    if (!R.slot_query) {
        if ((rc = R.slot_query.alloc(kMaxBatchQueries))) return rc;
        if ((rc = R.thr_key.alloc(kMaxBatchQueries))) return rc;
        if ((rc = R.out_off.alloc(kMaxBatchQueries))) return rc;
        if ((rc = R.max_count.alloc(kMaxBatchQueries))) return rc;
        if ((rc = R.lims.alloc(kMaxBatchQueries + 1))) return rc;
        if ((rc = R.cand_count.alloc((size_t)kMaxBatchQueries * dpq::kRegionStride))) return rc;
    }
    // the tables (and the plain-code scratch) in the active lane's workspace, grown if need be; its plan stays as it is
    if ((rc = ensure_workspace(x, b.nqp, std::max(1, x->ws().cap)))) return rc;
    if (b.scratch && (rc = ensure_batch_raw(x))) return rc;
    const bool tiled = b.scratch && !b.one_tile;
    if (tiled && (rc = ensure_order(x))) return rc;
    if ((rc = build_tables(x, b, src, stream))) return rc;

    // regions: splits_for's workgroups per query group, auto-sized as a top-k level's (or dpq_open_opts.cand_capacity)
    const int nseg = x->img.n_segments;
    const int splits = splits_for(nseg, n_groups);
    const int region_cap = x->cap_auto ? std::max(256, 16384 / splits) : std::max(1, x->cap / splits);
    const Workspace& w = x->ws();
    dpq::ScanArgs sa{};
    sa.img = x->img;
    if (b.one_tile) sa.img.raw = x->d_plain_image;
    sa.fp32_accum = x->plain ? 1 : 0;
    sa.lut32 = b.labelled ? w.d_lut32r.get() : w.d_lut32.get();
    sa.lut_min = w.d_lut_min;
    sa.lut_stat = w.d_lut_stat;
    sa.thr_key = R.thr_key;
    sa.slot_query = R.slot_query;
    sa.n_queries = slots;
    sa.seg_list = tiled ? x->d_order.get() : nullptr;
    sa.n_seg_pass = nseg;
    sa.cand_count = R.cand_count;
    sa.region_off = 0;
    sa.counters = x->prof && !x->prof_scan_only ? x->d_counters.get() : nullptr;
    sa.qtab = w.d_qtab;
    sa.tight_hist = nullptr;  // the radius is the final threshold

    // n_live queries in slots [0, n_live), padded with unused slots to whole query groups.  Only the live slots get
    // candidate regions: an unused slot's filter tables reject every node (quantise_kernel), so the scan never writes
    // its region, and range_emit_kernel leaves it alone (out_off -1).
    auto scan_and_count = [&](int n_live, int rcap, int64_t* lims_out, std::vector<uint32_t>* max_count) -> int {
        const int n_slots = (n_live + QG - 1) / QG * QG, ng = n_slots / QG;
        const int64_t stride = (int64_t)splits * rcap;
        int rc2 = grow(R.cand_key, &R.key_n, (size_t)n_live * stride);
        if (rc2) return rc2;
        R.last_max_keys = std::max(R.last_max_keys, (int64_t)n_live * stride);
        DPQ_HIP(hipMemcpyAsync(R.slot_query, slot_query.data(), sizeof(int32_t) * n_slots, hipMemcpyHostToDevice, stream));
        DPQ_HIP(hipMemcpyAsync(R.thr_key, thr.data(), sizeof(uint64_t) * n_slots, hipMemcpyHostToDevice, stream));
        sa.cand_key = R.cand_key;
        sa.cand_stride = stride;
        sa.region_cap = rcap;
        if ((rc2 = range_scan(x, b, sa, ng, splits, stream))) return rc2;
        dpq::RangeCountArgs ca{};
        ca.slot_query = R.slot_query;
        ca.cand_count = R.cand_count;
        ca.n_slots = n_slots;
        ca.n_regions = splits;
        ca.n_queries = nq;
        ca.max_count = R.max_count;
        ca.lims = R.lims;
        {
            Timer t(x, stream, 2);
            DPQ_HIP(dpq::launch_range_count(ca, stream));
        }
        max_count->resize((size_t)n_slots);
        DPQ_HIP(hipMemcpyAsync(lims_out, R.lims, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, stream));
        DPQ_HIP(hipMemcpyAsync(max_count->data(), R.max_count, sizeof(uint32_t) * n_slots, hipMemcpyDeviceToHost, stream));
        DPQ_HIP(hipStreamSynchronize(stream));  // the sizes of the lists
        return DPQ_OK;
    };
    std::vector<uint32_t> max_count;
    if ((rc = scan_and_count(n_active, region_cap, lims.data(), &max_count))) return rc;
    for (int q = 0; q <= nq; ++q) res->lims[(size_t)base + q] = res_base + lims[(size_t)q];
    const int64_t total = res_base + lims[(size_t)nq];
    res->ids.resize((size_t)total);
    res->dists.resize((size_t)total);

    dpq::RangeEmitArgs ea{};
    ea.cand_count = R.cand_count;
    ea.cand_key = R.cand_key;
    ea.cand_stride = (int64_t)splits * region_cap;
    ea.region_off = 0;
    ea.region_cap = region_cap;
    ea.n_regions = splits;
    ea.n_codes_total = x->plain ? -1 : x->img.n_codes_total;
    std::vector<int> emit, over;
    for (int s = 0; s < n_active; ++s) (max_count[(size_t)s] > (uint32_t)region_cap ? over : emit).push_back(s);
    if ((rc = range_emit(x, ea, slots, emit, slot_query, lims, res_base, res, stream))) return rc;
    if (over.empty()) return DPQ_OK;

    // Lists that overflowed their regions: scanned again, as many at a time as kRangeChunkKeys of regions hold (at least
    // one), with regions as large as the fullest of them: n2 x splits x that keys for n2 queries.  splits x the fullest
    // region is about the list's length where its keys spread over the shard (a radius that admits most of it), and
    // at most splits times it where they all sit in one workgroup's segments.
    const std::vector<int32_t> q_of(slot_query.begin(), slot_query.begin() + n_active);
    const std::vector<uint64_t> k_of(thr.begin(), thr.begin() + n_active);
    const std::vector<uint32_t> need(max_count.begin(), max_count.begin() + n_active);
    for (size_t i = 0; i < over.size();) {
        size_t j = i;
        uint32_t rcap = 0;
        for (; j < over.size(); ++j) {
            const uint32_t r2 = std::max(rcap, need[(size_t)over[j]]);
            if (j > i && (int64_t)(j - i + 1) * splits * (int64_t)r2 > kRangeChunkKeys) break;
            rcap = r2;
        }
        if ((int64_t)rcap * splits > INT32_MAX) return fail(DPQ_ERR_NOMEM, "range search: candidate regions too large");
        const int n2 = (int)(j - i), slots2 = (n2 + QG - 1) / QG * QG;
        std::fill(slot_query.begin(), slot_query.end(), -1);
        for (int k = 0; k < n2; ++k) {
            slot_query[(size_t)k] = q_of[(size_t)over[i + k]];
            thr[(size_t)k] = k_of[(size_t)over[i + k]];
        }
        std::vector<int64_t> lims2((size_t)nq + 1);
        if ((rc = scan_and_count(n2, (int)rcap, lims2.data(), &max_count))) return rc;
        for (int k = 0; k < n2; ++k) {
            const int q = slot_query[(size_t)k];
            if (max_count[(size_t)k] > rcap || lims2[(size_t)q + 1] - lims2[(size_t)q] != lims[(size_t)q + 1] - lims[(size_t)q])
                return fail(DPQ_ERR_STATE, "range search: the rerun of an overflowed query found a different count");
        }
        ea.cand_key = R.cand_key;
        ea.cand_stride = (int64_t)splits * rcap;
        ea.region_cap = (int)rcap;
        std::vector<int> emit2((size_t)n2);
        std::iota(emit2.begin(), emit2.end(), 0);
        if ((rc = range_emit(x, ea, slots2, emit2, slot_query, lims, res_base, res, stream))) return rc;
        if (x->prof) x->prof_acc.overflow_reruns += n2;
        i = j;
    }
    return DPQ_OK;
}

// What a range call leaves allocated: the candidate and output buffers of an ordinary call stay for the next one.
void range_trim(dpq_index* x) {
    RangeWs& R = x->range;
    if (R.key_n > ((size_t)40 << 20)) R.cand_key.reset(), R.key_n = 0;  // (a full sub-batch's regions: 32 M keys)
    if (R.out_n > ((size_t)16 << 20)) R.out_ids.reset(), R.out_dists.reset(), R.out_n = 0;
    R.scratch.reset();
    R.scratch_n = 0;
}

int open_from_payload(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, int K,
                      const dpq_open_opts* opts, dpq_index** out) {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    dpq_open_opts o{};
    if (opts) o = *opts;
    if (M != 8 && M != 16)
        return fail(DPQ_ERR_ARG, "this build has scan kernels for M = 8 (reference format) and M = 16 (own extension)");
    if (K < 1 || K > 256) return fail(DPQ_ERR_ARG, "K must be in 1..256 (one byte per sub-code)");
    if (o.global_offset < 0 || o.global_n_codes < 0 || (o.global_offset != 0 && o.global_n_codes == 0) ||
        (o.global_n_codes > 0 && o.global_offset + n_codes > o.global_n_codes))
        return fail(DPQ_ERR_ARG, "global_offset / global_n_codes do not enclose this payload (a part of a larger index "
                                 "needs global_n_codes > 0)");
    if (n_codes >= (int64_t)INT32_MAX || o.global_n_codes >= (int64_t)INT32_MAX || o.global_offset + n_codes >= (int64_t)INT32_MAX)
        return fail(DPQ_ERR_ARG, "ids beyond 2^31 - 1: results carry int32 DFS positions (h:2979)");
    if (o.chunks_per_segment > dpq::kSortMax / dpq::kChunk)
        return fail(DPQ_ERR_ARG, "chunks_per_segment must be <= 64 (a segment is the cascade's level-0 unit)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (o.device < 0 || o.device >= ndev) return fail(DPQ_ERR_NO_DEVICE, "device ordinal out of range");

    dpq::SoA soa;
    std::string err;
    // threshold bootstrap: auto = on from 64 K nodes per shard (estimated before the byte-balanced cut)
    const int64_t n_scan = o.num_codes > 0 ? std::min<int64_t>(o.num_codes, n_codes) : n_codes;
    const int64_t per_shard = n_scan / std::max(1, o.shard_count);
    int mi_stride = o.bootstrap < 0 ? 0 : dpq::bootstrap_stride_for(per_shard);
    if (o.bootstrap > 0 && mi_stride == 0 && per_shard >= 16384) mi_stride = 1;  // forced on (tests, experiments)
    // the strand image (the stream pass's own layout, ~1.2 x the payload in host RAM and HBM) only where run_batch
    // will read it: big shards (cut by bytes: a margin on the estimate), or forced (tests, experiments)
    const Tuning tune0 = resolve_tuning(o);
    const bool want_strands = tune0.strands && (tune0.force_strands || per_shard >= dpq::kStrandMinNodes / 4 * 3);
    int rc = dpq::transcode(payload, n_bytes, n_codes, M, o.shard_rank, o.shard_count, o.chunks_per_segment, &soa,
                            &err, o.num_codes, mi_stride, 0, want_strands ? 1 : 0);
    if (rc) return fail(rc, err);

    DPQ_HIP(hipSetDevice(o.device));
    dpq_index* x = new dpq_index();
    x->device = o.device;
    x->M = M;
    x->K = K;
    x->cap_auto = o.cand_capacity <= 0;
    x->cap = o.cand_capacity;
    x->batch_decode = o.batch_decode;
    x->tune = tune0;
    auto up = [&](auto& buf, const void* src, size_t bytes) -> int {
        using T = typename std::remove_reference_t<decltype(buf)>::value_type;
        int r = buf.alloc((bytes + sizeof(T) - 1) / sizeof(T) + 64 / sizeof(T));
        if (r) return r;
        if (bytes) {
            hipError_t e = hipMemcpy(buf, src, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(DPQ_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
        }
        return DPQ_OK;
    };
    rc = up(x->d_nib, soa.nib.data(), soa.nib.size());
    if (!rc) rc = up(x->d_par, soa.par.data(), soa.par.size());
    if (!rc) rc = up(x->d_carry, soa.carry.data(), soa.carry.size());
    if (!rc) rc = up(x->d_mask, soa.mask.data(), soa.mask.size());
    if (!rc) rc = up(x->d_delta, soa.delta.data(), soa.delta.size());
    if (!rc) rc = up(x->d_seg_off, soa.seg_delta_off.data(), soa.seg_delta_off.size() * 8);
    if (!rc) rc = up(x->d_ckpt, soa.seg_ckpt.data(), soa.seg_ckpt.size());
    if (o.global_offset != 0)
        for (uint32_t& id : soa.mi_id) id += (uint32_t)o.global_offset;
    if (!rc && soa.mi_stride > 0 && (int64_t)soa.mi_id.size() >= 16384) {
        rc = up(x->d_mi_cell, soa.mi_cell_start.data(), soa.mi_cell_start.size() * 4);
        if (!rc) rc = up(x->d_mi_code, soa.mi_code.data(), soa.mi_code.size() * 4);
        if (!rc) rc = up(x->d_mi_id, soa.mi_id.data(), soa.mi_id.size() * 4);
        x->boot = !rc;
        x->boot_classes = soa.mi_classes;
    }
    if (!rc && x->tune.relabel && soa.relabel.size() == (size_t)M * 256) {
        rc = up(x->d_relabel, soa.relabel.data(), soa.relabel.size());
    }
    if (!rc && x->boot && x->tune.strands && soa.n_strips > 0 && soa.n_strips < INT32_MAX) {
        rc = up(x->d_st_ckpt, soa.st_ckpt.data(), soa.st_ckpt.size() * 8);
        if (!rc) rc = up(x->d_st_mask, soa.st_mask.data(), soa.st_mask.size() * 4);
        if (!rc) rc = up(x->d_st_depth, soa.st_depth.data(), soa.st_depth.size() * 2);
        // (st_poff stays on the host: the kernel computes a lane's offset inside a phase as a wave prefix sum of the lanes'
        // byte counts; the array exists for the CPU-side checks of the image)
        if (!rc) rc = up(x->d_st_pbase, soa.st_pbase.data(), soa.st_pbase.size() * 4);
        if (!rc) rc = up(x->d_st_delta, soa.st_delta.data(), soa.st_delta.size());
        if (!rc) {
            // strips are visited in a low-discrepancy order too (every prefix a spread sample of the shard)
            const int64_t ns = soa.n_strips;
            const std::vector<uint32_t> order = golden_order(ns);
            rc = up(x->d_strip_order, order.data(), order.size() * 4);
            const int64_t S = soa.nodes_per_segment();
            if (!rc && dpq::kStripNodes % S == 0) {
                std::vector<uint32_t> segs;
                x->strip_seg_off.assign((size_t)ns + 1, 0);
                for (int64_t j = 0; j < ns; ++j) {
                    const int64_t s0 = (int64_t)order[(size_t)j] * (dpq::kStripNodes / S);
                    for (int64_t t = s0; t < std::min(s0 + dpq::kStripNodes / S, soa.n_segments); ++t) segs.push_back((uint32_t)t);
                    x->strip_seg_off[(size_t)j + 1] = (int64_t)segs.size();
                }
                rc = up(x->d_strip_segs, segs.data(), segs.size() * 4);
            }
        }
        if (!rc) {
            x->img.st_ckpt = x->d_st_ckpt;
            x->img.st_mask = x->d_st_mask;
            x->img.st_depth = x->d_st_depth;
            x->img.st_pbase = x->d_st_pbase;
            x->img.st_delta = x->d_st_delta;
            x->img.n_strips = (int32_t)soa.n_strips;
            x->strand_bytes = soa.strand_bytes();
        }
    }
    if (rc) {
        dpq_close(x);
        return rc;
    }
    x->img.nib = x->d_nib;
    x->img.par = x->d_par;
    x->img.carry = x->d_carry;
    x->img.mask = x->d_mask;
    x->img.delta = x->d_delta;
    x->img.seg_delta_off = x->d_seg_off;
    x->img.seg_ckpt = x->d_ckpt;
    x->img.n_local = soa.node_hi - soa.node_lo;
    x->img.n_codes_total = o.global_n_codes > 0 ? o.global_n_codes : soa.n_codes_total;
    x->img.id_base = (uint32_t)(o.global_offset + soa.node_lo);
    x->img.n_segments = (int32_t)soa.n_segments;
    x->img.chunks_per_segment = soa.chunks_per_segment;
    x->img.M = M;
    x->img.K = K;

    dpq_info& inf = x->info;
    inf.n_codes_total = x->img.n_codes_total;
    inf.n_bytes_total = soa.n_bytes_total;
    inf.node_lo = o.global_offset + soa.node_lo;
    inf.node_hi = o.global_offset + soa.node_hi;
    inf.algorithmic_bytes = soa.algorithmic_bytes;
    inf.device_bytes = soa.device_bytes();
    inf.bootstrap_bytes = x->boot ? soa.bootstrap_bytes() : 0;
    inf.bootstrap_stride = x->boot ? soa.mi_stride : 0;
    inf.batch_decode_mb = batch_decode_possible(x) ? (int32_t)((batch_raw_bytes(x) + (1 << 20) - 1) >> 20) : 0;
    inf.strand_bytes = x->strand_bytes;
    inf.n_diffs = soa.n_diffs;
    inf.M = M;
    inf.K = K;
    inf.Ds = 0;
    inf.n_segments = (int32_t)soa.n_segments;
    inf.chunks_per_segment = soa.chunks_per_segment;
    inf.max_depth = soa.max_depth;
    inf.device = o.device;
    inf.cand_capacity = x->cap;
    *out = x;
    return DPQ_OK;
}

int open_plain(const uint8_t* codes, int64_t n_codes, int M, int K, const dpq_open_opts* opts, dpq_index** out) {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    dpq_open_opts o{};
    if (opts) o = *opts;
    if (!codes || n_codes < 1 || n_codes >= (int64_t)INT32_MAX) return fail(DPQ_ERR_ARG, "bad codes / n_codes");
    if (M != 8 && M != 16) return fail(DPQ_ERR_ARG, "M must be 8 or 16");
    if (K < 1 || K > 256) return fail(DPQ_ERR_ARG, "K must be in 1..256 (one byte per sub-code)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (o.device < 0 || o.device >= ndev) return fail(DPQ_ERR_NO_DEVICE, "device ordinal out of range");
    int cps = o.chunks_per_segment <= 0 ? dpq::kDefaultChunksPerSegment : o.chunks_per_segment;
    if (cps > dpq::kSortMax / dpq::kChunk) return fail(DPQ_ERR_ARG, "chunks_per_segment must be <= 64");
    int count = o.shard_count <= 0 ? 1 : o.shard_count;
    if (o.shard_rank < 0 || o.shard_rank >= count) return fail(DPQ_ERR_ARG, "bad shard_rank / shard_count");
    if (o.num_codes < 0 || (int64_t)o.num_codes > n_codes) return fail(DPQ_ERR_ARG, "num_codes outside 0..n_codes");
    if (o.num_codes > 0) n_codes = o.num_codes;  // scan only the first num_codes codes (h:2625-2629)
    const int64_t S = (int64_t)dpq::kChunk * cps;
    const int64_t nseg_total = (n_codes + S - 1) / S;
    const int64_t seg_lo = nseg_total * o.shard_rank / count, seg_hi = nseg_total * (o.shard_rank + 1) / count;
    const int64_t lo = std::min(seg_lo * S, n_codes), hi = std::min(seg_hi * S, n_codes);
    DPQ_HIP(hipSetDevice(o.device));
    dpq_index* x = new dpq_index();
    x->device = o.device;
    x->M = M;
    x->K = K;
    x->plain = true;
    x->tune = resolve_tuning(o);
    x->cap_auto = o.cand_capacity <= 0;
    x->cap = o.cand_capacity;
    const size_t padded = (size_t)(seg_hi - seg_lo) * S * M;
    int rc = x->d_raw.alloc(padded + 64);
    if (!rc) {
        hipError_t e = hipMemset(x->d_raw, 0, padded + 64);
        if (e == hipSuccess && hi > lo)
            e = hipMemcpy(x->d_raw, codes + (size_t)lo * M, (size_t)(hi - lo) * M, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(DPQ_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
    }
    if (rc) {
        dpq_close(x);
        return rc;
    }
    {
        int mi_stride = o.bootstrap < 0 ? 0 : dpq::bootstrap_stride_for(hi - lo);
        if (o.bootstrap > 0 && mi_stride == 0 && hi - lo >= 16384) mi_stride = 1;
        if (mi_stride > 0) {
            dpq::SoA mi;
            std::vector<uint32_t> ids;
            std::vector<uint8_t> cds;
            for (int64_t i = lo; i < hi; i += mi_stride) {
                ids.push_back((uint32_t)i);
                cds.insert(cds.end(), codes + (size_t)i * M, codes + (size_t)(i + 1) * M);
            }
            dpq::build_multi_index(ids, cds, M, mi_stride, dpq::bootstrap_classes_for((int64_t)ids.size()), &mi);
            auto upl = [&](DevBuf<uint32_t>& d, const std::vector<uint32_t>& v) -> int {
                int r = d.alloc(v.size() + 16);
                if (r) return r;
                if (!v.empty() && hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
                    return fail(DPQ_ERR_HIP, "upload of the bootstrap multi-index failed");
                return DPQ_OK;
            };
            rc = upl(x->d_mi_cell, mi.mi_cell_start);
            if (!rc) rc = upl(x->d_mi_code, mi.mi_code);
            if (!rc) rc = upl(x->d_mi_id, mi.mi_id);
            if (rc) {
                dpq_close(x);
                return rc;
            }
            x->boot = true;
            x->boot_classes = mi.mi_classes;
            x->info.bootstrap_bytes = mi.bootstrap_bytes();
            x->info.bootstrap_stride = mi_stride;
        }
    }
    x->img.raw = x->d_raw;
    x->img.n_local = hi - lo;
    x->img.n_codes_total = n_codes;
    x->img.id_base = (uint32_t)lo;
    x->img.n_segments = (int32_t)(seg_hi - seg_lo);
    x->img.chunks_per_segment = cps;
    x->img.M = M;
    x->img.K = K;
    dpq_info& inf = x->info;
    inf.n_codes_total = n_codes;
    inf.n_bytes_total = n_codes * M;
    inf.node_lo = lo;
    inf.node_hi = hi;
    inf.algorithmic_bytes = (hi - lo) * M;
    inf.device_bytes = (int64_t)padded;
    inf.M = M;
    inf.K = K;
    inf.n_segments = x->img.n_segments;
    inf.chunks_per_segment = cps;
    inf.device = o.device;
    inf.cand_capacity = x->cap;
    *out = x;
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_version(void) { return DPQ_VERSION; }

const char* dpq_strerror(int status) {
    switch (status) {
        case DPQ_OK: return "ok";
        case DPQ_ERR_ARG: return "bad argument";
        case DPQ_ERR_IO: return "i/o error";
        case DPQ_ERR_FORMAT: return "malformed DTC stream";
        case DPQ_ERR_NO_DEVICE: return "no usable GPU";
        case DPQ_ERR_HIP: return "HIP runtime error";
        case DPQ_ERR_NOMEM: return "out of memory";
        case DPQ_ERR_STATE: return "call out of order";
        case DPQ_ERR_TOPK: return "top_k exceeds the number of codes";
        default: return "unknown status";
    }
}

const char* dpq_last_error(void) { return g_last_error.c_str(); }

int dpq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n < 0 ? 0 : n;
}

int dpq_tree_build_gpu(const uint8_t* codes, int64_t n_codes, int M, int K, int max_height_folds,
                       const float* codewords, int Ds, int device, dpq_tree** out) {
    return guarded([&]() -> int {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!codes || n_codes < 1 || n_codes >= (int64_t)INT32_MAX || M < 1 || M > 16 || K < 1 || K > 256 ||
        max_height_folds < 1)
        return fail(DPQ_ERR_ARG, "bad argument to dpq_tree_build_gpu");
    std::string err;
    std::vector<uint32_t> finalists;
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    // DPQ_DEV=1 DPQ_BUILD_PREFILTER=0: every position subset sorted whole, as rounds 2 - 3 did (developer A/B; same tree)
    const bool prefilter = !(dev_mode() && getenv("DPQ_BUILD_PREFILTER") && atoi(getenv("DPQ_BUILD_PREFILTER")) == 0);
    int rc = dpq::find_edges_gpu(codes, n_codes, M, max_height_folds, device, &finalists, &edges, &err, prefilter);
    if (rc) return fail(rc, err);
    dpq_tree* t = new dpq_tree();
    // DPQ_DEV=1 DPQ_BUILD_LAYOUT=host keeps the layout on the host (developer A/B; same tree either way)
    static const bool host_layout = dev_mode() && getenv("DPQ_BUILD_LAYOUT") &&
                                    std::string(getenv("DPQ_BUILD_LAYOUT")) == "host";
    rc = host_layout ? dpq::layout_tree(codes, n_codes, M, K, max_height_folds, codewords, Ds, finalists, &edges, &t->tree, &err)
                     : dpq::layout_tree_gpu(codes, n_codes, M, K, max_height_folds, codewords, Ds, finalists, &edges, device,
                                            &t->tree, &err);
    if (rc) {
        delete t;
        return fail(rc, err);
    }
    *out = t;
    return DPQ_OK;
    });
}

int dpq_open_file(const char* path, int M, int K, const dpq_open_opts* opts, dpq_index** out) {
    return guarded([&]() -> int {
    if (!path || !out) return fail(DPQ_ERR_ARG, "NULL argument");
    std::vector<uint8_t> buf;
    std::string err;
    int rc = dpq::read_file(path, &buf, &err);
    if (rc) return fail(rc, err);
    if (buf.size() < 16) return fail(DPQ_ERR_FORMAT, std::string("file shorter than its header: ") + path);
    int64_t h[2];
    memcpy(h, buf.data(), 16);  // h:2823-2824
    if (h[1] < 0 || (uint64_t)h[1] > buf.size() - 16)
        return fail(DPQ_ERR_FORMAT, "n_bytes in the header exceeds the file size");
    return open_from_payload(buf.data() + 16, h[1], h[0], M, K, opts, out);
    });
}

int dpq_open_memory(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, int K,
                    const dpq_open_opts* opts, dpq_index** out) {
    return guarded([&]() -> int {
    return open_from_payload(payload, n_bytes, n_codes, M, K, opts, out);
    });
}

int dpq_open_plain_memory(const uint8_t* codes, int64_t n_codes, int M, int K, const dpq_open_opts* opts,
                          dpq_index** out) {
    return guarded([&]() -> int {
    return open_plain(codes, n_codes, M, K, opts, out);
    });
}

int dpq_open_plain_file(const char* path, int M, int K, const dpq_open_opts* opts, dpq_index** out) {
    return guarded([&]() -> int {
    if (!path || !out) return fail(DPQ_ERR_ARG, "NULL argument");
    std::vector<uint8_t> codes;
    int64_t n = 0;
    std::string err;
    int rc = dpq::read_codes_plain(path, M, &n, &codes, &err);
    if (rc) return fail(rc, err);
    return open_plain(codes.data(), n, M, K, opts, out);
    });
}

int dpq_set_codebook(dpq_index* x, const float* codewords, int Ds) {
    return guarded([&]() -> int {
    if (!x || !codewords || Ds < 1 || Ds > 4096) return fail(DPQ_ERR_ARG, "bad codebook argument");
    if (int rc = dpq_finish(x)) return rc;  // batches in flight still read the old codebook
    DPQ_HIP(hipSetDevice(x->device));
    const size_t n = (size_t)x->M * x->K * Ds;
    int rc = x->d_codebook.alloc(n);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(x->d_codebook, codewords, n * sizeof(float), hipMemcpyHostToDevice));
    x->Ds = Ds;
    x->info.Ds = Ds;
    if (x->boot) {
        // neighbour lists of the bootstrap's 8 sort slots (slot s: sub-space 2 (s / 2) (M / 8) + (s & 1)): for every
        // centroid all centroids of its sub-space, nearest first (ties by index; centroids beyond K last)
        std::vector<uint8_t> nbr((size_t)8 * 256 * 256);
        std::vector<std::pair<double, int>> row(256);
        for (int sl = 0; sl < 8; ++sl) {
            const int sub = 2 * (sl >> 1) * (x->M / 8) + (sl & 1);
            const float* cw = codewords + (size_t)sub * x->K * Ds;
            for (int c = 0; c < 256; ++c) {
                for (int o = 0; o < 256; ++o) {
                    double d2 = 1e300;  // beyond K: last
                    if (c < x->K && o < x->K) {
                        d2 = 0;
                        for (int d = 0; d < Ds; ++d) {
                            const double df = (double)cw[(size_t)c * Ds + d] - (double)cw[(size_t)o * Ds + d];
                            d2 += df * df;
                        }
                    }
                    row[(size_t)o] = {d2, o};
                }
                std::sort(row.begin(), row.end());
                for (int o = 0; o < 256; ++o) nbr[((size_t)sl * 256 + c) * 256 + o] = (uint8_t)row[(size_t)o].second;
            }
        }
        rc = x->d_nbr.alloc(nbr.size());
        if (rc) return rc;
        DPQ_HIP(hipMemcpy(x->d_nbr, nbr.data(), nbr.size(), hipMemcpyHostToDevice));
    }
    return DPQ_OK;
    });
}

int dpq_get_info(const dpq_index* x, dpq_info* info) {
    return guarded([&]() -> int {
    if (!x || !info) return fail(DPQ_ERR_ARG, "NULL argument");
    *info = x->info;
    info->cand_capacity = x->cap_auto ? 0 : x->cap;
    return DPQ_OK;
    });
}

int dpq_close(dpq_index* x) {
    return guarded([&]() -> int {
    if (!x) return DPQ_OK;
    hipSetDevice(x->device);
    if (!x->pending.empty()) {  // batches still in flight: let them drain before their buffers go
        hipDeviceSynchronize();
        x->pending.clear();
    }
    for (auto& ep : x->events) {
        hipEventDestroy(ep.a);
        hipEventDestroy(ep.b);
    }
    for (auto e : x->ev_pool) hipEventDestroy(e);
    for (int l = 0; l < 2; ++l) {
        if (x->lane_stream[l]) hipStreamDestroy(x->lane_stream[l]);
        if (x->lane_ready[l]) hipEventDestroy(x->lane_ready[l]);
    }
    for (auto& hs : x->host_slots)
        if (hs.kernels_done) hipEventDestroy(hs.kernels_done);
    if (x->image_done) hipEventDestroy(x->image_done);
    if (x->copy_in) hipStreamDestroy(x->copy_in);
    if (x->copy_out) hipStreamDestroy(x->copy_out);
    if (x->h_overflow) hipHostFree(x->h_overflow);
    if (x->h_any) hipHostFree(x->h_any);
    if (x->h_tables_bad) hipHostFree(x->h_tables_bad);
    delete x;  // (the device buffers go with it)
    return DPQ_OK;
    });
}

}  // extern "C"

int check_batch_args(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists) {
    if (!x || !d_queries || !d_ids || !d_dists || nq < 0) return fail(DPQ_ERR_ARG, "NULL argument or nq < 0");
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, "dpq_set_codebook has not been called");
    if (top_k < 1 || top_k > dpq::kMaxTopK) return fail(DPQ_ERR_ARG, "top_k must be in 1..2048");
    if ((int64_t)top_k > x->img.n_codes_total)
        return fail(DPQ_ERR_TOPK, "top_k exceeds the number of codes in the index");
    return DPQ_OK;
}

extern "C" {

int dpq_finish(dpq_index* x) {
    return guarded([&]() -> int {
    if (!x) return fail(DPQ_ERR_ARG, "NULL index");
    if (x->pending.empty()) return DPQ_OK;
    DPQ_HIP(hipSetDevice(x->device));
    std::vector<dpq_index::Pending> todo;
    todo.swap(x->pending);
    {
        std::vector<hipStream_t> seen;
        hipError_t e = hipSuccess;
        for (const auto& p : todo)
            if (std::find(seen.begin(), seen.end(), p.stream) == seen.end()) {
                const hipError_t r = hipStreamSynchronize(p.stream);
                if (e == hipSuccess) e = r;
                seen.push_back(p.stream);
            }
        if (e != hipSuccess) {  // the device is in an error state: nothing can be rerun; the batches stay pending
            x->pending.insert(x->pending.begin(), todo.begin(), todo.end());
            return fail(DPQ_ERR_HIP, std::string("dpq_finish: ") + hipGetErrorString(e));
        }
    }
    // Every stream a pending batch ran on is idle from here on (synchronised above; nothing is enqueued while this
    // function runs: a handle belongs to one thread at a time), so a rerun may use whichever lane's workspace is
    // active.  Every batch is settled even if one fails: its callers' buffers must not keep an incomplete list behind
    // a later dpq_finish that has nothing left to report.  The first error is returned.
    int first_rc = DPQ_OK;
    std::string first_msg;
    for (const auto& p : todo) {
        if (*reinterpret_cast<volatile uint32_t*>(x->h_any + p.flag_slot) == 0) continue;
        // a query of this batch dropped candidates: answer the batch again, synchronously (it reruns what overflows)
        x->finish_reruns++;
        int rc = run_batch(x, TableSource{p.d_queries}, p.nq, p.top_k, p.d_ids, p.d_dists, p.stream);
        if (p.host_slot >= 0) x->host_slots[p.host_slot].redo = true;  // its results went down before this
        if (rc && !first_rc) {
            first_rc = rc;
            first_msg = g_last_error;
        }
    }
    // host-to-host batches: their results are on the way down (copy_out), or go down again after a rerun
    bool any_host = false;
    for (auto& hs : x->host_slots) any_host = any_host || hs.busy;
    if (any_host) {
        hipError_t e = x->copy_out ? hipStreamSynchronize(x->copy_out) : hipSuccess;
        for (auto& hs : x->host_slots) {
            if (hs.busy && hs.redo && !hs.direct && e == hipSuccess) {
                e = hipMemcpy(hs.h_ids, hs.d_ids, hs.n_out * sizeof(int32_t), hipMemcpyDeviceToHost);
                if (e == hipSuccess) e = hipMemcpy(hs.h_d, hs.d_d, hs.n_out * sizeof(float), hipMemcpyDeviceToHost);
            }
            hs.busy = hs.redo = false;
        }
        if (e != hipSuccess && !first_rc) {
            first_rc = DPQ_ERR_HIP;
            first_msg = std::string("dpq_finish (results to the host): ") + hipGetErrorString(e);
        }
    }
    if (first_rc) return fail(first_rc, first_msg);
    return DPQ_OK;
    });
}

namespace {
int enqueue_async(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists, void* hip_stream,
                  bool allow_lanes, int host_slot = -1);
}

int dpq_query_batch_device_async(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                                 float* d_dists, void* hip_stream) {
    return guarded([&]() -> int { return enqueue_async(x, d_queries, nq, top_k, d_ids, d_dists, hip_stream, true); });
}

int dpq_query_batch_device_ordered(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                                   float* d_dists, void* hip_stream) {
    return guarded([&]() -> int { return enqueue_async(x, d_queries, nq, top_k, d_ids, d_dists, hip_stream, false); });
}

int dpq_finish_count(dpq_index* x, int32_t* rerun_batches) {
    return guarded([&]() -> int {
    if (!x) return fail(DPQ_ERR_ARG, "NULL index");
    const int64_t before = x->finish_reruns;
    int rc = dpq_finish(x);
    if (rerun_batches) *rerun_batches = (int32_t)(x->finish_reruns - before);
    return rc;
    });
}

namespace {
int enqueue_async(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists, void* hip_stream,
                  bool allow_lanes, int host_slot) {
    {
    int rc = check_batch_args(x, d_queries, nq, top_k, d_ids, d_dists);
    if (rc || nq == 0) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    hipStream_t user = reinterpret_cast<hipStream_t>(hip_stream);
    // DPQ_OPT_NO_ASYNC_OVERLAP: every batch on the caller's stream with one workspace (round 1's behaviour)
    const bool overlap = x->tune.async_overlap && allow_lanes;
    auto in_flight_on_other_stream = [&]() {
        for (const auto& p : x->pending)
            if (p.user_stream != user) return true;
        return false;
    };
    if (overlap) {
        // Laned batches are ordered by the caller's stream: a batch for another stream first settles what is in flight.
        if (in_flight_on_other_stream() && (rc = dpq_finish(x))) return rc;
    } else {
        // A stream-ordered batch runs on the caller's stream.  Batches still running on a lane's own stream are
        // settled first.  Up to TWO caller streams may have stream-ordered batches in flight: each is given one of the
        // two workspaces (a stream's batches follow each other, so its workspace is never shared) -- a caller that
        // alternates its steps between two streams gets the overlap of two lanes with every step still consumable in
        // stream order (the sharded driver: select -> pack -> all-gather -> merge behind each batch).  A third stream
        // settles everything first.
        bool laned = false;
        for (const auto& p : x->pending) laned = laned || p.stream != p.user_stream;
        if (laned && (rc = dpq_finish(x))) return rc;
        int lane = -1;
        for (int k = 0; k < 2; ++k)
            if (x->ordered_stream_set[k] && x->ordered_stream[k] == user) lane = k;
        if (lane < 0) {
            for (int k = 0; k < 2 && lane < 0; ++k) {
                bool busy = false;
                for (const auto& p : x->pending) busy = busy || (x->ordered_stream_set[k] && p.user_stream == x->ordered_stream[k]);
                if (!x->ordered_stream_set[k] || !busy) lane = k;
            }
            if (lane < 0) {
                if ((rc = dpq_finish(x))) return rc;
                lane = 0;
            }
            x->ordered_stream[lane] = user;
            x->ordered_stream_set[lane] = true;
        }
        use_lane(x, lane);
    }
    const int D = x->M * x->Ds;
    for (int base = 0; base < nq; base += kMaxBatchQueries) {
        const int n = std::min(kMaxBatchQueries, nq - base);
        if ((int)x->pending.size() >= dpq_index::kFlagSlots - 1 && (rc = dpq_finish(x))) return rc;
        const int slot = 1 + (int)x->pending.size();
        hipStream_t stream = user;
        if (overlap) {
            // the batch runs on its lane's stream once the caller's stream has reached this point (its inputs are
            // there); a lane's batches follow each other on the lane's stream, so its workspace is never shared
            const int lane = (int)(x->async_seq++ & 1);
            if (!x->lane_stream[lane]) {
                DPQ_HIP(hipStreamCreateWithFlags(&x->lane_stream[lane], hipStreamNonBlocking));
                DPQ_HIP(hipEventCreateWithFlags(&x->lane_ready[lane], hipEventDisableTiming));
            }
            use_lane(x, lane);
            stream = x->lane_stream[lane];
            DPQ_HIP(hipEventRecord(x->lane_ready[lane], user));
            DPQ_HIP(hipStreamWaitEvent(stream, x->lane_ready[lane], 0));
        }
        rc = run_batch(x, TableSource{d_queries + (size_t)base * D}, n, top_k, d_ids + (size_t)base * top_k,
                       d_dists + (size_t)base * top_k, stream, slot);
        if (rc) return rc;
        x->pending.push_back({d_queries + (size_t)base * D, n, top_k, d_ids + (size_t)base * top_k,
                              d_dists + (size_t)base * top_k, stream, user, slot, host_slot});
    }
    if (x->prof) {
        x->prof_acc.query_batches++;
        x->prof_acc.queries += nq;
    }
    return DPQ_OK;
    }
}
}  // namespace

}  // extern "C"

// dpq_query_batch_device and its filtered twin (filt != NULL): synchronous on `hip_stream`.
int query_device(dpq_index* x, const dpq_filter* filt, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                 float* d_dists, void* hip_stream) {
    if (x && !x->pending.empty()) {  // keep the order of the batches on this index
        int rc = dpq_finish(x);
        if (rc) return rc;
    }
    int rc = check_batch_args(x, d_queries, nq, top_k, d_ids, d_dists);
    if (rc || nq == 0) return rc;
    return query_device_src(x, filt, TableSource{d_queries}, nq, top_k, d_ids, d_dists, hip_stream);
}

namespace {
// The source of the sub-batch of n queries from query `base` on: device pointers advanced; tables in host memory go up
// into the handle's staging buffer (the batch before it has been answered: every caller is synchronous).
int sub_source(dpq_index* x, const TableSource& src, int base, int n, TableSource* s) {
    const size_t q_floats = (size_t)x->M * x->Ds, t_floats = (size_t)x->M * x->K;
    *s = src;
    if (s->d_queries) s->d_queries += (size_t)base * q_floats;
    if (s->d_tables) s->d_tables += (size_t)base * t_floats;
    if (src.h_tables) {
        DPQ_HIP(hipMemcpy(x->d_tab_stage, src.h_tables + (size_t)base * t_floats, (size_t)n * t_floats * sizeof(float),
                          hipMemcpyHostToDevice));
        s->d_tables = x->d_tab_stage;
    }
    return DPQ_OK;
}
}  // namespace

int query_device_src(dpq_index* x, const dpq_filter* filt, const TableSource& src, int nq, int top_k, int32_t* d_ids,
                     float* d_dists, void* hip_stream) {
    DPQ_HIP(hipSetDevice(x->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    for (int base = 0; base < nq; base += kMaxBatchQueries) {
        const int n = std::min(kMaxBatchQueries, nq - base);
        TableSource s;
        int rc = sub_source(x, src, base, n, &s);
        if (rc) return rc;
        rc = run_batch(x, s, n, top_k, d_ids + (size_t)base * top_k, d_dists + (size_t)base * top_k, stream, 0, filt);
        if (rc) return rc;
    }
    if (x->prof) {
        x->prof_acc.query_batches++;
        x->prof_acc.queries += nq;
    }
    return DPQ_OK;
}

int ensure_out_stage(dpq_index* x, size_t oe) {
    if (oe <= x->out_stage_elems) return DPQ_OK;
    x->out_stage_elems = 0;
    x->d_dists_stage.reset();
    int rc = x->d_ids_stage.alloc(oe);
    if (!rc) rc = x->d_dists_stage.alloc(oe);
    if (rc) return rc;
    x->out_stage_elems = oe;
    return DPQ_OK;
}

namespace {
// dpq_query_batch and its filtered twin: host buffers through the handle's staging buffers.
int query_host(dpq_index* x, const dpq_filter* filt, const float* queries, int nq, int top_k, int32_t* ids, float* dists) {
    if (!x || !queries || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, "NULL argument or nq < 0");
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, "dpq_set_codebook has not been called");
    if (nq == 0) return DPQ_OK;
    if (top_k < 1 || top_k > dpq::kMaxTopK) return fail(DPQ_ERR_ARG, "top_k must be in 1..2048");
    DPQ_HIP(hipSetDevice(x->device));
    const size_t qf = (size_t)nq * x->M * x->Ds, oe = (size_t)nq * top_k;
    if (qf > x->q_stage_floats) {
        x->q_stage_floats = 0;
        int rc = x->d_q_stage.alloc(qf);
        if (rc) return rc;
        x->q_stage_floats = qf;
    }
    if (int rc = ensure_out_stage(x, oe)) return rc;
    DPQ_HIP(hipMemcpy(x->d_q_stage, queries, qf * sizeof(float), hipMemcpyHostToDevice));
    int rc = query_device(x, filt, x->d_q_stage, nq, top_k, x->d_ids_stage, x->d_dists_stage, nullptr);
    if (rc) return rc;
    DPQ_HIP(hipDeviceSynchronize());
    DPQ_HIP(hipMemcpy(ids, x->d_ids_stage, oe * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, x->d_dists_stage, oe * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}
}  // namespace

int check_filter(const dpq_index* x, const dpq_filter* f) {
    if (!x) return fail(DPQ_ERR_ARG, "NULL index");
    if (!f) return fail(DPQ_ERR_ARG, "filter is NULL");
    if (f->owner != x->serial) return fail(DPQ_ERR_ARG, "the filter was made for another index handle");
    return DPQ_OK;
}

extern "C" {

int dpq_query_batch_device(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists,
                           void* hip_stream) {
    return guarded([&]() -> int { return query_device(x, nullptr, d_queries, nq, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_query_batch(dpq_index* x, const float* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int { return query_host(x, nullptr, queries, nq, top_k, ids, dists); });
}

int dpq_query_batch_filtered(dpq_index* x, const dpq_filter* f, const float* queries, int nq, int top_k, int32_t* ids,
                             float* dists) {
    return guarded([&]() -> int {
    int rc = check_filter(x, f);
    if (rc) return rc;
    return query_host(x, f, queries, nq, top_k, ids, dists);
    });
}

int dpq_query_batch_device_filtered(dpq_index* x, const dpq_filter* f, const float* d_queries, int nq, int top_k,
                                    int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    int rc = check_filter(x, f);
    if (rc) return rc;
    return query_device(x, f, d_queries, nq, top_k, d_ids, d_dists, hip_stream);
    });
}

int dpq_range_search(dpq_index* x, const float* queries, int nq, const float* radii, dpq_range_result** out) {
    return guarded([&]() -> int {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!x || nq < 0 || (nq > 0 && (!queries || !radii))) return fail(DPQ_ERR_ARG, "NULL argument or nq < 0");
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, "dpq_set_codebook has not been called");
    for (int q = 0; q < nq; ++q)
        if (std::isnan(radii[q])) return fail(DPQ_ERR_ARG, "radius of query " + std::to_string(q) + " is NaN");
    if (!x->pending.empty()) {  // keep the order of the batches on this index
        int rc = dpq_finish(x);
        if (rc) return rc;
    }
    if (nq > 0) {
        DPQ_HIP(hipSetDevice(x->device));
        const size_t qf = (size_t)nq * x->M * x->Ds;
        if (qf > x->q_stage_floats) {
            x->q_stage_floats = 0;
            int rc = x->d_q_stage.alloc(qf);
            if (rc) return rc;
            x->q_stage_floats = qf;
        }
        DPQ_HIP(hipMemcpy(x->d_q_stage, queries, qf * sizeof(float), hipMemcpyHostToDevice));
    }
    return range_search_src(x, TableSource{x->d_q_stage}, nq, radii, out);
    });
}

}  // extern "C"

int range_search_src(dpq_index* x, const TableSource& src, int nq, const float* radii, dpq_range_result** out) {
    x->range.last_max_keys = 0;
    std::unique_ptr<dpq_range_result> res(new dpq_range_result());
    res->nq = nq;
    res->lims.assign((size_t)nq + 1, 0);
    if (nq > 0) {
        DPQ_HIP(hipSetDevice(x->device));
        int rc = DPQ_OK;
        for (int base = 0; base < nq && !rc; base += kMaxBatchQueries) {
            const int n = std::min(kMaxBatchQueries, nq - base);
            TableSource s;
            if ((rc = sub_source(x, src, base, n, &s))) break;
            rc = range_batch(x, s, n, radii + base, base, res.get(), nullptr);
        }
        range_trim(x);
        if (rc) return rc;
        if (x->prof) x->prof_acc.queries += nq;
    }
    *out = res.release();
    return DPQ_OK;
}

extern "C" {

int dpq_range_result_get(const dpq_range_result* r, int32_t* nq, const int64_t** lims, const int32_t** ids,
                         const float** dists) {
    if (!r || !nq || !lims || !ids || !dists) return fail(DPQ_ERR_ARG, "NULL argument");
    *nq = r->nq;
    *lims = r->lims.data();
    *ids = r->ids.data();
    *dists = r->dists.data();
    return DPQ_OK;
}

void dpq_range_result_free(dpq_range_result* r) { delete r; }

// The reference's interface is host vectors in, host results out (h:2805-2810), one call per query (main:328-339).  Pipelined:
// the queries of batch i + 1 go up and the results of batch i - 1 come down (two copy streams) beside batch i's kernels
// (the two lanes of dpq_query_batch_device_async); dpq_finish settles everything and answers again, synchronously, any
// batch in which a query overflowed its candidate buffers.
int dpq_query_batch_host_async(dpq_index* x, const float* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    int rc = check_batch_args(x, queries, nq, top_k, ids, dists);
    if (rc || nq == 0) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    if (!x->copy_in) {
        DPQ_HIP(hipStreamCreateWithFlags(&x->copy_in, hipStreamNonBlocking));
        DPQ_HIP(hipStreamCreateWithFlags(&x->copy_out, hipStreamNonBlocking));
    }
    // batches enqueued through another entry point (another caller stream) are settled first: enqueue_async does that
    int slot = (int)(x->host_seq % dpq_index::kHostSlots);
    if (x->host_slots[slot].busy) {  // every slot in flight: settle them all (the oldest is the one wanted)
        if ((rc = dpq_finish(x))) return rc;
    }
    x->host_seq++;
    dpq_index::HostSlot& hs = x->host_slots[slot];
    const size_t qf = (size_t)nq * x->M * x->Ds, oe = (size_t)nq * top_k;
    if (qf > hs.qf) {
        hs.qf = 0;
        if ((rc = hs.d_q.alloc(qf))) return rc;
        hs.qf = qf;
    }
    // Page-locked result buffers (dpq_pin_host / hipHostRegister / hipHostMalloc) are mapped into the device's address
    // space: the select kernel then writes the lists straight into them (posted writes over PCIe) and no copy is
    // enqueued at all -- a hipMemcpyAsync costs the host ~10 us, three of them per batch held the pipelined rate at the
    // synchronous call's.  Pageable buffers take staging buffers and copies on copy_out.
    void *m_ids = nullptr, *m_d = nullptr;
    const bool direct = hipHostGetDevicePointer(&m_ids, ids, 0) == hipSuccess && hipHostGetDevicePointer(&m_d, dists, 0) == hipSuccess;
    if (!direct) (void)hipGetLastError();  // (an unregistered pointer is not an error of this call)
    if (!direct && oe > hs.oe) {
        hs.oe = 0;
        hs.d_d.reset();
        if ((rc = hs.d_ids.alloc(oe)) || (rc = hs.d_d.alloc(oe))) return rc;
        hs.oe = oe;
    }
    if (!hs.kernels_done) DPQ_HIP(hipEventCreateWithFlags(&hs.kernels_done, hipEventDisableTiming));
    // (pageable caller memory makes this copy synchronous with the host; pinned memory -- dpq_pin_host -- lets it overlap)
    DPQ_HIP(hipMemcpyAsync(hs.d_q, queries, qf * sizeof(float), hipMemcpyHostToDevice, x->copy_in));
    const size_t first = x->pending.size();
    int32_t* const out_ids = direct ? static_cast<int32_t*>(m_ids) : hs.d_ids.get();
    float* const out_d = direct ? static_cast<float*>(m_d) : hs.d_d.get();
    if ((rc = enqueue_async(x, hs.d_q, nq, top_k, out_ids, out_d, x->copy_in, true, slot))) return rc;
    // (enqueue_async may have settled older batches: the entries of this one are the pending tail)
    const size_t begin = std::min(first, x->pending.size());
    hs.h_ids = ids;
    hs.h_d = dists;
    hs.n_out = oe;
    hs.busy = true;
    hs.redo = false;
    hs.direct = direct;
    if (direct) return DPQ_OK;
    // results down once the batch's last kernel is through: the copy waits on every stream the batch's parts ran on
    std::vector<hipStream_t> seen;
    for (size_t i = begin; i < x->pending.size(); ++i) {
        const auto& p = x->pending[i];
        if (p.host_slot != slot || std::find(seen.begin(), seen.end(), p.stream) != seen.end()) continue;
        seen.push_back(p.stream);
        DPQ_HIP(hipEventRecord(hs.kernels_done, p.stream));
        DPQ_HIP(hipStreamWaitEvent(x->copy_out, hs.kernels_done, 0));
    }
    DPQ_HIP(hipMemcpyAsync(ids, hs.d_ids, oe * sizeof(int32_t), hipMemcpyDeviceToHost, x->copy_out));
    DPQ_HIP(hipMemcpyAsync(dists, hs.d_d, oe * sizeof(float), hipMemcpyDeviceToHost, x->copy_out));
    return DPQ_OK;
    });
}

// Page-locks / releases caller memory (hipHostRegister) so that dpq_query_batch_host_async's copies run beside the kernels;
// for callers that do not link the HIP runtime themselves.
int dpq_pin_host(void* ptr, int64_t bytes) {
    return guarded([&]() -> int {
    if (!ptr || bytes <= 0) return fail(DPQ_ERR_ARG, "NULL pointer or no bytes");
    DPQ_HIP(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
    return DPQ_OK;
    });
}

int dpq_unpin_host(void* ptr) {
    return guarded([&]() -> int {
    if (!ptr) return fail(DPQ_ERR_ARG, "NULL pointer");
    DPQ_HIP(hipHostUnregister(ptr));
    return DPQ_OK;
    });
}

int dpq_merge_topk_device(const int32_t* d_ids, const float* d_dists, int n_lists, int nq, int top_k,
                          int32_t* d_out_ids, float* d_out_dists, int device, void* hip_stream) {
    return guarded([&]() -> int {
    if (!d_ids || !d_dists || !d_out_ids || !d_out_dists || n_lists < 1 || nq < 0 || top_k < 1)
        return fail(DPQ_ERR_ARG, "bad merge argument");
    if ((int64_t)n_lists * top_k > 16384) return fail(DPQ_ERR_ARG, "n_lists * top_k exceeds 16384");
    if (nq == 0) return DPQ_OK;  // nothing to merge: no device is touched
    DPQ_HIP(hipSetDevice(device));
    DPQ_HIP(dpq::launch_merge(d_ids, d_dists, n_lists, nq, top_k, top_k, d_out_ids, d_out_dists,
                              reinterpret_cast<hipStream_t>(hip_stream)));
    return DPQ_OK;
    });
}

int dpq_merge_topk_device_packed(const int32_t* d_packed, int n_lists, int nq, int top_k, int32_t* d_out_ids,
                                 float* d_out_dists, int device, void* hip_stream) {
    return guarded([&]() -> int {
    if (!d_packed || !d_out_ids || !d_out_dists || n_lists < 1 || nq < 0 || top_k < 1)
        return fail(DPQ_ERR_ARG, "bad merge argument");
    if ((int64_t)n_lists * top_k > 16384) return fail(DPQ_ERR_ARG, "n_lists * top_k exceeds 16384");
    if (nq == 0) return DPQ_OK;  // nothing to merge: no device is touched
    DPQ_HIP(hipSetDevice(device));
    DPQ_HIP(dpq::launch_merge(d_packed, reinterpret_cast<const float*>(d_packed + top_k), n_lists, nq, top_k, 2 * top_k,
                              d_out_ids, d_out_dists, reinterpret_cast<hipStream_t>(hip_stream)));
    return DPQ_OK;
    });
}

int dpq_profile_enable(dpq_index* x, int on) {
    return guarded([&]() -> int {
    if (!x) return fail(DPQ_ERR_ARG, "NULL index");
    x->prof = on != 0;
    x->prof_scan_only = on == 2;
    return DPQ_OK;
    });
}

int dpq_profile_reset(dpq_index* x) {
    return guarded([&]() -> int {
    if (!x) return fail(DPQ_ERR_ARG, "NULL index");
    hipSetDevice(x->device);
    for (auto& ep : x->events) {
        x->ev_pool.push_back(ep.a);
        x->ev_pool.push_back(ep.b);
    }
    x->events.clear();
    memset(&x->prof_acc, 0, sizeof x->prof_acc);
    if (x->d_counters) hipMemset(x->d_counters, 0, 16);
    return DPQ_OK;
    });
}

int dpq_profile_read(dpq_index* x, dpq_profile* out) {
    return guarded([&]() -> int {
    if (!x || !out) return fail(DPQ_ERR_ARG, "NULL argument");
    DPQ_HIP(hipSetDevice(x->device));
    if (x->prof_failed) {
        x->prof_failed = false;
        return fail(DPQ_ERR_HIP, "a profiling event could not be created or recorded; timings are incomplete");
    }
    for (auto& ep : x->events) {
        DPQ_HIP(hipEventSynchronize(ep.b));
        float ms = 0.f;
        DPQ_HIP(hipEventElapsedTime(&ms, ep.a, ep.b));
        if (ep.kind == 0) x->prof_acc.lut_ms += ms;
        if (ep.kind == 1) x->prof_acc.scan_ms += ms;
        if (ep.kind == 2) x->prof_acc.select_ms += ms;
        if (ep.kind == 3) x->prof_acc.quantise_ms += ms;
        if (ep.kind == 4) x->prof_acc.decode_ms += ms;
        if (ep.kind == 5) x->prof_acc.bootstrap_ms += ms;
        x->ev_pool.push_back(ep.a);
        x->ev_pool.push_back(ep.b);
    }
    x->events.clear();
    if (x->d_counters) {
        unsigned long long h[2] = {0, 0};
        DPQ_HIP(hipMemcpy(h, x->d_counters, 16, hipMemcpyDeviceToHost));
        x->prof_acc.exact_checks = (int64_t)h[0];
        x->prof_acc.candidates = (int64_t)h[1];
    }
    *out = x->prof_acc;
    return DPQ_OK;
    });
}

}  // extern "C"
