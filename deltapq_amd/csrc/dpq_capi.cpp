// dpq_capi.cpp -- the C-ABI of include/deltapq_amd.h: index lifetime, the
// threshold-cascade driver around the scan/select kernels, profiling.
// Compiled with hipcc (HIP runtime calls only; kernels live in dpq_kernels.hip).
//
// There is no CPU implementation of the query in this library: every
// dpq_query_* call runs the HIP kernels or fails with an error code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <memory>
#include <new>
#include <numeric>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/deltapq_amd.h"
#include "dpq_build.h"
#include "dpq_filter.h"
#include "dpq_flat.h"
#include "dpq_format.h"
#include "dpq_kernels.h"
#include "dpq_lookup.h"
#include "dpq_opq.h"
#include "dpq_procrustes.h"
#include "dpq_refine.h"
#include "dpq_train.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

// No C++ exception may cross the C ABI (a corrupt header can ask for a multi-GB vector): every
// extern "C" entry point runs its body through guarded().
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(DPQ_ERR_NOMEM, "out of host memory");
    } catch (const std::length_error& e) {
        return fail(DPQ_ERR_NOMEM, std::string("allocation size out of range: ") + e.what());
    } catch (const std::exception& e) {
        return fail(DPQ_ERR_STATE, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(DPQ_ERR_STATE, "internal error: unknown exception");
    }
}

#define DPQ_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            return fail(DPQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
        }                                                                                          \
    } while (0)

template <class T>
int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return fail(DPQ_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return DPQ_OK;
}

// An owned device array: alloc() goes through dev_alloc's error path, the destructor frees it.  Reads as a T*.
template <class T>
class DevBuf {
  public:
    using value_type = T;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    // frees what it holds, then allocates `count` elements (at least one); on failure it holds nothing
    int alloc(size_t count) {
        reset();
        return dev_alloc(&p_, count);
    }
    void reset() {
        if (p_) hipFree(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

  private:
    T* p_ = nullptr;
};

struct EventPair {
    int kind;  // 0 lut, 1 scan, 2 select, 3 quantise, 4 per-batch decode, 5 bootstrap
    hipEvent_t a, b;
};

constexpr int kMaxBatchQueries = 2048;

}  // namespace

struct dpq_soa {
    dpq::SoA soa;
};

struct dpq_tree {
    dpq::Tree tree;
};

// dpq_range_search's answer: CSR lists in host memory, owned by the library until dpq_range_result_free.
struct dpq_range_result {
    int32_t nq = 0;
    std::vector<int64_t> lims;  // [nq + 1]
    std::vector<int32_t> ids;
    std::vector<float> dists;
};

// A filter of dpq_query_batch_*_filtered: the bitmap of the caller's reported ids, re-indexed by this handle's local
// node positions (bit l = node id_base + l, the even-N rule applied) and uploaded once.
struct dpq_filter {
    uint64_t owner = 0;              // dpq_index::serial of the handle it was made for
    DevBuf<uint32_t> bits;           // [n_segments x nodes per segment / 32] words
    int64_t n_allowed = 0;           // local nodes it allows
    mutable DevBuf<uint32_t> l0_id;  // the level-0 list with the nodes it does not allow as padding (run_batch)
    mutable int l0_n = -1;           // entries of l0_id (-1: not made yet)
    // what dpq_filter_combine and dpq_filter_to_bitmap need of the handle (filter_geom)
    int device = 0;
    bool plain = false;
    int64_t base = 0, n_local = 0, N = 0, n_words = 0;
};

inline uint64_t next_flat_serial() {
    static std::atomic<uint64_t> next{1};
    return next++;
}

// Raw vectors resident on one GPU (exact search).  An fp32 handle (dpq_flat.hip) stores rows padded to Dp floats; a byte
// handle (dpq_flat_u8.hip) stores them biased to int8 and padded to Dp bytes, with an int32 norm per row.
struct dpq_flat {
    int device = 0;
    int64_t n = 0, id_offset = 0;
    int D = 0, Dp = 0;
    bool u8 = false;              // opened by dpq_flat_open_u8
    DevBuf<float> base;           // [n][Dp]
    DevBuf<int8_t> base8;         // [n][Dp] (byte handle)
    DevBuf<int32_t> norm8;        // [n rounded up to 4]
    DevBuf<uint32_t> map;         // DFS position -> row (dpq_flat_set_id_map)
    std::vector<uint32_t> h_map;  // its host copy: dpq_flat_rerank checks candidates on the host
    // workspaces, grown on demand and kept until dpq_flat_close
    DevBuf<uint64_t> keys;
    DevBuf<dpq::FlatQueryState> state;
    DevBuf<float> d_q, d_dists;
    DevBuf<int32_t> d_ids, d_cand;
    DevBuf<uint32_t> flag;
    DevBuf<uint8_t> q_raw;        // a byte handle's queries as given, biased and padded into q8, their norms in qnorm
    DevBuf<int8_t> q8;
    DevBuf<int32_t> qnorm;
    size_t keys_n = 0, state_n = 0, q_n = 0, out_n = 0, cand_n = 0, q_raw_n = 0, q8_n = 0, qnorm_n = 0;
    // filtered and range search
    const uint64_t serial = next_flat_serial();  // what a dpq_flat_filter remembers of the handle it was made for
    DevBuf<uint64_t> r_thr, r_pool, r_sorted;    // radius keys of a query batch; the lists of a sub-batch, unsorted / sorted
    DevBuf<int64_t> r_offs;                      // [queries of a sub-batch + 1] list starts in the pool
    size_t r_thr_n = 0, r_pool_n = 0, r_sorted_n = 0, r_offs_n = 0;
};

// A filter of dpq_flat_search_filtered* / dpq_flat_range_search*: the ascending list of the handle's eligible rows.
struct dpq_flat_filter {
    uint64_t owner = 0;      // dpq_flat::serial
    int device = 0;
    DevBuf<uint32_t> list;   // [n_allowed]
    int64_t n_allowed = 0;
};

namespace {
uint64_t next_index_serial() {
    static std::atomic<uint64_t> next{1};
    return next++;
}
}  // namespace

// Plan and tiling knobs of a handle: dpq_open_opts' fields with the defaults filled in (resolve_tuning).
struct Tuning {
    // batches up to this size take stream_kernel (1, 2 or 4 queries per pass).  Measured at 125 M codes (ms per call,
    // stream / 64-query filter path): 1 query 0.64 / 1.26, 2: 0.66 / 1.22, 4: 0.85 / 1.22, 8 (two passes of four, or one of
    // eight at 8 wavefronts per CU): 1.7-2.3 / 1.21, 16: 4.3 / 1.23 -- the switch-over sits behind four
    int stream_max = 4;
    int coarse_below = 128;
    int plan_ratios[3] = {0, 0, 0};
    int boot_cap = 0, boot_target = 0;
    int boot_variant = 1;  // bootstrap_kernel's V (dpq_kernels.hip); 0 = the kernel of rounds 2 - 3  [DPQ_BOOT_VARIANT]
    int select_threads = 0;  // select_kernel block size, 0 = by top_k  [DPQ_SELECT_THREADS]
    int select_fast = 1;     // the last level as a bucket sort from one histogram pass (select_kernel)  [DPQ_SELECT_FAST=0: radix select + rank count / bitonic network]
    int64_t batch_tile_nodes = (int64_t)16 << 20;
    bool relabel = true, fuse_quantise = true, async_overlap = true, boot_fullsort = false, tighten = true, strands = true,
         force_strands = false;
    bool strand1 = true;  // one query per pass takes strand1_kernel  [DPQ_OPT_NO_STRAND1, DPQ_STRAND1=0: strand_kernel<1>]
    int s1_debug = 0;     // developer experiments of strand1_kernel  [DPQ_S1_DEBUG]
};

// The device buffers of dpq_range_search beside the lanes' workspaces (which it uses for its tables only).  The slot
// arrays hold one sub-batch; the candidate and output buffers grow to what a call needs.
struct RangeWs {
    DevBuf<int32_t> slot_query;    // [kMaxBatchQueries] slot -> query of the sub-batch
    DevBuf<uint64_t> thr_key;      // [kMaxBatchQueries]
    DevBuf<int64_t> out_off;       // [kMaxBatchQueries] where a slot's list goes in the output chunk
    DevBuf<uint32_t> max_count;    // [kMaxBatchQueries]
    DevBuf<int64_t> lims;          // [kMaxBatchQueries + 1]
    DevBuf<uint32_t> cand_count;   // [kMaxBatchQueries][kRegionStride]
    DevBuf<uint64_t> cand_key;     // [slots][splits * region_cap]
    DevBuf<int32_t> out_ids;
    DevBuf<float> out_dists;
    DevBuf<uint64_t> scratch;      // [2 * out] HBM sort of lists beyond the emit kernel's LDS
    size_t key_n = 0, out_n = 0, scratch_n = 0;
    int64_t last_max_keys = 0;     // candidate keys the largest scan launch of the last call laid out (dpq_debug_range_keys)
};

// The device buffers of the code lookup (dpq_get_codes / dpq_reconstruct / dpq_decode_range), apart from every search
// lane's workspace.  The staging buffers of the host variants hold one slice; the tile is dpq_decode_range's scratch.
struct LookupWs {
    DevBuf<uint32_t> flag;       // [1] raised by a request that names no node of the handle
    DevBuf<int32_t> ids;         // [slice] host variants: the slice's ids
    DevBuf<uint8_t> codes;       // [slice][M]
    DevBuf<float> vecs;          // [slice rows][M * Ds]
    DevBuf<uint8_t> tile;        // [tile segments][S][M] decoded codes of dpq_decode_range's current tile
    DevBuf<uint32_t> tile_segs;  // [tile segments] the tile's segment list
    size_t ids_n = 0, codes_n = 0, vecs_n = 0, tile_n = 0, tile_segs_n = 0;
};

// The device buffers a batch works in (one per pipeline lane), sized for `slots` padded queries and `cap` candidates each.
struct Workspace {
    int slots = 0, cap = 0;
    DevBuf<float> d_lut32;         // exact tables [query][8][256]
    DevBuf<float> d_lut32r;        // the same, rows by the labels of the plain-code scratch (only with d_relabel)
    DevBuf<float> d_lut_min;       // [query][8] minima (anchor of the filter quantisation)
    DevBuf<uint4> d_qtab;          // [slot groups][128 KB] filter tables of the cascade level being scanned
    DevBuf<uint32_t> d_cand_count;
    DevBuf<uint32_t> d_overflow;   // [slots] overflow flags
    DevBuf<uint32_t> d_tight;      // [slots][kTightWords] tightening counters of the level being scanned (strand1: its
                                   // one slot's kS1HistWords, what one query group's rows hold)
    DevBuf<uint64_t> d_cand_key, d_thr_key;  // candidate keys [slots][cap], threshold keys [slots]
    DevBuf<uint64_t> d_scratch;    // [slots][cap] contiguous copy of a slot's keys when they exceed the select's LDS list
    DevBuf<uint8_t> d_batch_raw;   // tiled plain-code scratch (a shard larger than one tile): the tile being scanned, decoded
                                   // per batch; kept when the rest grows.  A one-tile shard: dpq_index::d_plain_image
};

struct dpq_index {
    Tuning tune;
    const uint64_t serial = next_index_serial();  // unique per handle of the process (dpq_filter's owner)
    int device = 0;
    int M = 8, K = 256, Ds = 0;
    int cap = 0;
    bool cap_auto = true;
    dpq_info info{};
    dpq::DeviceImage img;
    // owned device memory of the image
    // strand image (dpq_format.h): the stream pass's own layout of the same nodes (M = 8, shards with a bootstrap)
    DevBuf<uint64_t> d_st_ckpt;
    DevBuf<uint32_t> d_st_mask;
    DevBuf<uint16_t> d_st_depth;
    DevBuf<uint32_t> d_st_pbase, d_strip_order;
    DevBuf<uint32_t> d_strip_segs;         // the segments of the strips, in strip visiting order (a level too small for the
    std::vector<int64_t> strip_seg_off;    // strand pass runs the chunk-per-wavefront pass over ITS strips' segments)
    DevBuf<uint8_t> d_st_delta;
    int64_t strand_bytes = 0;
    DevBuf<uint8_t> d_nib, d_par, d_carry, d_mask, d_delta, d_ckpt, d_raw;
    bool plain = false;  // uncompressed comparator index (fp32-accumulate rule, no id quirk)
    DevBuf<uint64_t> d_seg_off;
    // threshold bootstrap: inverted multi-index over the shard's nodes (dpq::SoA::mi_*); boot = it is in use
    DevBuf<uint32_t> d_mi_cell, d_mi_code, d_mi_id;
    bool boot = false;
    int boot_classes = 0;
    DevBuf<unsigned long long> d_boot_stamps;  // developer diagnostics (dpq_debug_boot_stamps)
    DevBuf<unsigned long long> d_s1_stamps;    // developer diagnostics (dpq_debug_strand1_stamps)
    int batch_decode = 0;            // dpq_open_opts.batch_decode
    DevBuf<uint8_t> d_relabel;       // [M][256] code value -> label in the plain-code scratch (bank-aware; NULL = code values)
    // The plain-code image of a shard that one tile holds (batch_tile_segments): every node's (relabelled) codes in
    // shard order, shared by both lanes and every entry point.  It is decoded ONCE per handle, by the first batch that
    // scans it, on that batch's stream (ensure_plain_image).  Nothing invalidates it: its only inputs are the device
    // image and d_relabel, both fixed at dpq_open_*; dpq_set_codebook changes tables, never codes.
    DevBuf<uint8_t> d_plain_image;
    hipEvent_t image_done = nullptr;     // recorded behind the decode
    hipStream_t image_stream = nullptr;  // the stream the decode was enqueued on
    int image_state = 0;                 // 0: not decoded; 1: enqueued, batches on other streams wait for image_done;
                                         // 2: the host has seen image_done complete, nothing waits any more
    DevBuf<uint8_t> d_nbr;           // [8][256][256] centroid neighbour lists of the bootstrap's sub-spaces (dpq_set_codebook)
    DevBuf<float> d_codebook;
    DevBuf<unsigned long long> d_counters;  // [2] scan statistics (dpq_profile.exact_checks / candidates)
    uint32_t* h_overflow = nullptr;  // pinned
    // pinned + mapped words, one per batch in flight: set by select_kernel when any query of the batch overflowed
    static constexpr int kFlagSlots = 64;
    uint32_t* h_any = nullptr;       // [kFlagSlots]; slot 0 serves the synchronous calls
    uint32_t* d_any = nullptr;       // device address of h_any
    struct Pending {                 // a batch enqueued by dpq_query_batch_device_async and not yet finished
        const float* d_queries;
        int nq, top_k;
        int32_t* d_ids;
        float* d_dists;
        hipStream_t stream;          // the stream it runs on (the caller's, or one of the two lane streams)
        hipStream_t user_stream;     // the stream the caller enqueued it on
        int flag_slot;
        int host_slot = -1;          // >= 0: a dpq_query_batch_host_async batch staged in host_slots[host_slot]
    };
    // dpq_query_batch_host_async: up to kHostSlots batches in flight, each with its own staging buffers; queries go up
    // on copy_in (the lanes' batches wait for it), results come down on copy_out behind the batch's last kernel
    static constexpr int kHostSlots = 16;
    struct HostSlot {
        DevBuf<float> d_q;
        DevBuf<int32_t> d_ids;
        DevBuf<float> d_d;
        size_t qf = 0, oe = 0;       // capacities (floats / elements)
        int32_t* h_ids = nullptr;    // the caller's buffers of the batch in flight
        float* h_d = nullptr;
        size_t n_out = 0;
        bool busy = false, redo = false;
        bool direct = false;         // the result buffers are page-locked and mapped: the select kernel writes them itself
        hipEvent_t kernels_done = nullptr;
    };
    HostSlot host_slots[kHostSlots];
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    uint64_t host_seq = 0;
    // Pipelined batches alternate between two LANES = two workspaces + two internal streams, so that a batch's
    // table build runs under the previous batch's scan (the scan fills every CU's LDS and half its wave slots:
    // the LUT kernel needs neither) and its bootstrap next to the previous batch's select.  Every batch works in
    // the ACTIVE lane's workspace.
    Workspace lane[2];
    int active_lane = 0;
    Workspace& ws() { return lane[active_lane]; }
    const Workspace& ws() const { return lane[active_lane]; }
    hipStream_t lane_stream[2] = {nullptr, nullptr};
    hipEvent_t lane_ready[2] = {nullptr, nullptr};   // recorded on the caller's stream: the batch's inputs are there
    uint64_t async_seq = 0;
    hipStream_t ordered_stream[2] = {nullptr, nullptr};  // caller streams with stream-ordered batches: stream k <-> workspace k
    bool ordered_stream_set[2] = {false, false};
    int64_t finish_reruns = 0;       // batches dpq_finish had to answer again (a query overflowed its candidate buffers)
    std::vector<Pending> pending;
    // staging for the host-pointer entry point
    DevBuf<float> d_q_stage;
    DevBuf<int32_t> d_ids_stage;
    DevBuf<float> d_dists_stage;
    size_t q_stage_floats = 0, out_stage_elems = 0;
    // cascade plan: visiting order of the segments, level bounds, decoded level 0
    int plan_top_k = -1, plan_cap = -1, plan_coarse = -1;
    std::vector<int> level_off, level_cnt;
    RangeWs range;                   // dpq_range_search
    LookupWs lookup;                 // dpq_get_codes / dpq_reconstruct / dpq_decode_range
    DevBuf<uint32_t> d_vec_id;       // [n_local] local node -> original vector id (dpq_set_vec_ids; the _vec filter constructors)
    bool vec_ids_set = false;
    DevBuf<unsigned long long> d_filter_count;  // [1] the set bits of the filter being built (dpq_filter_create_* on the device)
    DevBuf<uint32_t> d_order;
    DevBuf<uint32_t> d_l0_id, d_l0_code;
    int l0_segments = 0;
    // profiling
    bool prof = false;
    bool prof_scan_only = false;     // events around the scan launches only (each event pair costs ~4 us of stream time)
    std::vector<EventPair> events;
    std::vector<hipEvent_t> ev_pool;
    dpq_profile prof_acc{};
    hipEvent_t get_event() {
        if (!ev_pool.empty()) {
            hipEvent_t e = ev_pool.back();
            ev_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        // timing events between kernels of one stream: no system-scope fence needed (saves ~2 us per record)
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) {
            prof_failed = true;
            return nullptr;
        }
        return e;
    }
    bool prof_failed = false;        // an event could not be created / recorded: dpq_profile_read reports it
    // developer hooks (dpq_debug_scan_time mode 3): the last batch's bootstrap and first-level scan launches as they were;
    // they point into the active workspace, so switching lanes or growing the workspace clears them
    dpq::BootArgs dbg_ba{};
    dpq::ScanArgs dbg_sa{};
    int dbg_boot_slots = 0, dbg_groups = 0, dbg_splits = 0;
};

namespace {

// Developer diagnostics (the dpq_debug_* entry points, include/deltapq_amd.h) and developer environment variables are
// live only in a process started with DPQ_DEV=1.
bool dev_mode() {
    const char* dev = getenv("DPQ_DEV");
    return dev && atoi(dev) != 0;
}
#define DPQ_DEV_ONLY() \
    if (!dev_mode()) return fail(DPQ_ERR_STATE, "developer diagnostics: start the process with DPQ_DEV=1")

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
    if ((rc = w.d_qtab.alloc((size_t)(slots / dpq::queries_per_group(x->M) + 1) *
                             (dpq::qtab_bytes_per_group(x->M) / sizeof(uint4)))))
        return rc;
    if ((rc = w.d_cand_count.alloc((size_t)slots * dpq::kRegionStride))) return rc;
    if ((rc = w.d_cand_key.alloc((size_t)slots * cap))) return rc;
    if ((rc = w.d_scratch.alloc((size_t)slots * cap))) return rc;
    if ((rc = w.d_overflow.alloc((size_t)slots))) return rc;
    if ((rc = w.d_tight.alloc((size_t)slots * dpq::kTightWords))) return rc;
    if ((rc = w.d_thr_key.alloc((size_t)slots))) return rc;
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

int splits_for(int n_seg_pass, int n_groups) {
    // One workgroup per CU is resident (LDS), so aim at ONE chip-wave: <= 256 workgroups.  Small levels
    // still spread over as many CUs as they have segments: the exact checks of the filter survivors
    // are bound by each CU's vector-memory address rate, not by its wavefront count.
    const int want = std::max(1, dpq::kMaxSplits / std::max(1, n_groups));
    return std::max(1, std::min(n_seg_pass, want));
}

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
int build_tables(dpq_index* x, const Batch& b, const float* d_queries, hipStream_t stream) {
    Workspace& w = x->ws();
    int rc;
    if (b.one_tile && (rc = ensure_plain_image(x, stream))) return rc;
    {
        Timer t(x, stream, 0);
        // batches that scan the plain-code scratch also get the tables in the scratch's label order
        DPQ_HIP(dpq::launch_lut_build(x->d_codebook, d_queries, b.nq, b.nqp, x->M, x->K, x->Ds, w.d_lut32, w.d_lut_min,
                                      nullptr, w.d_overflow, b.scratch ? x->d_relabel.get() : nullptr, w.d_lut32r,
                                      x->tune.tighten ? w.d_tight.get() : nullptr, stream));
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

// Filter level l >= 1 (sa.seg_list / n_seg_pass): its tables, then its scan by every query group -- in tiles of the
// plain-code scratch (decode a tile in list order, scan it with all groups, next tile) where one tile does not hold the
// shard.
int filter_level(dpq_index* x, const Batch& b, size_t l, dpq::ScanArgs sa, dpq::SelectArgs& se, hipStream_t stream) {
    const Workspace& w = x->ws();
    const Regions rg = regions_for(x, sa.n_seg_pass, b.ngroups, b.top_k, b.cap);
    sa.region_cap = se.region_cap = rg.region_cap;
    se.n_regions = 1 + rg.splits;
    if (!(b.boot_tables && l == 1)) {  // the bootstrap kernel wrote the first level's tables itself
        Timer t(x, stream, 3);
        DPQ_HIP(dpq::launch_quantise(sa, b.ngroups, stream));
    }
    if (b.scratch && !b.one_tile) {
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
            {
                Timer t(x, stream, 1);
                DPQ_HIP(dpq::launch_scan(tile, b.ngroups, rg.splits, stream));
            }
            if (x->prof && t0 > 0) x->prof_acc.scan_launches++;
        }
    } else {
        Timer t(x, stream, 1);
        DPQ_HIP(dpq::launch_scan(sa, b.ngroups, rg.splits, stream));
        if (l == 1 && !sa.filter) {
            x->dbg_sa = sa;
            x->dbg_groups = b.ngroups;
            x->dbg_splits = rg.splits;
        }
    }
    if (x->prof) {
        x->prof_acc.scan_launches++;
        x->prof_acc.scan_stream_bytes +=
            (int64_t)((double)x->info.device_bytes * sa.n_seg_pass / std::max(1, x->img.n_segments));
    }
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
int run_batch(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists,
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
    if ((rc = build_tables(x, b, d_queries, stream))) return rc;
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

template <class T>
int grow(DevBuf<T>& buf, size_t* have, size_t want) {
    if (want <= *have && buf) return DPQ_OK;
    *have = 0;
    int rc = buf.alloc(want);
    if (!rc) *have = want;
    return rc;
}

// The filter scan of one range launch: the slots' tables from their thresholds, then every segment -- in tiles of the
// plain-code scratch where one tile does not hold the shard (as filter_level does).
int range_scan(dpq_index* x, const Batch& b, dpq::ScanArgs sa, int n_groups, int splits, hipStream_t stream) {
    const Workspace& w = x->ws();
    DPQ_HIP(hipMemsetAsync(sa.cand_count, 0, sizeof(uint32_t) * (size_t)n_groups * dpq::queries_per_group(x->M) *
                                                 dpq::kRegionStride, stream));
    if (sa.n_seg_pass <= 0) return DPQ_OK;
    {
        Timer t(x, stream, 3);
        DPQ_HIP(dpq::launch_quantise(sa, n_groups, stream));
    }
    if (b.scratch && !b.one_tile) {
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
    } else {
        Timer t(x, stream, 1);
        DPQ_HIP(dpq::launch_scan(sa, n_groups, splits, stream));
        if (x->prof) x->prof_acc.scan_launches++;
    }
    return DPQ_OK;
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

// One sub-batch (nq <= kMaxBatchQueries) of dpq_range_search: d_queries on the device, radii on the host; appends its
// lists to res (res->lims[base .. base + nq] are filled, base = the number of queries before it).
int range_batch(dpq_index* x, const float* d_queries, int nq, const float* radii, int base, dpq_range_result* res,
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
    if ((rc = build_tables(x, b, d_queries, stream))) return rc;

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

void fill_info_from_soa(const dpq::SoA& s, dpq_info* inf) {
    memset(inf, 0, sizeof *inf);
    inf->n_codes_total = s.n_codes_total;
    inf->n_bytes_total = s.n_bytes_total;
    inf->node_lo = s.node_lo;
    inf->node_hi = s.node_hi;
    inf->algorithmic_bytes = s.algorithmic_bytes;
    inf->device_bytes = s.device_bytes();
    inf->bootstrap_bytes = s.bootstrap_bytes();
    inf->bootstrap_stride = s.mi_stride;
    inf->strand_bytes = s.n_strips > 0 ? s.strand_bytes() : 0;
    inf->n_diffs = s.n_diffs;
    inf->M = s.M;
    inf->n_segments = (int32_t)s.n_segments;
    inf->chunks_per_segment = s.chunks_per_segment;
    inf->max_depth = s.max_depth;
    inf->device = -1;
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

int dpq_read_dtc_header(const char* path, int64_t* n_codes, int64_t* n_bytes) {
    return guarded([&]() -> int {
    if (!path || !n_codes || !n_bytes) return fail(DPQ_ERR_ARG, "NULL argument");
    std::string err;
    int rc = dpq::read_dtc_header(path, n_codes, n_bytes, &err);
    return rc ? fail(rc, err) : DPQ_OK;
    });
}

int dpq_read_codewords(const char* path, int32_t* M, int32_t* K, int32_t* Ds, float* out) {
    return guarded([&]() -> int {
    if (!path || !M || !K || !Ds) return fail(DPQ_ERR_ARG, "NULL argument");
    std::string err;
    std::vector<float> v;
    int m, k, ds;
    int rc = dpq::read_codewords(path, &m, &k, &ds, out ? &v : nullptr, &err);
    if (rc) return fail(rc, err);
    *M = m;
    *K = k;
    *Ds = ds;
    if (out) memcpy(out, v.data(), v.size() * sizeof(float));
    return DPQ_OK;
    });
}

int dpq_read_vecs(const char* path, int is_bvecs, int64_t* n, int32_t* D, float* out, int64_t cap) {
    return guarded([&]() -> int {
    if (!path || !n || !D) return fail(DPQ_ERR_ARG, "NULL argument");
    std::string err;
    std::vector<float> v;
    int d = 0;
    int rc = dpq::read_vecs(path, is_bvecs != 0, n, &d, out ? &v : nullptr, cap, &err);
    if (rc) return fail(rc, err);
    *D = d;
    if (out) memcpy(out, v.data(), v.size() * sizeof(float));
    return DPQ_OK;
    });
}

int dpq_dtc_file_name(const char* dataset_dir, int M, int K, int64_t N, char* out, int64_t out_len) {
    return guarded([&]() -> int {
    if (!dataset_dir || !out) return fail(DPQ_ERR_ARG, "NULL argument");
    std::string s = dpq::dtc_file_name(dataset_dir, M, K, N);
    if ((int64_t)s.size() + 1 > out_len) return fail(DPQ_ERR_ARG, "output buffer too small");
    memcpy(out, s.c_str(), s.size() + 1);
    return DPQ_OK;
    });
}

int dpq_dtc_validate(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, dpq_dtc_stats* stats) {
    return guarded([&]() -> int {
    std::string err;
    int rc = dpq::validate(payload, n_bytes, n_codes, M, stats, &err);
    return rc ? fail(rc, err) : DPQ_OK;
    });
}

int dpq_soa_build(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, const dpq_open_opts* opts,
                  dpq_soa** out) {
    return guarded([&]() -> int {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    dpq_open_opts o{};
    if (opts) o = *opts;
    dpq_soa* s = new dpq_soa();
    std::string err;
    int rc = dpq::transcode(payload, n_bytes, n_codes, M, o.shard_rank, o.shard_count, o.chunks_per_segment, &s->soa,
                            &err, o.num_codes, o.bootstrap > 0 && M % 4 == 0 ? o.bootstrap : 0);
    if (rc) {
        delete s;
        *out = nullptr;
        return fail(rc, err);
    }
    *out = s;
    return DPQ_OK;
    });
}

int dpq_soa_info(const dpq_soa* soa, dpq_info* info) {
    return guarded([&]() -> int {
    if (!soa || !info) return fail(DPQ_ERR_ARG, "NULL argument");
    fill_info_from_soa(soa->soa, info);
    return DPQ_OK;
    });
}

int dpq_soa_array(const dpq_soa* soa, int which, const void** ptr, int64_t* n_bytes) {
    return guarded([&]() -> int {
    if (!soa || !ptr || !n_bytes) return fail(DPQ_ERR_ARG, "NULL argument");
    const dpq::SoA& s = soa->soa;
    switch (which) {
        case 0: *ptr = s.nib.data(); *n_bytes = (int64_t)s.nib.size(); break;
        case 1: *ptr = s.mask.data(); *n_bytes = (int64_t)s.mask.size(); break;
        case 2: *ptr = s.delta.data(); *n_bytes = (int64_t)s.delta.size(); break;
        case 3: *ptr = s.seg_delta_off.data(); *n_bytes = (int64_t)s.seg_delta_off.size() * 8; break;
        case 4: *ptr = s.seg_ckpt.data(); *n_bytes = (int64_t)s.seg_ckpt.size(); break;
        case 5: *ptr = s.mi_cell_start.data(); *n_bytes = (int64_t)s.mi_cell_start.size() * 4; break;
        case 6: *ptr = s.mi_code.data(); *n_bytes = (int64_t)s.mi_code.size() * 4; break;
        case 7: *ptr = s.mi_id.data(); *n_bytes = (int64_t)s.mi_id.size() * 4; break;
        case 8: *ptr = s.par.data(); *n_bytes = (int64_t)s.par.size(); break;
        case 9: *ptr = s.carry.data(); *n_bytes = (int64_t)s.carry.size(); break;
        case 10: *ptr = s.st_ckpt.data(); *n_bytes = (int64_t)s.st_ckpt.size() * 8; break;
        case 11: *ptr = s.st_mask.data(); *n_bytes = (int64_t)s.st_mask.size() * 4; break;
        case 12: *ptr = s.st_poff.data(); *n_bytes = (int64_t)s.st_poff.size() * 2; break;
        case 13: *ptr = s.st_pbase.data(); *n_bytes = (int64_t)s.st_pbase.size() * 4; break;
        case 14: *ptr = s.st_delta.data(); *n_bytes = (int64_t)s.st_delta.size(); break;
        case 15: *ptr = s.st_depth.data(); *n_bytes = (int64_t)s.st_depth.size() * 2; break;
        default: return fail(DPQ_ERR_ARG, "which must be 0..15");
    }
    return DPQ_OK;
    });
}

void dpq_soa_free(dpq_soa* soa) { delete soa; }

int dpq_dtc_encode(const uint8_t* root_code, const uint8_t* depths, const uint16_t* masks, const uint8_t* deltas,
                   int64_t n_codes, int M, uint8_t* out, int64_t* n_bytes) {
    return guarded([&]() -> int {
    std::string err;
    int rc = dpq::encode(root_code, depths, masks, deltas, n_codes, M, out, n_bytes, &err);
    return rc ? fail(rc, err) : DPQ_OK;
    });
}

int dpq_tree_build(const uint8_t* codes, int64_t n_codes, int M, int K, int max_height_folds, const float* codewords,
                   int Ds, dpq_tree** out) {
    return guarded([&]() -> int {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    dpq_tree* t = new dpq_tree();
    std::string err;
    int rc = dpq::build_tree(codes, n_codes, M, K, max_height_folds, codewords, Ds, &t->tree, &err);
    if (rc) {
        delete t;
        return fail(rc, err);
    }
    *out = t;
    return DPQ_OK;
    });
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

int dpq_tree_stats(const dpq_tree* t, dpq_dtc_stats* stats) {
    return guarded([&]() -> int {
    if (!t || !stats) return fail(DPQ_ERR_ARG, "NULL argument");
    const dpq::Tree& tr = t->tree;
    memset(stats, 0, sizeof *stats);
    stats->n_codes = tr.n;
    stats->n_diffs = tr.n_diffs;
    stats->n_bytes = tr.M + tr.n_diffs + (tr.n - 1) * dpq::mask_bytes_for(tr.M) + tr.n / 2;  // h:1765 for M = 8
    for (int d = 0; d < 16; ++d) stats->depth_hist[d] = tr.depth_hist[d];
    stats->max_depth = tr.max_depth;
    stats->M = tr.M;
    return DPQ_OK;
    });
}

int dpq_tree_array(const dpq_tree* t, int which, const void** ptr, int64_t* n_bytes) {
    return guarded([&]() -> int {
    if (!t || !ptr || !n_bytes) return fail(DPQ_ERR_ARG, "NULL argument");
    const dpq::Tree& tr = t->tree;
    switch (which) {
        case 0: *ptr = tr.vec_id.data(); *n_bytes = (int64_t)tr.vec_id.size() * 4; break;
        case 1: *ptr = tr.parent_pos.data(); *n_bytes = (int64_t)tr.parent_pos.size() * 4; break;
        case 2: *ptr = tr.depth.data(); *n_bytes = (int64_t)tr.depth.size(); break;
        case 3: *ptr = tr.mask.data(); *n_bytes = (int64_t)tr.mask.size() * 2; break;
        case 4: *ptr = tr.deltas.data(); *n_bytes = (int64_t)tr.deltas.size(); break;
        case 5: *ptr = tr.root_code.data(); *n_bytes = (int64_t)tr.root_code.size(); break;
        case 6: *ptr = tr.edges.data(); *n_bytes = (int64_t)tr.edges.size() * 8; break;
        default: return fail(DPQ_ERR_ARG, "which must be 0..6");
    }
    return DPQ_OK;
    });
}

int dpq_tree_encode(const dpq_tree* t, uint8_t* out, int64_t* n_bytes) {
    return guarded([&]() -> int {
    if (!t || !n_bytes) return fail(DPQ_ERR_ARG, "NULL argument");
    const dpq::Tree& tr = t->tree;
    std::string err;
    int rc = dpq::encode(tr.root_code.data(), tr.depth.data(), tr.mask.data(), tr.deltas.data(), tr.n, tr.M, out,
                         n_bytes, &err);
    return rc ? fail(rc, err) : DPQ_OK;
    });
}

int dpq_tree_write_files(const dpq_tree* t, const char* dataset_dir) {
    return guarded([&]() -> int {
    if (!t || !dataset_dir) return fail(DPQ_ERR_ARG, "NULL argument");
    std::string err;
    int rc = dpq::tree_write_files(t->tree, dataset_dir, &err);
    return rc ? fail(rc, err) : DPQ_OK;
    });
}

void dpq_tree_free(dpq_tree* t) { delete t; }

int dpq_read_qnode_ids(const char* path, int64_t n_codes, uint32_t* vec_ids) {
    return guarded([&]() -> int {
    if (!path || !vec_ids || n_codes < 0) return fail(DPQ_ERR_ARG, "bad argument");
    std::vector<uint32_t> ids;
    std::string err;
    int rc = dpq::read_qnode_ids(path, n_codes, &ids, &err);
    if (rc) return fail(rc, err);
    memcpy(vec_ids, ids.data(), ids.size() * 4);
    return DPQ_OK;
    });
}

int dpq_read_codes_plain(const char* path, int M, int64_t* n_codes, uint8_t* out) {
    return guarded([&]() -> int {
    if (!path || !n_codes || M < 1) return fail(DPQ_ERR_ARG, "bad argument");
    std::vector<uint8_t> codes;
    std::string err;
    int rc = dpq::read_codes_plain(path, M, n_codes, out ? &codes : nullptr, &err);
    if (rc) return fail(rc, err);
    if (out) memcpy(out, codes.data(), codes.size());
    return DPQ_OK;
    });
}

int dpq_read_codes_plain_ex(const char* path, int M, int K, int with_id, int64_t* n_codes, uint8_t* codes_out,
                            int32_t* ids_out) {
    return guarded([&]() -> int {
    if (!path || !n_codes || M < 1 || K < 1) return fail(DPQ_ERR_ARG, "bad argument");
    if (K > 256 && with_id) return fail(DPQ_ERR_ARG, "K > 256 with ids is not implemented in the reference either (pq_tree.cpp:1051-1054)");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    int64_t n = 0;
    if (fread(&n, sizeof(int64_t), 1, f) != 1 || n < 0 || n > (int64_t)INT32_MAX) {
        fclose(f);
        return fail(DPQ_ERR_FORMAT, std::string("bad header in ") + path);
    }
    *n_codes = n;
    int rc = DPQ_OK;
    if (codes_out || ids_out) {
        const size_t cb = (size_t)M * (K > 256 ? 2 : 1), rec = cb + (with_id ? 4 : 0);
        std::vector<uint8_t> buf((size_t)std::min<int64_t>(n, 1 << 16) * rec);
        for (int64_t base = 0; base < n && !rc; base += 1 << 16) {
            const size_t m = (size_t)std::min<int64_t>(1 << 16, n - base);
            if (fread(buf.data(), rec, m, f) != m) rc = fail(DPQ_ERR_IO, std::string("short read on ") + path);
            for (size_t i = 0; i < m && !rc; ++i) {
                if (codes_out) memcpy(codes_out + ((size_t)base + i) * cb, buf.data() + i * rec, cb);
                if (ids_out && with_id) memcpy(ids_out + (size_t)base + i, buf.data() + i * rec + cb, 4);
            }
        }
    }
    fclose(f);
    return rc;
    });
}

int dpq_write_codes_plain(const char* path, const uint8_t* codes, int64_t n_codes, int M) {
    return guarded([&]() -> int {
    if (!path || (!codes && n_codes > 0) || n_codes < 0 || M < 1) return fail(DPQ_ERR_ARG, "bad argument");
    std::string err;
    int rc = dpq::write_codes_plain(path, codes, n_codes, M, &err);
    return rc ? fail(rc, err) : DPQ_OK;
    });
}

int dpq_encode_pq(const float* vectors, int64_t n, int D, const float* codewords, int M, int K, int Ds, int device,
                  uint8_t* codes_out) {
    return guarded([&]() -> int {
    if (!vectors || !codewords || !codes_out || n < 0 || D < 1 || M < 1 || K < 1 || K > 256 || Ds < 1)
        return fail(DPQ_ERR_ARG, "bad argument to dpq_encode_pq");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(DPQ_ERR_NO_DEVICE, "device ordinal out of range");
    if (n == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(device));
    DevBuf<float> d_v, d_c;
    DevBuf<uint8_t> d_o;
    const int64_t tile = 1 << 20;  // vectors per upload
    int rc = d_v.alloc((size_t)std::min(n, tile) * D);
    if (!rc) rc = d_c.alloc((size_t)M * K * Ds);
    if (!rc) rc = d_o.alloc((size_t)std::min(n, tile) * M);
    if (rc) return rc;
    hipError_t e = hipMemcpy(d_c, codewords, (size_t)M * K * Ds * sizeof(float), hipMemcpyHostToDevice);
    for (int64_t base = 0; base < n && e == hipSuccess; base += tile) {
        const int64_t m = std::min(tile, n - base);
        e = hipMemcpy(d_v, vectors + (size_t)base * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = dpq::launch_encode_pq(d_v, m, D, d_c, M, K, Ds, d_o, nullptr);
        if (e == hipSuccess) e = hipMemcpy(codes_out + (size_t)base * M, d_o, (size_t)m * M, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(DPQ_ERR_HIP, std::string("dpq_encode_pq: ") + hipGetErrorString(e));
    return DPQ_OK;
    });
}

// The argument checks dpq_train_codebook, dpq_kmeanspp_seed and dpq_train_potential share; 0 or a failed status.
static int train_check_shape(const char* who, int64_t n, int D, int M, int K) {
    const std::string w = std::string(who) + ": ";
    if (D < 1 || M < 1 || M > 256) return fail(DPQ_ERR_ARG, w + "D < 1 or M outside 1..256");
    if (K < 2 || K > 256) return fail(DPQ_ERR_ARG, w + "K outside 2..256 (one byte per label)");
    if (n < K) return fail(DPQ_ERR_ARG, w + "fewer vectors than codewords (K > n)");
    if (n * M >= ((int64_t)1 << 31)) return fail(DPQ_ERR_ARG, w + "n * M >= 2^31");
    const size_t lds = dpq::train_lds_bytes(K, (D + M - 1) / M);
    if (lds == 0 || lds > 160 * 1024)
        return fail(DPQ_ERR_ARG, w + "a sub-space's codewords need more than 160 KB of LDS");
    return DPQ_OK;
}

static int train_select_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(DPQ_ERR_NO_DEVICE, "device ordinal out of range");
    DPQ_HIP(hipSetDevice(device));
    return DPQ_OK;
}

// the random-rows start (header comment): K rows without replacement, the same rows for every sub-space
static void train_rows_start(const float* vectors, int64_t n, int D, int M, int K, int Ds, uint64_t seed, float* codewords) {
    std::vector<int64_t> p((size_t)n);
    std::iota(p.begin(), p.end(), (int64_t)0);
    uint64_t s = seed;
    for (int i = 0; i < K; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        std::swap(p[(size_t)i], p[(size_t)i + (size_t)(z % (uint64_t)(n - i))]);
        for (int m = 0; m < M; ++m)
            for (int d = 0; d < Ds; ++d) {
                const int col = m * Ds + d;
                codewords[((size_t)m * K + i) * Ds + d] = col < D ? vectors[(size_t)p[(size_t)i] * D + col] : 0.0f;
            }
    }
}

int dpq_train_codebook(const float* vectors, int64_t n, int D, int M, int K, const dpq_train_opts* opts, float* codewords,
                       dpq_train_stats* stats) {
    return guarded([&]() -> int {
    const int device = opts ? opts->device : 0, max_iters = opts ? opts->max_iters : 25;
    const int init = opts ? opts->init : 0, restarts = opts ? opts->restarts : 0;
    const bool use_initial = opts && opts->use_initial;
    const uint64_t seed = opts ? opts->seed : 0;
    if (!vectors || !codewords) return fail(DPQ_ERR_ARG, "dpq_train_codebook: NULL argument");
    if (max_iters < 1 || max_iters > 64) return fail(DPQ_ERR_ARG, "dpq_train_codebook: max_iters outside 1..64");
    if (init < 0 || init > 1) return fail(DPQ_ERR_ARG, "dpq_train_codebook: init outside 0..1");
    if (restarts < 0 || restarts > 16) return fail(DPQ_ERR_ARG, "dpq_train_codebook: restarts outside 0..16");
    if (init == 1 && use_initial)
        return fail(DPQ_ERR_ARG, "dpq_train_codebook: init = 1 (k-means++) together with use_initial");
    int rc = train_check_shape("dpq_train_codebook", n, D, M, K);
    if (rc) return rc;
    const int Ds = (D + M - 1) / M;
    if ((rc = train_select_device(device))) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    const int runs = std::max(1, restarts);
    const size_t sub_floats = (size_t)K * Ds;  // one sub-space's codewords
    std::string err;
    dpq::Trainer trainer;
    if ((rc = trainer.open(vectors, n, D, M, K, Ds, &err))) return fail(rc, "dpq_train_codebook: " + err);
    std::vector<float> start, run_cb;   // restarts: the caller's start is kept, `codewords` collects the winners
    std::vector<double> pot((size_t)M), best((size_t)M);
    if (runs > 1) {
        run_cb.resize((size_t)M * sub_floats);
        if (use_initial) start.assign(codewords, codewords + (size_t)M * sub_floats);
    }
    dpq::TrainStats sum;
    sum.converged = 1;
    for (int r = 0; r < runs; ++r) {
        float* cb = runs > 1 ? run_cb.data() : codewords;
        if (init == 1) {
            rc = trainer.seed_kmeanspp(seed + (uint64_t)r, nullptr, nullptr, &err);
        } else {
            if (!use_initial) train_rows_start(vectors, n, D, M, K, Ds, seed + (uint64_t)r, cb);
            rc = trainer.set_codebook(use_initial && runs > 1 ? start.data() : cb, &err);
        }
        dpq::TrainStats st;
        if (!rc) rc = trainer.lloyd(max_iters, &st, &err);
        if (!rc) rc = trainer.get_codebook(cb, &err);
        if (!rc && runs > 1) rc = trainer.potential(pot.data(), &err);
        if (rc) return fail(rc, "dpq_train_codebook: " + err);
        if (runs > 1)
            for (int m = 0; m < M; ++m)
                if (r == 0 || pot[(size_t)m] < best[(size_t)m]) {  // strict: a tie stays with the lower r
                    best[(size_t)m] = pot[(size_t)m];
                    memcpy(codewords + (size_t)m * sub_floats, cb + (size_t)m * sub_floats, sub_floats * sizeof(float));
                }
        if (r == 0) memcpy(sum.distortion, st.distortion, sizeof st.distortion);
        sum.iters_run = std::max(sum.iters_run, st.iters_run);
        sum.converged = sum.converged && st.converged;
        sum.reseeded += st.reseeded;
        sum.gpu_ms += st.gpu_ms;
        sum.rounds_ms += st.rounds_ms;
        sum.assign_ms += st.assign_ms;
        sum.update_ms += st.update_ms;
        sum.repair_ms += st.repair_ms;
    }
    sum.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->iters_run = sum.iters_run;
        stats->converged = sum.converged;
        stats->reseeded = sum.reseeded;
        memcpy(stats->distortion, sum.distortion, sizeof sum.distortion);
        stats->gpu_ms = sum.gpu_ms;
        stats->wall_ms = sum.wall_ms;
        stats->rounds_ms = sum.rounds_ms;
        stats->assign_ms = sum.assign_ms;
        stats->update_ms = sum.update_ms;
        stats->repair_ms = sum.repair_ms;
    }
    return DPQ_OK;
    });
}

int dpq_kmeanspp_seed(const float* vectors, int64_t n, int D, int M, int K, uint64_t seed, int device, float* codewords_out,
                      double* potential_out) {
    return guarded([&]() -> int {
    if (!vectors || !codewords_out) return fail(DPQ_ERR_ARG, "dpq_kmeanspp_seed: NULL argument");
    int rc = train_check_shape("dpq_kmeanspp_seed", n, D, M, K);
    if (rc) return rc;
    if ((rc = train_select_device(device))) return rc;
    std::string err;
    dpq::Trainer trainer;
    rc = trainer.open(vectors, n, D, M, K, (D + M - 1) / M, &err);
    if (!rc) rc = trainer.seed_kmeanspp(seed, potential_out, nullptr, &err);
    if (!rc) rc = trainer.get_codebook(codewords_out, &err);
    return rc ? fail(rc, "dpq_kmeanspp_seed: " + err) : DPQ_OK;
    });
}

int dpq_train_potential(const float* vectors, int64_t n, int D, const float* codewords, int M, int K, int Ds, int device,
                        double* potential_out) {
    return guarded([&]() -> int {
    if (!vectors || !codewords || !potential_out) return fail(DPQ_ERR_ARG, "dpq_train_potential: NULL argument");
    int rc = train_check_shape("dpq_train_potential", n, D, M, K);
    if (rc) return rc;
    if (Ds != (D + M - 1) / M) return fail(DPQ_ERR_ARG, "dpq_train_potential: Ds is not ceil(D / M)");
    if ((rc = train_select_device(device))) return rc;
    std::string err;
    dpq::Trainer trainer;
    rc = trainer.open(vectors, n, D, M, K, Ds, &err);
    if (!rc) rc = trainer.set_codebook(codewords, &err);
    if (!rc) rc = trainer.potential(potential_out, &err);
    return rc ? fail(rc, "dpq_train_potential: " + err) : DPQ_OK;
    });
}

int dpq_write_codewords(const char* path, const float* codewords, int M, int K, int Ds) {
    return guarded([&]() -> int {
    if (!path || !codewords || M < 1 || K < 1 || Ds < 1) return fail(DPQ_ERR_ARG, "bad argument to dpq_write_codewords");
    FILE* f = fopen(path, "w");
    if (!f) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    fprintf(f, "%d,%d,%d\n", M, K, Ds);  // pq.cpp:273
    for (int m = 0; m < M; ++m) {
        fprintf(f, "%d:\n", m);
        for (int k = 0; k < K; ++k) {
            for (int d = 0; d < Ds; ++d) fprintf(f, "%.9g,", (double)codewords[((size_t)m * K + k) * Ds + d]);
            fprintf(f, "\n");
        }
    }
    if (fclose(f) != 0) return fail(DPQ_ERR_IO, std::string("short write on ") + path);
    return DPQ_OK;
    });
}

// ---- exact search over raw vectors (dpq_flat.hip, dpq_flat_u8.hip) ----------------------------------------------

}  // extern "C"

namespace {

// Candidates of dpq_flat_rerank*, all device pointers; ends with one flag word read back.
template <class Q>
int flat_rerank_on_device(const char* fn, dpq_flat* f, const Q* d_queries, int nq, const int32_t* d_cand, int n_cand,
                          int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    const size_t n_pad = dpq::flat_rerank_keys(n_cand);
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)nq, ((size_t)64 << 20) / (n_pad * sizeof(uint64_t))));
    int rc = grow(f->keys, &f->keys_n, (size_t)per * n_pad);
    if (rc) return rc;
    if (!f->flag.get() && (rc = f->flag.alloc(1))) return rc;
    DPQ_HIP(hipMemsetAsync(f->flag, 0, sizeof(uint32_t), stream));
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const uint32_t* map = f->h_map.empty() ? nullptr : f->map.get();
        if constexpr (std::is_same<Q, uint8_t>::value)
            DPQ_HIP(dpq::launch_flat_rerank_u8(f->base8, f->n, f->D, f->Dp, d_queries + (size_t)q0 * f->D, m,
                                               d_cand + (size_t)q0 * n_cand, n_cand, top_k, f->id_offset, map,
                                               (int64_t)f->h_map.size(), f->keys, f->flag, d_ids + (size_t)q0 * top_k,
                                               d_dists + (size_t)q0 * top_k, stream));
        else
            DPQ_HIP(dpq::launch_flat_rerank(f->base, f->n, f->D, f->Dp, d_queries + (size_t)q0 * f->D, m,
                                            d_cand + (size_t)q0 * n_cand, n_cand, top_k, f->id_offset, map,
                                            (int64_t)f->h_map.size(), f->keys, f->flag, d_ids + (size_t)q0 * top_k,
                                            d_dists + (size_t)q0 * top_k, stream));
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(&bad, f->flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, std::string(fn) + ": a candidate names no row of this handle");
    return DPQ_OK;
}

// A handle takes the calls of its own kind only: the fp32 functions an fp32 handle, the _u8 functions a byte handle.
int flat_kind(const dpq_flat* f, bool u8, const char* fn, const char* other) {
    if (f->u8 == u8) return DPQ_OK;
    return fail(DPQ_ERR_ARG, std::string(fn) + (u8 ? ": the handle holds fp32 vectors (dpq_flat_open); call "
                                                   : ": the handle holds byte vectors (dpq_flat_open_u8); call ") + other);
}

int flat_rerank_args(const char* fn, const char* other, const dpq_flat* f, bool u8, const void* queries, int nq,
                     const void* cand, int n_cand, int top_k, const void* ids, const void* dists) {
    if (!f || !queries || !cand || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, std::string(fn) + ": NULL argument or nq < 0");
    if (int rc = flat_kind(f, u8, fn, other)) return rc;
    if (top_k < 1 || top_k > n_cand || n_cand > dpq::kFlatMaxTopK)
        return fail(DPQ_ERR_ARG, std::string(fn) + ": needs 1 <= top_k <= n_cand <= 16384");
    return DPQ_OK;
}

// The checks of dpq_flat_open / dpq_flat_open_u8: the arguments before any device call, then the device.
int flat_open_args(const char* fn, const void* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    const std::string who(fn);
    if (out) *out = nullptr;
    if (!vectors || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 1) return fail(DPQ_ERR_ARG, who + ": n < 1");
    if (D < 1 || D > dpq::kFlatMaxD) return fail(DPQ_ERR_ARG, who + ": D outside 1..2048");
    if (id_offset < 0 || n + id_offset >= ((int64_t)1 << 31))
        return fail(DPQ_ERR_ARG, who + ": id_offset < 0 or n + id_offset >= 2^31 (ids are int32)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(DPQ_ERR_NO_DEVICE, "device ordinal out of range");
    DPQ_HIP(hipSetDevice(device));
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

// Uploads m queries as the distance kernels read them: fp32 rows padded to Dp, or bytes biased and padded with norms.
template <class Q>
int flat_stage_queries(dpq_flat* f, const Q* src, int m, std::vector<float>* padded) {
    const int D = f->D, Dp = f->Dp;
    if constexpr (std::is_same<Q, uint8_t>::value) {
        DPQ_HIP(hipMemcpy(f->q_raw, src, (size_t)m * D, hipMemcpyHostToDevice));
        DPQ_HIP(dpq::launch_flat_u8_prepare(f->q_raw, m, D, Dp, f->q8, f->qnorm, nullptr));
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

template <class Q>
int flat_grow_queries(dpq_flat* f, size_t qb) {
    if constexpr (std::is_same<Q, uint8_t>::value) {
        int rc = grow(f->q_raw, &f->q_raw_n, qb * f->D);
        if (!rc) rc = grow(f->q8, &f->q8_n, qb * f->Dp);
        if (!rc) rc = grow(f->qnorm, &f->qnorm_n, qb);
        return rc;
    } else {
        return grow(f->d_q, &f->q_n, qb * f->Dp);
    }
}

// The handle's rows, all of them or those a filter lists, and queries [a, a + m) of the staged batch, as the launchers
// of dpq_flat.h take them.
dpq::FlatBase flat_base(const dpq_flat* f, const dpq_flat_filter* ff) {
    return {f->base, f->base8, f->norm8, f->Dp, f->id_offset, ff != nullptr, ff ? ff->list.get() : nullptr,
            ff ? ff->n_allowed : f->n};
}

dpq::FlatQueries flat_queries(const dpq_flat* f, int a, int m) {
    if (f->u8) return {nullptr, f->q8.get() + (size_t)a * f->Dp, f->qnorm.get() + a, m};
    return {f->d_q.get() + (size_t)a * f->Dp, nullptr, nullptr, m};
}

// What dpq_flat_search[_u8] and dpq_flat_search_filtered[_u8] share once their arguments are checked: the buffers, the
// batches of staged queries, the copies down and the check of every query's state.  ff NULL: all rows, top_k <= n.
template <class Q>
int flat_search_run(const std::string& who, dpq_flat* f, const dpq_flat_filter* ff, const Q* queries, int nq, int top_k,
                    int32_t* ids, float* dists) {
    if (nq == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(f->device));
    const int qb = std::min(nq, dpq::flat_query_batch(top_k));
    int rc = grow(f->keys, &f->keys_n, (size_t)qb * dpq::flat_key_capacity(top_k));
    if (!rc) rc = grow(f->state, &f->state_n, (size_t)qb);
    if (!rc) rc = flat_grow_queries<Q>(f, (size_t)qb);
    if (!rc) rc = grow_outputs(f, (size_t)qb * top_k);
    if (rc) return rc;
    const dpq::FlatBase base = flat_base(f, ff);
    const uint32_t expect = (uint32_t)std::min<int64_t>(top_k, base.n_entries);
    std::vector<float> padded;
    std::vector<dpq::FlatQueryState> st((size_t)qb);
    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        if ((rc = flat_stage_queries(f, queries + (size_t)q0 * f->D, m, &padded))) return rc;
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

}  // namespace

extern "C" {

int dpq_flat_open(const float* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    if (int rc = flat_open_args("dpq_flat_open", vectors, n, D, device, id_offset, out)) return rc;
    std::unique_ptr<dpq_flat> f(new dpq_flat);
    f->device = device;
    f->n = n;
    f->id_offset = id_offset;
    f->D = D;
    f->Dp = dpq::flat_padded_d(D);
    int rc = f->base.alloc((size_t)n * f->Dp);
    if (rc) return fail(rc, "dpq_flat_open: the vectors do not fit into device memory (" + g_last_error + ")");
    if (f->Dp == D) {
        DPQ_HIP(hipMemcpy(f->base, vectors, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice));
    } else {
        const int64_t tile = 1 << 18;  // rows per upload; padded on the device
        DevBuf<float> tmp;
        if ((rc = tmp.alloc((size_t)std::min(n, tile) * D))) return rc;
        for (int64_t r0 = 0; r0 < n; r0 += tile) {
            const int64_t m = std::min(tile, n - r0);
            DPQ_HIP(hipMemcpy(tmp, vectors + (size_t)r0 * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice));
            DPQ_HIP(dpq::launch_flat_pad_rows(tmp, m, D, f->Dp, f->base.get() + (size_t)r0 * f->Dp, nullptr));
            DPQ_HIP(hipDeviceSynchronize());
        }
    }
    *out = f.release();
    return DPQ_OK;
    });
}

int dpq_flat_open_u8(const uint8_t* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out) {
    return guarded([&]() -> int {
    if (int rc = flat_open_args("dpq_flat_open_u8", vectors, n, D, device, id_offset, out)) return rc;
    std::unique_ptr<dpq_flat> f(new dpq_flat);
    f->device = device;
    f->n = n;
    f->id_offset = id_offset;
    f->D = D;
    f->Dp = dpq::flat_u8_padded_d(D);
    f->u8 = true;
    int rc = f->base8.alloc((size_t)n * f->Dp);
    if (!rc) rc = f->norm8.alloc((size_t)((n + 3) & ~(int64_t)3));
    if (rc) return fail(rc, "dpq_flat_open_u8: the vectors do not fit into device memory (" + g_last_error + ")");
    // the norm array's padding is read by the last stripe's 16-byte loads (and masked afterwards): keep it defined
    DPQ_HIP(hipMemset(f->norm8.get() + ((n - 1) & ~(int64_t)3), 0, 4 * sizeof(int32_t)));
    const int64_t tile = std::max<int64_t>(1, ((int64_t)128 << 20) / D);  // rows per upload (128 MB); biased on the device
    DevBuf<uint8_t> tmp;
    if ((rc = tmp.alloc((size_t)std::min(n, tile) * D))) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += tile) {
        const int64_t m = std::min(tile, n - r0);
        DPQ_HIP(hipMemcpy(tmp, vectors + (size_t)r0 * D, (size_t)m * D, hipMemcpyHostToDevice));
        DPQ_HIP(dpq::launch_flat_u8_prepare(tmp, m, D, f->Dp, f->base8.get() + (size_t)r0 * f->Dp, f->norm8.get() + r0,
                                            nullptr));
        DPQ_HIP(hipDeviceSynchronize());
    }
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
    if (!f || !queries || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, "dpq_flat_search: NULL argument or nq < 0");
    if (top_k < 1 || top_k > DPQ_FLAT_MAX_TOPK) return fail(DPQ_ERR_ARG, "dpq_flat_search: top_k outside 1..DPQ_FLAT_MAX_TOPK");
    if (int rc = flat_kind(f, false, "dpq_flat_search", "dpq_flat_search_u8")) return rc;
    if (top_k > f->n) return fail(DPQ_ERR_TOPK, "dpq_flat_search: top_k exceeds the number of vectors");
    return flat_search_run("dpq_flat_search", f, nullptr, queries, nq, top_k, ids, dists);
    });
}

int dpq_flat_search_u8(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    if (!f || !queries || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, "dpq_flat_search_u8: NULL argument or nq < 0");
    if (top_k < 1 || top_k > DPQ_FLAT_MAX_TOPK)
        return fail(DPQ_ERR_ARG, "dpq_flat_search_u8: top_k outside 1..DPQ_FLAT_MAX_TOPK");
    if (int rc = flat_kind(f, true, "dpq_flat_search_u8", "dpq_flat_search")) return rc;
    if (top_k > f->n) return fail(DPQ_ERR_TOPK, "dpq_flat_search_u8: top_k exceeds the number of vectors");
    return flat_search_run("dpq_flat_search_u8", f, nullptr, queries, nq, top_k, ids, dists);
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

// After the arguments that need no handle, before the handle is read.
int flat_device_present(const std::string& who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DPQ_ERR_NO_DEVICE, who + ": no HIP device visible; this library has no CPU fallback");
    return DPQ_OK;
}

int flat_filter_owner(const dpq_flat* f, const dpq_flat_filter* ff, const std::string& who) {
    if (ff->owner == f->serial) return DPQ_OK;
    return fail(DPQ_ERR_ARG, who + ": the filter was made for another handle");
}

// dpq_flat_search_filtered / _u8: Q is float or uint8_t, the handle of the same kind.
template <class Q>
int flat_search_filtered_call(const char* fn, const char* other, dpq_flat* f, const dpq_flat_filter* ff, const Q* queries,
                              int nq, int top_k, int32_t* ids, float* dists) {
    constexpr bool u8 = std::is_same<Q, uint8_t>::value;
    const std::string who(fn);
    if (!f || !ff || !queries || !ids || !dists || nq < 0)
        return fail(DPQ_ERR_ARG, who + ": NULL argument (the filter included) or nq < 0");
    if (top_k < 1 || top_k > DPQ_FLAT_MAX_TOPK) return fail(DPQ_ERR_ARG, who + ": top_k outside 1..DPQ_FLAT_MAX_TOPK");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = flat_kind(f, u8, fn, other)) return rc;
    if (int rc = flat_filter_owner(f, ff, who)) return rc;
    return flat_search_run(who, f, ff, queries, nq, top_k, ids, dists);
}

// One distance pass of a range search over queries [a, a + m) of the staged batch: counting (pool NULL) or emitting.
int flat_range_pass(dpq_flat* f, const dpq_flat_filter* ff, int a, int m, uint64_t* pool) {
    dpq::FlatQueryState* state = f->state.get() + a;
    DPQ_HIP(dpq::launch_flat_range_state(state, f->r_thr.get() + a, m, nullptr));
    DPQ_HIP(dpq::launch_flat_range_pass(flat_base(f, ff), flat_queries(f, a, m), pool, f->r_offs, state, nullptr));
    return DPQ_OK;
}

// dpq_flat_range_search / _u8.  Count, then emit: a pass over a batch of queries counts every list, the host lays the
// lists out, and sub-batches of at most kFlatRangePoolKeys keys (or one longer list) are formed again into the pool,
// sorted there and brought down.
template <class Q>
int flat_range_call(const char* fn, const char* other, dpq_flat* f, const dpq_flat_filter* ff, const Q* queries, int nq,
                    const float* radii, dpq_range_result** out) {
    constexpr bool u8 = std::is_same<Q, uint8_t>::value;
    const std::string who(fn);
    if (!out) return fail(DPQ_ERR_ARG, who + ": out is NULL");
    *out = nullptr;
    if (!f || nq < 0 || (nq > 0 && (!queries || !radii))) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    for (int q = 0; q < nq; ++q)
        if (std::isnan(radii[q])) return fail(DPQ_ERR_ARG, who + ": radius of query " + std::to_string(q) + " is NaN");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = flat_kind(f, u8, fn, other)) return rc;
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
    if (!rc) rc = flat_grow_queries<Q>(f, (size_t)qb);
    if (!rc) rc = grow(f->r_thr, &f->r_thr_n, (size_t)qb);
    if (!rc) rc = grow(f->r_offs, &f->r_offs_n, (size_t)qb + 1);
    if (rc) return rc;
    std::vector<float> padded;
    std::vector<dpq::FlatQueryState> st((size_t)qb);
    std::vector<uint64_t> thr((size_t)qb), sorted;
    std::vector<int64_t> offs;
    for (int q0 = 0; q0 < nq && !rc; q0 += qb) {
        const int m = std::min(qb, nq - q0);
        if ((rc = flat_stage_queries(f, queries + (size_t)q0 * f->D, m, &padded))) break;
        for (int q = 0; q < m; ++q) {  // d < r on non-negative floats is bits(d) < bits(r); key 0 lets nothing pass
            const float r = radii[q0 + q];
            uint32_t bits = 0;
            if (r > 0.0f) memcpy(&bits, &r, sizeof bits);
            thr[(size_t)q] = (uint64_t)bits << 32;
        }
        DPQ_HIP(hipMemcpy(f->r_thr, thr.data(), (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice));
        if ((rc = flat_range_pass(f, ff, 0, m, nullptr))) break;
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
                if ((rc = flat_range_pass(f, ff, a, b - a, f->r_pool))) break;
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
                    const uint32_t bits = (uint32_t)(sorted[i] >> 32);
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
    return flat_search_filtered_call("dpq_flat_search_filtered", "dpq_flat_search_filtered_u8", f, ff, queries, nq, top_k, ids,
                                     dists);
    });
}

int dpq_flat_search_filtered_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k,
                                int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_search_filtered_call("dpq_flat_search_filtered_u8", "dpq_flat_search_filtered", f, ff, queries, nq, top_k, ids,
                                     dists);
    });
}

int dpq_flat_range_search(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, const float* radii,
                          dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call("dpq_flat_range_search", "dpq_flat_range_search_u8", f, ff, queries, nq, radii, out);
    });
}

int dpq_flat_range_search_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, const float* radii,
                             dpq_range_result** out) {
    return guarded([&]() -> int {
    return flat_range_call("dpq_flat_range_search_u8", "dpq_flat_range_search", f, ff, queries, nq, radii, out);
    });
}

int dpq_range_recall(int nq, const int64_t* found_lims, const int32_t* found_ids, const int64_t* truth_lims,
                     const int32_t* truth_ids, double* recall, double* precision) {
    return guarded([&]() -> int {
    if (nq < 0 || !found_lims || !truth_lims || (found_lims[nq] > found_lims[0] && !found_ids) ||
        (truth_lims[nq] > truth_lims[0] && !truth_ids))
        return fail(DPQ_ERR_ARG, "bad argument to dpq_range_recall");
    int64_t hits = 0, n_found = 0, n_truth = 0;
    std::vector<int32_t> a, b, both;
    auto ids_of = [](const int64_t* lims, const int32_t* ids, int q, std::vector<int32_t>* v) {
        v->clear();
        for (int64_t i = lims[q]; i < lims[q + 1]; ++i)
            if (ids[i] >= 0) v->push_back(ids[i]);  // negative ids are ignored
        std::sort(v->begin(), v->end());
        v->erase(std::unique(v->begin(), v->end()), v->end());  // an id counts once per query
    };
    for (int q = 0; q < nq; ++q) {
        if (found_lims[q + 1] < found_lims[q] || truth_lims[q + 1] < truth_lims[q])
            return fail(DPQ_ERR_ARG, "dpq_range_recall: lims must not descend");
        ids_of(found_lims, found_ids, q, &a);
        ids_of(truth_lims, truth_ids, q, &b);
        both.clear();
        std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(both));
        hits += (int64_t)both.size();
        n_found += (int64_t)a.size();
        n_truth += (int64_t)b.size();
    }
    if (recall) *recall = n_truth ? (double)hits / (double)n_truth : 1.0;
    if (precision) *precision = n_found ? (double)hits / (double)n_found : 1.0;
    return DPQ_OK;
    });
}

int dpq_bitmap_to_dfs(const uint32_t* words, int64_t n_bits, const uint32_t* vec_id, int64_t n_codes, uint32_t* words_out) {
    return guarded([&]() -> int {
    if (n_bits < 0 || (n_bits > 0 && !words) || !vec_id || n_codes < 1 || !words_out)
        return fail(DPQ_ERR_ARG, "bad argument to dpq_bitmap_to_dfs");
    std::fill(words_out, words_out + (n_codes + 1 + 31) / 32, 0u);
    for (int64_t p = 0; p < n_codes; ++p) {
        const int64_t v = vec_id[p];
        if (v >= n_bits || !((words[v >> 5] >> (v & 31)) & 1u)) continue;
        const int64_t r = ((n_codes & 1) == 0 && p == n_codes - 1) ? n_codes : p;  // the even-N id of the last DFS node
        words_out[r >> 5] |= 1u << (r & 31);
    }
    return DPQ_OK;
    });
}

int dpq_write_bitmap(const char* path, const uint32_t* words, int64_t n_bits) {
    return guarded([&]() -> int {
    if (!path || n_bits < 0 || (n_bits > 0 && !words)) return fail(DPQ_ERR_ARG, "bad argument to dpq_write_bitmap");
    FILE* fp = fopen(path, "wb");
    if (!fp) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    const size_t n_words = (size_t)((n_bits + 31) / 32);
    const bool ok = fwrite(&n_bits, sizeof n_bits, 1, fp) == 1 && (n_words == 0 || fwrite(words, sizeof(uint32_t), n_words, fp) == n_words);
    if (fclose(fp) != 0 || !ok) return fail(DPQ_ERR_IO, std::string("short write on ") + path);
    return DPQ_OK;
    });
}

int dpq_read_bitmap(const char* path, int64_t* n_bits, uint32_t* words) {
    return guarded([&]() -> int {
    if (!path || !n_bits) return fail(DPQ_ERR_ARG, "bad argument to dpq_read_bitmap");
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    std::unique_ptr<FILE, int (*)(FILE*)> closer(fp, fclose);
    int64_t nb = 0;
    if (fread(&nb, sizeof nb, 1, fp) != 1 || nb < 0) return fail(DPQ_ERR_IO, std::string("no bitmap header in ") + path);
    const int64_t n_words = (nb + 31) / 32;
    if (fseeko(fp, 0, SEEK_END) != 0) return fail(DPQ_ERR_IO, std::string("cannot seek in ") + path);
    if ((int64_t)ftello(fp) < 8 + 4 * n_words)
        return fail(DPQ_ERR_IO, std::string(path) + " is shorter than its " + std::to_string(nb) + " bits");
    *n_bits = nb;
    if (!words || n_words == 0) return DPQ_OK;
    if (fseeko(fp, 8, SEEK_SET) != 0 || fread(words, sizeof(uint32_t), (size_t)n_words, fp) != (size_t)n_words)
        return fail(DPQ_ERR_IO, std::string("short read on ") + path);
    return DPQ_OK;
    });
}

}  // extern "C"

namespace {

// dpq_flat_rerank_device / _u8_device: Q is float or uint8_t, the handle of the same kind.
template <class Q>
int flat_rerank_device_call(const char* fn, const char* other, dpq_flat* f, const Q* d_queries, int nq,
                            const int32_t* d_cand_ids, int n_cand, int top_k, int32_t* d_ids, float* d_dists,
                            void* hip_stream) {
    int rc = flat_rerank_args(fn, other, f, std::is_same<Q, uint8_t>::value, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids,
                              d_dists);
    if (rc || nq == 0) return rc;
    DPQ_HIP(hipSetDevice(f->device));
    return flat_rerank_on_device(fn, f, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids, d_dists, (hipStream_t)hip_stream);
}

// dpq_flat_rerank / _u8: the candidates are checked on the host, then queries and candidates go up and the answer down.
template <class Q>
int flat_rerank_host_call(const char* fn, const char* other, dpq_flat* f, const Q* queries, int nq,
                          const int32_t* cand_ids, int n_cand, int top_k, int32_t* ids, float* dists) {
    constexpr bool u8 = std::is_same<Q, uint8_t>::value;
    int rc = flat_rerank_args(fn, other, f, u8, queries, nq, cand_ids, n_cand, top_k, ids, dists);
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
    if constexpr (u8) {
        rc = grow(f->q_raw, &f->q_raw_n, (size_t)nq * f->D);
        d_q = f->q_raw;
    } else {
        rc = grow(f->d_q, &f->q_n, (size_t)nq * f->D);
        d_q = f->d_q;
    }
    if (!rc) rc = grow(f->d_cand, &f->cand_n, (size_t)nq * n_cand);
    if (!rc) rc = grow_outputs(f, (size_t)nq * top_k);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(d_q, queries, (size_t)nq * f->D * sizeof(Q), hipMemcpyHostToDevice));
    DPQ_HIP(hipMemcpy(f->d_cand, cand_ids, (size_t)nq * n_cand * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = flat_rerank_on_device(fn, f, d_q, nq, f->d_cand, n_cand, top_k, f->d_ids, f->d_dists, nullptr);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(ids, f->d_ids, (size_t)nq * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, f->d_dists, (size_t)nq * top_k * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_flat_rerank_device(dpq_flat* f, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand, int top_k,
                           int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call("dpq_flat_rerank", "dpq_flat_rerank_u8_device", f, d_queries, nq, d_cand_ids, n_cand,
                                   top_k, d_ids, d_dists, hip_stream);
    });
}

int dpq_flat_rerank(dpq_flat* f, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k, int32_t* ids,
                    float* dists) {
    return guarded([&]() -> int {
    return flat_rerank_host_call("dpq_flat_rerank", "dpq_flat_rerank_u8", f, queries, nq, cand_ids, n_cand, top_k, ids, dists);
    });
}

int dpq_flat_rerank_u8_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                              int top_k, int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    return flat_rerank_device_call("dpq_flat_rerank_u8_device", "dpq_flat_rerank_device", f, d_queries, nq, d_cand_ids,
                                   n_cand, top_k, d_ids, d_dists, hip_stream);
    });
}

int dpq_flat_rerank_u8(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                       int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    return flat_rerank_host_call("dpq_flat_rerank_u8", "dpq_flat_rerank", f, queries, nq, cand_ids, n_cand, top_k, ids, dists);
    });
}

}  // extern "C"

namespace {

// Records [first, first + count) of an .fvecs / .bvecs file into out[count][D]: T = float widens bytes, T = uint8_t
// (bvecs only) keeps them.
template <class T>
int read_vecs_range(const char* fn, const char* path, bool is_bvecs, int64_t first, int64_t count, int32_t* D, T* out) {
    if (!path || !D || first < 0 || count < 0) return fail(DPQ_ERR_ARG, std::string("bad argument to ") + fn);
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    std::unique_ptr<FILE, int (*)(FILE*)> closer(fp, fclose);
    int32_t d = 0;
    if (fread(&d, sizeof d, 1, fp) != 1 || d < 1 || d > (1 << 20)) return fail(DPQ_ERR_IO, std::string("no vector header in ") + path);
    const int64_t rec = 4 + (int64_t)d * (is_bvecs ? 1 : 4);
    if (fseeko(fp, 0, SEEK_END) != 0) return fail(DPQ_ERR_IO, std::string("cannot seek in ") + path);
    const int64_t n_file = (int64_t)ftello(fp) / rec;
    if (first + count > n_file)
        return fail(DPQ_ERR_IO, std::string(path) + " holds " + std::to_string(n_file) + " vectors, asked for [" +
                                    std::to_string(first) + ", " + std::to_string(first + count) + ")");
    *D = d;
    if (!out || count == 0) return DPQ_OK;
    if (fseeko(fp, (off_t)(first * rec), SEEK_SET) != 0) return fail(DPQ_ERR_IO, std::string("cannot seek in ") + path);
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)8 << 20) / rec);  // records per read
    std::vector<uint8_t> raw((size_t)(std::min(chunk, count) * rec));
    for (int64_t r0 = 0; r0 < count; r0 += chunk) {
        const int64_t m = std::min(chunk, count - r0);
        if (fread(raw.data(), (size_t)rec, (size_t)m, fp) != (size_t)m) return fail(DPQ_ERR_IO, std::string("short read on ") + path);
        for (int64_t r = 0; r < m; ++r) {
            const uint8_t* p = raw.data() + (size_t)(r * rec);
            int32_t dd;
            memcpy(&dd, p, 4);
            if (dd != d) return fail(DPQ_ERR_IO, std::string("a record of another dimension in ") + path);
            T* o = out + (size_t)(r0 + r) * d;
            if (is_bvecs)
                for (int j = 0; j < d; ++j) o[j] = (T)p[4 + j];
            else
                memcpy(o, p + 4, (size_t)d * 4);
        }
    }
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_read_vecs_range(const char* path, int is_bvecs, int64_t first, int64_t count, int32_t* D, float* out) {
    return guarded([&]() -> int { return read_vecs_range("dpq_read_vecs_range", path, is_bvecs != 0, first, count, D, out); });
}

int dpq_read_bvecs_range(const char* path, int64_t first, int64_t count, int32_t* D, uint8_t* out) {
    return guarded([&]() -> int { return read_vecs_range("dpq_read_bvecs_range", path, true, first, count, D, out); });
}

int dpq_write_groundtruth(const char* path, const int32_t* ids, const float* dists, int nq, int top_k) {
    return guarded([&]() -> int {
    if (!path || !ids || !dists || nq < 0 || top_k < 1) return fail(DPQ_ERR_ARG, "bad argument to dpq_write_groundtruth");
    FILE* fp = fopen(path, "w");
    if (!fp) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    fprintf(fp, "%d,%d\n", nq, top_k);  // pqbase.cpp:300
    for (int q = 0; q < nq; ++q) {
        for (int r = 0; r < top_k; ++r)
            fprintf(fp, "%d,%.9g,", ids[(size_t)q * top_k + r], (double)dists[(size_t)q * top_k + r]);  // pqbase.cpp:308
        fprintf(fp, "\n");
    }
    if (fclose(fp) != 0) return fail(DPQ_ERR_IO, std::string("short write on ") + path);
    return DPQ_OK;
    });
}

int dpq_read_groundtruth(const char* path, int32_t* nq, int32_t* top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    if (!path || !nq || !top_k || (ids == nullptr) != (dists == nullptr)) return fail(DPQ_ERR_ARG, "bad argument to dpq_read_groundtruth");
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    std::unique_ptr<FILE, int (*)(FILE*)> closer(fp, fclose);
    int a = 0, b = 0;
    if (fscanf(fp, "%d ,%d", &a, &b) != 2 || a < 0 || b < 1) return fail(DPQ_ERR_IO, std::string("no `nq,top_k` line in ") + path);
    *nq = a;
    *top_k = b;
    if (!ids) return DPQ_OK;
    std::string text;
    char blk[1 << 16];
    size_t got;
    while ((got = fread(blk, 1, sizeof blk, fp)) > 0) text.append(blk, got);
    const char* p = text.c_str();
    for (size_t i = 0; i < (size_t)a * b; ++i) {  // pqbase.cpp:328: id, distance, each followed by one separator
        char* e = nullptr;
        const long long id = strtoll(p, &e, 10);
        if (e == p || *e != ',') return fail(DPQ_ERR_IO, std::string("malformed entry in ") + path);
        p = e + 1;
        const float d = strtof(p, &e);
        if (e == p || *e != ',') return fail(DPQ_ERR_IO, std::string("malformed entry in ") + path);
        p = e + 1;
        ids[i] = (int32_t)id;
        dists[i] = d;
    }
    return DPQ_OK;
    });
}

int dpq_recall(const int32_t* found, int found_stride, int R, const int32_t* truth, int truth_stride, int k, int nq,
               double* recall) {
    return guarded([&]() -> int {
    if (!found || !truth || !recall || R < 1 || k < 1 || nq < 1 || found_stride < R || truth_stride < k)
        return fail(DPQ_ERR_ARG, "bad argument to dpq_recall");
    int64_t hits = 0;
    std::vector<int32_t> t;
    for (int q = 0; q < nq; ++q) {
        t.assign(truth + (size_t)q * truth_stride, truth + (size_t)q * truth_stride + k);
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        while (!t.empty() && t.front() < 0) t.erase(t.begin());  // padding
        std::vector<char> hit(t.size(), 0);
        for (int r = 0; r < R; ++r) {
            const int32_t id = found[(size_t)q * found_stride + r];
            if (id < 0) continue;
            const size_t at = (size_t)(std::lower_bound(t.begin(), t.end(), id) - t.begin());
            if (at == t.size() || t[at] != id || hit[at]) continue;  // an id found twice counts once
            hit[at] = 1;
            ++hits;
        }
    }
    *recall = (double)hits / ((double)nq * k);
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
    delete x;  // (the device buffers go with it)
    return DPQ_OK;
    });
}

namespace {

int check_batch_args(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists) {
    if (!x || !d_queries || !d_ids || !d_dists || nq < 0) return fail(DPQ_ERR_ARG, "NULL argument or nq < 0");
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, "dpq_set_codebook has not been called");
    if (top_k < 1 || top_k > dpq::kMaxTopK) return fail(DPQ_ERR_ARG, "top_k must be in 1..2048");
    if ((int64_t)top_k > x->img.n_codes_total)
        return fail(DPQ_ERR_TOPK, "top_k exceeds the number of codes in the index");
    return DPQ_OK;
}

}  // namespace

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
        int rc = run_batch(x, p.d_queries, p.nq, p.top_k, p.d_ids, p.d_dists, p.stream);
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
        rc = run_batch(x, d_queries + (size_t)base * D, n, top_k, d_ids + (size_t)base * top_k,
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

namespace {
// dpq_query_batch_device and its filtered twin (filt != NULL): synchronous on `hip_stream`.
int query_device(dpq_index* x, const dpq_filter* filt, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                 float* d_dists, void* hip_stream) {
    if (x && !x->pending.empty()) {  // keep the order of the batches on this index
        int rc = dpq_finish(x);
        if (rc) return rc;
    }
    int rc = check_batch_args(x, d_queries, nq, top_k, d_ids, d_dists);
    if (rc || nq == 0) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    const int D = x->M * x->Ds;
    for (int base = 0; base < nq; base += kMaxBatchQueries) {
        const int n = std::min(kMaxBatchQueries, nq - base);
        rc = run_batch(x, d_queries + (size_t)base * D, n, top_k, d_ids + (size_t)base * top_k,
                       d_dists + (size_t)base * top_k, stream, 0, filt);
        if (rc) return rc;
    }
    if (x->prof) {
        x->prof_acc.query_batches++;
        x->prof_acc.queries += nq;
    }
    return DPQ_OK;
}

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
    if (oe > x->out_stage_elems) {
        x->out_stage_elems = 0;
        x->d_dists_stage.reset();
        int rc = x->d_ids_stage.alloc(oe);
        if (!rc) rc = x->d_dists_stage.alloc(oe);
        if (rc) return rc;
        x->out_stage_elems = oe;
    }
    DPQ_HIP(hipMemcpy(x->d_q_stage, queries, qf * sizeof(float), hipMemcpyHostToDevice));
    int rc = query_device(x, filt, x->d_q_stage, nq, top_k, x->d_ids_stage, x->d_dists_stage, nullptr);
    if (rc) return rc;
    DPQ_HIP(hipDeviceSynchronize());
    DPQ_HIP(hipMemcpy(ids, x->d_ids_stage, oe * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, x->d_dists_stage, oe * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
}

int check_filter(const dpq_index* x, const dpq_filter* f) {
    if (!x) return fail(DPQ_ERR_ARG, "NULL index");
    if (!f) return fail(DPQ_ERR_ARG, "filter is NULL");
    if (f->owner != x->serial) return fail(DPQ_ERR_ARG, "the filter was made for another index handle");
    return DPQ_OK;
}
}  // namespace

int dpq_query_batch_device(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists,
                           void* hip_stream) {
    return guarded([&]() -> int { return query_device(x, nullptr, d_queries, nq, top_k, d_ids, d_dists, hip_stream); });
}

int dpq_query_batch(dpq_index* x, const float* queries, int nq, int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int { return query_host(x, nullptr, queries, nq, top_k, ids, dists); });
}

namespace {
// Words of a filter's bitmap on this handle: every node of every segment (the scan reads whole segments' words).
int64_t filter_words(const dpq_index* x) {
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    const int64_t n_nodes = std::max<int64_t>(x->img.n_local, (int64_t)x->img.n_segments * S);
    return std::max<int64_t>(1, (n_nodes + 31) / 32);
}

void fill_filter_state(const dpq_index* x, dpq_filter* f, int64_t n_words) {
    f->owner = x->serial;
    f->device = x->device;
    f->plain = x->plain;
    f->base = x->img.id_base;
    f->n_local = x->img.n_local;
    f->N = x->img.n_codes_total;
    f->n_words = n_words;
}
}  // namespace

int dpq_filter_create(dpq_index* x, const uint32_t* words, int64_t n_bits, dpq_filter** out) {
    return guarded([&]() -> int {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!x || n_bits < 0 || (n_bits > 0 && !words)) return fail(DPQ_ERR_ARG, "NULL argument or n_bits < 0");
    DPQ_HIP(hipSetDevice(x->device));
    // Local bit l (node id_base + l) = the caller's bit of the id the handle reports for that node: id_base + l, or N
    // for the last node of an even-N DTC index (report_id).  The bitmap covers every node of every segment (the scan
    // reads whole segments' words); nodes past n_local stay 0.
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    const int64_t n_local = x->img.n_local, n_nodes = std::max<int64_t>(n_local, (int64_t)x->img.n_segments * S);
    const int64_t n_words = std::max<int64_t>(1, (n_nodes + 31) / 32), user_words = (n_bits + 31) / 32;
    const int64_t base = x->img.id_base;
    auto user_bit = [&](int64_t r) -> uint32_t { return r < n_bits ? (words[r >> 5] >> (r & 31)) & 1u : 0u; };
    std::vector<uint32_t> h((size_t)n_words, 0u);
    int64_t allowed = 0;
    for (int64_t w = 0; w < n_words && 32 * w < n_local; ++w) {
        const int64_t g0 = base + 32 * w;  // global position of local bit 32 w
        if (g0 >= n_bits) break;
        const int64_t lo = g0 >> 5;
        const int sh = (int)(g0 & 31);
        uint32_t v = words[lo] >> sh;
        if (sh && lo + 1 < user_words) v |= words[lo + 1] << (32 - sh);
        const int64_t valid = std::min<int64_t>(32, std::min(n_bits - g0, n_local - 32 * w));
        if (valid < 32) v &= (1u << valid) - 1u;
        h[(size_t)w] = v;
    }
    const int64_t N = x->img.n_codes_total;
    if (!x->plain && (N & 1) == 0 && N - 1 >= base && N - 1 < base + n_local) {  // the even-N rule
        const int64_t l = N - 1 - base;
        h[(size_t)(l >> 5)] = (h[(size_t)(l >> 5)] & ~(1u << (l & 31))) | (user_bit(N) << (l & 31));
    }
    for (uint32_t v : h) allowed += __builtin_popcount(v);
    std::unique_ptr<dpq_filter> f(new dpq_filter());
    f->owner = x->serial;
    f->n_allowed = allowed;
    int rc = f->bits.alloc((size_t)n_words);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(f->bits, h.data(), (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    fill_filter_state(x, f.get(), n_words);
    *out = f.release();
    return DPQ_OK;
    });
}

void dpq_filter_free(dpq_filter* f) { delete f; }

int dpq_filter_count(const dpq_filter* f, int64_t* n_allowed) {
    if (!f || !n_allowed) return fail(DPQ_ERR_ARG, "NULL argument");
    *n_allowed = f->n_allowed;
    return DPQ_OK;
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

}  // extern "C"

// ---- filter construction on the device (include/deltapq_amd.h; kernels in dpq_filter.hip) ----
namespace {

dpq::FilterGeom filter_geom(bool plain, int64_t base, int64_t n_local, int64_t N, int64_t n_words) {
    dpq::FilterGeom g{};
    g.base = base;
    g.n_local = n_local;
    g.n_words = n_words;
    g.N = N;
    g.even = (!plain && (N & 1) == 0) ? 1 : 0;
    g.tail_l = (g.even && N - 1 >= base && N - 1 < base + n_local) ? N - 1 - base : -1;
    return g;
}

// The frame of every device constructor: allocates the filter, clears the handle's count word on `stream`, lets
// `build(geom, bits, count)` enqueue its kernels there, and reads the count back -- the call's one host round trip.
template <class Build>
int filter_build(dpq_index* x, hipStream_t stream, dpq_filter** out, Build&& build) {
    DPQ_HIP(hipSetDevice(x->device));
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    int rc;
    if (!x->d_filter_count.get() && (rc = x->d_filter_count.alloc(1))) return rc;
    std::unique_ptr<dpq_filter> f(new dpq_filter());
    fill_filter_state(x, f.get(), filter_words(x));
    if ((rc = f->bits.alloc((size_t)f->n_words))) return rc;
    const dpq::FilterGeom g = filter_geom(f->plain, f->base, f->n_local, f->N, f->n_words);
    DPQ_HIP(hipMemsetAsync(x->d_filter_count, 0, sizeof(unsigned long long), stream));
    hipError_t e = build(g, f->bits.get(), x->d_filter_count.get());
    unsigned long long allowed = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&allowed, x->d_filter_count, sizeof allowed, hipMemcpyDeviceToHost, stream);
    const hipError_t es = hipStreamSynchronize(stream);  // (also after a failed launch: nothing may still write the bitmap)
    DPQ_HIP(e);
    DPQ_HIP(es);
    f->n_allowed = (int64_t)allowed;
    *out = f.release();
    return DPQ_OK;
}

// A host array for the length of one call on the device (freed when the caller's DevBuf goes).
template <class T>
int upload_temp(DevBuf<T>* d, const T* h, int64_t n) {
    if (n <= 0) return DPQ_OK;
    if (int rc = d->alloc((size_t)n)) return rc;
    DPQ_HIP(hipMemcpy(d->get(), h, (size_t)n * sizeof(T), hipMemcpyHostToDevice));
    return DPQ_OK;
}

int filter_out_arg(dpq_filter** out) {
    if (!out) return fail(DPQ_ERR_ARG, "out is NULL");
    *out = nullptr;
    return DPQ_OK;
}

int filter_bitmap_args(const dpq_index* x, const void* words, int64_t n_bits, const char* who) {
    if (!x || n_bits < 0 || (n_bits > 0 && !words)) return fail(DPQ_ERR_ARG, std::string(who) + ": NULL argument or n_bits < 0");
    return DPQ_OK;
}

int filter_ids_args(const dpq_index* x, const void* ids, int64_t n, const char* who) {
    if (!x || n < 0 || (n > 0 && !ids)) return fail(DPQ_ERR_ARG, std::string(who) + ": NULL argument or n < 0");
    return DPQ_OK;
}

int filter_ids_on_device(dpq_index* x, const int32_t* d_ids, int64_t n, int invert, hipStream_t stream, dpq_filter** out) {
    return filter_build(x, stream, out, [&](const dpq::FilterGeom& g, uint32_t* bits, unsigned long long* count) {
        return dpq::launch_filter_ids_build(d_ids, n, invert, g, bits, count, stream);
    });
}

int filter_vec_on_device(dpq_index* x, const uint32_t* d_words, int64_t n_bits, hipStream_t stream, dpq_filter** out) {
    return filter_build(x, stream, out, [&](const dpq::FilterGeom& g, uint32_t* bits, unsigned long long* count) {
        return dpq::launch_filter_gather(d_words, n_bits, x->d_vec_id, g, bits, count, stream);
    });
}

}  // namespace

extern "C" {

int dpq_filter_create_device(dpq_index* x, const uint32_t* d_words, int64_t n_bits, void* hip_stream, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (!rc) rc = filter_bitmap_args(x, d_words, n_bits, "dpq_filter_create_device");
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    return filter_build(x, stream, out, [&](const dpq::FilterGeom& g, uint32_t* bits, unsigned long long* count) {
        return dpq::launch_filter_reindex(d_words, n_bits, g, bits, count, stream);
    });
    });
}

int dpq_filter_create_ids_device(dpq_index* x, const int32_t* d_ids, int64_t n, int invert, void* hip_stream, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (!rc) rc = filter_ids_args(x, d_ids, n, "dpq_filter_create_ids_device");
    if (rc) return rc;
    return filter_ids_on_device(x, d_ids, n, invert, reinterpret_cast<hipStream_t>(hip_stream), out);
    });
}

int dpq_filter_create_ids(dpq_index* x, const int32_t* ids, int64_t n, int invert, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (!rc) rc = filter_ids_args(x, ids, n, "dpq_filter_create_ids");
    if (rc) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    DevBuf<int32_t> d_ids;
    if ((rc = upload_temp(&d_ids, ids, n))) return rc;
    return filter_ids_on_device(x, d_ids, n, invert, nullptr, out);
    });
}

int dpq_filter_create_range(dpq_index* x, int64_t lo, int64_t hi, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (rc) return rc;
    if (!x || lo > hi) return fail(DPQ_ERR_ARG, "dpq_filter_create_range: NULL index or lo > hi");
    const int64_t lo0 = std::max<int64_t>(lo, 0), hi0 = std::max<int64_t>(hi, 0);  // (no reported id is negative)
    return filter_build(x, nullptr, out, [&](const dpq::FilterGeom& g, uint32_t* bits, unsigned long long* count) {
        return dpq::launch_filter_range(lo0, hi0, g, bits, count, nullptr);
    });
    });
}

int dpq_set_vec_ids(dpq_index* x, const uint32_t* vec_id, int64_t n) {
    return guarded([&]() -> int {
    if (!x || n < 0 || (n > 0 && !vec_id)) return fail(DPQ_ERR_ARG, "dpq_set_vec_ids: NULL argument or n < 0");
    if (n != x->img.n_local) return fail(DPQ_ERR_ARG, "dpq_set_vec_ids: n must be node_hi - node_lo of this handle");
    DPQ_HIP(hipSetDevice(x->device));
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    x->vec_ids_set = false;
    if (int rc = x->d_vec_id.alloc((size_t)n)) return rc;
    if (n > 0) DPQ_HIP(hipMemcpy(x->d_vec_id, vec_id, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    x->vec_ids_set = true;
    return DPQ_OK;
    });
}

int dpq_filter_create_vec_device(dpq_index* x, const uint32_t* d_words, int64_t n_bits, void* hip_stream, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (!rc) rc = filter_bitmap_args(x, d_words, n_bits, "dpq_filter_create_vec_device");
    if (rc) return rc;
    if (!x->vec_ids_set) return fail(DPQ_ERR_STATE, "dpq_set_vec_ids has not been called");
    return filter_vec_on_device(x, d_words, n_bits, reinterpret_cast<hipStream_t>(hip_stream), out);
    });
}

int dpq_filter_create_vec(dpq_index* x, const uint32_t* words, int64_t n_bits, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (!rc) rc = filter_bitmap_args(x, words, n_bits, "dpq_filter_create_vec");
    if (rc) return rc;
    if (!x->vec_ids_set) return fail(DPQ_ERR_STATE, "dpq_set_vec_ids has not been called");
    DPQ_HIP(hipSetDevice(x->device));
    DevBuf<uint32_t> d_words;
    if ((rc = upload_temp(&d_words, words, (n_bits + 31) / 32))) return rc;
    return filter_vec_on_device(x, d_words, n_bits, nullptr, out);
    });
}

int dpq_filter_combine(dpq_index* x, int op, const dpq_filter* a, const dpq_filter* b, dpq_filter** out) {
    return guarded([&]() -> int {
    int rc = filter_out_arg(out);
    if (rc) return rc;
    if (!x) return fail(DPQ_ERR_ARG, "dpq_filter_combine: NULL index");
    if (op < DPQ_FILTER_AND || op > DPQ_FILTER_NOT) return fail(DPQ_ERR_ARG, "dpq_filter_combine: unknown op");
    if (!a || (op == DPQ_FILTER_NOT ? b != nullptr : b == nullptr))
        return fail(DPQ_ERR_ARG, "dpq_filter_combine: NOT takes one filter (b NULL), every other op two");
    if (a->owner != x->serial || (b && b->owner != x->serial))
        return fail(DPQ_ERR_ARG, "dpq_filter_combine: a filter was made for another index handle");
    return filter_build(x, nullptr, out, [&](const dpq::FilterGeom& g, uint32_t* bits, unsigned long long* count) {
        return dpq::launch_filter_combine(a->bits, b ? b->bits.get() : nullptr, (dpq::FilterOp)op, g, bits, count, nullptr);
    });
    });
}

int dpq_filter_to_bitmap(const dpq_filter* f, uint32_t* words_out, int64_t n_bits) {
    return guarded([&]() -> int {
    if (!f || n_bits < 0 || (n_bits > 0 && !words_out)) return fail(DPQ_ERR_ARG, "dpq_filter_to_bitmap: NULL argument or n_bits < 0");
    if (n_bits == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(f->device));
    std::vector<uint32_t> h((size_t)f->n_words);
    DPQ_HIP(hipMemcpy(h.data(), f->bits, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::fill(words_out, words_out + (n_bits + 31) / 32, 0u);
    const bool even = !f->plain && (f->N & 1) == 0;
    for (int64_t w = 0; w < f->n_words && 32 * w < f->n_local; ++w)
        for (uint32_t v = h[(size_t)w]; v; v &= v - 1) {
            const int64_t pos = f->base + 32 * w + __builtin_ctz(v);
            const int64_t r = (even && pos == f->N - 1) ? f->N : pos;  // report_id
            if (r < n_bits) words_out[r >> 5] |= 1u << (r & 31);
        }
    return DPQ_OK;
    });
}

int dpq_bitmap_from_mask_device(const uint8_t* d_mask, int64_t n, uint32_t* d_words_out, int device, void* hip_stream) {
    return guarded([&]() -> int {
    if (n < 0 || (n > 0 && (!d_mask || !d_words_out))) return fail(DPQ_ERR_ARG, "dpq_bitmap_from_mask_device: NULL argument or n < 0");
    if (n == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(device));
    DPQ_HIP(dpq::launch_bitmap_from_mask(d_mask, n, d_words_out, reinterpret_cast<hipStream_t>(hip_stream)));
    return DPQ_OK;
    });
}

int dpq_bitmap_from_ids_device(const int32_t* d_ids, int64_t n, int64_t n_bits, uint32_t* d_words_out, int device,
                               void* hip_stream) {
    return guarded([&]() -> int {
    if (n < 0 || n_bits < 0 || (n > 0 && !d_ids) || (n_bits > 0 && !d_words_out))
        return fail(DPQ_ERR_ARG, "dpq_bitmap_from_ids_device: NULL argument, n < 0 or n_bits < 0");
    if (n_bits == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(device));
    DPQ_HIP(dpq::launch_bitmap_from_ids(d_ids, n, n_bits, d_words_out, reinterpret_cast<hipStream_t>(hip_stream)));
    return DPQ_OK;
    });
}

// ---- code lookup: dpq_get_codes / dpq_reconstruct / dpq_decode_range (include/deltapq_amd.h) ----
namespace {

constexpr size_t kLookupVecBytes = (size_t)64 << 20;       // staging of reconstructed rows (host variant), per slice
constexpr int64_t kLookupTileNodes = (int64_t)4 << 20;     // dpq_decode_range: nodes decoded per tile

// Does the reported id (>= 0) name a node of this handle?  The inverse of report_id (dpq_kernels.hip) and of the
// handle's position range; lookup_kernel applies the same rule on the device.
bool lookup_id_ok(const dpq_index* x, int64_t id) {
    const int64_t N = x->img.n_codes_total;
    int64_t pos = id;
    if (!x->plain && (N & 1) == 0) {
        if (id == N)
            pos = N - 1;
        else if (id == N - 1)
            return false;
    }
    const int64_t l = pos - (int64_t)x->img.id_base;
    return l >= 0 && l < x->img.n_local;
}

// Chooses the path of a call of n requests and, for the grouped path, decodes every segment of the handle once into
// the lookup's scratch: *img is the image the call's launches read (img->raw set = the decoded scratch).
int lookup_begin(dpq_index* x, int64_t n, hipStream_t stream, dpq::DeviceImage* img) {
    LookupWs& lw = x->lookup;
    *img = x->img;
    const int64_t image_bytes = (int64_t)x->img.n_segments * dpq::kChunk * x->img.chunks_per_segment * x->M;
    const bool possible = !x->plain && x->img.n_segments > 0 && image_bytes <= dpq::kLookupGroupedMaxBytes;
    bool grouped = possible && n >= dpq::kLookupGroupedPerSegment * (int64_t)x->img.n_segments;
    if (possible && dev_mode())
        if (const char* e = getenv("DPQ_LOOKUP_GROUPED")) grouped = atoi(e) != 0;  // developer A/B: 0 never, 1 always
    if (!grouped) return DPQ_OK;
    if (int rc = grow(lw.tile, &lw.tile_n, (size_t)image_bytes)) return rc;
    DPQ_HIP(dpq::launch_decode_list(x->img, nullptr, x->img.n_segments, nullptr, reinterpret_cast<uint32_t*>(lw.tile.get()),
                                    stream));
    img->raw = lw.tile;
    return DPQ_OK;
}

// A scratch beyond the kept bound (one dpq_decode_range tile) is released once the call's work is done.
void lookup_end(dpq_index* x) {
    LookupWs& lw = x->lookup;
    if (lw.tile_n > (size_t)(kLookupTileNodes + 1024 * dpq::kChunk) * x->M) {
        lw.tile.reset();
        lw.tile_n = 0;
    }
}

// n requests, all device pointers, in launches of kLookupSlice on `stream`; ends with the flag word read back.
int lookup_run(dpq_index* x, const dpq::DeviceImage& img, const int32_t* d_ids, int64_t n, uint8_t* d_codes, float* d_vecs,
               hipStream_t stream, const char* who) {
    LookupWs& lw = x->lookup;
    int rc;
    if (!lw.flag.get() && (rc = lw.flag.alloc(1))) return rc;
    DPQ_HIP(hipMemsetAsync(lw.flag, 0, sizeof(uint32_t), stream));
    const size_t D = (size_t)x->M * x->Ds;
    for (int64_t i0 = 0; i0 < n; i0 += dpq::kLookupSlice) {
        dpq::LookupArgs a{};
        a.img = img;
        a.ids = d_ids + i0;
        a.n = std::min(dpq::kLookupSlice, n - i0);
        a.even_rule = x->plain ? 0 : 1;
        if (d_vecs) {
            a.out_vecs = d_vecs + (size_t)i0 * D;
            a.codebook = x->d_codebook;
            a.Ds = x->Ds;
        } else {
            a.out_codes = d_codes + (size_t)i0 * x->M;
        }
        a.flag = lw.flag;
        DPQ_HIP(dpq::launch_lookup(a, stream));
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(&bad, lw.flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, std::string(who) + ": an id names no node of this handle");
    return DPQ_OK;
}

// One call with device pointers: path choice, launches, release.
int lookup_on_device(dpq_index* x, const int32_t* d_ids, int64_t n, uint8_t* d_codes, float* d_vecs, hipStream_t stream,
                     const char* who) {
    dpq::DeviceImage img;
    int rc = lookup_begin(x, n, stream, &img);
    if (!rc) rc = lookup_run(x, img, d_ids, n, d_codes, d_vecs, stream, who);
    if (rc) hipStreamSynchronize(stream);  // (a failed call: nothing may still read the scratch)
    lookup_end(x);
    return rc;
}

// The argument rules shared by the four id-list entry points; finishes pending asynchronous batches.
int lookup_args(dpq_index* x, const void* ids, int64_t n, const void* out, bool recon, const char* who) {
    if (!x || n < 0 || (n > 0 && (!ids || !out))) return fail(DPQ_ERR_ARG, std::string(who) + ": NULL argument or n < 0");
    if (recon && !x->d_codebook) return fail(DPQ_ERR_STATE, "dpq_set_codebook has not been called");
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    return DPQ_OK;
}

int lookup_host(dpq_index* x, const int32_t* ids, int64_t n, uint8_t* codes_out, float* vecs_out, const char* who) {
    int rc = lookup_args(x, ids, n, codes_out ? (const void*)codes_out : (const void*)vecs_out, vecs_out != nullptr, who);
    if (rc || n == 0) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= 0 && !lookup_id_ok(x, ids[i])) {
            char msg[160];
            snprintf(msg, sizeof msg, "%s: ids[%lld] = %d names no node of this handle", who, (long long)i, (int)ids[i]);
            return fail(DPQ_ERR_ARG, msg);
        }
    DPQ_HIP(hipSetDevice(x->device));
    LookupWs& lw = x->lookup;
    const size_t D = (size_t)x->M * x->Ds;
    int64_t slice = dpq::kLookupSlice;
    if (vecs_out) slice = std::max<int64_t>(1, std::min<int64_t>(slice, (int64_t)(kLookupVecBytes / (D * sizeof(float)))));
    slice = std::min(slice, n);
    rc = grow(lw.ids, &lw.ids_n, (size_t)slice);
    if (!rc && vecs_out) rc = grow(lw.vecs, &lw.vecs_n, (size_t)slice * D);
    if (!rc && codes_out) rc = grow(lw.codes, &lw.codes_n, (size_t)slice * x->M);
    if (rc) return rc;
    // the path is chosen once for the whole call: a grouped call decodes the handle once, whatever the number of slices
    dpq::DeviceImage img;
    rc = lookup_begin(x, n, nullptr, &img);
    for (int64_t i0 = 0; !rc && i0 < n; i0 += slice) {
        const int64_t m = std::min(slice, n - i0);
        hipError_t e = hipMemcpy(lw.ids, ids + i0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            rc = lookup_run(x, img, lw.ids, m, codes_out ? lw.codes.get() : nullptr, vecs_out ? lw.vecs.get() : nullptr, nullptr,
                            who);
        if (e == hipSuccess && !rc)
            e = vecs_out ? hipMemcpy(vecs_out + (size_t)i0 * D, lw.vecs, (size_t)m * D * sizeof(float), hipMemcpyDeviceToHost)
                         : hipMemcpy(codes_out + (size_t)i0 * x->M, lw.codes, (size_t)m * x->M, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(DPQ_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    hipDeviceSynchronize();
    lookup_end(x);
    return rc;
}

}  // namespace

int dpq_get_codes(dpq_index* x, const int32_t* ids, int64_t n, uint8_t* codes_out) {
    return guarded([&]() -> int { return lookup_host(x, ids, n, codes_out, nullptr, "dpq_get_codes"); });
}

int dpq_reconstruct(dpq_index* x, const int32_t* ids, int64_t n, float* vectors_out) {
    return guarded([&]() -> int {
    if (!vectors_out && n != 0) return fail(DPQ_ERR_ARG, "dpq_reconstruct: NULL argument or n < 0");
    return lookup_host(x, ids, n, nullptr, vectors_out, "dpq_reconstruct");
    });
}

int dpq_get_codes_device(dpq_index* x, const int32_t* d_ids, int64_t n, uint8_t* d_codes, void* hip_stream) {
    return guarded([&]() -> int {
    int rc = lookup_args(x, d_ids, n, d_codes, false, "dpq_get_codes_device");
    if (rc || n == 0) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    return lookup_on_device(x, d_ids, n, d_codes, nullptr, (hipStream_t)hip_stream, "dpq_get_codes_device");
    });
}

int dpq_reconstruct_device(dpq_index* x, const int32_t* d_ids, int64_t n, float* d_vectors, void* hip_stream) {
    return guarded([&]() -> int {
    int rc = lookup_args(x, d_ids, n, d_vectors, true, "dpq_reconstruct_device");
    if (rc || n == 0) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    return lookup_on_device(x, d_ids, n, nullptr, d_vectors, (hipStream_t)hip_stream, "dpq_reconstruct_device");
    });
}

int dpq_decode_range(dpq_index* x, int64_t first, int64_t count, uint8_t* codes_out) {
    return guarded([&]() -> int {
    if (!x || !codes_out) return fail(DPQ_ERR_ARG, "dpq_decode_range: NULL argument");
    if (first < 0 || count < 0 || first < x->info.node_lo || first > x->info.node_hi || count > x->info.node_hi - first)
        return fail(DPQ_ERR_ARG, "dpq_decode_range: [first, first + count) is not inside the handle's [node_lo, node_hi)");
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    if (count == 0) return DPQ_OK;
    DPQ_HIP(hipSetDevice(x->device));
    const int M = x->M;
    const int64_t l0 = first - x->info.node_lo, l1 = l0 + count;  // local positions
    if (x->plain) {
        DPQ_HIP(hipMemcpy(codes_out, x->d_raw.get() + (size_t)l0 * M, (size_t)count * M, hipMemcpyDeviceToHost));
        return DPQ_OK;
    }
    // the segments that cover the range, a tile at a time through the per-batch decode (no relabelling) into the
    // lookup's own scratch; the partial first and last segments are trimmed by the copies
    LookupWs& lw = x->lookup;
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    const int64_t seg0 = l0 / S, seg1 = (l1 + S - 1) / S;
    const int64_t tile = std::min(std::max<int64_t>(1, kLookupTileNodes / S), seg1 - seg0);
    int rc = grow(lw.tile, &lw.tile_n, (size_t)(tile * S * M));
    if (!rc) rc = grow(lw.tile_segs, &lw.tile_segs_n, (size_t)tile);
    if (rc) return rc;
    std::vector<uint32_t> segs((size_t)tile);
    for (int64_t t0 = seg0; t0 < seg1; t0 += tile) {
        const int64_t nt = std::min(tile, seg1 - t0);
        for (int64_t j = 0; j < nt; ++j) segs[(size_t)j] = (uint32_t)(t0 + j);
        DPQ_HIP(hipMemcpy(lw.tile_segs, segs.data(), (size_t)nt * sizeof(uint32_t), hipMemcpyHostToDevice));
        DPQ_HIP(dpq::launch_decode_list(x->img, lw.tile_segs, (int)nt, nullptr, reinterpret_cast<uint32_t*>(lw.tile.get()),
                                        nullptr));
        const int64_t a = std::max(l0, t0 * S), b = std::min(l1, (t0 + nt) * S);
        DPQ_HIP(hipMemcpy(codes_out + (size_t)(a - l0) * M, lw.tile.get() + (size_t)(a - t0 * S) * M, (size_t)(b - a) * M,
                          hipMemcpyDeviceToHost));
    }
    return DPQ_OK;
    });
}

int dpq_dtc_decode(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, int64_t first, int64_t count,
                   uint8_t* codes_out) {
    return guarded([&]() -> int {
    std::string err;
    int rc = dpq::decode_codes(payload, n_bytes, n_codes, M, first, count, codes_out, &err);
    return rc ? fail(rc, err) : DPQ_OK;
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
    x->range.last_max_keys = 0;
    std::unique_ptr<dpq_range_result> res(new dpq_range_result());
    res->nq = nq;
    res->lims.assign((size_t)nq + 1, 0);
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
        const int D = x->M * x->Ds;
        int rc = DPQ_OK;
        for (int base = 0; base < nq && !rc; base += kMaxBatchQueries) {
            const int n = std::min(kMaxBatchQueries, nq - base);
            rc = range_batch(x, x->d_q_stage + (size_t)base * D, n, radii + base, base, res.get(), nullptr);
        }
        range_trim(x);
        if (rc) return rc;
        if (x->prof) x->prof_acc.queries += nq;
    }
    *out = res.release();
    return DPQ_OK;
    });
}

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

int dpq_merge_topk_host(const int32_t* ids, const float* dists, int n_lists, int nq, int top_k, int32_t* out_ids,
                        float* out_dists) {
    return guarded([&]() -> int {
    if (!ids || !dists || !out_ids || !out_dists || n_lists < 1 || nq < 0 || top_k < 1)
        return fail(DPQ_ERR_ARG, "bad merge argument");
    std::vector<uint64_t> keys;
    for (int q = 0; q < nq; ++q) {
        keys.clear();
        for (int l = 0; l < n_lists; ++l)
            for (int r = 0; r < top_k; ++r) {
                const size_t o = ((size_t)l * nq + q) * top_k + r;
                if (ids[o] < 0) continue;
                uint32_t bits;
                memcpy(&bits, &dists[o], 4);
                keys.push_back(((uint64_t)bits << 32) | (uint32_t)ids[o]);
            }
        const size_t kk = std::min((size_t)top_k, keys.size());
        std::partial_sort(keys.begin(), keys.begin() + kk, keys.end());
        for (int r = 0; r < top_k; ++r) {
            const size_t o = (size_t)q * top_k + r;
            if ((size_t)r < kk) {
                out_ids[o] = (int32_t)(keys[r] & 0xffffffffu);
                uint32_t bits = (uint32_t)(keys[r] >> 32);
                memcpy(&out_dists[o], &bits, 4);
            } else {
                out_ids[o] = -1;
                out_dists[o] = INFINITY;
            }
        }
    }
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

// Developer hook: time the level-0 select (shared, query-independent candidate list).
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

// ---- residual re-ranking (include/deltapq_amd.h "residual re-ranking"; kernels in dpq_refine.hip) ----
// A second PQ level over the residuals of a handle's nodes: its own copy of the level-1 codebook, its codebook, a code
// per node, and the workspaces of one slice.
struct dpq_refine {
    uint64_t owner = 0;        // dpq_index::serial of the handle it was made for
    dpq_index* idx = nullptr;  // that handle: it outlives the level (header)
    int device = 0;
    int M = 0, K = 0, Ds = 0, D1 = 0, M2 = 0, K2 = 0, Ds2 = 0;
    int64_t n_local = 0;
    DevBuf<float> cw1, cw2;    // [M][K][Ds] as dpq_set_codebook received it when the level was made; [M2][K2][Ds2]
    DevBuf<uint8_t> codes2;    // [n_local][M2]
    // workspaces, grown on demand and kept until dpq_refine_free
    DevBuf<uint8_t> codes1;    // [slice][M] level-1 codes of a slice of candidates
    DevBuf<uint64_t> keys;
    DevBuf<uint32_t> flag;
    DevBuf<float> d_q, d_dists, d_cdist;
    DevBuf<int32_t> d_cand, d_ids;
    size_t codes1_n = 0, keys_n = 0, q_n = 0, out_n = 0, cand_n = 0, cdist_n = 0;
};

namespace {

// rows of D1 floats one slice holds: at most 2^20, and at most 128 MB of them
int64_t refine_slice_rows(int D1) {
    return std::max<int64_t>(1, std::min<int64_t>(dpq::kRefineSlice, ((int64_t)1 << 25) / D1));
}

// the rules of a level's shape that need no handle
int refine_shape_args(const std::string& who, int M2, int K2, int Ds2) {
    if (M2 < 1 || M2 > dpq::kRefineMaxM2) return fail(DPQ_ERR_ARG, who + ": M2 outside 1..64");
    if (K2 < 2 || K2 > 256) return fail(DPQ_ERR_ARG, who + ": K2 outside 2..256 (one byte per code)");
    if (Ds2 < 1) return fail(DPQ_ERR_ARG, who + ": Ds2 < 1");
    return DPQ_OK;
}

// ... and those that need its D1
int refine_shape_fits(const std::string& who, int D1, int M2, int Ds2) {
    if (Ds2 != (D1 + M2 - 1) / M2) return fail(DPQ_ERR_ARG, who + ": Ds2 is not ceil(M * Ds / M2)");
    if ((int64_t)(M2 - 1) * Ds2 >= D1) return fail(DPQ_ERR_ARG, who + ": (M2 - 1) * Ds2 >= M * Ds, a sub-space with no real dimension");
    return DPQ_OK;
}

// a handle a level can stand on: a codebook, and an M the code lookup decodes
int refine_handle_ok(const std::string& who, const dpq_index* x) {
    if (!x->d_codebook) return fail(DPQ_ERR_STATE, who + ": dpq_set_codebook has not been called");
    if (x->M != 8 && x->M != 16) return fail(DPQ_ERR_ARG, who + ": needs a handle of M = 8 or M = 16");
    return DPQ_OK;
}

int refine_rows_fit(const std::string& who, const dpq_index* x, int D) {
    if ((D + x->M - 1) / x->M != x->Ds) return fail(DPQ_ERR_ARG, who + ": ceil(D / M) is not the codebook's Ds");
    return DPQ_OK;
}

dpq::RefineIds refine_ids(const dpq_index* x) {
    dpq::RefineIds r{};
    r.id_base = (int64_t)x->img.id_base;
    r.n_local = x->img.n_local;
    r.n_total = x->img.n_codes_total;
    r.even_rule = x->plain ? 0 : 1;
    return r;
}

dpq::RefineLevelArgs refine_level(const dpq_refine* r) {
    dpq::RefineLevelArgs lv{};
    lv.cw1 = r->cw1;
    lv.cw2 = r->cw2;
    lv.codes2 = r->codes2;
    lv.M = r->M; lv.K = r->K; lv.Ds = r->Ds; lv.D1 = r->D1;
    lv.M2 = r->M2; lv.K2 = r->K2; lv.Ds2 = r->Ds2;
    return lv;
}

// level-1 side only: residuals against a codebook on the device
dpq::RefineLevelArgs refine_level1(const dpq_index* x, const float* d_cw1) {
    dpq::RefineLevelArgs lv{};
    lv.cw1 = d_cw1;
    lv.M = x->M; lv.K = x->K; lv.Ds = x->Ds; lv.D1 = x->M * x->Ds;
    return lv;
}

// the reported id of local node l: the inverse of lookup_id_ok
int32_t refine_report_id(const dpq_index* x, int64_t l) {
    const int64_t pos = (int64_t)x->img.id_base + l, N = x->img.n_codes_total;
    return (int32_t)(!x->plain && (N & 1) == 0 && pos == N - 1 ? N : pos);
}

int refine_ids_ok(const dpq_index* x, const int32_t* ids, int64_t n, const std::string& who) {
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= 0 && !lookup_id_ok(x, ids[i])) {
            char msg[96];
            snprintf(msg, sizeof msg, ": entry %lld = %d names no node of this handle", (long long)i, (int)ids[i]);
            return fail(DPQ_ERR_ARG, who + msg);
        }
    return DPQ_OK;
}

// The level-1 codes of local nodes [l0, l0 + m), m <= 2^20, on the device: the rows of a plain handle, or the segments
// that cover them decoded into the lookup's scratch (dpq_decode_range's path).  *codes stays valid until that scratch
// is used again.
int refine_decode_slice(dpq_index* x, int64_t l0, int64_t m, const uint8_t** codes) {
    const int M = x->M;
    if (x->plain) {
        *codes = x->d_raw.get() + (size_t)l0 * M;
        return DPQ_OK;
    }
    LookupWs& lw = x->lookup;
    const int64_t S = (int64_t)dpq::kChunk * x->img.chunks_per_segment;
    const int64_t seg0 = l0 / S, seg1 = (l0 + m + S - 1) / S, nt = seg1 - seg0;
    int rc = grow(lw.tile, &lw.tile_n, (size_t)(nt * S * M));
    if (!rc) rc = grow(lw.tile_segs, &lw.tile_segs_n, (size_t)nt);
    if (rc) return rc;
    std::vector<uint32_t> segs((size_t)nt);
    for (int64_t j = 0; j < nt; ++j) segs[(size_t)j] = (uint32_t)(seg0 + j);
    DPQ_HIP(hipMemcpy(lw.tile_segs, segs.data(), (size_t)nt * sizeof(uint32_t), hipMemcpyHostToDevice));
    DPQ_HIP(dpq::launch_decode_list(x->img, lw.tile_segs, (int)nt, nullptr, reinterpret_cast<uint32_t*>(lw.tile.get()), nullptr));
    *codes = lw.tile.get() + (size_t)(l0 - seg0 * S) * M;
    return DPQ_OK;
}

// dpq_residuals after its checks: ids and rows a slice at a time through the code lookup.
int residuals_host(dpq_index* x, const int32_t* ids, int64_t n, const float* vectors, int D, float* out, const char* who) {
    const int D1 = x->M * x->Ds;
    const int64_t slice = std::min(n, refine_slice_rows(D1));
    LookupWs& lw = x->lookup;
    DevBuf<float> d_rows, d_res;
    int rc = grow(lw.ids, &lw.ids_n, (size_t)slice);
    if (!rc) rc = grow(lw.codes, &lw.codes_n, (size_t)slice * x->M);
    if (!rc) rc = d_rows.alloc((size_t)slice * D);
    if (!rc) rc = d_res.alloc((size_t)slice * D1);
    if (rc) return rc;
    const dpq::RefineLevelArgs lv = refine_level1(x, x->d_codebook);
    for (int64_t i0 = 0; i0 < n; i0 += slice) {
        const int64_t m = std::min(slice, n - i0);
        DPQ_HIP(hipMemcpy(lw.ids, ids + i0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
        DPQ_HIP(hipMemcpy(d_rows, vectors + (size_t)i0 * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice));
        if ((rc = lookup_on_device(x, lw.ids, m, lw.codes, nullptr, nullptr, who))) return rc;
        DPQ_HIP(dpq::launch_refine_residual(d_rows, m, D, lw.ids, lw.codes, lv, d_res, nullptr));
        DPQ_HIP(hipMemcpy(out + (size_t)i0 * D1, d_res, (size_t)m * D1 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return DPQ_OK;
}

// A level over handle x from a codebook on the host and codes on the host (h_codes2) or already on the device.
int refine_make(dpq_index* x, const float* cw2, int M2, int K2, int Ds2, const uint8_t* h_codes2, DevBuf<uint8_t>* d_codes2,
                dpq_refine** out) {
    std::unique_ptr<dpq_refine> r(new dpq_refine);
    r->owner = x->serial;
    r->idx = x;
    r->device = x->device;
    r->M = x->M; r->K = x->K; r->Ds = x->Ds; r->D1 = x->M * x->Ds;
    r->M2 = M2; r->K2 = K2; r->Ds2 = Ds2;
    r->n_local = x->img.n_local;
    const size_t n1 = (size_t)r->M * r->K * r->Ds, n2 = (size_t)M2 * K2 * Ds2, nc = (size_t)r->n_local * M2;
    int rc = r->cw1.alloc(n1);
    if (!rc) rc = r->cw2.alloc(n2);
    if (!rc) rc = r->flag.alloc(1);
    if (!rc && !d_codes2) rc = r->codes2.alloc(nc);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(r->cw1, x->d_codebook, n1 * sizeof(float), hipMemcpyDeviceToDevice));
    DPQ_HIP(hipMemcpy(r->cw2, cw2, n2 * sizeof(float), hipMemcpyHostToDevice));
    if (d_codes2)
        r->codes2 = std::move(*d_codes2);
    else
        DPQ_HIP(hipMemcpy(r->codes2, h_codes2, nc, hipMemcpyHostToDevice));
    *out = r.release();
    return DPQ_OK;
}

// Candidates of dpq_refine_rerank*, all device pointers; ends with one flag word read back.
int refine_rerank_on_device(const char* fn, dpq_refine* r, const float* d_queries, int nq, const int32_t* d_cand, int n_cand,
                            int top_k, int32_t* d_ids, float* d_dists, hipStream_t stream) {
    dpq_index* x = r->idx;
    const size_t n_pad = dpq::refine_rerank_keys(n_cand);
    const int per = (int)std::max<int64_t>(1, std::min<int64_t>(nq, dpq::kRefineSlice / n_cand));
    int rc = grow(r->codes1, &r->codes1_n, (size_t)per * n_cand * r->M);
    if (!rc) rc = grow(r->keys, &r->keys_n, (size_t)per * n_pad);
    if (rc) return rc;
    DPQ_HIP(hipMemsetAsync(r->flag, 0, sizeof(uint32_t), stream));
    const dpq::RefineLevelArgs lv = refine_level(r);
    const dpq::RefineIds rid = refine_ids(x);
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int m = std::min(per, nq - q0);
        const int32_t* cand = d_cand + (size_t)q0 * n_cand;
        // the slice's level-1 codes by the code lookup (a candidate that names no node ends the call there)
        if ((rc = lookup_on_device(x, cand, (int64_t)m * n_cand, r->codes1, nullptr, stream, fn))) return rc;
        DPQ_HIP(dpq::launch_refine_rerank(d_queries + (size_t)q0 * r->D1, m, cand, n_cand, top_k, r->codes1, lv, rid, r->keys,
                                          r->flag, d_ids + (size_t)q0 * top_k, d_dists + (size_t)q0 * top_k, stream));
    }
    uint32_t bad = 0;
    DPQ_HIP(hipMemcpyAsync(&bad, r->flag, sizeof bad, hipMemcpyDeviceToHost, stream));
    DPQ_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(DPQ_ERR_ARG, std::string(fn) + ": a candidate names no node of this handle");
    return DPQ_OK;
}

int refine_rerank_args(const std::string& who, const void* r, const void* queries, int nq, const void* cand, int n_cand,
                       int top_k, const void* ids, const void* dists) {
    if (!r || !queries || !cand || !ids || !dists || nq < 0) return fail(DPQ_ERR_ARG, who + ": NULL argument or nq < 0");
    if (top_k < 1 || top_k > n_cand || n_cand > dpq::kRefineMaxCand)
        return fail(DPQ_ERR_ARG, who + ": needs 1 <= top_k <= n_cand <= 16384");
    return DPQ_OK;
}

int refine_grow_outputs(dpq_refine* r, size_t want) {
    if (r->out_n >= want) return DPQ_OK;
    r->out_n = 0;
    int rc = r->d_ids.alloc(want);
    if (!rc) rc = r->d_dists.alloc(want);
    if (!rc) r->out_n = want;
    return rc;
}

// settles what is in flight on the level's handle and selects its device
int refine_enter(dpq_refine* r) {
    if (!r->idx->pending.empty())
        if (int rc = dpq_finish(r->idx)) return rc;
    DPQ_HIP(hipSetDevice(r->device));
    return DPQ_OK;
}

}  // namespace

extern "C" {

int dpq_residuals(dpq_index* x, const int32_t* ids, int64_t n, const float* vectors, int D, float* out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_residuals";
    if (!x || n < 0 || (n > 0 && (!ids || !vectors || !out))) return fail(DPQ_ERR_ARG, who + ": NULL argument or n < 0");
    if (D < 1) return fail(DPQ_ERR_ARG, who + ": D < 1");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = refine_handle_ok(who, x)) return rc;
    if (int rc = refine_rows_fit(who, x, D)) return rc;
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    if (n == 0) return DPQ_OK;
    if (int rc = refine_ids_ok(x, ids, n, who)) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    return residuals_host(x, ids, n, vectors, D, out, "dpq_residuals");
    });
}

int dpq_refine_create(dpq_index* x, const float* codewords2, int M2, int K2, int Ds2, const uint8_t* codes2, int64_t n_local,
                      dpq_refine** out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_refine_create";
    if (out) *out = nullptr;
    if (!x || !codewords2 || !codes2 || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = refine_shape_args(who, M2, K2, Ds2)) return rc;
    if (n_local < 1) return fail(DPQ_ERR_ARG, who + ": n_local < 1");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = refine_handle_ok(who, x)) return rc;
    if (int rc = refine_shape_fits(who, x->M * x->Ds, M2, Ds2)) return rc;
    if (n_local != x->img.n_local) return fail(DPQ_ERR_ARG, who + ": n_local is not the handle's node count");
    for (size_t i = 0; i < (size_t)n_local * M2; ++i)
        if (codes2[i] >= K2) return fail(DPQ_ERR_ARG, who + ": a code byte >= K2");
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    return refine_make(x, codewords2, M2, K2, Ds2, codes2, nullptr, out);
    });
}

void dpq_refine_free(dpq_refine* r) {
    if (!r) return;
    hipSetDevice(r->device);
    delete r;
}

int dpq_refine_get(const dpq_refine* r, int32_t* M2, int32_t* K2, int32_t* Ds2, int64_t* n_local, float* codewords2,
                   uint8_t* codes2) {
    return guarded([&]() -> int {
    if (!r) return fail(DPQ_ERR_ARG, "dpq_refine_get: NULL level");
    if (M2) *M2 = r->M2;
    if (K2) *K2 = r->K2;
    if (Ds2) *Ds2 = r->Ds2;
    if (n_local) *n_local = r->n_local;
    if (!codewords2 && !codes2) return DPQ_OK;
    DPQ_HIP(hipSetDevice(r->device));
    if (codewords2)
        DPQ_HIP(hipMemcpy(codewords2, r->cw2, (size_t)r->M2 * r->K2 * r->Ds2 * sizeof(float), hipMemcpyDeviceToHost));
    if (codes2) DPQ_HIP(hipMemcpy(codes2, r->codes2, (size_t)r->n_local * r->M2, hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_refine_build(dpq_index* x, const float* vectors, int64_t n_rows, int D, const uint32_t* vec_id,
                     const dpq_refine_opts* opts, dpq_refine** out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_refine_build";
    if (out) *out = nullptr;
    if (!x || !vectors || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n_rows < 1 || D < 1) return fail(DPQ_ERR_ARG, who + ": n_rows < 1 or D < 1");
    dpq_refine_opts o{};
    if (opts) o = *opts;
    if (o.M2 != 0 || o.K2 != 0)
        if (int rc = refine_shape_args(who, o.M2 ? o.M2 : 1, o.K2 ? o.K2 : 256, 1)) return rc;
    if (o.train_n < 0) return fail(DPQ_ERR_ARG, who + ": train_n < 0");
    if (o.max_iters < 0 || o.max_iters > 64) return fail(DPQ_ERR_ARG, who + ": max_iters outside 0..64");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = refine_handle_ok(who, x)) return rc;
    if (int rc = refine_rows_fit(who, x, D)) return rc;
    const int M = x->M, D1 = M * x->Ds;
    const int M2 = o.M2 ? o.M2 : M, K2 = o.K2 ? o.K2 : 256, Ds2 = (D1 + M2 - 1) / M2;
    if (int rc = refine_shape_fits(who, D1, M2, Ds2)) return rc;
    const int64_t n_local = x->img.n_local;
    if (!vec_id && n_rows != n_local) return fail(DPQ_ERR_ARG, who + ": without vec_id, n_rows must be the handle's node count");
    if (vec_id)
        for (int64_t l = 0; l < n_local; ++l)
            if ((int64_t)vec_id[l] >= n_rows) return fail(DPQ_ERR_ARG, who + ": a vec_id entry >= n_rows");
    const int64_t train_n = o.train_n ? o.train_n : std::min<int64_t>(n_local, (int64_t)256 * K2);
    if (train_n > n_local) return fail(DPQ_ERR_ARG, who + ": train_n above the handle's node count");
    if (!x->pending.empty())
        if (int rc = dpq_finish(x)) return rc;
    DPQ_HIP(hipSetDevice(x->device));
    auto row_of = [&](int64_t l) { return vectors + (size_t)(vec_id ? (int64_t)vec_id[l] : l) * D; };

    // the codebook: residuals of the sample, trained by the public trainer
    std::vector<float> cw2((size_t)M2 * K2 * Ds2);
    {
        std::vector<int32_t> s_ids((size_t)train_n);
        std::vector<float> s_rows((size_t)train_n * D), s_res((size_t)train_n * D1);
        for (int64_t i = 0; i < train_n; ++i) {
            const int64_t l = (int64_t)(((__int128)i * n_local) / train_n);
            s_ids[(size_t)i] = refine_report_id(x, l);
            memcpy(&s_rows[(size_t)i * D], row_of(l), (size_t)D * sizeof(float));
        }
        if (int rc = residuals_host(x, s_ids.data(), train_n, s_rows.data(), D, s_res.data(), "dpq_refine_build")) return rc;
        dpq_train_opts t{};
        t.device = x->device;
        t.max_iters = o.max_iters ? o.max_iters : 25;
        t.seed = o.seed;
        t.init = o.init;
        t.restarts = o.restarts;
        if (int rc = dpq_train_codebook(s_res.data(), train_n, D1, M2, K2, &t, cw2.data(), nullptr)) return rc;
        DPQ_HIP(hipSetDevice(x->device));
    }

    // the codes: every node, a slice at a time -- gather, upload, residual and encode on the device
    const int64_t slice = std::min(n_local, refine_slice_rows(D1));
    DevBuf<float> d_rows, d_res, d_cw2;
    DevBuf<uint8_t> d_codes2;
    int rc = d_rows.alloc((size_t)slice * D);
    if (!rc) rc = d_res.alloc((size_t)slice * D1);
    if (!rc) rc = d_cw2.alloc(cw2.size());
    if (!rc) rc = d_codes2.alloc((size_t)n_local * M2);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(d_cw2, cw2.data(), cw2.size() * sizeof(float), hipMemcpyHostToDevice));
    const dpq::RefineLevelArgs lv = refine_level1(x, x->d_codebook);
    std::vector<float> stage;
    for (int64_t l0 = 0; l0 < n_local; l0 += slice) {
        const int64_t m = std::min(slice, n_local - l0);
        const float* src = vectors + (size_t)l0 * D;
        if (vec_id) {
            stage.resize((size_t)m * D);
            for (int64_t i = 0; i < m; ++i) memcpy(&stage[(size_t)i * D], row_of(l0 + i), (size_t)D * sizeof(float));
            src = stage.data();
        }
        DPQ_HIP(hipMemcpy(d_rows, src, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice));
        const uint8_t* codes1 = nullptr;
        if ((rc = refine_decode_slice(x, l0, m, &codes1))) return rc;
        DPQ_HIP(dpq::launch_refine_residual(d_rows, m, D, nullptr, codes1, lv, d_res, nullptr));
        DPQ_HIP(dpq::launch_encode_pq(d_res, m, D1, d_cw2, M2, K2, Ds2, d_codes2.get() + (size_t)l0 * M2, nullptr));
        DPQ_HIP(hipDeviceSynchronize());
    }
    return refine_make(x, cw2.data(), M2, K2, Ds2, nullptr, &d_codes2, out);
    });
}

int dpq_refine_reconstruct(dpq_refine* r, const int32_t* ids, int64_t n, float* out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_refine_reconstruct";
    if (!r || n < 0 || (n > 0 && (!ids || !out))) return fail(DPQ_ERR_ARG, who + ": NULL argument or n < 0");
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = refine_enter(r)) return rc;
    if (n == 0) return DPQ_OK;
    dpq_index* x = r->idx;
    if (int rc = refine_ids_ok(x, ids, n, who)) return rc;
    const int64_t slice = std::min(n, refine_slice_rows(r->D1));
    LookupWs& lw = x->lookup;
    DevBuf<float> d_out;
    int rc = grow(lw.ids, &lw.ids_n, (size_t)slice);
    if (!rc) rc = grow(lw.codes, &lw.codes_n, (size_t)slice * r->M);
    if (!rc) rc = d_out.alloc((size_t)slice * r->D1);
    if (rc) return rc;
    const dpq::RefineLevelArgs lv = refine_level(r);
    const dpq::RefineIds rid = refine_ids(x);
    for (int64_t i0 = 0; i0 < n; i0 += slice) {
        const int64_t m = std::min(slice, n - i0);
        DPQ_HIP(hipMemcpy(lw.ids, ids + i0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
        if ((rc = lookup_on_device(x, lw.ids, m, lw.codes, nullptr, nullptr, "dpq_refine_reconstruct"))) return rc;
        DPQ_HIP(dpq::launch_refine_reconstruct(lw.ids, m, lw.codes, lv, rid, d_out, nullptr));
        DPQ_HIP(hipMemcpy(out + (size_t)i0 * r->D1, d_out, (size_t)m * r->D1 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return DPQ_OK;
    });
}

int dpq_refine_rerank_device(dpq_refine* r, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand, int top_k,
                             int32_t* d_ids, float* d_dists, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_refine_rerank_device";
    if (int rc = refine_rerank_args(who, r, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids, d_dists)) return rc;
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = refine_enter(r)) return rc;
    if (nq == 0) return DPQ_OK;
    return refine_rerank_on_device("dpq_refine_rerank_device", r, d_queries, nq, d_cand_ids, n_cand, top_k, d_ids, d_dists,
                                   (hipStream_t)hip_stream);
    });
}

int dpq_refine_rerank(dpq_refine* r, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k, int32_t* ids,
                      float* dists) {
    return guarded([&]() -> int {
    const std::string who = "dpq_refine_rerank";
    if (int rc = refine_rerank_args(who, r, queries, nq, cand_ids, n_cand, top_k, ids, dists)) return rc;
    if (int rc = flat_device_present(who)) return rc;
    if (int rc = refine_enter(r)) return rc;
    if (nq == 0) return DPQ_OK;
    if (int rc = refine_ids_ok(r->idx, cand_ids, (int64_t)nq * n_cand, who)) return rc;
    int rc = grow(r->d_q, &r->q_n, (size_t)nq * r->D1);
    if (!rc) rc = grow(r->d_cand, &r->cand_n, (size_t)nq * n_cand);
    if (!rc) rc = refine_grow_outputs(r, (size_t)nq * top_k);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(r->d_q, queries, (size_t)nq * r->D1 * sizeof(float), hipMemcpyHostToDevice));
    DPQ_HIP(hipMemcpy(r->d_cand, cand_ids, (size_t)nq * n_cand * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = refine_rerank_on_device("dpq_refine_rerank", r, r->d_q, nq, r->d_cand, n_cand, top_k, r->d_ids, r->d_dists, nullptr);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(ids, r->d_ids, (size_t)nq * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, r->d_dists, (size_t)nq * top_k * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_query_batch_refined(dpq_index* x, dpq_refine* r, const dpq_filter* filter, const float* queries, int nq, int n_cand,
                            int top_k, int32_t* ids, float* dists) {
    return guarded([&]() -> int {
    const std::string who = "dpq_query_batch_refined";
    if (!x) return fail(DPQ_ERR_ARG, who + ": NULL index");
    // (the candidates are the PQ answer: the queries stand in for their pointer in the shared check)
    if (int rc = refine_rerank_args(who, r, queries, nq, queries, n_cand, top_k, ids, dists)) return rc;
    if (int rc = flat_device_present(who)) return rc;
    if (r->owner != x->serial) return fail(DPQ_ERR_ARG, who + ": the level was made for another index handle");
    if (filter)
        if (int rc = check_filter(x, filter)) return rc;
    if (int rc = refine_enter(r)) return rc;
    if (int rc = check_batch_args(x, queries, nq, n_cand, ids, dists)) return rc;  // n_cand as the PQ call's top_k
    if (nq == 0) return DPQ_OK;
    int rc = grow(r->d_q, &r->q_n, (size_t)nq * r->D1);
    if (!rc) rc = grow(r->d_cand, &r->cand_n, (size_t)nq * n_cand);
    if (!rc) rc = grow(r->d_cdist, &r->cdist_n, (size_t)nq * n_cand);
    if (!rc) rc = refine_grow_outputs(r, (size_t)nq * top_k);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(r->d_q, queries, (size_t)nq * r->D1 * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = query_device(x, filter, r->d_q, nq, n_cand, r->d_cand, r->d_cdist, nullptr))) return rc;
    rc = refine_rerank_on_device("dpq_query_batch_refined", r, r->d_q, nq, r->d_cand, n_cand, top_k, r->d_ids, r->d_dists,
                                 nullptr);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(ids, r->d_ids, (size_t)nq * top_k * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPQ_HIP(hipMemcpy(dists, r->d_dists, (size_t)nq * top_k * sizeof(float), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

// ---- OPQ: rotation, cross-covariance, Procrustes, the training loop (dpq_opq.hip, dpq_procrustes.cpp) ----------------

static int opq_check_dim(const std::string& who, int D) {
    if (D < 1 || D > dpq::kOpqMaxD) return fail(DPQ_ERR_ARG, who + ": D outside 1..1024");
    return DPQ_OK;
}

int dpq_rotate_device(const float* d_vectors, int64_t n, int D, const float* d_R, float* d_out, void* hip_stream) {
    return guarded([&]() -> int {
    const std::string who = "dpq_rotate_device";
    if (!d_vectors || !d_R || !d_out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 0) return fail(DPQ_ERR_ARG, who + ": n < 0");
    if (int rc = opq_check_dim(who, D)) return rc;
    if (d_out == d_vectors) return fail(DPQ_ERR_ARG, who + ": out must not alias vectors");
    if (int rc = flat_device_present(who)) return rc;
    const hipError_t e = dpq::launch_opq_rotate(d_vectors, n, D, d_R, d_out, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(DPQ_ERR_HIP, who + ": " + hipGetErrorString(e));
    return DPQ_OK;
    });
}

int dpq_rotate(const float* vectors, int64_t n, int D, const float* R, int device, float* out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_rotate";
    if (!vectors || !R || !out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 0) return fail(DPQ_ERR_ARG, who + ": n < 0");
    if (int rc = opq_check_dim(who, D)) return rc;
    if (out == vectors) return fail(DPQ_ERR_ARG, who + ": out must not alias vectors");
    if (int rc = train_select_device(device)) return rc;
    if (n == 0) return DPQ_OK;
    const int64_t tile = std::min(n, dpq::kOpqSlice);
    DevBuf<float> d_x, d_r, d_o;
    int rc = d_x.alloc((size_t)tile * D);
    if (!rc) rc = d_o.alloc((size_t)tile * D);
    if (!rc) rc = d_r.alloc((size_t)D * D);
    if (rc) return rc;
    hipError_t e = hipMemcpy(d_r, R, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice);
    for (int64_t base = 0; base < n && e == hipSuccess; base += tile) {
        const int64_t m = std::min(tile, n - base);
        e = hipMemcpy(d_x, vectors + (size_t)base * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = dpq::launch_opq_rotate(d_x, m, D, d_r, d_o, nullptr);
        if (e == hipSuccess) e = hipMemcpy(out + (size_t)base * D, d_o, (size_t)m * D * sizeof(float), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(DPQ_ERR_HIP, who + ": " + hipGetErrorString(e));
    return DPQ_OK;
    });
}

int dpq_cross_covariance(const float* vectors, int64_t n, int D, const uint8_t* codes, const float* codewords, int M, int K,
                         int Ds, int device, double* C_out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_cross_covariance";
    if (!vectors || !codes || !codewords || !C_out) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (n < 1) return fail(DPQ_ERR_ARG, who + ": n < 1");
    if (int rc = opq_check_dim(who, D)) return rc;
    if (M < 1 || M > 256 || K < 1 || K > 256 || Ds < 1) return fail(DPQ_ERR_ARG, who + ": M or K outside 1..256, or Ds < 1");
    if ((int64_t)M * Ds != D) return fail(DPQ_ERR_ARG, who + ": D is not M * Ds");
    if (K < 256)
        for (int64_t i = 0; i < n * M; ++i)
            if (codes[i] >= K) return fail(DPQ_ERR_ARG, who + ": a code byte is >= K");
    if (int rc = train_select_device(device)) return rc;
    const int64_t leaves = (n + dpq::kOpqLeaf - 1) / dpq::kOpqLeaf;
    DevBuf<float> d_x, d_cw;
    DevBuf<uint8_t> d_codes;
    DevBuf<double> d_S, d_C;
    int rc = d_x.alloc((size_t)n * D);
    if (!rc) rc = d_codes.alloc((size_t)n * M);
    if (!rc) rc = d_cw.alloc((size_t)M * K * Ds);
    if (!rc) rc = d_S.alloc((size_t)std::min(leaves, dpq::opq_cross_leaves_per_pass(D)) * D * D);
    if (!rc) rc = d_C.alloc((size_t)D * D);
    if (rc) return rc;
    DPQ_HIP(hipMemcpy(d_x, vectors, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice));
    DPQ_HIP(hipMemcpy(d_codes, codes, (size_t)n * M, hipMemcpyHostToDevice));
    DPQ_HIP(hipMemcpy(d_cw, codewords, (size_t)M * K * Ds * sizeof(float), hipMemcpyHostToDevice));
    DPQ_HIP(dpq::launch_opq_cross(d_x, n, D, d_codes, d_cw, M, K, Ds, d_S, d_C, nullptr));
    DPQ_HIP(hipMemcpy(C_out, d_C, (size_t)D * D * sizeof(double), hipMemcpyDeviceToHost));
    return DPQ_OK;
    });
}

int dpq_procrustes(const double* C, int D, double* R_out, int32_t* degenerate) {
    return guarded([&]() -> int {
    const std::string who = "dpq_procrustes";
    if (!C || !R_out || !degenerate) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = opq_check_dim(who, D)) return rc;
    if (C == R_out) return fail(DPQ_ERR_ARG, who + ": R_out must not alias C");
    int deg = 1;
    dpq::procrustes(C, D, R_out, &deg, nullptr);
    *degenerate = deg;
    return DPQ_OK;
    });
}

int dpq_write_rotation(const char* path, const float* R, int D) {
    return guarded([&]() -> int {
    const std::string who = "dpq_write_rotation";
    if (!path || !R) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = opq_check_dim(who, D)) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    const int32_t d32 = D;
    bool ok = true;
    for (int i = 0; i < D && ok; ++i)
        ok = fwrite(&d32, 4, 1, f) == 1 && fwrite(R + (size_t)i * D, sizeof(float), (size_t)D, f) == (size_t)D;
    if (fclose(f) != 0 || !ok) return fail(DPQ_ERR_IO, std::string("short write on ") + path);
    return DPQ_OK;
    });
}

int dpq_read_rotation(const char* path, int32_t* D, float* out) {
    return guarded([&]() -> int {
    const std::string who = "dpq_read_rotation";
    if (!path || !D) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(DPQ_ERR_IO, std::string("cannot open ") + path);
    int rc = DPQ_OK;
    int32_t d32 = 0;
    if (fread(&d32, 4, 1, f) != 1 || d32 < 1 || d32 > dpq::kOpqMaxD) {
        rc = fail(DPQ_ERR_FORMAT, std::string(path) + ": not a rotation file (first dimension word outside 1..1024)");
    } else {
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        if (size != (long)d32 * (4 + 4 * (long)d32))
            rc = fail(DPQ_ERR_FORMAT, std::string(path) + ": not a square matrix of D rows (file size is not D * (4 + 4 D))");
    }
    if (!rc) {
        *D = d32;
        fseek(f, 0, SEEK_SET);
        std::vector<float> row((size_t)d32);
        for (int i = 0; i < d32 && !rc; ++i) {
            int32_t h = 0;
            if (fread(&h, 4, 1, f) != 1 || fread(row.data(), sizeof(float), (size_t)d32, f) != (size_t)d32)
                rc = fail(DPQ_ERR_IO, std::string("short read on ") + path);
            else if (h != d32)
                rc = fail(DPQ_ERR_FORMAT, std::string(path) + ": a row's dimension word differs from the first");
            else if (out)
                memcpy(out + (size_t)i * d32, row.data(), (size_t)d32 * sizeof(float));
        }
    }
    fclose(f);
    return rc;
    });
}

int dpq_opq_train(const float* vectors, int64_t n, int D, int M, int K, const dpq_opq_opts* opts, float* rotation,
                  float* codewords, dpq_opq_stats* stats) {
    return guarded([&]() -> int {
    const std::string who = "dpq_opq_train";
    const int device = opts ? opts->device : 0, outer = opts ? opts->outer_iters : 8;
    const int init_iters = opts ? opts->init_iters : 25, inner_iters = opts ? opts->inner_iters : 4;
    const int init = opts ? opts->init : 0, restarts = opts ? opts->restarts : 0;
    const uint64_t seed = opts ? opts->seed : 0;
    const bool use_rot = opts && opts->use_initial_rotation;
    if (!vectors || !rotation || !codewords) return fail(DPQ_ERR_ARG, who + ": NULL argument");
    if (int rc = opq_check_dim(who, D)) return rc;
    if (M < 1 || D % M != 0) return fail(DPQ_ERR_ARG, who + ": D is not a multiple of M (pad the vectors and say so)");
    if (outer < 0 || outer > 64) return fail(DPQ_ERR_ARG, who + ": outer_iters outside 0..64");
    if (init_iters < 1 || init_iters > 64) return fail(DPQ_ERR_ARG, who + ": init_iters outside 1..64");
    if (inner_iters < 1 || inner_iters > 64) return fail(DPQ_ERR_ARG, who + ": inner_iters outside 1..64");
    if (init < 0 || init > 1) return fail(DPQ_ERR_ARG, who + ": init outside 0..1");
    if (restarts < 0 || restarts > 16) return fail(DPQ_ERR_ARG, who + ": restarts outside 0..16");
    if (int rc = train_check_shape("dpq_opq_train", n, D, M, K)) return rc;
    if (int rc = train_select_device(device)) return rc;
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    const auto wall0 = clock::now();
    const int Ds = D / M;
    const size_t rot_n = (size_t)D * D, cb_n = (size_t)M * K * Ds;
    dpq_opq_stats st{};
    std::vector<float> R(rot_n, 0.0f), cb(cb_n), xr((size_t)n * D);
    std::vector<double> pot((size_t)M), C(rot_n), R64(rot_n);
    std::vector<uint8_t> codes((size_t)n * M);
    if (use_rot)
        memcpy(R.data(), rotation, rot_n * sizeof(float));
    else
        for (int i = 0; i < D; ++i) R[(size_t)i * D + i] = 1.0f;

    auto add_train = [&](const dpq_train_stats& t) {
        st.gpu_ms += t.gpu_ms;
        st.rounds_ms += t.rounds_ms;
        st.assign_ms += t.assign_ms;
        st.update_ms += t.update_ms;
        st.repair_ms += t.repair_ms;
    };
    auto rotate_now = [&]() -> int {
        const auto t0 = clock::now();
        const int rc = dpq_rotate(vectors, n, D, R.data(), device, xr.data());
        st.rotate_ms += ms_since(t0);
        return rc;
    };
    auto objective_now = [&](double* obj) -> int {
        if (int rc = dpq_train_potential(xr.data(), n, D, cb.data(), M, K, Ds, device, pot.data())) return rc;
        double s = 0.0;
        for (int m = 0; m < M; ++m) s = s + pot[(size_t)m];
        *obj = s;
        return DPQ_OK;
    };
    double best = 0.0;
    auto keep_if_best = [&](int t) {
        if (t == 0 || st.objective[t] < best) {  // strict: a tie stays with the lower t
            best = st.objective[t];
            st.best_t = t;
            memcpy(rotation, R.data(), rot_n * sizeof(float));
            memcpy(codewords, cb.data(), cb_n * sizeof(float));
        }
    };

    // t = 0 (the caller's rotation was copied above: `rotation` is free to collect the best pair from here on)
    if (int rc = rotate_now()) return rc;
    dpq_train_opts to{};
    to.device = device;
    to.max_iters = init_iters;
    to.seed = seed;
    to.init = init;
    to.restarts = restarts;
    dpq_train_stats ts{};
    if (int rc = dpq_train_codebook(xr.data(), n, D, M, K, &to, cb.data(), &ts)) return rc;
    add_train(ts);
    if (int rc = objective_now(&st.objective[0])) return rc;
    keep_if_best(0);

    for (int t = 1; t <= outer; ++t) {
        if (int rc = dpq_encode_pq(xr.data(), n, D, cb.data(), M, K, Ds, device, codes.data())) return rc;
        auto t0 = clock::now();
        if (int rc = dpq_cross_covariance(vectors, n, D, codes.data(), cb.data(), M, K, Ds, device, C.data())) return rc;
        st.cross_ms += ms_since(t0);
        t0 = clock::now();
        int32_t deg = 0;
        if (int rc = dpq_procrustes(C.data(), D, R64.data(), &deg)) return rc;
        if (deg)
            ++st.degenerate;
        else
            for (size_t e = 0; e < rot_n; ++e) R[e] = (float)R64[e];
        st.rotation_residual[t - 1] = dpq::orthogonality_residual(R.data(), D);
        st.procrustes_ms += ms_since(t0);
        if (int rc = rotate_now()) return rc;
        dpq_train_opts ti{};
        ti.device = device;
        ti.max_iters = inner_iters;
        ti.use_initial = 1;
        if (int rc = dpq_train_codebook(xr.data(), n, D, M, K, &ti, cb.data(), &ts)) return rc;
        add_train(ts);
        if (int rc = objective_now(&st.objective[t])) return rc;
        keep_if_best(t);
        st.outer_run = t;
    }
    st.wall_ms = ms_since(wall0);
    if (stats) *stats = st;
    return DPQ_OK;
    });
}

}  // extern "C"
