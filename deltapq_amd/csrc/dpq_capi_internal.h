// dpq_capi_internal.h -- what the C API sources (dpq_capi*.cpp) share: the error slot, the owned device buffer, the
// handle and workspace structs, and the few helpers one feature file borrows from another.  Included by those .cpp
// files only: no .hip file and no kernel header includes it.
#pragma once
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
#include "dpq_candidates.h"
#include "dpq_filter.h"
#include "dpq_flat.h"
#include "dpq_format.h"
#include "dpq_ivf.h"
#include "dpq_kernels.h"
#include "dpq_lookup.h"
#include "dpq_opq.h"
#include "dpq_procrustes.h"
#include "dpq_refine.h"
#include "dpq_tables.h"
#include "dpq_train.h"

// Nothing declared here is part of the library's interface: all of it stays out of the dynamic symbol table.
#pragma GCC visibility push(hidden)

// The calling thread's last error (dpq_last_error); returns `code`.  One slot per thread for the whole library:
// defined in dpq_capi.cpp.
int fail(int code, const std::string& msg);

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

// Raw vectors resident on one GPU (exact search): rows of `format` padded to Dp values (dpq_flat.h: fp32, fp16 / bf16, or
// bytes stored as int8 with an int32 norm per row).  A handle takes the calls whose queries are of
// dpq::flat_query_format(format).
struct dpq_flat {
    int device = 0;
    int64_t n = 0, id_offset = 0;
    int D = 0, Dp = 0;
    int format = dpq::kFlatF32;   // what the open call stored: dpq::kFlatF32 .. kFlatSQ4
    DevBuf<uint8_t> rows;         // [n][Dp] values of `format`; a quantised handle: its quantiser in front of them, (lo, step)
    size_t rows_at = 0;           // [flat_sq_quant_len(Dp)], and the byte at which the rows start
    std::vector<float> sq_lo, sq_step;  // a quantised handle's quantiser [D], as dpq_flat_sq_get returns it
    DevBuf<int32_t> norm8;        // [n rounded up to 4] a byte handle's row norms
    DevBuf<int32_t> rsum8;        // [n rounded up to 4] a u8 handle's row terms of the inner product: made by its first
                                  // inner-product search or range call, kept until dpq_flat_close
    DevBuf<uint32_t> map;         // DFS position -> row (dpq_flat_set_id_map)
    std::vector<uint32_t> h_map;  // its host copy: dpq_flat_rerank checks candidates on the host
    // workspaces, grown on demand and kept until dpq_flat_close
    DevBuf<uint64_t> keys;
    DevBuf<dpq::FlatQueryState> state;
    DevBuf<float> d_q, d_dists;
    DevBuf<int32_t> d_ids, d_cand;
    DevBuf<uint32_t> flag;
    DevBuf<uint8_t> q_raw;        // a byte handle's queries as given, biased (u8) and padded into q8, their norms in qnorm,
    DevBuf<int8_t> q8;            // their terms of the inner product (u8) in qsum
    DevBuf<int32_t> qnorm, qsum;
    size_t keys_n = 0, state_n = 0, q_n = 0, out_n = 0, cand_n = 0, q_raw_n = 0, q8_n = 0, qnorm_n = 0, qsum_n = 0;
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

// An inverted file over one handle's nodes (dpq_ivf_*, dpq_capi_ivf.cpp): the lists in device memory of their own, and
// the workspace every search on it works in -- apart from every search lane's workspace, tables included.
struct dpq_ivf {
    dpq_index* idx = nullptr;       // the handle it was made on; freed before dpq_close
    int device = 0;
    int nlist = 0, M = 0, D = 0;      // D = M * Ds of the centroids (0: none set)
    int64_t n_assigned = 0, n_unassigned = 0, max_list_len = 0;
    std::vector<int64_t> h_offsets; // [nlist + 1] host copy (dpq_ivf_get, dpq_ivf_get_info)
    DevBuf<int64_t> offsets;        // [nlist + 1]
    DevBuf<int32_t> ids;            // [n_assigned] reported ids, ascending inside a list
    DevBuf<uint8_t> codes;          // [n_assigned][M] plain code values in list order
    DevBuf<float> centroids;        // [nlist][D] (launch_flat_search's rows: D is a multiple of 8); NULL: none set
    int64_t device_bytes = 0;       // of the four above
    // workspace, grown on demand and kept until dpq_ivf_free
    DevBuf<float> lut32, lut_min;          // [slice queries][M][256] exact tables, [slice queries][M][4]
    DevBuf<int32_t> probes;                // [slice queries][nprobe] the pre-pass's rows
    DevBuf<int32_t> part_ids, tmp_ids;     // [nprobe][slice queries][top_k] the lists' answers; [slice queries][top_k] a
    DevBuf<float> part_dists, tmp_dists;   // merge round's
    DevBuf<uint32_t> flag;                 // [2] a probe names no list; a table entry is no distance
    DevBuf<uint64_t> keys;                 // coarse step: a batch's key buffers and states
    DevBuf<dpq::FlatQueryState> state;
    DevBuf<float> d_in, d_dists, d_cdists; // host forms: queries, distances; the coarse step's distances
    DevBuf<int32_t> d_probes, d_ids;       // ... probes, ids
    size_t lut_n = 0, min_n = 0, probes_n = 0, part_ids_n = 0, part_dists_n = 0, tmp_ids_n = 0, tmp_dists_n = 0,
           keys_n = 0, state_n = 0, in_n = 0, dists_n = 0, cdists_n = 0, dprobes_n = 0, ids_n = 0;
    // inner product (dpq_ivf_search*_ip): a slice's tables [slice queries][M][K]; gaps and bias where the caller passes none
    DevBuf<float> tab, d_gaps, d_bias;
    size_t tab_n = 0, gaps_n = 0, bias_n = 0;
    // range search (dpq_ivf_range_search*): the radius keys of the call; a slice's counts and their exclusive scan
    // [slice queries][nprobe] + 1; a group's list starts [queries + 1]; the pool of a group's keys, unsorted and sorted
    // (at most dpq::kIvfRangePoolKeys each: a longer single list works in buffers of the call)
    DevBuf<uint64_t> r_thr, r_pool, r_sorted;
    DevBuf<int64_t> r_counts, r_offs, r_qoffs;
    size_t r_thr_n = 0, r_pool_n = 0, r_sorted_n = 0, r_counts_n = 0, r_offs_n = 0, r_qoffs_n = 0;
};

uint64_t next_index_serial();  // dpq_capi.cpp: one counter for the process

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

// The device buffers of the candidate search (dpq_candidate_search* / dpq_candidate_distances*), apart from every search
// lane's workspace, its tables included.  The work buffers hold one slice (at most 2^20 candidates of at most 2048
// queries); the staging buffers of the host forms hold a whole call.
struct CandWs {
    DevBuf<float> lut32;      // [slice queries][M][256] exact tables
    DevBuf<float> lut_min;    // [slice queries][M][4] the table build writes its partial minima unconditionally
    DevBuf<int32_t> local;    // [slice] the candidates with everything that is not a node of this handle as -1
    DevBuf<uint8_t> codes;    // [slice][M] their level-1 codes
    DevBuf<uint64_t> keys;    // [slice queries][cand_keys(n_cand)]
    DevBuf<uint32_t> flag;    // [2] a candidate names no node of the index; a table entry is no distance
    DevBuf<float> d_in, d_dists;    // host forms: queries or tables, and the distances
    DevBuf<int32_t> d_cand, d_ids;  // ... the candidates and the ids
    size_t lut_n = 0, min_n = 0, local_n = 0, codes_n = 0, keys_n = 0, in_n = 0, dists_n = 0, cand_n = 0, ids_n = 0;
};

// Where a batch's exact tables come from: queries against the handle's codebook (lut_build_kernel), or the caller's own
// tables[nq][M][K] (tables_ingest_kernel), which raises *d_bad when an entry is not a distance.
struct TableSource {
    const float* d_queries = nullptr;
    const float* d_tables = nullptr;
    uint32_t* d_bad = nullptr;
    const float* h_tables = nullptr;  // host forms: tables in host memory, staged one sub-batch at a time (d_tab_stage)
};

// The device buffers a batch works in (one per pipeline lane), sized for `slots` padded queries and `cap` candidates each.
struct Workspace {
    int slots = 0, cap = 0;
    DevBuf<float> d_lut32;         // exact tables [query][8][256]
    DevBuf<float> d_lut32r;        // the same, rows by the labels of the plain-code scratch (only with d_relabel)
    DevBuf<float> d_lut_min;       // [query][8] minima (anchor of the filter quantisation)
    DevBuf<float> d_lut_stat;      // [query][8] the 32nd largest entry of every row (M = 8: the split of the filter's saturations)
    DevBuf<uint4> d_qtab;          // [slot groups][128 KB] filter tables of the cascade level being scanned
    DevBuf<uint32_t> d_cand_count;
    DevBuf<uint32_t> d_overflow;   // [slots] overflow flags
    DevBuf<uint32_t> d_tight;      // [slots][kTightWords] tightening counters of the level being scanned (strand1: its
                                   // one slot's kS1HistWords, what one query group's rows hold)
    DevBuf<uint64_t> d_cand_key, d_thr_key;  // candidate keys [slots][cap], threshold keys [slots]
    DevBuf<uint64_t> d_scratch;    // [slots][cap] contiguous copy of a slot's keys when they exceed the select's LDS list
    DevBuf<uint8_t> d_batch_raw;   // tiled plain-code scratch (a shard larger than one tile): the tile being scanned, decoded
                                   // per batch; kept when the rest grows.  A one-tile shard: dpq_index::d_plain_image
    // dpq_debug_filter_tables: the query groups of the last batch's first filter level and how many filter levels have
    // written d_qtab since that batch began (1: the first level's tables are still there)
    int dbg_qtab_groups = 0, dbg_qtab_levels = 0;
    int dbg_qtab_nq = 0;             // > 0: d_dbg_thr holds that batch's thresholds as its first level's tables saw them
    DevBuf<uint64_t> d_dbg_thr;      // [slots] (written only in a process started with DPQ_DEV=1)
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
    CandWs cand;                     // dpq_candidate_search* / dpq_candidate_distances*
    DevBuf<uint32_t> d_vec_id;       // [n_local] local node -> original vector id (dpq_set_vec_ids; the _vec filter constructors)
    bool vec_ids_set = false;
    DevBuf<unsigned long long> d_filter_count;  // [1] the set bits of the filter being built (dpq_filter_create_* on the device)
    // search by tables and inner-product search (dpq_capi_tables.cpp), kept until dpq_close
    uint32_t* h_tables_bad = nullptr;    // pinned + mapped word tables_ingest_kernel raises; d_tables_bad: its device address
    uint32_t* d_tables_bad = nullptr;
    DevBuf<float> d_tab_stage;           // [one sub-batch][M][K] tables of the host forms / of the inner-product forms
    DevBuf<float> d_ip_bias, d_ip_gaps;  // [nq], [nq][top_k] where the caller of an inner-product form passes none
    size_t tab_stage_n = 0, ip_bias_n = 0, ip_gaps_n = 0;
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

// Developer diagnostics (the dpq_debug_* entry points, include/deltapq_amd.h) and developer environment variables are
// live only in a process started with DPQ_DEV=1.
bool dev_mode();  // dpq_capi.cpp
#define DPQ_DEV_ONLY() \
    if (!dev_mode()) return fail(DPQ_ERR_STATE, "developer diagnostics: start the process with DPQ_DEV=1")

template <class T>
int grow(DevBuf<T>& buf, size_t* have, size_t want) {
    if (want <= *have && buf) return DPQ_OK;
    *have = 0;
    int rc = buf.alloc(want);
    if (!rc) *have = want;
    return rc;
}

// Helpers one feature file borrows from another (defined in the file named).
int check_batch_args(dpq_index* x, const float* d_queries, int nq, int top_k, int32_t* d_ids, float* d_dists);  // dpq_capi.cpp
int query_device(dpq_index* x, const dpq_filter* filt, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                 float* d_dists, void* hip_stream);                                                             // dpq_capi.cpp
int check_filter(const dpq_index* x, const dpq_filter* f);                                                      // dpq_capi.cpp
// query_device / dpq_range_search behind their argument checks, for either table source (src's pointers name the first
// query; sub-batches advance them); the caller has finished the pending batches
int query_device_src(dpq_index* x, const dpq_filter* filt, const TableSource& src, int nq, int top_k, int32_t* d_ids,
                     float* d_dists, void* hip_stream);                                                         // dpq_capi.cpp
int range_search_src(dpq_index* x, const TableSource& src, int nq, const float* radii, dpq_range_result** out);  // dpq_capi.cpp
int ensure_out_stage(dpq_index* x, size_t elems);  // d_ids_stage / d_dists_stage                                  dpq_capi.cpp
int splits_for(int n_seg_pass, int n_groups);  // scan workgroups per query group                                dpq_capi.cpp
int flat_device_present(const std::string& who);                                                                // dpq_capi_flat.cpp
bool lookup_id_ok(const dpq_index* x, int64_t id);                                                              // dpq_capi_lookup.cpp
int lookup_on_device(dpq_index* x, const int32_t* d_ids, int64_t n, uint8_t* d_codes, float* d_vecs, hipStream_t stream,
                     const char* who);                                                                          // dpq_capi_lookup.cpp
int opq_check_dim(const std::string& who, int D);                                                               // dpq_capi_train.cpp

#pragma GCC visibility pop
