/* deltapq_amd.h -- C-ABI of the MI355X-native DeltaPQ query engine.
 *
 * This is the drop-in boundary for ONE path of RunhuiWang/DeltaPQ: the
 * delta-tree scan behind `deltapq -task query` / `-task query_im`.  The
 * reference has no FFI layer; its boundary is a C++ free function called once
 * per query (citations are file:line into the reference repository):
 *
 *   void query_processing_scan_compressed_codes_opt_o_direct(
 *       const string& dataset_path, const vector<float>& query, int top_k,
 *       int M, int K, int m_Ds, uint num_codes,
 *       const vector<PQ::Array>& m_codewords,
 *       vector<pair<int,float>>& results, uchar** decoder);
 *                                   deltapq_create_approx_tree.h:2805-2810
 *   void query_processing_scan_compressed_codes_opt_in_memory(
 *       uchar* codes, long long n_bytes, ...same...);
 *                                   deltapq_create_approx_tree.h:3731-3736
 *
 * A C-ABI replacement splits that call into load-once / query-many:
 *
 *   reference                                   this library
 *   ------------------------------------------  ---------------------------------
 *   open()+read() of the DTC file per query     dpq_open_file / dpq_open_memory
 *     (h:2812-2824; main:624-634 for query_im)    (parse, validate, transcode to
 *                                                 SoA, upload to HBM -- once)
 *   m_codewords argument (h:2809)               dpq_set_codebook
 *   one call per query (main:328-339)           dpq_query_batch[_device]
 *   results[top_k] of (int id, float dist),     ids[nq][top_k] int32,
 *     ascending (h:2977-2982)                     dists[nq][top_k] float, ascending
 *   decoder[256] argument (main:312-325)        gone (popcount / byte permute on GPU)
 *   PQ::ReadCodewords (pq.cpp:288-312)          dpq_read_codewords
 *   PQ::Learn (pq.cpp:112-157, cv::kmeans)      dpq_train_codebook (own semantics; k-means++ start and restarts too)
 *   PQ::WriteCodewords (pq.cpp:267-286)         dpq_write_codewords
 *   ReadTopN(query.{fvecs,bvecs})               dpq_read_vecs
 *     (utils.cpp:14-110)
 *   brute force over base.{ext}                 dpq_flat_open[_u8] / dpq_flat_search[_u8] (exact L2,
 *     (main.cpp:107-166, 569-669)                 the reference's bits), dpq_flat_rerank
 *   recall (main.cpp:727-803)                   dpq_recall, dpq_read/write_groundtruth
 *   (none: the reference never reads a code     dpq_get_codes / dpq_reconstruct / dpq_decode_range,
 *     back out of its index)                      dpq_dtc_decode (FAISS's sa_decode / reconstruct_batch)
 *   (none: FAISS's IndexFlat::search with an    dpq_flat_filter_create / dpq_flat_search_filtered[_u8]
 *     IDSelector)
 *   (none: FAISS's IndexFlat::range_search)     dpq_flat_range_search[_u8], dpq_range_recall
 *   (none: FAISS's IndexRefine over two PQ      dpq_refine_build / dpq_refine_rerank / dpq_query_batch_refined
 *     indexes; ADC+R)                             (a second PQ level over the residuals re-ranks a shortlist)
 *   (none: FAISS's METRIC_INNER_PRODUCT over    dpq_query_batch_ip / dpq_ip_tables / dpq_ip_scores
 *     PQ codes)
 *   (none: a caller's own distance tables:      dpq_query_batch_tables / dpq_range_search_tables
 *     weights, masks, residual queries)
 *   (none: FAISS's IndexPQ distance computer    dpq_candidate_search[_device][_tables] / dpq_candidate_distances[_device]
 *     over ids; search with a per-query           (PQ distances and top-k over each query's own id list)
 *     IDSelectorArray)
 *   (none: FAISS's IndexIVFPQ with              dpq_ivf_create[_device] / dpq_ivf_build / dpq_ivf_set_centroids,
 *     by_residual = false: inverted lists,        dpq_ivf_probe / dpq_ivf_search[_device] / dpq_ivf_search_probes[_device]
 *     nprobe)                                     (lists over the index's nodes, probed per query)
 *   (none: FAISS's IndexIVF::train,             dpq_ivf_train / dpq_ivf_assign[_device], dpq_write_vecs
 *     quantizer->assign)                          (the coarse quantiser's centroids, learned and applied on the GPU)
 *   (none: FAISS's IndexFlatIP: search, an      dpq_flat_search_ip / dpq_flat_search_filtered_ip /
 *     IDSelector, range_search; re-ranking by     dpq_flat_range_search_ip / dpq_flat_rerank_ip[_device],
 *     inner product)                              dpq_merge_topk_ip_host
 *   (none: IndexFlatIP over bytes; FAISS's      dpq_flat_*_ip_u8 on a dpq_flat_open_u8 handle; dpq_flat_open_i8 and
 *     ScalarQuantizer QT_8bit_direct_signed)      dpq_flat_*_i8 / dpq_flat_*_ip_i8 (signed int8 rows, both metrics)
 *   (none: FAISS's IndexScalarQuantizer fp16 /  dpq_flat_open_half / dpq_flat_open_narrowed, then every fp32-query
 *     bf16 under IndexFlat's calls, and           dpq_flat_* call; dpq_half_from_float / dpq_half_to_float
 *     IndexRefineFlat over it)
 *   (none: FAISS's IndexScalarQuantizer         dpq_sq_train / dpq_sq_encode / dpq_sq_decode, dpq_flat_open_sq /
 *     QT_8bit / QT_4bit under IndexFlat's         dpq_flat_open_quantised, dpq_flat_sq_get, then every fp32-query
 *     calls, IndexRefine over it)                 dpq_flat_* call
 *   (none: FAISS's IndexBinaryFlat: Hamming     dpq_flat_open_bits / dpq_flat_open_binarised / dpq_bits_from_float,
 *     search, range search, an IDSelector,        dpq_flat_search_bits / dpq_flat_search_filtered_bits /
 *     re-ranking over packed bits)                dpq_flat_range_search_bits / dpq_flat_rerank_bits[_device]
 *
 * Conventions: plain pointers and sizes only; the caller owns every host
 * buffer it passes, the library owns device memory.  Every function returns a
 * dpq_status (0 = OK, negative = error) instead of the reference's
 * print-and-continue (h:2819-2821); dpq_last_error() gives a thread-local
 * detail string.  A handle is bound to one GPU and is safe to use from one
 * thread at a time.  Nothing here falls back to a CPU implementation: without
 * a usable GPU dpq_open_* fails with DPQ_ERR_NO_DEVICE.
 *
 * Result semantics (identical to the reference, see DESIGN.md "Parity"):
 *   - ids are DFS positions in the index (h:2910, 2979), NOT original vector ids;
 *   - distance = fp64 sum of the M fp32 table entries, rounded to fp32, which is
 *     bit-identical to the reference's incremental fp64 stack (h:2889-2907);
 *   - for even N the last DFS node is reported with id N, not N-1 (h:2949, 2970);
 *   - equal-distance results are ordered by ascending id (the reference emits
 *     them in libstdc++ heap order); at the k-th boundary the lowest ids win;
 *   - NaN inputs (codebook or queries) are out of scope; a distance of +inf (an entry or a sum that overflows fp32)
 *     is an ordinary value, ordered by its bit pattern like any other: real ids at +inf precede padding.
 */
#ifndef DELTAPQ_AMD_H
#define DELTAPQ_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPQ_VERSION 100 /* 0.1.0 */

typedef enum dpq_status {
    DPQ_OK = 0,
    DPQ_ERR_ARG = -1,       /* bad argument (NULL, M/K unsupported, top_k < 1, ...) */
    DPQ_ERR_IO = -2,        /* cannot open / short read */
    DPQ_ERR_FORMAT = -3,    /* DTC stream violates the format invariants */
    DPQ_ERR_NO_DEVICE = -4, /* no usable gfx950 GPU / bad device ordinal */
    DPQ_ERR_HIP = -5,       /* HIP runtime error (message in dpq_last_error) */
    DPQ_ERR_NOMEM = -6,
    DPQ_ERR_STATE = -7,     /* e.g. query before dpq_set_codebook */
    DPQ_ERR_TOPK = -8       /* top_k > number of codes (reference: pops an empty heap, h:2977-2981) */
} dpq_status;

typedef struct dpq_index dpq_index; /* opaque: one DTC index (or one shard of it) resident on one GPU */
typedef struct dpq_soa dpq_soa;     /* opaque: host-side transcoded image (no GPU needed) */
typedef struct dpq_tree dpq_tree;   /* opaque: a DeltaTree in DFS layout built from raw PQ codes (host) */

/* Options for dpq_open_*.  Zero-initialise, then set what you need. */
typedef struct dpq_open_opts {
    int32_t device;             /* HIP device ordinal */
    int32_t shard_rank;         /* this handle holds shard `shard_rank` of `shard_count` */
    int32_t shard_count;        /* 0 or 1 = whole index; shards are contiguous DFS-position ranges
                                   cut at segment boundaries and balanced by payload bytes */
    int32_t chunks_per_segment; /* 64-node chunks per independently decodable segment; 0 = default (2) */
    int32_t cand_capacity;      /* candidate keys per query and cascade level, shared out evenly to the scan
                                 * workgroups of the query's group; 0 = auto (16 K keys, >= 256 per workgroup) */
    int32_t num_codes;          /* 0 = the whole index; n > 0 = scan only the first n codes of it, the reference's `-N`
                                 * smaller than the header's n_codes (h:2825-2829 "scan only part of the codes").
                                 * Odd n: exactly the reference's result.  Even n: the reference reads the pair byte of
                                 * node n-1 as a whole-byte depth (>= 16: a stack row out of bounds, undefined); this
                                 * build decodes node n-1 with its real depth and reports it with id n, as the trailing
                                 * rule (h:2949, 2970) does for an index of n codes. */
    int32_t bootstrap;          /* threshold bootstrap (an inverted multi-index over the shard's nodes, 12 B per
                                 * sampled node, that gives every query a tight first threshold): 0 = automatic (on
                                 * from 64 K nodes per shard), 1 = on (from 16 K nodes), -1 = off (the spread-sample
                                 * cascade alone).  Results are identical either way.  dpq_soa_build: > 0 = build the
                                 * multi-index with this sampling stride. */
    int32_t batch_decode;       /* where the delta decode happens.  0 = automatic: a batch of >= 3 query groups (64 queries
                                 * each; 32 at M = 16) decodes every segment ONCE, tile by tile (16 M nodes of a filter
                                 * level's segment list at a time; a shard up to that size is one tile), into a
                                 * plain-code scratch (M bytes per node of a tile, per pipeline lane: at most 128 MB at
                                 * M = 8, cache-resident) that all its groups' filter passes read; smaller batches
                                 * decode inside the scan, once per group.  1 = scratch always, -1 = never,
                                 * n >= 2 = scratch always with tiles of n segments (testing aid).  Results are
                                 * identical either way. */
    int64_t global_offset;      /* the payload is a self-contained PART of a larger index (its first node carries a
                                 * whole code): ids are reported as global_offset + position in this payload */
    int64_t global_n_codes;     /* 0 = this payload is the whole index (global_offset must then be 0); else N of the
                                 * larger index (the even-N id rule h:2949, 2970 then applies to its last node only) */
    /* ---- plan and tiling knobs.  0 = the measured default; results are identical whatever they hold.  They are
     * part of the options (not of the environment) so that the ranks of a multi-GPU launch cannot diverge from
     * each other through their environments.  With DPQ_DEV=1 in the environment -- developer sweeps only -- the
     * variables named in brackets override them, read once per dpq_open_*. ---- */
    int32_t stream_max_queries; /* batches of up to this many queries take the stream kernel (1, 2 or 4 queries per pass over
                                 * the compressed image, exact tables in LDS, no filter tables) instead of the 64-query
                                 * filter scan: 0 = the measured switch-over (4), -1 = never  [DPQ_STREAM_MAX_QUERIES] */
    int32_t coarse_below;       /* batches of up to this many queries use the coarse cascade plan on shards without a
                                 * threshold bootstrap; 0 = 128  [DPQ_COARSE_BELOW] */
    int32_t plan_ratios[3];     /* force the size ratios between consecutive filter levels (each >= 2); 0 = automatic
                                 *   [DPQ_PLAN_RATIOS=a,b,c] */
    int32_t boot_cap;           /* nodes a bootstrap block may hold (2048..16384); 0 = 3072 / 6144 (M = 16) up to
                                 * top-256, then 12288 (M = 8 up to top-640: 6144)  [DPQ_BOOT_CAP] */
    int32_t boot_target;        /* nodes after which the bootstrap stops walking cells; 0 = boot_cap  [DPQ_BOOT_TARGET] */
    int32_t flags;              /* DPQ_OPT_* bits below */
    int64_t batch_tile_nodes;   /* nodes per tile of the per-batch plain-code scratch; 0 = 16 M  [DPQ_BATCH_TILE_NODES] */
} dpq_open_opts;

/* dpq_open_opts.flags (developer A/B switches; every combination gives the same results) */
#define DPQ_OPT_NO_RELABEL 1u       /* plain-code scratch holds code values, not bank-aware labels  [DPQ_RELABEL=0] */
#define DPQ_OPT_NO_FUSE_QUANTISE 2u /* first filter level's tables by quantise_kernel, not by the bootstrap  [DPQ_FUSE_QUANTISE=0] */
#define DPQ_OPT_NO_ASYNC_OVERLAP 4u /* dpq_query_batch_device_async: one workspace, the caller's stream  [DPQ_ASYNC_OVERLAP=0] */
#define DPQ_OPT_BOOT_FULLSORT 8u    /* bootstrap ranks all 256 centroids exactly  [DPQ_BOOT_FULLSORT=1] */
#define DPQ_OPT_NO_TIGHTEN 16u      /* filter scans keep a level's thresholds as they were when it started instead of lowering
                                     * them as candidates accumulate  [DPQ_TIGHTEN=0] */
#define DPQ_OPT_NO_STRANDS 32u      /* no second, lane-per-run layout of the index for batches of up to four queries (they then
                                     * take the wavefront-per-chunk decode; saves ~1.2 x the payload in HBM)  [DPQ_STRANDS=0] */
#define DPQ_OPT_FORCE_STRANDS 64u   /* that layout for every small batch, whatever the shard size (by default from 8 M codes per
                                     * GPU): tests, experiments  [DPQ_STRANDS=2] */
#define DPQ_OPT_NO_STRAND1 128u      /* one query per pass over that layout takes the exact-table kernel (strand_kernel<1>) instead of
                                     * the bound-table kernel with in-kernel tightening (strand1_kernel)  [DPQ_STRAND1=0] */

typedef struct dpq_info {
    int64_t n_codes_total;     /* N of the whole index (header field 0, h:1839-1840) */
    int64_t n_bytes_total;     /* payload bytes of the whole index (header field 1, h:1841) */
    int64_t node_lo, node_hi;  /* DFS positions [lo, hi) held by this handle */
    int64_t algorithmic_bytes; /* DTC payload bytes that encode [lo, hi): the per-query roofline numerator */
    int64_t device_bytes;      /* HBM bytes of the SoA image (nibbles + masks + deltas + tables) */
    int64_t n_diffs;           /* changed bytes in [lo, hi) */
    int32_t M, K, Ds;
    int32_t n_segments;
    int32_t chunks_per_segment;
    int32_t max_depth;
    int32_t device;
    int32_t cand_capacity;
    int64_t bootstrap_bytes;   /* HBM bytes of the threshold-bootstrap multi-index (0 = not in use) */
    int32_t bootstrap_stride;  /* every bootstrap_stride-th node is in it */
    int32_t batch_decode_mb;   /* MB of plain codes one tile holds.  A shard of one tile keeps ONE such image per handle,
                                * decoded once by the first batch that scans it and shared by both pipeline lanes; a
                                * larger shard decodes tile by tile, per batch, into a scratch per pipeline lane.
                                * 0 = this handle always decodes inside the scan */
    int64_t strand_bytes;      /* HBM bytes of the strand image (the stream pass's own layout of the same nodes, resident
                                * beside the SoA image on shards from 8 M codes); 0 = not built */
} dpq_info;

/* Per-kernel device time accumulated since the last dpq_profile_reset, measured
 * with hipEvents recorded on the launch stream (profiling must be enabled). */
typedef struct dpq_profile {
    double lut_ms, scan_ms, select_ms; /* summed over launches */
    int64_t lut_launches, scan_launches, select_launches;
    int64_t scan_node_query_pairs;     /* (code, query) distance evaluations issued by scan launches */
    int64_t scan_stream_bytes;         /* SoA bytes the scan launches had to read at least once */
    int64_t query_batches, queries;
    int64_t overflow_reruns;           /* queries that needed a second final pass (candidate overflow) */
    int64_t exact_checks;              /* (code, query) pairs the filter let through, checked exactly in the scan */
    int64_t candidates;                /* pairs that passed the exact check (counted with dpq_profile_enable(idx, 1) only) */
    double quantise_ms;                /* filter-table builds (one per scan launch; dpq_profile_enable(idx, 1) only) */
    double decode_ms;                  /* per-batch decodes into the plain-code scratch (dpq_profile_enable(idx, 1) only) */
    double bootstrap_ms;               /* threshold bootstrap launches (NOT part of select_ms; dpq_profile_enable(idx, 1) only) */
    int64_t bootstrap_launches;
    /* which kernel the stream pass (batches of up to stream_max_queries) ran, launch by launch (all three are also
     * counted in scan_launches / scan_ms): wavefront per chunk, lane per run with exact tables, lane per run with the
     * one-query bound table */
    int64_t stream_launches, strand_launches, strand1_launches;
} dpq_profile;

typedef struct dpq_dtc_stats {
    int64_t n_codes, n_bytes, n_diffs;
    int64_t depth_hist[16];
    int32_t max_depth;
    int32_t M;
} dpq_dtc_stats;

/* ---- library ---------------------------------------------------------- */
int dpq_version(void);
const char* dpq_strerror(int status);
const char* dpq_last_error(void);
/* Number of usable GPUs (0 if none / no driver).  Never fails. */
int dpq_device_count(void);

/* ---- loaders around the path (host only; a10 in SURVEY.md section 8) ---- */
/* DTC file header: int64 n_codes, int64 n_bytes (h:1839-1841, read at h:2823-2824). */
int dpq_read_dtc_header(const char* path, int64_t* n_codes, int64_t* n_bytes);
/* PQ::ReadCodewords (pq.cpp:288-312).  Call with out == NULL to get the shape. */
int dpq_read_codewords(const char* path, int32_t* M, int32_t* K, int32_t* Ds, float* out);
/* ReadTopN over .fvecs / .bvecs (utils.cpp:14-110).  Call with out == NULL to
 * get the count and dimension; at most `cap` vectors are stored. */
int dpq_read_vecs(const char* path, int is_bvecs, int64_t* n, int32_t* D, float* out, int64_t cap);
/* Reference file name of the index: <dir>/M{M}K{K}_Approx_compressed_codes_opt_N{N} (h:2812-2814). */
int dpq_dtc_file_name(const char* dataset_dir, int M, int K, int64_t N, char* out, int64_t out_len);

/* ---- format (host only) ------------------------------------------------ */
/* Walk a DTC payload, checking every invariant the scan relies on
 * (depth >= 1, depth <= deepest-seen + 1, depth < M, byte count == n_bytes). */
int dpq_dtc_validate(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, dpq_dtc_stats* stats);
/* Transcode (a shard of) a DTC payload into the structure-of-arrays image the
 * GPU scans, on the host.  Used by dpq_open_* and exposed for CPU-only tests. */
int dpq_soa_build(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, const dpq_open_opts* opts,
                  dpq_soa** out);
int dpq_soa_info(const dpq_soa* soa, dpq_info* info);
/* Borrowed pointers into the image (valid until dpq_soa_free):
 * which = 0 depth nibbles, 1 masks, 2 deltas, 3 segment delta offsets (u64[n_seg+1]),
 * 4 segment ancestor checkpoints (u8[n_seg][levels][M]), 5-7 the bootstrap multi-index (cell starts, codes, ids),
 * 8 parent lanes, 9 carry lanes, 10-14 the strand image of the stream pass (checkpoints u64[strips][8][64],
 * mask bytes u32[strips][16][64] (four nodes each), phase offsets u16[strips][16][64], phase starts u32[strips*16+1] in
 * 16-byte units, changed bytes), 15 the strand image's depth nibbles u16[strips][16][64] (four nodes each). */
int dpq_soa_array(const dpq_soa* soa, int which, const void** ptr, int64_t* n_bytes);
void dpq_soa_free(dpq_soa* soa);
/* Serialise a tree given as per-node arrays into the reference DTC payload
 * (qnodes_to_compressed_codes_opt, h:1765-1826).  depths[0] must be 0;
 * masks[i] bit m set <=> position m changes; deltas = changed bytes in node
 * order, ascending position.  Call with out == NULL to get n_bytes. */
int dpq_dtc_encode(const uint8_t* root_code, const uint8_t* depths, const uint16_t* masks, const uint8_t* deltas,
                   int64_t n_codes, int M, uint8_t* out, int64_t* n_bytes);
/* The inverse of dpq_dtc_encode: codes [first, first + count) of a DTC payload in DFS order, codes_out[count][M].
 * Positions, not reported ids: no even-N rule here.  M <= 8 and this build's M = 16 extension.  A stream
 * dpq_dtc_validate refuses: DPQ_ERR_FORMAT; first < 0, count < 0 or first + count > n_codes: DPQ_ERR_ARG; count == 0:
 * DPQ_OK (codes_out may then be NULL). */
int dpq_dtc_decode(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, int64_t first, int64_t count,
                   uint8_t* codes_out);

/* ---- callers either side of the path -------------- */
/* DeltaTree construction, `deltapq -task approx_tree` with -method 1 (create_approx_tree h:970-1065:
 * find_edges_by_diff_approx h:1207-1332, edges_to_tree_index_approx_dfs_layout h:1334-1487).  Host code.
 * codes[n][M] raw PQ codes; codewords [M][K][Ds] may be NULL (it only orders siblings). */
int dpq_tree_build(const uint8_t* codes, int64_t n_codes, int M, int K, int max_height_folds, const float* codewords,
                   int Ds, dpq_tree** out);
/* Same tree, with the edge search (the sort/group passes over all position subsets) on GPU `device`;
 * the result is identical to dpq_tree_build's, node for node. */
int dpq_tree_build_gpu(const uint8_t* codes, int64_t n_codes, int M, int K, int max_height_folds,
                       const float* codewords, int Ds, int device, dpq_tree** out);
int dpq_tree_stats(const dpq_tree* t, dpq_dtc_stats* stats);
/* Borrowed arrays: which = 0 vec_id u32[n] (DFS position -> original id, QNode.vec_id h:80), 1 parent_pos u32[n],
 * 2 depth u8[n], 3 mask u16[n], 4 changed bytes, 5 root code u8[M], 6 edges (parent id, child id) u32[n-1][2]. */
int dpq_tree_array(const dpq_tree* t, int which, const void** ptr, int64_t* n_bytes);
/* DTC payload of the tree (qnodes_to_compressed_codes_opt h:1765-1826); out == NULL returns the size. */
int dpq_tree_encode(const dpq_tree* t, uint8_t* out, int64_t* n_bytes);
/* Writes the reference's three artefacts into dataset_dir: M{M}K{K}H{h}_Approx_Edges_N{N} (h:1326-1327),
 * M{M}K{K}_Approx_TreeNodesDFS_N{N} (60-byte QNode records h:1484; M <= 8), the DTC index (h:1839-1842). */
int dpq_tree_write_files(const dpq_tree* t, const char* dataset_dir);
void dpq_tree_free(dpq_tree* t);
/* DFS position -> original vector id from a TreeNodesDFS file (QNode.vec_id, h:80, h:1166). */
int dpq_read_qnode_ids(const char* path, int64_t n_codes, uint32_t* vec_ids);
/* codes.bin.plain.M{M}K{K}N{N}: PQTree::Read / Write (pq_tree.cpp:1011-1081).  out == NULL returns n_codes. */
int dpq_read_codes_plain(const char* path, int M, int64_t* n_codes, uint8_t* out);
int dpq_write_codes_plain(const char* path, const uint8_t* codes, int64_t n_codes, int M);
/* The other record layouts PQTree::Read knows (pq_tree.cpp:1050-1078): K > 256 stores two bytes per position
 * (little-endian uint16), `with_id` (flag approx_with_id, main:64) appends a 4-byte int id to every M-byte code.
 * codes_out: n * M * (K > 256 ? 2 : 1) bytes; ids_out: n int32 (with_id only); either may be NULL (first call:
 * both NULL to learn n).  K > 256 together with with_id is refused, as in the reference (pq_tree.cpp:1051-1054).
 * The scan engine itself indexes one byte per position (K <= 256), like the DTC format. */
int dpq_read_codes_plain_ex(const char* path, int M, int K, int with_id, int64_t* n_codes, uint8_t* codes_out,
                            int32_t* ids_out);
/* PQ encoding on the GPU: nearest centroid per sub-space in fp32, first minimum wins
 * (PQTree::EncodePlain pq_tree.cpp:215-237; host buffers in/out). */
int dpq_encode_pq(const float* vectors, int64_t n, int D, const float* codewords, int M, int K, int Ds, int device,
                  uint8_t* codes_out);

/* ---- codebook learning -----------------------------------------------------
 * Replaces PQ::Learn (pq.cpp:112-157): Lloyd's k-means per sub-space on the GPU, output float [M][K][Ds] with
 * Ds = ceil(D / M), the layout dpq_set_codebook and dpq_encode_pq take.  NO REFERENCE SEMANTICS (cv::kmeans): the
 * reference calls cv::kmeans with KMEANS_PP_CENTERS and three random restarts after a parallel random shuffle
 * (main.cpp:262), which cannot be reproduced; the rules below are this build's own, restated on the CPU in
 * tests/_kmeans_restatement.py and met by the GPU bit for bit.  Each sub-space is trained on its own; short vectors
 * are zero padded as dpq_encode_pq pads them (pq.cpp:114-123).
 *   Start   use_initial != 0: the caller's codewords.  Otherwise, init == 0: K rows drawn without replacement on the
 *           host, the same rows for every sub-space: p = 0 .. n-1, s = seed; for i = 0 .. K-1: s += 0x9E3779B97F4A7C15,
 *           z = s, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^= z >> 31
 *           (splitmix64, mod 2^64), j = i + z % (n - i), swap p[i], p[j]; codeword i = vector p[i].
 *           init == 1: k-means++ on the GPU, every sub-space m on its own (what dpq_kmeanspp_seed returns).  RNG state
 *           s = seed + m * 0xD6E8FEB86659FD93 (mod 2^64); next(): s += 0x9E3779B97F4A7C15, then the finaliser above
 *           gives z.  Centre 0 is sub-vector next() % n, and w_i is the Assign distance of sub-vector i to it.  Then for
 *           j = 1 .. K-1, with z = next():
 *             leaves   a leaf is 256 consecutive vectors (the last may be short); S_l is the fp64 sum, from +0.0, of
 *                      (double)w_i in ascending i, one add after the other; T_0 = S_0, T_l = T_{l-1} + S_l, one fp64
 *                      add after the other; total is the last T.
 *             total == 0   the smallest index that is not yet a centre of this sub-space is chosen.
 *             otherwise    u = (double)(z >> 11) * 2^-53, r = u * total (one fp64 multiply); the leaf is the first l
 *                      with T_l > r, or, if there is none, the last l with S_l > 0; r' = r - (l ? T_{l-1} : 0.0); walk
 *                      the leaf in ascending i with t = +0.0, t += (double)w_i: the first i with t > r' is chosen,
 *                      or, if there is none, the leaf's last i with w_i > 0.
 *             update   centre j is sub-vector i; then every w_i = (d < w_i ? d : w_i), d the Assign distance to it.
 *   Potential  of a sub-space for given weights: `total` by the leaf rule above.  The seeding's potential is that of
 *           its final w; a codebook's (dpq_train_potential) that of the winning distances of one Assign.
 *   Restarts  restarts R > 1: run r = 0 .. R-1 is a complete, independent run (start and rounds) with seed + r
 *           (mod 2^64).  Every sub-space on its own keeps the run whose FINAL codebook has the lowest potential, a
 *           tie going to the lowest r.  Stats: the millisecond fields and `reseeded` sum over the runs, iters_run is
 *           the largest, converged is 1 only if every run converged, distortion[] is run 0's trace.
 *   Assign  dpq_encode_pq's arithmetic: per codeword `diff = v - c; dist += diff * diff` in fp32, subtract, multiply
 *           and add rounded separately, dimensions in order, strict `<` (the lowest k wins a tie).  The labels of a
 *           round are dpq_encode_pq(vectors, the codebook entering that round): the search starts at FLT_MAX, so the
 *           label is 0 when no distance is below FLT_MAX.  The winning distance is the computed distance to the
 *           reported label, never the FLT_MAX the search starts from: it is +inf when every distance overflows (and
 *           the potential, the distortion and the restart comparison are +inf with it: runs that tie there keep the
 *           lowest r).  NaN inputs are unspecified.
 *   Stop    a sub-space stops right after an assignment (not the first) that changes no label and leaves no cluster
 *           empty: its codebook already is the mean of those labels.  It is not touched again.  Otherwise after
 *           max_iters rounds.
 *   Update  cluster with members: per dimension the fp64 sum, starting from +0.0, of the members' fp32 values in
 *           ascending vector index, one add after the other, divided in fp64 by (double)count, rounded once to fp32.
 *   Empty   with E empty clusters after an assignment, the sub-space's vectors are ranked by (winning distance
 *           descending, vector index ascending); the j-th empty cluster in ascending k takes the j-th ranked vector's
 *           sub-vector.  The donor stays in its old cluster's mean of this round.
 *   Distortion  per round the fp64 sum over vectors and sub-spaces of the winning fp32 distances (a stopped
 *           sub-space contributes its last assignment's); the order of that sum is not part of the contract.
 * The same input gives the same bytes, run to run.  opts == NULL: device 0, 25 rounds, seed 0.  DPQ_ERR_ARG, before
 * any device call: a NULL pointer, D < 1, M < 1 or > 256, K outside 2..256, K > n, n * M >= 2^31, max_iters
 * outside 1..64, init outside 0..1, restarts outside 0..16, init == 1 together with use_initial != 0, a sub-space
 * whose codewords need more than 160 KB of LDS (Ds > 160, or 4 * K * W + 1072 > 163840 bytes with W = Ds rounded up to
 * 4, 8, 12, 16, 24, 32, 64, 96, 128 or 160: K <= 254 at Ds 129..160, every K at Ds <= 128).
 * Without a GPU: DPQ_ERR_NO_DEVICE.  Device memory: about 4 * n * M * (Ds rounded up to 4..160) + 16 * n * M bytes. */
typedef struct dpq_train_opts {
    int32_t device;
    int32_t max_iters;   /* 1..64 */
    uint64_t seed;       /* of the seeded start */
    int32_t use_initial; /* != 0: `codewords` holds the start on entry */
    int32_t init;        /* the start without use_initial: 0 random rows, 1 k-means++ */
    int32_t restarts;    /* 0..16 runs, the best per sub-space kept; 0 and 1: one run */
    int32_t reserved[1]; /* 0 */
} dpq_train_opts;

typedef struct dpq_train_stats {
    int32_t iters_run;     /* rounds run = entries of distortion[] */
    int32_t converged;     /* 1: every sub-space stopped by the rule */
    int64_t reseeded;      /* empty clusters repaired, all rounds and sub-spaces */
    double distortion[64]; /* per round */
    double gpu_ms;         /* assign_ms + update_ms + repair_ms (device events) */
    double wall_ms;        /* the whole call, upload included */
    double rounds_ms;      /* host clock around the rounds; minus gpu_ms = the host round trips */
    double assign_ms, update_ms, repair_ms; /* update_ms: label sort + means */
} dpq_train_stats;

/* codewords: float [M][K][Ds], in (use_initial) and out.  stats may be NULL. */
int dpq_train_codebook(const float* vectors, int64_t n, int D, int M, int K, const dpq_train_opts* opts, float* codewords,
                       dpq_train_stats* stats);
/* The k-means++ start alone (Start, init == 1): codewords_out float [M][K][Ds], Ds = ceil(D / M); potential_out
 * double [M], the potential of the final weights, may be NULL.  dpq_train_codebook with init = 1 equals
 * dpq_train_codebook with use_initial = 1 on this output, byte for byte.  Argument checks as dpq_train_codebook's. */
int dpq_kmeanspp_seed(const float* vectors, int64_t n, int D, int M, int K, uint64_t seed, int device, float* codewords_out,
                      double* potential_out);
/* The leaf-ordered potential (Potential above) of any codebook [M][K][Ds], Ds = ceil(D / M): potential_out double [M].
 * The restart rule compares runs by it; the same inputs give the same bits.  Argument checks as dpq_train_codebook's. */
int dpq_train_potential(const float* vectors, int64_t n, int D, const float* codewords, int M, int K, int Ds, int device,
                        double* potential_out);
/* PQ::WriteCodewords' text format (pq.cpp:267-286) with nine significant digits, so that dpq_read_codewords and the
 * reference's `ifs >> float` (pq.cpp:288-312) read back the same bits; the reference's own default precision (six
 * digits) loses them. */
int dpq_write_codewords(const char* path, const float* codewords, int M, int K, int Ds);

/* Plain (uncompressed) PQ index for the comparator scan `-task pqscan` (h:2590-2678): raw codes[n][M],
 * distance accumulated in **fp32** in ascending m (h:2658-2662), ids = positions in the code file (no
 * even-N quirk).  The handle is used with dpq_set_codebook / dpq_query_batch* like a DTC index. */
int dpq_open_plain_memory(const uint8_t* codes, int64_t n_codes, int M, int K, const dpq_open_opts* opts,
                          dpq_index** out);
/* <path> = codes.bin.plain.M{M}K{K}N{N} (pq_tree.cpp:1011-1031). */
int dpq_open_plain_file(const char* path, int M, int K, const dpq_open_opts* opts, dpq_index** out);

/* ---- index lifetime (GPU) ---------------------------------------------- */
/* Replaces the per-query open()/read() of h:2812-2824: loads
 * <path> = int64 n_codes, int64 n_bytes, payload. */
int dpq_open_file(const char* path, int M, int K, const dpq_open_opts* opts, dpq_index** out);
/* In-memory twin (h:3731-3733: `uchar* codes, long long n_bytes`). */
int dpq_open_memory(const uint8_t* payload, int64_t n_bytes, int64_t n_codes, int M, int K,
                    const dpq_open_opts* opts, dpq_index** out);
/* m_codewords[M][K][Ds] (h:2809), row-major fp32, copied to the GPU. */
int dpq_set_codebook(dpq_index* idx, const float* codewords, int Ds);
int dpq_get_info(const dpq_index* idx, dpq_info* info);
int dpq_close(dpq_index* idx);

/* ---- the hot path ------------------------------------------------------- */
/* Answer nq queries (host buffers; synchronous).  queries[nq][M*Ds];
 * ids[nq][top_k], dists[nq][top_k] ascending by (distance, id).  With
 * shard_count > 1 the lists are this shard's partial top-k with GLOBAL DFS
 * positions; rows are padded with id -1 / +inf when the shard holds fewer than
 * top_k codes. */
int dpq_query_batch(dpq_index* idx, const float* queries, int nq, int top_k, int32_t* ids, float* dists);
/* Same with device pointers, enqueued on `hip_stream` (a hipStream_t, NULL =
 * default stream), asynchronous with respect to the host except for one
 * overflow check at the end of the batch. */
int dpq_query_batch_device(dpq_index* idx, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                           float* d_dists, void* hip_stream);
/* Pipelined variant: enqueues the batch and returns at once.  The batch starts once `hip_stream` has reached the
 * point of this call (an event is recorded on it) and runs on one of two internal streams with its own workspace,
 * alternately, so that consecutive batches overlap (a batch's table build runs under the previous batch's scan).
 * Inputs and outputs belong to the library until dpq_finish(idx): they must stay valid, the inputs must not be
 * changed and the outputs not read before it returns.  dpq_finish waits for every enqueued batch and answers again,
 * synchronously, any batch in which a query overflowed its candidate buffers.  A call with a different
 * `hip_stream` first finishes what is in flight; up to 63 batches may be in flight, the 64th call finishes the
 * earlier ones first.  The synchronous entry points finish pending batches before they start.
 * (dpq_open_opts.flags & DPQ_OPT_NO_ASYNC_OVERLAP: every batch on `hip_stream` itself, one workspace.) */
int dpq_query_batch_device_async(dpq_index* idx, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                                 float* d_dists, void* hip_stream);
int dpq_finish(dpq_index* idx);
/* The same pipeline with HOST buffers in and out -- the reference's interface (h:2805-2810: host query, host results),
 * its per-query loop (main:328-339) turned into batches in flight: the queries of batch i + 1 go up and the results of
 * batch i - 1 come down beside batch i's kernels.  Up to sixteen batches in flight (a seventeenth call
 * settles the earlier ones first); `queries`, `ids` and `dists` belong to the library until dpq_finish(idx) returns.  Page-locked
 * buffers (dpq_pin_host / dpq_unpin_host = hipHostRegister, for callers that do not link the HIP runtime) make it a
 * pipeline: the queries go up on a copy stream and the result lists are written by the select kernel straight into the
 * mapped buffers; pageable memory works through staging copies, without the overlap. */
int dpq_query_batch_host_async(dpq_index* idx, const float* queries, int nq, int top_k, int32_t* ids, float* dists);
int dpq_pin_host(void* ptr, int64_t bytes);
int dpq_unpin_host(void* ptr);
/* ---- range search ---------------------------------------------------------
 * Every code within a radius of each query (FAISS's range_search).  For query q the list holds every code whose
 * distance d is STRICTLY below radii[q] (d < r, FAISS's L2 convention), d being exactly the distance dpq_query_batch
 * reports, to the bit (the DTC fp64-sum rule; fp32 accumulation on a dpq_open_plain_* index).  Ids follow the top-k
 * rules: DFS positions, global on shards and parts, the even-N id of the last node.  Within a list the entries are
 * ascending by (distance, id).  A radius <= 0 gives an empty list, +inf every code of the handle; a NaN radius is
 * DPQ_ERR_ARG.  With shard_count > 1 the lists are this shard's part of the answer (dpq_range_search on each shard,
 * then concatenate per query and sort by (distance, id): deltapq_amd.dist.merge_range_host).
 * The length of a list depends on the data, so the library owns the answer (host memory) until
 * dpq_range_result_free.  Synchronous; pending asynchronous batches are finished first.  The plan, workspaces and
 * results of later top-k calls are not affected.  Device memory: the call grows the active lane's table buffers like
 * a top-k batch of its size and keeps buffers of its own for the next call, at most 320 MB of candidate keys (a
 * 2048-query sub-batch's regions take 268 MB at the default cand_capacity) and 128 MB of output lists, until dpq_close; larger
 * buffers a call needed (long lists, reruns of overflowed lists) are released before it returns. */
typedef struct dpq_range_result dpq_range_result;
/* queries[nq][M*Ds], radii[nq]: host memory. */
int dpq_range_search(dpq_index* idx, const float* queries, int nq, const float* radii, dpq_range_result** out);
/* Borrowed pointers, valid until dpq_range_result_free: lims[nq + 1] (lims[0] = 0), ids / dists [lims[nq]];
 * query q owns entries [lims[q], lims[q + 1]). */
int dpq_range_result_get(const dpq_range_result* r, int32_t* nq, const int64_t** lims, const int32_t** ids,
                         const float** dists);
void dpq_range_result_free(dpq_range_result* r);  /* NULL: nothing happens */

/* ---- filtered top-k search ------------------------------------------------
 * The k nearest codes among those an id bitmap allows (FAISS's IDSelector).  A filter is a bitmap over REPORTED ids:
 * bit i is bit (i & 31) of words[i >> 5] (little-endian within a uint32_t), n_bits bits.  A code is eligible iff its
 * reported id r -- exactly the id dpq_query_batch would report for it: global DFS positions on shards and parts
 * (global_offset), position = id on a plain index, and the even-N rule (the last node of an even-N DTC index is
 * reported as N, so bit N governs it and bit N - 1 governs nothing; N = num_codes under the same rule) -- satisfies
 * r < n_bits and bit r is set.
 * The result is the unfiltered algorithm applied to the eligible codes only: per query top_k entries ascending by
 * (distance, id), distances bit-identical to what dpq_query_batch reports for the same code, rows padded with id -1 /
 * +inf when fewer than top_k codes of the handle are eligible (none at all: an all-padding result, not an error).  One
 * filter applies to every query of a call.  With shard_count > 1 each shard's result is its partial filtered top-k:
 * dpq_merge_topk_* (deltapq_amd.dist) merge them unchanged, every rank building its filter from the same global bitmap.
 * The calls are synchronous; pending asynchronous batches are finished first; the asynchronous, ordered and
 * host-async pipelines have no filtered form.  A NULL filter or one made on another handle is DPQ_ERR_ARG.  Plans,
 * workspaces and results of later unfiltered calls are not affected.  Device memory: the filter holds n_local / 8 bytes
 * (rounded up to whole segments) plus, on handles without a bootstrap, a 15 KB copy of the level-0 id list. */
typedef struct dpq_filter dpq_filter;
/* words[(n_bits + 31) / 32], host memory, read during the call only.  Uploads to the index's device the part of the
 * bitmap this handle can report (its [node_lo, node_hi) range, even-N rule applied), once.  n_bits >= 0. */
int dpq_filter_create(dpq_index* idx, const uint32_t* words, int64_t n_bits, dpq_filter** out);
void dpq_filter_free(dpq_filter* f);   /* NULL: nothing happens */
/* Nodes of its handle the filter allows. */
int dpq_filter_count(const dpq_filter* f, int64_t* n_allowed);
/* Host buffers, synchronous (the contract of dpq_query_batch). */
int dpq_query_batch_filtered(dpq_index* idx, const dpq_filter* f, const float* queries, int nq, int top_k,
                             int32_t* ids, float* dists);
/* Device buffers on hip_stream (the contract of dpq_query_batch_device). */
int dpq_query_batch_device_filtered(dpq_index* idx, const dpq_filter* f, const float* d_queries, int nq, int top_k,
                                    int32_t* d_ids, float* d_dists, void* hip_stream);

/* ---- filter construction on the device ------------------------------------------
 * Every other way of making a dpq_filter, with the work in HIP kernels on the handle's GPU (dpq_filter.hip) instead of
 * dpq_filter_create's host pass: from a bitmap over reported ids that already lives on the GPU, from an id list (allow-
 * or deny-list), from an id range, from a bitmap over ORIGINAL vector ids through a resident position -> vector-id map,
 * and from other filters (AND / OR / AND-NOT / XOR / NOT); plus the read-back of a filter and two packing helpers.
 * Same result: a filter from any constructor is indistinguishable from the one dpq_filter_create makes from the
 * equivalent host bitmap -- the same bits, the same dpq_filter_count, the same owner check; it serves both filtered query
 * calls on shards, parts, prefixes, plain handles and at M = 16.  Ids are REPORTED ids under the rules of the section
 * above (global positions, the even-N rule: id N names the last node of an even-N DTC index and N - 1 names nothing).
 * An id or bit that names no node of THIS handle is skipped, never an error: every shard builds from the same global
 * list.  A negative id is padding.  Duplicates are harmless.
 * Synchronous: a constructor enqueues its kernels on hip_stream (NULL = the default stream; the host forms use the
 * default stream) and returns once the count of allowed nodes has been read back -- that one small read-back is the
 * call's only host round trip (the convention of dpq_get_codes_device).  On return the filter is complete and usable on
 * any stream.  Inputs must be complete on hip_stream's order; pending asynchronous batches are finished first.
 * Arguments are checked before any device call; DPQ_ERR_ARG: NULL out (*out is cleared wherever out is given), NULL
 * index, n_bits < 0, n < 0, a NULL pointer with a non-zero size, lo > hi, an unknown op, b given with DPQ_FILTER_NOT or
 * missing otherwise, a filter of another handle, dpq_set_vec_ids with n != node_hi - node_lo.  n == 0 and n_bits == 0
 * are legal and give empty filters (full ones with invert).  A _vec constructor before dpq_set_vec_ids: DPQ_ERR_STATE.
 * Device memory: a filter costs what dpq_filter_create's costs; the vector-id map 4 bytes per node of the handle until
 * dpq_close; the host forms' temporary uploads are freed before they return. */
#define DPQ_FILTER_AND 0     /* a & b */
#define DPQ_FILTER_OR 1      /* a | b */
#define DPQ_FILTER_ANDNOT 2  /* a & ~b */
#define DPQ_FILTER_XOR 3     /* a ^ b */
#define DPQ_FILTER_NOT 4     /* every node of the handle a does not allow; b must be NULL */
/* d_words[(n_bits + 31) / 32]: a bitmap over reported ids on the handle's GPU (dpq_filter_create's, without the upload). */
int dpq_filter_create_device(dpq_index* idx, const uint32_t* d_words, int64_t n_bits, void* hip_stream, dpq_filter** out);
/* An id list: invert == 0 allows exactly the listed ids, != 0 every node of the handle except them.  ids[n]: host. */
int dpq_filter_create_ids(dpq_index* idx, const int32_t* ids, int64_t n, int invert, dpq_filter** out);
int dpq_filter_create_ids_device(dpq_index* idx, const int32_t* d_ids, int64_t n, int invert, void* hip_stream,
                                 dpq_filter** out);
/* Reported ids in [lo, hi). */
int dpq_filter_create_range(dpq_index* idx, int64_t lo, int64_t hi, dpq_filter** out);
/* vec_id[n], host: the original vector id of local node l (position node_lo + l), n == node_hi - node_lo -- the handle's
 * slice of dpq_tree_array(.., 0) / dpq_read_qnode_ids.  Uploaded once and kept until dpq_close or the next call.  Only the
 * _vec constructors use it: searches keep reporting DFS positions. */
int dpq_set_vec_ids(dpq_index* idx, const uint32_t* vec_id, int64_t n);
/* A bitmap over ORIGINAL vector ids: node l is allowed iff vec_id[l] < n_bits and bit vec_id[l] is set -- what
 * dpq_bitmap_to_dfs followed by dpq_filter_create gives, without the host pass.  words: host; d_words: the handle's GPU. */
int dpq_filter_create_vec(dpq_index* idx, const uint32_t* words, int64_t n_bits, dpq_filter** out);
int dpq_filter_create_vec_device(dpq_index* idx, const uint32_t* d_words, int64_t n_bits, void* hip_stream, dpq_filter** out);
/* op: DPQ_FILTER_*; a and b filters of idx.  The operands are left as they are. */
int dpq_filter_combine(dpq_index* idx, int op, const dpq_filter* a, const dpq_filter* b, dpq_filter** out);
/* The filter back as a bitmap over reported ids: bit r = 1 iff the filter allows the node its handle reports as r; bits
 * that name no node of the handle are 0.  words_out[(n_bits + 31) / 32]: host.  Works after dpq_close of the handle. */
int dpq_filter_to_bitmap(const dpq_filter* f, uint32_t* words_out, int64_t n_bits);
/* Helpers for any id space: a device bitmap of (n_bits + 31) / 32 words from a device byte mask (d_mask[n], non-zero =
 * set, n_bits = n, the tail word zero-padded) or a device id list (cleared first; ids outside [0, n_bits) are skipped).
 * Enqueued on hip_stream of GPU `device` and NOT waited for: a constructor called on the same stream sees the result. */
int dpq_bitmap_from_mask_device(const uint8_t* d_mask, int64_t n, uint32_t* d_words_out, int device, void* hip_stream);
int dpq_bitmap_from_ids_device(const int32_t* d_ids, int64_t n, int64_t n_bits, uint32_t* d_words_out, int device,
                               void* hip_stream);

/* ---- code lookup ------------------------------------------------------------
 * The codes an opened index holds, or their codebook vectors, for any reported ids (FAISS's sa_decode / reconstruct /
 * reconstruct_batch), decoded on the GPU from the very image the searches scan.  Every segment is decodable on its own
 * from its checkpoint, so a request costs the decode of at most one segment, not a walk from the root.
 * Ids: an id names a node exactly as a search result does -- global DFS positions on shards (shard_rank / shard_count)
 * and parts (global_offset), position = id on a dpq_open_plain_* index, and the even-N rule: the last node of an even-N
 * DTC index is named by N and N - 1 names nothing (N = num_codes under the same rule when a prefix is opened).
 * dpq_decode_range counts POSITIONS [first, first + count) inside the handle's [node_lo, node_hi), without the even-N
 * renaming: row i of codes_out is position first + i.
 * A non-negative id that names no node OF THIS HANDLE -- outside [node_lo, node_hi), beyond the opened prefix, the N - 1
 * hole -- is DPQ_ERR_ARG: the host variants check on the host before any device work; the device variants raise one flag
 * word that is read back at the end of the call, and their outputs are then unspecified.  Gathering across shards is
 * the caller's business (split the ids by dpq_info.node_lo / node_hi).  A NEGATIVE id is padding, so a padded top-k row
 * can be passed straight in: its code row is M zero bytes, its reconstructed row M * Ds quiet NaNs (0x7FC00000).  The
 * same id given twice yields two equal rows; the order of `ids` is kept.  n == 0 is DPQ_OK.
 * Reconstructed vectors: vectors_out[i][m * Ds + d] = codewords[m][code[m]][d], the very floats dpq_set_codebook
 * received, in the layout of queries[nq][M * Ds]; a code byte >= K has no codeword and gives Ds quiet NaNs.  Without a
 * codebook dpq_reconstruct* is DPQ_ERR_STATE; dpq_get_codes* and dpq_decode_range need none.
 * The calls are synchronous (the device variants return once the flag word is back, with the rows complete); pending
 * asynchronous batches are finished first.  Plans, workspaces and results of later searches are not affected.  Large n
 * is processed in slices of 1 Mi ids (2^20; reconstructed rows to the host: at most 64 MB of them per slice).
 * n == 0 needs no buffers (NULL is accepted); otherwise a NULL pointer is DPQ_ERR_ARG.
 * A call (or slice) of 16 or more ids per segment of a DTC handle whose decoded codes fit 256 MB takes the grouped path:
 * every segment is decoded once into a scratch image and all its requests are served from it (same results).
 * Device memory, kept until dpq_close: the host variants' staging of one slice (4 MB of ids, M MB of codes, 64 MB of
 * rows) and a scratch of up to one 4 Mi-node tile of decoded codes (M * 4 MB) shared by dpq_decode_range and the grouped
 * path; the device variants keep the flag word and that scratch only.  A grouped call on a larger handle allocates its
 * image (at most 256 MB) and releases it before it returns. */
/* ids[n]: reported ids, exactly what dpq_query_batch reports.  Host buffers. */
int dpq_get_codes(dpq_index* idx, const int32_t* ids, int64_t n, uint8_t* codes_out /* [n][M] */);
/* Device buffers on the handle's GPU, enqueued on hip_stream (NULL = default stream). */
int dpq_get_codes_device(dpq_index* idx, const int32_t* d_ids, int64_t n, uint8_t* d_codes, void* hip_stream);
int dpq_reconstruct(dpq_index* idx, const int32_t* ids, int64_t n, float* vectors_out /* [n][M*Ds] */);
int dpq_reconstruct_device(dpq_index* idx, const int32_t* d_ids, int64_t n, float* d_vectors, void* hip_stream);
/* The handle's codes for positions [first, first + count) in DFS order: the bulk path, host out. */
int dpq_decode_range(dpq_index* idx, int64_t first, int64_t count, uint8_t* codes_out /* [count][M] */);

/* Merge n_lists partial top-k lists per query (lists[l][nq][top_k]) into the
 * final top_k by (distance, id).  Host version for the single-process
 * multi-GPU CLI, device version for use after an RCCL all-gather.
 * Contract, the same for all three calls unless said otherwise:
 *  - A row with id < 0 is padding, whatever its id and distance.  The answer holds the top_k smallest valid rows by
 *    (distance bit pattern as uint32, id), then rows of id -1 / +inf.  A valid row of distance +inf precedes them.
 *  - Each list must be ascending by (distance bits, id) with its padding rows last -- what every query call of this
 *    library delivers.  An unsorted list is a precondition violation for the two device calls (the answer is then
 *    unspecified, within the output's bounds); the host call sorts and tolerates it.
 *  - Repeated keys are kept, not merged away: a (distance, id) row that occurs in two lists (a prefix handle and the
 *    whole index, a rank gathered twice, replica answers) or twice in one list occurs as often in the answer, as far
 *    as top_k reaches.  Host and device calls answer alike, to the bit.
 *  - DPQ_ERR_ARG before any device call: a NULL pointer, n_lists < 1, top_k < 1, nq < 0; for the device calls also
 *    n_lists * top_k > 16384 (a query's keys are merged in 128 KB of LDS).  nq == 0: DPQ_OK, nothing is touched. */
int dpq_merge_topk_host(const int32_t* ids, const float* dists, int n_lists, int nq, int top_k, int32_t* out_ids,
                        float* out_dists);
int dpq_merge_topk_device(const int32_t* d_ids, const float* d_dists, int n_lists, int nq, int top_k,
                          int32_t* d_out_ids, float* d_out_dists, int device, void* hip_stream);
/* The same on the tensor the one all-gather of the path delivers: d_packed[n_lists][nq][2 * top_k] int32, a row =
 * top_k ids followed by the bit patterns of the top_k fp32 distances (what every rank contributes in ONE collective). */
int dpq_merge_topk_device_packed(const int32_t* d_packed, int n_lists, int nq, int top_k, int32_t* d_out_ids,
                                 float* d_out_dists, int device, void* hip_stream);

/* Stream-ordered variant for callers that consume the result ON THE DEVICE, in stream order (the sharded driver:
 * select -> pack -> all-gather -> merge without a host round trip per batch): the batch is enqueued on `hip_stream`
 * itself; work enqueued on that stream afterwards sees the result -- PROVIDED no query of the batch overflowed its
 * candidate buffers, which only dpq_finish can tell (it answers such a batch again; whatever consumed the first
 * answer must then be redone).  dpq_finish_count reports how many batches that happened to.
 * Up to TWO streams may have stream-ordered batches in flight at once: each is given one of the library's two
 * workspaces, so a caller that alternates its steps between two streams overlaps a step's table build and bootstrap
 * with the previous step's scan and select (a third stream, or a dpq_query_batch_device_async batch, first settles
 * what is in flight). */
int dpq_query_batch_device_ordered(dpq_index* idx, const float* d_queries, int nq, int top_k, int32_t* d_ids,
                                   float* d_dists, void* hip_stream);
int dpq_finish_count(dpq_index* idx, int32_t* rerun_batches);

/* ---- exact search over raw vectors: ground truth, recall, re-ranking --------
 * Every distance above is a PQ approximation.  A dpq_flat holds the raw fp32 vectors [n][D] on one GPU and gives true
 * squared L2 distances: over all of them (ground truth, the reference's `pqtree -task groundtruth`, main.cpp:569-669)
 * or over a candidate list per query (re-ranking a PQ answer, main.cpp:898-939).
 * The arithmetic is the reference's brute force (main.cpp:150-156), met bit for bit.  For a base vector v and a query
 * q, both fp32 [D], acc is an fp64 value starting at +0.0; for d = 0 .. D-1 in ascending order:
 *     t = v[d] - q[d]      in fp32, rounded;
 *     s = t * t            in fp32, rounded on its own (no fused multiply-add);
 *     acc += (double)s     one add after the other.
 * The reported distance is (float)acc, round to nearest even (the reference keeps pair<float, uint>); it is the SQUARED
 * distance, as in the reference's file.  Results are ordered by (distance, id) ascending and at the k-th boundary the
 * lowest ids win -- the engine's rule above; the reference's heap order among exact ties is not reproduced.  Ids are
 * row numbers plus the handle's id_offset, int32.  Behaviour for non-finite inputs (NaN, infinities, or values whose
 * squared difference overflows) is unspecified.  tests/_exact_restatement.py restates these rules in numpy.
 * A handle is bound to one GPU and is used from one thread at a time.  Device memory: 4 * n * (D rounded up to a
 * multiple of 4) bytes, plus workspaces of at most about 200 MB kept until dpq_flat_close. */
typedef struct dpq_flat dpq_flat;
#define DPQ_FLAT_MAX_TOPK 16384 /* the reference's README runs groundtruth with -topk 10000 */

/* vectors[n][D], host memory, copied to GPU `device`.  DPQ_ERR_ARG before any device call: a NULL pointer, n < 1, D
 * outside 1..2048, id_offset < 0, n + id_offset >= 2^31.  Without a GPU: DPQ_ERR_NO_DEVICE.  Vectors that do not fit
 * into device memory: DPQ_ERR_NOMEM -- search a larger base part by part, each part a handle with its own id_offset,
 * and merge the answers with dpq_merge_topk_host. */
int dpq_flat_open(const float* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out);
int dpq_flat_close(dpq_flat* f);
/* Exact top_k of every query over all n vectors.  Host buffers, synchronous; queries[nq][D]; ids[nq][top_k],
 * dists[nq][top_k] ascending by (distance, id).  top_k outside 1..DPQ_FLAT_MAX_TOPK: DPQ_ERR_ARG; top_k > n:
 * DPQ_ERR_TOPK; nq == 0: DPQ_OK. */
int dpq_flat_search(dpq_flat* f, const float* queries, int nq, int top_k, int32_t* ids, float* dists);
/* map[n_map]: DFS position -> row of this handle (QNode.vec_id, dpq_tree_array 0 / dpq_read_qnode_ids), uploaded once.
 * With a map set, the candidates of dpq_flat_rerank* are DFS positions as dpq_query_batch reports them.  An entry
 * >= n is DPQ_ERR_ARG. */
int dpq_flat_set_id_map(dpq_flat* f, const uint32_t* map, int64_t n_map);
/* Exact distances of the given candidates only, the best top_k of them: cand_ids[nq][n_cand], 1 <= top_k <= n_cand <=
 * 16384.  A negative candidate is padding and is skipped.  Without a map a candidate is an id of this handle (row = id
 * - id_offset) and the same id is reported back.  With a map a candidate c is a DFS position: the row is map[c], the
 * reported id map[c] + id_offset, and for an even n_map the candidate n_map means position n_map - 1 (the even-N rule
 * above).  A candidate that names no row is DPQ_ERR_ARG (the host variant checks on the host before any device work;
 * the device variant reads one flag word back at its end, and its outputs are then unspecified).  A row named twice by
 * one query counts once.  Output ascending by (exact distance, reported id), rows padded with id -1 / +inf when fewer
 * than top_k candidates are valid. */
int dpq_flat_rerank(dpq_flat* f, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                    int32_t* ids, float* dists);
/* Same with device pointers on the handle's GPU, enqueued on `hip_stream` (NULL = default stream); returns after the
 * flag word has come back, i.e. with the results complete. */
int dpq_flat_rerank_device(dpq_flat* f, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand, int top_k,
                           int32_t* d_ids, float* d_dists, void* hip_stream);

/* Byte vectors (.bvecs data: SIFT1B and its kin, queries included) on the int8 matrix cores.  The contract is that of
 * the fp32 functions of the same name applied to the bytes widened to fp32: squared L2 reported as fp32, keys
 * `distance bits << 32 | id` ordered by (distance, id), the lowest ids winning at the k-th boundary; id_offset, the
 * DPQ_ERR_TOPK rule, nq == 0, the top_k limits, padding with -1 / +inf, a row named twice counting once, the flag word of
 * the device variant and the id map with its even-n_map rule all carry over.  dpq_flat_set_id_map, dpq_flat_close and
 * dpq_merge_topk_host work on a byte handle unchanged.
 * Why the bits are the same: with v, q in {0..255}^D and D <= 2048 every intermediate of the arithmetic above is an
 * exactly representable integer -- |t| <= 255, s <= 65025, acc <= 2048 * 65025 = 133 171 200 < 2^31 -- so acc equals the
 * int32 value sum (v[d] - q[d])^2 whatever the order of the sum, and the reported distance is (float)(int32) of it, round
 * to nearest even: the bits of dpq_flat_search on the widened data and of the reference (main.cpp:150-156 after
 * ReadTopN's widening).  Two different integer distances above 2^24 can round to the same float; they are then ordered
 * by id, because the key is built from the float's bits and not from the integer.
 * Handle kinds do not mix: a _u8 call on a handle of dpq_flat_open, or dpq_flat_search / dpq_flat_rerank* on a handle of
 * dpq_flat_open_u8, is DPQ_ERR_ARG with a message that names the other function.
 * Device memory: n * (D rounded up to a multiple of 32, the K step of v_mfma_i32_32x32x32_i8) bytes of biased vectors
 * plus 4 * n bytes of int32 norms, plus the same workspaces; while dpq_flat_open_u8 runs, an upload buffer of at most
 * 128 MB on top of that, freed before it returns.  dpq_flat_open_u8 checks its arguments as dpq_flat_open
 * does, before any device call. */
int dpq_flat_open_u8(const uint8_t* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out);
int dpq_flat_search_u8(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* dists);
int dpq_flat_rerank_u8(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                       int32_t* ids, float* dists);
int dpq_flat_rerank_u8_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                              int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);

/* ---- exact filtered and range search ------------------------------------------
 * The two other kinds of search the PQ index offers (dpq_query_batch_filtered, dpq_range_search), answered exactly over
 * the raw vectors of a dpq_flat: their ground truth.  FAISS's IndexFlat::search with an IDSelector, and
 * IndexFlat::range_search; the reference has neither.
 * Filter: the bitmap convention of dpq_filter -- bit i is bit (i & 31) of words[i >> 5], n_bits bits -- over the handle's
 * REPORTED ids, row + id_offset: row r is eligible iff r + id_offset < n_bits and that bit is set.  n_bits >= 0, and
 * n_bits == 0 allows nothing.  A base searched in parts builds each part's filter from the same global bitmap, and
 * dpq_merge_topk_host merges the partial lists unchanged.  The id map of dpq_flat_set_id_map plays no part in it.  A
 * filter works on the handle it was made for, fp32 or byte; one made on another handle is DPQ_ERR_ARG.  A NULL filter
 * is DPQ_ERR_ARG in the _filtered calls and means "every row of the handle" in the range calls.  On the device a filter
 * is the ascending list of its eligible rows (4 bytes each), so a search costs what the eligible rows cost.
 * Filtered top-k: the contract of dpq_flat_search[_u8] applied to the eligible rows only -- top_k entries ascending by
 * (distance, id), the distance bits those of dpq_flat_search, the lowest ids winning at the k-th boundary -- with rows
 * padded with id -1 / +inf when fewer than top_k rows are eligible (none at all: an all-padding answer, not an error;
 * there is no DPQ_ERR_TOPK here).  top_k outside 1..DPQ_FLAT_MAX_TOPK is DPQ_ERR_ARG; nq == 0 is DPQ_OK.
 * Range search: for query q every eligible row whose reported fp32 distance d satisfies d < radii[q], STRICTLY (the rule
 * of dpq_range_search); d is the squared L2 with the bits of dpq_flat_search, on a byte handle (float)(int32) of the
 * integer sum.  Within a list the entries ascend by (distance, id).  A radius <= 0 gives an empty list, +inf every
 * eligible row; a NaN radius is DPQ_ERR_ARG, checked before any device work.  The answer is a dpq_range_result, the type
 * dpq_range_search returns: dpq_range_result_get / dpq_range_result_free serve both.  A failed host allocation for the
 * lists is DPQ_ERR_NOMEM.
 * Handle kinds do not mix: a _u8 call on an fp32 handle or the reverse is DPQ_ERR_ARG with a message that names the other
 * function.  Order of the checks: the arguments that need no handle (NULL pointers, nq < 0, top_k, n_bits, NaN radii),
 * then the device (none visible: DPQ_ERR_NO_DEVICE), then the handle (its kind, the filter's owner).  Host buffers,
 * synchronous, one thread per handle at a time.
 * Device memory of a range call: it counts every list in one pass over the distances and forms them a second time to
 * write them (no list is ever cut short, no rerun), 1024 queries at a time, in sub-batches of queries whose lists
 * together hold at most 2^19 entries: 4 MB of keys and as much again sorted, kept until dpq_flat_close, plus the
 * segmented sort's workspace.  A single list longer than that makes a sub-batch of its own with buffers of 16 bytes per
 * entry (at most 16 * n), released before the call returns. */
typedef struct dpq_flat_filter dpq_flat_filter;
/* words[(n_bits + 31) / 32], host memory, read during the call only.  Uploads the handle's slice of the bitmap and
 * compacts it on the device into the row list (popcount, prefix sum, emit). */
int dpq_flat_filter_create(dpq_flat* f, const uint32_t* words, int64_t n_bits, dpq_flat_filter** out);
void dpq_flat_filter_free(dpq_flat_filter* ff);  /* NULL: nothing happens */
/* Rows of its handle the filter allows. */
int dpq_flat_filter_count(const dpq_flat_filter* ff, int64_t* n_allowed);
int dpq_flat_search_filtered(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, int top_k, int32_t* ids,
                             float* dists);
int dpq_flat_search_filtered_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k,
                                int32_t* ids, float* dists);
/* ff may be NULL: every row of the handle is eligible.  queries[nq][D], radii[nq]: host memory. */
int dpq_flat_range_search(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, const float* radii,
                          dpq_range_result** out);
int dpq_flat_range_search_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, const float* radii,
                             dpq_range_result** out);

/* Host only.  Two range answers in lims / ids form over the same nq queries and in the same id space (mapping ids is the
 * caller's job), summed over the queries: recall = |found & truth| / |truth|, precision = |found & truth| / |found|; a
 * zero denominator gives 1.0.  An id counts once per query; negative ids are ignored.  Either output may be NULL. */
int dpq_range_recall(int nq, const int64_t* found_lims, const int32_t* found_ids, const int64_t* truth_lims,
                     const int32_t* truth_ids, double* recall, double* precision);
/* Host only.  A bitmap over ORIGINAL vector ids -> the bitmap dpq_filter_create takes for the DTC index built from those
 * vectors.  vec_id[n_codes]: DFS position -> vector id (dpq_tree_array(.., 0) or dpq_read_qnode_ids).  For position p
 * with reported id r, bit r of the output is bit vec_id[p] of the input, or 0 when vec_id[p] >= n_bits; r = p, except that
 * the last node of an even n_codes is reported as n_codes (bit n_codes - 1 then stays 0). */
int dpq_bitmap_to_dfs(const uint32_t* words, int64_t n_bits, const uint32_t* vec_id, int64_t n_codes,
                      uint32_t* words_out /* [(n_codes + 1 + 31) / 32] */);
/* Host only.  A bitmap file: int64 n_bits, then (n_bits + 31) / 32 little-endian uint32 words.  Read with words == NULL to
 * learn n_bits.  A file shorter than its header says: DPQ_ERR_IO. */
int dpq_write_bitmap(const char* path, const uint32_t* words, int64_t n_bits);
int dpq_read_bitmap(const char* path, int64_t* n_bits, uint32_t* words);

/* Host only.  Vectors [first, first + count) of an .fvecs / .bvecs file (the streaming read of main.cpp:607-640);
 * out[count][D] may be NULL to learn D.  A range past the end of the file: DPQ_ERR_IO. */
int dpq_read_vecs_range(const char* path, int is_bvecs, int64_t first, int64_t count, int32_t* D, float* out);
/* The same over a .bvecs file with the bytes kept as they are (for dpq_flat_open_u8); the same errors. */
int dpq_read_bvecs_range(const char* path, int64_t first, int64_t count, int32_t* D, uint8_t* out);
/* The reference's ground-truth text file (PQBase::write_groundtruth / read_groundtruth, pqbase.cpp:294-332): a first
 * line `nq,top_k`, then one line per query of `id,dist,` pairs.  Distances are written with nine significant digits so
 * that they read back to the same bits (the reference's six digits lose them).  Read with ids == dists == NULL to
 * learn the shape. */
int dpq_write_groundtruth(const char* path, const int32_t* ids, const float* dists, int nq, int top_k);
int dpq_read_groundtruth(const char* path, int32_t* nq, int32_t* top_k, int32_t* ids, float* dists);
/* recall = (1 / (nq * k)) * sum over q of |found[q][0..R) intersected with truth[q][0..k)|, negative ids ignored, an id
 * counted once.  found[nq][found_stride], truth[nq][truth_stride].  R = k is the reference's measure
 * (main.cpp:783-796); k = 1 gives 1-recall@R. */
int dpq_recall(const int32_t* found, int found_stride, int R, const int32_t* truth, int truth_stride, int k, int nq,
               double* recall);

/* ---- exact inner-product search over raw vectors -------------------------------
 * The exact counterpart of dpq_query_batch_ip: every kind of exact search above, by inner product instead of squared L2,
 * on an fp32 handle of dpq_flat_open.  FAISS's IndexFlatIP; the reference has no inner product.
 * The arithmetic, met bit for bit.  For a base vector v and a query q, both fp32 [D], acc is an fp64 value starting at
 * +0.0; for d = 0 .. D-1 in ascending order:
 *     acc = acc + (double)v[d] * (double)q[d].
 * The product of two fp32 values is exact in fp64, so each step is one rounding and a fused multiply-add or a multiply
 * followed by an add give the same bits: the rule does not depend on -ffp-contract.  The score is s = (float)acc, round
 * to nearest even.  A score of -0.0 is reported and ordered as +0.0 (a tiny negative acc rounds to -0.0; acc itself is
 * never -0.0).  This is the rule of dpq_ip_tables' p[m][k]; one lane owns one score from the first dimension to the
 * last.  tests/_exact_ip_restatement.py restates these rules in numpy.
 * Order: (score descending, id ascending); at the k-th boundary the lowest ids win.  The selection is that of
 * dpq_flat_search, on keys `hi << 32 | id` with, u being the bits of the normalised score,
 *     hi = (u & 0x80000000) ? u : (~u & 0x7fffffff),
 * so that ascending keys are descending scores (+inf, 3.5, 1.0, 1e-40, 0.0, -1e-40, -1.0, -inf map to ascending hi), and
 * the all-ones padding key has the high word of a negative NaN and collides with no score.  Padding rows are id -1 with
 * score -inf.  Non-finite inputs, and scores that overflow fp32, are unspecified.
 * What carries over from the L2 function of the same shape: dpq_flat_search_ip -- the argument checks, DPQ_ERR_TOPK, nq
 * == 0 and id_offset of dpq_flat_search; dpq_flat_search_filtered_ip -- the filter, the padding and the all-padding
 * answer of an empty filter of dpq_flat_search_filtered; dpq_flat_rerank_ip[_device] -- candidates, negative candidates
 * as padding, the id map with its even-n_map rule, a row named twice counting once and the flag word of
 * dpq_flat_rerank[_device]; the order of the checks of each.
 * Range: the list of query q holds every eligible row with s > thresholds[q], STRICTLY (FAISS's inner-product
 * convention); the `dists` array of the dpq_range_result holds the scores, and a list is ordered by (score descending, id
 * ascending).  A threshold of -inf keeps every row, +inf none, -0.0 is read as +0.0; a NaN threshold is DPQ_ERR_ARG,
 * checked before any device work.
 * Byte handles take byte queries: an fp32-query _ip call on a handle of dpq_flat_open_u8 is DPQ_ERR_ARG with a message
 * that names the _ip_u8 call ("exact inner product over byte vectors" below). */
int dpq_flat_search_ip(dpq_flat* f, const float* queries, int nq, int top_k, int32_t* ids, float* scores);
int dpq_flat_search_filtered_ip(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, int top_k, int32_t* ids,
                                float* scores);
/* ff may be NULL: every row of the handle is eligible.  queries[nq][D], thresholds[nq]: host memory. */
int dpq_flat_range_search_ip(dpq_flat* f, const dpq_flat_filter* ff, const float* queries, int nq, const float* thresholds,
                             dpq_range_result** out);
int dpq_flat_rerank_ip(dpq_flat* f, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k, int32_t* ids,
                       float* scores);
int dpq_flat_rerank_ip_device(dpq_flat* f, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand, int top_k,
                              int32_t* d_ids, float* d_scores, void* hip_stream);
/* Host only: dpq_merge_topk_host for lists of scores.  ids / scores [n_lists][nq][top_k]; the answer is the best top_k of
 * a query's n_lists * top_k rows by (score descending, id ascending).  A row with id < 0 is padding; repeated rows are
 * kept; missing rows are padded with -1 / -inf; -0.0 is reported as +0.0.  A base searched part by part, each part a
 * handle with its own id_offset, merges its dpq_flat_search_ip answers here (dpq_merge_topk_host orders by distance bits,
 * which puts every negative score last and the positive ones upside down).  DPQ_ERR_ARG: a NULL pointer, n_lists < 1,
 * top_k < 1, nq < 0. */
int dpq_merge_topk_ip_host(const int32_t* ids, const float* scores, int n_lists, int nq, int top_k, int32_t* out_ids,
                           float* out_scores);

/* ---- exact inner product over byte vectors; signed int8 storage -------------------
 * The last two cells of the table of kinds x metrics: inner product on a handle of dpq_flat_open_u8, and a handle kind
 * for signed bytes -- embeddings quantised to int8 and scored by dot product -- with both metrics.  Both run on the int8
 * matrix cores (v_mfma_i32_32x32x32_i8) over rows of one byte per value.  Every answer is an integer below 2^31 in
 * magnitude, so the contract is once more "the bits of the fp32 call over the rows widened to fp32", with no tolerance.
 * Unsigned bytes, inner product (the _ip_u8 calls; const uint8_t* queries).  v, q in {0..255}^D, D <= 2048:
 * S = sum v[d] * q[d] is an integer, 0 <= S <= 2048 * 65025 = 133 171 200 < 2^31, and the score is (float)(int32)S, round
 * to nearest even.  These are the bits of dpq_flat_search_ip over the widened rows: its fp64 accumulator holds S exactly,
 * whatever the order.  Order, key word and padding (-1 / -inf) are those of the fp32 inner-product calls above; range
 * search keeps s > threshold, strictly, with -0.0 read as +0.0 and a NaN threshold refused first.  Two different
 * integers above 2^24 that round to the same float are ordered by id: the key is built from the float's bits.
 * The stored rows are v' = v - 128 and the staged queries q' = q - 128, so the kernel forms
 *     S = v'.q' + rs[row] + qs[query],   rs = 128 sum v' + 16384 D,   qs = 128 sum q',
 * in int32: |v'.q'| <= 2^25, 0 <= rs < 2^26, |qs| <= 2^25.  The rows' terms rs are made by the FIRST inner-product search
 * or range call on the handle, in one pass over the stored rows, and cost 4 * n bytes of device memory from then until
 * dpq_flat_close; dpq_flat_open_u8 and the L2 calls keep their device memory and their behaviour.  The re-rank forms
 * the products of the bytes themselves and needs no such array.
 * Signed bytes (dpq_flat_open_i8 and the _i8 calls; const int8_t* vectors and queries).  v, q in {-128..127}^D.
 * L2: sum (v[d] - q[d])^2 <= 2048 * 255^2 < 2^31, reported as (float)(int32): the bits of dpq_flat_search over the
 * widened rows.  Inner product: |S| <= 2048 * 128^2 = 2^25, reported as (float)(int32)S -- the int8 dot product itself,
 * with no correction term; negative scores take the sign branch of the key word, an integer 0 is +0.0.  Device memory:
 * that of dpq_flat_open_u8.
 * What carries over unchanged from the call of the same shape (dpq_flat_search_u8 for dpq_flat_search_i8,
 * dpq_flat_search_ip for dpq_flat_search_ip_u8, and so on): every argument check and its order (arguments, then
 * device, then handle), DPQ_ERR_TOPK, nq == 0, id_offset, the padding rows, filters (dpq_flat_filter_create and
 * dpq_flat_filter_count work on an i8 handle), dpq_flat_set_id_map with the even-n_map rule, negative candidates as
 * padding, a row named twice counting once, the flag word of the device forms, dpq_flat_close, dpq_merge_topk_host (L2)
 * and dpq_merge_topk_ip_host (scores).
 * Handle kinds do not mix: fp32 (and half, and scalar-quantised), u8 and i8 handles each take the calls of their own kind; any other is
 * DPQ_ERR_ARG with a message that names the function to call instead.  fp32 queries against byte rows are out of scope. */
int dpq_flat_open_i8(const int8_t* vectors, int64_t n, int D, int device, int64_t id_offset, dpq_flat** out);
int dpq_flat_search_ip_u8(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* scores);
int dpq_flat_search_filtered_ip_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k,
                                   int32_t* ids, float* scores);
int dpq_flat_range_search_ip_u8(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq,
                                const float* thresholds, dpq_range_result** out);
int dpq_flat_rerank_ip_u8(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                          int32_t* ids, float* scores);
int dpq_flat_rerank_ip_u8_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                 int top_k, int32_t* d_ids, float* d_scores, void* hip_stream);
int dpq_flat_search_i8(dpq_flat* f, const int8_t* queries, int nq, int top_k, int32_t* ids, float* dists);
int dpq_flat_search_filtered_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, int top_k,
                                int32_t* ids, float* dists);
int dpq_flat_range_search_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, const float* radii,
                             dpq_range_result** out);
int dpq_flat_rerank_i8(dpq_flat* f, const int8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                       int32_t* ids, float* dists);
int dpq_flat_rerank_i8_device(dpq_flat* f, const int8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                              int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);
int dpq_flat_search_ip_i8(dpq_flat* f, const int8_t* queries, int nq, int top_k, int32_t* ids, float* scores);
int dpq_flat_search_filtered_ip_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq, int top_k,
                                   int32_t* ids, float* scores);
int dpq_flat_range_search_ip_i8(dpq_flat* f, const dpq_flat_filter* ff, const int8_t* queries, int nq,
                                const float* thresholds, dpq_range_result** out);
int dpq_flat_rerank_ip_i8(dpq_flat* f, const int8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                          int32_t* ids, float* scores);
int dpq_flat_rerank_ip_i8_device(dpq_flat* f, const int8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                 int top_k, int32_t* d_ids, float* d_scores, void* hip_stream);

/* ---- exact search over half-precision vectors: fp16 and bf16 storage -------------
 * Embeddings are stored as fp16 or bf16.  A half handle keeps such rows on the GPU as they are, 16 bits per value, at
 * half the device memory, half the upload and half the bytes a re-rank gathers of an fp32 handle over the same rows.
 * FAISS's IndexScalarQuantizer(QT_fp16 / QT_bf16) under IndexFlat's calls, and IndexRefineFlat over it.
 * There are no new search calls.  Every fp32-query call above takes an fp32 handle or a half handle: dpq_flat_search,
 * dpq_flat_search_ip, dpq_flat_search_filtered, dpq_flat_search_filtered_ip, dpq_flat_range_search,
 * dpq_flat_range_search_ip, dpq_flat_rerank, dpq_flat_rerank_device, dpq_flat_rerank_ip, dpq_flat_rerank_ip_device,
 * dpq_flat_filter_create, dpq_flat_filter_count, dpq_flat_set_id_map, dpq_flat_close.  Queries stay fp32 and are never
 * narrowed.  A _u8 call on a half handle is DPQ_ERR_ARG with a message that names the fp32 function.
 * The contract.  Widening fp16 or bf16 to fp32 is exact, so there is no tolerance: any call above on a half handle gives
 * ids, float bits and lims equal, bit for bit, to the same call on a dpq_flat_open handle over dpq_half_to_float(vectors).
 * The L2 rule (fp32 subtract, fp32 square, fp64 accumulate in ascending d), the inner-product rule (fp64 accumulate of
 * exact products, -0.0 reported as +0.0), the key order and the padding rows, DPQ_ERR_TOPK, the id map with its
 * even-n_map rule, the flag word of the device forms and the order of the argument checks all carry over unchanged.
 * Narrowing (dpq_half_from_float on the host, dpq_flat_open_narrowed on the device: the same bits): round to nearest,
 * ties to even.  bf16: with u the fp32 bits, (u + 0x7fff + ((u >> 16) & 1)) >> 16.  fp16: the IEEE conversion with
 * gradual underflow -- 2^-24 gives 0x0001, 2^-25 gives 0x0000, 2^-25 * (1 + 2^-20) gives 0x0001, 65519.99 gives 0x7bff,
 * 65520 gives 0x7c00.  -0.0 keeps its sign.  NaN inputs are out of scope.  A value that narrows to an infinity is stored
 * as one; searches over it fall under the exact search's "non-finite: unspecified" clause.  Subnormal halves are kept,
 * never flushed, when they are widened.  tests/_half_restatement.py restates both rules and the widening in numpy.
 * Device memory: 2 * n * (D rounded up to a multiple of 8) bytes, plus the workspaces of an fp32 handle; while
 * dpq_flat_open_narrowed runs (and dpq_flat_open_half with D not a multiple of 8), an upload buffer of at most 128 MB on
 * top of that, freed before it returns. */
#define DPQ_HALF_F16  1   /* IEEE binary16 */
#define DPQ_HALF_BF16 2   /* bfloat16: the upper 16 bits of a binary32 */
/* Host only, no device.  in[count] -> out[count]; count == 0 is DPQ_OK.  DPQ_ERR_ARG: a NULL pointer with count > 0,
 * count < 0, format outside {DPQ_HALF_F16, DPQ_HALF_BF16}. */
int dpq_half_from_float(const float* in, int64_t count, int format, uint16_t* out);
int dpq_half_to_float(const uint16_t* in, int64_t count, int format, float* out);
/* vectors[n][D], host memory, 16-bit values of `format`, uploaded as they are.  The arguments are checked as
 * dpq_flat_open checks them, before any device call; format outside {1, 2} is DPQ_ERR_ARG; no visible device is
 * DPQ_ERR_NO_DEVICE. */
int dpq_flat_open_half(const uint16_t* vectors /* [n][D], host */, int64_t n, int D, int format, int device,
                       int64_t id_offset, dpq_flat** out);
/* The same handle from fp32 rows (an .fvecs base, or what dpq_read_vecs_range returns), narrowed on the GPU in upload
 * slices of at most 128 MB: indistinguishable from dpq_flat_open_half over dpq_half_from_float of the same rows. */
int dpq_flat_open_narrowed(const float* vectors /* [n][D], host */, int64_t n, int D, int format, int device,
                           int64_t id_offset, dpq_flat** out);

/* ---- exact search over scalar-quantised vectors: 8 and 4 bits per dimension ---
 * Between a PQ code (8 B per 128-d vector, 16 B with a refine level) and a half handle (256 B) sits a scalar quantiser:
 * one byte (128 B) or one nibble (64 B) per dimension, with a trained offset and step per dimension, under fp32 queries.
 * FAISS's IndexScalarQuantizer(QT_8bit / QT_4bit) under IndexFlat's calls, and IndexRefine over it.  The rules below
 * are this library's own; tests/_sq_restatement.py restates them in numpy and the GPU meets them bit for bit.
 * bits is DPQ_SQ_8BIT or DPQ_SQ_4BIT and L = 2^bits - 1.  A quantiser over D dimensions is two fp32 arrays, lo[D] and
 * step[D].
 * Train (dpq_sq_train).  Per dimension lo[d] is the minimum and hi[d] the maximum of the training values; a result of
 * -0.0 is stored as +0.0.  step[d] = (float)(((double)hi[d] - (double)lo[d]) / (double)L): one fp64 subtract, one fp64
 * divide, one rounding to fp32.  A constant column gives step = +0.0.  Non-finite inputs, and a range whose step is not
 * finite, are out of scope.  lo = 0.1f (0x3dcccccd), hi = 0.7f (0x3f333333): the 8-bit step is 0x3b1a33cd, the 4-bit
 * step 0x3d23d70a.
 * Encode.  step[d] == 0 gives code 0.  Otherwise u = ((double)v - (double)lo[d]) / (double)step[d], one fp64 subtract and
 * one fp64 divide; c = rint(u), ties to even, clamped to [0, L] before the conversion to an integer: values outside the
 * trained range saturate.  With lo = 0, step = 1 and 8 bits, 0.5, 1.5, 2.5, 254.5, 255.5, 300 and -3 encode to 0, 2, 2,
 * 254, 255, 255 and 0.  Under the quantiser above 0.4f encodes to 128 at 8 bits and to 8 at 4 bits.
 * Decode.  x = lo[d] + (float)c * step[d] in fp32, the product and the sum each rounded on its own; no fused
 * multiply-add.  Under the quantiser above code 128 decodes to 0x3ecd6700 at 8 bits, code 8 to 0x3ed70a3d at 4 bits;
 * lo = 0x3eb0f069, step = 0x3b82a8a7, c = 111 decodes to 0x3f49c676 (a fused decode would give 0x3f49c675).
 * Storage.  8 bits: one byte per dimension, D bytes per row.  4 bits: dimension 2j in the low nibble and 2j + 1 in the
 * high nibble of byte j, (D + 1) / 2 bytes per row; the spare nibble of an odd D is written as 0 and ignored when read.
 * Search.  There are no new search calls: a quantised handle takes every fp32-query call the half section lists.  Queries
 * are fp32 and never quantised.  Every such call on a quantised handle gives ids, float bits and lims equal, bit for bit,
 * to the same call on a dpq_flat_open handle over dpq_sq_decode of the codes.  The L2 and the inner-product rule, the key
 * order and the padding rows, DPQ_ERR_TOPK, the id map with its even-n_map rule, the flag word of the device forms and
 * the order of the argument checks all carry over unchanged.  A _u8 or _i8 call on a quantised handle is DPQ_ERR_ARG
 * with a message that names the fp32 function.
 * Argument errors, DPQ_ERR_ARG, in this order and before any device call: a NULL pointer; n < 1; D outside 1..2048; bits
 * outside {4, 8}; id_offset as in dpq_flat_open; a lo that is not finite; a step that is negative, NaN or infinite;
 * exactly one of lo / step given to dpq_flat_open_quantised.  Then the device: DPQ_ERR_NO_DEVICE without one.
 * Device memory of a handle: n * Dp bytes at 8 bits (Dp = D rounded up to a multiple of 16), n * Dp / 2 bytes at 4 bits
 * (Dp = D rounded up to a multiple of 32), 8 bytes per padded dimension (rounded up to 32 dimensions), and the
 * workspaces of an fp32 handle; while a call runs that uploads in slices, a buffer of at most 128 MB on top of that. */
#define DPQ_SQ_8BIT 8
#define DPQ_SQ_4BIT 4
/* vectors[n][D], host memory -> lo_out[D], step_out[D].  The minima and maxima are reduced on the GPU, over upload
 * slices of at most 128 MB. */
int dpq_sq_train(const float* vectors, int64_t n, int D, int bits, int device, float* lo_out, float* step_out);
/* vectors[n][D], host memory -> codes_out[n][D] (8 bits) or [n][(D + 1) / 2] (4 bits), encoded on the GPU in the same
 * slices. */
int dpq_sq_encode(const float* vectors, int64_t n, int D, int bits, const float* lo, const float* step, int device,
                  uint8_t* codes_out);
/* Host only, no device: codes as dpq_sq_encode writes them -> out[n][D]. */
int dpq_sq_decode(const uint8_t* codes, int64_t n, int D, int bits, const float* lo, const float* step, float* out);
/* A handle over codes the caller already has, uploaded as they are and padded on the GPU. */
int dpq_flat_open_sq(const uint8_t* codes, int64_t n, int D, int bits, const float* lo, const float* step, int device,
                     int64_t id_offset, dpq_flat** out);
/* The same handle from fp32 rows, quantised on the GPU in upload slices of at most 128 MB.  lo and step are both given,
 * or both NULL: the quantiser is then trained on these very rows.  Indistinguishable from dpq_sq_train (when NULL), then
 * dpq_sq_encode, then dpq_flat_open_sq. */
int dpq_flat_open_quantised(const float* vectors /* [n][D], host */, int64_t n, int D, int bits, const float* lo,
                            const float* step, int device, int64_t id_offset, dpq_flat** out);
/* The quantiser of a quantised handle: *bits, lo_out[D], step_out[D].  DPQ_ERR_ARG on a handle of any other kind. */
int dpq_flat_sq_get(const dpq_flat* f, int* bits, float* lo_out, float* step_out);

/* ---- exact search over binary vectors: one bit per dimension, by Hamming distance ---
 * The bottom of the storage ladder: sign-binarised embeddings, perceptual hashes and LSH sketches, 1 bit per dimension
 * (128 B for 1024 dimensions), compared by the number of differing dimensions.  FAISS's IndexBinaryFlat.  The rules below
 * are this library's own; tests/_exact_bits_restatement.py restates them in numpy and the GPU meets them bit for bit.
 * Row layout.  A row is D bits in (D + 7) / 8 bytes; dimension d is bit d & 7 of byte d >> 3 (numpy's
 * packbits(..., bitorder="little"), and the convention of this library's bitmaps).  1 <= D <= DPQ_FLAT_BITS_MAX_D.  The
 * spare high bits of a row's last byte are ignored, whatever they hold, in base rows and in queries alike.
 * Distance.  The distance of a query and a row is the number of dimensions in which they differ, reported as (float) of
 * that integer, which is exact.  Keys, order and padding are those of the L2 calls: rows ascend by (distance, reported
 * id), reported id = row + id_offset, a list shorter than top_k is padded with -1 / +inf; top_k outside
 * 1..DPQ_FLAT_MAX_TOPK is DPQ_ERR_ARG and top_k > n DPQ_ERR_TOPK (not for the filtered call).  Range search is strict
 * (d < r); every query's list is sorted by (distance, id); the result is a dpq_range_result.  Re-ranking follows
 * dpq_flat_rerank's rules: negative candidates are padding, a row named twice counts once, the id map with its even-n_map
 * rule, 1 <= top_k <= n_cand <= 16384, a candidate that names no row is DPQ_ERR_ARG (the device form raises a flag word
 * that is read back at the end).
 * Call kinds.  A bits handle takes the _bits calls only: every other dpq_flat_* search, range or re-rank call on it is
 * DPQ_ERR_ARG with a message that names the _bits call of the same shape (there is no inner product over bits), and a
 * _bits call on a handle of any other kind is refused the same way.  dpq_flat_set_id_map, dpq_flat_filter_create,
 * dpq_flat_close and dpq_merge_topk_host work on a bits handle unchanged.
 * Binarising.  bit d = (v[d] > t[d]), the comparison in fp32, with t the caller's thresholds[D] or all zeros when
 * thresholds is NULL: NaN and -0.0 > 0 give 0.  There is no training step, so nothing depends on a reduction order.
 * Argument errors, DPQ_ERR_ARG, in this order and before any device call: a NULL pointer; n < 1; D outside
 * 1..DPQ_FLAT_BITS_MAX_D; id_offset as in dpq_flat_open.  Then the device: DPQ_ERR_NO_DEVICE without one.
 * Device memory of a handle: n * Rp bytes, Rp = (D + 7) / 8 rounded up to a multiple of 16, and the workspaces of a byte
 * handle; while a call runs that uploads in slices, a buffer of at most 128 MB on top of that. */
#define DPQ_FLAT_BITS_MAX_D 4096
/* A handle over packed rows the caller already has, uploaded as they are; masked and padded on the GPU. */
int dpq_flat_open_bits(const uint8_t* rows /* [n][(D+7)/8], host */, int64_t n, int D /* bits */, int device,
                       int64_t id_offset, dpq_flat** out);
/* vectors[n][D], host memory -> bits_out[n][(D+7)/8], spare bits 0; binarised on the GPU in upload slices of at most
 * 128 MB. */
int dpq_bits_from_float(const float* vectors /* [n][D], host */, int64_t n, int D, const float* thresholds /* [D] or NULL */,
                        int device, uint8_t* bits_out /* [n][(D+7)/8], spare bits 0 */);
/* The same handle from fp32 rows, binarised on the device slice by slice, as dpq_flat_open_quantised encodes:
 * indistinguishable from dpq_bits_from_float, then dpq_flat_open_bits. */
int dpq_flat_open_binarised(const float* vectors, int64_t n, int D, const float* thresholds, int device, int64_t id_offset,
                            dpq_flat** out);
/* queries [nq][(D+7)/8] throughout; otherwise the argument lists and rules of the _u8 call of the same shape. */
int dpq_flat_search_bits(dpq_flat* f, const uint8_t* queries, int nq, int top_k, int32_t* ids, float* dists);
int dpq_flat_search_filtered_bits(dpq_flat* f, const dpq_flat_filter* ff, const uint8_t* queries, int nq, int top_k,
                                  int32_t* ids, float* dists);
int dpq_flat_range_search_bits(dpq_flat* f, const dpq_flat_filter* ff /* may be NULL */, const uint8_t* queries, int nq,
                               const float* radii, dpq_range_result** out);
int dpq_flat_rerank_bits(dpq_flat* f, const uint8_t* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                         int32_t* ids, float* dists);
int dpq_flat_rerank_bits_device(dpq_flat* f, const uint8_t* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);

/* ---- residual re-ranking: a second PQ level refines a shortlist ---------------
 * Every answer of dpq_query_batch is a coarse PQ approximation, and dpq_flat_rerank needs the raw vectors on the GPU
 * (512 B per SIFT vector against 8 B of code).  A dpq_refine is a second product quantizer over the RESIDUALS of the
 * handle's nodes against their level-1 reconstruction (Jegou, Tavenard, Douze, Amsaleg, "Searching in one billion
 * vectors: re-rank with source coding", ICASSP 2011; FAISS's IndexRefine over two PQ indexes): M2 more bytes per
 * node, and a shortlist is re-ranked by the distance to the two-level reconstruction.
 * Definitions.  The handle has M, K, Ds (dpq_set_codebook) and D1 = M * Ds, the width of its queries.  A level has M2,
 * K2 and Ds2 = ceil(D1 / M2), codewords2 [M2][K2][Ds2] and one code c2[M2] per node of the handle.  For node p with
 * level-1 code c1 and j = 0 .. D1-1:
 *     a[j] = codewords1[j / Ds][c1[j / Ds]][j % Ds]     the very floats dpq_set_codebook received; the level keeps its
 *                                                       own device copy taken when it is made: a later
 *                                                       dpq_set_codebook does not change a level;
 *     r[j] = v[j] - a[j]                                the residual: one fp32 subtraction, rounded; v is the node's
 *                                                       raw vector [D], zero padded to D1; ceil(D / M) must be Ds;
 *     c2   = dpq_encode_pq(r, D = D1, codewords2, M2, K2, Ds2)   with its padding of r to M2 * Ds2 and its
 *                                                       first-minimum rule;
 *     b[j] = codewords2[j / Ds2][c2[j / Ds2]][j % Ds2];
 *     x[j] = a[j] + b[j]                                the reconstruction: one fp32 add, rounded.
 * The refined distance of a query q [D1] to the node is the exact search's arithmetic (above) over the row x: for j
 * ascending t = x[j] - q[j] in fp32, s = t * t in fp32 rounded on its own, acc += (double)s from +0.0; the result is
 * (float)acc.  No fused multiply-add, no distance split across lanes, no |q-a|^2 - 2 (q-a).b + |b|^2 shortcut.
 * tests/_refine_restatement.py restates these rules in numpy; the GPU meets them bit for bit.
 * Results follow dpq_flat_rerank's rules: keys `distance bits << 32 | reported id` ascending; the reported id is the
 * candidate id itself; a negative candidate is padding; a node named twice by one query counts once; rows are padded
 * with -1 / +inf; 1 <= top_k <= n_cand <= 16384.  A non-negative candidate or id that names no node of the handle --
 * by the code lookup's id rules: global positions on shards and parts, prefixes, plain handles, the even-N rule -- is
 * DPQ_ERR_ARG: the host forms check on the host before any device work, the device form raises a flag word that is
 * read back at the end (its outputs are then unspecified).
 * DPQ_ERR_ARG for a level's shape: M2 outside 1..64, K2 outside 2..256, Ds2 != ceil(D1 / M2), (M2 - 1) * Ds2 >= D1 (a
 * sub-space without a real dimension).  A level made on another handle is DPQ_ERR_ARG.  Before dpq_set_codebook:
 * DPQ_ERR_STATE.  Argument checks that need no device come first.  All entry points are synchronous and finish
 * pending asynchronous batches first.  A level must be freed before the dpq_close of its handle.  Handles of M = 8 and
 * M = 16 (what the code lookup decodes).
 * Shards: every shard has its own level over its own nodes; the partial refined lists merge with dpq_merge_topk_*
 * unchanged.  The merged answer re-ranks the UNION of the shards' shortlists (n_cand candidates per shard), which can
 * only add candidates over a single handle's shortlist of n_cand.
 * Device memory: M2 bytes per node of the handle plus the two codebooks, until dpq_refine_free; workspaces of one
 * slice of 2^20 candidates (M MB of level-1 codes, 16 MB of keys) kept with the level; dpq_refine_build adds one
 * slice's rows and residuals (at most 128 MB each) while it runs. */
typedef struct dpq_refine dpq_refine;
typedef struct dpq_refine_opts {
    int32_t M2;        /* 0 = M */
    int32_t K2;        /* 0 = 256 */
    int64_t train_n;   /* residuals the codebook is trained on; 0 = min(n_local, 256 * K2) */
    int32_t max_iters; /* 0 = 25; then dpq_train_opts' meaning */
    int32_t init, restarts;
    int32_t reserved;  /* 0 */
    uint64_t seed;
} dpq_refine_opts;
/* Row i of out[n][D1] is the residual of the node ids[i] names against vectors[i] (vectors[n][D]); a negative id gives
 * D1 quiet NaNs.  Host buffers. */
int dpq_residuals(dpq_index* idx, const int32_t* ids, int64_t n, const float* vectors, int D, float* out);
/* Uploads a ready-made level: codewords2 [M2][K2][Ds2], codes2[n_local][M2], row l for position node_lo + l; n_local
 * must be the handle's node count; a code byte >= K2 is DPQ_ERR_ARG.  With dpq_refine_get, dpq_write_codewords and
 * dpq_write_codes_plain this is how a level is saved and loaded again. */
int dpq_refine_create(dpq_index* idx, const float* codewords2, int M2, int K2, int Ds2, const uint8_t* codes2,
                      int64_t n_local, dpq_refine** out);
void dpq_refine_free(dpq_refine* r);  /* NULL: nothing happens */
/* The shape, and with non-NULL pointers the codewords [M2][K2][Ds2] and codes [n_local][M2] back (host). */
int dpq_refine_get(const dpq_refine* r, int32_t* M2, int32_t* K2, int32_t* Ds2, int64_t* n_local, float* codewords2,
                   uint8_t* codes2);
/* Trains and encodes a level from raw vectors [n_rows][D] (host).  The row of local node l is vectors[vec_id[l]]
 * (vec_id [n_local], an entry >= n_rows is DPQ_ERR_ARG), or vectors[l] when vec_id is NULL (then n_rows = n_local).
 * opts NULL = all defaults.  By definition the composition of public calls, byte for byte: the sample positions
 * l_i = floor(i * n_local / train_n), i = 0 .. train_n - 1; dpq_residuals of the sample; dpq_train_codebook(those,
 * train_n, D1, M2, K2, the options, the handle's device); then for every node dpq_residuals and dpq_encode_pq; then
 * dpq_refine_create.  It streams the nodes in slices of at most 2^20 (host gather into staging, upload, residual and
 * encode on the device), so device memory stays bounded whatever n_local. */
int dpq_refine_build(dpq_index* idx, const float* vectors, int64_t n_rows, int D, const uint32_t* vec_id,
                     const dpq_refine_opts* opts, dpq_refine** out);
/* x rows [n][D1] of reported ids, with dpq_reconstruct's padding rule (a negative id: D1 quiet NaNs).  Host buffers. */
int dpq_refine_reconstruct(dpq_refine* r, const int32_t* ids, int64_t n, float* out);
/* queries[nq][D1], cand_ids[nq][n_cand] -> ids / dists [nq][top_k].  Host buffers.  Candidates are processed in slices
 * of at most 2^20, so the level-1 code scratch stays at M MB. */
int dpq_refine_rerank(dpq_refine* r, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                      int32_t* ids, float* dists);
/* Device pointers on the handle's GPU, enqueued on `hip_stream` (NULL = default stream); returns after the flag word
 * has come back, i.e. with the results complete (dpq_flat_rerank_device's conventions). */
int dpq_refine_rerank_device(dpq_refine* r, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                             int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);
/* The PQ top-n_cand on the device (dpq_query_batch_device, or _device_filtered when filter is not NULL), then the
 * refined re-rank of those lists, with no host round trip in between.  By definition dpq_query_batch[_filtered] with
 * top_k = n_cand followed by dpq_refine_rerank; n_cand is bound by both (<= 2048), and n_cand above the handle's codes
 * is DPQ_ERR_TOPK.  Host buffers. */
int dpq_query_batch_refined(dpq_index* idx, dpq_refine* r, const dpq_filter* filter, const float* queries, int nq,
                            int n_cand, int top_k, int32_t* ids, float* dists);

/* ---- OPQ: a learned rotation in front of the product quantizer -----------------
 * Non-parametric Optimized Product Quantization (Ge, He, Ke, Sun, CVPR 2013): an orthogonal R is learned together with
 * the codebooks; vectors and queries are rotated (x . R) before they are encoded or looked up.  The index, the scans,
 * the filters and the refine level are untouched: they hold codes of rotated vectors.  L2 distances do not see R, so
 * exact search, ground truth and the exact re-rank keep the raw vectors.  NO REFERENCE SEMANTICS: the rules are this
 * build's own, restated in tests/_opq_restatement.py and met by the GPU bit for bit.
 *   Rotation   R is float [D][D], row-major, out = x . R.  out[i][j]: acc = +0.0 in fp64; for d = 0 .. D-1 ascending
 *           acc = acc + (double)x[i][d] * (double)R[d][j]; out[i][j] = (float)acc.  The product of two fp32 values is
 *           exact in fp64 (48 significant bits, exponent in range), so a fused multiply-add and a separate multiply and
 *           add give the same bits; the kernel uses v_fma_f64.  Not allowed: fp32 accumulation, another dimension
 *           order, a sum split across lanes.  1 <= D <= 1024.  out must not alias x (the same pointer: DPQ_ERR_ARG).
 *           +inf from an overflowing final conversion is an ordinary value; NaN inputs are out of scope.
 *   Cross-covariance   C[d][j] = sum over i of (double)x[i][d] * (double)y[i][j], double [D][D], where
 *           y[i][j] = codewords[j / Ds][codes[i][j / Ds]][j % Ds] is the reconstruction (never materialised on the
 *           host) and D = M * Ds.  Order, the trainer's leaf rule with a leaf of 1024 consecutive rows (the last may be
 *           short): S_l is the fp64 sum, from +0.0, over the leaf's rows in ascending i, one add after the other;
 *           T_0 = S_0, T_l = T_{l-1} + S_l; C = the last T.  No floating-point atomics.  A code byte >= K: DPQ_ERR_ARG.
 *           Device memory: the inputs, plus at most 256 MiB of leaf sums (leaves are taken in passes of
 *           max(1, 256 MiB / (8 D^2)), at most 65535, the chain running on through the passes).
 *   Procrustes   dpq_procrustes returns, in fp64 on the host, the orthogonal polar factor U . V^T of C = U . S . V^T
 *           by one-sided (Hestenes) Jacobi.  The library is built with -ffp-contract=off: every multiply and add below
 *           is rounded on its own.
 *             scale    A = C * 2^-e, e the binary exponent that brings the largest |C[i][j]| into [0.5, 1) (exact).
 *                      V = the identity.
 *             sweep    pairs (p, q), p < q, cyclic: p = 0 .. D-2 ascending, inside it q = p+1 .. D-1 ascending.
 *                      alpha = sum_i A[i][p]^2, beta = sum_i A[i][q]^2, gamma = sum_i A[i][p] * A[i][q]: column sums in
 *                      ascending row order from +0.0, of the columns as they are at that moment.  The pair is skipped
 *                      when gamma * gamma <= (D * 2^-104) * alpha * beta.  Otherwise zeta = (beta - alpha) / (2 * gamma),
 *                      t = (zeta >= 0 ? 1 : -1) / (|zeta| + sqrt(1 + zeta * zeta)), c = 1 / sqrt(1 + t * t), s = c * t,
 *                      and for every row i of A and of V: (a, b) = (M[i][p], M[i][q]); M[i][p] = c * a - s * b;
 *                      M[i][q] = s * a + c * b.
 *             stop     after a sweep without a rotation, or after 64 sweeps.
 *             answer   sigma_j = sqrt(sum_i A[i][j]^2); U[i][j] = A[i][j] / sigma_j; R[i][k] = the sum over j
 *                      ascending, from +0.0, of U[i][j] * V[k][j].
 *           *degenerate = 1 and R_out untouched when the smallest sigma is at or below D * 2^-52 times the largest, or
 *           an entry of C (or a sigma) is not finite: the polar factor is not unique there.  The same input gives the
 *           same bytes.  Needs no device.
 *   Training   dpq_opq_train is BY DEFINITION this composition of the public calls, byte for byte.  D % M == 0 (else
 *           DPQ_ERR_ARG: zero padding makes C singular; a caller pads the vectors and says so), Ds = D / M.
 *             t = 0    R_0 = the identity, or the caller's matrix (use_initial_rotation); X^ = dpq_rotate(X, R_0);
 *                      cb_0 = dpq_train_codebook(X^; max_iters = init_iters, seed, init, restarts);
 *                      obj_0 = the sum over m ascending, in fp64 from +0.0, of dpq_train_potential(X^, cb_0)[m].
 *             t = 1 .. outer_iters   codes = dpq_encode_pq(X^, cb_{t-1}); C = dpq_cross_covariance(X -- not X^ --,
 *                      codes, cb_{t-1}); R64 = dpq_procrustes(C); R_t = (float)R64 entry by entry, or R_{t-1} when
 *                      degenerate (counted in the stats); X^ = dpq_rotate(X, R_t); cb_t = dpq_train_codebook(X^;
 *                      use_initial = cb_{t-1}, max_iters = inner_iters, init = 0, restarts = 0); obj_t as above.
 *           Returned: the pair (R_t, cb_t) with the lowest obj_t, a tie going to the lowest t.  So outer_iters = 0 with
 *           the identity returns dpq_train_codebook's bytes, and the result is never worse than its own start by its
 *           own measure.  opts == NULL: device 0, 8 outer steps, 25 first rounds, 4 inner rounds, seed 0, random rows.
 * DPQ_ERR_ARG before any device call: a NULL pointer, D outside 1..1024, n < 0 (n < 1 for the cross-covariance),
 * D != M * Ds, D % M != 0, outer_iters outside 0..64, init_iters or inner_iters outside 1..64, and what
 * dpq_train_codebook refuses.  Without a GPU: DPQ_ERR_NO_DEVICE, except dpq_procrustes, dpq_write_rotation and
 * dpq_read_rotation, which need none. */
typedef struct dpq_opq_opts {
    int32_t device;
    int32_t outer_iters;          /* 0..64 */
    int32_t init_iters;           /* 1..64: rounds of the first training */
    int32_t inner_iters;          /* 1..64: rounds of every later one */
    uint64_t seed;                /* seed, init, restarts: handed to the first dpq_train_codebook */
    int32_t init;
    int32_t restarts;
    int32_t use_initial_rotation; /* != 0: `rotation` holds R_0 on entry */
    int32_t reserved[1];          /* 0 */
} dpq_opq_opts;

typedef struct dpq_opq_stats {
    int32_t outer_run;             /* outer steps run */
    int32_t best_t;                /* the step whose pair was returned */
    int32_t degenerate;            /* steps whose Procrustes solve was degenerate (the rotation was kept) */
    int32_t reserved;
    double objective[65];          /* obj_t, t = 0 .. outer_run */
    double rotation_residual[64];  /* max |R_t^T R_t - I|, t = 1 .. outer_run at [t - 1]; fp64 on the host */
    double gpu_ms, wall_ms, rounds_ms, assign_ms, update_ms, repair_ms; /* the trainer's, summed; wall_ms: this call */
    double rotate_ms, cross_ms, procrustes_ms; /* host clock around those calls (transfers included) */
} dpq_opq_stats;

/* Host buffers; slices of at most 2^20 rows, so device memory stays bounded whatever n. */
int dpq_rotate(const float* vectors, int64_t n, int D, const float* R, int device, float* out);
/* Device pointers on the current device; enqueued on `hip_stream` (NULL = default stream) and nothing else: no host
 * round trip, no allocation, no synchronisation.  The call a query loop puts in front of dpq_query_batch_device*. */
int dpq_rotate_device(const float* d_vectors, int64_t n, int D, const float* d_R, float* d_out, void* hip_stream);
/* Host buffers: vectors float [n][D], codes uint8 [n][M], codewords float [M][K][Ds]; C_out double [D][D]. */
int dpq_cross_covariance(const float* vectors, int64_t n, int D, const uint8_t* codes, const float* codewords, int M, int K,
                         int Ds, int device, double* C_out);
int dpq_procrustes(const double* C, int D, double* R_out, int32_t* degenerate);
/* rotation: float [D][D], in (use_initial_rotation) and out; codewords: float [M][K][D / M] out; stats may be NULL. */
int dpq_opq_train(const float* vectors, int64_t n, int D, int M, int K, const dpq_opq_opts* opts, float* rotation,
                  float* codewords, dpq_opq_stats* stats);
/* The rotation file: the .fvecs layout, D rows of (int32 D, D floats), so dpq_read_vecs reads it too.  By convention
 * M{M}K{K}rotation.fvecs beside M{M}K{K}codewords.txt.  dpq_read_rotation: out == NULL only reports *D; a file that is
 * truncated, not square or above D = 1024 is DPQ_ERR_FORMAT. */
int dpq_write_rotation(const char* path, const float* R, int D);
int dpq_read_rotation(const char* path, int32_t* D, float* out);

/* ---- search by distance tables, and inner product -------------------------------
 * Every search above builds, per query, M tables T[m][k] = |q_m - c[m][k]|^2 and from there on reads nothing but
 * those tables.  These calls take the tables from the caller instead: tables[nq][M][K], fp32, row-major, M and K the
 * handle's.
 *   Relation to the query forms   The answer is what dpq_query_batch[_filtered] / dpq_range_search give, with
 *           tables[q][m][k] standing where the L2 rule's T[m][k] of query q stands: the distance of a code is the
 *           fp64 sum of its M fp32 entries rounded once to fp32 (a dpq_open_plain_* handle: fp32 accumulation in
 *           ascending m), results are ordered by (distance bits, id), and ids, padding, shards, parts, prefixes, the
 *           even-N id, DPQ_ERR_TOPK and the sub-batches of 2048 queries are those of the query forms.
 *   No codebook   The calls work before dpq_set_codebook.  A handle with a codebook uses its centroid neighbour lists
 *           as they are: they only decide which cells the threshold bootstrap walks first; every threshold comes
 *           from nodes evaluated with the caller's tables, so the answer does not depend on them.
 *   Entries   A finite value >= 0 or +inf is an ordinary value; -0.0 is read as +0.0.  A negative entry, -inf or a NaN
 *           is DPQ_ERR_ARG: the host forms check every entry on the host before any device work; the device form
 *           raises one flag word that comes back with the call's closing synchronisation, and its outputs are then
 *           unspecified.  No kernel behind the ingest ever sees such an entry (it reads +inf in its place).
 *   Exact tables   Call a query's table exact when its finite non-zero entries are whole multiples of one power of two
 *           2^g and its per-sub-space maxima add up to less than 2^53 * 2^g.  Every fp64 sum of M entries is then exact
 *           in any order and the answer is defined to the bit on every scan path.  For other tables a distance is the
 *           fp32 rounding of an fp64 sum of the entries in an order the scan path chooses (what L2 tables get too).
 *           Sufficient: at M = 8, finite non-zero fp32 entries within a factor 2^26 of each other; 2^25 at M = 16.
 *   Calling conventions   Synchronous; pending asynchronous batches are finished first; plans, workspaces and results
 *           of later calls are unaffected.  The host forms stage one sub-batch of tables on the device, at most
 *           2048 * M * K * 4 bytes, kept until dpq_close.  filter may be NULL.  The asynchronous, ordered, host-async
 *           and refined pipelines have no tables form. */
int dpq_query_batch_tables(dpq_index* idx, const dpq_filter* filter, const float* tables, int nq, int top_k,
                           int32_t* ids, float* dists);
/* Device pointers on the handle's GPU, on `hip_stream` (NULL = default stream); returns with the results complete. */
int dpq_query_batch_device_tables(dpq_index* idx, const dpq_filter* filter, const float* d_tables, int nq, int top_k,
                                  int32_t* d_ids, float* d_dists, void* hip_stream);
int dpq_range_search_tables(dpq_index* idx, const float* tables, int nq, const float* radii, dpq_range_result** out);

/* Inner-product search (FAISS's METRIC_INNER_PRODUCT over PQ codes) on top of the table search.  NO REFERENCE
 * SEMANTICS: the rules are this build's own, restated in tests/_tables_restatement.py and met by the GPU bit for bit.
 * With the handle's M, K, Ds, its codebook c and a query q[M * Ds]:
 *   Dot product   p[m][k] = (float)acc: acc = +0.0 in fp64; for d = 0 .. Ds-1 ascending
 *           acc = acc + (double)q[m * Ds + d] * (double)c[m][k][d] (the product of two fp32 values is exact in fp64, so a
 *           fused multiply-add gives the same bits: the rotation rule of the OPQ section).
 *   Maximum   top[m] = the largest p[m][k] over k < K.
 *   Table entry   e[m][k] = top[m] - p[m][k], one fp32 subtraction: >= +0, and +0 at every maximum.
 *   Bias   B = (float) of the fp64 sum from +0.0, m ascending, of (double)top[m].
 *   Gap   g of a code = dpq_query_batch_tables' distance under the table e.  Results are ordered by (g bits, id): by
 *           descending approximate inner product, the lowest ids first among equals.
 *   Score   s = (float)((double)B - (double)g).  A padding row is id -1, gap +inf, score -inf.
 *   Inputs   finite queries and codewords with finite dot products; anything else is out of scope (the search forms
 *           return DPQ_ERR_ARG where a NaN reaches a table).
 * B depends on the query and the codebook only: shards merge their (ids, gaps) with dpq_merge_topk_* unchanged and
 * convert once with dpq_ip_scores.  s is the usual ADC inner product sum_m <q_m, c_m> to within the roundings named; an
 * orthogonal OPQ rotation leaves it alone (rotate the queries first).  The search forms keep one sub-batch of tables
 * (the buffer of the table forms, at most 2048 * M * K * 4 bytes) and, where the caller passes none, their gaps and
 * biases with the handle until dpq_close. */
/* Needs dpq_set_codebook (else DPQ_ERR_STATE).  tables_out[nq][M][K], bias_out[nq]. */
int dpq_ip_tables(dpq_index* idx, const float* queries, int nq, float* tables_out, float* bias_out);
/* Enqueue only: no allocation, no synchronisation (dpq_rotate_device's convention). */
int dpq_ip_tables_device(dpq_index* idx, const float* d_queries, int nq, float* d_tables, float* d_bias, void* hip_stream);
/* scores[nq][top_k] descending; gaps_out [nq][top_k] and bias_out [nq] may be NULL.  filter may be NULL. */
int dpq_query_batch_ip(dpq_index* idx, const dpq_filter* filter, const float* queries, int nq, int top_k, int32_t* ids,
                       float* scores, float* gaps_out, float* bias_out);
int dpq_query_batch_device_ip(dpq_index* idx, const dpq_filter* filter, const float* d_queries, int nq, int top_k,
                              int32_t* d_ids, float* d_scores, float* d_gaps, float* d_bias, void* hip_stream);
/* Host only, no device: scores from merged gaps (shards).  A negative id gives -inf. */
int dpq_ip_scores(const float* bias, const float* gaps, const int32_t* ids, int nq, int top_k, float* scores_out);

/* ---- candidate search: PQ distances and top-k over each query's own ids ---------
 * Every search above runs over the whole handle, or over one filter shared by the whole batch.  These calls take, per
 * query, the list of ids that matter for THAT query -- what a graph or inverted-list traversal hands over, the allowed
 * rows of one tenant of a mixed batch, the hits of a text retriever, the lists of dpq_range_search or of another handle
 * -- and answer with their PQ distances (the _distances forms) or the best top_k of them (the _search forms).  Beside
 * dpq_flat_rerank* (raw rows) and dpq_refine_rerank* (two-level reconstructions) this is the plain one-level ranker: it
 * needs nothing but the index.  cand_ids is [nq][n_cand], row-major; ragged lists are padded to n_cand with -1.
 *   Distance   of candidate c for query q: to the bit what dpq_query_batch reports for id c on this handle.  With T the
 *           query's exact table (the L2 rule of every search, or the caller's tables[q] under the rules of "search by
 *           distance tables": M and K the handle's, columns K .. 255 at +inf) and code the node's M bytes: on a DTC
 *           handle (float) of the fp64 sum, m ascending, of the fp32 entries T[m][code[m]]; on a dpq_open_plain_* handle
 *           `float dist += T[m][code[m]]`, m ascending, M roundings.  +inf is an ordinary value; NaN inputs are out of
 *           scope.  tests/_candidates_restatement.py restates the rules in numpy; the GPU meets them bit for bit.
 *   Ids     A candidate is a reported id, exactly as dpq_query_batch reports it: a global DFS position, with the even-N
 *           rule (on a DTC index of even N the id N names position N - 1).  A negative candidate is padding.  A
 *           candidate that names a node of the index but not of this handle -- another shard's: its position lies in
 *           [0, n_codes_total) outside [node_lo, node_hi) -- is skipped like padding, so every shard can be handed the
 *           same lists and the partial answers merge with dpq_merge_topk_* unchanged.  A candidate that names no node of
 *           the whole index (beyond N; N - 1 on an even-N DTC index; N on a plain one) is DPQ_ERR_ARG: the host forms
 *           check on the host before any device work, the device forms raise a flag word that is read back once at the
 *           end of the call (their outputs are then unspecified).
 *   Search  The best top_k valid candidates by key `distance bits << 32 | id`, ascending; the reported id is the
 *           candidate itself; a node named twice by one query counts once; rows are padded with -1 / +inf when fewer
 *           than top_k candidates are valid.  1 <= top_k <= n_cand <= 16384 (else DPQ_ERR_ARG).
 *   Distances   dists[q][j] is the distance of cand_ids[q][j], in place; padding and skipped entries get a quiet NaN.
 *           1 <= n_cand <= 16384.
 *   Tables  A table entry that is negative, -inf or a NaN is DPQ_ERR_ARG, as in dpq_query_batch_tables: checked on the
 *           host by the host form, by a flag word in the device form.  The _tables forms work before dpq_set_codebook;
 *           the query forms are DPQ_ERR_STATE there.  Inner product composes: dpq_ip_tables, then
 *           dpq_candidate_search_tables (the distances are gaps), then dpq_ip_scores.
 *   State   Handles of M = 8 and M = 16 (what the code lookup decodes).  nq == 0 is DPQ_OK and writes nothing.  All
 *           forms are synchronous and finish pending asynchronous batches first; the device forms enqueue on
 *           `hip_stream` (NULL = default stream) and return with the results complete (dpq_refine_rerank_device's
 *           conventions).  The calls work in buffers of their own, kept with the handle until dpq_close -- one slice of
 *           at most 2^20 candidates of at most 2048 queries: their tables (M KB a query), M bytes of code and 8 bytes
 *           of key a candidate -- and never write into a search lane's workspace: dpq_query_batch before and after
 *           gives the same answer.  The host forms also keep their staging of a whole call.  Argument checks that need
 *           no device come first. */
int dpq_candidate_search(dpq_index* idx, const float* queries, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                         int32_t* ids, float* dists);
int dpq_candidate_search_device(dpq_index* idx, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);
/* tables[nq][M][K] standing where the queries' L2 tables stand. */
int dpq_candidate_search_tables(dpq_index* idx, const float* tables, int nq, const int32_t* cand_ids, int n_cand, int top_k,
                                int32_t* ids, float* dists);
int dpq_candidate_search_device_tables(dpq_index* idx, const float* d_tables, int nq, const int32_t* d_cand_ids, int n_cand,
                                       int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);
/* dists[nq][n_cand]. */
int dpq_candidate_distances(dpq_index* idx, const float* queries, int nq, const int32_t* cand_ids, int n_cand, float* dists);
int dpq_candidate_distances_device(dpq_index* idx, const float* d_queries, int nq, const int32_t* d_cand_ids, int n_cand,
                                   float* d_dists, void* hip_stream);

/* ---- IVF search: inverted lists over the index, probed per query -----------------
 * FAISS's IndexIVFPQ with by_residual = false.  NO REFERENCE COUNTERPART.  A dpq_ivf holds nlist lists over the nodes of
 * ONE dpq_index; a query scans only the lists it probes, so it touches a fraction of the handle.  The answer is a
 * shortlist like any other: dpq_refine_rerank*, dpq_flat_rerank* and dpq_candidate_search* re-rank it unchanged.
 *   Ownership  The structure is bound to the handle it was made on, is freed (dpq_ivf_free) BEFORE dpq_close of that
 *           handle, and is used from the handle's thread.  Handles of M = 8 and M = 16, DTC and dpq_open_plain_*.
 *   Memory  Device memory of its own: offsets[nlist + 1] int64; ids[n_assigned] int32, the REPORTED ids of the listed
 *           nodes -- global DFS positions (shards, parts with global_offset, num_codes prefixes), the even-N rule applied
 *           -- ascending inside a list; codes[n_assigned][M], the same nodes' plain code values in list order; and,
 *           where set, centroids[nlist][M * Ds].  M + 4 bytes per listed node beside the compressed image.
 *   Labels  dpq_ivf_create[_device]: labels[l] is the list of LOCAL node l (position node_lo + l), n must be node_hi -
 *           node_lo, a negative label puts the node in no list, empty lists are legal, 1 <= nlist <= 65536.  A label >=
 *           nlist is DPQ_ERR_ARG: the host form checks before any device work, the device form raises one flag word read
 *           back at the end (dpq_get_codes_device's convention).  The lists are made on the device: a count per list, an
 *           exclusive scan, a stable sort of (label, position), a gather of the codes from the bulk decode in tiles of at
 *           most 4 Mi nodes.
 *   Centroids  dpq_ivf_build: centroids[nlist][M * Ds] in host memory; a codebook must be set (else DPQ_ERR_STATE); M *
 *           Ds > 2048 is DPQ_ERR_ARG.  The label of a node is the centroid nearest to its RECONSTRUCTION (dpq_reconstruct's
 *           row) under the exact search's arithmetic: per dimension the fp32 difference and its fp32 square, each rounded,
 *           summed in fp64 in dimension order and rounded to fp32; the lowest list wins a tie.  Non-finite rows are
 *           unspecified.  The centroids are kept.  dpq_ivf_set_centroids attaches centroids[nlist][M * Ds] to a structure
 *           made from labels -- for callers who assign by their ORIGINAL vectors (through vec_id), as FAISS does.
 *   Probes  dpq_ivf_search_probes[_device]: probes[nq][nprobe] are list numbers of the caller's choice; a negative entry
 *           is padding; a list named twice by one query counts once; an entry >= nlist is DPQ_ERR_ARG (host form: checked
 *           on the host; device form: a flag word, the outputs then unspecified, the next call works).  dpq_ivf_probe:
 *           the nprobe nearest centroids of each query, ordered by (exact L2 distance, list number) under the arithmetic
 *           above; empty lists are probed like any other; dists_out may be NULL.  dpq_ivf_search[_device] is dpq_ivf_probe
 *           followed by dpq_ivf_search_probes.  Without centroids dpq_ivf_probe and dpq_ivf_search* are DPQ_ERR_STATE.
 *   Answer  For query q: the unfiltered search applied to the union of the probed lists.  Distances are to the bit what
 *           dpq_query_batch reports for the same id on the same handle ("candidate search" above: the fp64 sum rounded
 *           once on a DTC handle, fp32 accumulation on a plain one).  Results ascend by key `distance bits << 32 | id`,
 *           the lowest ids win at the k-th boundary, a real id at +inf comes before padding, rows are padded with -1 /
 *           +inf.  On shards every rank takes the same centroids or probes and its own labels; the partial answers merge
 *           with dpq_merge_topk_* unchanged.
 *   Limits  1 <= top_k <= 2048, 1 <= nprobe <= min(nlist, 1024), else DPQ_ERR_ARG; nq == 0 is DPQ_OK.  Argument errors
 *           that need no device come before any device call.
 *   State   Calls are synchronous (the device forms enqueue on `hip_stream`, NULL = default stream, and return with the
 *           results complete) and finish pending asynchronous batches first.  They work in a workspace owned by the
 *           dpq_ivf -- per slice of at most 2048 queries their tables and the partial answers [nprobe][queries][top_k],
 *           at most 256 MB -- and never write a search lane's workspace, tables included.
 * tests/_ivf_restatement.py restates the rules in numpy; the GPU meets them bit for bit. */
typedef struct dpq_ivf dpq_ivf;
typedef struct dpq_ivf_stats {
    int64_t n_assigned;    /* nodes in a list */
    int64_t n_unassigned;  /* nodes with a negative label */
    int64_t max_list_len;
    int64_t device_bytes;  /* offsets, ids, codes and centroids (the workspace of the searches is not counted) */
    int32_t nlist;
    int32_t has_centroids;
} dpq_ivf_stats;
int dpq_ivf_create(dpq_index* idx, const int32_t* labels, int64_t n, int nlist, dpq_ivf** out);
int dpq_ivf_create_device(dpq_index* idx, const int32_t* d_labels, int64_t n, int nlist, void* hip_stream, dpq_ivf** out);
int dpq_ivf_build(dpq_index* idx, const float* centroids, int nlist, dpq_ivf** out);
int dpq_ivf_set_centroids(dpq_ivf* ivf, const float* centroids, int nlist);
void dpq_ivf_free(dpq_ivf* ivf); /* NULL: nothing happens */
int dpq_ivf_get_info(const dpq_ivf* ivf, dpq_ivf_stats* out);
/* offsets_out[nlist + 1], ids_out[n_assigned] (may be NULL: the offsets only). */
int dpq_ivf_get(const dpq_ivf* ivf, int64_t* offsets_out, int32_t* ids_out);
int dpq_ivf_search_probes(dpq_ivf* ivf, const float* queries, int nq, const int32_t* probes, int nprobe, int top_k,
                          int32_t* ids, float* dists);
int dpq_ivf_search_probes_device(dpq_ivf* ivf, const float* d_queries, int nq, const int32_t* d_probes, int nprobe, int top_k,
                                 int32_t* d_ids, float* d_dists, void* hip_stream);
/* lists_out[nq][nprobe], dists_out[nq][nprobe]. */
int dpq_ivf_probe(dpq_ivf* ivf, const float* queries, int nq, int nprobe, int32_t* lists_out, float* dists_out);
int dpq_ivf_search(dpq_ivf* ivf, const float* queries, int nq, int nprobe, int top_k, int32_t* ids, float* dists);
int dpq_ivf_search_device(dpq_ivf* ivf, const float* d_queries, int nq, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
                          void* hip_stream);

/* ---- IVF search: filters, caller tables, inner product and range search ----------
 * FAISS's IDSelector, METRIC_INNER_PRODUCT and range_search on an IndexIVFPQ.  NO REFERENCE COUNTERPART.  For a query q
 * let U(q) be the set of nodes in the lists it probes (probe handling is dpq_ivf_search_probes' rule: negative entries
 * are padding, a list named twice counts once, an entry >= nlist is DPQ_ERR_ARG).  Every call below is an existing
 * exhaustive call applied to U(q) instead of to the whole handle.
 *   Filter  A node of U(q) is eligible iff dpq_query_batch_filtered would find it eligible under the same dpq_filter:
 *           by REPORTED id r, r < n_bits and bit r set; the even-N rule applies (bit N governs the last node of an even-N
 *           DTC index, bit N - 1 governs nothing); global ids on shards, parts and prefixes.  The answer is the IVF answer
 *           over the eligible nodes: the same distance bits, order by key `distance bits << 32 | id`, padding -1 / +inf.
 *           No eligible node gives an all-padding row and is no error.  One filter per call.  A NULL filter in the
 *           _filtered forms, or a filter whose owner is not the IVF's handle, is DPQ_ERR_ARG before any device work; in
 *           the tables, inner-product and range forms `filter` may be NULL.
 *   Tables  tables[nq][M][K] stand where the L2 tables stand, under dpq_candidate_search_tables' entry rules: negative,
 *           -inf or NaN is DPQ_ERR_ARG (host check in the host form, a flag word read back at the end in the device form,
 *           the outputs then unspecified, the next call works); -0.0 is read as +0.0; columns K .. 255 are +inf.  The forms
 *           work before dpq_set_codebook.  The distance is the candidate search's: the fp64 sum in ascending m rounded
 *           once on a DTC handle, fp32 accumulation on a plain one.  There are no queries, hence no coarse step: these
 *           forms take the caller's probes only.
 *   Inner product  dpq_ip_tables, then the tables form, then dpq_ip_scores: ids, scores descending, optional gaps and
 *           bias as dpq_query_batch_ip gives them (gaps / bias may be NULL); padding is -1, gap +inf, score -inf.
 *           dpq_ivf_probe_ip: the nprobe centroids of largest EXACT inner product with each query under
 *           dpq_flat_search_ip's arithmetic and order -- score descending, list number ascending -- and their scores
 *           (scores_out may be NULL); what FAISS does with an inner-product quantiser.  dpq_ivf_search[_device]_ip is
 *           dpq_ivf_probe_ip followed by dpq_ivf_search_probes[_device]_ip; a caller who wants the L2 coarse step calls
 *           dpq_ivf_probe and passes its rows.
 *   Range   radii[nq] follow dpq_range_search's rules to the letter: d < r strictly; r <= 0 gives an empty list; r = +inf
 *           gives every eligible node of U(q), those at +inf included; a NaN radius is DPQ_ERR_ARG before any device
 *           work.  The answer is a dpq_range_result (host-owned; dpq_range_result_get, dpq_range_result_free); each list
 *           ascends by (distance bits, id).  Host forms only, as dpq_range_search is.  Two passes over the probed lists,
 *           count then emit, per slice of at most 2048 queries; the keys of a group of queries are laid out, sorted and
 *           brought down through a pool of at most 2 x 64 MB kept with the dpq_ivf; one query whose list alone exceeds
 *           the pool works in buffers of the call, released before it returns.
 *   Everything else -- the limits of top_k and nprobe, nq == 0, synchronous calls that finish pending asynchronous
 *           batches, the workspace owned by the dpq_ivf, never writing a search lane's workspace, argument checks that
 *           need no device first -- is as in "IVF search" above.  Partial answers of shards merge with dpq_merge_topk_*
 *           (inner product: the _ip merges); range lists of shards merge on the host by (distance, id).
 * tests/_ivf_modes_restatement.py restates the rules in numpy; the GPU meets them bit for bit. */
int dpq_ivf_search_filtered(dpq_ivf* ivf, const dpq_filter* filter, const float* queries, int nq, int nprobe, int top_k,
                            int32_t* ids, float* dists);
int dpq_ivf_search_device_filtered(dpq_ivf* ivf, const dpq_filter* filter, const float* d_queries, int nq, int nprobe,
                                   int top_k, int32_t* d_ids, float* d_dists, void* hip_stream);
int dpq_ivf_search_probes_filtered(dpq_ivf* ivf, const dpq_filter* filter, const float* queries, int nq,
                                   const int32_t* probes, int nprobe, int top_k, int32_t* ids, float* dists);
int dpq_ivf_search_probes_device_filtered(dpq_ivf* ivf, const dpq_filter* filter, const float* d_queries, int nq,
                                          const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
                                          void* hip_stream);
int dpq_ivf_search_probes_tables(dpq_ivf* ivf, const dpq_filter* filter, const float* tables, int nq, const int32_t* probes,
                                 int nprobe, int top_k, int32_t* ids, float* dists);
int dpq_ivf_search_probes_device_tables(dpq_ivf* ivf, const dpq_filter* filter, const float* d_tables, int nq,
                                        const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_dists,
                                        void* hip_stream);
/* lists_out[nq][nprobe], scores_out[nq][nprobe] (may be NULL). */
int dpq_ivf_probe_ip(dpq_ivf* ivf, const float* queries, int nq, int nprobe, int32_t* lists_out, float* scores_out);
int dpq_ivf_search_ip(dpq_ivf* ivf, const dpq_filter* filter, const float* queries, int nq, int nprobe, int top_k,
                      int32_t* ids, float* scores, float* gaps_out, float* bias_out);
int dpq_ivf_search_device_ip(dpq_ivf* ivf, const dpq_filter* filter, const float* d_queries, int nq, int nprobe, int top_k,
                             int32_t* d_ids, float* d_scores, float* d_gaps, float* d_bias, void* hip_stream);
int dpq_ivf_search_probes_ip(dpq_ivf* ivf, const dpq_filter* filter, const float* queries, int nq, const int32_t* probes,
                             int nprobe, int top_k, int32_t* ids, float* scores, float* gaps_out, float* bias_out);
int dpq_ivf_search_probes_device_ip(dpq_ivf* ivf, const dpq_filter* filter, const float* d_queries, int nq,
                                    const int32_t* d_probes, int nprobe, int top_k, int32_t* d_ids, float* d_scores,
                                    float* d_gaps, float* d_bias, void* hip_stream);
int dpq_ivf_range_search(dpq_ivf* ivf, const dpq_filter* filter, const float* queries, int nq, int nprobe,
                         const float* radii, dpq_range_result** out);
int dpq_ivf_range_search_probes(dpq_ivf* ivf, const dpq_filter* filter, const float* queries, int nq, const int32_t* probes,
                                int nprobe, const float* radii, dpq_range_result** out);

/* ---- IVF training: the coarse quantiser's centroids, learned and applied on the GPU ---
 * FAISS's IndexIVF::train and quantizer->assign.  NO REFERENCE COUNTERPART.  One codebook over the WHOLE vector, nlist up
 * to 65536: what dpq_ivf_build and dpq_ivf_set_centroids take, and what dpq_train_codebook (a codebook per sub-space,
 * K <= 256) cannot give.  With vectors v[n][D] and centroids c[nlist][D], both fp32:
 *   Distance  the exact search's arithmetic, which dpq_ivf_build and dpq_ivf_probe use, so a trained set is consistent
 *           with the labels and probes an IVF makes from it: an fp64 acc starts at +0.0; for d ascending t = c[d] - v[d]
 *           in fp32, s = t * t in fp32, each rounded on its own, acc += (double)s; the distance is (float)acc.  This is
 *           NOT dpq_train_codebook's fp32 accumulation.
 *   Assign  the label of a vector is the list with the smallest key `distance bits << 32 | list`: the lowest list wins a
 *           tie.  The winning distance is the distance to that list.  +inf is an ordinary value: if every distance is
 *           +inf the label is 0.  NaN inputs are unspecified.
 *   Start   use_initial != 0: the caller's centroids.  Otherwise dpq_train_codebook's "rows" start with K = nlist (the
 *           splitmix64 partial shuffle of "codebook learning" above): centroid i is vector p[i].
 *   Stop    right after an assignment (not the first) that changes no label and leaves no list empty: the centroids
 *           already are the means of those labels.  Otherwise after max_iters rounds.
 *   Update  list with members: per dimension the fp64 sum, starting from +0.0, of the members' fp32 values in ascending
 *           vector index, one add after the other, divided in fp64 by (double)count, rounded once to fp32.
 *   Empty   with E empty lists after an assignment, the vectors are ranked by (winning distance descending, vector index
 *           ascending); the j-th empty list in ascending order takes the j-th ranked vector.  The donor stays in its old
 *           list's mean of this round.
 *   Distortion  per round the fp64 sum of the winning fp32 distances; the order of that sum is not part of the contract,
 *           but the same input gives the same bits run to run.
 * The same input gives the same centroid bytes, run to run.  tests/_ivf_train_restatement.py restates the rules in
 * numpy; the GPU meets them bit for bit.  opts == NULL: device 0, 25 rounds, seed 0.
 *   Limits  DPQ_ERR_ARG, before any device call: a NULL pointer (stats and dists_out may be NULL), D outside 1..2048,
 *           nlist outside 1..65536, n outside 1..2^31 - 1 (dpq_ivf_assign*: n == 0 is DPQ_OK), and for dpq_ivf_train
 *           nlist > n, max_iters outside 1..64, a non-zero reserved word.  Without a GPU: DPQ_ERR_NO_DEVICE.
 *   Memory  dpq_ivf_train holds on the device 4 * n * Dp bytes of rows (Dp = D rounded up to 4), 24 * n bytes of labels,
 *           winning distances and sort arrays, 4 * nlist * Dp of centroids and the sorts' scratch; dpq_ivf_assign works in
 *           tiles of at most 256 MB of rows.  A failed allocation is DPQ_ERR_NOMEM; everything is freed before the call
 *           returns.  dpq_ivf_assign_device allocates nothing. */
typedef struct dpq_ivf_train_opts {
    int32_t device;
    int32_t max_iters;   /* 1..64 */
    uint64_t seed;       /* of the seeded start */
    int32_t use_initial; /* != 0: `centroids` holds the start on entry */
    int32_t reserved[3]; /* 0 */
} dpq_ivf_train_opts;

typedef struct dpq_ivf_train_stats {
    int32_t iters_run;     /* rounds run = entries of distortion[] */
    int32_t converged;     /* 1: stopped by the rule */
    int64_t reseeded;      /* empty lists repaired, all rounds */
    double distortion[64]; /* per round */
    double gpu_ms;         /* assign_ms + update_ms + repair_ms (device events) */
    double wall_ms;        /* the whole call, upload included */
    double rounds_ms;      /* host clock around the rounds; minus gpu_ms = the host round trips */
    double assign_ms, update_ms, repair_ms; /* assign: the arg-min; update: lists, distortion and means */
} dpq_ivf_train_stats;

/* vectors [n][D] host; centroids [nlist][D] host, in (use_initial) and out.  stats may be NULL. */
int dpq_ivf_train(const float* vectors, int64_t n, int D, int nlist, const dpq_ivf_train_opts* opts, float* centroids,
                  dpq_ivf_train_stats* stats);
/* Assign alone: labels_out [n] int32, dists_out [n] float (may be NULL); host buffers. */
int dpq_ivf_assign(const float* centroids, int nlist, int D, const float* vectors, int64_t n, int device, int32_t* labels_out,
                   float* dists_out);
/* Device pointers on the current device, enqueue only: no allocation, no synchronisation (dpq_rotate_device's
 * convention); d_dists may be NULL.  Needs D % 4 == 0 and 16-byte aligned rows, else DPQ_ERR_ARG. */
int dpq_ivf_assign_device(const float* d_centroids, int nlist, int D, const float* d_vectors, int64_t n, int32_t* d_labels,
                          float* d_dists, void* hip_stream);
/* Host only: n rows of (int32 D, D floats), the .fvecs layout dpq_read_vecs reads. */
int dpq_write_vecs(const char* path, const float* vectors, int64_t n, int D);

/* ---- measurement -------------------------------------------------------- */
int dpq_profile_enable(dpq_index* idx, int on);  /* 0 off, 1 every kernel, 2 scan launches only (less event overhead) */
int dpq_profile_reset(dpq_index* idx);
int dpq_profile_read(dpq_index* idx, dpq_profile* out);

/* ---- developer diagnostics ----------------------------------------------
 * Not part of the drop-in boundary: timing and instrumentation hooks used by scripts/ (limiter studies, kernel
 * section marks).  They return DPQ_ERR_STATE unless the process was started with DPQ_DEV=1 in its environment, and
 * only then read their own DPQ_DEBUG_* variables.  A query call never goes through them. */
/* `reps` filter-scan launches over the whole shard for nq slots of the last batch with the filter pinned (pass_all 0:
 * nothing survives, 1: everything, 2: the batch's thresholds, 3: the last batch's bootstrap + first level as they ran). */
int dpq_debug_scan_time(dpq_index* idx, int nq, int pass_all, int reps, int splits, float* ms_out);
/* One launch of the STAMPS build of the scan kernel (M = 8): per-section cycle sums over all wavefronts. */
int dpq_debug_scan_stamps(dpq_index* idx, int nq, int splits, unsigned long long* out, int n_out, float* ms_out);
/* Phase marks of the bootstrap and the last select launch (first call arms them). */
int dpq_debug_boot_stamps(dpq_index* idx, int nq, double* out);
/* The level-0 select alone (shards without a bootstrap). */
int dpq_debug_select_time(dpq_index* idx, int nq, int top_k, int flags, int reps, float* ms_out);
/* Candidate keys the largest scan launch of the last dpq_range_search laid out (its live slots x regions). */
int dpq_debug_range_keys(dpq_index* idx, int64_t* max_keys);
/* Per-wavefront marks of strand1_kernel on the 100 MHz clock, [256][16][16] words (first call arms them). */
int dpq_debug_strand1_stamps(dpq_index* idx, unsigned long long* out, int n_words);
/* The first filter level's tables of the last batch answered on `lane` (0 or 1), in the scan's LDS layout
 * ([query group][g][m][code] x 16 bytes), followed at M = 8 by one 16-byte record per slot: the eight saturation bytes a
 * table builder gives the slot and the u64 threshold key its fields were built from (recomputed by the hook; the batch
 * itself must have run with DPQ_DEV=1).  DPQ_ERR_STATE unless that batch ran exactly one filter level. */
int dpq_debug_filter_tables(dpq_index* idx, int lane, void* out, int64_t bytes);
/* The code value -> label map [M][256] of the plain-code scratch, in whose label order the rows of a scratch batch's
 * filter tables stand.  DPQ_ERR_STATE: the handle has none (labels are code values). */
int dpq_debug_relabel(dpq_index* idx, unsigned char* out, int bytes);

#ifdef __cplusplus
}
#endif
#endif /* DELTAPQ_AMD_H */
