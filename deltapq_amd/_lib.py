"""ctypes binding of include/deltapq_amd.h (deltapq_amd/csrc/libdeltapq_amd.so).

The library is the product: if it is missing this module raises ImportError --
there is no Python or CPU implementation of the query path to fall back to.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPQ_LIB_PATH") or os.path.join(_HERE, "csrc", "libdeltapq_amd.so")   # DPQ_LIB_PATH: developer A/B builds

c_i32, c_i64, c_f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
P = ctypes.POINTER


class OpenOpts(ctypes.Structure):
    _fields_ = [("device", c_i32), ("shard_rank", c_i32), ("shard_count", c_i32), ("chunks_per_segment", c_i32),
                ("cand_capacity", c_i32), ("num_codes", c_i32), ("bootstrap", c_i32), ("batch_decode", c_i32),
                ("global_offset", c_i64), ("global_n_codes", c_i64),
                # plan and tiling knobs (0 = measured default), see include/deltapq_amd.h
                ("stream_max_queries", c_i32), ("coarse_below", c_i32), ("plan_ratios", c_i32 * 3), ("boot_cap", c_i32),
                ("boot_target", c_i32), ("flags", c_i32), ("batch_tile_nodes", c_i64)]


class Info(ctypes.Structure):
    _fields_ = [("n_codes_total", c_i64), ("n_bytes_total", c_i64), ("node_lo", c_i64), ("node_hi", c_i64),
                ("algorithmic_bytes", c_i64), ("device_bytes", c_i64), ("n_diffs", c_i64), ("M", c_i32),
                ("K", c_i32), ("Ds", c_i32), ("n_segments", c_i32), ("chunks_per_segment", c_i32),
                ("max_depth", c_i32), ("device", c_i32), ("cand_capacity", c_i32), ("bootstrap_bytes", c_i64),
                ("bootstrap_stride", c_i32), ("batch_decode_mb", c_i32), ("strand_bytes", c_i64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Profile(ctypes.Structure):
    _fields_ = [("lut_ms", ctypes.c_double), ("scan_ms", ctypes.c_double), ("select_ms", ctypes.c_double),
                ("lut_launches", c_i64), ("scan_launches", c_i64), ("select_launches", c_i64),
                ("scan_node_query_pairs", c_i64), ("scan_stream_bytes", c_i64), ("query_batches", c_i64),
                ("queries", c_i64), ("overflow_reruns", c_i64), ("exact_checks", c_i64), ("candidates", c_i64),
                ("quantise_ms", ctypes.c_double), ("decode_ms", ctypes.c_double), ("bootstrap_ms", ctypes.c_double),
                ("bootstrap_launches", c_i64), ("stream_launches", c_i64), ("strand_launches", c_i64),
                ("strand1_launches", c_i64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DtcStats(ctypes.Structure):
    _fields_ = [("n_codes", c_i64), ("n_bytes", c_i64), ("n_diffs", c_i64), ("depth_hist", c_i64 * 16),
                ("max_depth", c_i32), ("M", c_i32)]


class TrainOpts(ctypes.Structure):
    _fields_ = [("device", c_i32), ("max_iters", c_i32), ("seed", ctypes.c_uint64), ("use_initial", c_i32),
                ("init", c_i32), ("restarts", c_i32), ("reserved", c_i32 * 1)]


class TrainStats(ctypes.Structure):
    _fields_ = [("iters_run", c_i32), ("converged", c_i32), ("reseeded", c_i64), ("distortion", ctypes.c_double * 64),
                ("gpu_ms", ctypes.c_double), ("wall_ms", ctypes.c_double), ("rounds_ms", ctypes.c_double),
                ("assign_ms", ctypes.c_double), ("update_ms", ctypes.c_double), ("repair_ms", ctypes.c_double)]


class RefineOpts(ctypes.Structure):
    _fields_ = [("M2", c_i32), ("K2", c_i32), ("train_n", c_i64), ("max_iters", c_i32), ("init", c_i32),
                ("restarts", c_i32), ("reserved", c_i32), ("seed", ctypes.c_uint64)]


class OpqOpts(ctypes.Structure):
    _fields_ = [("device", c_i32), ("outer_iters", c_i32), ("init_iters", c_i32), ("inner_iters", c_i32),
                ("seed", ctypes.c_uint64), ("init", c_i32), ("restarts", c_i32), ("use_initial_rotation", c_i32),
                ("reserved", c_i32 * 1)]


class OpqStats(ctypes.Structure):
    _fields_ = [("outer_run", c_i32), ("best_t", c_i32), ("degenerate", c_i32), ("reserved", c_i32),
                ("objective", ctypes.c_double * 65), ("rotation_residual", ctypes.c_double * 64),
                ("gpu_ms", ctypes.c_double), ("wall_ms", ctypes.c_double), ("rounds_ms", ctypes.c_double),
                ("assign_ms", ctypes.c_double), ("update_ms", ctypes.c_double), ("repair_ms", ctypes.c_double),
                ("rotate_ms", ctypes.c_double), ("cross_ms", ctypes.c_double), ("procrustes_ms", ctypes.c_double)]


class IvfStats(ctypes.Structure):
    _fields_ = [("n_assigned", c_i64), ("n_unassigned", c_i64), ("max_list_len", c_i64), ("device_bytes", c_i64),
                ("nlist", c_i32), ("has_centroids", c_i32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IvfTrainOpts(ctypes.Structure):
    _fields_ = [("device", c_i32), ("max_iters", c_i32), ("seed", ctypes.c_uint64), ("use_initial", c_i32),
                ("reserved", c_i32 * 3)]


class IvfTrainStats(ctypes.Structure):
    _fields_ = TrainStats._fields_


# every symbol include/deltapq_amd.h declares: (name, restype, argtypes)
_VP = ctypes.c_void_p
SYMBOLS = [
    ("dpq_version", ctypes.c_int, []),
    ("dpq_strerror", ctypes.c_char_p, [ctypes.c_int]),
    ("dpq_last_error", ctypes.c_char_p, []),
    ("dpq_device_count", ctypes.c_int, []),
    ("dpq_read_dtc_header", ctypes.c_int, [ctypes.c_char_p, P(c_i64), P(c_i64)]),
    ("dpq_read_codewords", ctypes.c_int, [ctypes.c_char_p, P(c_i32), P(c_i32), P(c_i32), _VP]),
    ("dpq_read_vecs", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, P(c_i64), P(c_i32), _VP, c_i64]),
    ("dpq_dtc_file_name", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, c_i64, ctypes.c_char_p, c_i64]),
    ("dpq_dtc_validate", ctypes.c_int, [_VP, c_i64, c_i64, ctypes.c_int, P(DtcStats)]),
    ("dpq_soa_build", ctypes.c_int, [_VP, c_i64, c_i64, ctypes.c_int, P(OpenOpts), P(_VP)]),
    ("dpq_soa_info", ctypes.c_int, [_VP, P(Info)]),
    ("dpq_soa_array", ctypes.c_int, [_VP, ctypes.c_int, P(_VP), P(c_i64)]),
    ("dpq_soa_free", None, [_VP]),
    ("dpq_dtc_encode", ctypes.c_int, [_VP, _VP, _VP, _VP, c_i64, ctypes.c_int, _VP, P(c_i64)]),
    ("dpq_dtc_decode", ctypes.c_int, [_VP, c_i64, c_i64, ctypes.c_int, c_i64, c_i64, _VP]),
    ("dpq_tree_build", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_int, P(_VP)]),
    ("dpq_tree_build_gpu", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, P(_VP)]),
    ("dpq_tree_stats", ctypes.c_int, [_VP, P(DtcStats)]),
    ("dpq_tree_array", ctypes.c_int, [_VP, ctypes.c_int, P(_VP), P(c_i64)]),
    ("dpq_tree_encode", ctypes.c_int, [_VP, _VP, P(c_i64)]),
    ("dpq_tree_write_files", ctypes.c_int, [_VP, ctypes.c_char_p]),
    ("dpq_tree_free", None, [_VP]),
    ("dpq_read_qnode_ids", ctypes.c_int, [ctypes.c_char_p, c_i64, _VP]),
    ("dpq_read_codes_plain", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, P(c_i64), _VP]),
    ("dpq_write_codes_plain", ctypes.c_int, [ctypes.c_char_p, _VP, c_i64, ctypes.c_int]),
    ("dpq_read_codes_plain_ex", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(c_i64), _VP, _VP]),
    ("dpq_encode_pq", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP]),
    ("dpq_train_codebook", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(TrainOpts), _VP, P(TrainStats)]),
    ("dpq_kmeanspp_seed", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, _VP, _VP]),
    ("dpq_train_potential", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP]),
    ("dpq_write_codewords", ctypes.c_int, [ctypes.c_char_p, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("dpq_open_plain_memory", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, P(OpenOpts), P(_VP)]),
    ("dpq_open_plain_file", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, P(OpenOpts), P(_VP)]),
    ("dpq_open_file", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, P(OpenOpts), P(_VP)]),
    ("dpq_open_memory", ctypes.c_int, [_VP, c_i64, c_i64, ctypes.c_int, ctypes.c_int, P(OpenOpts), P(_VP)]),
    ("dpq_set_codebook", ctypes.c_int, [_VP, _VP, ctypes.c_int]),
    ("dpq_get_info", ctypes.c_int, [_VP, P(Info)]),
    ("dpq_close", ctypes.c_int, [_VP]),
    ("dpq_query_batch", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_query_batch_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_query_batch_device_async", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_query_batch_device_ordered", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_finish_count", ctypes.c_int, [_VP, P(c_i32)]),
    ("dpq_finish", ctypes.c_int, [_VP]),
    ("dpq_merge_topk_host", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_merge_topk_device", ctypes.c_int,
     [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, _VP]),
    ("dpq_merge_topk_device_packed", ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, _VP]),
    ("dpq_query_batch_host_async", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_pin_host", ctypes.c_int, [_VP, c_i64]),
    ("dpq_unpin_host", ctypes.c_int, [_VP]),
    ("dpq_range_search", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_range_result_get", ctypes.c_int, [_VP, P(c_i32), P(_VP), P(_VP), P(_VP)]),
    ("dpq_range_result_free", None, [_VP]),
    ("dpq_filter_create", ctypes.c_int, [_VP, _VP, c_i64, P(_VP)]),
    ("dpq_filter_free", None, [_VP]),
    ("dpq_filter_count", ctypes.c_int, [_VP, P(c_i64)]),
    ("dpq_query_batch_filtered", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_query_batch_device_filtered", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_filter_create_device", ctypes.c_int, [_VP, _VP, c_i64, _VP, P(_VP)]),
    ("dpq_filter_create_ids", ctypes.c_int, [_VP, _VP, c_i64, ctypes.c_int, P(_VP)]),
    ("dpq_filter_create_ids_device", ctypes.c_int, [_VP, _VP, c_i64, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_filter_create_range", ctypes.c_int, [_VP, c_i64, c_i64, P(_VP)]),
    ("dpq_set_vec_ids", ctypes.c_int, [_VP, _VP, c_i64]),
    ("dpq_filter_create_vec", ctypes.c_int, [_VP, _VP, c_i64, P(_VP)]),
    ("dpq_filter_create_vec_device", ctypes.c_int, [_VP, _VP, c_i64, _VP, P(_VP)]),
    ("dpq_filter_combine", ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, P(_VP)]),
    ("dpq_filter_to_bitmap", ctypes.c_int, [_VP, _VP, c_i64]),
    ("dpq_bitmap_from_mask_device", ctypes.c_int, [_VP, c_i64, _VP, ctypes.c_int, _VP]),
    ("dpq_bitmap_from_ids_device", ctypes.c_int, [_VP, c_i64, c_i64, _VP, ctypes.c_int, _VP]),
    ("dpq_get_codes", ctypes.c_int, [_VP, _VP, c_i64, _VP]),
    ("dpq_get_codes_device", ctypes.c_int, [_VP, _VP, c_i64, _VP, _VP]),
    ("dpq_reconstruct", ctypes.c_int, [_VP, _VP, c_i64, _VP]),
    ("dpq_reconstruct_device", ctypes.c_int, [_VP, _VP, c_i64, _VP, _VP]),
    ("dpq_decode_range", ctypes.c_int, [_VP, c_i64, c_i64, _VP]),
    ("dpq_flat_open", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_flat_close", ctypes.c_int, [_VP]),
    ("dpq_flat_search", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_set_id_map", ctypes.c_int, [_VP, _VP, c_i64]),
    ("dpq_flat_rerank", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_rerank_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_flat_open_u8", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_flat_search_u8", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_rerank_u8", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_rerank_u8_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_flat_filter_create", ctypes.c_int, [_VP, _VP, c_i64, P(_VP)]),
    ("dpq_flat_filter_free", None, [_VP]),
    ("dpq_flat_filter_count", ctypes.c_int, [_VP, P(c_i64)]),
    ("dpq_flat_search_filtered", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_search_filtered_u8", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_range_search", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_flat_range_search_u8", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_flat_search_ip", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_search_filtered_ip", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_range_search_ip", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_flat_rerank_ip", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_rerank_ip_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_merge_topk_ip_host", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_open_i8", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, c_i64, P(_VP)]),
] + [
    # the byte forms of the inner-product calls (u8 handles) and every call of an i8 handle: the argument lists of the
    # fp32 call of the same shape
    ("dpq_flat_%s%s%s" % (shape, suffix, tail), ctypes.c_int, args)
    for suffix in ("_ip_u8", "_i8", "_ip_i8")
    for shape, tail, args in (
        ("search", "", [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
        ("search_filtered", "", [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
        ("range_search", "", [_VP, _VP, _VP, ctypes.c_int, _VP, P(_VP)]),
        ("rerank", "", [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
        ("rerank", "_device", [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]))
] + [
    ("dpq_half_from_float", ctypes.c_int, [_VP, c_i64, ctypes.c_int, _VP]),
    ("dpq_half_to_float", ctypes.c_int, [_VP, c_i64, ctypes.c_int, _VP]),
    ("dpq_flat_open_half", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_flat_open_narrowed", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_sq_train", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_sq_encode", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, _VP]),
    ("dpq_sq_decode", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_flat_open_sq", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_flat_open_quantised", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_flat_sq_get", ctypes.c_int, [_VP, P(ctypes.c_int), _VP, _VP]),
    ("dpq_flat_open_bits", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_bits_from_float", ctypes.c_int, [_VP, c_i64, ctypes.c_int, _VP, ctypes.c_int, _VP]),
    ("dpq_flat_open_binarised", ctypes.c_int, [_VP, c_i64, ctypes.c_int, _VP, ctypes.c_int, c_i64, P(_VP)]),
    ("dpq_flat_search_bits", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_search_filtered_bits", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_range_search_bits", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_flat_rerank_bits", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_flat_rerank_bits_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_range_recall", ctypes.c_int, [ctypes.c_int, _VP, _VP, _VP, _VP, P(ctypes.c_double), P(ctypes.c_double)]),
    ("dpq_bitmap_to_dfs", ctypes.c_int, [_VP, c_i64, _VP, c_i64, _VP]),
    ("dpq_write_bitmap", ctypes.c_int, [ctypes.c_char_p, _VP, c_i64]),
    ("dpq_read_bitmap", ctypes.c_int, [ctypes.c_char_p, P(c_i64), _VP]),
    ("dpq_read_vecs_range", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, c_i64, c_i64, P(c_i32), _VP]),
    ("dpq_read_bvecs_range", ctypes.c_int, [ctypes.c_char_p, c_i64, c_i64, P(c_i32), _VP]),
    ("dpq_write_groundtruth", ctypes.c_int, [ctypes.c_char_p, _VP, _VP, ctypes.c_int, ctypes.c_int]),
    ("dpq_read_groundtruth", ctypes.c_int, [ctypes.c_char_p, P(c_i32), P(c_i32), _VP, _VP]),
    ("dpq_recall", ctypes.c_int,
     [_VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(ctypes.c_double)]),
    ("dpq_residuals", ctypes.c_int, [_VP, _VP, c_i64, _VP, ctypes.c_int, _VP]),
    ("dpq_refine_create", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, c_i64, P(_VP)]),
    ("dpq_refine_free", None, [_VP]),
    ("dpq_refine_get", ctypes.c_int, [_VP, P(c_i32), P(c_i32), P(c_i32), P(c_i64), _VP, _VP]),
    ("dpq_refine_build", ctypes.c_int, [_VP, _VP, c_i64, ctypes.c_int, _VP, P(RefineOpts), P(_VP)]),
    ("dpq_refine_reconstruct", ctypes.c_int, [_VP, _VP, c_i64, _VP]),
    ("dpq_refine_rerank", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_refine_rerank_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_query_batch_refined", ctypes.c_int,
     [_VP, _VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_rotate", ctypes.c_int, [_VP, c_i64, ctypes.c_int, _VP, ctypes.c_int, _VP]),
    ("dpq_rotate_device", ctypes.c_int, [_VP, c_i64, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_cross_covariance", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP]),
    ("dpq_procrustes", ctypes.c_int, [_VP, ctypes.c_int, _VP, P(c_i32)]),
    ("dpq_opq_train", ctypes.c_int,
     [_VP, c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(OpqOpts), _VP, _VP, P(OpqStats)]),
    ("dpq_write_rotation", ctypes.c_int, [ctypes.c_char_p, _VP, ctypes.c_int]),
    ("dpq_read_rotation", ctypes.c_int, [ctypes.c_char_p, P(c_i32), _VP]),
    ("dpq_query_batch_tables", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_query_batch_device_tables", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_range_search_tables", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_ip_tables", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, _VP]),
    ("dpq_ip_tables_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_query_batch_ip", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP]),
    ("dpq_query_batch_device_ip", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP, _VP]),
    ("dpq_ip_scores", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP]),
    ("dpq_candidate_search", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_candidate_search_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_candidate_search_tables", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_candidate_search_device_tables", ctypes.c_int,
     [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_candidate_distances", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, _VP]),
    ("dpq_candidate_distances_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_create", ctypes.c_int, [_VP, _VP, c_i64, ctypes.c_int, P(_VP)]),
    ("dpq_ivf_create_device", ctypes.c_int, [_VP, _VP, c_i64, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_ivf_build", ctypes.c_int, [_VP, _VP, ctypes.c_int, P(_VP)]),
    ("dpq_ivf_set_centroids", ctypes.c_int, [_VP, _VP, ctypes.c_int]),
    ("dpq_ivf_free", None, [_VP]),
    ("dpq_ivf_get_info", ctypes.c_int, [_VP, P(IvfStats)]),
    ("dpq_ivf_get", ctypes.c_int, [_VP, _VP, _VP]),
    ("dpq_ivf_search_probes", ctypes.c_int, [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search_probes_device", ctypes.c_int,
     [_VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_ivf_probe", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search_device", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_ivf_search_filtered", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search_device_filtered", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_ivf_search_probes_filtered", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search_probes_device_filtered", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_ivf_search_probes_tables", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search_probes_device_tables", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    ("dpq_ivf_probe_ip", ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_search_ip", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP]),
    ("dpq_ivf_search_device_ip", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP, _VP]),
    ("dpq_ivf_search_probes_ip", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP]),
    ("dpq_ivf_search_probes_device_ip", ctypes.c_int,
     [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, _VP, _VP]),
    ("dpq_ivf_range_search", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_ivf_range_search_probes", ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, ctypes.c_int, _VP, P(_VP)]),
    ("dpq_ivf_train", ctypes.c_int, [_VP, c_i64, ctypes.c_int, ctypes.c_int, P(IvfTrainOpts), _VP, P(IvfTrainStats)]),
    ("dpq_ivf_assign", ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, c_i64, ctypes.c_int, _VP, _VP]),
    ("dpq_ivf_assign_device", ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, c_i64, _VP, _VP, _VP]),
    ("dpq_write_vecs", ctypes.c_int, [ctypes.c_char_p, _VP, c_i64, ctypes.c_int]),
    ("dpq_profile_enable", ctypes.c_int, [_VP, ctypes.c_int]),
    ("dpq_profile_reset", ctypes.c_int, [_VP]),
    ("dpq_profile_read", ctypes.c_int, [_VP, P(Profile)]),
    # developer diagnostics (DPQ_DEV=1 only; scripts/)
    ("dpq_debug_scan_time", ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(ctypes.c_float)]),
    ("dpq_debug_scan_stamps", ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, P(ctypes.c_ulonglong), ctypes.c_int, P(ctypes.c_float)]),
    ("dpq_debug_boot_stamps", ctypes.c_int, [_VP, ctypes.c_int, P(ctypes.c_double)]),
    ("dpq_debug_select_time", ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(ctypes.c_float)]),
    ("dpq_debug_strand1_stamps", ctypes.c_int, [_VP, _VP, ctypes.c_int]),
    ("dpq_debug_range_keys", ctypes.c_int, [_VP, P(c_i64)]),
    ("dpq_debug_filter_tables", ctypes.c_int, [_VP, ctypes.c_int, _VP, c_i64]),
    ("dpq_debug_relabel", ctypes.c_int, [_VP, _VP, ctypes.c_int]),
]

_lib = None
_hip_runtime = None


def _bind_hip_runtime():
    """Load THE HIP runtime of this process with RTLD_GLOBAL before the C-ABI
    library (which is built with -no-hip-rt and resolves hip* against it).
    A process must not mix two runtimes: PyTorch-ROCm wheels bundle their own
    libamdhip64.so, so when torch is installed we bind to that one (whether or
    not torch has been imported yet); otherwise to /opt/rocm's."""
    global _hip_runtime
    if _hip_runtime is not None:
        return _hip_runtime
    import importlib.util
    candidates = []
    override = os.environ.get("DPQ_HIP_RUNTIME")
    if override:
        candidates.append(override)
    try:
        spec = importlib.util.find_spec("torch")
        if spec is not None and spec.submodule_search_locations:
            candidates.append(os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so"))
    except (ImportError, ValueError):
        pass
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    candidates += [os.path.join(rocm, "lib", "libamdhip64.so"), "libamdhip64.so"]
    last = None
    for path in candidates:
        if os.path.isabs(path) and not os.path.exists(path):
            continue
        try:
            _hip_runtime = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            return _hip_runtime
        except OSError as e:
            last = e
    raise ImportError("cannot load a HIP runtime (libamdhip64.so): %s" % last)


def load():
    """Load the C-ABI library, binding every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `make -C deltapq_amd/csrc` (or __graft_entry__.build()); "
            "the DeltaPQ query path has no CPU fallback" % LIB_PATH)
    _bind_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


class DpqError(RuntimeError):
    def __init__(self, status, where):
        lib = load()
        self.status = status
        detail = lib.dpq_last_error().decode(errors="replace")
        super().__init__("%s failed: %s (%d)%s" % (where, lib.dpq_strerror(status).decode(), status,
                                                  ": " + detail if detail else ""))


def check(status, where):
    if status != 0:
        raise DpqError(status, where)
