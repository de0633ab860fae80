"""ctypes binding of liblemon_hip.so (include/lemon_hip.h).

The product path has NO CPU fallback: if the library is missing or a call fails, we raise.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "liblemon_hip.so")

METRIC_IP = 0
METRIC_L2 = 1
MAX_K = 64            # per scan pass and in lemon_neighbors
KSWEEP_MAX_KS = 16   # LEMON_KSWEEP_MAX_KS: values of k per lemon_grid_f1_ks call
MAX_K_DEEP = 2048     # lemon_index_search (passes of MAX_K, include/lemon_hip.h)
ATTENTION_MAX_SEQ = 4096   # LEMON_ATTENTION_MAX_SEQ (include/lemon_hip.h)
ALGO_AUTO, ALGO_F32_MFMA, ALGO_BF16_FILTER = 0, 1, 2

# every symbol include/lemon_hip.h declares
EXPORTS = [
    "lemon_last_error", "lemon_version", "lemon_normalize_rows", "lemon_paired_distance",
    "lemon_d1_normalized", "lemon_class_confidence", "lemon_paired_metric", "lemon_preprocess_u8", "lemon_preprocess_u8_f16x3t", "lemon_preprocess_ragged", "lemon_attention_f32", "lemon_attention_set_f16", "lemon_attention_set_stream_min", "lemon_attention_set_head_dims", "lemon_attention_get_head_dims", "lemon_attention_last_kernel", "lemon_attention_split3", "lemon_attention_f32_varlen", "lemon_attention_split3_varlen", "lemon_attention_f16x3_varlen", "lemon_attention_f16x3t_varlen", "lemon_layernorm_f32", "lemon_vision_tokens_ln", "lemon_text_tokens", "lemon_linear_f32", "lemon_linear_bf16x6", "lemon_split3_f32", "lemon_layernorm_split3", "lemon_linear_f16x3", "lemon_pack_weight_f16x3t", "lemon_layernorm_f16x3t", "lemon_linear_f16x3t", "lemon_linear_f16x3t_ln", "lemon_linear_f16x3t_chain", "lemon_ln_finalize", "lemon_rowstats_f16x3t", "lemon_unpack_act_f16x3t", "lemon_linear_f16x3t_set_profiling", "lemon_linear_f16x3t_set_mfma", "lemon_linear_f16x3t_last_kernel", "lemon_linear_f16x3t_profile_read", "lemon_attention_f16x3t", "lemon_split_f16x3", "lemon_layernorm_f16x3", "lemon_attention_f16x3", "lemon_linear_load_tuned",
    "lemon_linear_dump_tuned", "lemon_linear_set_tuning", "lemon_linear_stamp", "lemon_index_create", "lemon_index_free", "lemon_index_add",
    "lemon_index_ntotal", "lemon_index_dim", "lemon_index_data", "lemon_index_search",
    "lemon_index_set_algo", "lemon_index_set_wide_filter", "lemon_index_last_scan_kernel", "lemon_index_set_query_dedup", "lemon_index_last_search_info", "lemon_index_set_profiling",
    "lemon_index_profile_read", "lemon_debug_scan_plan", "lemon_neighbors", "lemon_discrepancy", "lemon_discrepancy_cache", "lemon_discrepancy_ks", "lemon_discrepancy_ks_host", "lemon_score", "lemon_grid_f1",
    "lemon_grid_f1_ks", "lemon_grid_f1_ks_workspace_bytes",
    "lemon_index_l2_from_ip", "lemon_l2_from_ip_host", "lemon_neighbors_metrics",
    "lemon_kmeans_assign", "lemon_kmeans_update", "lemon_kmeans_split", "lemon_kmeans_train", "lemon_kmeans_workspace_bytes",
    "lemon_knn_label_disagreement", "lemon_jpeg_info", "lemon_jpeg_entropy", "lemon_jpeg_reconstruct_host", "lemon_jpeg_decode",
    "lemon_jpeg_pack", "lemon_jpeg_entropy_device", "lemon_jpeg_entropy_workspace_bytes", "lemon_jpeg_entropy_par_host",
    "lemon_jpeg_prog_info", "lemon_jpeg_prog_entropy", "lemon_jpeg_prog_pack", "lemon_jpeg_prog_entropy_device",
    "lemon_jpeg_prog_entropy_workspace_bytes", "lemon_jpeg_prog_entropy_par_host",
    "lemon_png_info", "lemon_png_idat", "lemon_png_decode", "lemon_png_decode_workspace_bytes", "lemon_png_decode_host", "lemon_png_inflate", "lemon_png_inflate_host",
    "lemon_tokenizer_create_bpe", "lemon_tokenizer_create_wordpiece", "lemon_tokenizer_free", "lemon_tokenizer_table_info",
    "lemon_tokenize", "lemon_tokenize_host",
    "lemon_hparam_search_workspace_bytes", "lemon_hparam_search", "lemon_hparam_search_host", "lemon_hparam_objective_host",
    "lemon_hparam_search_set_test_knobs",
    "lemon_lbfgs_polish", "lemon_lbfgs_polish_host", "lemon_lbfgs_proxy_host", "lemon_lbfgs_math_host",
    "lemon_eval_metrics_workspace_bytes", "lemon_eval_metrics", "lemon_eval_metrics_host", "lemon_eval_metrics_kde_host",
]


class LemonHipError(RuntimeError):
    pass


SEARCH_NELDER_MEAD, SEARCH_POWELL = 0, 1   # LEMON_SEARCH_*
SEARCH_METHODS = {"Nelder-Mead": SEARCH_NELDER_MEAD, "Powell": SEARCH_POWELL}


class SearchResult(ctypes.Structure):      # LemonSearchResult
    _fields_ = [("x", ctypes.c_double * 6), ("fun", ctypes.c_double), ("nfev", ctypes.c_int32), ("nit", ctypes.c_int32),
                ("status", ctypes.c_int32), ("pad", ctypes.c_int32)]


class PolishResult(ctypes.Structure):      # LemonPolishResult
    _fields_ = [("x", ctypes.c_double * 6), ("loss", ctypes.c_double), ("nfev", ctypes.c_int32), ("nit", ctypes.c_int32),
                ("status", ctypes.c_int32), ("pad", ctypes.c_int32)]


class EvalSegment(ctypes.Structure):       # LemonEvalSegment
    _fields_ = [("offset", ctypes.c_int64), ("n", ctypes.c_int64), ("prevalence", ctypes.c_double), ("thres_from", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class EvalRecord(ctypes.Structure):        # LemonEvalRecord
    _fields_ = [("auroc", ctypes.c_double), ("auprc", ctypes.c_double), ("thres", ctypes.c_double * 3),
                ("counts", (ctypes.c_int64 * 4) * 3), ("status", ctypes.c_int32), ("kde_branch", ctypes.c_int32),
                ("bisect_fallback", ctypes.c_int32), ("pad", ctypes.c_int32)]


EVAL_OK, EVAL_NONFINITE, EVAL_ONE_CLASS, EVAL_FEW_ROWS, EVAL_ZERO_VARIANCE, EVAL_SOURCE = range(6)      # LEMON_EVAL_*

POLISH_OUTER_STEPS = 20                    # optimizer.step calls of torch_minimize (lib/metrics/utils.py:129-141)


class SearchInfo(ctypes.Structure):
    _fields_ = [("algo", ctypes.c_int), ("grid", ctypes.c_int), ("block", ctypes.c_int),
                ("query_panel", ctypes.c_int), ("db_splits", ctypes.c_int),
                ("nq", ctypes.c_int64), ("n", ctypes.c_int64), ("d", ctypes.c_int), ("k", ctypes.c_int),
                ("nq_distinct", ctypes.c_int64)]


_lib = None


def load():
    """Load the HIP library (after torch, so that both share torch's libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise LemonHipError(
            f"{SO_PATH} is missing: build it with `python -m lemon_amd.build` "
            "(or __graft_entry__.build()). There is no CPU fallback for the LEMoN hot path.")
    try:
        import torch  # noqa: F401  (loads the ROCm runtime the library resolves against)
    except ImportError:
        pass
    lib = ctypes.CDLL(SO_PATH, mode=ctypes.RTLD_GLOBAL)
    c_i64, c_int, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.lemon_last_error.restype = ctypes.c_char_p
    lib.lemon_version.argtypes = [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.lemon_normalize_rows.argtypes = [vp, c_i64, c_int, vp, vp]
    lib.lemon_paired_distance.argtypes = [c_int, vp, vp, c_i64, c_int, vp, vp]
    lib.lemon_d1_normalized.argtypes = [c_int, vp, c_i64, c_int, vp, c_int, vp, vp, vp]
    lib.lemon_paired_metric.argtypes = [c_int, vp, vp, c_i64, c_int, vp, vp]
    lib.lemon_class_confidence.argtypes = [c_int, vp, c_i64, c_int, vp, c_int, vp, vp, vp]
    lib.lemon_preprocess_u8.argtypes = [vp, c_i64, c_int, c_int, vp, vp, c_int, vp, vp, c_int, c_int, c_int, c_int,
                                        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_int, vp, vp]
    lib.lemon_preprocess_u8_f16x3t.argtypes = [vp, c_i64, c_int, c_int, vp, vp, c_int, vp, vp, c_int, c_int, c_int, c_int,
                                        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), c_int, vp, vp]
    lib.lemon_preprocess_ragged.argtypes = [vp, c_i64, c_i64, vp, c_i64, c_i64, vp, vp, vp, c_int, ctypes.POINTER(ctypes.c_float),
                                            ctypes.POINTER(ctypes.c_float), c_int, c_int, vp, vp]
    lib.lemon_grid_f1.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, c_i64, c_int, vp, c_int, ctypes.c_double, c_int, vp, vp, vp, vp]
    lib.lemon_grid_f1_ks.argtypes = [vp] * 8 + [c_i64, c_int, ctypes.POINTER(c_int), c_int, ctypes.POINTER(ctypes.c_double), c_int,
                                     ctypes.c_double, c_int, vp, c_i64, vp, vp, vp, vp]
    lib.lemon_grid_f1_ks_workspace_bytes.argtypes = [c_i64, c_int, c_int, ctypes.POINTER(ctypes.c_double)]
    lib.lemon_grid_f1_ks_workspace_bytes.restype = c_i64
    lib.lemon_attention_f32.argtypes = [vp, c_i64, c_int, c_int, c_int, c_int, vp, vp]
    lib.lemon_attention_split3.argtypes = [vp, c_i64, c_int, c_int, c_int, c_int, vp, vp]
    lib.lemon_attention_f16x3.argtypes = [vp, c_i64, c_int, c_int, c_int, c_int, vp, vp]
    for name in ("f32", "split3", "f16x3", "f16x3t"):        # (qkv, batch, seq_len, heads, head_dim, lengths, out, stream)
        getattr(lib, f"lemon_attention_{name}_varlen").argtypes = [vp, c_i64, c_int, c_int, c_int, vp, vp, vp]
    lib.lemon_layernorm_f32.argtypes = [vp, vp, vp, ctypes.c_float, c_i64, c_int, vp, vp]
    lib.lemon_vision_tokens_ln.argtypes = [vp, vp, vp, vp, vp, ctypes.c_float, c_i64, c_int, c_int, vp, vp]
    lib.lemon_text_tokens.argtypes = [vp, c_i64, vp, vp, c_i64, c_int, c_int, c_int, vp, vp]
    lib.lemon_linear_f32.argtypes = [vp, vp, vp, vp, c_i64, c_int, c_int, ctypes.c_float, c_int, vp, vp]
    lib.lemon_linear_bf16x6.argtypes = [vp, vp, vp, vp, c_i64, c_int, c_int, ctypes.c_float, c_int, vp, vp]
    lib.lemon_split3_f32.argtypes = [vp, c_i64, c_int, c_int, vp, vp]
    lib.lemon_layernorm_split3.argtypes = [vp, vp, vp, ctypes.c_float, c_i64, c_int, vp, vp]
    lib.lemon_linear_f16x3.argtypes = [vp, vp, vp, vp, c_i64, c_int, c_int, ctypes.c_float, c_int, vp, vp]
    lib.lemon_split_f16x3.argtypes = [vp, c_i64, c_int, c_int, ctypes.c_float, vp, vp]
    lib.lemon_pack_weight_f16x3t.argtypes = [vp, c_int, c_int, ctypes.c_float, vp, vp]
    lib.lemon_layernorm_f16x3t.argtypes = [vp, vp, vp, ctypes.c_float, c_i64, c_int, vp, vp]
    lib.lemon_linear_f16x3t.argtypes = [vp, vp, vp, vp, c_i64, c_int, c_int, ctypes.c_float, c_int, c_int, vp, vp]
    lib.lemon_linear_f16x3t_ln.argtypes = [vp, vp, vp, vp, c_i64, c_int, c_int, ctypes.c_float, c_int, c_int, vp, vp, vp, vp, vp, vp]
    lib.lemon_linear_f16x3t_chain.argtypes = [vp, vp, vp, vp, vp, c_i64, c_int, c_int, ctypes.c_float, vp, vp, vp, vp]
    lib.lemon_ln_finalize.argtypes = [vp, c_i64, c_int, ctypes.c_float, vp, vp]
    lib.lemon_rowstats_f16x3t.argtypes = [vp, ctypes.c_float, c_i64, c_int, vp, vp, vp]
    lib.lemon_unpack_act_f16x3t.argtypes = [vp, c_i64, c_int, vp, vp]
    lib.lemon_attention_set_f16.argtypes = [c_int]
    lib.lemon_attention_set_stream_min.argtypes = [c_int]
    lib.lemon_attention_set_head_dims.argtypes = [c_int]
    lib.lemon_attention_get_head_dims.argtypes = []
    lib.lemon_attention_last_kernel.argtypes = []
    lib.lemon_attention_last_kernel.restype = ctypes.c_char_p
    lib.lemon_linear_f16x3t_set_profiling.argtypes = [c_int]
    lib.lemon_linear_f16x3t_set_mfma.argtypes = [c_int]
    lib.lemon_linear_f16x3t_last_kernel.argtypes = []
    lib.lemon_linear_f16x3t_last_kernel.restype = ctypes.c_char_p
    lib.lemon_linear_f16x3t_profile_read.argtypes = [ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.lemon_attention_f16x3t.argtypes = [vp, c_i64, c_int, c_int, c_int, c_int, vp, vp]
    lib.lemon_layernorm_f16x3.argtypes = [vp, vp, vp, ctypes.c_float, c_i64, c_int, vp, vp]
    lib.lemon_linear_load_tuned.argtypes = [ctypes.c_char_p]
    lib.lemon_linear_dump_tuned.argtypes = [ctypes.c_char_p]
    lib.lemon_linear_set_tuning.argtypes = [c_int]
    lib.lemon_linear_stamp.argtypes = [ctypes.POINTER(c_int), ctypes.c_char_p, c_int]
    lib.lemon_index_create.argtypes = [c_int, c_int, ctypes.POINTER(vp)]
    lib.lemon_index_free.argtypes = [vp]
    lib.lemon_index_add.argtypes = [vp, vp, c_i64, vp]
    lib.lemon_index_ntotal.argtypes = [vp]
    lib.lemon_index_ntotal.restype = c_i64
    lib.lemon_index_dim.argtypes = [vp]
    lib.lemon_index_data.argtypes = [vp]
    lib.lemon_index_data.restype = vp
    lib.lemon_index_search.argtypes = [vp, vp, c_i64, c_int, vp, vp, vp]
    lib.lemon_index_set_algo.argtypes = [vp, c_int]
    lib.lemon_index_set_query_dedup.argtypes = [vp, c_int]
    lib.lemon_index_set_wide_filter.argtypes = [vp, c_int]
    lib.lemon_index_last_scan_kernel.argtypes = [vp]
    lib.lemon_index_last_scan_kernel.restype = ctypes.c_char_p
    lib.lemon_index_last_search_info.argtypes = [vp, ctypes.POINTER(SearchInfo)]
    lib.lemon_index_set_profiling.argtypes = [vp, c_int]
    lib.lemon_index_profile_read.argtypes = [vp, ctypes.POINTER(c_i64)] + [ctypes.POINTER(ctypes.c_double)] * 3
    ip = ctypes.POINTER(c_int)
    lib.lemon_debug_scan_plan.argtypes = [c_int, c_int, ip, ip, ip, c_int, ip, ip, c_int, ip]
    lib.lemon_neighbors.argtypes = [vp, vp, vp, vp, vp, c_i64, c_int, c_int, vp, c_int, vp, vp] + [vp] * 9 + [vp]
    lib.lemon_index_l2_from_ip.argtypes = [vp, vp, c_i64, vp, vp, c_int, c_int, vp, vp, vp, vp]
    lib.lemon_l2_from_ip_host.argtypes = [vp, vp, c_i64, ctypes.c_float, vp, vp, c_i64, c_int, c_int, vp, vp, vp]
    lib.lemon_neighbors_metrics.argtypes = [vp] * 6 + [c_i64, c_int, c_int, vp, c_int, vp, vp, c_int] + [vp] * 18 + [vp, vp, vp]
    lib.lemon_discrepancy.argtypes = [c_int, vp, vp, vp, vp, c_i64, c_int, c_int, vp, vp]
    lib.lemon_discrepancy_cache.argtypes = [vp, c_int, vp, vp]
    lib.lemon_discrepancy_ks.argtypes = [vp, vp, vp, vp, vp, c_i64, vp, c_int, c_int, c_int, vp, c_i64, c_int, vp, vp]
    lib.lemon_discrepancy_ks_host.argtypes = [c_int, vp, c_i64, c_int, vp, vp, c_i64, vp, c_int, vp, c_int, c_int, vp]
    lib.lemon_score.argtypes = [vp] * 7 + [c_i64, c_int, ctypes.POINTER(ctypes.c_double), vp, vp, vp, vp]
    lib.lemon_kmeans_assign.argtypes = [vp, c_i64, c_int, vp, c_int, vp, vp, vp]
    lib.lemon_kmeans_update.argtypes = [vp, c_i64, c_int, vp, vp, c_int, vp, vp, vp, vp, c_i64, vp]
    lib.lemon_kmeans_split.argtypes = [vp, c_int, c_int, vp, vp]
    lib.lemon_kmeans_train.argtypes = [vp, c_i64, c_int, c_int, c_int, vp, vp, vp, vp, vp, c_i64, vp]
    lib.lemon_kmeans_workspace_bytes.argtypes = [c_i64, c_int, c_int]
    lib.lemon_kmeans_workspace_bytes.restype = c_i64
    lib.lemon_knn_label_disagreement.argtypes = [vp, c_i64, c_int, c_int, c_int, vp, vp, c_i64, vp, vp, vp]
    lib.lemon_jpeg_info.argtypes = [vp, c_i64, vp]
    lib.lemon_jpeg_entropy.argtypes = [vp, c_i64, vp, c_i64, vp]
    lib.lemon_jpeg_reconstruct_host.argtypes = [vp, c_i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp]
    lib.lemon_jpeg_decode.argtypes = [vp, c_i64, c_i64, vp, c_i64, c_i64, vp, c_i64, vp, c_i64, vp]
    lib.lemon_jpeg_pack.argtypes = [vp, c_i64, vp, c_i64, vp, ctypes.POINTER(c_i64)]
    lib.lemon_jpeg_entropy_device.argtypes = [vp, c_i64, c_i64, vp, c_i64, c_i64, ctypes.c_int32, vp, c_i64, vp, vp, c_i64, vp]
    lib.lemon_jpeg_entropy_workspace_bytes.argtypes = [c_i64, c_i64, c_i64]
    lib.lemon_jpeg_entropy_workspace_bytes.restype = c_i64
    lib.lemon_jpeg_entropy_par_host.argtypes = [vp, c_i64, ctypes.c_int32, vp, c_i64, ctypes.POINTER(ctypes.c_int32)]
    lib.lemon_jpeg_prog_info.argtypes = [vp, c_i64, vp]
    lib.lemon_jpeg_prog_entropy.argtypes = [vp, c_i64, vp, c_i64, vp]
    lib.lemon_jpeg_prog_pack.argtypes = [vp, c_i64, vp, c_i64, vp, ctypes.POINTER(c_i64)]
    lib.lemon_jpeg_prog_entropy_device.argtypes = [vp, c_i64, c_i64, vp, c_i64, ctypes.c_int32, vp, c_i64, vp, vp, c_i64, vp]
    lib.lemon_jpeg_prog_entropy_workspace_bytes.argtypes = [c_i64, c_i64, ctypes.c_int32]
    lib.lemon_jpeg_prog_entropy_workspace_bytes.restype = c_i64
    lib.lemon_jpeg_prog_entropy_par_host.argtypes = [vp, c_i64, vp, c_i64, ctypes.POINTER(ctypes.c_int32)]
    lib.lemon_png_info.argtypes = [vp, c_i64, vp]
    lib.lemon_png_idat.argtypes = [vp, c_i64, vp, c_i64]
    lib.lemon_png_idat.restype = c_i64
    lib.lemon_png_decode.argtypes = [vp, c_i64, c_i64, vp, vp, c_i64, vp, c_i64, vp, vp]
    lib.lemon_png_decode_workspace_bytes.argtypes = [c_i64, c_i64]
    lib.lemon_png_decode_workspace_bytes.restype = c_i64
    lib.lemon_png_decode_host.argtypes = [vp, c_i64] + [ctypes.c_int32] * 4 + [vp, vp]
    lib.lemon_png_inflate.argtypes = [vp, c_i64, c_i64, vp, vp, c_i64, vp, vp]
    lib.lemon_png_inflate_host.argtypes = [vp, c_i64, vp, c_i64, vp]
    i32 = ctypes.c_int32
    lib.lemon_tokenizer_create_bpe.argtypes = [vp, vp, vp, vp, c_i64, i32, i32, ctypes.POINTER(vp)]
    lib.lemon_tokenizer_create_wordpiece.argtypes = [vp, vp, vp, c_i64, i32, i32, i32, c_int, c_int, c_int, ctypes.POINTER(vp)]
    lib.lemon_tokenizer_free.argtypes = [vp]
    lib.lemon_tokenizer_table_info.argtypes = [vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), ctypes.POINTER(c_int)]
    lib.lemon_tokenize.argtypes = [vp, vp, c_i64, vp, c_i64, c_int, i32, vp, vp, vp, vp]
    lib.lemon_tokenize_host.argtypes = [vp, vp, c_i64, vp, c_i64, c_int, i32, vp, vp, vp]
    lib.lemon_hparam_search_workspace_bytes.argtypes = [c_i64, c_int]
    lib.lemon_hparam_search_workspace_bytes.restype = c_i64
    lib.lemon_hparam_search.argtypes = [vp] * 8 + [c_i64, c_int, c_int, vp, vp, vp, c_i64, vp, vp]
    lib.lemon_hparam_search_host.argtypes = [vp] * 8 + [c_i64, c_int, c_int, vp, vp, vp, c_i64, vp]
    lib.lemon_hparam_objective_host.argtypes = [vp] * 8 + [c_i64, c_int, c_int, c_int, c_int, vp]
    lib.lemon_hparam_objective_host.restype = ctypes.c_double
    lib.lemon_hparam_search_set_test_knobs.argtypes = [c_int] * 5
    lib.lemon_lbfgs_polish.argtypes = [vp] * 8 + [c_i64, c_int, c_int, vp, vp, c_int, vp, vp]
    lib.lemon_lbfgs_polish_host.argtypes = [vp] * 8 + [c_i64, c_int, c_int, vp, vp, c_int, vp]
    lib.lemon_lbfgs_proxy_host.argtypes = [vp] * 8 + [c_i64, c_int, c_int, c_int, c_int, vp, vp]
    lib.lemon_lbfgs_proxy_host.restype = ctypes.c_double
    lib.lemon_lbfgs_math_host.argtypes = [c_int, vp, c_i64, vp]
    lib.lemon_eval_metrics_workspace_bytes.argtypes = [c_i64, c_int, c_int]
    lib.lemon_eval_metrics_workspace_bytes.restype = c_i64
    lib.lemon_eval_metrics.argtypes = [vp, vp, c_i64, vp, c_int, vp, c_i64, vp, vp]
    lib.lemon_eval_metrics_host.argtypes = [vp, vp, c_i64, vp, c_int, vp]
    lib.lemon_eval_metrics_kde_host.argtypes = [vp, c_i64, vp, vp]
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().lemon_last_error().decode("utf-8", "replace")
        raise LemonHipError(f"{what} failed (rc={rc}): {msg}")
