"""ctypes binding of ``libmcevidence_hip.so`` (C ABI: ``include/mcevidence_hip.h``).

This is the only place the package touches native code.  There is no CPU
fallback: if the shared library is missing, or no MI355X is visible when a
compute entry point is called, an exception is raised.

Error mapping follows what the replaced scikit-learn call would raise
(``/root/reference/MCEvidence.py:1093-1104``): argument problems ->
``ValueError`` (sklearn raises ValueError for ``n_neighbors > n_samples_fit``),
runtime/device problems -> ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MCE_LIB: another build of the same library -- same-box A/B of kernel variants, tools/; never a different backend)
LIB_PATH = os.environ.get("MCE_LIB") or os.path.join(_HERE, "libmcevidence_hip.so")

MCE_OK = 0
MCE_ERR_INVALID = -1
MCE_ERR_K_RANGE = -2
MCE_ERR_HIP = -3
MCE_ERR_NO_DEVICE = -4
MCE_ERR_WORKSPACE = -5
MCE_ERR_DIM_RANGE = -6
MCE_ERR_VERIFY = -7
MCE_MAX_K = 32
MCE_MAX_DIM = 63
SELF_NONE, SELF_INCLUDE, SELF_EXCLUDE = 0, 1, 2

#: every symbol include/mcevidence_hip.h declares: name -> (restype, argtypes)
_c = ctypes
_P = _c.c_void_p
SIGNATURES = {
    "mce_abi_version": (_c.c_int, []),
    "mce_device_count": (_c.c_int, []),
    "mce_last_error": (_c.c_char_p, []),
    "mce_last_kernel": (_c.c_char_p, []),
    "mce_last_verify_rows": (_c.c_int32, []),
    "mce_source_hash": (_c.c_char_p, []),
    "mce_release_device_memory": (None, []),
    "mce_set_search_mode": (_c.c_int, [_c.c_int]),
    "mce_get_search_mode": (_c.c_int, []),
    "mce_set_prune_mode": (_c.c_int, [_c.c_int]),
    "mce_get_prune_mode": (_c.c_int, []),
    "mce_set_sym_mode": (_c.c_int, [_c.c_int]),
    "mce_get_sym_mode": (_c.c_int, []),
    "mce_last_prune_stats": (_c.c_int, [_c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "mce_set_profiling": (None, [_c.c_int]),
    "mce_last_kernel_ms": (_c.c_double, []),
    "mce_last_search_stats": (_c.c_int, [_c.c_void_p, _c.c_int32]),
    "mce_debug_mfma_tile_f16": (_c.c_int, [_P, _P, _c.c_int32, _P, _c.c_int32]),
    "mce_debug_mfma_tiles_f16": (_c.c_int, [_P, _P, _c.c_int32, _c.c_int32, _P, _c.c_int32]),
    "mce_options_push": (_c.c_int, [_P]),
    "mce_options_pop": (_c.c_int, []),
    "mce_knn_f64_opt": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _c.c_int32, _P]),
    "mce_knn_dotp_f64_opt": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int32, _P]),
    "mce_knn_dotp_f64_dev_opt": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _P, _P, _P, _c.c_size_t, _P, _P]),
    "mce_knn_workspace_bytes_opt": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _P]),
    "mce_knn_f64": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _c.c_int32]),
    "mce_dotp_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _c.c_int32]),
    "mce_knn_dotp_f64": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int32]),
    "mce_evidence_feed_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32,
                                         _P, _P, _P, _P, _P, _c.c_int32]),
    "mce_evidence_feed_part_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32,
                                              _P, _P, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _c.c_int32]),
    "mce_evidence_feed_whiten_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _P, _c.POINTER(_c.c_double), _P,
                                                _c.POINTER(_c.c_uint64), _c.c_int32]),
    "mce_evidence_feed_part_dev_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32,
                                                  _P, _P, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _c.c_int32]),
    "mce_evidence_feed_whiten_dev_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _P, _c.POINTER(_c.c_double), _P,
                                                    _c.POINTER(_c.c_uint64), _c.c_int32]),
    "mce_knn_dotp_part_f64_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _c.c_size_t, _P]),
    "mce_knn_dotp_part_f64": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _c.c_int32]),
    "mce_knn_dotp_part_prepared_f64_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _c.c_size_t, _P]),
    "mce_prune_part_applies": (_c.c_int32, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32]),
    "mce_prune_part_prepare_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int64),
                                              _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _P, _c.c_size_t, _P]),
    "mce_pairs_once_blocks": (_c.c_int32, [_c.c_int64, _c.c_int32, _c.c_int32]),
    "mce_pairs_once_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32]),
    "mce_pairs_once_prepare_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int64), _P,
                                              _c.c_size_t, _P]),
    "mce_pairs_once_sweep_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _c.c_size_t, _P]),
    "mce_pairs_once_export_dev": (_c.c_int, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _c.c_size_t, _P]),
    "mce_pairs_once_finish_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _c.c_int64, _P, _P, _P,
                                             _c.c_size_t, _P]),
    "mce_verify_workspace_bytes": (_c.c_size_t, [_c.c_int32, _c.c_int32]),
    "mce_verify_knn_f64_dev": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _c.c_int32, _c.c_int32,
                                          _c.c_uint64, _P, _P, _c.c_size_t, _P]),
    "mce_verify_knn_f64": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _c.c_int32, _c.c_int32,
                                      _c.c_uint64, _P, _c.c_int32]),
    "mce_chain_dev_open": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.POINTER(_P), _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64)]),
    "mce_chain_dev_read": (_c.c_int, [_P, _P, _P, _c.c_int32]),
    "mce_chain_dev_close": (None, [_P]),
    "mce_chain_dev_read_dev": (_c.c_int, [_P, _P, _P, _c.c_int32]),
    "mce_chain_select_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int32]),
    "mce_chain_gather_workspace_bytes": (_c.c_size_t, [_c.c_int32]),
    "mce_chain_reduce_workspace_bytes": (_c.c_size_t, [_c.c_int64]),
    "mce_chain_weights_dev": (_c.c_int, [_P, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_double, _c.POINTER(_c.c_int32), _P, _P, _c.c_size_t, _P]),
    "mce_chain_select_count_dev": (_c.c_int, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_double, _P, _c.c_int64, _c.POINTER(_c.c_int64), _P, _c.c_size_t, _P]),
    "mce_chain_select_fill_dev": (_c.c_int, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_double, _c.c_int64, _c.c_int64, _P, _P, _P, _c.c_size_t, _P]),
    "mce_chain_gather_dev": (_c.c_int, [_P, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P,
                                        _P, _c.c_size_t, _P]),
    "mce_chain_reduce_dev": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int32, _P, _P, _P, _c.c_size_t, _P]),
    "mce_chain_corr_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int64]),
    "mce_chain_corr_dev": (_c.c_int, [_P, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_double, _c.c_int64, _c.POINTER(_c.c_int32), _P,
                                      _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _P, _P, _P, _c.POINTER(_c.c_int64), _P, _c.c_size_t, _P]),
    "mce_chain_corr_f64": (_c.c_int, [_P, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_double, _c.c_int64, _c.POINTER(_c.c_int32), _P,
                                      _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64), _P, _P, _P, _c.POINTER(_c.c_int64), _c.c_int32]),
    "mce_chain_conv_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32]),
    "mce_chain_conv_dev": (_c.c_int, [_P, _P, _c.c_int32, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _P, _c.c_size_t, _P]),
    "mce_chain_conv_f64": (_c.c_int, [_P, _P, _c.c_int32, _c.c_int32, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _c.c_int32]),
    "mce_knn_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32]),
    "mce_dotp_workspace_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int32]),
    "mce_knn_f64_dev": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _P, _c.c_size_t, _P]),
    "mce_dotp_f64_dev": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _c.c_size_t, _P]),
    "mce_eig_sym_batch_dev_f64": (_c.c_int, [_P, _c.c_int32, _c.c_int64, _P, _P, _P, _P, _P]),
    "mce_eig_sym_batch_f64": (_c.c_int, [_P, _c.c_int32, _c.c_int64, _c.c_int32, _P, _P, _P, _P, _c.c_int32]),
    "mce_last_eig_stats": (_c.c_int, [_c.c_void_p, _c.c_int32]),
    "mce_knn_dotp_f64_dev": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64, _P, _P, _P, _P, _P, _c.c_size_t, _P]),
}



class FeedProblem(ctypes.Structure):
    """``mce_feed_problem`` of include/mcevidence_hip.h (one evidence problem of a batch)."""
    _fields_ = [("S1", _P), ("n1", _c.c_int64), ("ld1", _c.c_int64),
                ("S2", _P), ("n2", _c.c_int64), ("ld2", _c.c_int64),
                ("d", _c.c_int32), ("cov_mode", _c.c_int32), ("kmax", _c.c_int32), ("status", _c.c_int32),
                ("w", _P), ("fs", _P), ("dotp", _P), ("eigenvalues", _P), ("jacobian", _c.c_double)]


SIGNATURES["mce_evidence_feed_batch_f64"] = (_c.c_int, [_c.POINTER(FeedProblem), _c.c_int64, _P, _c.c_int32])
SIGNATURES["mce_feed_problem_size"] = (_c.c_size_t, [])
SIGNATURES["mce_evidence_feed_batch_dev_f64"] = (_c.c_int, [_c.POINTER(FeedProblem), _c.c_int64, _c.c_int32])
MCE_MAX_PREFIX = 256
_PREFIX_ARGS = [_P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _c.c_int32, _P, _P, _P, _c.c_int32]
SIGNATURES["mce_evidence_feed_prefix_f64"] = (_c.c_int, _PREFIX_ARGS)
SIGNATURES["mce_evidence_feed_prefix_dev_f64"] = (_c.c_int, _PREFIX_ARGS)


class FarmFile(ctypes.Structure):
    """``mce_farm_file``: one file of a wave -- its first global token, tokens, rows, columns, status (0 ok, 1 ragged, 2 a field
    that is not a number, at ``bad_row`` / ``bad_col`` inside the file)."""
    _fields_ = [("tok_base", _c.c_int64), ("ntok", _c.c_int64), ("nrows", _c.c_int64), ("ncols", _c.c_int64), ("status", _c.c_int64),
                ("bad_row", _c.c_int64), ("bad_col", _c.c_int64)]


FARM_OK, FARM_RAGGED, FARM_NOT_A_NUMBER = 0, 1, 2
SIGNATURES["mce_chain_farm_create"] = (_c.c_int, [_c.c_int64, _c.c_int32, _c.POINTER(_P), _c.POINTER(_P)])
SIGNATURES["mce_chain_farm_destroy"] = (None, [_P])
SIGNATURES["mce_chain_farm_structure"] = (_c.c_int, [_P, _P, _P, _c.c_int32, _c.c_int64, _c.POINTER(FarmFile), _c.POINTER(_c.c_int64)])
SIGNATURES["mce_chain_farm_parse"] = (_c.c_int, [_P, _P, _c.POINTER(FarmFile), _c.c_int32])
SIGNATURES["mce_chain_farm_stats"] = (_c.c_int, [_P, _P, _c.c_int32])
SIGNATURES["mce_chain_farm_prep_workspace_bytes"] = (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int64])
SIGNATURES["mce_chain_farm_prep_dev"] = (_c.c_int, [_P, _P, _c.c_int32, _P, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _P,
                                                     _P, _c.c_size_t, _P])

MCE_JACK_MAX_GROUPS = 64
SIGNATURES["mce_jack_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32])
SIGNATURES["mce_jack_dotp_dev"] = (_c.c_int, [_P, _P, _c.c_int64, _c.c_int32, _P, _P, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P,
                                              _P, _P, _P, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_jack_dotp_f64"] = (_c.c_int, [_P, _P, _c.c_int64, _c.c_int32, _P, _P, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P,
                                              _P, _P, _P, _P, _c.c_int32])

MCE_DIV_MAX_K, MCE_DIV_MAX_DIM, MCE_DIV_REPORT = 16, 64, 4
SIGNATURES["mce_div_whiten_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32])
SIGNATURES["mce_div_whiten_dev"] = (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int32, _P, _P, _P, _P, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_div_whiten_f64"] = (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int32, _P, _P, _P, _P, _P, _c.c_int32])
SIGNATURES["mce_knn_div_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32])
_DIV_TERMS_ARGS = [_P, _P, _P, _P, _c.c_int64, _c.c_int32, _P, _P, _P, _c.c_int64, _P, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _P, _P, _P, _P, _P, _P]
SIGNATURES["mce_knn_div_terms_dev"] = (_c.c_int, _DIV_TERMS_ARGS + [_P, _c.c_size_t, _P])
SIGNATURES["mce_knn_div_terms_f64"] = (_c.c_int, _DIV_TERMS_ARGS + [_c.c_int32])


class MomentsSeg(ctypes.Structure):
    """``mce_moments_seg``: one system of ``mce_like_moments_*`` -- the addresses of its fs and w columns, its rows."""
    _fields_ = [("fs", _P), ("w", _P), ("n", _c.c_int64)]


MCE_MOMENTS_OUT = 6
MOMENTS_FIELDS = ("W", "c", "v", "A2", "rows", "status")
MOMENTS_OK, MOMENTS_NOT_FINITE, MOMENTS_NO_WEIGHT = 0, 3, 5
SIGNATURES["mce_like_moments_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32])
SIGNATURES["mce_like_moments_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_like_moments_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32])


class SummarySeg(ctypes.Structure):
    """``mce_summary_seg``: one system of ``mce_param_summary_*`` -- its raw rows (address, row stride in doubles, rows, measured
    columns) and the addresses of its w and fs columns"""
    _fields_ = [("x", _P), ("ld", _c.c_int64), ("n", _c.c_int64), ("d", _c.c_int32), ("w", _P), ("fs", _P)]


MCE_SUMMARY_MAX_Q = 16
MCE_SUMMARY_HEAD = 8
MCE_SUMMARY_PASS_ELEMS = 1 << 25
SIGNATURES["mce_param_summary_out_doubles"] = (_c.c_size_t, [_c.c_int32, _c.c_int32])
SIGNATURES["mce_param_summary_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int64])
SIGNATURES["mce_param_summary_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _c.c_int64, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_param_summary_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _c.c_int64, _P, _c.c_int32])


class CovSeg(ctypes.Structure):
    """``mce_cov_seg``: one system of ``mce_param_cov_*`` -- its raw rows (address, row stride in doubles, rows, measured columns) and
    the address of its w column"""
    _fields_ = [("x", _P), ("ld", _c.c_int64), ("n", _c.c_int64), ("d", _c.c_int32), ("w", _P)]


MCE_COV_HEAD = 8
SIGNATURES["mce_param_cov_out_doubles"] = (_c.c_size_t, [_c.c_int32])
SIGNATURES["mce_param_cov_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_cov_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_param_cov_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32])


class KdeSeg(ctypes.Structure):
    """``mce_kde_seg``: one system of ``mce_kde_shift_*`` -- its rows (address, row stride in doubles, rows, measured columns), the address
    of its w column, the HOST addresses of linv[d * d], mean[d] and point[d], c = 1 / (2 h^2), and the optional addresses of the densities
    [n + 1] and of the whitened rows [n, d]"""
    _fields_ = [("x", _P), ("ld", _c.c_int64), ("n", _c.c_int64), ("d", _c.c_int32), ("w", _P), ("linv", _P), ("mean", _P), ("point", _P),
                ("c", _c.c_double), ("dens", _P), ("zout", _P)]


MCE_KDE_OUT = 16
MCE_KDE_MAX_DIM = 64
SIGNATURES["mce_kde_shift_out_doubles"] = (_c.c_size_t, [])
SIGNATURES["mce_kde_shift_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32])
SIGNATURES["mce_kde_shift_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_kde_shift_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32])

MCE_MARGINALS_HEAD = 8
MCE_MARGINALS_MAX_P = 7
MCE_CONTOURS_HEAD = 8
MCE_CONTOURS_MAX_COLS = 32
SIGNATURES["mce_param_marginals_out_doubles"] = (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_marginals_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_marginals_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_param_marginals_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _c.c_int32])
SIGNATURES["mce_param_marginals_bounded_out_doubles"] = (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_marginals_bounded_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_marginals_bounded_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_param_marginals_bounded_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _c.c_int32])
SIGNATURES["mce_param_contours_out_doubles"] = (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_contours_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_contours_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_param_contours_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _c.c_int32])
SIGNATURES["mce_param_contours_bounded_out_doubles"] = (_c.c_size_t, [_c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_contours_bounded_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32])
SIGNATURES["mce_param_contours_bounded_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _P, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_param_contours_bounded_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32, _P, _P, _c.c_int32, _c.c_int32, _c.c_double, _P, _c.c_int32])


class JackGroupsSeg(ctypes.Structure):
    """``mce_jack_groups_seg``: one system of ``mce_jack_groups_dev`` (rows / src / out: device addresses; part_first: a host array)."""
    _fields_ = [("rows", _P), ("src", _P), ("part_first", _P), ("nparts", _c.c_int64), ("n", _c.c_int64), ("N", _c.c_int64), ("G", _c.c_int32),
                ("by", _c.c_int32), ("out", _P)]


class JackLeaveOutSeg(ctypes.Structure):
    """``mce_jack_leave_out_seg``: one system of ``mce_jack_leave_out_*`` -- the addresses of its w, fs (or none) and group columns."""
    _fields_ = [("w", _P), ("fs", _P), ("g", _P), ("n", _c.c_int64), ("G", _c.c_int32)]


MCE_JACK_LEAVE_OUT = 8
JACK_LEAVE_OUT_FIELDS = ("nrows", "SumW", "W", "c", "v", "A2", "rows", "status")
JACK_BY = {"blocks": 0, "chains": 1}
SIGNATURES["mce_jack_groups_dev"] = (_c.c_int, [_P, _c.c_int32, _P])
SIGNATURES["mce_jack_leave_out_workspace_bytes"] = (_c.c_size_t, [_c.c_int64, _c.c_int32, _c.c_int32])
SIGNATURES["mce_jack_leave_out_dev"] = (_c.c_int, [_P, _c.c_int32, _P, _P, _c.c_size_t, _P])
SIGNATURES["mce_jack_leave_out_f64"] = (_c.c_int, [_P, _c.c_int32, _P, _c.c_int32])

_lib = None


def load():
    """Load the shared library (once).  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        path = LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                "mcevidence_amd: %s not found -- build it with `make -C mcevidence_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback." % path)
        # PyTorch-ROCm wheels bundle their own HIP/HSA runtime (torch/lib/libamdhip64.so, same
        # soname as /opt/rocm's).  Two HSA runtimes in one process cannot both own the GPU, so
        # when torch is installed let it load its runtime FIRST; our library then binds to the
        # already-loaded libamdhip64.so.7.  torch is plumbing here, never a compute fallback.
        if "torch" not in sys.modules and os.environ.get("MCE_SKIP_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:  # torch absent: plain ROCm runtime from /opt/rocm
                pass
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("MCE_LIB") and not hasattr(lib, name):
                continue                                         # (an older build in an A/B run lacks the newest entry points)
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.mce_abi_version() not in (2, 3) or lib.mce_feed_problem_size() != ctypes.sizeof(FeedProblem):
            raise RuntimeError("mcevidence_amd: ABI version mismatch")
        _lib = lib
    return _lib


def last_error():
    return load().mce_last_error().decode("utf-8", "replace")


def last_kernel():
    return load().mce_last_kernel().decode("utf-8", "replace")


def source_hash():
    """SHA-256 of the kernel sources the loaded library was built from (csrc/Makefile: src_hash.h)"""
    return load().mce_source_hash().decode("ascii")


MODE_AUTO, MODE_F64, MODE_F16_FILTER = 0, 1, 2


def set_search_mode(mode):
    """0/2: fp16-MFMA filter + exact fp64 refine where supported; 1: fp64 MFMA sweep only."""
    check(load().mce_set_search_mode(int(mode)))


def get_search_mode():
    return int(load().mce_get_search_mode())


PRUNE_AUTO, PRUNE_OFF, PRUNE_FORCE = 0, 1, 2


def set_prune_mode(mode):
    """spatial pruning of the search (low d, large reference sets): 0 auto, 1 never, 2 whenever possible"""
    check(load().mce_set_prune_mode(int(mode)))


def get_prune_mode():
    return int(load().mce_get_prune_mode())


SYM_AUTO, SYM_OFF, SYM_FORCE = 0, 1, 2


def set_sym_mode(mode):
    """symmetric sweep of auto-evidence searches (each pair of rows multiplied once): 0 auto, 1 never, 2 whenever possible"""
    check(load().mce_set_sym_mode(int(mode)))


def get_sym_mode():
    return int(load().mce_get_sym_mode())


def last_prune_stats():
    """(fraction of block x chunk pairs staged, fraction of wave x tile products multiplied) of the last
    pruned search run through a ``*_dev`` call on this thread (its workspace must still exist)."""
    a, b = _c.c_double(), _c.c_double()
    check(load().mce_last_prune_stats(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def release_device_memory():
    load().mce_release_device_memory()


def set_profiling(on):
    load().mce_set_profiling(1 if on else 0)


def last_kernel_ms():
    return float(load().mce_last_kernel_ms())


class Options(_c.Structure):
    """``mce_options``: the search / prune / symmetric modes of ONE call (-1: the process default); ``verify`` > 0:
    re-check that many query rows after the search by an exact fp64 scan of all reference rows (RuntimeError if one
    disagrees; host-pointer entry points); ``eig_mode``: who solves the evidence feed's eigen-systems -- ``EIG_DEFAULT`` (0:
    the process default, ``MCE_FEED_EIG=host|hip``), ``EIG_HOST`` or ``EIG_DEVICE``."""
    _fields_ = [("size", _c.c_int32), ("search_mode", _c.c_int32), ("prune_mode", _c.c_int32), ("sym_mode", _c.c_int32),
                ("same_set", _c.c_int32), ("verify", _c.c_int32), ("eig_mode", _c.c_int32), ("reserved", _c.c_int32 * 1)]

    def __init__(self, search_mode=-1, prune_mode=-1, sym_mode=-1, same_set=-1, verify=-1, eig_mode=0):
        super().__init__(_c.sizeof(Options), int(search_mode), int(prune_mode), int(sym_mode), int(same_set), int(verify), int(eig_mode))


EIG_DEFAULT, EIG_HOST, EIG_DEVICE = 0, 1, 2
EIG_STATUS_INTS = 4          # status of one solve: code (0 ok, 1 not finite, 2 an eigenvalue not > 0), its index, sweeps, rotations
EIG_MAX_DIM = 127


class options(object):
    """``with _capi.options(sym_mode=_capi.SYM_FORCE): ...`` -- the modes apply to the library calls THIS THREAD makes
    inside the block (mce_options_push / mce_options_pop); other threads are not affected."""

    def __init__(self, **modes):
        self.opt = Options(**modes)

    def __enter__(self):
        check(load().mce_options_push(_c.byref(self.opt)))
        return self

    def __exit__(self, *exc):
        check(load().mce_options_pop())
        return False


def last_search_stats():
    """dict(flops_main, flops_all, search_ms, kernel_ms) of the last search on this thread (mce_last_search_stats)."""
    out = (_c.c_double * 4)()
    check(load().mce_last_search_stats(_c.cast(out, _c.c_void_p), 4))
    return dict(flops_main=out[0], flops_all=out[1], search_ms=out[2], kernel_ms=out[3])


def eig_sym_batch(cov, mode=EIG_DEVICE, device=0):
    """Both eigen-solvers of the evidence feed through one door (``mce_eig_sym_batch_f64``): ``cov`` [nsys, d, d] (or one [d, d])
    symmetric matrices; ``mode`` ``EIG_HOST`` (cyclic Jacobi on one core) or ``EIG_DEVICE`` (one workgroup per system).  Returns
    (evec [nsys, d, d], eigenvectors in the columns; scale [nsys, d] = 1 / sqrt(lam); lam [nsys, d], descending; status [nsys, 4] =
    code, index, sweeps, rotations).  A system with a non-zero code fails alone: identity, unit scales."""
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    if cov.ndim == 2:
        cov = cov[None]
    if cov.ndim != 3 or cov.shape[1] != cov.shape[2] or cov.shape[0] < 1 or cov.shape[1] < 1:
        raise ValueError("cov must be [nsys, d, d]")
    nsys, d = cov.shape[0], cov.shape[1]
    evec = np.zeros((nsys, d, d))
    scale = np.zeros((nsys, d))
    lam = np.zeros((nsys, d))
    status = np.zeros((nsys, EIG_STATUS_INTS), dtype=np.int32)
    check(load().mce_eig_sym_batch_f64(cov.ctypes.data, d, nsys, int(mode), evec.ctypes.data, scale.ctypes.data, lam.ctypes.data, status.ctypes.data,
                                       int(device)))
    return evec, scale, lam, status


def eig_sym_batch_dev(d_cov, d, nsys, d_evec, d_scale, d_lam, d_status, stream=0):
    """``mce_eig_sym_batch_dev_f64``: device ADDRESSES, enqueue only."""
    check(load().mce_eig_sym_batch_dev_f64(d_cov, int(d), int(nsys), d_evec, d_scale, d_lam, d_status, stream or None))


def last_eig_stats():
    """dict(device, host, max_sweeps, rotations): what the calling thread's last evidence-feed call solved where (mce_last_eig_stats)"""
    out = (_c.c_double * 4)()
    check(load().mce_last_eig_stats(_c.cast(out, _c.c_void_p), 4))
    return dict(device=int(out[0]), host=int(out[1]), max_sweeps=int(out[2]), rotations=int(out[3]))


def check(rc):
    if rc == MCE_OK:
        return
    msg = last_error()
    if rc in (MCE_ERR_INVALID, MCE_ERR_K_RANGE, MCE_ERR_WORKSPACE, MCE_ERR_DIM_RANGE):
        raise ValueError(msg)
    raise RuntimeError("mcevidence_amd HIP backend: " + msg)


def device_count():
    return int(load().mce_device_count())


def require_device():
    n = device_count()
    if n < 1:
        raise RuntimeError("mcevidence_amd: no HIP device visible (this package has no CPU fallback)")
    return n


def _f64(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("%s contains NaN or infinity" % name)   # sklearn's check_array does the same
    return a


def _f64_fs(a, name="fs"):
    """fs = logL - max(logL) <= 0 (reference :1062-1064).  -inf is a legitimate entry -- a row with zero
    likelihood, exp(fs) = 0, a harmless zero term in the reference's sum and in the kernel's -- so only NaN
    and +inf are refused."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if np.isnan(a).any() or (a == np.inf).any():
        raise ValueError("%s contains NaN or +infinity" % name)
    return a


def chain_dev_parse(text_ptr, nbytes, device=0):
    """Chain text at host address ``text_ptr`` (``nbytes`` bytes, valid for the duration of the call) -> (fp64 array
    [rows, columns], stats) through mce_chain_dev_open / _read / _close.  stats: dict(tokens, patched, ms_upload, ms_structure,
    ms_parse, ms_download).  ValueError: ragged lines or a field that is not a number; RuntimeError: no device, HIP failure."""
    lib = load()
    handle = _P()
    nrows, ncols = _c.c_int64(), _c.c_int64()
    check(lib.mce_chain_dev_open(text_ptr, int(nbytes), int(device), _c.byref(handle), _c.byref(nrows), _c.byref(ncols)))
    try:
        out = np.empty((nrows.value, ncols.value), dtype=np.float64)
        st = (_c.c_double * 6)()
        check(lib.mce_chain_dev_read(handle, out.ctypes.data, _c.cast(st, _P), 6))
    finally:
        lib.mce_chain_dev_close(handle)
    return out, dict(tokens=int(st[0]), patched=int(st[1]), ms_upload=st[2], ms_structure=st[3], ms_parse=st[4], ms_download=st[5])


class ChainPart(ctypes.Structure):
    """``mce_chain_part``: one burned chain on the device -- address of its first kept row, rows kept."""
    _fields_ = [("rows", _P), ("nrows", _c.c_int64)]


def chain_parts(parts):
    """[(device address, rows)] -> the C array the ``mce_chain_*_dev`` calls take"""
    arr = (ChainPart * max(len(parts), 1))()
    for i, (ptr, nrows) in enumerate(parts):
        arr[i].rows = ptr or None
        arr[i].nrows = int(nrows)
    return arr


def chain_dev_open(text_ptr, nbytes, device=0):
    """mce_chain_dev_open -> (handle, rows, columns); close it with ``chain_dev_close`` (the text must stay valid until then)"""
    handle = _P()
    nrows, ncols = _c.c_int64(), _c.c_int64()
    check(load().mce_chain_dev_open(text_ptr, int(nbytes), int(device), _c.byref(handle), _c.byref(nrows), _c.byref(ncols)))
    return handle, int(nrows.value), int(ncols.value)


def chain_dev_read_dev(handle, d_out):
    """mce_chain_dev_read_dev: the parsed values into the DEVICE buffer at address ``d_out``; returns the reader's stats"""
    st = (_c.c_double * 6)()
    check(load().mce_chain_dev_read_dev(handle, d_out or None, _c.cast(st, _P), 6))
    return dict(tokens=int(st[0]), patched=int(st[1]), ms_upload=st[2], ms_structure=st[3], ms_parse=st[4], ms_download=st[5])


def chain_dev_close(handle):
    load().mce_chain_dev_close(handle)


FARM_STATS = ("waves", "files", "allocs", "allocs_wave", "grows", "tokens", "patched", "ms_upload", "ms_structure", "ms_parse", "ms_patch", "capacity")


def chain_farm_create(capacity_bytes, device=0):
    """mce_chain_farm_create -> (handle, address of the pinned staging buffer of ``capacity_bytes``)"""
    handle, staging = _P(), _P()
    check(load().mce_chain_farm_create(int(capacity_bytes), int(device), _c.byref(handle), _c.byref(staging)))
    return handle, int(staging.value)


def chain_farm_destroy(handle):
    load().mce_chain_farm_destroy(handle)


def chain_farm_structure(handle, file_off, file_len, wave_bytes):
    """mce_chain_farm_structure -> (the C array of ``FarmFile`` that ``chain_farm_parse`` takes, tokens of the wave)"""
    off = np.ascontiguousarray(file_off, dtype=np.int64)
    ln = np.ascontiguousarray(file_len, dtype=np.int64)
    if off.ndim != 1 or off.shape != ln.shape:
        raise ValueError("file_off and file_len must be 1-D of one length")
    files = (FarmFile * max(len(off), 1))()
    ntok = _c.c_int64(0)
    check(load().mce_chain_farm_structure(handle, off.ctypes.data if len(off) else None, ln.ctypes.data if len(ln) else None, len(off), int(wave_bytes),
                                          files, _c.byref(ntok)))
    return files, int(ntok.value)


def chain_farm_parse(handle, d_out, files, nfiles):
    """mce_chain_farm_parse: global token k into the DEVICE buffer at address ``d_out``; updates ``files[f].status``"""
    check(load().mce_chain_farm_parse(handle, d_out or None, files, int(nfiles)))


def chain_farm_stats(handle):
    st = (_c.c_double * 12)()
    check(load().mce_chain_farm_stats(handle, _c.cast(st, _P), 12))
    return {k: (float(st[i]) if k.startswith("ms_") else int(st[i])) for i, k in enumerate(FARM_STATS)}


def chain_farm_prep_workspace_bytes(nroots, nparts, nrows):
    return int(load().mce_chain_farm_prep_workspace_bytes(int(nroots), int(nparts), int(nrows)))


def chain_farm_prep_dev(root_nparts, root_ncols, parts, iw, ilike, itheta, pos_lnp, d_params, d_w, d_like, d_fs, ws, ws_bytes, stream=0):
    """mce_chain_farm_prep_dev -> float64 [nroots, 4]: (max(logL), SumW, NaN likelihoods, weights that are not finite) per root;
    ``parts``: [(device address, rows)] of all roots, root after root"""
    rn = np.ascontiguousarray(root_nparts, dtype=np.int32)
    rc = np.ascontiguousarray(root_ncols, dtype=np.int64)
    if rn.ndim != 1 or rn.shape != rc.shape:
        raise ValueError("root_nparts and root_ncols must be 1-D of one length")
    out = np.zeros((max(len(rn), 1), 4))
    arr = chain_parts(parts)
    check(load().mce_chain_farm_prep_dev(rn.ctypes.data if len(rn) else None, rc.ctypes.data if len(rc) else None, len(rn), _c.cast(arr, _P), len(parts),
                                         int(iw), int(ilike), int(itheta), 1 if pos_lnp else 0, d_params or None, d_w or None, d_like or None, d_fs or None,
                                         out.ctypes.data, ws or None, int(ws_bytes), stream or None))
    return out[:len(rn)]


def chain_select_workspace_bytes(n, nparts):
    return int(load().mce_chain_select_workspace_bytes(int(n), int(nparts)))


def chain_gather_workspace_bytes(nparts):
    return int(load().mce_chain_gather_workspace_bytes(int(nparts)))


def chain_reduce_workspace_bytes(n):
    return int(load().mce_chain_reduce_workspace_bytes(int(n)))


def chain_weights_dev(parts, ncols, iw, thinlen, ws, ws_bytes, stream=0):
    """mce_chain_weights_dev -> (rule, dict(rows, sum_int, max_int, frac, bad)); ``parts``: [(device address, rows)]"""
    rule = _c.c_int32(0)
    tot = (_c.c_double * 5)()
    arr = chain_parts(parts)
    check(load().mce_chain_weights_dev(_c.cast(arr, _P), len(parts), int(ncols), int(iw), float(thinlen), _c.byref(rule), _c.cast(tot, _P),
                                       ws or None, int(ws_bytes), stream or None))
    return int(rule.value), dict(rows=int(tot[0]), sum_int=int(tot[1]), max_int=int(tot[2]), frac=float(tot[3]), bad=int(tot[4]))


def chain_select_count_dev(n, nparts, rule, thinlen, d_edges, nedges, ws, ws_bytes, stream=0):
    n_out = _c.c_int64(0)
    check(load().mce_chain_select_count_dev(int(n), int(nparts), int(rule), float(thinlen), d_edges or None, int(nedges), _c.byref(n_out), ws or None,
                                            int(ws_bytes), stream or None))
    return int(n_out.value)


def chain_select_fill_dev(n, nparts, rule, thinlen, nedges, n_out, d_src, d_new_w, ws, ws_bytes, stream=0):
    check(load().mce_chain_select_fill_dev(int(n), int(nparts), int(rule), float(thinlen), int(nedges), int(n_out), d_src or None, d_new_w or None,
                                           ws or None, int(ws_bytes), stream or None))


def chain_gather_dev(parts, ncols, iw, ilike, itheta, d_src, d_new_w, n_thin, d_rows, n_out, d_params, d_w, d_like, d_full, ws, ws_bytes, stream=0):
    arr = chain_parts(parts)
    check(load().mce_chain_gather_dev(_c.cast(arr, _P), len(parts), int(ncols), int(iw), int(ilike), int(itheta), d_src or None,
                                      d_new_w or None, int(n_thin), d_rows or None, int(n_out), d_params or None, d_w or None, d_like or None,
                                      d_full or None, ws or None, int(ws_bytes), stream or None))


def chain_reduce_dev(d_like, d_w, n, pos_lnp, d_fs, ws, ws_bytes, stream=0):
    """mce_chain_reduce_dev -> (max(logL), SumW, NaN likelihoods, weights that are not finite)"""
    out = (_c.c_double * 4)()
    check(load().mce_chain_reduce_dev(d_like or None, d_w or None, int(n), 1 if pos_lnp else 0, d_fs or None, _c.cast(out, _P), ws or None, int(ws_bytes),
                                      stream or None))
    return float(out[0]), float(out[1]), int(out[2]), int(out[3])


def chain_corr_workspace_bytes(n, nparts, ndim, max_lag):
    return int(load().mce_chain_corr_workspace_bytes(int(n), int(nparts), int(ndim), int(max_lag)))


def _chain_corr(call, parts, ncols, iw, itheta, ndim, min_corr, max_lag, want_rho, tail):
    rule, units, cap, rows = _c.c_int32(0), _c.c_int64(0), _c.c_int64(0), _c.c_int64(0)
    status = (_c.c_int32 * 2)()
    nd = max(int(ndim), 1)
    length = np.zeros(nd)
    cut = np.zeros(nd, dtype=np.int64)
    rho = np.full((max(int(max_lag), 0) + 1, nd), np.nan) if want_rho else None
    arr = chain_parts(parts)
    check(call(_c.cast(arr, _P), len(parts), int(ncols), int(iw), int(itheta), int(ndim), float(min_corr), int(max_lag), _c.byref(rule), _c.cast(status, _P),
               _c.byref(units), _c.byref(cap), length.ctypes.data, cut.ctypes.data, rho.ctypes.data if want_rho else None, _c.byref(rows), *tail))
    return dict(rule=int(rule.value), status=int(status[0]), column=int(status[1]), units=int(units.value), cap=int(cap.value), per_param=length, cut=cut,
                rho=rho[:int(rows.value)] if want_rho else None, rho_rows=int(rows.value))


def chain_corr_dev(parts, ncols, iw, itheta, ndim, min_corr, max_lag, ws, ws_bytes, stream=0, want_rho=False):
    """mce_chain_corr_dev -> dict(rule, status, column, units, cap, per_param [ndim], cut [ndim], rho [lags summed, ndim] or None, rho_rows);
    ``parts``: [(device address, rows)]"""
    return _chain_corr(load().mce_chain_corr_dev, parts, ncols, iw, itheta, ndim, min_corr, max_lag, want_rho, (ws or None, int(ws_bytes), stream or None))


def chain_corr(arrays, iw, itheta, ndim, min_corr=0.05, max_lag=1024, device=0, want_rho=True):
    """mce_chain_corr_f64: the same from HOST arrays (one 2-D fp64 array per burned chain), uploaded by the library"""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    if not arrays or any(a.ndim != 2 or a.shape[1] != arrays[0].shape[1] for a in arrays):
        raise ValueError("chains must be 2-D arrays of one column count")
    parts = [(a.ctypes.data if a.shape[0] else 0, a.shape[0]) for a in arrays]
    return _chain_corr(load().mce_chain_corr_f64, parts, arrays[0].shape[1], iw, itheta, ndim, min_corr, max_lag, want_rho, (int(device),))


CONV_MAX_SEGMENTS = 128


def chain_conv_workspace_bytes(nrows_total, nseg, nsys, ndim):
    return int(load().mce_chain_conv_workspace_bytes(int(nrows_total), int(nseg), int(nsys), int(ndim)))


def _chain_conv(call, segs, seg_sys, nsys, ncols, iw, itheta, ndim, tail):
    nsys, nd = int(nsys), max(int(ndim), 1)
    r = np.full(max(nsys, 1), np.nan)
    per = np.full((max(nsys, 1), nd), np.nan)
    status = np.zeros((max(nsys, 1), 2), dtype=np.int32)
    used = np.zeros(max(nsys, 1), dtype=np.int32)
    sys_ = np.ascontiguousarray(seg_sys, dtype=np.int32)
    if sys_.shape != (len(segs),):
        raise ValueError("chain conv: one system number per segment expected")
    arr = chain_parts(segs)
    check(call(_c.cast(arr, _P), sys_.ctypes.data, len(segs), nsys, int(ncols), int(iw), int(itheta), int(ndim), r.ctypes.data, per.ctypes.data,
               status.ctypes.data, used.ctypes.data, *tail))
    return dict(r_minus_1=r, per_param=per, status=status[:, 0].copy(), column=status[:, 1].copy(), used=used)


def chain_conv_dev(segs, seg_sys, nsys, ncols, iw, itheta, ndim, ws, ws_bytes, stream=0):
    """mce_chain_conv_dev: the Gelman-Rubin R-1 of ``nsys`` systems of segments that are on the device -> dict(r_minus_1 [nsys],
    per_param [nsys, ndim], status [nsys], column [nsys], used [nsys]); ``segs``: [(device address, rows)], ``seg_sys``: the system of each"""
    return _chain_conv(load().mce_chain_conv_dev, segs, seg_sys, nsys, ncols, iw, itheta, ndim, (ws or None, int(ws_bytes), stream or None))


def chain_conv(arrays, seg_sys, nsys, iw, itheta, ndim, device=0):
    """mce_chain_conv_f64: the same from HOST arrays (one 2-D fp64 array per segment), uploaded by the library"""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    if not arrays or any(a.ndim != 2 or a.shape[1] != arrays[0].shape[1] for a in arrays):
        raise ValueError("segments must be 2-D arrays of one column count")
    segs = [(a.ctypes.data if a.shape[0] else 0, a.shape[0]) for a in arrays]
    return _chain_conv(load().mce_chain_conv_f64, segs, seg_sys, nsys, arrays[0].shape[1], iw, itheta, ndim, (int(device),))


def like_moments_workspace_bytes(nrows_total, nseg):
    return int(load().mce_like_moments_workspace_bytes(int(nrows_total), int(nseg)))


def _like_moments(call, segs, tail):
    arr = (MomentsSeg * max(len(segs), 1))()
    for i, (fs, w, n) in enumerate(segs):
        arr[i].fs, arr[i].w, arr[i].n = fs or None, w or None, int(n)
    out = np.full((max(len(segs), 1), MCE_MOMENTS_OUT), np.nan)
    check(call(_c.cast(arr, _P), len(segs), out.ctypes.data, *tail))
    return out[:len(segs)]


def like_moments_dev(segs, ws, ws_bytes, stream=0):
    """mce_like_moments_dev: the weighted moments of the likelihood column of ``len(segs)`` systems that are on the device -> float64
    [nseg, 6]: ``MOMENTS_FIELDS`` per system; ``segs``: [(device address of fs, device address of w, rows)]"""
    return _like_moments(load().mce_like_moments_dev, segs, (ws or None, int(ws_bytes), stream or None))


def like_moments(systems, device=0):
    """mce_like_moments_f64: the same from HOST arrays, ``systems`` = [(fs, w)], uploaded by the library"""
    keep = [(np.ascontiguousarray(f, dtype=np.float64).reshape(-1), np.ascontiguousarray(w, dtype=np.float64).reshape(-1)) for f, w in systems]
    if any(f.shape != w.shape for f, w in keep):
        raise ValueError("like moments: fs and w of one length expected")
    return _like_moments(load().mce_like_moments_f64, [(f.ctypes.data if f.size else 0, w.ctypes.data if w.size else 0, f.size) for f, w in keep], (int(device),))


def _host_systems(systems, who, with_fs=False):
    """``systems`` = [(x[n, ld], d, w)] host arrays (``with_fs``: [(x[n, ld], d, w, fs or None)]) -> (what keeps them alive, [(address of x,
    ld, n, d, address of w)] (``with_fs``: and the address of fs, or 0))"""
    keep = []
    for system in systems:
        x, d, w, f = system if with_fs else (*system, None)
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x.reshape(-1, max(int(d), 1)) if x.ndim != 2 else x
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        f = None if f is None else np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
        if x.shape[0] != w.size or (f is not None and f.size != w.size):
            raise ValueError("%s: rows%s of one length expected" % (who, ", w and fs" if with_fs else " and w"))
        keep.append((x, int(d), w, f))
    fs = (lambda f: (f.ctypes.data if f is not None and f.size else 0,)) if with_fs else (lambda f: ())
    return keep, [(x.ctypes.data if x.size else 0, x.shape[1], w.size, d, w.ctypes.data if w.size else 0) + fs(f) for x, d, w, f in keep]


def _seg_array(seg_type, segs):
    """``segs`` = [(x, ld, n, d, w)] or [(x, ld, n, d, w, fs)], addresses -> the ``SummarySeg`` or ``CovSeg`` array of a call"""
    arr = (seg_type * max(len(segs), 1))()
    for i, (x, ld, n, d, w, *fs) in enumerate(segs):
        arr[i].x, arr[i].ld, arr[i].n, arr[i].d, arr[i].w = x or None, int(ld), int(n), int(d), w or None
        if fs:
            arr[i].fs = fs[0] or None
    return arr


def _split(out, sizes):
    """``out`` cut into the blocks of ``sizes`` doubles, one behind the other"""
    at = np.concatenate(([0], np.cumsum(sizes))).astype(int)
    return [out[at[i]:at[i + 1]] for i in range(len(sizes))]


def param_summary_out_doubles(d, nq):
    return int(load().mce_param_summary_out_doubles(int(d), int(nq)))


def param_summary_workspace_bytes(nrows_total, nrows_max, nseg, dmax, nq, pass_elems=0):
    return int(load().mce_param_summary_workspace_bytes(int(nrows_total), int(nrows_max), int(nseg), int(dmax), int(nq), int(pass_elems)))


def _param_summary(call, segs, q, pass_elems, tail):
    arr = _seg_array(SummarySeg, segs)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    nq = q.size
    sizes = [summary_block_doubles(d, nq) if 1 <= int(d) <= 127 else 0 for _, _, _, d, _, _ in segs]
    out = np.full(max(sum(sizes), 1), np.nan)
    check(call(_c.cast(arr, _P), len(segs), q.ctypes.data, nq, int(pass_elems), out.ctypes.data, *tail))
    return _split(out, sizes)


def summary_block_doubles(d, nq):
    """doubles of one system's result block: MCE_SUMMARY_HEAD + d * (5 + nq)"""
    return MCE_SUMMARY_HEAD + int(d) * (5 + int(nq))


def param_summary_dev(segs, q, ws, ws_bytes, stream=0, pass_elems=0):
    """mce_param_summary_dev: the posterior summary of ``len(segs)`` systems that are on the device -> one float64 block per system
    (``summary.from_block`` reads it); ``segs``: [(device address of the rows, row stride in doubles, rows, measured columns, device
    address of w, device address of fs or 0)], ``q``: the targets"""
    return _param_summary(load().mce_param_summary_dev, segs, q, pass_elems, (ws or None, int(ws_bytes), stream or None))


def param_summary(systems, q, device=0, pass_elems=0):
    """mce_param_summary_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w, fs or None)], uploaded by the library"""
    keep, segs = _host_systems(systems, "param summary", with_fs=True)
    return _param_summary(load().mce_param_summary_f64, segs, q, pass_elems, (int(device),))


def param_cov_out_doubles(d):
    return int(load().mce_param_cov_out_doubles(int(d)))


def param_cov_workspace_bytes(nrows_total, nseg, dmax):
    return int(load().mce_param_cov_workspace_bytes(int(nrows_total), int(nseg), int(dmax)))


def cov_block_doubles(d):
    """doubles of one system's result block: MCE_COV_HEAD + d + d (d + 1) / 2"""
    return MCE_COV_HEAD + int(d) + int(d) * (int(d) + 1) // 2


def _param_cov(call, segs, tail):
    arr = _seg_array(CovSeg, segs)
    sizes = [cov_block_doubles(d) if 1 <= int(d) <= 127 else 0 for _, _, _, d, _ in segs]
    out = np.full(max(sum(sizes), 1), np.nan)
    check(call(_c.cast(arr, _P), len(segs), out.ctypes.data, *tail))
    return _split(out, sizes)


def param_cov_dev(segs, ws, ws_bytes, stream=0):
    """mce_param_cov_dev: the weighted mean and covariance of ``len(segs)`` systems that are on the device -> one float64 block per
    system (``covariance.from_block`` reads it); ``segs``: [(device address of the rows, row stride in doubles, rows, measured columns,
    device address of w)]"""
    return _param_cov(load().mce_param_cov_dev, segs, (ws or None, int(ws_bytes), stream or None))


def param_cov(systems, device=0):
    """mce_param_cov_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w)], uploaded by the library"""
    keep, segs = _host_systems(systems, "param cov")
    return _param_cov(load().mce_param_cov_f64, segs, (int(device),))


def kde_shift_out_doubles():
    return int(load().mce_kde_shift_out_doubles())


def kde_shift_workspace_bytes(nrows_total, nseg, dmax):
    return int(load().mce_kde_shift_workspace_bytes(int(nrows_total), int(nseg), int(dmax)))


def _kde_shift(call, segs, tail):
    """``segs``: [(x, ld, n, d, w, linv, mean, point, c, dens, zout)], linv / mean / point host arrays (or None), the rest addresses"""
    arr = (KdeSeg * max(len(segs), 1))()
    keep = []
    for i, (x, ld, n, d, w, linv, mean, point, c, dens, zout) in enumerate(segs):
        host = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (linv, mean, point)]
        if 1 <= int(d) <= MCE_KDE_MAX_DIM and any(a is not None and a.size != k for a, k in zip(host, (int(d) * int(d), int(d), int(d)))):
            raise ValueError("kde shift: segment %d: linv[d * d], mean[d] and point[d] expected" % i)
        keep.append(host)
        arr[i].x, arr[i].ld, arr[i].n, arr[i].d, arr[i].w = x or None, int(ld), int(n), int(d), w or None
        arr[i].linv, arr[i].mean, arr[i].point = [None if a is None else a.ctypes.data for a in host]
        arr[i].c, arr[i].dens, arr[i].zout = float(c), dens or None, zout or None
    out = np.full(max(len(segs), 1) * MCE_KDE_OUT, np.nan)
    check(call(_c.cast(arr, _P), len(segs), out.ctypes.data, *tail))
    return [out[i * MCE_KDE_OUT:(i + 1) * MCE_KDE_OUT] for i in range(len(segs))]


def kde_shift_dev(segs, ws, ws_bytes, stream=0):
    """mce_kde_shift_dev: the leave-one-out kernel density sums of ``len(segs)`` systems that are on the device -> one float64 block of
    MCE_KDE_OUT doubles per system (``shift_kde.from_block`` reads it); ``segs``: [(device address of the rows, row stride in doubles,
    rows, measured columns, device address of w, linv, mean, point (host arrays), c, device address of the densities or 0, of the
    whitened rows or 0)]"""
    return _kde_shift(load().mce_kde_shift_dev, segs, (ws or None, int(ws_bytes), stream or None))


def kde_shift(systems, device=0, want_dens=False, want_z=False):
    """mce_kde_shift_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w, linv, mean, point, c)], uploaded by the library ->
    [(block, dens[n + 1] or None, z[n, d] or None)]"""
    keep, segs = [], []
    for x, d, w, linv, mean, point, c in systems:
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x.reshape(-1, max(int(d), 1)) if x.ndim != 2 else x
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if x.shape[0] != w.size:
            raise ValueError("kde shift: rows and w of one length expected")
        dens = np.full(w.size + 1, np.nan) if want_dens else None
        z = np.zeros((w.size, max(int(d), 1))) if want_z else None
        keep.append((x, w, dens, z))
        segs.append((x.ctypes.data if x.size else 0, x.shape[1], w.size, int(d), w.ctypes.data if w.size else 0, linv, mean, point, c,
                     0 if dens is None else dens.ctypes.data, 0 if z is None else z.ctypes.data))
    blocks = _kde_shift(load().mce_kde_shift_f64, segs, (int(device),))
    return [(b, k[2], k[3]) for b, k in zip(blocks, keep)]


def param_marginals_out_doubles(d, np_, grid):
    return int(load().mce_param_marginals_out_doubles(int(d), int(np_), int(grid)))


def param_marginals_workspace_bytes(nrows_total, nseg, dmax, np_, grid):
    return int(load().mce_param_marginals_workspace_bytes(int(nrows_total), int(nseg), int(dmax), int(np_), int(grid)))


def marginals_block_doubles(d, np_, grid):
    """doubles of one system's result block: MCE_MARGINALS_HEAD + d * (10 + 4 np + grid)"""
    return MCE_MARGINALS_HEAD + int(d) * (10 + 4 * int(np_) + int(grid))


def _param_marginals(call, segs, bounds, probs, grid, scale, tail):
    """``bounds``: None (the plain entry points), or per system (lo[d], hi[d]) -> the HOST array of a bounded call, 2 d doubles per
    segment, which goes in front of ``probs``"""
    arr = _seg_array(SummarySeg, segs)
    extra = ()
    if bounds is not None:
        if len(bounds) != len(segs):
            raise ValueError("param marginals: one pair of bounds arrays per system expected")
        flat = []
        for (_, _, _, d, _), (lo, hi) in zip(segs, bounds):
            lo, hi = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (lo, hi))
            if lo.size != max(int(d), 0) or hi.size != lo.size:
                raise ValueError("param marginals: %d lower and %d upper bounds for %d columns" % (lo.size, hi.size, d))
            flat += [lo, hi]
        flat = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(0))
        extra = (flat.ctypes.data if flat.size else None,)
    block_doubles = marginals_block_doubles if bounds is None else marginals_bounded_block_doubles
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    npr, grid = probs.size, int(grid)
    shape_ok = 1 <= npr <= MCE_MARGINALS_MAX_P and grid in (64, 128, 256, 512, 1024)
    sizes = [block_doubles(d, npr, grid) if shape_ok and 1 <= int(d) <= 127 else 0 for _, _, _, d, _ in segs]
    out = np.full(max(sum(sizes), 1), np.nan)
    check(call(_c.cast(arr, _P), len(segs), *extra, probs.ctypes.data, npr, grid, float(scale), out.ctypes.data, *tail))
    return _split(out, sizes)


def param_marginals_dev(segs, probs, grid, scale, ws, ws_bytes, stream=0):
    """mce_param_marginals_dev: the 1-D marginal densities, modes and HPD regions of ``len(segs)`` systems that are on the device -> one
    float64 block per system (``marginals.from_block`` reads it); ``segs``: [(device address of the rows, row stride in doubles, rows,
    measured columns, device address of w)]"""
    return _param_marginals(load().mce_param_marginals_dev, segs, None, probs, grid, scale, (ws or None, int(ws_bytes), stream or None))


def param_marginals(systems, probs, grid, scale, device=0):
    """mce_param_marginals_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w)], uploaded by the library"""
    keep, segs = _host_systems(systems, "param marginals")
    return _param_marginals(load().mce_param_marginals_f64, segs, None, probs, grid, scale, (int(device),))


def param_marginals_bounded_out_doubles(d, np_, grid):
    return int(load().mce_param_marginals_bounded_out_doubles(int(d), int(np_), int(grid)))


def param_marginals_bounded_workspace_bytes(nrows_total, nseg, dmax, np_, grid):
    return int(load().mce_param_marginals_bounded_workspace_bytes(int(nrows_total), int(nseg), int(dmax), int(np_), int(grid)))


def marginals_bounded_block_doubles(d, np_, grid):
    """doubles of one system's result block: MCE_MARGINALS_HEAD + d * (14 + 4 np + grid)"""
    return MCE_MARGINALS_HEAD + int(d) * (14 + 4 * int(np_) + int(grid))


def param_marginals_bounded_dev(segs, bounds, probs, grid, scale, ws, ws_bytes, stream=0):
    """mce_param_marginals_bounded_dev: ``param_marginals_dev`` with hard prior bounds, ``bounds`` = [(lo[d], hi[d])] per system (HOST
    arrays, -inf / +inf: open) -> one float64 block per system (``marginals.from_block_bounded`` reads it)"""
    return _param_marginals(load().mce_param_marginals_bounded_dev, segs, bounds, probs, grid, scale, (ws or None, int(ws_bytes), stream or None))


def param_marginals_bounded(systems, bounds, probs, grid, scale, device=0):
    """mce_param_marginals_bounded_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w)], uploaded by the library"""
    keep, segs = _host_systems(systems, "param marginals")
    return _param_marginals(load().mce_param_marginals_bounded_f64, segs, bounds, probs, grid, scale, (int(device),))


def param_contours_out_doubles(nc, np_, grid):
    return int(load().mce_param_contours_out_doubles(int(nc), int(np_), int(grid)))


def param_contours_workspace_bytes(nrows_total, nseg, dmax, nc, np_, grid):
    return int(load().mce_param_contours_workspace_bytes(int(nrows_total), int(nseg), int(dmax), int(nc), int(np_), int(grid)))


def contours_block_doubles(nc, np_, grid):
    """doubles of one system's result block: MCE_CONTOURS_HEAD + 9 nc + P (4 + 7 np + grid^2), P = nc (nc - 1) / 2"""
    nc, grid = int(nc), int(grid)
    return MCE_CONTOURS_HEAD + 9 * nc + (nc * (nc - 1) // 2) * (4 + 7 * int(np_) + grid * grid)


def contours_bounded_block_doubles(nc, np_, grid):
    """doubles of one system's result block: MCE_CONTOURS_HEAD + 13 nc + P (4 + 7 np + grid^2), P = nc (nc - 1) / 2"""
    return contours_block_doubles(nc, np_, grid) + 4 * int(nc)


def _param_contours(call, segs, cols, probs, grid, scale, tail, bounds=None):
    """``bounds``: None (the plain entry points), or per system (lo[nc], hi[nc]) of the chosen columns -> the HOST array of a bounded
    call, 2 nc doubles per segment, which goes in front of ``probs``"""
    arr = _seg_array(SummarySeg, segs)
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    extra = ()
    if bounds is not None:
        if len(bounds) != len(segs):
            raise ValueError("param contours: one pair of bounds arrays per system expected")
        flat = []
        for lo, hi in bounds:
            lo, hi = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (lo, hi))
            if lo.size != cols.size or hi.size != cols.size:
                raise ValueError("param contours: %d lower and %d upper bounds for %d columns" % (lo.size, hi.size, cols.size))
            flat += [lo, hi]
        flat = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(0))
        extra = (flat.ctypes.data if flat.size else None,)
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    npr, grid = probs.size, int(grid)
    shape_ok = 1 <= npr <= MCE_MARGINALS_MAX_P and grid in (32, 64) and 2 <= cols.size <= MCE_CONTOURS_MAX_COLS
    size = (contours_block_doubles if bounds is None else contours_bounded_block_doubles)(cols.size, npr, grid) if shape_ok else 0
    out = np.full(max(size * len(segs), 1), np.nan)
    check(call(_c.cast(arr, _P), len(segs), cols.ctypes.data, cols.size, *extra, probs.ctypes.data, npr, grid, float(scale), out.ctypes.data, *tail))
    return _split(out, [size] * len(segs))


def param_contours_dev(segs, cols, probs, grid, scale, ws, ws_bytes, stream=0):
    """mce_param_contours_dev: the 2-D joint densities, modes and credible regions of every pair of the columns ``cols`` of ``len(segs)``
    systems that are on the device -> one float64 block per system (``contours.from_block`` reads it); ``segs``: [(device address of the
    rows, row stride in doubles, rows, measured columns, device address of w)]"""
    return _param_contours(load().mce_param_contours_dev, segs, cols, probs, grid, scale, (ws or None, int(ws_bytes), stream or None))


def param_contours(systems, cols, probs, grid, scale, device=0):
    """mce_param_contours_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w)], uploaded by the library"""
    keep, segs = _host_systems(systems, "param contours")
    return _param_contours(load().mce_param_contours_f64, segs, cols, probs, grid, scale, (int(device),))


def param_contours_bounded_out_doubles(nc, np_, grid):
    return int(load().mce_param_contours_bounded_out_doubles(int(nc), int(np_), int(grid)))


def param_contours_bounded_workspace_bytes(nrows_total, nseg, dmax, nc, np_, grid):
    return int(load().mce_param_contours_bounded_workspace_bytes(int(nrows_total), int(nseg), int(dmax), int(nc), int(np_), int(grid)))


def param_contours_bounded_dev(segs, cols, bounds, probs, grid, scale, ws, ws_bytes, stream=0):
    """mce_param_contours_bounded_dev: ``param_contours_dev`` with hard prior bounds, ``bounds`` = [(lo[nc], hi[nc])] per system (HOST
    arrays of the chosen columns, -inf / +inf: open) -> one float64 block per system (``contours.from_block_bounded`` reads it)"""
    return _param_contours(load().mce_param_contours_bounded_dev, segs, cols, probs, grid, scale, (ws or None, int(ws_bytes), stream or None), bounds=bounds)


def param_contours_bounded(systems, cols, bounds, probs, grid, scale, device=0):
    """mce_param_contours_bounded_f64: the same from HOST arrays, ``systems`` = [(x[n, ld], d, w)], uploaded by the library"""
    keep, segs = _host_systems(systems, "param contours")
    return _param_contours(load().mce_param_contours_bounded_f64, segs, cols, probs, grid, scale, (int(device),), bounds=bounds)


def jack_groups_dev(segs, stream=0):
    """mce_jack_groups_dev: the jackknife group of every row of ``len(segs)`` systems in one launch.  ``segs``: [(rows, src, part_first,
    n, N, G, by, out)] with rows / src / out device addresses (rows, src: 0 for none), part_first a sequence of the parts' first rows
    (``by="chains"``) or None, by "blocks" / "chains"; int32 [n] is written at ``out``"""
    arr = (JackGroupsSeg * max(len(segs), 1))()
    keep = []
    for i, (rows, src, part_first, n, N, G, by, out) in enumerate(segs):
        pf = np.ascontiguousarray([] if part_first is None else part_first, dtype=np.int64)
        keep.append(pf)
        arr[i].rows, arr[i].src, arr[i].part_first = rows or None, src or None, pf.ctypes.data if pf.size else None
        arr[i].nparts, arr[i].n, arr[i].N, arr[i].G, arr[i].by, arr[i].out = int(pf.size), int(n), int(N), int(G), JACK_BY[by], out or None
    check(load().mce_jack_groups_dev(_c.cast(arr, _P), len(segs), stream or None))


def jack_leave_out_workspace_bytes(nrows_total, nseg, Gmax):
    return int(load().mce_jack_leave_out_workspace_bytes(int(nrows_total), int(nseg), int(Gmax)))


def _jack_leave_out(call, segs, tail):
    arr = (JackLeaveOutSeg * max(len(segs), 1))()
    for i, (w, fs, g, n, G) in enumerate(segs):
        arr[i].w, arr[i].fs, arr[i].g, arr[i].n, arr[i].G = w or None, fs or None, g or None, int(n), int(G)
    nslots = [int(G) + 1 if 0 <= int(G) <= MCE_JACK_MAX_GROUPS else 1 for _, _, _, _, G in segs]
    out = np.full((max(sum(nslots), 1), MCE_JACK_LEAVE_OUT), np.nan)
    check(call(_c.cast(arr, _P), len(segs), out.ctypes.data, *tail))
    at = np.concatenate([[0], np.cumsum(nslots)]).astype(int)
    return [out[at[i]:at[i + 1]].copy() for i in range(len(segs))]


def jack_leave_out_dev(segs, ws, ws_bytes, stream=0):
    """mce_jack_leave_out_dev: the leave-one-group-out blocks of ``len(segs)`` systems that are on the device -> one float64
    [G + 1, 8] per system (``JACK_LEAVE_OUT_FIELDS``; row 0: nothing deleted, row 1 + b: group b deleted); ``segs``: [(device address
    of w, of fs or 0, of the int32 groups, rows, G)]"""
    return _jack_leave_out(load().mce_jack_leave_out_dev, segs, (ws or None, int(ws_bytes), stream or None))


def jack_leave_out(systems, device=0):
    """mce_jack_leave_out_f64: the same from HOST arrays, ``systems`` = [(w, fs or None, g, G)], uploaded by the library"""
    keep = [(np.ascontiguousarray(w, dtype=np.float64).reshape(-1), None if f is None else np.ascontiguousarray(f, dtype=np.float64).reshape(-1),
             np.ascontiguousarray(g, dtype=np.int32).reshape(-1), int(G)) for w, f, g, G in systems]
    if any((f is not None and f.shape != w.shape) or g.shape != w.shape for w, f, g, _ in keep):
        raise ValueError("jackknife leave-out: w, fs and g of one length expected")
    return _jack_leave_out(load().mce_jack_leave_out_f64,
                           [(w.ctypes.data if w.size else 0, f.ctypes.data if f is not None and f.size else 0, g.ctypes.data if g.size else 0, w.size, G)
                            for w, f, g, G in keep], (int(device),))


# ---------------------------------------------------------------------------
# host-pointer wrappers (NumPy in, NumPy out)
# ---------------------------------------------------------------------------
def knn(X, Y, K, self_mode=SELF_NONE, self_offset=0, return_index=True, device=0, options=None):
    """K nearest reference rows (Euclidean) for every query row.  Returns
    (dist[nq,K] ascending, idx[nq,K] int64 or None).  ``options``: an ``Options`` for THIS call (mce_knn_f64_opt)."""
    lib = load()
    X = _f64(X, "X")
    Y = _f64(Y, "Y")
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError("X and Y must be 2-D with the same number of columns, got %r and %r" % (X.shape, Y.shape))
    nq, d = X.shape
    nr = Y.shape[0]
    K = int(K)
    dist = np.empty((nq, K), dtype=np.float64)
    idx = np.empty((nq, K), dtype=np.int64) if return_index else None
    if options is None:
        check(lib.mce_knn_f64(X.ctypes.data, nq, Y.ctypes.data, nr, d, K, int(self_mode), int(self_offset),
                              dist.ctypes.data, idx.ctypes.data if idx is not None else None, int(device)))
    else:
        check(lib.mce_knn_f64_opt(X.ctypes.data, nq, Y.ctypes.data, nr, d, K, int(self_mode), int(self_offset),
                                  dist.ctypes.data, idx.ctypes.data if idx is not None else None, int(device), _c.addressof(options)))
    return dist, idx


def last_verify_rows():
    """rows the run-time certificate of the most recent host-pointer search re-checked (0: it did not run)"""
    return int(load().mce_last_verify_rows())


def verify_knn(X, Y, dist, self_mode=SELF_NONE, self_offset=0, nsample=1024, seed=0, device=0):
    """Run-time certificate of a finished search (mce_verify_knn_f64): ``nsample`` query rows spread over X are re-checked
    against ``dist`` (what ``knn`` returned for them) by an exact fp64 scan of all of Y -- none of the search's machinery.
    NaN and negative entries fail their row, and so does +inf in a column that the usable reference rows could have filled.
    Returns the number of rows that failed (0 = the sample agrees)."""
    lib = load()
    X = _f64(X, "X")
    Y = _f64(Y, "Y")
    dist = _f64_allow_inf(dist)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1] or dist.ndim != 2 or dist.shape[0] != X.shape[0]:
        raise ValueError("shape mismatch: X %r, Y %r, dist %r" % (X.shape, Y.shape, dist.shape))
    failed = _c.c_int32(0)
    rc = lib.mce_verify_knn_f64(X.ctypes.data, X.shape[0], Y.ctypes.data, Y.shape[0], X.shape[1], dist.shape[1], int(self_mode), int(self_offset),
                                dist.ctypes.data, dist.shape[1], int(nsample), int(seed) & (2 ** 64 - 1), _c.addressof(failed), int(device))
    if rc not in (MCE_OK, MCE_ERR_VERIFY):
        check(rc)
    return int(failed.value)


def dotp(dist, w, fs, d, k0, kmax, device=0):
    """sum_j V_d(dist[j,k]) / w[j] * exp(fs[j]) for k in [k0,kmax) (entries < k0 are 0)."""
    lib = load()
    dist = _f64_allow_inf(dist)
    w = _f64(w, "weight")
    fs = _f64_fs(fs)
    if dist.ndim != 2 or w.shape != (dist.shape[0],) or fs.shape != w.shape:
        raise ValueError("shape mismatch: dist %r, w %r, fs %r" % (dist.shape, w.shape, fs.shape))
    out = np.zeros(int(kmax), dtype=np.float64)
    check(lib.mce_dotp_f64(dist.ctypes.data, dist.shape[0], dist.shape[1], int(k0), int(kmax), int(d),
                           w.ctypes.data, fs.ctypes.data, out.ctypes.data, int(device)))
    return out


def _f64_allow_inf(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def knn_dotp(X, Y, w, fs, kmax, k0, self_offset=0, return_dist=False, devices=None):
    """Fused search + reduction.  Returns dotp[kmax] (and dist[nq,kmax-k0] if asked)."""
    lib = load()
    X = _f64(X, "X")
    Y = X if Y is None else _f64(Y, "Y")
    w = _f64(w, "weight")
    fs = _f64_fs(fs)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError("X and Y must be 2-D with the same number of columns")
    nq, d = X.shape
    if w.shape != (nq,) or fs.shape != (nq,):
        raise ValueError("weight and fs must have one entry per query row")
    out = np.zeros(int(kmax), dtype=np.float64)
    dist = np.empty((nq, int(kmax) - int(k0)), dtype=np.float64) if return_dist else None
    if devices is None:
        devs, ndev = None, 0
    else:
        arr = (ctypes.c_int32 * len(devices))(*[int(x) for x in devices])
        devs, ndev = ctypes.cast(arr, ctypes.c_void_p), len(devices)
    check(lib.mce_knn_dotp_f64(X.ctypes.data, nq, Y.ctypes.data, Y.shape[0], d, int(kmax), int(k0), int(self_offset),
                               w.ctypes.data, fs.ctypes.data, out.ctypes.data,
                               dist.ctypes.data if dist is not None else None, devs, ndev))
    return (out, dist) if return_dist else out


def knn_dotp_part(Y, w, fs, kmax, part, nparts, device=0):
    """Partial auto-evidence sums over part ``part`` of ``nparts`` of the queries (the library chooses the
    partition; the parts add up to ``knn_dotp(Y, None, w, fs, kmax, 1)``).  One call per rank / device."""
    lib = load()
    Y = _f64(Y, "Y")
    w = _f64(w, "weight")
    fs = _f64_fs(fs)
    if Y.ndim != 2 or w.shape != (Y.shape[0],) or fs.shape != w.shape:
        raise ValueError("Y must be 2-D, weight and fs one entry per row")
    out = np.zeros(int(kmax), dtype=np.float64)
    check(lib.mce_knn_dotp_part_f64(Y.ctypes.data, Y.shape[0], Y.shape[1], int(kmax), int(part), int(nparts),
                                    w.ctypes.data, fs.ctypes.data, out.ctypes.data, int(device)))
    return out


def _rows_f64(a, name, d, check=True):
    """2-D fp64 array whose rows are contiguous in their first d columns (row stride arbitrary).
    ``check=False``: the callee detects NaN / infinity itself (the device covariance turns non-finite and
    the call fails with ValueError), sparing a host pass over the whole matrix."""
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < d:
        raise ValueError("%s must be 2-D with at least %d columns" % (name, d))
    if a.dtype != np.float64 or a.strides[1] != 8 or a.strides[0] % 8 != 0 or a.strides[0] < 8 * d:
        a = np.ascontiguousarray(a[:, :d], dtype=np.float64)
    if check and not np.all(np.isfinite(a[:, :d])):
        raise ValueError("%s contains NaN or infinity" % name)
    return a


def _feed_host_args(S1, S2, d, w, f, sentence, shifted=True):
    """The host inputs of a feed entry point: ((S1, S2, w, f) as the checked fp64 arrays the library reads -- keep them alive over the
    call --, (S1, n1, ld1, S2, n2, ld2) as its leading ctypes arguments).  ``f``: the likelihood terms fs (``_f64_fs``), or with
    ``shifted=False`` the log-likelihoods as they are; ``sentence``: the caller's words for w / f without one entry per row of S1."""
    S1 = _rows_f64(S1, "samples", d, check=False)
    S2 = None if S2 is None else _rows_f64(S2, "samples2", d, check=False)
    w = _f64(w, "weight")
    f = _f64_fs(f) if shifted else np.ascontiguousarray(f, dtype=np.float64)
    if w.shape != (S1.shape[0],) or f.shape != w.shape:
        raise ValueError(sentence)
    rows2 = (None, 0, 0) if S2 is None else (S2.ctypes.data, S2.shape[0], S2.strides[0] // 8)
    return (S1, S2, w, f), (S1.ctypes.data, S1.shape[0], S1.strides[0] // 8) + rows2


def evidence_feed(S1, S2, d, cov_mode, kmax, w, fs, device=0):
    """Covariance + whitening + kNN + reduction on the device from ONE upload of the raw parameter
    rows.  Returns (dotp[kmax], jacobian, eigenvalues[d])."""
    lib = load()
    (S1, S2, w, fs), rows = _feed_host_args(S1, S2, d, w, fs, "weight and fs must have one entry per s1 row")
    out = np.zeros(int(kmax))
    jac = ctypes.c_double(0.0)
    ev = np.zeros(int(d))
    check(lib.mce_evidence_feed_f64(*rows, int(d), int(cov_mode), int(kmax),
                                    w.ctypes.data, fs.ctypes.data, out.ctypes.data, ctypes.byref(jac), ev.ctypes.data, int(device)))
    return out, float(jac.value), ev


def evidence_feed_part(S1, S2, d, cov_mode, kmax, w, fs, part, nparts, device=0, want_checksum=True):
    """One rank's share of ``evidence_feed`` (``mce_evidence_feed_part_f64``): every rank passes the same arrays, uploads them
    once, whitens on its device and searches its share.  Returns (dotp_part[kmax], jacobian, eigenvalues[d], checksum) --
    the partial sums still to be all-reduced over the ranks, and the device-side fingerprint of the uploaded inputs
    (None if not asked for)."""
    lib = load()
    (S1, S2, w, fs), rows = _feed_host_args(S1, S2, d, w, fs, "weight and fs must have one entry per s1 row")
    out = np.zeros(int(kmax))
    jac = ctypes.c_double(0.0)
    ev = np.zeros(int(d))
    csum = ctypes.c_uint64(0)
    check(lib.mce_evidence_feed_part_f64(*rows, int(d), int(cov_mode), int(kmax),
                                         w.ctypes.data, fs.ctypes.data, int(part), int(nparts), out.ctypes.data, ctypes.byref(jac),
                                         ev.ctypes.data, ctypes.byref(csum) if want_checksum else None, int(device)))
    return out, float(jac.value), ev, (int(csum.value) if want_checksum else None)


def evidence_feed_part_dev(dS1, n1, ld1, dS2, n2, ld2, d, cov_mode, kmax, d_w, d_fs, part, nparts, device=0, want_checksum=True):
    """``evidence_feed_part`` with the inputs on the device already (``mce_evidence_feed_part_dev_f64``): device POINTERS (rows
    ``ld`` doubles apart; ``dS2`` = 0 for auto evidence), produced on a stream the caller has synchronised.  Same returns."""
    lib = load()
    out = np.zeros(int(kmax))
    jac = ctypes.c_double(0.0)
    ev = np.zeros(int(d))
    csum = ctypes.c_uint64(0)
    check(lib.mce_evidence_feed_part_dev_f64(dS1, int(n1), int(ld1), dS2 or None, int(n2) if dS2 else 0, int(ld2) if dS2 else 0, int(d), int(cov_mode), int(kmax),
                                             d_w, d_fs, int(part), int(nparts), out.ctypes.data, ctypes.byref(jac), ev.ctypes.data,
                                             ctypes.byref(csum) if want_checksum else None, int(device)))
    return out, float(jac.value), ev, (int(csum.value) if want_checksum else None)


def evidence_feed_whiten_dev(dS1, n1, ld1, d, kmax, d_w, d_fs, d_X_out, d_w_out, d_fs_out, device=0, want_checksum=True):
    """``evidence_feed_whiten`` with the inputs on the device already (``mce_evidence_feed_whiten_dev_f64``)."""
    lib = load()
    jac = ctypes.c_double(0.0)
    ev = np.zeros(int(d))
    csum = ctypes.c_uint64(0)
    check(lib.mce_evidence_feed_whiten_dev_f64(dS1, int(n1), int(ld1), int(d), int(kmax), d_w, d_fs, d_X_out, d_w_out, d_fs_out, ctypes.byref(jac),
                                               ev.ctypes.data, ctypes.byref(csum) if want_checksum else None, int(device)))
    return float(jac.value), ev, (int(csum.value) if want_checksum else None)


def evidence_feed_whiten(S1, d, kmax, w, fs, d_X_out, d_w_out, d_fs_out, device=0, want_checksum=True):
    """The feeders alone (``mce_evidence_feed_whiten_f64``, auto evidence): upload, covariance, eigen-system, whitening; the
    whitened rows, weights and likelihood terms are left in the caller's DEVICE buffers (pointers; [n, d], [n], [n] doubles).
    Returns (jacobian, eigenvalues[d], checksum)."""
    lib = load()
    (S1, _, w, fs), rows = _feed_host_args(S1, None, d, w, fs, "weight and fs must have one entry per row")
    jac = ctypes.c_double(0.0)
    ev = np.zeros(int(d))
    csum = ctypes.c_uint64(0)
    check(lib.mce_evidence_feed_whiten_f64(*rows[:3], int(d), int(kmax), w.ctypes.data, fs.ctypes.data,
                                           d_X_out, d_w_out, d_fs_out, ctypes.byref(jac), ev.ctypes.data,
                                           ctypes.byref(csum) if want_checksum else None, int(device)))
    return float(jac.value), ev, (int(csum.value) if want_checksum else None)


def _prefix_arg(prefix):
    prefix = np.ascontiguousarray(prefix, dtype=np.int64)
    if prefix.ndim != 1:
        raise ValueError("prefix must be a 1-D sequence of row counts")
    return prefix


def evidence_feed_prefix(S1, S2, d, cov_mode, kmax, w, logl, prefix, device=0):
    """Convergence batches in ONE library call (``mce_evidence_feed_prefix_f64``): entry b is ``evidence_feed`` on the first
    ``prefix[b]`` rows of S1 with ``fs = logl[:p] - max(logl[:p])`` -- with ``cov_mode`` 0 whitened by the eigen-system of ALL rows.
    ``logl``: the log-likelihoods, not shifted (a NaN makes every prefix that holds it NaN, like ``np.amax``).
    Returns (dotp[B, kmax], loglmax[B], jacobian[B])."""
    lib = load()
    (S1, S2, w, logl), rows = _feed_host_args(S1, S2, d, w, logl, "weight and logl must have one entry per s1 row", shifted=False)
    prefix = _prefix_arg(prefix)
    B = len(prefix)
    out = np.zeros((max(B, 1), max(int(kmax), 0)))
    lmax = np.zeros(max(B, 1))
    jac = np.zeros(max(B, 1))
    check(lib.mce_evidence_feed_prefix_f64(*rows, int(d), int(cov_mode), int(kmax),
                                           w.ctypes.data, logl.ctypes.data, prefix.ctypes.data if B else None, B,
                                           out.ctypes.data, lmax.ctypes.data, jac.ctypes.data, int(device)))
    return out[:B], lmax[:B], jac[:B]


def evidence_feed_prefix_dev(dS1, n1, ld1, dS2, n2, ld2, d, cov_mode, kmax, d_w, d_logl, prefix, device=0):
    """``evidence_feed_prefix`` with the inputs on the device already (``mce_evidence_feed_prefix_dev_f64``): device ADDRESSES on
    ``device`` (rows ``ld`` doubles apart; ``dS2`` = 0 for auto evidence), produced on a stream the caller has synchronised.
    ``prefix`` and the returns stay host-side."""
    lib = load()
    prefix = _prefix_arg(prefix)
    B = len(prefix)
    out = np.zeros((max(B, 1), max(int(kmax), 0)))
    lmax = np.zeros(max(B, 1))
    jac = np.zeros(max(B, 1))
    check(lib.mce_evidence_feed_prefix_dev_f64(dS1 or None, int(n1), int(ld1), dS2 or None, int(n2) if dS2 else 0, int(ld2) if dS2 else 0, int(d),
                                               int(cov_mode), int(kmax), d_w or None, d_logl or None, prefix.ctypes.data if B else None, B,
                                               out.ctypes.data, lmax.ctypes.data, jac.ctypes.data, int(device)))
    return out[:B], lmax[:B], jac[:B]


def _devices_arg(devices):
    if devices is None:
        return None, 0
    arr = (ctypes.c_int32 * len(devices))(*[int(x) for x in devices])
    return arr, len(devices)


def _raise_for(rc, msg):
    if rc in (MCE_ERR_INVALID, MCE_ERR_K_RANGE, MCE_ERR_WORKSPACE, MCE_ERR_DIM_RANGE):
        return ValueError(msg)
    return RuntimeError("mcevidence_amd HIP backend: " + msg)


def evidence_feed_batch(problems, devices=None, return_exceptions=False):
    """Many independent evidence problems in ONE library call (``mce_evidence_feed_batch_f64``).

    ``problems``: sequence of ``(S1, S2, d, cov_mode, kmax, w, fs)`` with the meaning of
    :func:`evidence_feed`.  Returns a list of ``(dotp[kmax], jacobian, eigenvalues[d])`` in the same
    order.  A failing problem raises (the first one, like a loop of single calls would) unless
    ``return_exceptions`` is set, in which case its slot holds the exception instead."""
    lib = load()
    n = len(problems)
    arr = (FeedProblem * max(n, 1))()
    keep = []                                  # arrays the C struct points into
    outs = []
    for i, (S1, S2, d, cov_mode, kmax, w, fs) in enumerate(problems):
        d, kmax = int(d), int(kmax)
        (S1, S2, w, fs), rows = _feed_host_args(S1, S2, d, w, fs, "problem %d: weight and fs must have one entry per s1 row" % i)
        out = np.zeros(max(kmax, 0))
        ev = np.zeros(max(d, 0))
        keep.append((S1, S2, w, fs))
        outs.append((out, ev))
        q = arr[i]
        q.S1, q.n1, q.ld1, q.S2, q.n2, q.ld2 = rows
        q.d, q.cov_mode, q.kmax = d, int(cov_mode), kmax
        q.w, q.fs, q.dotp, q.eigenvalues = w.ctypes.data, fs.ctypes.data, out.ctypes.data, ev.ctypes.data
    devs, ndev = _devices_arg(devices)
    rc = lib.mce_evidence_feed_batch_f64(arr, n, ctypes.cast(devs, _P) if devs is not None else None, ndev)
    if rc != MCE_OK and all(arr[i].status == MCE_OK for i in range(n)):
        check(rc)                              # the machinery failed (allocation, device), not a problem
    results = []
    for i in range(n):
        st = int(arr[i].status)
        if st == MCE_OK:
            results.append((outs[i][0], float(arr[i].jacobian), outs[i][1]))
            continue
        # the library keeps only the first failure's text; later ones get a generic message
        first = all(int(arr[j].status) == MCE_OK for j in range(i))
        exc = _raise_for(st, last_error() if first else "problem %d failed with status %d" % (i, st))
        if not return_exceptions:
            raise exc
        results.append(exc)
    return results


def evidence_feed_batch_dev(problems, device=0, return_exceptions=False):
    """``evidence_feed_batch`` with the inputs on the device already (``mce_evidence_feed_batch_dev_f64``).  ``problems``: sequence
    of ``(dS1, n1, ld1, dS2, n2, ld2, d, cov_mode, kmax, d_w, d_fs)`` -- device ADDRESSES on ``device`` (``dS2`` = 0: auto evidence),
    produced on a stream the caller has synchronised.  Same returns and failure semantics."""
    lib = load()
    n = len(problems)
    arr = (FeedProblem * max(n, 1))()
    outs = []
    for i, (dS1, n1, ld1, dS2, n2, ld2, d, cov_mode, kmax, d_w, d_fs) in enumerate(problems):
        d, kmax = int(d), int(kmax)
        out = np.zeros(max(kmax, 0))
        ev = np.zeros(max(d, 0))
        outs.append((out, ev))
        q = arr[i]
        q.S1, q.n1, q.ld1 = dS1 or None, int(n1), int(ld1)
        if dS2:
            q.S2, q.n2, q.ld2 = dS2, int(n2), int(ld2)
        q.d, q.cov_mode, q.kmax = d, int(cov_mode), kmax
        q.w, q.fs, q.dotp, q.eigenvalues = d_w or None, d_fs or None, out.ctypes.data, ev.ctypes.data
    rc = lib.mce_evidence_feed_batch_dev_f64(arr, n, int(device))
    if rc != MCE_OK and all(arr[i].status == MCE_OK for i in range(n)):
        check(rc)                              # the machinery failed (allocation, device), not a problem
    results = []
    for i in range(n):
        st = int(arr[i].status)
        if st == MCE_OK:
            results.append((outs[i][0], float(arr[i].jacobian), outs[i][1]))
            continue
        first = all(int(arr[j].status) == MCE_OK for j in range(i))
        exc = _raise_for(st, last_error() if first else "problem %d failed with status %d" % (i, st))
        if not return_exceptions:
            raise exc
        results.append(exc)
    return results


# ---------------------------------------------------------------------------
# device-pointer wrappers (raw addresses: torch tensors' data_ptr(), stream handle)
# ---------------------------------------------------------------------------
def knn_workspace_bytes(nq, nr, d, K, options=None):
    """Scratch bytes a *_dev search needs.  ``options=Options(same_set=0)``: queries and references will be two buffers
    (cross evidence with equal halves): no scratch for the symmetric sweep is reserved."""
    if options is None:
        n = int(load().mce_knn_workspace_bytes(int(nq), int(nr), int(d), int(K)))
    else:
        n = int(load().mce_knn_workspace_bytes_opt(int(nq), int(nr), int(d), int(K), _c.addressof(options)))
    if n == 0:
        raise ValueError(last_error())
    return n


def dotp_workspace_bytes(nq, kmax):
    return int(load().mce_dotp_workspace_bytes(int(nq), int(kmax)))


def knn_dev(dX, nq, dY, nr, d, K, self_mode, self_offset, d_dist, d_idx, ws, ws_bytes, stream=0):
    check(load().mce_knn_f64_dev(dX, nq, dY, nr, d, K, self_mode, self_offset, d_dist, d_idx or None, ws, ws_bytes, stream or None))


def verify_workspace_bytes(nsample, K):
    """scratch bytes of ``verify_knn_dev`` (0: invalid sizes)"""
    return int(load().mce_verify_workspace_bytes(int(nsample), int(K)))


def verify_knn_dev(dX, nq, dY, nr, d, K, self_mode, self_offset, d_dist, ld, nsample, seed, d_result, ws, ws_bytes, stream=0):
    """mce_verify_knn_f64_dev: the run-time certificate on device buffers, on the caller's stream, never synchronises;
    ``d_result`` (2 int32 on the device) receives {rows checked, rows that failed}.  Returns the error code (MCE_OK: launched)."""
    return int(load().mce_verify_knn_f64_dev(dX, int(nq), dY, int(nr), int(d), int(K), int(self_mode), int(self_offset), d_dist, int(ld), int(nsample),
                                             int(seed) & (2 ** 64 - 1), d_result, ws, int(ws_bytes), stream or None))


def dotp_dev(d_dist, nq, ld, k0, kmax, d, d_w, d_fs, d_dotp, ws, ws_bytes, stream=0):
    check(load().mce_dotp_f64_dev(d_dist, nq, ld, k0, kmax, d, d_w, d_fs, d_dotp, ws, ws_bytes, stream or None))


def jack_workspace_bytes(nq, G, kmax):
    """scratch bytes of ``jack_dotp_dev``"""
    n = int(load().mce_jack_workspace_bytes(int(nq), int(G), int(kmax)))
    if n == 0:
        raise ValueError("jackknife: invalid sizes nq=%d G=%d kmax=%d" % (nq, G, kmax))
    return n


def jack_dotp_dev(d_dist, d_idx, nq, L, d_qid, d_gq, d_gr, nr, G, k0, kmax, d, d_w, d_fs, d_dotp_groups, d_dotp_full, d_short_rows, d_nshort,
                  ws, ws_bytes, stream=0):
    """the leave-one-group-out sums of lists that are on the device (``mce_jack_dotp_dev``); device POINTERS, the stream is
    synchronised on return"""
    check(load().mce_jack_dotp_dev(d_dist, d_idx, int(nq), int(L), d_qid or None, d_gq, d_gr, int(nr), int(G), int(k0), int(kmax), int(d), d_w, d_fs,
                                   d_dotp_groups, d_dotp_full, d_short_rows, d_nshort, ws, ws_bytes, stream or None))


def jack_dotp(dist, idx, gq, gr, G, k0, kmax, d, w, fs, qid=None, device=0):
    """``mce_jack_dotp_f64``: the leave-one-group-out sums from neighbour lists ``dist`` / ``idx`` [nq, L] on the host.
    Returns (dotp_groups[G, kmax], dotp_full[kmax], short_rows int64, ascending)."""
    lib = load()
    dist = _f64_allow_inf(dist)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    gq = np.ascontiguousarray(gq, dtype=np.int32)
    gr = np.ascontiguousarray(gr, dtype=np.int32)
    w = _f64(w, "weight")
    fs = _f64_fs(fs)
    if dist.ndim != 2 or idx.shape != dist.shape or w.shape != (dist.shape[0],) or fs.shape != w.shape or gq.shape != w.shape or gr.ndim != 1:
        raise ValueError("shape mismatch: dist %r, idx %r, w %r, fs %r, gq %r, gr %r" % (dist.shape, idx.shape, w.shape, fs.shape, gq.shape, gr.shape))
    nq, L = dist.shape
    if qid is not None:
        qid = np.ascontiguousarray(qid, dtype=np.int64)
        if qid.shape != (nq,):
            raise ValueError("qid must have one entry per query row")
    G, kmax = int(G), int(kmax)
    groups = np.zeros((max(G, 1), max(kmax, 1)), dtype=np.float64)
    full = np.zeros(max(kmax, 1), dtype=np.float64)
    short = np.zeros(max(nq, 1), dtype=np.int64)
    nshort = _c.c_int64(0)
    check(lib.mce_jack_dotp_f64(dist.ctypes.data, idx.ctypes.data, nq, L, qid.ctypes.data if qid is not None else None, gq.ctypes.data, gr.ctypes.data,
                                gr.shape[0], G, int(k0), kmax, int(d), w.ctypes.data, fs.ctypes.data, groups.ctypes.data, full.ctypes.data,
                                short.ctypes.data, _c.addressof(nshort), int(device)))
    return groups, full, short[:int(nshort.value)].copy()


def div_whiten_workspace_bytes(n, d):
    """scratch bytes of ``div_whiten_dev``"""
    nb = int(load().mce_div_whiten_workspace_bytes(int(n), int(d)))
    if nb == 0:
        raise ValueError("knn divergence: invalid sizes n=%d d=%d" % (n, d))
    return nb


def _div_metric(linv, mean, d):
    linv = np.ascontiguousarray(linv, dtype=np.float64)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    if 1 <= int(d) <= MCE_DIV_MAX_DIM and (linv.size != int(d) * int(d) or mean.size != int(d)):
        raise ValueError("knn divergence: linv[d * d] and mean[d] expected")
    return linv, mean


def div_whiten_dev(d_x, ld, n, d, linv, mean, d_w, d_z, ws, ws_bytes, stream=0):
    """``mce_div_whiten_dev``: z = linv (x - mean) of rows that are on the device, into ``d_z`` (packed [n, d]); ``linv`` / ``mean`` are host
    arrays.  Returns the report: (sum of w, weights that are not > 0 or not finite, lowest non-finite column or -1, rows)."""
    linv, mean = _div_metric(linv, mean, d)
    report = np.full(MCE_DIV_REPORT, np.nan)
    check(load().mce_div_whiten_dev(d_x or None, int(ld), int(n), int(d), linv.ctypes.data, mean.ctypes.data, d_w or None, d_z or None, report.ctypes.data,
                                    ws or None, int(ws_bytes), stream or None))
    return report


def div_whiten(x, d, linv, mean, w, device=0):
    """``mce_div_whiten_f64``: the same from HOST arrays ``x`` [n, ld] and ``w`` [n] -> (z[n, d], report)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or x.shape[0] != w.size:
        raise ValueError("knn divergence: rows and w of one length expected")
    linv, mean = _div_metric(linv, mean, d)
    z = np.zeros((w.size, max(int(d), 1)))
    report = np.full(MCE_DIV_REPORT, np.nan)
    check(load().mce_div_whiten_f64(x.ctypes.data, x.shape[1], w.size, int(d), linv.ctypes.data, mean.ctypes.data, w.ctypes.data, z.ctypes.data,
                                    report.ctypes.data, int(device)))
    return z, report


def knn_div_workspace_bytes(nq, nP, G, K):
    """scratch bytes of ``knn_div_terms_dev``"""
    n = int(load().mce_knn_div_workspace_bytes(int(nq), int(nP), int(G), int(K)))
    if n == 0:
        raise ValueError("knn divergence: invalid sizes nq=%d nP=%d G=%d K=%d" % (nq, nP, G, K))
    return n


def knn_div_terms_dev(d_distP, d_idxP, d_distQ, d_idxQ, nq, L, d_qid, d_gq, d_grP, nP, d_grQ, nQ, G, K, d, d_aq, d_aP, d_bQ, d_sums, d_short_rows,
                      d_nshort, ws, ws_bytes, stream=0):
    """the sums of the k-NN relative entropy from lists that are on the device (``mce_knn_div_terms_dev``); device POINTERS, the stream
    is synchronised on return"""
    check(load().mce_knn_div_terms_dev(d_distP, d_idxP, d_distQ, d_idxQ, int(nq), int(L), d_qid or None, d_gq or None, d_grP or None, int(nP),
                                       d_grQ or None, int(nQ), int(G), int(K), int(d), d_aq, d_aP, d_bQ, d_sums, d_short_rows, d_nshort, ws, int(ws_bytes),
                                       stream or None))


def knn_div_terms(distP, idxP, distQ, idxQ, gq, grP, grQ, G, K, d, aq, aP, bQ, qid=None, device=0):
    """``mce_knn_div_terms_f64``: the sums from the two neighbour lists [nq, L] of every query row on the host; ``gq`` / ``grP`` / ``grQ``
    may be None where ``G`` is 0.  Returns (sums[G + 1, K, 2], short_rows int64, ascending)."""
    lib = load()
    distP, distQ = _f64_allow_inf(distP), _f64_allow_inf(distQ)
    idxP, idxQ = np.ascontiguousarray(idxP, dtype=np.int64), np.ascontiguousarray(idxQ, dtype=np.int64)
    aq, aP, bQ = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (aq, aP, bQ))
    if distP.ndim != 2 or idxP.shape != distP.shape or distQ.shape != distP.shape or idxQ.shape != distP.shape or aq.shape != (distP.shape[0],):
        raise ValueError("shape mismatch: distP %r, idxP %r, distQ %r, idxQ %r, aq %r" % (distP.shape, idxP.shape, distQ.shape, idxQ.shape, aq.shape))
    nq, L = distP.shape
    groups = [None if g is None else np.ascontiguousarray(g, dtype=np.int32).reshape(-1) for g in (gq, grP, grQ)]
    for g, n, what in zip(groups, (nq, aP.size, bQ.size), ("gq", "grP", "grQ")):
        if g is not None and g.size != n:
            raise ValueError("knn divergence: %s must have one entry per row" % what)
    if qid is not None:
        qid = np.ascontiguousarray(qid, dtype=np.int64)
        if qid.shape != (nq,):
            raise ValueError("qid must have one entry per query row")
    G, K = int(G), int(K)
    sums = np.zeros((max(G, 0) + 1, max(K, 1), 2), dtype=np.float64)
    short = np.zeros(max(nq, 1), dtype=np.int64)
    nshort = _c.c_int64(0)
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    check(lib.mce_knn_div_terms_f64(distP.ctypes.data, idxP.ctypes.data, distQ.ctypes.data, idxQ.ctypes.data, nq, L, ptr(qid), ptr(groups[0]), ptr(groups[1]),
                                    aP.size, ptr(groups[2]), bQ.size, G, K, int(d), aq.ctypes.data, aP.ctypes.data, bQ.ctypes.data, sums.ctypes.data,
                                    short.ctypes.data, _c.addressof(nshort), int(device)))
    return sums, short[:int(nshort.value)].copy()


def prune_part_applies(nr, d, kmax, nparts):
    """Does an auto-evidence search of this shape on ``nparts`` ranks take the pruned walk with a preparation that can be distributed?"""
    return bool(load().mce_prune_part_applies(int(nr), int(d), int(kmax), int(nparts)))


def prune_part_prepare_dev(dY, nr, d, kmax, part, nparts, ws, ws_bytes, stream=0, want_range=False):
    """This rank's part of the DISTRIBUTED k-d preparation of a pruned auto-evidence search (``mce_prune_part_prepare_dev``): returns
    (byte offset into ``ws``, count) of the int32 permutation array -- final inside the rank's range, zeros elsewhere: gather the
    ranges (or all-reduce(SUM) the array) over the ranks, then ``knn_dotp_part_prepared_dev`` -- or (0, 0) when there is nothing to
    exchange (call ``knn_dotp_part_dev``).  ``want_range``: also the rank's range (lo, hi) in positions."""
    off, cnt, lo, hi = _c.c_size_t(0), _c.c_int64(0), _c.c_int64(0), _c.c_int64(0)
    check(load().mce_prune_part_prepare_dev(dY, nr, d, kmax, part, nparts, _c.byref(off), _c.byref(cnt), _c.byref(lo), _c.byref(hi), ws, ws_bytes, stream or None))
    if want_range:
        return int(off.value), int(cnt.value), int(lo.value), int(hi.value)
    return int(off.value), int(cnt.value)


def knn_dotp_part_prepared_dev(dY, nr, d, kmax, part, nparts, d_w, d_fs, d_dotp, ws, ws_bytes, stream=0):
    check(load().mce_knn_dotp_part_prepared_f64_dev(dY, nr, d, kmax, part, nparts, d_w, d_fs, d_dotp, ws, ws_bytes, stream or None))


def knn_dotp_part_dev(dY, nr, d, kmax, part, nparts, d_w, d_fs, d_dotp, ws, ws_bytes, stream=0):
    check(load().mce_knn_dotp_part_f64_dev(dY, nr, d, kmax, part, nparts, d_w, d_fs, d_dotp, ws, ws_bytes, stream or None))


def pairs_once_blocks(nr, d, kmax):
    """Sorted 512-row blocks of the all-pairs-once partition for this shape (the length of its flags array); 0: the shape
    does not take the one-pass symmetric sweep and the partition does not exist (``mce_pairs_once_blocks``)."""
    return int(load().mce_pairs_once_blocks(int(nr), int(d), int(kmax)))


def pairs_once_workspace_bytes(nr, d, kmax, nparts):
    return int(load().mce_pairs_once_workspace_bytes(int(nr), int(d), int(kmax), int(nparts)))


def pairs_once_prepare_dev(dY, nr, d, kmax, part, nparts, ws, ws_bytes, stream=0):
    """-> (byte offset of the rows' bounds inside the workspace, their number): float64, to be all-reduced with MIN"""
    off, cnt = _c.c_size_t(0), _c.c_int64(0)
    check(load().mce_pairs_once_prepare_dev(dY, nr, d, kmax, part, nparts, _c.byref(off), _c.byref(cnt), ws, ws_bytes, stream or None))
    return int(off.value), int(cnt.value)


def pairs_once_sweep_dev(dY, nr, d, kmax, part, nparts, d_counts, d_flags, ws, ws_bytes, stream=0):
    check(load().mce_pairs_once_sweep_dev(dY, nr, d, kmax, part, nparts, d_counts, d_flags, ws, ws_bytes, stream or None))


def pairs_once_export_dev(nr, d, kmax, part, nparts, d_send, ws, ws_bytes, stream=0):
    check(load().mce_pairs_once_export_dev(nr, d, kmax, part, nparts, d_send or None, ws, ws_bytes, stream or None))


def pairs_once_finish_dev(dY, nr, d, kmax, part, nparts, d_w, d_fs, d_recv, nrecv, d_flags, d_dotp, ws, ws_bytes, stream=0):
    check(load().mce_pairs_once_finish_dev(dY, nr, d, kmax, part, nparts, d_w, d_fs, d_recv or None, nrecv, d_flags, d_dotp, ws, ws_bytes,
                                           stream or None))


def knn_dotp_dev(dX, nq, dY, nr, d, kmax, k0, self_offset, d_w, d_fs, d_dotp, d_dist_out, ws, ws_bytes, stream=0):
    check(load().mce_knn_dotp_f64_dev(dX, nq, dY, nr, d, kmax, k0, self_offset, d_w, d_fs, d_dotp, d_dist_out or None,
                                      ws, ws_bytes, stream or None))


def debug_mfma_tile(yprime, xprime, device=0):
    """Test hook (mce_debug_mfma_tile_f16): the 32 x 32 fp32 tile ``yprime @ xprime.T`` as the filter kernels' MFMA
    sequence computes it; ``yprime``, ``xprime``: float16 arrays [32, 16 * kst]."""
    y = np.ascontiguousarray(yprime, dtype=np.float16)
    x = np.ascontiguousarray(xprime, dtype=np.float16)
    if y.shape != x.shape or y.shape[0] != 32 or y.shape[1] % 16 or not 1 <= y.shape[1] // 16 <= 8:
        raise ValueError("yprime and xprime must be float16 [32, 16*kst], kst = 1..8")
    out = np.empty((32, 32), dtype=np.float32)
    check(load().mce_debug_mfma_tile_f16(y.ctypes.data, x.ctypes.data, y.shape[1] // 16, out.ctypes.data, int(device)))
    return out


def debug_mfma_tiles(yprime, xprime, device=0):
    """``debug_mfma_tile`` for a batch: float16 arrays [ntiles, 32, 16 * kst] -> float32 [ntiles, 32, 32] (row, query)."""
    y = np.ascontiguousarray(yprime, dtype=np.float16)
    x = np.ascontiguousarray(xprime, dtype=np.float16)
    if y.ndim != 3 or y.shape != x.shape or y.shape[1] != 32 or y.shape[2] % 16 or not 1 <= y.shape[2] // 16 <= 8:
        raise ValueError("yprime and xprime must be float16 [ntiles, 32, 16*kst], kst = 1..8")
    out = np.empty((y.shape[0], 32, 32), dtype=np.float32)
    check(load().mce_debug_mfma_tiles_f16(y.ctypes.data, x.ctypes.data, y.shape[2] // 16, y.shape[0], out.ctypes.data, int(device)))
    return out
