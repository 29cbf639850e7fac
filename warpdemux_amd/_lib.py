"""ctypes binding of libwdx_hip.so (C ABI: include/wdx.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C warpdemux_amd/csrc``.
There is NO CPU fallback: if the shared object is missing or no MI355X is visible, every entry
point raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $WDX_LIB_PATH: development only (tools/ab.sh benches two builds of the library in one GPU session)
LIB_PATH = os.environ.get("WDX_LIB_PATH") or os.path.join(_HERE, "csrc", "libwdx_hip.so")

WDX_SUCCESS = 0
WDX_ERR_INVALID = -1
WDX_ERR_NO_DEVICE = -2
WDX_ERR_HIP = -3
WDX_ERR_UNSUPPORTED = -4
WDX_ERR_NO_REFS = -5

K_FINGERPRINT, K_DTW, K_TRANSPOSE, K_COUNT, K_SVM, K_REDUCE, K_FINGERPRINT_MAIN, K_FINGERPRINT_CLIP, K_FINGERPRINT_TAIL = 0, 1, 2, 3, 4, 5, 6, 7, 8
K_MLP = 9
K_BOOST = 10
K_ADC_DEV_WINDOWS = 11   # the window decode ahead of every slice of an *_adc_dev call (int16 device shards)
K_REFINE_OPTIMAL = 12     # fingerprint_refine_optimal_kernel alone (OPT_REFINE_OPTIMAL_CPTS)
K_MEDOID = 13             # per-label medoids: pre-pass, tile kernels (or the general route's chunk sums), reduce kernel
K_SELF_NEAREST = 14       # leave-one-out nearest neighbours: pre-pass, tile kernels and finish kernel (or the general route's dispatches + rows kernel)
K_SVM_FIT = 15            # the batched SMO solve (wdx_svm_solve_device, wdx_svm_solve): its one launch
K_MLP_FIT = 16            # the MLP trainer (wdx_mlp_fit_device, wdx_mlp_fit): one event pair per epoch, 2 n_layers launches per step
K_BOOST_FIT = 17          # the Fpt_Boost trainer (wdx_boost_fit_device, wdx_boost_fit): one event pair per call, 1 + n_trees (3 depth + 4) launches
K_SVM_KERNEL = 18         # the kernel matrix of wdx_svm_kernel_device: its one launch
K_SVM_CV_COUPLE = 20      # the out-of-fold probabilities of wdx_svm_cv_couple_device: its one launch
K_THRESHOLDS = 19         # accuracy thresholds (wdx_accuracy_thresholds_device, wdx_accuracy_thresholds): the histogram pass and the selection
K_DETECT = 21             # adapter boundary detection (wdx_detect_rows, wdx_detect_rows_adc and the host-buffer forms): its one launch

# wdx_ctx_set_option selectors (diagnostics; the product path leaves all of them 0)
OPT_EXACT_PATH, OPT_NO_WAVEFRONT_DTW, OPT_NO_SHORT_DTW, OPT_SVM_SCALAR, OPT_DEBUG_OCCUPANCY, OPT_FAST_PEAK_CAP = 1, 2, 3, 4, 5, 6
OPT_FAST_EXACT_SCORES = 7
OPT_FAST_MAIN_CAP = 8
OPT_FAST_CHAIN_MIN_READS = 9
OPT_EXACT_NO_PEAK_LIST = 10
OPT_MAX_LAUNCH_SLICE = 11
OPT_NO_PEAK_FILTER = 12
OPT_NO_WAVE_CLIP_LONG = 13
OPT_NO_CLIP_REUSE = 14
OPT_NO_SPLIT_TAIL = 15
OPT_DTW_UNFUSED = 16
OPT_MLP_CHUNK_ROWS = 17
OPT_BOOST_CHUNK_ROWS = 18
OPT_BOOST_KERNEL = 19   # 0 by batch size | 1 lane-per-read | 2 tree-parallel
OPT_LONG_WINDOWS = 20   # product option: 1 = adapter windows up to WDX_MAX_LONG_ADAPTER_SAMPLES (0 / 1, else ValueError)
OPT_LONG_REFINE_WINDOWS = 21   # ... the same for the consensus-refinement branch, which looks at this option only
OPT_ADC_DEV_SLICE_READS = 22   # reads per slice of the *_adc_dev entries (0 = as many as the staging budget holds)
OPT_REFINE_OPTIMAL_CPTS = 23   # product option of the refinement branch: barcode tails cut at their optimal change-points
                               # (segmentation.refinement_optimal_cpts; ``RefineParams.optimal_cpts`` sets it)
OPT_WIDE_DTW = 24   # product option of the DTW seam: 1 = effective windows 33 .. L at L <= DTW_WIDE_MAX_L (``window=None`` included) on the
                    # wide-window kernel instead of the scratch rows; the fused device entries then accept such references (0 / 1)
DTW_WIDE_MAX_L = 256   # WDX_DTW_WIDE_MAX_L
OPT_MEDOID_GENERAL = 25   # diagnostic: per-label medoids through the DTW dispatch + chunk sums instead of the tile kernels (same bits)
MEDOID_MAX_GROUP = 32768   # WDX_MEDOID_MAX_GROUP: rows of one label in wdx_medoids_device / wdx_dtw_medoids (beyond: NotImplementedError)
SVM_MAX_CLASSES = 16   # classes of a resident DTW_SVM (wdx_svm_set_model refuses more)
OPT_SELF_MATRIX_GENERAL = 26   # diagnostic: the self-distance matrix through the DTW dispatch + a mask kernel instead of the tile kernels (same bits)
SELF_MATRIX_MAX_ROWS = 65536   # WDX_SELF_MATRIX_MAX_ROWS: rows of wdx_self_matrix_device / wdx_dtw_self_matrix (beyond: NotImplementedError)
OPT_DBA_GENERAL = 27   # diagnostic: barycenter steps on two rolling rows per lane in global memory instead of the register band (same bits)
OPT_SELF_NEAREST_GENERAL = 28   # diagnostic: leave-one-out neighbours through the DTW dispatch + a rows kernel instead of the tile kernels (same bits)
SVM_FIT_MAX_ROWS = 16384   # WDX_SVM_FIT_MAX_ROWS: rows of one problem of wdx_svm_solve_device / wdx_svm_solve (beyond: NotImplementedError in Python)
# (threads, rows per thread) of the solver's instantiations (wdx_svm_fit_plan.h: kSvmFitKernels); a call runs the smallest that holds its largest problem
SVM_FIT_KERNELS = ((64, 4), (256, 8), (1024, 16))
SVM_KERNEL_MAX_ROWS = 1 << 20   # WDX_SVM_KERNEL_MAX_ROWS
SVM_KERNEL_MAX_POWER = 16       # WDX_SVM_KERNEL_MAX_POWER: pwr_dist of wdx_svm_kernel_device (beyond: NotImplementedError)
SVM_CV_MAX_FOLDS = 16   # WDX_SVM_CV_MAX_FOLDS
THRESHOLDS_MAX_CLASSES, THRESHOLDS_MAX_RESOLUTION, THRESHOLDS_MAX_TARGETS = 16, 4096, 16   # WDX_THRESHOLDS_MAX_*
DBA_MAX_L = 1024   # WDX_DBA_MAX_L: longest series of wdx_dba_step_device / wdx_dtw_dba_step (beyond: NotImplementedError)
COMM_ID_BYTES = 128
ABI_VERSION = 4

NORM_CODES = {"none": 0, "mean": 1, "median": 2}

# every symbol include/wdx.h declares (tests check the .so exports each of them)
EXPORTS = [
    "wdx_abi_version", "wdx_last_error", "wdx_device_count", "wdx_ctx_create", "wdx_ctx_destroy",
    "wdx_ctx_synchronize", "wdx_ctx_stream", "wdx_ctx_set_option", "wdx_comm_available", "wdx_comm_info", "wdx_comm_unique_id", "wdx_comm_init",
    "wdx_comm_destroy", "wdx_reduce_counts", "wdx_reduce_counts_host", "wdx_dtw_matrix", "wdx_set_refs", "wdx_refs_generation", "wdx_dtw_matrix_dev",
    "wdx_fingerprint_batch", "wdx_fingerprint_refine_batch", "wdx_fingerprint_refine_dev", "wdx_fingerprint_dev", "wdx_demux_batch", "wdx_demux_submit", "wdx_demux_wait", "wdx_demux_submit_ex", "wdx_demux_wait_ex",
    "wdx_host_alloc", "wdx_host_alloc_on", "wdx_host_free", "wdx_host_register", "wdx_host_unregister", "wdx_live_tick", "wdx_svm_set_model",
    "wdx_svm_predict_dev", "wdx_dtw_svm_predict", "wdx_demux_svm_dev", "wdx_demux_workspace_bytes", "wdx_demux_dev",
    "wdx_kernel_timing", "wdx_kernel_time", "wdx_kernel_time_reset", "wdx_dtw_last_launch", "wdx_synth_lengths_dev",
    "wdx_synth_fill_dev", "wdx_fingerprint_profile_dev", "wdx_calib_read_dev", "wdx_selftest_score_dev", "wdx_selftest_clip_dev", "wdx_selftest_optimal_cpts_dev",
    "wdx_feeder_ring_bytes", "wdx_feeder_ring_init", "wdx_feeder_serve", "wdx_feeder_run", "wdx_feeder_demux", "wdx_feeder_predict", "wdx_feeder_stop",
    "wdx_feeder_served", "wdx_feeder_stats", "wdx_feeder_alive", "wdx_feeder_selftest",
    "wdx_mlp_set_model", "wdx_mlp_predict_dev", "wdx_dtw_mlp_predict", "wdx_demux_mlp_dev",
    "wdx_demux_submit_adc", "wdx_fingerprint_batch_adc", "wdx_demux_batch_adc", "wdx_calibrate_adc_dev", "wdx_feeder_run_adc",
    "wdx_demux_submit_refine", "wdx_demux_wait_refine", "wdx_demux_refine_workspace_bytes", "wdx_demux_refine_dev",
    "wdx_feeder_ring_bytes_refine", "wdx_feeder_ring_init_refine", "wdx_feeder_run_refine",
    "wdx_boost_set_model", "wdx_boost_predict_dev", "wdx_boost_predict", "wdx_demux_boost_dev", "wdx_feeder_predict_boost",
    "wdx_live_tick_ex",
    "wdx_fingerprint_adc_dev", "wdx_fingerprint_refine_adc_dev", "wdx_demux_adc_workspace_bytes",
    "wdx_demux_refine_adc_workspace_bytes", "wdx_adc_dev_staging_bytes", "wdx_demux_adc_dev", "wdx_demux_refine_adc_dev",
    "wdx_demux_svm_adc_dev", "wdx_demux_mlp_adc_dev", "wdx_demux_boost_adc_dev",
    "wdx_nearest_dev", "wdx_demux_nearest_dev", "wdx_dtw_nearest",
    "wdx_medoids_device", "wdx_dtw_medoids",
    "wdx_self_matrix_device", "wdx_dtw_self_matrix",
    "wdx_dba_step_device", "wdx_dtw_dba_step",
    "wdx_self_nearest_device", "wdx_dtw_self_nearest",
    "wdx_svm_solve_device", "wdx_svm_solve",
    "wdx_mlp_fit_device", "wdx_mlp_fit",
    "wdx_boost_fit_device", "wdx_boost_fit",
    "wdx_svm_kernel_device", "wdx_svm_cv_couple_device",
    "wdx_accuracy_thresholds_device", "wdx_accuracy_thresholds",
    "wdx_detect_rows", "wdx_detect_rows_adc", "wdx_detect_batch", "wdx_detect_batch_adc",
]


class SegParamsC(C.Structure):
    """wdx_seg_params (include/wdx.h)"""

    _fields_ = [
        ("padding", C.c_int32),
        ("sig_norm", C.c_int32),
        ("outlier_thresh", C.c_float),
        ("min_obs_per_base", C.c_int32),
        ("running_stat_width", C.c_int32),
        ("num_events", C.c_int32),
        ("accept_less_cpts", C.c_int32),
        ("seg_norm", C.c_int32),
        ("barcode_num_events", C.c_int32),
        ("clip_bounds_f64", C.c_int32),
        ("outlier_thresh_f64", C.c_double),
    ]


class RefineParamsC(C.Structure):
    """wdx_refine_params (include/wdx.h)"""

    _fields_ = [
        ("query", C.c_void_p),
        ("n_query", C.c_int32),
        ("subseq_norm", C.c_int32),
        ("penalty", C.c_double),
        ("psi", C.c_int32 * 4),
        ("ub_start", C.c_int32),
        ("lb_end", C.c_int32),
        ("ub_end", C.c_int32),
        ("barcode_segm_events", C.c_int32),
        ("barcode_keep_events", C.c_int32),
    ]


# wdx_dtw_launch_info.family / .layout (include/wdx.h)
DTW_NONE, DTW_WAVEFRONT, DTW_SHORT, DTW_BAND, DTW_SCRATCH, DTW_SHORT_SVM, DTW_WIDE = range(7)
DTW_FAMILY_NAMES = ("none", "wavefront", "short", "band", "scratch", "short+svm", "wide")
DTW_LAYOUT_ROW_MAJOR, DTW_LAYOUT_READ_MINOR, DTW_LAYOUT_REFS_AS_LANES = range(3)
DTW_LAYOUT_NAMES = ("row-major", "read-minor", "refs-as-lanes")


class DtwLaunchInfoC(C.Structure):
    """wdx_dtw_launch_info (include/wdx.h)"""

    _fields_ = [
        ("family", C.c_int32),
        ("band_w", C.c_int32),
        ("exact_w", C.c_int32),
        ("layout", C.c_int32),
        ("fused_argmin", C.c_int32),
        ("launches", C.c_int32),
        ("refs_per_block", C.c_int32),
        ("window", C.c_int32),
        ("grid_x", C.c_int64),
        ("grid_y", C.c_int64),
    ]


class SvmModelC(C.Structure):
    """wdx_svm_model (include/wdx.h)"""

    _fields_ = [
        ("n_classes", C.c_int32),
        ("n_sv", C.c_int32),
        ("n_train", C.c_int32),
        ("pwr_dist", C.c_int32),
        ("gamma", C.c_double),
        ("n_support", C.c_void_p),
        ("support", C.c_void_p),
        ("dual_coef", C.c_void_p),
        ("rho", C.c_void_p),
        ("probA", C.c_void_p),
        ("probB", C.c_void_p),
        ("label_map", C.c_void_p),
        ("thresholds", C.c_void_p),
    ]


# wdx_mlp_model (include/wdx.h)
MLP_MAX_LAYERS, MLP_MAX_WIDTH, MLP_MAX_SCALERS = 5, 512, 4
MLP_ACT = {"identity": 0, "logistic": 1, "tanh": 2, "relu": 3}   # WDX_MLP_ACT_*


MLP_FIT_MAX_BATCH = 1024   # WDX_MLP_FIT_MAX_BATCH: rows of one minibatch of wdx_mlp_fit_device / wdx_mlp_fit (beyond: NotImplementedError)
MLP_FIT_MAX_CLASSES = 16
MLP_FIT_STATES = ("max_epochs", "tol", "nonfinite_input", "nonfinite_loss")   # WDX_MLP_FIT_*


class MlpFitParamsC(C.Structure):
    """wdx_mlp_fit_params (include/wdx.h)"""

    _fields_ = [
        ("n_layers", C.c_int32), ("hidden_activation", C.c_int32), ("n_classes", C.c_int32), ("batch_size", C.c_int32),
        ("max_epochs", C.c_int32), ("n_iter_no_change", C.c_int32), ("sizes", C.c_int32 * (MLP_MAX_LAYERS + 1)),
        ("lr", C.c_double), ("alpha", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("epsilon", C.c_double),
        ("tol", C.c_double),
    ]


class MlpModelC(C.Structure):
    """wdx_mlp_model (include/wdx.h)"""

    _fields_ = [
        ("n_layers", C.c_int32), ("dtype_bytes", C.c_int32), ("hidden_activation", C.c_int32), ("n_classes", C.c_int32),
        ("n_scalers", C.c_int32), ("pad_", C.c_int32), ("sizes", C.c_int32 * (MLP_MAX_LAYERS + 1)),
        ("coefs", C.c_void_p * MLP_MAX_LAYERS), ("intercepts", C.c_void_p * MLP_MAX_LAYERS),
        ("scaler_mean", C.c_void_p * MLP_MAX_SCALERS), ("scaler_scale", C.c_void_p * MLP_MAX_SCALERS),
        ("label_map", C.c_void_p), ("thresholds", C.c_void_p),
    ]


# wdx_boost_model (include/wdx.h)
BOOST_MAX_FEATURES, BOOST_MAX_DEPTH, BOOST_MAX_DIM = 254, 16, 16
# the tree-parallel kernel (wdx_boost.hip): reads per workgroup, trees per chunk, and the largest batch that takes it by
# default (WDX_BOOST_SMALL_READS / _TREE_CHUNK / _SMALL_MAX_READS; 0 would mean through OPT_BOOST_KERNEL only)
BOOST_SMALL_READS, BOOST_TREE_CHUNK, BOOST_SMALL_MAX_READS = 16, 1024, 65536


# the Fpt_Boost trainer (WDX_BOOST_FIT_*: deepest tree, most borders per feature, most rows, most trees per call, the workspace
# cap in bytes, the bits of a quantised gradient, the rows of one histogram workgroup; beyond the limits: NotImplementedError)
BOOST_FIT_MAX_DEPTH, BOOST_FIT_MAX_BORDERS, BOOST_FIT_MAX_ROWS, BOOST_FIT_MAX_TREES = 8, 255, 1 << 24, 1 << 20
BOOST_FIT_MAX_WORKSPACE, BOOST_FIT_GRAD_BITS, BOOST_FIT_ROWS = 4 << 30, 20, 2047
BOOST_FIT_MAX_CLASSES = 16


class BoostFitParamsC(C.Structure):
    """wdx_boost_fit_params (include/wdx.h)"""

    _fields_ = [
        ("n_features", C.c_int32), ("n_classes", C.c_int32), ("n_trees", C.c_int32), ("depth", C.c_int32), ("border_count", C.c_int32),
        ("reserved", C.c_int32), ("learning_rate", C.c_double), ("l2_leaf_reg", C.c_double),
    ]


class BoostModelC(C.Structure):
    """wdx_boost_model (include/wdx.h)"""

    _fields_ = [
        ("n_trees", C.c_int32), ("n_features", C.c_int32), ("dim", C.c_int32), ("n_classes", C.c_int32),
        ("depth", C.c_void_p), ("split_feature", C.c_void_p), ("split_border", C.c_void_p), ("split_nan_true", C.c_void_p),
        ("leaf_values", C.c_void_p), ("scale", C.c_double), ("bias", C.c_void_p), ("label_map", C.c_void_p),
        ("thresholds", C.c_void_p),
    ]


WANT_FPT, WANT_DIST, WANT_DWELL, WANT_STATS, WANT_SVM = 0x01, 0x02, 0x04, 0x08, 0x10   # WDX_WANT_*
WANT_REFINE_IDX = 0x20   # refine minibatches only (wdx_demux_submit_refine, a refine feeder ring)
WANT_BOOST = 0x40        # prob / pred / conf of the resident boost model on the minibatch's fingerprints (never with WANT_SVM)


class MinibatchInC(C.Structure):
    """wdx_minibatch_in (include/wdx.h)"""

    _fields_ = [
        ("sig", C.c_void_p), ("n_reads", C.c_int64), ("stride", C.c_int64), ("row_off", C.c_void_p), ("row_len", C.c_void_p),
        ("a_start", C.c_void_p), ("a_end", C.c_void_p), ("ok", C.c_void_p),
    ]


class MinibatchAdcInC(C.Structure):
    """wdx_minibatch_adc_in (include/wdx.h)"""

    _fields_ = [
        ("adc", C.c_void_p), ("n_reads", C.c_int64), ("stride", C.c_int64), ("row_len", C.c_void_p), ("offset", C.c_void_p),
        ("scale", C.c_void_p), ("row_off", C.c_void_p), ("row_win", C.c_void_p), ("a_start", C.c_void_p), ("a_end", C.c_void_p),
        ("ok", C.c_void_p),
    ]


class AdcDevInC(C.Structure):
    """wdx_adc_dev_in (include/wdx.h): an int16 shard in device memory"""

    _fields_ = [
        ("adc", C.c_void_p), ("row_off", C.c_void_p), ("stride", C.c_int64), ("row_len", C.c_void_p), ("offset", C.c_void_p),
        ("scale", C.c_void_p), ("row_win", C.c_void_p),
    ]


DETECT_MAX_TRACE = 16384   # WDX_DETECT_MAX_TRACE
DETECT_OK, DETECT_SHORT, DETECT_NO_START, DETECT_NO_ROOM, DETECT_NO_POLYA = 0, 1, 2, 3, 4   # WDX_DETECT_*


class DetectParamsC(C.Structure):
    """wdx_detect_params (include/wdx.h)"""

    _fields_ = [
        ("max_obs_trace", C.c_int32), ("quant_per_pa", C.c_float), ("find_start", C.c_int32), ("open_pore_pa", C.c_float),
        ("start_win", C.c_int32), ("max_start", C.c_int32), ("min_obs_adapter", C.c_int32), ("max_obs_adapter", C.c_int32),
        ("polya_win", C.c_int32), ("step_win", C.c_int32), ("refine", C.c_int32), ("min_shift_pa", C.c_float),
        ("max_polya_var", C.c_float),
    ]


class MinibatchOutC(C.Structure):
    """wdx_minibatch_out (include/wdx.h)"""

    _fields_ = [
        ("status", C.c_void_p), ("call", C.c_void_p), ("dist", C.c_void_p), ("fpt", C.c_void_p), ("dwell", C.c_void_p),
        ("stats", C.c_void_p), ("prob", C.c_void_p), ("pred", C.c_void_p), ("conf", C.c_void_p),
    ]


LIVE_TAIL_NONE, LIVE_TAIL_SVM, LIVE_TAIL_MLP, LIVE_TAIL_BOOST = 0, 1, 2, 3   # WDX_LIVE_TAIL_*


class LiveInC(C.Structure):
    """wdx_live_in (include/wdx.h)"""

    _fields_ = [
        ("rows", C.c_void_p), ("adc_rows", C.c_void_p), ("offset", C.c_void_p), ("scale", C.c_void_p), ("row_len", C.c_void_p),
        ("n_reads", C.c_int64), ("a_start", C.c_void_p), ("a_end", C.c_void_p), ("ok", C.c_void_p), ("tail", C.c_int32),
        ("pad_", C.c_int32),
    ]


class FeederGeometryC(C.Structure):
    """wdx_feeder_geometry (include/wdx.h)"""

    _fields_ = [
        ("n_slots", C.c_int32), ("n_events", C.c_int32), ("n_classes", C.c_int32), ("sample_format", C.c_int32),
        ("max_reads", C.c_int64), ("max_stride", C.c_int64), ("n_refs", C.c_int64),
    ]


FEEDER_SAMPLES_FLOAT32, FEEDER_SAMPLES_INT16 = 0, 1   # WDX_FEEDER_SAMPLES_*


class FeederJobC(C.Structure):
    """wdx_feeder_job (include/wdx.h)"""

    _fields_ = [
        ("sig", C.c_void_p), ("n_reads", C.c_int64), ("stride", C.c_int64), ("a_start", C.c_void_p), ("a_end", C.c_void_p),
        ("ok", C.c_void_p), ("want", C.c_uint32), ("pad_", C.c_uint32),
        ("status", C.c_void_p), ("call", C.c_void_p), ("dist", C.c_void_p), ("fpt", C.c_void_p), ("dwell", C.c_void_p),
        ("stats", C.c_void_p), ("prob", C.c_void_p), ("pred", C.c_void_p), ("conf", C.c_void_p),
    ]


class FeederJobAdcC(C.Structure):
    """wdx_feeder_job_adc (include/wdx.h)"""

    _fields_ = [
        ("adc", C.c_void_p), ("n_reads", C.c_int64), ("stride", C.c_int64), ("row_len", C.c_void_p), ("offset", C.c_void_p),
        ("scale", C.c_void_p), ("a_start", C.c_void_p), ("a_end", C.c_void_p), ("ok", C.c_void_p), ("want", C.c_uint32),
        ("pad_", C.c_uint32),
        ("status", C.c_void_p), ("call", C.c_void_p), ("dist", C.c_void_p), ("fpt", C.c_void_p), ("dwell", C.c_void_p),
        ("stats", C.c_void_p), ("prob", C.c_void_p), ("pred", C.c_void_p), ("conf", C.c_void_p),
    ]


def addr(a):
    """Address of a NumPy array as an int for a c_void_p FIELD of a ctypes structure (None -> NULL)."""
    return None if a is None else a.ctypes.data


class WdxError(RuntimeError):
    pass


class WdxNoDevice(WdxError):
    """WDX_ERR_NO_DEVICE: no usable HIP device / runtime / RCCL in this process."""


_lib = None
_lock = threading.Lock()


def _preload_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (soname libamdhip64.so.7) but request it as "libamdhip64.so", so if libwdx_hip.so pulled in
    /opt/rocm's copy first a later `import torch` would load a second runtime and lose the GPU.
    Loading torch's copy first (when torch is installed) makes both resolve to the same object;
    without torch the RUNPATH of libwdx_hip.so finds /opt/rocm.  $WDX_HIP_RUNTIME overrides."""
    cand = os.environ.get("WDX_HIP_RUNTIME")
    if not cand:
        try:
            import importlib.util

            spec = importlib.util.find_spec("torch")
            if spec and spec.origin:
                c = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
                if os.path.exists(c):
                    cand = c
        except Exception:
            cand = None
    if cand:
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """dlopen the engine; raises if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise WdxError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C warpdemux_amd/csrc` (there is no CPU fallback)"
            )
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, u64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
        P = C.POINTER
        L.wdx_abi_version.restype = C.c_int
        L.wdx_abi_version.argtypes = []
        # (checked before any other symbol is bound: an older library then fails with this message, not with an
        # AttributeError on the first export it lacks)
        have = L.wdx_abi_version()
        if have != ABI_VERSION:
            raise WdxError(f"{LIB_PATH}: ABI version {have}, this package binds version {ABI_VERSION} -- rebuild it "
                           "(make -C warpdemux_amd/csrc)")
        L.wdx_last_error.restype = C.c_char_p
        L.wdx_last_error.argtypes = []
        L.wdx_device_count.restype = C.c_int
        L.wdx_device_count.argtypes = []
        L.wdx_ctx_create.restype = C.c_int
        L.wdx_ctx_create.argtypes = [C.c_int, P(vp)]
        L.wdx_ctx_destroy.restype = None
        L.wdx_ctx_destroy.argtypes = [vp]
        L.wdx_ctx_synchronize.restype = C.c_int
        L.wdx_ctx_synchronize.argtypes = [vp, vp]
        L.wdx_ctx_stream.restype = C.c_int
        L.wdx_ctx_stream.argtypes = [vp, P(vp)]
        L.wdx_ctx_set_option.restype = C.c_int
        L.wdx_ctx_set_option.argtypes = [vp, i32, i64]
        L.wdx_comm_available.restype = C.c_int
        L.wdx_comm_available.argtypes = []
        L.wdx_comm_info.restype = C.c_int
        L.wdx_comm_info.argtypes = [vp, P(i32), P(i32), P(i32)]
        L.wdx_comm_unique_id.restype = C.c_int
        L.wdx_comm_unique_id.argtypes = [vp]
        L.wdx_comm_init.restype = C.c_int
        L.wdx_comm_init.argtypes = [vp, vp, i32, i32]
        L.wdx_comm_destroy.restype = C.c_int
        L.wdx_comm_destroy.argtypes = [vp]
        L.wdx_reduce_counts.restype = C.c_int
        L.wdx_reduce_counts.argtypes = [vp, vp, i32, vp]
        L.wdx_reduce_counts_host.restype = C.c_int
        L.wdx_reduce_counts_host.argtypes = [vp, vp, i32]
        L.wdx_dtw_matrix.restype = C.c_int
        L.wdx_dtw_matrix.argtypes = [vp, vp, i64, vp, i64, i64, i32, f64, vp, vp]
        L.wdx_refs_generation.restype = C.c_int
        L.wdx_refs_generation.argtypes = [vp, P(C.c_int64)]
        L.wdx_set_refs.restype = C.c_int
        L.wdx_set_refs.argtypes = [vp, vp, i64, i64, i32, f64]
        L.wdx_dtw_matrix_dev.restype = C.c_int
        L.wdx_dtw_matrix_dev.argtypes = [vp, vp, i64, vp, vp, vp]
        L.wdx_fingerprint_batch.restype = C.c_int
        L.wdx_fingerprint_batch.argtypes = [vp, vp, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp]
        L.wdx_fingerprint_refine_batch.restype = C.c_int
        L.wdx_fingerprint_refine_batch.argtypes = [vp, vp, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp, vp, vp]
        L.wdx_fingerprint_refine_dev.restype = C.c_int
        L.wdx_fingerprint_refine_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp, vp, vp, vp]
        L.wdx_svm_set_model.restype = C.c_int
        L.wdx_svm_set_model.argtypes = [vp, P(SvmModelC)]
        L.wdx_svm_predict_dev.restype = C.c_int
        L.wdx_svm_predict_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp]
        L.wdx_dtw_svm_predict.restype = C.c_int
        L.wdx_dtw_svm_predict.argtypes = [vp, vp, i64, vp, vp, vp]
        L.wdx_demux_batch.restype = C.c_int
        L.wdx_demux_batch.argtypes = [vp, vp, i64, i64, vp, vp, vp, P(SegParamsC), i64, vp, vp, vp, vp]
        L.wdx_demux_submit.restype = C.c_int
        L.wdx_demux_submit.argtypes = [vp, i32, vp, i64, i64, vp, vp, vp, P(SegParamsC), i64, i32, i32]
        L.wdx_demux_wait.restype = C.c_int
        L.wdx_demux_wait.argtypes = [vp, i32, vp, vp, vp, vp]
        L.wdx_host_alloc.restype = C.c_int
        L.wdx_host_alloc.argtypes = [C.c_size_t, P(vp)]
        L.wdx_host_free.restype = C.c_int
        L.wdx_host_free.argtypes = [vp]
        L.wdx_host_alloc_on.restype = C.c_int
        L.wdx_host_alloc_on.argtypes = [C.c_int, C.c_size_t, P(vp)]
        L.wdx_host_register.restype = C.c_int
        L.wdx_host_register.argtypes = [vp, C.c_size_t]
        L.wdx_host_unregister.restype = C.c_int
        L.wdx_host_unregister.argtypes = [vp]
        L.wdx_live_tick.restype = C.c_int
        L.wdx_live_tick.argtypes = [vp, vp, vp, i64, vp, vp, vp, P(SegParamsC), i64, i32, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_fingerprint_dev.restype = C.c_int
        L.wdx_fingerprint_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp]
        L.wdx_demux_workspace_bytes.restype = i64
        L.wdx_demux_workspace_bytes.argtypes = [i64, i32]
        L.wdx_demux_dev.restype = C.c_int
        L.wdx_demux_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_demux_svm_dev.restype = C.c_int
        L.wdx_demux_svm_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, vp, vp, i64, vp]
        L.wdx_kernel_timing.restype = C.c_int
        L.wdx_kernel_timing.argtypes = [vp, C.c_int]
        L.wdx_dtw_last_launch.restype = C.c_int
        L.wdx_dtw_last_launch.argtypes = [vp, P(DtwLaunchInfoC)]
        L.wdx_kernel_time.restype = C.c_int
        L.wdx_kernel_time.argtypes = [vp, C.c_int, P(f64), P(i64)]
        L.wdx_kernel_time_reset.restype = C.c_int
        L.wdx_kernel_time_reset.argtypes = [vp]
        L.wdx_fingerprint_profile_dev.restype = C.c_int
        L.wdx_fingerprint_profile_dev.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, P(SegParamsC), vp, vp, i64, i32, i32, vp]
        L.wdx_selftest_optimal_cpts_dev.restype = C.c_int
        L.wdx_selftest_optimal_cpts_dev.argtypes = [vp, vp, vp, i64, i32, i32, i64, i32, vp, vp, vp]
        L.wdx_selftest_score_dev.restype = C.c_int
        L.wdx_selftest_score_dev.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        L.wdx_selftest_clip_dev.restype = C.c_int
        L.wdx_selftest_clip_dev.argtypes = [vp, vp, vp, i64, i64, vp, vp, P(SegParamsC), i32, vp, vp]
        L.wdx_calib_read_dev.restype = C.c_int
        L.wdx_calib_read_dev.argtypes = [vp, vp, i64, vp, vp]
        L.wdx_synth_lengths_dev.restype = C.c_int
        L.wdx_synth_lengths_dev.argtypes = [vp, u64, i64, i64, i32, vp, vp, vp]
        L.wdx_synth_fill_dev.restype = C.c_int
        L.wdx_synth_fill_dev.argtypes = [vp, u64, i64, i64, i32, i32, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_demux_submit_ex.restype = C.c_int
        L.wdx_demux_submit_ex.argtypes = [vp, i32, P(MinibatchInC), P(SegParamsC), i64, C.c_uint32]
        L.wdx_demux_wait_ex.restype = C.c_int
        L.wdx_demux_wait_ex.argtypes = [vp, i32, P(MinibatchOutC)]
        L.wdx_feeder_ring_bytes.restype = C.c_size_t
        L.wdx_feeder_ring_bytes.argtypes = [P(FeederGeometryC)]
        L.wdx_feeder_ring_init.restype = C.c_int
        L.wdx_feeder_ring_init.argtypes = [vp, C.c_size_t, P(FeederGeometryC), P(SegParamsC)]
        L.wdx_feeder_serve.restype = C.c_int
        L.wdx_feeder_serve.argtypes = [vp, vp]
        L.wdx_feeder_run.restype = C.c_int
        L.wdx_feeder_run.argtypes = [vp, P(FeederJobC)]
        L.wdx_feeder_demux.restype = C.c_int
        L.wdx_feeder_demux.argtypes = [vp, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp]
        L.wdx_feeder_predict.restype = C.c_int
        L.wdx_feeder_predict.argtypes = [vp, vp, i64, vp, vp, vp]
        L.wdx_feeder_stop.restype = C.c_int
        L.wdx_feeder_stop.argtypes = [vp]
        L.wdx_feeder_served.restype = C.c_int
        L.wdx_feeder_served.argtypes = [vp, P(i64)]
        L.wdx_feeder_stats.restype = C.c_int
        L.wdx_feeder_stats.argtypes = [vp, P(i64), P(i64), P(i32)]
        L.wdx_feeder_alive.restype = C.c_int
        L.wdx_feeder_alive.argtypes = [vp]
        L.wdx_feeder_selftest.restype = C.c_int
        L.wdx_feeder_selftest.argtypes = [vp, i32]
        L.wdx_mlp_set_model.restype = C.c_int
        L.wdx_mlp_set_model.argtypes = [vp, P(MlpModelC)]
        L.wdx_mlp_predict_dev.restype = C.c_int
        L.wdx_mlp_predict_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp]
        L.wdx_dtw_mlp_predict.restype = C.c_int
        L.wdx_dtw_mlp_predict.argtypes = [vp, vp, i64, vp, vp, vp, P(i64)]
        L.wdx_demux_mlp_dev.restype = C.c_int
        L.wdx_demux_mlp_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, vp, vp, vp,
                                        i64, vp]
        L.wdx_demux_submit_adc.restype = C.c_int
        L.wdx_demux_submit_adc.argtypes = [vp, i32, P(MinibatchAdcInC), P(SegParamsC), i64, C.c_uint32]
        L.wdx_fingerprint_batch_adc.restype = C.c_int
        L.wdx_fingerprint_batch_adc.argtypes = [vp, P(MinibatchAdcInC), P(SegParamsC), vp, vp, vp, vp]
        L.wdx_demux_batch_adc.restype = C.c_int
        L.wdx_demux_batch_adc.argtypes = [vp, P(MinibatchAdcInC), P(SegParamsC), i64, vp, vp, vp, vp]
        L.wdx_calibrate_adc_dev.restype = C.c_int
        L.wdx_calibrate_adc_dev.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp]
        L.wdx_feeder_run_adc.restype = C.c_int
        L.wdx_feeder_run_adc.argtypes = [vp, P(FeederJobAdcC)]
        L.wdx_demux_submit_refine.restype = C.c_int
        L.wdx_demux_submit_refine.argtypes = [vp, i32, P(MinibatchInC), P(MinibatchAdcInC), P(SegParamsC), P(RefineParamsC), i64,
                                              C.c_uint32]
        L.wdx_demux_wait_refine.restype = C.c_int
        L.wdx_demux_wait_refine.argtypes = [vp, i32, P(MinibatchOutC), vp]
        L.wdx_demux_refine_workspace_bytes.restype = i64
        L.wdx_demux_refine_workspace_bytes.argtypes = [i64, i32]
        L.wdx_demux_refine_dev.restype = C.c_int
        L.wdx_demux_refine_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp]
        L.wdx_feeder_ring_bytes_refine.restype = C.c_size_t
        L.wdx_feeder_ring_bytes_refine.argtypes = [P(FeederGeometryC)]
        L.wdx_feeder_ring_init_refine.restype = C.c_int
        L.wdx_feeder_ring_init_refine.argtypes = [vp, C.c_size_t, P(FeederGeometryC), P(SegParamsC), P(RefineParamsC)]
        L.wdx_feeder_run_refine.restype = C.c_int
        L.wdx_feeder_run_refine.argtypes = [vp, P(FeederJobC), P(FeederJobAdcC), vp]
        L.wdx_boost_set_model.restype = C.c_int
        L.wdx_boost_set_model.argtypes = [vp, P(BoostModelC)]
        L.wdx_boost_predict_dev.restype = C.c_int
        L.wdx_boost_predict_dev.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp]
        L.wdx_boost_predict.restype = C.c_int
        L.wdx_boost_predict.argtypes = [vp, vp, i64, vp, vp, vp, vp]
        L.wdx_demux_boost_dev.restype = C.c_int
        L.wdx_demux_boost_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp,
                                          vp, vp, vp, vp, vp, vp]
        L.wdx_feeder_predict_boost.restype = C.c_int
        L.wdx_feeder_predict_boost.argtypes = [vp, vp, i64, vp, vp, vp]
        L.wdx_live_tick_ex.restype = C.c_int
        L.wdx_live_tick_ex.argtypes = [vp, P(LiveInC), P(SegParamsC), P(RefineParamsC), i64, C.c_uint32, P(MinibatchOutC), vp,
                                       P(i64)]
        A = P(AdcDevInC)
        L.wdx_fingerprint_adc_dev.restype = C.c_int
        L.wdx_fingerprint_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp]
        L.wdx_fingerprint_refine_adc_dev.restype = C.c_int
        L.wdx_fingerprint_refine_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp,
                                                     vp, vp, vp]
        L.wdx_demux_adc_workspace_bytes.restype = i64
        L.wdx_demux_adc_workspace_bytes.argtypes = [vp, i64, i64, i32]
        L.wdx_demux_refine_adc_workspace_bytes.restype = i64
        L.wdx_demux_refine_adc_workspace_bytes.argtypes = [vp, i64, i64, i32]
        L.wdx_adc_dev_staging_bytes.restype = i64
        L.wdx_adc_dev_staging_bytes.argtypes = [vp, i64, i64, i32]
        L.wdx_demux_adc_dev.restype = C.c_int
        L.wdx_demux_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_demux_refine_adc_dev.restype = C.c_int
        L.wdx_demux_refine_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp, vp, vp,
                                               vp, vp, vp, vp, vp]
        L.wdx_demux_svm_adc_dev.restype = C.c_int
        L.wdx_demux_svm_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, vp, vp, i64, vp]
        L.wdx_demux_mlp_adc_dev.restype = C.c_int
        L.wdx_demux_mlp_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
        L.wdx_demux_boost_adc_dev.restype = C.c_int
        L.wdx_demux_boost_adc_dev.argtypes = [vp, A, i64, i64, vp, vp, vp, P(SegParamsC), P(RefineParamsC), vp, vp, vp, vp, vp,
                                              vp, vp, vp, vp]
        L.wdx_nearest_dev.restype = C.c_int
        L.wdx_nearest_dev.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_demux_nearest_dev.restype = C.c_int
        L.wdx_demux_nearest_dev.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, P(SegParamsC), vp, vp, vp, vp, vp, i64, vp,
                                            vp, vp, vp, vp, vp, vp, vp]
        L.wdx_dtw_nearest.restype = C.c_int
        L.wdx_dtw_nearest.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]
        L.wdx_medoids_device.restype = C.c_int
        L.wdx_medoids_device.argtypes = [vp, vp, i64, i64, vp, i64, vp, C.c_int32, C.c_double, vp, vp, vp, vp, vp, vp]
        L.wdx_dtw_medoids.restype = C.c_int
        L.wdx_dtw_medoids.argtypes = [vp, vp, i64, i64, vp, i64, vp, C.c_int32, C.c_double, vp, vp, vp, vp, vp]
        L.wdx_self_matrix_device.restype = C.c_int
        L.wdx_self_matrix_device.argtypes = [vp, vp, i64, i64, vp, C.c_int32, C.c_double, vp, i64, vp]
        L.wdx_dtw_self_matrix.restype = C.c_int
        L.wdx_dtw_self_matrix.argtypes = [vp, vp, i64, i64, vp, C.c_int32, C.c_double, vp, i64]
        L.wdx_self_nearest_device.restype = C.c_int
        L.wdx_self_nearest_device.argtypes = [vp, vp, i64, i64, vp, vp, C.c_int32, C.c_double, vp, vp, vp]
        L.wdx_dtw_self_nearest.restype = C.c_int
        L.wdx_dtw_self_nearest.argtypes = [vp, vp, i64, i64, vp, vp, C.c_int32, C.c_double, vp, vp]
        L.wdx_dba_step_device.restype = C.c_int
        L.wdx_dba_step_device.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp, C.c_int32, C.c_double, vp, vp, vp, vp, vp, vp]
        L.wdx_dtw_dba_step.restype = C.c_int
        L.wdx_dtw_dba_step.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp, C.c_int32, C.c_double, vp, vp, vp, vp, vp]
        L.wdx_svm_solve_device.restype = C.c_int
        L.wdx_svm_solve_device.argtypes = [vp, vp, i64, i64, vp, i64, vp, i64, vp, i64, C.c_double, i64, vp, vp, vp, vp, vp, vp]
        L.wdx_mlp_fit_device.restype = C.c_int
        L.wdx_mlp_fit_device.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_mlp_fit.restype = C.c_int
        L.wdx_mlp_fit.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_boost_fit_device.restype = C.c_int
        L.wdx_boost_fit_device.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_boost_fit.restype = C.c_int
        L.wdx_boost_fit.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_svm_solve.restype = C.c_int
        L.wdx_svm_solve.argtypes = [vp, vp, i64, i64, vp, i64, vp, i64, vp, i64, C.c_double, i64, vp, vp, vp, vp, vp]
        L.wdx_svm_kernel_device.restype = C.c_int
        L.wdx_svm_kernel_device.argtypes = [vp, vp, i64, i64, C.c_double, C.c_int32, vp, i64, vp]
        L.wdx_svm_cv_couple_device.restype = C.c_int
        L.wdx_svm_cv_couple_device.argtypes = [vp, vp, i64, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
        L.wdx_accuracy_thresholds_device.restype = C.c_int
        L.wdx_accuracy_thresholds_device.argtypes = [vp, vp, i64, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.wdx_accuracy_thresholds.restype = C.c_int
        L.wdx_accuracy_thresholds.argtypes = [vp, vp, i64, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp]
        L.wdx_detect_rows.restype = C.c_int
        L.wdx_detect_rows.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_detect_rows_adc.restype = C.c_int
        L.wdx_detect_rows_adc.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_detect_batch.restype = C.c_int
        L.wdx_detect_batch.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.wdx_detect_batch_adc.restype = C.c_int
        L.wdx_detect_batch_adc.argtypes = [vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
        return L


def check(rc: int):
    """Map a WDX_ERR_* code to the exception the reference's Python would raise."""
    if rc == WDX_SUCCESS:
        return
    msg = load().wdx_last_error().decode("utf-8", "replace")
    if rc == WDX_ERR_INVALID:
        raise ValueError(msg)
    if rc == WDX_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == WDX_ERR_NO_DEVICE:
        raise WdxNoDevice(f"[wdx {rc}] {msg}")
    raise WdxError(f"[wdx {rc}] {msg}")


def ptr(a):
    """void* of a NumPy array (host) -- None passes NULL."""
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """Owns one wdx_ctx (device workspaces + resident reference set).  Created lazily per process
    and per device so that fork()ed workers (file_proc.py:1197) each initialise HIP themselves."""

    def __init__(self, device: int = 0):
        L = load()
        h = C.c_void_p()
        check(L.wdx_ctx_create(int(device), C.byref(h)))
        self._h = h
        self._L = L
        self.device = int(device)
        self.pid = os.getpid()
        self.long_windows = False
        self.long_refine_windows = False
        self.refine_optimal = False
        self.wide_dtw = False

    @property
    def handle(self):
        if self._h is None:
            raise WdxError("context destroyed")
        if self.pid != os.getpid():
            raise WdxError("this context was created in another process (fork): create one per process")
        return self._h

    def set_option(self, option: int, value: int = 1):
        """Diagnostic switch (wdx_ctx_set_option); tests and profiling tools only -- and OPT_LONG_WINDOWS /
        OPT_LONG_REFINE_WINDOWS, which the ``long_windows=`` keyword of the classes and module-level calls sets, and
        OPT_WIDE_DTW, which their ``wide_dtw=`` keyword sets (users of the reference-named functions of
        `parallel_distances` set it here, on `default_context()`)."""
        check(self._L.wdx_ctx_set_option(self.handle, int(option), int(value)))
        if int(option) == OPT_LONG_WINDOWS:
            self.long_windows = bool(value)
        elif int(option) == OPT_LONG_REFINE_WINDOWS:
            self.long_refine_windows = bool(value)
        elif int(option) == OPT_REFINE_OPTIMAL_CPTS:
            self.refine_optimal = bool(value)
        elif int(option) == OPT_WIDE_DTW:
            self.wide_dtw = bool(value)

    def set_long_windows(self):
        """Both product options on: what an object that owns its context does for ``long_windows=True`` -- its plain calls
        look at OPT_LONG_WINDOWS, its refining ones at OPT_LONG_REFINE_WINDOWS."""
        self.set_option(OPT_LONG_WINDOWS, 1)
        self.set_option(OPT_LONG_REFINE_WINDOWS, 1)

    @contextlib.contextmanager
    def long_windows_for_call(self, on: bool):
        """OPT_LONG_WINDOWS = ``on`` for the duration of one call on a shared context, then what it was before -- also when
        the call raises."""
        before = getattr(self, "long_windows", False)
        if bool(on) != before:
            self.set_option(OPT_LONG_WINDOWS, int(bool(on)))
        try:
            yield self
        finally:
            if bool(on) != before:
                self.set_option(OPT_LONG_WINDOWS, int(before))

    @contextlib.contextmanager
    def wide_dtw_for_call(self, on: bool):
        """OPT_WIDE_DTW = ``on`` for the duration of one call on a shared context, then what it was before -- also when the
        call raises."""
        before = self.wide_dtw
        if bool(on) != before:
            self.set_option(OPT_WIDE_DTW, int(bool(on)))
        try:
            yield self
        finally:
            if bool(on) != before:
                self.set_option(OPT_WIDE_DTW, int(before))

    @contextlib.contextmanager
    def long_refine_windows_for_call(self, on: bool):
        """`long_windows_for_call` for a call of the consensus-refinement branch: OPT_LONG_REFINE_WINDOWS = ``on`` for its
        duration, then what it was before -- also when the call raises."""
        before = getattr(self, "long_refine_windows", False)
        if bool(on) != before:
            self.set_option(OPT_LONG_REFINE_WINDOWS, int(bool(on)))
        try:
            yield self
        finally:
            if bool(on) != before:
                self.set_option(OPT_LONG_REFINE_WINDOWS, int(before))

    @contextlib.contextmanager
    def refine_options_for_call(self, refine, long_windows=None):
        """The options of one call of the consensus-refinement branch on this context: OPT_REFINE_OPTIMAL_CPTS from
        ``refine.optimal_cpts`` (None: a plain call, nothing changes) and, unless ``long_windows`` is None,
        OPT_LONG_REFINE_WINDOWS -- for the call's duration, then what they were before, also when the call raises."""
        on = bool(getattr(refine, "optimal_cpts", False))
        before = getattr(self, "refine_optimal", False)
        if on and (long_windows or (long_windows is None and getattr(self, "long_refine_windows", False))):
            raise ValueError("optimal_cpts and long_windows do not go together (WDX_OPT_REFINE_OPTIMAL_CPTS serves adapter "
                             "windows of up to MAX_ADAPTER_SAMPLES samples)")
        if refine is not None and on != before:
            self.set_option(OPT_REFINE_OPTIMAL_CPTS, int(on))
        try:
            if long_windows is None:
                yield self
            else:
                with self.long_refine_windows_for_call(long_windows):
                    yield self
        finally:
            if refine is not None and on != before:
                self.set_option(OPT_REFINE_OPTIMAL_CPTS, int(before))

    def synchronize(self, stream=None):
        check(self._L.wdx_ctx_synchronize(self.handle, stream))

    def dtw_last_launch(self) -> DtwLaunchInfoC:
        """Which DTW kernel the latest dispatch through this context took (wdx_dtw_last_launch; tests, diagnostics)."""
        info = DtwLaunchInfoC()
        check(self._L.wdx_dtw_last_launch(self.handle, C.byref(info)))
        return info

    def close(self):
        if self._h is not None and self.pid == os.getpid():
            self._L.wdx_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ctx: dict[tuple[int, int, int], Context] = {}


def default_context(device: int | None = None) -> Context:
    """Per-(process, thread, device) context.  Device defaults to $WDX_DEVICE or 0."""
    if device is None:
        device = int(os.environ.get("WDX_DEVICE", "0"))
    key = (os.getpid(), threading.get_ident(), device)
    c = _ctx.get(key)
    if c is None:
        c = Context(device)
        _ctx[key] = c
    return c
