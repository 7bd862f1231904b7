"""ctypes binding of the C ABI declared in include/pod_mi355x.h.

The product path has NO CPU fallback: if the HIP library is missing or a kernel entry point
returns an error, a RuntimeError is raised.  Tensors are passed as raw device pointers
(`tensor.data_ptr()`), the stream as the current torch HIP stream handle -- torch is plumbing
(device memory + streams), the kernels are ours.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p
from typing import Optional

import torch

from .build import LIB

POD_ABI_VERSION = 18
POD_MAX_LEVELS = 8
POD_MAX_CLASSES = 16
POD_MAX_RUNS = 64
POD_MAX_TOPK = 2048
POD_MAX_PROP_SAMPLES = 1024
POD_MAX_CLS_SAMPLES = 64
POD_MAX_CANDIDATES = 8192
POD_MAX_DETECTIONS = 128
POD_COCO_MAX_IOU, POD_COCO_MAX_REC, POD_COCO_MAX_AREA, POD_COCO_MAX_MAXDET, POD_COCO_MAX_KEEP, POD_COCO_LDS_GT = 16, 128, 4, 4, 128, 64
POD_CALIB_MAX_EDGES, POD_CALIB_BLOCK = 15, 1024
POD_VIS_MAX_INSTANCES, POD_VIS_INST_WORDS, POD_VIS_PRIM_WORDS, POD_VIS_LAUNCH_FRAMES = 256, 32, 12, 8
POD_VIS_COLOUR_ENTROPY, POD_VIS_COLOUR_FIXED, POD_VIS_COLOUR_PALETTE, POD_VIS_COLOUR_ARRAY = 0, 1, 2, 3
POD_VIS_COV_BY_RANK, POD_VIS_COV_OWN = 0, 1
POD_VIS_LABEL_BOX, POD_VIS_LABEL_GLYPH = 3, 4
POD_RESIZE_MAX_SIDE = 32768
POD_TRAIN_BATCH_MAX_FRAMES = 64
POD_SGD_CHUNK = 4096
POD_REG_LOSS_MOMENTS, POD_REG_LOSS_ENERGY, POD_MAX_REG_SAMPLES = 1, 2, 4096
POD_FULL_COV_NLL, POD_FULL_COV_MOMENTS, POD_FULL_COV_ENERGY = 1, 2, 3
POD_SGD_MAX_GROUPS = 8
POD_PDQ_MAX_SIDE, POD_PDQ_MAX_FRAME = 256, 32768
(POD_CORRUPT_GAUSSIAN_NOISE, POD_CORRUPT_SPECKLE_NOISE, POD_CORRUPT_IMPULSE_NOISE, POD_CORRUPT_GAUSSIAN_BLUR, POD_CORRUPT_DEFOCUS_BLUR,
 POD_CORRUPT_BRIGHTNESS, POD_CORRUPT_CONTRAST, POD_CORRUPT_SATURATE, POD_CORRUPT_KINDS) = range(9)
POD_RECAL_CHUNK, POD_RECAL_MAX_SEGMENTS, POD_RECAL_MAX_GRID, POD_RECAL_MAX_QUANTILES = 256, 64, 4096, 64
POD_SGD_CLIP_OFF, POD_SGD_CLIP_VALUE, POD_SGD_CLIP_NORM, POD_SGD_CLIP_FULL_MODEL = 0, 1, 2, 3

EXPORTS = ("pod_abi_version", "pod_mc_merge_score", "pod_maybe_words", "pod_score_maybe", "pod_merge_score_fused", "pod_reset_counters", "pod_level_topk", "pod_gather_candidates", "pod_gather_decode",
           "pod_decode_cov", "pod_nms_scratch_bytes", "pod_nms_cluster", "pod_bayes_fuse", "pod_anchor_stats_merge",
           "pod_ensemble_append", "pod_ensemble_merge",
           "pod_finalize", "pod_reg_nll", "pod_relu_dropout", "pod_bias_act", "pod_bias_act_to_nchw", "pod_bias_act_to_nhwc", "pod_expand_dropout", "pod_match_groundtruth", "pod_run_image", "pod_run_image_part", "pod_run_image_modes",
           "pod_absmax", "pod_wino_filter_transform", "pod_wino_conv3x3", "pod_wino_filter_split_bytes", "pod_wino_filter_transform_split", "pod_wino_conv3x3_split", "pod_sparse_reach", "pod_sparse_live_blocks", "pod_wino_reduce", "pod_conv1x1_filter_split_bytes", "pod_conv1x1_filter_split", "pod_conv1x1_split", "pod_reduce_partials", "pod_stem7x7_filter_split", "pod_stem7x7_split", "pod_maxpool3x3s2_cl", "pod_im2col3x3s2_cl",
           "pod_coco_eval_scratch_bytes", "pod_coco_eval_images", "pod_coco_accumulate_workspace_bytes", "pod_coco_accumulate",
           "pod_calib_keys", "pod_calib_reg_counts", "pod_calib_min_uncertainty_workspace_bytes", "pod_calib_min_uncertainty",
           "pod_calib_marginal_sort_workspace_bytes", "pod_calib_marginal_sort", "pod_calib_marginal_bins", "pod_calib_marginal_error_workspace_bytes",
           "pod_calib_marginal_error", "pod_vis_layout", "pod_vis_render", "pod_resize_taps", "pod_resize_coeffs", "pod_resize_frame_u8",
           "pod_label_anchors", "pod_train_loss_partials", "pod_train_loss",
           "pod_conv3x3_wgrad_partials", "pod_conv3x3_wgrad", "pod_relu_dropout_backward",
           "pod_conv1x1_wgrad_partials", "pod_conv1x1_wgrad", "pod_col2im3x3s2_cl", "pod_upsample2_sum_cl",
           "pod_conv1x1_wgrad_strided_partials", "pod_conv1x1_wgrad_strided", "pod_subsample2_scatter_cl",
           "pod_sgd_chunk_map", "pod_sgd_step", "pod_grad_bucket_layout", "pod_grad_pack",
           "pod_reg_score_partials", "pod_reg_score_loss", "pod_full_cov_partials", "pod_full_cov_loss",
           "pod_sgd_solver_workspace_bytes", "pod_sgd_step_solver", "pod_sgd_solver_reset",
           "pod_stem7x7_wgrad_partials", "pod_stem7x7_wgrad", "pod_maxpool3x3s2_backward_cl",
           "pod_train_batch_tiles", "pod_train_batch_u8",
           "pod_retinanet_infer_workspace", "pod_retinanet_score", "pod_retinanet_topk", "pod_retinanet_decode", "pod_retinanet_postprocess",
           "pod_retinanet_infer_image", "pod_reg_scores",
           "pod_pdq_workspace_bytes", "pod_pdq_pairs", "pod_pdq_assign",
           "pod_corrupt_scratch_bytes", "pod_corrupt_frame_u8",
           "pod_recal_workspace_bytes", "pod_recal_cls_sums", "pod_recal_reg_z", "pod_recal_moment", "pod_recal_ece_grid", "pod_recal_apply")
_SIZE_QUERIES = ("pod_abi_version", "pod_nms_scratch_bytes", "pod_coco_eval_scratch_bytes", "pod_coco_accumulate_workspace_bytes", "pod_maybe_words",
                 "pod_wino_filter_split_bytes", "pod_conv1x1_filter_split_bytes", "pod_calib_min_uncertainty_workspace_bytes",
                 "pod_calib_marginal_sort_workspace_bytes", "pod_calib_marginal_error_workspace_bytes", "pod_train_loss_partials",
                 "pod_conv3x3_wgrad_partials", "pod_conv1x1_wgrad_partials", "pod_conv1x1_wgrad_strided_partials", "pod_sgd_chunk_map",
                 "pod_grad_bucket_layout", "pod_reg_score_partials", "pod_full_cov_partials", "pod_sgd_solver_workspace_bytes",
                 "pod_stem7x7_wgrad_partials", "pod_train_batch_tiles", "pod_retinanet_infer_workspace", "pod_pdq_workspace_bytes", "pod_corrupt_scratch_bytes",
                 "pod_recal_workspace_bytes")
# include/pod_mi355x_test.h: test support (the dumps of the in-kernel draws, the generator and box_muller16 on given inputs, the f16 split) -- exported for tests/ and tools/, not part of the boundary
TEST_EXPORTS = ("pod_dump_cls_normals", "pod_dump_box_normals", "pod_debug_f16_split2", "pod_debug_philox4x32", "pod_debug_box_muller16")
POD_MODE_STANDARD_NMS, POD_MODE_BAYES_OD, POD_MODE_ANCHOR_STATISTICS = 0, 1, 2
POD_PART_SELECT, POD_PART_FINISH, POD_PART_CANDIDATES, POD_PART_FRONT, POD_PART_TAIL = 1, 2, 4, 5, 8
POD_MAX_MODE_TAILS = 8


class PodLevel(Structure):
    _fields_ = [("cls", c_void_p), ("cls_var", c_void_p), ("delta", c_void_p), ("reg_var", c_void_p), ("eps_cls", c_void_p),
                ("run_stride_cls", c_int64), ("run_stride_delta", c_int64), ("run_stride_reg", c_int64),
                ("H", c_int32), ("W", c_int32), ("anchor_base", c_int32), ("reserved", c_int32)]


class PodConfig(Structure):
    _fields_ = [("n_levels", c_int32), ("n_runs", c_int32), ("num_anchors", c_int32), ("num_classes", c_int32),
                ("cov_dims", c_int32), ("has_cls_var", c_int32), ("merge_quirk", c_int32), ("cls_samples", c_int32),
                ("prop_samples", c_int32), ("topk", c_int32), ("max_detections", c_int32),
                ("score_thresh", c_float), ("nms_thresh", c_float), ("affinity_thresh", c_float),
                ("box_weights", c_float * 4), ("philox_seed", c_uint64)]


class PodWorkspace(Structure):
    """include/pod_mi355x.h: PodWorkspace (device pointers of the per-geometry workspace, caller-owned)."""
    _fields_ = [(n, c_void_p) for n in (
        "anchors", "mean_cls", "mean_cls_var", "mean_delta", "mean_reg_var", "cand_keys", "cand_count", "maybe_bits",
        "sel_keys", "sel_count", "cat_keys", "cat_level", "probs_dense", "n_total", "cand_anchor_idx", "cand_level", "cand_class", "cand_score", "cand_probs",
        "cand_delta", "cand_reg_var", "cand_anchor", "cand_run_delta", "boxes", "cov", "keep", "n_keep", "nms_scratch",
        "m_boxes", "m_cov", "m_scores", "m_classes", "m_probs")] + [("n_capacity", c_int32), ("reserved", c_int32)]


class PodDetections(Structure):
    """include/pod_mi355x.h: PodDetections (pod_finalize's outputs)."""
    _fields_ = [(n, c_void_p) for n in ("boxes", "cov", "scores", "classes", "probs", "records", "n_det")]


class PodModeTail(Structure):
    """include/pod_mi355x.h: PodModeTail (one inference config of a pod_run_image_modes call)."""
    _fields_ = [("mode", c_int32), ("box_merge_mode", c_int32), ("cls_merge_mode", c_int32), ("reserved", c_int32), ("out", PodDetections)]


class PodConvSet(Structure):
    """include/pod_mi355x.h: PodConvSet (one convolution of a pod_wino_conv3x3_split launch)."""
    _fields_ = [("in_", c_void_p), ("out", c_void_p), ("Us", c_void_p), ("bias", c_void_p), ("in_amax", c_void_p), ("out_amax", c_void_p),
                ("offset", c_uint64), ("first_block", c_int32), ("replicas", c_int32), ("k_planes", c_int32), ("reserved", c_int32)]


class PodWinoConv(Structure):
    """include/pod_mi355x.h: PodWinoConv."""
    _fields_ = [("blocks", c_void_p), ("n_blocks", c_int32), ("n_sets", c_int32), ("C", c_int32), ("K", c_int32), ("relu", c_int32), ("p", c_float),
                ("seed", c_uint64), ("epoch", c_void_p), ("n_splits", c_int32), ("reserved", c_int32), ("split_stride", c_int64), ("live_blocks", c_void_p),
                ("sets", PodConvSet * 4)]


class PodCocoParams(Structure):
    """include/pod_mi355x.h: PodCocoParams (K17, COCO bbox evaluation)."""
    _fields_ = [("n_iou", c_int32), ("n_rec", c_int32), ("n_area", c_int32), ("n_maxdet", c_int32), ("n_cat", c_int32), ("reserved", c_int32),
                ("iou_thrs", c_double * POD_COCO_MAX_IOU), ("rec_thrs", c_double * POD_COCO_MAX_REC), ("area_rng", c_double * (2 * POD_COCO_MAX_AREA)),
                ("max_dets", c_int32 * POD_COCO_MAX_MAXDET)]


class PodVisList(Structure):
    """include/pod_mi355x.h: PodVisList (K19, one instance list of pod_vis_layout)."""
    _fields_ = [(n, c_void_p) for n in ("boxes", "cov", "probs", "colours", "count", "out", "n_out")] + \
               [(n, c_int32) for n in ("max_n", "box_stride", "cov_stride", "prob_stride", "n_probs", "colour_mode", "colour_stride", "cov_pairing")] + \
               [("colour", c_float * 4), ("frame_h", c_int32), ("frame_w", c_int32), ("scale", c_float), ("alpha", c_float)]


class PodVisFrame(Structure):
    """include/pod_mi355x.h: PodVisFrame (K19, one frame of pod_vis_render)."""
    _fields_ = [("src", c_void_p), ("sy", c_int64), ("sx", c_int64), ("sc", c_int64)] + \
               [(n, c_int32) for n in ("src_h", "src_w", "bgr", "bilinear", "frame_h", "frame_w", "out_h", "out_w")] + \
               [("dst", c_void_p), ("scale", c_float), ("stroke", c_float), ("inst", c_void_p * 2), ("n_inst", c_void_p * 2),
                ("labels", c_void_p), ("atlas", c_void_p), ("n_labels", c_int32), ("reserved", c_int32)]


class PodLevelGrad(Structure):
    """include/pod_mi355x.h: PodLevelGrad (K21, the gradient planes of one level)."""
    _fields_ = [(n, c_void_p) for n in ("cls", "cls_var", "delta", "reg_var")]


class PodSgdTensor(Structure):
    """include/pod_mi355x.h: PodSgdTensor (K25, one tensor of pod_sgd_step's table)."""
    _fields_ = [(n, c_void_p) for n in ("w", "grad", "momentum", "folded", "scale")] + [("n", c_int64), ("per_channel", c_int64)]


class PodSgdSolver(Structure):
    """include/pod_mi355x.h: PodSgdSolver (K29, the settings of one pod_sgd_step_solver call)."""
    _fields_ = [(n, c_int32) for n in ("n_groups", "nesterov", "clip_type", "guard")] + \
               [("lr", c_float * POD_SGD_MAX_GROUPS), ("wd", c_float * POD_SGD_MAX_GROUPS), ("momentum", c_float), ("clip_value", c_float),
                ("iteration", c_int64), ("watch", c_void_p * 4)]


class PodSgdSolverStatus(Structure):
    """include/pod_mi355x.h: PodSgdSolverStatus (K29, the first 32 bytes of the solver's workspace)."""
    _fields_ = [("bad_steps", c_int64), ("first_bad_iteration", c_int64), ("last_norm", c_double), ("poisoned", c_int32), ("reserved", c_int32)]


class PodTrainFrame(Structure):
    """include/pod_mi355x.h: PodTrainFrame (K31, one frame of pod_train_batch_u8's table)."""
    _fields_ = [("src", c_void_p), ("in_h", c_int32), ("in_w", c_int32), ("row_stride", c_int64),
                ("xbounds", c_void_p), ("xcoeffs", c_void_p), ("xk", c_int32), ("reserved0", c_int32),
                ("ybounds", c_void_p), ("ycoeffs", c_void_p), ("yk", c_int32), ("reserved1", c_int32),
                ("dst", c_void_p), ("out_h", c_int32), ("out_w", c_int32), ("flip_channels", c_int32), ("hflip", c_int32), ("first_tile", c_int64)]


class PodRetinaNetLayout(Structure):
    """include/pod_mi355x.h: PodRetinaNetLayout (K32, byte offsets into pod_retinanet_infer_image's workspace)."""
    _fields_ = [(n, c_int64) for n in ("cand_keys", "cand_count", "sel_keys", "sel_count", "cat_keys", "cat_level", "n_total", "cand_flat", "cand_level",
                                       "boxes", "scores", "classes", "keep", "n_keep", "nms_scratch", "total")]


class PodCorruption(Structure):
    """include/pod_mi355x.h: PodCorruption (K35, one corruption of pod_corrupt_frame_u8)."""
    _fields_ = [("kind", c_int32), ("radius", c_int32), ("p0", c_double), ("p1", c_double), ("taps", c_void_p),
                ("impulse_threshold", c_uint32), ("reserved", c_uint32), ("key", c_uint64)]


class PodError(RuntimeError):
    pass


_lib = None


def library_path() -> str:
    return os.environ.get("POD_MI355X_LIB", LIB)


def load() -> ctypes.CDLL:
    """Loads libpod_mi355x.so (built by `python -m pod_compare_amd.build`); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise PodError("HIP library {} not found: run `python -m pod_compare_amd.build` (hipcc, gfx950). "
                       "There is no CPU fallback for the hot path.".format(path))
    lib = ctypes.CDLL(path)
    for name in EXPORTS + TEST_EXPORTS:
        if not hasattr(lib, name):
            raise PodError("{} does not export {}".format(path, name))
    P = c_void_p
    lib.pod_abi_version.restype = ctypes.c_int
    lib.pod_nms_scratch_bytes.restype = c_size_t
    lib.pod_nms_scratch_bytes.argtypes = [c_int32]
    lib.pod_reset_counters.argtypes = [P, c_int32, P]
    lib.pod_mc_merge_score.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, P, P, P, P, P, P]
    lib.pod_maybe_words.argtypes = [POINTER(PodConfig), POINTER(PodLevel)]
    lib.pod_maybe_words.restype = c_int64
    lib.pod_score_maybe.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, P, P, P, P, P]
    lib.pod_merge_score_fused.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, P, P, P, P]
    lib.pod_level_topk.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, P, P, P, P, P, P]
    lib.pod_gather_candidates.argtypes = [POINTER(PodConfig), POINTER(PodLevel)] + [P] * 16
    lib.pod_gather_decode.argtypes = [POINTER(PodConfig), POINTER(PodLevel)] + [P] * 18      # 17 pointers and the stream
    lib.pod_decode_cov.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, c_int32, P, P, P, P, P, P, P, c_int32, P, P, P]
    lib.pod_nms_cluster.argtypes = [POINTER(PodConfig), P, c_int32, P, P, P, P, P, P, P]
    lib.pod_bayes_fuse.argtypes = [POINTER(PodConfig), P, P, P, P, P, P, P, P, c_int32, c_int32, P, P, P, P, P, P]
    lib.pod_anchor_stats_merge.argtypes = [POINTER(PodConfig), P, P, P, P, P, P, P, P, P, P, P, P, P]
    lib.pod_ensemble_append.argtypes = [POINTER(PodConfig), P, P, P, P, P, P, c_int32, P, P, P, P, P, P]
    lib.pod_ensemble_merge.argtypes = [POINTER(PodConfig), P, c_int32, P, P, P, P, P, P, P, P, P, P, P, P]
    lib.pod_finalize.argtypes = [POINTER(PodConfig)] + [P] * 7 + [c_float] * 4 + [P] * 7 + [P]
    lib.pod_reg_nll.argtypes = [P, P, P, c_int32, P, P]
    lib.pod_match_groundtruth.argtypes = [P, P, P, P, c_int32, P, P, P, c_int32, c_int32, c_float, c_float, P, P, P, P, P, P]
    lib.pod_relu_dropout.argtypes = [P, c_int64, c_float, c_uint64, c_uint64, P]
    lib.pod_bias_act_to_nchw.argtypes = [P, P, P, c_int64, c_int32, c_int64, c_int32, c_float, c_uint64, c_uint64, P]
    lib.pod_bias_act_to_nhwc.argtypes = [P, P, P, c_int64, c_int32, c_int64, c_int32, P]
    lib.pod_expand_dropout.argtypes = [P, P, c_int64, c_int32, c_float, c_uint64, c_uint64, P, P]
    lib.pod_wino_filter_transform.argtypes = [P, P, c_int32, c_int32, P]
    lib.pod_wino_conv3x3.argtypes = [P, P, P, P, P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_uint64, c_uint64, P, P]
    lib.pod_wino_filter_split_bytes.argtypes = [c_int32, c_int32]
    lib.pod_wino_filter_split_bytes.restype = c_int64
    lib.pod_wino_filter_transform_split.argtypes = [P, P, c_int32, c_int32, P]
    lib.pod_wino_conv3x3_split.argtypes = [POINTER(PodWinoConv), P]
    lib.pod_absmax.argtypes = [P, c_int64, P, P]
    lib.pod_sparse_reach.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, P, P, P, P]
    lib.pod_sparse_live_blocks.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, c_int32, P, c_int32, c_int32, P, P]
    lib.pod_debug_f16_split2.argtypes = [P, c_float, P, c_int64, P]
    lib.pod_debug_philox4x32.argtypes = [P, P, c_int64, P]
    lib.pod_debug_box_muller16.argtypes = [P, P, c_int64, P]
    lib.pod_wino_reduce.argtypes = [P, c_int32, c_int64, P, P, c_int64, c_int32, c_int32, c_int32, P, P]
    lib.pod_reduce_partials.argtypes = [P, c_int32, c_int64, P, P, P, c_int64, c_int32, c_int32, P, P]
    lib.pod_stem7x7_filter_split.argtypes = [P, P, P]
    lib.pod_stem7x7_split.argtypes = [P, c_int32, c_int32, c_int32, P, P, P, P, P, c_int32, c_int32, c_int32, P, P, P]
    lib.pod_maxpool3x3s2_cl.argtypes = [P, P, c_int32, c_int32, c_int32, P]
    lib.pod_im2col3x3s2_cl.argtypes = [P, P, c_int32, c_int32, c_int32, c_int32, P]
    lib.pod_conv1x1_filter_split.argtypes = [P, P, c_int32, c_int32, P]
    lib.pod_conv1x1_split.argtypes = [P, P, P, P, P] + [c_int32] * 9 + [P, c_int32, P, P, P]
    lib.pod_conv1x1_filter_split_bytes.argtypes = [c_int32, c_int32]
    lib.pod_conv1x1_filter_split_bytes.restype = c_int64
    lib.pod_bias_act.argtypes = [P, P, P, P, c_int64, c_int32, c_int64, c_int32, c_float, c_uint64, c_uint64, P]
    lib.pod_dump_cls_normals.argtypes = [POINTER(PodConfig), POINTER(PodLevel), c_int32, P, P]
    lib.pod_dump_box_normals.argtypes = [POINTER(PodConfig), P, c_int32, P, P]
    lib.pod_run_image.argtypes = [POINTER(PodConfig), POINTER(PodLevel), POINTER(PodWorkspace), c_int32, c_int32, c_int32,
                                  c_int32, c_int32, c_int32, c_int32, POINTER(PodDetections), P]
    lib.pod_run_image_part.argtypes = [POINTER(PodConfig), POINTER(PodLevel), POINTER(PodWorkspace), c_int32, c_int32, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, POINTER(PodDetections), c_int32, P]
    lib.pod_run_image_modes.argtypes = [POINTER(PodConfig), POINTER(PodLevel), POINTER(PodWorkspace), POINTER(PodModeTail), c_int32,
                                        c_int32, c_int32, c_int32, c_int32, P]
    lib.pod_coco_eval_scratch_bytes.argtypes = [c_int32, c_int32]
    lib.pod_coco_eval_scratch_bytes.restype = c_size_t
    lib.pod_coco_eval_images.argtypes = [POINTER(PodCocoParams), P, c_int32] + [P] * 12 + [P]
    lib.pod_coco_accumulate_workspace_bytes.argtypes = [c_int64]
    lib.pod_coco_accumulate_workspace_bytes.restype = c_size_t
    lib.pod_coco_accumulate.argtypes = [POINTER(PodCocoParams), P, c_int32, c_int64] + [P] * 9 + [P]
    lib.pod_calib_keys.argtypes = [P, c_int32, P, P, c_int32, c_int32, P, P, P, P, P]
    lib.pod_calib_reg_counts.argtypes = [P, P, P, P, c_int32, P, c_int32, P, P]
    lib.pod_calib_min_uncertainty_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.pod_calib_min_uncertainty_workspace_bytes.restype = c_size_t
    lib.pod_calib_min_uncertainty.argtypes = [P, P, P, c_int32, c_int32, P, P, P, c_int32, c_int32, c_int64, P, P, P, P]
    lib.pod_calib_marginal_sort_workspace_bytes.argtypes = [c_int32]
    lib.pod_calib_marginal_sort_workspace_bytes.restype = c_size_t
    lib.pod_calib_marginal_sort.argtypes = [P, c_int32, P, P, P, P]
    lib.pod_calib_marginal_bins.argtypes = [P, c_int32, P, c_int32, P, P]
    lib.pod_calib_marginal_error_workspace_bytes.argtypes = [c_int32]
    lib.pod_calib_marginal_error_workspace_bytes.restype = c_size_t
    lib.pod_calib_marginal_error.argtypes = [P, P, P, c_int32, P, c_int32, P, c_int32, P, P, P]
    lib.pod_vis_layout.argtypes = [POINTER(PodVisList), c_int32, P]
    lib.pod_vis_render.argtypes = [POINTER(PodVisFrame), c_int32, P]
    lib.pod_resize_taps.argtypes = [c_int32, c_int32]
    lib.pod_resize_coeffs.argtypes = [c_int32, c_int32, P, P]
    lib.pod_resize_frame_u8.argtypes = [P, c_int32, c_int32, c_int64, P, P, c_int32, P, P, c_int32, P, c_int32, c_int32, c_int32, P]
    lib.pod_label_anchors.argtypes = [P, c_int32, P, P, P, c_int32, c_int32, c_int32, c_float, c_float, P, P, P, P, P]
    lib.pod_train_loss_partials.argtypes = [POINTER(PodConfig), POINTER(PodLevel)]
    lib.pod_train_loss_partials.restype = c_int64
    lib.pod_train_loss.argtypes = [POINTER(PodConfig), POINTER(PodLevel), POINTER(PodLevelGrad), P, P, P, c_int32, P, c_int32,
                                   c_float, c_float, c_float, P, P, P, P, P, P]
    lib.pod_conv3x3_wgrad_partials.argtypes = [P, c_int32, c_int32, c_int32, c_int32, c_int32]
    lib.pod_conv3x3_wgrad_partials.restype = c_int64
    lib.pod_conv3x3_wgrad.argtypes = [P, P, P, c_int32, c_int32, c_int32, c_int32, c_int32, P, P, P, P, P, P]
    lib.pod_relu_dropout_backward.argtypes = [P, P, P, c_int64, c_float, P, P]
    lib.pod_conv1x1_wgrad_partials.argtypes = [c_int64, c_int32, c_int32]
    lib.pod_conv1x1_wgrad_partials.restype = c_int64
    lib.pod_conv1x1_wgrad.argtypes = [P, P, c_int64, c_int32, c_int32, P, P, P, P, P, P]
    lib.pod_col2im3x3s2_cl.argtypes = [P, P, P, P, c_int32, c_int32, c_int32, P, P]
    lib.pod_upsample2_sum_cl.argtypes = [P, c_int32, c_int32, P, P, c_int32, P, P]
    lib.pod_conv1x1_wgrad_strided_partials.argtypes = [c_int32] * 6
    lib.pod_conv1x1_wgrad_strided_partials.restype = c_int64
    lib.pod_conv1x1_wgrad_strided.argtypes = [P, P] + [c_int32] * 6 + [P] * 6
    lib.pod_subsample2_scatter_cl.argtypes = [P, P, P, P, c_int32, c_int32, c_int32, P, P]
    lib.pod_sgd_chunk_map.argtypes = [POINTER(PodSgdTensor), c_int32, P, c_int64]
    lib.pod_sgd_chunk_map.restype = c_int64
    lib.pod_sgd_step.argtypes = [POINTER(PodSgdTensor), P, c_int32, P, c_int64, c_float, c_float, c_float, P]
    lib.pod_grad_bucket_layout.argtypes = [POINTER(PodSgdTensor), c_int32, P]
    lib.pod_grad_bucket_layout.restype = c_int64
    lib.pod_grad_pack.argtypes = [POINTER(PodSgdTensor), P, c_int32, P, c_int64, P, P, c_int64, c_float, P]
    lib.pod_reg_score_partials.argtypes = [POINTER(PodConfig), POINTER(PodLevel)]
    lib.pod_reg_score_partials.restype = c_int64
    lib.pod_reg_score_loss.argtypes = [POINTER(PodConfig), POINTER(PodLevel), POINTER(PodLevelGrad), P, P, P, c_int32, P, c_int32,
                                       c_int32, c_int32, c_float, P, P, P, P, P, P]
    lib.pod_full_cov_partials.argtypes = lib.pod_reg_score_partials.argtypes
    lib.pod_full_cov_partials.restype = c_int64
    lib.pod_full_cov_loss.argtypes = lib.pod_reg_score_loss.argtypes
    lib.pod_sgd_solver_workspace_bytes.argtypes = [c_int32, c_int64]
    lib.pod_sgd_solver_workspace_bytes.restype = c_size_t
    lib.pod_sgd_step_solver.argtypes = [POINTER(PodSgdTensor), P, c_int32, P, c_int64, P, P, POINTER(PodSgdSolver), P, P]
    lib.pod_sgd_solver_reset.argtypes = [P, P]
    lib.pod_stem7x7_wgrad_partials.argtypes = [c_int32] * 5
    lib.pod_stem7x7_wgrad_partials.restype = c_int64
    lib.pod_stem7x7_wgrad.argtypes = [P, c_int32, c_int32, c_int32, c_int32, P, P, P, c_int32, c_int32, P, P, P, P, P]
    lib.pod_maxpool3x3s2_backward_cl.argtypes = [P, P, P, c_int32, c_int32, c_int32, P, P]
    lib.pod_train_batch_tiles.argtypes = [POINTER(PodTrainFrame), c_int32]
    lib.pod_train_batch_tiles.restype = c_int64
    lib.pod_train_batch_u8.argtypes = [POINTER(PodTrainFrame), P, c_int32, c_int64, P]
    lib.pod_retinanet_infer_workspace.argtypes = [POINTER(PodConfig), POINTER(PodLevel), POINTER(PodRetinaNetLayout)]
    lib.pod_retinanet_infer_workspace.restype = c_int64
    lib.pod_retinanet_score.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, P]
    lib.pod_retinanet_topk.argtypes = lib.pod_level_topk.argtypes
    lib.pod_retinanet_decode.argtypes = [POINTER(PodConfig), POINTER(PodLevel)] + [P] * 11
    lib.pod_retinanet_postprocess.argtypes = [POINTER(PodConfig)] + [P] * 5 + [c_float] * 4 + [P] * 5
    lib.pod_retinanet_infer_image.argtypes = [POINTER(PodConfig), POINTER(PodLevel), P, P, c_int32, c_int32, c_int32, c_int32, P, P, P, P, P]
    lib.pod_reg_scores.argtypes = [P, P, P, c_int32, c_int32, c_uint64, P, P, P, P, P]
    lib.pod_pdq_workspace_bytes.argtypes = [c_int32]
    lib.pod_pdq_workspace_bytes.restype = c_size_t
    lib.pod_pdq_pairs.argtypes = [P, P, P, P, c_int32, P, P, P, c_int32, P, P, c_double, P, P, P, P, P]      # the first four: host tables
    lib.pod_pdq_assign.argtypes = [P, P, P, c_int32, P, P, P, P, P, P]
    lib.pod_corrupt_scratch_bytes.argtypes = [c_int32, c_int32, c_int32]
    lib.pod_corrupt_scratch_bytes.restype = c_size_t
    lib.pod_corrupt_frame_u8.argtypes = [P, c_int32, c_int32, c_int64, P, c_int64, POINTER(PodCorruption), P, c_size_t, P]
    lib.pod_recal_workspace_bytes.argtypes = [c_int64, c_int32]
    lib.pod_recal_workspace_bytes.restype = c_size_t
    lib.pod_recal_cls_sums.argtypes = [P, P, c_int64, c_double, P, c_int32, P, P, P]
    lib.pod_recal_reg_z.argtypes = [P, P, P, P, c_int32, c_int32, P, P, P, P, P]
    lib.pod_recal_moment.argtypes = [P, P, c_int64, c_int32, P, P, P, P, P, P]
    lib.pod_recal_ece_grid.argtypes = [P, P, c_int64, c_int32, c_int32, P, c_int32, c_int32, P, c_int32, P, P, P, P, P, P]
    lib.pod_recal_apply.argtypes = [P, P, c_int32, c_int32, c_int32, c_double, P, c_int32, P, P]
    for name in EXPORTS + TEST_EXPORTS:
        if name not in _SIZE_QUERIES:
            getattr(lib, name).restype = ctypes.c_int
    if lib.pod_abi_version() != POD_ABI_VERSION:
        raise PodError("ABI version mismatch: library {} vs binding {}".format(lib.pod_abi_version(), POD_ABI_VERSION))
    _lib = lib
    return lib


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "pod_mi355x kernels need contiguous tensors"
    return t.data_ptr()


def current_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise PodError("{} failed with code {} ({})".format(what, rc, {-1: "invalid argument", -2: "HIP launch error"}.get(rc, "?")))
