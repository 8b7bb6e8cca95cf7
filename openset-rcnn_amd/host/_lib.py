"""ctypes binding of libosr_hip.so (include/osr.h). The product path has no fallback: if the library is
missing or an entry point fails, an exception is raised -- never a silent eager/CPU substitute."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must be imported first: libosr_hip.so then binds to torch's libamdhip64.so.7)

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libosr_hip.so")

OSR_MAX_LEVELS = 8
OSR_F32, OSR_F16, OSR_BF16 = 0, 1, 2
RPN_SELECT_MAXK, RPN_SELECT_WIDE_MAXK = 2048, 8192  # csrc/osr_select.h SEL_MAXK; include/osr.h OSR_RPN_SELECT_WIDE_MAXK
ABI_VERSION = 1


class OsrError(RuntimeError):
    pass


ERR_UNSUPPORTED = -2  # include/osr.h OSR_ERR_UNSUPPORTED: nothing was launched, the caller takes its other path


class ConvParams(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("hi", C.c_int32), ("wi", C.c_int32), ("cin", C.c_int32),
        ("ho", C.c_int32), ("wo", C.c_int32), ("cout", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32),
        ("pad_h", C.c_int32), ("pad_w", C.c_int32),
        ("in_stride_n", C.c_int64), ("in_stride_h", C.c_int64), ("in_stride_w", C.c_int64),
        ("out_stride_n", C.c_int64), ("out_stride_h", C.c_int64), ("out_stride_w", C.c_int64),
        ("res_stride_n", C.c_int64), ("res_stride_h", C.c_int64), ("res_stride_w", C.c_int64),
        ("relu", C.c_int32), ("res_mode", C.c_int32), ("pad_mode", C.c_int32),
        ("in_dtype", C.c_int32), ("out_dtype", C.c_int32), ("concurrency", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("row_seg_counts", C.c_void_p), ("row_seg_rows", C.c_int32),
    ]


class ConvLevel(C.Structure):
    """include/osr.h osr_conv_level: one pyramid level of a multi-level launch."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("deltas", C.c_void_p), ("ctr", C.c_void_p), ("weight", C.c_void_p), ("bias", C.c_void_p),
                ("n", C.c_int32), ("hi", C.c_int32), ("wi", C.c_int32), ("reserved", C.c_int32)]


MAX_CONV_LEVELS = 6


class BottleneckParams(C.Structure):
    _fields_ = [("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32), ("cmid", C.c_int32), ("cout", C.c_int32),
                ("dtype", C.c_int32), ("has_proj", C.c_int32)]


class LinearSplitParams(C.Structure):
    """include/osr.h osr_linear_split_params."""
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("relu", C.c_int32), ("ldx", C.c_int64), ("ldo", C.c_int64),
                ("row_seg_counts", C.c_void_p), ("row_seg_rows", C.c_int32), ("reserved", C.c_int32)]


class LossOptions(C.Structure):
    _fields_ = [("box_loss_type", C.c_int32), ("box_smooth_l1_beta", C.c_float), ("aux_smooth_l1_beta", C.c_float)]


BOX_LOSS_TYPES = {"iou": 0, "smooth_l1": 1, "giou": 2, "diou": 3, "ciou": 4}
PLN_DISTANCES = {"COS": 0, "L1": 1, "L2": 2}


class RpnLevels(C.Structure):
    _fields_ = [
        ("num_levels", C.c_int32), ("num_anchors", C.c_int32),
        ("h", C.c_int32 * OSR_MAX_LEVELS), ("w", C.c_int32 * OSR_MAX_LEVELS),
        ("stride", C.c_int32 * OSR_MAX_LEVELS), ("offset", C.c_int64 * OSR_MAX_LEVELS),
    ]


class SgdSegment(C.Structure):
    """include/osr.h osr_sgd_segment: one parameter (a row range of a master) of osr_sgd_step_multi_ex / osr_grad_norm_partials."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("momentum", C.c_void_p), ("row_scale", C.c_void_p), ("lowp", C.c_void_p),
                ("n", C.c_int64), ("row_elems", C.c_int64), ("lowp_dtype", C.c_int32), ("chunk0", C.c_int32), ("nchunks", C.c_int32),
                ("lr_factor", C.c_float), ("weight_decay", C.c_float), ("nesterov", C.c_int32)]


OSR_CLIP_NONE, OSR_CLIP_VALUE, OSR_CLIP_NORM = 0, 1, 2


class PackTensor(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("cin", C.c_int32),
                ("elem_bytes", C.c_int32), ("reserved", C.c_int32)]


class RoiOptions(C.Structure):
    """include/osr.h osr_roi_options: the pooler's `aligned` and `sampling_ratio` (NULL = {1, 0})."""
    _fields_ = [("aligned", C.c_int32), ("sampling_ratio", C.c_int32)]


class GnTerm(C.Structure):
    """include/osr.h osr_gn_term: one term of osr_gn_relu_merge."""
    _fields_ = [("x", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("h", C.c_int32), ("w", C.c_int32), ("up2", C.c_int32), ("reserved", C.c_int32)]


GN_MAX_TERMS = 4
SEMSEG_LABELS, SEMSEG_VALUES = 0, 1
PANOPTIC_MAX_INSTANCES = 1024  # csrc/osr_panoptic.hip PC_MAX_K
PANOPTIC_MAX_STUFF = 255       # labels 1 .. 255
CONF_LABELS, CONF_VALUES = 0, 1
PQ_MAX_GT, PQ_MAX_PRED = 1023, 2047  # csrc/osr_seg_eval.hip PP_MAX_G / PP_MAX_P
COCO_BBOX, COCO_KEYPOINTS = 0, 1
COCO_MAX_CAP, COCO_MAX_DET, COCO_MAX_THRS, COCO_MAX_AREAS, COCO_MAX_KPTS, COCO_MAX_GROUP = 1024, 128, 16, 8, 32, 4096  # csrc/osr_eval_match.h EM_MAX_*, csrc/osr_coco_eval.hip CM_MAX_KP
OS_COCO_MAX_CAP, OS_COCO_MAX_DET, OS_COCO_MAX_THRS, OS_COCO_MAX_AREAS, OS_COCO_MAX_GT = 1024, 128, 16, 8, 4096  # csrc/osr_eval_match.h EM_MAX_*
OS_COCO_SETS = 3  # flag words per (detection, area range): own slot, other known, unknown
LVIS_MAX_CAP, LVIS_MAX_DET, LVIS_MAX_THRS, LVIS_MAX_AREAS, LVIS_MAX_GROUP = 1024, 512, 16, 8, 4096  # csrc/osr_lvis_eval.hip LV_MAX_DET, csrc/osr_eval_match.h EM_MAX_*
VOC_MAX_CAP, VOC_MAX_GT = 1024, 4096  # csrc/osr_eval_match.h EM_MAX_CAP / EM_MAX_G (the flag bits: host/evaluation.py VOC_*)


PROPOSAL_MAX_CAP, PROPOSAL_MAX_GT, PROPOSAL_MAX_AREAS, PROPOSAL_MAX_LIMITS, PROPOSAL_MAX_THRS = 2048, 1024, 8, 8, 16  # csrc/osr_proposal_recall.hip PR_MAX_*


class Pyramid(C.Structure):
    _fields_ = [
        ("num_levels", C.c_int32), ("c", C.c_int32),
        ("h", C.c_int32 * OSR_MAX_LEVELS), ("w", C.c_int32 * OSR_MAX_LEVELS),
        ("scale", C.c_float * OSR_MAX_LEVELS), ("data", C.c_void_p * OSR_MAX_LEVELS),
    ]


P, I32, I64, F32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
F32x3, F32x4 = C.c_float * 3, C.c_float * 4

# name -> (restype, argtypes); mirrors include/osr.h one to one
PROTOTYPES = {
    "osr_abi_version": (I32, []),
    "osr_last_error": (C.c_char_p, []),
    "osr_stem_padded_width": (I32, [I32]),
    "osr_preprocess": (I32, [P, I32, I32, I32, I32, I32, I32, C.POINTER(C.c_float), C.POINTER(C.c_float), P, I32, P]),
    "osr_conv2d_fwd": (I32, [C.POINTER(ConvParams), P, P, P, P, P, P]),
    "osr_conv2d_fwd_workspace_bytes": (I64, [C.POINTER(ConvParams)]),
    "osr_conv2d_fwd_describe": (I32, [C.POINTER(ConvParams), I32, P, I32]),
    "osr_conv2d_fwd_masked": (I32, [C.POINTER(ConvParams), P, P, P, P, P, P, P]),
    "osr_conv2d_chain_fwd": (I32, [C.POINTER(ConvParams), P, P, P, P, P, I32, P, P, P]),
    "osr_conv2d_chain_fwd_ex": (I32, [C.POINTER(ConvParams), P, P, P, P, P, I32, P, P, P, P]),
    "osr_bottleneck_fwd": (I32, [C.POINTER(BottleneckParams), P, P, P, P, P, P, P, P, P, P, P]),
    "osr_resize_tmp_bytes": (I64, [I32, I32]),
    "osr_resize_bilinear_u8": (I32, [P, I32, I32, I64, P, P, I32, P, P, I32, I32, I32, I32, I32, P, I64, P, P]),
    "osr_resize_bilinear_u8_planar": (I32, [P, I32, I32, I32, P, P, I32, P, P, I32, I32, I32, I32, I32, I32, P, I64, P, P]),
    "osr_stem_maxpool_fwd": (I32, [P, I32, I32, I32, P, I32, P, P, I32, P]),
    "osr_stem_maxpool_fwd_raw": (I32, [P, I32, I32, I32, I32, I32, I32, C.POINTER(C.c_float), C.POINTER(C.c_float), P, I32, P, P, I32, P]),
    "osr_maxpool3x3s2": (I32, [P, I32, I32, I32, I32, P, I32, P]),
    "osr_stem_pool_bwd": (I32, [P, P, I32, I32, I32, I32, P, I32, P]),
    "osr_stem_wgrad_workspace_bytes": (I64, [I32, I32, I32]),
    "osr_stem_wgrad": (I32, [P, P, I32, I32, I32, P, I32, P, I64, I32, P]),
    "osr_subsample2": (I32, [P, I32, I32, I32, I32, P, I32, P]),
    "osr_deform_cols": (I32, [P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, P, I32, P]),
    "osr_gemm_f32": (I32, [P, I64, P, P, P, I64, I32, I32, I32, I32, P]),
    "osr_gemm_f32_tn_workspace_bytes": (I64, [I32, I32, I32]),
    "osr_gemm_f32_tn": (I32, [P, I64, P, I64, P, I64, I32, I32, I32, P, I64, P]),
    "osr_split_rows_bf16": (I32, [P, I32, I32, P, P, P]),
    "osr_linear_split_fwd": (I32, [C.POINTER(LinearSplitParams), P, P, P, P, P, P]),
    "osr_conv2d_split_fwd": (I32, [C.POINTER(ConvParams), P, P, P, P, P, P, P]),
    "osr_split_rows_bf16_t": (I32, [P, I32, I32, P, P, P]),
    "osr_linear_split_dgrad": (I32, [P, I64, P, P, P, I64, P, I64, I32, I32, I32, P, I32, P]),
    "osr_linear_split_wgrad_workspace_bytes": (I64, [I32, I32, I32]),
    "osr_linear_split_wgrad": (I32, [P, I64, P, I64, P, I64, I32, I32, I32, P, I32, P, I64, P]),
    "osr_cfrpn_head_tail": (I32, [P, I32, I64, I32, P, P, P, P, P, P, P]),
    "osr_cfrpn_head_fwd": (I32, [C.POINTER(ConvParams), P, P, P, P, P, P, P, P]),
    "osr_cfrpn_head_fwd_ex": (I32, [C.POINTER(ConvParams), P, P, P, P, P, P, P, P, P]),
    "osr_conv2d_fwd_pair": (I32, [C.POINTER(ConvParams), P, P, P, I32, I32, P, P, P, I32, I32, P, P]),
    "osr_conv2d_fwd_levels": (I32, [C.POINTER(ConvParams), I32, C.POINTER(ConvLevel), P, P, P]),
    "osr_cfrpn_head_fwd_levels": (I32, [C.POINTER(ConvParams), I32, C.POINTER(ConvLevel), P, P, P, P, P]),
    "osr_rpn_select_capacity": (I32, [C.POINTER(RpnLevels), I32]),
    "osr_rpn_select_workspace_bytes": (I64, [C.POINTER(RpnLevels), I32, I32]),
    "osr_rpn_select": (I32, [C.POINTER(RpnLevels), P, P, P, I32, P, I32, F32, P, P, P, P, P, P, P, I64, P]),
    "osr_rpn_select_ex": (I32, [C.POINTER(RpnLevels), P, P, P, I32, P, I32, F32, I32, P, P, P, P, P, P, P, P, P, I64, P]),
    "osr_rpn_select_wide_capacity": (I32, [C.POINTER(RpnLevels), I32]),
    "osr_rpn_select_wide_workspace_bytes": (I64, [C.POINTER(RpnLevels), I32, I32]),
    "osr_rpn_select_wide": (I32, [C.POINTER(RpnLevels), P, P, P, I32, P, I32, F32, I32, P, P, P, P, P, P, P, P, P, I64, P]),
    "osr_retinanet_select_capacity": (I32, [C.POINTER(RpnLevels), I32]),
    "osr_retinanet_select_workspace_bytes": (I64, [C.POINTER(RpnLevels), I32, I32, I32]),
    "osr_retinanet_select": (I32, [C.POINTER(RpnLevels), P, P, I32, I64, P, I64, I32, I32, I32, F32, P, P, P, P, P, P, P, P, P, I64, P]),
    # Panoptic FPN (csrc/osr_semseg.hip, csrc/osr_panoptic.hip)
    "osr_group_norm_stats_workspace_bytes": (I64, [I32, I32, I32, I32]),
    "osr_group_norm_stats": (I32, [P, I32, I32, I32, I32, I32, F32, P, P, P, I64, P]),
    "osr_gn_relu_merge": (I32, [C.POINTER(GnTerm), I32, I32, I32, I32, I32, I32, P, P]),
    "osr_semseg_resample": (I32, [P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, P, P]),
    "osr_panoptic_combine_workspace_bytes": (I64, [I32, I32, I32]),
    "osr_panoptic_combine": (I32, [P, P, P, P, I32, P, I32, I32, F32, I32, F32, P, P, P, P, P, I64, P]),
    # segmentation evaluators (csrc/osr_seg_eval.hip)
    "osr_semseg_confusion": (I32, [P, I32, P, I32, I32, I32, I32, P, P, P]),
    "osr_panoptic_pair_counts": (I32, [P, P, I32, P, I32, I32, I32, P, P, P]),
    "osr_pq_accumulate": (I32, [P, I32, I32, P, P, I32, P, P, P, P]),
    # COCO box / keypoint matching (csrc/osr_coco_eval.hip)
    "osr_coco_match_workspace_bytes": (I64, [I32, I32, I32]),
    "osr_coco_match": (I32, [I32, P, P, P, P, P, I32, I32, I32, I32, P, P, P, P, P, P, I32, I32, P, I32, P, I32, I32, P, P, P, P, P, I64, P]),
    # open-set COCO matching (csrc/osr_os_coco_eval.hip)
    "osr_lvis_match_workspace_bytes": (I64, [I32, I32, I32, I32]),
    "osr_lvis_match": (I32, [P, P, P, P, I32, I32, I32, P, P, P, P, I32, P, P, P, I32, I32, P, I32, P, I32, I32, P, P, P, P, P, I64, P]),
    "osr_os_coco_match_workspace_bytes": (I64, [I32, I32]),
    "osr_os_coco_match": (I32, [P, P, P, P, I32, I32, P, I32, I32, P, P, P, P, P, P, I32, I32, P, I32, P, I32, I32, P, P, P, P, I64, P]),
    # open-set VOC matching (csrc/osr_voc_eval.hip)
    "osr_voc_match": (I32, [P, P, P, P, P, I32, I32, I32, P, I32, P, P, P, I32, I32, C.c_double, P, P, P, P, P, P]),
    # box-proposal recall (csrc/osr_proposal_recall.hip)
    "osr_proposal_recall": (I32, [P, P, P, I32, I32, P, P, P, I32, I32, P, I32, P, I32, P, I32, P, P, P, P]),
    "osr_fastrcnn_candidates": (I32, [P, P, I32, I32, P, P, I32, I32, P, P, F32, P, P, P, P, P, P]),
    "osr_cascade_refine": (I32, [P, P, P, I32, I32, P, P, I32, P, P, P, I32, I32, F32, P, P, P, P, P, P, P]),
    "osr_cascade_candidates": (I32, [P, I32, P, I32, P, P, I32, I32, P, P, F32, P, P, P, P, P, P]),
    "osr_roi_align_fwd": (I32, [C.POINTER(Pyramid), I32, I32, P, P, I64, I32, I32, I32, I32, P, I32, P]),
    "osr_roi_align_fwd_ordered": (I32, [C.POINTER(Pyramid), I32, I32, P, P, I64, I32, I32, I32, I32, P, P, P, I32, P]),
    "osr_roi_align_fwd_ordered_ex": (I32, [C.POINTER(Pyramid), I32, I32, P, P, I64, I32, I32, I32, I32, P, P, I32, P, I32, P]),
    "osr_roi_align_fwd_ordered_opt": (I32, [C.POINTER(Pyramid), I32, I32, P, P, I64, I32, I32, I32, I32, P, P, I32, C.POINTER(RoiOptions), P, I32, P]),
    "osr_roi_align_fwd_strided": (I32, [C.POINTER(Pyramid), I32, I32, P, P, I64, I32, I32, I32, I32, I32, P, P, I32, C.POINTER(RoiOptions), P, I32, P]),
    "osr_avgpool_rows": (I32, [P, I32, I64, I32, I32, P, I32, P, P]),
    "osr_roi_locality_order_workspace_bytes": (I64, [I32, I64]),
    "osr_roi_locality_order": (I32, [C.POINTER(Pyramid), I32, P, P, I64, I32, I32, I32, P, P, P, I64, P]),
    "osr_box_predictor_tail": (I32, [P, I64, I32, P, P, P, P, P, P, C.POINTER(C.c_float), I32, F32, P, P, P, P, P, P]),
    "osr_nms_topk_workspace_bytes": (I64, [I32, I64]),
    "osr_nms_topk": (I32, [P, P, P, P, I32, I64, P, F32, I32, P, P, P, I64, P]),
    "osr_gather_rows": (I32, [P, I64, I32, P, P, I32, I32, P, P]),
    "osr_l2_normalize_rows": (I32, [P, I32, I32, P, P]),
    "osr_pln_tail": (I32, [P, I64, I32, P, I32, I32, F32, I64, P, P, I32, P, P, P]),
    "osr_pln_tail_ex": (I32, [P, I64, I32, P, I32, I32, I32, F32, I64, P, P, I32, P, P, P]),
    "osr_softmax_candidates": (I32, [P, I32, P, P, P, P, I32, I32, I64, F32, F32, P, P, P, P, P, P, P, P, P, P]),
    "osr_assemble_detections": (I32, [P, P, P, P, P, I64, I32, P, P, P, P, I64, I32, I32, I64, P, P, P, P, P, P]),
    "osr_detector_postprocess": (I32, [P, P, P, P, I32, I32, P, P, P, P, P, P, P]),
    "osr_mask_upsample_predict": (I32, [P, I32, I64, I32, I32, I32, P, P, P, P, I32, P, P, I32, P, P]),
    "osr_paste_masks": (I32, [P, P, I64, I32, I32, I32, F32, P, P]),
    # keypoint branch (csrc/osr_keypoint.hip)
    "osr_keypoint_upsample": (I32, [P, I32, I64, I32, I32, I32, P, P, P, I32, P, P]),
    "osr_heatmaps_to_keypoints": (I32, [P, P, I64, I32, I32, P, I32, P, P]),
    # mask branch, training (csrc/osr_mask_train.hip)
    "osr_mask_targets": (I32, [P, I32, I32, I32, I32, P, P, P, P, I32, I32, P, P]),
    "osr_mask_loss_fwd": (I32, [P, P, I64, I32, I32, P, P, I32, F32, P, P, I64, P]),
    "osr_mask_loss_bwd": (I32, [P, P, I64, I32, I32, P, P, I32, F32, P, P, I64, P]),
    "osr_mask_upsample_predict_ex": (I32, [P, I32, I64, I32, I32, I32, P, P, P, P, I32, P, P, I32, P, P, P]),
    "osr_mask_upsample_predict_bwd_workspace_bytes": (I64, [I64, I32, I32]),
    "osr_mask_upsample_predict_bwd": (I32, [P, I32, I64, I32, I32, I32, P, P, P, P, I32, P, P, I32, P, P, I32, P, P, P, P, P, I64, P]),
    "osr_tta_boxes_to_original": (I32, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, P, P, P, P, P]),
    "osr_tta_boxes_to_augmented": (I32, [P, P, P, I32, I32, I32, I32, I32, P, P]),
    "osr_tta_reduce_masks": (I32, [P, P, I32, P, I32, I32, I32, P, P]),
    # training step, forward half
    "osr_rpn_match_anchors": (I32, [P, P, I32, P, P, I32, F32, F32, F32, F32, P, P, P, P, P, I64, P]),
    "osr_subsample_labels": (I32, [P, P, I32, I64, I32, F32, P, P, P]),
    "osr_rpn_anchor_targets": (I32, [P, P, I32, P, P, I32, P, P, P, P, P]),
    "osr_rpn_losses_fwd": (I32, [P, P, I32, P, P, P, P, P, P, F32, F32, I32, P, P, I64, P]),
    "osr_rpn_losses_fwd_ex": (I32, [P, P, I32, P, P, P, P, P, P, F32, F32, I32, P, P, P, I64, P]),
    "osr_roi_match_sample_workspace_bytes": (I64, [I32, I64, I32]),
    "osr_roi_match_and_sample": (I32, [P, P, P, I64, P, P, P, I32, I32, P, I32, I32, F32, F32, P, P, P, P, P, P, P, P, P, I64, P]),
    "osr_roi_match_and_sample_ex": (I32, [P, P, P, I64, P, P, P, I32, I32, P, I32, I32, F32, F32, P, P, P, P, P, P, P, P, P, P, I64, P]),
    "osr_roi_box_losses_fwd": (I32, [P, I32, P, I32, I32, P, P, P, P, I64, I32, P, F32, F32, P, P, I64, P]),
    "osr_roi_box_losses_fwd_ex": (I32, [P, I32, P, I32, I32, P, P, P, P, I64, I32, P, F32, F32, P, P, P, I64, P]),
    "osr_pln_loss_fwd": (I32, [P, I64, I32, P, I32, P, P, F32, F32, F32, F32, P, P, I64, P]),
    "osr_pln_loss_fwd_ex": (I32, [P, I64, I32, P, I32, I32, I32, P, P, F32, F32, F32, F32, P, P, I64, P]),
    "osr_softmax_ce_loss_fwd": (I32, [P, I64, I32, P, I32, F32, P, P, I64, P]),
    # training step, backward half
    "osr_conv2d_wgrad_workspace_bytes": (I64, [P]),
    "osr_conv2d_wgrad": (I32, [P, P, P, P, I32, P, I64, P]),
    "osr_conv2d_dgrad_s2": (I32, [P, P, P, P, P, P, P]),
    "osr_bias_grad": (I32, [P, I32, I64, I32, P, I32, P, I64, P]),
    "osr_rpn_losses_bwd": (I32, [P, P, I32, P, P, P, P, P, P, F32, F32, I32, F32, P, P]),
    "osr_rpn_losses_bwd_ex": (I32, [P, P, I32, P, P, P, P, P, P, F32, F32, I32, F32, P, P, P]),
    "osr_cfrpn_tail_bwd_workspace_bytes": (I64, []),
    "osr_cfrpn_tail_bwd": (I32, [P, I32, I64, P, P, P, P, P, I32, P, I64, P]),
    "osr_rpn_sparse_rows_workspace_bytes": (I64, []),
    "osr_rpn_sparse_rows": (I32, [P, I64, I32, P, P, P, P, I64, P]),
    "osr_rpn_gather_cols": (I32, [P, P, I32, I32, P, I32, P, P, P, P]),
    "osr_rpn_scatter_cols_add": (I32, [P, I32, P, P, P, I32, P]),
    "osr_roi_box_losses_bwd": (I32, [P, P, P, P, P, I64, I32, P, F32, F32, F32, P, P, I64, P]),
    "osr_roi_box_losses_bwd_ex": (I32, [P, P, P, P, P, I64, I32, P, F32, F32, F32, P, P, P, I64, P]),
    "osr_softmax_ce_loss_bwd": (I32, [P, I64, I32, P, I32, F32, F32, P, P, I64, P]),
    # stock heads (csrc/osr_std_train.hip) and the width-generalised sparse RPN backward
    "osr_std_rpn_losses_fwd": (I32, [P, P, I32, P, P, P, P, P, F32, F32, F32, I32, P, P, I64, P]),
    "osr_std_rpn_losses_bwd": (I32, [P, P, I32, P, P, P, P, P, F32, F32, F32, I32, F32, P, P]),
    "osr_fastrcnn_losses_fwd": (I32, [P, P, I32, I32, P, P, P, I64, I32, P, F32, F32, F32, P, P, I64, P]),
    "osr_fastrcnn_losses_bwd": (I32, [P, P, I32, I32, P, P, P, I64, I32, P, F32, F32, F32, F32, P, P, P, I64, P]),
    "osr_std_rpn_tail_bwd_workspace_bytes": (I64, []),
    "osr_std_rpn_tail_bwd": (I32, [P, I64, P, I32, P, P, I32, P, P, P, I64, P]),
    "osr_rpn_sparse_rows_ex": (I32, [P, I64, I32, I32, P, P, P, P, I64, P]),
    "osr_rpn_gather_cols_ex": (I32, [P, P, I32, I32, P, I32, P, I32, P, P, P]),
    "osr_pln_loss_bwd_workspace_bytes": (I64, [I64]),
    "osr_pln_loss_bwd": (I32, [P, I64, I32, P, I32, P, P, F32, F32, F32, F32, F32, P, P, I32, P, I64, P]),
    "osr_pln_loss_bwd_ex": (I32, [P, I64, I32, P, I32, I32, I32, P, P, F32, F32, F32, F32, F32, P, P, I32, P, I64, P]),
    "osr_roi_align_bwd": (I32, [P, I32, P, P, I64, I32, I32, I32, I32, P, I32, P]),
    "osr_roi_align_bwd_dense": (I32, [P, I32, P, P, I64, I32, I32, I32, I32, I32, P, I32, I32, P]),
    "osr_roi_align_bwd_opt": (I32, [P, I32, P, P, I64, I32, I32, I32, I32, P, I32, C.POINTER(RoiOptions), P]),
    "osr_roi_align_bwd_dense_opt": (I32, [P, I32, P, P, I64, I32, I32, I32, I32, I32, P, I32, I32, C.POINTER(RoiOptions), P]),
    "osr_relu_mask": (I32, [P, I32, P, I32, I64, P]),
    "osr_add_cast": (I32, [P, P, P, I32, I64, P]),
    "osr_pool_bwd": (I32, [P, I32, I32, P, P, I32, I32, I32, I32, I32, I32, P]),
    "osr_check_finite": (I32, [P, I64, P, P]),
    "osr_pack_dgrad_weight": (I32, [P, P, I32, I32, I32, I32, I32, P]),
    "osr_pack_dgrad_weight_multi": (I32, [P, P, I32, P]),
    "osr_grad_norm_partials": (I32, [P, P, I32, I32, F32, F32, P, P, P]),
    "osr_sgd_step_multi_ex": (I32, [P, P, I32, I32, F32, F32, F32, I32, F32, F32, P, P, P]),
}

_lib = None


def load() -> C.CDLL:
    """Load libosr_hip.so; raises OsrError when it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OsrError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError => header/library mismatch
        fn.restype = res
        fn.argtypes = args
    ver = lib.osr_abi_version()
    if ver != ABI_VERSION:
        raise OsrError(f"libosr_hip.so ABI version {ver} != binding version {ABI_VERSION}")
    _lib = lib
    return lib


def check(status: int, name: str) -> None:
    if status != 0:
        msg = load().osr_last_error()
        raise OsrError(f"{name} failed (status {status}): {msg.decode() if msg else ''}")
