"""[d2] CascadeROIHeads (Cascade R-CNN, Cai & Vasconcelos 2018; detectron2's Misc/cascade_mask_rcnn_R_50_FPN_*.yaml) on the HIP path:
S box stages, each with a box head and a class-agnostic FastRCNNOutputLayers of its own, each fed the previous stage's decoded boxes.
Everything below the RoI heads -- backbone, FPN, the stock RPN -- and the mask head are StandardRCNNEngine's. A stage is the stock
engine's own chain (osr_roi_align_fwd, FC1 / FC2 on the MFMA kernels, osr_gemm_f32 for cls_score / bbox_pred, osr_fastrcnn_losses_fwd
in training); between two stages sits one osr_cascade_refine launch, behind the last one osr_cascade_candidates (csrc/osr_cascade.hip, csrc/osr_det_tail.hip).
The row lists keep their fixed capacity from stage to stage: a row that stops existing gets batch_idx -1 and class -1, which RoIAlign
and the loss kernels already skip."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .engine_std import StandardRCNNEngine, check_std_supported, std_loss_beta
from .weights import pack_fc1_weight

CASCADE_DEFAULT_CFG = dict(
    cascade_bbox_reg_weights=((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0)), cascade_ious=(0.5, 0.6, 0.7),
)


def check_cascade_options(ious, weights, first_iou=None, cls_agnostic=True) -> int:
    """MODEL.ROI_BOX_CASCADE_HEAD as [d2] CascadeROIHeads._init_box_head asserts it (+ the stage limit of osr_cascade_candidates);
    ValueError naming the key. -> the number of stages."""
    ious, weights = tuple(ious), tuple(weights)
    if len(ious) != len(weights):
        raise ValueError(f"MODEL.ROI_BOX_CASCADE_HEAD.IOUS has {len(ious)} entries, MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS has {len(weights)}: "
                         "one of each per stage")
    if not 1 <= len(ious) <= ops.CASCADE_MAX_STAGES:
        raise ValueError(f"MODEL.ROI_BOX_CASCADE_HEAD.IOUS: {len(ious)} stages; the HIP path runs 1 .. {ops.CASCADE_MAX_STAGES} (OSR_CASCADE_MAX_STAGES)")
    for w in weights:
        ok = isinstance(w, (tuple, list)) and len(w) == 4 and all(isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0 for v in w)
        if not ok:
            raise ValueError(f"MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS: every entry is four positive numbers, got {w!r}")
    if not cls_agnostic:
        raise ValueError("MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False: CascadeROIHeads only supports class-agnostic regression")
    if first_iou is not None and float(ious[0]) != float(first_iou):
        raise ValueError(f"MODEL.ROI_BOX_CASCADE_HEAD.IOUS[0] {ious[0]} != MODEL.ROI_HEADS.IOU_THRESHOLDS[0] {first_iou}: the first stage trains on the "
                         "sampled proposals' labels")
    return len(ious)


class CascadeRCNNEngine(StandardRCNNEngine):
    ROI_LOSSES_NEED_IMAGE_HW = True

    def __init__(self, params: Dict[str, torch.Tensor], cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device: str = "cuda",
                 conv: str = "storage"):
        full = dict(CASCADE_DEFAULT_CFG)
        if cfg:
            full.update(cfg)
        super().__init__(params, full, dtype, device, conv)

    def _init_roi_heads(self, params) -> None:
        dev, c, dtype = self.device, self.cfg, self.dtype
        f32 = lambda k: params[k].float().contiguous().to(dev)  # noqa: E731
        self._init_mask_head(params)
        S = 0
        while f"roi_heads.box_predictor.{S}.cls_score.weight" in params:
            S += 1
        self.has_roi = S > 0
        self.num_stages = S
        if not self.has_roi:
            return
        weights = tuple(tuple(float(v) for v in w) for w in c["cascade_bbox_reg_weights"])
        if check_cascade_options(c["cascade_ious"], weights) != S:
            raise ValueError(f"the parameters carry {S} cascade stages, MODEL.ROI_BOX_CASCADE_HEAD.IOUS {len(c['cascade_ious'])}")
        self.stage_weights, self.stage_ious = weights, tuple(float(v) for v in c["cascade_ious"])
        k = c["std_num_classes"]
        self.fc1_ws, self.fc1_bs, self.fc2_ws, self.fc2_bs, self.cls_ws, self.cls_bs, self.box_ws, self.box_bs = ([] for _ in range(8))
        for s in range(S):
            bh, bp = f"roi_heads.box_head.{s}.", f"roi_heads.box_predictor.{s}."
            self.fc1_ws.append(pack_fc1_weight(params[bh + "fc1.weight"], 256, c["pooler_resolution"], dtype).to(dev))
            self.fc1_bs.append(params[bh + "fc1.bias"].float().to(dev))
            self.fc2_ws.append(params[bh + "fc2.weight"].to(dtype).contiguous().to(dev))
            self.fc2_bs.append(params[bh + "fc2.bias"].float().to(dev))
            self.cls_ws.append(f32(bp + "cls_score.weight")); self.cls_bs.append(f32(bp + "cls_score.bias"))
            self.box_ws.append(f32(bp + "bbox_pred.weight")); self.box_bs.append(f32(bp + "bbox_pred.bias"))
            if self.cls_ws[s].shape[0] != k + 1 or self.box_ws[s].shape[0] != 4:
                raise ValueError(f"cascade stage {s}: cls_score needs NUM_CLASSES + 1 rows and bbox_pred 4 (MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG True)")

    def _box_stage_params(self, s: int):
        return (f"roi_heads.box_head.{s}", self.fc1_ws[s], self.fc1_bs[s], self.fc2_ws[s], self.fc2_bs[s], self.cls_ws[s], self.cls_bs[s],
                self.box_ws[s], self.box_bs[s])

    # ---- [d2] CascadeROIHeads._forward_box (inference) --------------------------------------------------------------------------
    def _roi_heads(self, feats, sel, image_hw, keep=None, mask: bool = True):
        c, S = self.cfg, self.num_stages
        n = sel["boxes"].shape[0]
        boxes, bidx = sel["boxes"].view(-1, 4), sel["batch_idx"]
        all_logits = []
        for s in range(S):
            if s > 0:  # the previous stage's boxes, decoded and clipped; every row stays, so the stages' scores stay aligned
                ref = ops.cascade_refine(boxes, bidx, deltas, n, image_hw, self.stage_weights[s - 1])
                boxes, bidx = ref["boxes"], ref["batch_idx"]
            pooled, h1, box_feats, logits, deltas = self._box_stage(feats, boxes, bidx, s)
            all_logits.append(logits)
            if keep is not None:
                keep.update({f"pooled_s{s}": pooled, f"logits_s{s}": logits, f"deltas_s{s}": deltas, f"boxes_s{s}": boxes, f"box_feats_s{s}": box_feats})
        cands = ops.cascade_candidates(all_logits, deltas, boxes.view(n, -1, 4), bidx, image_hw, c["std_num_classes"], self.stage_weights[S - 1],
                                       c["score_thresh_test"])
        return self._detections(feats, cands, n, keep, mask)

    # ---- [d2] CascadeROIHeads._forward_box (training) ---------------------------------------------------------------------------
    def roi_losses_forward(self, feats: Dict[str, torch.Tensor], prop_boxes, prop_scores, prop_counts, gt_boxes, gt_classes, gt_count,
                           keys_roi: torch.Tensor, gt_masks: Optional[torch.Tensor] = None, image_hw: Optional[torch.Tensor] = None):
        """Stage 0 trains on label_and_sample_proposals' rows; stage s > 0 on the previous stage's decoded boxes (detached, clipped,
        empty ones dropped), re-labelled against the ground truth at IOUS[s] (osr_cascade_refine). Returns (dict: loss_cls_stage{s},
        loss_box_reg_stage{s}, roi_counts (n,3) of stage 0, stage_counts / stage_stats per stage (+ loss_mask, mask_stats); state with
        `stages`, a list of what each stage's backward reads). The mask branch reads stage 0's sampled rows, as [d2] does."""
        c, S = self.cfg, self.num_stages
        check_std_supported(c)
        if image_hw is None:
            raise ValueError("CascadeROIHeads: roi_losses_forward needs image_hw (the boxes handed from stage to stage are clipped to the image)")
        if self.has_mask and gt_masks is None:
            raise ValueError("MODEL.MASK_ON: training the mask branch needs gt_masks (INPUT.MASK_FORMAT \"bitmask\" ground truth)")
        k = c["std_num_classes"]
        n = prop_boxes.shape[0]
        smp = ops.roi_match_and_sample(prop_boxes, prop_scores, prop_counts, gt_boxes, gt_classes, gt_count, keys_roi,
                                       k, c["roi_batch_size"], c["roi_positive_fraction"], self.stage_ious[0])
        boxes, bidx = smp["boxes"].view(-1, 4), smp["batch_idx"]
        cls, gtb, counts = smp["gt_classes"].view(-1), smp["gt_boxes"].view(-1, 4), smp["counts"]
        out, stages = dict(roi_counts=smp["counts"], stage_counts=[], stage_stats=[]), []
        for s in range(S):
            if s > 0:
                ref = ops.cascade_refine(boxes, bidx, deltas, n, image_hw, self.stage_weights[s - 1], True, gt_boxes, gt_classes, gt_count, k,
                                         self.stage_ious[s])
                boxes, bidx, cls, gtb, counts = ref["boxes"], ref["batch_idx"], ref["gt_classes"], ref["gt_boxes"], ref["counts"]
            pooled, h1, box_feats, logits, deltas = self._box_stage(feats, boxes, bidx, s)
            st = ops.fastrcnn_losses_fwd(logits, deltas, boxes, gtb, cls, k, True, self.stage_weights[s], std_loss_beta(c, "roi_box"),
                                         c["std_cls_loss_weight"], c["box_reg_weight"])
            out[f"loss_cls_stage{s}"], out[f"loss_box_reg_stage{s}"] = st[0], st[1]
            out["stage_counts"].append(counts)
            out["stage_stats"].append(st)
            stages.append(dict(boxes=boxes, batch_idx=bidx, cls=cls, gt_boxes=gtb, pooled=pooled, h1=h1, box_feats=box_feats, logits=logits,
                               deltas=deltas))
        state = dict(smp=smp, stages=stages)
        if self.has_mask:
            mst, state["mask"] = self.mask_losses_forward(feats, smp, gt_masks, image_hw)
            out.update(loss_mask=mst[0], mask_stats=mst)
        return out, state
