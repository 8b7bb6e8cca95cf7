"""BASELINE config 1 on the HIP path: the stock detectron2 Faster R-CNN that /root/reference/configs/Base-RCNN-FPN.yaml describes
on its own -- PROPOSAL_GENERATOR "RPN" with "StandardRPNHead" (three aspect ratios per cell, objectness logits, Box2BoxTransform
deltas, per-level NMS at 0.7, post-NMS top-k) and ROI_HEADS "StandardROIHeads" with FastRCNNOutputLayers (softmax over 80 + 1
classes, class-specific box deltas, per-class NMS at 0.5, 100 detections per image). None of that code lives in /root/reference
(it is detectron2's); the reference only selects it by name (Base-RCNN-FPN.yaml:2-33), and SURVEY.md 8b lists the names as part of
the drop-in surface. Same kernels as the open-set path: the MFMA convolutions, osr_gemm_f32 for the small output layers,
osr_rpn_select_ex (decode mode 1), osr_nms_topk, osr_roi_align_fwd, plus osr_fastrcnn_candidates."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops
from .engine import PYRAMID, RPN_CONV, OpensetRCNNEngine, loss_types_of
from .weights import pack_deconv_weight, pack_fc1_weight, pack_keypoint_deconv_weight

STD_DEFAULT_CFG = dict(
    anchor_ratios=(0.5, 1.0, 2.0), post_nms_topk_test=1000, rpn_nms_thresh=0.7, rpn_bbox_reg_weights=(1.0, 1.0, 1.0, 1.0),
    std_num_classes=80, score_thresh_test=0.05, std_nms_thresh_test=0.5, std_detections_per_image=100, cls_agnostic_bbox_reg=False,
    # training ([d2] defaults; Base-RCNN-FPN.yaml:17-18 sets the two top-k values)
    post_nms_topk_train=1000, rpn_cls_weight=1.0, std_cls_loss_weight=1.0,
    loss_types=dict(rpn_box=("smooth_l1", 0.0), roi_box=("smooth_l1", 0.0)),
    # the mask branch (MODEL.MASK_ON; ROI_MASK_HEAD of Base-RCNN-FPN.yaml:29-33): built when the parameters carry a mask head
    mask_pooler_resolution=14, mask_pooler_aligned=True, mask_pooler_sampling_ratio=0,
    # the keypoint branch (MODEL.KEYPOINT_ON; ROI_KEYPOINT_HEAD): built when the parameters carry a keypoint head
    keypoint_pooler_resolution=14, keypoint_pooler_aligned=True, keypoint_pooler_sampling_ratio=0,
)


def cell_anchor_table(sizes, ratios) -> torch.Tensor:
    """[d2] DefaultAnchorGenerator.generate_cell_anchors per level: for (size, ratio): area = size^2, w = sqrt(area / ratio),
    h = ratio * w, anchor [-w/2, -h/2, w/2, h/2], computed in double and rounded to fp32 as torch.tensor() does. (L, A, 4).
    A level's entry of `sizes` is one size or a list of sizes (RetinaNet: three per level): size-major, then ratio, [d2]'s order."""
    rows = []
    for level in sizes:
        cells = []
        for z in (level if isinstance(level, (list, tuple)) else (level,)):
            for r in ratios:
                w = math.sqrt(float(z) ** 2 / r)
                h = r * w
                cells.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
        rows.append(cells)
    return torch.tensor(rows, dtype=torch.float32)


class StandardRCNNEngine(OpensetRCNNEngine):
    has_keypoint = False  # (set by _init_keypoint_head; an engine whose RoI heads are built elsewhere has no keypoint head)

    def __init__(self, params: Dict[str, torch.Tensor], cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device: str = "cuda",
                 conv: str = "storage"):
        if conv != "storage":
            raise ValueError(f"conv {conv!r}: the stock Faster R-CNN engine multiplies in its storage dtype (conv=\"storage\")")
        full = dict(STD_DEFAULT_CFG)
        if cfg:
            full.update(cfg)
        super().__init__(params, full, dtype, device)

    def _init_rpn(self, params) -> None:
        dev, c = self.device, self.cfg
        f32 = lambda k: params[k].float().contiguous().to(dev)  # noqa: E731
        self.has_rpn = "proposal_generator.rpn_head.objectness_logits.weight" in params
        if not self.has_rpn:
            return
        self.num_anchors = len(c["anchor_ratios"])
        self.rpn_wo = f32("proposal_generator.rpn_head.objectness_logits.weight").view(self.num_anchors, -1)
        self.rpn_bo = f32("proposal_generator.rpn_head.objectness_logits.bias")
        self.rpn_wd = f32("proposal_generator.rpn_head.anchor_deltas.weight").view(self.num_anchors * 4, -1)
        self.rpn_bd = f32("proposal_generator.rpn_head.anchor_deltas.bias")
        self.cell_anchors = cell_anchor_table(c["anchor_sizes"], c["anchor_ratios"]).to(dev)
        self.fuse_rpn_head = False

    def _init_roi_heads(self, params) -> None:
        dev, c, dtype = self.device, self.cfg, self.dtype
        f32 = lambda k: params[k].float().contiguous().to(dev)  # noqa: E731
        self.has_roi = "roi_heads.box_predictor.cls_score.weight" in params
        self._init_mask_head(params)
        self._init_keypoint_head(params)
        if not self.has_roi:
            return
        self.fc1_w = pack_fc1_weight(params["roi_heads.box_head.fc1.weight"], 256, c["pooler_resolution"], dtype).to(dev)
        self.fc1_b = params["roi_heads.box_head.fc1.bias"].float().to(dev)
        self.fc2_w = params["roi_heads.box_head.fc2.weight"].to(dtype).contiguous().to(dev)
        self.fc2_b = params["roi_heads.box_head.fc2.bias"].float().to(dev)
        self.cls_w, self.cls_b = f32("roi_heads.box_predictor.cls_score.weight"), f32("roi_heads.box_predictor.cls_score.bias")
        self.box_w, self.box_b = f32("roi_heads.box_predictor.bbox_pred.weight"), f32("roi_heads.box_predictor.bbox_pred.bias")
        k = c["std_num_classes"]
        assert self.cls_w.shape[0] == k + 1 and self.box_w.shape[0] in (4, 4 * k), "cls_score: K+1 rows; bbox_pred: 4 or 4K rows"

    def _init_mask_head(self, params) -> None:
        """[d2] MaskRCNNConvUpsampleHead: mask_fcn1..N (3x3, packed with the other convolutions by _pack_convs), deconv in the fused
        kernel's fragment order, the 1x1 predictor as an fp32 (rows, CONV_DIM) matrix -- one row when CLS_AGNOSTIC_MASK."""
        dev, c = self.device, self.cfg
        pre = "roi_heads.mask_head."
        self.has_mask = pre + "deconv.weight" in params
        if not self.has_mask:
            return
        ops.check_pooler_options(c["mask_pooler_aligned"], c["mask_pooler_sampling_ratio"])
        self.mask_num_conv = 0
        while f"{pre}mask_fcn{self.mask_num_conv + 1}.weight" in params:
            self.mask_num_conv += 1
        self.mask_deconv_w = pack_deconv_weight(params[pre + "deconv.weight"], self.dtype).to(dev)
        self.mask_deconv_b = params[pre + "deconv.bias"].float().contiguous().to(dev)
        pw = params[pre + "predictor.weight"].float()
        self.mask_pred_w = pw.reshape(pw.shape[0], -1).contiguous().to(dev)
        self.mask_pred_b = params[pre + "predictor.bias"].float().contiguous().to(dev)
        assert self.mask_pred_w.shape[0] in (1, c["std_num_classes"]), "mask predictor: 1 (CLS_AGNOSTIC_MASK) or NUM_CLASSES rows"

    # ---- [d2] StandardROIHeads._forward_mask + mask_rcnn_inference (inference) ---------------------------------------------------
    def _mask_head(self, feats, boxes, classes, counts):
        """boxes (n, topk, 4) fp32, classes (n, topk) int64, counts (n,) int32: the padded detection lists (or any boxes: the head is
        callable on its own). -> probs (n, topk, 2P, 2P) fp32, the sigmoid of each detection's class row (row 0 when class-agnostic);
        the rows beyond an image's count, and rows with class -1, are zeros. No host sync: the capacities are fixed."""
        c = self.cfg
        if not self.has_mask:
            raise ops.OsrError("this engine was built without a mask head (MODEL.MASK_ON False)")
        n, topk = boxes.shape[0], boxes.shape[1]
        res = c["mask_pooler_resolution"]
        x = self.pool_mask_rois(feats, boxes.reshape(-1, 4).contiguous(), ops.padded_batch_idx(counts, topk))
        for i in range(self.mask_num_conv):
            x = self._conv(x, f"roi_heads.mask_head.mask_fcn{i + 1}", 1, 1, relu=True)
        probs = ops.mask_upsample_predict(x, self.mask_deconv_w, self.mask_deconv_b, self.mask_pred_w, self.mask_pred_b,
                                          classes.reshape(-1).contiguous(), counts, topk)
        return probs.view(n, topk, 2 * res, 2 * res)

    def pool_mask_rois(self, feats, boxes, batch_idx):
        """pool_rois with the mask pooler's three options (ROI_MASK_HEAD.POOLER_*) -> (m, R, R, 256)."""
        c = self.cfg
        return ops.roi_align([feats[k] for k in PYRAMID[:4]], c["pooler_scales"], boxes, batch_idx, c["mask_pooler_resolution"], self.dtype,
                             c["canonical_level"], c["canonical_size"], 2, aligned=c["mask_pooler_aligned"],
                             sampling_ratio=c["mask_pooler_sampling_ratio"])

    def _init_keypoint_head(self, params) -> None:
        """[d2] KRCNNConvDeconvUpsampleHead: conv_fcn1..N (3x3, packed with the other convolutions by _pack_convs) and score_lowres in
        the fused tail's fragment order (weights.pack_keypoint_deconv_weight)."""
        dev, c = self.device, self.cfg
        pre = "roi_heads.keypoint_head."
        self.has_keypoint = pre + "score_lowres.weight" in params
        if not self.has_keypoint:
            return
        ops.check_pooler_options(c["keypoint_pooler_aligned"], c["keypoint_pooler_sampling_ratio"])
        self.keypoint_num_conv = 0
        while f"{pre}conv_fcn{self.keypoint_num_conv + 1}.weight" in params:
            self.keypoint_num_conv += 1
        self.keypoint_deconv_w = pack_keypoint_deconv_weight(params[pre + "score_lowres.weight"], self.dtype).to(dev)
        self.keypoint_deconv_b = params[pre + "score_lowres.bias"].float().contiguous().to(dev)

    # ---- [d2] StandardROIHeads._forward_keypoint + keypoint_rcnn_inference (inference) ---------------------------------------------
    def _keypoint_head(self, feats, boxes, counts):
        """boxes (n, topk, 4) fp32, counts (n,) int32: the padded detection lists (or any boxes: the head is callable on its own).
        -> (keypoints (n, topk, K, 3) fp32 {x, y, score} in the boxes' coordinates, heatmaps (n, topk, K, 4P, 4P) fp32); the rows
        beyond an image's count are zeros. The conv_fcn layers skip the tiles of those rows. No host sync: the capacities are fixed."""
        c = self.cfg
        if not self.has_keypoint:
            raise ops.OsrError("this engine was built without a keypoint head (MODEL.KEYPOINT_ON False)")
        n, topk = boxes.shape[0], boxes.shape[1]
        res = c["keypoint_pooler_resolution"]
        flat = boxes.reshape(-1, 4).contiguous()
        x = self.pool_keypoint_rois(feats, flat, ops.padded_batch_idx(counts, topk))
        seg = (counts * (res * res), topk * res * res)  # (an image's detections are a prefix of its topk * P * P pixel rows)
        for i in range(self.keypoint_num_conv):
            x = self._conv(x, f"roi_heads.keypoint_head.conv_fcn{i + 1}", 1, 1, relu=True, row_seg=seg)
        heat = ops.keypoint_upsample(x, self.keypoint_deconv_w, self.keypoint_deconv_b, counts, topk)
        kp = ops.heatmaps_to_keypoints(heat, flat, counts, topk)
        k = heat.shape[1]
        kp = kp.view(n, topk, k, 4)
        return torch.cat((kp[..., :2], kp[..., 3:]), dim=-1), heat.view(n, topk, k, 4 * res, 4 * res)

    def pool_keypoint_rois(self, feats, boxes, batch_idx):
        """pool_rois with the keypoint pooler's three options (ROI_KEYPOINT_HEAD.POOLER_*) -> (m, R, R, 256)."""
        c = self.cfg
        return ops.roi_align([feats[k] for k in PYRAMID[:4]], c["pooler_scales"], boxes, batch_idx, c["keypoint_pooler_resolution"], self.dtype,
                             c["canonical_level"], c["canonical_size"], 2, aligned=c["keypoint_pooler_aligned"],
                             sampling_ratio=c["keypoint_pooler_sampling_ratio"])

    def _levels(self, shapes, n):
        key = (tuple(shapes), n)
        if key not in self._lv_cache:
            self._lv_cache[key] = ops.make_rpn_levels(shapes, self.cfg["fpn_strides"], n, self.num_anchors)
        return self._lv_cache[key]

    # ---- [d2] RPN.forward (inference) -------------------------------------------------------------------------------------------
    def _rpn(self, feats, image_hw, keep=None, topk=None, post_topk=None):
        c = self.cfg
        fl = [feats[k] for k in PYRAMID]
        n = fl[0].shape[0]
        shapes = [(f.shape[1], f.shape[2]) for f in fl]
        rows = [n * h * w for h, w in shapes]
        a = self.num_anchors
        # StandardRPNHead: 3x3 conv + ReLU on the MFMA kernel with an fp32 hidden state, then the two 1x1 convs as exact-fp32 GEMMs.
        # With NHWC rows the (N,A,H,W)->(N,H*W*A) / (N,A*4,H,W)->(N,H*W*A,4) flattening of [d2] RPN.forward is a no-op: row-major
        # (pixel, anchor) is exactly the memory order of the (rows, A) and (rows, A*4) GEMM outputs.
        t_all = torch.empty((sum(rows), 256), dtype=torch.float32, device=self.device)
        off = 0
        for f, r in zip(fl, rows):
            self._conv(f, RPN_CONV, 1, 1, relu=True, out=t_all[off:off + r], out_dtype=torch.float32)
            off += r
        logits = ops.gemm_f32(t_all, self.rpn_wo, self.rpn_bo).view(-1)
        deltas = ops.gemm_f32(t_all, self.rpn_wd, self.rpn_bd).view(-1, 4)
        # level offsets of make_rpn_levels count anchors (pixels * A): the GEMM outputs above are laid out exactly so
        k = c["pre_nms_topk_test"] if topk is None else topk
        sel = ops.rpn_select(self._levels(shapes, n), self.cell_anchors, logits, deltas, n, image_hw, k, c["min_box_size"],
                             b2b_weights=c["rpn_bbox_reg_weights"])
        # [d2] find_top_rpn_proposals: batched NMS with the level as category, then the first POST_NMS_TOPK of the keep list
        post = c["post_nms_topk_test"] if post_topk is None else post_topk
        pk, pcnt = ops.nms_topk(sel["boxes"], sel["scores"], sel["level"], None, n, sel["cap"], sel["counts"], c["rpn_nms_thresh"], post)
        boxes = ops.gather_rows(sel["boxes"].view(-1, 4), sel["cap"], pk, pcnt)
        scores = ops.gather_rows(sel["scores"].view(-1), sel["cap"], pk, pcnt).view(n, post)
        out = dict(boxes=boxes, scores=scores, counts=pcnt, batch_idx=ops.padded_batch_idx(pcnt, post), cap=post, pre=sel, keep_idx=pk,
                   status_flags=sel["status_flags"], levels=self._levels(shapes, n), pred_logits=logits, pred_deltas=deltas)
        if keep is not None:
            keep.update(rpn_t=t_all, rpn_logits=logits, rpn_deltas=deltas, rpn_shapes=shapes, rpn_pre=sel, rpn_keep=pk)
        return out

    # ---- [d2] StandardROIHeads._forward_box (inference) -----------------------------------------------------------------------
    def forward_device(self, images, image_hw, hp, wp, keep=None, mask: bool = True):
        """mask=False: the pass without the per-detection branches behind the boxes (the mask head and the keypoint head) -- the four
        box outputs, whichever heads the engine has ([d2] GeneralizedRCNNWithTTA._turn_off_roi_heads: the box stage of test-time
        augmentation). The engine's state is not touched. What follows the four box outputs otherwise: output_fields()."""
        if mask:
            return super().forward_device(images, image_hw, hp, wp, keep)
        feats = self._backbone(images, hp, wp, keep)
        sel = self._rpn(feats, image_hw, keep)
        if keep is not None:
            keep.update(feats=feats, sel=sel)
        return self._roi_heads(feats, sel, image_hw, keep, mask=False)

    def output_fields(self, mask: bool = True):
        """The names of the tensors forward_device returns behind (boxes, scores, classes, counts), in order -- what to_instances
        takes as `fields`. mask: forward_device's flag."""
        names = ()
        if self.has_mask and mask:
            names += ("pred_masks",)
        if self.has_keypoint and mask:
            names += ("pred_keypoints", "pred_keypoint_heatmaps")
        return names

    def _box_stage_params(self, s: int):
        """Box stage s: (its box head's parameter prefix, fc1_w, fc1_b, fc2_w, fc2_b, cls_w, cls_b, box_w, box_b). StandardROIHeads has one."""
        return "roi_heads.box_head", self.fc1_w, self.fc1_b, self.fc2_w, self.fc2_b, self.cls_w, self.cls_b, self.box_w, self.box_b

    def _box_stage(self, feats, boxes, batch_idx, s: int = 0):
        """A box stage on its rows: RoIAlign, FC1, FC2, cls_score, bbox_pred. -> (pooled (m, P, P, 256), h1, box_feats, logits, deltas)."""
        head, fc1_w, fc1_b, fc2_w, fc2_b, cls_w, cls_b, box_w, box_b = self._box_stage_params(s)
        pooled = self.pool_rois(feats, boxes, batch_idx)
        h1 = self._linear(pooled, fc1_w, fc1_b, True, name=head + ".fc1")
        box_feats = self._linear(h1, fc2_w, fc2_b, True, torch.float32, name=head + ".fc2")
        return self.pooled_bin_major(pooled), h1, box_feats, ops.gemm_f32(box_feats, cls_w, cls_b), ops.gemm_f32(box_feats, box_w, box_b)

    def _roi_heads(self, feats, sel, image_hw, keep=None, mask: bool = True):
        c = self.cfg
        pooled, h1, box_feats, logits, deltas = self._box_stage(feats, sel["boxes"].view(-1, 4), sel["batch_idx"])
        cands = ops.fastrcnn_candidates(logits, deltas, sel["boxes"], sel["counts"], image_hw, c["std_num_classes"], c["bbox_reg_weights"],
                                        c["score_thresh_test"])
        if keep is not None:
            keep.update(pooled=pooled, h1=h1, box_feats=box_feats, logits=logits, deltas=deltas)
        return self._detections(feats, cands, sel["boxes"].shape[0], keep, mask)

    def _detections(self, feats, cands, n, keep=None, mask: bool = True):
        """[d2] fast_rcnn_inference behind the candidates: per-class NMS, the best DETECTIONS_PER_IMAGE, then the mask head and the
        keypoint head on them (mask=False: neither). The outputs behind the first four are named by output_fields(mask)."""
        c = self.cfg
        ob, osc, ocl, dcnt, dk = ops.nms_gather(cands["boxes"], cands["scores"], cands["cls"], None, n, cands["cap"], cands["count"],
                                                c["std_nms_thresh_test"], c["std_detections_per_image"])
        if keep is not None:
            keep.update(cands=cands, det_keep=dk, det_count=dcnt)
        out = (ob, osc, ocl, dcnt)
        if self.has_mask and mask:  # (a fifth output only when the engine has a mask head: MASK_ON False returns what it always has)
            out += (self._mask_head(feats, ob, ocl, dcnt),)
        if self.has_keypoint and mask:  # (two more, last, only with a keypoint head: output_fields names them)
            out += self._keypoint_head(feats, ob, dcnt)
        return out

    # ---- [d2] RPN.label_and_sample_anchors + RPN.losses (training) ---------------------------------------------------------------
    def rpn_targets_forward(self, lv, n: int, gt_boxes: torch.Tensor, gt_count: torch.Tensor, keys: Dict[str, torch.Tensor],
                            keep: Optional[dict] = None) -> dict:
        """Matcher(RPN.IOU_THRESHOLDS, [0, -1, 1], allow_low_quality_matches) -- one label set: the objectness thresholds of the shared
        kernel are set to the regression ones and its second output is dropped --, subsample_labels(BATCH_SIZE_PER_IMAGE,
        POSITIVE_FRACTION) with the keys 'rpn_reg', and the matched GT box of every anchor. A function of the ground truth only."""
        c = self.cfg
        thr = c["rpn_iou_thresholds"]
        midx, miou, lab, _ = ops.rpn_match_anchors(lv, self.cell_anchors, n, gt_boxes, gt_count, thr, thr)
        if keep is not None:
            keep.update(matched_idx=midx, matched_iou=miou, labels_pre=lab.clone())
        ops.subsample_labels_(lab, keys["rpn_reg"], c["rpn_batch_size"], c["rpn_positive_fraction"])
        mboxes, _ = ops.rpn_anchor_targets(lv, self.cell_anchors, n, gt_boxes, gt_count, midx, lab)
        return dict(labels=lab, matched_boxes=mboxes)

    def rpn_losses_forward(self, sel: dict, n: int, gt_boxes: torch.Tensor, gt_count: torch.Tensor, keys: Dict[str, torch.Tensor],
                           keep: Optional[dict] = None, targets: Optional[dict] = None):
        """-> (4 floats: loss_rpn_cls, loss_rpn_loc, num_pos, num_neg; the targets the backward reads)."""
        c = self.cfg
        check_std_supported(c)
        tg = targets if targets is not None else self.rpn_targets_forward(sel["levels"], n, gt_boxes, gt_count, keys, keep)
        rpn = ops.std_rpn_losses_fwd(sel["levels"], self.cell_anchors, n, sel["pred_logits"], sel["pred_deltas"], tg["labels"], tg["matched_boxes"],
                                     c["rpn_bbox_reg_weights"], std_loss_beta(c, "rpn_box"), c["rpn_cls_weight"], c["rpn_loc_weight"], c["rpn_batch_size"])
        return rpn, dict(tg)

    # ---- [d2] StandardROIHeads.label_and_sample_proposals + FastRCNNOutputLayers.losses (training) ---------------------------------
    def mask_losses_forward(self, feats: Dict[str, torch.Tensor], smp: dict, gt_masks: torch.Tensor, image_hw: Optional[torch.Tensor]):
        """[d2] StandardROIHeads._forward_mask in training + mask_rcnn_loss on the foreground rows of the sampled proposals
        (select_foreground_proposals). osr_roi_match_and_sample writes an image's foreground rows first, so the mask rows are the
        prefix of F = int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION) rows per image with the foreground count as rows_valid: fixed
        capacities, no host sync, no compaction. gt_masks (n, gmax, Hm, Wm) uint8 planes padded to the batch's image size.
        -> ((6,) {loss_mask, foreground rows, incorrect, positive, false positive, false negative}, what the backward reads)."""
        c = self.cfg
        n, bs = smp["boxes"].shape[0], smp["boxes"].shape[1]
        f = max(int(c["roi_batch_size"] * c["roi_positive_fraction"]), 1)
        f = min(f, bs)
        res = c["mask_pooler_resolution"]
        if gt_masks.dim() != 4 or gt_masks.shape[0] != n or gt_masks.dtype != torch.uint8:
            raise ValueError(f"gt_masks must be (n, gmax, H, W) uint8 planes, got {tuple(gt_masks.shape)} {gt_masks.dtype}")
        boxes = smp["boxes"][:, :f].contiguous()
        cls = smp["gt_classes"][:, :f].reshape(-1).contiguous()
        gidx = smp["gt_idx"][:, :f].contiguous()
        rows_valid = smp["counts"][:, 1].contiguous()
        bidx = ops.padded_batch_idx(rows_valid, f)
        pooled = self.pool_mask_rois(feats, boxes.view(-1, 4), bidx)
        acts, x = [], pooled
        for i in range(self.mask_num_conv):
            x = self._conv(x, f"roi_heads.mask_head.mask_fcn{i + 1}", 1, 1, relu=True)
            acts.append(x)
        k = self.mask_pred_w.shape[0]
        logits = ops.mask_upsample_logits(x, self.mask_deconv_w, self.mask_deconv_b, self.mask_pred_w, self.mask_pred_b, cls, rows_valid, f)
        targets = ops.mask_targets(gt_masks, boxes, gidx, rows_valid, 2 * res, image_hw)
        st = ops.mask_loss_fwd(logits, targets, k, cls, rows_valid, f)
        return st, dict(boxes=boxes.view(-1, 4), batch_idx=bidx, cls=cls, gt_idx=gidx, rows_valid=rows_valid, seg_rows=f, pooled=pooled, acts=acts,
                        logits=logits, targets=targets)

    def roi_losses_forward(self, feats: Dict[str, torch.Tensor], prop_boxes, prop_scores, prop_counts, gt_boxes, gt_classes, gt_count,
                           keys_roi: torch.Tensor, gt_masks: Optional[torch.Tensor] = None, image_hw: Optional[torch.Tensor] = None):
        """Proposals (detached) + GT appended, Matcher([IOU_THRESHOLDS[0]], [0, 1]), background = NUM_CLASSES, BATCH_SIZE_PER_IMAGE /
        POSITIVE_FRACTION sampling, box head, cls_score / bbox_pred, the two losses. Returns (dict: loss_cls, loss_box_reg,
        roi_counts (n,3), stats (7); state dict with what the backward reads). An engine with a mask head also runs the mask branch
        (mask_losses_forward; gt_masks is then required): loss_mask, mask_stats (6) and state["mask"]."""
        c = self.cfg
        check_std_supported(c)
        if self.has_keypoint:
            raise NotImplementedError(KEYPOINT_LOSS_MESSAGE)
        if self.has_mask and gt_masks is None:
            raise ValueError("MODEL.MASK_ON: training the mask branch needs gt_masks (INPUT.MASK_FORMAT \"bitmask\" ground truth)")
        k = c["std_num_classes"]
        smp = ops.roi_match_and_sample(prop_boxes, prop_scores, prop_counts, gt_boxes, gt_classes, gt_count, keys_roi,
                                       k, c["roi_batch_size"], c["roi_positive_fraction"], c["roi_iou_threshold"])
        boxes = smp["boxes"].view(-1, 4)
        pooled, h1, box_feats, logits, deltas = self._box_stage(feats, boxes, smp["batch_idx"])
        cls = smp["gt_classes"].view(-1)
        st = ops.fastrcnn_losses_fwd(logits, deltas, boxes, smp["gt_boxes"].view(-1, 4), cls, k, self.box_w.shape[0] == 4, c["bbox_reg_weights"],
                                     std_loss_beta(c, "roi_box"), c["std_cls_loss_weight"], c["box_reg_weight"])
        state = dict(smp=smp, boxes=boxes, pooled=pooled, h1=h1, box_feats=box_feats, logits=logits, deltas=deltas, cls=cls)
        out = dict(loss_cls=st[0], loss_box_reg=st[1], roi_counts=smp["counts"], stats=st)
        if self.has_mask:
            mst, state["mask"] = self.mask_losses_forward(feats, smp, gt_masks, image_hw)
            out.update(loss_mask=mst[0], mask_stats=mst)
        return out, state


KEYPOINT_LOSS_MESSAGE = ("MODEL.KEYPOINT_ON: the keypoint loss (keypoint_rcnn_loss) is not built on the HIP path -- the keypoint branch runs at "
                         "inference only; train the box (and mask) branches with MODEL.KEYPOINT_ON False")


def std_loss_beta(cfg: dict, key: str) -> float:
    return float(loss_types_of(cfg)[key][1])


def check_std_supported(cfg: dict) -> None:
    """The stock heads train with BBOX_REG_LOSS_TYPE "smooth_l1" (the [d2] default Base-RCNN-FPN.yaml keeps) for the RPN and the box
    head; giou / diou / ciou are refused here, at model build time (modeling.RPN / StandardROIHeads call this), not at the first
    iteration."""
    lt = loss_types_of(cfg)
    for key, name in (("rpn_box", "MODEL.RPN.BBOX_REG_LOSS_TYPE"), ("roi_box", "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE")):
        if lt[key][0] != "smooth_l1":
            raise NotImplementedError(f"{name} '{lt[key][0]}': the stock RPN / StandardROIHeads train with \"smooth_l1\" only on the HIP path")
        if lt[key][1] < 0.0:
            raise ValueError(f"{name}: negative SMOOTH_L1_BETA")
