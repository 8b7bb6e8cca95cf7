"""Faster R-CNN R50-C4 on the HIP path: [d2] Base-RCNN-C4.yaml -- BACKBONE "build_resnet_backbone" (stem, res2..res4: one feature map at
stride 16, no FPN), PROPOSAL_GENERATOR "RPN" on that one level (5 sizes x 3 ratios = 15 anchors per cell, 6000 proposals into the NMS,
1000 out of it) and ROI_HEADS "Res5ROIHeads": a 14 x 14 RoIAlign on res4, the three bottlenecks of res5 run per RoI, their spatial mean,
and FastRCNNOutputLayers on the 2048 means. Inference only.

The trunk, the bottlenecks, the RPN tail, the candidates and both NMS passes are the stock engine's. What is this engine's own:
  - the RPN keeps more proposals per level than osr_rpn_select serves: ops.rpn_select_wide above 2048;
  - with STRIDE_IN_1X1 (the MSRA weights of every C4 zoo model) res5.0 enters through two 1 x 1 convolutions of stride 2, which read the
    even bins of the pooled grid and nothing else: ops.roi_align(bin_stride=2) pools those bins only, and res5.0 runs with both layers at
    stride 1 on the 7 x 7 result -- the same arithmetic on a quarter of the samples and a quarter of the pooled bytes;
  - ops.avgpool_rows for the mean.
The engine takes [d2]'s C4 parameter names (backbone.stem.*, backbone.res{2,3,4}.*: no `bottom_up`; roi_heads.res5.{0,1,2}.*)."""
from __future__ import annotations

import re
from typing import Dict, Optional

import torch

from . import ops
from .engine import BOTTOM_UP, RPN_CONV
from .engine_std import StandardRCNNEngine, cell_anchor_table

C4_FEATURE = "res4"
C4_STRIDE = 16
RES5 = "roi_heads.res5"
C4_DEFAULT_CFG = dict(
    anchor_sizes=((32, 64, 128, 256, 512),), pre_nms_topk_test=6000, post_nms_topk_test=1000,
    pooler_resolution=14, pooler_scales=(1.0 / C4_STRIDE,),
)
TRAINING_MESSAGE = ('MODEL.ROI_HEADS.NAME "Res5ROIHeads" runs at inference only on the HIP path: the backward of res5 on pooled RoIs and of '
                    'the strided pooler have no kernels yet. Train an FPN model (StandardROIHeads / CascadeROIHeads), or evaluate C4 weights')


def trunk_names(params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """[d2]'s C4 backbone names (backbone.stem.*, backbone.res{2,3,4}.*) -> the names the shared trunk walk reads
    (backbone.bottom_up.*). Everything else, roi_heads.res5.* included, keeps its name."""
    out = {}
    for k, v in params.items():
        m = re.match(r"backbone\.(stem|res[234])\.(.+)", k)
        out[f"{BOTTOM_UP}.{m.group(1)}.{m.group(2)}" if m else k] = v
    return out


class C4RCNNEngine(StandardRCNNEngine):
    # pool the bins res5.0 reads and nothing else (ops.roi_align bin_stride=2), or the full grid followed by ops.subsample2: the same
    # tensor bit for bit (tests/test_roi_align_strided.py); DESIGN.md 7 item 19 records which is faster
    STRIDED_POOL = True

    def __init__(self, params: Dict[str, torch.Tensor], cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device: str = "cuda",
                 conv: str = "storage"):
        full = dict(C4_DEFAULT_CFG)
        if cfg:
            full.update(cfg)
        if any(f"{RES5}.{b}.conv2_offset.weight" in params for b in range(3)) or tuple(full.get("deform_on_per_stage") or ())[3:4] == (True,):
            raise ValueError("MODEL.RESNETS.DEFORM_ON_PER_STAGE[3]: res5 is the RoI head of a C4 model and has no deformable form ([d2] asserts the same)")
        super().__init__(trunk_names(params), full, dtype, device, conv)

    def _init_rpn(self, params) -> None:
        super()._init_rpn(params)
        if not self.has_rpn:
            return
        c = self.cfg
        sizes = c["anchor_sizes"][0]
        sizes = tuple(sizes) if isinstance(sizes, (list, tuple)) else (sizes,)
        # one level; its cell anchors size-major, then ratio ([d2] generate_cell_anchors)
        self.num_anchors = len(sizes) * len(c["anchor_ratios"])
        hidden = params[RPN_CONV + ".weight"].shape[0]  # (1024 for res4; the width comes from the weights)
        f32 = lambda k: params[k].float().contiguous().to(self.device)  # noqa: E731
        self.rpn_wo = f32("proposal_generator.rpn_head.objectness_logits.weight").view(self.num_anchors, hidden)
        self.rpn_wd = f32("proposal_generator.rpn_head.anchor_deltas.weight").view(self.num_anchors * 4, hidden)
        self.cell_anchors = cell_anchor_table([list(sizes)], c["anchor_ratios"]).to(self.device)

    def _init_roi_heads(self, params) -> None:
        dev, c = self.device, self.cfg
        f32 = lambda k: params[k].float().contiguous().to(dev)  # noqa: E731
        self.has_mask = self.has_keypoint = False
        self.has_roi = "roi_heads.box_predictor.cls_score.weight" in params
        if not self.has_roi:
            return
        res = c["pooler_resolution"]
        if isinstance(res, bool) or not isinstance(res, int) or not 1 <= res <= ops.MAX_POOLED_FWD:
            raise ValueError(f"MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION {res!r}: an integer 1 .. {ops.MAX_POOLED_FWD}")
        self.cls_w, self.cls_b = f32("roi_heads.box_predictor.cls_score.weight"), f32("roi_heads.box_predictor.cls_score.bias")
        self.box_w, self.box_b = f32("roi_heads.box_predictor.bbox_pred.weight"), f32("roi_heads.box_predictor.bbox_pred.bias")
        k = c["std_num_classes"]
        assert self.cls_w.shape[0] == k + 1 and self.box_w.shape[0] in (4, 4 * k), "cls_score: K+1 rows; bbox_pred: 4 or 4K rows"

    # ---- [d2] build_resnet_backbone with OUT_FEATURES ["res4"] ------------------------------------------------------------------------
    def _backbone(self, images: torch.Tensor, hp: int, wp: int, keep: Optional[dict] = None, normalized: bool = False) -> Dict[str, torch.Tensor]:
        x, _, stem = self._stem(images, hp, wp, normalized, keep_stem=keep is not None)
        _, res = self._stages(x, 2, 4)
        if keep is not None:
            keep["stem"] = stem
            keep.update(res)
        return {C4_FEATURE: res[C4_FEATURE]}

    def _levels(self, shapes, n):
        key = (tuple(shapes), n)
        if key not in self._lv_cache:
            self._lv_cache[key] = ops.make_rpn_levels(shapes, (C4_STRIDE,), n, self.num_anchors)
        return self._lv_cache[key]

    # ---- [d2] RPN.forward (inference) on one level ------------------------------------------------------------------------------------
    def _rpn(self, feats, image_hw, keep=None, topk=None, post_topk=None):
        c = self.cfg
        f = feats[C4_FEATURE]
        n, h, w, _ = f.shape
        shapes = [(h, w)]
        # StandardRPNHead as in the parent: the 3x3 conv + ReLU with an fp32 hidden state, the two 1x1 convs as exact-fp32 GEMMs whose
        # (rows, A) / (rows, 4A) outputs are [d2]'s (N, H*W*A) / (N, H*W*A, 4) flattening already
        t = self._conv(f, RPN_CONV, 1, 1, relu=True, out_dtype=torch.float32)
        t = t.view(-1, t.shape[-1])
        logits = ops.gemm_f32(t, self.rpn_wo, self.rpn_bo).view(-1)
        deltas = ops.gemm_f32(t, self.rpn_wd, self.rpn_bd).view(-1, 4)
        k = c["pre_nms_topk_test"] if topk is None else topk
        lv = self._levels(shapes, n)
        select = ops.rpn_select_wide if k > ops.RPN_SELECT_MAXK else ops.rpn_select
        sel = self._hbm("rpn_select" + ("_wide" if k > ops.RPN_SELECT_MAXK else ""),
                        lambda: select(lv, self.cell_anchors, logits, deltas, n, image_hw, k, c["min_box_size"], b2b_weights=c["rpn_bbox_reg_weights"]),
                        lambda: logits.numel() * 4 + n * min(k, h * w * self.num_anchors) * (16 + 16 + 4 + 4 + 4 + 4))
        post = c["post_nms_topk_test"] if post_topk is None else post_topk
        pk, pcnt = ops.nms_topk(sel["boxes"], sel["scores"], sel["level"], None, n, sel["cap"], sel["counts"], c["rpn_nms_thresh"], post)
        boxes = ops.gather_rows(sel["boxes"].view(-1, 4), sel["cap"], pk, pcnt)
        scores = ops.gather_rows(sel["scores"].view(-1), sel["cap"], pk, pcnt).view(n, post)
        out = dict(boxes=boxes, scores=scores, counts=pcnt, batch_idx=ops.padded_batch_idx(pcnt, post), cap=post, pre=sel, keep_idx=pk,
                   status_flags=sel["status_flags"], levels=lv, pred_logits=logits, pred_deltas=deltas)
        if keep is not None:
            keep.update(rpn_t=t, rpn_logits=logits, rpn_deltas=deltas, rpn_shapes=shapes, rpn_pre=sel, rpn_keep=pk)
        return out

    # ---- [d2] Res5ROIHeads._shared_roi_transform + box_predictor (inference) ------------------------------------------------------------
    def pool_res5_rois(self, feats, boxes, batch_idx, fill_padding: bool = True):
        """The input of res5.0's stride-1 form -> (pooled, stride left for res5.0). With STRIDE_IN_1X1: the even bins of the P x P grid
        (P >= 8: pooled directly; smaller grids: the full pool subsampled), stride 1. Without: the full grid, stride 2."""
        c = self.cfg
        res = c["pooler_resolution"]
        es = feats[C4_FEATURE].element_size()

        def pool(stride):
            q = -(-res // stride)
            return self._hbm("roi_align" + (" (even bins)" if stride == 2 else ""),
                             lambda: ops.roi_align([feats[C4_FEATURE]], c["pooler_scales"], boxes, batch_idx, res, self.dtype, c["canonical_level"],
                                                   c["canonical_size"], 4, fill_padding=fill_padding, aligned=c["pooler_aligned"],
                                                   sampling_ratio=c["pooler_sampling_ratio"], bin_stride=stride),
                             lambda: feats[C4_FEATURE].numel() * es + boxes.shape[0] * (q * q * feats[C4_FEATURE].shape[-1] * es + 20))
        if not c["stride_in_1x1"]:
            return pool(1), 2
        if self.STRIDED_POOL and res > 7:
            return pool(2), 1
        return ops.subsample2(pool(1)), 1

    def _box_stage(self, feats, boxes, batch_idx, s: int = 0, img_seg=None, fill_padding: bool = True):
        """The box stage on its rows: RoIAlign, res5, the spatial mean, cls_score, bbox_pred. img_seg = (counts, rows per image) of the
        padded per-image RoI lists: the convolutions skip the tiles that hold only padding RoIs and the mean writes those rows as zeros.
        -> (pooled (m, q, q, 1024), res5's output (m, o, o, 2048) with o = ceil(POOLER_RESOLUTION / 2), box_feats (m, 2048) fp32,
        logits, deltas)."""
        pooled, stride = self.pool_res5_rois(feats, boxes, batch_idx, fill_padding)
        row_segs = None
        if img_seg is not None:
            # the convolutions' row_seg, once per pass: res5's layers write q x q rows per RoI (conv1 of a block whose stride sits in
            # conv2) or o x o rows (every other layer)
            q = pooled.shape[1]
            row_segs = {r: (img_seg[0] * r, img_seg[1] * r) for r in {q * q, (-(-q // stride)) ** 2}}
        x = pooled
        for b in range(3):
            x = self._bottleneck(x, f"{RES5}.{b}", b == 0, stride if b == 0 else 1, row_segs=row_segs)
        rv, sr = img_seg if img_seg is not None else (None, 0)
        box_feats = self._hbm("avgpool_rows", lambda: ops.avgpool_rows(x, rv, sr), x.numel() * x.element_size() + x.shape[0] * x.shape[-1] * 4)
        return pooled, x, box_feats, ops.gemm_f32(box_feats, self.cls_w, self.cls_b), ops.gemm_f32(box_feats, self.box_w, self.box_b)

    def _roi_heads(self, feats, sel, image_hw, keep=None, mask: bool = True):
        c = self.cfg
        cap = sel["boxes"].shape[1]
        # (the padding rows of pooled are zero-filled only when `keep` hands them out: nothing downstream reads them)
        pooled, res5_out, box_feats, logits, deltas = self._box_stage(feats, sel["boxes"].view(-1, 4), sel["batch_idx"], img_seg=(sel["counts"], cap),
                                                                      fill_padding=keep is not None)
        cands = ops.fastrcnn_candidates(logits, deltas, sel["boxes"], sel["counts"], image_hw, c["std_num_classes"], c["bbox_reg_weights"],
                                        c["score_thresh_test"])
        if keep is not None:
            keep.update(pooled=pooled, res5_out=res5_out, box_feats=box_feats, logits=logits, deltas=deltas)
        return self._detections(feats, cands, sel["boxes"].shape[0], keep, mask)

    # ---- training: not on this path ---------------------------------------------------------------------------------------------------
    def forward_losses(self, *a, **k):
        raise NotImplementedError(TRAINING_MESSAGE)

    def rpn_losses_forward(self, *a, **k):
        raise NotImplementedError(TRAINING_MESSAGE)

    def roi_losses_forward(self, *a, **k):
        raise NotImplementedError(TRAINING_MESSAGE)
