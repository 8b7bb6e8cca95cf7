"""One training step of the stock detectron2 Faster R-CNN that Base-RCNN-FPN.yaml selects (BASELINE config 1: RPN with
StandardRPNHead, StandardROIHeads with FastRCNNConvFCHead + FastRCNNOutputLayers) on the HIP path.

Everything below the heads -- frozen prefix, res3..res5, FPN, their backward, the flat gradient buffer and its all-reduce buckets,
SGD with momentum, loss scaling and the overflow / diverged-proposal verdicts -- is OpensetRCNNTrainer's (this class only replaces
the heads). The heads:
  RPN        anchors (level, y, x, a) with A = len(ASPECT_RATIOS), Matcher + subsample (osr_rpn_match_anchors with one label set,
             osr_subsample_labels), BCE objectness + smooth-L1 deltas (osr_std_rpn_losses_fwd / _bwd), proposals for the RoI heads:
             PRE_NMS_TOPK_TRAIN per level, NMS with the level as category, POST_NMS_TOPK_TRAIN per image, detached.
             Backward: the loss gradient (rows, 5A) is non-zero on the sampled anchors only, so the head's backward runs on the
             listed pixels (osr_rpn_sparse_rows_ex / osr_rpn_gather_cols_ex, hidden state recomputed, osr_std_rpn_tail_bwd for the two
             1x1 convs, then the 3x3 conv's weight gradient and per-tap data gradient as in the Openset trainer).
  RoI heads  GT appended, Matcher([0.5]), 512 rows per image at 25 % foreground (osr_roi_match_and_sample), box head FC1 / FC2 on
             the MFMA kernels, cls_score / bbox_pred as exact-fp32 GEMMs, cross entropy + smooth-L1 (osr_fastrcnn_losses_fwd / _bwd),
             class-agnostic or class-specific regression.
The loss dict is {loss_rpn_cls, loss_rpn_loc, loss_cls, loss_box_reg}."""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .engine import PYRAMID, RPN_CONV
from .engine_std import StandardRCNNEngine, check_std_supported, std_loss_beta
from .train import OpensetRCNNTrainer
from .weights import pack_fc1_weight

LOSS_KEYS = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg")


def _pad16(x: int) -> int:
    return (x + 15) // 16 * 16


class StandardRCNNTrainer(OpensetRCNNTrainer):
    """OpensetRCNNTrainer with the stock heads. Masters: backbone / FPN convs, rpn_head.conv, then "rpn_tail" = [objectness_logits;
    anchor_deltas] (5A,256) + (5A) (one storage the engine's two GEMMs read as views), fc1, fc2, "box" (bbox_pred), "cls" (cls_score)
    -- reverse order of gradient completion, as the base class lays them out."""

    SPLIT_BOX_HEAD = False  # (box_head="split" is refused with the stock engine's ValueError)

    @staticmethod
    def _make_engine(params, cfg, dtype, device, class_map):
        eng = StandardRCNNEngine(params, cfg, dtype, device)
        check_std_supported(eng.cfg)
        return eng

    def _add_head_masters(self, params) -> None:
        e, dev = self.eng, self.eng.device
        a = e.num_anchors
        # one (5A,256) storage: the forward's two GEMMs read row views of it, the tail backward reads it whole
        e.rpn_wtail = torch.cat([e.rpn_wo, e.rpn_wd]).contiguous()
        e.rpn_btail = torch.cat([e.rpn_bo, e.rpn_bd]).contiguous()
        e.rpn_wo, e.rpn_wd, e.rpn_bo, e.rpn_bd = e.rpn_wtail[:a], e.rpn_wtail[a:], e.rpn_btail[:a], e.rpn_btail[a:]
        self.master["rpn_tail.w"], self.master["rpn_tail.b"] = e.rpn_wtail, e.rpn_btail
        self.master["fc1.w"] = pack_fc1_weight(params["roi_heads.box_head.fc1.weight"], 256, e.cfg["pooler_resolution"], torch.float32).to(dev)
        self.lowp["fc1.w"] = e.fc1_w
        self.master["fc1.b"] = e.fc1_b
        self.master["fc2.w"] = params["roi_heads.box_head.fc2.weight"].detach().float().contiguous().to(dev)
        self.lowp["fc2.w"] = e.fc2_w
        self.master["fc2.b"] = e.fc2_b
        self.master["box.w"], self.master["box.b"] = e.box_w, e.box_b
        self.master["cls.w"], self.master["cls.b"] = e.cls_w, e.cls_b
        self._pixel_lv: Dict[tuple, object] = {}

    def _param_rows(self):
        a = self.eng.num_anchors
        return {"rpn_tail.w": [0, a, 5 * a], "rpn_tail.b": [0, a, 5 * a]}  # objectness_logits, anchor_deltas

    def _refresh_heads(self) -> None:
        e = self.eng
        if not hasattr(self, "t_cls"):  # zero-padded transposes of the fp32 output layers: the padding columns are written once
            self.t_cls = torch.zeros((e.cls_w.shape[1], _pad16(e.cls_w.shape[0])), dtype=torch.float32, device=e.device)
            self.t_box = torch.zeros((e.box_w.shape[1], _pad16(e.box_w.shape[0])), dtype=torch.float32, device=e.device)
        self.t_cls[:, : e.cls_w.shape[0]].copy_(e.cls_w.t())
        self.t_box[:, : e.box_w.shape[0]].copy_(e.box_w.t())
        # the RPN 3x3 conv's weight as the (2304, 256) matrix of its per-tap data gradient y = dt . W (a function of the parameters)
        w3 = e.w[RPN_CONV + ".w"].view(256, 9 * 256)
        if not hasattr(self, "w3_t"):
            self.w3_t = torch.empty((9 * 256, 256), dtype=w3.dtype, device=e.device)
        self.w3_t.copy_(w3.t())

    def _pixel_levels(self, shapes, n):
        """Level table of the pixel rows (one row per location): what the sparse gather / scatter walk."""
        key = (tuple(shapes), n)
        if key not in self._pixel_lv:
            self._pixel_lv[key] = ops.make_rpn_levels(shapes, self.eng.cfg["fpn_strides"], n, 1)
        return self._pixel_lv[key]

    # ---- forward -----------------------------------------------------------------------------------------------
    RPN_SAVED = ("rpn_shapes",)

    def _rpn_forward(self, feats, image_hw, keep: dict) -> dict:
        c = self.eng.cfg
        return self.eng._rpn(feats, image_hw, keep, topk=c["pre_nms_topk_train"], post_topk=c["post_nms_topk_train"])

    @staticmethod
    def _loss_dict(n, rpn, roi, sel, roi_state):
        losses = dict(loss_rpn_cls=rpn[0], loss_rpn_loc=rpn[1], loss_cls=roi["loss_cls"], loss_box_reg=roi["loss_box_reg"])
        return losses, dict(n=n, rpn_counts=rpn[2:4], roi_counts=roi["roi_counts"], stats=roi["stats"])

    def event_scalars(self) -> Dict[str, float]:
        """The scalars [d2] RPN / StandardROIHeads / FastRCNNOutputLayers put into EventStorage for the last forward: rpn/num_pos_anchors,
        rpn/num_neg_anchors (per image), roi_head/num_fg_samples, roi_head/num_bg_samples (means over the images),
        fast_rcnn/cls_accuracy (only when a row was sampled), fast_rcnn/fg_cls_accuracy and fast_rcnn/false_negative (only when a
        foreground row exists) -- what [d2] FastRCNNOutputLayers puts."""
        lf = getattr(self, "_last_forward", None)
        if lf is None:
            return {}
        n = lf["n"]
        host = torch.cat([lf["rpn_counts"].view(-1), lf["roi_counts"].to(torch.float32).view(-1), lf["stats"][2:7]]).cpu().tolist()
        rc, roi, st = host[:2], host[2:2 + 3 * n], host[2 + 3 * n:]
        rows, correct, fg, fg_correct, fg_bg = st
        out = {"rpn/num_pos_anchors": rc[0] / n, "rpn/num_neg_anchors": rc[1] / n,
               "roi_head/num_fg_samples": sum(roi[1::3]) / n, "roi_head/num_bg_samples": sum(roi[2::3]) / n}
        if rows > 0:
            out["fast_rcnn/cls_accuracy"] = correct / rows
            if fg > 0:
                out["fast_rcnn/fg_cls_accuracy"] = fg_correct / fg
                out["fast_rcnn/false_negative"] = fg_bg / fg
        return out

    # ---- backward ----------------------------------------------------------------------------------------------
    def _backward(self, s, n, grad_scale: float = 1.0, overlap: bool = True, prefetch=None):
        """Gradients of grad_scale * (sum of the four losses), times the loss scale, into self.grad."""
        if not self.sparse_rpn_bwd:
            raise NotImplementedError("StandardRCNNTrainer: the stock RPN head's backward runs on the sampled anchors only (sparse_rpn_bwd)")
        e, c, g = self.eng, self.eng.cfg, self.grad
        S = self._backward_begin(grad_scale, overlap)
        dt = self.dtype
        p, sel = s["p"], s["sel"]
        rn = RPN_CONV

        def rpn_chain():
            d = ops.std_rpn_losses_bwd(sel["levels"], e.cell_anchors, n, sel["pred_logits"], sel["pred_deltas"], s["labels"], s["matched_boxes"],
                                       c["rpn_bbox_reg_weights"], std_loss_beta(c, "rpn_box"), c["rpn_cls_weight"], c["rpn_loc_weight"],
                                       c["rpn_batch_size"], S)
            # one label set: at most BATCH_SIZE_PER_IMAGE sampled anchors per image, so at most that many pixel rows. A longer list
            # (another sampler, NaN in unsampled rows) poisons the update exactly as in the Openset trainer (see there)
            cap = n * int(c["rpn_batch_size"])
            ids, rmap, cnt2 = ops.rpn_sparse_rows_ex(d, cap)
            rows_fit = (cnt2[1:2] <= min(cap, self.sparse_rows_cap or cap)).to(torch.int32)
            plv = self._pixel_levels(s["rpn_shapes"], n)
            cols, d_rows = ops.rpn_gather_cols_ex(plv, [p[k_] for k_ in PYRAMID], n, ids, d)
            w3 = e.w[rn + ".w"].view(256, 9 * 256)
            t_rows = ops.linear(cols, w3, e.w[rn + ".b"], relu=True, out_dtype=torch.float32)
            dt_rows, _, _ = ops.std_rpn_tail_bwd(t_rows, e.rpn_wtail, d_rows, dt, dw=g["rpn_tail.w"], db=g["rpn_tail.b"])
            y_rows = self._sparse_rpn_conv_bwd(cols, dt_rows, rows_fit, self.w3_t)
            return (rmap, y_rows), torch.cuda.current_stream(self.device).record_event()

        rpn_grad, rpn_ready = self._on_side(rpn_chain)
        self._done("rpn_tail.w", "rpn_tail.b", rn + ".w", rn + ".b")
        # --- Fast R-CNN losses -> cls_score / bbox_pred (fp32) -> box head -> RoIAlign ---
        k = c["std_num_classes"]
        d_logits, d_deltas = ops.fastrcnn_losses_bwd(s["logits"], s["deltas"], s["boxes"], s["smp"]["gt_boxes"].view(-1, 4), s["cls"], k,
                                                     e.box_w.shape[0] == 4, c["bbox_reg_weights"], std_loss_beta(c, "roi_box"),
                                                     c["std_cls_loss_weight"], c["box_reg_weight"], S)
        d_bf = self._f32_linear_bwd(s["box_feats"], d_logits, self.t_cls, "cls", dy_pad=self.t_cls.shape[1])
        d_bf2 = self._f32_linear_bwd(s["box_feats"], d_deltas, self.t_box, "box", dy_pad=self.t_box.shape[1])
        d_bf = ops.add_cast(d_bf, d_bf2, torch.float32)
        d_feat = self._box_head_bwd(s, d_bf, n)
        # --- RPN 3x3 conv: col2im of the listed anchors' per-tap gradients into the RoI heads' feature gradient (p6: into zeros) ---
        self._join_side(rpn_ready, rpn_grad)
        self._backward_trunk(s, self._sparse_rpn_scatter(self._pixel_levels(s["rpn_shapes"], n), s, n, rpn_grad, d_feat), prefetch)

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters under detectron2 names and layouts (StandardRPNHead, FastRCNNOutputLayers keys)."""
        out = self._export_trunk()
        a = self.eng.num_anchors
        t_w, t_b = self.master["rpn_tail.w"].cpu(), self.master["rpn_tail.b"].cpu()
        out["proposal_generator.rpn_head.objectness_logits.weight"] = t_w[:a].reshape(a, -1, 1, 1).clone()
        out["proposal_generator.rpn_head.objectness_logits.bias"] = t_b[:a].clone()
        out["proposal_generator.rpn_head.anchor_deltas.weight"] = t_w[a:].reshape(4 * a, -1, 1, 1).clone()
        out["proposal_generator.rpn_head.anchor_deltas.bias"] = t_b[a:].clone()
        for short, long in (("cls", "roi_heads.box_predictor.cls_score"), ("box", "roi_heads.box_predictor.bbox_pred")):
            out[long + ".weight"], out[long + ".bias"] = self.master[short + ".w"].cpu().clone(), self.master[short + ".b"].cpu().clone()
        return out
