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
  Mask head  (MODEL.MASK_ON, bitmask ground truth) [d2] mask_rcnn_loss on the foreground prefix of every image's sampled rows
             (F = int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION) rows, the foreground count as rows_valid): 14 x 14 RoIAlign, mask_fcn*
             on the MFMA convolution, the fused deconv + predictor tail with a logits output, targets cut from the matched instance's
             bitmask (osr_mask_targets), BCE (osr_mask_loss_fwd / _bwd). Backward: osr_mask_upsample_predict_bwd (predictor, ReLU,
             deconv in one launch), the mask_fcn layers' data / weight / bias gradients, the per-sample RoIAlign scatter, summed with
             the box branch's feature gradient. The branch's gradients travel with an extra power-of-two factor (MASK_GRAD_SCALE)
             that is divided out where they become fp32: the mean over 28 x 28 pixels makes them ~10^3 smaller than the box branch's.
The loss dict is {loss_rpn_cls, loss_rpn_loc, loss_cls, loss_box_reg} (+ loss_mask)."""
from __future__ import annotations

import math
from typing import Dict, List

import torch

from . import ops
from .engine import PYRAMID, RPN_CONV
from .engine_std import StandardRCNNEngine, check_std_supported, std_loss_beta
from .train import OpensetRCNNTrainer
from .weights import pack_deconv_weight, pack_fc1_weight, unpack_deconv_weight

LOSS_KEYS = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg")  # (+ "loss_mask" from a trainer with the mask branch)
MASK_PRE = "roi_heads.mask_head."


def _pad16(x: int) -> int:
    return (x + 15) // 16 * 16


class StandardRCNNTrainer(OpensetRCNNTrainer):
    """OpensetRCNNTrainer with the stock heads. Masters: backbone / FPN convs, rpn_head.conv, then "rpn_tail" = [objectness_logits;
    anchor_deltas] (5A,256) + (5A) (one storage the engine's two GEMMs read as views), fc1, fc2, "box" (bbox_pred), "cls" (cls_score)
    -- reverse order of gradient completion, as the base class lays them out."""

    SPLIT_BOX_HEAD = False  # (box_head="split" is refused with the stock engine's ValueError)
    # The mask branch's gradients carry an extra power-of-two factor on top of the loss scale from the loss down to the places where
    # they turn fp32 (parameter gradients, the RoIAlign scatter's input), where it is divided out exactly: d loss_mask / d logit is
    # 1 / (foreground rows x 784) per pixel, which with [d2]'s 0.001 predictor initialiser puts the deconv's output gradient into
    # fp16's subnormals (measured: DESIGN section 7 item 10). The factor is MASK_GRAD_SCALE, lowered so that loss scale x factor
    # never exceeds MASK_SCALE_PRODUCT = 2^20: |d logit| <= 2^20 / 784 = 1337 then, whatever the number of foreground rows, so the
    # gradient of the upsampled activation overflows fp16 only with predictor weights above 49 -- the branch adds no overflow
    # exposure at a loss scale the user configured higher.
    MASK_GRAD_SCALE = 1024.0
    MASK_SCALE_PRODUCT = 2.0 ** 20

    def _mask_grad_scale(self) -> float:
        room = self.MASK_SCALE_PRODUCT / max(self.loss_scale, 1.0)
        return float(min(self.MASK_GRAD_SCALE, 2.0 ** max(math.floor(math.log2(room)), 0))) if room >= 1.0 else 1.0

    @staticmethod
    def _make_engine(params, cfg, dtype, device, class_map):
        eng = StandardRCNNEngine(params, cfg, dtype, device)
        check_std_supported(eng.cfg)
        return eng

    def _add_mask_masters(self, params) -> None:
        """mask_fcn1..N (3x3 convs like the trunk's: packed fp32 master, storage-type copy, backward-data copy), the deconv in the
        tail kernels' fragment order (master and gradient fp32 in that order, so the update refreshes the forward's operand in place;
        the backward's transposed operand is re-packed in _refresh_heads), the predictor's (rows, CONV_DIM) fp32 matrix, the biases.
        Reverse order of gradient completion, in front of the box head's."""
        e = self.eng
        for i in range(e.mask_num_conv):
            self._add_conv(f"{MASK_PRE}mask_fcn{i + 1}", params, bias=True)
        self.master["mask_deconv.w"] = pack_deconv_weight(params[MASK_PRE + "deconv.weight"].detach().float(), torch.float32, frag_elems=8).to(e.device)
        self.lowp["mask_deconv.w"] = e.mask_deconv_w
        self.master["mask_deconv.b"] = e.mask_deconv_b
        self.master["mask_pred.w"], self.master["mask_pred.b"] = e.mask_pred_w, e.mask_pred_b

    def _add_head_masters(self, params) -> None:
        e, dev = self.eng, self.eng.device
        a = e.num_anchors
        if e.has_mask:
            if self.dtype == torch.float32:
                raise ValueError("MODEL.MASK_ON: the mask branch trains in fp16 / bf16 (kernel_dtype float32 is an inference mode of the mask head)")
            if e.cfg["mask_pooler_resolution"] < 8:
                raise ValueError("MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION below 8: the mask tail's backward needs 8 .. 14")
            self._add_mask_masters(params)
        # one (5A,256) storage: the forward's two GEMMs read row views of it, the tail backward reads it whole
        e.rpn_wtail = torch.cat([e.rpn_wo, e.rpn_wd]).contiguous()
        e.rpn_btail = torch.cat([e.rpn_bo, e.rpn_bd]).contiguous()
        e.rpn_wo, e.rpn_wd, e.rpn_bo, e.rpn_bd = e.rpn_wtail[:a], e.rpn_wtail[a:], e.rpn_btail[:a], e.rpn_btail[a:]
        self.master["rpn_tail.w"], self.master["rpn_tail.b"] = e.rpn_wtail, e.rpn_btail
        self._add_box_masters(params)
        self._pixel_lv: Dict[tuple, object] = {}

    def _add_box_masters(self, params) -> None:
        """The box head and the two output layers (CascadeRCNNTrainer: one set per stage)."""
        e, dev = self.eng, self.eng.device
        self.master["fc1.w"] = pack_fc1_weight(params["roi_heads.box_head.fc1.weight"], 256, e.cfg["pooler_resolution"], torch.float32).to(dev)
        self.lowp["fc1.w"] = e.fc1_w
        self.master["fc1.b"] = e.fc1_b
        self.master["fc2.w"] = params["roi_heads.box_head.fc2.weight"].detach().float().contiguous().to(dev)
        self.lowp["fc2.w"] = e.fc2_w
        self.master["fc2.b"] = e.fc2_b
        self.master["box.w"], self.master["box.b"] = e.box_w, e.box_b
        self.master["cls.w"], self.master["cls.b"] = e.cls_w, e.cls_b

    def _param_rows(self):
        a = self.eng.num_anchors
        return {"rpn_tail.w": [0, a, 5 * a], "rpn_tail.b": [0, a, 5 * a]}  # objectness_logits, anchor_deltas

    def _refresh_heads(self) -> None:
        e = self.eng
        self._refresh_box_heads()
        # the RPN 3x3 conv's weight as the (2304, 256) matrix of its per-tap data gradient y = dt . W (a function of the parameters)
        w3 = e.w[RPN_CONV + ".w"].view(256, 9 * 256)
        if not hasattr(self, "w3_t"):
            self.w3_t = torch.empty((9 * 256, 256), dtype=w3.dtype, device=e.device)
        self.w3_t.copy_(w3.t())
        if e.has_mask:  # the tail backward's second operand: the deconv weight packed with Cin and Cmid exchanged
            wt = pack_deconv_weight(unpack_deconv_weight(e.mask_deconv_w).transpose(0, 1), self.dtype)
            if not hasattr(self, "mask_deconv_wt"):
                self.mask_deconv_wt = torch.empty_like(wt)
            self.mask_deconv_wt.copy_(wt)

    def _refresh_box_heads(self) -> None:
        e = self.eng
        if not hasattr(self, "t_cls"):  # zero-padded transposes of the fp32 output layers: the padding columns are written once
            self.t_cls = torch.zeros((e.cls_w.shape[1], _pad16(e.cls_w.shape[0])), dtype=torch.float32, device=e.device)
            self.t_box = torch.zeros((e.box_w.shape[1], _pad16(e.box_w.shape[0])), dtype=torch.float32, device=e.device)
        self.t_cls[:, : e.cls_w.shape[0]].copy_(e.cls_w.t())
        self.t_box[:, : e.box_w.shape[0]].copy_(e.box_w.t())

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
        last = dict(n=n, rpn_counts=rpn[2:4], roi_counts=roi["roi_counts"], stats=roi["stats"])
        if "loss_mask" in roi:
            losses["loss_mask"] = roi["loss_mask"]
            last.update(mask_stats=roi["mask_stats"], mask_side=roi_state["mask"]["logits"].shape[-1])
        return losses, last

    def event_scalars(self) -> Dict[str, float]:
        """The scalars [d2] RPN / StandardROIHeads / FastRCNNOutputLayers put into EventStorage for the last forward: rpn/num_pos_anchors,
        rpn/num_neg_anchors (per image), roi_head/num_fg_samples, roi_head/num_bg_samples (means over the images),
        fast_rcnn/cls_accuracy (only when a row was sampled), fast_rcnn/fg_cls_accuracy and fast_rcnn/false_negative (only when a
        foreground row exists) -- what [d2] FastRCNNOutputLayers puts. With the mask branch: mask_rcnn/accuracy, mask_rcnn/false_positive,
        mask_rcnn/false_negative as [d2] mask_rcnn_loss computes them (logit > 0 against the target, denominators at least 1)."""
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
        if "mask_stats" in lf:
            out.update(ops.mask_loss_scalars(lf["mask_stats"], lf["mask_side"]))
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
        d_feat = self._box_branch_bwd(s, n, S)
        if e.has_mask:  # the branch's share joins the box branch's feature gradient (storage type) in front of the trunk
            share = self._mask_head_bwd(s, n, S)
            d_feat = [ops.add_cast(a_, b_, self.dtype) for a_, b_ in zip(share, self._roi_share(d_feat))] + list(d_feat[4:])
        # --- RPN 3x3 conv: col2im of the listed anchors' per-tap gradients into the RoI heads' feature gradient (p6: into zeros) ---
        self._join_side(rpn_ready, rpn_grad)
        self._backward_trunk(s, self._sparse_rpn_scatter(self._pixel_levels(s["rpn_shapes"], n), s, n, rpn_grad, d_feat), prefetch)

    def _box_branch_bwd(self, s, n, S: float):
        """Fast R-CNN losses -> cls_score / bbox_pred (fp32) -> box head -> RoIAlign: the box branch's share of the p2..p5 feature
        gradient (times S); writes its masters' gradients."""
        e, c = self.eng, self.eng.cfg
        k = c["std_num_classes"]
        d_logits, d_deltas = ops.fastrcnn_losses_bwd(s["logits"], s["deltas"], s["boxes"], s["smp"]["gt_boxes"].view(-1, 4), s["cls"], k,
                                                     e.box_w.shape[0] == 4, c["bbox_reg_weights"], std_loss_beta(c, "roi_box"),
                                                     c["std_cls_loss_weight"], c["box_reg_weight"], S)
        d_bf = self._f32_linear_bwd(s["box_feats"], d_logits, self.t_cls, "cls", dy_pad=self.t_cls.shape[1])
        d_bf2 = self._f32_linear_bwd(s["box_feats"], d_deltas, self.t_box, "box", dy_pad=self.t_box.shape[1])
        d_bf = ops.add_cast(d_bf, d_bf2, torch.float32)
        return self._box_head_bwd(s, d_bf, n)

    def _mask_head_bwd(self, s, n, S: float) -> List[torch.Tensor]:
        """loss_mask's gradient: BCE -> predictor, ReLU, deconv (one launch) -> ReLU, mask_fcnN .. mask_fcn1 -> 14 x 14 RoIAlign. Writes
        the mask masters' gradients; returns the branch's share of the p2..p5 feature gradient (fp32, times S)."""
        e, c, g, dt = self.eng, self.eng.cfg, self.grad, self.dtype
        ms, p = s["mask"], s["p"]
        B = self._mask_grad_scale()
        k, cls, rv, f = e.mask_pred_w.shape[0], ms["cls"], ms["rows_valid"], ms["seg_rows"]
        d_logits = ops.mask_loss_bwd(ms["logits"], ms["targets"], k, cls, rv, f, scale=S * B)
        acts = ms["acts"]
        x_top = acts[-1] if acts else ms["pooled"]
        # (no conv below the tail: its data gradient goes straight to RoIAlign's fp32 sums)
        o = ops.mask_upsample_predict_bwd(x_top, e.mask_deconv_w, self.mask_deconv_wt, e.mask_deconv_b, e.mask_pred_w, d_logits, cls, rv, f,
                                          dx_dtype=None if acts else torch.float32)
        dx, gup = o["dx"], o["g"]

        def tail_grads():
            torch.mul(o["d_pred_w"], 1.0 / B, out=g["mask_pred.w"])
            torch.mul(o["d_pred_b"], 1.0 / B, out=g["mask_pred.b"])
            torch.mul(o["d_deconv_b"], 1.0 / B, out=g["mask_deconv.b"])
            dw = ops.deconv_wgrad(x_top, gup)
            torch.mul(pack_deconv_weight(dw, torch.float32, frag_elems=8), 1.0 / B, out=g["mask_deconv.w"])
        self._wg(tail_grads, x_top, gup, o["d_pred_w"], o["d_pred_b"], o["d_deconv_b"])
        self._done("mask_pred.w", "mask_pred.b", "mask_deconv.w", "mask_deconv.b")
        res = c["mask_pooler_resolution"]
        if acts:
            ops.relu_mask_(dx, acts[-1])
        for i in range(len(acts), 0, -1):
            name = f"{MASK_PRE}mask_fcn{i}"
            below = acts[i - 2] if i > 1 else ms["pooled"]

            def layer_grads(name=name, below=below, dx=dx):
                ops.conv2d_wgrad(below, dx, 3, 3, 1, 1, dw=g[name + ".w"])
                ops.bias_grad(dx, g[name + ".b"])
                g[name + ".w"].mul_(1.0 / B)
                g[name + ".b"].mul_(1.0 / B)
            self._wg(layer_grads, below, dx)
            self._done(name + ".w", name + ".b")
            # (the ReLU below a layer rides in its data gradient's epilogue; the lowest layer's leaves in fp32 for RoIAlign's sums)
            dx = ops.conv2d_dgrad(dx, self.wd[name], (res, res), 1, 1, mask=acts[i - 2] if i > 1 else None,
                                  out_dtype=None if i > 1 else torch.float32)
        dx.mul_(1.0 / B)
        shapes = [(p[k_].shape[1], p[k_].shape[2]) for k_ in PYRAMID[:4]]
        share = ops.roi_align_bwd(dx, shapes, n, c["pooler_scales"], ms["boxes"], ms["batch_idx"], c["canonical_level"], c["canonical_size"], 2,
                                  aligned=c["mask_pooler_aligned"], sampling_ratio=c["mask_pooler_sampling_ratio"], per_sample=True)
        return share

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """The trainable parameters under detectron2 names and layouts (StandardRPNHead, FastRCNNOutputLayers keys; with the mask
        branch MaskRCNNConvUpsampleHead's: mask_fcn* come with the other convolutions, deconv (Cin, Cmid, 2, 2), predictor (K, Cmid, 1, 1))."""
        out = self._export_rpn_and_mask()
        for short, long in (("cls", "roi_heads.box_predictor.cls_score"), ("box", "roi_heads.box_predictor.bbox_pred")):
            out[long + ".weight"], out[long + ".bias"] = self.master[short + ".w"].cpu().clone(), self.master[short + ".b"].cpu().clone()
        return out

    def _export_rpn_and_mask(self) -> Dict[str, torch.Tensor]:
        """The trunk, the box head's FC layers, the mask head and the RPN head's output layers."""
        out = self._export_trunk()
        if self.eng.has_mask:
            out[MASK_PRE + "deconv.weight"] = unpack_deconv_weight(self.master["mask_deconv.w"]).cpu()
            out[MASK_PRE + "deconv.bias"] = self.master["mask_deconv.b"].cpu().clone()
            pw = self.master["mask_pred.w"].cpu()
            out[MASK_PRE + "predictor.weight"] = pw.reshape(pw.shape[0], pw.shape[1], 1, 1).clone()
            out[MASK_PRE + "predictor.bias"] = self.master["mask_pred.b"].cpu().clone()
        a = self.eng.num_anchors
        t_w, t_b = self.master["rpn_tail.w"].cpu(), self.master["rpn_tail.b"].cpu()
        out["proposal_generator.rpn_head.objectness_logits.weight"] = t_w[:a].reshape(a, -1, 1, 1).clone()
        out["proposal_generator.rpn_head.objectness_logits.bias"] = t_b[:a].clone()
        out["proposal_generator.rpn_head.anchor_deltas.weight"] = t_w[a:].reshape(4 * a, -1, 1, 1).clone()
        out["proposal_generator.rpn_head.anchor_deltas.bias"] = t_b[a:].clone()
        return out
