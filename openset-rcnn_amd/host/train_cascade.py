"""One training step of Cascade R-CNN ([d2] CascadeROIHeads over the stock RPN; configs/cascade_rcnn_fpn.yaml) on the HIP path.

StandardRCNNTrainer with S box stages: the trunk, the RPN head, the mask branch, the flat gradient buffer, SGD and the loss scaling are
the base classes'. Per stage s the masters are fc1_s{s}, fc2_s{s}, box_s{s} (bbox_pred, class-agnostic: 4 rows) and cls_s{s}
(cls_score), laid out in reverse order of gradient completion: the backward walks the stages from the last to the first, and inside
a stage from the output layers down.
  Forward   CascadeRCNNEngine.roi_losses_forward: stage 0 on label_and_sample_proposals' rows, stage s > 0 on the previous stage's
            decoded boxes re-labelled at IOUS[s] (osr_cascade_refine); every stage its own osr_fastrcnn_losses_fwd with its own
            regression weights. The boxes between the stages carry no gradient ([d2] detaches them).
  Backward  per stage: osr_fastrcnn_losses_bwd, the two fp32 linears, the box head (FC2, FC1), RoIAlign's backward. [d2] puts
            _ScaleGradient(1 / S) on the pooled features, so a stage's gradient INTO the pyramid is multiplied by 1 / S (on the rows
            handed to RoIAlign's backward) while the gradients of the stage's own parameters are not. The S shares are summed in fp32,
            the mask branch's share joins them, then the trunk's backward runs as for the stock heads.
The loss dict is {loss_rpn_cls, loss_rpn_loc, loss_cls_stage{s}, loss_box_reg_stage{s}} (+ loss_mask)."""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .engine_cascade import CascadeRCNNEngine
from .engine_std import check_std_supported, std_loss_beta
from .train_std import StandardRCNNTrainer, _pad16
from .weights import pack_fc1_weight


class CascadeRCNNTrainer(StandardRCNNTrainer):
    @staticmethod
    def _make_engine(params, cfg, dtype, device, class_map):
        eng = CascadeRCNNEngine(params, cfg, dtype, device)
        check_std_supported(eng.cfg)
        return eng

    def _add_box_masters(self, params) -> None:
        e, dev = self.eng, self.eng.device
        for s in range(e.num_stages):
            bh = f"roi_heads.box_head.{s}."
            self.master[f"fc1_s{s}.w"] = pack_fc1_weight(params[bh + "fc1.weight"], 256, e.cfg["pooler_resolution"], torch.float32).to(dev)
            self.lowp[f"fc1_s{s}.w"] = e.fc1_ws[s]
            self.master[f"fc1_s{s}.b"] = e.fc1_bs[s]
            self.master[f"fc2_s{s}.w"] = params[bh + "fc2.weight"].detach().float().contiguous().to(dev)
            self.lowp[f"fc2_s{s}.w"] = e.fc2_ws[s]
            self.master[f"fc2_s{s}.b"] = e.fc2_bs[s]
            self.master[f"box_s{s}.w"], self.master[f"box_s{s}.b"] = e.box_ws[s], e.box_bs[s]
            self.master[f"cls_s{s}.w"], self.master[f"cls_s{s}.b"] = e.cls_ws[s], e.cls_bs[s]
        # (the base class packs the backward-data copies of "the" box head from these two: stage 0's)
        e.fc1_w, e.fc2_w = e.fc1_ws[0], e.fc2_ws[0]

    def _refresh_box_heads(self) -> None:
        e, S = self.eng, self.eng.num_stages
        if not hasattr(self, "t_cls_s"):
            self.t_cls_s = [torch.zeros((w.shape[1], _pad16(w.shape[0])), dtype=torch.float32, device=e.device) for w in e.cls_ws]
            self.t_box_s = [torch.zeros((w.shape[1], _pad16(w.shape[0])), dtype=torch.float32, device=e.device) for w in e.box_ws]
            # stage 0's backward-data weights are the base class's wd["fc1"] / wd["fc2"] (refreshed with the convolutions'); the later
            # stages' are packed here
            self.wd["fc1_s0"], self.wd["fc2_s0"] = self.wd["fc1"], self.wd["fc2"]
            for s in range(1, S):
                for fc, w in (("fc1", e.fc1_ws[s]), ("fc2", e.fc2_ws[s])):
                    self.wd[f"{fc}_s{s}"] = torch.empty((w.shape[1], 1, 1, w.shape[0]), dtype=w.dtype, device=e.device)
        for s in range(S):
            self.t_cls_s[s][:, : e.cls_ws[s].shape[0]].copy_(e.cls_ws[s].t())
            self.t_box_s[s][:, : e.box_ws[s].shape[0]].copy_(e.box_ws[s].t())
        for s in range(1, S):
            for fc, w in (("fc1", e.fc1_ws[s]), ("fc2", e.fc2_ws[s])):
                ops.pack_dgrad_weight(w, self.wd[f"{fc}_s{s}"].view(w.shape[1], w.shape[0]))

    # ---- forward -----------------------------------------------------------------------------------------------
    @staticmethod
    def _loss_dict(n, rpn, roi, sel, roi_state):
        losses = dict(loss_rpn_cls=rpn[0], loss_rpn_loc=rpn[1])
        losses.update({k: v for k, v in roi.items() if k.startswith(("loss_cls_stage", "loss_box_reg_stage"))})
        last = dict(n=n, rpn_counts=rpn[2:4], roi_counts=roi["roi_counts"], stage_counts=roi["stage_counts"], stage_stats=roi["stage_stats"])
        if "loss_mask" in roi:
            losses["loss_mask"] = roi["loss_mask"]
            last.update(mask_stats=roi["mask_stats"], mask_side=roi_state["mask"]["logits"].shape[-1])
        return losses, last

    def event_scalars(self) -> Dict[str, float]:
        """StandardRCNNTrainer's rpn/* and roi_head/* scalars (stage 0's sampler), and per stage what [d2] CascadeROIHeads puts under
        the name scope "stage{s}": stage{s}/roi_head/num_fg_samples, num_bg_samples for s >= 1 (_match_and_label_boxes; means over the
        images), stage{s}/fast_rcnn/cls_accuracy (when the stage has a row), fg_cls_accuracy and false_negative (when it has a
        foreground row) for every s."""
        lf = getattr(self, "_last_forward", None)
        if lf is None:
            return {}
        n, S = lf["n"], len(lf["stage_stats"])
        host = torch.cat([lf["rpn_counts"].view(-1)] + [c.to(torch.float32).view(-1) for c in lf["stage_counts"]] +
                         [st[2:7] for st in lf["stage_stats"]]).cpu().tolist()
        rc, cnt, st = host[:2], host[2:2 + 3 * n * S], host[2 + 3 * n * S:]
        out = {"rpn/num_pos_anchors": rc[0] / n, "rpn/num_neg_anchors": rc[1] / n}
        for s in range(S):
            roi = cnt[3 * n * s:3 * n * (s + 1)]
            pre = "" if s == 0 else f"stage{s}/"
            out[pre + "roi_head/num_fg_samples"] = sum(roi[1::3]) / n
            out[pre + "roi_head/num_bg_samples"] = sum(roi[2::3]) / n
            rows, correct, fg, fg_correct, fg_bg = st[5 * s:5 * (s + 1)]
            if rows > 0:
                out[f"stage{s}/fast_rcnn/cls_accuracy"] = correct / rows
                if fg > 0:
                    out[f"stage{s}/fast_rcnn/fg_cls_accuracy"] = fg_correct / fg
                    out[f"stage{s}/fast_rcnn/false_negative"] = fg_bg / fg
        if "mask_stats" in lf:
            out.update(ops.mask_loss_scalars(lf["mask_stats"], lf["mask_side"]))
        return out

    # ---- backward ----------------------------------------------------------------------------------------------
    def _box_branch_bwd(self, s, n, S: float):
        e, c = self.eng, self.eng.cfg
        k, ns = c["std_num_classes"], e.num_stages
        total = None
        for i in range(ns - 1, -1, -1):
            st = s["stages"][i]
            d_logits, d_deltas = ops.fastrcnn_losses_bwd(st["logits"], st["deltas"], st["boxes"], st["gt_boxes"], st["cls"], k, True,
                                                         e.stage_weights[i], std_loss_beta(c, "roi_box"), c["std_cls_loss_weight"],
                                                         c["box_reg_weight"], S)
            d_bf = self._f32_linear_bwd(st["box_feats"], d_logits, self.t_cls_s[i], f"cls_s{i}", dy_pad=self.t_cls_s[i].shape[1])
            d_bf2 = self._f32_linear_bwd(st["box_feats"], d_deltas, self.t_box_s[i], f"box_s{i}", dy_pad=self.t_box_s[i].shape[1])
            d_bf = ops.add_cast(d_bf, d_bf2, torch.float32)
            # (_box_head_bwd reads a stage as it reads the stock heads' state: the pyramid, and the rows' image index under "smp")
            view = dict(st, p=s["p"], smp=dict(batch_idx=st["batch_idx"]))
            if ns == 1:  # (one stage: the stock heads' backward, launch for launch)
                return self._box_head_bwd(view, d_bf, n, fc=("fc1_s0", "fc2_s0"))
            share = self._box_head_bwd(view, d_bf, n, fc=(f"fc1_s{i}", f"fc2_s{i}"), pooled_grad_scale=1.0 / ns, feat_f32=True)
            if total is None:
                total = share
            else:
                for acc, d in zip(total, share):
                    acc.add_(d)
        return total

    def _export_box_heads(self, out: Dict[str, torch.Tensor]) -> None:
        for s in range(self.eng.num_stages):
            self._export_box_head(out, f"fc1_s{s}", f"fc2_s{s}", f"roi_heads.box_head.{s}.")

    def export_state_dict(self) -> Dict[str, torch.Tensor]:
        """StandardRCNNTrainer's, with the box stages under [d2] CascadeROIHeads' names: roi_heads.box_head.{s}.fc1 / fc2,
        roi_heads.box_predictor.{s}.cls_score / bbox_pred."""
        out = self._export_rpn_and_mask()
        for s in range(self.eng.num_stages):
            for short, long in ((f"cls_s{s}", f"roi_heads.box_predictor.{s}.cls_score"), (f"box_s{s}", f"roi_heads.box_predictor.{s}.bbox_pred")):
                out[long + ".weight"], out[long + ".bias"] = self.master[short + ".w"].cpu().clone(), self.master[short + ".b"].cpu().clone()
        return out
