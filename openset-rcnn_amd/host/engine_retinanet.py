"""The one-stage detector of detectron2's zoo on the HIP path: META_ARCHITECTURE "RetinaNet" (configs/retinanet_fpn.yaml, restating
[d2] Base-RetinaNet.yaml) at inference. Written from memory of detectron2 v0.6; the kernel contract is include/osr.h's.

  build_retinanet_resnet_fpn_backbone [d2]   -> _fpn: laterals / outputs on res3..res5, LastLevelP6P7 on res5 (p6 = conv3x3/2(res5),
                                                p7 = conv3x3/2(relu(p6)); p6 itself is not rectified)
  RetinaNetHead.forward [d2]                 -> _head: NUM_CONVS x (3x3 + ReLU) per subnet, one launch per layer over p3..p7
                                                (ops.conv2d_levels), cls_score / bbox_pred per level into level-major buffers
  RetinaNet.inference_single_image [d2]      -> ops.retinanet_select (threshold, top TOPK_CANDIDATES_TEST per level, sigmoid, decode)
                                                -> ops.nms_topk (per class, NMS_THRESH_TEST, TEST.DETECTIONS_PER_IMAGE) -> gather

The trunk (stem, res2..res5, deformable stages included) is StandardRCNNEngine's; there is no RPN and there are no RoI heads. Inference
only: the focal loss, the matching over all anchors and the head's backward have no kernels yet."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .engine_std import StandardRCNNEngine, cell_anchor_table
from .weights import pack_conv_weight

RETINA_PYRAMID = ("p3", "p4", "p5", "p6", "p7")
RETINA_FPN_LEVELS = (3, 4, 5)
TOP_BLOCK = "backbone.top_block"
HEAD = "head"
TRAINING_MESSAGE = ('MODEL.META_ARCHITECTURE "RetinaNet" runs at inference only on the HIP path: the focal loss, the anchor matching over '
                    "all anchors and the head's backward have no kernels yet")

RETINANET_DEFAULT_CFG = dict(
    fpn_strides=(8, 16, 32, 64, 128),
    retina_anchor_sizes=tuple(tuple(x * 2 ** (i / 3) for i in range(3)) for x in (32, 64, 128, 256, 512)),
    retina_num_classes=80, retina_num_convs=4, retina_score_thresh=0.05, retina_topk=1000, retina_nms_thresh=0.5,
    retina_bbox_reg_weights=(1.0, 1.0, 1.0, 1.0),
)


def check_retina_anchors(sizes, ratios, num_levels: int = len(RETINA_PYRAMID)) -> int:
    """MODEL.ANCHOR_GENERATOR.SIZES / ASPECT_RATIOS as the head reads them -> A, the anchors per cell: one list of sizes per level
    (or one list for all), the same number on every level. ValueError naming the key otherwise."""
    key = "MODEL.ANCHOR_GENERATOR.SIZES"
    if not isinstance(sizes, (list, tuple)) or not sizes or not all(isinstance(s, (list, tuple)) and len(s) for s in sizes):
        raise ValueError(f"{key} {sizes!r}: a list of non-empty size lists")
    if len(sizes) not in (1, num_levels):
        raise ValueError(f"{key}: {len(sizes)} lists for {num_levels} levels (one per level, or one for all)")
    if len(set(len(s) for s in sizes)) != 1:
        raise ValueError(f"{key} {sizes!r}: every level must have the same number of sizes (A = sizes x ratios is one number)")
    return len(sizes[0]) * len(ratios)


class RetinaNetEngine(StandardRCNNEngine):
    def __init__(self, params: Dict[str, torch.Tensor], cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device: str = "cuda",
                 conv: str = "storage"):
        full = dict(RETINANET_DEFAULT_CFG)
        if cfg:
            full.update(cfg)
        sizes = full["retina_anchor_sizes"]
        if len(sizes) == 1:
            sizes = tuple(sizes) * len(RETINA_PYRAMID)
        full["retina_anchor_sizes"] = tuple(tuple(float(v) for v in s) for s in sizes)
        full["std_nms_thresh_test"] = full["retina_nms_thresh"]
        super().__init__(params, full, dtype, device, conv)  # (conv="split" is refused there: ValueError)

    # ---- packing ----------------------------------------------------------------------------------------------------------------
    def _pack_convs(self, params):
        """cls_score / bbox_pred: zero rows up to the next output width the forward convolution takes (a multiple of 8: A * 4 = 36 ->
        40), as conv2_offset is packed; the select kernel reads the padded width as its row pitch and never the padding."""
        w = super()._pack_convs(params)
        for name in ("cls_score", "bbox_pred"):
            pre = f"{HEAD}.{name}"
            if pre + ".weight" not in params:
                continue
            v = params[pre + ".weight"].float()
            rows = (v.shape[0] + 7) // 8 * 8
            w[pre + ".w"] = pack_conv_weight(torch.cat((v, v.new_zeros((rows - v.shape[0],) + tuple(v.shape[1:])))), self.dtype).to(self.device)
            w[pre + ".b"] = torch.cat((params[pre + ".bias"].float(), torch.zeros(rows - v.shape[0]))).contiguous().to(self.device)
        return w

    def _init_rpn(self, params) -> None:
        c = self.cfg
        self.has_rpn = False
        self.num_anchors = check_retina_anchors(c["retina_anchor_sizes"], c["anchor_ratios"])
        self.cell_anchors = cell_anchor_table(c["retina_anchor_sizes"], c["anchor_ratios"]).to(self.device)

    def _init_roi_heads(self, params) -> None:
        c = self.cfg
        self.has_roi = self.has_mask = False
        self.has_head = f"{HEAD}.cls_score.weight" in params
        if not self.has_head:
            return
        a, k = self.num_anchors, c["retina_num_classes"]
        rows_cls, rows_box = params[f"{HEAD}.cls_score.weight"].shape[0], params[f"{HEAD}.bbox_pred.weight"].shape[0]
        if rows_cls != a * k or rows_box != a * 4:
            raise ValueError(f"head.cls_score has {rows_cls} rows and head.bbox_pred {rows_box}; MODEL.RETINANET.NUM_CLASSES {k} with {a} anchors "
                             f"per cell (MODEL.ANCHOR_GENERATOR.SIZES x ASPECT_RATIOS) needs {a * k} and {a * 4}")
        self.num_convs = 0
        while f"{HEAD}.cls_subnet.{2 * self.num_convs}.weight" in params:
            self.num_convs += 1
        self.pitch_cls = self.w[f"{HEAD}.cls_score.w"].shape[0]
        self.pitch_box = self.w[f"{HEAD}.bbox_pred.w"].shape[0]

    # ---- [d2] FPN on res3..res5 + LastLevelP6P7 ------------------------------------------------------------------------------------
    def _fpn(self, res, save: Optional[dict] = None):
        if save is not None:
            raise NotImplementedError(TRAINING_MESSAGE)
        lat = {5: self._conv(res["res5"], "backbone.fpn_lateral5")}
        for lvl in (4, 3):
            lat[lvl] = self._conv(res[f"res{lvl}"], f"backbone.fpn_lateral{lvl}", residual=lat[lvl + 1], res_mode=2)
        lats = [lat[l] for l in RETINA_FPN_LEVELS]
        outs = None
        if self.fuse_levels:
            ws = [self.w[f"backbone.fpn_output{l}.w"] for l in RETINA_FPN_LEVELS]
            bs = [self.w[f"backbone.fpn_output{l}.b"] for l in RETINA_FPN_LEVELS]
            outs = self._timed("backbone.fpn_output3-5 (three levels, one launch)", lambda: ops.conv2d_levels(lats, ws, bs),
                               lambda o: self._levels_cost(lats, o, sum(x.numel() // x.shape[-1] * w_.numel() for x, w_ in zip(lats, ws)), sum(w_.numel() for w_ in ws)))
        out = {}
        for i, lvl in enumerate(RETINA_FPN_LEVELS):
            out[f"p{lvl}"] = outs[i] if outs is not None else self._conv(lat[lvl], f"backbone.fpn_output{lvl}", 1, 1)
        # [d2] v0.6 LastLevelP6P7(in_feature="res5"): p6 from res5, p7 from relu(p6); the p6 handed on is not rectified
        p6 = self._conv(res["res5"], TOP_BLOCK + ".p6", 2, 1)
        p6r = self._hbm(TOP_BLOCK + ".p7 input (relu of p6)", lambda: ops.relu_mask_(p6.clone(), p6), 2 * p6.numel() * p6.element_size())
        out["p6"] = p6
        out["p7"] = self._conv(p6r, TOP_BLOCK + ".p7", 2, 1)
        return out

    @staticmethod
    def _levels_cost(xs, outs, macs, wnumel):
        es = xs[0].element_size()
        return 2.0 * macs, (sum(x.numel() for x in xs) + sum(o.numel() for o in outs) + wnumel) * es, 2.0 * macs

    # ---- [d2] RetinaNetHead.forward ---------------------------------------------------------------------------------------------
    def _tower_layer(self, xs, name):
        """One 3x3 + ReLU layer of a subnet on p3..p7 with its shared weight: one launch, or one per level outside its envelope."""
        w, b = self.w[name + ".w"], self.w[name + ".b"]
        if self.fuse_levels:
            outs = self._timed(name + " (p3-p7, one launch)", lambda: ops.conv2d_levels(xs, w, b, relu=True),
                               lambda o: self._levels_cost(xs, o, sum(x.numel() // x.shape[-1] for x in xs) * w.numel(), w.numel()))
            if outs is not None:
                return outs
        return [self._conv(x, name, 1, 1, relu=True) for x in xs]

    def _head(self, feats, keep: Optional[dict] = None):
        """-> (logits, deltas): the level-major buffers ops.retinanet_select reads, rows of pitch_cls / pitch_box channels per cell.
        Logits in the storage dtype (fp32 in the parity engine), deltas in fp32."""
        xs = [feats[k] for k in RETINA_PYRAMID]
        n = xs[0].shape[0]
        cells = [n * x.shape[1] * x.shape[2] for x in xs]
        towers = {}
        for sub in ("cls_subnet", "bbox_subnet"):
            t = xs
            for i in range(self.num_convs):
                t = self._tower_layer(t, f"{HEAD}.{sub}.{2 * i}")
            towers[sub] = t
        logits = torch.empty((sum(cells) * self.pitch_cls,), dtype=self.dtype, device=self.device)
        deltas = torch.empty((sum(cells) * self.pitch_box,), dtype=torch.float32, device=self.device)
        off = 0
        for tc, tb, r in zip(towers["cls_subnet"], towers["bbox_subnet"], cells):
            self._conv(tc, f"{HEAD}.cls_score", 1, 1, out=logits[off * self.pitch_cls:(off + r) * self.pitch_cls], out_dtype=self.dtype)
            self._conv(tb, f"{HEAD}.bbox_pred", 1, 1, out=deltas[off * self.pitch_box:(off + r) * self.pitch_box], out_dtype=torch.float32)
            off += r
        if keep is not None:
            keep.update(cls_tower=towers["cls_subnet"], bbox_tower=towers["bbox_subnet"])
        return logits, deltas

    # ---- [d2] RetinaNet.inference ---------------------------------------------------------------------------------------------------
    def _select(self, feats, logits, deltas):
        c = self.cfg
        xs = [feats[k] for k in RETINA_PYRAMID]
        n = xs[0].shape[0]
        shapes = [(x.shape[1], x.shape[2]) for x in xs]
        lv = self._levels(shapes, n)
        k, topk = c["retina_num_classes"], c["retina_topk"]
        # algorithmic bytes: every logit once + the selected elements' deltas + the padded outputs
        return self._hbm("retinanet_select", lambda: ops.retinanet_select(lv, self.cell_anchors, logits, deltas, n, k, topk, c["retina_score_thresh"],
                                                                          c["retina_bbox_reg_weights"], self.pitch_cls, self.pitch_box),
                         logits.numel() * logits.element_size() + n * len(shapes) * topk * (16 + 16 + 4 * 4))

    def _retina_detections(self, cands, n, keep: Optional[dict] = None):
        """The batched NMS behind the candidates ([d2] batched_nms by class at NMS_THRESH_TEST) and the best DETECTIONS_PER_IMAGE."""
        c = self.cfg
        topk, cap = c["std_detections_per_image"], cands["cap"]
        seg = torch.full((n,), cap, dtype=torch.int32, device=self.device)
        ob, osc, ocl, dcnt, dk = ops.nms_gather(cands["c_boxes"], cands["c_scores"], cands["c_cls"], cands["c_cand"], n, cap, seg, c["std_nms_thresh_test"], topk,
                                                timed=lambda nms: self._hbm("nms_topk(retinanet, per class)", nms, n * cap * 28))
        if keep is not None:
            keep.update(cands=cands, det_keep=dk, det_count=dcnt)
        return ob, osc, ocl, dcnt

    def forward_device(self, images, image_hw, hp, wp, keep=None, mask: bool = True):
        """-> padded (boxes (n, DETECTIONS_PER_IMAGE, 4), scores, classes int64 (-1 padding), counts) in the model input's coordinates,
        not clipped ([d2] v0.6 leaves that to detector_postprocess). No host sync; capturable."""
        if not self.has_head:
            raise ops.OsrError("this engine was built without the RetinaNet head's parameters (head.cls_score.weight)")
        feats = self._backbone(images, hp, wp, keep)
        logits, deltas = self._head(feats, keep)
        cands = self._select(feats, logits, deltas)
        if keep is not None:
            keep.update(feats=feats, logits=logits, deltas=deltas)
        return self._retina_detections(cands, images.shape[0], keep)

    # ---- training: refused by name ----------------------------------------------------------------------------------------------
    def forward_losses(self, *a, **k):
        raise NotImplementedError(TRAINING_MESSAGE)

    def rpn_losses_forward(self, *a, **k):
        raise NotImplementedError(TRAINING_MESSAGE)

    def roi_losses_forward(self, *a, **k):
        raise NotImplementedError(TRAINING_MESSAGE)
