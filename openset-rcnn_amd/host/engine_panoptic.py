"""Panoptic FPN of detectron2's zoo on the HIP path: META_ARCHITECTURE "PanopticFPN" (configs/panoptic_fpn.yaml, restating [d2]
Base-Panoptic-FPN.yaml) and "SemanticSegmentor" at inference. Written from memory of detectron2 v0.6; the kernel contract is
include/osr.h's.

  SemSegFPNHead.layers [d2]                -> _sem_seg_head: per feature p2..p5, head_length x (3x3 conv on the forward convolution,
                                              GroupNorm(32) statistics (ops.group_norm_stats), GN + ReLU + bilinear x2 (ops.gn_relu_merge));
                                              the four last stages are normalised, rectified, upsampled and summed p2 + p3 + p4 + p5 in
                                              ONE launch; the 1x1 predictor writes fp32 stride-4 logits, its rows padded to a multiple of 8
  sem_seg_postprocess + argmax [d2]        -> ops.semseg_resample on the stride-4 logits (modeling.PanopticFPN / SemanticSegmentor)
  combine_semantic_and_instance_outputs    -> ops.panoptic_combine (modeling.PanopticFPN)

The detector is StandardRCNNEngine's, mask branch included; an engine built without RPN / RoI parameters (SemanticSegmentor) runs the
trunk and the semantic head only. Inference only: the semantic loss and the GroupNorm backward have no kernels yet."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .engine_std import StandardRCNNEngine
from .weights import pack_conv_weight, sem_seg_head_lengths

SEM_SEG = "sem_seg_head"
SEM_SEG_FEATURES = ("p2", "p3", "p4", "p5")
SEM_SEG_CONVS_DIMS = (64, 128, 256)
SEM_SEG_NORMS = ("GN", "")
SEM_SEG_MAX_CLASSES = 255


def training_message(meta_arch: str) -> str:
    return (f'MODEL.META_ARCHITECTURE "{meta_arch}" runs at inference only on the HIP path: the semantic loss and the GroupNorm backward have '
            "no kernels yet")


PANOPTIC_DEFAULT_CFG = dict(sem_seg_num_classes=54, sem_seg_convs_dim=128, sem_seg_norm="GN", sem_seg_common_stride=4,
                            combine_overlap_thresh=0.5, combine_stuff_area_limit=4096, combine_instances_confidence_thresh=0.5)


def check_sem_seg_options(name: str, in_features, num_classes, convs_dim, common_stride, norm) -> None:
    """MODEL.SEM_SEG_HEAD as the HIP path takes it; ValueError naming the key otherwise."""
    if name != "SemSegFPNHead":
        raise ValueError(f"MODEL.SEM_SEG_HEAD.NAME {name!r}: only \"SemSegFPNHead\" is built on the HIP path")
    if norm not in SEM_SEG_NORMS:
        raise ValueError(f"MODEL.SEM_SEG_HEAD.NORM {norm!r}: \"GN\" (GroupNorm(32), osr_group_norm_stats) or \"\"")
    if isinstance(convs_dim, bool) or convs_dim not in SEM_SEG_CONVS_DIMS:
        raise ValueError(f"MODEL.SEM_SEG_HEAD.CONVS_DIM {convs_dim!r}: one of {SEM_SEG_CONVS_DIMS} (32 groups of 2, 4 or 8 channels)")
    if isinstance(common_stride, bool) or common_stride != 4:
        raise ValueError(f"MODEL.SEM_SEG_HEAD.COMMON_STRIDE {common_stride!r}: the HIP path merges the head at stride 4")
    if list(in_features) != list(SEM_SEG_FEATURES):
        raise ValueError(f"MODEL.SEM_SEG_HEAD.IN_FEATURES {list(in_features)!r}: the HIP path reads {list(SEM_SEG_FEATURES)}")
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= SEM_SEG_MAX_CLASSES:
        raise ValueError(f"MODEL.SEM_SEG_HEAD.NUM_CLASSES {num_classes!r}: 1 .. {SEM_SEG_MAX_CLASSES} (the combine kernel keeps a 256-entry label table)")


class PanopticFPNEngine(StandardRCNNEngine):
    def __init__(self, params: Dict[str, torch.Tensor], cfg: Optional[dict] = None, dtype: torch.dtype = torch.float16, device: str = "cuda",
                 conv: str = "storage"):
        full = dict(PANOPTIC_DEFAULT_CFG)
        if cfg:
            full.update(cfg)
        check_sem_seg_options("SemSegFPNHead", SEM_SEG_FEATURES, full["sem_seg_num_classes"], full["sem_seg_convs_dim"], full["sem_seg_common_stride"],
                              full["sem_seg_norm"])
        super().__init__(params, full, dtype, device, conv)  # (conv="split" is refused there: ValueError)

    # ---- packing ----------------------------------------------------------------------------------------------------------------
    def _pack_convs(self, params):
        """The head's 3x3 layers are packed as the other 3x3 layers are (NORM "GN": a zero bias, the layer has none); the predictor gets
        zero rows up to the next output width the forward convolution takes (a multiple of 8: 54 -> 56), as cls_score is packed;
        osr_semseg_resample reads the padded width as its pitch and never the padding."""
        own = {k: v for k, v in params.items() if k.startswith(SEM_SEG + ".")}
        w = super()._pack_convs({k: v for k, v in params.items() if k not in own})
        for k, v in own.items():
            if not k.endswith(".weight") or v.dim() != 4:
                continue
            pre = k[: -len(".weight")]
            v = v.float()
            bias = own[pre + ".bias"].float() if pre + ".bias" in own else torch.zeros(v.shape[0])
            if pre == SEM_SEG + ".predictor":
                rows = (v.shape[0] + 7) // 8 * 8
                v = torch.cat((v, v.new_zeros((rows - v.shape[0],) + tuple(v.shape[1:]))))
                bias = torch.cat((bias, torch.zeros(rows - bias.shape[0])))
            w[pre + ".w"] = pack_conv_weight(v, self.dtype).to(self.device)
            w[pre + ".b"] = bias.contiguous().to(self.device)
        return w

    def _init_roi_heads(self, params) -> None:
        super()._init_roi_heads(params)
        c = self.cfg
        self.has_sem_seg = f"{SEM_SEG}.predictor.weight" in params
        if not self.has_sem_seg:
            return
        k, dim = c["sem_seg_num_classes"], c["sem_seg_convs_dim"]
        pw = params[f"{SEM_SEG}.predictor.weight"]
        if tuple(pw.shape) != (k, dim, 1, 1):
            raise ValueError(f"sem_seg_head.predictor.weight is {tuple(pw.shape)}; MODEL.SEM_SEG_HEAD.NUM_CLASSES {k} with CONVS_DIM {dim} needs {(k, dim, 1, 1)}")
        self.sem_lengths = sem_seg_head_lengths(c["sem_seg_common_stride"])
        self.sem_pitch = self.w[f"{SEM_SEG}.predictor.w"].shape[0]
        self.sem_gn = {}
        for feat, length in self.sem_lengths.items():
            for i in range(length):
                name = f"{SEM_SEG}.{feat}.{2 * i}"
                if name + ".weight" not in params:
                    raise ValueError(f"{name}.weight is missing: SemSegFPNHead has {length} convolution(s) on {feat}")
                gn = name + ".norm.weight" in params
                if gn != (c["sem_seg_norm"] == "GN"):
                    raise ValueError(f"{name}: MODEL.SEM_SEG_HEAD.NORM {c['sem_seg_norm']!r} but the parameters " + ("carry" if gn else "lack") + " .norm.weight")
                if gn:
                    self.sem_gn[name] = tuple(params[name + s].float().contiguous().to(self.device) for s in (".norm.weight", ".norm.bias"))

    # ---- [d2] SemSegFPNHead.layers ------------------------------------------------------------------------------------------------
    def _gn_stats(self, name, y):
        return self._hbm(name + ".norm (statistics)", lambda: ops.group_norm_stats(y), y.numel() * y.element_size())

    def _gn_merge(self, name, terms):
        def nbytes():
            es = terms[0][0].element_size()
            out_elems = terms[0][0].numel() * (4 if terms[0][4] else 1)
            return (sum(t[0].numel() for t in terms) + out_elems) * es
        return self._hbm(name, lambda: ops.gn_relu_merge(terms), nbytes)

    def _sem_seg_head(self, feats, keep: Optional[dict] = None):
        """-> the stride-4 logits (n, hp / 4, wp / 4, sem_pitch) fp32; channels [NUM_CLASSES, sem_pitch) are padding. GroupNorm's
        statistics run over the whole padded map, as [d2]'s do over its ImageList."""
        if not self.has_sem_seg:
            raise ops.OsrError("this engine was built without the semantic head's parameters (sem_seg_head.predictor.weight)")
        last, stages = [], {}
        for feat, length in self.sem_lengths.items():
            x = feats[feat]
            up2 = feat != "p2"  # (every stage of a feature above the common stride ends in the x2 upsample)
            for i in range(length):
                name = f"{SEM_SEG}.{feat}.{2 * i}"
                y = self._conv(x, name, 1, 1)
                gamma, beta = self.sem_gn.get(name, (None, None))
                term = (y, self._gn_stats(name, y) if gamma is not None else None, gamma, beta, up2)
                stages[name] = y
                if i + 1 < length:
                    x = self._gn_merge(name + " GN + ReLU + x2", [term])
                    stages[name + ".out"] = x
                else:
                    last.append(term)
        total = self._gn_merge(SEM_SEG + " GN + ReLU + x2, p2 + p3 + p4 + p5 (one launch)", last)
        logits = self._conv(total, SEM_SEG + ".predictor", 1, 0, out_dtype=torch.float32)
        if keep is not None:
            keep.update(sem_stages=stages, sem_terms=last, sem_sum=total, sem_logits=logits)
        return logits

    def forward_device(self, images, image_hw, hp, wp, keep=None, mask: bool = True):
        """-> the stock detections (boxes, scores, classes, counts, mask probabilities when the engine has a mask head) followed by the
        stride-4 semantic logits; the logits alone from an engine without RPN / RoI parameters. No host sync; capturable."""
        feats = self._backbone(images, hp, wp, keep)
        if keep is not None:
            keep.update(feats=feats)
        logits = self._sem_seg_head(feats, keep)
        if not (self.has_rpn and self.has_roi):
            return (logits,)
        sel = self._rpn(feats, image_hw, keep)
        if keep is not None:
            keep.update(sel=sel)
        return tuple(self._roi_heads(feats, sel, image_hw, keep, mask=mask)) + (logits,)

    # ---- training: refused by name ----------------------------------------------------------------------------------------------
    def forward_losses(self, *a, **k):
        raise NotImplementedError(training_message("PanopticFPN"))

    def rpn_losses_forward(self, *a, **k):
        raise NotImplementedError(training_message("PanopticFPN"))

    def roi_losses_forward(self, *a, **k):
        raise NotImplementedError(training_message("PanopticFPN"))
