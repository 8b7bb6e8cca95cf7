"""Host-side mirror of the reference's plug-in surface: the detectron2-style registries and the
registered names the yaml files select --

    META_ARCHITECTURE "GeneralizedRCNN", BACKBONE.NAME "build_resnet_fpn_backbone",
    PROPOSAL_GENERATOR.NAME "ClsFreeRPN"  (classification_free_rpn.py:165), RPN.HEAD_NAME "ClsFreeRPNHead" (:50),
    ROI_HEADS.NAME "OpensetROIHeads" (osrcnn_roi_heads.py:26), ROI_BOX_HEAD.NAME "FastRCNNConvFCHead"

-- with the same constructor configuration keys, forward signatures, output field names and state-dict key names.
The modules own fp32 parameters under detectron2's names (checkpoint compatible); their inference forwards run on
the HIP library through `OpensetRCNNEngine` (no eager path). Training: `model(batched_inputs)` in training mode returns the six
losses as GPU scalars whose sum's `.backward()` runs the explicit HIP backward (no autograd graph is recorded: one
torch.autograd.Function stands for the whole step), so the loop body of train.py:135-146 runs as written with
`solver.build_optimizer` / `build_lr_scheduler`; `GeneralizedRCNN.make_trainer()` returns the object that does the work
(`trainer.step()` = forward + backward + all-reduce + SGD in one call). `ClsFreeRPN.forward(..., gt_instances)` and
`OpensetROIHeads.forward(..., targets)` return `(proposals, losses)` with the reference's keys -- loss VALUES: gradients exist
only through the model-level call, which fuses both modules' backward passes into one explicit sequence of launches.
Feature maps cross these signatures as logical (N,C,H,W) tensors in channels_last memory (= the kernels' NHWC)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import ops, parallel
from .config import CfgNode
from .engine import DEFAULT_CFG, OpensetRCNNEngine, check_deform_options, refuse_deform_training
from .engine_c4 import C4_FEATURE, C4_STRIDE, TRAINING_MESSAGE as C4_TRAINING_MESSAGE, C4RCNNEngine
from .engine_cascade import CascadeRCNNEngine, check_cascade_options
from .engine_panoptic import PanopticFPNEngine, check_sem_seg_options, training_message as panoptic_training_message
from .engine_retinanet import RETINA_PYRAMID, TRAINING_MESSAGE as RETINANET_TRAINING_MESSAGE, RetinaNetEngine, check_retina_anchors
from .engine_std import KEYPOINT_LOSS_MESSAGE, StandardRCNNEngine, check_std_supported
from .structures import Boxes, ImageList, Instances, ShapeSpec
from .weights import R50_BLOCKS, R50_MID, fold_frozen_bn


class Registry:
    def __init__(self, name: str):
        self._name = name
        self._map: Dict[str, object] = {}

    def register(self, obj=None):
        if obj is None:
            def deco(o):
                self._do(o.__name__, o)
                return o
            return deco
        self._do(obj.__name__, obj)
        return obj

    def _do(self, name, obj):
        assert name not in self._map, f"'{name}' already registered in '{self._name}'"
        self._map[name] = obj

    def get(self, name: str):
        if name not in self._map:
            raise KeyError(f"No object named '{name}' found in '{self._name}' registry (have: {sorted(self._map)})")
        return self._map[name]

    def __contains__(self, name):
        return name in self._map


META_ARCH_REGISTRY = Registry("META_ARCH")
BACKBONE_REGISTRY = Registry("BACKBONE")
PROPOSAL_GENERATOR_REGISTRY = Registry("PROPOSAL_GENERATOR")
RPN_HEAD_REGISTRY = Registry("RPN_HEAD")
ROI_HEADS_REGISTRY = Registry("ROI_HEADS")
ROI_BOX_HEAD_REGISTRY = Registry("ROI_BOX_HEAD")
ROI_MASK_HEAD_REGISTRY = Registry("ROI_MASK_HEAD")
ROI_KEYPOINT_HEAD_REGISTRY = Registry("ROI_KEYPOINT_HEAD")



def pad_ground_truth(instances: List["Instances"], masks_hw: Optional[Tuple[int, int]] = None):
    """list[Instances{gt_boxes, gt_classes}] -> padded CPU tensors (n,gmax,4) fp32, (n,gmax) int64, (n) int32 counts.
    masks_hw = (Hm, Wm): a fourth tensor, the gt_masks (BitMasks) of the instances as (n, gmax, Hm, Wm) uint8 planes, each image's
    bitmasks in the top left corner, zeros elsewhere; ValueError when an image with instances carries no gt_masks."""
    n = len(instances)
    gmax = max(1, max(len(x) for x in instances))
    gt = torch.zeros((n, gmax, 4), dtype=torch.float32)
    gcls = torch.zeros((n, gmax), dtype=torch.int64)
    gcnt = torch.zeros((n,), dtype=torch.int32)
    for i, x in enumerate(instances):
        k = len(x)
        gcnt[i] = k
        if k:
            gt[i, :k] = x.gt_boxes.tensor.float().cpu()
            gcls[i, :k] = x.gt_classes.cpu()
    if masks_hw is None:
        return gt, gcls, gcnt
    planes = torch.zeros((n, gmax) + tuple(int(v) for v in masks_hw), dtype=torch.uint8)
    for i, x in enumerate(instances):
        if len(x) == 0:
            continue
        if not x.has("gt_masks"):
            raise ValueError(f"INPUT.MASK_FORMAT \"bitmask\": image {i} of the batch has {len(x)} instances but no gt_masks "
                             "(the mapper attaches them from each annotation's `segmentation`)")
        m = x.gt_masks.tensor if hasattr(x.gt_masks, "tensor") else x.gt_masks
        if m.dim() != 3 or m.shape[0] != len(x) or m.shape[1] > planes.shape[2] or m.shape[2] > planes.shape[3]:
            raise ValueError(f"gt_masks of image {i}: {tuple(m.shape)} does not fit {len(x)} instances of an image within {tuple(planes.shape[2:])}")
        planes[i, : len(x), : m.shape[1], : m.shape[2]] = m.cpu().to(torch.uint8)
    return gt, gcls, gcnt, planes


class _ExplicitBackward(torch.autograd.Function):
    """Stands for the whole training step in torch's autograd: forward hands out the loss values the HIP kernels computed (six for
    Openset R-CNN, four for the stock heads),
    backward runs OpensetRCNNTrainer._backward (the explicit sequence of data-gradient / weight-gradient launches) when
    `losses.backward()` reaches it. The gradients land in the trainer's flat fp32 buffer, where the optimizer mirror reads them."""

    @staticmethod
    def forward(ctx, hook, trainer, saved, n, *values):
        ctx.trainer, ctx.saved, ctx.n = trainer, saved, n
        return tuple(v.detach().clone() for v in values)

    @staticmethod
    def backward(ctx, *grads):
        if ctx.saved is None:
            raise RuntimeError("the HIP backward of this iteration has already run (its saved activations are released)")
        vals = [float(g) if g is not None else 0.0 for g in grads]  # one small D2H read; train.py:138 syncs on the losses anyway
        if min(vals) != max(vals) or vals[0] <= 0.0:
            raise NotImplementedError(f"the HIP backward differentiates a uniformly weighted sum of the {len(vals)} losses (train.py:136); got d total / d loss = {vals}")
        ctx.trainer._backward(ctx.saved, ctx.n, grad_scale=vals[0])
        ctx.trainer.grads_ready = True
        ctx.saved = None
        return (None,) * (4 + len(grads))



def _to_nhwc(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Logical NCHW -> contiguous NHWC view/copy of the kernel dtype (free when already channels_last + dtype)."""
    return x.to(dtype).permute(0, 2, 3, 1).contiguous()


class _EngineOwner(nn.Module):
    """Lazily packs this module's parameters (under canonical names) into an OpensetRCNNEngine."""
    _prefix = ""
    _engine_cls = OpensetRCNNEngine

    def __init__(self):
        super().__init__()
        self._eng: Optional[OpensetRCNNEngine] = None
        self._shared: Optional[OpensetRCNNEngine] = None
        self._eng_cfg: dict = {}
        self._class_map = None
        self.kernel_dtype = torch.float16
        # how the box head's FC1 / FC2 multiply (OpensetRCNNEngine box_head): "storage", or "split" = fp32 operands as bf16 terms.
        # An attribute, not a yaml key: the reference's config files load unchanged
        self.box_head_precision = "storage"
        # how the convolutions multiply (OpensetRCNNEngine conv): "storage", or "split" = the fp32 parity mode (kernel_dtype float32)
        # on the bf16 matrix instruction. An attribute, not a yaml key, like box_head_precision
        self.conv_precision = "storage"

    def engine(self) -> OpensetRCNNEngine:
        if self._shared is not None:
            return self._shared
        want = self._box_head_precision()
        if self._eng is not None and getattr(self._eng, "box_head", "storage") != want:
            self._eng = None  # (box_head_precision was changed after the engine was packed)
        conv = self.conv_precision
        if self._eng is not None and getattr(self._eng, "conv", "storage") != conv:
            self._eng = None  # (so was conv_precision)
        if conv == "split" and self.kernel_dtype != torch.float32:
            raise ValueError('conv_precision "split" needs kernel_dtype == torch.float32: it is a mode of the fp32 engine')
        if self._eng is None:
            sd = {self._prefix + k: v.detach() for k, v in self.state_dict().items()}
            dev = next(iter(sd.values())).device
            if dev.type != "cuda":
                raise ops.OsrError("the model must be on the GPU (model.to('cuda')): the HIP path has no CPU fallback")
            sd = fold_frozen_bn({k: v.cpu() for k, v in sd.items()})
            if self._engine_cls is OpensetRCNNEngine:
                self._eng = OpensetRCNNEngine(sd, self._eng_cfg, self.kernel_dtype, str(dev), self._class_map, box_head=want, conv=conv)
            else:
                if want != "storage":
                    raise ValueError(f"box_head_precision {want!r}: the stock Faster R-CNN engine keeps its box head")
                self._eng = self._engine_cls(sd, self._eng_cfg, self.kernel_dtype, str(dev), conv=conv)  # ("split" is refused: ValueError)
        return self._eng

    def _box_head_precision(self) -> str:
        return self.box_head_precision

    def refresh(self):
        self._eng = None

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.refresh()
        return r


# ---------------------------------------------------------------------------------------------------------------
# backbone
# ---------------------------------------------------------------------------------------------------------------
class FrozenBatchNorm2d(nn.Module):
    def __init__(self, c: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(c))
        self.register_buffer("bias", torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c) - eps)


class _ConvBN(nn.Module):
    def __init__(self, cin, cout, k, gain=1.0):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin, k, k) * gain * math.sqrt(2.0 / (cout * k * k)))
        self.norm = FrozenBatchNorm2d(cout)


class _ConvBias(nn.Module):
    def __init__(self, cin, cout, k, gain=1.0):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin, k, k) * gain * math.sqrt(2.0 / (cout * k * k)))
        self.bias = nn.Parameter(torch.zeros(cout))


class _Bottleneck(nn.Module):
    """[d2] BottleneckBlock; with offset_channels > 0 a DeformBottleneckBlock: `conv2_offset` (3x3, bias, no norm, zero-initialised as
    [d2] does) predicts conv2's sampling offsets (and mask logits), conv2 keeps its names, shape and FrozenBN."""

    def __init__(self, cin, mid, cout, first, offset_channels: int = 0):
        super().__init__()
        if first:
            self.shortcut = _ConvBN(cin, cout, 1, 0.7)
        self.conv1 = _ConvBN(cin, mid, 1)
        self.conv2 = _ConvBN(mid, mid, 3)
        if offset_channels:
            self.conv2_offset = _ConvBias(mid, offset_channels, 3)
            nn.init.constant_(self.conv2_offset.weight, 0)
        self.conv3 = _ConvBN(mid, cout, 1, 0.5)


class _Stem(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = _ConvBN(3, 64, 7, 0.02)


class _BottomUp(nn.Module):
    def __init__(self, deform_on_per_stage=(False, False, False, False), offset_channels: int = 0):
        super().__init__()
        self.stem = _Stem()
        cin = 64
        for si, (nb, mid) in enumerate(zip(R50_BLOCKS, R50_MID)):
            blocks = []
            for b in range(nb):
                blocks.append(_Bottleneck(cin, mid, mid * 4, b == 0, offset_channels if deform_on_per_stage[si] else 0))
                cin = mid * 4
            setattr(self, f"res{si + 2}", nn.Sequential(*blocks))


def deform_options_from(cfg: CfgNode) -> dict:
    """MODEL.RESNETS.DEFORM_ON_PER_STAGE / DEFORM_MODULATED / DEFORM_NUM_GROUPS -> the engine's three keys, validated
    (engine.check_deform_options: a ValueError names the key)."""
    r = cfg.MODEL.RESNETS
    on = check_deform_options(r.DEFORM_ON_PER_STAGE, r.DEFORM_MODULATED, r.DEFORM_NUM_GROUPS)
    return dict(deform_on_per_stage=on, deform_modulated=bool(r.DEFORM_MODULATED), deform_num_groups=int(r.DEFORM_NUM_GROUPS))


class ResNetFPN(_EngineOwner):
    """[d2] build_resnet_fpn_backbone for R-50 (Base-RCNN-FPN.yaml:3-8): parameters under backbone.bottom_up.* /
    backbone.fpn_{lateral,output}{2..5}.*; forward(x) takes the normalised, padded (N,3,H,W) fp32 batch."""
    _prefix = "backbone."

    def __init__(self, cfg: CfgNode):
        super().__init__()
        assert cfg.MODEL.RESNETS.DEPTH == 50, "only R-50 is on the hot path (VOC-COCO / GraspNet yaml: DEPTH 50)"
        assert cfg.MODEL.RESNETS.NORM == "FrozenBN", "only FrozenBN is on the hot path"
        deform = deform_options_from(cfg)  # (ValueError naming the key when the model is built)
        self.bottom_up = _BottomUp(deform["deform_on_per_stage"], ops.deform_offset_channels(deform["deform_num_groups"], deform["deform_modulated"]))
        self._eng_cfg = {"stride_in_1x1": bool(cfg.MODEL.RESNETS.STRIDE_IN_1X1), **deform}  # (a stand-alone backbone's engine)
        for lvl, c in zip((2, 3, 4, 5), (256, 512, 1024, 2048)):
            setattr(self, f"fpn_lateral{lvl}", _ConvBias(c, 256, 1, 0.7))
            setattr(self, f"fpn_output{lvl}", _ConvBias(256, 256, 3, 0.7))
        self._out_features = ["p2", "p3", "p4", "p5", "p6"]
        self.size_divisibility = 32

    def output_shape(self) -> Dict[str, ShapeSpec]:
        return {f"p{l}": ShapeSpec(channels=256, stride=2 ** l) for l in range(2, 7)}

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        n, _, h, w = x.shape
        assert h % 32 == 0 and w % 32 == 0, "pad the batch to a multiple of 32 (ImageList.from_tensors(..., 32))"
        feats = self.engine()._backbone(x.float().contiguous(), h, w, normalized=True)
        return {k: v.permute(0, 3, 1, 2) for k, v in feats.items()}  # logical NCHW, channels_last memory


@BACKBONE_REGISTRY.register()
def build_resnet_fpn_backbone(cfg: CfgNode, input_shape=None):
    return ResNetFPN(cfg)


C4_BACKBONE, C4_ROI_HEADS = "build_resnet_backbone", "Res5ROIHeads"


def check_c4_options(cfg: CfgNode) -> None:
    """What a C4 model (BACKBONE.NAME "build_resnet_backbone" with ROI_HEADS.NAME "Res5ROIHeads") takes; a ValueError names the key.
    The two names come together: the head runs res5 on res4's RoIs, and no other head reads a single stride-16 map here."""
    m = cfg.MODEL
    if (m.BACKBONE.NAME == C4_BACKBONE) != (m.ROI_HEADS.NAME == C4_ROI_HEADS):
        raise ValueError(f"MODEL.BACKBONE.NAME {m.BACKBONE.NAME!r} with MODEL.ROI_HEADS.NAME {m.ROI_HEADS.NAME!r}: \"{C4_ROI_HEADS}\" runs on "
                         f"\"{C4_BACKBONE}\" (one stride-16 map, res5 as the RoI head) and on nothing else; the FPN backbones take "
                         "StandardROIHeads / CascadeROIHeads / OpensetROIHeads")
    if m.BACKBONE.NAME != C4_BACKBONE:
        return
    if list(m.RESNETS.OUT_FEATURES) != [C4_FEATURE]:
        raise ValueError(f"MODEL.RESNETS.OUT_FEATURES {list(m.RESNETS.OUT_FEATURES)!r}: {C4_BACKBONE} is built for [\"{C4_FEATURE}\"] "
                         "(Base-RCNN-C4.yaml); res5 is the RoI head's")
    if int(m.RESNETS.RES5_DILATION) != 1:
        raise ValueError(f"MODEL.RESNETS.RES5_DILATION {m.RESNETS.RES5_DILATION}: 1 only -- DC5 needs a dilated 3x3 convolution, which has no kernel")
    on = check_deform_options(m.RESNETS.DEFORM_ON_PER_STAGE, m.RESNETS.DEFORM_MODULATED, m.RESNETS.DEFORM_NUM_GROUPS)
    if on[3]:
        raise ValueError("MODEL.RESNETS.DEFORM_ON_PER_STAGE[3]: res5 is the RoI head of a C4 model and is not deformable ([d2] asserts the same)")
    if m.MASK_ON:
        raise ValueError(f"MODEL.MASK_ON with {C4_ROI_HEADS}: the fused mask tail takes at most 448 input channels, res5's RoI features have 2048")
    if m.KEYPOINT_ON:
        raise ValueError(f"MODEL.KEYPOINT_ON with {C4_ROI_HEADS}: the keypoint branch is built for StandardROIHeads")
    if cfg.TEST.AUG.ENABLED:
        raise ValueError(f"TEST.AUG: test-time augmentation is implemented for StandardROIHeads only, not {C4_ROI_HEADS}")
    if list(m.RPN.IN_FEATURES) != [C4_FEATURE] or list(m.ROI_HEADS.IN_FEATURES) != [C4_FEATURE]:
        raise ValueError(f"MODEL.RPN.IN_FEATURES {list(m.RPN.IN_FEATURES)!r} / MODEL.ROI_HEADS.IN_FEATURES {list(m.ROI_HEADS.IN_FEATURES)!r}: "
                         f"[\"{C4_FEATURE}\"] with {C4_BACKBONE}")
    if len(m.ANCHOR_GENERATOR.SIZES) != 1:
        raise ValueError(f"MODEL.ANCHOR_GENERATOR.SIZES {m.ANCHOR_GENERATOR.SIZES!r}: one list (one level) with {C4_BACKBONE}")
    k = int(m.RPN.PRE_NMS_TOPK_TEST)
    if not 1 <= k <= ops.RPN_SELECT_WIDE_MAXK:
        raise ValueError(f"MODEL.RPN.PRE_NMS_TOPK_TEST {k}: 1 .. {ops.RPN_SELECT_WIDE_MAXK} per level on the HIP path")


def c4_engine_cfg_from(cfg: CfgNode) -> dict:
    """engine_cfg_from for a C4 model: every anchor size of the one level, and the one pooler scale."""
    e = engine_cfg_from(cfg)
    e.update(anchor_sizes=(tuple(float(z) for z in cfg.MODEL.ANCHOR_GENERATOR.SIZES[0]),), pooler_scales=(1.0 / C4_STRIDE,))
    return e


class ResNetC4(_EngineOwner):
    """[d2] build_resnet_backbone for R-50 with OUT_FEATURES ["res4"] (Base-RCNN-C4.yaml): stem and res2..res4 under [d2]'s names
    backbone.stem.* / backbone.res{2,3,4}.* (no `bottom_up`); forward(x) takes the normalised, padded (N,3,H,W) fp32 batch and returns
    {"res4": (N,1024,H/16,W/16)}."""
    _prefix = "backbone."
    _engine_cls = C4RCNNEngine

    def __init__(self, cfg: CfgNode):
        super().__init__()
        assert cfg.MODEL.RESNETS.DEPTH == 50, "only R-50 is on the hot path (VOC-COCO / GraspNet yaml: DEPTH 50)"
        assert cfg.MODEL.RESNETS.NORM == "FrozenBN", "only FrozenBN is on the hot path"
        check_c4_options(cfg)
        deform = deform_options_from(cfg)
        off = ops.deform_offset_channels(deform["deform_num_groups"], deform["deform_modulated"])
        self.stem = _Stem()
        cin = 64
        for si, (nb, mid) in enumerate(zip(R50_BLOCKS[:3], R50_MID[:3])):
            blocks = []
            for b in range(nb):
                blocks.append(_Bottleneck(cin, mid, mid * 4, b == 0, off if deform["deform_on_per_stage"][si] else 0))
                cin = mid * 4
            setattr(self, f"res{si + 2}", nn.Sequential(*blocks))
        self._eng_cfg = {"stride_in_1x1": bool(cfg.MODEL.RESNETS.STRIDE_IN_1X1), **deform}  # (a stand-alone backbone's engine)
        self._out_features = [C4_FEATURE]
        self.size_divisibility = 32  # ([d2] pads a C4 batch to its largest image only; the trunk's kernels take multiples of 32)

    def output_shape(self) -> Dict[str, ShapeSpec]:
        return {C4_FEATURE: ShapeSpec(channels=1024, stride=C4_STRIDE)}

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        n, _, h, w = x.shape
        assert h % 32 == 0 and w % 32 == 0, "pad the batch to a multiple of 32 (ImageList.from_tensors(..., 32))"
        feats = self.engine()._backbone(x.float().contiguous(), h, w, normalized=True)
        return {k: v.permute(0, 3, 1, 2) for k, v in feats.items()}  # logical NCHW, channels_last memory


@BACKBONE_REGISTRY.register()
def build_resnet_backbone(cfg: CfgNode, input_shape=None):
    return ResNetC4(cfg)


# ---------------------------------------------------------------------------------------------------------------
# CF-RPN
# ---------------------------------------------------------------------------------------------------------------
class _Conv3x3ReLU(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        self.bias = nn.Parameter(torch.zeros(cout))


@RPN_HEAD_REGISTRY.register()
class ClsFreeRPNHead(_EngineOwner):
    """classification_free_rpn.py:50-162. forward(features) -> (list[(N,A*4,Hi,Wi)], list[(N,A,Hi,Wi)] sigmoid-ed)."""
    _prefix = "proposal_generator.rpn_head."

    def __init__(self, cfg: CfgNode = None, input_shape: List[ShapeSpec] = None, *, in_channels: int = 256, num_anchors: int = 1,
                 box_dim: int = 4):
        super().__init__()
        if cfg is not None:
            in_channels = input_shape[0].channels
            assert len(set(s.channels for s in input_shape)) == 1, "Each level must have the same channel!"
            assert list(cfg.MODEL.RPN.CONV_DIMS) == [-1], "only the single-conv head is on the hot path"
            num_anchors = len(cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS[0]) * len(cfg.MODEL.ANCHOR_GENERATOR.SIZES[0])
        assert in_channels == 256 and num_anchors == 1 and box_dim == 4, "HIP CF-RPN head: 256 channels, A=1 (VOC-COCO/GraspNet yaml)"
        self.conv = _Conv3x3ReLU(in_channels, in_channels)
        self.anchor_deltas = nn.Conv2d(in_channels, num_anchors * box_dim, kernel_size=1)
        self.centerness = nn.Conv2d(in_channels, num_anchors, kernel_size=1)
        for m in (self.conv, self.anchor_deltas, self.centerness):  # classification_free_rpn.py:105-108
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)

    def forward(self, features: List[torch.Tensor]):
        eng = self.engine()
        deltas, ctrs = [], []
        for x in features:
            n, _, h, w = x.shape
            d, c = ops.cfrpn_head_fused(_to_nhwc(x, eng.dtype), eng.w["proposal_generator.rpn_head.conv.w"],
                                        eng.w["proposal_generator.rpn_head.conv.b"], eng.rpn_wtail, eng.rpn_btail)
            deltas.append(d.view(n, h, w, 4).permute(0, 3, 1, 2))
            ctrs.append(c.view(n, h, w, 1).permute(0, 3, 1, 2))
        return deltas, ctrs


@PROPOSAL_GENERATOR_REGISTRY.register()
class ClsFreeRPN(nn.Module):
    """classification_free_rpn.py:165-610. forward(images, features, gt_instances=None) ->
    (list[Instances{proposal_boxes, objectness_logits}], losses dict)."""

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec]):
        super().__init__()
        self.in_features = list(cfg.MODEL.RPN.IN_FEATURES)
        shapes = [input_shape[f] for f in self.in_features]
        self.rpn_head = RPN_HEAD_REGISTRY.get(cfg.MODEL.RPN.HEAD_NAME)(cfg, shapes)
        self.strides = [s.stride for s in shapes]
        self.anchor_sizes = [float(s[0]) for s in cfg.MODEL.ANCHOR_GENERATOR.SIZES]
        assert len(self.anchor_sizes) == len(self.in_features)
        self.pre_nms_topk = {True: cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, False: cfg.MODEL.RPN.PRE_NMS_TOPK_TEST}
        self.post_nms_topk = {True: cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN, False: cfg.MODEL.RPN.POST_NMS_TOPK_TEST}  # accepted, unused (F1)
        self.nms_thresh = {True: cfg.MODEL.RPN.NMS_THRESH, False: cfg.MODEL.RPN.NMS_THRESH_TEST}                  # idem
        self.min_box_size = float(cfg.MODEL.PROPOSAL_GENERATOR.MIN_SIZE)
        self.loss_weight = {"loss_rpn_loc": cfg.MODEL.RPN.BBOX_REG_LOSS_WEIGHT * cfg.MODEL.RPN.LOSS_WEIGHT,
                            "loss_rpn_ctr": cfg.MODEL.RPN.CTR_REG_LOSS_WEIGHT * cfg.MODEL.RPN.LOSS_WEIGHT}
        self.rpn_head._eng_cfg = engine_cfg_from(cfg)  # a stand-alone ClsFreeRPN trains / selects with the yaml's hyper-parameters
        self.sampler_generator = torch.Generator().manual_seed(max(int(cfg.SEED), 0))  # uniform keys replacing torch.randperm (H6)

    def select(self, features: Dict[str, torch.Tensor], image_sizes: List[Tuple[int, int]]):
        """Device-resident result of predict_proposals (padded arrays + counts), as the engine consumes it."""
        feats = [features[f] for f in self.in_features]
        deltas, ctrs = self.rpn_head(feats)
        n = feats[0].shape[0]
        shapes = [(f.shape[2], f.shape[3]) for f in feats]
        # (N,4,H,W)/(N,1,H,W) views of NHWC memory -> level-major (N*H*W, 4) / (N*H*W)
        d_cat = torch.cat([d.permute(0, 2, 3, 1).reshape(-1, 4) for d in deltas]).contiguous()
        c_cat = torch.cat([c.permute(0, 2, 3, 1).reshape(-1) for c in ctrs]).contiguous()
        dev = d_cat.device
        lv = ops.make_rpn_levels(shapes, self.strides, n, 1)
        cell = torch.tensor([[[-s / 2, -s / 2, s / 2, s / 2]] for s in self.anchor_sizes], dtype=torch.float32, device=dev)
        hw = torch.tensor(image_sizes, dtype=torch.int32, device=dev)
        sel = ops.rpn_select(lv, cell, c_cat, d_cat, n, hw, int(self.pre_nms_topk[self.training]), self.min_box_size)
        sel.update(pred_deltas=d_cat, pred_ctr=c_cat, levels=lv)
        return sel, hw

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], gt_instances: Optional[List[Instances]] = None):
        sel, _ = self.select(features, images.image_sizes)
        losses = {}
        if self.training:
            # classification_free_rpn.py:531-547: targets + both losses on the head outputs. Loss VALUES (GPU scalars): the
            # gradients of a training step come from the model-level call (see the module docstring).
            assert gt_instances is not None, "RPN requires gt_instances in training!"
            n, dev = len(gt_instances), sel["boxes"].device
            gt, _, gcnt = pad_ground_truth(gt_instances)
            r = sel["pred_ctr"].numel() // n
            keys = {k: torch.rand((n, r), generator=self.sampler_generator).to(dev) for k in ("rpn_reg", "rpn_obj")}
            with torch.no_grad():
                rpn, _ = self.rpn_head.engine().rpn_losses_forward(sel, n, gt.to(dev), gcnt.to(dev), keys)
            losses = {"loss_rpn_loc": rpn[0], "loss_rpn_ctr": rpn[1]}
        # the list-of-Instances API needs the lengths on the host: one D2H copy brings the selection's status word with them
        host = torch.cat((sel["counts"], sel["status_flags"])).cpu().tolist()
        counts = host[:-1]
        if self.training and host[-1] != 0:  # find_top_proposals.py:96-101 (at test time the rows are dropped silently: the kernel did)
            raise FloatingPointError("Predicted boxes or scores contain Inf/NaN. Training has diverged.")
        if self.training:  # the scalars classification_free_rpn.py:459-463,553-554 puts into EventStorage
            pos_reg, neg_reg, pos_obj, neg_obj = [float(v) for v in rpn[2:6].tolist()]
            self.storage = {"rpn/num_pos_anchors": pos_reg / n, "rpn/num_neg_anchors": neg_reg / n, "rpn/obj_num_pos_anchors": pos_obj / n,
                            "rpn/obj_num_neg_anchors": neg_obj / n, "rpn/num_proposals": sum(counts) / max(n, 1)}
        out = []
        for i, size in enumerate(images.image_sizes):
            r = Instances(size)
            r.proposal_boxes = Boxes(sel["boxes"][i, : counts[i]])
            r.objectness_logits = sel["scores"][i, : counts[i]]
            out.append(r)
        return out, losses


@RPN_HEAD_REGISTRY.register()
class StandardRPNHead(_EngineOwner):
    """[d2] StandardRPNHead (RPN.HEAD_NAME default; Base-RCNN-FPN.yaml leaves it): 3x3 conv + ReLU, `objectness_logits` 1x1 (A) and
    `anchor_deltas` 1x1 (A*4); init N(0, 0.01), zero bias. forward(features) -> (list[(N,A,Hi,Wi)] logits, list[(N,A*4,Hi,Wi)] deltas)
    -- [d2]'s order: logits first."""
    _prefix = "proposal_generator.rpn_head."
    _engine_cls = StandardRCNNEngine

    def __init__(self, cfg: CfgNode, input_shape: List[ShapeSpec]):
        super().__init__()
        in_channels = input_shape[0].channels
        assert len(set(s.channels for s in input_shape)) == 1, "Each level must have the same channel!"
        assert list(cfg.MODEL.RPN.CONV_DIMS) == [-1] and in_channels in (256, 1024)  # (an FPN level, or res4 of a C4 backbone)
        self.num_anchors = len(cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS[0]) * len(cfg.MODEL.ANCHOR_GENERATOR.SIZES[0])
        self.conv = _Conv3x3ReLU(in_channels, in_channels)
        self.objectness_logits = nn.Conv2d(in_channels, self.num_anchors, kernel_size=1)
        self.anchor_deltas = nn.Conv2d(in_channels, self.num_anchors * 4, kernel_size=1)
        for m in (self.conv, self.objectness_logits, self.anchor_deltas):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)

    def forward(self, features: List[torch.Tensor]):
        eng = self.engine()
        logits, deltas = [], []
        for x in features:
            n, _, h, w = x.shape
            t = ops.conv2d(_to_nhwc(x, eng.dtype), eng.w["proposal_generator.rpn_head.conv.w"], eng.w["proposal_generator.rpn_head.conv.b"], 1, 1, True,
                           out_dtype=torch.float32).view(-1, self.conv.weight.shape[0])
            logits.append(ops.gemm_f32(t, eng.rpn_wo, eng.rpn_bo).view(n, h, w, -1).permute(0, 3, 1, 2))
            deltas.append(ops.gemm_f32(t, eng.rpn_wd, eng.rpn_bd).view(n, h, w, -1).permute(0, 3, 1, 2))
        return logits, deltas


@PROPOSAL_GENERATOR_REGISTRY.register()
class RPN(nn.Module):
    """[d2] RPN (PROPOSAL_GENERATOR.NAME default, Base-RCNN-FPN.yaml:9-21), inference branch: anchors with the yaml's aspect
    ratios, StandardRPNHead, Box2BoxTransform(RPN.BBOX_REG_WEIGHTS) decode, per-level top PRE_NMS_TOPK, NMS at RPN.NMS_THRESH per
    level, first POST_NMS_TOPK. forward(images, features, gt_instances=None) -> (list[Instances{proposal_boxes,
    objectness_logits}], {}). Training (gt_instances given): [d2] label_and_sample_anchors + losses -- loss_rpn_cls (BCE objectness),
    loss_rpn_loc (smooth-L1 deltas) as VALUES (the gradients come from the model-level call, see the module docstring) -- and the
    training proposals (PRE_NMS_TOPK_TRAIN per level, POST_NMS_TOPK_TRAIN per image)."""

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec]):
        super().__init__()
        self.in_features = list(cfg.MODEL.RPN.IN_FEATURES)
        shapes = [input_shape[f] for f in self.in_features]
        self.rpn_head = RPN_HEAD_REGISTRY.get(cfg.MODEL.RPN.HEAD_NAME)(cfg, shapes)
        self.rpn_head._eng_cfg = engine_cfg_from(cfg)
        if cfg.MODEL.BACKBONE.NAME == C4_BACKBONE:  # one level with every size: the C4 engine's anchors and its wide select
            self.rpn_head._eng_cfg = c4_engine_cfg_from(cfg)
            self.rpn_head._engine_cls = C4RCNNEngine
        check_std_supported(self.rpn_head._eng_cfg)  # (an unsupported loss type is refused when the model is built)
        self.sampler_generator = torch.Generator().manual_seed(max(int(cfg.SEED), 0))  # uniform keys replacing torch.randperm (H6)

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], gt_instances: Optional[List[Instances]] = None):
        eng = self.rpn_head.engine()
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        dev = feats[self.in_features[0]].device
        hw = torch.tensor(images.image_sizes, dtype=torch.int32, device=dev)
        losses = {}
        if self.training and isinstance(eng, C4RCNNEngine):
            raise NotImplementedError(C4_TRAINING_MESSAGE)
        if self.training:
            assert gt_instances is not None, "RPN requires gt_instances in training!"
            c, n = eng.cfg, len(gt_instances)
            sel = eng._rpn(feats, hw, topk=c["pre_nms_topk_train"], post_topk=c["post_nms_topk_train"])
            gt, _, gcnt = pad_ground_truth(gt_instances)
            keys = {"rpn_reg": torch.rand((n, sel["pred_logits"].numel() // n), generator=self.sampler_generator).to(dev)}
            with torch.no_grad():
                rpn, _ = eng.rpn_losses_forward(sel, n, gt.to(dev), gcnt.to(dev), keys)
            losses = {"loss_rpn_cls": rpn[0], "loss_rpn_loc": rpn[1]}
        else:
            sel = eng._rpn(feats, hw)
        host = torch.cat((sel["counts"], sel["status_flags"])).cpu().tolist()
        counts = host[:-1]
        if self.training and host[-1] != 0:  # [d2] find_top_rpn_proposals raises in training (at test time the kernel drops the rows)
            raise FloatingPointError("Predicted boxes or scores contain Inf/NaN. Training has diverged.")
        if self.training:
            pos, neg = [float(v) for v in rpn[2:4].tolist()]
            self.storage = {"rpn/num_pos_anchors": pos / n, "rpn/num_neg_anchors": neg / n}
        out = []
        for i, size in enumerate(images.image_sizes):
            r = Instances(size)
            r.proposal_boxes = Boxes(sel["boxes"][i, : counts[i]])
            r.objectness_logits = sel["scores"][i, : counts[i]]
            out.append(r)
        return out, losses


# ---------------------------------------------------------------------------------------------------------------
# RoI heads
# ---------------------------------------------------------------------------------------------------------------
@ROI_BOX_HEAD_REGISTRY.register()
class FastRCNNConvFCHead(nn.Module):
    """[d2] box head with NUM_FC=2 (Base-RCNN-FPN.yaml:24-27): fc1 (c*7*7 -> 1024), fc2 (1024 -> 1024), ReLU each."""

    def __init__(self, cfg: CfgNode, input_shape: ShapeSpec):
        super().__init__()
        assert cfg.MODEL.ROI_BOX_HEAD.NUM_CONV == 0 and cfg.MODEL.ROI_BOX_HEAD.NUM_FC == 2
        fc = cfg.MODEL.ROI_BOX_HEAD.FC_DIM
        self.fc1 = nn.Linear(input_shape.channels * input_shape.height * input_shape.width, fc)
        self.fc2 = nn.Linear(fc, fc)
        self.output_shape = ShapeSpec(channels=fc)


class OpensetFastRCNNOutputLayers(nn.Module):
    """osrcnn_fast_rcnn.py:148-264: bbox_pred (class-agnostic 4) and iou_pred (1, sigmoid)."""

    def __init__(self, cfg: CfgNode, input_shape: ShapeSpec):
        super().__init__()
        assert cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG, "the Openset yaml files use class-agnostic box regression"
        self.bbox_pred = nn.Linear(input_shape.channels, 4)
        self.iou_pred = nn.Linear(input_shape.channels, 1)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        nn.init.normal_(self.iou_pred.weight, std=0.01)
        nn.init.constant_(self.bbox_pred.bias, 0)
        nn.init.constant_(self.iou_pred.bias, 0)


class PLN(nn.Module):
    """prototype_learning_network.py:17-97: encoder, decoder, `representatives` (num_known*reps, emd)."""

    def __init__(self, cfg: CfgNode):
        super().__init__()
        fd, ed = cfg.MODEL.ROI_BOX_HEAD.FC_DIM, cfg.MODEL.PLN.EMD_DIM
        if cfg.MODEL.PLN.DISTANCE_TYPE not in ("COS", "L1", "L2"):
            raise ValueError(f"MODEL.PLN.DISTANCE_TYPE '{cfg.MODEL.PLN.DISTANCE_TYPE}': one of COS, L1, L2 (prototype_learning_network.py:155-160)")
        self.encoder = nn.Linear(fd, ed)
        self.decoder = nn.Linear(ed, fd)
        for l in (self.encoder, self.decoder):
            nn.init.normal_(l.weight, std=0.01)
            nn.init.constant_(l.bias, 0)
        self.representatives = nn.Parameter(torch.randn(cfg.MODEL.ROI_HEADS.NUM_KNOWN_CLASSES * cfg.MODEL.PLN.REPS_PER_CLASS, ed))


class SoftMaxClassifier(nn.Module):
    """softmax_classifier.py:170-245: cls_score (FC_DIM -> num_known+1)."""

    def __init__(self, cfg: CfgNode):
        super().__init__()
        self.cls_score = nn.Linear(cfg.MODEL.ROI_BOX_HEAD.FC_DIM, cfg.MODEL.ROI_HEADS.NUM_KNOWN_CLASSES + 1)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.constant_(self.cls_score.bias, 0)


def freeze_at_of(cfg: CfgNode) -> int:
    """MODEL.BACKBONE.FREEZE_AT as [d2] ResNet.freeze reads it: >= 1 freezes the stem, >= k freezes stage res<k>; values above 5
    freeze the whole bottom-up network (act as 5), negative values are refused."""
    v = int(cfg.MODEL.BACKBONE.FREEZE_AT)
    if v < 0:
        raise ValueError(f"MODEL.BACKBONE.FREEZE_AT must be >= 0, got {v}")
    return min(v, 5)


POOLER_TYPES = {"ROIAlignV2": True, "ROIAlign": False}  # MODEL.ROI_BOX_HEAD.POOLER_TYPE -> `aligned` of torchvision's roi_align


def pooler_options_from(cfg: CfgNode, head: str = "ROI_BOX_HEAD") -> Tuple[bool, int]:
    """MODEL.<head>.POOLER_TYPE / POOLER_SAMPLING_RATIO (head: ROI_BOX_HEAD, or ROI_MASK_HEAD for the mask branch) as [d2] ROIPooler
    reads them -> (aligned, sampling_ratio) of the RoIAlign kernels. "ROIPool" and "ROIAlignRotated" have no kernel and a negative ratio
    no meaning: ValueError when the model is built."""
    bh = cfg.MODEL[head]
    if bh.POOLER_TYPE not in POOLER_TYPES:
        raise ValueError(f"MODEL.{head}.POOLER_TYPE {bh.POOLER_TYPE!r}: one of {tuple(POOLER_TYPES)}")
    ratio = bh.POOLER_SAMPLING_RATIO
    if isinstance(ratio, bool) or not isinstance(ratio, int) or not 0 <= ratio <= ops.MAX_SAMPLING_RATIO:
        raise ValueError(f"MODEL.{head}.POOLER_SAMPLING_RATIO {ratio!r}: 0 (adaptive grid) or an integer S in 1 .. {ops.MAX_SAMPLING_RATIO} "
                         "(S x S samples per bin)")
    return POOLER_TYPES[bh.POOLER_TYPE], int(ratio)


def engine_cfg_from(cfg: CfgNode) -> dict:
    """yaml keys -> engine hyper-parameters."""
    rh, bh, rpn = cfg.MODEL.ROI_HEADS, cfg.MODEL.ROI_BOX_HEAD, cfg.MODEL.RPN
    aligned, sampling_ratio = pooler_options_from(cfg)
    return dict(
        pooler_aligned=aligned, pooler_sampling_ratio=sampling_ratio,
        pixel_mean=tuple(cfg.MODEL.PIXEL_MEAN), pixel_std=tuple(cfg.MODEL.PIXEL_STD),
        anchor_sizes=tuple(float(s[0]) for s in cfg.MODEL.ANCHOR_GENERATOR.SIZES),
        pre_nms_topk_test=cfg.MODEL.RPN.PRE_NMS_TOPK_TEST, min_box_size=float(cfg.MODEL.PROPOSAL_GENERATOR.MIN_SIZE),
        pooler_resolution=bh.POOLER_RESOLUTION, bbox_reg_weights=tuple(bh.BBOX_REG_WEIGHTS), mean_type=rh.MEAN_TYPE,
        obj_score_thresh=rh.OBJ_SCORE_THRESH_TEST, nms_thresh_test=rh.NMS_THRESH_TEST, detections_per_image=cfg.TEST.DETECTIONS_PER_IMAGE,
        known_score_thresh=rh.KNOWN_SCORE_THRESH, known_nms_thresh=rh.KNOWN_NMS_THRESH, known_topk=rh.KNOWN_TOPK,
        unknown_score_thresh=rh.UNKNOWN_SCORE_THRESH, unknown_nms_thresh=rh.UNKNOWN_NMS_THRESH, unknown_topk=rh.UNKNOWN_TOPK,
        stride_in_1x1=bool(cfg.MODEL.RESNETS.STRIDE_IN_1X1), **deform_options_from(cfg),
        num_classes=rh.NUM_CLASSES, num_known=rh.NUM_KNOWN_CLASSES, reps_per_class=cfg.MODEL.PLN.REPS_PER_CLASS, pln_distance=cfg.MODEL.PLN.DISTANCE_TYPE,
        # the reference hard-codes the unknown id: 80 with --opendet-benchmark, else 1000
        unknown_id=80 if cfg.OPENDET_BENCHMARK else 1000, unk_thr=cfg.MODEL.PLN.UNK_THR,
        # training step
        pre_nms_topk_train=cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, rpn_batch_size=cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE,
        rpn_positive_fraction=cfg.MODEL.RPN.POSITIVE_FRACTION, rpn_positive_fraction_objectness=cfg.MODEL.RPN.POSITIVE_FRACTION_OBJECTNESS,
        rpn_iou_thresholds=tuple(cfg.MODEL.RPN.IOU_THRESHOLDS), rpn_iou_thresholds_objectness=tuple(cfg.MODEL.RPN.IOU_THRESHOLDS_OBJECTNESS),
        rpn_loc_weight=rpn.BBOX_REG_LOSS_WEIGHT * rpn.LOSS_WEIGHT, rpn_ctr_weight=rpn.CTR_REG_LOSS_WEIGHT * rpn.LOSS_WEIGHT,
        roi_batch_size=rh.BATCH_SIZE_PER_IMAGE, roi_positive_fraction=rh.POSITIVE_FRACTION, roi_iou_threshold=float(rh.IOU_THRESHOLDS[0]),
        box_reg_weight=bh.BBOX_REG_LOSS_WEIGHT, iou_reg_weight=bh.IOU_REG_LOSS_WEIGHT, pln_alpha=cfg.MODEL.PLN.ALPHA, pln_beta=cfg.MODEL.PLN.BETA,
        pln_iou_threshold=cfg.MODEL.PLN.IOU_THRESHOLD, pln_loss_weight=cfg.MODEL.PLN.LOSS_WEIGHT, cls_loss_weight=bh.CLS_LOSS_WEIGHT,
        # the stock detectron2 modules of Base-RCNN-FPN.yaml (BASELINE config 1; engine_std.StandardRCNNEngine)
        anchor_ratios=tuple(float(r) for r in cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS[0]), post_nms_topk_test=cfg.MODEL.RPN.POST_NMS_TOPK_TEST,
        rpn_nms_thresh=cfg.MODEL.RPN.NMS_THRESH, rpn_bbox_reg_weights=tuple(cfg.MODEL.RPN.BBOX_REG_WEIGHTS), std_num_classes=rh.NUM_CLASSES,
        score_thresh_test=rh.SCORE_THRESH_TEST, std_nms_thresh_test=rh.NMS_THRESH_TEST, std_detections_per_image=cfg.TEST.DETECTIONS_PER_IMAGE,
        cls_agnostic_bbox_reg=bool(bh.CLS_AGNOSTIC_BBOX_REG), post_nms_topk_train=cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN, rpn_cls_weight=rpn.LOSS_WEIGHT,
        # [d2] CascadeROIHeads (engine_cascade.CascadeRCNNEngine): one entry per stage
        cascade_bbox_reg_weights=tuple(tuple(w) if isinstance(w, (list, tuple)) else w for w in cfg.MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS),
        cascade_ious=tuple(cfg.MODEL.ROI_BOX_CASCADE_HEAD.IOUS),
        # checked by engine.check_supported_losses when a loss is first computed (inference never needs them)
        loss_types=dict(rpn_box=(rpn.BBOX_REG_LOSS_TYPE, float(rpn.SMOOTH_L1_BETA)), rpn_ctr=(rpn.CTR_REG_LOSS_TYPE, float(rpn.CTR_SMOOTH_L1_BETA)),
                        roi_box=(bh.BBOX_REG_LOSS_TYPE, float(bh.SMOOTH_L1_BETA)), roi_iou=(bh.IOU_REG_LOSS_TYPE, float(bh.IOU_SMOOTH_L1_BETA))),
    )


@ROI_HEADS_REGISTRY.register()
class OpensetROIHeads(_EngineOwner):
    """osrcnn_roi_heads.py:26-329. forward(images, features, proposals, targets=None) ->
    (list[Instances{pred_boxes, scores, pred_classes}], {}) at inference."""
    _prefix = "roi_heads."

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec], class_id: Optional[torch.Tensor] = None):
        super().__init__()
        self.in_features = self.box_in_features = list(cfg.MODEL.ROI_HEADS.IN_FEATURES)
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.pooler_scales = tuple(1.0 / input_shape[k].stride for k in self.in_features)
        ch = input_shape[self.in_features[0]].channels
        self.box_head = ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)(cfg, ShapeSpec(channels=ch, height=res, width=res))
        self.box_predictor = OpensetFastRCNNOutputLayers(cfg, self.box_head.output_shape)
        self.dml = PLN(cfg)
        self.softmaxcls = SoftMaxClassifier(cfg)
        self.num_classes = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        self._eng_cfg = engine_cfg_from(cfg)
        self._eng_cfg["pooler_scales"] = self.pooler_scales
        # GraspNet: sorted contiguous ids of the known categories (prototype_learning_network.py:80-95); VOC-COCO: identity
        self._class_map = class_id
        self.sampler_generator = torch.Generator().manual_seed(max(int(cfg.SEED), 0))  # uniform keys replacing torch.randperm (H6)

    def forward_device(self, features: Dict[str, torch.Tensor], sel: dict, image_hw: torch.Tensor):
        eng = self.engine()
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        return eng._roi_heads(feats, sel, image_hw)

    @staticmethod
    def _pack_proposals(proposals: List[Instances]):
        n = len(proposals)
        dev = proposals[0].proposal_boxes.tensor.device
        counts = [len(p) for p in proposals]
        cap = max(max(counts), 1)
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
        scores = torch.zeros((n, cap), dtype=torch.float32, device=dev)
        bidx = torch.full((n, cap), -1, dtype=torch.int32, device=dev)
        for i, p in enumerate(proposals):
            boxes[i, : counts[i]] = p.proposal_boxes.tensor
            scores[i, : counts[i]] = p.objectness_logits
            bidx[i, : counts[i]] = i
        return boxes, scores, bidx, torch.tensor(counts, dtype=torch.int32, device=dev), cap

    def _forward_train(self, features: Dict[str, torch.Tensor], proposals: List[Instances], targets: List[Instances]):
        """osrcnn_roi_heads.py:268-277: label_and_sample_proposals + the four head losses. Returns the sampled proposals (with
        gt_classes / gt_boxes / ious attached, as :203-216 does) and the loss VALUES (see the module docstring for gradients)."""
        eng = self.engine()
        boxes, scores, _, counts, cap = self._pack_proposals(proposals)
        n, dev = len(proposals), boxes.device
        gt, gcls, gcnt = pad_ground_truth(targets)
        keys = torch.rand((n, cap + gt.shape[1]), generator=self.sampler_generator).to(dev)
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        with torch.no_grad():
            losses, st = eng.roi_losses_forward(feats, boxes, scores, counts, gt.to(dev), gcls.to(dev), gcnt.to(dev), keys)
        smp = st["smp"]
        nsmp = smp["counts"][:, 0].cpu().tolist()  # rows actually sampled per image (<= BATCH_SIZE_PER_IMAGE)
        out = []
        for i, p in enumerate(proposals):
            k = int(nsmp[i])
            r = Instances(p.image_size)
            r.proposal_boxes = Boxes(smp["boxes"][i, :k])
            r.objectness_logits = smp["logits"][i, :k]
            r.gt_classes = smp["gt_classes"][i, :k]
            r.gt_boxes = Boxes(smp["gt_boxes"][i, :k])
            r.ious = smp["ious"][i, :k]
            out.append(r)
        return out, {k: v for k, v in losses.items() if k.startswith("loss_")}

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], proposals: List[Instances],
                targets: Optional[List[Instances]] = None):
        del images
        if self.training:
            assert targets, "'targets' argument is required during training"
            return self._forward_train(features, proposals, targets)
        n = len(proposals)
        boxes, scores, bidx, counts, cap = self._pack_proposals(proposals)
        dev = boxes.device
        sel = dict(boxes=boxes, scores=scores, batch_idx=bidx.view(-1), counts=counts, cap=cap)
        hw = torch.tensor([p.image_size for p in proposals], dtype=torch.int32, device=dev)
        res = OpensetRCNNEngine.to_instances(self.forward_device(features, sel, hw), n)
        out = []
        for r, p in zip(res, proposals):
            inst = Instances(p.image_size)
            inst.pred_boxes = Boxes(r["pred_boxes"])
            inst.scores = r["scores"]
            inst.pred_classes = r["pred_classes"]
            out.append(inst)
        return out, {}


@ROI_MASK_HEAD_REGISTRY.register()
class MaskRCNNConvUpsampleHead(nn.Module):
    """[d2] MaskRCNNConvUpsampleHead (Base-RCNN-FPN.yaml:29-33) with [d2]'s parameter names, so that model-zoo mask_rcnn checkpoints
    load: mask_fcn1..NUM_CONV (3x3, CONV_DIM, ReLU), deconv (ConvTranspose2d 2x2 stride 2, ReLU), predictor (1x1 to one map when
    CLS_AGNOSTIC_MASK, else NUM_CLASSES maps). Initialisers: c2_msra_fill for the convolutions, normal(std=0.001) for the predictor."""

    def __init__(self, cfg: CfgNode, input_shape: ShapeSpec):
        super().__init__()
        mh = cfg.MODEL.ROI_MASK_HEAD
        if mh.NORM != "":
            raise ValueError(f"MODEL.ROI_MASK_HEAD.NORM {mh.NORM!r}: the mask head's convolutions have no normalisation on the HIP path (\"\")")
        dim, cur = int(mh.CONV_DIM), input_shape.channels
        if mh.NUM_CONV < 0 or dim % 64 or cur % 64 or (mh.NUM_CONV == 0 and cur > 448) or (mh.NUM_CONV > 0 and dim > 448):
            raise ValueError(f"MODEL.ROI_MASK_HEAD: NUM_CONV >= 0 and CONV_DIM a multiple of 64, at most 448 (got {mh.NUM_CONV}, {dim})")
        self.num_conv = int(mh.NUM_CONV)
        for k in range(self.num_conv):
            conv = nn.Conv2d(cur, dim, 3, padding=1)
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(conv.bias, 0)
            self.add_module(f"mask_fcn{k + 1}", conv)
            cur = dim
        self.deconv = nn.ConvTranspose2d(cur, dim, 2, stride=2)
        nn.init.kaiming_normal_(self.deconv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.deconv.bias, 0)
        self.num_mask_classes = 1 if mh.CLS_AGNOSTIC_MASK else int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        self.predictor = nn.Conv2d(dim, self.num_mask_classes, 1)
        nn.init.normal_(self.predictor.weight, std=0.001)
        nn.init.constant_(self.predictor.bias, 0)


@ROI_KEYPOINT_HEAD_REGISTRY.register()
class KRCNNConvDeconvUpsampleHead(nn.Module):
    """[d2] KRCNNConvDeconvUpsampleHead with [d2]'s parameter names, so that model-zoo keypoint_rcnn checkpoints load: conv_fcn1..N
    (3x3, CONV_DIMS[i], ReLU), score_lowres (ConvTranspose2d 4x4 stride 2 pad 1 to NUM_KEYPOINTS maps), then bilinear x2 (no
    parameters). Initialiser: kaiming_normal_(fan_out, relu) for every weight, zero biases. What the fused tail
    (ops.keypoint_upsample) and the convolution do not take is refused here by key name."""

    def __init__(self, cfg: CfgNode, input_shape: ShapeSpec):
        super().__init__()
        kh = cfg.MODEL.ROI_KEYPOINT_HEAD
        dims = [int(d) for d in kh.CONV_DIMS]
        if not dims:
            raise ValueError("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS is empty: the head needs at least one conv_fcn layer")
        if any(d < 64 or d % 64 or d > 512 for d in dims):
            raise ValueError(f"MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS {tuple(dims)}: every entry a multiple of 64, at most 512")
        k = kh.NUM_KEYPOINTS
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 32:
            raise ValueError(f"MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS {k!r}: an integer 1 .. 32 (the MFMA tile of the fused tail)")
        cur = input_shape.channels
        self.num_conv, self.num_keypoints = len(dims), int(k)
        for i, d in enumerate(dims):
            conv = nn.Conv2d(cur, d, 3, padding=1)
            self.add_module(f"conv_fcn{i + 1}", conv)
            cur = d
        self.score_lowres = nn.ConvTranspose2d(cur, self.num_keypoints, 4, stride=2, padding=1)
        for name, prm in self.named_parameters():
            if name.endswith("bias"):
                nn.init.constant_(prm, 0)
            else:
                nn.init.kaiming_normal_(prm, mode="fan_out", nonlinearity="relu")


MASK_LOSS_MESSAGE = ("MODEL.MASK_ON with INPUT.MASK_FORMAT \"polygon\": the mask loss (mask_rcnn_loss) trains on bitmask ground truth only "
                     "-- rasterising polygons needs pycocotools, which the HIP path does not have. Set INPUT.MASK_FORMAT \"bitmask\" "
                     "(2-D arrays or uncompressed RLE per annotation) to train the mask branch; at inference the mask head runs either way")


class FastRCNNOutputLayers(nn.Module):
    """[d2] FastRCNNOutputLayers: cls_score (K+1) and bbox_pred (4, or 4K when not class-agnostic); init std 0.01 / 0.001."""

    def __init__(self, cfg: CfgNode, input_shape: ShapeSpec):
        super().__init__()
        k = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        self.cls_score = nn.Linear(input_shape.channels, k + 1)
        self.bbox_pred = nn.Linear(input_shape.channels, 4 if cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG else 4 * k)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        for l in (self.cls_score, self.bbox_pred):
            nn.init.constant_(l.bias, 0)


@ROI_HEADS_REGISTRY.register()
class StandardROIHeads(_EngineOwner):
    """[d2] StandardROIHeads (Base-RCNN-FPN.yaml:22-28), box branch, inference: ROIPooler(7x7, ROIAlignV2) -> FastRCNNConvFCHead ->
    FastRCNNOutputLayers.inference (softmax, Box2BoxTransform(10,10,5,5), SCORE_THRESH_TEST, per-class NMS_THRESH_TEST,
    TEST.DETECTIONS_PER_IMAGE). forward(images, features, proposals, targets=None) -> (list[Instances{pred_boxes, scores,
    pred_classes}], {}). Training (targets given): label_and_sample_proposals + the box branch's loss_cls / loss_box_reg VALUES and the
    sampled proposals (gradients: the model-level call, see the module docstring)."""
    _prefix = "roi_heads."
    _engine_cls = StandardRCNNEngine
    _keypoint_branch = True  # (CascadeROIHeads: False -- MODEL.KEYPOINT_ON is refused there)

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec], class_id=None):
        super().__init__()
        self.keypoint_on = bool(cfg.MODEL.KEYPOINT_ON)
        if self.keypoint_on and (not self._keypoint_branch or cfg.MODEL.ROI_HEADS.NUM_CLASSES != 1):
            raise ValueError(f"MODEL.KEYPOINT_ON: the keypoint branch is built for StandardROIHeads with ROI_HEADS.NUM_CLASSES 1, the one-class "
                             f"person detector of [d2]'s Keypoint R-CNN configs (got {type(self).__name__}, NUM_CLASSES {cfg.MODEL.ROI_HEADS.NUM_CLASSES})")
        self.in_features = self.box_in_features = list(cfg.MODEL.ROI_HEADS.IN_FEATURES)
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        ch = input_shape[self.in_features[0]].channels
        self.box_head = ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)(cfg, ShapeSpec(channels=ch, height=res, width=res))
        self.box_predictor = FastRCNNOutputLayers(cfg, self.box_head.output_shape)
        self._eng_cfg = engine_cfg_from(cfg)
        self._eng_cfg["pooler_scales"] = tuple(1.0 / input_shape[k].stride for k in self.in_features)
        check_std_supported(self._eng_cfg)  # (an unsupported loss type is refused when the model is built)
        self.sampler_generator = torch.Generator().manual_seed(max(int(cfg.SEED), 0))  # uniform keys replacing torch.randperm (H6)
        # [d2] StandardROIHeads._init_mask_head: the mask branch pools the same levels with its own resolution / type / ratio
        self.mask_on = bool(cfg.MODEL.MASK_ON)
        self.mask_format = str(cfg.INPUT.get("MASK_FORMAT", "polygon")) if "INPUT" in cfg else "polygon"
        if self.mask_on and self.mask_format not in ("polygon", "bitmask"):
            raise ValueError(f"INPUT.MASK_FORMAT {self.mask_format!r}: \"polygon\" or \"bitmask\"")
        if self.mask_on:
            mh = cfg.MODEL.ROI_MASK_HEAD
            aligned, ratio = pooler_options_from(cfg, "ROI_MASK_HEAD")
            mres = mh.POOLER_RESOLUTION
            if isinstance(mres, bool) or not isinstance(mres, int) or not 1 <= mres <= ops.MAX_POOLED_FWD:
                raise ValueError(f"MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION {mres!r}: an integer 1 .. {ops.MAX_POOLED_FWD}")
            self.mask_in_features = self.in_features
            self.mask_head = ROI_MASK_HEAD_REGISTRY.get(mh.NAME)(cfg, ShapeSpec(channels=ch, height=mres, width=mres))
            self._eng_cfg.update(mask_pooler_resolution=int(mres), mask_pooler_aligned=aligned, mask_pooler_sampling_ratio=ratio)
        # [d2] StandardROIHeads._init_keypoint_head: the same levels again, with the keypoint pooler's resolution / type / ratio
        if self.keypoint_on:
            kh = cfg.MODEL.ROI_KEYPOINT_HEAD
            aligned, ratio = pooler_options_from(cfg, "ROI_KEYPOINT_HEAD")
            kres = kh.POOLER_RESOLUTION
            if isinstance(kres, bool) or not isinstance(kres, int) or not 8 <= kres <= 14:
                raise ValueError(f"MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION {kres!r}: an integer 8 .. 14 (the fused tail keeps one RoI's map on chip)")
            if kh.NAME not in ROI_KEYPOINT_HEAD_REGISTRY:
                raise ValueError(f"MODEL.ROI_KEYPOINT_HEAD.NAME {kh.NAME!r}: not a registered keypoint head")
            self.keypoint_in_features = self.in_features
            self.keypoint_head = ROI_KEYPOINT_HEAD_REGISTRY.get(kh.NAME)(cfg, ShapeSpec(channels=ch, height=kres, width=kres))
            self._eng_cfg.update(keypoint_pooler_resolution=int(kres), keypoint_pooler_aligned=aligned, keypoint_pooler_sampling_ratio=ratio)

    def _forward_train(self, features: Dict[str, torch.Tensor], proposals: List[Instances], targets: List[Instances]):
        """[d2] label_and_sample_proposals + FastRCNNOutputLayers.losses: the sampled proposals (gt_classes / gt_boxes attached) and the
        loss values."""
        if self.keypoint_on:
            raise NotImplementedError(KEYPOINT_LOSS_MESSAGE)
        if self.mask_on and self.mask_format != "bitmask":
            raise NotImplementedError(MASK_LOSS_MESSAGE)
        eng = self.engine()
        boxes, scores, _, counts, cap = OpensetROIHeads._pack_proposals(proposals)
        n, dev = len(proposals), boxes.device
        mask_kw = {}
        if self.mask_on:
            sizes = [tuple(int(v) for v in t.image_size) for t in targets]
            gt, gcls, gcnt, planes = pad_ground_truth(targets, (max(s[0] for s in sizes), max(s[1] for s in sizes)))
            mask_kw = dict(gt_masks=planes.to(dev), image_hw=torch.tensor(sizes, dtype=torch.int32, device=dev))
        else:
            gt, gcls, gcnt = pad_ground_truth(targets)
        if eng.ROI_LOSSES_NEED_IMAGE_HW and not mask_kw:
            mask_kw = dict(image_hw=torch.tensor([tuple(int(v) for v in t.image_size) for t in targets], dtype=torch.int32, device=dev))
        keys = torch.rand((n, cap + gt.shape[1]), generator=self.sampler_generator).to(dev)
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        with torch.no_grad():
            losses, st = eng.roi_losses_forward(feats, boxes, scores, counts, gt.to(dev), gcls.to(dev), gcnt.to(dev), keys, **mask_kw)
        smp = st["smp"]  # ([d2] CascadeROIHeads returns these too: the first stage's sampled proposals)
        host = smp["counts"].cpu()
        self.storage = {"roi_head/num_fg_samples": float(host[:, 1].sum()) / n, "roi_head/num_bg_samples": float(host[:, 2].sum()) / n}
        out = []
        for i, p in enumerate(proposals):
            k = int(host[i, 0])
            r = Instances(p.image_size)
            r.proposal_boxes = Boxes(smp["boxes"][i, :k])
            r.objectness_logits = smp["logits"][i, :k]
            r.gt_classes = smp["gt_classes"][i, :k]
            r.gt_boxes = Boxes(smp["gt_boxes"][i, :k])
            out.append(r)
        return out, {k: v for k, v in losses.items() if k.startswith("loss_")}

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], proposals: List[Instances], targets=None):
        del images
        if self.training:
            assert targets, "'targets' argument is required during training"
            return self._forward_train(features, proposals, targets)
        eng = self.engine()
        n = len(proposals)
        boxes, scores, bidx, counts, cap = OpensetROIHeads._pack_proposals(proposals)
        sel = dict(boxes=boxes, scores=scores, batch_idx=bidx.view(-1), counts=counts, cap=cap)
        hw = torch.tensor([p.image_size for p in proposals], dtype=torch.int32, device=boxes.device)
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        res = OpensetRCNNEngine.to_instances(eng._roi_heads(feats, sel, hw), n, eng.output_fields())
        out = []
        for r, p in zip(res, proposals):
            out.append(_std_instances(p.image_size, r))
        return out, {}


    def forward_with_given_boxes(self, features: Dict[str, torch.Tensor], instances: List[Instances]) -> List[Instances]:
        """[d2] StandardROIHeads.forward_with_given_boxes: the mask and keypoint branches on boxes the caller supplies. instances carry
        pred_boxes and pred_classes; they come back with pred_masks (k, 1, M, M) probabilities (MASK_ON) and pred_keypoints (k, K, 3) /
        pred_keypoint_heatmaps (k, K, 4P, 4P) (KEYPOINT_ON) added, every other field as given -- unchanged when the model has neither
        head. features: the NCHW pyramid of the backbone."""
        assert not self.training, "forward_with_given_boxes is an inference entry"
        for inst in instances:
            if not (inst.has("pred_boxes") and inst.has("pred_classes")):
                raise ValueError("forward_with_given_boxes: every Instances needs pred_boxes and pred_classes")
        if not (self.mask_on or self.keypoint_on):
            return instances
        eng = self.engine()
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        return self._attach_branches(eng, feats, instances)

    @staticmethod
    def _attach_branches(eng, feats: Dict[str, torch.Tensor], instances: List[Instances]) -> List[Instances]:
        """The engine's mask and keypoint heads (those it has) on the given boxes, over its NHWC pyramid. The lists are padded to the
        engine's detection capacity (or the longest list, when longer), so a pass's own detections run through the very launches that
        made its masks and keypoints."""
        dev = eng.device
        n = len(instances)
        cap = max([int(eng.cfg["std_detections_per_image"])] + [len(i) for i in instances])
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32)
        classes = torch.full((n, cap), -1, dtype=torch.int64)
        for i, inst in enumerate(instances):
            k = len(inst)
            boxes[i, :k] = inst.pred_boxes.tensor.detach().float().cpu()
            classes[i, :k] = inst.pred_classes.detach().to(torch.int64).cpu()
        counts = torch.tensor([len(i) for i in instances], dtype=torch.int32)
        boxes, counts = boxes.to(dev), counts.to(dev)
        probs = eng._mask_head(feats, boxes, classes.to(dev), counts) if eng.has_mask else None
        kp, heat = eng._keypoint_head(feats, boxes, counts) if eng.has_keypoint else (None, None)
        out = []
        for i, inst in enumerate(instances):
            r = Instances(inst.image_size, **inst.get_fields())
            if probs is not None:
                r.pred_masks = probs[i, : len(inst)].unsqueeze(1)
            if kp is not None:
                r.pred_keypoints, r.pred_keypoint_heatmaps = kp[i, : len(inst)], heat[i, : len(inst)]
            out.append(r)
        return out


@ROI_HEADS_REGISTRY.register()
class CascadeROIHeads(StandardROIHeads):
    """[d2] CascadeROIHeads (Cascade R-CNN; configs/cascade_rcnn_fpn.yaml): S = len(MODEL.ROI_BOX_CASCADE_HEAD.IOUS) box stages.
    `box_head` and `box_predictor` are ModuleLists of S entries under [d2]'s parameter names (roi_heads.box_head.{s}.fc1.weight,
    roi_heads.box_predictor.{s}.cls_score.weight, roi_heads.box_predictor.{s}.bbox_pred.weight with 4 rows), so model-zoo cascade
    checkpoints load. Inference: every stage refines the previous stage's boxes, the stages' class scores are averaged, the last
    stage's boxes are kept. Training: stage 0 on label_and_sample_proposals' rows, stage s on the previous stage's boxes re-labelled
    at IOUS[s]; losses loss_cls_stage{s} / loss_box_reg_stage{s}; the mask head (MODEL.MASK_ON) trains on stage 0's rows and runs on
    the final detections. What [d2] asserts is refused with a ValueError when the model is built."""
    _engine_cls = CascadeRCNNEngine

    _keypoint_branch = False

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec], class_id=None):
        ch = cfg.MODEL.ROI_BOX_CASCADE_HEAD
        stages = check_cascade_options(ch.IOUS, ch.BBOX_REG_WEIGHTS, first_iou=cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS[0],
                                       cls_agnostic=bool(cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG))
        super().__init__(cfg, input_shape, class_id)
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        shape = ShapeSpec(channels=input_shape[self.in_features[0]].channels, height=res, width=res)
        heads = [ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)(cfg, shape) for _ in range(stages)]
        self.box_predictor = nn.ModuleList([FastRCNNOutputLayers(cfg, h.output_shape) for h in heads])
        self.box_head = nn.ModuleList(heads)
        self.num_cascade_stages = stages


@ROI_HEADS_REGISTRY.register()
class Res5ROIHeads(_EngineOwner):
    """[d2] Res5ROIHeads (Base-RCNN-C4.yaml), box branch, inference: ROIPooler(14x14, ROIAlignV2) on res4 -> res5's three bottlenecks per
    RoI -> the spatial mean -> FastRCNNOutputLayers.inference. Parameters under [d2]'s names roi_heads.res5.{0,1,2}.* and
    roi_heads.box_predictor.{cls_score,bbox_pred}.*, so faster_rcnn_R_50_C4 checkpoints load. forward(images, features, proposals) ->
    (list[Instances{pred_boxes, scores, pred_classes}], {}). Not a StandardROIHeads: no mask or keypoint branch, no given boxes, no
    test-time augmentation. Training raises NotImplementedError naming the head."""
    _prefix = "roi_heads."
    _engine_cls = C4RCNNEngine

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec], class_id=None):
        super().__init__()
        check_c4_options(cfg)
        self.in_features = self.box_in_features = list(cfg.MODEL.ROI_HEADS.IN_FEATURES)
        if C4_FEATURE not in input_shape:
            raise ValueError(f"MODEL.ROI_HEADS.NAME \"{C4_ROI_HEADS}\" on a backbone without \"{C4_FEATURE}\" ({sorted(input_shape)}): it needs "
                             f"MODEL.BACKBONE.NAME \"{C4_BACKBONE}\"")
        self.mask_on = self.keypoint_on = False
        cin, mid, cout = input_shape[C4_FEATURE].channels, R50_MID[3], R50_MID[3] * 4
        self.res5 = nn.Sequential(*[_Bottleneck(cin if b == 0 else cout, mid, cout, b == 0) for b in range(R50_BLOCKS[3])])
        self.box_predictor = FastRCNNOutputLayers(cfg, ShapeSpec(channels=cout))
        self._eng_cfg = c4_engine_cfg_from(cfg)
        res = self._eng_cfg["pooler_resolution"]
        if isinstance(res, bool) or not isinstance(res, int) or not 1 <= res <= ops.MAX_POOLED_FWD:
            raise ValueError(f"MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION {res!r}: an integer 1 .. {ops.MAX_POOLED_FWD}")

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], proposals: List[Instances], targets=None):
        del images
        if self.training:
            raise NotImplementedError(C4_TRAINING_MESSAGE)
        eng = self.engine()
        n = len(proposals)
        boxes, scores, bidx, counts, cap = OpensetROIHeads._pack_proposals(proposals)
        sel = dict(boxes=boxes, scores=scores, batch_idx=bidx.view(-1), counts=counts, cap=cap)
        hw = torch.tensor([p.image_size for p in proposals], dtype=torch.int32, device=boxes.device)
        feats = {k: _to_nhwc(features[k], eng.dtype) for k in self.in_features}
        res = OpensetRCNNEngine.to_instances(eng._roi_heads(feats, sel, hw), n, eng.output_fields())
        return [_std_instances(p.image_size, r) for r, p in zip(res, proposals)], {}


def _std_instances(image_size, r: dict) -> Instances:
    """Instances of one image from OpensetRCNNEngine.to_instances' dict; pred_masks (k, 1, M, M) probabilities when the engine has a
    mask head ([d2] mask_rcnn_inference), pred_keypoints (k, K, 3) {x, y, score} and pred_keypoint_heatmaps (k, K, 4P, 4P) when it has a
    keypoint head ([d2] keypoint_rcnn_inference)."""
    inst = Instances(image_size, pred_boxes=Boxes(r["pred_boxes"]), scores=r["scores"], pred_classes=r["pred_classes"])
    for f in ("pred_masks", "pred_keypoints", "pred_keypoint_heatmaps"):
        if f in r:
            inst.set(f, r[f])
    return inst


# ---------------------------------------------------------------------------------------------------------------
# meta architecture
# ---------------------------------------------------------------------------------------------------------------
MASK_THRESHOLD = 0.5  # [d2] detector_postprocess's mask_threshold


def detector_postprocess(results: Instances, output_height: int, output_width: int, mask_threshold: float = MASK_THRESHOLD) -> Instances:
    """[d2] rescale to the requested output resolution, clip, drop empty boxes; pred_masks (k, 1, M, M) probabilities on the GPU are
    then pasted into (k, H, W) bool bitmasks at the output resolution (ops.paste_masks: [d2] paste_masks_in_image); pred_keypoints
    (k, K, 3) have x and y multiplied by the scale factors (scores as they are) and lose the rows of dropped boxes, as the
    pred_keypoint_heatmaps do, which are otherwise passed through."""
    sx, sy = output_width / results.image_size[1], output_height / results.image_size[0]
    fields = dict(results.get_fields())
    masks = fields.pop("pred_masks", None)
    kpts, heat = fields.pop("pred_keypoints", None), fields.pop("pred_keypoint_heatmaps", None)
    out = Instances((output_height, output_width), **fields)
    b = out.pred_boxes.clone()
    b.scale(sx, sy)
    b.clip(out.image_size)
    out.pred_boxes = b
    keep = b.nonempty()
    out = out[keep]
    if masks is not None:
        probs = masks[keep.to(masks.device)][:, 0].float().contiguous()
        boxes = out.pred_boxes.tensor.float().to(probs.device).contiguous()
        out.pred_masks = ops.paste_masks(probs, boxes, output_height, output_width, mask_threshold).bool()
    if kpts is not None:
        out.pred_keypoints = kpts[keep.to(kpts.device)] * kpts.new_tensor([sx, sy, 1.0])
    if heat is not None:
        out.pred_keypoint_heatmaps = heat[keep.to(heat.device)]
    return out


@META_ARCH_REGISTRY.register()
class GeneralizedRCNN(_EngineOwner):
    """[d2] GeneralizedRCNN as the reference builds it (train.py:189): backbone + proposal_generator + roi_heads.
    model(list[dict{image,height,width}]) -> list[{"instances": Instances}] in eval mode (train.py:96)."""
    _prefix = ""

    def __init__(self, cfg: CfgNode, class_id: Optional[torch.Tensor] = None):
        super().__init__()
        check_c4_options(cfg)  # (a C4 backbone and Res5ROIHeads come together: ValueError naming both keys)
        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg)
        shapes = self.backbone.output_shape()
        self.proposal_generator = PROPOSAL_GENERATOR_REGISTRY.get(cfg.MODEL.PROPOSAL_GENERATOR.NAME)(cfg, shapes)
        self.roi_heads = ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, shapes, class_id)
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), False)
        self._eng_cfg = engine_cfg_from(cfg)
        self._freeze_at = freeze_at_of(cfg)  # the trainer's (a negative value is refused here, when the model is built)
        self._class_map = class_id
        self._engine_cls = self.roi_heads._engine_cls if isinstance(self.roi_heads, (StandardROIHeads, Res5ROIHeads)) else OpensetRCNNEngine
        self._c4 = isinstance(self.roi_heads, Res5ROIHeads)
        if self._c4:
            self._eng_cfg = dict(self.roi_heads._eng_cfg)
        elif issubclass(self._engine_cls, StandardRCNNEngine):
            self._eng_cfg["pooler_scales"] = self.roi_heads._eng_cfg["pooler_scales"]
        self._trainer = None
        self._hook: Optional[torch.Tensor] = None
        self.sampler_generator = torch.Generator().manual_seed(max(int(cfg.SEED), 0))  # uniform keys replacing torch.randperm (H6)

    @property
    def device(self):
        return self.pixel_mean.device

    def _box_head_precision(self) -> str:
        """The box head's own setting (model.roi_heads.box_head_precision) decides, the model's attribute otherwise."""
        own = self.roi_heads.box_head_precision
        return own if own != "storage" else self.box_head_precision

    def engine(self) -> OpensetRCNNEngine:
        eng = super().engine()
        for child in (self.backbone, self.proposal_generator.rpn_head, self.roi_heads):
            child._shared = eng  # one packed copy of the weights for the whole model
        return eng

    def preprocess_image(self, batched_inputs: List[dict]) -> ImageList:
        images = [(x["image"].to(self.device).float() - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        return ImageList.from_tensors(images, self.backbone.size_divisibility)

    def forward(self, batched_inputs: List[dict]):
        """[d2] GeneralizedRCNN.forward. Eval mode: list[{"instances": Instances}]. Training mode (train.py:135): the dict of the six
        losses, GPU scalars whose sum's .backward() runs the explicit HIP backward of this iteration into the trainer's gradient
        buffer (`solver.build_optimizer(cfg, model).step()` then all-reduces and applies it)."""
        if not self.training:
            return self.inference(batched_inputs)
        self._refuse_c4_training()
        self._refuse_keypoint_training()
        trainer = self.trainer()
        tensors = self._train_tensors(batched_inputs, self.sampler_generator)
        with torch.no_grad():
            # (several ranks: all apply the same verdicts -- those of the updates up to two iterations back -- at the same iteration)
            trainer.poll_overflow(wait=parallel.is_dist(), lag=trainer.MULTI_RANK_LAG if parallel.is_dist() else 0)
            losses, saved = trainer._forward(*tensors[:8], **self._mask_kwargs(tensors))
        names = list(losses)
        outs = _ExplicitBackward.apply(self._grad_hook(), trainer, saved, tensors[0].shape[0], *[losses[k] for k in names])
        trainer.grads_ready = False
        return dict(zip(names, outs))

    def event_scalars(self) -> Dict[str, float]:
        """The ten scalars the reference's training forward puts into EventStorage (rpn/num_{pos,neg}_anchors, rpn/obj_num_{pos,neg}_anchors,
        rpn/num_proposals, roi_head/num_{fg,bg}_samples, softmax_classifier/{cls_accuracy,fg_cls_accuracy,false_negative}) for the last
        training-mode forward of this model (OpensetRCNNTrainer.event_scalars)."""
        return self._trainer.event_scalars() if self._trainer is not None else {}

    def _grad_hook(self) -> torch.Tensor:
        """A 0-d leaf that requires grad: what makes torch call _ExplicitBackward.backward (it receives no gradient itself)."""
        if self._hook is None or self._hook.device != self.device:
            self._hook = torch.zeros((), device=self.device, requires_grad=True)
        return self._hook

    def trainer(self):
        """The trainer behind training-mode forwards, built on first use with the module's current parameters
        (`solver.build_optimizer` sets its learning rate, momentum and weight decay from cfg.SOLVER)."""
        if self._trainer is None:
            self._trainer = self.make_trainer()
        return self._trainer

    def train(self, mode: bool = True):
        """Leaving training mode writes the trained masters back into the module's parameters, so that eval-mode forwards,
        state_dict() and checkpoints see them ([d2] trains the module's parameters in place)."""
        if not mode and self.training and self._trainer is not None:
            self.load_trainer_state(self._trainer, keep_trainer=True)
        return super().train(mode)

    def make_trainer(self, lr: float = 0.005, momentum: float = 0.9, weight_decay: float = 1e-4, loss_scale: float = 1024.0):
        """The training loop body of train.py:132-148 as one object: `losses = trainer.step(...)` replaces
        `loss_dict = model(data); losses.backward(); optimizer.step()` (there is no autograd graph on the HIP path). The trainer
        owns fp32 master copies of this model's trainable parameters (the backbone stages MODEL.BACKBONE.FREEZE_AT leaves
        trainable, un-folded from their FrozenBN; FPN; heads);
        `load_trainer_state(trainer)` writes them back into the module for evaluation / checkpointing."""
        from .train import OpensetRCNNTrainer
        from .train_cascade import CascadeRCNNTrainer
        from .train_std import StandardRCNNTrainer
        self._refuse_c4_training()  # (NotImplementedError naming MODEL.ROI_HEADS.NAME "Res5ROIHeads")
        refuse_deform_training(self._eng_cfg)  # (NotImplementedError naming MODEL.RESNETS.DEFORM_ON_PER_STAGE)
        self._refuse_keypoint_training()
        if self._mask_training() is False:
            raise NotImplementedError(MASK_LOSS_MESSAGE)
        if self.conv_precision != "storage":
            raise ValueError(f"conv_precision {self.conv_precision!r}: the split-precision convolutions are an inference mode; set it back to \"storage\" to train")
        if self.device.type != "cuda":
            raise ops.OsrError("the model must be on the GPU (model.to('cuda')): the HIP path has no CPU fallback")
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        bn = {}
        for k in sd:
            if k.endswith(".norm.weight"):
                pre = k[: -len(".norm.weight")]
                scale = sd[pre + ".norm.weight"] * (sd[pre + ".norm.running_var"] + 1e-5).rsqrt()
                bn[pre] = (sd[pre + ".weight"], scale)
        # class_map: the GraspNet id_map of the PLN / classifier losses (prototype_learning_network.py:80-95) -- without it the
        # trainer would treat dataset ids 0..NUM_KNOWN-1 as the known classes
        if issubclass(self._engine_cls, StandardRCNNEngine):  # the trainer by engine class: Base-RCNN-FPN.yaml's stock heads, or the cascade
            cls = CascadeRCNNTrainer if issubclass(self._engine_cls, CascadeRCNNEngine) else StandardRCNNTrainer
            return cls(fold_frozen_bn(sd), self._eng_cfg, self.kernel_dtype, str(self.device), lr=lr, momentum=momentum,
                       weight_decay=weight_decay, loss_scale=loss_scale, freeze_at=self._freeze_at, frozen_bn=bn,
                       box_head=self._box_head_precision())  # ("split" is refused: ValueError, as engine() does)
        # the trainer's box head multiplies as the model's engine does: a model evaluated with box_head_precision="split" trains that way
        return OpensetRCNNTrainer(fold_frozen_bn(sd), self._eng_cfg, self.kernel_dtype, str(self.device), lr=lr, momentum=momentum,
                                  weight_decay=weight_decay, loss_scale=loss_scale, freeze_at=self._freeze_at, frozen_bn=bn,
                                  class_map=self._class_map, box_head=self._box_head_precision())

    def load_trainer_state(self, trainer, keep_trainer: bool = False) -> None:
        sd = dict(self.state_dict())
        for k, v in trainer.export_state_dict().items():
            assert k in sd and tuple(sd[k].shape) == tuple(v.shape), k
            sd[k] = v
        kept = self._trainer if keep_trainer else None
        self.load_state_dict(sd)
        self._trainer = kept  # (load_state_dict drops a cached trainer: its masters would no longer match the module)

    def refresh(self):
        super().refresh()
        self._trainer = None
        for child in (self.backbone, self.proposal_generator.rpn_head, self.roi_heads):
            child._shared = None
            child.refresh()

    def _stack_images(self, imgs: List[torch.Tensor]):
        """One (N,3,H,W) device tensor for a list of CHW images: same-size uint8/float32 images are stacked as they are (the
        fused normalise+pad kernel takes both); a ragged batch is padded bottom/right with the pixel mean, so that the
        normalised padding is exactly zero, as ImageList.from_tensors does after normalisation ([d2])."""
        sizes = [(int(i.shape[-2]), int(i.shape[-1])) for i in imgs]
        if len(set(sizes)) == 1 and len(set(i.dtype for i in imgs)) == 1 and imgs[0].dtype in (torch.uint8, torch.float32):
            return torch.stack([i.to(self.device) for i in imgs]), sizes
        hm, wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
        batch = self.pixel_mean.to(self.device).float().expand(3, hm, wm).unsqueeze(0).repeat(len(imgs), 1, 1, 1)
        for k, im in enumerate(imgs):
            batch[k, :, : sizes[k][0], : sizes[k][1]] = im.to(self.device).float()
        return batch, sizes

    def _train_tensors(self, batched_inputs: List[dict], generator: Optional[torch.Generator] = None):
        """The tensors a training iteration consumes: stacked images, their true sizes, the padded size, ground truth padded to
        the batch maximum, and the uniform keys that replace torch.randperm in the two samplers (seeded by `generator`)."""
        ecfg = {**DEFAULT_CFG, **self._eng_cfg}
        batch, sizes = self._stack_images([x["image"] for x in batched_inputs])
        n, dev = len(sizes), self.device
        hm, wm = int(batch.shape[-2]), int(batch.shape[-1])
        planes = None
        if self._mask_training():  # (bitmask ground truth: planes padded to the batch's image size)
            gt, gcls, gcnt, planes = pad_ground_truth([x["instances"] for x in batched_inputs], (hm, wm))
        else:
            gt, gcls, gcnt = pad_ground_truth([x["instances"] for x in batched_inputs])
        gmax = gt.shape[1]
        d = ecfg["size_divisibility"]
        hp, wp = (hm + d - 1) // d * d, (wm + d - 1) // d * d
        shapes = [((hp // s), (wp // s)) for s in ecfg["fpn_strides"][:4]]
        shapes.append(((shapes[-1][0] - 1) // 2 + 1, (shapes[-1][1] - 1) // 2 + 1))
        r = sum(a * b for a, b in shapes)
        cap = sum(min(ecfg["pre_nms_topk_train"], a * b) for a, b in shapes)
        if issubclass(self._engine_cls, StandardRCNNEngine):  # A anchors per location; the RoI heads sample from the POST_NMS_TOPK_TRAIN list
            r *= len(ecfg["anchor_ratios"])
            cap = ecfg["post_nms_topk_train"]
        # (the stock RPN has one label set: no objectness keys)
        kinds = (("rpn_reg", (n, r)), ("roi", (n, cap + gmax))) if issubclass(self._engine_cls, StandardRCNNEngine) else \
            (("rpn_reg", (n, r)), ("rpn_obj", (n, r)), ("roi", (n, cap + gmax)))
        keys = {k: torch.rand(shape, generator=generator).to(dev) for k, shape in kinds}
        hw = torch.tensor(sizes, dtype=torch.int32, device=dev)
        out = (batch, hw, hp, wp, gt.to(dev), gcls.to(dev), gcnt.to(dev), keys)
        return out if planes is None else out + (planes.to(dev),)  # (a ninth tensor only when the mask branch trains)

    def _refuse_c4_training(self) -> None:
        if getattr(self, "_c4", False):
            raise NotImplementedError(C4_TRAINING_MESSAGE)

    def _refuse_keypoint_training(self) -> None:
        if getattr(self.roi_heads, "keypoint_on", False):
            raise NotImplementedError(KEYPOINT_LOSS_MESSAGE)

    def _mask_training(self) -> Optional[bool]:
        """None: the model has no mask branch; True: it trains (INPUT.MASK_FORMAT "bitmask"); False: training is refused."""
        if not getattr(self.roi_heads, "mask_on", False):
            return None
        return self.roi_heads.mask_format == "bitmask"

    @staticmethod
    def _mask_kwargs(tensors) -> dict:
        """_train_tensors' ninth tensor as the trainer's / engine's keyword."""
        return {"gt_masks": tensors[8]} if len(tensors) > 8 else {}

    @torch.no_grad()
    def losses_forward(self, batched_inputs: List[dict], generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """The loss dict GeneralizedRCNN.forward returns in training mode ([d2]; train.py:189 trainer loop), forward values
        only: loss_rpn_loc, loss_rpn_ctr, loss_box_reg, loss_iou, loss_dml, loss_cls. Each input dict carries "image" and
        "instances" (gt_boxes: Boxes, gt_classes); a ragged batch is padded to its largest image. `generator` seeds the
        uniform keys that replace torch.randperm in the two samplers."""
        self._refuse_c4_training()
        refuse_deform_training(self._eng_cfg)
        self._refuse_keypoint_training()
        if self._mask_training() is False:
            raise NotImplementedError(MASK_LOSS_MESSAGE)
        tensors = self._train_tensors(batched_inputs, generator)
        out = self.engine().forward_losses(*tensors[:8], **self._mask_kwargs(tensors))
        return {k: v for k, v in out.items() if k.startswith("loss_")}

    @torch.no_grad()
    def train_step(self, trainer, batched_inputs: List[dict], generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """One iteration of train.py:132-148 on the trainer made by make_trainer(): forward, explicit backward, gradient
        all-reduce over the ranks and the SGD update; returns the loss dict (GPU scalars, this rank's values)."""
        tensors = self._train_tensors(batched_inputs, generator)
        out = trainer.step(*tensors[:8], **self._mask_kwargs(tensors))
        return {k: v for k, v in out.items() if k.startswith("loss_")}

    @torch.no_grad()
    def inference(self, batched_inputs: List[dict], detected_instances: Optional[List[Instances]] = None, do_postprocess: bool = True):
        """[d2] GeneralizedRCNN.inference. detected_instances (one Instances with pred_boxes / pred_classes per input, in the model
        input's coordinates): the box branch is skipped, the instances are returned as given with pred_masks from the mask head on
        those boxes (unchanged by a model without one) -- StandardROIHeads only."""
        eng = self.engine()
        batch, sizes = self._stack_images([x["image"] for x in batched_inputs])
        if detected_instances is not None:
            if not isinstance(self.roi_heads, StandardROIHeads):
                raise ValueError("detected_instances: StandardROIHeads only (the Openset heads have no forward_with_given_boxes)")
            if len(detected_instances) != len(batched_inputs):
                raise ValueError(f"detected_instances: {len(detected_instances)} Instances for {len(batched_inputs)} inputs")
            insts = list(detected_instances)
            if self.roi_heads.mask_on or self.roi_heads.keypoint_on:
                d = eng.cfg["size_divisibility"]
                hp, wp = (int(batch.shape[-2]) + d - 1) // d * d, (int(batch.shape[-1]) + d - 1) // d * d
                insts = StandardROIHeads._attach_branches(eng, eng._backbone(batch, hp, wp), insts)
            if do_postprocess:
                insts = [detector_postprocess(r, int(inp.get("height", s[0])), int(inp.get("width", s[1])))
                         for r, inp, s in zip(insts, batched_inputs, sizes)]
            return [{"instances": r} for r in insts]
        res = eng.forward(batch, sizes)
        if len(res) > 4:  # mask / keypoint head: their outputs follow the boxes through the per-image postprocess (paste; scale)
            insts = [_std_instances(s, r) for r, s in zip(OpensetRCNNEngine.to_instances(res, len(sizes), eng.output_fields()), sizes)]
            if do_postprocess:
                insts = [detector_postprocess(r, int(inp.get("height", s[0])), int(inp.get("width", s[1])))
                         for r, inp, s in zip(insts, batched_inputs, sizes)]
            return [{"instances": r} for r in insts]
        if do_postprocess:  # [d2] detector_postprocess on the device: rescale, clip, drop empties
            outs = [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) for inp, s in zip(batched_inputs, sizes)]
            scale = torch.tensor([[ow / s[1], oh / s[0]] for (oh, ow), s in zip(outs, sizes)], dtype=torch.float32, device=self.device)
            res = ops.detector_postprocess(res[0], res[1], res[2], res[3], scale, torch.tensor(outs, dtype=torch.int32, device=self.device))
        else:
            outs = sizes
        insts = OpensetRCNNEngine.to_instances(res, len(sizes))
        return [{"instances": Instances(o, pred_boxes=Boxes(r["pred_boxes"]), scores=r["scores"], pred_classes=r["pred_classes"])}
                for r, o in zip(insts, outs)]


# ---------------------------------------------------------------------------------------------------------------
# ProposalNetwork
# ---------------------------------------------------------------------------------------------------------------
PROPOSAL_NETWORK_KEY = 'MODEL.META_ARCHITECTURE "ProposalNetwork"'
PROPOSAL_NETWORK_TRAINING_MESSAGE = (f'{PROPOSAL_NETWORK_KEY} runs at inference only on the HIP path: the trainers are built around the RoI heads\' '
                                     'samplers and losses. Train the GeneralizedRCNN of the same backbone and proposal generator, and load its '
                                     'checkpoint here (the roi_heads.* keys are reported as unexpected)')


@META_ARCH_REGISTRY.register()
class ProposalNetwork(_EngineOwner):
    """[d2] ProposalNetwork: backbone + proposal generator, no RoI heads, under detectron2's parameter names (backbone.*,
    proposal_generator.*). model(list[dict{image,height,width}]) -> list[{"proposals": Instances(proposal_boxes, objectness_logits)}]
    in eval mode: the engine's backbone and RPN stage with the test-time top-k values, then [d2] detector_postprocess for proposals on
    the device (scale to height / width, clip, drop empty boxes). PROPOSAL_GENERATOR.NAME "RPN" on the FPN or the C4 backbone, or
    "ClsFreeRPN" (kernel_dtype float16 / bfloat16 / float32). No RoI-head weight exists, so none is packed."""
    _prefix = ""

    def __init__(self, cfg: CfgNode, class_id: Optional[torch.Tensor] = None):
        super().__init__()
        for on, key in ((cfg.MODEL.MASK_ON, "MODEL.MASK_ON"), (cfg.MODEL.KEYPOINT_ON, "MODEL.KEYPOINT_ON"), (cfg.TEST.AUG.ENABLED, "TEST.AUG")):
            if on:
                raise ValueError(f"{key} with {PROPOSAL_NETWORK_KEY}: a proposal network has no RoI heads, so no mask or keypoint branch and no "
                                 "detections to augment")
        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg)  # (a C4 backbone checks its own keys: PRE_NMS_TOPK_TEST <= 8192)
        self.proposal_generator = PROPOSAL_GENERATOR_REGISTRY.get(cfg.MODEL.PROPOSAL_GENERATOR.NAME)(cfg, self.backbone.output_shape())
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), False)
        head = self.proposal_generator.rpn_head
        self._eng_cfg = dict(head._eng_cfg)  # the proposal generator's own engine: the stock RPN's, the C4 RPN's or the CF-RPN's
        self._engine_cls = head._engine_cls

    @property
    def device(self):
        return self.pixel_mean.device

    _stack_images = GeneralizedRCNN._stack_images

    def engine(self) -> OpensetRCNNEngine:
        eng = super().engine()
        for child in (self.backbone, self.proposal_generator.rpn_head):
            child._shared = eng  # one packed copy of the weights for the whole model
        return eng

    def refresh(self):
        super().refresh()
        for child in (self.backbone, self.proposal_generator.rpn_head):
            child._shared = None
            child.refresh()

    def forward(self, batched_inputs: List[dict]):
        if self.training:
            raise NotImplementedError(PROPOSAL_NETWORK_TRAINING_MESSAGE)
        return self.inference(batched_inputs)

    def make_trainer(self, *a, **k):
        raise NotImplementedError(PROPOSAL_NETWORK_TRAINING_MESSAGE)

    def trainer(self):
        raise NotImplementedError(PROPOSAL_NETWORK_TRAINING_MESSAGE)

    def losses_forward(self, *a, **k):
        raise NotImplementedError(PROPOSAL_NETWORK_TRAINING_MESSAGE)

    @torch.no_grad()
    def inference(self, batched_inputs: List[dict], do_postprocess: bool = True):
        """[d2] ProposalNetwork.forward. do_postprocess=False: the proposals as the RPN stage leaves them, in the model input's
        coordinates. One D2H copy (the counts): the list-of-Instances form needs the lengths on the host."""
        eng = self.engine()
        batch, sizes = self._stack_images([x["image"] for x in batched_inputs])
        d = eng.cfg["size_divisibility"]
        hp, wp = (int(batch.shape[-2]) + d - 1) // d * d, (int(batch.shape[-1]) + d - 1) // d * d
        image_hw = torch.tensor(sizes, dtype=torch.int32).to(self.device, non_blocking=True)
        sel = eng._rpn(eng._backbone(batch, hp, wp), image_hw)
        n, cap = len(sizes), int(sel["cap"])
        boxes, logits, counts = sel["boxes"].view(n, cap, 4), sel["scores"].view(n, cap), sel["counts"]
        outs = sizes
        if do_postprocess:
            outs = [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) for inp, s in zip(batched_inputs, sizes)]
            scale = torch.tensor([[ow / s[1], oh / s[0]] for (oh, ow), s in zip(outs, sizes)], dtype=torch.float32, device=self.device)
            boxes, logits, _, counts = ops.detector_postprocess(boxes.contiguous(), logits.contiguous(), torch.zeros((n, cap), dtype=torch.int64, device=self.device),
                                                                counts, scale, torch.tensor(outs, dtype=torch.int32, device=self.device))
        host = counts.cpu().tolist()
        return [{"proposals": Instances(o, proposal_boxes=Boxes(boxes[i, :host[i]]), objectness_logits=logits[i, :host[i]])} for i, o in enumerate(outs)]


# ---------------------------------------------------------------------------------------------------------------
# RetinaNet
# ---------------------------------------------------------------------------------------------------------------
class LastLevelP6P7(nn.Module):
    """[d2] v0.6 LastLevelP6P7: p6 = conv3x3/2(res5), p7 = conv3x3/2(relu(p6))."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.p6 = _ConvBias(in_channels, out_channels, 3, 0.7)
        self.p7 = _ConvBias(out_channels, out_channels, 3, 0.7)


class RetinaNetResNetFPN(_EngineOwner):
    """[d2] build_retinanet_resnet_fpn_backbone for R-50 (Base-RetinaNet.yaml): laterals and output convs on res3..res5 only (no
    fpn_lateral2 / fpn_output2), top block LastLevelP6P7 fed from res5; forward(x) -> p3..p7."""
    _prefix = "backbone."
    _engine_cls = RetinaNetEngine

    def __init__(self, cfg: CfgNode):
        super().__init__()
        assert cfg.MODEL.RESNETS.DEPTH == 50, "only R-50 is on the hot path"
        assert cfg.MODEL.RESNETS.NORM == "FrozenBN", "only FrozenBN is on the hot path"
        if list(cfg.MODEL.FPN.IN_FEATURES) != ["res3", "res4", "res5"]:
            raise ValueError(f"MODEL.FPN.IN_FEATURES {list(cfg.MODEL.FPN.IN_FEATURES)!r}: build_retinanet_resnet_fpn_backbone reads res3, res4, res5")
        deform = deform_options_from(cfg)
        self.bottom_up = _BottomUp(deform["deform_on_per_stage"], ops.deform_offset_channels(deform["deform_num_groups"], deform["deform_modulated"]))
        self._eng_cfg = {"stride_in_1x1": bool(cfg.MODEL.RESNETS.STRIDE_IN_1X1), **deform}
        for lvl, c in zip((3, 4, 5), (512, 1024, 2048)):
            setattr(self, f"fpn_lateral{lvl}", _ConvBias(c, 256, 1, 0.7))
            setattr(self, f"fpn_output{lvl}", _ConvBias(256, 256, 3, 0.7))
        self.top_block = LastLevelP6P7(2048, 256)
        self._out_features = list(RETINA_PYRAMID)
        self.size_divisibility = 32

    def output_shape(self) -> Dict[str, ShapeSpec]:
        return {f"p{l}": ShapeSpec(channels=256, stride=2 ** l) for l in range(3, 8)}

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        n, _, h, w = x.shape
        assert h % 32 == 0 and w % 32 == 0, "pad the batch to a multiple of 32 (ImageList.from_tensors(..., 32))"
        feats = self.engine()._backbone(x.float().contiguous(), h, w, normalized=True)
        return {k: v.permute(0, 3, 1, 2) for k, v in feats.items()}


@BACKBONE_REGISTRY.register()
def build_retinanet_resnet_fpn_backbone(cfg: CfgNode, input_shape=None):
    return RetinaNetResNetFPN(cfg)


class RetinaNetHead(nn.Module):
    """[d2] RetinaNetHead under its parameter names: cls_subnet / bbox_subnet of NUM_CONVS x (3x3 conv 256 -> 256, ReLU) shared across
    the levels (cls_subnet.{0,2,4,6}), cls_score (3x3, 256 -> A*K), bbox_pred (3x3, 256 -> A*4). Weights N(0, 0.01), zero bias,
    cls_score.bias = -log((1 - PRIOR_PROB) / PRIOR_PROB)."""

    def __init__(self, cfg: CfgNode, input_shape: List[ShapeSpec], num_anchors: int):
        super().__init__()
        rn = cfg.MODEL.RETINANET
        ch = input_shape[0].channels
        assert ch == 256 and len(set(s.channels for s in input_shape)) == 1, "the head reads 256 channels on every level"
        for name in ("cls_subnet", "bbox_subnet"):
            layers = []
            for _ in range(int(rn.NUM_CONVS)):
                layers += [nn.Conv2d(ch, ch, 3, padding=1), nn.ReLU()]
            setattr(self, name, nn.Sequential(*layers))
        self.cls_score = nn.Conv2d(ch, num_anchors * int(rn.NUM_CLASSES), 3, padding=1)
        self.bbox_pred = nn.Conv2d(ch, num_anchors * 4, 3, padding=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.cls_score.bias, -math.log((1 - rn.PRIOR_PROB) / rn.PRIOR_PROB))


def retinanet_engine_cfg_from(cfg: CfgNode) -> dict:
    rn = cfg.MODEL.RETINANET
    return dict(pixel_mean=tuple(cfg.MODEL.PIXEL_MEAN), pixel_std=tuple(cfg.MODEL.PIXEL_STD), stride_in_1x1=bool(cfg.MODEL.RESNETS.STRIDE_IN_1X1),
                **deform_options_from(cfg), anchor_ratios=tuple(float(r) for r in cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS[0]),
                retina_anchor_sizes=tuple(tuple(float(v) for v in s) for s in cfg.MODEL.ANCHOR_GENERATOR.SIZES),
                retina_num_classes=int(rn.NUM_CLASSES), retina_num_convs=int(rn.NUM_CONVS), retina_score_thresh=float(rn.SCORE_THRESH_TEST),
                retina_topk=int(rn.TOPK_CANDIDATES_TEST), retina_nms_thresh=float(rn.NMS_THRESH_TEST),
                retina_bbox_reg_weights=tuple(float(v) for v in rn.BBOX_REG_WEIGHTS), std_detections_per_image=int(cfg.TEST.DETECTIONS_PER_IMAGE))


@META_ARCH_REGISTRY.register()
class RetinaNet(_EngineOwner):
    """[d2] RetinaNet (configs/retinanet_fpn.yaml): backbone (p3..p7) + RetinaNetHead, at inference. model(list[dict{image, height,
    width}]) -> list[{"instances": Instances(pred_boxes, scores, pred_classes)}] in eval mode. Training mode, make_trainer() and
    losses_forward raise NotImplementedError naming the meta architecture; TEST.AUG, MASK_ON, KEYPOINT_ON, RETINANET.NORM and
    conv_precision "split" are ValueErrors."""
    _prefix = ""
    _engine_cls = RetinaNetEngine
    TTA_MESSAGE = ('TEST.AUG: test-time augmentation is implemented for META_ARCHITECTURE "GeneralizedRCNN" with StandardROIHeads only, not for '
                   'META_ARCHITECTURE "RetinaNet"')

    def __init__(self, cfg: CfgNode, class_id: Optional[torch.Tensor] = None):
        super().__init__()
        rn = cfg.MODEL.RETINANET
        if rn.NORM != "":
            raise ValueError(f"MODEL.RETINANET.NORM {rn.NORM!r}: the head's convolutions have no normalisation on the HIP path (\"\")")
        if cfg.MODEL.MASK_ON or cfg.MODEL.KEYPOINT_ON:
            raise ValueError('MODEL.MASK_ON / MODEL.KEYPOINT_ON with META_ARCHITECTURE "RetinaNet": a one-stage detector has no mask or keypoint head')
        if cfg.TEST.AUG.ENABLED:
            raise ValueError(self.TTA_MESSAGE)
        if list(rn.IN_FEATURES) != list(RETINA_PYRAMID):
            raise ValueError(f"MODEL.RETINANET.IN_FEATURES {list(rn.IN_FEATURES)!r}: the HIP path reads {list(RETINA_PYRAMID)}")
        if int(rn.NUM_CONVS) < 0 or int(rn.NUM_CLASSES) < 1 or int(rn.TOPK_CANDIDATES_TEST) < 1:
            raise ValueError("MODEL.RETINANET: NUM_CONVS >= 0, NUM_CLASSES >= 1, TOPK_CANDIDATES_TEST >= 1")
        if int(rn.TOPK_CANDIDATES_TEST) > 2048:
            raise ValueError(f"MODEL.RETINANET.TOPK_CANDIDATES_TEST {rn.TOPK_CANDIDATES_TEST}: at most 2048 per level on the HIP path")
        self.num_anchors = check_retina_anchors(cfg.MODEL.ANCHOR_GENERATOR.SIZES, cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS[0])
        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg)
        shapes = self.backbone.output_shape()
        missing = [f for f in rn.IN_FEATURES if f not in shapes]
        if missing:
            raise ValueError(f"MODEL.BACKBONE.NAME {cfg.MODEL.BACKBONE.NAME!r} has no {missing}: RetinaNet needs build_retinanet_resnet_fpn_backbone")
        self.head = RetinaNetHead(cfg, [shapes[f] for f in rn.IN_FEATURES], self.num_anchors)
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), False)
        self._eng_cfg = retinanet_engine_cfg_from(cfg)
        self.num_classes = int(rn.NUM_CLASSES)

    @property
    def device(self):
        return self.pixel_mean.device

    def engine(self) -> RetinaNetEngine:
        eng = super().engine()
        self.backbone._shared = eng  # one packed copy of the weights for the whole model
        return eng

    def refresh(self):
        super().refresh()
        self.backbone._shared = None
        self.backbone.refresh()

    def forward(self, batched_inputs: List[dict]):
        if self.training:
            raise NotImplementedError(RETINANET_TRAINING_MESSAGE)
        return self.inference(batched_inputs)

    def make_trainer(self, *a, **k):
        raise NotImplementedError(RETINANET_TRAINING_MESSAGE)

    trainer = make_trainer  # (run_net.py's training loop asks for model.trainer())

    def losses_forward(self, *a, **k):
        raise NotImplementedError(RETINANET_TRAINING_MESSAGE)

    @torch.no_grad()
    def inference(self, batched_inputs: List[dict], do_postprocess: bool = True):
        """[d2] RetinaNet.inference + detector_postprocess on the device (rescale to each input's height / width, clip, drop empties)."""
        eng = self.engine()
        batch, sizes = GeneralizedRCNN._stack_images(self, [x["image"] for x in batched_inputs])
        res = eng.forward(batch, sizes)
        outs = [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) if do_postprocess else s for inp, s in zip(batched_inputs, sizes)]
        # (without postprocessing the boxes are still clipped to the image: [d2] v0.6 clips nowhere else)
        scale = torch.tensor([[ow / s[1], oh / s[0]] for (oh, ow), s in zip(outs, sizes)], dtype=torch.float32, device=self.device)
        res = ops.detector_postprocess(res[0], res[1], res[2], res[3], scale, torch.tensor(outs, dtype=torch.int32, device=self.device))
        insts = OpensetRCNNEngine.to_instances(res, len(sizes))
        return [{"instances": Instances(o, pred_boxes=Boxes(r["pred_boxes"]), scores=r["scores"], pred_classes=r["pred_classes"])}
                for r, o in zip(insts, outs)]


# ---------------------------------------------------------------------------------------------------------------
# Panoptic FPN
# ---------------------------------------------------------------------------------------------------------------
class _ConvGN(nn.Module):
    """A bias-free 3x3 convolution with its GroupNorm(32) under [d2] Conv2d's names: `.weight`, `.norm.weight`, `.norm.bias`."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        self.norm = nn.GroupNorm(32, cout)


class _Conv3x3(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        self.bias = nn.Parameter(torch.zeros(cout))


class SemSegFPNHead(nn.Module):
    """[d2] SemSegFPNHead under its parameter names: per input feature of stride s, head_length = max(1, log2(s) - log2(COMMON_STRIDE))
    times (3x3 conv, NORM, ReLU, and a bilinear x2 where s != COMMON_STRIDE) as a Sequential whose even entries are the convolutions
    (`<feat>.<2k>.weight`, `.norm.*` with NORM "GN", `.bias` with NORM "") and whose odd entries are the parameterless upsamples; the
    results are summed and a 1x1 `predictor` gives NUM_CLASSES logits at COMMON_STRIDE. c2_msra_fill; GroupNorm weight 1, bias 0."""

    def __init__(self, cfg: CfgNode, input_shape: Dict[str, ShapeSpec]):
        super().__init__()
        h = cfg.MODEL.SEM_SEG_HEAD
        check_sem_seg_options(h.NAME, h.IN_FEATURES, h.NUM_CLASSES, h.CONVS_DIM, h.COMMON_STRIDE, h.NORM)
        self.in_features = list(h.IN_FEATURES)
        missing = [f for f in self.in_features if f not in input_shape]
        if missing:
            raise ValueError(f"MODEL.SEM_SEG_HEAD.IN_FEATURES: MODEL.BACKBONE.NAME {cfg.MODEL.BACKBONE.NAME!r} has no {missing}")
        self.common_stride, self.num_classes, dim = int(h.COMMON_STRIDE), int(h.NUM_CLASSES), int(h.CONVS_DIM)
        for feat in self.in_features:
            stride, cin = input_shape[feat].stride, input_shape[feat].channels
            length = max(1, int(math.log2(stride) - math.log2(self.common_stride)))
            layers = []
            for k in range(length):
                layers.append(_ConvGN(cin if k == 0 else dim, dim) if h.NORM == "GN" else _Conv3x3(cin if k == 0 else dim, dim))
                nn.init.kaiming_normal_(layers[-1].weight, mode="fan_out", nonlinearity="relu")
                if stride != self.common_stride:
                    layers.append(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))
            setattr(self, feat, nn.Sequential(*layers))
        self.predictor = nn.Conv2d(dim, self.num_classes, 1)
        nn.init.kaiming_normal_(self.predictor.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.predictor.bias, 0)


def sem_seg_engine_cfg_from(cfg: CfgNode) -> dict:
    h, comb = cfg.MODEL.SEM_SEG_HEAD, cfg.MODEL.PANOPTIC_FPN.COMBINE
    return dict(sem_seg_num_classes=int(h.NUM_CLASSES), sem_seg_convs_dim=int(h.CONVS_DIM), sem_seg_norm=str(h.NORM), sem_seg_common_stride=int(h.COMMON_STRIDE),
                combine_overlap_thresh=float(comb.OVERLAP_THRESH), combine_stuff_area_limit=int(comb.STUFF_AREA_LIMIT),
                combine_instances_confidence_thresh=float(comb.INSTANCES_CONFIDENCE_THRESH))


def _refuse_sem_seg_extras(cfg: CfgNode, meta_arch: str) -> str:
    """The refusals the two semantic meta architectures share; -> the TEST.AUG message."""
    msg = ('TEST.AUG: test-time augmentation is implemented for META_ARCHITECTURE "GeneralizedRCNN" with StandardROIHeads only, not for '
           f'META_ARCHITECTURE "{meta_arch}"')
    if cfg.MODEL.KEYPOINT_ON:
        raise ValueError("MODEL.KEYPOINT_ON: the HIP path has no keypoint head (box, mask and semantic branches only)")
    if cfg.TEST.AUG.ENABLED:
        raise ValueError(msg)
    return msg


def _sem_seg_outputs(eng, logits: torch.Tensor, num_classes: int, sizes, outs):
    """[d2] sem_seg_postprocess per image from the stride-4 logits: (C, oh, ow) fp32."""
    return [ops.semseg_resample(logits[i], num_classes, s, o, labels=False) for i, (s, o) in enumerate(zip(sizes, outs))]


@META_ARCH_REGISTRY.register()
class SemanticSegmentor(_EngineOwner):
    """[d2] SemanticSegmentor: backbone + SemSegFPNHead at inference. model(list[dict{image, height, width}]) ->
    list[{"sem_seg": (NUM_CLASSES, height, width) fp32 logits}] in eval mode. Training mode, make_trainer(), trainer() and
    losses_forward raise NotImplementedError naming the meta architecture."""
    _prefix = ""
    _engine_cls = PanopticFPNEngine
    META_ARCH = "SemanticSegmentor"

    def __init__(self, cfg: CfgNode, class_id: Optional[torch.Tensor] = None):
        super().__init__()
        self.TTA_MESSAGE = _refuse_sem_seg_extras(cfg, self.META_ARCH)
        self.backbone = BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg)
        self.sem_seg_head = SemSegFPNHead(cfg, self.backbone.output_shape())
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), False)
        self._eng_cfg = dict(pixel_mean=tuple(cfg.MODEL.PIXEL_MEAN), pixel_std=tuple(cfg.MODEL.PIXEL_STD), stride_in_1x1=bool(cfg.MODEL.RESNETS.STRIDE_IN_1X1),
                             **deform_options_from(cfg), **sem_seg_engine_cfg_from(cfg))
        self.num_classes = int(cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES)

    @property
    def device(self):
        return self.pixel_mean.device

    def engine(self) -> PanopticFPNEngine:
        eng = super().engine()
        self.backbone._shared = eng  # one packed copy of the weights for the whole model
        return eng

    def refresh(self):
        super().refresh()
        self.backbone._shared = None
        self.backbone.refresh()

    def forward(self, batched_inputs: List[dict]):
        if self.training:
            raise NotImplementedError(panoptic_training_message(self.META_ARCH))
        return self.inference(batched_inputs)

    def make_trainer(self, *a, **k):
        raise NotImplementedError(panoptic_training_message(self.META_ARCH))

    trainer = make_trainer

    def losses_forward(self, *a, **k):
        raise NotImplementedError(panoptic_training_message(self.META_ARCH))

    @torch.no_grad()
    def inference(self, batched_inputs: List[dict]):
        eng = self.engine()
        batch, sizes = GeneralizedRCNN._stack_images(self, [x["image"] for x in batched_inputs])
        (logits,) = eng.forward(batch, sizes)
        outs = [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) for inp, s in zip(batched_inputs, sizes)]
        return [{"sem_seg": r} for r in _sem_seg_outputs(eng, logits, self.num_classes, sizes, outs)]


@META_ARCH_REGISTRY.register()
class PanopticFPN(GeneralizedRCNN):
    """[d2] PanopticFPN (configs/panoptic_fpn.yaml): GeneralizedRCNN with StandardROIHeads (MASK_ON) plus SemSegFPNHead, at inference.
    model(list[dict{image, height, width}]) -> list[{"sem_seg": (C, H, W) fp32 logits, "instances": Instances, "panoptic_seg":
    ((H, W) int32, segments_info)}] in eval mode; "panoptic_seg" only with MODEL.PANOPTIC_FPN.COMBINE.ENABLED. segments_info is [d2]'s
    list of dicts (things: id, isthing, score, category_id, instance_id; stuff: id, isthing, category_id, area). Training mode,
    make_trainer(), trainer() and losses_forward raise NotImplementedError naming the meta architecture."""
    META_ARCH = "PanopticFPN"

    def __init__(self, cfg: CfgNode, class_id: Optional[torch.Tensor] = None):
        tta_message = _refuse_sem_seg_extras(cfg, self.META_ARCH)
        comb = cfg.MODEL.PANOPTIC_FPN.COMBINE
        if cfg.MODEL.ROI_HEADS.NAME != "StandardROIHeads":
            raise ValueError(f'MODEL.ROI_HEADS.NAME {cfg.MODEL.ROI_HEADS.NAME!r} with META_ARCHITECTURE "PanopticFPN": the HIP path combines the '
                             'detections of "StandardROIHeads" only')
        if comb.ENABLED and not cfg.MODEL.MASK_ON:
            raise ValueError("MODEL.PANOPTIC_FPN.COMBINE.ENABLED needs MODEL.MASK_ON True: the panoptic map is painted from the instance masks")
        super().__init__(cfg, class_id)
        self.TTA_MESSAGE = tta_message
        self.sem_seg_head = SemSegFPNHead(cfg, self.backbone.output_shape())
        self._engine_cls = PanopticFPNEngine
        self._eng_cfg.update(sem_seg_engine_cfg_from(cfg))
        self._eng_cfg.update({k: v for k, v in self.roi_heads._eng_cfg.items() if k.startswith("mask_pooler_")})
        self.combine_enabled = bool(comb.ENABLED)
        self.sem_num_classes = int(cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES)

    def forward(self, batched_inputs: List[dict]):
        if self.training:
            raise NotImplementedError(panoptic_training_message(self.META_ARCH))
        return self.inference(batched_inputs)

    def make_trainer(self, *a, **k):
        raise NotImplementedError(panoptic_training_message(self.META_ARCH))

    def trainer(self, *a, **k):
        raise NotImplementedError(panoptic_training_message(self.META_ARCH))

    def losses_forward(self, *a, **k):
        raise NotImplementedError(panoptic_training_message(self.META_ARCH))

    @torch.no_grad()
    def inference(self, batched_inputs: List[dict], do_postprocess: bool = True):
        """[d2] PanopticFPN.inference: the stock detector with its device postprocess (masks pasted at the requested size), the semantic
        logits resampled from stride 4 by one kernel per image, and combine_semantic_and_instance_outputs on the device."""
        eng = self.engine()
        c = eng.cfg
        batch, sizes = self._stack_images([x["image"] for x in batched_inputs])
        res = eng.forward(batch, sizes)
        dets, logits = res[:-1], res[-1]
        outs = [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) if do_postprocess else s for inp, s in zip(batched_inputs, sizes)]
        insts = [_std_instances(s, r) for r, s in zip(OpensetRCNNEngine.to_instances(dets, len(sizes)), sizes)]
        insts = [detector_postprocess(r, o[0], o[1]) for r, o in zip(insts, outs)]
        sem = _sem_seg_outputs(eng, logits, self.sem_num_classes, sizes, outs)
        results = []
        for i, (r, s, o) in enumerate(zip(insts, sizes, outs)):
            out = {"sem_seg": sem[i], "instances": r}
            if self.combine_enabled:
                labels = ops.semseg_resample(logits[i], self.sem_num_classes, s, o, labels=True)
                dev = labels.device
                pan, table, scores, count = ops.panoptic_combine(r.pred_masks.contiguous(), r.scores.float().to(dev).contiguous(),
                                                                 r.pred_classes.to(torch.int64).to(dev).contiguous(), labels, c["combine_overlap_thresh"],
                                                                 c["combine_stuff_area_limit"], c["combine_instances_confidence_thresh"])
                out["panoptic_seg"] = (pan, ops.segments_info_from_table(table, scores, count))
            results.append(out)
        return results


def build_model(cfg: CfgNode, class_id: Optional[torch.Tensor] = None) -> nn.Module:
    """[d2] detectron2.modeling.build_model (train.py:189)."""
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg, class_id)
    return model.to(torch.device(cfg.MODEL.DEVICE))
