"""Checkpoint import for the HIP path: the two on-disk formats the reference loads --

  * `.pth` written by [d2] DetectionCheckpointer (train.py:113-118, :195-197): torch.save({"model": state_dict, ...}) with
    detectron2 parameter names (the names host/modeling.py's modules own), FrozenBN statistics included;
  * `detectron2://ImageNetPretrained/MSRA/R-50.pkl` (VOC-COCO yaml:3): a pickled {blob name: ndarray} dict in Caffe2 / MSRA
    naming (conv1_w, res_conv1_bn_s, res2_0_branch2a_w, res2_0_branch2a_bn_b, ..., fc1000_w), BN already reduced to a
    scale/shift pair. [d2] loads it through name heuristics; the mapping is closed-form for R-50 and written out below.

and the two forms of torchvision's ImageNet ResNet-50 (stride in the 3x3: build the model with MODEL.RESNETS.STRIDE_IN_1X1
False) --

  * the `.pkl` of detectron2's tools/convert-torchvision-to-d2.py: {"model": {name: ndarray}, "__author__": ...,
    "matching_heuristics": True} with backbone names lacking the `backbone.bottom_up.` prefix (stem.conv1.weight,
    res2.0.conv1.norm.running_var, res2.0.shortcut.weight, stem.fc.weight, ...);
  * the raw `resnet50().state_dict()` saved as `.pth` (conv1 / bn1 / layer{1..4}.{b}.conv{1,2,3} / bn{1,2,3} / downsample.{0,1} / fc).

Both carry real BatchNorm statistics (not pre-reduced like the MSRA blobs); `weights.fold_frozen_bn` folds them.

Checkpoints of the other zoo families ([d2] `.pth`, or the model zoo's `.pkl` = {"model": {name: ndarray}, "__author__": ...} without
"matching_heuristics") load by name as they are: mask_rcnn, cascade, dconv, retinanet_R_50_FPN (backbone.top_block.p6 / p7, head.*) and panoptic_fpn_R_50 (sem_seg_head.*: its
GroupNorm `.norm.weight` / `.norm.bias` carry no running statistics and are not folded) and faster_rcnn_R_50_C4 (backbone.stem.* /
backbone.res{2,3,4}.* without `bottom_up`, roi_heads.res5.*). A backbone-only checkpoint loaded into a C4 model is renamed to those names
(c4_names).

Nothing here reads from the network: paths are local files. The result is a flat {d2 name: fp32 tensor} dict, ready for
`model.load_state_dict` (host/modeling.py) or, after `weights.fold_frozen_bn`, for `OpensetRCNNEngine`."""
from __future__ import annotations

import logging
import pickle
import re
from typing import Dict, Iterable, List, Tuple

import numpy as np
import torch

_BRANCH = {"branch1": "shortcut", "branch2a": "conv1", "branch2b": "conv2", "branch2c": "conv3"}
_BN = {"s": "norm.weight", "b": "norm.bias", "rm": "norm.running_mean", "riv": "norm.running_var"}


def convert_msra_name(name: str) -> str:
    """One Caffe2/MSRA blob name -> the detectron2 backbone parameter name ("" for blobs the detector does not use)."""
    if name.startswith("fc1000") or name.endswith("_momentum"):
        return ""
    m = re.fullmatch(r"conv1_(w|b)", name)
    if m:
        return "backbone.bottom_up.stem.conv1." + ("weight" if m.group(1) == "w" else "bias")
    m = re.fullmatch(r"res_conv1_bn_(s|b|rm|riv)", name)
    if m:
        return "backbone.bottom_up.stem.conv1." + _BN[m.group(1)]
    m = re.fullmatch(r"res(\d)_(\d+)_(branch1|branch2a|branch2b|branch2c)_(w|b|bn_s|bn_b|bn_rm|bn_riv)", name)
    if m:
        stage, blk, br, kind = m.groups()
        leaf = {"w": "weight", "b": "bias"}.get(kind) or _BN[kind[3:]]
        return f"backbone.bottom_up.res{stage}.{int(blk)}.{_BRANCH[br]}.{leaf}"
    raise KeyError(f"unrecognised MSRA/Caffe2 blob name '{name}'")


def convert_msra_state(blobs: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
    """Whole MSRA R-50 dict -> d2-named tensors. BN blobs hold scale/shift only; FrozenBN's running_mean = 0 and
    running_var = 1 - eps make `scale * rsqrt(var + eps)` reproduce the stored scale exactly ([d2] FrozenBatchNorm2d init)."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in blobs.items():
        name = convert_msra_name(k)
        if name:
            out[name] = torch.from_numpy(np.ascontiguousarray(v)).float()
    for k in [k for k in out if k.endswith(".norm.weight")]:
        pre = k[: -len("weight")]
        c = out[k].numel()
        out.setdefault(pre + "running_mean", torch.zeros(c))
        out.setdefault(pre + "running_var", torch.ones(c) - 1e-5)
    return out


_TV_LEAF = {"weight", "bias", "running_mean", "running_var"}
_BOTTOM_UP = "backbone.bottom_up."
log = logging.getLogger(__name__)


class CheckpointState(dict):
    """load_checkpoint's result: {d2 name: tensor}, and `origin`, the format it came from ("d2", "msra" or "torchvision": a
    torchvision ResNet, stride in the 3x3)."""

    def __init__(self, items, origin: str):
        super().__init__(items)
        self.origin = origin


def convert_d2_backbone_name(name: str) -> str:
    """A backbone name of detectron2's converted torchvision `.pkl` (no `backbone.bottom_up.` prefix) -> this model's name
    ("" for the classifier and the BatchNorm step counters, which the detector does not use)."""
    if name.startswith("stem.fc.") or name.endswith(".num_batches_tracked"):
        return ""
    if re.fullmatch(r"stem\.conv1\.(weight|norm\.(weight|bias|running_mean|running_var))", name) or \
            re.fullmatch(r"res[2-5]\.\d+\.(shortcut|conv1|conv2|conv3)\.(weight|norm\.(weight|bias|running_mean|running_var))", name) or \
            re.fullmatch(r"res[2-5]\.\d+\.conv2_offset\.(weight|bias)", name):  # ([d2] DeformBottleneckBlock: bias, no norm)
        return _BOTTOM_UP + name
    raise KeyError(f"unrecognised detectron2 backbone name '{name}'")


def convert_torchvision_name(name: str) -> str:
    """One torchvision resnet50 state-dict name -> this model's name ("" for fc.* and num_batches_tracked)."""
    if name.startswith("fc.") or name.endswith(".num_batches_tracked"):
        return ""
    if name == "conv1.weight":
        return _BOTTOM_UP + "stem.conv1.weight"
    m = re.fullmatch(r"bn1\.(\w+)", name)
    if m and m.group(1) in _TV_LEAF:
        return _BOTTOM_UP + "stem.conv1.norm." + m.group(1)
    m = re.fullmatch(r"layer([1-4])\.(\d+)\.(conv[123]\.weight|bn[123]\.\w+|downsample\.[01]\.\w+)", name)
    if m:
        layer, blk, rest = m.groups()
        pre = f"{_BOTTOM_UP}res{int(layer) + 1}.{blk}."
        mm = re.fullmatch(r"conv([123])\.weight", rest)
        if mm:
            return pre + f"conv{mm.group(1)}.weight"
        mm = re.fullmatch(r"bn([123])\.(\w+)", rest)
        if mm and mm.group(2) in _TV_LEAF:
            return pre + f"conv{mm.group(1)}.norm.{mm.group(2)}"
        if rest == "downsample.0.weight":
            return pre + "shortcut.weight"
        mm = re.fullmatch(r"downsample\.1\.(\w+)", rest)
        if mm and mm.group(1) in _TV_LEAF:
            return pre + "shortcut.norm." + mm.group(1)
    raise KeyError(f"unrecognised torchvision ResNet name '{name}'")


def _is_d2_backbone(names) -> bool:
    return "stem.conv1.weight" in names and any(re.match(r"res[2-5]\.\d+\.", k) for k in names)


def _is_torchvision(names) -> bool:
    return "conv1.weight" in names and "bn1.running_var" in names and any(k.startswith("layer1.0.") for k in names)


def _converted(state: Dict[str, object], convert) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in state.items():
        name = convert(k)
        if name:
            out[name] = (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).float()
    return out


def load_checkpoint(path: str) -> CheckpointState:
    """Read a `.pth` or `.pkl` checkpoint into a flat {d2 name: tensor} dict (fp32, CPU). The format is told by its names:
    a torchvision ResNet (raw or converted by detectron2's tools) is mapped to this model's names."""
    if path.endswith(".pkl"):
        with open(path, "rb") as f:
            data = pickle.load(f, encoding="latin1")
        if isinstance(data, dict) and "model" in data and "__author__" in data:  # already converted by detectron2's tools
            model = data["model"]
            if not data.get("matching_heuristics", False):
                return CheckpointState({k: torch.as_tensor(np.asarray(v)).float() for k, v in model.items()}, "d2")
            if _is_d2_backbone(model):  # tools/convert-torchvision-to-d2.py
                return CheckpointState(_converted(model, convert_d2_backbone_name), "torchvision")
            data = model
        if isinstance(data, dict) and "blobs" in data:
            data = data["blobs"]
        return CheckpointState(convert_msra_state({k: np.asarray(v) for k, v in data.items()}), "msra")
    data = torch.load(path, map_location="cpu", weights_only=False)
    state = data["model"] if isinstance(data, dict) and "model" in data else data
    if _is_torchvision(state):  # torch.save(torchvision.models.resnet50(...).state_dict())
        return CheckpointState(_converted(state, convert_torchvision_name), "torchvision")
    out = {}
    for k, v in state.items():
        k = k[len("module."):] if k.startswith("module.") else k  # DDP-wrapped saves (train.py:201-205)
        out[k] = torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v
        if out[k].is_floating_point():
            out[k] = out[k].float()
    return CheckpointState(out, "d2")


def c4_names(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A backbone-only checkpoint's names (backbone.bottom_up.*: what the MSRA and torchvision converters above produce) as a C4 model
    owns them ([d2] build_resnet_backbone + Res5ROIHeads): stem and res2..res4 directly under `backbone.`, res5 under `roi_heads.`."""
    out = {}
    for k, v in state.items():
        m = re.fullmatch(r"backbone\.bottom_up\.(stem|res[2-5])\.(.+)", k)
        if not m:
            out[k] = v
        elif m.group(1) == "res5":
            out["roi_heads.res5." + m.group(2)] = v
        else:
            out[f"backbone.{m.group(1)}.{m.group(2)}"] = v
    return CheckpointState(out, state.origin) if isinstance(state, CheckpointState) else out


def load_into(model: torch.nn.Module, state: Dict[str, torch.Tensor], strict: bool = False) -> Tuple[List[str], List[str]]:
    """[d2] Checkpointer semantics: load matching names, report (missing, unexpected); shape mismatches raise. A backbone-only
    checkpoint (MSRA R-50) leaves FPN / RPN / RoI-head parameters at their initial values, as in the reference's training
    start. A torchvision checkpoint loaded into a model built with MODEL.RESNETS.STRIDE_IN_1X1 True (the MSRA layout) is
    loaded, with a warning: its weights were trained with the stride in the 3x3."""
    if getattr(state, "origin", None) == "torchvision" and getattr(model, "_eng_cfg", {}).get("stride_in_1x1", True):
        log.warning("loading a torchvision ResNet checkpoint into a model with MODEL.RESNETS.STRIDE_IN_1X1 True: torchvision puts "
                    "the stride in the 3x3 convolution; set STRIDE_IN_1X1 False (detectron2's convert-torchvision-to-d2 recipe)")
    own = model.state_dict()
    if "backbone.stem.conv1.weight" in own and "backbone.bottom_up.stem.conv1.weight" in state:
        state = c4_names(state)  # (a backbone-only checkpoint into a C4 model: res5 is its RoI head's)
    for k, v in state.items():
        if k in own and tuple(own[k].shape) != tuple(v.shape):
            raise ValueError(f"shape mismatch for '{k}': checkpoint {tuple(v.shape)} vs model {tuple(own[k].shape)}")
    missing = [k for k in own if k not in state]
    unexpected = [k for k in state if k not in own]
    if strict and (missing or unexpected):
        raise KeyError(f"missing {missing[:5]}... unexpected {unexpected[:5]}...")
    merged = dict(own)
    merged.update({k: v for k, v in state.items() if k in own})
    model.load_state_dict(merged)
    return missing, unexpected


def msra_names_for(d2_names: Iterable[str]) -> Dict[str, str]:
    """Inverse mapping (d2 backbone name -> MSRA blob name); used by the tests to fabricate an R-50.pkl look-alike."""
    inv_branch = {v: k for k, v in _BRANCH.items()}
    inv_bn = {v: k for k, v in _BN.items()}
    out = {}
    for n in d2_names:
        m = re.fullmatch(r"backbone\.bottom_up\.stem\.conv1\.(.+)", n)
        if m:
            leaf = m.group(1)
            out[n] = "conv1_w" if leaf == "weight" else ("conv1_b" if leaf == "bias" else "res_conv1_bn_" + inv_bn[leaf])
            continue
        m = re.fullmatch(r"backbone\.bottom_up\.res(\d)\.(\d+)\.(shortcut|conv1|conv2|conv3)\.(.+)", n)
        if m:
            stage, blk, br, leaf = m.groups()
            kind = {"weight": "w", "bias": "b"}.get(leaf) or "bn_" + inv_bn[leaf]
            out[n] = f"res{stage}_{blk}_{inv_branch[br]}_{kind}"
    return out
