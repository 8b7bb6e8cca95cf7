"""TEST.AUG: test-time augmentation for the stock heads ([d2] v0.6 modeling/test_time_augmentation.py: DatasetMapperTTA +
GeneralizedRCNNWithTTA), on the device.

Per input dict {"image": (3, hi, wi) uint8, "height": ho, "width": wo}: for every s in TEST.AUG.MIN_SIZES the model input image is
resized with ResizeShortestEdge(s, TEST.AUG.MAX_SIZE) (Pillow BILINEAR) and, with TEST.AUG.FLIP, also mirrored; every augmentation
goes through the detector without its mask branch; the detections are mapped back to (ho, wo), concatenated in augmentation order
and merged by fast_rcnn_inference_single_image(.., 1e-8, NMS_THRESH_TEST, DETECTIONS_PER_IMAGE); with MODEL.MASK_ON the mask branch
then runs on the merged boxes in every augmentation and the maps (those of flipped augmentations mirrored back) are averaged.

Between the upload of a group's images and the merged result everything stays in the engine's padded tensors: resize + flip
(osr_resize_bilinear_u8_planar), box maps (osr_tta_boxes_to_original / _to_augmented), merge (osr_nms_topk + osr_gather_rows) and
mask mean (osr_tta_reduce_masks). The images of one call that share (hi, wi) form a group; a group takes one engine pass per
augmentation over all its images; groups run in order of first appearance and results return in input order."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
from torch import nn

from . import ops
from .data import pil_resample_coeffs, shortest_edge_size
from .engine import OpensetRCNNEngine
from .structures import Boxes, Instances


def tta_augmentations(hi: int, wi: int, ho: int, wo: int, min_sizes: Sequence[int], max_size: int, flip: bool) -> List[Tuple[int, int, bool]]:
    """[d2] DatasetMapperTTA's augmentation list for a model input image of (hi, wi) whose output resolution is (ho, wo):
    (ha, wa, flipped) per augmentation, "resize" then "resize + flip" for every min size in order. The resize acts on the model
    input image, so (ho, wo) only enters the box maps (the leading resize (ho, wo) -> (hi, wi) of each transform list)."""
    del ho, wo
    out = []
    for s in min_sizes:
        ha, wa = shortest_edge_size(int(hi), int(wi), int(s), int(max_size))
        out.append((ha, wa, False))
        if flip:
            out.append((ha, wa, True))
    return out


class GeneralizedRCNNWithTTA(nn.Module):
    """[d2] GeneralizedRCNNWithTTA(cfg, model): wrapper(batched_inputs) -> list[{"instances": Instances}] at each input's
    (height, width). Stock family only: GeneralizedRCNN with RPN + StandardROIHeads, with or without the mask head."""

    def __init__(self, cfg, model):
        super().__init__()
        from .modeling import CascadeROIHeads, GeneralizedRCNN, PanopticFPN, RetinaNet, SemanticSegmentor, StandardROIHeads
        if isinstance(model, RetinaNet):
            raise ValueError(RetinaNet.TTA_MESSAGE)
        if isinstance(model, (PanopticFPN, SemanticSegmentor)):
            raise ValueError(model.TTA_MESSAGE)
        if isinstance(getattr(model, "roi_heads", None), CascadeROIHeads):
            raise ValueError("TEST.AUG: test-time augmentation is not implemented for CascadeROIHeads (the merge re-scores the augmented boxes with "
                             "one box head; a cascade has one per stage)")
        if not isinstance(model, GeneralizedRCNN) or not isinstance(model.roi_heads, StandardROIHeads):
            raise ValueError(f"TEST.AUG: test-time augmentation is implemented for StandardROIHeads only, not {type(getattr(model, 'roi_heads', model)).__name__} "
                             "(the merge indexes a (rows, NUM_CLASSES + 1) score table with the class id, which the Openset heads' unknown id does not fit)")
        if cfg.MODEL.KEYPOINT_ON:
            raise ValueError("TEST.AUG: MODEL.KEYPOINT_ON is not supported (box and mask branches only)")
        if cfg.MODEL.LOAD_PROPOSALS:
            raise ValueError("TEST.AUG: MODEL.LOAD_PROPOSALS is not supported (the augmented inputs carry no precomputed proposals)")
        if model.training:
            raise ValueError("TEST.AUG: the model is in training mode; test-time augmentation is inference only (model.eval())")
        self.cfg = cfg.clone()
        self.model = model
        aug = cfg.TEST.AUG
        self.min_sizes = tuple(int(s) for s in aug.MIN_SIZES)
        self.max_size = int(aug.MAX_SIZE)
        self.flip = bool(aug.FLIP)
        if not self.min_sizes:
            raise ValueError("TEST.AUG.MIN_SIZES is empty")
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self._tables: Dict[tuple, tuple] = {}

    # ---- resize (+ flip) of a stacked group -----------------------------------------------------------------------------------------
    def _axis(self, n_in: int, n_out: int, dev):
        key = (n_in, n_out, str(dev))
        if key not in self._tables:
            b, c = pil_resample_coeffs(n_in, n_out)
            self._tables[key] = (torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev), int(b[0, 0]), int(b[-1, 0] + b[-1, 1]), int(c.shape[1]))
        return self._tables[key]

    def augment(self, images: torch.Tensor, ha: int, wa: int, flipped: bool) -> torch.Tensor:
        """(n, 3, hi, wi) uint8 on the GPU -> (n, 3, ha, wa): Pillow BILINEAR, then the mirror (one launch pair; equal sizes without a
        flip are the images themselves)."""
        hi, wi = int(images.shape[-2]), int(images.shape[-1])
        if (ha, wa) == (hi, wi) and not flipped:
            return images
        xb, xc, _, _, kx = self._axis(wi, wa, images.device)
        yb, yc, y_first, y_last, ky = self._axis(hi, ha, images.device)
        return ops.resize_bilinear_u8_planar(images, xb, xc, kx, yb, yc, ky, y_first, y_last - y_first, ha, wa, mirror=flipped)

    @staticmethod
    def _padded(eng, h: int, w: int) -> Tuple[int, int]:
        d = eng.cfg["size_divisibility"]
        return (h + d - 1) // d * d, (w + d - 1) // d * d

    # ---- one group: images of one (hi, wi) --------------------------------------------------------------------------------------------
    def box_stage(self, eng, images: torch.Tensor, sizes: torch.Tensor, augs):
        """Every augmentation through the detector without its mask branch, the detections mapped to (ho, wo) and merged. -> padded
        (boxes (n, topk, 4), scores, classes int64 with -1 beyond the count, counts)."""
        n, dev = int(images.shape[0]), images.device
        topk = int(eng.cfg["std_detections_per_image"])
        cap = len(augs) * topk
        c_boxes = torch.empty((n, cap, 4), dtype=torch.float32, device=dev)
        c_scores = torch.empty((n, cap), dtype=torch.float32, device=dev)
        c_cls = torch.empty((n, cap), dtype=torch.int32, device=dev)
        c_cand = torch.empty((n, cap), dtype=torch.int32, device=dev)
        for a, (ha, wa, fl) in enumerate(augs):
            img = self.augment(images, ha, wa, fl)
            hw = torch.tensor([[ha, wa]] * n, dtype=torch.int32).to(dev, non_blocking=True)
            b, s, c, cnt = eng.forward_device(img, hw, *self._padded(eng, ha, wa), mask=False)
            ops.tta_boxes_to_original(b, s, c, cnt, sizes, ha, wa, fl, a * topk, c_boxes, c_scores, c_cls, c_cand)
        seg_len = torch.full((n,), cap, dtype=torch.int32, device=dev)
        return ops.nms_gather(c_boxes, c_scores, c_cls, c_cand, n, cap, seg_len, self.nms_thresh, topk)[:4]

    def mask_stage(self, eng, images: torch.Tensor, sizes: torch.Tensor, augs, mb, mc, cnt) -> torch.Tensor:
        """The mask branch on the merged boxes in every augmentation (its pyramid recomputed: the pass is deterministic), the mean of
        the maps. -> (n, topk, M, M) fp32."""
        maps = None
        for a, (ha, wa, fl) in enumerate(augs):
            img = self.augment(images, ha, wa, fl)
            feats = eng._backbone(img, *self._padded(eng, ha, wa))
            probs = eng._mask_head(feats, ops.tta_boxes_to_augmented(mb, cnt, sizes, ha, wa, fl), mc, cnt)
            if maps is None:
                maps = torch.empty((len(augs),) + tuple(probs.shape), dtype=torch.float32, device=probs.device)
            maps[a].copy_(probs)
        flips = torch.tensor([int(fl) for _, _, fl in augs], dtype=torch.int32).to(maps.device)
        return ops.tta_reduce_masks(maps, flips, cnt)

    def _group(self, inputs: List[dict], do_postprocess: bool = True) -> List[dict]:
        from .modeling import detector_postprocess
        model = self.model
        eng = model.engine()
        images = torch.stack([x["image"].to(model.device) for x in inputs]).contiguous()
        hi, wi = int(images.shape[-2]), int(images.shape[-1])
        outs = [(int(x.get("height", hi)), int(x.get("width", wi))) for x in inputs]
        sizes = torch.tensor([[hi, wi, oh, ow] for oh, ow in outs], dtype=torch.int32).to(images.device)
        augs = tta_augmentations(hi, wi, hi, wi, self.min_sizes, self.max_size, self.flip)
        res = self.box_stage(eng, images, sizes, augs)
        mask_on = bool(model.roi_heads.mask_on)
        if mask_on:
            res = res + (self.mask_stage(eng, images, sizes, augs, res[0], res[2], res[3]),)
        out = []
        for r, (oh, ow) in zip(OpensetRCNNEngine.to_instances(res, len(inputs)), outs):
            inst = Instances((oh, ow), pred_boxes=Boxes(r["pred_boxes"]), scores=r["scores"], pred_classes=r["pred_classes"])
            if mask_on:
                inst.pred_masks = r["pred_masks"]
                if do_postprocess:
                    inst = detector_postprocess(inst, oh, ow)
            out.append({"instances": inst})
        return out

    @torch.no_grad()
    def forward(self, batched_inputs: List[dict], do_postprocess: bool = True) -> List[dict]:
        """do_postprocess=False (MASK_ON only makes a difference): the merged Instances keep the averaged pred_masks (k, 1, M, M)
        instead of going through detector_postprocess, which clips, drops empty boxes and pastes the masks."""
        if self.model.training:
            raise ValueError("TEST.AUG: the model is in training mode; test-time augmentation is inference only (model.eval())")
        groups: Dict[tuple, List[int]] = {}
        for i, x in enumerate(batched_inputs):
            im = x["image"]
            if im.dtype != torch.uint8:
                raise ValueError(f"TEST.AUG: input {i} is {im.dtype}; test-time augmentation resizes uint8 images only (Pillow BILINEAR)")
            if im.dim() != 3 or im.shape[0] != 3:
                raise ValueError(f"TEST.AUG: input {i} has shape {tuple(im.shape)}; expected (3, h, w)")
            groups.setdefault((int(im.shape[1]), int(im.shape[2])), []).append(i)
        results: List[dict] = [None] * len(batched_inputs)
        for idx in groups.values():  # (dicts keep insertion order: groups in order of first appearance)
            for i, r in zip(idx, self._group([batched_inputs[i] for i in idx], do_postprocess)):
                results[i] = r
        return results
