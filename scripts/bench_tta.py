"""Test-time augmentation (TEST.AUG, host/tta.py) at the benchmark's shape: 16 synthetic 800 x 1333 uint8 frames, the stock model,
the default TEST.AUG (nine min sizes x flip = 18 augmentations per image), MODEL.MASK_ON off and on.

Per configuration, in one run:
  wrapper            GeneralizedRCNNWithTTA(cfg, model)(inputs), wall clock with a device sync around the call -> images/s;
  engine_passes      its engine work alone on pre-augmented images (device events): the 18 mask-off passes, and with MASK_ON the 18
                     backbone + mask-head passes on the merged boxes;
  device_glue        its glue alone (device events): resize + flip, box maps, merge (osr_nms_topk + gathers), mask mean;
  host_composition   the same TTA composed on the host from the pieces the package had before: PIL resize, numpy flip,
                     model.inference per augmentation, numpy box maps, a torch-CPU per-class NMS, inference(detected_instances=...)
                     per augmentation with a CPU mean, detector_postprocess -> images/s.

Writes profiles/tta_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N, H, W = 16, 800, 1333
F = np.float32


def mask_params(g, rows):
    pre = "roi_heads.mask_head."
    p = {}
    for i in range(1, 5):
        p[f"{pre}mask_fcn{i}.weight"] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        p[f"{pre}mask_fcn{i}.bias"] = torch.zeros(256)
    p[pre + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (2.0 / 256) ** 0.5
    p[pre + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
    p[pre + "predictor.weight"] = torch.randn(rows, 256, 1, 1, generator=g) * (2.0 / 256) ** 0.5
    p[pre + "predictor.bias"] = torch.zeros(rows)
    return p


def build(mask_on: bool, dtype):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    from openset_rcnn_amd.host.weights import random_standard_params
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda:0", "MODEL.MASK_ON", str(mask_on), "TEST.AUG.ENABLED", "True"])
    model = M.build_model(cfg)
    p = dict(random_standard_params(0))
    if mask_on:
        p.update(mask_params(torch.Generator().manual_seed(4000), 1 if cfg.MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK else cfg.MODEL.ROI_HEADS.NUM_CLASSES))
    sd = model.state_dict()
    for k, v in p.items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    model.kernel_dtype = dtype
    return cfg, model.eval()


def wall(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(times), 2), min_ms=round(min(times), 2), max_ms=round(max(times), 2), reps=reps)


def events(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(times), 2), min_ms=round(min(times), 2), max_ms=round(max(times), 2), reps=reps)


# ---- the host composition ---------------------------------------------------------------------------------------------------------------
def map_boxes(b: np.ndarray, size, ha, wa, flip, inverse: bool) -> np.ndarray:
    """[d2] transform list of one augmentation on (k, 4) fp32 boxes (see host/tta.py), forward or inverse."""
    hi, wi, ho, wo = size
    steps = ([("r", ho, wo, hi, wi)] if (ho, wo) != (hi, wi) else []) + [("r", hi, wi, ha, wa)] + ([("f",)] if flip else [])
    b = b.astype(F).copy()
    for s in (reversed(steps) if inverse else steps):
        if s[0] == "f":
            x0, x1 = F(wa) - b[:, 0], F(wa) - b[:, 2]
            b[:, 0], b[:, 2] = np.minimum(x0, x1), np.maximum(x0, x1)
        else:
            _, h0, w0, h1, w1 = s if not inverse else (s[0], s[3], s[4], s[1], s[2])
            b[:, 0::2] *= F(float(w1) / float(w0))
            b[:, 1::2] *= F(float(h1) / float(h0))
    return b


def cpu_nms(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, thr: float, topk: int) -> torch.Tensor:
    """Per-class greedy NMS (score descending, ties lower index first, IoU > thr suppresses), the first topk kept by score."""
    keep = torch.zeros(len(boxes), dtype=torch.bool)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    for c in classes.unique().tolist():
        ids = torch.nonzero(classes == c).squeeze(1)
        ids = ids[torch.argsort(scores[ids], descending=True, stable=True)]
        b, a = boxes[ids], area[ids]
        dead = torch.zeros(len(ids), dtype=torch.bool)
        for i in range(len(ids)):
            if dead[i]:
                continue
            keep[ids[i]] = True
            w = (torch.minimum(b[i, 2], b[i + 1:, 2]) - torch.maximum(b[i, 0], b[i + 1:, 0])).clamp(min=0)
            h = (torch.minimum(b[i, 3], b[i + 1:, 3]) - torch.maximum(b[i, 1], b[i + 1:, 1])).clamp(min=0)
            inter = w * h
            dead[i + 1:] |= inter / (a[i] + a[i + 1:] - inter) > thr
    kept = torch.nonzero(keep).squeeze(1)
    return kept[torch.argsort(scores[kept], descending=True, stable=True)][:topk]


def host_tta(cfg, model, inputs):
    from PIL import Image
    from openset_rcnn_amd.host.modeling import detector_postprocess
    from openset_rcnn_amd.host.structures import Boxes, Instances
    from openset_rcnn_amd.host.tta import tta_augmentations
    aug = cfg.TEST.AUG
    thr, topk, mask_on = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST), int(cfg.TEST.DETECTIONS_PER_IMAGE), bool(cfg.MODEL.MASK_ON)
    hi, wi = (int(v) for v in inputs[0]["image"].shape[1:])  # (one group: the frames share their size)
    sizes = [(hi, wi, int(x["height"]), int(x["width"])) for x in inputs]
    augs = tta_augmentations(hi, wi, hi, wi, tuple(aug.MIN_SIZES), int(aug.MAX_SIZE), bool(aug.FLIP))
    hwc = [np.ascontiguousarray(x["image"].numpy().transpose(1, 2, 0)) for x in inputs]

    def batch(ha, wa, fl):
        out = []
        for im in hwc:
            r = im if (ha, wa) == (hi, wi) else np.asarray(Image.fromarray(im).resize((wa, ha), Image.BILINEAR))
            r = np.flip(r, axis=1) if fl else r
            out.append({"image": torch.from_numpy(np.ascontiguousarray(r.transpose(2, 0, 1)))})
        return out
    cands = [([], [], []) for _ in inputs]
    for ha, wa, fl in augs:
        for k, r in enumerate(model.inference(batch(ha, wa, fl), do_postprocess=False)):
            inst = r["instances"]
            cands[k][0].append(map_boxes(inst.pred_boxes.tensor.numpy(), sizes[k], ha, wa, fl, True))
            cands[k][1].append(inst.scores)
            cands[k][2].append(inst.pred_classes)
    merged = []
    for k, (b, s, c) in enumerate(cands):
        ho, wo = sizes[k][2], sizes[k][3]
        b, s, c = torch.from_numpy(np.concatenate(b)), torch.cat(s), torch.cat(c)
        ok = torch.isfinite(b).all(dim=1) & torch.isfinite(s)
        b, s, c = b[ok], s[ok], c[ok]
        b = torch.stack((b[:, 0].clamp(0, wo), b[:, 1].clamp(0, ho), b[:, 2].clamp(0, wo), b[:, 3].clamp(0, ho)), dim=1)
        ok = s > 1e-8
        b, s, c = b[ok], s[ok], c[ok]
        kept = cpu_nms(b, s, c, thr, topk)
        merged.append((b[kept], s[kept], c[kept]))
    sums = None
    if mask_on:
        sums = [torch.zeros((len(m[0]), 28, 28)) for m in merged]
        for ha, wa, fl in augs:
            det = [Instances((ha, wa), pred_boxes=Boxes(torch.from_numpy(map_boxes(m[0].numpy(), sizes[k], ha, wa, fl, False))), pred_classes=m[2])
                   for k, m in enumerate(merged)]
            for k, r in enumerate(model.inference(batch(ha, wa, fl), detected_instances=det, do_postprocess=False)):
                pm = r["instances"].pred_masks[:, 0].cpu()
                sums[k] += torch.flip(pm, dims=[-1]) if fl else pm
    out = []
    for k, m in enumerate(merged):
        ho, wo = sizes[k][2], sizes[k][3]
        inst = Instances((ho, wo), pred_boxes=Boxes(m[0]), scores=m[1], pred_classes=m[2])
        if mask_on:
            inst.pred_masks = (sums[k] / len(augs)).unsqueeze(1).to(model.device)
            inst = detector_postprocess(inst, ho, wo)
        out.append({"instances": inst})
    return out


# ---- the wrapper's parts ----------------------------------------------------------------------------------------------------------------
def parts(wrapper, model, inputs):
    """-> (engine-passes closure, glue closure) over the wrapper's own tensors of one call."""
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.tta import tta_augmentations
    eng = model.engine()
    images = torch.stack([x["image"].to(model.device) for x in inputs]).contiguous()
    n, topk = len(inputs), int(eng.cfg["std_detections_per_image"])
    sizes = torch.tensor([[H, W, int(x["height"]), int(x["width"])] for x in inputs], dtype=torch.int32, device=model.device)
    augs = tta_augmentations(H, W, H, W, wrapper.min_sizes, wrapper.max_size, wrapper.flip)
    mask_on = bool(model.roi_heads.mask_on)
    pre = [wrapper.augment(images, ha, wa, fl) for ha, wa, fl in augs]
    hws = [torch.tensor([[ha, wa]] * n, dtype=torch.int32, device=model.device) for ha, wa, _ in augs]
    merged = wrapper.box_stage(eng, images, sizes, augs)
    dets = [eng.forward_device(img, hw, *wrapper._padded(eng, ha, wa), mask=False) for img, hw, (ha, wa, _) in zip(pre, hws, augs)]
    aug_boxes = [ops.tta_boxes_to_augmented(merged[0], merged[3], sizes, ha, wa, fl) for ha, wa, fl in augs]
    maps = torch.rand((len(augs), n, topk, 28, 28), device=model.device) if mask_on else None
    flips = torch.tensor([int(fl) for _, _, fl in augs], dtype=torch.int32, device=model.device)
    cap = len(augs) * topk
    cb, cs = torch.empty((n, cap, 4), device=model.device), torch.empty((n, cap), device=model.device)
    cc, cd = torch.empty((n, cap), dtype=torch.int32, device=model.device), torch.empty((n, cap), dtype=torch.int32, device=model.device)
    seg = torch.full((n,), cap, dtype=torch.int32, device=model.device)

    def passes():
        for img, hw, (ha, wa, _) in zip(pre, hws, augs):
            eng.forward_device(img, hw, *wrapper._padded(eng, ha, wa), mask=False)
        if mask_on:
            for img, ab, (ha, wa, _) in zip(pre, aug_boxes, augs):
                eng._mask_head(eng._backbone(img, *wrapper._padded(eng, ha, wa)), ab, merged[2], merged[3])

    def glue():
        for a, (ha, wa, fl) in enumerate(augs):
            wrapper.augment(images, ha, wa, fl)
            ops.tta_boxes_to_original(*dets[a], sizes, ha, wa, fl, a * topk, cb, cs, cc, cd)
        keep, cnt = ops.nms_topk(cb, cs, cc, cd, n, cap, seg, wrapper.nms_thresh, topk)
        ops.gather_rows(cb.view(-1, 4), cap, keep, cnt)
        ops.gather_rows(cs.view(-1), cap, keep, cnt)
        ops.gather_rows(cc.view(-1).view(torch.float32), cap, keep, cnt)
        if mask_on:
            for ha, wa, fl in augs:
                wrapper.augment(images, ha, wa, fl)
                ops.tta_boxes_to_augmented(merged[0], merged[3], sizes, ha, wa, fl)
            ops.tta_reduce_masks(maps, flips, merged[3])
    return passes, glue, len(augs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_line.json"))
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    g = torch.Generator().manual_seed(1234)
    frames = [torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8) for _ in range(N)]
    inputs = [{"image": f, "height": H, "width": W} for f in frames]
    result = dict(batch=N, image=f"3x{H}x{W}", dtype=args.dtype, device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps)
    for mask_on in (False, True):
        cfg, model = build(mask_on, getattr(torch, args.dtype))
        wrapper = GeneralizedRCNNWithTTA(cfg, model)
        out = wrapper(inputs)  # warm-up: packs the weights, fills the allocator pools
        line = dict(detections=[len(o["instances"]) for o in out])
        line["wrapper"] = wall(lambda: wrapper(inputs), args.reps)
        line["wrapper"]["images_per_s"] = round(N / line["wrapper"]["median_ms"] * 1e3, 2)
        passes, glue, num_aug = parts(wrapper, model, inputs)
        line["augmentations"] = num_aug
        line["engine_passes"] = events(passes, args.reps)
        line["device_glue"] = events(glue, args.reps)
        host_tta(cfg, model, inputs[:1])  # warm-up of the host path's own shapes (batch 1 is another launch plan: not timed)
        line["host_composition"] = wall(lambda: host_tta(cfg, model, inputs), args.host_reps)
        line["host_composition"]["images_per_s"] = round(N / line["host_composition"]["median_ms"] * 1e3, 2)
        line["wrapper_over_host"] = round(line["host_composition"]["median_ms"] / line["wrapper"]["median_ms"], 2)
        result["mask_on" if mask_on else "mask_off"] = line
        print(json.dumps({("mask_on" if mask_on else "mask_off"): line}), flush=True)
        del wrapper, model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
