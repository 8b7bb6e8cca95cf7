"""META_ARCHITECTURE "PanopticFPN" (host/engine_panoptic.py) at the benchmark's shape: 16 synthetic 800 x 1333 uint8 frames (padded to
800 x 1344), fp16, seeded synthetic weights. In one run, the two sides of every comparison interleaved, medians of device-event times
(the combine step: host clock around work that ends in a synchronise, because both sides end on the host):

  (a) pass        the Panoptic FPN engine pass (Mask R-CNN + the semantic head) against the stock Mask R-CNN engine pass;
  (b) launches    per-launch times of the semantic head in one profiled pass: its convolutions, the statistics, the merges;
  (c) gn          the head's last step -- four GroupNorm statistics + the four-term GN / ReLU / x2 / sum launch -- against
                  F.group_norm + relu + F.interpolate + add on the same fp16 values (NCHW, torch's layout);
  (d) resample    ops.semseg_resample in label mode for the 16 images against the two F.interpolate + argmax;
  (e) combine     ops.panoptic_combine + segments_info_from_table (one D2H copy per image) against detectron2's loop with its .item()
                  calls on device tensors, 100 instances per image.

Bytes are algorithmic: what each step has to read and write once. Writes profiles/panoptic_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N, H, W, C, K_INST = 16, 800, 1333, 54, 100
DEV = "cuda:0"
COMBINE = dict(overlap_thresh=0.5, stuff_area_limit=4096, instances_confidence_thresh=0.5)


def events(fns, reps, warmup=2, host_clock=False):
    """Median time of each fn, the fns alternating inside every repetition: device events, or the host clock around a synchronise."""
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= warmup:
                times[i].append((t1 - t0) * 1e3 if host_clock else e0.elapsed_time(e1))
    return [dict(median_ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=reps) for t in times]


def compare(name, hip, torch_ops, nbytes, reps, host_clock=False):
    th, tt = events([hip, torch_ops], reps, host_clock=host_clock)
    return dict(hip=th, torch_ops=tt, algorithmic_bytes=int(nbytes), hip_gb_per_s=round(nbytes / th["median_ms"] / 1e6, 1),
                torch_over_hip=round(tt["median_ms"] / th["median_ms"], 2), hip_not_slower=bool(th["median_ms"] <= tt["median_ms"]),
                clock="host clock around a synchronise" if host_clock else "device events")


def torch_combine(masks, scores, classes, labels, overlap_thresh, stuff_area_limit, instances_confidence_thresh):
    """[d2] v0.6 combine_semantic_and_instance_outputs, as it is written there, on device tensors."""
    pan = torch.zeros_like(labels, dtype=torch.int32)
    sorted_inds = torch.argsort(-scores)
    cur, info = 0, []
    for inst_id in sorted_inds:
        score = scores[inst_id].item()
        if score < instances_confidence_thresh:
            break
        mask = masks[inst_id]
        mask_area = mask.sum().item()
        if mask_area == 0:
            continue
        intersect = (mask > 0) & (pan > 0)
        intersect_area = intersect.sum().item()
        if intersect_area * 1.0 / mask_area > overlap_thresh:
            continue
        if intersect_area > 0:
            mask = mask & (pan == 0)
        cur += 1
        pan[mask] = cur
        info.append({"id": cur, "isthing": True, "score": score, "category_id": classes[inst_id].item(), "instance_id": inst_id.item()})
    for label in torch.unique(labels).cpu().tolist():
        if label == 0:
            continue
        mask = (labels == label) & (pan == 0)
        mask_area = mask.sum().item()
        if mask_area < stuff_area_limit:
            continue
        cur += 1
        pan[mask] = cur
        info.append({"id": cur, "isthing": False, "category_id": label, "area": mask_area})
    return pan, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panoptic_line.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_panoptic.py measures on the GPU; none found")
    ge.load_package()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_panoptic import PanopticFPNEngine
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.weights import random_panoptic_params
    n = args.batch
    hp, wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    h4, w4 = hp // 4, wp // 4
    res = dict(gpu=torch.cuda.get_device_name(0), batch=n, image=[H, W], padded=[hp, wp], dtype="float16", sem_classes=C, instances_per_image=K_INST)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    hw = torch.tensor([(H, W)] * n, dtype=torch.int32, device=DEV)
    P = random_panoptic_params(0)
    pan_eng = PanopticFPNEngine(P, None, torch.float16, DEV)
    stock = StandardRCNNEngine({k: v for k, v in P.items() if not k.startswith("sem_seg_head.")}, None, torch.float16, DEV)

    # (a) the two passes, interleaved
    pa, sa = events([lambda: pan_eng.forward_device(images, hw, hp, wp), lambda: stock.forward_device(images, hw, hp, wp)], args.reps)
    res["pass"] = dict(panoptic_fpn=pa, stock_mask_rcnn=sa, added_ms=round(pa["median_ms"] - sa["median_ms"], 3), ratio=round(pa["median_ms"] / sa["median_ms"], 3))

    # (b) one profiled pass: the semantic head's launches
    pan_eng.profile, pan_eng.profile_hbm = [], []
    keep = {}
    out = pan_eng.forward_device(images, hw, hp, wp, keep)
    torch.cuda.synchronize()
    prof, hbm = pan_eng.resolve_profile()
    pan_eng.profile = pan_eng.profile_hbm = None
    res["launches"] = dict(
        convolutions=[dict(name=nm, ms=round(e0.elapsed_time(e1), 3), tflops=round(fl / e0.elapsed_time(e1) / 1e9, 1)) for nm, fl, e0, e1, _, _ in prof if nm.startswith("sem_seg_head")],
        elementwise=[dict(name=nm, ms=round(e0.elapsed_time(e1), 3), algorithmic_gb_per_s=round(nb / e0.elapsed_time(e1) / 1e6, 1)) for nm, nb, e0, e1, _ in hbm if nm.startswith("sem_seg_head")],
        note="one profiled pass (events between launches), not a median")
    res["launches"]["head_ms"] = round(sum(d["ms"] for d in res["launches"]["convolutions"]) + sum(d["ms"] for d in res["launches"]["elementwise"]), 3)
    logits = out[-1].clone()
    terms = [(t[0].clone(), t[2], t[3], t[4]) for t in keep["sem_terms"]]
    del keep, out

    # (c) the head's last step
    nchw = [x.permute(0, 3, 1, 2).contiguous() for x, _, _, _ in terms]
    affine = [(gm.half(), bt.half()) for _, gm, bt, _ in terms]

    def hip_gn():
        return ops.gn_relu_merge([(x, ops.group_norm_stats(x), gm, bt, up) for x, gm, bt, up in terms])

    def torch_gn():
        total = None
        for x, (gm, bt), (_, _, _, up) in zip(nchw, affine, terms):
            v = F.relu(F.group_norm(x, 32, gm, bt, 1e-5))
            if up:
                v = F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
            total = v if total is None else total + v
        return total
    gn_bytes = sum(2 * x.numel() for x, _, _, _ in terms) * 2 + n * h4 * w4 * terms[0][0].shape[-1] * 2  # inputs twice (statistics, merge) + the sum
    res["gn_relu_up2_sum"] = compare("gn", hip_gn, torch_gn, gn_bytes, args.reps)
    del nchw

    # (d) the head's output path, label mode
    planes = logits[..., :C].permute(0, 3, 1, 2).contiguous()

    def hip_resample():
        return [ops.semseg_resample(logits[i], C, (H, W), (H, W), labels=True) for i in range(n)]

    def torch_resample():
        outs = []
        for i in range(n):
            x = F.interpolate(planes[i:i + 1], scale_factor=4, mode="bilinear", align_corners=False)[:, :, :H, :W]
            outs.append(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)[0].argmax(dim=0))
        return outs
    res["semseg_resample_labels"] = compare("resample", hip_resample, torch_resample, logits.numel() * 4 + n * H * W * 4, args.reps)
    res["semseg_resample_labels"]["torch_materialises_bytes_per_image"] = C * hp * wp * 4
    labels = hip_resample()
    del planes

    # (e) the combine step, per image; 100 random boxes as masks, scores spread over (0.3, 1)
    gi = torch.Generator().manual_seed(2)
    masks = torch.zeros((n, K_INST, H, W), dtype=torch.bool, device=DEV)
    for i in range(n):
        for k in range(K_INST):
            bh, bw = int(torch.randint(30, 300, (1,), generator=gi)), int(torch.randint(30, 300, (1,), generator=gi))
            y0, x0 = int(torch.randint(0, H - bh, (1,), generator=gi)), int(torch.randint(0, W - bw, (1,), generator=gi))
            masks[i, k, y0:y0 + bh, x0:x0 + bw] = True
    scores = (torch.rand((n, K_INST), generator=gi) * 0.7 + 0.3).to(DEV)
    classes = torch.randint(0, 80, (n, K_INST), generator=gi).to(DEV)

    def hip_combine():
        outs = []
        for i in range(n):
            pan, table, sc, cnt = ops.panoptic_combine(masks[i], scores[i], classes[i], labels[i], **COMBINE)
            outs.append((pan, ops.segments_info_from_table(table, sc, cnt)))
        return outs

    def torch_loop():
        return [torch_combine(masks[i], scores[i], classes[i], labels[i], **COMBINE) for i in range(n)]
    a, b = hip_combine(), torch_loop()
    same = all(torch.equal(x[0], y[0]) and [d["id"] for d in x[1]] == [d["id"] for d in y[1]] for x, y in zip(a, b))
    res["panoptic_combine"] = compare("combine", hip_combine, torch_loop, masks.numel() + n * H * W * 8, args.reps, host_clock=True)
    res["panoptic_combine"].update(results_equal=bool(same), segments_per_image=round(sum(len(x[1]) for x in a) / n, 1))
    res["all_hip_steps_not_slower"] = all(res[k]["hip_not_slower"] for k in ("gn_relu_up2_sum", "semseg_resample_labels", "panoptic_combine"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
