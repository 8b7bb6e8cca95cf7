"""Box-proposal recall (csrc/osr_proposal_recall.hip, host/proposal_evaluation.py) on a synthetic set the size of COCO val2017: 5000
images x 1000 proposals in batches of 16, ground-truth counts with a long tail up to about 90.

  - ops.proposal_recall per batch (4 area ranges x limits 100 / 1000 in one launch), device events, every batch of the set;
  - the same eight passes composed from torch device ops -- the reference's loop moved onto the device: per pass a sort, the IoU
    matrix, and per round two max reductions and two row / column fills -- on the first batches, interleaved with the launch on the
    same batch (device events around the whole batch: the chain is bound by its launches, which is the point);
  - the CPU specification (evaluate_box_proposals' loop, host clock) on the first images, whose sums must equal the kernel's;
  - the ProposalNetwork pass (backbone + RPN with POST_NMS_TOPK_TEST 2000 and 1000 + the proposal post-process) beside the stock
    Faster R-CNN pass of the same run, batch 16 at 800 x 1333, median of 10 interleaved launches.

Writes profiles/proposal_recall_line.json (or --out)."""
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

IMAGES, PROPOSALS, BATCH = 5000, 1000, 16
AREAS, LIMITS = ("all", "small", "medium", "large"), (100, 1000)
TORCH_BATCHES, CPU_IMAGES = 8, 256
LAUNCHES, WARMUP = 10, 2
N, H, W = 16, 800, 1333


def synthetic_batch(rng, n):
    """-> (boxes (n, PROPOSALS, 4), logits (n, PROPOSALS), counts (n), gt_boxes (NG, 4), gt_area (NG), seg_off (n + 1)) numpy. Ground
    truths per image: 1 + a geometric tail (mean about 7, cut at 90); a third of the proposals are jittered copies of ground truths."""
    per = np.minimum(1 + rng.geometric(1.0 / 6.5, size=n) - 1 + (rng.random(n) < 0.03) * rng.integers(20, 80, size=n), 90).astype(np.int64)
    per[rng.random(n) < 0.01] = 0
    ng = int(per.sum())
    side = np.exp(rng.normal(4.2, 0.9, size=(ng, 2))).clip(4, 600)
    xy = rng.random((ng, 2)) * np.array([640.0, 480.0])
    gt = np.concatenate([xy, xy + side], axis=1).astype(np.float32)
    area = (side[:, 0] * side[:, 1] * 0.7).astype(np.float32)  # (a mask's area: below the box's)
    seg = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
    pside = np.exp(rng.normal(4.2, 1.0, size=(n, PROPOSALS, 2))).clip(4, 640)
    pxy = rng.random((n, PROPOSALS, 2)) * np.array([640.0, 480.0])
    boxes = np.concatenate([pxy, pxy + pside], axis=2).astype(np.float32)
    for i in range(n):
        if per[i]:
            k = PROPOSALS // 3
            src = gt[seg[i] + rng.integers(0, per[i], size=k)]
            jit = src + (rng.normal(0, 0.12, size=(k, 4)) * np.tile(src[:, 2:] - src[:, :2], 2)).astype(np.float32)
            jit[:, 2:] = np.maximum(jit[:, 2:], jit[:, :2] + 1)
            boxes[i, rng.permutation(PROPOSALS)[:k]] = jit
    logits = rng.normal(0, 2, size=(n, PROPOSALS)).astype(np.float32)
    return boxes, logits, np.full(n, PROPOSALS, dtype=np.int32), gt, area, seg


def torch_device_sums(PE, boxes, logits, counts, gt_boxes, gt_area, seg, area_ranges, thresholds):
    """The reference's eight passes from torch device ops -> (hits (A, L, T) int64, num_pos (A) int64) on the device."""
    dev = boxes.device
    hits = torch.zeros((len(AREAS), len(LIMITS), len(thresholds)), dtype=torch.int64, device=dev)
    num_pos = torch.zeros(len(AREAS), dtype=torch.int64, device=dev)
    thr = thresholds.to(dev)
    for a in range(len(AREAS)):
        lo, hi = area_ranges[a, 0].to(dev), area_ranges[a, 1].to(dev)
        for l, limit in enumerate(LIMITS):
            for i in range(boxes.shape[0]):
                k, g0, g1 = int(counts[i]), int(seg[i]), int(seg[i + 1])
                if k == 0 or g1 == g0:
                    continue
                order = logits[i, :k].sort(descending=True, stable=True)[1]
                b = boxes[i, :k][order]
                ar = gt_area[g0:g1]
                g = gt_boxes[g0:g1][(ar >= lo) & (ar <= hi)]
                if l == 0:
                    num_pos[a] += len(g)
                if len(g) == 0:
                    continue
                b = b[:limit]
                ov = PE.pairwise_iou(b, g)
                rec = torch.zeros(len(g), dtype=torch.float32, device=dev)
                for j in range(min(len(b), len(g))):
                    best, row = ov.max(dim=0)
                    v, gi = best.max(dim=0)
                    bi = row[gi]
                    rec[j] = ov[bi, gi]
                    ov[bi, :] = -1
                    ov[:, gi] = -1
                hits[a, l] += (rec[None, :] >= thr[:, None]).sum(dim=1)
    return hits, num_pos


def interleaved(fns, launches=LAUNCHES):
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for k in fns}
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for i in range(launches):
        for k, fn in fns.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        t = [a.elapsed_time(b) for a, b in ev[k]]
        out[k] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))
    return out


def spread(t):
    return dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), calls=len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_recall_line.json"))
    ap.add_argument("--images", type=int, default=IMAGES)
    ap.add_argument("--skip-models", action="store_true")
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host import proposal_evaluation as PE
    dev = "cuda:0"
    thresholds, area_ranges = PE.default_thresholds(), PE.area_range_tensor(AREAS)
    result = dict(device=torch.cuda.get_device_name(0), images=args.images, proposals_per_image=PROPOSALS, batch=BATCH, areas=list(AREAS),
                  limits=list(LIMITS), grid="one workgroup of 1024 threads per (image, area range, limit)")

    def write(final=False):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        if final:
            print("wrote", args.out)

    rng = np.random.default_rng(2017)
    batches = [synthetic_batch(rng, min(BATCH, args.images - lo)) for lo in range(0, args.images, BATCH)]
    per_image = np.concatenate([np.diff(b[5]) for b in batches])
    result["ground_truths"] = dict(total=int(per_image.sum()), mean=round(float(per_image.mean()), 2), max=int(per_image.max()),
                                   images_without=int((per_image == 0).sum()))
    result["batches"] = len(batches)
    on = [tuple(torch.from_numpy(a).to(dev) for a in b) for b in batches]
    torch.cuda.synchronize()

    def launch(t, b):
        return ops.proposal_recall(t[0], t[1], t[2], t[3], t[4], t[5], int(np.diff(b[5]).max()), area_ranges, LIMITS, thresholds)

    # ---- the launch, every batch of the set; the sums stay on the device ----
    for t, b in zip(on[:3], batches[:3]):
        launch(t, b)
    torch.cuda.synchronize()
    ev, sums = [], None
    t0 = time.perf_counter()
    for t, b in zip(on, batches):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        hits, num_pos, _ = launch(t, b)
        e[1].record()
        ev.append(e)
        s = (hits.sum(dim=0, dtype=torch.int64), num_pos.sum(dim=0, dtype=torch.int64))
        sums = s if sums is None else (sums[0] + s[0], sums[1] + s[1])
    torch.cuda.synchronize()
    result["host_s_for_the_set"] = round(time.perf_counter() - t0, 3)
    times = [a.elapsed_time(b) for a, b in ev]
    result["proposal_recall_per_batch"] = dict(spread(times), clock="device events", sum_ms_for_the_set=round(sum(times), 2))
    figures = {}
    h, p = sums[0].cpu(), sums[1].cpu()
    for l, limit in enumerate(LIMITS):
        for a, area in enumerate(AREAS):
            figures[f"AR{PE.REPORTED_AREAS[area]}@{limit}"] = round(float(PE.finish(h[a, l], int(p[a]), thresholds)["ar"]) * 100, 3)
    result["figures"] = figures
    print(json.dumps(result["proposal_recall_per_batch"]), json.dumps(figures), flush=True)
    write()

    # ---- the same passes from torch device ops, interleaved with the launch on the same batch ----
    torch_device_sums(PE, *on[0], area_ranges, thresholds)  # warm-up
    torch.cuda.synchronize()
    tk, tt, equal = [], [], True
    for t, b in zip(on[1:1 + TORCH_BATCHES], batches[1:1 + TORCH_BATCHES]):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        hits, num_pos, _ = launch(t, b)
        e[1].record()
        e[2].record()
        th, tp = torch_device_sums(PE, *t, area_ranges, thresholds)
        e[3].record()
        torch.cuda.synchronize()
        tk.append(e[0].elapsed_time(e[1]))
        tt.append(e[2].elapsed_time(e[3]))
        equal = equal and bool(torch.equal(hits.sum(dim=0, dtype=torch.int64), th)) and bool(torch.equal(num_pos.sum(dim=0, dtype=torch.int64), tp))
    result["torch_device_ops_per_batch"] = dict(spread(tt), clock="device events around the batch's chain of launches", kernel_on_the_same_batches=spread(tk),
                                                sums_equal_the_kernels=equal, ratio_of_medians=round(statistics.median(tt) / statistics.median(tk), 1),
                                                scaled_to_the_set_s=round(statistics.median(tt) * len(batches) / 1e3, 1))
    print(json.dumps(result["torch_device_ops_per_batch"]), flush=True)
    write()

    # ---- the CPU specification on the first images ----
    nb = CPU_IMAGES // BATCH
    spec_h = np.zeros((len(AREAS), len(LIMITS), len(thresholds)), dtype=np.int64)
    spec_p = np.zeros(len(AREAS), dtype=np.int64)
    t0 = time.perf_counter()
    for b in batches[:nb]:
        for i in range(len(b[2])):
            g0, g1 = int(b[5][i]), int(b[5][i + 1])
            for a, area in enumerate(AREAS):
                for l, limit in enumerate(LIMITS):
                    ov = PE.match_image(torch.from_numpy(b[0][i]), torch.from_numpy(b[1][i]), torch.from_numpy(b[3][g0:g1]), torch.from_numpy(b[4][g0:g1]),
                                        PE.AREA_RANGES[area], limit)
                    if ov is None:
                        continue
                    ov = ov[ov >= 0]
                    spec_h[a, l] += (ov[None, :] >= thresholds[:, None]).sum(dim=1).numpy()
                    if l == 0:
                        spec_p[a] += len(ov)
    cpu_s = time.perf_counter() - t0
    kh, kp = None, None
    for t, b in zip(on[:nb], batches[:nb]):
        hits, num_pos, _ = launch(t, b)
        s = (hits.sum(dim=0, dtype=torch.int64), num_pos.sum(dim=0, dtype=torch.int64))
        kh, kp = (s[0], s[1]) if kh is None else (kh + s[0], kp + s[1])
    same = bool(np.array_equal(kh.cpu().numpy(), spec_h) and np.array_equal(kp.cpu().numpy(), spec_p))
    assert same, "the kernel's sums differ from the specification's"
    result["cpu_specification"] = dict(images=nb * BATCH, seconds=round(cpu_s, 3), scaled_to_the_set_s=round(cpu_s * args.images / (nb * BATCH), 1), clock="host clock",
                                       sums_equal_the_kernels=same)
    print(json.dumps(result["cpu_specification"]), flush=True)
    write()

    # ---- the ProposalNetwork pass beside the stock Faster R-CNN pass ----
    if not args.skip_models:
        from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
        from openset_rcnn_amd.host.weights import random_standard_params
        params = random_standard_params(0)
        fpn = StandardRCNNEngine(params, None, dtype=torch.float16, device=dev)
        no_heads = {k: v for k, v in params.items() if not k.startswith("roi_heads.")}
        pn = {post: StandardRCNNEngine(no_heads, dict(post_nms_topk_test=post), dtype=torch.float16, device=dev) for post in (2000, 1000)}
        assert not pn[2000].has_roi and fpn.has_roi
        images = torch.randint(0, 256, (N, 3, H, W), generator=torch.Generator().manual_seed(1234), dtype=torch.uint8).to(dev)
        hw = torch.tensor([(H, W)] * N, dtype=torch.int32, device=dev)
        scale = torch.ones((N, 2), dtype=torch.float32, device=dev)
        zeros = {post: torch.zeros((N, post), dtype=torch.int64, device=dev) for post in pn}

        def proposal_pass(post):
            e = pn[post]
            sel = e._rpn(e._backbone(images, 800, 1344), hw)
            return ops.detector_postprocess(sel["boxes"].view(N, post, 4), sel["scores"].view(N, post), zeros[post], sel["counts"], scale, hw)
        out = proposal_pass(2000)
        torch.cuda.synchronize()
        t = interleaved({"proposal_network_pass_post_2000": lambda: proposal_pass(2000), "proposal_network_pass_post_1000": lambda: proposal_pass(1000),
                         "stock_faster_rcnn_pass": lambda: fpn.forward_device(images, hw, 800, 1344)})
        t["proposals_of_the_pass"] = [int(c) for c in out[3].cpu()]
        t.update(batch=N, image=f"3x{H}x{W}", dtype="float16", launches=LAUNCHES)
        result["passes_ms"] = t
        print(json.dumps(t), flush=True)
    write(True)


if __name__ == "__main__":
    main()
