"""The segmentation evaluators' device steps (csrc/osr_seg_eval.hip) at the benchmark's shape: 16 images of 800 x 1333, C = 54 classes,
about 40 ground-truth and 40 predicted segments per image drawn as blocky regions. In one run, both sides of every comparison
interleaved, medians of 5 device-event times over the 16 images:

  (a) confusion_values   ops.semseg_confusion on the (C, H, W) fp32 values against torch.argmax + torch.bincount;
  (b) confusion_labels   the same on (H, W) int32 labels against torch.bincount alone;
  (c) pair_counts        ops.panoptic_pair_counts against panopticapi's form on the device: torch.unique(return_counts=True) on the
                         64-bit key gt_id * OFFSET + pred_id;
  (d) pq_accumulate      ops.pq_accumulate against the same rules written with torch device ops on the (G + 2, P + 1) table.

Beside them, on the host clock and per image: the numpy form of (a) and (c) (np.argmax + np.bincount, np.unique), on the first
--host-images images only because it is slow, and the PIL decode of the two ground-truth PNGs, which is what bounds the evaluators'
wall time per image once the pixel passes run on the device. Writes profiles/seg_eval_line.json (or --out)."""
import argparse
import io
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

N, H, W, C, SEGMENTS, NCAT, IGNORE = 16, 800, 1333, 54, 40, 133, 255
OFFSET = 256 * 256 * 256
DEV = "cuda:0"


def events(fns, reps, warmup=2):
    """Median device-event time of each fn, the fns alternating inside every repetition."""
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[i].append(e0.elapsed_time(e1))
    return [dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), reps=reps) for t in times]


def host_clock(fn, reps, warmup=1):
    t = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=reps)


def compare(hip, torch_ops, nbytes, reps, n):
    th, tt = events([hip, torch_ops], reps)
    return dict(hip=th, torch_ops=tt, images=n, hip_us_per_image=round(th["median_ms"] / n * 1e3, 2), torch_us_per_image=round(tt["median_ms"] / n * 1e3, 2),
                algorithmic_bytes=int(nbytes), hip_gb_per_s=round(nbytes / th["median_ms"] / 1e6, 1), torch_over_hip=round(tt["median_ms"] / th["median_ms"], 2),
                hip_faster=bool(th["median_ms"] < tt["median_ms"]), clock="device events")


def blocky_map(gen, h, w, n, cell):
    rows, cols = (h + cell - 1) // cell, (w + cell - 1) // cell
    small = (torch.randperm(rows * cols, generator=gen) % n).view(rows, cols)  # (every value occurs when there are at least n cells)
    return small.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[:h, :w].contiguous()


def make_image(gen, h, w):
    """-> gt ids (h, w) int64 (0 = VOID), the listed segments' tables, the predicted map, the semantic ground truth and labels."""
    ids = torch.cat((torch.zeros(1, dtype=torch.int64), torch.sort(torch.randperm(1 << 22, generator=gen)[:SEGMENTS] + 1).values))
    index = blocky_map(gen, h, w, SEGMENTS + 1, 96)  # 0 = VOID, k = the k-th listed segment
    gt_ids_map = ids[index]
    slot_g = torch.randint(0, NCAT, (SEGMENTS,), generator=gen)
    crowd = (torch.rand(SEGMENTS, generator=gen) < 0.1).to(torch.int64)
    area = torch.bincount(index.reshape(-1), minlength=SEGMENTS + 1)[1:]
    pick = torch.zeros(SEGMENTS, dtype=torch.int64)
    for s in set(slot_g[crowd.bool()].tolist()):
        pick[[i for i in range(SEGMENTS) if crowd[i] and slot_g[i] == s][-1]] = 1
    meta = torch.stack((slot_g, crowd, area, pick), dim=1).to(torch.int32)
    # the prediction: the ground truth moved by a few pixels, its ids renumbered, 15 % of the categories changed
    renumber = torch.cat((torch.zeros(1, dtype=torch.int64), torch.randperm(SEGMENTS, generator=gen) + 1))
    pred = renumber[torch.roll(index, (5, 7), dims=(0, 1))].to(torch.int32).contiguous()
    slot_p = torch.zeros(SEGMENTS, dtype=torch.int32)
    keep = torch.rand(SEGMENTS, generator=gen) < 0.85
    slot_p[renumber[1:] - 1] = torch.where(keep, slot_g, torch.randint(0, NCAT, (SEGMENTS,), generator=gen)).to(torch.int32)
    present = ids[1:].tolist()
    sem_gt = (blocky_map(gen, h, w, C + 1, 96)).to(torch.uint8)
    sem_gt[sem_gt == C] = IGNORE
    labels = blocky_map(gen, h, w, C, 112).to(torch.int32)
    rgb = torch.stack((gt_ids_map % 256, gt_ids_map // 256 % 256, gt_ids_map // 65536), dim=-1).to(torch.uint8)
    return dict(rgb=rgb, gt_ids=torch.tensor(present, dtype=torch.int32), meta=meta, pred=pred, slot_p=slot_p, sem_gt=sem_gt, labels=labels)


def torch_confusion(pred, gt, conf, values):
    lab = pred.argmax(dim=0) if values else pred.long()
    g = gt.long()
    col = torch.where(g == IGNORE, C, g)
    conf += torch.bincount((lab * (C + 1) + col).reshape(-1), minlength=(C + 1) ** 2).view(C + 1, C + 1)


def torch_pair_counts(rgb, pred):
    r = rgb.long()
    key = (r[..., 0] + 256 * r[..., 1] + 65536 * r[..., 2]) * OFFSET + pred.long()
    return torch.unique(key.reshape(-1), return_counts=True)


def torch_pq(table, meta, slot_p, pq_counts, pq_iou):
    """The rules of include/osr.h osr_pq_accumulate with torch device ops (the IoU adds are unordered here)."""
    g_n = meta.shape[0]
    t = table.long()
    slot_g, crowd, area_g, pick = meta[:, 0].long(), meta[:, 1].bool(), meta[:, 2].long(), meta[:, 3].bool()
    slot_p = slot_p.long()
    area_p, void_p, inter = t.sum(dim=0)[1:], t[0, 1:], t[1:1 + g_n, 1:]
    union = area_p[None] + area_g[:, None] - inter - void_p[None]
    iou = inter.double() / union.double()
    match = (inter > 0) & ~crowd[:, None] & (slot_g[:, None] == slot_p[None]) & (iou > 0.5)
    gi, pi = match.nonzero(as_tuple=True)
    pq_counts[:, 0].index_add_(0, slot_g[gi], torch.ones_like(gi))
    pq_iou.index_add_(0, slot_g[gi], iou[gi, pi])
    fn = ~crowd & ~match.any(dim=1)
    pq_counts[:, 2].index_add_(0, slot_g[fn], torch.ones_like(slot_g[fn]))
    shield = torch.zeros((pq_counts.shape[0], t.shape[1] - 1), dtype=torch.int64, device=t.device)
    shield[slot_g[pick]] = inter[pick]
    covered = void_p + shield[slot_p, torch.arange(slot_p.numel(), device=t.device)]
    fp = ~match.any(dim=0) & (area_p > 0) & ~(covered.double() / area_p.double() > 0.5)
    pq_counts[:, 1].index_add_(0, slot_p[fp], torch.ones_like(slot_p[fp]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_eval_line.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=N)
    ap.add_argument("--host-images", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_eval.py measures on the GPU; none found")
    from PIL import Image
    ge.load_package()
    from openset_rcnn_amd.host import ops
    n = args.batch
    gen = torch.Generator().manual_seed(0)
    host = [make_image(gen, H, W) for _ in range(n)]
    dev = [{k: v.to(DEV) for k, v in im.items()} for im in host]
    for im in dev:  # values whose argmax is the label map, with noise below the top
        v = torch.rand((C, H, W), device=DEV)
        v.scatter_(0, im["labels"].long()[None], 2.0)
        im["values"] = v
    res = dict(gpu=torch.cuda.get_device_name(0), images=n, image=[H, W], classes=C, categories=NCAT,
               gt_segments_per_image=round(sum(len(im["gt_ids"]) for im in host) / n, 1), pred_segments_per_image=SEGMENTS)
    zeros = lambda *shape, dt=torch.int64: torch.zeros(shape, dtype=dt, device=DEV)  # noqa: E731

    # (a), (b) the confusion matrix
    for key, field, values, per_pixel in (("confusion_values", "values", True, 4 * C + 1), ("confusion_labels", "labels", False, 5)):
        conf_h, inv, conf_t = zeros(C + 1, C + 1), zeros(1), zeros(C + 1, C + 1)

        def hip():
            for im in dev:
                ops.semseg_confusion(im[field], im["sem_gt"], C, IGNORE, conf_h, inv)

        def tch():
            for im in dev:
                torch_confusion(im[field], im["sem_gt"], conf_t, values)
        hip(), tch()
        same = bool(torch.equal(conf_h, conf_t)) and int(inv[0]) == 0
        res[key] = compare(hip, tch, n * H * W * per_pixel, args.reps, n)
        res[key]["results_equal"] = same

    # (c) the pair counts
    flags = zeros(3)
    tables = [zeros(len(im["gt_ids"]) + 2, SEGMENTS + 1, dt=torch.int32) for im in host]

    def hip_pairs():
        for im, t in zip(dev, tables):
            ops.panoptic_pair_counts(im["rgb"], im["gt_ids"], im["pred"], SEGMENTS, flags, out=t)

    def torch_pairs():
        return [torch_pair_counts(im["rgb"], im["pred"]) for im in dev]
    hip_pairs()
    same = True
    for im, t, (keys, cnt) in zip(host, tables, torch_pairs()):
        row_of = {0: 0, **{int(v): 1 + i for i, v in enumerate(im["gt_ids"].tolist())}}
        ref = torch.zeros_like(t, device="cpu")
        for k, c in zip(keys.cpu().tolist(), cnt.cpu().tolist()):
            ref[row_of[k // OFFSET], k % OFFSET] += c
        same = same and bool(torch.equal(t.cpu(), ref))
    res["pair_counts"] = compare(hip_pairs, torch_pairs, n * H * W * 7, args.reps, n)
    res["pair_counts"]["results_equal"] = same and flags.tolist() == [0, 0, 0]

    # (d) the matching
    st_h, iou_h, st_t, iou_t = zeros(NCAT, 3), zeros(NCAT, dt=torch.float64), zeros(NCAT, 3), zeros(NCAT, dt=torch.float64)

    def hip_pq():
        for im, t in zip(dev, tables):
            ops.pq_accumulate(t, im["meta"], im["slot_p"], st_h, iou_h, flags)

    def torch_pq_all():
        for im, t in zip(dev, tables):
            torch_pq(t, im["meta"], im["slot_p"], st_t, iou_t)
    hip_pq(), torch_pq_all()
    same = bool(torch.equal(st_h, st_t)) and bool(torch.allclose(iou_h, iou_t, rtol=1e-12, atol=0)) and flags.tolist() == [0, 0, 0]
    tp, fp, fn = (int(v) for v in st_h.sum(dim=0).tolist())  # of one pass over the images (the timed repeats go on accumulating)
    res["pq_accumulate"] = compare(hip_pq, torch_pq_all, sum(t.numel() * 4 for t in tables), args.reps, n)
    res["pq_accumulate"].update(results_equal=same, tp=tp, fp=fp, fn=fn)

    # the host: numpy's form of (a) and (c), and the PNG decodes
    k = max(1, min(args.host_images, n))
    np_values = [dev[i]["values"].cpu().numpy() for i in range(k)]
    np_img = [{f: host[i][f].numpy() for f in ("sem_gt", "rgb", "pred")} for i in range(k)]

    def numpy_confusion():
        for v, im in zip(np_values, np_img):
            g = im["sem_gt"].astype(np.int64)
            np.bincount((v.argmax(axis=0) * (C + 1) + np.where(g == IGNORE, C, g)).reshape(-1), minlength=(C + 1) ** 2)

    def numpy_pairs():
        for im in np_img:
            r = im["rgb"].astype(np.int64)
            np.unique((r[..., 0] + 256 * r[..., 1] + 65536 * r[..., 2]) * OFFSET + im["pred"].astype(np.int64), return_counts=True)
    pngs = []
    for im in np_img:
        a, b = io.BytesIO(), io.BytesIO()
        Image.fromarray(im["rgb"]).save(a, format="PNG")
        Image.fromarray(im["sem_gt"]).save(b, format="PNG")
        pngs.append((a.getvalue(), b.getvalue()))

    def decode(which):
        def fn():
            for pair in pngs:
                img = Image.open(io.BytesIO(pair[which]))
                np.array(img.convert("RGB") if which == 0 else img)
        return fn
    per = lambda d: round(d["median_ms"] / k, 3)  # noqa: E731
    res["host"] = dict(images=k, clock="host clock", numpy_confusion_values_ms_per_image=per(host_clock(numpy_confusion, 3)),
                       numpy_pair_counts_ms_per_image=per(host_clock(numpy_pairs, 3)), png_decode_panoptic_ms_per_image=per(host_clock(decode(0), 5)),
                       png_decode_sem_seg_ms_per_image=per(host_clock(decode(1), 5)), png_bytes=[len(pngs[0][0]), len(pngs[0][1])])
    steps = ("confusion_values", "confusion_labels", "pair_counts", "pq_accumulate")
    res["all_hip_steps_faster"] = all(res[s]["hip_faster"] for s in steps)
    res["all_results_equal"] = all(res[s]["results_equal"] for s in steps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
