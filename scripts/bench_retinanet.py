"""META_ARCHITECTURE "RetinaNet" (host/engine_retinanet.py) at the benchmark's shape: 16 synthetic 800 x 1333 uint8 frames, fp16, K = 80,
seeded synthetic weights. In one run, the two sides of every comparison interleaved, medians of device-event times:

  (a) pass            the RetinaNet engine pass against the stock Faster R-CNN engine pass (eager launches, one stream);
  (b) launches        per-launch times of one profiled RetinaNet pass: the eight tower launches, cls_score, select, NMS;
  (c) select          ops.retinanet_select alone on synthetic logits of the pass's geometry, two ways: "sparse" (trained-like: bias -4.595,
                      about 1 % of the logits above logit(0.05)) and "all_pass" (every logit above the threshold: the survivor lists
                      overflow and the exact pass over the logits runs). Time and achieved bytes/s over the algorithmic bytes (the
                      logits once + the outputs);
  (d) torch_ops       the same selection composed from torch device ops (sigmoid, >, nonzero, sort, index arithmetic, decode).

Writes profiles/retinanet_line.json (or --out)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N, H, W, K, A, TOPK = 16, 800, 1333, 80, 9, 1000
DEV = "cuda:0"
CLAMP = math.log(1000.0 / 16.0)


def events(fns, reps, warmup=2):
    """Median device-event time of each fn, the fns alternating inside every repetition."""
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[i].append(e0.elapsed_time(e1))
    return [dict(median_ms=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=reps) for t in times]


def torch_select(logits_lv, deltas_lv, anchors, strides, thresh_score, topk):
    """[d2] RetinaNet.inference_single_image before the NMS, per (image, level), from torch device ops. logits_lv[l] (n, h, w, A*K),
    deltas_lv[l] (n, h, w, A*4) fp32. No padding to fixed capacities: what a direct port would run."""
    out = []
    for l, (lg, dl) in enumerate(zip(logits_lv, deltas_lv)):
        n, h, w, _ = lg.shape
        for img in range(n):
            s = torch.sigmoid(lg[img].reshape(-1).float())
            idx = torch.nonzero(s > thresh_score).reshape(-1)
            sc, order = torch.sort(s[idx], descending=True)
            order = order[:topk]
            idx, sc = idx[order], sc[:topk]
            t = torch.div(idx, K, rounding_mode="floor")
            cls = idx - t * K
            cell = torch.div(t, A, rounding_mode="floor")
            a = t - cell * A
            d = dl[img].reshape(-1, 4)[t]
            sx, sy = ((cell % w) * strides[l]).float(), (torch.div(cell, w, rounding_mode="floor") * strides[l]).float()
            ca = anchors[l][a]
            ax1, ay1, ax2, ay2 = sx + ca[:, 0], sy + ca[:, 1], sx + ca[:, 2], sy + ca[:, 3]
            aw, ah = ax2 - ax1, ay2 - ay1
            cx, cy = ax1 + 0.5 * aw, ay1 + 0.5 * ah
            pw, ph = torch.exp(d[:, 2].clamp(max=CLAMP)) * aw, torch.exp(d[:, 3].clamp(max=CLAMP)) * ah
            pcx, pcy = d[:, 0] * aw + cx, d[:, 1] * ah + cy
            out.append((torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1), sc, cls))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retinanet_line.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retinanet.py measures on the GPU; none found")
    ge.load_package()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_retinanet import RetinaNetEngine
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.weights import random_retinanet_params, random_standard_params
    n = args.batch
    res = dict(gpu=torch.cuda.get_device_name(0), batch=n, image=[H, W], dtype="float16", num_classes=K, topk=TOPK)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    hw = torch.tensor([(H, W)] * n, dtype=torch.int32, device=DEV)
    hp, wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    retina = RetinaNetEngine(random_retinanet_params(0), None, torch.float16, DEV)
    stock = StandardRCNNEngine(random_standard_params(0), None, torch.float16, DEV)

    # (a) the two passes, interleaved
    ra, sa = events([lambda: retina.forward_device(images, hw, hp, wp), lambda: stock.forward_device(images, hw, hp, wp)], args.reps)
    res["pass"] = dict(retinanet=ra, stock_faster_rcnn=sa, ratio=round(ra["median_ms"] / sa["median_ms"], 3),
                       retinanet_images_per_s=round(n / ra["median_ms"] * 1e3, 1), stock_images_per_s=round(n / sa["median_ms"] * 1e3, 1))

    # (b) one profiled pass, per launch
    retina.profile, retina.profile_hbm = [], []
    keep = {}
    retina.forward_device(images, hw, hp, wp, keep)
    torch.cuda.synchronize()
    prof, hbm = retina.resolve_profile()
    retina.profile = retina.profile_hbm = None
    groups = {}
    for name, flops, e0, e1, nbytes, _ in prof:
        key = "towers" if "subnet" in name else name if name in ("head.cls_score", "head.bbox_pred") else "trunk + FPN"
        d = groups.setdefault(key, dict(ms=0.0, launches=0, flops=0.0))
        d["ms"] += e0.elapsed_time(e1); d["launches"] += 1; d["flops"] += flops
    for d in groups.values():
        d["tflops"] = round(d["flops"] / d["ms"] / 1e9, 1)
        d["ms"] = round(d["ms"], 3)
        del d["flops"]
    res["launches"] = dict(groups=groups, towers=[dict(name=nm, ms=round(e0.elapsed_time(e1), 3)) for nm, _, e0, e1, _, _ in prof if "subnet" in nm],
                           hbm=[dict(name=nm, ms=round(e0.elapsed_time(e1), 3), algorithmic_gb_per_s=round(nb / e0.elapsed_time(e1) / 1e6, 1)) for nm, nb, e0, e1, _ in hbm],
                           candidates_passing=int(keep["cands"]["counts"].sum()), note="one profiled pass (events between launches), not a median")
    del keep

    # (c) + (d) the select alone on the pass's geometry
    h5, w5 = hp // 32, wp // 32
    dims = [(hp // 8, wp // 8), (hp // 16, wp // 16), (h5, w5), ((h5 - 1) // 2 + 1, (w5 - 1) // 2 + 1)]
    dims.append(((dims[3][0] - 1) // 2 + 1, (dims[3][1] - 1) // 2 + 1))
    strides = (8, 16, 32, 64, 128)
    lv = ops.make_rpn_levels(dims, strides, n, A)
    anchors = retina.cell_anchors
    cells = sum(n * h * w for h, w in dims)
    gd = torch.Generator(device=DEV).manual_seed(1)
    deltas = (torch.rand((cells * 4 * A,), generator=gd, device=DEV) * 2 - 1) * 0.5
    thr = ops.retinanet_logit_thresh(0.05)
    res["select"] = {}
    for case in ("sparse", "all_pass"):
        logits = torch.randn((cells * A * K,), generator=gd, device=DEV, dtype=torch.float32)
        # sparse: N(-4.595, 0.71^2): logit(0.05) = -2.944 lies 2.33 sigma above the bias, 1 % pass. all_pass: nothing below -2.9
        logits = (logits.clamp_(min=-2.9) if case == "all_pass" else logits.mul_(0.71).add_(-4.595)).to(torch.float16)
        frac = float((logits.float() > thr).float().mean())
        lg_lv, dl_lv, off = [], [], 0
        for h, w in dims:
            lg_lv.append(logits[off * A * K:(off + n * h * w) * A * K].view(n, h, w, A * K))
            dl_lv.append(deltas[off * A * 4:(off + n * h * w) * A * 4].view(n, h, w, A * 4))
            off += n * h * w
        out = ops.retinanet_select(lv, anchors, logits, deltas, n, K, TOPK, 0.05)
        nbytes = logits.numel() * 2 + n * 5 * TOPK * (16 + 4 * 4) + int(out["counts"].sum()) * 16
        fns = [lambda: ops.retinanet_select(lv, anchors, logits, deltas, n, K, TOPK, 0.05, out=out)]
        if case != "all_pass" or n <= 16:
            fns.append(lambda: torch_select(lg_lv, dl_lv, anchors, strides, 0.05, TOPK))
        t = events(fns, args.reps)
        entry = dict(fraction_above_threshold=round(frac, 5), kernel=t[0], algorithmic_bytes=nbytes,
                     kernel_gb_per_s=round(nbytes / t[0]["median_ms"] / 1e6, 1))
        if len(t) > 1:
            entry.update(torch_ops=t[1], torch_over_kernel=round(t[1]["median_ms"] / t[0]["median_ms"], 2))
        res["select"][case] = entry
        del logits, lg_lv, out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
