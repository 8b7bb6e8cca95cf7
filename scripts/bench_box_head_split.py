"""What the split-precision box head (OpensetRCNNEngine box_head="split": fp32 pooled rows and fp32 weights as two bf16 terms each,
three bf16 MFMA products, csrc/osr_linear_split.hip) costs and gives, in one process. Batch 16 of 3x800x1333 synthetic uint8 images,
random-init weights (weights.random_params, seed 0), one GPU.

  1. fc1 / fc2 alone on the real pooled rows of that pass (the first count[i] rows of every image's list, packed): the fp32 kernel
     (ops.linear on fp32 tensors), the split kernel (ops.linear_split) and the fp16 kernel (ops.linear on fp16 tensors); after
     WARMUP launches, the median of LAUNCHES launches timed one at a time with HIP events.
  2. The captured single pass (hipGraph, one lane, one stream) replayed STEPS times after 2 warm-up replays, as bench.py's graph_rate
     does, for the fast mode, for fp32_points=("pooled", "h1") (the fp32-kernel box head) and for box_head="split".
  3. Agreement of the three modes' final detections with the fp32 parity mode on the tests' four seeded 256x384 images
     (host/agreement.py: same class, IoU >= 0.99, |score difference| <= 1e-2, one to one).
Prints one JSON line.

    python scripts/bench_box_head_split.py [--steps 20] [--launches 20] [--warmup 5] [--batch 16]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def _timed(fn, warm, k):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return dict(median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4), max_ms=round(times[-1], 4))


def _graph_rate(eng, images, image_hw, steps, warm=2):
    graph, out = eng.capture(images, image_hw, 800, 1344, 1)
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    del graph, out
    return dict(images_per_sec=round(images.shape[0] / dt, 1), ms_per_pass=round(dt * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    ge.load_package()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.agreement import detection_agreement
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import random_params, with_known_unknown_mix
    dev = "cuda:0"
    n, h, w = args.batch, 800, 1333
    g = torch.Generator().manual_seed(99)
    images = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    image_hw = torch.tensor([(h, w)] * n, dtype=torch.int32, device=dev)
    params = random_params(0)
    modes = dict(fast={}, fp32_points_pooled_h1=dict(fp32_points=("pooled", "h1")), split=dict(box_head="split"))

    # ---- 1. the two layers alone, on the real rows of the pass ----
    eng = OpensetRCNNEngine(params, dtype=torch.float16, device=dev, box_head="split")
    keep = {}
    eng.forward(images, [(h, w)] * n, keep=keep)
    torch.cuda.synchronize()
    cap, counts = keep["sel"]["cap"], [int(c) for c in keep["sel"]["counts"].cpu()]
    pooled = keep["pooled"].view(n, cap, -1)
    x1 = torch.cat([pooled[i, :counts[i]] for i in range(n)]).contiguous()
    hh = keep["h1"].view(n, cap, -1)
    x2 = torch.cat([hh[i, :counts[i]] for i in range(n)]).contiguous()
    del keep, pooled, hh
    layers = {}
    for name, x, split_w, bias in (("fc1", x1, eng.fc1_split, eng.fc1_b), ("fc2", x2, eng.fc2_split, eng.fc2_b)):
        w32 = (split_w[0].float() + split_w[1].float()).contiguous()  # (the fp32 weight to 2^-17: timing operands)
        w16, x16 = w32.half(), x.half()
        m, k = x.shape
        fl = 2.0 * m * k * w32.shape[0]
        ops.LINEAR_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
        r = dict(rows=m, k=k, n=w32.shape[0],
                 f32=_timed(lambda: ops.linear(x, w32, bias, relu=True, out_dtype=torch.float32), args.warmup, args.launches),
                 split=_timed(lambda: ops.linear_split(x, split_w, bias, relu=True), args.warmup, args.launches),
                 f16=_timed(lambda: ops.linear(x16, w16, bias, relu=True), args.warmup, args.launches))
        assert ops.LINEAR_SPLIT_COUNT["launches"] == args.warmup + args.launches
        ops.LINEAR_SPLIT_COUNT = None
        r["f32_over_split"] = round(r["f32"]["median_ms"] / r["split"]["median_ms"], 2)
        r["split_over_f16"] = round(r["split"]["median_ms"] / r["f16"]["median_ms"], 2)
        r["split_layer_tflops"] = round(fl / r["split"]["median_ms"] / 1e9, 1)   # the layer's FLOPs; the kernel spends three bf16 products on each
        layers[name] = r
        del w32, w16, x16
    del eng, x1, x2
    torch.cuda.empty_cache()

    # ---- 2. the captured pass of each mode ----
    passes = {}
    for name, kw in modes.items():
        e = OpensetRCNNEngine(params, dtype=torch.float16, device=dev, **kw)
        passes[name] = _graph_rate(e, images, image_hw, args.steps)
        del e
        torch.cuda.empty_cache()

    # ---- 3. detection agreement with the fp32 parity mode on the tests' four 256 x 384 images ----
    sn, sh, sw = 4, 256, 384
    g = torch.Generator().manual_seed(2024)
    small = torch.randint(0, 256, (sn, 3, sh, sw), generator=g, dtype=torch.uint8).to(dev)
    sizes = [(sh, sw), (sh, sw), (sh - 16, sw - 40), (sh - 6, sw)]
    keep = {}
    e32 = OpensetRCNNEngine(params, dtype=torch.float32, device=dev)
    e32.forward(small, sizes, keep=keep)
    cnt = keep["cnt1"].cpu()
    emb = torch.cat([keep["emb"].view(sn, 1000, -1)[i, :int(cnt[i])] for i in range(sn)]).cpu()
    mixed = with_known_unknown_mix(params, emb)
    del e32, keep

    def dets(dtype, **kw):
        e = OpensetRCNNEngine(mixed, dtype=dtype, device=dev, **kw)
        out = e.forward(small, sizes)
        torch.cuda.synchronize()
        return [(d["pred_boxes"], d["scores"], d["pred_classes"]) for d in e.to_instances(out, sn)]

    ref = dets(torch.float32)
    agreement = {}
    for name, kw in modes.items():
        a = detection_agreement(dets(torch.float16, **kw), ref)
        agreement[name] = dict(fraction=round(a["fraction"], 4), matched=a["matched"], reference_detections=a["reference_detections"])
    print(json.dumps(dict(batch=n, image="3x800x1333", steps=args.steps, launches=args.launches, real_rows=layers["fc1"]["rows"], list_rows=n * cap,
                          layers=layers, passes=passes, agreement_with_fp32_parity_mode=agreement)))


if __name__ == "__main__":
    main()
