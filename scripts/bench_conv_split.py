"""What the split parity mode (OpensetRCNNEngine dtype=float32, conv="split": fp32 storage, the convolutions and FC1 / FC2 as two bf16
terms per operand and three bf16 MFMA products, csrc/osr_conv_split.hip) costs and gives against the fp32 parity mode, in one process.
Batch 16 of 3x800x1333 synthetic uint8 images, random-init weights (weights.random_params, seed 0), one GPU.

  1. The captured single pass (hipGraph, one lane, one stream) of the fp32 parity mode and of the split parity mode: after 2 warm-up
     replays each, STEPS replays each, alternated one by one; the pair of measurements is taken twice (the spread).
  2. Single layers at the pass's shapes, osr_conv2d_fwd with fp32 operands against osr_conv2d_split_fwd on the same random inputs:
     the stem, conv1 / conv2 / conv3 of a block of each stage, fpn_output2 and the CF-RPN head's conv over p2; after WARMUP launches,
     the median of LAUNCHES launches timed one at a time with HIP events. Per layer: the layer's TFLOP/s on both kernels, the bf16
     TFLOP/s the split kernel issues (three products per element pair) and, for the three largest layers, its share of the bf16 dense
     peak.
  3. Agreement of the split parity mode's final detections with the fp32 parity mode on the tests' four seeded 256x384 images
     (host/agreement.py: same class, IoU >= 0.99, |score difference| <= 1e-2, one to one).
Prints one JSON line and writes it to profiles/conv_split_line.json. Fails without a GPU.

    python scripts/bench_conv_split.py [--steps 20] [--launches 10] [--warmup 3] [--batch 16]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0  # MI355X, dense bf16 matrix peak (vendor figure)


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


def _alternated(graphs, n_images, steps, warm=2):
    """graphs: name -> captured pass. One replay of each in turn, `steps` times, every replay timed on its own."""
    for g in graphs.values():
        for _ in range(warm):
            g.replay()
    torch.cuda.synchronize()
    total = {k: 0.0 for k in graphs}
    for _ in range(steps):
        for k, g in graphs.items():
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            total[k] += time.perf_counter() - t0
    return {k: dict(images_per_sec=round(n_images * steps / v, 1), ms_per_pass=round(v / steps * 1e3, 3)) for k, v in total.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_split.py needs a GPU")
    ge.load_package()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.agreement import detection_agreement
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_stem_weight, random_params, split_conv_weight, split_stem_weight, with_known_unknown_mix
    dev = "cuda:0"
    n, h, w = args.batch, 800, 1333
    hp, wp = 800, 1344
    g = torch.Generator().manual_seed(99)
    images = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    image_hw = torch.tensor([(h, w)] * n, dtype=torch.int32, device=dev)
    params = random_params(0)

    # ---- 1. the captured passes, alternated; the pair twice ----
    engines = dict(fp32=OpensetRCNNEngine(params, dtype=torch.float32, device=dev), split=OpensetRCNNEngine(params, dtype=torch.float32, device=dev, conv="split"))
    captured = {k: e.capture(images, image_hw, hp, wp, 1) for k, e in engines.items()}
    graphs = {k: c[0] for k, c in captured.items()}
    passes = [_alternated(graphs, n, args.steps) for _ in range(2)]
    for p in passes:
        p["split_over_fp32"] = round(p["split"]["images_per_sec"] / p["fp32"]["images_per_sec"], 3)
    del captured, graphs, engines
    torch.cuda.empty_cache()

    # ---- 2. single layers at the pass's shapes ----
    layers = {}

    def layer(name, cin, cout, k, hh, ww, relu=True):
        gl = torch.Generator().manual_seed(len(layers))
        x = torch.randn(n, hh, ww, cin, generator=gl).clamp(min=0).to(dev)
        wt = torch.randn(cout, cin, k, k, generator=gl) * (2.0 / (k * k * cin)) ** 0.5
        b = torch.zeros(cout, device=dev)
        w32, ws = pack_conv_weight(wt, torch.float32).to(dev), tuple(t.to(dev) for t in split_conv_weight(wt))
        pad = k // 2
        r = dict(shape=f"{k}x{k} {cin}->{cout} at {n}x{hh}x{ww}", gflop=round(2.0 * n * hh * ww * cout * k * k * cin / 1e9, 2),
                 f32=_timed(lambda: ops.conv2d(x, w32, b, 1, pad, relu), args.warmup, args.launches),
                 split=_timed(lambda: ops.conv2d_split(x, ws, b, 1, pad, relu), args.warmup, args.launches))
        layers[name] = r

    xpad = ops.preprocess(images, hp, wp, (103.53, 116.28, 123.675), (1.0, 1.0, 1.0), dtype=torch.float32)
    sw = params["backbone.bottom_up.stem.conv1.weight"]
    sb = torch.zeros(64, device=dev)
    sw32, sws = pack_stem_weight(sw, torch.float32).to(dev), tuple(t.to(dev) for t in split_stem_weight(sw))
    layers["stem"] = dict(shape=f"7x7/2 3->64 at {n}x{hp}x{wp}", gflop=round(2.0 * n * (hp // 2) * (wp // 2) * 64 * 147 / 1e9, 2),
                          f32=_timed(lambda: ops.stem_conv(xpad, sw32, sb, hp, wp), args.warmup, args.launches),
                          split=_timed(lambda: ops.stem_conv_split(xpad, sws, sb, hp, wp), args.warmup, args.launches))
    del xpad
    for stage, c in ((2, 64), (3, 128), (4, 256), (5, 512)):
        hh, ww = hp >> stage, wp >> stage
        layer(f"res{stage}.1.conv1", 4 * c, c, 1, hh, ww)
        layer(f"res{stage}.1.conv2", c, c, 3, hh, ww)
        layer(f"res{stage}.1.conv3", c, 4 * c, 1, hh, ww)
        torch.cuda.empty_cache()
    layer("fpn_output2", 256, 256, 3, hp >> 2, wp >> 2, relu=False)
    layer("rpn_head.conv(p2)", 256, 256, 3, hp >> 2, wp >> 2)
    torch.cuda.empty_cache()
    largest = sorted(layers, key=lambda k: -layers[k]["gflop"])[:3]
    for name, r in layers.items():
        r["f32_over_split"] = round(r["f32"]["median_ms"] / r["split"]["median_ms"], 2)
        r["f32_layer_tflops"] = round(r["gflop"] / r["f32"]["median_ms"], 1)
        r["split_layer_tflops"] = round(r["gflop"] / r["split"]["median_ms"], 1)  # the layer's FLOPs ...
        r["split_bf16_tflops"] = round(3.0 * r["gflop"] / r["split"]["median_ms"], 1)  # ... and the three bf16 products the kernel spends on each
        if name in largest:
            r["share_of_bf16_dense_peak"] = round(r["split_bf16_tflops"] / BF16_DENSE_PEAK_TFLOPS, 3)

    # ---- 3. detection agreement with the fp32 parity mode on the tests' four 256 x 384 images ----
    sn, sh, sw_ = 4, 256, 384
    g = torch.Generator().manual_seed(2024)
    small = torch.randint(0, 256, (sn, 3, sh, sw_), generator=g, dtype=torch.uint8).to(dev)
    sizes = [(sh, sw_), (sh, sw_), (sh - 16, sw_ - 40), (sh - 6, sw_)]
    keep = {}
    e32 = OpensetRCNNEngine(params, dtype=torch.float32, device=dev)
    e32.forward(small, sizes, keep=keep)
    cnt = keep["cnt1"].cpu()
    emb = torch.cat([keep["emb"].view(sn, 1000, -1)[i, :int(cnt[i])] for i in range(sn)]).cpu()
    mixed = with_known_unknown_mix(params, emb)
    del e32, keep

    def dets(**kw):
        e = OpensetRCNNEngine(mixed, dtype=torch.float32, device=dev, **kw)
        out = e.forward(small, sizes)
        torch.cuda.synchronize()
        return [(d["pred_boxes"], d["scores"], d["pred_classes"]) for d in e.to_instances(out, sn)]

    a = detection_agreement(dets(conv="split"), dets())
    agreement = dict(fraction=round(a["fraction"], 4), matched=a["matched"], reference_detections=a["reference_detections"],
                     max_score_abs_diff=a["max_score_abs_diff"], max_box_abs_diff_px=a["max_box_abs_diff_px"])
    line = json.dumps(dict(batch=n, image="3x800x1333", steps=args.steps, launches=args.launches, passes=passes, layers=layers,
                           largest_layers=largest, bf16_dense_peak_tflops=BF16_DENSE_PEAK_TFLOPS, agreement_with_fp32_parity_mode=agreement))
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "conv_split_line.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
