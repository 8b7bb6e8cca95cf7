"""The mask branch of the stock heads (MODEL.MASK_ON) at the benchmark's shape: batch 16 at 800 x 1333, 100 detections per image.

Per-launch device-event times (median of LAUNCHES, interleaved) of the 14 x 14 pooler, the four mask_fcn convolutions, the fused
deconv + predictor + sigmoid launch (osr_mask_upsample_predict) and the paste of one image's 100 masks at 800 x 1333, on full lists
of 100 seeded boxes per image; the fused launch against the unfused composition of the ops the library had before it -- a 1 x 1
osr_conv2d_fwd to 4 x Cmid channels (+ bias, ReLU), a pixel shuffle, osr_gemm_f32 with the predictor row, a sigmoid -- whose
(R, 28, 28, Cmid) intermediate goes through HBM; and the whole stock pass (eager, one stream) with and without the mask head.

Writes profiles/mask_head_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LAUNCHES, WARMUP = 10, 2
N, TOPK, H, W = 16, 100, 800, 1333
SC = (0.25, 0.125, 0.0625, 0.03125)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_head_line.json"))
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.weights import pack_conv_weight, random_standard_params
    dt = getattr(torch, args.dtype)
    base = random_standard_params(0)
    g = torch.Generator().manual_seed(4000)
    mp = mask_params(g, 1)  # CLS_AGNOSTIC_MASK True, as Base-RCNN-FPN.yaml sets it
    eng = StandardRCNNEngine({**base, **mp}, dtype=dt, device="cuda:0")
    eng0 = StandardRCNNEngine(base, dtype=dt, device="cuda:0")
    images = torch.randint(0, 256, (N, 3, H, W), generator=torch.Generator().manual_seed(1234), dtype=torch.uint8).cuda()
    hw = torch.tensor([(H, W)] * N, dtype=torch.int32, device="cuda")
    keep = {}
    res = eng.forward_device(images, hw, 800, 1344, keep)
    torch.cuda.synchronize()
    feats = keep["feats"]
    result = dict(batch=N, image=f"3x{H}x{W}", detections_per_image=TOPK, dtype=args.dtype, launches=LAUNCHES, device=torch.cuda.get_device_name(0),
                  detections_of_the_pass=[int(c) for c in res[3].cpu()])

    # full lists of seeded boxes: 100 per image, 16 .. 500 px a side
    ctr = torch.rand(N, TOPK, 2, generator=g) * torch.tensor([W * 1.0, H * 1.0])
    size = torch.exp(torch.rand(N, TOPK, 2, generator=g) * 3.4 + 2.8)
    boxes = torch.cat(((ctr - size / 2).clamp(min=0), torch.minimum(ctr + size / 2, torch.tensor([W * 1.0, H * 1.0]))), dim=2).cuda().contiguous()
    classes = torch.zeros((N, TOPK), dtype=torch.int64, device="cuda")
    counts = torch.full((N,), TOPK, dtype=torch.int32, device="cuda")
    bidx = torch.arange(N, dtype=torch.int32, device="cuda").repeat_interleave(TOPK)
    fl = [feats[k] for k in ("p2", "p3", "p4", "p5")]
    r = N * TOPK
    x0 = ops.roi_align(fl, SC, boxes.view(-1, 4), bidx, 14, dt)
    x = x0
    xs = [x0]
    for i in range(4):
        x = eng._conv(x, f"roi_heads.mask_head.mask_fcn{i + 1}", 1, 1, relu=True)
        xs.append(x)
    fused = lambda: ops.mask_upsample_predict(x, eng.mask_deconv_w, eng.mask_deconv_b, eng.mask_pred_w, eng.mask_pred_b, classes.view(-1), counts, TOPK)  # noqa: E731

    # the unfused composition: deconv as a 1x1 convolution to (tap, channel) columns, pixel shuffle, fp32 GEMM with the predictor row
    dw = mp["roi_heads.mask_head.deconv.weight"]  # (cin, cmid, 2, 2)
    w1 = pack_conv_weight(dw.permute(2, 3, 1, 0).reshape(4 * 256, 256, 1, 1), dt).cuda()
    b1 = mp["roi_heads.mask_head.deconv.bias"].float().repeat(4).cuda()

    def unfused():
        hcol = ops.conv2d(x, w1, b1, 1, 0, True)  # (r, 14, 14, 4 * 256): column t * 256 + n
        hpix = hcol.view(r, 14, 14, 2, 2, 256).permute(0, 1, 3, 2, 4, 5).float().reshape(r * 784, 256)  # (r, y, dy, x, dx, n) fp32 rows
        return torch.sigmoid(ops.gemm_f32(hpix, eng.mask_pred_w, eng.mask_pred_b)).view(r, 28, 28)
    a, b = fused(), unfused()
    torch.cuda.synchronize()
    result["fused_vs_unfused_max_abs_diff"] = float((a - b).abs().max())

    probs = a.view(N, TOPK, 28, 28)
    pb = boxes[0].contiguous()
    fns = {"pooler_14x14": lambda: ops.roi_align(fl, SC, boxes.view(-1, 4), bidx, 14, dt),
           "pooler_7x7_same_rois": lambda: ops.roi_align(fl, SC, boxes.view(-1, 4), bidx, 7, dt),
           "fused_deconv_predictor": fused, "unfused_conv1x1_shuffle_gemm": unfused,
           "paste_100_masks_one_image": lambda: ops.paste_masks(probs[0], pb, H, W)}
    for i in range(4):
        fns[f"mask_fcn{i + 1}"] = (lambda i=i: eng._conv(xs[i], f"roi_heads.mask_head.mask_fcn{i + 1}", 1, 1, relu=True))
    t = interleaved(fns)
    t["four_convolutions_median_ms"] = round(sum(t[f"mask_fcn{i + 1}"]["median_ms"] for i in range(4)), 4)
    flops = 2.0 * r * 196 * 256 * 1024
    t["fused_tflops"] = round(flops / t["fused_deconv_predictor"]["median_ms"] * 1e-9, 1)
    t["unfused_over_fused"] = round(t["unfused_conv1x1_shuffle_gemm"]["median_ms"] / t["fused_deconv_predictor"]["median_ms"], 2)
    result["launches_ms"] = t
    print(json.dumps(t), flush=True)

    passes = interleaved({"stock_pass_with_mask_head": lambda: eng.forward_device(images, hw, 800, 1344),
                          "stock_pass_without": lambda: eng0.forward_device(images, hw, 800, 1344)}, launches=6)
    result["passes_ms"] = passes
    print(json.dumps(passes), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
