"""The keypoint branch of the stock heads (MODEL.KEYPOINT_ON) at the benchmark's shape: batch 16 at 800 x 1333, up to 100 detections
per image, KRCNNConvDeconvUpsampleHead with eight 512-channel layers and 17 keypoints.

Device-event times, median of LAUNCHES, interleaved:
  - the stock pass (eager, one stream) of a one-class detector without the branch, and the same pass followed by the keypoint head on
    seeded person-like boxes with 5 and with 100 live rows per image (the fill of the padded lists is set here, not left to what
    random weights detect);
  - the head's steps at both fills: the 14 x 14 pooler, the eight conv_fcn layers (row segments: padded rows are skipped), the fused
    tail osr_keypoint_upsample, osr_heatmaps_to_keypoints;
  - the fused tail against F.conv_transpose2d + F.interpolate on the device (same dtype, NCHW), 1600 RoIs;
  - osr_heatmaps_to_keypoints against detectron2's per-RoI loop in torch on the device (F.interpolate bicubic to the box size, argmax,
    the score's exp-sum), 16 x 100 RoIs with sides of 50 .. 400 px.

Writes profiles/keypoint_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LAUNCHES, WARMUP = 10, 2
N, TOPK, H, W, K = 16, 100, 800, 1333, 17
DIMS = (512,) * 8


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


def keypoint_params(g):
    pre, p, cur = "roi_heads.keypoint_head.", {}, 256
    for i, d in enumerate(DIMS):
        p[f"{pre}conv_fcn{i + 1}.weight"] = torch.randn(d, cur, 3, 3, generator=g) * (2.0 / (d * 9)) ** 0.5
        p[f"{pre}conv_fcn{i + 1}.bias"] = torch.zeros(d)
        cur = d
    p[pre + "score_lowres.weight"] = torch.randn(cur, K, 4, 4, generator=g) * (2.0 / (cur * 16)) ** 0.5
    p[pre + "score_lowres.bias"] = torch.zeros(K)
    return p


def torch_decode_loop(maps, rois):
    """[d2] heatmaps_to_keypoints as detectron2 runs it: a Python loop over the RoIs, every step on the device."""
    r, k = maps.shape[:2]
    out = maps.new_zeros((r, k, 4))
    wh = (rois[:, 2:] - rois[:, :2]).clamp(min=1)
    whc = wh.ceil()
    sizes = whc.to(torch.int64).cpu().tolist()  # (the one host sync [d2] has too: the resized shapes)
    corr = wh / whc
    for i in range(r):
        wc, hc = sizes[i]
        u = F.interpolate(maps[i:i + 1], size=(hc, wc), mode="bicubic", align_corners=False)[0].reshape(k, -1)
        best, pos = u.max(dim=1)
        out[i, :, 0] = ((pos % wc).float() + 0.5) * corr[i, 0] + rois[i, 0]
        out[i, :, 1] = (torch.div(pos, wc, rounding_mode="floor").float() + 0.5) * corr[i, 1] + rois[i, 1]
        out[i, :, 2] = best
        out[i, :, 3] = 1.0 / torch.exp(maps[i].reshape(k, -1) - best[:, None]).sum(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_line.json"))
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--skip-torch", action="store_true", help="leave the two torch-device baselines out")
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.weights import random_standard_params
    dt = getattr(torch, args.dtype)
    base = random_standard_params(0, num_classes=1)
    g = torch.Generator().manual_seed(4100)
    kp = keypoint_params(g)
    cfg = dict(std_num_classes=1)
    eng = StandardRCNNEngine({**base, **kp}, cfg, dtype=dt, device="cuda:0")
    eng0 = StandardRCNNEngine(base, cfg, dtype=dt, device="cuda:0")
    images = torch.randint(0, 256, (N, 3, H, W), generator=torch.Generator().manual_seed(1234), dtype=torch.uint8).cuda()
    hw = torch.tensor([(H, W)] * N, dtype=torch.int32, device="cuda")
    keep = {}
    res = eng0.forward_device(images, hw, 800, 1344, keep)
    torch.cuda.synchronize()
    feats = keep["feats"]
    result = dict(batch=N, image=f"3x{H}x{W}", detections_per_image=TOPK, conv_dims=list(DIMS), num_keypoints=K, dtype=args.dtype, launches=LAUNCHES,
                  device=torch.cuda.get_device_name(0), detections_of_the_pass=[int(c) for c in res[3].cpu()])

    # full lists of seeded person-like boxes: 100 per image, 50 .. 400 px a side
    size = torch.rand(N, TOPK, 2, generator=g) * 350 + 50
    tl = torch.rand(N, TOPK, 2, generator=g) * (torch.tensor([W * 1.0, H * 1.0]) - size)
    boxes = torch.cat((tl, tl + size), dim=2).cuda().contiguous()
    fills = {f: torch.full((N,), f, dtype=torch.int32, device="cuda") for f in (5, 100)}

    def run(write):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh)
            fh.write("\n")
        if write:
            print("wrote", args.out)

    # ---- the head's steps at both fills ----
    flat = boxes.view(-1, 4)
    steps = {}
    for f, cnt in fills.items():
        bidx = ops.padded_batch_idx(cnt, TOPK)
        seg = (cnt * 196, TOPK * 196)
        xs = [eng.pool_keypoint_rois(feats, flat, bidx)]
        for i in range(len(DIMS)):
            xs.append(eng._conv(xs[-1], f"roi_heads.keypoint_head.conv_fcn{i + 1}", 1, 1, relu=True, row_seg=seg))
        heat = ops.keypoint_upsample(xs[-1], eng.keypoint_deconv_w, eng.keypoint_deconv_b, cnt, TOPK)
        fns = {"pooler_14x14": lambda bidx=bidx: eng.pool_keypoint_rois(feats, flat, bidx),
               "keypoint_upsample": lambda xs=xs, cnt=cnt: ops.keypoint_upsample(xs[-1], eng.keypoint_deconv_w, eng.keypoint_deconv_b, cnt, TOPK),
               "heatmaps_to_keypoints": lambda heat=heat, cnt=cnt: ops.heatmaps_to_keypoints(heat, flat, cnt, TOPK)}
        for i in range(len(DIMS)):
            fns[f"conv_fcn{i + 1}"] = (lambda i=i, xs=xs, seg=seg: eng._conv(xs[i], f"roi_heads.keypoint_head.conv_fcn{i + 1}", 1, 1, relu=True, row_seg=seg))
        t = interleaved(fns)
        t["eight_convolutions_median_ms"] = round(sum(t[f"conv_fcn{i + 1}"]["median_ms"] for i in range(len(DIMS))), 4)
        steps[f"fill_{f}"] = t
        if f == 100:
            x_full, heat_full = xs[-1], heat
        print(json.dumps({f"fill_{f}": t}), flush=True)
    result["head_steps_ms"] = steps

    # ---- the pass without the branch, and followed by the head at both fills ----
    fns = {"stock_pass_without": lambda: eng0.forward_device(images, hw, 800, 1344)}
    for f, cnt in fills.items():
        fns[f"stock_pass_then_keypoint_head_fill_{f}"] = (lambda cnt=cnt: (eng0.forward_device(images, hw, 800, 1344), eng._keypoint_head(feats, boxes, cnt)))
    result["passes_ms"] = interleaved(fns)
    print(json.dumps(result["passes_ms"]), flush=True)
    result["torch_baselines"] = "not measured"
    run(False)

    if not args.skip_torch:
        # ---- Kernel A against torch on the device ----
        w = kp["roi_heads.keypoint_head.score_lowres.weight"].to(dt).cuda()
        b = kp["roi_heads.keypoint_head.score_lowres.bias"].to(dt).cuda()
        x_nchw = x_full.permute(0, 3, 1, 2).contiguous()
        cnt = fills[100]

        def torch_tail():
            return F.interpolate(F.conv_transpose2d(x_nchw, w, b, stride=2, padding=1).float(), scale_factor=2, mode="bilinear", align_corners=False)
        a, c = ops.keypoint_upsample(x_full, eng.keypoint_deconv_w, eng.keypoint_deconv_b, cnt, TOPK), torch_tail()
        torch.cuda.synchronize()
        tb = dict(tail_max_abs_diff=float((a - c).abs().max()))
        t = interleaved({"keypoint_upsample": lambda: ops.keypoint_upsample(x_full, eng.keypoint_deconv_w, eng.keypoint_deconv_b, cnt, TOPK),
                         "torch_conv_transpose2d_interpolate": torch_tail})
        t["torch_over_fused"] = round(t["torch_conv_transpose2d_interpolate"]["median_ms"] / t["keypoint_upsample"]["median_ms"], 2)
        tb["tail_ms"] = t
        print(json.dumps(t), flush=True)
        # ---- Kernel B against the per-RoI torch loop on the device ----
        d1, d2 = ops.heatmaps_to_keypoints(heat_full, flat, cnt, TOPK), torch_decode_loop(heat_full, flat)
        torch.cuda.synchronize()
        tb["decode_positions_equal_share"] = float(((d1[..., :2] - d2[..., :2]).abs().amax(dim=-1) < 1e-3).float().mean())
        t = interleaved({"heatmaps_to_keypoints": lambda: ops.heatmaps_to_keypoints(heat_full, flat, cnt, TOPK),
                         "torch_per_roi_loop": lambda: torch_decode_loop(heat_full, flat)})
        t["torch_over_fused"] = round(t["torch_per_roi_loop"]["median_ms"] / t["heatmaps_to_keypoints"]["median_ms"], 2)
        tb["decode_ms"] = t
        print(json.dumps(t), flush=True)
        result["torch_baselines"] = tb
    run(True)


if __name__ == "__main__":
    main()
