"""Faster R-CNN R50-C4 (host/engine_c4.py) at the benchmark's shape: batch 16 at 800 x 1333, res4 = 50 x 84 cells x 15 anchors =
63 000 anchors per image, 6000 into the NMS, 1000 proposals per image into res5.

Device-event times, median of LAUNCHES, interleaved:
  - the whole C4 pass against the stock FPN pass (eager, one stream), and how many proposals / detections the random weights give;
  - the wide select (6000 of 63 000 per image) beside osr_rpn_select at its limit (2048) on the same scores;
  - the pooler on full lists of seeded boxes (16 x 1000): the even bins pooled directly (bin_stride 2) against the full 14 x 14 pool
    followed by subsample2, which give the same tensor;
  - the res5 head on those rows: its three bottlenecks, and the whole box stage (pool, res5, mean, predictor);
  - avgpool_rows against x.float().mean(1) on the device.

Writes profiles/c4_line.json (or --out)."""
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
N, POST, H, W = 16, 1000, 800, 1333


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "c4_line.json"))
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_c4 import C4_FEATURE, RES5, C4RCNNEngine
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.weights import random_c4_params, random_standard_params
    dt = getattr(torch, args.dtype)
    eng = C4RCNNEngine(random_c4_params(0), None, dtype=dt, device="cuda:0")
    fpn = StandardRCNNEngine(random_standard_params(0), None, dtype=dt, device="cuda:0")
    images = torch.randint(0, 256, (N, 3, H, W), generator=torch.Generator().manual_seed(1234), dtype=torch.uint8).cuda()
    hw = torch.tensor([(H, W)] * N, dtype=torch.int32, device="cuda")
    keep = {}
    res = eng.forward_device(images, hw, 800, 1344, keep)
    torch.cuda.synchronize()
    feats, sel = keep["feats"], keep["sel"]
    f = feats[C4_FEATURE]
    result = dict(batch=N, image=f"3x{H}x{W}", res4=list(f.shape), dtype=args.dtype, launches=LAUNCHES, device=torch.cuda.get_device_name(0),
                  proposals_of_the_pass=[int(c) for c in sel["counts"].cpu()], detections_of_the_pass=[int(c) for c in res[3].cpu()])

    def write(final):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh)
            fh.write("\n")
        if final:
            print("wrote", args.out)

    # ---- the whole pass against the stock FPN pass ----
    result["passes_ms"] = interleaved({"c4_pass": lambda: eng.forward_device(images, hw, 800, 1344),
                                       "stock_fpn_pass": lambda: fpn.forward_device(images, hw, 800, 1344)})
    print(json.dumps(result["passes_ms"]), flush=True)
    write(False)

    # ---- the wide select on the pass's own logits and deltas ----
    lv, c = eng._levels(keep["rpn_shapes"], N), eng.cfg
    logits, deltas = keep["rpn_logits"], keep["rpn_deltas"]
    result["anchors_per_image"] = logits.numel() // N
    result["select_ms"] = interleaved({
        "rpn_select_wide_6000": lambda: ops.rpn_select_wide(lv, eng.cell_anchors, logits, deltas, N, hw, 6000, 0.0, b2b_weights=c["rpn_bbox_reg_weights"]),
        "rpn_select_wide_2048": lambda: ops.rpn_select_wide(lv, eng.cell_anchors, logits, deltas, N, hw, 2048, 0.0, b2b_weights=c["rpn_bbox_reg_weights"]),
        "rpn_select_2048": lambda: ops.rpn_select(lv, eng.cell_anchors, logits, deltas, N, hw, 2048, 0.0, b2b_weights=c["rpn_bbox_reg_weights"])})
    print(json.dumps(result["select_ms"]), flush=True)
    write(False)

    # ---- full lists of seeded boxes: 1000 per image, 32 .. 400 px a side ----
    g = torch.Generator().manual_seed(4200)
    size = torch.rand(N, POST, 2, generator=g) * 368 + 32
    tl = torch.rand(N, POST, 2, generator=g) * (torch.tensor([W * 1.0, H * 1.0]) - size)
    boxes = torch.cat((tl, tl + size), dim=2).cuda().contiguous().view(-1, 4)
    counts = torch.full((N,), POST, dtype=torch.int32, device="cuda")
    bidx = ops.padded_batch_idx(counts, POST)
    order = ops.roi_locality_order([f], c["pooler_scales"], boxes, bidx, c["canonical_level"], c["canonical_size"], 4)

    def pool(stride):
        return ops.roi_align([f], c["pooler_scales"], boxes, bidx, 14, dt, c["canonical_level"], c["canonical_size"], 4, order=order, bin_stride=stride)
    a, b = pool(2), ops.subsample2(pool(1))
    torch.cuda.synchronize()
    result["strided_pool_equals_full_pool_subsampled"] = bool(torch.equal(a, b))
    t = interleaved({"pool_even_bins": lambda: pool(2), "pool_full_14x14": lambda: pool(1), "pool_full_then_subsample2": lambda: ops.subsample2(pool(1)),
                     "locality_order": lambda: ops.roi_locality_order([f], c["pooler_scales"], boxes, bidx, c["canonical_level"], c["canonical_size"], 4)})
    t["full_then_subsample_over_even_bins"] = round(t["pool_full_then_subsample2"]["median_ms"] / t["pool_even_bins"]["median_ms"], 3)
    result["pooler_ms"] = t
    print(json.dumps(t), flush=True)
    write(False)

    # ---- res5 on those rows, block by block, and the whole box stage ----
    seg = (counts, POST)
    segs = {49: (counts * 49, POST * 49)}
    xs = [a]
    for blk in range(3):
        xs.append(eng._bottleneck(xs[-1], f"{RES5}.{blk}", blk == 0, 1, row_segs=segs))
    fns = {f"res5_{blk}": (lambda blk=blk: eng._bottleneck(xs[blk], f"{RES5}.{blk}", blk == 0, 1, row_segs=segs)) for blk in range(3)}
    fns["box_stage"] = lambda: eng._box_stage(feats, boxes, bidx, img_seg=seg, fill_padding=False)
    t = interleaved(fns)
    t["three_blocks_median_ms"] = round(sum(t[f"res5_{blk}"]["median_ms"] for blk in range(3)), 4)
    result["res5_head_ms"] = t
    print(json.dumps(t), flush=True)
    write(False)

    # ---- the mean ----
    x = xs[-1].view(N * POST, 49, 2048)
    m1, m2 = ops.avgpool_rows(x), x.float().mean(1)
    torch.cuda.synchronize()
    t = interleaved({"avgpool_rows": lambda: ops.avgpool_rows(x), "avgpool_rows_segments": lambda: ops.avgpool_rows(x, counts, POST),
                     "torch_float_mean": lambda: x.float().mean(1)})
    t["torch_over_avgpool_rows"] = round(t["torch_float_mean"]["median_ms"] / t["avgpool_rows"]["median_ms"], 2)
    t["max_abs_diff_to_torch"] = float((m1 - m2).abs().max())
    t["read_gb_per_s"] = round(x.numel() * x.element_size() / t["avgpool_rows"]["median_ms"] / 1e6, 1)
    result["mean_ms"] = t
    print(json.dumps(t), flush=True)
    write(True)


if __name__ == "__main__":
    main()
