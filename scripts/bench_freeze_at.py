"""The Openset train step (VOC-COCO yaml, batch 16, 3x800x1333, fp16, one GPU) at several MODEL.BACKBONE.FREEZE_AT values: what
training more (or less) of the backbone costs per iteration. Random-init weights, synthetic uint8 images with 8 GT boxes each, a
learning rate small enough that every update is applied; WARMUP untimed steps, then STEPS steps timed one at a time with HIP
events. Prints one JSON line: per value, median / min / max ms per step and the trainable parameter count.

    python scripts/bench_freeze_at.py [--values 0,1,2] [--steps 10] [--warmup 3]

The stem kernels of FREEZE_AT 0 (osr_stem_pool_bwd, osr_stem_wgrad's two launches) and the stem forward's two launches, from a kernel
trace of the FREEZE_AT 0 step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python scripts/bench_freeze_at.py --values 0 --steps 5
    python scripts/bench_freeze_at.py --stats OUT/.../run_kernel_stats.csv"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", default="0,1,2")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel_stats.csv: list the stem kernels' rows and exit")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if args.stats:
        import csv
        with open(args.stats) as f:
            rows = [r for r in csv.DictReader(f) if "stem" in r["Name"] or "maxpool" in r["Name"].lower()]
        print(json.dumps([{k: r[k] for k in ("Name", "Calls", "AverageNs", "TotalDurationNs") if k in r} for r in rows]))
        return
    ge.load_package()
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import random_params
    dev = "cuda:0"
    g = torch.Generator().manual_seed(99)
    n, h, w, ngt = args.batch, 800, 1333, 8
    images = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    hw = torch.tensor([(h, w)] * n, dtype=torch.int32, device=dev)
    ctr = torch.rand(n, ngt, 2, generator=g) * torch.tensor([w * 0.8, h * 0.8]) + 40
    size = torch.rand(n, ngt, 2, generator=g) * 480 + 32
    gt = torch.cat((ctr - size / 2, ctr + size / 2), dim=2)
    gt[..., 0::2].clamp_(0, w)
    gt[..., 1::2].clamp_(0, h)
    gcls = torch.randint(0, 20, (n, ngt), generator=g)
    gcnt = torch.full((n,), ngt, dtype=torch.int32)
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    r = sum(a * b for a, b in shapes)
    cap = sum(min(2000, a * b) for a, b in shapes)
    keys = {k: torch.rand(s, generator=g).to(dev) for k, s in (("rpn_reg", (n, r)), ("rpn_obj", (n, r)), ("roi", (n, cap + ngt)))}
    a = (images, hw, 800, 1344, gt.to(dev), gcls.to(dev), gcnt.to(dev), keys)
    params = random_params(0)
    out = {}
    for v in (int(x) for x in args.values.split(",") if x):
        tr = OpensetRCNNTrainer(params, dtype=torch.float16, device=dev, lr=1e-5, loss_scale=1024.0, freeze_at=v)
        for _ in range(args.warmup):
            tr.step(*a)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.step(*a)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        tr.poll_overflow(wait=True)
        times.sort()
        out[str(v)] = dict(median_ms=round(times[len(times) // 2], 3), min_ms=round(times[0], 3), max_ms=round(times[-1], 3),
                           num_params=tr.num_params, overflow_steps=tr.overflow_steps)
        del tr
        torch.cuda.empty_cache()
    print(json.dumps(dict(batch=n, steps=args.steps, freeze_at=out)))


if __name__ == "__main__":
    main()
