"""MODEL.RESNETS.STRIDE_IN_1X1 False against True: the Openset train step (batch 16, 3x800x1333, fp16, one GPU, FREEZE_AT 2) in both
layouts, set up as scripts/bench_freeze_at.py sets it up (random-init weights, synthetic images and boxes, WARMUP untimed steps, then
STEPS steps timed one at a time with HIP events). Prints one JSON line: per layout, median / min / max ms per step.

    python scripts/bench_stride_in_3x3.py [--steps 10] [--warmup 3]

--kernel runs only the stride-2 3x3 data gradient (osr_conv2d_dgrad_s2, ReLU mask in the epilogue as the trainer launches it) at the
three layer shapes of the step, res3.0 / res4.0 / res5.0 conv2, ITERS times each -- for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s2 -- python scripts/bench_stride_in_3x3.py --kernel"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def kernel_only(iters: int) -> None:
    from openset_rcnn_amd.host import ops
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    for c, hi, wi in ((128, 200, 336), (256, 100, 168), (512, 50, 84)):
        dy = torch.randn(16, (hi + 1) // 2, (wi + 1) // 2, c, generator=g).half().to(dev)
        wd = (torch.randn(c, 3, 3, c, generator=g) * 0.05).half().to(dev)
        act = torch.randn(16, hi, wi, c, generator=g).half().to(dev)
        for _ in range(iters):
            ops.conv2d_dgrad(dy, wd, (hi, wi), 2, 1, mask=act)
        torch.cuda.synchronize()
    print(json.dumps(dict(kernel="osr_conv2d_dgrad_s2", iters=iters)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ge.load_package()
    if args.kernel:
        kernel_only(args.iters)
        return
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import random_params
    dev = "cuda:0"
    g = torch.Generator().manual_seed(99)
    n, h, w, ngt = 16, 800, 1333, 8
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
    for flag in (True, False):
        tr = OpensetRCNNTrainer(params, dict(stride_in_1x1=flag), dtype=torch.float16, device=dev, lr=1e-5, loss_scale=1024.0, freeze_at=2)
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
        out["stride_in_1x1" if flag else "stride_in_3x3"] = dict(median_ms=round(times[len(times) // 2], 3), min_ms=round(times[0], 3),
                                                                 max_ms=round(times[-1], 3), overflow_steps=tr.overflow_steps)
        del tr
        torch.cuda.empty_cache()
    print(json.dumps(dict(batch=n, steps=args.steps, freeze_at=2, train_step=out)))


if __name__ == "__main__":
    main()
