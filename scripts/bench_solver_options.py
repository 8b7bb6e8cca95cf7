"""Cost of the [d2] solver options on the Openset train step (VOC-COCO yaml, batch 16, 3x800x1333, fp16, one GPU): the update
(osr_check_finite + osr_sgd_step_multi_ex, csrc/osr_solver.hip) with every option off, with value clipping, with norm clipping
(NORM_TYPE 2: the fused norm / overflow pass osr_grad_norm_partials replaces osr_check_finite) and with norm clipping, a bias group
and Nesterov. Random-init weights,
synthetic uint8 images with 8 GT boxes each; WARMUP untimed steps, then STEPS whole steps timed one at a time with HIP events, then
UPDATES update launches alone (the gradient of the last step, re-applied). Prints one JSON line: per variant, median / min / max ms.

    python scripts/bench_solver_options.py [--steps 10] [--warmup 3] [--updates 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def _timed(fn, k):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    ge.load_package()
    from openset_rcnn_amd.host.solver import SolverOptions
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
    variants = {"off": None, "value": SolverOptions(clip="value", clip_value=1e-3),
                "norm": SolverOptions(clip="norm", clip_value=1e-2, norm_type=2.0),
                "norm_bias_nesterov": SolverOptions(bias_lr_factor=2.0, weight_decay_bias=0.0, nesterov=True, clip="norm", clip_value=1e-2)}
    tr = OpensetRCNNTrainer(params, dtype=torch.float16, device=dev, lr=1e-5, loss_scale=1024.0)
    out = {}
    for name, opts in variants.items():
        tr.solver_options = opts
        for _ in range(args.warmup):
            tr.step(*a)
        torch.cuda.synchronize()
        res = dict(step=_timed(lambda: tr.step(*a), args.steps))
        res["update"] = _timed(lambda: tr._update(1), args.updates)
        tr.poll_overflow(wait=True)
        res["overflow_steps"] = tr.overflow_steps
        out[name] = res
    print(json.dumps(dict(batch=n, steps=args.steps, updates=args.updates, grad_mb=round(tr.grad_flat.numel() * 4 / 1e6, 1), variants=out)))


if __name__ == "__main__":
    main()
