"""What training the box head in split precision (OpensetRCNNTrainer box_head="split": fp32 pooled rows, weights and gradients as two
bf16 terms each, three bf16 MFMA products; csrc/osr_linear_split.hip, csrc/osr_linear_split_bwd.hip) costs, in one run. Batch 16 of
3x800x1333 synthetic uint8 images, random-init weights (weights.random_params, seed 0), one GPU.

  1. The two backward kernels alone at the FC1 / FC2 shapes (m = batch x 512 sampled RoIs): the weight gradient on the split kernel
     (ops.linear_split_wgrad), on the exact-f32 kernel (ops.gemm_f32_tn) and on the fp16 launch it replaces (ops.conv2d_wgrad on 1x1
     views); the data gradient on the split kernel (ops.linear_split_dgrad), on the exact-f32 kernel (ops.linear on fp32 tensors) and
     on the fp16 launch it replaces (ops.conv2d_dgrad). After WARMUP launches, the median of LAUNCHES launches timed one at a time
     with HIP events. Required: FC1's f32 / split ratio >= 2 for both (the ratio the forward kernel had to meet).
  2. The batch-16 Openset training step (forward + backward + update, bench.py's train_step_leg loop) in both modes, each in a child
     process of its own (a trainer's streams and allocator state disturb the next one's timing): the median of 10 timings of 3 steps.
     --parent-tree DIR: the same loop from the package under DIR (a built checkout of the parent commit), default mode.
Prints one JSON line and writes it to profiles/box_head_split_train_line.json.

    python scripts/bench_box_head_split_train.py [--launches 20] [--warmup 5] [--batch 16] [--parent-tree DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROIS_PER_IMAGE = 512


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


def step_child(tree: str, mode: str, batch: int) -> None:
    """Child process: the training step of the package under `tree` in `mode`; prints one JSON line."""
    sys.path.insert(0, tree)
    import __graft_entry__ as ge
    ge.load_package()
    import bench
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import random_params
    dev = "cuda:0"
    n = batch
    images = torch.randint(0, 256, (n, 3, 800, 1333), generator=torch.Generator().manual_seed(99), dtype=torch.uint8).to(dev)
    hw = torch.tensor([(800, 1333)] * n, dtype=torch.int32, device=dev)
    kw = dict(box_head=mode) if mode != "storage" else {}
    tr = OpensetRCNNTrainer(random_params(0), dtype=torch.float16, device=dev, lr=1e-4, loss_scale=1024.0, **kw)
    gt, gcls, gcnt = bench.synthetic_gt(n, 800, 1333)
    shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    r = sum(a * b for a, b in shapes)
    cap = sum(min(2000, a * b) for a, b in shapes)
    g = torch.Generator().manual_seed(0)
    keys = {k: torch.rand(s, generator=g).to(dev) for k, s in (("rpn_reg", (n, r)), ("rpn_obj", (n, r)), ("roi", (n, cap + gt.shape[1])))}
    args = (images, hw, 800, 1344, gt.to(dev), gcls.to(dev), gcnt.to(dev), keys)
    for _ in range(5):
        losses = tr.step(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(10):
        t0 = time.perf_counter()
        for _ in range(3):
            losses = tr.step(*args)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / 3 * 1e3)
    times.sort()
    print(json.dumps(dict(mode=mode, median_ms=round(times[5], 3), min_ms=round(times[0], 3), max_ms=round(times[-1], 3),
                          loss=round(float(sum(float(v) for v in losses.values())), 5), overflow_steps=tr.overflow_steps,
                          peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20))))


def _run_step_child(tree: str, mode: str, batch: int) -> dict:
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-step", tree, mode, "--batch", str(batch)], capture_output=True, text=True,
                         timeout=300)
    if out.returncode != 0:
        raise RuntimeError(f"step child ({tree}, {mode}) failed with status {out.returncode}:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-step", nargs=2, default=None, metavar=("TREE", "MODE"))
    args = ap.parse_args()
    if args.child_step:
        step_child(args.child_step[0], args.child_step[1], args.batch)
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.load_package()
    from openset_rcnn_amd.host import ops
    dev = "cuda:0"
    m = args.batch * ROIS_PER_IMAGE
    g = torch.Generator().manual_seed(3)

    # ---- 1. the backward kernels alone ----
    layers = {}
    for name, k, n in (("fc1", 12544, 1024), ("fc2", 1024, 1024)):
        x = (torch.randn(m, k, generator=g) * torch.exp(torch.randn(m, 1, generator=g) * 1.2)).to(dev)
        dy = (torch.randn(m, n, generator=g) * (torch.rand(m, n, generator=g) < 0.5)).to(dev)
        w = (torch.randn(n, k, generator=g) * (2.0 / k) ** 0.5).to(dev)
        wt32 = w.t().contiguous()                      # (k, n): the exact-f32 data gradient is a linear layer with this weight
        wt_split = ops.split_rows_bf16_t(w)
        zero_b = torch.zeros(k, device=dev)
        x16, dy16 = x.half(), dy.half()
        wd16 = ops.pack_dgrad_weight(w.half()).view(k, 1, 1, n)
        dw = torch.empty(n, k, device=dev)
        fl = 2.0 * m * k * n
        ops.LINEAR_SPLIT_WGRAD_COUNT = {"launches": 0, "flops": 0.0}
        ops.LINEAR_SPLIT_DGRAD_COUNT = {"launches": 0, "flops": 0.0}
        r = dict(rows=m, k=k, n=n)
        r["wgrad"] = dict(split=_timed(lambda: ops.linear_split_wgrad(x, dy, dw=dw), args.warmup, args.launches),
                          f32=_timed(lambda: ops.gemm_f32_tn(dy, x, out=dw), args.warmup, args.launches),
                          f16=_timed(lambda: ops.conv2d_wgrad(x16.view(1, m, 1, k), dy16.view(1, m, 1, n), 1, 1, dw=dw.view(n, 1, 1, k)), args.warmup, args.launches))
        r["dgrad"] = dict(split=_timed(lambda: ops.linear_split_dgrad(dy, wt_split), args.warmup, args.launches),
                          f32=_timed(lambda: ops.linear(dy, wt32, zero_b, out_dtype=torch.float32), args.warmup, args.launches),
                          f16=_timed(lambda: ops.conv2d_dgrad(dy16.view(1, m, 1, n), wd16, (m, 1)), args.warmup, args.launches))
        assert ops.LINEAR_SPLIT_WGRAD_COUNT["launches"] == ops.LINEAR_SPLIT_DGRAD_COUNT["launches"] == args.warmup + args.launches
        ops.LINEAR_SPLIT_WGRAD_COUNT = ops.LINEAR_SPLIT_DGRAD_COUNT = None
        for kind in ("wgrad", "dgrad"):
            t = r[kind]
            t["f32_over_split"] = round(t["f32"]["median_ms"] / t["split"]["median_ms"], 2)
            t["split_over_f16"] = round(t["split"]["median_ms"] / t["f16"]["median_ms"], 2)
            t["split_layer_tflops"] = round(fl / t["split"]["median_ms"] / 1e9, 1)  # the contraction's FLOPs; the kernel spends three bf16 products on each
        r["transposed_split"] = _timed(lambda: ops.split_rows_bf16_t(w, out=wt_split), args.warmup, args.launches)
        layers[name] = r
        del x, dy, w, wt32, wt_split, x16, dy16, wd16, dw
        torch.cuda.empty_cache()
    required = dict(fc1_wgrad_f32_over_split=layers["fc1"]["wgrad"]["f32_over_split"], fc1_dgrad_f32_over_split=layers["fc1"]["dgrad"]["f32_over_split"],
                    bar=2.0)
    required["met"] = required["fc1_wgrad_f32_over_split"] >= 2.0 and required["fc1_dgrad_f32_over_split"] >= 2.0

    # ---- 2. the training step, one child process per configuration ----
    steps = dict(default=_run_step_child(ROOT, "storage", args.batch), split=_run_step_child(ROOT, "split", args.batch))
    if args.parent_tree:
        steps["parent_commit_default"] = _run_step_child(os.path.abspath(args.parent_tree), "storage", args.batch)
    steps["split_minus_default_ms"] = round(steps["split"]["median_ms"] - steps["default"]["median_ms"], 3)
    line = json.dumps(dict(batch=args.batch, image="3x800x1333", rows=m, launches=args.launches, layers=layers, required_ratio=required, train_step=steps))
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "box_head_split_train_line.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
