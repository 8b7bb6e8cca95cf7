"""What the mask branch costs a training step: the stock-heads step of scripts/bench_std_train.py (configs/base_rcnn_fpn.yaml, batch 16,
800 x 1333, fp16, one GPU, random-init weights, 7 ground-truth boxes per image with their boxes as bitmasks) with MODEL.MASK_ON False and
True in the same run -- 5 warm-up steps, then STEPS timed steps each (HIP events around each step). The mask branch runs on the padded
capacity of int(BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION) rows per image; the measured foreground fill of those rows (what a later
compaction would save) is recorded beside the times. Writes profiles/mask_train_line.json and prints it.

    python scripts/bench_mask_train.py [STEPS] [--out PATH]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.load_package()
from openset_rcnn_amd.host import modeling as M  # noqa: E402
from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg  # noqa: E402
from openset_rcnn_amd.host.structures import BitMasks, Boxes, Instances  # noqa: E402
from openset_rcnn_amd.host.weights import random_standard_params  # noqa: E402

H, W, N, GT = 800, 1333, 16, 7
PRE = "roi_heads.mask_head."


def build(mask_on: bool):
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda:0", "MODEL.MASK_ON", str(mask_on), "INPUT.MASK_FORMAT", "bitmask"])
    model = M.build_model(cfg)
    sd = model.state_dict()
    for k, v in random_standard_params(0).items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)  # (the mask head keeps the module's own [d2] initialisers)
    model.train()
    tr = model.trainer()
    tr.lr = 1e-5  # every timed update is applied (random weights diverge at the default rate)
    return model, tr


def make_batch():
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    batch = []
    for _ in range(N):
        xy = torch.rand(GT, 2, generator=g) * torch.tensor([1000.0, 600.0])
        wh = 30 + torch.rand(GT, 2, generator=g) * 300
        b = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([float(W), float(H)]))], 1)
        masks = torch.stack([(xx >= r[0]) & (xx < r[2]) & (yy >= r[1]) & (yy < r[3]) for r in b])
        batch.append({"image": torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8),
                      "instances": Instances((H, W), gt_boxes=Boxes(b), gt_classes=torch.randint(0, 80, (GT,), generator=g), gt_masks=BitMasks(masks))})
    return batch


def measure(mask_on: bool, batch, steps: int) -> dict:
    model, tr = build(mask_on)
    tensors = [model._train_tensors(batch, torch.Generator().manual_seed(s)) for s in range(2)]
    run = lambda t: tr.step(*t[:8], **model._mask_kwargs(t))  # noqa: E731
    for i in range(5):
        run(tensors[i % 2])
    torch.cuda.synchronize()
    times, fills = [], []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = run(tensors[i % 2])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
        if mask_on:  # (read after the timed region) foreground rows of this step / the rows the branch ran on
            cap = N * max(int(tr.eng.cfg["roi_batch_size"] * tr.eng.cfg["roi_positive_fraction"]), 1)
            fills.append(float(tr._last_forward["mask_stats"][1]) / cap)
    tr.poll_overflow(wait=True)
    times.sort()
    line = dict(median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], steps=steps, overflow_steps=tr.overflow_steps,
                losses={k: float(v) for k, v in out.items()})
    if mask_on:
        line.update(mask_rows_capacity=cap, foreground_fill_mean=sum(fills) / len(fills), foreground_fill_min=min(fills), foreground_fill_max=max(fills))
    del model, tr
    torch.cuda.empty_cache()
    return line


def main():
    args = [a for a in sys.argv[1:]]
    out_path = os.path.join(ROOT, "profiles", "mask_train_line.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    steps = int(args[0]) if args else 20
    batch = make_batch()
    res = dict(workload="stock heads train step, batch 16, 800 x 1333, fp16, 7 GT per image (boxes as bitmasks), random-init weights",
               device=torch.cuda.get_device_name(0), mask_off=measure(False, batch, steps), mask_on=measure(True, batch, steps))
    res["mask_branch_ms"] = res["mask_on"]["median_ms"] - res["mask_off"]["median_ms"]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
