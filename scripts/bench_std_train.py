"""The stock-heads train step (configs/base_rcnn_fpn.yaml: RPN + StandardROIHeads) at batch 16, 800 x 1333, fp16, on one GPU:
synthetic uint8 images with 7 GT boxes each, random-init weights (weights.random_standard_params), a learning rate small enough that
every update is applied; 5 warm-up steps, then STEPS timed steps (HIP events around each step, one step at a time). Prints one JSON
line: median / min / max ms per step, skipped updates, the last losses.

    python scripts/bench_std_train.py [STEPS]"""
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
from openset_rcnn_amd.host.structures import Boxes, Instances  # noqa: E402
from openset_rcnn_amd.host.weights import random_standard_params  # noqa: E402

cfg = get_cfg()
add_openset_rcnn_config(cfg)
cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
cfg.merge_from_list(["MODEL.DEVICE", "cuda:0"])
model = M.build_model(cfg)
sd = model.state_dict()
for k, v in random_standard_params(0).items():
    if k in sd:
        sd[k] = v
    elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
        sd[k[:-5] + ".norm.bias"] = v
model.load_state_dict(sd)
model.train()
tr = model.trainer()
tr.lr = 1e-5  # every timed update is applied (random weights diverge at the default rate)
g = torch.Generator().manual_seed(0)
batch = []
for i in range(16):
    k = 7
    xy = torch.rand(k, 2, generator=g) * torch.tensor([1000.0, 600.0])
    wh = 30 + torch.rand(k, 2, generator=g) * 300
    b = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([1333.0, 800.0]))], 1)
    batch.append({"image": torch.randint(0, 256, (3, 800, 1333), generator=g, dtype=torch.uint8),
                  "instances": Instances((800, 1333), gt_boxes=Boxes(b), gt_classes=torch.randint(0, 80, (k,), generator=g))})
tensors = [model._train_tensors(batch, torch.Generator().manual_seed(s)) for s in range(2)]
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
for i in range(5):
    tr.step(*tensors[i % 2])
torch.cuda.synchronize()
times = []
for i in range(steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = tr.step(*tensors[i % 2])
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
tr.poll_overflow(wait=True)
times.sort()
res = dict(median_ms=times[len(times) // 2], min_ms=times[0], max_ms=times[-1], steps=steps, overflow_steps=tr.overflow_steps,
           losses={k: float(v) for k, v in out.items()})
print(json.dumps(res))
