"""CascadeROIHeads (three stages, configs/cascade_rcnn_fpn.yaml) against StandardROIHeads (configs/base_rcnn_fpn.yaml) at the
benchmark's shape, in one run: batch 16 at 800 x 1333, fp16, seeded synthetic weights and images.

* the inference pass (engine.forward_device, eager, one stream): device-event times of the two engines, interleaved;
* the train step (trainer.step: forward, backward, update; 7 ground-truth boxes per image): device-event times of the two trainers,
  interleaved, a learning rate small enough that every update is applied. Both trainers sample from POST_NMS_TOPK_TRAIN 2000
  proposals (the cascade file's value) so that the difference is the heads';
* the glue launches on the pass's own tensors: osr_cascade_refine (inference form on 1000 rows per image, training form with ground
  truth on the 512 sampled rows) and osr_cascade_candidates (three stages) beside osr_fastrcnn_candidates.

Writes profiles/cascade_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N, H, W, HP, WP = 16, 800, 1333, 800, 1344
WARMUP = 2


def interleaved(fns, launches):
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


def build(yaml, params, *opts):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda:0"] + list(opts))
    model = M.build_model(cfg)
    sd = model.state_dict()
    for k, v in params.items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_line.json"))
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.structures import Boxes, Instances
    from openset_rcnn_amd.host.weights import random_cascade_params, random_standard_params
    std = build("base_rcnn_fpn.yaml", random_standard_params(0), "MODEL.RPN.POST_NMS_TOPK_TRAIN", "2000")
    cas = build("cascade_rcnn_fpn.yaml", random_cascade_params(0, stages=3))
    g = torch.Generator().manual_seed(1234)
    images = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8).cuda()
    hw = torch.tensor([(H, W)] * N, dtype=torch.int32, device="cuda")
    result = dict(batch=N, image=f"3x{H}x{W}", dtype="float16", stages=3, device=torch.cuda.get_device_name(0))

    # ---- inference ----
    e_std, e_cas = std.eval().engine(), cas.eval().engine()
    keep = {}
    res = e_cas.forward_device(images, hw, HP, WP, keep)
    torch.cuda.synchronize()
    result["detections_of_the_cascade_pass"] = [int(c) for c in res[3].cpu()]
    result["inference_ms"] = interleaved({"standard_roi_heads": lambda: e_std.forward_device(images, hw, HP, WP),
                                          "cascade_roi_heads": lambda: e_cas.forward_device(images, hw, HP, WP)}, args.passes)
    print(json.dumps(result["inference_ms"]), flush=True)

    # ---- the glue launches, on the pass's own tensors ----
    sel, k = keep["sel"], e_cas.cfg["std_num_classes"]
    b0, d0, bidx = keep["boxes_s0"], keep["deltas_s0"], sel["batch_idx"]
    logits = [keep[f"logits_s{s}"] for s in range(3)]
    b2 = keep["boxes_s2"].view(N, -1, 4)
    xy = torch.rand(N, 7, 2, generator=g) * torch.tensor([1000.0, 600.0])
    gt = torch.cat([xy, torch.minimum(xy + 30 + torch.rand(N, 7, 2, generator=g) * 300, torch.tensor([1333.0, 800.0]))], 2).cuda().contiguous()
    gcls = torch.randint(0, 80, (N, 7), generator=g).cuda()
    gcnt = torch.full((N,), 7, dtype=torch.int32, device="cuda")
    tb, td, tbi = b0.view(N, -1, 4)[:, :512].reshape(-1, 4).contiguous(), d0.view(N, -1, 4)[:, :512].reshape(-1, 4).contiguous(), \
        bidx.view(N, -1)[:, :512].reshape(-1).contiguous()
    w = e_cas.stage_weights
    result["glue_launches_ms"] = interleaved({
        "cascade_refine_inference_1000_rows": lambda: ops.cascade_refine(b0, bidx, d0, N, hw, w[0]),
        "cascade_refine_training_512_rows": lambda: ops.cascade_refine(tb, tbi, td, N, hw, w[0], True, gt, gcls, gcnt, k, 0.6),
        "cascade_candidates_3_stages": lambda: ops.cascade_candidates(logits, keep["deltas_s2"], b2, bidx, hw, k, w[2], 0.05),
        "fastrcnn_candidates": lambda: ops.fastrcnn_candidates(logits[0], d0, sel["boxes"], sel["counts"], hw, k, w[0], 0.05)}, 20)
    print(json.dumps(result["glue_launches_ms"]), flush=True)
    del keep

    # ---- the train step ----
    batch = []
    for i in range(N):
        xy = torch.rand(7, 2, generator=g) * torch.tensor([1000.0, 600.0])
        b = torch.cat([xy, torch.minimum(xy + 30 + torch.rand(7, 2, generator=g) * 300, torch.tensor([1333.0, 800.0]))], 1)
        batch.append({"image": images[i].cpu(), "instances": Instances((H, W), gt_boxes=Boxes(b), gt_classes=torch.randint(0, 80, (7,), generator=g))})
    trainers, tensors = {}, {}
    for name, model in (("standard_roi_heads", std), ("cascade_roi_heads", cas)):
        model.train()
        trainers[name] = model.trainer()
        trainers[name].lr = 1e-5  # every timed update is applied (random weights diverge at the default rate)
        tensors[name] = [model._train_tensors(batch, torch.Generator().manual_seed(s)) for s in range(2)]
    it = {name: 0 for name in trainers}

    def step(name):
        trainers[name].step(*tensors[name][it[name] % 2])
        it[name] += 1
    result["train_step_ms"] = interleaved({name: (lambda name=name: step(name)) for name in trainers}, args.steps)
    for name, tr in trainers.items():
        tr.poll_overflow(wait=True)
        result["train_step_ms"][name]["overflow_steps"] = tr.overflow_steps
    print(json.dumps(result["train_step_ms"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
