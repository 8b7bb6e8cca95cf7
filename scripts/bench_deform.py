"""Deformable conv2 in res3..res5 (MODEL.RESNETS.DEFORM_ON_PER_STAGE [False, True, True, True], configs/mask_rcnn_dconv_c3_c5.yaml with the
mask head off) against the plain trunk (configs/base_rcnn_fpn.yaml) at the benchmark's shape, in one run: batch 16 at 800 x 1333, fp16,
seeded synthetic weights and images, conv2_offset drawn for offsets of about one pixel (zero offsets would read like a plain im2col).

* the inference pass (engine.forward_device, eager, one stream): device-event times of the two engines, interleaved, medians;
* per stage, the three launches of every deformable block -- conv2_offset, the gather (osr_deform_cols) and the 1x1 contraction -- summed
  over the stage's blocks, from profiled passes (engine.profile: one event pair per launch), medians over the passes;
* beside them the same layers' plain 3x3 conv2 of the plain engine, measured in the same run with res3's chained conv2 -> conv3 launch
  switched off (so that conv2 is a launch of its own), and the chained launches' own time.

Writes profiles/deform_conv_line.json (or --out)."""
import argparse
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from scripts.bench_cascade import build, interleaved  # noqa: E402

N, H, W, HP, WP = 16, 800, 1333, 800, 1344
C3_C5 = (False, True, True, True)
KINDS = {"conv2_offset": r"\.conv2_offset$", "gather": r"\.conv2 \(deform gather\)$", "contraction": r"\.conv2 \(deform contraction\)$",
         "plain_conv2": r"\.conv2$", "chained_conv2_conv3": r"\.conv2\+conv3 \(chained\)$"}


def profiled(eng, images, hw, passes):
    """{stage: {kind: median over the passes of the summed device time, ms}} of the conv2-side launches of res3..res5."""
    runs = []
    for _ in range(passes + 1):  # (the first pass is a warm-up)
        eng.profile = []
        eng.forward_device(images, hw, HP, WP)
        torch.cuda.synchronize()
        prof, _ = eng.resolve_profile()
        eng.profile = None
        sums = {}
        for name, _, e0, e1, nbytes, _ in prof:
            m = re.search(r"\.res([2-5])\.\d+(\..*)$", name)
            if not m:
                continue
            for kind, pat in KINDS.items():
                if re.search(pat, m.group(2)):
                    s = sums.setdefault(f"res{m.group(1)}", {}).setdefault(kind, [0.0, 0.0])
                    s[0] += e0.elapsed_time(e1)
                    s[1] += nbytes
        runs.append(sums)
    out = {}
    for stage in sorted(runs[-1]):
        out[stage] = {kind: dict(median_ms=round(statistics.median(r[stage][kind][0] for r in runs[1:]), 4),
                                 algorithmic_mb=round(runs[-1][stage][kind][1] / 1e6, 1)) for kind in runs[-1][stage]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_conv_line.json"))
    ap.add_argument("--passes", type=int, default=8)
    args = ap.parse_args()
    ge.load_package()._lib.load()
    from openset_rcnn_amd.host.weights import deform_offset_params, random_standard_params
    params = random_standard_params(0)
    plain = build("base_rcnn_fpn.yaml", params)
    deform = build("mask_rcnn_dconv_c3_c5.yaml", dict(params, **deform_offset_params(C3_C5, std=1.0)), "MODEL.MASK_ON", "False")
    g = torch.Generator().manual_seed(1234)
    images = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8).cuda()
    hw = torch.tensor([(H, W)] * N, dtype=torch.int32, device="cuda")
    e_plain, e_deform = plain.eval().engine(), deform.eval().engine()
    assert e_deform.deform == C3_C5 and not any(e_plain.deform)
    result = dict(batch=N, image=f"3x{H}x{W}", dtype="float16", deform_on_per_stage=list(C3_C5), modulated=False, groups=1,
                  device=torch.cuda.get_device_name(0))
    result["inference_ms"] = interleaved({"plain_trunk": lambda: e_plain.forward_device(images, hw, HP, WP),
                                          "deformable_c3_c5": lambda: e_deform.forward_device(images, hw, HP, WP)}, args.passes)
    print(json.dumps(result["inference_ms"]), flush=True)
    result["deformable_conv2_launches"] = profiled(e_deform, images, hw, args.passes)
    print(json.dumps(result["deformable_conv2_launches"]), flush=True)
    result["plain_chained_res3"] = profiled(e_plain, images, hw, args.passes).get("res3", {})
    e_plain.chain_res3 = False
    result["plain_conv2_launches"] = profiled(e_plain, images, hw, args.passes)
    e_plain.chain_res3 = True
    print(json.dumps(result["plain_conv2_launches"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
