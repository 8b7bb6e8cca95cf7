"""RoIAlign under the four pooler option pairs (ROIAlignV2 | ROIAlign) x (sampling ratio 0 | 2) on the benchmark's own proposals:
batch 16 at 800 x 1333, the proposal lists of a default fp16 pass, fp16 and fp32 features.

Forward (roi_align_kernel, precomputed locality order) and the pixel-centric backward (roi_align_bwd_dense_kernel) are timed per
launch with device events; the four pairs are interleaved launch by launch, the median of 20 launches per pair is taken, and the
whole set runs twice: `median_ms` is the mean of a pair's two medians, and the difference of the default pair's two medians is the
spread every comparison below is read against.

  --parent-lib PATH   a libosr_hip.so built from the parent commit: its osr_roi_align_fwd_ordered_ex joins the interleave
                      (condition 1: the default pair must not have become slower than the parent's kernel)
  --per-level         the forward at (V2, 0) and (V2, 2) on the RoIs of one level at a time
  --stream-lib PATH   a libosr_hip.so of this commit built with -DRA_GATHER_BIN=1e9f (the gather never taken): the (V2, 2) forward
                      on 4096 square RoIs per bin width of 2 .. 10 level pixels, streamed against the shipped switch-over
                      (the measurement RA_GATHER_BIN in csrc/osr_roi_align.hip is chosen from)

Writes profiles/roi_pooler_line.json (or --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

PAIRS = [("V2,0", True, 0), ("V2,2", True, 2), ("ROIAlign,0", False, 0), ("ROIAlign,2", False, 2)]
SC = (0.25, 0.125, 0.0625, 0.03125)
LAUNCHES, WARMUP = 20, 3


def interleaved(fns):
    """{name: launch} -> {name: median ms of LAUNCHES launches}, the launches of the different names taking turns."""
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)] for k in fns}
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for i in range(LAUNCHES):
        for k, fn in fns.items():
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in ev[k]) for k in fns}


def two_sets(fns, default="V2,0"):
    a, b = interleaved(fns), interleaved(fns)
    return dict(set1_ms=a, set2_ms=b, median_ms={k: 0.5 * (a[k] + b[k]) for k in fns}, default_spread_ms=abs(a[default] - b[default]))


def switch_over(stream_lib_path, lib, _lib, ops):
    """ms of the (V2, 2) forward on 4096 square RoIs of one bin width on a 2 x 64 x 96 x 256 fp16 level: 'stream' (gather disabled)
    against 'shipped' (gather from RA_GATHER_BIN * S pixels on), and 'adaptive' = (V2, 0) on the same RoIs."""
    stream = C.CDLL(os.path.abspath(stream_lib_path))
    res, argt = _lib.PROTOTYPES["osr_roi_align_fwd_ordered_opt"]
    stream.osr_roi_align_fwd_ordered_opt.restype, stream.osr_roi_align_fwd_ordered_opt.argtypes = res, argt
    g = torch.Generator().manual_seed(77)
    h, w, m = 64, 96, 4096
    feat = [torch.randn(2, h, w, 256, generator=g).half().cuda()]
    py = ops._pyramid(feat, (1.0,))
    bidx = torch.randint(0, 2, (m,), generator=g, dtype=torch.int32).cuda()
    ident = torch.arange(m, dtype=torch.int32, device="cuda")
    out = torch.empty((m, 7, 7, 256), dtype=torch.float16, device="cuda")
    table = {}
    for b in (2.0, 3.0, 3.5, 4.0, 4.5, 5.0, 6.0, 8.0, 10.0):
        side = 7.0 * b
        xy = torch.rand(m, 2, generator=g) * torch.tensor([w - side, h - side]).clamp(min=0.0)
        boxes = torch.cat((xy, xy + side), dim=1).cuda().contiguous()

        def launch(which, s):
            opt = _lib.RoiOptions(1, s)
            st = which.osr_roi_align_fwd_ordered_opt(C.byref(py), ops._DT[torch.float16], 2, C.c_void_p(boxes.data_ptr()), C.c_void_p(bidx.data_ptr()),
                                                     m, 7, 2, 224, 2, C.c_void_p(ident.data_ptr()), None, 0, C.byref(opt), C.c_void_p(out.data_ptr()),
                                                     ops._DT[torch.float16], ops._stream())
            assert st == 0, st
        # (one level, min_level 2 with canonical level 2: every box lands on it)
        r = interleaved({"stream": lambda: launch(stream, 2), "shipped": lambda: launch(lib, 2), "adaptive": lambda: launch(lib, 0)})
        table[f"bin_{b}px"] = {k: round(v, 4) for k, v in r.items()}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--per-level", action="store_true")
    ap.add_argument("--stream-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_pooler_line.json"))
    args = ap.parse_args()
    pkg = ge.load_package()
    lib = pkg._lib.load()
    from openset_rcnn_amd.host import _lib, ops
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import random_params
    eng = OpensetRCNNEngine(random_params(0), device="cuda:0")
    g = torch.Generator().manual_seed(1234)
    images = torch.randint(0, 256, (16, 3, 800, 1333), generator=g, dtype=torch.uint8).cuda()
    hw = torch.tensor([(800, 1333)] * 16, dtype=torch.int32, device="cuda")
    keep = {}
    eng.forward_device(images, hw, 800, 1344, keep)
    torch.cuda.synchronize()
    feats, sel = keep["feats"], keep["sel"]
    n, cap = 16, sel["cap"]
    bb, ii = sel["boxes"].view(-1, 4).contiguous(), sel["batch_idx"].view(-1).contiguous()
    m = bb.shape[0]
    area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    lvl = torch.floor(4 + torch.log2(torch.sqrt(area.clamp(min=1e-6)) / 224 + 1e-8)).clamp(2, 5)
    per_level = [int(((lvl == l) & (ii >= 0)).sum()) for l in (2, 3, 4, 5)]
    result = dict(rois=m, valid=int((ii >= 0).sum()), per_level=per_level, launches=LAUNCHES, sets=2, device=torch.cuda.get_device_name(0))
    print(json.dumps({k: result[k] for k in ("rois", "valid", "per_level")}), flush=True)

    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        res, argt = _lib.PROTOTYPES["osr_roi_align_fwd_ordered_ex"]
        parent.osr_roi_align_fwd_ordered_ex.restype, parent.osr_roi_align_fwd_ordered_ex.argtypes = res, argt

    for name, dt in (("fp16", torch.float16), ("fp32", torch.float32)):
        fl = [feats[k].to(dt) for k in ("p2", "p3", "p4", "p5")]
        order = ops.roi_locality_order(fl, SC, bb, ii)
        fwd = {tag: (lambda al=al, s=s: ops.roi_align(fl, SC, bb, ii, 7, dt, order=order, fill_padding=False, aligned=al, sampling_ratio=s))
               for tag, al, s in PAIRS}
        if parent is not None:
            py = ops._pyramid(fl, SC)
            out = torch.empty((m, 7, 7, 256), dtype=dt, device="cuda")
            code = ops._DT[dt]
            nvalid = C.c_void_p(order.data_ptr() + 4 * m)

            def parent_launch():
                st = parent.osr_roi_align_fwd_ordered_ex(C.byref(py), code, n, C.c_void_p(bb.data_ptr()), C.c_void_p(ii.data_ptr()), m, 7, 4, 224, 2,
                                                         C.c_void_p(order.data_ptr()), nvalid, 1, C.c_void_p(out.data_ptr()), code, ops._stream())
                assert st == 0, st
            parent_launch()
            torch.cuda.synchronize()
            mine = ops.roi_align(fl, SC, bb, ii, 7, dt, order=order, fill_padding=False)
            real = ii >= 0
            assert torch.equal(out[real], mine[real]), "the default pair no longer computes the parent's bits"
            fwd["parent V2,0"] = parent_launch
        r = two_sets(fwd)
        med = r["median_ms"]
        r["ratio_V2,2_over_V2,0"] = med["V2,2"] / med["V2,0"]
        r["condition2_fixed_grid_not_slower"] = med["V2,2"] <= med["V2,0"] + r["default_spread_ms"]
        if parent is not None:
            r["condition1_default_within_spread_of_parent"] = med["V2,0"] <= med["parent V2,0"] + r["default_spread_ms"]
        result[f"forward_{name}"] = r
        print(f"forward {name}: " + json.dumps(r), flush=True)

        if args.per_level:
            lv_res = {}
            for l in (2, 3, 4, 5):
                il = torch.where((lvl == l) & (ii >= 0), ii, torch.full_like(ii, -1))
                ol = ops.roi_locality_order(fl, SC, bb, il)
                f2 = {tag: (lambda al=al, s=s: ops.roi_align(fl, SC, bb, il, 7, dt, order=ol, fill_padding=False, aligned=al, sampling_ratio=s))
                      for tag, al, s in PAIRS[:2]}
                lv_res[f"p{l}"] = two_sets(f2)["median_ms"]
            result[f"forward_{name}_per_level"] = lv_res
            print(f"forward {name} per level: " + json.dumps(lv_res), flush=True)

        if dt == torch.float16:  # the training step's form: fp16 d_pooled, the storage dtype straight out of the kernel
            dout = torch.randn((m, 7, 7, 256), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=torch.float16)
            shapes = [(f.shape[1], f.shape[2]) for f in fl]
            bwd = {tag: (lambda al=al, s=s: ops.roi_align_bwd(dout, shapes, n, SC, bb, ii, rois_per_image=cap, out_dtype=dt, aligned=al,
                                                            sampling_ratio=s)) for tag, al, s in PAIRS}
            r = two_sets(bwd)
            r["ratio_V2,2_over_V2,0"] = r["median_ms"]["V2,2"] / r["median_ms"]["V2,0"]
            result["backward_dense_fp16"] = r
            print("backward dense fp16: " + json.dumps(r), flush=True)

    if args.stream_lib:
        result["switch_over_fp16_V2,2"] = switch_over(args.stream_lib, lib, _lib, ops)
        print("switch-over: " + json.dumps(result["switch_over_fp16_V2,2"]), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
