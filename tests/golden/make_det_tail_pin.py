"""Generator of tests/golden/det_tail_pin_v1.npz: fixed inputs of the stock detection tails in front of the NMS and what the HIP
library answered for them on an MI355X at one commit (the fixture's `parent_commit`). tests/test_det_tail_pin.py replays the inputs
through the same replay() and compares bit patterns, so that a rewrite of these kernels is held to what they computed before it.

Provenance: DEVICE-generated, not oracle-generated: the record is the library's own earlier answer (the oracle tests hold the same
kernels to the reference arithmetic elsewhere). Regenerate only when a kernel's result is meant to change:
    python tests/golden/make_det_tail_pin.py --parent <commit> [--out <file>]

The cases (arrays `in_<case>_*` are inputs, `out_<case>_*` the record; padded candidate lists are stored as each image's valid prefix):
  cand     osr_fastrcnn_candidates (class-agnostic and per-class deltas) and osr_cascade_candidates with 1..4 stages: 3 images of
           1025 rows (two passes of the 1024-thread loop, the second of one row), 3 classes, counts {1018, 0, 1025}; the cascade
           calls take the same lists through batch_idx with holes, one in the middle of a row list
  rpn      osr_rpn_select_ex, decode mode 1: two levels, the second shorter than its top-k
  retina   osr_retinanet_select: the same pyramid, fp32 logits
  tail     osr_box_predictor_tail at k = 4
  refine   osr_cascade_refine with and without ground truth and drop_empty
Every case carries the edge rows: a NaN in dx and in dw, +Inf / -Inf in dw, dw above the log(1000/16) clamp, dx = 3e38, a source
box of zero width, boxes beyond each image corner, an Inf and a NaN logit, a row whose only hot class sits beside another class's
NaN delta. Every probability (logit, for RetinaNet) stays at least 1e-3 relative away from its threshold."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "det_tail_pin_v1.npz")
NAN, INF = float("nan"), float("inf")
WEIGHTS = (10.0, 10.0, 5.0, 5.0)

# candidates
C_N, C_ROWS, C_K, C_COUNTS, C_THRESH = 3, 1025, 3, (1018, 0, 1025), 0.2
C_HW = ((120, 160), (100, 100), (90, 140))
C_HOLES = ((0, 0), (0, 500), (2, 600), (2, 601), (2, 1023))  # (image, row) of the cascade's extra batch_idx holes
# selects
S_SHAPES, S_STRIDES, S_A, S_N, S_TOPK = ((3, 4), (1, 2)), (8, 16), 3, 2, 16
S_HW = ((20, 30), (24, 28))
S_CELLS = (((-8.0, -4.0, 8.0, 4.0), (-6.0, -6.0, 6.0, 6.0), (-4.0, -8.0, 4.0, 8.0)),
           ((-16.0, -8.0, 16.0, 8.0), (0.0, -12.0, 0.0, 12.0), (-8.0, -16.0, 8.0, 16.0)))  # (level 1's second anchor has zero width)
R_K, R_THRESH = 2, 0.05
# refine
F_N, F_ROWS, F_GMAX, F_K, F_IOU = 3, 260, 3, 5, 0.5
F_HW = ((120, 160), (100, 100), (90, 140))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _edge_rows(deltas, boxes, hw, r0):
    """Writes the delta / box edge rows at r0 .. r0 + 9 (deltas (m, >= 4): the first class's four; boxes (m, 4)); returns the count."""
    ih, iw = hw
    deltas[r0:r0 + 10] = 0.0
    deltas[r0 + 0, 0] = NAN
    deltas[r0 + 1, 2] = NAN
    deltas[r0 + 2, 2] = INF
    deltas[r0 + 3, 2] = -INF
    deltas[r0 + 4, 2] = 100.0   # 100 / 5 is above the clamp
    deltas[r0 + 5, 0] = 3e38
    boxes[r0 + 5] = torch.tensor([10.0, 10.0, 10.5, 12.0])  # (3e37 * 0.5 stays finite: clipped, not dropped)
    boxes[r0 + 6, 2] = boxes[r0 + 6, 0]  # zero width
    boxes[r0 + 6, 0:4:2] += 1.0
    boxes[r0 + 7] = torch.tensor([-50.0, -40.0, -10.0, -5.0])
    boxes[r0 + 8] = torch.tensor([iw + 10.0, -30.0, iw + 60.0, -2.0])
    boxes[r0 + 9] = torch.tensor([-40.0, ih + 5.0, -3.0, ih + 50.0])
    boxes[r0 + 10] = torch.tensor([iw + 5.0, ih + 5.0, iw + 70.0, ih + 60.0])
    deltas[r0 + 10] = 0.0
    return 11


def _cand_inputs():
    g = _gen(201)
    m, k = C_N * C_ROWS, C_K
    logits = [torch.randn(m, k + 1, generator=g) * 2.0 for _ in range(4)]
    deltas = torch.randn(m, k * 4, generator=g) * torch.tensor([3.0, 3.0, 1.5, 1.5] * k)
    xy = torch.rand(m, 2, generator=g) * 100
    boxes = torch.cat((xy, xy + torch.rand(m, 2, generator=g) * 50 + 2), dim=1)
    hot0, hot1, hot2 = torch.tensor([5.0, 0.0, 0.0, -1.0]), torch.tensor([0.0, 5.0, 0.0, -1.0]), torch.tensor([0.0, -1.0, 5.0, 0.0])
    edge = []

    def hot(r, pattern):
        for lg in logits:
            lg[r] = pattern
        edge.append(r)
    r0 = 3
    ne = _edge_rows(deltas, boxes, C_HW[0], r0)
    for r in range(r0, r0 + ne):
        hot(r, hot0)
    r = r0 + ne
    hot(r, hot0); logits[0][r, 1] = INF
    hot(r + 1, hot0); logits[0][r + 1, 2] = NAN
    hot(r + 2, hot0); logits[3][r + 2, 0] = NAN          # (only the four-stage average sees it)
    hot(r + 3, hot1); deltas[r + 3, 2] = NAN             # class 1 is hot, class 0's dw is NaN
    hot(r + 4, hot1); deltas[r + 4, 8] = NAN             # class 1 is hot, class 2's dx is NaN: dropped only with per-class deltas
    r2 = 2 * C_ROWS
    hot(r2 + 1020, hot0); deltas[r2 + 1020, 2] = NAN
    hot(r2 + 1022, hot2); deltas[r2 + 1022, 3] = NAN     # class 2 is hot, class 0's dh is NaN
    hot(r2 + 1024, hot2)                                 # the one row of the second pass emits
    # no probability, of one stage or of an average over the first S, within 2e-3 relative of the threshold (fp64 restatement)
    is_edge = torch.zeros(m, dtype=torch.bool)
    is_edge[edge] = True
    for _ in range(64):
        probs = [torch.softmax(lg.double(), dim=-1) for lg in logits]
        near = torch.zeros(m, dtype=torch.bool)
        for s in range(1, 5):
            avg = sum(probs[:s]) / s
            near |= ((avg[:, :k] - C_THRESH).abs() <= 2e-3 * C_THRESH).any(dim=1)
        assert not bool((near & is_edge).any())
        if not bool(near.any()):
            break
        for lg in logits:
            lg[near] = torch.randn(int(near.sum()), k + 1, generator=g) * 2.0
    else:
        raise AssertionError("could not move every probability off the threshold")
    counts = torch.tensor(C_COUNTS, dtype=torch.int32)
    bidx = torch.where(torch.arange(C_ROWS)[None, :] < counts[:, None], torch.arange(C_N, dtype=torch.int32)[:, None],
                       torch.tensor(-1, dtype=torch.int32))
    for i, j in C_HOLES:
        bidx[i, j] = -1
    live = (torch.arange(C_ROWS)[None, :] < counts[:, None]).reshape(-1)  # only each image's valid prefix is stored
    out = {f"in_cand_logits{s}": logits[s][live].numpy() for s in range(4)}
    out.update(in_cand_deltas=deltas[live].numpy(), in_cand_boxes=boxes[live].numpy(), in_cand_counts=counts.numpy(),
               in_cand_bidx=bidx.reshape(-1).numpy(), in_cand_hw=np.array(C_HW, np.int32))
    return out


def _select_edges(deltas0, deltas1, key0, key1):
    """deltas<l> (n, anchors of level l, 4), key<l> (n, anchors of level l) scores whose largest values are selected first."""
    d = deltas1[0]
    d[0, 0] = NAN
    d[2, 2] = NAN
    d[3, 2] = INF
    d[4, 3] = -INF   # (the zero-width anchor)
    d[5, 2] = 100.0
    deltas1[1][0, 2] = -INF
    deltas0[0][0, 0] = 3e38; key0[0][0] = 9.0
    deltas0[0][35, 1] = NAN; key0[0][35] = 8.5
    key0[0][5] = INF
    key0[0][7] = NAN
    key0[1][11] = INF


def _rpn_inputs():
    g = _gen(202)
    cnt = [h * w * S_A for h, w in S_SHAPES]
    scores = [torch.randn(S_N, c, generator=g) * 2.0 for c in cnt]
    deltas = [torch.randn(S_N, c, 4, generator=g) * torch.tensor([3.0, 3.0, 1.5, 1.5]) for c in cnt]
    _select_edges(deltas[0], deltas[1], scores[0], scores[1])
    return dict(in_rpn_scores=torch.cat([s.reshape(-1) for s in scores]).numpy(), in_rpn_deltas=torch.cat([d.reshape(-1, 4) for d in deltas]).numpy(),
                in_rpn_hw=np.array(S_HW, np.int32), in_sel_cells=np.array(S_CELLS, np.float32))


def _retina_inputs():
    g = _gen(203)
    cnt = [h * w * S_A for h, w in S_SHAPES]
    thr = float(np.log(R_THRESH / (1.0 - R_THRESH)))
    logits = [torch.randn(S_N, c, R_K, generator=g) * 2.0 + 1.0 for c in cnt]
    for lg in logits:  # every logit at least 1e-2 away from the threshold logit (-2.94)
        near = (lg - thr).abs() <= 1e-2
        lg[near] += 0.5
    deltas = [torch.randn(S_N, c, 4, generator=g) * torch.tensor([3.0, 3.0, 1.5, 1.5]) for c in cnt]
    _select_edges(deltas[0], deltas[1], logits[0][:, :, 0], logits[1][:, :, 1])  # (views: level 0's class 0, level 1's class 1)
    logits[1][1][3, 0] = -INF
    return dict(in_retina_logits=torch.cat([x.reshape(-1) for x in logits]).numpy(), in_retina_deltas=torch.cat([d.reshape(-1) for d in deltas]).numpy())


def _tail_inputs():
    g = _gen(204)
    m, k = 14, 4
    # d0 = 2 x0 - 2 x1, d1 = x1, d2 = 2 x2 - 2 x3, d3 = x3, iou logit = (x0 + x1) / 2, each plus its bias: a dot product of four terms
    # whose zero weights meet only finite values, so that one delta can be NaN or Inf beside finite ones
    w = torch.tensor([[2.0, -2.0, 0, 0], [0, 1.0, 0, 0], [0, 0, 2.0, -2.0], [0, 0, 0, 1.0], [0.5, 0.5, 0, 0]])
    b = torch.tensor([0.125, -0.25, 0.0625, 0.03125, 0.1])
    x = torch.randn(m, k, generator=g)
    xy = torch.rand(m, 2, generator=g) * 80
    props = torch.cat((xy, xy + torch.rand(m, 2, generator=g) * 40 + 2), dim=1)
    ctr = torch.rand(m, generator=g) * 0.9 + 0.05
    bidx = torch.tensor([0] * 7 + [1] * 7, dtype=torch.int32)
    hw = (60, 90), (70, 50)
    x[0] = torch.tensor([3e38, 3e38, 0.0, 0.0])        # d0 = Inf - Inf = NaN, d1 = 3e38
    x[1] = torch.tensor([0.0, 0.0, 3e38, 3e38])        # d2 = NaN, d3 = 3e38 (above the clamp)
    x[2] = torch.tensor([0.0, 0.0, 3e38, 0.0])         # d2 = +Inf
    x[3] = torch.tensor([0.0, 0.0, -3e38, 0.0])        # d2 = -Inf
    x[4] = torch.tensor([0.0, 0.0, 30.0, 0.0])         # d2 / 5 above the clamp
    x[5] = torch.tensor([1.5e38, 0.0, 0.0, 0.0])       # d0 = 3e38
    props[5] = torch.tensor([10.0, 10.0, 10.5, 12.0])
    props[6, 2] = props[6, 0]                          # zero width
    bidx[7] = -1
    props[8] = torch.tensor([-50.0, -40.0, -10.0, -5.0]); x[8] *= 0.1
    props[9] = torch.tensor([60.0, -30.0, 110.0, -2.0]); x[9] *= 0.1
    props[10] = torch.tensor([-40.0, 75.0, -3.0, 120.0]); x[10] *= 0.1
    props[11] = torch.tensor([55.0, 75.0, 120.0, 130.0]); x[11] *= 0.1
    ctr[12] = NAN
    ctr[13] = INF
    return dict(in_tail_x=x.numpy(), in_tail_w=w.numpy(), in_tail_b=b.numpy(), in_tail_props=props.numpy(), in_tail_ctr=ctr.numpy(),
                in_tail_bidx=bidx.numpy(), in_tail_hw=np.array(hw, np.int32))


def _refine_inputs():
    g = _gen(205)
    m = F_N * F_ROWS
    deltas = torch.randn(m, 4, generator=g) * torch.tensor([3.0, 3.0, 1.5, 1.5])
    xy = torch.rand(m, 2, generator=g) * 100
    boxes = torch.cat((xy, xy + torch.rand(m, 2, generator=g) * 50 + 2), dim=1)
    _edge_rows(deltas, boxes, F_HW[0], 3)
    _edge_rows(deltas, boxes, F_HW[2], 2 * F_ROWS + 240)   # (in the second pass of the 256-thread loop)
    counts = torch.tensor([F_ROWS, 0, F_ROWS - 3], dtype=torch.int32)
    bidx = torch.where(torch.arange(F_ROWS)[None, :] < counts[:, None], torch.arange(F_N, dtype=torch.int32)[:, None], torch.tensor(-1, dtype=torch.int32))
    bidx[0, 0] = -1
    bidx[0, 130] = -1
    bidx[2, 256] = -1
    gxy = torch.rand(F_N, F_GMAX, 2, generator=g) * 80
    gt = torch.cat((gxy, gxy + torch.rand(F_N, F_GMAX, 2, generator=g) * 60 + 10), dim=2)
    return dict(in_refine_boxes=boxes.numpy(), in_refine_deltas=deltas.numpy(), in_refine_bidx=bidx.reshape(-1).numpy(), in_refine_hw=np.array(F_HW, np.int32),
                in_refine_gt=gt.numpy(), in_refine_gt_classes=torch.randint(0, F_K, (F_N, F_GMAX), generator=g).numpy(),
                in_refine_gt_count=np.array([3, 1, 0], np.int32))


def make_inputs():
    out = {}
    for f in (_cand_inputs, _rpn_inputs, _retina_inputs, _tail_inputs, _refine_inputs):
        out.update(f())
    return out


def _padded(rows, counts, width):
    """(sum(counts), ...) stored prefixes -> (n * width, ...) with zero rows behind each image's prefix."""
    out = np.zeros((len(counts) * width,) + rows.shape[1:], rows.dtype)
    o = 0
    for i, c in enumerate(counts):
        out[i * width:i * width + c] = rows[o:o + c]
        o += c
    return out


def replay(ops, inp, dev):
    """Runs every case on `dev`; -> {name: numpy array} under the names of the fixture's `out_` entries (without the prefix)."""
    def t(name, pad=None):
        a = inp["in_" + name]
        return torch.from_numpy(np.ascontiguousarray(a if pad is None else _padded(a, *pad))).to(dev)
    out = {}

    # ---- candidates ----
    counts = [int(c) for c in inp["in_cand_counts"]]
    pad = (counts, C_ROWS)
    logits = [t(f"cand_logits{s}", pad) for s in range(4)]
    deltas3, boxes = t("cand_deltas", pad), t("cand_boxes", pad).view(C_N, C_ROWS, 4)
    deltas1 = deltas3[:, :4].contiguous()
    cnt, bidx, hw = t("cand_counts"), t("cand_bidx"), t("cand_hw")

    def put(tag, o):
        c = o["count"].cpu()
        out[tag + "_count"] = c.numpy()
        for key in ("boxes", "scores", "cls", "row"):
            out[f"{tag}_{key}"] = np.concatenate([o[key][i, :int(c[i])].cpu().numpy() for i in range(C_N)])
    put("cand_fr1", ops.fastrcnn_candidates(logits[0], deltas1, boxes, cnt, hw, C_K, WEIGHTS, C_THRESH))
    put("cand_fr3", ops.fastrcnn_candidates(logits[0], deltas3, boxes, cnt, hw, C_K, WEIGHTS, C_THRESH))
    for s in range(1, 5):
        put(f"cand_cc{s}", ops.cascade_candidates(logits[:s], deltas1, boxes, bidx, hw, C_K, WEIGHTS, C_THRESH))

    # ---- selects ----
    lv = ops.make_rpn_levels(list(S_SHAPES), list(S_STRIDES), S_N, S_A)
    o = ops.rpn_select(lv, t("sel_cells"), t("rpn_scores"), t("rpn_deltas"), S_N, t("rpn_hw"), S_TOPK, 0.0, b2b_weights=WEIGHTS)
    for key in ("boxes", "scores", "src_index", "batch_idx", "level", "counts", "status_flags"):
        out["rpn_" + key] = o[key].cpu().numpy()
    o = ops.retinanet_select(lv, t("sel_cells"), t("retina_logits"), t("retina_deltas"), S_N, R_K, S_TOPK, R_THRESH, WEIGHTS)
    for key in ("c_boxes", "c_scores", "c_cls", "c_cand", "c_src", "counts", "status_flags"):
        out["retina_" + key] = o[key].cpu().numpy()

    # ---- box predictor tail ----
    for mean_type in (0, 1):
        o = ops.box_predictor_tail(t("tail_x"), t("tail_w"), t("tail_b"), t("tail_props"), t("tail_ctr"), t("tail_bidx"), t("tail_hw"), WEIGHTS,
                                   mean_type, 0.3)
        for key in ("pred_deltas", "pred_iou", "boxes", "score", "cand"):
            out[f"tail{mean_type}_{key}"] = o[key].cpu().numpy()

    # ---- cascade refine ----
    for with_gt in (False, True):
        for drop in (False, True):
            gt = (t("refine_gt"), t("refine_gt_classes"), t("refine_gt_count"), F_K, F_IOU) if with_gt else ()
            o = ops.cascade_refine(t("refine_boxes"), t("refine_bidx"), t("refine_deltas"), F_N, t("refine_hw"), WEIGHTS, drop, *gt)
            for key, v in o.items():
                out[f"refine_gt{int(with_gt)}_drop{int(drop)}_{key}"] = v.cpu().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit whose library answers are recorded")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg._lib.load()
    inp = make_inputs()
    rec = replay(pkg.ops, inp, "cuda:0")
    torch.cuda.synchronize()
    again = replay(pkg.ops, inp, "cuda:0")  # the record must be a fixed point of the library it was taken from
    for k, v in rec.items():
        assert v.tobytes() == again[k].tobytes(), k
    for k in sorted(rec):
        if k.endswith("_count") or k.endswith("counts"):
            print(k, rec[k].reshape(-1).tolist())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, parent_commit=np.array(args.parent), device=np.array(torch.cuda.get_device_name(0)),
                        **inp, **{"out_" + k: v for k, v in rec.items()})
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
