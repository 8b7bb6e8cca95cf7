"""osr_cascade_refine (csrc/osr_cascade.hip) and osr_cascade_candidates (csrc/osr_det_tail.hip) against a torch fp32 restatement
of detectron2's CascadeROIHeads written here: predict_boxes + _create_proposals_from_boxes + _match_and_label_boxes between two stages, and the
averaged scores + fast_rcnn_inference_single_image up to its NMS behind the last one.

Integer outputs (classes, matched indices, batch_idx, counts) are compared bit-exactly, boxes under the project's 1e-4 fp32 contract
(|got - ref| <= 1e-4 pixels on boxes inside images of at most 220 pixels: the device's expf against libm's; measured 7.6e-6 to
1.5e-5). The tolerances of the candidates test are the issue's: scores 1e-6 (measured 8.9e-8), boxes 1e-4 (measured 1.5e-5), rows
whose score lies within 1e-6 of the threshold left out of the set comparison (fewer than 1 % of them)."""
import math

import numpy as np
import pytest
import torch

DEV = "cuda:0"
CLAMP = math.log(1000.0 / 16.0)


def _next_up(x: float) -> float:
    """The fp32 value one float above fp32(x)."""
    return float(np.nextafter(np.float32(x), np.float32(2.0)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def ref_apply_deltas(deltas, boxes, weights):
    """[d2] Box2BoxTransform.apply_deltas, class-agnostic."""
    wx, wy, ww, wh = weights
    widths, heights = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    ctr_x, ctr_y = boxes[:, 0] + 0.5 * widths, boxes[:, 1] + 0.5 * heights
    dx, dy = deltas[:, 0] / wx, deltas[:, 1] / wy
    dw, dh = torch.clamp(deltas[:, 2] / ww, max=CLAMP), torch.clamp(deltas[:, 3] / wh, max=CLAMP)
    pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
    pw, ph = torch.exp(dw) * widths, torch.exp(dh) * heights
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1)


def ref_clip(b, h, w):
    """[d2] Boxes.clip (a NaN stays a NaN)."""
    return torch.stack((b[:, 0].clamp(min=0, max=w), b[:, 1].clamp(min=0, max=h), b[:, 2].clamp(min=0, max=w), b[:, 3].clamp(min=0, max=h)), dim=1)


def ref_pairwise_iou(gt, b):
    """[d2] pairwise_iou (G, R): inter / (a1 + a2 - inter) where inter > 0, else 0."""
    a1 = ((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))[:, None]
    a2 = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    w = (torch.min(gt[:, None, 2], b[None, :, 2]) - torch.max(gt[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.min(gt[:, None, 3], b[None, :, 3]) - torch.max(gt[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = w * h
    return torch.where(inter > 0, inter / (a1 + a2 - inter), torch.zeros(()))


def ref_refine(boxes, bidx, deltas, n, hw, weights, drop_empty, gt=None, gcls=None, gcnt=None, num_classes=0, thr=0.5):
    m = boxes.shape[0]
    rows = m // n
    ob, obi = torch.zeros(m, 4), torch.full((m,), -1, dtype=torch.int32)
    ocl, ogt, ogi = torch.full((m,), -1, dtype=torch.int64), torch.zeros(m, 4), torch.full((m,), -1, dtype=torch.int32)
    counts = torch.zeros(n, 3, dtype=torch.int32)
    for i in range(n):
        sl = slice(i * rows, (i + 1) * rows)
        b = ref_clip(ref_apply_deltas(deltas[sl], boxes[sl], weights), float(hw[i][0]), float(hw[i][1]))
        ex = bidx[sl] >= 0
        if drop_empty:  # [d2] Boxes.nonempty
            ex = ex & ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        ob[sl] = torch.where(ex[:, None], b, torch.zeros(()))
        obi[sl] = torch.where(ex, torch.tensor(i, dtype=torch.int32), torch.tensor(-1, dtype=torch.int32))
        counts[i, 0] = int(ex.sum())
        if gt is None:
            continue
        g = int(gcnt[i])
        if g == 0:  # every row background, zero gt_boxes
            ocl[sl] = torch.where(ex, torch.tensor(num_classes), torch.tensor(-1))
            counts[i, 2] = int(ex.sum())
            continue
        iou = ref_pairwise_iou(gt[i, :g], b)                                      # (g, rows); a NaN box gives NaN
        iou = torch.where(torch.isnan(iou), torch.zeros(()), iou)              # (fmaxf / `>` on the device: a NaN never wins)
        best = iou.max(dim=0).values
        first = torch.where(iou == best[None, :], torch.arange(g)[:, None], torch.tensor(g)).min(dim=0).values  # lowest index among equals
        fg = best >= torch.tensor(thr, dtype=torch.float32)
        ocl[sl] = torch.where(ex, torch.where(fg, gcls[i, first], torch.tensor(num_classes)), torch.tensor(-1))
        ogt[sl] = torch.where(ex[:, None], gt[i, first], torch.zeros(()))
        ogi[sl] = torch.where(ex & fg, first.to(torch.int32), torch.tensor(-1, dtype=torch.int32))
        counts[i, 1], counts[i, 2] = int((ex & fg).sum()), int((ex & ~fg).sum())
    return dict(boxes=ob, batch_idx=obi, counts=counts, gt_classes=ocl, gt_boxes=ogt, gt_idx=ogi)


# ---- osr_cascade_refine ---------------------------------------------------------------------------------------------------------
ROWS = 64
HW = ((100, 120), (80, 90))
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
# image 1's three boxes: g0 for the exact-threshold rows; g1 / g2 overlap a row equally (the lower index wins)
GT3 = ((0.0, 0.0, 10.0, 6.0), (50.0, 20.0, 80.0, 60.0), (52.0, 20.0, 82.0, 60.0))
NAN = float("nan")


def _refine_case(count0):
    """2 images x 64 rows. Every image's first rows are the edge cases; the rest are random boxes (some near the ground truth) with
    random deltas; a few rows do not exist."""
    g = torch.Generator().manual_seed(11)
    n = 2
    boxes, deltas = torch.zeros(n, ROWS, 4), torch.zeros(n, ROWS, 4)
    bidx = torch.arange(n, dtype=torch.int32)[:, None].repeat(1, ROWS)
    gt = torch.zeros(n, 3, 4)
    gt[0, 0] = torch.tensor(GT3[0])
    gt[1] = torch.tensor(GT3)
    gcls = torch.tensor([[4, 0, 0], [2, 6, 1]], dtype=torch.int64)
    gcnt = torch.tensor([count0, 3], dtype=torch.int32)
    for i, (h, w) in enumerate(HW):
        xy = torch.rand(ROWS, 2, generator=g) * torch.tensor([w * 0.8, h * 0.8])
        wh = torch.rand(ROWS, 2, generator=g) * 40 + 4
        boxes[i] = torch.cat((xy, xy + wh), dim=1)
        deltas[i] = torch.randn(ROWS, 4, generator=g) * torch.tensor([2.0, 2.0, 1.0, 1.0])
        near = torch.tensor(GT3)[torch.randint(0, 3, (16,), generator=g)] + torch.randn(16, 4, generator=g) * 2.0  # rows around the ground truth
        boxes[i, 40:56] = near
        deltas[i, 40:56] *= 0.1
        special = [
            ((0.0, 0.0, 10.0, 10.0), (0, 0, 0, 0)),          # 0: IoU with g0 = 60 / 100 = fl(0.6)
            ((0.0, 0.0, 10.0, 12.0), (0, 0, 0, 0)),          # 1: IoU with g0 = 60 / 120 = 0.5
            ((51.0, 20.0, 81.0, 60.0), (0, 0, 0, 0)),        # 2: IoU 1160 / 1240 with g1 AND g2 (foreground tie)
            ((60.0, 30.0, 70.0, 40.0), (0, 0, 0, 0)),        # 3: inside g1 and g2, IoU 100 / 1200 with both (background tie: matched box g1)
            ((w - 20.0, 10.0, w - 2.0, 30.0), (30.0, 0, 0, 0)),  # 4: the deltas move it past the right edge: clips to an empty box
            ((w + 10.0, 10.0, w + 30.0, 30.0), (0, 0, 0, 0)),    # 5: wholly outside the image, right
            ((-30.0, -30.0, -5.0, -5.0), (0, 0, 0, 0)),      # 6: wholly outside, top left
            ((20.0, 20.0, 30.0, 30.0), (0, 0, 500.0, 500.0)),    # 7: size deltas beyond the scale clamp
            ((20.0, 20.0, 30.0, 30.0), (NAN, 0, 0, 0)),      # 8: a NaN centre delta
            ((20.0, 20.0, 30.0, 30.0), (0, 0, 0, NAN)),      # 9: a NaN size delta (torch.clamp keeps it, fminf would not)
            ((20.0, 20.0, 20.0, 30.0), (0, 0, 0, 0)),        # 10: a zero-width input box
            ((NAN, NAN, NAN, NAN), (NAN, NAN, NAN, NAN)),    # 11: does not exist (garbage stays unread)
        ]
        for j, (b, d) in enumerate(special):
            boxes[i, j], deltas[i, j] = torch.tensor(b), torch.tensor([float(v) for v in d])
        bidx[i, 11] = -1
        bidx[i, 33] = -1
        bidx[i, 60:] = -1
    return n, boxes.view(-1, 4), bidx.view(-1), deltas.view(-1, 4), torch.tensor(HW, dtype=torch.int32), gt, gcls, gcnt


def _close(got, ref, what):
    """The 1e-4 fp32 contract; NaNs in the same places. Prints the measured error."""
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), what
    fin = ~torch.isnan(ref)
    err = float((got[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
    print(f"[{what}] max |got - ref| = {err:.3e} (bound 1e-4)")
    assert err <= 1e-4, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("drop_empty", [False, True], ids=["keep", "drop_empty"])
@pytest.mark.parametrize("count0", [0, 1])
@pytest.mark.parametrize("thr", [0.5, _next_up(0.5), 0.6, _next_up(0.6)], ids=["0.5", "0.5+1ulp", "0.6", "0.6+1ulp"])
def test_cascade_refine_with_ground_truth(osr, drop_empty, count0, thr):
    from openset_rcnn_amd.host import ops
    n, boxes, bidx, deltas, hw, gt, gcls, gcnt = _refine_case(count0)
    ref = ref_refine(boxes, bidx, deltas, n, HW, WEIGHTS, drop_empty, gt, gcls, gcnt, 80, thr)
    got = ops.cascade_refine(boxes.to(DEV), bidx.to(DEV), deltas.to(DEV), n, hw.to(DEV), WEIGHTS, drop_empty, gt.to(DEV), gcls.to(DEV),
                             gcnt.to(DEV), 80, thr)
    got = {k: v.cpu() for k, v in got.items()}
    for k in ("batch_idx", "gt_classes", "gt_idx", "counts"):
        assert torch.equal(got[k], ref[k]), (k, got[k], ref[k])
    _close(got["boxes"], ref["boxes"], "refine boxes")
    _close(got["gt_boxes"], ref["gt_boxes"], "refine gt_boxes")
    # ---- the edge rows, spelled out (image 1: three ground-truth boxes) ----
    r = ROWS
    cls, gi, bi = got["gt_classes"], got["gt_idx"], got["batch_idx"]
    at6, at5 = thr <= float(np.float32(0.6)), thr <= 0.5  # IoU exactly at the threshold is foreground, one float below is not
    assert (int(cls[r + 0]), int(gi[r + 0])) == ((2, 0) if at6 else (80, -1))
    assert (int(cls[r + 1]), int(gi[r + 1])) == ((2, 0) if at5 else (80, -1))
    assert (int(cls[r + 2]), int(gi[r + 2])) == (6, 1)                                      # equal IoU with g1 and g2: the lower index
    assert (int(cls[r + 3]), int(gi[r + 3])) == (80, -1) and got["gt_boxes"][r + 3].tolist() == list(GT3[1])  # background keeps the matched box
    for j in (4, 5, 6, 10):  # empty after the clip: kept at inference, dropped in training
        assert int(bi[r + j]) == (-1 if drop_empty else 1) and int(cls[r + j]) == (-1 if drop_empty else 80)
        if drop_empty:
            assert got["boxes"][r + j].tolist() == [0.0] * 4 and got["gt_boxes"][r + j].tolist() == [0.0] * 4
    assert got["boxes"][r + 7].tolist() == [0.0, 0.0, 90.0, 80.0]  # 10 * 1000 / 16 wide and high, clipped to the image
    for j in (8, 9):
        assert bool(torch.isnan(got["boxes"][r + j]).any()) != drop_empty and int(bi[r + j]) == (-1 if drop_empty else 1)
    assert int(bi[r + 11]) == -1 and int(cls[r + 11]) == -1 and got["boxes"][r + 11].tolist() == [0.0] * 4
    if count0 == 0:  # no ground truth in image 0: background everywhere, zero gt_boxes
        ex = bi[:r] >= 0
        assert bool((cls[:r][ex] == 80).all()) and not bool(got["gt_boxes"][:r].any()) and int(got["counts"][0, 1]) == 0
    assert int(got["counts"][1, 1]) > 3 and int(got["counts"][1, 2]) > 3  # the random rows give both kinds


@pytest.mark.gpu
def test_cascade_refine_at_inference_and_repeats(osr):
    from openset_rcnn_amd.host import ops
    n, boxes, bidx, deltas, hw, gt, gcls, gcnt = _refine_case(1)
    ref = ref_refine(boxes, bidx, deltas, n, HW, (20.0, 20.0, 10.0, 10.0), False)
    dev = [t.to(DEV) for t in (boxes, bidx, deltas)]
    got = ops.cascade_refine(*dev, n, hw.to(DEV), (20.0, 20.0, 10.0, 10.0))
    assert set(got) == {"boxes", "batch_idx", "counts"}
    assert torch.equal(got["batch_idx"].cpu(), bidx)  # every existing row stays
    assert torch.equal(got["counts"].cpu(), ref["counts"]) and got["counts"][:, 1:].abs().sum().item() == 0
    _close(got["boxes"].cpu(), ref["boxes"], "refine boxes, inference")
    again = ops.cascade_refine(*dev, n, hw.to(DEV), (20.0, 20.0, 10.0, 10.0))
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)  # bit-identical (NaNs included)
    full = ops.cascade_refine(*dev, n, hw.to(DEV), WEIGHTS, True, gt.to(DEV), gcls.to(DEV), gcnt.to(DEV), 80, 0.5)
    full2 = ops.cascade_refine(*dev, n, hw.to(DEV), WEIGHTS, True, gt.to(DEV), gcls.to(DEV), gcnt.to(DEV), 80, 0.5)
    assert all(torch.equal(full[k], full2[k]) for k in full)


@pytest.mark.gpu
def test_cascade_refine_many_rows_and_bad_arguments(osr):
    """More rows than one pass of the workgroup (256 threads), a row count that is no multiple of it; gmax above the LDS table."""
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(5)
    n, rows = 3, 601
    xy = torch.rand(n * rows, 2, generator=g) * 150
    boxes = torch.cat((xy, xy + torch.rand(n * rows, 2, generator=g) * 60 + 1), dim=1)
    deltas = torch.randn(n * rows, 4, generator=g) * torch.tensor([2.0, 2.0, 1.0, 1.0])
    bidx = torch.arange(n, dtype=torch.int32)[:, None].repeat(1, rows)
    bidx[torch.rand(n, rows, generator=g) < 0.1] = -1
    hwl = ((200, 220), (160, 180), (128, 160))
    gt = torch.tensor([[[10.0, 10.0, 90.0, 100.0], [100.0, 50.0, 190.0, 150.0]]]).repeat(n, 1, 1)
    gcls = torch.tensor([[1, 2]] * n, dtype=torch.int64)
    gcnt = torch.tensor([2, 1, 2], dtype=torch.int32)
    ref = ref_refine(boxes, bidx.view(-1), deltas, n, hwl, WEIGHTS, True, gt, gcls, gcnt, 5, 0.3)
    hw = torch.tensor(hwl, dtype=torch.int32).to(DEV)
    got = ops.cascade_refine(boxes.to(DEV), bidx.view(-1).to(DEV), deltas.to(DEV), n, hw, WEIGHTS, True, gt.to(DEV), gcls.to(DEV), gcnt.to(DEV), 5, 0.3)
    got = {k: v.cpu() for k, v in got.items()}
    # (a random row within an ulp of the threshold could flip; none does with this seed, and the comparison stays exact)
    for k in ("batch_idx", "gt_classes", "gt_idx", "counts"):
        assert torch.equal(got[k], ref[k]), k
    _close(got["boxes"], ref["boxes"], "refine boxes, 3 x 601 rows")
    assert int(got["counts"][:, 1].min()) > 0
    big = ops.CASCADE_MAX_GT + 1
    with pytest.raises(ops.OsrError, match="gmax"):
        ops.cascade_refine(boxes.to(DEV), bidx.view(-1).to(DEV), deltas.to(DEV), n, hw, WEIGHTS, True, torch.zeros(n, big, 4, device=DEV),
                           torch.zeros(n, big, dtype=torch.int64, device=DEV), gcnt.to(DEV), 5, 0.3)
    with pytest.raises(ops.OsrError, match="positive"):
        ops.cascade_refine(boxes.to(DEV), bidx.view(-1).to(DEV), deltas.to(DEV), n, hw, (10.0, 10.0, 0.0, 5.0))


# ---- osr_cascade_candidates -----------------------------------------------------------------------------------------------------
def _cand_case(stages, n=2, rows=1100, k=7, seed=3):
    """rows > 1024: a second pass of the workgroup. The first stage's logits favour a class per row so that a good share of the
    scores passes the threshold; NaN / Inf logits and deltas in a few rows; rows that do not exist at the end and in the middle."""
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn(n * rows, k + 1, generator=g) * 2.0 for _ in range(stages)]
    deltas = torch.randn(n * rows, 4, generator=g) * torch.tensor([3.0, 3.0, 1.5, 1.5])
    xy = torch.rand(n * rows, 2, generator=g) * 100
    boxes = torch.cat((xy, xy + torch.rand(n * rows, 2, generator=g) * 50 + 2), dim=1).view(n, rows, 4)
    counts = torch.tensor([rows, rows - 400][:n], dtype=torch.int32)
    bidx = torch.where(torch.arange(rows)[None, :] < counts[:, None], torch.arange(n, dtype=torch.int32)[:, None], torch.tensor(-1, dtype=torch.int32))
    logits[0][5, 2] = NAN
    logits[-1][6, 0] = float("inf")
    deltas[7, 0] = NAN
    deltas[8, 3] = NAN
    deltas[9, 2] = float("inf")   # clamped: stays a candidate row
    deltas[10, 1] = float("inf")  # a non-finite centre: dropped
    return logits, deltas, boxes.contiguous(), counts, bidx.contiguous().view(-1), torch.tensor([(128, 160), (120, 140)][:n], dtype=torch.int32), k


@pytest.mark.gpu
def test_cascade_candidates_one_stage_is_fastrcnn_candidates(osr):
    """Both entry points launch one kernel template (cand_kernel<1>), so this compares a kernel with itself: what it still checks is
    that a row list given by batch_idx selects the rows its prefix counts select. What the two separate kernels computed before they
    were merged is held by tests/test_det_tail_pin.py."""
    from openset_rcnn_amd.host import ops
    logits, deltas, boxes, counts, bidx, hw, k = _cand_case(1)
    dev = lambda t: t.to(DEV)  # noqa: E731
    want = ops.fastrcnn_candidates(dev(logits[0]), dev(deltas), dev(boxes), dev(counts), dev(hw), k, WEIGHTS, 0.05)
    got = ops.cascade_candidates([dev(logits[0])], dev(deltas), dev(boxes), dev(bidx), dev(hw), k, WEIGHTS, 0.05)
    assert got["cap"] == want["cap"] and torch.equal(got["count"], want["count"])
    for i, c in enumerate(want["count"].cpu().tolist()):
        assert c > 100
        for key in ("boxes", "scores", "cls", "row"):
            assert got[key].shape == want[key].shape and torch.equal(got[key][i, :c], want[key][i, :c]), (i, key)


def _ref_candidates(logits, deltas, boxes, bidx, hw, k, weights, thr):
    """Per image: (rows, classes, scores, boxes) of the candidates in row-major order, and every existing valid row's scores."""
    n, rows = boxes.shape[0], boxes.shape[1]
    stages = len(logits)
    out = []
    for i in range(n):
        sl = slice(i * rows, (i + 1) * rows)
        probs = [torch.softmax(l[sl], dim=-1) for l in logits]
        scores = sum(probs) * (1.0 / stages)  # [d2] CascadeROIHeads._forward_box
        b = ref_apply_deltas(deltas[sl], boxes[i], weights)
        valid = torch.isfinite(b).all(dim=1) & torch.isfinite(scores).all(dim=1) & (bidx[sl] >= 0)
        b = ref_clip(b, float(hw[i][0]), float(hw[i][1]))
        sc = scores[:, :-1]
        mask = (sc > thr) & valid[:, None]
        idx = mask.nonzero()
        out.append(dict(row=idx[:, 0], cls=idx[:, 1], score=sc[mask], box=b[idx[:, 0]], scores=sc, valid=valid))
    return out


@pytest.mark.gpu
def test_cascade_candidates_three_stages_match_the_restatement(osr):
    from openset_rcnn_amd.host import ops
    thr, w3 = 0.05, (30.0, 30.0, 15.0, 15.0)
    logits, deltas, boxes, counts, bidx, hw, k = _cand_case(3)
    bidx = bidx.clone()
    bidx[20:25] = -1  # rows that do not exist, in the middle of an image's list
    ref = _ref_candidates(logits, deltas, boxes, bidx, hw, k, w3, thr)
    dev = lambda t: t.to(DEV)  # noqa: E731
    args = ([dev(l) for l in logits], dev(deltas), dev(boxes), dev(bidx), dev(hw), k, w3, thr)
    got = ops.cascade_candidates(*args)
    again = ops.cascade_candidates(*args)
    cnt = got["count"].cpu().tolist()
    rows = boxes.shape[1]
    worst_s = worst_b = 0.0
    for i, r in enumerate(ref):
        c = cnt[i]
        assert torch.equal(got["count"], again["count"])
        for key in ("boxes", "scores", "cls", "row"):  # a repeat is bit-identical
            assert torch.equal(got[key][i, :c], again[key][i, :c]), key
        # rows with a score within 1e-6 of the threshold may fall on either side: left out of the set comparison (< 1 % of the rows)
        near = ((r["scores"] - thr).abs() <= 1e-6).any(dim=1) & r["valid"]
        assert int(near.sum()) < 0.01 * rows, int(near.sum())
        grow, gcls = got["row"][i, :c].cpu().long(), got["cls"][i, :c].cpu().long()
        gk, rk = ~near[grow], ~near[r["row"]]
        assert torch.equal(grow[gk], r["row"][rk]) and torch.equal(gcls[gk], r["cls"][rk]), i
        assert int(rk.sum()) > 200  # (the case is not empty)
        ds = float((got["scores"][i, :c].cpu()[gk] - r["score"][rk]).abs().max())
        db = float((got["boxes"][i, :c].cpu()[gk] - r["box"][rk]).abs().max())
        worst_s, worst_b = max(worst_s, ds), max(worst_b, db)
    print(f"[cascade_candidates, 3 stages] max |score - ref| = {worst_s:.3e} (bound 1e-6), max |box - ref| = {worst_b:.3e} (bound 1e-4)")
    assert worst_s <= 1e-6 and worst_b <= 1e-4
    # rows 5 (NaN logit), 6 (Inf logit), 7 / 8 (NaN deltas), 10 (Inf centre delta) and the rows that do not exist give no candidate
    rows0 = set(got["row"][0, :cnt[0]].cpu().tolist())
    assert not rows0 & {5, 6, 7, 8, 10, 20, 21, 22, 23, 24}
    with pytest.raises(ops.OsrError, match="stages"):
        ops.cascade_candidates([args[0][0]] * 5, *args[1:])


# ---- osr_nms_topk beyond 1024 kept boxes ([d2]'s cascade configs: RPN.POST_NMS_TOPK_TRAIN 2000) -----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("topk", [1024, 1025, 2000, 2048])
def test_nms_topk_keeps_up_to_2048(osr, topk):
    """The keep list of the RPN's per-level NMS at a POST_NMS_TOPK above the 1024-entry table: index for index the C oracle's
    batched NMS (the level as category), more than 1024 boxes kept."""
    from openset_rcnn_amd.host import ops
    from oracle import c_binding as CO
    rng = np.random.default_rng(17)
    nseg, stride, lens = 2, 4000, [4000, 2600]
    xy = rng.uniform(0, 1200, (nseg, stride, 2)).astype(np.float32)
    boxes = np.concatenate((xy, xy + rng.uniform(8, 90, (nseg, stride, 2)).astype(np.float32)), axis=2)
    scores = rng.standard_normal((nseg, stride)).astype(np.float32)
    scores[0, 100:110] = scores[0, 99]  # ties: the lower index first
    lvl = rng.integers(0, 5, (nseg, stride)).astype(np.int32)
    keep, cnt = ops.nms_topk(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(lvl).to(DEV), None, nseg, stride,
                             torch.tensor(lens, dtype=torch.int32).to(DEV), 0.7, topk)
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    for s in range(nseg):
        k = CO.batched_nms(boxes[s, : lens[s]], scores[s, : lens[s]], lvl[s, : lens[s]].astype(np.int64), 0.7)
        assert len(k) > 2048  # (the list is cut by topk, not by the NMS)
        assert cnt[s] == topk and keep[s].tolist() == k[:topk].tolist(), f"segment {s}"
    if topk == 2048:
        with pytest.raises(ops.OsrError, match="topk"):
            ops.nms_topk(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(lvl).to(DEV), None, nseg, stride,
                         torch.tensor(lens, dtype=torch.int32).to(DEV), 0.7, 2049)
