"""The Openset heads' training kernels (csrc/osr_train_fwd.hip, osr_train_bwd.hip, the dense RoIAlign backward of osr_roi_align.hip) at
production sizes and at their edges, against plain fp64 restatements on the CPU (the oracle's functions on .double() inputs where they
allow it).

Paths reached (VOC-COCO training: batch 16 at 800 x 1344, 512 sampled RoIs per image):
- rpn_losses_kernel / rpn_losses_bwd_kernel at n = 16, A = 1 (1 432 368 anchors) and A = 3 (4 297 104): the forward's 256 x 256 threads
  loop 1 432 368 / 65 536 = 22 times (66 at A = 3), the backward's 1024 x 256 threads 5.5 times (16.4). Labels at the sampler's density
  (256 per image) and dense (every turn has work); every box loss type; the level-major pred_off indexing on all five levels.
- cfrpn_tail_bwd_kernel + cfrpn_tail_bwd_reduce over the same 1 432 368 rows: each of the 512 x 4 = 2048 waves takes ~700 rows
  (dw in registers over all of them); the reduce's 16 groups sum per = 2048 / 16 = 128 partials each.
- roi_box_losses_kernel, ce_loss_kernel (256 x 256 threads) and their backward kernels (256 x 256) at m = 8192 and m = 65 537: the
  second grid turn takes row 65 536 (a foreground row with a valid softmax target, so dropping it changes every result).
- pln_loss_kernel / pln_bwd_rows_kernel (1024 waves): 8 turns of osr_pln_row at m = 8192, 9 at 8229. pln_bwd_protos_kernel walks
  the rows in PLN_LIST = 512 chunks: 16 of them, a partial 17th of 37 rows at m = 8229, and one chunk whose 512 rows all name the same
  prototype (a full hit list). K = 28 x 5 prototypes at d = 256 is 146 064 B of dynamic LDS in the prototype pass. d = 1024 runs the
  OSR_PLN_REG instance; d = 1536 (forward) the out-of-register path; 80 x 4 = 320 prototypes > 256 workgroups give the forward's
  centre-term loop a second turn. Two classes share identical prototypes (exact ties of the inter argmin) and some IoUs equal the
  threshold exactly (foreground is IoU > threshold).
- roi_align_bwd_dense_kernel at n = 16, S = 512, c = 256 on P2-P5 of 800 x 1344: all four waves hold channels (ch = wid * 64 + lane),
  the hit test runs two passes of its 256-thread loop and the wave-0 compaction 8 ballots (16 at S = 1024, a partial one at S = 300);
  RoIs clustered on a ground-truth box hit some 8 x 8 tiles more than 256 times (double-buffered s_w across many hits).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O
from tests.test_std_kernels_full_size import _level_major_index

DEV = "cuda:0"
SHAPES = O.level_shapes(800, 1344)
NAN, INF = float("nan"), float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(name, err, tol):
    """Prints the observed error next to its bound (pytest -s shows it) and checks it."""
    print(f"[err] {name}: {err:.3e} (tol {tol:.1e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.1e}"


def _max_err(got, ref):
    """Largest elementwise |got - ref| relative to max|ref| (fp64)."""
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _apart(pred, gt, margin=0.02):
    """Moves target coordinates (in place) at least `margin` px away from every coordinate of the same axis of the predicted box. The
    box losses' gradients jump where two such coordinates meet (which box defines the intersection or the enclosing box; the kernels
    route the gradient to the strictly selected one, torch splits ties), and fp32 rounding moves that point by ~1e-4 px."""
    for _ in range(3):
        for k in range(4):
            ax = [0, 2] if k % 2 == 0 else [1, 3]
            near = ((gt[:, k:k + 1] - pred[:, ax]).abs() < margin).any(1)
            gt[near, k] += 3.0 * margin * (1.0 if k >= 2 else -1.0)
    return gt


def _poison_values(g, k):
    return torch.tensor([NAN, INF, -INF])[torch.randint(0, 3, (k,), generator=g)]


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


# ------------------------------------------------------------------------------------------------------------------------------
# 1. ClsFreeRPN.losses, forward and backward
# ------------------------------------------------------------------------------------------------------------------------------
def _rpn_case(seed, n, a, dense):
    """Labels image-major (n, R) as the target kernels leave them; predictions level-major as the head writes them."""
    from openset_rcnn_amd.host.engine_std import cell_anchor_table
    ratios = (1.0,) if a == 1 else (0.5, 1.0, 2.0)
    g = _gen(seed)
    anchors = torch.cat(O.anchor_grid(SHAPES, O.FPN_STRIDES, O.ANCHOR_SIZES, ratios))
    R = anchors.shape[0]
    if dense:  # every anchor labelled: every grid turn has positives, negatives and ignored anchors
        lr = torch.randint(-1, 2, (n, R), generator=g).to(torch.int8)
        lo = torch.randint(-1, 2, (n, R), generator=g).to(torch.int8)
    else:  # the sampler's density: 256 per image, <= 128 positive (regression) / any share positive (objectness, fraction 1.0)
        lr = torch.full((n, R), -1, dtype=torch.int8)
        lo = torch.full((n, R), -1, dtype=torch.int8)
        edge, off = [], 0
        for h, w in SHAPES:  # every level's first and last pixel
            edge += list(range(off, off + a)) + list(range(off + (h * w - 1) * a, off + h * w * a))
            off += h * w * a
        for i in range(n):
            for lab, cap in ((lr, 129), (lo, 257)):
                pick = torch.randperm(R, generator=g)[:256]
                npos = 0 if i == 5 else int(torch.randint(1, cap, (1,), generator=g))  # image 5: no positive
                lab[i, pick] = 0
                lab[i, pick[:npos]] = 1
        lr[0, edge] = 1
        lo[0, edge] = 1
    ctr = 0.5 * (anchors[:, :2] + anchors[:, 2:])
    wh = (anchors[:, 2:] - anchors[:, :2]) * torch.exp(torch.randn(n, R, 2, generator=g) * 0.3)
    c = ctr + torch.randn(n, R, 2, generator=g) * 4.0
    matched = torch.cat([c - 0.5 * wh, c + 0.5 * wh], -1).contiguous()
    ctr_t = torch.rand(n, R, generator=g)
    m = n * R
    # ltrb deltas mostly positive; x1 / y2 negative on some rows (the ReLU of apply_deltas), never both of one axis (no empty box)
    deltas = (torch.randn(m, 4, generator=g) * 0.4).abs() + 0.05
    u = torch.rand(m, generator=g)
    deltas[u < 0.1, 0] *= -1.0
    deltas[(u >= 0.1) & (u < 0.2), 3] *= -1.0
    pctr = torch.rand(m, generator=g) * 0.96 + 0.02  # sigmoid outputs
    pi = _level_major_index(SHAPES, n, a)
    anc = anchors.double().repeat(n, 1)
    cx, cy = 0.5 * (anc[:, 0] + anc[:, 2]), 0.5 * (anc[:, 1] + anc[:, 3])
    aw, ah = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    dd = deltas.double()[pi.view(-1)].clamp(min=0)
    pb = torch.stack([cx - dd[:, 0] * aw, cy - dd[:, 1] * ah, cx + dd[:, 2] * aw, cy + dd[:, 3] * ah], 1)
    matched = _apart(pb, matched.view(-1, 4).double()).float().view(n, R, 4).contiguous()
    lv_args = (SHAPES, O.FPN_STRIDES, n, a)
    cell = cell_anchor_table(O.ANCHOR_SIZES, ratios)
    return dict(n=n, a=a, anchors=anchors, lr=lr, lo=lo, matched=matched, ctr_t=ctr_t, deltas=deltas, pctr=pctr, lv_args=lv_args,
                cell=cell, pi=pi)


def _rpn_reference(c, box, ctr_beta):
    """fp64 losses through O.rpn_losses and the (rows, 5) gradient w.r.t. {4 deltas, centerness logit}, level-major."""
    dl = c["deltas"].double().requires_grad_(True)
    cl = c["pctr"].double().requires_grad_(True)
    pi = c["pi"]
    ref = O.rpn_losses(c["anchors"].double(), dl[pi], cl[pi], c["lr"], c["lo"], c["matched"].double(), c["ctr_t"].double(), box_loss=box,
                       ctr_beta=ctr_beta)
    (ref["loss_rpn_loc"] + ref["loss_rpn_ctr"]).backward()
    p = cl.detach()
    d = torch.cat([dl.grad, (cl.grad * p * (1.0 - p)).unsqueeze(1)], 1)  # through the sigmoid
    return ref, d


def _run_rpn(ops, c, t, box, ctr_beta):
    lv = ops.make_rpn_levels(*c["lv_args"])
    cell = c["cell"].to(DEV)
    kw = dict(box_loss=box, ctr_beta=ctr_beta)
    out = ops.rpn_losses_fwd(lv, cell, c["n"], *t, **kw)
    d = ops.rpn_losses_bwd(lv, cell, c["n"], *t, loss_scale=1.0, **kw)
    torch.cuda.synchronize()
    return out.cpu(), d.cpu()


def _check_rpn(ops, seed, a, dense, box, ctr_beta):
    c = _rpn_case(seed, 16, a, dense)
    t = [x.to(DEV).contiguous() for x in (c["deltas"], c["pctr"], c["lr"], c["lo"], c["matched"], c["ctr_t"])]
    out, d = _run_rpn(ops, c, t, box, ctr_beta)
    ref, dref = _rpn_reference(c, box, ctr_beta)
    name = f"rpn {box[0]} A{a} {'dense' if dense else 'sampled'}"
    assert [int(v) for v in out[2:6]] == [ref["num_pos"], ref["num_neg"], ref["obj_num_pos"], ref["obj_num_neg"]]
    _report(name + " loss_loc", abs(out[0].item() / float(ref["loss_rpn_loc"]) - 1.0), 5e-5)
    _report(name + " loss_ctr", abs(out[1].item() / float(ref["loss_rpn_ctr"]) - 1.0), 5e-5)
    assert d.shape == dref.shape
    _report(name + " d_out5", _max_err(d, dref), 1e-4)
    lr_lm = torch.empty(c["deltas"].shape[0], dtype=torch.int8)
    lr_lm[c["pi"].view(-1)] = c["lr"].view(-1)
    lo_lm = torch.empty_like(lr_lm)
    lo_lm[c["pi"].view(-1)] = c["lo"].view(-1)
    assert (d[lr_lm != 1, :4] == 0).all()       # delta columns of non-positive anchors: exactly 0
    assert (d[lo_lm == -1, 4] == 0).all()       # centerness column of ignored anchors: exactly 0
    out2, d2 = _run_rpn(ops, c, t, box, ctr_beta)
    assert torch.equal(out2, out) and torch.equal(d2, d)
    # NaN / Inf where the loss does not look: deltas / matched boxes of non-positives, centerness / its target of ignored anchors
    g = _gen(seed + 1)
    pd, pc, pm, pt = c["deltas"].clone(), c["pctr"].clone(), c["matched"].clone(), c["ctr_t"].clone()
    nd, nc = lr_lm != 1, lo_lm == -1
    pd[nd] = _poison_values(g, int(nd.sum()) * 4).view(-1, 4)
    pc[nc] = _poison_values(g, int(nc.sum()))
    pm[c["lr"] != 1] = _poison_values(g, int((c["lr"] != 1).sum()) * 4).view(-1, 4)
    pt[c["lo"] == -1] = _poison_values(g, int((c["lo"] == -1).sum()))
    tp = [x.to(DEV).contiguous() for x in (pd, pc, c["lr"], c["lo"], pm, pt)]
    out3, d3 = _run_rpn(ops, c, tp, box, ctr_beta)
    assert torch.equal(out3, out) and torch.equal(d3, d)


RPN_BOXES = [(("iou", 0.0), 0.0), (("giou", 0.0), 0.0), (("diou", 0.0), 0.0), (("ciou", 0.0), 0.0), (("smooth_l1", 0.1), 0.2)]


@pytest.mark.gpu
@pytest.mark.parametrize("box,ctr_beta", RPN_BOXES, ids=[b[0][0] for b in RPN_BOXES])
def test_rpn_losses_sampled_labels(ops, box, ctr_beta):
    """A = 1, 256 sampled anchors per image (image 5 without a positive, image 0 positive on every level's first and last pixel)."""
    _check_rpn(ops, 11, 1, False, box, ctr_beta)


@pytest.mark.gpu
@pytest.mark.parametrize("box,ctr_beta", [RPN_BOXES[0], RPN_BOXES[4]], ids=["iou", "smooth_l1"])
def test_rpn_losses_dense_labels(ops, box, ctr_beta):
    _check_rpn(ops, 12, 1, True, box, ctr_beta)


@pytest.mark.gpu
def test_rpn_losses_three_anchors(ops):
    """A = 3 (ratios 0.5, 1, 2): 4.3 M anchors through the same level table."""
    _check_rpn(ops, 13, 3, False, ("iou", 0.0), 0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. ClsFreeRPNHead tail backward
# ------------------------------------------------------------------------------------------------------------------------------
TAIL_ROWS = sum(16 * h * w for h, w in SHAPES)  # 1 432 368


def _ulp(x, dtype):
    """Spacing of the output format at |x| (subnormals included)."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


@pytest.fixture(scope="module")
def tail_inputs():
    g = torch.Generator(device=DEV).manual_seed(21)
    t = torch.randn(TAIL_ROWS, 256, device=DEV, generator=g).relu_()
    gc = _gen(22)
    zero_rows = torch.cat([torch.tensor([0, 1, TAIL_ROWS - 1]), torch.randperm(TAIL_ROWS, generator=gc)[:5000]])
    t[zero_rows.to(DEV)] = 0.0  # the clamped-norm branch
    w = torch.randn(5, 256, generator=gc) * 0.5
    # sparse: the sampled anchors only (16 x 256, a share of them on all-zero rows); dense: every row but 10 %
    sp_rows = torch.unique(torch.cat([zero_rows[:300], torch.tensor([2, TAIL_ROWS - 2]), torch.randperm(TAIL_ROWS, generator=gc)[:4096]]))
    d_sparse = torch.zeros(TAIL_ROWS, 5)
    d_sparse[sp_rows] = torch.randn(len(sp_rows), 5, generator=gc)
    d_dense = torch.randn(TAIL_ROWS, 5, generator=gc)
    d_dense[torch.rand(TAIL_ROWS, generator=gc) < 0.1] = 0.0
    return t, w, {"sparse": d_sparse, "dense": d_dense}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sparse", "dense"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_cfrpn_tail_bwd_full_pyramid(ops, tail_inputs, dtype, form):
    """dt within 1 ulp of the output type of the fp64 value plus 2^-18 of its terms' scale (|d| |W| + |u| sum(|u| |d| |W|)) / ||t||; exact zeros on rows without a gradient
    and where t <= 0. dw / db within (rows per wave + partials per group + 16 groups + 10) * 2^-24 * sum|terms|: the kernel's fixed
    fp32 summation order, and u's own rounding."""
    t32, w, ds = tail_inputs
    d = ds[form]
    td = t32.to(dtype)
    dt, dw, db = ops.cfrpn_tail_bwd(td, w.to(DEV), d.to(DEV))
    dt2, dw2, db2 = ops.cfrpn_tail_bwd(td, w.to(DEV), d.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(dt2, dt) and torch.equal(dw2, dw) and torch.equal(db2, db)
    t, dt = td.cpu(), dt.cpu()
    w64 = w.double()
    ref_dw, abs_dw = torch.zeros(5, 256, dtype=torch.float64), torch.zeros(5, 256, dtype=torch.float64)
    worst = 0.0
    for r0 in range(0, TAIL_ROWS, 65536):
        tc = t[r0:r0 + 65536].double()
        dc = d[r0:r0 + 65536].double()
        nrm = tc.norm(dim=1, keepdim=True)
        inv = 1.0 / nrm.clamp(min=1e-12)
        u = tc * inv
        du = dc @ w64
        dot = (u * du).sum(1, keepdim=True)
        ref = torch.where(nrm > 1e-12, (du - u * dot) * inv, du * inv) * (tc > 0)
        adu = dc.abs() @ w64.abs()  # (du and u . du are sums that cancel: their error scales with the sums of |terms|)
        scale = (adu + u.abs() * (u.abs() * adu).sum(1, keepdim=True)) * inv
        got = dt[r0:r0 + 65536]
        err = (got.double() - ref).abs()
        bound = _ulp(ref.float(), dtype).double() + 2.0 ** -18 * scale
        worst = max(worst, float((err / bound).max()))
        assert (got[~(tc > 0)] == 0).all() and (got[(dc == 0).all(1)] == 0).all()
        ref_dw += dc.t() @ u
        abs_dw += dc.abs().t() @ u.abs()
    _report(f"tail {form} {dtype} dt (in units of its bound)", worst, 1.0)
    nparts = 512 * 4
    bound = (math.ceil(TAIL_ROWS / nparts) + nparts // 16 + 16 + 10) * 2.0 ** -24
    _report(f"tail {form} {dtype} dw (units of sum|terms|)", float(((dw.cpu().double() - ref_dw).abs() / abs_dw.clamp(min=1e-30)).max()), bound)
    d64 = d.double()
    ref_db, abs_db = d64.sum(0), d64.abs().sum(0)
    _report(f"tail {form} {dtype} db (units of sum|terms|)", float(((db.cpu().double() - ref_db).abs() / abs_db).max()), bound)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. RoI box / IoU losses and softmax cross entropy
# ------------------------------------------------------------------------------------------------------------------------------
NC = {20: 81, 28: 88}  # NUM_CLASSES of voc_coco.yaml / graspnet.yaml


def _roi_case(seed, m, k):
    """Rows in 512-row image blocks: known classes, unknown ones in [K, NUM_CLASSES), background (== NUM_CLASSES) and padding (-1)
    scattered through every block; image 1 all padding. Row m - 1 is a known-class foreground row (the second grid turn at 65 537)."""
    nc = NC[k]
    g = _gen(seed)
    u = torch.rand(m, generator=g)
    cls = torch.randint(0, k, (m,), generator=g)
    cls[u < 0.55] = nc
    cls[(u >= 0.55) & (u < 0.62)] = torch.randint(k, nc, (m,), generator=g)[(u >= 0.55) & (u < 0.62)]
    cls[(u >= 0.62) & (u < 0.72)] = -1
    cls[512:1024] = -1
    cls[m - 1] = 3
    p = torch.rand(m, 2, generator=g) * 600.0
    prop = torch.cat([p, p + 8.0 + torch.rand(m, 2, generator=g) * 300.0], 1)
    gtb = prop + torch.randn(m, 4, generator=g) * 8.0
    gtb[:, 2:] = torch.maximum(gtb[:, 2:], gtb[:, :2] + 1.0)
    pred = torch.randn(m, 5, generator=g) * 0.5
    pred[:, 4] *= 4.0  # IoU logits
    big = torch.rand(m, generator=g)
    pred[big < 0.03, 2] = 25.0 + torch.rand(m, generator=g)[big < 0.03]   # beyond the scale clamp: 25 / 5 > log(1000 / 16)
    pred[(big >= 0.03) & (big < 0.05), 3] = 30.0
    pred[m - 1, :4] = torch.tensor([3.0, -2.0, 1.0, -1.0])  # (a large loss on the last row)
    gtb = _apart(_b2b_apply64(pred.double(), prop.double()), gtb.double()).float()
    gi = torch.rand(m, generator=g)
    logits = torch.randn(m, k + 1, generator=g) * 3.0
    hot = torch.nonzero(torch.rand(m, generator=g) < 0.05).view(-1)  # |x| ~ 100: exp overflows fp32 without the max subtraction
    logits[hot, torch.randint(0, k + 1, (len(hot),), generator=g)] = 100.0
    logits[hot[::2]] -= 100.0 * (torch.rand(len(hot[::2]), 1, generator=g) > 0.5)
    return cls, prop, gtb, pred, gi, logits


def _b2b_apply64(deltas, boxes, weights=(10.0, 10.0, 5.0, 5.0)):
    """O.b2b_apply_deltas without its cast to fp32."""
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    dw = torch.clamp(deltas[:, 2] / weights[2], max=O.SCALE_CLAMP)
    dh = torch.clamp(deltas[:, 3] / weights[3], max=O.SCALE_CLAMP)
    pcx, pcy = deltas[:, 0] / weights[0] * w + cx, deltas[:, 1] / weights[1] * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1)


def _box_reference(cls, prop, gtb, pred, gi, nc, box, iou_beta):
    valid = cls >= 0
    p = pred.double().requires_grad_(True)
    pv, c = p[valid], cls[valid]
    fg = c < nc
    r = max(c.numel(), 1)
    if box[0] == "smooth_l1":  # the targets in fp32, as [d2] Box2BoxTransform.get_deltas forms them (and the kernels)
        tgt = O.b2b_get_deltas(prop[valid][fg], gtb[valid][fg]).double()
        lb = O.smooth_l1(pv[fg, :4] - tgt, box[1]).sum() / r * 0.5
    else:  # (O.roi_box_losses decodes in fp32)
        dec = _b2b_apply64(pv[fg, :4], prop[valid][fg].double())
        lb = O.box_pair_losses(dec, gtb[valid][fg].double(), box[0]).sum() / r * 0.5
    li = O.smooth_l1(torch.sigmoid(pv[fg, 4]) - gi[valid][fg].double(), iou_beta).sum() / r * 0.5
    if valid.any():
        (lb + li).backward()
        grad = p.grad
    else:
        lb, li, grad = torch.zeros(()), torch.zeros(()), torch.zeros_like(p)
    return float(lb.detach()), float(li.detach()), int(valid.sum()), grad


def _run_box(ops, t, nc, box, iou_beta):
    pred, prop, gtb, cls, gi = t
    out = ops.roi_box_losses_fwd(pred[:, :4], pred[:, 4], prop, gtb, cls, gi, nc, iou_is_logit=True, box_loss=box, iou_beta=iou_beta)
    d = ops.roi_box_losses_bwd(pred, prop, gtb, cls, gi, nc, loss_scale=1.0, box_loss=box, iou_beta=iou_beta)
    torch.cuda.synchronize()
    return out.cpu(), d.cpu()


ROI_BOXES = [(("smooth_l1", 0.0), 0.0), (("smooth_l1", 0.5), 0.1), (("iou", 0.0), 0.0), (("giou", 0.0), 0.0), (("diou", 0.0), 0.0),
             (("ciou", 0.0), 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("box,iou_beta", ROI_BOXES, ids=[f"{b[0][0]}{b[0][1]}" for b in ROI_BOXES])
@pytest.mark.parametrize("m,k", [(8192, 20), (65537, 20), (8192, 28), (65537, 28)])
def test_roi_box_losses_full_size(ops, m, k, box, iou_beta):
    nc = NC[k]
    cls, prop, gtb, pred, gi, _ = _roi_case(100 + m + k, m, k)
    t = [x.to(DEV).contiguous() for x in (pred, prop, gtb, cls, gi)]
    out, d = _run_box(ops, t, nc, box, iou_beta)
    lb, li, rows, dref = _box_reference(cls, prop, gtb, pred, gi, nc, box, iou_beta)
    name = f"roi box {box[0]} m{m} K{k}"
    assert int(out[2]) == rows
    _report(name + " loss_box", abs(out[0].item() / lb - 1.0), 5e-5)
    _report(name + " loss_iou", abs(out[1].item() / li - 1.0), 5e-5)
    _report(name + " d_pred", _max_err(d, dref), 1e-4)
    off = (cls < 0) | (cls == nc)
    assert (d[off] == 0).all()                                       # padding and background rows: exactly 0
    if box[0] != "smooth_l1":
        assert (d[pred[:, 2] / 5.0 >= O.SCALE_CLAMP, 2] == 0).all()  # beyond the scale clamp: exactly 0
        assert (d[pred[:, 3] / 5.0 >= O.SCALE_CLAMP, 3] == 0).all()
    out2, d2 = _run_box(ops, t, nc, box, iou_beta)
    assert torch.equal(out2, out) and torch.equal(d2, d)
    g = _gen(m + 1)
    pp, pb, pg, pi = pred.clone(), prop.clone(), gtb.clone(), gi.clone()
    k_off = int(off.sum())
    pp[off] = _poison_values(g, k_off * 5).view(-1, 5)
    pb[off] = _poison_values(g, k_off * 4).view(-1, 4)
    pg[off] = _poison_values(g, k_off * 4).view(-1, 4)
    pi[off] = _poison_values(g, k_off)
    out3, d3 = _run_box(ops, [x.to(DEV).contiguous() for x in (pp, pb, pg, cls, pi)], nc, box, iou_beta)
    assert torch.equal(out3, out) and torch.equal(d3, d)


def _run_ce(ops, logits, cls, nc):
    out = ops.softmax_ce_loss_fwd(logits, cls, nc, 0.9)
    d = ops.softmax_ce_loss_bwd(logits, cls, nc, 0.9, loss_scale=1.0)
    torch.cuda.synchronize()
    return out.cpu(), d.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(8192, 20), (65537, 20), (8192, 28), (65537, 28)])
def test_softmax_ce_loss_full_size(ops, m, k):
    """Logits of +-100 on 5 % of the rows (exp overflows without the max subtraction); unknown classes and padding are not counted."""
    nc = NC[k]
    cls, _, _, _, _, logits = _roi_case(200 + m + k, m, k)
    t = (logits.to(DEV).contiguous(), cls.to(DEV))
    out, d = _run_ce(ops, *t, nc)
    valid = cls >= 0
    lg = logits.double().requires_grad_(True)
    ref = O.softmax_ce_loss(lg[valid], cls[valid], nc, k, 0.9)
    ref.backward()
    _report(f"ce m{m} K{k} loss", abs(out[0].item() / float(ref) - 1.0), 5e-5)
    _report(f"ce m{m} K{k} d_logits", _max_err(d, lg.grad), 1e-4)
    off = (cls < 0) | ((cls >= k) & (cls < nc))
    assert (d[off] == 0).all()
    assert torch.isfinite(d).all()
    out2, d2 = _run_ce(ops, *t, nc)
    assert torch.equal(out2, out) and torch.equal(d2, d)
    pl = logits.clone()
    pl[off] = _poison_values(_gen(m), int(off.sum()) * (k + 1)).view(-1, k + 1)
    out3, d3 = _run_ce(ops, pl.to(DEV).contiguous(), cls.to(DEV), nc)
    assert torch.equal(out3, out) and torch.equal(d3, d)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["padding", "unknown"])
def test_roi_losses_no_counted_row(ops, fill):
    """No row counts: every row padding (box, IoU and CE losses 0) or every row an unknown class (CE over no row: 0). Gradients 0."""
    m, k = 8192, 20
    nc = NC[k]
    cls, prop, gtb, pred, gi, logits = _roi_case(300, m, k)
    cls = torch.full((m,), -1, dtype=torch.int64) if fill == "padding" else torch.randint(k, nc, (m,), generator=_gen(301))
    out, d = _run_box(ops, [x.to(DEV).contiguous() for x in (pred, prop, gtb, cls, gi)], nc, ("smooth_l1", 0.0), 0.0)
    ce, dce = _run_ce(ops, logits.to(DEV).contiguous(), cls.to(DEV), nc)
    assert ce.tolist() == [0.0] and (dce == 0).all()
    if fill == "padding":
        assert out.tolist() == [0.0, 0.0, 0.0] and (d == 0).all()
    else:
        lb, li, rows, dref = _box_reference(cls, prop, gtb, pred, gi, nc, ("smooth_l1", 0.0), 0.0)
        assert int(out[2]) == rows == m and torch.isfinite(d).all()
        _report("roi box all-unknown d_pred", _max_err(d, dref), 1e-4)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. PLN loss
# ------------------------------------------------------------------------------------------------------------------------------
def _first_argmin(x, dim):
    """argmin with ties to the lowest index (the kernels' rule: a later candidate replaces the current one only if strictly smaller)."""
    mn = x.min(dim, keepdim=True).values
    idx = torch.arange(x.shape[dim]).view([-1 if i == (dim % x.dim()) else 1 for i in range(x.dim())]).expand_as(x)
    return torch.where(x == mn, idx, torch.full_like(idx, x.shape[dim])).min(dim).values


def _pln_case(seed, m, k, reps, d, twins=(7, 12), full_chunk=None):
    nc = NC.get(k, 81)
    g = _gen(seed)
    protos = torch.randn(k * reps, d, generator=g) * 1.5
    if twins:
        a, b = twins
        protos[b * reps:(b + 1) * reps] = protos[a * reps:(a + 1) * reps]  # identical prototypes: exact ties of the inter argmin
    u = torch.rand(m, generator=g)
    cls = torch.randint(0, k, (m,), generator=g)
    cls[u < 0.4] = nc
    cls[(u >= 0.4) & (u < 0.45)] = torch.randint(k, nc, (m,), generator=g)[(u >= 0.4) & (u < 0.45)]
    cls[(u >= 0.45) & (u < 0.5)] = -1
    ious = torch.rand(m, generator=g) * 0.5 + 0.4
    ious[torch.rand(m, generator=g) < 0.06] = 0.5  # == IOU_THRESHOLD: not foreground
    if full_chunk is not None:
        cls[full_chunk * 512:(full_chunk + 1) * 512] = 5
        ious[full_chunk * 512:(full_chunk + 1) * 512] = 0.9
    near = protos[cls.clamp(0, k - 1) * reps + torch.randint(0, reps, (m,), generator=g)]
    emb = torch.randn(m, d, generator=g) + torch.rand(m, 1, generator=g) * 3.0 * near
    return emb, protos, cls, ious


def _pln_reference(emb, protos, cls, ious, k, reps, alpha, beta, weight, twins=(7, 12), thr=0.5):
    """fp64 PLN loss and its gradients w.r.t. the embeddings and the raw prototypes (COS). The argmins are restated explicitly with
    the kernels' tie rule (lowest index); the twins' distance columns are equalised for the selection, since the fp64 matmul need not
    give bit-equal columns for equal prototypes. Returns (loss, O.pln_loss_terms' loss, d_emb, d_protos, hits per prototype)."""
    e = emb.double().requires_grad_(True)
    p = protos.double().requires_grad_(True)
    rows = max(int((cls >= 0).sum()), 1)
    fg = (cls >= 0) & (cls < k) & (ious > thr)
    new, rep = F.normalize(e[fg]), F.normalize(p)
    y = cls[fg]
    dist = 1.0 - new @ rep.t()
    with torch.no_grad():
        dd = dist.clone()
        if twins:
            a, b = twins
            dd[:, b * reps:(b + 1) * reps] = dd[:, a * reps:(a + 1) * reps]
        f = dd.shape[0]
        q = _first_argmin(dd.view(f, k, reps), 2)                      # nearest prototype of each class
        md = dd.view(f, k, reps).gather(2, q.unsqueeze(2)).squeeze(2)
        ar = torch.arange(f)
        md[ar, y] = INF
        ic = _first_argmin(md, 1)                                       # nearest other class
        i_intra, i_inter = y * reps + q[ar, y], ic * reps + q[ar, ic]
    intra, inter = dist[ar, i_intra], dist[ar, i_inter]
    cd = (1.0 - rep @ rep.t()).clone()
    blk = torch.arange(k * reps) // reps
    with torch.no_grad():
        cdd = cd.clone()
        cdd[blk.view(-1, 1) == blk.view(1, -1)] = INF
        jc = _first_argmin(cdd, 1)
    cdist = cd[torch.arange(k * reps), jc]
    loss = (torch.clamp(intra - alpha, min=0).sum() + torch.clamp(beta - inter, min=0).sum() + torch.clamp(beta + alpha - cdist, min=0).sum())
    loss = loss * weight / rows
    loss.backward()
    oracle = O.pln_loss_terms(F.normalize(emb.double()), F.normalize(protos.double()), cls, ious, alpha, beta, k, thr, reps, "COS") * weight / rows
    # rows that name prototype j (intra or inter pair), per 512-row chunk of the row list
    fg_rows = torch.nonzero(fg).view(-1)
    hits = torch.zeros((len(cls) + 511) // 512, k * reps, dtype=torch.int64)
    for idx in (i_intra, i_inter):
        hits.index_put_((fg_rows // 512, idx), torch.ones(len(idx), dtype=torch.int64), accumulate=True)
    both = i_intra == i_inter
    hits.index_put_((fg_rows[both] // 512, i_intra[both]), -torch.ones(int(both.sum()), dtype=torch.int64), accumulate=True)
    return float(loss), float(oracle), e.grad, p.grad, hits


PLN_CASES = {  # name: m, K, reps, d, alpha, beta, full chunk
    "K20": (8192, 20, 1, 256, 0.1, 0.9, 3),
    "K20-partial-chunk": (8192 + 37, 20, 1, 256, 0.1, 0.9, 2),
    "K28-reps5": (8192, 28, 5, 256, 0.05, 0.95, None),
    "d1024": (8192, 20, 1, 1024, 0.1, 0.9, 7),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PLN_CASES))
def test_pln_loss_full_size(ops, case):
    m, k, reps, d, alpha, beta, full = PLN_CASES[case]
    emb, protos, cls, ious = _pln_case(400 + m + d + k, m, k, reps, d, full_chunk=full)
    loss, oracle, g_emb, g_protos, hits = _pln_reference(emb, protos, cls, ious, k, reps, alpha, beta, 0.5)
    assert loss == pytest.approx(oracle, rel=1e-12)  # the restatement is the oracle's loss
    if full is not None:
        assert int(hits[full].max()) == 512          # one chunk's hit list exactly full
    assert int(hits.gt(0).sum(0).max()) > 1          # (prototypes named from several chunks)
    t = [x.to(DEV).contiguous() for x in (emb, protos, cls, ious)]
    fw = ops.pln_loss_fwd(t[0], F.normalize(protos).to(DEV), t[2], t[3], 0.5, alpha, beta, 0.5, reps=reps).cpu()
    de, dp = ops.pln_loss_bwd(t[0], t[1], t[2], t[3], 0.5, alpha, beta, 0.5, loss_scale=1.0, reps=reps)
    de2, dp2 = ops.pln_loss_bwd(t[0], t[1], t[2], t[3], 0.5, alpha, beta, 0.5, loss_scale=1.0, reps=reps)
    torch.cuda.synchronize()
    assert torch.equal(dp2, dp) and torch.equal(de2, de)
    de, dp = de.cpu(), dp.cpu()
    _report(f"pln {case} loss", abs(fw[0].item() / oracle - 1.0), 2e-5)
    _report(f"pln {case} d_emb", _max_err(de, g_emb), 1e-4)
    _report(f"pln {case} d_protos", _max_err(dp, g_protos), 1e-4)
    fg = (cls >= 0) & (cls < k) & (ious > 0.5)
    assert (de[~fg] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m,k,reps,d", [(8192, 80, 4, 64), (8192, 20, 1, 1536)], ids=["320-prototypes", "d1536"])
def test_pln_loss_forward_only_shapes(ops, m, k, reps, d):
    """Forward only (the backward takes d <= 1024): 320 prototypes (the centre-term loop's second turn over 256 workgroups) and
    d = 1536 > OSR_PLN_REG * 64 (the row is re-read from memory per prototype)."""
    emb, protos, cls, ious = _pln_case(500 + d, m, k, reps, d)
    oracle = float(O.pln_loss_terms(F.normalize(emb.double()), F.normalize(protos.double()), cls, ious, 0.1, 0.9, k, 0.5, reps, "COS")) * 0.5 / int((cls >= 0).sum())
    fw = ops.pln_loss_fwd(emb.to(DEV), F.normalize(protos).to(DEV), cls.to(DEV), ious.to(DEV), 0.5, 0.1, 0.9, 0.5, reps=reps).cpu()
    _report(f"pln forward K{k}x{reps} d{d} loss", abs(fw[0].item() / oracle - 1.0), 2e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. Dense RoIAlign backward at training size
# ------------------------------------------------------------------------------------------------------------------------------
RA_SCALES = (0.25, 0.125, 0.0625, 0.03125)
RA_SHAPES = SHAPES[:4]
RA_CH = [0, 1, 63, 64, 127, 128, 191, 192, 255]  # the first and last lane of every wave
P7 = 7


def _axis_weights(lo, hi, scale, size):
    """(r, 7, size) fp64: the weight of every pixel of one axis in every bin, the oracle's roi_align_torch sample positions and taps
    restated in vectorised fp32 (same operations in the same order); a sample outside [-1, size] has weight 0. Returns (weights, grid)."""
    f32 = np.float32
    s = lo.astype(f32) * f32(scale) - f32(0.5)
    e = hi.astype(f32) * f32(scale) - f32(0.5)
    rl = (e - s).astype(f32)
    bs = (rl / f32(P7)).astype(f32)
    grid = np.ceil(rl.astype(np.float64) / P7).astype(np.int64)
    gmax = max(int(grid.max()), 1) if len(grid) else 1
    r = len(lo)
    pb = np.arange(P7, dtype=f32).reshape(1, P7, 1)
    ii = np.arange(gmax, dtype=f32).reshape(1, 1, gmax)
    a = (s.reshape(-1, 1, 1) + pb * bs.reshape(-1, 1, 1)).astype(f32)
    b = ((ii + f32(0.5)) * bs.reshape(-1, 1, 1)).astype(f32) / np.maximum(grid, 1).astype(f32).reshape(-1, 1, 1)
    v = (a + b.astype(f32)).astype(f32)
    ok = (ii < grid.reshape(-1, 1, 1)) & ~((v < -1.0) | (v > size))
    vv = np.maximum(v, f32(0.0))
    vl = np.clip(vv.astype(np.int64), 0, size - 1)
    edge = vv.astype(np.int64) >= size - 1
    vh = np.where(edge, size - 1, vl + 1)
    vv = np.where(edge, vl.astype(f32), vv)
    fl = (vv - vl.astype(f32)).astype(f32)
    wl = (f32(1.0) - fl).astype(np.float64) * ok
    wh = fl.astype(np.float64) * ok
    out = np.zeros((r, P7, size))
    rr = np.broadcast_to(np.arange(r).reshape(-1, 1, 1), v.shape)
    bb = np.broadcast_to(np.arange(P7).reshape(1, -1, 1), v.shape)
    np.add.at(out, (rr, bb, vl), wl)
    np.add.at(out, (rr, bb, vh), wh)
    return out, grid


def _roi_levels(boxes):
    return O.assign_levels(boxes)


def _roi_align_bwd_ref(boxes, bidx, dout, n, shapes=RA_SHAPES, scales=RA_SCALES):
    """fp64 gradient of the feature pyramid (list of (n, h, w, c)) for dout (m, 7, 7, c) fp64, the RoIAlign forward being separable:
    d feat[y][x] = sum over RoIs and bins of wy[by][y] wx[bx][x] d out[by][bx] / count."""
    lv = _roi_levels(boxes)
    outs = []
    c = dout.shape[-1]
    for l, (h, w) in enumerate(shapes):
        o = torch.zeros(n, h, w, c, dtype=torch.float64)
        for b in range(n):
            ids = torch.nonzero((lv == l) & (bidx == b)).view(-1)
            if len(ids) == 0:
                continue
            bx = boxes[ids].numpy()
            wy, gy = _axis_weights(bx[:, 1], bx[:, 3], scales[l], h)
            wx, gx = _axis_weights(bx[:, 0], bx[:, 2], scales[l], w)
            wy = torch.from_numpy(wy / np.maximum(gy * gx, 1).reshape(-1, 1, 1))
            u = torch.einsum("rqx,rpqc->rpxc", torch.from_numpy(wx), dout[ids])
            o[b] = (wy.reshape(-1, h).t() @ u.reshape(-1, w * c)).view(h, w, c)
        outs.append(o)
    return outs


def _ra_boxes(g, k, img_w=1344.0, img_h=800.0):
    """k RoIs spread over the image: log-uniform sizes, aspect ratios up to ~4, some crossing the border."""
    ctr = torch.rand(k, 2, generator=g) * torch.tensor([img_w + 100.0, img_h + 100.0]) - 50.0
    sz = torch.exp(torch.rand(k, 1, generator=g) * math.log(900.0 / 8.0)) * 8.0
    asp = torch.exp(torch.randn(k, 1, generator=g) * 0.5)
    wh = torch.cat([sz * asp.sqrt(), sz / asp.sqrt()], 1)
    return torch.cat([ctr - 0.5 * wh, ctr + 0.5 * wh], 1)


def _ra_list(seed, n, S):
    """The image-major (n * S) list of the sampler: per image a few GT boxes with jittered copies (25 %; 70 % around one large box in
    images 0 and 1, whose tiles are then hit by more than 256 RoIs), the rest spread, and padding rows (batch_idx -1, NaN boxes)
    inside the block."""
    g = _gen(seed)
    boxes = torch.full((n * S, 4), NAN)
    bidx = torch.full((n * S,), -1, dtype=torch.int32)
    for b in range(n):
        npad = int(torch.randint(S // 16, S // 8 + 1, (1,), generator=g))
        nv = S - npad
        gt = _ra_boxes(g, 3)
        gt[0] = torch.tensor([350.0, 150.0, 1000.0, 640.0]) + torch.randn(4, generator=g) * 20.0
        frac = 0.7 if b < 2 else 0.25
        nj = int(frac * nv)
        src = gt[0].expand(nj, 4) if b < 2 else gt[torch.randint(0, 3, (nj,), generator=g)]
        wh = (src[:, 2:] - src[:, :2]).repeat(1, 2)
        jit = src + torch.randn(nj, 4, generator=g) * 0.06 * wh
        rois = torch.cat([jit, _ra_boxes(g, nv - nj)])
        rois = rois[torch.randperm(nv, generator=g)]
        slots = torch.sort(torch.randperm(S, generator=g)[:nv]).values + b * S
        boxes[slots] = rois
        bidx[slots] = b
    return boxes, bidx


def _dense_bwd(dout, n, boxes, bidx, S, out_dtype):
    """osr_roi_align_bwd_dense itself (ops.roi_align_bwd would take the scatter kernel if it refused), into NaN-filled outputs:
    every element must be written."""
    from openset_rcnn_amd.host import _lib, ops
    lib = _lib.load()
    m, c = dout.shape[0], dout.shape[-1]
    outs = [torch.full((n, h, w, c), NAN, dtype=out_dtype, device=DEV) for h, w in RA_SHAPES]
    py = _lib.Pyramid()
    py.num_levels, py.c = len(outs), c
    for i, (f, s) in enumerate(zip(outs, RA_SCALES)):
        py.h[i], py.w[i], py.scale[i], py.data[i] = f.shape[1], f.shape[2], s, f.data_ptr()
    st = lib.osr_roi_align_bwd_dense(C.byref(py), n, ops._p(boxes), ops._p(bidx), m, S, P7, 4, 224, 2, ops._p(dout), ops._DT[dout.dtype],
                                     ops._DT[out_dtype], ops._stream())
    assert st == 0, f"osr_roi_align_bwd_dense: status {st}"
    torch.cuda.synchronize()
    return outs


def _ra_inputs(seed, n, S, dtype):
    boxes, bidx = _ra_list(seed, n, S)
    g = torch.Generator(device=DEV).manual_seed(seed)
    dout = torch.randn(n * S, P7, P7, 256, device=DEV, generator=g)
    pad = torch.nonzero(bidx < 0).view(-1)
    dout[pad.to(DEV)] = _poison_values(_gen(seed), len(pad) * P7 * P7 * 256).view(-1, P7, P7, 256).to(DEV)  # garbage behind padding
    return boxes, bidx, dout.to(dtype)


def _ra_max_hits(boxes, bidx, n):
    """Most RoIs of one image meeting one 8 x 8 tile by the kernel's conservative footprint test."""
    lv = _roi_levels(boxes.nan_to_num())
    best = 0
    for l, ((h, w), s) in enumerate(zip(RA_SHAPES, RA_SCALES)):
        for b in range(n):
            bx = boxes[(lv == l) & (bidx == b)]
            if len(bx) == 0:
                continue
            cov = torch.zeros((h + 7) // 8, (w + 7) // 8, dtype=torch.int64)
            lo = torch.floor(bx[:, :2] * s - 0.5) - 1
            hi = torch.floor(bx[:, 2:] * s - 0.5) + 2
            for (x0, y0), (x1, y1) in zip(lo.tolist(), hi.tolist()):
                tx0, ty0 = max(int(x0), 0) // 8, max(int(y0), 0) // 8
                tx1, ty1 = min(int(x1), w - 1) // 8, min(int(y1), h - 1) // 8
                if tx1 >= tx0 and ty1 >= ty0:
                    cov[ty0:ty1 + 1, tx0:tx1 + 1] += 1
            best = max(best, int(cov.max()))
    return best


RA_CASES = {"n16-S512-fp16": (16, 512, torch.float16), "n16-S512-bf16": (16, 512, torch.bfloat16), "n8-S1024-fp16": (8, 1024, torch.float16),
            "n16-S300-bf16": (16, 300, torch.bfloat16)}


@pytest.fixture(scope="module")
def ra_runs(ops):
    cache = {}

    def get(case):
        if case not in cache:
            n, S, dt = RA_CASES[case]
            boxes, bidx, dout = _ra_inputs(700 + S + n, n, S, dt)
            bd, id_ = boxes.to(DEV), bidx.to(DEV)
            f32 = _dense_bwd(dout, n, bd, id_, S, torch.float32)
            cache[case] = (n, S, dt, boxes, bidx, dout, f32)
        return cache[case]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(RA_CASES))
def test_roi_align_bwd_dense_training_size(ops, ra_runs, case):
    """Against the fp64 restatement on every pixel of every level for the channels RA_CH, against the scatter kernel on the full
    tensor, bit-identical on repeat; the low-precision output is the fp32 result rounded once."""
    n, S, dt, boxes, bidx, dout, got = ra_runs(case)
    bd, id_ = boxes.to(DEV), bidx.to(DEV)
    if S == 512:
        assert _ra_max_hits(boxes, bidx, n) > 256
    again = _dense_bwd(dout, n, bd, id_, S, torch.float32)
    low = _dense_bwd(dout, n, bd, id_, S, dt)
    scat = ops.roi_align_bwd(dout, RA_SHAPES, n, RA_SCALES, bd, id_)
    torch.cuda.synchronize()
    for l in range(4):
        assert torch.isfinite(got[l]).all(), f"level {l}: an element not written, or garbage behind a padding row read"
        assert torch.equal(again[l], got[l]), f"level {l}: not bit-reproducible"
        assert torch.equal(low[l], got[l].to(dt)), f"level {l}: low-precision output is not the fp32 sums rounded once"
        _report(f"roi_align dense {case} level {l} vs scatter", float((got[l] - scat[l]).abs().max() / scat[l].abs().max()), 1e-5)
    del again, low, scat
    ch = torch.tensor(RA_CH)
    valid = bidx >= 0
    sub = torch.zeros(n * S, P7, P7, len(RA_CH), dtype=torch.float64)
    sub[valid] = dout[:, :, :, ch.to(DEV)].cpu().double()[valid]
    ref = _roi_align_bwd_ref(boxes.nan_to_num(), bidx, sub, n)
    for l in range(4):
        _report(f"roi_align dense {case} level {l} vs fp64", _max_err(got[l][..., ch.to(DEV)].cpu(), ref[l]), 2e-5)


@pytest.mark.gpu
def test_roi_align_bwd_dense_keeps_an_inf(ops, ra_runs):
    """An Inf in one RoI's d out (one bin, channel 64) must reach every pixel that bin weighs (the overflow skip of the training step
    relies on it) and may spread only inside the 8 x 8 tiles the RoI's footprint reaches, in that channel; every other channel is
    bit-identical to the clean run."""
    n, S, dt, boxes, bidx, dout, clean = ra_runs("n16-S512-fp16")
    lv = _roi_levels(boxes.nan_to_num())
    ph, pw, chn = 3, 2, 64
    h, w = RA_SHAPES[1]
    for r in torch.nonzero((bidx == 3) & (lv == 1)).view(-1).tolist():  # the first RoI of image 3 on P3 whose bin (3, 2) has weight
        bx = boxes[r:r + 1].numpy()
        wy, _ = _axis_weights(bx[:, 1], bx[:, 3], RA_SCALES[1], h)
        wx, _ = _axis_weights(bx[:, 0], bx[:, 2], RA_SCALES[1], w)
        must = torch.from_numpy(np.outer(wy[0, ph] > 0, wx[0, pw] > 0))
        if must.any():
            break
    bad = dout.clone()
    bad[r, ph, pw, chn] = INF
    got = _dense_bwd(bad, n, boxes.to(DEV), bidx.to(DEV), S, torch.float32)
    rows_t = torch.from_numpy(wy[0].sum(0) > 0)
    cols_t = torch.from_numpy(wx[0].sum(0) > 0)
    ty = torch.zeros((h + 7) // 8, dtype=torch.bool).index_fill_(0, torch.nonzero(rows_t).view(-1) // 8, True)
    tx = torch.zeros((w + 7) // 8, dtype=torch.bool).index_fill_(0, torch.nonzero(cols_t).view(-1) // 8, True)
    allowed = (ty.view(-1, 1) & tx.view(1, -1)).repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w]
    assert int(must.sum()) > 0
    for l in range(4):
        other = torch.ones(256, dtype=torch.bool, device=DEV)
        other[chn] = False
        assert torch.equal(got[l][..., other], clean[l][..., other]), f"level {l}: another channel changed"
        bad_px = ~torch.isfinite(got[l][..., chn]).cpu()
        if l != 1:
            assert not bad_px.any()
            continue
        assert not bad_px[torch.arange(n) != 3].any(), "the Inf reached another image"
        assert bad_px[3][must].all(), "the Inf was dropped where its bin has weight"
        assert not bad_px[3][~allowed].any(), "non-finite outside the tiles the RoI's footprint reaches"
        print(f"[err] roi_align Inf: {int(must.sum())} weighted pixels non-finite, {int(bad_px[3].sum())} non-finite in "
              f"{int(allowed.sum())} pixels of the reached tiles")


def test_roi_align_bwd_reference_matches_the_oracle():
    """The vectorised restatement above against autograd through O.roi_align_torch (fp64) on clustered, spread, border-crossing,
    sub-pixel and wide RoIs of two images (CPU only)."""
    g = _gen(900)
    boxes = torch.cat([_ra_boxes(g, 40), torch.tensor([[-40.0, -30.0, 90.0, 50.0], [1200.0, 700.0, 1400.0, 840.0], [50.3, 60.2, 51.1, 61.0],
                                                       [4.0, 100.0, 1300.0, 112.0], [0.0, 0.0, 1344.0, 800.0]])])
    boxes = torch.cat([boxes, boxes[:6] + torch.randn(6, 4, generator=g)])
    bidx = torch.randint(0, 2, (len(boxes),), generator=g, dtype=torch.int32)
    c = 3
    dout = torch.randn(len(boxes), P7, P7, c, generator=g, dtype=torch.float64)
    ref = _roi_align_bwd_ref(boxes, bidx, dout, 2)
    lv = _roi_levels(boxes)
    for l, ((h, w), s) in enumerate(zip(RA_SHAPES, RA_SCALES)):
        ids = torch.nonzero(lv == l).view(-1)
        feat = torch.zeros(2, c, h, w, dtype=torch.float64, requires_grad=True)
        if len(ids):
            rois = torch.cat([bidx[ids].double().unsqueeze(1), boxes[ids].double()], 1)
            O.roi_align_torch(feat, rois, s).backward(dout[ids].permute(0, 3, 1, 2))
            assert _max_err(ref[l].permute(0, 3, 1, 2), feat.grad) < 1e-6, f"level {l}"
        else:
            assert (ref[l] == 0).all()
