"""The stock heads' training kernels (csrc/osr_std_train.hip, the _ex sparse RPN backward) at production sizes and at their edges,
against plain restatements on the CPU: fp64 for sums and gradients, fp32 where d2 itself computes in fp32 (the regression targets
of Box2BoxTransform.get_deltas, the argmax).

Paths reached:
- osr_std_rpn_losses_fwd/_bwd at n = 16, 800 x 1344, A = 3 (4.3 M anchors): the forward's 256 x 256 threads loop ~66 times, the
  backward's 4096-block grid ~4 times.
- osr_fastrcnn_losses_fwd at m = 65537 > 256 workgroups x 256 threads: its grid-stride loop runs a second turn.
- osr_std_rpn_tail_bwd at 4096 and 5000 rows: each of the 256 waves accumulates 16-20 rows in registers; every width 5..40, so every
  template instance including the default branch (40).
- osr_rpn_sparse_rows_ex / osr_rpn_gather_cols_ex over the 1.43 M pixel rows of n = 16 at 800 x 1344, widths 1, 15, 40 and 64.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

DEV = "cuda:0"
STRIDES = (4, 8, 16, 32, 64)
SIZES = (32, 64, 128, 256, 512)


def _smooth_l1(x, beta):
    if beta < 1e-5:
        return x.abs()
    n = x.abs()
    return torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)


def _get_deltas32(src, tgt, w):
    """[d2] Box2BoxTransform.get_deltas in fp32, the precision d2 forms the regression targets in."""
    src, tgt = src.float(), tgt.float()
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tcx, tcy = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    return torch.stack([w[0] * (tcx - scx) / sw, w[1] * (tcy - scy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)], 1)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. [d2] RPN.losses
# ------------------------------------------------------------------------------------------------------------------------------
def _level_major_index(shapes, n, a):
    """(n, R) int64: element index in the level-major (rows * A) prediction buffers of anchor r of image i (level, y, x, a minor)."""
    cols, off = [], 0
    for h, w in shapes:
        k = h * w * a
        cols.append(off + torch.arange(n).view(n, 1) * k + torch.arange(k).view(1, k))
        off += n * k
    return torch.cat(cols, 1)


def _rpn_case(seed, n, shapes, a, ratios):
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_std import cell_anchor_table
    g = torch.Generator().manual_seed(seed)
    lv = ops.make_rpn_levels(shapes, STRIDES, n, a)
    cell = cell_anchor_table(SIZES, ratios)
    anchors = torch.cat(O.anchor_grid(shapes, STRIDES, SIZES, ratios))  # (R, 4), one image
    R = anchors.shape[0]
    pi = _level_major_index(shapes, n, a)
    labels = torch.full((n, R), -1, dtype=torch.int8)
    # sampled anchors: every level's first and last pixel (all A anchors), the image's first and last anchor, and random ones
    edge, off = [], 0
    for h, w in shapes:
        edge += list(range(off, off + a)) + list(range(off + (h * w - 1) * a, off + h * w * a))
        off += h * w * a
    for i in range(n):
        pick = torch.unique(torch.cat([torch.tensor(edge), torch.randperm(R, generator=g)[:256 - len(edge)]]))[:256]
        npos = 0 if i == 5 else int(torch.randint(1, 99 if i == 0 else 129, (1,), generator=g))  # image 5: no positive
        perm = pick[torch.randperm(len(pick), generator=g)]
        labels[i, perm] = 0
        labels[i, perm[:npos]] = 1
        if i == 0:
            labels[i, edge] = 1  # (positives on every level's boundary pixels of image 0)
    ctr = 0.5 * (anchors[:, :2] + anchors[:, 2:])
    wh = (anchors[:, 2:] - anchors[:, :2]) * torch.exp(torch.randn(n, R, 2, generator=g) * 0.3)
    c = ctr + torch.randn(n, R, 2, generator=g) * 4.0
    matched = torch.cat([c - 0.5 * wh, c + 0.5 * wh], -1).contiguous()
    m = n * R
    logits = torch.randn(m, generator=g) * 3.0
    logits[torch.randperm(m, generator=g)[: m // 50]] = 100.0 * torch.sign(torch.randn(m // 50, generator=g))
    deltas = torch.randn(m, 4, generator=g) * 0.5
    return ops, lv, cell, anchors, pi, logits, deltas, labels, matched


def _rpn_reference(logits, deltas, labels, matched, anchors, pi, n, a, beta, batch=256):
    """fp64 losses over the sampled anchors and the (rows, 5A) gradient, scattered into zeros."""
    lab = labels.view(-1).long()
    idx = pi.view(-1)
    sel, pos = lab >= 0, lab == 1
    lg = logits[idx[sel]].double().requires_grad_(True)
    dl = deltas[idx[pos]].double().requires_grad_(True)
    anc = anchors.unsqueeze(0).expand(n, -1, -1).reshape(-1, 4)
    tgt = _get_deltas32(anc[pos], matched.view(-1, 4)[pos], (1.0, 1.0, 1.0, 1.0)).double()
    norm = batch * n
    l_cls = F.binary_cross_entropy_with_logits(lg, lab[sel].double(), reduction="sum") / norm
    l_loc = _smooth_l1(dl - tgt, beta).sum() / norm
    (l_cls + l_loc).backward()
    g_lg = torch.zeros(logits.numel())
    g_lg[idx[sel]] = lg.grad.float()
    g_dl = torch.zeros(logits.numel(), 4)
    g_dl[idx[pos]] = dl.grad.float()
    d = torch.cat([g_lg.view(-1, a), g_dl.view(-1, 4 * a)], 1)
    return l_cls.item(), l_loc.item(), int(pos.sum()), int((lab == 0).sum()), d


def _run_rpn(ops, lv, cell, n, t, beta):
    args = (lv, cell.to(DEV), n, *t, (1.0, 1.0, 1.0, 1.0), beta, 1.0, 1.0, 256)
    out = ops.std_rpn_losses_fwd(*args)
    d = ops.std_rpn_losses_bwd(*args, loss_scale=1.0)
    torch.cuda.synchronize()
    return out.cpu(), d.cpu()


def _check_rpn(seed, n, shapes, a, ratios, beta, poison):
    ops, lv, cell, anchors, pi, logits, deltas, labels, matched = _rpn_case(seed, n, shapes, a, ratios)
    t = [x.to(DEV).contiguous() for x in (logits, deltas, labels, matched)]
    out, d = _run_rpn(ops, lv, cell, n, t, beta)
    rc, rl, npos, nneg, dref = _rpn_reference(logits, deltas, labels, matched, anchors, pi, n, a, beta)
    assert out[0].item() == pytest.approx(rc, rel=1e-5) and out[1].item() == pytest.approx(rl, rel=1e-5)
    assert int(out[2]) == npos and int(out[3]) == nneg
    assert d.shape == dref.shape == (logits.numel() // a, 5 * a)
    assert torch.allclose(d, dref, rtol=1e-5, atol=1e-9)
    lab_lm = torch.empty(logits.numel(), dtype=torch.int8)
    lab_lm[pi.view(-1)] = labels.view(-1)
    assert (d[:, :a].reshape(-1)[lab_lm < 0] == 0).all()                       # unsampled: exactly 0
    assert (d[:, a:].reshape(-1, 4)[lab_lm != 1] == 0).all()                    # delta columns of non-positives: exactly 0
    out2, d2 = _run_rpn(ops, lv, cell, n, t, beta)
    assert torch.equal(out2, out) and torch.equal(d2, d)                        # bitwise repeatable
    if poison:
        # d2 indexes only the sampled anchors' logits and the positives' deltas and matched boxes: nothing else may reach the result
        g = torch.Generator().manual_seed(seed + 1)
        bad = torch.tensor([float("nan"), float("inf"), -float("inf")])
        unl, neg = lab_lm < 0, lab_lm == 0
        pl, pd, pm = logits.clone(), deltas.clone(), matched.clone()
        pl[unl] = bad[torch.randint(0, 3, (int(unl.sum()),), generator=g)]
        pd[unl | neg] = bad[torch.randint(0, 3, (int((unl | neg).sum()), 4), generator=g)]
        pm[labels != 1] = bad[torch.randint(0, 3, (int((labels != 1).sum()), 4), generator=g)]
        tp = [x.to(DEV).contiguous() for x in (pl, pd, labels, pm)]
        out3, d3 = _run_rpn(ops, lv, cell, n, tp, beta)
        assert torch.equal(out3, out) and torch.equal(d3, d)


@pytest.mark.gpu
def test_std_rpn_losses_production_pyramid(osr):
    """n = 16, 800 x 1344 padded, A = 3: 4.3 M anchors, <= 256 sampled and <= 128 positive per image, image 5 without a positive,
    sampled anchors on every level's first and last pixel; logits of +-100; NaN / Inf where d2 does not look (bit-identical)."""
    _check_rpn(1, 16, O.level_shapes(800, 1344), 3, (0.5, 1.0, 2.0), 0.0, poison=True)


@pytest.mark.gpu
@pytest.mark.parametrize("a,ratios", [(1, (1.0,)), (8, (0.25, 0.4, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0))], ids=["A1", "A8"])
@pytest.mark.parametrize("beta", [0.0, 0.1])
def test_std_rpn_losses_anchor_counts(osr, a, ratios, beta):
    """A = 1 and A = 8 on a small 5-level pyramid: the pi / A row arithmetic and d_rows of width 5 and 40."""
    _check_rpn(2 + a, 3, O.level_shapes(128, 192), a, ratios, beta, poison=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. [d2] FastRCNNOutputLayers.losses
# ------------------------------------------------------------------------------------------------------------------------------
def _roi_case(seed, m, k, agnostic):
    """Rows in 512-row image blocks as osr_roi_match_and_sample leaves them: foreground, background, then padding (class -1) at the
    end of every block. Image 1 is all background, image 2 all padding. Some rows tie the GT class's logit with the maximum."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(m, k + 1, generator=g) * 3.0
    deltas = torch.randn(m, 4 if agnostic else 4 * k, generator=g) * 0.3
    p = torch.rand(m, 2, generator=g) * 600.0
    prop = torch.cat([p, p + 8.0 + torch.rand(m, 2, generator=g) * 300.0], 1)
    gtb = prop + torch.randn(m, 4, generator=g) * 6.0
    gtb[:, 2:] = torch.maximum(gtb[:, 2:], gtb[:, :2] + 1.0)
    cls = torch.full((m,), -1, dtype=torch.int64)
    for b0 in range(0, m, 512):
        b1, img = min(b0 + 512, m), b0 // 512
        nrow = b1 - b0
        nvalid = 0 if img == 2 else int(torch.randint(nrow // 2, nrow + 1, (1,), generator=g))
        nfg = 0 if img == 1 else int(torch.randint(0, nvalid // 4 + 1, (1,), generator=g))
        cls[b0:b0 + nfg] = torch.randint(0, k, (nfg,), generator=g)
        cls[b0 + nfg:b0 + nvalid] = k
    valid = torch.nonzero(cls >= 0).view(-1)
    if len(valid) > 0 and k > 1:
        # ties: GT class with background, GT class with another class below / above it
        tie = valid[torch.randperm(len(valid), generator=g)[: max(1, len(valid) // 10)]]
        for j, r in enumerate(tie.tolist()):
            c = int(cls[r])
            other = [k, (c + 1) % (k + 1), (c - 1) % (k + 1)][j % 3]
            if other == c:
                continue
            top = float(logits[r].max()) + 1.0
            logits[r, c] = top
            logits[r, other] = top
    return logits, deltas, prop, gtb, cls


def _roi_reference(logits, deltas, prop, gtb, cls, k, agnostic, beta, box_w):
    lg = logits.double().requires_grad_(True)
    dl = deltas.double().requires_grad_(True)
    valid = cls >= 0
    nvalid = int(valid.sum())
    ce = F.cross_entropy(lg[valid], cls[valid], reduction="sum") / max(nvalid, 1)
    fg = valid & (cls < k)
    idx = torch.nonzero(fg).view(-1)
    tgt = _get_deltas32(prop[idx], gtb[idx], (10.0, 10.0, 5.0, 5.0)).double()
    sel = dl[idx] if agnostic else dl.view(-1, k, 4)[idx, cls[idx]]
    box = _smooth_l1(sel - tgt, beta).sum() / max(nvalid, 1) * box_w
    (ce + box).backward()
    pred = logits[valid].argmax(1)  # (first maximum)
    c = cls[valid]
    fgm = c < k
    stats = [nvalid, int((pred == c).sum()), int(fgm.sum()), int((pred[fgm] == c[fgm]).sum()), int((pred[fgm] == k).sum())]
    return ce.item(), box.item(), stats, lg.grad.float(), dl.grad.float()


def _run_roi(ops, t, k, agnostic, beta, box_w):
    out = ops.fastrcnn_losses_fwd(*t, k, agnostic, (10.0, 10.0, 5.0, 5.0), beta, 1.0, box_w)
    dlg, ddl = ops.fastrcnn_losses_bwd(*t, k, agnostic, (10.0, 10.0, 5.0, 5.0), beta, 1.0, box_w, loss_scale=1.0)
    torch.cuda.synchronize()
    return out.cpu(), dlg.cpu(), ddl.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("k,agnostic", [(80, False), (80, True), (1, False)], ids=["K80", "K80-agnostic", "K1"])
@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 8192, 65537])
def test_fastrcnn_losses_reduction_edges(osr, m, k, agnostic, beta):
    """m = 65537 exceeds the forward's 256 x 256 threads (grid-stride loop); 8192 = 16 images x 512 rows is production."""
    from openset_rcnn_amd.host import ops
    logits, deltas, prop, gtb, cls = _roi_case(m + k, m, k, agnostic)
    t = [x.to(DEV).contiguous() for x in (logits, deltas, prop, gtb, cls)]
    out, dlg, ddl = _run_roi(ops, t, k, agnostic, beta, 0.7)
    ce, box, stats, g_lg, g_dl = _roi_reference(logits, deltas, prop, gtb, cls, k, agnostic, beta, 0.7)
    assert out[0].item() == pytest.approx(ce, rel=1e-5, abs=1e-30) and out[1].item() == pytest.approx(box, rel=1e-5, abs=1e-30)
    assert [int(v) for v in out[2:7]] == stats
    # (the existing tolerance of test_std_train_losses: 1e-5 relative to the gradient's scale)
    assert torch.allclose(dlg, g_lg, rtol=1e-5, atol=1e-5 * float(g_lg.abs().max()))
    assert torch.allclose(ddl, g_dl, rtol=1e-5, atol=1e-5 * float(g_dl.abs().max()))
    pad = cls < 0
    assert (dlg[pad] == 0).all() and (ddl[pad] == 0).all()
    assert (ddl[cls == k] == 0).all()
    out2, dlg2, ddl2 = _run_roi(ops, t, k, agnostic, beta, 0.7)
    assert torch.equal(out2, out) and torch.equal(dlg2, dlg) and torch.equal(ddl2, ddl)
    # poison: NaN in the padding rows' logits and deltas and in every delta group of a foreground row but its GT class's
    pl, pd = logits.clone(), deltas.clone()
    pl[pad], pd[pad] = float("nan"), float("nan")
    if not agnostic:
        fg = torch.nonzero((cls >= 0) & (cls < k)).view(-1)
        keep = pd.view(-1, k, 4)[fg, cls[fg]].clone()
        pd.view(-1, k, 4)[fg] = float("nan")
        pd.view(-1, k, 4)[fg, cls[fg]] = keep
    tp = [x.to(DEV).contiguous() for x in (pl, pd, prop, gtb, cls)]
    out3, dlg3, ddl3 = _run_roi(ops, tp, k, agnostic, beta, 0.7)
    assert torch.equal(out3, out) and torch.equal(dlg3, dlg) and torch.equal(ddl3, ddl)


@pytest.mark.gpu
def test_fastrcnn_losses_empty_input(osr):
    """m = 0: d2's cross_entropy returns 0 for an empty input; every loss and statistic is 0 and the backward writes nothing."""
    from openset_rcnn_amd.host import ops
    k = 80
    t = [torch.empty(s, dtype=dt, device=DEV) for s, dt in (((0, k + 1), torch.float32), ((0, 4 * k), torch.float32), ((0, 4), torch.float32),
                                                            ((0, 4), torch.float32), ((0,), torch.int64))]
    out, dlg, ddl = _run_roi(ops, t, k, False, 0.0, 1.0)
    assert out.tolist() == [0.0] * 7 and dlg.shape == (0, k + 1) and ddl.shape == (0, 4 * k)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. StandardRPNHead tail backward
# ------------------------------------------------------------------------------------------------------------------------------
def _ulp(x, dtype):
    """Spacing of the output format at |x| (subnormals included)."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("width", [5, 10, 15, 20, 25, 30, 35, 40])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 4096, 5000])
def test_std_rpn_tail_bwd_elementwise(osr, rows, width, dtype):
    """dW / db within the bound of the fixed summation order, (rows_per_wave + 256) * 2^-24 * sum|terms|; dt within 1 ulp of the
    fp64 value rounded to the output type (d and W are short dyadic numbers, so the kernel's fp32 sum for dt is exact)."""
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(rows * 64 + width)
    t = torch.randn(rows, 256, generator=g)
    u = torch.rand(rows, 256, generator=g)
    t[u < 0.3] = -t[u < 0.3].abs()
    t[(u >= 0.3) & (u < 0.35)] = 0.0
    t[(u >= 0.35) & (u < 0.4)] = -0.0
    d = torch.randint(-64, 65, (rows, width), generator=g).float() / 64.0
    d[torch.rand(rows, generator=g) < 0.3] = 0.0  # (rows without a gradient, as the sparse list's tail)
    w = torch.randint(-128, 129, (width, 256), generator=g).float() / 1024.0
    dt, dw, db = ops.std_rpn_tail_bwd(t.to(DEV), w.to(DEV), d.to(DEV), dtype)
    torch.cuda.synchronize()
    dt, dw, db = dt.cpu(), dw.cpu(), db.cpu()
    t64, d64 = t.double(), d.double()
    rpw = math.ceil(rows / 256)
    bound = (rpw + 256) * 2.0 ** -24
    ref_dw, abs_dw = d64.t() @ t64, d64.abs().t() @ t64.abs()
    ref_db, abs_db = d64.sum(0), d64.abs().sum(0)
    assert ((dw.double() - ref_dw).abs() <= bound * abs_dw).all()
    assert ((db.double() - ref_db).abs() <= bound * abs_db).all()
    ref_dt = ((d64 @ w.double()) * (t64 > 0)).to(dtype)
    err = (dt.float() - ref_dt.float()).abs()
    assert (err <= _ulp(ref_dt.float(), dtype)).all()
    assert (dt[~(t > 0)].float() == 0).all()
    dt2, dw2, db2 = ops.std_rpn_tail_bwd(t.to(DEV), w.to(DEV), d.to(DEV), dtype)
    assert torch.equal(dt2.cpu(), dt) and torch.equal(dw2.cpu(), dw) and torch.equal(db2.cpu(), db)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. osr_rpn_sparse_rows_ex / osr_rpn_gather_cols_ex at full size
# ------------------------------------------------------------------------------------------------------------------------------
def _feat_bits(l, img, y, x, c):
    """A 16-bit pattern that changes with every coordinate: the test's features, restated on the CPU for the listed pixels."""
    h = (x * 73856093) ^ (y * 19349663) ^ (img * 83492791) ^ (l * 2654435761) ^ (c * 40503)
    return ((h ^ (h >> 16)) & 0x7BFF).to(torch.int16)  # (bit 10 clear: never an fp16 Inf / NaN)


@pytest.fixture(scope="module")
def full_pyramid():
    n, shapes = 16, O.level_shapes(800, 1344)
    feats = []
    for l, (h, w) in enumerate(shapes):
        f = torch.empty((n, h, w, 256), dtype=torch.int16, device=DEV)
        yy = torch.arange(h, device=DEV, dtype=torch.int64).view(h, 1, 1)
        xx = torch.arange(w, device=DEV, dtype=torch.int64).view(1, w, 1)
        cc = torch.arange(256, device=DEV, dtype=torch.int64).view(1, 1, 256)
        for i in range(n):
            f[i] = _feat_bits(l, i, yy, xx, cc)
        feats.append(f.view(torch.float16))
    return n, shapes, feats


def _decode(rid, shapes, n):
    off = 0
    for l, (h, w) in enumerate(shapes):
        if rid < off + n * h * w:
            loc = rid - off
            return l, loc // (h * w), (loc % (h * w)) // w, loc % w
        off += n * h * w
    raise AssertionError(rid)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 15, 40, 64])
def test_sparse_rows_and_gather_cols_ex_full_size(osr, full_pyramid, width):
    """The 1.43 M pixel rows of n = 16 at 800 x 1344. Listed rows sit on every (level, image)'s first and last pixel; some are
    nonzero only in their last column, one only by a NaN. Then a list that overflows (found > cap)."""
    from openset_rcnn_amd.host import ops
    n, shapes, feats = full_pyramid
    rows = sum(n * h * w for h, w in shapes)
    g = torch.Generator().manual_seed(width)
    pick = set(torch.randperm(rows, generator=g)[:3000].tolist())
    off = 0
    for h, w in shapes:
        for i in range(n):
            pick |= {off + i * h * w, off + (i + 1) * h * w - 1}
        off += n * h * w
    pick = torch.tensor(sorted(pick))
    d = torch.zeros(rows, width)
    d[pick] = torch.randn(len(pick), width, generator=g)
    if width > 1:
        d[pick, torch.randint(0, width, (len(pick),), generator=g)] = 0.0  # (some zeros inside listed rows)
    last = pick[torch.randperm(len(pick), generator=g)[:200]]
    d[last] = 0.0
    d[last, width - 1] = torch.rand(len(last), generator=g) + 0.5     # nonzero only in the last column
    d[pick[7]] = 0.0
    d[pick[7], width // 2] = float("nan")                             # nonzero only by a NaN
    want = np.nonzero((d.numpy() != 0).any(1))[0]
    assert len(want) == len(pick)
    dd = d.to(DEV)
    cap = len(want) + 37
    ids, rmap, cnt = ops.rpn_sparse_rows_ex(dd, cap)
    lv = ops.make_rpn_levels(shapes, STRIDES, n, 1)
    cols, dl = ops.rpn_gather_cols_ex(lv, feats, n, ids, dd)
    torch.cuda.synchronize()
    ids, rmap, cnt = ids.cpu(), rmap.cpu(), cnt.cpu()
    assert cnt.tolist() == [len(want), len(want)]
    assert np.array_equal(ids[: len(want)].numpy(), want) and (ids[len(want):] == -1).all()
    ref_map = torch.full((rows,), -1, dtype=torch.int32)
    ref_map[torch.from_numpy(want)] = torch.arange(len(want), dtype=torch.int32)
    assert torch.equal(rmap, ref_map)
    dl = dl.cpu()
    assert torch.equal(dl[: len(want)].view(torch.int32), d[torch.from_numpy(want)].view(torch.int32))
    assert (dl[len(want):] == 0).all()
    cols = cols.cpu().view(cap, 9, 256).view(torch.int16)
    assert (cols[len(want):] == 0).all()
    # im2col rows of the listed pixels on level / image boundaries and a sample of the others; taps outside the map are zero
    bset = set()
    off = 0
    for h, w in shapes:
        for i in range(n):
            bset |= {off + i * h * w, off + (i + 1) * h * w - 1}
        off += n * h * w
    check = [j for j, r in enumerate(want.tolist()) if r in bset] + list(range(0, len(want), 97))
    cc = torch.arange(256, dtype=torch.int64)
    for j in check:
        l, img, y, x = _decode(int(want[j]), shapes, n)
        h, w = shapes[l]
        for tap in range(9):
            yy, xx = y + tap // 3 - 1, x + tap % 3 - 1
            ref = _feat_bits(l, img, torch.tensor(yy), torch.tensor(xx), cc) if 0 <= yy < h and 0 <= xx < w else torch.zeros(256, dtype=torch.int16)
            assert torch.equal(cols[j, tap], ref), (j, tap)
    # an overflowing list: the first cap rows in ascending order, found counted in full, the rest unmapped
    small = len(want) // 3
    ids2, rmap2, cnt2 = ops.rpn_sparse_rows_ex(dd, small)
    torch.cuda.synchronize()
    assert cnt2.cpu().tolist() == [small, len(want)]
    assert np.array_equal(ids2.cpu().numpy(), want[:small])
    ref_map2 = ref_map.clone()
    ref_map2[ref_map2 >= small] = -1
    assert torch.equal(rmap2.cpu(), ref_map2)
