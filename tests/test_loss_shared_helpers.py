"""The building blocks the loss kernels share (csrc/osr_loss_common.h, the Box2BoxTransform pair of csrc/osr_box_loss.h and
csrc/osr_boxes.h, the mask head's row rule of csrc/osr_mask_mfma.h) through every entry point that is built from them, at the smallest shapes at which they can
go wrong: less than a wave of rows, a ragged second wave group, one row in a second grid-stride turn, no counted row at all, two
pyramid levels with A = 1 and A = 3, a mask batch whose segments end early.

Per entry point: two runs on the same input are bit-identical (the fixed summation order the shared reduction carries for all of
them), and the loss values agree with a float64 restatement written here at the tolerance the entry point's own test uses
(tests/test_train_fwd.py: 1e-5, PLN 2e-5; tests/test_std_train_losses.py: 1e-5; tests/test_mask_train_kernels.py: 1e-4).
The error texts of the merged level-table checks still name their own entry point."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def _twice(fn):
    """fn() -> tensor or tuple of tensors, run twice: the first result on the CPU, after requiring the second to be bit-identical."""
    a, b = fn(), fn()
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "two runs on the same input must be bit-identical"
    return [x.cpu() for x in a]


# ------------------------------------------------------------------------------------------------------
# float64 restatements
# ------------------------------------------------------------------------------------------------------
def _get_deltas64(src, tgt, w):
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    return torch.stack([w[0] * (tx - sx) / sw, w[1] * (ty - sy) / sh, w[2] * torch.log(tw / sw), w[3] * torch.log(th / sh)], 1)


def _apply_deltas64(d, src, w):
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    clamp = torch.log(torch.tensor(1000.0 / 16, dtype=torch.float64))
    pw, ph = torch.exp(torch.minimum(d[:, 2] / w[2], clamp)) * sw, torch.exp(torch.minimum(d[:, 3] / w[3], clamp)) * sh
    px, py = d[:, 0] / w[0] * sw + sx, d[:, 1] / w[1] * sh + sy
    return torch.stack([px - 0.5 * pw, py - 0.5 * ph, px + 0.5 * pw, py + 0.5 * ph], 1)


def _iou_loss64(p, g):
    """1 - clamp(diag(pairwise_iou(p, g)), min=1e-6): inter / union where inter > 0, else 0."""
    iw = (torch.minimum(p[:, 2], g[:, 2]) - torch.maximum(p[:, 0], g[:, 0])).clamp(min=0)
    ih = (torch.minimum(p[:, 3], g[:, 3]) - torch.maximum(p[:, 1], g[:, 1])).clamp(min=0)
    inter = iw * ih
    union = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter
    iou = torch.where(inter > 0, inter / union, torch.zeros_like(inter))
    return 1.0 - iou.clamp(min=1e-6)


# ------------------------------------------------------------------------------------------------------
# anchor lists: n = 2, levels of 5 x 7 and 3 x 4 cells, strides 4 and 8
# ------------------------------------------------------------------------------------------------------
N, SHAPES, STRIDES = 2, [(5, 7), (3, 4)], (4, 8)


def _anchor_case(ops, a, seed):
    """Level table, cell anchors, the image-major anchor list, labels from {-1, 0, 1} with no positive on the second level, and
    matched boxes that overlap their anchor."""
    g = torch.Generator().manual_seed(seed)
    lv = ops.make_rpn_levels(SHAPES, list(STRIDES), N, a)
    half = torch.tensor([[[8.0 * (l + 1) * (1 + 0.5 * k), 8.0 * (l + 1) / (1 + 0.5 * k)] for k in range(a)] for l in range(len(SHAPES))])
    cell = torch.cat((-half, half), dim=2).contiguous()  # (levels, a, 4)
    anchors = []
    for l, ((h, w), s) in enumerate(zip(SHAPES, STRIDES)):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) * s, torch.arange(w, dtype=torch.float32) * s, indexing="ij")
        anchors.append((torch.stack([xs, ys, xs, ys], -1).view(-1, 1, 4) + cell[l].view(1, a, 4)).view(-1, 4))
    anchors = torch.cat(anchors)
    r, r0 = anchors.shape[0], SHAPES[0][0] * SHAPES[0][1] * a
    labels = torch.randint(-1, 2, (N, r), generator=g).to(torch.int8)
    labels[:, r0:][labels[:, r0:] == 1] = 0  # the second level holds no positive anchor
    assert int((labels[:, :r0] == 1).sum()) > 0
    gt = anchors.unsqueeze(0) + torch.randn(N, r, 4, generator=g)  # (the narrowest anchor is 8 wide: the matched box keeps a positive size)
    return dict(lv=lv, cell=cell.to(DEV), anchors=anchors, labels=labels, gt=gt.contiguous(), a=a, r=r, g=g)


def _level_major(x, a):
    """(N, R, ...) image-major -> the level-major order of the prediction buffers."""
    out, off = [], 0
    for h, w in SHAPES:
        k = h * w * a
        out.append(x[:, off:off + k].reshape(N * k, *x.shape[2:]))
        off += k
    return torch.cat(out)


def test_cf_rpn_losses_a1(ops):
    c = _anchor_case(ops, 1, 5)
    g, r = c["g"], c["r"]
    pd, pc = torch.randn(N, r, 4, generator=g) * 0.8, torch.rand(N, r, generator=g)  # image-major here, level-major for the kernel
    lo = torch.randint(-1, 2, (N, r), generator=g).to(torch.int8)
    ct = torch.rand(N, r, generator=g)
    args = (c["lv"], c["cell"], N, _level_major(pd, 1).to(DEV), _level_major(pc, 1).to(DEV), c["labels"].to(DEV), lo.to(DEV), c["gt"].to(DEV), ct.to(DEV))
    out, = _twice(lambda: ops.rpn_losses_fwd(*args, loc_weight=0.5, ctr_weight=0.5, batch_size_per_image=256))
    _twice(lambda: ops.rpn_losses_bwd(*args, loc_weight=0.5, ctr_weight=0.5, batch_size_per_image=256, loss_scale=8.0))
    # "iou" loss of the decoded box (ReLU of the ltrb deltas, scaled by the anchor's size) + L1 centerness, both / (256 n)
    an = c["anchors"].double().unsqueeze(0).expand(N, -1, -1).reshape(-1, 4)
    d, lr, gt = pd.double().view(-1, 4).clamp(min=0), c["labels"].view(-1), c["gt"].double().view(-1, 4)
    cx, cy, aw, ah = 0.5 * (an[:, 0] + an[:, 2]), 0.5 * (an[:, 1] + an[:, 3]), an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    pb = torch.stack([cx - d[:, 0] * aw, cy - d[:, 1] * ah, cx + d[:, 2] * aw, cy + d[:, 3] * ah], 1)
    pos, obj = lr == 1, lo.view(-1) != -1
    loc = float(_iou_loss64(pb[pos], gt[pos]).sum()) / (256 * N) * 0.5
    ctr = float((pc.double().view(-1) - ct.double().view(-1))[obj].abs().sum()) / (256 * N) * 0.5
    print(f"cf-rpn: loc {float(out[0]):.8f} (float64 {loc:.8f}) ctr {float(out[1]):.8f} (float64 {ctr:.8f})")
    assert float(out[0]) == pytest.approx(loc, rel=1e-5, abs=1e-7) and float(out[1]) == pytest.approx(ctr, rel=1e-5, abs=1e-7)
    assert [int(v) for v in out[2:]] == [int(pos.sum()), int((lr == 0).sum()), int((lo == 1).sum()), int((lo == 0).sum())]


def test_stock_rpn_losses_a3(ops):
    a = 3
    c = _anchor_case(ops, a, 6)
    g, r = c["g"], c["r"]
    lg, dl = torch.randn(N, r, generator=g) * 2.0, torch.randn(N, r, 4, generator=g) * 0.5
    bw = (1.0, 1.0, 1.0, 1.0)
    args = (c["lv"], c["cell"], N, _level_major(lg, a).to(DEV), _level_major(dl, a).to(DEV), c["labels"].to(DEV), c["gt"].to(DEV), bw, 0.0, 1.0, 1.0, 256)
    out, = _twice(lambda: ops.std_rpn_losses_fwd(*args))
    d, = _twice(lambda: ops.std_rpn_losses_bwd(*args, loss_scale=8.0))
    assert d.shape == (r * N // a, 5 * a)
    lab = c["labels"].view(-1)
    an = c["anchors"].double().unsqueeze(0).expand(N, -1, -1).reshape(-1, 4)
    pos, valid = lab == 1, lab >= 0
    cls = float(F.binary_cross_entropy_with_logits(lg.double().view(-1)[valid], lab[valid].double(), reduction="sum")) / (256 * N)
    tgt = _get_deltas64(an[pos], c["gt"].double().view(-1, 4)[pos], bw)
    loc = float((dl.double().view(-1, 4)[pos] - tgt).abs().sum()) / (256 * N)
    print(f"stock rpn: cls {float(out[0]):.8f} (float64 {cls:.8f}) loc {float(out[1]):.8f} (float64 {loc:.8f})")
    assert float(out[0]) == pytest.approx(cls, rel=1e-5) and float(out[1]) == pytest.approx(loc, rel=1e-5, abs=1e-7)
    assert int(out[2]) == int(pos.sum()) and int(out[3]) == int((lab == 0).sum())
    # the in-level idx % A / idx / A split: anchor (pixel row p, a) of the level-major list writes columns a and A + 4a .. of row p
    lab_l = _level_major(c["labels"], a).view(-1, a)
    assert bool((d[:, :a][lab_l < 0] == 0).all()) and bool((d[:, :a][lab_l >= 0] != 0).all())
    assert bool((d[:, a:].view(-1, a, 4)[lab_l != 1] == 0).all())


# ------------------------------------------------------------------------------------------------------
# row lists
# ------------------------------------------------------------------------------------------------------
K, NC = 3, 7  # known classes (PLN, CE), foreground classes of the RoI heads: ids 0..NC-1 foreground, NC background, -1 padding
ROWS = [(1, False), (257, False), (65537, False), (257, True)]
ROW_IDS = ["m1", "m257", "m65537", "none-counted"]


def _row_case(m, none_counted, seed=17):
    """Class ids mixing padding (-1), foreground (known: < K; unknown to PLN / CE: K .. NC-1) and background (NC); boxes; IoUs."""
    g = torch.Generator().manual_seed(seed + m)
    cls = torch.randint(-1, NC + 1, (m,), generator=g)
    if m == 1:
        cls[0] = 1
    if none_counted:
        cls[:] = -1
    p = torch.rand(m, 2, generator=g) * 200
    prop = torch.cat([p, p + 8 + torch.rand(m, 2, generator=g) * 100], 1)
    gtb = prop + torch.randn(m, 4, generator=g) * 3
    gtb[:, 2:] = torch.max(gtb[:, 2:], gtb[:, :2] + 2)  # (a matched box keeps a positive size: its logarithm is a regression target)
    return g, cls, prop.contiguous(), gtb.contiguous(), torch.rand(m, generator=g)


@pytest.mark.parametrize("m,none_counted", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("box_loss", ["smooth_l1", "iou"])
def test_roi_box_iou_losses(ops, m, none_counted, box_loss):
    g, cls, prop, gtb, gi = _row_case(m, none_counted)
    pred5 = torch.cat((torch.randn(m, 4, generator=g) * 0.5, torch.randn(m, 1, generator=g)), 1).contiguous()  # 4 deltas, the IoU logit
    rw = (10.0, 10.0, 5.0, 5.0)
    t = [x.to(DEV) for x in (pred5, prop, gtb, cls, gi)]
    out, = _twice(lambda: ops.roi_box_losses_fwd(t[0][:, :4], t[0][:, 4], t[1], t[2], t[3], t[4], NC, rw, 0.5, 0.5, iou_is_logit=True, box_loss=(box_loss, 0.0)))
    _twice(lambda: ops.roi_box_losses_bwd(*t, NC, rw, 0.5, 0.5, loss_scale=4.0, box_loss=(box_loss, 0.0)))
    rows, fg = int((cls >= 0).sum()), (cls >= 0) & (cls < NC)
    d, s, tg = pred5[fg, :4].double(), prop[fg].double(), gtb[fg].double()
    per = (d - _get_deltas64(s, tg, rw)).abs().sum() if box_loss == "smooth_l1" else _iou_loss64(_apply_deltas64(d, s, rw), tg).sum()
    box = float(per) * 0.5 / max(rows, 1)
    iou = float((torch.sigmoid(pred5[fg, 4].double()) - gi[fg].double()).abs().sum()) * 0.5 / max(rows, 1)
    print(f"roi box m={m} {box_loss}: box {float(out[0]):.8f} (float64 {box:.8f}) iou {float(out[1]):.8f} (float64 {iou:.8f}) rows {int(out[2])}")
    assert float(out[0]) == pytest.approx(box, rel=1e-5) and float(out[1]) == pytest.approx(iou, rel=1e-5)
    assert int(out[2]) == rows and (rows > 0) != none_counted


@pytest.mark.parametrize("m,none_counted", ROWS, ids=ROW_IDS)
def test_fastrcnn_losses(ops, m, none_counted):
    g, cls, prop, gtb, _ = _row_case(m, none_counted)
    logits, deltas = torch.randn(m, NC + 1, generator=g) * 3, torch.randn(m, 4 * NC, generator=g) * 0.3  # class-specific regression
    rw = (10.0, 10.0, 5.0, 5.0)
    t = [x.to(DEV).contiguous() for x in (logits, deltas, prop, gtb, cls)]
    out, = _twice(lambda: ops.fastrcnn_losses_fwd(*t, NC, False, rw, 0.0, 1.0, 0.7))
    _twice(lambda: ops.fastrcnn_losses_bwd(*t, NC, False, rw, 0.0, 1.0, 0.7, loss_scale=4.0))
    valid, fg = cls >= 0, (cls >= 0) & (cls < NC)
    rows = int(valid.sum())
    ce = float(F.cross_entropy(logits[valid].double(), cls[valid], reduction="sum")) / max(rows, 1)
    sel = deltas.double().view(m, NC, 4)[fg, cls[fg]]
    box = float((sel - _get_deltas64(prop[fg].double(), gtb[fg].double(), rw)).abs().sum()) * 0.7 / max(rows, 1)
    pred = logits[valid].argmax(1)
    cv = cls[valid]
    stats = [rows, int((pred == cv).sum()), int(fg.sum()), int((pred == cv)[cv < NC].sum()), int((pred[cv < NC] == NC).sum())]
    print(f"fast r-cnn m={m}: cls {float(out[0]):.8f} (float64 {ce:.8f}) box {float(out[1]):.8f} (float64 {box:.8f})")
    assert float(out[0]) == pytest.approx(ce, rel=1e-5) and float(out[1]) == pytest.approx(box, rel=1e-5)
    assert [int(v) for v in out[2:7]] == stats


@pytest.mark.parametrize("m,none_counted", ROWS, ids=ROW_IDS)
def test_softmax_ce_loss(ops, m, none_counted):
    g, cls, _, _, _ = _row_case(m, none_counted)
    cls = cls.clamp(min=0) if not none_counted else torch.full((m,), K + 1, dtype=torch.int64)  # K .. NC-1: ids that map to "ignored"
    logits = torch.randn(m, K + 1, generator=g) * 3
    t = (logits.to(DEV), cls.to(DEV))
    out, = _twice(lambda: ops.softmax_ce_loss_fwd(*t, NC, 0.9))
    d, = _twice(lambda: ops.softmax_ce_loss_bwd(*t, NC, 0.9, loss_scale=4.0))
    tgt = torch.where(cls < K, cls, torch.where(cls == NC, torch.full_like(cls, K), torch.full_like(cls, -1)))
    ok = tgt >= 0
    want = 0.9 * float(F.cross_entropy(logits[ok].double(), tgt[ok], reduction="mean")) if int(ok.sum()) else 0.0
    print(f"softmax ce m={m}: {float(out[0]):.8f} (float64 {want:.8f}), {int(ok.sum())} rows with a target")
    assert float(out[0]) == pytest.approx(want, rel=1e-5)
    assert bool((d[~ok] == 0).all()) and (int(ok.sum()) > 0) != none_counted


@pytest.mark.parametrize("m,none_counted", ROWS, ids=ROW_IDS)
def test_pln_loss(ops, m, none_counted):
    g, cls, _, _, gi = _row_case(m, none_counted)
    d, alpha, beta = 8, 0.3, 1.1
    protos = torch.randn(K, d, generator=g)
    emb = torch.randn(m, d, generator=g) + 0.8 * protos[cls.clamp(0, K - 1)]
    t = (emb.to(DEV), cls.to(DEV), gi.to(DEV))
    out, = _twice(lambda: ops.pln_loss_fwd(t[0], F.normalize(protos).to(DEV), t[1], t[2], 0.5, alpha, beta, 1.0))
    _twice(lambda: ops.pln_loss_bwd(t[0], protos.to(DEV), t[1], t[2], 0.5, alpha, beta, 1.0, loss_scale=4.0))
    # COS distance 1 - e.p between normalised vectors; a foreground row (known class, IoU above 0.5) pays relu(own - alpha) +
    # relu(beta - nearest other); every prototype pays relu(beta + alpha - nearest other prototype); / max(rows with class >= 0, 1)
    p64 = F.normalize(protos.double())
    fg = (cls >= 0) & (cls < K) & (gi > 0.5)
    dist = 1.0 - F.normalize(emb[fg].double()) @ p64.t()
    own = F.one_hot(cls[fg], K).bool()
    terms = (dist[own] - alpha).clamp(min=0).sum() + (beta - dist.masked_fill(own, 1000.0).min(dim=1)[0]).clamp(min=0).sum()
    pp = (1.0 - p64 @ p64.t()).masked_fill(torch.eye(K, dtype=torch.bool), 1000.0)
    want = float(terms + (beta + alpha - pp.min(dim=1)[0]).clamp(min=0).sum()) / max(int((cls >= 0).sum()), 1)
    print(f"pln m={m}: {float(out[0]):.8f} (float64 {want:.8f}), {int(fg.sum())} foreground rows")
    assert want > 0 and float(out[0]) == pytest.approx(want, rel=2e-5)


# ------------------------------------------------------------------------------------------------------
# mask loss: 3 rows of 4 x 4, segments of 2 rows of which 1 and 0 exist, 2 predictor rows
# ------------------------------------------------------------------------------------------------------
def test_mask_loss_segments_and_classes(ops):
    g = torch.Generator().manual_seed(23)
    logits = (torch.rand(3, 4, 4, generator=g) * 2 - 1) * 6.0
    targets = (torch.rand(3, 4, 4, generator=g) < 0.4).to(torch.uint8)
    classes = torch.tensor([1, 0, 1], dtype=torch.int64)
    rv = torch.tensor([1, 0], dtype=torch.int32)
    t = (logits.to(DEV), targets.to(DEV), 2, classes.to(DEV), rv.to(DEV), 2)
    out, = _twice(lambda: ops.mask_loss_fwd(*t, loss_weight=1.0))
    d, = _twice(lambda: ops.mask_loss_bwd(*t, scale=16.0))
    x, y = logits[0].double(), targets[0].double()  # row 0 is the only row that exists
    want = float(F.binary_cross_entropy_with_logits(x, y, reduction="mean"))
    wrong = (x > 0) != (y > 0.5)
    counts = [1.0, float(wrong.sum()), float(y.sum()), float((wrong & (y < 0.5)).sum()), float((wrong & (y > 0.5)).sum())]
    print(f"mask loss: {float(out[0]):.8f} (float64 {want:.8f})")
    assert abs(float(out[0]) - want) <= 1e-4 * abs(want)
    assert out[1:].tolist() == counts
    assert bool((d[0] != 0).all()) and float(d[1:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------
# the merged level-table checks keep each entry point's own words
# ------------------------------------------------------------------------------------------------------
def _level_calls(ops, a):
    """name -> call(lv) for the entry points that fill the shared level table, on valid tensors of the small anchor case."""
    c = _anchor_case(ops, a, 9)
    r = c["r"]
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    lab, box, cell = c["labels"].to(DEV), c["gt"].to(DEV), c["cell"]
    gt, cnt = z(N, 2, 4), torch.ones(N, dtype=torch.int32, device=DEV)
    cf = (z(N * r, 4), z(N * r), lab, lab, box, z(N, r))
    std = (z(N * r), z(N * r, 4), lab, box)
    return {
        "osr_rpn_match_anchors": lambda lv: ops.rpn_match_anchors(lv, cell, N, gt, cnt),
        "osr_rpn_anchor_targets": lambda lv: ops.rpn_anchor_targets(lv, cell, N, gt, cnt, z(N, r, dt=torch.int32), lab),
        "osr_rpn_losses_fwd": lambda lv: ops.rpn_losses_fwd(lv, cell, N, *cf),
        "osr_rpn_losses_bwd": lambda lv: ops.rpn_losses_bwd(lv, cell, N, *cf),
        "osr_std_rpn_losses_fwd": lambda lv: ops.std_rpn_losses_fwd(lv, cell, N, *std),
        "osr_std_rpn_losses_bwd": lambda lv: ops.std_rpn_losses_bwd(lv, cell, N, *std),
    }, c["lv"]


STOCK_TEXT = r"bad level table \(1 <= A <= 8, offsets in whole pixels\)"


def test_bad_level_table_names_its_entry_point(osr, ops):
    calls, _ = _level_calls(ops, 1)
    bad = ops.make_rpn_levels([], [], N, 1)  # num_levels = 0
    for name, call in calls.items():
        text = STOCK_TEXT if "std" in name else "bad level table"
        with pytest.raises(osr.OsrError, match=f"{name}: {text}"):
            call(bad)
    stock = {k: v for k, v in _level_calls(ops, 3)[0].items() if "std" in k}
    nine = ops.make_rpn_levels(SHAPES, list(STRIDES), N, 9)
    ragged = ops.make_rpn_levels(SHAPES, list(STRIDES), N, 3)
    ragged.offset[1] += 1  # not a whole pixel row of 3 anchors
    for name, call in stock.items():
        for lvl in (nine, ragged):
            with pytest.raises(osr.OsrError, match=f"{name}: {STOCK_TEXT}"):
                call(lvl)
