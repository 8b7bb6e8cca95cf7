"""The stock heads' loss kernels (csrc/osr_std_train.hip) against [d2] RPN.losses / FastRCNNOutputLayers.losses restated in plain
torch, with autograd for the gradients: forward values and gradients in fp32, padding rows, an image without GT, beta > 0,
class-agnostic and class-specific regression, logits of +-30, and bitwise repeatability."""
import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

DEV = "cuda:0"


def _smooth_l1(x, beta):
    if beta < 1e-5:
        return x.abs()
    n = x.abs()
    return torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)


def _rpn_case(seed, n=2, shapes=((8, 10), (4, 5)), strides=(4, 8), a=3, big_logits=False):
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.engine_std import cell_anchor_table
    g = torch.Generator().manual_seed(seed)
    lv = ops.make_rpn_levels(list(shapes), list(strides), n, a)
    cell = cell_anchor_table([32.0, 64.0][: len(shapes)], (0.5, 1.0, 2.0)[:a]).to(DEV)
    per = [h * w * a for h, w in shapes]
    rows = sum(n * p for p in per)
    logits = torch.randn(rows, generator=g) * (30.0 if big_logits else 2.0)
    if big_logits:
        logits = torch.where(torch.rand(rows, generator=g) < 0.5, torch.full_like(logits, 30.0), torch.full_like(logits, -30.0))
    deltas = torch.randn(rows, 4, generator=g) * 0.5
    R = sum(per)
    labels = torch.full((n, R), -1, dtype=torch.int8)
    u = torch.rand(n, R, generator=g)
    labels[u < 0.3] = 0
    labels[u < 0.08] = 1
    labels[1, :] = torch.where(labels[1] == 1, torch.zeros_like(labels[1]), labels[1])  # image 1: no GT -> no positive
    gt = torch.tensor([10.0, 12.0, 40.0, 35.0]) + torch.randn(n, R, 4, generator=g).abs() * torch.tensor([0.0, 0.0, 5.0, 5.0])
    return ops, lv, cell, n, shapes, strides, a, logits.to(DEV), deltas.to(DEV), labels.to(DEV), gt.contiguous().to(DEV)


def _image_major_to_level(x, n, shapes, a):
    """(n, R, ...) image-major anchors -> level-major (sum_l n*h*w*a, ...) as the head writes them."""
    out, off = [], 0
    for h, w in shapes:
        k = h * w * a
        out.append(x[:, off:off + k].reshape(n * k, *x.shape[2:]))
        off += k
    return torch.cat(out)


def _anchors(shapes, strides, a, cell):
    rows = []
    for l, ((h, w), s) in enumerate(zip(shapes, strides)):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32) * s, torch.arange(w, dtype=torch.float32) * s, indexing="ij")
        sh = torch.stack([xs, ys, xs, ys], -1).view(-1, 1, 4)
        rows.append((sh + cell[l].cpu().view(1, a, 4)).view(-1, 4))
    return torch.cat(rows)


def _rpn_reference(logits, deltas, labels, gt, n, shapes, strides, a, cell, beta, batch=256, cls_w=1.0, loc_w=1.0):
    lg = logits.detach().cpu().double().requires_grad_(True)
    dl = deltas.detach().cpu().double().requires_grad_(True)
    lab_l = _image_major_to_level(labels.cpu(), n, shapes, a).long()
    gt_l = _image_major_to_level(gt.cpu(), n, shapes, a).double()
    anc = _anchors(shapes, strides, a, cell)
    anc_l = _image_major_to_level(anc.unsqueeze(0).expand(n, -1, -1), n, shapes, a).double()
    tgt = O.b2b_get_deltas(anc_l, gt_l, (1.0, 1.0, 1.0, 1.0))
    pos, valid = lab_l == 1, lab_l >= 0
    norm = batch * n
    l_cls = F.binary_cross_entropy_with_logits(lg[valid], lab_l[valid].double(), reduction="sum") / norm * cls_w
    l_loc = _smooth_l1(dl[pos] - tgt[pos], beta).sum() / norm * loc_w
    (l_cls + l_loc).backward()
    return l_cls.item(), l_loc.item(), int(pos.sum()), int((lab_l == 0).sum()), lg.grad.float(), dl.grad.float()


@pytest.mark.gpu
@pytest.mark.parametrize("beta,big", [(0.0, False), (0.1, False), (0.0, True)], ids=["l1", "beta0.1", "logits30"])
def test_std_rpn_losses_forward_and_gradient(osr, beta, big):
    ops, lv, cell, n, shapes, strides, a, logits, deltas, labels, gt = _rpn_case(3, big_logits=big)
    out = ops.std_rpn_losses_fwd(lv, cell, n, logits, deltas, labels, gt, (1, 1, 1, 1), beta, 1.0, 1.0, 256)
    d = ops.std_rpn_losses_bwd(lv, cell, n, logits, deltas, labels, gt, (1, 1, 1, 1), beta, 1.0, 1.0, 256, loss_scale=8.0)
    torch.cuda.synchronize()
    rc, rl, npos, nneg, g_lg, g_dl = _rpn_reference(logits, deltas, labels, gt, n, shapes, strides, a, cell, beta)
    o = out.cpu()
    assert o[0].item() == pytest.approx(rc, rel=1e-5) and o[1].item() == pytest.approx(rl, rel=1e-5, abs=1e-7)
    assert int(o[2]) == npos and int(o[3]) == nneg and npos > 0
    d = d.cpu() / 8.0
    assert d.shape == (logits.numel() // a, 5 * a)
    assert torch.allclose(d[:, :a].reshape(-1), g_lg, rtol=1e-5, atol=1e-9)
    assert torch.allclose(d[:, a:].reshape(-1, 4), g_dl, rtol=1e-5, atol=1e-9)
    # only sampled anchors carry a gradient; the image without GT has no positive, so no delta gradient there
    lab_l = _image_major_to_level(labels.cpu(), n, shapes, a)
    assert (d[:, :a].reshape(-1)[lab_l.view(-1) < 0] == 0).all()
    # bitwise reproducible
    out2 = ops.std_rpn_losses_fwd(lv, cell, n, logits, deltas, labels, gt, (1, 1, 1, 1), beta, 1.0, 1.0, 256)
    d2 = ops.std_rpn_losses_bwd(lv, cell, n, logits, deltas, labels, gt, (1, 1, 1, 1), beta, 1.0, 1.0, 256, loss_scale=8.0)
    assert torch.equal(out2.cpu(), out.cpu()) and torch.equal(d2.cpu() / 8.0, d)


def _roi_case(seed, m=40, k=5, agnostic=True):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(m, k + 1, generator=g) * 3
    deltas = torch.randn(m, 4 if agnostic else 4 * k, generator=g) * 0.3
    p = torch.rand(m, 2, generator=g) * 50
    prop = torch.cat([p, p + 20 + torch.rand(m, 2, generator=g) * 30], 1)
    gtb = prop + torch.randn(m, 4, generator=g) * 3
    cls = torch.randint(0, k + 1, (m,), generator=g)
    cls[-7:] = -1  # padding rows
    cls[:3] = k    # background
    return logits, deltas, prop, gtb, cls


def _roi_reference(logits, deltas, prop, gtb, cls, k, agnostic, beta, box_w=1.0):
    lg = logits.double().requires_grad_(True)
    dl = deltas.double().requires_grad_(True)
    valid = cls >= 0
    ce = F.cross_entropy(lg[valid], cls[valid], reduction="mean")
    fg = valid & (cls < k)
    tgt = O.b2b_get_deltas(prop[fg].double(), gtb[fg].double(), (10.0, 10.0, 5.0, 5.0))
    idx = torch.nonzero(fg).view(-1)
    sel = dl[idx] if agnostic else dl.view(-1, k, 4)[idx, cls[idx]]
    box = _smooth_l1(sel - tgt, beta).sum() / max(int(valid.sum()), 1) * box_w
    (ce + box).backward()
    pred = logits[valid].argmax(1)
    c = cls[valid]
    fgm = c < k
    stats = [int(valid.sum()), int((pred == c).sum()), int(fgm.sum()), int((pred[fgm] == c[fgm]).sum()), int((pred[fgm] == k).sum())]
    return ce.item(), box.item(), stats, lg.grad.float(), dl.grad.float()


@pytest.mark.gpu
@pytest.mark.parametrize("agnostic", [True, False], ids=["agnostic", "class-specific"])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_fastrcnn_losses_forward_and_gradient(osr, agnostic, beta):
    from openset_rcnn_amd.host import ops
    k = 5
    logits, deltas, prop, gtb, cls = _roi_case(7, k=k, agnostic=agnostic)
    args = [t.to(DEV).contiguous() for t in (logits, deltas, prop, gtb, cls)]
    out = ops.fastrcnn_losses_fwd(*args, k, agnostic, (10.0, 10.0, 5.0, 5.0), beta, 1.0, 0.7)
    dlg, ddl = ops.fastrcnn_losses_bwd(*args, k, agnostic, (10.0, 10.0, 5.0, 5.0), beta, 1.0, 0.7, loss_scale=4.0)
    torch.cuda.synchronize()
    ce, box, stats, g_lg, g_dl = _roi_reference(logits, deltas, prop, gtb, cls, k, agnostic, beta, box_w=0.7)
    o = out.cpu()
    assert o[0].item() == pytest.approx(ce, rel=1e-5) and o[1].item() == pytest.approx(box, rel=1e-5)
    assert [int(v) for v in o[2:7]] == stats
    # (1e-5 relative to the gradient's scale: the kernel forms the regression targets in fp32, the reference in fp64)
    assert torch.allclose(dlg.cpu() / 4.0, g_lg, rtol=1e-5, atol=1e-5 * float(g_lg.abs().max()))
    assert torch.allclose(ddl.cpu() / 4.0, g_dl, rtol=1e-5, atol=1e-5 * float(g_dl.abs().max()))
    assert (dlg.cpu()[cls < 0] == 0).all() and (ddl.cpu()[cls < 0] == 0).all()
    out2 = ops.fastrcnn_losses_fwd(*args, k, agnostic, (10.0, 10.0, 5.0, 5.0), beta, 1.0, 0.7)
    dlg2, ddl2 = ops.fastrcnn_losses_bwd(*args, k, agnostic, (10.0, 10.0, 5.0, 5.0), beta, 1.0, 0.7, loss_scale=4.0)
    assert torch.equal(out2, out) and torch.equal(dlg2, dlg) and torch.equal(ddl2, ddl)
