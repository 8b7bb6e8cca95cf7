"""Sparse backward of the stock RPN head for A = 3 anchors per pixel: the (rows, 15) loss gradient listed by osr_rpn_sparse_rows_ex,
the im2col rows gathered by osr_rpn_gather_cols_ex, the recomputed hidden state, osr_std_rpn_tail_bwd for the two 1x1 convs, the
3x3 conv's weight gradient and per-tap data gradient scattered back (the trainer's sequence) -- against dense torch autograd of
[d2] StandardRPNHead on the same gradient. The _ex entry points with width 5 match the original ones bit for bit."""
import pytest
import torch

from oracle import osr_oracle as O

DEV = "cuda:0"


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm()))


@pytest.mark.gpu
def test_sparse_std_rpn_head_backward_matches_dense_autograd(osr):
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(11)
    n, a, shapes = 2, 3, [(12, 16), (6, 8)]
    feats32 = [torch.randn(n, h, w, 256, generator=g) for h, w in shapes]
    feats = [f.half().to(DEV) for f in feats32]
    w3 = torch.randn(256, 3, 3, 256, generator=g) * 0.02
    b3 = torch.randn(256, generator=g) * 0.1
    wt = torch.randn(5 * a, 256, generator=g) * 0.05
    rows = sum(n * h * w for h, w in shapes)
    d = torch.zeros(rows, 5 * a)
    pick = torch.randperm(rows, generator=g)[:60]
    d[pick] = torch.randn(60, 5 * a, generator=g)
    d[pick[:20], a:] = 0.0  # negatives: logit gradient only
    # --- HIP sequence (train_std.StandardRCNNTrainer._backward) ---
    cap = 128
    plv = ops.make_rpn_levels(shapes, [4, 8], n, 1)
    ids, rmap, cnt = ops.rpn_sparse_rows_ex(d.to(DEV), cap)
    cols, d_rows = ops.rpn_gather_cols_ex(plv, feats, n, ids, d.to(DEV))
    w3d = w3.half().to(DEV).contiguous()
    t_rows = ops.linear(cols, w3d.view(256, -1), b3.to(DEV), relu=True, out_dtype=torch.float32)
    dt_rows, dw_t, db_t = ops.std_rpn_tail_bwd(t_rows, wt.to(DEV).contiguous(), d_rows, torch.float16)
    dw3 = ops.conv2d_wgrad(cols.view(1, cap, 1, -1), dt_rows.view(1, cap, 1, 256), 1, 1).view(256, 3, 3, 256)
    db3 = ops.bias_grad(dt_rows)
    y = ops.linear(dt_rows, w3d.view(256, -1).t().contiguous(), ops._zero_bias(9 * 256, DEV), out_dtype=torch.float32)
    glist = [torch.zeros_like(f) for f in feats]
    ops.rpn_scatter_cols_add_(plv, n, rmap, y, glist)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [60, 60]
    # --- dense autograd: the head on the fp16-rounded features, its five-group outputs dotted with the same gradient ---
    p = {"proposal_generator.rpn_head.conv.weight": w3.half().float().permute(0, 3, 1, 2).clone().requires_grad_(True),
         "proposal_generator.rpn_head.conv.bias": b3.clone().requires_grad_(True),
         "proposal_generator.rpn_head.objectness_logits.weight": wt[:a].view(a, 256, 1, 1).clone().requires_grad_(True),
         "proposal_generator.rpn_head.objectness_logits.bias": torch.zeros(a, requires_grad=True),
         "proposal_generator.rpn_head.anchor_deltas.weight": wt[a:].view(4 * a, 256, 1, 1).clone().requires_grad_(True),
         "proposal_generator.rpn_head.anchor_deltas.bias": torch.zeros(4 * a, requires_grad=True)}
    xs = [f.half().float().permute(0, 3, 1, 2).clone().requires_grad_(True) for f in feats32]
    total, off = 0.0, 0
    for x, (h, w) in zip(xs, shapes):
        dl, lg = O.standard_rpn_head(x, p)
        r = n * h * w
        dd = d[off:off + r].view(n, h, w, 5 * a)
        total = total + (lg.permute(0, 2, 3, 1) * dd[..., :a]).sum() + (dl.permute(0, 2, 3, 1) * dd[..., a:]).sum()
        off += r
    total.backward()
    ref_dwt = torch.cat([p["proposal_generator.rpn_head.objectness_logits.weight"].grad.view(a, 256),
                         p["proposal_generator.rpn_head.anchor_deltas.weight"].grad.view(4 * a, 256)])
    ref_dbt = torch.cat([p["proposal_generator.rpn_head.objectness_logits.bias"].grad, p["proposal_generator.rpn_head.anchor_deltas.bias"].grad])
    checks = [(dw_t.cpu(), ref_dwt), (db_t.cpu(), ref_dbt), (dw3.cpu().float(), p["proposal_generator.rpn_head.conv.weight"].grad.permute(0, 2, 3, 1)),
              (db3.cpu(), p["proposal_generator.rpn_head.conv.bias"].grad)]
    checks += [(gl.cpu().float(), x.grad.permute(0, 2, 3, 1)) for gl, x in zip(glist, xs)]
    for got, ref in checks:
        assert _cos(got, ref) >= 0.999, (_cos(got, ref))
        assert abs(float(got.norm() / ref.norm()) - 1.0) < 0.01


@pytest.mark.gpu
def test_ex_entry_points_with_width_5_equal_the_originals(osr):
    from openset_rcnn_amd.host import ops
    g = torch.Generator().manual_seed(2)
    n, shapes = 1, [(8, 8), (4, 4)]
    feats = [torch.randn(n, h, w, 256, generator=g).half().to(DEV) for h, w in shapes]
    rows = sum(h * w for h, w in shapes)
    d = torch.zeros(rows, 5)
    d[torch.randperm(rows, generator=g)[:30]] = torch.randn(30, 5, generator=g)
    d = d.to(DEV)
    lv = ops.make_rpn_levels(shapes, [4, 8], n, 1)
    a1, a2 = ops.rpn_sparse_rows(d, 20), ops.rpn_sparse_rows_ex(d, 20)  # (a list that overflows: 30 rows found, 20 listed)
    assert all(torch.equal(x, y) for x, y in zip(a1, a2)) and a1[2].cpu().tolist() == [20, 30]
    c1, c2 = ops.rpn_gather_cols(lv, feats, n, a1[0], d), ops.rpn_gather_cols_ex(lv, feats, n, a1[0], d)
    assert torch.equal(c1[0], c2[0]) and torch.equal(c1[1], c2[1])
