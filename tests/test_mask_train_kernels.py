"""The training-side kernels of the mask branch (csrc/osr_mask_train.hip, the per-sample scatter of csrc/osr_roi_align.hip and
osr_roi_match_and_sample_ex), each against a reference written here or taken from the oracle:

  osr_mask_targets        float64 torchvision loop (BitMasks.crop_and_resize = roi_align(bitmask, box, M, aligned) >= 0.5); a pixel may
                          differ only where the float64 average lies within 1e-5 of the threshold (fp32 evaluation)
  osr_mask_loss_fwd/_bwd  float64 binary_cross_entropy_with_logits (mean) and its autograd gradient, 1e-4 relative (the fp32 contract);
                          the counts behind the three mask_rcnn/* scalars exactly
  osr_roi_align_bwd       at pooled 14 and 8: autograd of the oracle's differentiable RoIAlign, 1e-4 relative
  osr_roi_match_and_sample_ex   the matched ground-truth index of the oracle's matcher; every other output bit-identical to the
                          entry point without it"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M = 28


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


# ------------------------------------------------------------------------------------------------------
# osr_mask_targets
# ------------------------------------------------------------------------------------------------------
def _axis64(start, size, bins, grid, extent):
    """One axis of torchvision's pre_calc_for_bilinear_interpolate in float64: per (bin, sample) validity, low / high index and the
    two weights."""
    bsz = size / bins
    v = start + np.arange(bins)[:, None] * bsz + (np.arange(grid)[None, :] + 0.5) * bsz / max(grid, 1)
    ok = ~((v < -1.0) | (v > extent))
    v = np.maximum(v, 0.0)
    lo = v.astype(np.int64)
    edge = lo >= extent - 1
    lo = np.where(edge, extent - 1, lo)
    hi = np.where(edge, extent - 1, lo + 1)
    v = np.where(edge, lo.astype(np.float64), v)
    w_hi = v - lo
    return ok, lo, hi, 1.0 - w_hi, w_hi


def roi_align_plane64(plane: np.ndarray, box, m: int) -> np.ndarray:
    """roi_align(plane, box, m x m, spatial_scale 1, sampling_ratio 0, aligned=True) in float64: (m, m) bin averages. The grid is
    ceil(roi / m) as the fp32 kernels compute it (from the fp32 box)."""
    f32 = np.float32
    h, w = plane.shape
    sw32, sh32 = f32(box[0]) - f32(0.5), f32(box[1]) - f32(0.5)
    rw32, rh32 = f32(f32(box[2]) - f32(0.5)) - sw32, f32(f32(box[3]) - f32(0.5)) - sh32
    gh, gw = int(math.ceil(float(rh32) / m)), int(math.ceil(float(rw32) / m))
    sw, sh = float(box[0]) - 0.5, float(box[1]) - 0.5
    rw, rh = float(box[2]) - float(box[0]), float(box[3]) - float(box[1])
    if gh <= 0 or gw <= 0:
        return np.zeros((m, m))
    oky, yl, yh, wyl, wyh = _axis64(sh, rh, m, gh, h)
    okx, xl, xh, wxl, wxh = _axis64(sw, rw, m, gw, w)
    p = plane.astype(np.float64)
    # rows: (m, gh) x columns (m, gw) -> (m, gh, m, gw)
    top = p[yl[:, :, None, None], xl[None, None]] * wxl[None, None] + p[yl[:, :, None, None], xh[None, None]] * wxh[None, None]
    bot = p[yh[:, :, None, None], xl[None, None]] * wxl[None, None] + p[yh[:, :, None, None], xh[None, None]] * wxh[None, None]
    val = (top * wyl[:, :, None, None] + bot * wyh[:, :, None, None]) * (oky[:, :, None, None] & okx[None, None])
    return val.sum(axis=(1, 3)) / max(gh * gw, 1)


@functools.lru_cache(maxsize=None)
def _targets_case():
    """2 images with 48 x 64 planes, gmax 3, F 4, rows_valid [3, 0]: a rectangle, a disc and a checkerboard; seeded non-integer boxes
    of which one hangs over the image edge, one is under a pixel wide (grid 1) and one is wider than 56 px (grid >= 3)."""
    n, gmax, h, w, f = 2, 3, 48, 64, 4
    yy, xx = np.mgrid[0:h, 0:w]
    planes = np.zeros((n, gmax, h, w), dtype=np.uint8)
    planes[0, 0, 10:35, 12:50] = 1
    planes[0, 1] = ((yy - 24.0) ** 2 + (xx - 30.0) ** 2 <= 15.0 ** 2)
    planes[0, 2] = ((yy // 3 + xx // 3) % 2 == 0)
    planes[1] = planes[0]
    g = torch.Generator().manual_seed(3)
    jit = torch.rand(n * f, 4, generator=g).double().numpy()
    boxes = np.zeros((n * f, 4), dtype=np.float32)
    boxes[0] = [40.3 + jit[0, 0], 30.2 + jit[0, 1], 70.6 + jit[0, 2], 55.4 + jit[0, 3]]   # over the right and bottom edge
    boxes[1] = [20.1 + jit[1, 0], 8.3 + jit[1, 1], 20.1 + jit[1, 0] + 0.6, 40.7 + jit[1, 3]]  # under a pixel wide
    boxes[2] = [1.2 + jit[2, 0], 3.4 + jit[2, 1], 61.3 + jit[2, 2], 44.1 + jit[2, 3]]      # wider than 56 px: grid 3 along x
    boxes[3] = [5.5, 5.5, 30.5, 30.5]   # row 3 of image 0 does not exist (rows_valid 3)
    boxes[4:] = boxes[:4]               # image 1 has no mask row at all
    gt_idx = np.array([0, 1, 2, 0, 0, 1, 2, 0], dtype=np.int32)
    rows_valid = np.array([3, 0], dtype=np.int32)
    ref = np.stack([roi_align_plane64(planes[r // f, gt_idx[r]], boxes[r], M) for r in range(n * f)])
    return planes, boxes, gt_idx, rows_valid, ref


def test_mask_targets(ops):
    planes, boxes, gt_idx, rows_valid, ref = _targets_case()
    n, f = 2, 4
    exist = np.array([r % f < rows_valid[r // f] for r in range(n * f)])
    # preconditions, on the reference alone
    near = np.abs(ref[exist] - 0.5) <= 1e-5
    assert near.mean() <= 0.005, f"{near.mean():.4f} of the pixels sit on the threshold: pick another seed"
    rw = boxes[:, 2] - boxes[:, 0]
    assert boxes[0, 2] > 64 and boxes[0, 3] > 48 and rw[1] < 1.0 and math.ceil(rw[1] / M) == 1 and rw[2] > 56 and math.ceil(rw[2] / M) >= 3
    want = ref >= 0.5
    assert 0.1 < want[exist].mean() < 0.9, "the targets must not be trivial"
    out = ops.mask_targets(torch.from_numpy(planes).to(DEV), torch.from_numpy(boxes).view(n, f, 4).to(DEV),
                           torch.from_numpy(gt_idx).view(n, f).to(DEV), torch.from_numpy(rows_valid).to(DEV), M)
    assert out.shape == (n * f, M, M) and out.dtype == torch.uint8
    got = out.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    diff = (got[exist] != 0) != want[exist]
    print(f"mask_targets: {int(diff.sum())} pixels differ, {int(near.sum())} within 1e-5 of the threshold")
    assert not bool((diff & ~near).any()), f"{int((diff & ~near).sum())} pixels differ away from the threshold"
    assert int(got[~exist].max()) == 0, "rows beyond rows_valid are zeros"


def test_mask_targets_zero_area_box_and_unmatched_row(ops):
    planes, _, _, _, _ = _targets_case()
    boxes = torch.tensor([[[20.5, 20.5, 20.5, 20.5], [12.0, 10.0, 50.0, 35.0]]]).to(DEV)  # zero area; a box inside the rectangle
    gt_idx = torch.tensor([[0, -1]], dtype=torch.int32).to(DEV)
    out = ops.mask_targets(torch.from_numpy(planes[:1]).to(DEV), boxes, gt_idx, torch.tensor([2], dtype=torch.int32).to(DEV), M)
    assert int(out.max()) == 0, "a zero-area box has a 0 x 0 grid, and a row without a matched instance has no target"
    gt_idx = torch.tensor([[0, 0]], dtype=torch.int32).to(DEV)
    out = ops.mask_targets(torch.from_numpy(planes[:1]).to(DEV), boxes, gt_idx, torch.tensor([2], dtype=torch.int32).to(DEV), M)
    assert int(out[0].max()) == 0 and int(out[1].min()) == 1


def test_mask_targets_honour_the_image_size(ops):
    """A plane padded to a larger batch size: with image_hw the samples beyond the image's last row repeat that row ([d2] crops from
    the image's own bitmask); without it they blend into the zero padding."""
    h, w, hp, wp = 20, 24, 32, 32
    plane = np.zeros((1, 1, hp, wp), dtype=np.uint8)
    plane[0, 0, 5:h, 4:w] = 1
    box = np.array([20.2, 16.1, 24.0, 20.0], dtype=np.float32)  # a small box in the image's bottom right corner, inside the mask
    ref = roi_align_plane64(plane[0, 0, :h, :w], box, M)
    assert (np.abs(ref - 0.5) <= 1e-5).sum() == 0 and bool((ref >= 0.5).all())
    args = (torch.from_numpy(plane).to(DEV), torch.from_numpy(box).view(1, 1, 4).to(DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV),
            torch.ones(1, dtype=torch.int32, device=DEV), M)
    out = ops.mask_targets(*args, image_hw=torch.tensor([[h, w]], dtype=torch.int32, device=DEV)).cpu().numpy()[0]
    assert np.array_equal(out != 0, ref >= 0.5)
    padded = roi_align_plane64(plane[0, 0], box, M)
    assert (np.abs(padded - 0.5) <= 1e-5).sum() == 0 and not bool((padded >= 0.5).all()), "the corner bins blend into the padding"
    assert np.array_equal(ops.mask_targets(*args).cpu().numpy()[0] != 0, padded >= 0.5)


# ------------------------------------------------------------------------------------------------------
# osr_mask_loss_fwd / osr_mask_loss_bwd
# ------------------------------------------------------------------------------------------------------
def _loss_case(k):
    g = torch.Generator().manual_seed(11 + k)
    rows = 5
    logits = (torch.rand(rows, M, M, generator=g) * 2 - 1) * 30.0  # +-30: the naive form would overflow / cancel
    logits[0, :4] = torch.tensor([0.0, 1e-3, -1e-3, 29.5]).view(4, 1)
    targets = (torch.rand(rows, M, M, generator=g) < 0.4).to(torch.uint8)
    classes = torch.tensor([0, 2, -1, 1, 0] if k > 1 else [0, 0, -1, 0, 0], dtype=torch.int64)
    return logits, targets, classes


def _loss_reference(logits, targets, fg):
    x = logits[fg].double().requires_grad_(True)
    t = targets[fg].double()
    if x.numel() == 0:
        return 0.0, torch.zeros_like(logits, dtype=torch.float64), [0, 0, 0, 0, 0]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="mean")
    loss.backward()
    grad = torch.zeros_like(logits, dtype=torch.float64)
    grad[fg] = x.grad
    tb = t > 0.5
    wrong = (x.detach() > 0) != tb
    return float(loss.detach()), grad, [int(fg.sum()), int(wrong.sum()), int(tb.sum()), int((wrong & ~tb).sum()), int((wrong & tb).sum())]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("segments", [False, True])
def test_mask_loss_against_float64(ops, k, segments):
    logits, targets, classes = _loss_case(k)
    fg = classes >= 0
    rv, seg = None, 0
    if segments:  # two segments of 3 rows: the first holds 3 rows, the second 1 of its 2 (row 4 does not exist)
        rv, seg = torch.tensor([3, 1], dtype=torch.int32).to(DEV), 3
        fg = fg & torch.tensor([True, True, True, True, False])
    want, wgrad, counts = _loss_reference(logits, targets, fg)
    lg, tg, cl = logits.to(DEV), targets.to(DEV), classes.to(DEV)
    out = ops.mask_loss_fwd(lg, tg, k, cl, rv, seg, loss_weight=1.0).cpu()
    print(f"K={k} segments={segments}: loss {float(out[0]):.7f} (float64 {want:.7f})")
    assert abs(float(out[0]) - want) <= 1e-4 * abs(want)
    assert out[1:].tolist() == [float(c) for c in counts], "foreground rows, incorrect, positive, false positive, false negative"
    assert torch.equal(ops.mask_loss_fwd(lg, tg, k, cl, rv, seg).cpu(), out), "repeats are bit-identical"
    assert float(ops.mask_loss_fwd(lg, tg, k, cl, rv, seg, loss_weight=0.5)[0]) == pytest.approx(0.5 * float(out[0]), rel=1e-6)
    scale = 512.0
    d = ops.mask_loss_bwd(lg, tg, k, cl, rv, seg, scale=scale).cpu().double() / scale
    err = float((d - wgrad).abs().max()) / float(wgrad.abs().max())
    print(f"  d_logits: max abs err / max |ref| = {err:.3e}")
    assert err <= 1e-4
    assert float(d[~fg].abs().max()) == 0.0, "rows that do not count have exact zeros"
    sc = ops.mask_loss_scalars(out, M)
    numel = counts[0] * M * M
    assert sc["mask_rcnn/accuracy"] == 1.0 - counts[1] / max(numel, 1.0)
    assert sc["mask_rcnn/false_positive"] == counts[3] / max(numel - counts[2], 1.0)
    assert sc["mask_rcnn/false_negative"] == counts[4] / max(counts[2], 1.0)


def test_mask_loss_class_agnostic_without_classes(ops):
    logits, targets, _ = _loss_case(1)
    want, _, counts = _loss_reference(logits, targets, torch.ones(5, dtype=torch.bool))
    out = ops.mask_loss_fwd(logits.to(DEV), targets.to(DEV)).cpu()
    assert abs(float(out[0]) - want) <= 1e-4 * abs(want) and out[1:].tolist() == [float(c) for c in counts]


def test_mask_loss_without_a_foreground_row(ops):
    logits, targets, _ = _loss_case(3)
    none = torch.full((5,), -1, dtype=torch.int64).to(DEV)
    out = ops.mask_loss_fwd(logits.to(DEV), targets.to(DEV), 3, none).cpu()
    assert out.tolist() == [0.0] * 6, "no foreground row: the loss is exactly 0"
    d = ops.mask_loss_bwd(logits.to(DEV), targets.to(DEV), 3, none, scale=1024.0)
    assert float(d.abs().max()) == 0.0 and not bool(torch.isnan(d).any())
    rv = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.mask_loss_fwd(logits.to(DEV), targets.to(DEV), 1, None, rv, 5).cpu()
    assert out.tolist() == [0.0] * 6
    sc = ops.mask_loss_scalars(out, M)
    assert sc == {"mask_rcnn/accuracy": 1.0, "mask_rcnn/false_positive": 0.0, "mask_rcnn/false_negative": 0.0}


# ------------------------------------------------------------------------------------------------------
# osr_roi_align_bwd at pooled 8..14 (the pyramid and box set of tests/test_roi_align_p14.py, 2 images)
# ------------------------------------------------------------------------------------------------------
SCALES = (0.25, 0.125, 0.0625, 0.03125)
ROI_ROWS = [([10.0, 10.0, 10.0, 10.0], 0),        # zero area
            ([200.0, 150.0, 260.0, 190.0], 1),    # fully outside the image (p4)
            ([-20.0, -12.0, 14.0, 9.0], 0),       # negative coordinates (p3)
            ([0.0, 0.0, 96.0, 64.0], 1),          # the whole image (p5)
            ([30.2, 20.3, 30.7, 20.9], 0),        # sub-pixel (p2)
            ([5.0, 5.0, 20.0, 20.0], -1),         # padding row
            ([40.0, 30.0, 47.0, 38.0], 1),        # p2
            ([10.0, 8.0, 26.0, 22.0], 0),         # p3
            ([50.0, 10.0, 85.0, 40.0], 1),        # p4
            ([3.0, 2.0, 90.0, 60.0], 0)]          # p5
CANON = 28


def roi_align_torch_opt(feat, rois, scale, out_size, sampling_ratio, aligned):
    """oracle.roi_align_torch generalised to the pooler options (`aligned` False: offset 0, RoI at least 1 x 1; S > 0: a fixed grid):
    the sample positions follow oracle.roi_align_ref line by line, autograd traces the gathers and the weighted sums."""
    if aligned and sampling_ratio == 0:
        return O.roi_align_torch(feat, rois, scale, out_size)
    f32 = np.float32
    n, c, height, width = feat.shape
    off = f32(0.5) if aligned else f32(0.0)
    outs = []
    for r in range(rois.shape[0]):
        b = int(rois[r, 0])
        sw_, sh_ = f32(rois[r, 1]) * f32(scale) - off, f32(rois[r, 2]) * f32(scale) - off
        ew_, eh_ = f32(rois[r, 3]) * f32(scale) - off, f32(rois[r, 4]) * f32(scale) - off
        rw, rh = f32(ew_ - sw_), f32(eh_ - sh_)
        if not aligned:
            rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
        bh, bw = f32(rh / f32(out_size)), f32(rw / f32(out_size))
        gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(rh) / out_size))
        gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(float(rw) / out_size))
        count = float(max(gh * gw, 1))
        ys, xs, ws, bins = [], [], [], []
        for ph in range(out_size):
            for pw in range(out_size):
                for iy in range(gh):
                    y = f32(sh_ + f32(ph) * bh + f32(f32(iy) + f32(0.5)) * bh / f32(gh))
                    for ix in range(gw):
                        x = f32(sw_ + f32(pw) * bw + f32(f32(ix) + f32(0.5)) * bw / f32(gw))
                        if y < -1.0 or y > height or x < -1.0 or x > width:
                            continue
                        yy, xx = max(y, f32(0.0)), max(x, f32(0.0))
                        yl, xl = int(yy), int(xx)
                        if yl >= height - 1:
                            yh = yl = height - 1
                            yy = f32(yl)
                        else:
                            yh = yl + 1
                        if xl >= width - 1:
                            xh = xl = width - 1
                            xx = f32(xl)
                        else:
                            xh = xl + 1
                        ly, lx = f32(yy - f32(yl)), f32(xx - f32(xl))
                        hy, hx = f32(f32(1.0) - ly), f32(f32(1.0) - lx)
                        for (py_, px_, wgt) in ((yl, xl, hy * hx), (yl, xh, hy * lx), (yh, xl, ly * hx), (yh, xh, ly * lx)):
                            ys.append(py_); xs.append(px_); ws.append(float(wgt) / count); bins.append(ph * out_size + pw)
        o = feat.new_zeros((out_size * out_size, c))
        if ys:
            vals = feat[b][:, torch.tensor(ys), torch.tensor(xs)].t() * torch.tensor(ws, dtype=feat.dtype).unsqueeze(1)
            o = o.index_add(0, torch.tensor(bins), vals)
        outs.append(o.t().reshape(c, out_size, out_size))
    return torch.stack(outs)


@functools.lru_cache(maxsize=None)
def _roi_bwd_reference(pooled, aligned, ratio, c=8):
    g = torch.Generator().manual_seed(60 + pooled)
    boxes = torch.tensor([r[0] for r in ROI_ROWS], dtype=torch.float32)
    bidx = torch.tensor([r[1] for r in ROI_ROWS], dtype=torch.int32)
    shapes = [(64 // s, 96 // s) for s in (4, 8, 16, 32)]
    dout = torch.randn(len(ROI_ROWS), pooled, pooled, c, generator=g)
    lv = O.assign_levels(boxes, canonical_size=CANON)
    assert sorted(set(lv.tolist())) == [0, 1, 2, 3]
    grads = []
    for l, (s, (h, w)) in enumerate(zip(SCALES, shapes)):
        feat = torch.zeros(2, c, h, w, dtype=torch.float64, requires_grad=True)
        ids = torch.nonzero((lv == l) & (bidx >= 0)).squeeze(1)
        rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
        out = roi_align_torch_opt(feat, rois, s, pooled, ratio, aligned)  # (k, c, P, P)
        (out * dout[ids].permute(0, 3, 1, 2).double()).sum().backward()
        grads.append(feat.grad.permute(0, 2, 3, 1).contiguous())
    return boxes, bidx, shapes, dout, grads


@pytest.mark.parametrize("aligned,ratio", [(True, 0), (False, 0), (True, 2)])
@pytest.mark.parametrize("pooled", [14, 8])
def test_roi_align_bwd_at_the_mask_pooler_sizes(ops, pooled, aligned, ratio):
    boxes, bidx, shapes, dout, want = _roi_bwd_reference(pooled, aligned, ratio)
    got = ops.roi_align_bwd(dout.to(DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, CANON, 2, aligned=aligned, sampling_ratio=ratio,
                            per_sample=True)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape)
        err = float((a.cpu().double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"P={pooled} aligned={aligned} ratio={ratio} level {l}: max abs err / max |ref| = {err:.3e}")
        assert err <= 1e-4
    # the image-major form of the call (what the trainer passes) lands on the same kernel: pooled > 7 never takes the dense one
    m = boxes.shape[0]
    again = ops.roi_align_bwd(dout.to(DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, CANON, 2, rois_per_image=m // 2, aligned=aligned,
                              sampling_ratio=ratio, per_sample=True)
    for a, b in zip(again, want):
        assert float((a.cpu().double() - b).abs().max()) <= 1e-4 * float(b.abs().max())


def test_roi_align_bwd_half_precision_gradient(ops):
    boxes, bidx, shapes, dout, _ = _roi_bwd_reference(14, True, 0)
    want = ops.roi_align_bwd(dout.half().float().to(DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, CANON, 2, per_sample=True)
    got = ops.roi_align_bwd(dout.half().to(DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, CANON, 2, per_sample=True)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), "fp16 dout is read exactly; only the atomics' order differs"


def test_roi_align_bwd_pooled_7_is_unchanged_and_15_is_refused(osr, ops):
    """pooled 7 through the same entry point runs the kernel it has always run (against autograd, as tests/test_train_bwd.py does);
    pooled 15 is OSR_ERR_UNSUPPORTED with nothing launched (the zeroed pyramid stays zero)."""
    boxes, bidx, shapes, dout, want = _roi_bwd_reference(7, True, 0)
    got = ops.roi_align_bwd(dout.to(DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, CANON, 2)
    for a, b in zip(got, want):
        assert float((a.cpu().double() - b).abs().max()) <= 1e-4 * float(b.abs().max())
    lib, L = osr._lib.load(), osr._lib
    outs = [torch.zeros(2, h, w, 8, device=DEV) for h, w in shapes]
    py = ops._pyramid(outs, SCALES)
    d15 = torch.ones(len(ROI_ROWS), 15, 15, 8, device=DEV)
    b, bi = boxes.to(DEV), bidx.to(DEV)
    st = lib.osr_roi_align_bwd(C.byref(py), 2, C.c_void_p(b.data_ptr()), C.c_void_p(bi.data_ptr()), len(ROI_ROWS), 15, 4, CANON, 2,
                               C.c_void_p(d15.data_ptr()), L.OSR_F32, None)
    assert st == L.ERR_UNSUPPORTED and b"pooled size 1..14" in lib.osr_last_error()
    # the Python wrapper runs 8..14 only for a caller that asks for the per-sample scatter by name
    with pytest.raises(osr.OsrError, match="per_sample"):
        ops.roi_align_bwd(torch.zeros(len(ROI_ROWS), 14, 14, 8, device=DEV), shapes, 2, SCALES, b, bi, 4, CANON, 2)
    with pytest.raises(osr.OsrError, match="pooled size 1..14"):
        ops.roi_align_bwd(d15, shapes, 2, SCALES, b, bi, 4, CANON, 2, per_sample=True)
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in outs)


# ------------------------------------------------------------------------------------------------------
# osr_roi_match_and_sample_ex
# ------------------------------------------------------------------------------------------------------
def test_roi_match_and_sample_ex_matched_index(osr, ops):
    g = torch.Generator().manual_seed(5)
    n, pcap, gmax, bs = 3, 60, 4, 32
    counts_p, counts_g = [60, 40, 25], [4, 0, 2]
    gt = torch.zeros(n, gmax, 4)
    gt[0, :4] = torch.tensor([[20.0, 30.0, 120.0, 140.0], [200.0, 50.0, 320.0, 200.0], [20.0, 30.0, 120.0, 140.0], [150.0, 150.0, 260.0, 290.0]])
    gt[2, :2] = torch.tensor([[40.0, 40.0, 200.0, 220.0], [40.0, 40.0, 200.0, 220.0]])  # identical boxes: the lower index wins
    cls = torch.randint(0, 3, (n, gmax), generator=g)
    pb, pl = torch.zeros(n, pcap, 4), torch.zeros(n, pcap)
    for i, (p, c) in enumerate(zip(counts_p, counts_g)):
        k = p // 2 if c else 0
        if k:
            src = gt[i, torch.randint(0, c, (k,), generator=g)]
            wh = (src[:, 2:] - src[:, :2]).repeat(1, 2)
            pb[i, :k] = src + (torch.rand(k, 4, generator=g) - 0.5) * 0.3 * wh
        ctr = torch.rand(p - k, 2, generator=g) * torch.tensor([400.0, 300.0])
        size = torch.exp(torch.rand(p - k, 2, generator=g) * 3.0 + 1.5)
        pb[i, k:p] = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
        pl[i, :p] = torch.randn(p, generator=g)
    keys = torch.rand(n, pcap + gmax, generator=g)
    pcnt, gcnt = torch.tensor(counts_p, dtype=torch.int32), torch.tensor(counts_g, dtype=torch.int32)
    dev = [t.to(DEV) for t in (pb, pl, pcnt, gt, cls, gcnt, keys)]
    o = {k: v.cpu() for k, v in ops.roi_match_and_sample(*dev, 3, batch_size=bs).items()}
    gidx = o["gt_idx"]
    assert gidx.dtype == torch.int32 and tuple(gidx.shape) == (n, bs)
    saw_twin = False
    for i in range(n):
        p, c = counts_p[i], counts_g[i]
        ki = torch.cat((keys[i, :p], keys[i, pcap:pcap + c]))
        ref = O.roi_label_and_sample(pb[i, :p], pl[i, :p], gt[i, :c], cls[i, :c], ki, num_classes=3, batch_size=bs)
        nfg = ref["num_fg"]
        assert o["counts"][i].tolist() == [len(ref["sampled_idx"]), nfg, ref["num_bg"]]
        assert bool((gidx[i, nfg:] == -1).all()), "background and padding rows carry -1"
        if c == 0:
            assert nfg == 0
            continue
        assert nfg > 0
        midx, _ = O.matcher(O.pairwise_iou(gt[i, :c], torch.cat((pb[i, :p], gt[i, :c]))), [0.5], [0, 1], False)
        assert torch.equal(gidx[i, :nfg].long(), midx[ref["sampled_idx"][:nfg]]), f"image {i}"
        assert torch.equal(gt[i][gidx[i, :nfg].long()], o["gt_boxes"][i, :nfg]), "the index names the matched box the call returns"
        twins = (2,) if i == 0 else (1,)
        assert not any(int(t) in gidx[i, :nfg].tolist() for t in twins), "of two identical ground-truth boxes the lower index wins"
        saw_twin = saw_twin or 0 in gidx[i, :nfg].tolist()
    assert saw_twin
    # the entry point without the index: every other output bit-identical, through the C ABI
    lib = osr._lib.load()
    pbd, pld, pcd, gtd, cld, gcd, kyd = dev
    outs = dict(boxes=torch.empty(n, bs, 4), logits=torch.empty(n, bs), gt_classes=torch.empty(n, bs, dtype=torch.int64), ious=torch.empty(n, bs),
                gt_boxes=torch.empty(n, bs, 4), src=torch.empty(n, bs, dtype=torch.int32), batch_idx=torch.empty(n * bs, dtype=torch.int32),
                counts=torch.empty(n, 3, dtype=torch.int32))
    outs = {k: v.to(DEV) for k, v in outs.items()}
    wsb = lib.osr_roi_match_sample_workspace_bytes(n, pcap, gmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    p_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = lib.osr_roi_match_and_sample(p_(pbd), p_(pld), p_(pcd), pcap, p_(gtd), p_(cld), p_(gcd), gmax, n, p_(kyd), 3, bs, 0.25, 0.5,
                                      *(p_(outs[k]) for k in ("boxes", "logits", "gt_classes", "ious", "gt_boxes", "src", "batch_idx", "counts")),
                                      p_(ws), wsb, None)
    assert st == 0, lib.osr_last_error()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert torch.equal(v.cpu(), o[k]), k
