"""The training-side kernels of the mask branch (csrc/osr_mask_train.hip, the per-sample scatter of csrc/osr_roi_align.hip and
osr_roi_match_and_sample_ex), each against a reference written here or taken from the oracle:

  osr_mask_targets        float64 torchvision loop (BitMasks.crop_and_resize = roi_align(bitmask, box, M, aligned) >= 0.5); a pixel may
                          differ only where the float64 average lies within 1e-5 of the threshold (fp32 evaluation)
  osr_mask_loss_fwd/_bwd  float64 binary_cross_entropy_with_logits (mean) and its autograd gradient, 1e-4 relative (the fp32 contract);
                          the counts behind the three mask_rcnn/* scalars exactly
  osr_roi_align_bwd       at pooled 14 and 8: autograd of the oracle's differentiable RoIAlign, 1e-4 relative
  osr_roi_match_and_sample_ex   the matched ground-truth index of the oracle's matcher; every other output bit-identical to the
                          entry point without it

The mask targets and the loss are also run where their indexing takes another path: three images whose planes, boxes and sizes all
differ (asserted on the reference: swapping two planes or two images' boxes changes it), M = 16 / 17 / 20, every branch that writes
zeros, sample grids up to 6 x 10; the loss past one pass of each of its three grids (1408 rows, 1 103 872 pixels), at exactly 2^24
pixels and refused one row beyond, at M = 1 / 16 / 17, without rows, and at |x| up to 104.5, target bytes 2 / 128 / 255 and NaN / inf on
rows that do not count.
Measured on gfx950: mask targets -- no pixel differs in any case (0 or 1 pixel per case within 1e-5 of the threshold); loss 2e-8 ..
1e-7 relative (1e-3 of the bound); d_logits 9e-8 .. 1.6e-7 of max |ref| (2e-3 of the bound); every count exact."""
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


def _shapes(h, w, cell=3):
    """A rectangle, a disc and a checkerboard on an h x w plane."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((3, h, w), dtype=np.uint8)
    out[0, h // 5:(3 * h) // 4, w // 5:(4 * w) // 5] = 1
    out[1] = ((yy - h / 2.0) ** 2 + (xx - w / 2.0 + 2.0) ** 2 <= (0.3 * (h + w) / 2.0) ** 2)
    out[2] = ((yy // cell + xx // cell) % 2 == 0)
    return out


def _targets_reference(planes, boxes, gt_idx, rows_valid, m, image_hw=None):
    """-> (float64 bin averages (n * F, m, m), rows that have a target at all): the kernel's row rule restated (a row beyond
    rows_valid, without an instance of its own image, or with a box that is not finite is zeros), the image's own size cropping its
    plane, then the float64 RoIAlign loop."""
    n, gmax, hm, wm = planes.shape
    f = gt_idx.shape[1]
    ref, live = np.zeros((n * f, m, m)), np.zeros(n * f, dtype=bool)
    for i in range(n):
        h, w = (hm, wm) if image_hw is None else (min(max(int(image_hw[i][0]), 1), hm), min(max(int(image_hw[i][1]), 1), wm))
        for j in range(f):
            g, box = int(gt_idx[i, j]), boxes[i, j]
            if j >= rows_valid[i] or g < 0 or g >= gmax or not bool(np.isfinite(box).all()):
                continue
            live[i * f + j] = True
            ref[i * f + j] = roi_align_plane64(planes[i, g, :h, :w], box, m)
    return ref, live


def _targets_compare(ops, planes, boxes, gt_idx, rows_valid, m, image_hw=None, name=""):
    """The file's rule: a pixel may differ from (float64 average >= 0.5) only where that average is within 1e-5 of 0.5, and such
    pixels are at most 0.5 % of the live ones -- asserted on the reference before the launch. -> (got, want, live)."""
    ref, live = _targets_reference(planes, boxes, gt_idx, rows_valid, m, image_hw)
    near = np.abs(ref - 0.5) <= 1e-5
    assert live.any() and near[live].mean() <= 0.005, f"{name}: {near[live].mean():.4f} of the live pixels sit on the threshold"
    n, f = gt_idx.shape
    hw = None if image_hw is None else torch.tensor(np.asarray(image_hw), dtype=torch.int32, device=DEV)
    out = ops.mask_targets(torch.from_numpy(planes).to(DEV), torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).view(n, f, 4).to(DEV),
                           torch.from_numpy(np.ascontiguousarray(gt_idx, dtype=np.int32)).to(DEV),
                           torch.tensor(np.asarray(rows_valid), dtype=torch.int32, device=DEV), m, image_hw=hw)
    assert out.shape == (n * f, m, m) and out.dtype == torch.uint8
    got = out.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    want = ref >= 0.5
    diff = (got != 0) != want
    print(f"mask_targets {name}: {int(diff[live].sum())} of {int(live.sum()) * m * m} live pixels differ, {int(near[live].sum())} within 1e-5 of the threshold")
    assert not bool((diff & ~near).any()), f"{name}: {int((diff & ~near).sum())} pixels differ away from the threshold"
    assert not got[~live].any(), f"{name}: rows without a target are zeros"
    return got, want, live


@functools.lru_cache(maxsize=None)
def _three_image_case():
    """3 images, gmax 3, 40 x 56 planes: the three shapes shifted and permuted per image, so that all nine planes differ. F 5,
    rows_valid [2, 0, 5]; seeded non-integer boxes that differ per image; image 1 and 2 are smaller than the plane and a box of image 2
    hangs over its own bottom right corner (inside the plane)."""
    n, gmax, h, w, f = 3, 3, 40, 56, 5
    base = _shapes(h, w)
    planes = np.stack([np.stack([np.roll(base[(g + i) % 3], (2 * i, 5 * i), axis=(0, 1)) for g in range(gmax)]) for i in range(n)])
    g = torch.Generator().manual_seed(17)
    u = torch.rand(n, f, 4, generator=g).double().numpy()
    boxes = np.zeros((n, f, 4), dtype=np.float32)
    boxes[..., 0], boxes[..., 1] = u[..., 0] * 22.0, u[..., 1] * 12.0
    boxes[..., 2], boxes[..., 3] = boxes[..., 0] + 8.0 + u[..., 2] * 30.0, boxes[..., 1] + 8.0 + u[..., 3] * 22.0
    boxes[2, 4] = [30.3, 20.6, 54.7, 39.2]
    gt_idx = np.array([[2, 0, 1, 0, 2], [0, 1, 2, 0, 1], [1, 2, 0, 0, 2]], dtype=np.int32)
    rows_valid = np.array([2, 0, 5], dtype=np.int32)
    image_hw = np.array([[40, 56], [33, 47], [36, 50]], dtype=np.int32)
    return planes, boxes, gt_idx, rows_valid, image_hw


def test_mask_targets_every_image_and_plane_is_observed(ops):
    """img > 0 indexes the planes, the boxes, gt_idx, rows_valid and image_hw; here every one of them differs per image."""
    planes, boxes, gt_idx, rows_valid, image_hw = _three_image_case()
    n, gmax = planes.shape[:2]

    def want_of(pl, bx):
        ref, live = _targets_reference(pl, bx, gt_idx, rows_valid, M, image_hw)
        return (ref >= 0.5)[live]

    want = want_of(planes, boxes)
    assert 0.1 < want.mean() < 0.9, "the targets must not be trivial"
    assert boxes[2, 4, 2] > image_hw[2, 1] and boxes[2, 4, 3] > image_hw[2, 0], "a box hangs over its image's own edge"
    padded, live = _targets_reference(planes, boxes, gt_idx, rows_valid, M)
    assert not np.array_equal(want, (padded >= 0.5)[live]), "the image's own size must matter"
    # an indexing error cannot hide: swapping two planes of which a live row reads at least one, or two images' boxes, changes the
    # reference (image 1 has no row, image 0 two: their other planes are read by nothing)
    seen = {(i, int(gt_idx[i, j])) for i in range(n) for j in range(rows_valid[i])}
    assert {g for i, g in seen if i == 2} == {0, 1, 2} and len(seen) == 5
    flat = [(i, g) for i in range(n) for g in range(gmax)]
    for a in range(len(flat)):
        for b in range(a + 1, len(flat)):
            if flat[a] in seen or flat[b] in seen:
                sw = planes.copy()
                sw[flat[a]], sw[flat[b]] = planes[flat[b]], planes[flat[a]]
                assert not np.array_equal(want_of(sw, boxes), want), f"swapping planes {flat[a]} and {flat[b]} must change the reference"
    for a in range(n):
        for b in range(a + 1, n):
            sw = boxes.copy()
            sw[a], sw[b] = boxes[b], boxes[a]
            assert not np.array_equal(want_of(planes, sw), want), f"swapping the boxes of images {a} and {b} must change the reference"
    _targets_compare(ops, planes, boxes, gt_idx, rows_valid, M, image_hw, "3 images")


@pytest.mark.parametrize("m", [16, 17, 20])
def test_mask_targets_other_sides(ops, m):
    """M * M = 256 is exactly one pass of the workgroup, 289 and 400 leave a partial second one. Boxes exactly 16 and 32 pixels wide:
    at M = 16 the bin is exactly 1 or 2 pixels and ceil(size / M) sits on its boundary, exactly in fp32 and float64 alike."""
    planes, _, _, _, _ = _three_image_case()
    planes = planes[:2]
    boxes = np.array([[[3.25, 2.75, 19.25, 18.75], [10.25, 4.25, 42.25, 36.25], [6.4, 3.3, 40.9, 30.2], [0.0, 0.0, 1.0, 1.0]],
                      [[20.75, 11.25, 52.75, 27.25], [8.25, 1.25, 24.25, 33.25], [2.25, 6.75, 34.25, 38.75], [15.7, 9.1, 38.2, 35.6]]], dtype=np.float32)
    size = boxes[..., 2:] - boxes[..., :2]
    assert {float(v) for v in size[0, :2].ravel()} | {float(v) for v in size[1, :3].ravel()} == {16.0, 32.0}
    assert all(float(np.float32(v) / np.float32(16)) in (1.0, 2.0) for v in (16.0, 32.0))
    gt_idx = np.array([[0, 1, 2, 0], [2, 0, 1, 1]], dtype=np.int32)
    got, want, live = _targets_compare(ops, planes, boxes, gt_idx, np.array([3, 4]), m, None, f"M={m}")
    assert live.sum() == 7 and 0.1 < want[live].mean() < 0.9


def test_mask_targets_rows_without_a_target(ops):
    """Every branch that writes zeros, each one row between two live control rows: an instance index beyond gmax or negative, a
    box that is not finite, an inverted box (a sample grid of 0 or fewer), a box wholly outside the image on each side."""
    planes, _, _, _, _ = _three_image_case()
    n, gmax, h, w = planes.shape
    ok = [12.3, 6.4, 44.9, 33.7]
    rows = [(ok, 0), (ok, gmax), (ok, gmax + 5), (ok, -1), ([12.3, float("nan"), 44.9, 33.7], 0), ([12.3, 6.4, float("inf"), 33.7], 0),
            ([44.9, 6.4, 12.3, 33.7], 0), ([12.3, 33.7, 44.9, 6.4], 0), ([-40.2, 6.4, -10.1, 33.7], 0), ([w + 2.0, 6.4, w + 30.5, 33.7], 0),
            ([12.3, -35.5, 44.9, -8.2], 0), ([12.3, h + 1.5, 44.9, h + 25.0], 0), (ok, 1)]
    f = len(rows)
    boxes = np.zeros((n, f, 4), dtype=np.float32)
    boxes[:] = np.array([r[0] for r in rows], dtype=np.float32)
    gt_idx = np.tile(np.array([r[1] for r in rows], dtype=np.int32), (n, 1))
    ref, live = _targets_reference(planes, boxes, gt_idx, [f] * n, M)
    # on the reference alone: the inverted and the outside boxes are "live" rows whose float64 average is 0 everywhere
    assert live.reshape(n, f)[0].tolist() == [True] + [False] * 5 + [True] * 7 and float(np.abs(ref.reshape(n, f, M, M)[:, 6:12]).max()) == 0.0
    got, want, _ = _targets_compare(ops, planes, boxes, gt_idx, [f] * n, M, None, "zero branches")
    got = got.reshape(n, f, M, M)
    assert not got[:, 1:12].any(), "rows 1 .. 11 have no target"
    assert got[:, 0].any() and got[:, 12].any() and not np.array_equal(got[0, 0], got[1, 0]), "the control rows are live and differ per image"


def test_mask_targets_image_size_beyond_the_plane_and_zero(ops):
    planes, boxes, gt_idx, rows_valid, _ = _three_image_case()
    n, gmax, h, w = planes.shape
    args = (torch.from_numpy(planes).to(DEV), torch.from_numpy(boxes).to(DEV), torch.from_numpy(gt_idx).to(DEV), torch.from_numpy(rows_valid).to(DEV), M)
    plain = ops.mask_targets(*args)
    larger = ops.mask_targets(*args, image_hw=torch.tensor([[h + 9, w + 1], [h, w + 100], [4 * h, w]], dtype=torch.int32, device=DEV))
    assert torch.equal(larger, plain) and int(plain.max()) == 1, "an image size beyond the plane is the plane's"
    # an image size of 0 is taken as 1: the reference on the 1 x 1 crop, whose only pixel every valid sample reads
    boxes1 = np.array([[[-1.0, -1.2, 2.6, 2.2], [-0.4, -0.3, 1.2, 1.1]]] * n, dtype=np.float32)
    gt1 = np.array([[2, 0], [1, 2], [0, 1]], dtype=np.int32)
    assert {int(planes[i, gt1[i, j], 0, 0]) for i in range(n) for j in range(2)} == {0, 1}
    got, want, live = _targets_compare(ops, planes, boxes1, gt1, [2, 2, 2], M, [[0, 0], [0, 7], [1, 0]], "image_hw 0")
    assert live.all() and 0.05 < want.mean() < 0.95


@pytest.mark.parametrize("m,box,grid", [(28, [0.0, 0.0, 160.0, 96.0], (4, 6)), (16, [0.0, 0.0, 160.0, 96.0], (6, 10)),
                                        (16, [12.3, -2.0, 142.3, 98.0], (7, 9))])
def test_mask_targets_large_sample_grid(ops, m, box, grid):
    """Up to 60 samples per bin (the earlier cases stop at 3 per axis); the third box also hangs over the top and the bottom."""
    h, w = 96, 160
    # (no checkerboard here: with whole-pixel bins half of its samples are set, exactly, in a large share of the bins)
    yy, xx = np.mgrid[0:h, 0:w]
    sh = _shapes(h, w)
    planes = np.stack([sh[1] ^ (1.37 * yy + 0.61 * xx < 118.3), sh[0] ^ ((yy - 41.3) ** 2 + 0.4 * (xx - 97.7) ** 2 <= 35.1 ** 2)]).astype(np.uint8)[None]
    boxes = np.array([[box, box]], dtype=np.float32)
    assert (math.ceil((box[3] - box[1]) / m), math.ceil((box[2] - box[0]) / m)) == grid
    got, want, _ = _targets_compare(ops, planes, boxes, np.array([[1, 0]], dtype=np.int32), [2], m, None, f"grid {grid}")
    assert 0.1 < want.mean() < 0.9 and not np.array_equal(want[0], want[1])


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


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _loss_entry(osr, which, logits, targets, rows, m, k, classes, rv, seg, out, scale=1.0):
    """osr_mask_loss_fwd / _bwd through the C interface, into an output the caller owns (and has filled with a sentinel)."""
    lib = osr._lib.load()
    ws = torch.empty(256 * 6 * 4, dtype=torch.uint8, device=DEV)
    st = getattr(lib, f"osr_mask_loss_{which}")(_ptr(logits), _ptr(targets), rows, m, k, _ptr(classes), _ptr(rv), seg, scale, _ptr(out), _ptr(ws),
                                                ws.numel(), None)
    torch.cuda.synchronize()
    return st


def _live_rows(classes, num_rows, rows_valid, seg_rows, rows):
    """mt_row_class >= 0 (csrc/osr_mask_mfma.h) restated: the row exists in its segment, and its class is a predictor row -- any
    class >= 0 when the predictor has one row."""
    r = torch.arange(rows)
    live = torch.ones(rows, dtype=torch.bool)
    if rows_valid is not None:
        live &= (r % seg_rows) < rows_valid.long()[r // seg_rows]
    if classes is not None:
        live &= (classes >= 0) & ((classes < num_rows) | (num_rows == 1))
    return live


@functools.lru_cache(maxsize=None)
def _grid_case(k):
    """11 segments of 128 rows at M = 28: 1408 rows, 1 103 872 pixels -- more than the backward's 4096 workgroups x 256 threads, about
    17 trips of the forward's 65 536 threads and 6 of the row counter's 256."""
    g = torch.Generator().manual_seed(40 + k)
    nseg, seg = 11, 128
    rows = nseg * seg
    rv = torch.randint(0, seg + 1, (nseg,), generator=g).to(torch.int32)
    rv[1], rv[3], rv[6] = seg, 0, 1  # (the last segment keeps its draw: it straddles the backward's first grid pass)
    classes = torch.randint(-1, 4, (rows,), generator=g) if k > 1 else None  # (3 == num_rows: no predictor row)
    logits = (torch.rand(rows, M, M, generator=g) * 2 - 1) * 30.0
    targets = (torch.rand(rows, M, M, generator=g) < 0.4).to(torch.uint8)
    fg = _live_rows(classes, k, rv, seg, rows)
    return logits, targets, classes, rv, seg, fg, _loss_reference(logits, targets, fg)


@pytest.mark.parametrize("k", [3, 1])
def test_mask_loss_past_one_grid_pass(osr, ops, k):
    logits, targets, classes, rv, seg, fg, (want, wgrad, counts) = _grid_case(k)
    rows, mm, one_pass = logits.shape[0], M * M, 4096 * 256
    # on the reference alone: a kernel cut to its first trip, or a row counter cut to its first 256 rows, would not pass
    live = torch.nonzero(fg).squeeze(1)
    assert rows * mm > one_pass and int(fg.sum()) > 256 and bool(fg[256:].any())
    assert int(live[0]) * mm < one_pass <= int(live[-1]) * mm, "live pixels on both sides of the backward's first grid pass"
    assert bool((~fg)[one_pass // mm + 1:].any()), "and a row that does not count beyond it"
    assert sorted(rv.tolist())[0] == 0 and 1 in rv.tolist() and seg in rv.tolist()
    lg, tg, rvd = logits.to(DEV), targets.to(DEV), rv.to(DEV)
    cl = None if classes is None else classes.to(DEV)
    out = ops.mask_loss_fwd(lg, tg, k, cl, rvd, seg).cpu()
    print(f"K={k}: {int(fg.sum())} live rows, loss {float(out[0]):.7f} (float64 {want:.7f}, rel {abs(float(out[0]) - want) / want:.2e})")
    assert abs(float(out[0]) - want) <= 1e-4 * abs(want)
    assert out[1:].tolist() == [float(c) for c in counts], "foreground rows, incorrect, positive, false positive, false negative"
    assert torch.equal(ops.mask_loss_fwd(lg, tg, k, cl, rvd, seg).cpu(), out), "repeats are bit-identical"
    scale = 512.0
    d = torch.full_like(lg, float("nan"))
    assert _loss_entry(osr, "bwd", lg, tg, rows, M, k, cl, rvd, seg, d, scale) == 0
    assert not bool(torch.isnan(d).any()), "every pixel is written"
    assert torch.equal(ops.mask_loss_bwd(lg, tg, k, cl, rvd, seg, scale=scale), d), "repeats are bit-identical"
    d = d.cpu()
    err = float((d.double() / scale - wgrad).abs().max()) / float(wgrad.abs().max())
    print(f"  d_logits: max abs err / max |ref| = {err:.3e}")
    assert err <= 1e-4
    assert torch.equal(d[~fg], torch.zeros_like(d[~fg])), "rows that do not count have exact zeros"


def test_mask_loss_at_the_pixel_limit(osr, ops):
    """256 rows of 256 x 256 are exactly 2^24 pixels, the most the fp32 counts hold exactly; one row more is refused by both entry
    points with nothing written. The operands are drawn on the device (64 MB of logits); the float64 loss and the integer counts are
    taken on the CPU in chunks of 32 rows."""
    rows, m = 256, 256
    g = torch.Generator(device=DEV).manual_seed(7)
    lg = torch.randn(rows, m, m, device=DEV, generator=g) * 3.0
    tg = (torch.rand(rows, m, m, device=DEV, generator=g) < 0.4).to(torch.uint8)
    assert rows * m * m == 1 << 24
    out = ops.mask_loss_fwd(lg, tg).cpu()
    scale = 1024.0
    d = ops.mask_loss_bwd(lg, tg, scale=scale)
    total, counts, err, top = 0.0, [0, 0, 0, 0], 0.0, 0.0
    for r0 in range(0, rows, 32):
        x, t = lg[r0:r0 + 32].cpu().double(), tg[r0:r0 + 32].cpu() != 0
        total += float(torch.nn.functional.binary_cross_entropy_with_logits(x, t.double(), reduction="sum"))
        wrong = (x > 0) != t
        counts = [c + int(v.sum()) for c, v in zip(counts, (wrong, t, wrong & ~t, wrong & t))]
        ref = (torch.sigmoid(x) - t.double()) / float(1 << 24)
        err = max(err, float((d[r0:r0 + 32].cpu().double() / scale - ref).abs().max()))
        top = max(top, float(ref.abs().max()))
    want = total / float(1 << 24)
    print(f"2^24 pixels: loss {float(out[0]):.7f} (float64 {want:.7f}, rel {abs(float(out[0]) - want) / want:.2e}); d_logits {err / top:.3e} of max |ref|")
    assert abs(float(out[0]) - want) <= 1e-4 * want
    assert out[1:].tolist() == [256.0] + [float(c) for c in counts]
    assert err <= 1e-4 * top
    del d
    # one row more
    L, lib = osr._lib, osr._lib.load()
    lg1, tg1 = torch.zeros(rows + 1, m, m, device=DEV), torch.zeros(rows + 1, m, m, dtype=torch.uint8, device=DEV)
    out6 = torch.full((6,), -7.0, device=DEV)
    assert _loss_entry(osr, "fwd", lg1, tg1, rows + 1, m, 1, None, None, 0, out6) == L.ERR_UNSUPPORTED and b"2^24" in lib.osr_last_error()
    assert out6.tolist() == [-7.0] * 6
    d1 = torch.full((rows + 1, m, m), -7.0, device=DEV)
    assert _loss_entry(osr, "bwd", lg1, tg1, rows + 1, m, 1, None, None, 0, d1) == L.ERR_UNSUPPORTED and b"2^24" in lib.osr_last_error()
    assert bool((d1 == -7.0).all())
    with pytest.raises(osr.OsrError, match="2\\^24"):
        ops.mask_loss_fwd(lg1, tg1)
    with pytest.raises(osr.OsrError, match="2\\^24"):
        ops.mask_loss_bwd(lg1, tg1)


@functools.lru_cache(maxsize=None)
def _edge_case():
    """6 rows at M = 28 against 3 predictor rows, two segments of 3 with rows_valid (3, 2): rows 0, 1 and 4 count; row 2 has class -1,
    row 3 class 3 == num_rows, row 5 lies beyond its segment's count. Row 0 starts with the planted logits, each against both target
    values; rows 1 and 4 carry target bytes other than 0 and 1."""
    g = torch.Generator().manual_seed(29)
    logits = torch.randn(6, M, M, generator=g) * 3.0
    targets = (torch.rand(6, M, M, generator=g) < 0.4).to(torch.uint8)
    planted = [87.0, 89.0, 103.9, 104.5, 0.0, 1e-30]
    vals = torch.tensor([s * v for v in planted for s in (1.0, -1.0)], dtype=torch.float32)
    n = vals.numel()
    logits.view(6, -1)[0, :2 * n] = vals.repeat(2)
    targets.view(6, -1)[0, :n], targets.view(6, -1)[0, n:2 * n] = 0, 1
    targets[1, 3:6][targets[1, 3:6] != 0] = 2
    targets[1, 6:9][targets[1, 6:9] != 0] = 128
    targets[4][targets[4] != 0] = 255
    classes = torch.tensor([0, 2, -1, 3, 1, 0], dtype=torch.int64)
    rv = torch.tensor([3, 2], dtype=torch.int32)
    fg = _live_rows(classes, 3, rv, 3, 6)
    return logits, targets, classes, rv, fg, _loss_reference(logits, (targets != 0).to(torch.uint8), fg)


def test_mask_loss_value_edges(ops):
    """|x| of 87 .. 104.5, where expf(-|x|) is small, subnormal or 0; +-0 and +-1e-30; target bytes 2, 128 and 255, which are
    positives in the loss, the gradient and the count; and NaN / inf logits on the rows that do not count, which change nothing."""
    logits, targets, classes, rv, fg, (want, wgrad, counts) = _edge_case()
    assert fg.tolist() == [True, True, False, False, True, False]
    assert {2, 128, 255} <= set(targets[fg].unique().tolist()) and math.copysign(1.0, float(logits[0, 0, 9])) == -1.0 and float(logits[0, 0, 9]) == 0.0
    assert float(torch.tensor(-104.5).exp()) == 0.0 and 0.0 < float(torch.tensor(-89.0).exp()) < 1.18e-38, "fp32: exp(-104.5) is 0, exp(-89) subnormal"
    lg, tg, cl, rvd = logits.to(DEV), targets.to(DEV), classes.to(DEV), rv.to(DEV)
    out = ops.mask_loss_fwd(lg, tg, 3, cl, rvd, 3).cpu()
    print(f"edges: loss {float(out[0]):.7f} (float64 {want:.7f}, rel {abs(float(out[0]) - want) / want:.2e})")
    assert abs(float(out[0]) - want) <= 1e-4 * abs(want)
    assert out[1:].tolist() == [float(c) for c in counts] and counts[2] == int((targets[fg] != 0).sum())
    scale = 512.0
    d = ops.mask_loss_bwd(lg, tg, 3, cl, rvd, 3, scale=scale).cpu()
    # absolutely, against the largest reference magnitude: sigmoid(-89) is subnormal in fp32 and carries no relative accuracy
    err = float((d.double() / scale - wgrad).abs().max()) / float(wgrad.abs().max())
    print(f"  d_logits: max abs err / max |ref| = {err:.3e}")
    assert err <= 1e-4
    assert torch.equal(d[~fg], torch.zeros_like(d[~fg]))
    bad = logits.clone()
    bad[2] = float("nan")
    bad[3, ::2], bad[3, 1::2] = float("inf"), float("-inf")
    bad[5, :, ::3], bad[5, :, 1::3], bad[5, :, 2::3] = float("nan"), float("inf"), float("-inf")
    assert torch.equal(ops.mask_loss_fwd(bad.to(DEV), tg, 3, cl, rvd, 3).cpu(), out), "rows that do not count are not read into the loss"
    db = ops.mask_loss_bwd(bad.to(DEV), tg, 3, cl, rvd, 3, scale=scale).cpu()
    assert torch.equal(db[fg], d[fg]) and torch.equal(db[~fg], torch.zeros_like(db[~fg]))


@pytest.mark.parametrize("m", [1, 16, 17])
def test_mask_loss_other_sides(ops, m):
    """The pixel -> row division i / (M * M) with M * M = 1, 256 (one workgroup pass per row) and 289."""
    g = torch.Generator().manual_seed(70 + m)
    logits = (torch.rand(3, m, m, generator=g) * 2 - 1) * 8.0
    targets = (torch.rand(3, m, m, generator=g) < 0.4).to(torch.uint8)
    classes = torch.tensor([1, -1, 2], dtype=torch.int64)
    fg = classes >= 0
    want, wgrad, counts = _loss_reference(logits, targets, fg)
    out = ops.mask_loss_fwd(logits.to(DEV), targets.to(DEV), 3, classes.to(DEV)).cpu()
    assert abs(float(out[0]) - want) <= 1e-4 * abs(want) and out[1:].tolist() == [float(c) for c in counts]
    d = ops.mask_loss_bwd(logits.to(DEV), targets.to(DEV), 3, classes.to(DEV), scale=64.0).cpu()
    assert float((d.double() / 64.0 - wgrad).abs().max()) <= 1e-4 * float(wgrad.abs().max())
    assert torch.equal(d[1], torch.zeros(m, m))


@pytest.mark.parametrize("k", [1, 3])
def test_mask_loss_without_any_row(osr, ops, k):
    """rows == 0 (an empty tensor has no address, whatever the predictor's rows): six exact zeros and an empty gradient."""
    logits, targets = torch.empty(0, M, M, device=DEV), torch.empty(0, M, M, dtype=torch.uint8, device=DEV)
    classes = None if k == 1 else torch.empty(0, dtype=torch.int64, device=DEV)
    assert ops.mask_loss_fwd(logits, targets, k, classes).cpu().tolist() == [0.0] * 6
    d = ops.mask_loss_bwd(logits, targets, k, classes, scale=8.0)
    assert tuple(d.shape) == (0, M, M) and d.dtype == torch.float32
    out6 = torch.full((6,), -7.0, device=DEV)
    assert _loss_entry(osr, "fwd", None, None, 0, M, k, None, None, 0, out6) == 0 and out6.tolist() == [0.0] * 6
    assert _loss_entry(osr, "bwd", None, None, 0, M, k, None, None, 0, None) == 0


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
