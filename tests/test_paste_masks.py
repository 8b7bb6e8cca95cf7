"""osr_paste_masks (csrc/osr_mask_head.hip) against [d2] _do_paste_mask(skip_empty=False) restated with F.grid_sample in float64.

12 masks of sigmoid(2 * randn) pasted into a 37 x 53 image; the boxes include one that reaches outside the image on two sides, one
0.7 pixels wide and one covering the image. Bytes must be equal except at pixels whose reference value lies within 1e-5 of the
threshold (fp32 grid_sample differs from float64 by at most 1.8e-6 on these inputs); such pixels must be fewer than 0.1 % of the
non-zero pixels -- a condition on the inputs, asserted (0 with these). The output buffer is pre-filled with 0xFF: the kernel writes
every byte, the zeros outside the boxes included."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W, M, THR = 37, 53, 28, 0.5


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def _inputs():
    g = torch.Generator().manual_seed(77)
    masks = torch.sigmoid(2.0 * torch.randn(12, M, M, generator=g))
    x0 = torch.rand(12, generator=g) * (W - 12)
    y0 = torch.rand(12, generator=g) * (H - 10)
    bw = 3.0 + torch.rand(12, generator=g) * (W - 12 - x0).clamp(min=4.0)
    bh = 3.0 + torch.rand(12, generator=g) * (H - 10 - y0).clamp(min=4.0)
    boxes = torch.stack((x0, y0, x0 + bw, y0 + bh), dim=1)
    boxes[0] = torch.tensor([-8.5, -5.25, 20.3, 15.8])    # reaches outside the image on two sides
    boxes[1] = torch.tensor([30.0, 5.0, 30.7, 30.0])      # 0.7 pixels wide
    boxes[2] = torch.tensor([0.0, 0.0, float(W), float(H)])  # the whole image
    boxes[3] = torch.tensor([40.5, 20.5, 70.0, 50.0])     # ... and on the other two sides
    return masks, boxes


def _reference(masks, boxes):
    """[d2] _do_paste_mask(skip_empty=False) in float64 -> the sampled values (r, H, W)."""
    m, b = masks.double(), boxes.double()
    x0, y0, x1, y1 = b[:, 0:1], b[:, 1:2], b[:, 2:3], b[:, 3:4]
    img_y = torch.arange(0, H, dtype=torch.float64) + 0.5
    img_x = torch.arange(0, W, dtype=torch.float64) + 0.5
    img_y = (img_y - y0) / (y1 - y0) * 2 - 1
    img_x = (img_x - x0) / (x1 - x0) * 2 - 1
    gx = img_x[:, None, :].expand(len(b), H, W)
    gy = img_y[:, :, None].expand(len(b), H, W)
    return F.grid_sample(m[:, None], torch.stack([gx, gy], dim=3), align_corners=False)[:, 0]


def test_bytes_equal_the_grid_sample_reference(ops):
    masks, boxes = _inputs()
    ref = _reference(masks, boxes)
    want = (ref >= THR).to(torch.uint8)
    band = (ref - THR).abs() < 1e-5
    nonzero = int((ref > 0).sum())
    assert int(band.sum()) < 1e-3 * nonzero, "too many reference values at the threshold: choose other inputs"
    assert int(want[1].sum()) > 0 and int(want[0].sum()) > 0, "the thin box and the clipped box must paste something"
    out = torch.full((12, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    got = ops.paste_masks(masks.to(DEV), boxes.to(DEV), H, W, THR, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu()
    assert set(got.unique().tolist()) <= {0, 1}, "every byte is written, 0 or 1"
    diff = (got != want) & ~band
    print(f"pasted {int(want.sum())} ones of {want.numel()} bytes; {int(band.sum())} in the threshold band; {int(diff.sum())} differ")
    assert int(diff.sum()) == 0
    # every byte whose pixel centre lies outside its mask's box is 0
    ys = (torch.arange(H) + 0.5)[None, :, None]
    xs = (torch.arange(W) + 0.5)[None, None, :]
    b = boxes[:, :, None, None]
    outside = (xs < b[:, 0]) | (xs > b[:, 2]) | (ys < b[:, 1]) | (ys > b[:, 3])
    assert int(outside.sum()) > 0 and int(got[outside].sum()) == 0
    # a second run and a freshly allocated output give the same bytes
    assert torch.equal(ops.paste_masks(masks.to(DEV), boxes.to(DEV), H, W, THR).cpu(), got)


def test_other_thresholds_and_sizes(ops):
    masks, boxes = _inputs()
    for thr, (h, w) in ((0.3, (H, W)), (0.7, (5, 130)), (0.5, (70, 3))):
        sx, sy = w / W, h / H
        bx = boxes * torch.tensor([sx, sy, sx, sy])
        m, b = masks.double(), bx.double()
        iy = ((torch.arange(0, h, dtype=torch.float64) + 0.5) - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * 2 - 1
        ix = ((torch.arange(0, w, dtype=torch.float64) + 0.5) - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * 2 - 1
        grid = torch.stack([ix[:, None, :].expand(12, h, w), iy[:, :, None].expand(12, h, w)], dim=3)
        ref = F.grid_sample(m[:, None], grid, align_corners=False)[:, 0]
        band = (ref - thr).abs() < 1e-5
        got = ops.paste_masks(masks.to(DEV), bx.to(DEV), h, w, thr).cpu()
        assert got.shape == (12, h, w)
        assert int(((got != (ref >= thr).to(torch.uint8)) & ~band).sum()) == 0, (thr, h, w)


def test_no_masks(ops):
    out = ops.paste_masks(torch.zeros(0, M, M, device=DEV), torch.zeros(0, 4, device=DEV), H, W)
    assert out.shape == (0, H, W) and out.dtype == torch.uint8


def test_degenerate_boxes_paste_nothing(ops):
    """Among the ordinary boxes: a zero-width box, a zero-height box, a box with a NaN coordinate and one with x1 = inf paste nothing --
    an all-zero plane, every byte written over the 0xFF fill. (Zero extent: the sample coordinate is +-inf, never 0 / 0, as no pixel
    centre x + 0.5 equals the integer edge. NaN: every comparison is false. x1 = inf: every pixel samples u = -0.5, half of the
    mask's first column, below the threshold 0.5 as every probability is below 1 -- a condition on the inputs, asserted.)
    The inverted box (x1 < x0) is no special case of the definition: u = M - 1 - u' of the box with its edges swapped, so the
    float64 grid_sample restatement pastes the mask mirrored along x into [x1, x0], and so must the kernel."""
    masks, boxes = _inputs()
    assert float(masks.max()) < 1.0 - 1e-4
    boxes[4] = torch.tensor([20.0, 5.0, 20.0, 30.0])           # zero width
    boxes[5] = torch.tensor([10.0, 12.0, 40.0, 12.0])          # zero height
    boxes[6] = torch.tensor([40.0, 5.0, 12.0, 30.0])           # inverted along x
    boxes[7] = torch.tensor([float("nan"), 5.0, 30.0, 20.0])   # a NaN coordinate
    boxes[8] = torch.tensor([10.0, 5.0, float("inf"), 20.0])   # an inf coordinate
    nothing = [4, 5, 7, 8]
    rest = [i for i in range(12) if i not in nothing]
    ref = _reference(masks[rest], boxes[rest])
    want = (ref >= THR).to(torch.uint8)
    band = (ref - THR).abs() < 1e-5
    assert int(band.sum()) < 1e-3 * int((ref > 0).sum()), "too many reference values at the threshold: choose other inputs"
    inv = rest.index(6)
    swapped = boxes[6:7, [2, 1, 0, 3]]
    assert torch.equal(want[inv], (_reference(torch.flip(masks[6:7], dims=[-1]), swapped) >= THR).to(torch.uint8)[0]) and int(want[inv].sum()) > 0
    out = torch.full((12, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    got = ops.paste_masks(masks.to(DEV), boxes.to(DEV), H, W, THR, out=out).cpu()
    assert set(got.unique().tolist()) <= {0, 1}, "every byte is written, 0 or 1"
    for i in nothing:
        assert int(got[i].sum()) == 0, f"box {i} ({boxes[i].tolist()}) pasted something"
    diff = (got[rest] != want) & ~band
    print(f"ordinary and inverted boxes: {int(want.sum())} ones, {int(band.sum())} in the threshold band, {int(diff.sum())} differ")
    assert int(diff.sum()) == 0


def test_a_value_exactly_at_the_threshold_is_pasted(ops):
    """A mask of 0.5 everywhere in the box (0, 0, W, H) at threshold 0.5: one pixel in from each edge all four taps lie inside the mask,
    their weights sum to 1 and the blend of equal values is the value (products by 0.5 are exact; (1 - a) + a rounds to 1 for every
    fraction a of a coordinate >= 0.25) -- with >= every interior byte is 1. (On the rim a tap is outside: half the value, 0.)"""
    masks = torch.full((1, M, M), 0.5)
    boxes = torch.tensor([[0.0, 0.0, float(W), float(H)]])
    out = torch.full((1, H, W), 0xFF, dtype=torch.uint8, device=DEV)
    got = ops.paste_masks(masks.to(DEV), boxes.to(DEV), H, W, 0.5, out=out).cpu()
    assert set(got.unique().tolist()) <= {0, 1}, "every byte is written, 0 or 1"
    inner = got[0, 1:-1, 1:-1]
    assert int(inner.sum()) == inner.numel(), f"{inner.numel() - int(inner.sum())} interior pixels at the threshold were not pasted"
