"""osr_resize_bilinear_u8_planar: the resize (+ horizontal flip) of test-time augmentation on planar uint8 images equals
PIL.Image.resize(BILINEAR) (then np.flip along x) bit for bit, and the interleaved entry point on the transposed data gives the same
bits. Shapes: odd up-scaling (a wrong mirror index shows), down-scaling with a support wider than two taps, the copy case, a
one-column image, a one-row image and a one-pixel destination. The last tests give the two arguments Pillow's full-image tables
never exercise a value of their own: y_first > 0 (the rows above the first row the vertical pass reads are skipped) and, for the
interleaved entry, a row pitch wider than the image."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [((37, 53), (96, 137)), ((96, 128), (41, 55)), ((96, 128), (96, 128)), ((5, 1), (9, 3)), ((1, 40), (3, 17)), ((9, 7), (1, 1))]


def _tables(osr, n_in, n_out):
    from openset_rcnn_amd.host.data import pil_resample_coeffs
    b, c = pil_resample_coeffs(n_in, n_out)
    return torch.from_numpy(b).to(DEV), torch.from_numpy(c).to(DEV), int(b[0, 0]), int(b[-1, 0] + b[-1, 1]), int(c.shape[1])


def _pil(img_chw: np.ndarray, nh: int, nw: int) -> np.ndarray:
    from PIL import Image
    hwc = np.ascontiguousarray(img_chw.transpose(1, 2, 0))
    out = np.asarray(Image.fromarray(hwc).resize((nw, nh), Image.BILINEAR))
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def _run(osr, img: torch.Tensor, nh: int, nw: int, mirror: bool) -> torch.Tensor:
    h, w = int(img.shape[-2]), int(img.shape[-1])
    xb, xc, _, _, kx = _tables(osr, w, nw)
    yb, yc, y0, y1, ky = _tables(osr, h, nh)
    out = osr.ops.resize_bilinear_u8_planar(img, xb, xc, kx, yb, yc, ky, y0, y1 - y0, nh, nw, mirror=mirror)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("src, dst", CASES, ids=[f"{a[0]}x{a[1]}-to-{b[0]}x{b[1]}" for a, b in CASES])
def test_equals_pil_and_the_interleaved_entry(osr, src, dst):
    (h, w), (nh, nw) = src, dst
    rng = np.random.RandomState(1000 + h * w + nh)
    img = rng.randint(0, 256, size=(3, h, w), dtype=np.uint8)  # seeded, not symmetric
    ref = _pil(img, nh, nw)
    assert w == 1 or nw == 1 or not np.array_equal(ref, np.flip(ref, axis=2)), "precondition: the mirror must be visible"
    d = torch.from_numpy(img).to(DEV)
    plain = _run(osr, d, nh, nw, False)
    assert plain.shape == (3, nh, nw) and plain.dtype == torch.uint8
    assert np.array_equal(plain.cpu().numpy(), ref)
    mirrored = _run(osr, d, nh, nw, True)
    assert np.array_equal(mirrored.cpu().numpy(), np.flip(ref, axis=2))
    # the interleaved entry point on the transposed data
    xb, xc, _, _, kx = _tables(osr, w, nw)
    yb, yc, y0, y1, ky = _tables(osr, h, nh)
    inter = osr.ops.resize_bilinear_u8(d.permute(1, 2, 0).contiguous(), xb, xc, kx, yb, yc, ky, y0, y1 - y0, nh, nw)
    torch.cuda.synchronize()
    assert torch.equal(inter, plain)


def test_a_stacked_batch_equals_its_images(osr):
    """(n, 3, h, w): the planes of a group of same-size images in one launch pair."""
    rng = np.random.RandomState(7)
    imgs = rng.randint(0, 256, size=(2, 3, 37, 53), dtype=np.uint8)
    out = _run(osr, torch.from_numpy(imgs).to(DEV), 64, 91, True)
    assert out.shape == (2, 3, 64, 91)
    for i in range(2):
        assert np.array_equal(out[i].cpu().numpy(), np.flip(_pil(imgs[i], 64, 91), axis=2))


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
def test_y_first_skips_the_rows_above(osr, mirror):
    """37 x 53 -> 96 x 137 with k = 5 rows of 255 on top of the source (42 rows): every ybounds[:, 0] moved down by k, y_first = k and
    y_rows = the 37 rows the vertical pass reads. The horizontal pass must start at row y_first and the vertical pass must index its
    intermediate by ymin - y_first: the output is PIL's resize of the unpadded image, through the planar and the interleaved entry."""
    (h, w), (nh, nw), k = (37, 53), (96, 137), 5
    rng = np.random.RandomState(2000)
    img = rng.randint(0, 256, size=(3, h, w), dtype=np.uint8)
    ref = _pil(img, nh, nw)
    padded = np.concatenate([np.full((3, k, w), 255, dtype=np.uint8), img], axis=1)
    assert padded.shape == (3, h + k, w)
    d = torch.from_numpy(padded).to(DEV)
    xb, xc, _, _, kx = _tables(osr, w, nw)
    yb, yc, y0, y1, ky = _tables(osr, h, nh)
    assert (y0, y1) == (0, h)
    yb = yb.clone()
    yb[:, 0] += k
    out = osr.ops.resize_bilinear_u8_planar(d, xb, xc, kx, yb, yc, ky, k + y0, y1 - y0, nh, nw, mirror=mirror)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.flip(ref, axis=2) if mirror else ref)
    if not mirror:
        inter = osr.ops.resize_bilinear_u8(d.permute(1, 2, 0).contiguous(), xb, xc, kx, yb, yc, ky, k + y0, y1 - y0, nh, nw)
        torch.cuda.synchronize()
        assert np.array_equal(inter.cpu().numpy(), ref)


def test_interleaved_row_stride_wider_than_the_image(osr):
    """The image is the [:, :w] view of an (h, w + 7, 3) buffer whose other columns are 255, handed to the C entry with
    in_row_stride = (w + 7) * 3: the output equals PIL on the contiguous copy."""
    (h, w), (nh, nw), extra = (37, 53), (96, 137), 7
    rng = np.random.RandomState(2001)
    img = rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8)
    ref = _pil(np.ascontiguousarray(img.transpose(2, 0, 1)), nh, nw)
    wide = np.full((h, w + extra, 3), 255, dtype=np.uint8)
    wide[:, :w] = img
    d = torch.from_numpy(wide).to(DEV)
    xb, xc, _, _, kx = _tables(osr, w, nw)
    yb, yc, y0, y1, ky = _tables(osr, h, nh)
    tmp_bytes = (y1 - y0) * nw * 3
    tmp = torch.zeros((tmp_bytes,), dtype=torch.uint8, device=DEV)
    out = torch.zeros((3, nh, nw), dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    status = osr._lib.load().osr_resize_bilinear_u8(p(d), h, w, (w + extra) * 3, p(xb), p(xc), kx, p(yb), p(yc), ky, y0, y1 - y0, nh, nw, p(tmp),
                                                    tmp_bytes, p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    assert int((ref == 0).sum()) < ref.size // 50  # (the zero fill of `out` is not the answer)
