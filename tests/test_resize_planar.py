"""osr_resize_bilinear_u8_planar: the resize (+ horizontal flip) of test-time augmentation on planar uint8 images equals
PIL.Image.resize(BILINEAR) (then np.flip along x) bit for bit, and the interleaved entry point on the transposed data gives the same
bits. Shapes: odd up-scaling (a wrong mirror index shows), down-scaling with a support wider than two taps, the copy case, and a
one-column image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [((37, 53), (96, 137)), ((96, 128), (41, 55)), ((96, 128), (96, 128)), ((5, 1), (9, 3))]


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
    assert w == 1 or not np.array_equal(ref, np.flip(ref, axis=2)), "precondition: the mirror must be visible"
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
