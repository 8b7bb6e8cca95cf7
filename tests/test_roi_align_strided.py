"""osr_roi_align_fwd_strided: the pooler that produces only the bins a stride-2 1 x 1 convolution reads ([d2] Res5ROIHeads with
STRIDE_IN_1X1: res5.0.conv1 and res5.0.shortcut). Every bin it writes must be the same bits as that bin of the full grid
(osr_roi_align_fwd_ordered_opt), under every pooler option, for every kind of RoI, in any processing order."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M, N, H, W = 3000, 2, 20, 30          # RoIs, images, the stride-16 map of a 320 x 480 image
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


@pytest.fixture(scope="module")
def rois():
    """(boxes (M, 4), batch_idx (M,), a shuffled order (M,)): random boxes reaching past the image, and the special ones in front."""
    gg = torch.Generator().manual_seed(5)
    cx, cy = torch.rand(M, generator=gg) * 560 - 40, torch.rand(M, generator=gg) * 400 - 40
    w, h = torch.rand(M, generator=gg) ** 2 * 500 + 1, torch.rand(M, generator=gg) ** 2 * 340 + 1
    boxes = torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), dim=1)
    special = torch.tensor([
        [100.0, 80.0, 100.0, 80.0],      # zero area: a point
        [50.0, 60.0, 50.0, 200.0],       # zero width
        [30.0, 90.5, 300.0, 90.5],       # zero height
        [700.0, 500.0, 900.0, 640.0],    # wholly outside, beyond the far corner
        [-300.0, -200.0, -40.0, -30.0],  # wholly outside, before the origin
        [0.0, 0.0, 480.0, 320.0],        # the map itself
        [-50.0, -50.0, 600.0, 400.0],    # larger than the map
        [0.0, 0.0, 16.0, 16.0],          # one cell: bins far smaller than a pixel
    ])
    boxes[:len(special)] = special
    bidx = torch.randint(0, N, (M,), generator=gg, dtype=torch.int32)
    bidx[torch.rand(M, generator=gg) < 0.1] = -1   # padding rows, scattered
    bidx[:len(special)] = torch.arange(len(special), dtype=torch.int32) % N
    bidx[-40:] = -1                                 # and a padding tail, as the per-image lists end
    order = torch.randperm(M, generator=gg).to(torch.int32)
    return boxes.contiguous().to(DEV), bidx.to(DEV), order.to(DEV)


def features(c, dtype, levels):
    gg = torch.Generator().manual_seed(7 + c)
    out = []
    for l in range(levels):
        out.append(torch.randn(N, H >> l, W >> l, c, generator=gg).to(dtype).to(DEV))
    return out, [1.0 / (16 << l) for l in range(levels)]


def pool(ops, feats, scales, boxes, bidx, pooled, aligned, sr, **kw):
    # level = floor(4 + log2(sqrt(area) / 128)) clamped to the pyramid: boxes of 256 px and more go to the second level
    return ops.roi_align(feats, scales, boxes, bidx, pooled, feats[0].dtype, 4, 128, 4, aligned=bool(aligned), sampling_ratio=sr, **kw)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("aligned", [1, 0])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", [1024, 64])
@pytest.mark.parametrize("pooled", [14, 13, 8])
def test_every_bin_is_the_full_grids_bin(ops, rois, pooled, c, dtype, aligned, sr, levels):
    boxes, bidx, order = rois
    feats, scales = features(c, DTYPES[dtype], levels)
    full = pool(ops, feats, scales, boxes, bidx, pooled, aligned, sr)
    want = full[:, ::2, ::2]
    q = (pooled + 1) // 2
    got = pool(ops, feats, scales, boxes, bidx, pooled, aligned, sr, bin_stride=2)
    assert got.shape == (M, q, q, c) and got.dtype == full.dtype and got.is_contiguous()
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ from the full grid's"
    real = bidx >= 0
    assert bool((got[~real] == 0).all()), "padding rows are not zero"
    assert bool(torch.isfinite(got.float()).all())
    if aligned == 1 and sr == 0:
        assert bool((got[0] == 0).all())  # the zero-area box under {aligned, adaptive}: an empty grid
    assert bool((got[3] == 0).all()) and bool((got[4] == 0).all())  # wholly outside: no valid sample
    assert bool((got[5] != 0).any()) and bool((got[real][8:] != 0).any())
    # any processing order, same bits; with OSR_ROI_NO_PADDING_FILL the real rows are the same bits too
    shuffled = pool(ops, feats, scales, boxes, bidx, pooled, aligned, sr, bin_stride=2, order=order)
    assert torch.equal(shuffled, got)
    nofill = pool(ops, feats, scales, boxes, bidx, pooled, aligned, sr, bin_stride=2, order=order, fill_padding=False)
    assert torch.equal(nofill[real], got[real])


def test_two_levels_are_both_used(ops, rois):
    """(what the two-level cases above rest on: the RoI list reaches both levels, and the level changes the result)"""
    boxes, bidx, _ = rois
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    big = (area.sqrt() >= 256) & (bidx >= 0)
    assert 100 < int(big.sum()) < M - 100
    f2, s2 = features(64, torch.float16, 2)
    one = pool(ops, f2[:1], s2[:1], boxes, bidx, 14, 1, 0, bin_stride=2)
    two = pool(ops, f2, s2, boxes, bidx, 14, 1, 0, bin_stride=2)
    assert not torch.equal(one[big], two[big]) and torch.equal(one[~big], two[~big])


@pytest.mark.parametrize("fill", [True, False], ids=["fill", "no-padding-fill"])
def test_padding_rows_are_zeroed_or_left_alone(ops, osr, rois, fill):
    """The C call on a buffer of its own: with OSR_ROI_NO_PADDING_FILL the padding rows keep what the buffer held."""
    boxes, bidx, _ = rois
    feats, scales = features(64, torch.float16, 1)
    lib, L = osr._lib.load(), osr._lib
    py = ops._pyramid(feats, scales)
    out = torch.full((M, 7, 7, 64), 3.0, dtype=torch.float16, device=DEV)
    opt = L.RoiOptions(1, 0)
    st = lib.osr_roi_align_fwd_strided(ctypes.byref(py), L.OSR_F16, N, ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(bidx.data_ptr()), M, 14, 2,
                                       4, 128, 4, None, None, 0 if fill else 1, ctypes.byref(opt), ctypes.c_void_p(out.data_ptr()), L.OSR_F16,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    pad = bidx < 0
    assert bool((out[pad] == (0.0 if fill else 3.0)).all())
    assert torch.equal(out[~pad], pool(ops, feats, scales, boxes, bidx, 14, 1, 0, bin_stride=2)[~pad])


def test_bin_stride_one_is_the_present_call(ops, rois):
    boxes, bidx, _ = rois
    feats, scales = features(64, torch.bfloat16, 1)
    lib_out = pool(ops, feats, scales, boxes, bidx, 14, 1, 0)
    assert torch.equal(pool(ops, feats, scales, boxes, bidx, 14, 1, 0, bin_stride=1), lib_out)


def test_refusals(ops, osr, rois):
    boxes, bidx, _ = rois
    feats, scales = features(64, torch.float16, 1)
    for pooled, stride in ((7, 2), (14, 3), (8, 3), (1, 2)):
        with pytest.raises(osr._lib.OsrError, match=r"status -2"):
            pool(ops, feats, scales, boxes, bidx, pooled, 1, 0, bin_stride=stride)
    with pytest.raises(ValueError):
        pool(ops, feats, scales, boxes, bidx, 14, 1, 0, bin_stride=0)
