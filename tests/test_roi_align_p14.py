"""RoIAlign forward at pooled sizes 8..14 (the mask head's pooler; csrc/osr_roi_align.hip roi_align_big_kernel) against the oracle's
per-RoI loop (oracle.osr_oracle.roi_align_ref, generic in out_size), level by level.

Two pyramids: a 2-image 64 x 96 input (p2 16 x 24 .. p5 2 x 3, canonical size 28 so that the boxes land on all four levels) and a
1-image 160 x 224 input with canonical size 448, where the whole-image box and a wide strip stay on p2: bins up to 4 level pixels wide,
adaptive grid 4. The boxes include a zero-area box, one fully outside the image, one with negative coordinates, the whole image, a
sub-pixel box and a padding row. Tolerances: those of tests/test_hip_ops.py's RoIAlign tests for the same dtypes (fp32: rtol 1e-4,
atol 1e-5; fp16 in and out: rtol 2^-10, atol 2e-3)."""
import ctypes as C
import functools

import pytest
import torch

from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALES = (0.25, 0.125, 0.0625, 0.03125)
OPTIONS = [(True, 0), (False, 0), (True, 2)]


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(name: str, c: int):
    """-> (feats NCHW fp32 per level, boxes (m, 4), batch_idx (m,), canonical_size)."""
    g = torch.Generator().manual_seed(50 + c)
    if name == "small":  # 2 images of 64 x 96
        n, h, w, canon = 2, 64, 96, 28
        rows = [([10.0, 10.0, 10.0, 10.0], 0),        # zero area
                ([200.0, 150.0, 260.0, 190.0], 1),    # fully outside the image (p4)
                ([-20.0, -12.0, 14.0, 9.0], 0),       # negative coordinates (p3)
                ([0.0, 0.0, 96.0, 64.0], 1),          # the whole image (p5)
                ([30.2, 20.3, 30.7, 20.9], 0),        # sub-pixel (p2)
                ([5.0, 5.0, 20.0, 20.0], -1),         # padding row
                ([40.0, 30.0, 47.0, 38.0], 1),        # p2
                ([10.0, 8.0, 26.0, 22.0], 0),         # p3
                ([50.0, 10.0, 85.0, 40.0], 1),        # p4
                ([3.0, 2.0, 90.0, 60.0], 0)]          # p5
    else:  # 1 image of 160 x 224; the large boxes stay on p2 (40 x 56): bins of 2.9 .. 4 pixels, grid up to 4
        n, h, w, canon = 1, 160, 224, 448
        rows = [([0.0, 0.0, 224.0, 160.0], 0),        # the whole image: bins 4 x 2.86 pixels, grid 4 x 3
                ([5.0, 60.0, 215.0, 75.0], 0),        # a strip: bins 3.75 pixels wide, grid 4 x 1
                ([100.0, 20.0, 160.0, 150.0], 0),
                ([7.0, 7.0, 60.0, 30.0], -1),         # padding row
                ([-30.0, -30.0, 100.0, 90.0], 0)]     # negative coordinates, large
    feats = tuple(torch.randn(n, c, h // s, w // s, generator=g) for s in (4, 8, 16, 32))
    boxes = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    bidx = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    return feats, boxes, bidx, canon


@functools.lru_cache(maxsize=None)
def _reference(name: str, c: int, pooled: int, aligned: bool, ratio: int, dt: torch.dtype):
    """(m, c, P, P) from roi_align_ref per level, on the features as the kernel reads them (rounded to dt); padding rows zero."""
    feats, boxes, bidx, canon = _case(name, c)
    lv = O.assign_levels(boxes, canonical_size=canon)
    ref = torch.zeros(boxes.shape[0], c, pooled, pooled)
    for l, s in enumerate(SCALES):
        ids = torch.nonzero((lv == l) & (bidx >= 0)).squeeze(1)
        if len(ids):
            rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
            ref[ids] = torch.from_numpy(O.roi_align_ref(feats[l].to(dt).float().numpy(), rois.numpy(), s, pooled, ratio, aligned))
    return ref, lv


def _run(ops, name, c, pooled, aligned, ratio, dt, **kw):
    feats, boxes, bidx, canon = _case(name, c)
    fl = [nhwc(f).to(dt).to(DEV) for f in feats]
    return ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), pooled, dt, 4, canon, 2, aligned=aligned, sampling_ratio=ratio, **kw)


def _check(out, ref, dt, name):
    a, b = out.cpu().float().permute(0, 3, 1, 2), ref
    rtol, atol = (1e-4, 1e-5) if dt == torch.float32 else (2.0 ** -10, 2e-3)
    err = (a - b).abs()
    print(f"{name}: max abs err {float(err.max()):.3e} (max |ref| {float(b.abs().max()):.3f})")
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err {float(err.max()):.3e}"


@pytest.mark.parametrize("aligned,ratio", OPTIONS)
@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("pooled", [8, 13, 14])
@pytest.mark.parametrize("name", ["small", "large"])
def test_pooled_8_to_14_against_the_oracle(ops, name, pooled, dt, aligned, ratio):
    ref, lv = _reference(name, 16, pooled, aligned, ratio, dt)
    if name == "small":
        assert sorted(set(lv.tolist())) == [0, 1, 2, 3], "the boxes must land on all four levels"
    out = _run(ops, name, 16, pooled, aligned, ratio, dt)
    assert out.shape == (ref.shape[0], pooled, pooled, 16) and out.dtype == dt
    _check(out, ref, dt, f"{name} P={pooled} aligned={aligned} ratio={ratio} {dt}")
    pad = int(torch.nonzero(_case(name, 16)[2] < 0)[0])
    assert float(out[pad].abs().max()) == 0.0, "a padding row is filled with zeros"
    if name == "small" and aligned and ratio == 0:
        assert float(out[0].abs().max()) == 0.0, "a zero-area box has a 0 x 0 adaptive grid: zeros"


def test_adaptive_grid_reaches_four(ops):
    """The 'large' case's precondition: ceil(roi / 14) is 4 along x for the whole-image box and the strip (p2, 56 pixels wide)."""
    _, boxes, _, canon = _case("large", 16)
    lv = O.assign_levels(boxes, canonical_size=canon)
    assert lv[0] == 0 and lv[1] == 0
    for i in (0, 1):
        wpx = float(boxes[i, 2] - boxes[i, 0]) * 0.25
        assert wpx / 14 > 2.0 and -(-wpx // 14) == 4


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_256_channels(ops, dt):
    ref, _ = _reference("small", 256, 14, True, 0, dt)
    out = _run(ops, "small", 256, 14, True, 0, dt)
    _check(out, ref, dt, f"C=256 P=14 {dt}")


@pytest.mark.parametrize("aligned,ratio", OPTIONS)
def test_result_does_not_depend_on_the_order(ops, aligned, ratio):
    m = _case("small", 16)[1].shape[0]
    base = _run(ops, "small", 16, 13, aligned, ratio, torch.float32)  # the locality order
    for order in (torch.arange(m, dtype=torch.int32), torch.arange(m - 1, -1, -1, dtype=torch.int32),
                  torch.tensor([3, 7, 0, 9, 5, 1, 8, 2, 6, 4], dtype=torch.int32)):
        out = _run(ops, "small", 16, 13, aligned, ratio, torch.float32, order=order.to(DEV))
        assert torch.equal(out, base)
    assert torch.equal(_run(ops, "small", 16, 13, aligned, ratio, torch.float32), base), "repeats are bit-identical"


@pytest.mark.parametrize("entry", ["osr_roi_align_fwd", "osr_roi_align_fwd_ordered", "osr_roi_align_fwd_ordered_ex", "osr_roi_align_fwd_ordered_opt"])
def test_every_forward_entry_point_and_the_padding_fill(osr, ops, entry):
    """The four C entry points at pooled = 14 into a buffer pre-filled with 7: all pool the same bits; the padding row is zeroed, or
    left at 7 under OSR_ROI_NO_PADDING_FILL."""
    lib, L = osr._lib.load(), osr._lib
    feats, boxes, bidx, canon = _case("small", 16)
    fl = [nhwc(f).to(DEV) for f in feats]
    py = ops._pyramid(fl, SCALES)
    b, bi = boxes.to(DEV), bidx.to(DEV)
    m, pad = boxes.shape[0], 5
    want = _run(ops, "small", 16, 14, True, 0, torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    head = (C.byref(py), L.OSR_F32, 2, p(b), p(bi), m, 14, 4, canon, 2)
    for no_fill in ((0,) if entry in ("osr_roi_align_fwd", "osr_roi_align_fwd_ordered") else (0, 1)):
        out = torch.full((m, 14, 14, 16), 7.0, device=DEV)
        tail = (p(out), L.OSR_F32, None)
        if entry == "osr_roi_align_fwd":
            st = lib.osr_roi_align_fwd(*head, *tail)
        elif entry == "osr_roi_align_fwd_ordered":
            st = lib.osr_roi_align_fwd_ordered(*head, None, None, *tail)
        elif entry == "osr_roi_align_fwd_ordered_ex":
            st = lib.osr_roi_align_fwd_ordered_ex(*head, None, None, no_fill, *tail)
        else:
            st = lib.osr_roi_align_fwd_ordered_opt(*head, None, None, no_fill, C.byref(L.RoiOptions(1, 0)), *tail)
        assert st == 0, lib.osr_last_error()
        torch.cuda.synchronize()
        keep = torch.arange(m) != pad
        assert torch.equal(out[keep], want[keep])
        assert float(out[pad].min()) == float(out[pad].max()) == (7.0 if no_fill else 0.0)


def test_pooled_15_and_the_backward_at_8_are_refused(osr, ops):
    feats, boxes, bidx, canon = _case("small", 16)
    fl = [nhwc(f).to(DEV) for f in feats]
    with pytest.raises(osr.OsrError, match="pooled size 1..14"):
        ops.roi_align(fl, SCALES, boxes.to(DEV), bidx.to(DEV), 15, torch.float32, 4, canon, 2)
    shapes = [(f.shape[2], f.shape[3]) for f in feats]
    m = boxes.shape[0]
    with pytest.raises(osr.OsrError, match="pooled size 1..7"):
        ops.roi_align_bwd(torch.zeros(m, 8, 8, 16, device=DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, canon, 2)
    # 7 stays on the kernels it has always run
    ops.roi_align_bwd(torch.zeros(m, 7, 7, 16, device=DEV), shapes, 2, SCALES, boxes.to(DEV), bidx.to(DEV), 4, canon, 2)
