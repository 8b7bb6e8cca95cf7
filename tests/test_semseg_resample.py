"""osr_semseg_resample (csrc/osr_semseg.hip) against detectron2's two interpolations in float64 (tests/panoptic_common.py): C = 54 in a
pitch of 56, (h4, w4) = (16, 24), crops that are no multiples of 4, an upscale, the identity and a downscale. Values within 1e-4 max |ref|;
labels equal wherever the reference's top-two gap is at least 1e-4 max |ref| (the excluded share is bounded in
tests/test_panoptic_reference.py and here); an exact tie goes to the lower class; padding channels never win.

The tiled path passes the classes through LDS 56 at a time and carries the running argmax across the passes: RESAMPLE_WIDE_CASES has
57, 133 and 150 classes (two and three passes), a one-row map (h4 == 1, a 65-pixel output row) and a one-cell map, under the same rules.
Measured on the MI355X: max error 1.9e-6 (6.2e-7 of max |ref|) over the five cases in every storage type, 2.0e-5 (6.5e-6) on the
strong downscale with 133 classes; at most 0.19 % of the pixels excluded as near ties (0.20 % on the strong downscale)."""
import pytest
import torch

from tests.panoptic_common import (RESAMPLE_C as C, RESAMPLE_CASES, RESAMPLE_PITCH as PITCH, RESAMPLE_WIDE_CASES, resample_logits, resample_reference,
                                   resample_wide_logits, top_two_gap)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _padded(logits, fill=1000.0):
    """(h4, w4, C) -> (h4, w4, PITCH) with the padding channels far above every real logit."""
    out = torch.full(tuple(logits.shape[:2]) + (PITCH,), fill, dtype=logits.dtype)
    out[..., :C] = logits
    return out.contiguous()


@pytest.mark.parametrize("crop,out_hw", RESAMPLE_CASES, ids=["up", "identity", "down"])
def test_values_and_labels_match_the_two_interpolations(osr, crop, out_hw):
    ops = osr.ops
    logits = resample_logits()
    ref = resample_reference(logits, crop, out_hw)
    scale = float(ref.abs().max())
    dev = _padded(logits).to(DEV)
    values = ops.semseg_resample(dev, C, crop, out_hw, labels=False)
    assert values.dtype == torch.float32 and tuple(values.shape) == (C,) + tuple(out_hw)
    err = float((values.cpu().double() - ref).abs().max())
    print(f"[resample] {crop} -> {out_hw}: max err {err:.3e} = {err / scale:.3e} of max |ref| (bound 1e-4)")
    assert err <= 1e-4 * scale
    labels = ops.semseg_resample(dev, C, crop, out_hw, labels=True)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == tuple(out_hw)
    assert int(labels.min()) >= 0 and int(labels.max()) < C  # the padding channels hold 1000 and never win
    sure = top_two_gap(ref) >= 1e-4 * scale
    share = 1.0 - float(sure.double().mean())
    print(f"[resample] {crop} -> {out_hw}: {100 * share:.3f} % of the pixels excluded as near ties")
    assert share <= 0.005
    assert torch.equal(labels.cpu()[sure].long(), ref.argmax(dim=0)[sure])
    assert torch.equal(ops.semseg_resample(dev, C, crop, out_hw, labels=True), labels)
    assert torch.equal(ops.semseg_resample(dev, C, crop, out_hw, labels=False), values)


def test_a_strong_downscale_takes_the_untiled_path(osr):
    """(22, 397) -> (7, 70) over a 6 x 100 map: the first 64 output pixels of a row span ~94 stride-4 columns, more than a wave's LDS
    tile holds (40), so those waves read their taps from global memory; the last 6 pixels of each row span 11 and stay tiled."""
    ops = osr.ops
    torch.manual_seed(12)
    logits = torch.randn(6, 100, C)
    crop, out_hw = (22, 397), (7, 70)
    ref = resample_reference(logits, crop, out_hw)
    scale = float(ref.abs().max())
    dev = _padded(logits).to(DEV)
    values = ops.semseg_resample(dev, C, crop, out_hw, labels=False)
    assert float((values.cpu().double() - ref).abs().max()) <= 1e-4 * scale
    labels = ops.semseg_resample(dev, C, crop, out_hw, labels=True)
    sure = top_two_gap(ref) >= 1e-4 * scale
    assert float(sure.double().mean()) >= 0.99
    assert torch.equal(labels.cpu()[sure].long(), ref.argmax(dim=0)[sure])
    assert torch.equal(ops.semseg_resample(dev, C, crop, out_hw, labels=True), labels)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_low_precision_logits_are_read_as_stored(osr, dtype):
    ops = osr.ops
    crop, out_hw = RESAMPLE_CASES[0]
    stored = resample_logits().to(dtype)
    ref = resample_reference(stored.double(), crop, out_hw)
    values = ops.semseg_resample(_padded(stored, 1000.0).to(DEV), C, crop, out_hw, labels=False)
    assert float((values.cpu().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_an_exact_tie_goes_to_the_lower_class(osr):
    ops = osr.ops
    crop, out_hw = RESAMPLE_CASES[0]
    logits = resample_logits()
    logits[..., 7] = logits[..., 3] = logits.max(dim=2).values + 1.0  # classes 3 and 7 carry the same, largest, value at every cell
    labels = ops.semseg_resample(_padded(logits).to(DEV), C, crop, out_hw, labels=True)
    assert bool((labels == 3).all())
    flat = torch.zeros(16, 24, PITCH)
    flat[..., C:] = 5.0
    assert bool((ops.semseg_resample(flat.to(DEV), C, (64, 96), (64, 96), labels=True) == 0).all())


def test_bad_arguments_are_refused(osr):
    ops = osr.ops
    x = torch.zeros(16, 24, PITCH, device=DEV)
    with pytest.raises(osr.OsrError):
        ops.semseg_resample(x.cpu(), C, (64, 96), (64, 96), labels=True)
    with pytest.raises(osr.OsrError):
        ops.semseg_resample(x, C, (65, 96), (64, 96), labels=True)  # crop beyond 4 * h4
    with pytest.raises(osr.OsrError):
        ops.semseg_resample(x, PITCH + 1, (64, 96), (64, 96), labels=True)
    with pytest.raises(osr.OsrError):
        ops.semseg_resample(x, C, (64, 96), (0, 96), labels=True)


def _pad_to(logits, pitch, fill=1000.0):
    out = torch.full(tuple(logits.shape[:2]) + (pitch,), fill, dtype=logits.dtype)
    out[..., :logits.shape[2]] = logits
    return out.contiguous()


def _check_wide(ops, stored, c, pitch, crop, out_hw, what):
    """The file's rules on `stored` logits (h4, w4, c) of any storage type: the reference reads the stored values."""
    ref = resample_reference(stored.double(), crop, out_hw)
    scale = float(ref.abs().max())
    dev = _pad_to(stored, pitch).to(DEV)
    values = ops.semseg_resample(dev, c, crop, out_hw, labels=False)
    assert values.dtype == torch.float32 and tuple(values.shape) == (c,) + tuple(out_hw)
    err = float((values.cpu().double() - ref).abs().max())
    sure = top_two_gap(ref) >= 1e-4 * scale
    share = 1.0 - float(sure.double().mean())
    print(f"[resample] {what}: max err {err:.3e} = {err / scale:.3e} of max |ref| (bound 1e-4); {100 * share:.3f} % excluded as near ties")
    assert err <= 1e-4 * scale
    labels = ops.semseg_resample(dev, c, crop, out_hw, labels=True)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == tuple(out_hw)
    assert int(labels.min()) >= 0 and int(labels.max()) < c  # the padding channels hold 1000 and never win
    assert share <= 0.005
    assert torch.equal(labels.cpu()[sure].long(), ref.argmax(dim=0)[sure])
    assert torch.equal(ops.semseg_resample(dev, c, crop, out_hw, labels=True), labels)
    assert torch.equal(ops.semseg_resample(dev, c, crop, out_hw, labels=False), values)
    return ref


@pytest.mark.parametrize("case", RESAMPLE_WIDE_CASES, ids=[c[0] for c in RESAMPLE_WIDE_CASES])
def test_more_classes_than_one_pass_and_degenerate_maps(osr, case):
    name, c, pitch, _, crop, out_hw = case
    ref = _check_wide(osr.ops, resample_wide_logits(case), c, pitch, crop, out_hw, f"{name} C={c} fp32")
    if name in ("b", "c"):
        lab = ref.argmax(dim=0)
        assert float((lab >= 112).double().mean()) >= 0.10 and float((lab >= 56).double().mean()) >= 0.30


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", RESAMPLE_WIDE_CASES[:3], ids=[c[0] for c in RESAMPLE_WIDE_CASES[:3]])
def test_more_classes_than_one_pass_in_low_precision(osr, case, dtype):
    name, c, pitch, _, crop, out_hw = case
    _check_wide(osr.ops, resample_wide_logits(case).to(dtype), c, pitch, crop, out_hw, f"{name} C={c} {str(dtype)[6:]}")


@pytest.mark.parametrize("low,high", [(3, 100), (60, 120)])
def test_an_exact_tie_across_passes_goes_to_the_lower_class(osr, low, high):
    """The two classes lie in different 56-class passes: the carried `best` must not be replaced by an equal value of a later pass."""
    case = RESAMPLE_WIDE_CASES[1]
    _, c, pitch, _, crop, out_hw = case
    assert low // 56 != high // 56
    logits = resample_wide_logits(case)
    logits[..., high] = logits[..., low] = logits.max(dim=2).values + 1.0
    labels = osr.ops.semseg_resample(_pad_to(logits, pitch).to(DEV), c, crop, out_hw, labels=True)
    assert bool((labels == low).all()), torch.unique(labels).tolist()


def test_a_strong_downscale_with_three_times_56_classes(osr):
    """The geometry of test_a_strong_downscale_takes_the_untiled_path with C = 133: resample_direct loops over more than 56 classes."""
    torch.manual_seed(12)
    logits = torch.randn(6, 100, 133)
    ref = _check_wide(osr.ops, logits, 133, 136, (22, 397), (7, 70), "strong downscale C=133")
    assert float((ref.argmax(dim=0) >= 56).double().mean()) >= 0.30
