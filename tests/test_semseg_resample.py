"""osr_semseg_resample (csrc/osr_semseg.hip) against detectron2's two interpolations in float64 (tests/panoptic_common.py): C = 54 in a
pitch of 56, (h4, w4) = (16, 24), crops that are no multiples of 4, an upscale, the identity and a downscale. Values within 1e-4 max |ref|;
labels equal wherever the reference's top-two gap is at least 1e-4 max |ref| (the excluded share is bounded in
tests/test_panoptic_reference.py and here); an exact tie goes to the lower class; padding channels never win."""
import pytest
import torch

from tests.panoptic_common import RESAMPLE_C as C, RESAMPLE_CASES, RESAMPLE_PITCH as PITCH, resample_logits, resample_reference, top_two_gap

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
