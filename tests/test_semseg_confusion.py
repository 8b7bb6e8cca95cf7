"""osr_semseg_confusion (csrc/osr_seg_eval.hip) against np.bincount (tests/seg_eval_common.py): exact integer equality, in label
and value mode, on both sides of the LDS-histogram limit (C <= 126), with and without the 4-pixel vector path (37 x 53 is odd,
300 x 500 a multiple of 4 that spans several workgroups with a width that is no multiple of 16)."""
import numpy as np
import pytest
import torch

from tests.seg_eval_common import argmax_lowest, blocky, confusion_reference

DEV = "cuda:0"
IGNORE = 255
SHAPES = [(37, 53), (300, 500)]
CLASSES = [1, 19, 54, 126, 127, 255]


def _maps(h, w, c, seed):
    rng = np.random.default_rng(seed)
    labels = blocky(rng, h, w, c, cell=5)
    gt = blocky(rng, h, w, c, cell=7)
    gt[rng.random((h, w)) < 0.1] = IGNORE  # (at C = 255 the value 255 is the ignore label, not class 255)
    return labels, gt.astype(np.uint8)


def _values_for(labels, c, rng):
    """(C, h, w) fp32 whose argmax is `labels`: small integers (exact in fp32, full of ties below the top) and a top at the label."""
    v = rng.integers(-3, 3, size=(c,) + labels.shape).astype(np.float32)
    np.put_along_axis(v, labels[None], 7.0, axis=0)
    return v


def _run(osr, pred, gt, c, ignore=IGNORE, conf=None, invalid=None):
    conf = torch.zeros((c + 1, c + 1), dtype=torch.int64, device=DEV) if conf is None else conf
    invalid = torch.zeros((1,), dtype=torch.int64, device=DEV) if invalid is None else invalid
    pred = torch.from_numpy(pred).to(DEV)
    osr.ops.semseg_confusion(pred, torch.from_numpy(gt).to(DEV), c, ignore, conf, invalid)
    return conf, invalid


@pytest.mark.gpu
@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_label_mode_equals_bincount(osr, h, w, c):
    labels, gt = _maps(h, w, c, seed=c)
    ref, bad = confusion_reference(labels, gt, c, IGNORE)
    conf, invalid = _run(osr, labels.astype(np.int32), gt, c)
    assert bad == 0 and int(invalid[0]) == 0
    assert ref[:, c].sum() > 0 or c == 1
    assert np.array_equal(conf.cpu().numpy(), ref)
    again, _ = _run(osr, labels.astype(np.int32), gt, c)
    assert torch.equal(again, conf)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_value_mode_fuses_the_argmax(osr, h, w, c):
    labels, gt = _maps(h, w, c, seed=100 + c)
    values = _values_for(labels, c, np.random.default_rng(c))
    assert np.array_equal(argmax_lowest(values), labels)
    ref, _ = confusion_reference(labels, gt, c, IGNORE)
    conf, invalid = _run(osr, values, gt, c)
    assert int(invalid[0]) == 0 and np.array_equal(conf.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SHAPES)
def test_exact_ties_go_to_the_lowest_class(osr, h, w):
    c = 54
    rng = np.random.default_rng(5)
    values = rng.integers(0, 2, size=(c, h, w)).astype(np.float32)  # only 0 and 1: every pixel's top is shared by many classes
    values[:, 0, 0] = 0.0  # all equal: class 0
    labels = argmax_lowest(values)
    assert (values == values.max(axis=0)).sum(axis=0).min() >= 2
    _, gt = _maps(h, w, c, seed=6)
    ref, _ = confusion_reference(labels, gt, c, IGNORE)
    conf, _ = _run(osr, values, gt, c)
    assert np.array_equal(conf.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [54, 200])
def test_out_of_range_values_land_in_invalid_only(osr, c):
    h, w = 37, 53
    labels, gt = _maps(h, w, c, seed=9)
    gt[3, 4:9] = 200 if c == 54 else 230  # a ground-truth value in [C, 255] that is not the ignore label
    gt[5, 5] = c                          # (C itself is out of range too: column C is reserved for the ignore label)
    labels = labels.astype(np.int32)
    labels[10, 10], labels[11, 11] = -1, c
    ref, bad = confusion_reference(labels, gt, c, IGNORE)
    conf, invalid = _run(osr, labels, gt, c)
    assert bad == 8 and int(invalid[0]) == 8
    assert np.array_equal(conf.cpu().numpy(), ref) and int(conf.sum()) == h * w - 8


@pytest.mark.gpu
def test_an_ignore_value_below_c_takes_its_pixels_out(osr):
    c, h, w = 19, 37, 53
    labels, gt = _maps(h, w, c, seed=11)
    gt[gt == IGNORE] = 3
    ref, bad = confusion_reference(labels, gt, c, 3)
    conf, invalid = _run(osr, labels.astype(np.int32), gt, c, ignore=3)
    assert bad == 0 and int(invalid[0]) == 0 and ref[:, 3].sum() == 0 and ref[:, c].sum() > 0
    assert np.array_equal(conf.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [54, 255])
def test_one_pixel_image(osr, c):
    conf, invalid = _run(osr, np.array([[2 % c]], dtype=np.int32), np.array([[1 % c]], dtype=np.uint8), c)
    ref = np.zeros((c + 1, c + 1), dtype=np.int64)
    ref[2 % c, 1 % c] = 1
    assert np.array_equal(conf.cpu().numpy(), ref) and int(invalid[0]) == 0
    conf, _ = _run(osr, np.zeros((c, 1, 1), dtype=np.float32), np.array([[IGNORE]], dtype=np.uint8), c)
    assert int(conf[0, c]) == 1 and int(conf.sum()) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("c", [54, 255])
def test_two_calls_accumulate_into_one_matrix(osr, c):
    (la, ga), (lb, gb) = _maps(37, 53, c, seed=1), _maps(300, 500, c, seed=2)
    gb[0, 0] = 254 if c < 254 else gb[0, 0]
    conf, invalid = _run(osr, la.astype(np.int32), ga, c)
    _run(osr, lb.astype(np.int32), gb, c, conf=conf, invalid=invalid)
    (ra, ba), (rb, bb) = confusion_reference(la, ga, c, IGNORE), confusion_reference(lb, gb, c, IGNORE)
    assert np.array_equal(conf.cpu().numpy(), ra + rb) and int(invalid[0]) == ba + bb


@pytest.mark.gpu
@pytest.mark.parametrize("c", [54, 255])
@pytest.mark.parametrize("h,w", SHAPES)
def test_no_runs_and_one_run(osr, h, w, c):
    """Every pixel differs from both neighbours a thread visits next (its own next pixel is 256 or 1024 further on), and a constant map."""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    labels = ((idx + idx // 256 + idx // 1024) % c).astype(np.int32)
    gt = ((idx * 7 + idx // 256) % c).astype(np.uint8)
    conf, _ = _run(osr, labels, gt, c)
    assert np.array_equal(conf.cpu().numpy(), confusion_reference(labels, gt, c, IGNORE)[0])
    labels[:], gt[:] = c - 1, c // 2
    conf, _ = _run(osr, labels, gt, c)
    assert int(conf[c - 1, c // 2]) == h * w and int(conf.sum()) == h * w


def test_arguments_are_validated_without_a_gpu(osr):
    lib = osr._lib.load()
    one = (torch.zeros(8, dtype=torch.int64).data_ptr(),) * 4
    assert lib.osr_semseg_confusion(None, 0, None, 4, 4, 19, 255, None, None, None) == -1 and b"null pointer" in lib.osr_last_error()
    for c in (0, 256):
        assert lib.osr_semseg_confusion(one[0], 0, one[1], 4, 4, c, 255, one[2], one[3], None) == -1 and b"classes" in lib.osr_last_error()
    assert lib.osr_semseg_confusion(one[0], 2, one[1], 4, 4, 19, 255, one[2], one[3], None) == -1 and b"mode" in lib.osr_last_error()
    assert lib.osr_semseg_confusion(one[0], 0, one[1], 32768, 32769, 19, 255, one[2], one[3], None) == -1 and b"map" in lib.osr_last_error()
    with pytest.raises(osr.OsrError):
        osr.ops.semseg_confusion(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8), 19, 255, torch.zeros(20, 20, dtype=torch.int64),
                                 torch.zeros(1, dtype=torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(1100, 1000), (1099, 1001)], ids=["vector", "scalar"])
def test_a_workgroup_chunk_of_more_than_1024_pixels(osr, h, w):
    """se_chunk gives a workgroup 1024 pixels until the plane exceeds 4 * CUs * 1024 of them: 1 048 576 with 256 CUs. 1100 x 1000 (a
    multiple of 4: the vector path) and 1099 x 1001 (the scalar path) lie above that: the chunk is 2048, a block's first pixel is no
    longer blockIdx.x * 1024 and a thread takes a second step. On a device with more than 268 CUs these planes stop reaching
    chunk > 1024; the comparison still holds there."""
    c = 54
    assert h * w > 4 * 256 * 1024 and (h * w % 4 == 0) == (h == 1100)
    labels, gt = _maps(h, w, c, seed=21)
    ref, bad = confusion_reference(labels, gt, c, IGNORE)
    conf, invalid = _run(osr, labels.astype(np.int32), gt, c)
    assert bad == 0 and int(invalid[0]) == 0 and ref[:, c].sum() > 0
    assert np.array_equal(conf.cpu().numpy(), ref)
    again, _ = _run(osr, labels.astype(np.int32), gt, c)
    assert torch.equal(again, conf)
