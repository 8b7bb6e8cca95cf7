"""osr_proposal_recall against the specification (host/proposal_evaluation.py match_image), bit for bit and with nothing left out:
hits, num_pos and the overlap recorded at every ground truth, for the four area ranges and the limits 100 and 1000. The counts walk
the wave (63 / 64 / 65), the limits (99 / 100 / 101, 1000 / 1001), the block (257) and the capacity (2048); the ground truths walk
0, 1, 2, the wave, two passes of the 16 waves (130) and more ground truths than proposals. The references are computed once."""
import ctypes

import numpy as np
import pytest
import torch

from tests.proposal_common import AREAS, LIMITS, pad_batch, seeded_image, specification_outputs

DEV = "cuda:0"
COUNTS = (0, 1, 63, 64, 65, 99, 100, 101, 257, 1000, 1001, 2048)
GTS = (0, 1, 2, 64, 65, 130)
_cache = {}


def _case(name):
    """-> (images, padded batch arrays, the specification's (hits, num_pos, overlaps)), built once per name."""
    if name in _cache:
        return _cache[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "counts":      # every count of the issue, 7 ground truths each; cap 2048
        images, cap = [seeded_image(rng, k, 7) for k in COUNTS], 2048
    elif name == "gts":       # every ground-truth count on 100 proposals, and more ground truths than proposals (130 on 40, 65 on 1)
        images, cap = [seeded_image(rng, 100, g) for g in GTS] + [seeded_image(rng, 40, 130), seeded_image(rng, 1, 65), seeded_image(rng, 0, 3)], 128
    elif name == "copies":    # exact copies (IoU 1) of every ground truth among duplicates of them, and an image of disjoint boxes
        b, s, g, ar = seeded_image(rng, 60, 12)
        b[:24] = np.concatenate([g, g])
        far = seeded_image(rng, 30, 9)
        far[0][:, [0, 2]] += 5000.0
        images, cap = [(b, s, g, ar), far], 64
    elif name == "many":      # 40 small images: a grid of 320 workgroups, more than the device has compute units
        images, cap = [seeded_image(rng, int(rng.integers(1, 48)), int(rng.integers(0, 9))) for _ in range(40)], 48
    else:
        raise KeyError(name)
    batch = pad_batch(images, cap, rng)
    _cache[name] = (images, batch, specification_outputs(images))
    return _cache[name]


def _launch(osr, batch, want_overlaps=True):
    from openset_rcnn_amd.host import proposal_evaluation as PE
    boxes, logits, counts, gt_boxes, gt_area, seg_off = (torch.from_numpy(a).to(DEV) for a in batch)
    hits, num_pos, ov = osr.ops.proposal_recall(boxes, logits, counts, gt_boxes, gt_area, seg_off, int(np.diff(batch[5]).max()), PE.area_range_tensor(AREAS),
                                                LIMITS, PE.default_thresholds(), want_overlaps=want_overlaps)
    return hits.cpu().numpy(), num_pos.cpu().numpy(), None if ov is None else ov.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["counts", "gts", "copies", "many"])
def test_kernel_equals_the_specification_bit_for_bit(osr, name):
    images, batch, (w_hits, w_pos, w_ov) = _case(name)
    hits, num_pos, ov = _launch(osr, batch)
    assert np.array_equal(num_pos, w_pos)
    assert np.array_equal(ov.view(np.uint32), w_ov.view(np.uint32)), np.argwhere(ov != w_ov)[:8]
    assert np.array_equal(hits, w_hits)
    assert w_hits.sum() > 0 and (w_ov > 0).any()  # (the case scores something)
    if name == "copies":
        g = len(images[0][2])
        assert (w_ov[0, 1, :g] == 1.0).all() and (w_ov[0, 1, g:] == 0.0).all()  # every copy found; the far image scores zeros, and counts
    if name == "counts":
        assert (w_hits[:, 0, 0] != w_hits[:, 0, 1]).any()  # (the limit of 100 matters somewhere)
    # a second launch, without the overlaps: the same bits
    hits2, num_pos2, none = _launch(osr, batch, want_overlaps=False)
    assert none is None and np.array_equal(hits2, hits) and np.array_equal(num_pos2, num_pos)


@pytest.mark.gpu
def test_padding_rows_do_not_count(osr):
    images, batch, (w_hits, w_pos, _) = _case("gts")
    loud = [a.copy() for a in batch]
    for i, k in enumerate(batch[2]):
        loud[1][i, k:] = 100.0  # the rows past the count outrank everything and copy ground truths (pad_batch)
    hits, num_pos, _ = _launch(osr, loud, want_overlaps=False)
    assert np.array_equal(hits, w_hits) and np.array_equal(num_pos, w_pos)


def test_argument_validation_needs_no_gpu(osr):
    lib = osr._lib.load()
    f4, i4 = (ctypes.c_float * 8)(0, 1e10, 0, 1024, 0, 0, 0, 0), (ctypes.c_int32 * 2)(100, 1000)
    thr = (ctypes.c_float * 10)(*[0.5 + 0.05 * t for t in range(10)])
    fa = ctypes.cast(f4, ctypes.c_void_p)
    la, ta = ctypes.cast(i4, ctypes.c_void_p), ctypes.cast(thr, ctypes.c_void_p)
    call = lambda n=1, cap=8, ng=0, mg=0, ar=fa, a=2, lim=la, l=2, th=ta, t=10: lib.osr_proposal_recall(  # noqa: E731
        None, None, None, n, cap, None, None, None, ng, mg, ar, a, lim, l, th, t, None, None, None, None)
    assert call() == -1 and b"null pointer" in lib.osr_last_error()
    assert call(n=0) == 0  # nothing to do: no launch
    assert call(ar=None) == -1 and b"null pointer" in lib.osr_last_error()
    assert call(lim=None) == -1 and call(th=None) == -1
    for kw, word in ((dict(a=0), b"area ranges"), (dict(a=9), b"area ranges"), (dict(l=0), b"limits"), (dict(l=9), b"limits"), (dict(t=0), b"thresholds"),
                     (dict(t=17), b"thresholds"), (dict(n=-1), b"n -1")):
        assert call(**kw) == -1 and word in lib.osr_last_error(), kw
    zero = (ctypes.c_int32 * 2)(100, 0)
    assert call(lim=ctypes.cast(zero, ctypes.c_void_p)) == -1 and b"at least 1" in lib.osr_last_error()
    assert call(cap=2049) == -2 and b"at most 2048" in lib.osr_last_error()
    assert call(ng=2000, mg=1025) == -2 and b"at most 1024" in lib.osr_last_error()
    assert (osr._lib.PROPOSAL_MAX_CAP, osr._lib.PROPOSAL_MAX_GT) == (2048, 1024)
