"""osr_voc_match (csrc/osr_voc_eval.hip) against voc_match_reference, the numpy specification: flags, milli, match, deci and status
bit for bit with nothing left out. The shapes are the smallest that reach every path: a cap that is no multiple of a wave, a class
list longer than a wave and than one pass of the workgroup, a class with more ground truths than a wave has lanes, a full list of
1024, empty lists and images, classes and image indices outside their ranges, one class name and eighty-one."""
import ctypes

import numpy as np
import pytest

from tests.voc_eval_common import UNKNOWN, class_names, device_match, padded, seeded_voc, table_of

DEV = "cuda:0"
NAMES = ("flags", "milli", "match", "deci", "status")


def _reference(lists, index, C, tb, ovthresh=0.5):
    from openset_rcnn_amd.host.evaluation import voc_match_reference
    return voc_match_reference(*lists, index, C, tb.img_off, tb.box, tb.cls, tb.difficult, ovthresh)


def _check(osr, lists, index, C, tb):
    want = _reference(lists, index, C, tb)
    got = device_match(osr, DEV, lists, index, C, tb)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    return got


def seeded_case():
    """n = 3 at cap 72: an image with detections and objects, one with an empty list, one without ground truth; classes -1 and C."""
    annos, ids, names, _, dets = seeded_voc(3, num_images=12, max_dets=70)
    pick = [0, 1, 4]  # (image 4 has no object)
    assert not annos[ids[4]] and all(annos[ids[i]] for i in pick[:2])
    dets = [dict(dets[i]) for i in pick]
    dets[1] = {k: v[:0] for k, v in dets[1].items()}
    dets[2] = dict(dets[0])  # detections on the image without ground truth
    dets[0]["classes"] = dets[0]["classes"].copy()
    dets[0]["classes"][[3, 5]] = [-1, len(names)]
    tb = table_of(annos, ids, names)
    return padded(dets, 72), np.array(pick, dtype=np.int32), len(names), tb


@pytest.fixture(scope="module")
def seeded_ref(osr):
    lists, index, C, tb = seeded_case()
    return lists, index, C, tb, _reference(lists, index, C, tb)


@pytest.mark.gpu
def test_seeded_batch_equals_the_specification(osr, seeded_ref):
    from openset_rcnn_amd.host.evaluation import VOC_FP, VOC_TP, VOC_VALID
    lists, index, C, tb, want = seeded_ref
    counts = lists[3]
    assert counts.tolist()[1] == 0 and 8 < counts[0] < 72 and (want[0][2] == (VOC_VALID | VOC_FP)).sum() == counts[2]  # no ground truth: all fp
    assert want[0][0, 3] == 0 and want[0][0, 5] == 0 and (want[0][0, : counts[0]] & VOC_TP).any() and (want[0][:, 70:] == 0).all()
    got = device_match(osr, DEV, lists, index, C, tb)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.mark.gpu
def test_every_flag_combination_on_the_forty_image_set(osr):
    from openset_rcnn_amd.host.evaluation import VOC_FP, VOC_TP, VOC_UNK, VOC_VALID
    annos, ids, names, _, dets = seeded_voc(3)
    tb = table_of(annos, ids, names)
    flags = _check(osr, padded(dets, 32), np.arange(len(ids), dtype=np.int32), len(names), tb)[0]
    seen = set(flags.reshape(-1).tolist())  # difficult (valid alone), tp, fp (no overlap, or a duplicate), each with and without an unknown object under it
    assert {0, VOC_VALID, VOC_VALID | VOC_TP, VOC_VALID | VOC_FP, VOC_VALID | VOC_UNK, VOC_VALID | VOC_TP | VOC_UNK, VOC_VALID | VOC_FP | VOC_UNK} <= seen, seen


@pytest.mark.gpu
def test_repeats_are_bit_identical(osr, seeded_ref):
    lists, index, C, tb, _ = seeded_ref
    a, b = device_match(osr, DEV, lists, index, C, tb), device_match(osr, DEV, lists, index, C, tb)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _one_image(rng, names, gt_classes, gt_boxes, m, det_class, difficult=None):
    """One image: the given objects, and m detections of one class on jittered copies of them with scores on a coarse grid (ties)."""
    objs = [dict(name=names[c], difficult=int(difficult[j]) if difficult is not None else 0, bbox=[int(v) for v in b]) for j, (c, b) in enumerate(zip(gt_classes, gt_boxes))]
    src = rng.integers(0, len(objs), size=m)
    boxes = np.array([objs[s]["bbox"] for s in src], dtype=np.float64) - [1, 1, 0, 0] + rng.choice([0.0, 1.5, 30.0], size=(m, 1)) * rng.uniform(-1, 1, size=(m, 4))
    boxes = (np.rint(boxes * 20.0) / 20.0).astype(np.float32)
    scores = (rng.integers(1, 200, size=m) / 200.0).astype(np.float32)
    return {"a": objs}, dict(boxes=boxes, scores=scores, classes=np.full(m, det_class, dtype=np.int64))


@pytest.mark.gpu
def test_a_class_list_of_300_and_a_full_list_of_1024(osr):
    from openset_rcnn_amd.host.evaluation import VOC_FP, VOC_TP, VOC_UNK
    rng = np.random.default_rng(5)
    names = class_names(2, 0)
    g = np.array([[10, 10, 60, 80], [100, 40, 180, 120], [100, 40, 180, 120], [200, 150, 260, 199], [30, 120, 90, 190]])
    annos, d = _one_image(rng, names, [0, 0, 2, 0, 2], g, 300, 0, difficult=[0, 0, 0, 1, 0])
    tb = table_of(annos, ["a"], names)
    flags, milli, match, _, _ = _check(osr, padded([d], 304), np.zeros(1, dtype=np.int32), len(names), tb)
    live = flags[0, :300]
    assert ((live & VOC_TP) != 0).sum() == 2 and ((live & VOC_FP) != 0).sum() > 100 and ((live & VOC_UNK) != 0).sum() > 30 and (live == 1).any() and (flags[0, 300:] == 0).all()
    assert len(np.unique(milli[0, :300])) < 200  # rounded scores tie inside the one list
    annos, d = _one_image(rng, names, [0, 1, 2, 1, 0], g, 1024, 1)
    d["classes"][rng.permutation(1024)[:300]] = 0  # two lists that share the 1024 rows
    short = {k: v[:5] for k, v in d.items()}
    tb = table_of(annos, ["a"], names)
    flags = _check(osr, padded([d, short], 1024), np.zeros(2, dtype=np.int32), len(names), tb)[0]
    assert (flags[0] & 1).all() and (flags[1, :5] & 1).all() and (flags[1, 5:] == 0).all()


@pytest.mark.gpu
def test_seventy_ground_truths_of_one_class_with_equal_overlaps(osr):
    rng = np.random.default_rng(6)
    names = class_names(2, 0)
    x0, y0 = rng.integers(1, 400, size=70), rng.integers(1, 300, size=70)
    g = np.stack([x0, y0, x0 + rng.integers(10, 90, size=70), y0 + rng.integers(10, 90, size=70)], axis=1)
    g[64:70] = g[3:9]    # the same boxes on both sides of lane 63: the FIRST maximum is the lower entry
    cls = [0] * 70
    other = np.stack([x0[:20] + 3, y0[:20] + 2, x0[:20] + 50, y0[:20] + 60], axis=1)  # interleaved objects of the other classes
    order = rng.permutation(90)
    boxes, classes = np.concatenate([g, other])[order], np.array(cls + [1] * 10 + [2] * 10)[order]
    annos, d = _one_image(rng, names, classes, boxes, 120, 0)
    d["boxes"][:12] = (boxes[np.flatnonzero(classes == 0)[-12:]] - [1, 1, 0, 0]).astype(np.float32)  # exact hits on the LAST entries of the class
    tb = table_of(annos, ["a"], names)
    flags, _, match, _, _ = _check(osr, padded([d], 120), np.zeros(1, dtype=np.int32), len(names), tb)
    assert (match[0] >= 64).any() and (match[0] >= 0).sum() > 40 and set(tb.cls[match[0][match[0] >= 0]].tolist()) == {0}


@pytest.mark.gpu
@pytest.mark.parametrize("num_known,num_unseen", [(0, 0), (20, 60)])
def test_one_class_name_and_eighty_one(osr, num_known, num_unseen):
    annos, ids, names, _, dets = seeded_voc(9, num_images=6, num_known=max(num_known, 1), num_unseen=num_unseen)
    if num_known == 0:  # only "unknown": every object and every detection is of class 0
        names = [UNKNOWN]
        annos = {im: [dict(o, name=UNKNOWN) for o in objs] for im, objs in annos.items()}
        dets = [dict(d, classes=np.zeros_like(d["classes"])) for d in dets]
    assert len(names) == (1 if num_known == 0 else 81)
    tb = table_of(annos, ids, names)
    flags = _check(osr, padded(dets, 32), np.arange(6, dtype=np.int32), len(names), tb)[0]
    assert (flags & 2).any() and (flags & 4).any() and ((flags & 8) != 0).any() == (num_known > 0)


@pytest.mark.gpu
def test_an_image_index_outside_the_table_and_non_finite_rows(osr, seeded_ref):
    from openset_rcnn_amd.host.evaluation import VOC_NONFINITE, VOC_VALID
    lists, index, C, tb, clean = seeded_ref
    for bad in (-1, len(tb.img_off) - 1):
        outside = index.copy()
        outside[0] = bad
        got = _check(osr, lists, outside, C, tb)
        assert (got[0][0] == 0).all() and (got[2][0] == -1).all() and got[4][0] == 0
        assert all(np.array_equal(g[1:], w[1:]) for g, w in zip(got[:4], clean[:4]))  # the other images: as in the clean call
    boxes, scores, classes, counts = (a.copy() for a in lists)
    rows = np.flatnonzero((classes[0, : counts[0]] >= 0) & (classes[0, : counts[0]] < C))[:2]
    scores[0, rows[0]], boxes[0, rows[1], 2] = np.nan, np.inf
    got = _check(osr, (boxes, scores, classes, counts), index, C, tb)
    assert got[4][0] == 1 and (got[0][0, rows] == (VOC_VALID | VOC_NONFINITE)).all() and not (got[0][1:] & VOC_NONFINITE).any()
    assert all(np.array_equal(g[1:], w[1:]) for g, w in zip(got[:4], clean[:4])) and clean[4][0] == 0


def _call(lib, n=1, cap=8, C=5, num_images=3, num_gt=4, max_img=4, ptr=None):
    return lib.osr_voc_match(ptr, ptr, ptr, ptr, ptr, n, cap, C, ptr, num_images, ptr, ptr, ptr, num_gt, max_img, 0.5, ptr, ptr, ptr, ptr, ptr, None)


def test_refusals_need_no_gpu_and_write_nothing(osr):
    lib = osr._lib.load()
    L = osr._lib
    canary = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))  # every pointer of a refused call points here: a written byte would show
    ptr = ctypes.cast(canary, ctypes.c_void_p)
    for bad in (dict(cap=L.VOC_MAX_CAP + 1), dict(max_img=L.VOC_MAX_GT + 1), dict(C=0), dict(n=1 << 26, C=64)):
        assert _call(lib, ptr=ptr, **bad) == L.ERR_UNSUPPORTED and b"osr_voc_match" in lib.osr_last_error(), bad
    for bad in (dict(n=-1), dict(cap=-1), dict(num_images=-1), dict(num_gt=-1), dict(max_img=-1)):
        assert _call(lib, ptr=ptr, **bad) == -1 and b"osr_voc_match" in lib.osr_last_error(), bad
    assert bytes(canary) == b"\xa5" * 4096
    assert _call(lib, cap=L.VOC_MAX_CAP, max_img=L.VOC_MAX_GT, C=81) == -1 and b"osr_voc_match: null pointer" in lib.osr_last_error()  # at the limits: accepted so far
    assert _call(lib, n=0) == 0 and _call(lib, cap=0) == 0  # nothing to do: no launch, no pointer needed
