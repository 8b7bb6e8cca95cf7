"""The open-set evaluator's flag accumulation and osr_os_coco_match's refusals, without a GPU.

The flags are laid out by tests/os_coco_common.py from the numpy OpensetCOCOEval.evaluate() results, exactly as the kernel writes
them; OpensetCOCOEval.accumulate_from_flags must then give the arrays accumulate() gives from the per-image results, and the same
30 figures. The refusals need no device: every argument is validated before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from tests.os_coco_common import MAX_DETS, flat_detections, padded, reference_outputs, seeded_openset


@pytest.mark.parametrize("narrow", [False, True])
def test_flag_accumulation_equals_accumulate(osr, narrow):
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEval
    gt, image_ids, known_ids, reverse_map, dets = seeded_openset(5)
    assert len(image_ids) == 6 and len(gt["categories"]) == 5 and len(known_ids) == 3
    dets[3] = {k: v[:0] for k, v in dets[3].items()}  # an image without a detection
    processed = image_ids[:5]                          # the sixth image is never processed: its ground truths still count
    boxes, scores, classes, counts = padded(dets[:5])
    flags, rank, _, tb, _, ev1 = reference_outputs(osr, gt, known_ids, processed, boxes, scores, classes, counts, reverse_map)
    img_ids = [image_ids[0], image_ids[2], image_ids[5]] if narrow else None
    # the specification: evaluate() + accumulate() with every maxDets on the same records
    from tests.os_coco_common import records
    recs, _ = records(osr, processed, boxes, scores, classes, counts, reverse_map)
    ref = OpensetCOCOEval(gt, recs, known_ids, MAX_DETS, img_ids)
    ref.evaluate()
    ref.accumulate()
    ref.summarize()
    # the flag path
    ev = OpensetCOCOEval(dict(images=gt["images"], annotations=[]), [], known_ids, MAX_DETS, img_ids)
    image, slot, exists = flat_detections(ev, tb, processed, classes, counts, reverse_map)
    ev.accumulate_from_flags(image, slot, rank[exists], scores[exists], flags[exists], tb.npig(ev.area_rng, ev.img_ids))
    ev.summarize()
    assert (slot == -1).any() and (slot == 3).any() and (flags[..., 2] != 0).any() and (flags[..., 1] & 0xffff).any()  # the case holds what it claims
    for key, want in ref.eval_kdt.items():
        assert np.array_equal(ev.eval_kdt[key], want), key
    for key, want in ref.eval_unkdt.items():
        assert np.array_equal(ev.eval_unkdt[key], want), key
    assert list(ev.eval_kdt) == list(ref.eval_kdt) and list(ev.eval_unkdt) == list(ref.eval_unkdt)
    assert ref.stats.shape == (30,) and ev.stats.tobytes() == ref.stats.tobytes() and ev.k_det_as_unk == ref.k_det_as_unk
    assert (ref.eval_kdt["precision"] > 0).any() and (ref.eval_unkdt["precision"] > 0).any() and ref.eval_kdt["unk_det_as_known"].any()


def _call(lib, *, n=1, cap=8, L=4, K=2, num_gt=0, max_img=0, T=10, A=4, max_det=100):
    thrs, rng = (C.c_double * max(T, 1))(), (C.c_double * max(2 * A, 1))()
    return lib.osr_os_coco_match(None, None, None, None, n, cap, None, L, K, None, None, None, None, None, None, num_gt, max_img, thrs, T, rng, A, max_det,
                                 None, None, None, None, 0, None)


def test_every_limit_is_refused_without_a_gpu(osr):
    L = osr._lib
    lib = L.load()
    beyond = dict(cap=L.OS_COCO_MAX_CAP + 1, max_det=L.OS_COCO_MAX_DET + 1, T=L.OS_COCO_MAX_THRS + 1, A=L.OS_COCO_MAX_AREAS + 1, max_img=L.OS_COCO_MAX_GT + 1)
    assert beyond == dict(cap=1025, max_det=129, T=17, A=9, max_img=4097)
    for name, value in beyond.items():
        assert _call(lib, **{name: value}) == -2, name  # OSR_ERR_UNSUPPORTED
        assert b"osr_os_coco_match" in lib.osr_last_error(), name
    assert _call(lib, n=1 << 30, K=3) == -2 and b"osr_os_coco_match" in lib.osr_last_error()  # images x slots is no grid
    # at the limits the arguments pass this stage: the next refusal is the null pointers', still without a launch
    assert _call(lib, cap=1024, max_det=128, T=16, A=8, max_img=4096) == -1 and b"osr_os_coco_match: null pointer" in lib.osr_last_error()
    for bad in (dict(n=-1), dict(cap=-1), dict(L=0), dict(K=-1), dict(num_gt=-1), dict(max_det=0), dict(T=0), dict(A=0)):
        assert _call(lib, **bad) == -1 and b"osr_os_coco_match" in lib.osr_last_error(), bad
    assert _call(lib, n=0) == 0 and _call(lib, cap=0) == 0  # nothing to do: OSR_OK without a launch
    assert lib.osr_os_coco_match_workspace_bytes(100, 160) == 100 * 160 * 8 and lib.osr_os_coco_match_workspace_bytes(-1, 0) == -1
