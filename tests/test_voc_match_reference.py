"""The open-set VOC evaluator's device path without a GPU: the record rounding formulas against the text round trip, and
voc_match_reference (the kernel's numpy specification) followed by accumulate_from_flags against PascalVOCDetectionEvaluator's numpy
path (voc_eval on the text records) fed the same detections as CPU tensors."""
import numpy as np

from tests.voc_eval_common import UNKNOWN, class_names, reference_chunks, run_evaluator, same_detail, same_results, seeded_voc

BATCHES = ((0, 16), (16, 23), (23, 40))


def test_rounding_formulas_equal_the_text_round_trip(osr):
    from openset_rcnn_amd.host.evaluation import voc_record_numbers
    rng = np.random.default_rng(0)
    ties = np.arange(1, 4001, 2, dtype=np.float64) / 4.0                     # v * 10 = n + 0.5 exactly: "{:.1f}" ties
    score_ties = np.arange(1, 16, 2, dtype=np.float64) / 16.0                # s * 1000 = n + 0.5 exactly: "{:.3f}" ties
    v = np.concatenate([ties, ties - 1.0, -ties, rng.uniform(-50, 1400, 6000), np.rint(rng.uniform(0, 1400, 3000) * 20) / 20,
                        [0.0, -0.0, 1e-8, -1e-8, 16777216.0, 33554430.0, 9e17, -0.04, -1.04, 0.05, -9e17]]).astype(np.float32)
    v = v[: len(v) // 4 * 4].reshape(-1, 4)
    s = np.concatenate([score_ties, -score_ties, rng.uniform(0, 1, 4000), rng.integers(0, 2001, 3000) / 2000.0, [0.0, -0.0, 1.0, 0.9995, 0.0005, 1e-9, 2147483.0]])
    s = np.resize(s.astype(np.float32), len(v))
    t, k, finite = voc_record_numbers(v, s)
    assert finite.all()
    for row, trow, score, kk in zip(v, t, s, k):
        x0, y0, x1, y1 = row  # np.float32 scalars, as process() meets them
        text = f"{float(score):.3f} {x0 + 1:.1f} {y0 + 1:.1f} {x1:.1f} {y1:.1f}".split(" ")
        assert [float(z) for z in text] == [kk / 1000.0] + (trow / 10.0).tolist(), (row, score)
    # what the formulas are for: half-even ties, and the + 1 rounded in fp32 before the text
    assert voc_record_numbers([[0.25, 0.75, 0.25, 0.75]], [0.0625])[0].tolist() == [[12.0, 18.0, 2.0, 8.0]]  # 1.25 -> 1.2, 1.75 -> 1.8, 0.25 -> 0.2, 0.75 -> 0.8
    assert voc_record_numbers([[0, 0, 0, 0]], [0.0625])[1].tolist() == [62.0] and voc_record_numbers([[0, 0, 0, 0]], [0.1875])[1].tolist() == [188.0]
    assert voc_record_numbers([[16777216.0, 1e-8, 0, 0]], [0.5])[0].tolist() == [[167772160.0, 10.0, 0.0, 0.0]]
    bad = voc_record_numbers([[0, 0, 1, np.inf], [0, 0, 1, 1], [np.nan, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1e30, 1]], [0.5, np.nan, 0.5, 3e6, 0.5])[2]
    assert bad.tolist() == [False] * 5


def _both(osr, seed, sort_kind, mutate=None):
    annos, ids, names, num_known, dets = seeded_voc(seed)
    if mutate:
        mutate(dets)
    ev, want, want_detail = run_evaluator(osr, annos, ids, names, num_known, dets, BATCHES, ["cpu"] * 3, sort_kind=sort_kind)
    chunks = reference_chunks(annos, ids, names, dets, BATCHES)
    got_detail = {}
    got = ev.accumulate_from_flags(chunks, detail=got_detail)
    return ev, chunks, want, want_detail, got, got_detail


def test_reference_and_accumulation_equal_the_numpy_path_with_stable_ties(osr):
    from openset_rcnn_amd.host.evaluation import VOC_FP, VOC_TP, VOC_UNK, VOC_VALID
    ev, chunks, want, want_detail, got, got_detail = _both(osr, 3, "stable")
    flags, milli = np.concatenate([c["flags"] for c in chunks]), np.concatenate([c["milli"] for c in chunks])
    # the set holds what it claims: every flag combination, rows of no class name's list are impossible here, rounded-score ties
    seen = set(flags.tolist())
    assert {VOC_VALID, VOC_VALID | VOC_TP, VOC_VALID | VOC_FP, VOC_VALID | VOC_UNK, VOC_VALID | VOC_TP | VOC_UNK, VOC_VALID | VOC_FP | VOC_UNK} <= seen, seen
    assert len(np.unique(milli)) < len(milli)
    assert list(want) == ["mAP", "WI", "AOSE", "AP@K", "P@K", "R@K", "AP@U", "P@U", "R@U"]
    assert 0 < want["AP@K"] < 100 and 0 < want["AP@U"] < 100 and want["AOSE"] > 0 and want["WI"] > 0
    assert same_results(got, want)
    assert same_detail(got_detail, want_detail)  # rec, prec, ap, A-OSE, tp + fp and open-set fp curves per class: the tp / fp / is_unk sequences
    for c in range(ev.num_known_classes):        # WI picks the same detection of every known class
        a, b = got_detail[c][0], want_detail[c][0]
        assert len(a) == len(b) and (len(a) == 0 or int(np.argmin(np.abs(a - 0.8))) == int(np.argmin(np.abs(b - 0.8))))


def test_without_rounded_ties_the_default_sort_agrees_too(osr):
    def untie(dets):
        total = sum(len(d["scores"]) for d in dets)
        assert total < 1999
        values = iter(np.random.default_rng(1).permutation(np.arange(1, 1999))[:total])
        for d in dets:
            d["scores"] = np.array([next(values) / 1000.0 for _ in d["scores"]], dtype=np.float32)
    ev, chunks, want, want_detail, got, got_detail = _both(osr, 5, None, untie)
    # ties across CLASSES do not matter, inside a class they would: there are none
    for c in range(ev.total_num_class):
        m = np.concatenate([ch["milli"][ch["classes"] == c] for ch in chunks])
        assert len(np.unique(m)) == len(m)
    assert same_results(got, want) and same_detail(got_detail, want_detail)


def test_two_ranks_of_chunks_accumulate_like_the_concatenated_stream(osr):
    ev, chunks, want, want_detail, got, got_detail = _both(osr, 3, "stable")
    one = [{k: np.concatenate([c[k] for c in chunks]) for k in ("classes", "flags", "milli")}]
    ranks = chunks[:2] + chunks[2:]  # rank 0's chunks, then rank 1's: the order the gathered records are concatenated in
    a, b = {}, {}
    assert same_results(ev.accumulate_from_flags(one, detail=a), want) and same_results(ev.accumulate_from_flags(ranks, detail=b), want)
    assert same_detail(a, b) and same_detail(a, want_detail)


def _single(dets_boxes, scores, classes, objs, names):
    from openset_rcnn_amd.host.evaluation import VocGroundTruthTable, voc_match_reference
    tb = VocGroundTruthTable({"a": objs}, ["a"], names)
    n = len(scores)
    return voc_match_reference(np.array(dets_boxes, dtype=np.float32).reshape(1, n, 4), np.array(scores, dtype=np.float32).reshape(1, n),
                               np.array(classes, dtype=np.int64).reshape(1, n), np.array([n], dtype=np.int32), np.array([0], dtype=np.int32), len(names),
                               tb.img_off, tb.box, tb.cls, tb.difficult)


def test_an_overlap_of_exactly_one_half_is_a_false_positive(osr):
    from openset_rcnn_amd.host.evaluation import VOC_FP, VOC_VALID, _overlaps
    names = class_names(1, 0)
    # record [1, 1, 10, 5] (the detection's corner is 0-based) on ground truth [1, 1, 10, 10]: 50 / 100
    assert _overlaps(np.array([[1.0, 1.0, 10.0, 10.0]]), np.array([1.0, 1.0, 10.0, 5.0]))[0] == 0.5
    flags, milli, match, deci, status = _single([[0, 0, 10, 5]], [0.9], [0], [dict(name=names[0], difficult=0, bbox=[1, 1, 10, 10])], names)
    assert flags.tolist() == [[VOC_VALID | VOC_FP]] and match.tolist() == [[-1]] and deci.tolist() == [[[10, 10, 100, 50]]] and milli.tolist() == [[900]]


def test_of_two_identical_ground_truths_the_first_is_taken_and_taken_again(osr):
    from openset_rcnn_amd.host.evaluation import VOC_FP, VOC_TP, VOC_UNK, VOC_VALID
    names = class_names(1, 0)
    objs = [dict(name=UNKNOWN, difficult=0, bbox=[200, 200, 240, 240]), dict(name=names[0], difficult=0, bbox=[11, 11, 60, 60]),
            dict(name=names[0], difficult=0, bbox=[11, 11, 60, 60])]
    flags, milli, match, deci, status = _single([[10, 10, 60, 60], [10, 10, 60, 60], [199, 199, 240, 240]], [0.5, 0.9, 0.7], [0, 0, 0], objs, names)
    # list order is 0.9, 0.7, 0.5: row 1 takes the FIRST of the equal maxima (entry 1), row 0 meets it taken; row 2 lies on the unknown object
    assert flags.tolist() == [[VOC_VALID | VOC_FP, VOC_VALID | VOC_TP, VOC_VALID | VOC_FP | VOC_UNK]]
    assert match.tolist() == [[1, 1, -1]] and status.tolist() == [0]
