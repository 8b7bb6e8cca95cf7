"""PascalVOCDetectionEvaluator end to end on the device: the seeded 40-image open-set VOC set with device predictions in three batches
of two different caps. The device path (osr_voc_match per batch, one copy, accumulation from the flags) must return what the same
evaluator returns for CPU copies through voc_eval with kind="stable", write the same files and leave the same records; whatever it
cannot score must come out as the unchanged numpy path's result, with the reason logged."""
import numpy as np
import pytest
import torch

from tests.voc_eval_common import instances, run_evaluator, same_detail, same_results, seeded_voc

DEV = "cuda:0"
BATCHES = ((0, 16), (16, 23), (23, 40))


@pytest.fixture(scope="module")
def stable_cpu(osr, tmp_path_factory):
    """The numpy path on CPU tensors with stable ties: computed once, read by the tests."""
    data = seeded_voc(3)
    for i in range(*BATCHES[1]):  # the middle batch's lists are short: cap 16 there, 32 in the other two
        data[4][i] = {k: v[:12] for k, v in data[4][i].items()}
    out = tmp_path_factory.mktemp("cpu")
    ev, res, detail = run_evaluator(osr, *data, BATCHES, ["cpu"] * 3, output_dir=str(out), sort_kind="stable")
    return data, out, ev, res, detail


def _files(d, names):
    return {name: (d / "pascal_voc_eval" / f"{name}.txt").read_bytes() for name in names}


@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True])
def test_device_predictions_score_like_cpu_copies_and_leave_the_same_records(osr, stable_cpu, tmp_path, plain):
    from openset_rcnn_amd.host.evaluation import PascalVOCDetectionEvaluator
    (annos, ids, names, num_known, dets), cpu_dir, cpu_ev, cpu_res, cpu_detail = stable_cpu
    ev = PascalVOCDetectionEvaluator("", "", names, num_known, output_dir=str(tmp_path), annotations=annos, image_ids=ids)
    for lo, hi in BATCHES:  # `plain`: the bare namespaces tests/trained_parity.py passes instead of Instances
        ev.process([dict(image_id=im) for im in ids[lo:hi]], [dict(instances=instances(osr, d, DEV, plain)) for d in dets[lo:hi]])
    # until evaluate() nothing but device tensors is kept: no record, no host copy of a detection
    chunks = [c for kind, c in ev._segments if kind == "device"]
    assert len(chunks) == len(ev._segments) == 3 and len({c["cap"] for c in chunks}) == 2 and ev._merged is None and ev._host_reason is None
    for c in chunks:
        assert "host" not in c and all(c[k].is_cuda for k in ("boxes", "scores", "classes", "flags", "milli", "status"))
        assert not any(isinstance(v, np.ndarray) for v in c.values())
    detail = {}
    res = ev.evaluate(detail=detail)
    assert 0 < cpu_res["AP@K"] < 100 and cpu_res["AOSE"] > 0 and cpu_res["WI"] > 0
    assert same_results(res, cpu_res) and same_detail(detail, cpu_detail)
    assert _files(tmp_path, names) == _files(cpu_dir, names)
    assert dict(ev._predictions) == dict(cpu_ev._predictions) and sum(len(v) for v in ev._predictions.values()) == sum(len(d["scores"]) for d in dets)


@pytest.mark.gpu
def test_records_are_rebuilt_on_first_access_without_an_output_dir(osr, stable_cpu):
    (annos, ids, names, num_known, dets), _, cpu_ev, cpu_res, _ = stable_cpu
    ev, res, _ = run_evaluator(osr, annos, ids, names, num_known, dets, BATCHES, [DEV] * 3)
    assert same_results(res, cpu_res) and ev._merged is None
    assert dict(ev._predictions) == dict(cpu_ev._predictions)


def _numpy_and_device(osr, data, batches, caplog, extra=None):
    """The same processing on CPU tensors (the unchanged numpy path, default tie order) and on the device -> both results, the device
    evaluator and the warnings it logged."""
    from openset_rcnn_amd.host.evaluation import PascalVOCDetectionEvaluator
    annos, ids, names, num_known, dets = data
    out = []
    for devices in (["cpu"] * len(batches), [DEV] * len(batches)):
        ev = PascalVOCDetectionEvaluator("", "", names, num_known, annotations=annos, image_ids=ids)
        with caplog.at_level("WARNING"):
            caplog.clear()
            for (lo, hi), device in zip(batches, devices):
                ev.process([dict(image_id=im) for im in ids[lo:hi]], [dict(instances=instances(osr, d, device)) for d in dets[lo:hi]])
            if extra:
                extra(ev, devices[0])
            out.append(ev.evaluate())
            messages = [r.getMessage() for r in caplog.records if "PascalVOCDetectionEvaluator" in r.getMessage()]
    return out[0], out[1], ev, messages


@pytest.mark.gpu
def test_mixed_input_goes_through_the_numpy_path(osr, stable_cpu, caplog):
    data = stable_cpu[0]
    want = run_evaluator(osr, *data, BATCHES, ["cpu"] * 3)[1]
    with caplog.at_level("WARNING"):
        caplog.clear()
        ev, got, _ = run_evaluator(osr, *data, BATCHES, [DEV, "cpu", DEV])
    messages = [r.getMessage() for r in caplog.records]
    assert same_results(got, want) and len(messages) == 1 and "CPU and device input were mixed" in messages[0]
    assert [kind for kind, _ in ev._segments] == ["device", "host", "device"]


@pytest.mark.gpu
def test_an_unknown_image_id_and_an_image_processed_twice(osr, stable_cpu, caplog):
    data = stable_cpu[0]
    annos, ids, names, num_known, dets = data
    empty = {k: v[:0] for k, v in dets[0].items()}

    def stranger(ev, device):  # (an image the annotations do not hold can only be scored without detections: voc_eval looks every one up)
        ev.process([dict(image_id="nowhere")], [dict(instances=instances(osr, empty, device))])
    want, got, ev, messages = _numpy_and_device(osr, data, BATCHES, caplog, stranger)
    assert same_results(got, want) and len(messages) == 1 and "'nowhere' is not in the annotations" in messages[0]

    def again(ev, device):
        ev.process([dict(image_id=im) for im in ids[2:4]], [dict(instances=instances(osr, d, device)) for d in dets[2:4]])
    want, got, ev, messages = _numpy_and_device(osr, data, BATCHES, caplog, again)
    assert same_results(got, want) and len(messages) == 1 and f"{ids[2]!r} was processed twice" in messages[0]
    assert not same_results(want, stable_cpu[3])  # the second visit changed the figures, so the comparison says something


@pytest.mark.gpu
def test_a_list_of_1025_and_an_injected_nan(osr, stable_cpu, caplog):
    annos, ids, names, num_known, dets = stable_cpu[0]
    long = list(dets)
    long[17] = {k: np.resize(v, (1025,) + v.shape[1:]) for k, v in dets[20].items()}
    want, got, ev, messages = _numpy_and_device(osr, (annos, ids, names, num_known, long), BATCHES, caplog)
    assert same_results(got, want) and len(messages) == 1 and "1025 detections in one image" in messages[0]
    assert [kind for kind, _ in ev._segments] == ["device", "host", "host"]  # once a reason is known, the later batches are not matched either
    poisoned, j = list(dets), next(i for i in range(23, 40) if len(dets[i]["scores"]) > 1)
    poisoned[j] = dict(dets[j], scores=dets[j]["scores"].copy())
    poisoned[j]["scores"][1] = np.nan
    want, got, ev, messages = _numpy_and_device(osr, (annos, ids, names, num_known, poisoned), BATCHES, caplog)
    assert same_results(got, want) and len(messages) == 1 and "non-finite" in messages[0]
    assert [kind for kind, _ in ev._segments] == ["device"] * 3 and torch.cuda.is_available()
