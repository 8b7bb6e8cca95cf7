"""SemSegEvaluator, COCOPanopticEvaluator, DatasetEvaluators and the dataset registration behind them (host/seg_evaluation.py,
host/datasets.py). CPU: the final arithmetic on hand-written statistics, the registration of a three-image dataset written with PIL,
the rank merge. GPU: the same dataset through inference_on_dataset with a stub model, and the seeded PanopticFPN of
configs/panoptic_fpn.yaml on two images; every figure is compared with the numpy pipeline of tests/seg_eval_common.py."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.seg_eval_common import (PQReference, argmax_lowest, blocky, confusion_reference, ids_to_rgb, pair_counts_reference, pq_figures,
                                   sem_seg_figures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "panoptic_fpn.yaml"))
    cfg.merge_from_list(list(opts))
    return cfg


# ---- a synthetic panoptic dataset on disk ---------------------------------------------------------------------------------------------
def make_dataset(root, name, sizes, thing_ids, stuff_ids, seed, segments=9, coco_split=None):
    """Writes images, panoptic PNGs + JSON, semantic PNGs and an instances JSON in detectron2's "separated" format, registers it and
    returns what the reference pipeline needs: per image the id map, the segments (JSON order) and the semantic ground truth.
    coco_split "val": under detectron2's directory names below <root>/coco instead, and not registered (run_net.py does that)."""
    from openset_rcnn_amd.host import datasets as D
    rng = np.random.default_rng(seed)
    root = str(root)
    dirs = dict(images="images", panoptic="panoptic", sem="sem", pj="panoptic.json", ij="instances.json")
    if coco_split:
        root = os.path.join(root, "coco")
        os.makedirs(os.path.join(root, "annotations"))
        dirs = dict(images=f"{coco_split}2017", panoptic=f"panoptic_{coco_split}2017", sem=f"panoptic_stuff_{coco_split}2017",
                    pj=f"annotations/panoptic_{coco_split}2017.json", ij=f"annotations/instances_{coco_split}2017.json")
    for d in ("images", "panoptic", "sem"):
        os.makedirs(os.path.join(root, dirs[d]), exist_ok=True)
    cats = [dict(id=i, name=f"thing{i}", isthing=1) for i in thing_ids] + [dict(id=i, name=f"stuff{i}", isthing=0) for i in stuff_ids]
    rng.shuffle(cats)  # (the JSON need not list them in id order)
    stuff_contig = {i: k + 1 for k, i in enumerate(sorted(stuff_ids))}
    images, anns, inst, truth = [], [], [], []
    for n, (h, w) in enumerate(sizes):
        image_id, stem = 100 + 7 * n, f"im{n:03d}"
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, dirs["images"], stem + ".jpg"))
        seg_ids = [0] + sorted({int(v) for v in rng.integers(1, 1 << 24, size=segments)})
        ids_map = np.array(seg_ids, dtype=np.int64)[blocky(rng, h, w, len(seg_ids), cell=11)]
        segs = []
        for sid in seg_ids[1:]:
            cat = int(rng.choice(thing_ids + stuff_ids))
            area = int((ids_map == sid).sum())
            if area:
                segs.append(dict(id=sid, category_id=cat, area=area, iscrowd=int(cat in thing_ids and rng.random() < 0.3)))
        rng.shuffle(segs)
        sem = np.full((h, w), 255, dtype=np.uint8)
        for s in segs:
            sem[ids_map == s["id"]] = 0 if s["category_id"] in thing_ids else stuff_contig[s["category_id"]]
        Image.fromarray(ids_to_rgb(ids_map)).save(os.path.join(root, dirs["panoptic"], stem + ".png"))
        Image.fromarray(sem).save(os.path.join(root, dirs["sem"], stem + ".png"))
        images.append(dict(id=image_id, file_name=stem + ".jpg", height=h, width=w))
        anns.append(dict(image_id=image_id, file_name=stem + ".png", segments_info=segs))
        for s in segs:
            if s["category_id"] in thing_ids:
                ys, xs = np.nonzero(ids_map == s["id"])
                inst.append(dict(id=len(inst) + 1, image_id=image_id, category_id=s["category_id"], iscrowd=s["iscrowd"], area=s["area"],
                                 bbox=[int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]))
        truth.append(dict(image_id=image_id, ids_map=ids_map, segs=segs, sem=sem))
    pj, ij = os.path.join(root, dirs["pj"]), os.path.join(root, dirs["ij"])
    with open(pj, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=cats), f)
    with open(ij, "w") as f:
        json.dump(dict(images=images, annotations=inst, categories=[dict(id=i, name=f"thing{i}") for i in thing_ids]), f)
    if not coco_split:
        D.register_coco_panoptic_separated(name, os.path.join(root, "images"), os.path.join(root, "panoptic"), pj, os.path.join(root, "sem"), ij)
    return truth


def predictions_for(truth, thing_ids, stuff_ids, seed):
    """Per image a prediction near the ground truth: the id map shifted by one pixel, ids renumbered 1 .. n, a few categories
    changed; semantic values whose argmax is the shifted semantic map with some noise. Host arrays, model-side (contiguous) ids."""
    rng = np.random.default_rng(seed)
    things, stuff = sorted(thing_ids), sorted(stuff_ids)
    c = len(stuff) + 1
    out = []
    for t in truth:
        shifted = np.roll(t["ids_map"], (1, 1), axis=(0, 1))
        kept = [s for s in t["segs"] if (shifted == s["id"]).any()]
        rng.shuffle(kept)
        pan, info = np.zeros(shifted.shape, dtype=np.int32), []
        for k, s in enumerate(kept):
            pan[shifted == s["id"]] = k + 1
            cat = s["category_id"] if rng.random() < 0.8 else int(rng.choice(thing_ids + stuff_ids))
            isthing = cat in things
            info.append(dict(id=k + 1, isthing=isthing, category_id=things.index(cat) if isthing else stuff.index(cat) + 1))
        labels = np.roll(t["sem"], (1, 2), axis=(0, 1)).astype(np.int64)
        labels[labels == 255] = 0
        noise = rng.random(labels.shape) < 0.1
        labels[noise] = rng.integers(0, c, size=int(noise.sum()))
        values = rng.integers(-3, 3, size=(c,) + labels.shape).astype(np.float32)
        np.put_along_axis(values, labels[None], 5.0, axis=0)
        out.append(dict(sem_seg=values, pan=pan, info=info))
    return out


def reference_results(truth, preds, thing_ids, stuff_ids, ignore=255):
    """The whole pipeline in numpy: confusion matrix and PQ statistics image by image, then the figures."""
    things, stuff = sorted(thing_ids), sorted(stuff_ids)
    cats = sorted(thing_ids + stuff_ids)
    c = len(stuff) + 1
    conf = np.zeros((c + 1, c + 1), dtype=np.int64)
    pq = PQReference(len(cats))
    for t, p in zip(truth, preds):
        values = p["sem_seg"]
        m, bad = confusion_reference(argmax_lowest(values) if values.ndim == 3 else values, t["sem"], c, ignore)
        assert bad == 0
        conf += m
        if p.get("pan") is None:
            continue
        last_crowd = {}
        for s in t["segs"]:
            if s["iscrowd"]:
                last_crowd[s["category_id"]] = s["id"]
        segs = sorted(t["segs"], key=lambda s: s["id"])
        meta = np.array([[cats.index(s["category_id"]), s["iscrowd"], s["area"], int(last_crowd.get(s["category_id"]) == s["id"])] for s in segs],
                        dtype=np.int32).reshape(-1, 4)
        slots = [-1] * len(p["info"])
        for s in p["info"]:
            slots[s["id"] - 1] = cats.index(things[s["category_id"]] if s["isthing"] else stuff[s["category_id"] - 1])
        table, bad = pair_counts_reference(ids_to_rgb(t["ids_map"]), [s["id"] for s in segs], p["pan"], len(slots))
        assert bad == 0
        pq.add(table, meta, slots)
    assert pq.flags.tolist() == [0, 0, 0]
    names = ["things"] + [f"stuff{i}" for i in stuff]
    return {"sem_seg": sem_seg_figures(conf, names), "panoptic_seg": pq_figures(pq.counts, pq.iou, [i in thing_ids for i in cats])}, pq


def assert_same_figures(got, ref, tol=1e-9):
    assert set(got) == set(ref)
    for task in ref:
        assert set(got[task]) == set(ref[task]), task
        for k, v in ref[task].items():
            g = got[task][k]
            assert (math.isnan(g) and math.isnan(v)) or abs(g - v) <= tol, (task, k, g, v)


THINGS, STUFF = [1, 4, 9], [92, 93, 120, 200]
SIZES3 = [(60, 88), (75, 50), (64, 64)]


# ---- CPU: the formulas -----------------------------------------------------------------------------------------------------------------
def test_sem_seg_figures_on_a_hand_written_matrix(osr):
    from openset_rcnn_amd.host.seg_evaluation import sem_seg_results
    # classes a, b, c; c never occurs in the ground truth (but is predicted twice); the last column holds ignored pixels
    conf = np.array([[6, 1, 0, 9], [2, 3, 0, 9], [1, 1, 0, 9], [0, 0, 0, 0]])
    res = sem_seg_results(conf, ["a", "b", "c"])
    iou_a, iou_b = 6 / (9 + 7 - 6), 3 / (5 + 5 - 3)
    assert res["IoU-a"] == pytest.approx(100 * iou_a, abs=1e-12) and res["IoU-b"] == pytest.approx(100 * iou_b, abs=1e-12) and math.isnan(res["IoU-c"])
    assert res["ACC-a"] == pytest.approx(100 * 6 / 9, abs=1e-12) and math.isnan(res["ACC-c"])
    assert res["mIoU"] == pytest.approx(100 * (iou_a + iou_b) / 2, abs=1e-12)
    assert res["mACC"] == pytest.approx(100 * (6 / 9 + 3 / 5) / 2, abs=1e-12)
    assert res["fwIoU"] == pytest.approx(100 * (iou_a * 9 / 14 + iou_b * 5 / 14), abs=1e-12)
    assert res["pACC"] == pytest.approx(100 * 9 / 14, abs=1e-12)
    assert_same_figures({"sem_seg": res}, {"sem_seg": sem_seg_figures(conf, ["a", "b", "c"])})


def test_pq_figures_on_hand_written_statistics(osr):
    from openset_rcnn_amd.host.seg_evaluation import pq_results
    # category 0 (thing): 2 tp; 1 (thing): no tp but an fp and an fn; 2 (thing): never seen; 3 (stuff): one tp, one fn
    counts = np.array([[2, 1, 0], [0, 1, 1], [0, 0, 0], [1, 0, 1]])
    iou = np.array([1.5, 0.0, 0.0, 0.8])
    res = pq_results(counts, iou, [True, True, True, False])
    assert res["PQ_th"] == pytest.approx(100 * (1.5 / 2.5 + 0.0) / 2, abs=1e-12)
    assert res["SQ_th"] == pytest.approx(100 * (0.75 + 0.0) / 2, abs=1e-12) and res["RQ_th"] == pytest.approx(100 * (2 / 2.5) / 2, abs=1e-12)
    assert res["PQ_st"] == pytest.approx(100 * 0.8 / 1.5, abs=1e-12) and res["SQ_st"] == pytest.approx(80.0, abs=1e-12)
    assert res["PQ"] == pytest.approx(100 * (1.5 / 2.5 + 0.0 + 0.8 / 1.5) / 3, abs=1e-12)
    assert_same_figures({"p": res}, {"p": pq_figures(counts, iou, [True, True, True, False])})
    empty = pq_results(counts[:3], iou[:3], [True, True, True])  # no stuff category at all: the group reports 0
    assert empty["PQ_st"] == empty["SQ_st"] == empty["RQ_st"] == 0.0 and empty["PQ"] == empty["PQ_th"]


def test_rank_partials_merge_by_summing(osr):
    from openset_rcnn_amd.host import seg_evaluation as S
    a = dict(conf=np.array([[1, 2], [3, 4]]), invalid=0)
    b = dict(conf=np.array([[10, 0], [0, 5]]), invalid=2)
    m = S.merge_sem_seg_partials([a, b])
    assert m["conf"].tolist() == [[11, 2], [3, 9]] and m["invalid"] == 2
    pa = dict(counts=np.array([[1, 0, 2]]), iou=np.array([0.75]), flags=np.array([0, 0, 0]))
    pb = dict(counts=np.array([[2, 1, 0]]), iou=np.array([1.5]), flags=np.array([0, 1, 0]))
    m = S.merge_pq_partials([pa, pb])
    assert m["counts"].tolist() == [[3, 1, 2]] and m["iou"].tolist() == [2.25] and m["flags"].tolist() == [0, 1, 0]


def test_dataset_evaluators_merges_and_passes_none_through(osr):
    from openset_rcnn_amd.host.evaluation import DatasetEvaluators

    class One:
        def __init__(self, res):
            self.res, self.calls = res, []

        def reset(self):
            self.calls.append("reset")

        def process(self, i, o):
            self.calls.append((i, o))

        def evaluate(self):
            return self.res
    a, b = One({"x": {"k": 1}}), One({"y": {"k": 2}})
    ev = DatasetEvaluators([a, b])
    ev.reset()
    ev.process("in", "out")
    assert ev.evaluate() == {"x": {"k": 1}, "y": {"k": 2}} and a.calls == b.calls == ["reset", ("in", "out")]
    assert DatasetEvaluators([One(None), One(None)]).evaluate() is None


# ---- CPU: the registration -------------------------------------------------------------------------------------------------------------
def test_registration_metadata_dicts_and_evaluator_types(osr, tmp_path):
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host.data import DatasetMapper
    from openset_rcnn_amd.host.evaluation import DatasetEvaluators
    from openset_rcnn_amd.host.seg_evaluation import COCOPanopticEvaluator, SemSegEvaluator
    name = f"pan_{tmp_path.name}_reg"
    truth = make_dataset(tmp_path, name, SIZES3, THINGS, STUFF, seed=1)
    meta = D.MetadataCatalog.get(name)
    assert meta.evaluator_type == "coco_panoptic_seg" and meta.ignore_label == 255
    assert meta.thing_classes == ["thing1", "thing4", "thing9"] and meta.thing_dataset_id_to_contiguous_id == {1: 0, 4: 1, 9: 2}
    assert meta.stuff_classes == ["things", "stuff92", "stuff93", "stuff120", "stuff200"]
    assert meta.stuff_dataset_id_to_contiguous_id == {0: 0, 92: 1, 93: 2, 120: 3, 200: 4}
    dicts = D.DatasetCatalog[name]()
    assert [d["image_id"] for d in dicts] == [t["image_id"] for t in truth]
    for d, t in zip(dicts, truth):
        assert os.path.isfile(d["file_name"]) and os.path.isfile(d["sem_seg_file_name"]) and os.path.isfile(d["pan_seg_file_name"])
        assert np.array_equal(np.asarray(Image.open(d["sem_seg_file_name"])), t["sem"])
        assert [s["id"] for s in d["segments_info"]] == [s["id"] for s in t["segs"]]
        for s, raw in zip(d["segments_info"], t["segs"]):
            table = meta.thing_dataset_id_to_contiguous_id if s["isthing"] else meta.stuff_dataset_id_to_contiguous_id
            assert s["isthing"] == (raw["category_id"] in THINGS) and s["category_id"] == table[raw["category_id"]]
        assert len(d["annotations"]) == sum(1 for s in t["segs"] if s["category_id"] in THINGS)
    mapped = DatasetMapper(_cfg(), is_train=False)(dicts[0])  # the mapper passes the extra keys through
    assert all(mapped[k] == dicts[0][k] for k in ("sem_seg_file_name", "pan_seg_file_name", "segments_info")) and "annotations" not in mapped
    ev = D.get_evaluator(_cfg(), name)
    assert isinstance(ev, DatasetEvaluators) and [type(e) for e in ev._evaluators] == [SemSegEvaluator, COCOPanopticEvaluator]
    assert ev._evaluators[0].num_classes == 5 and ev._evaluators[1].isthing == [True, True, True, False, False, False, False]
    ev = D.get_evaluator(_cfg("MODEL.PANOPTIC_FPN.COMBINE.ENABLED", "False"), name)
    assert [type(e) for e in ev._evaluators] == [SemSegEvaluator]
    # the evaluator's tables of one image: rows in ascending id, the crowd pick on the category's last crowd segment of the JSON
    path, ids, gmeta = D.get_evaluator(_cfg(), name)._evaluators[1].ground_truth_tables(truth[0]["image_id"])
    assert path == dicts[0]["pan_seg_file_name"] and ids.tolist() == sorted(s["id"] for s in truth[0]["segs"])
    last = {}
    for s in truth[0]["segs"]:
        if s["iscrowd"]:
            last[s["category_id"]] = s["id"]
    assert [int(i) for i, m in zip(ids, gmeta) if m[3]] == sorted(last.values())
    sem_name = f"sem_{tmp_path.name}_reg"
    D.register_sem_seg(sem_name, str(tmp_path / "sem"), str(tmp_path / "images"), meta.stuff_classes, 255)
    sem_dicts = D.DatasetCatalog[sem_name]()
    assert [os.path.basename(d["sem_seg_file_name"]) for d in sem_dicts] == ["im000.png", "im001.png", "im002.png"]
    assert [os.path.basename(d["file_name"]) for d in sem_dicts] == ["im000.jpg", "im001.jpg", "im002.jpg"]
    assert type(D.get_evaluator(_cfg(), sem_name)) is SemSegEvaluator
    D.MetadataCatalog.get(f"odd_{tmp_path.name}").evaluator_type = "lvis"
    with pytest.raises(NotImplementedError, match="no Evaluator for the dataset"):
        D.get_evaluator(_cfg(), f"odd_{tmp_path.name}")


def test_run_net_registers_the_coco_panoptic_names_when_the_files_exist(osr, tmp_path):
    from openset_rcnn_amd.host import datasets as D
    D.register_coco_panoptic(str(tmp_path))  # nothing there: nothing registered
    assert "coco_2017_val_panoptic_separated" not in D.DatasetCatalog
    ann = tmp_path / "coco" / "annotations"
    os.makedirs(ann)
    cats = [dict(id=1, name="person", isthing=1), dict(id=92, name="banner", isthing=0)]
    (ann / "panoptic_val2017.json").write_text(json.dumps(dict(images=[], annotations=[], categories=cats)))
    (ann / "instances_val2017.json").write_text(json.dumps(dict(images=[], annotations=[], categories=cats[:1])))
    try:
        D.register_coco_panoptic(str(tmp_path))
        assert "coco_2017_val_panoptic_separated" in D.DatasetCatalog and "coco_2017_train_panoptic_separated" not in D.DatasetCatalog
        meta = D.MetadataCatalog.get("coco_2017_val_panoptic_separated")
        assert meta.panoptic_root == str(tmp_path / "coco" / "panoptic_val2017") and meta.sem_seg_root == str(tmp_path / "coco" / "panoptic_stuff_val2017")
        assert meta.stuff_classes == ["things", "banner"] and D.DatasetCatalog["coco_2017_val_panoptic_separated"]() == []
    finally:
        D.DatasetCatalog.pop("coco_2017_val_panoptic_separated", None)


def test_the_evaluators_refuse_host_tensors_and_missing_segments(osr, tmp_path):
    from openset_rcnn_amd.host import datasets as D
    name = f"pan_{tmp_path.name}_cpu"
    truth = make_dataset(tmp_path, name, SIZES3[:1], THINGS, STUFF, seed=2)
    pred = predictions_for(truth, THINGS, STUFF, seed=3)[0]
    d = D.DatasetCatalog[name]()[0]
    sem, pan = D.get_evaluator(_cfg(), name)._evaluators
    with pytest.raises(osr.OsrError, match="no CPU fallback"):
        sem.process([d], [{"sem_seg": torch.from_numpy(pred["sem_seg"])}])
    with pytest.raises(osr.OsrError, match="no CPU fallback"):
        pan.process([d], [{"panoptic_seg": (torch.from_numpy(pred["pan"]), pred["info"])}])
    with pytest.raises(ValueError, match="segments_info"):
        pan.process([d], [{"panoptic_seg": (torch.from_numpy(pred["pan"]), None)}])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
class StubModel:
    def __init__(self, truth, preds):
        self.by_id = {t["image_id"]: p for t, p in zip(truth, preds)}

    def __call__(self, batch):
        out = []
        for inp in batch:
            p = self.by_id[inp["image_id"]]
            out.append({"sem_seg": torch.from_numpy(p["sem_seg"]).to(DEV), "panoptic_seg": (torch.from_numpy(p["pan"]).to(DEV), p["info"])})
        return out


@pytest.mark.gpu
def test_three_images_through_inference_on_dataset(osr, tmp_path):
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host.evaluation import inference_on_dataset
    name = f"pan_{tmp_path.name}_gpu"
    truth = make_dataset(tmp_path, name, SIZES3, THINGS, STUFF, seed=4)
    preds = predictions_for(truth, THINGS, STUFF, seed=5)
    ref, pq = reference_results(truth, preds, THINGS, STUFF)
    assert pq.counts[:, 0].sum() >= 5 and pq.counts[:, 1].sum() >= 1 and pq.counts[:, 2].sum() >= 1  # (matches, fp and fn all occur)
    out_dir = tmp_path / "out"
    ev = D.get_evaluator(_cfg(), name, str(out_dir))
    dicts = D.DatasetCatalog[name]()
    got = inference_on_dataset(StubModel(truth, preds), [[d] for d in dicts], ev, rank=0, world=1)
    assert_same_figures(got, ref)
    n = len(THINGS) + len(STUFF)
    buf = ev._evaluators[1]._buf.cpu()
    assert np.array_equal(buf[: 3 * n].view(n, 3).numpy(), pq.counts)
    assert buf[3 * n + 3:].view(torch.float64).numpy().tobytes() == np.array(pq.iou).tobytes()  # one process: the ordered sum, bit for bit
    assert os.path.isfile(out_dir / "sem_seg_evaluation.json") and os.path.isfile(out_dir / "panoptic_evaluation.json")
    # a second pass starts from zero (reset) and label maps are accepted in place of values
    labels = [dict(p, sem_seg=argmax_lowest(p["sem_seg"]).astype(np.int32)) for p in preds]
    again = inference_on_dataset(StubModel(truth, labels), [dicts[:2], dicts[2:]], ev, rank=0, world=1)
    assert_same_figures(again, ref)


@pytest.mark.gpu
def test_a_bad_label_and_a_bad_segment_raise_at_evaluate(osr, tmp_path):
    from openset_rcnn_amd.host import datasets as D
    name = f"pan_{tmp_path.name}_bad"
    truth = make_dataset(tmp_path, name, SIZES3[:1], THINGS, STUFF, seed=6)
    pred = predictions_for(truth, THINGS, STUFF, seed=7)[0]
    d = D.DatasetCatalog[name]()[0]
    sem, pan = D.get_evaluator(_cfg(), name)._evaluators
    labels = torch.from_numpy(argmax_lowest(pred["sem_seg"]).astype(np.int32)).to(DEV)
    labels[0, :3] = 5  # C = 5: outside [0, 5)
    sem.reset()
    sem.process([d], [{"sem_seg": labels}])
    with pytest.raises(ValueError, match="3 pixels"):
        sem.evaluate()
    info = [dict(s) for s in pred["info"]]
    info[0]["category_id"] = 77  # unknown to the dataset: slot -1
    pan.reset()
    pan.process([d], [{"panoptic_seg": (torch.from_numpy(pred["pan"]).to(DEV), info)}])
    with pytest.raises(ValueError, match=r"flags\[2\]"):
        pan.evaluate()


@pytest.mark.gpu
def test_the_seeded_panoptic_fpn_scores_like_the_reference_on_its_own_outputs(osr, tmp_path):
    """configs/panoptic_fpn.yaml with the seeded weights of tests/test_panoptic_engine.py on its two images (128 x 160 pad); the ground
    truth is a synthetic panoptic dataset at the two output sizes with 5 thing and 53 stuff categories."""
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host.evaluation import inference_on_dataset
    from tests import test_panoptic_engine as E
    things, stuff = [1, 2, 3, 5, 8], list(range(92, 92 + 53))
    name = f"pan_{tmp_path.name}_fpn"
    truth = make_dataset(tmp_path, name, E.OUT_SIZES, things, stuff, seed=8, segments=12)
    model = E.model_of("PanopticFPN", torch.float32)
    dicts = D.DatasetCatalog[name]()
    kept = []

    image_of = {t["image_id"]: im for t, im in zip(truth, E.setup()["images"])}

    def run(batch):
        outs = model([dict(d, image=image_of[d["image_id"]]) for d in batch])
        kept.extend(outs)
        return outs
    ev = D.get_evaluator(E._cfg(), name)
    got = inference_on_dataset(run, [[d] for d in dicts], ev, rank=0, world=1)
    preds = [dict(sem_seg=o["sem_seg"].cpu().numpy(), pan=o["panoptic_seg"][0].cpu().numpy(), info=o["panoptic_seg"][1]) for o in kept]
    assert len(preds) == 2 and sum(len(p["info"]) for p in preds) >= 2
    ref, _ = reference_results(truth, preds, things, stuff)
    assert_same_figures(got, ref)


@pytest.mark.gpu
def test_run_net_eval_only_prints_both_tables(osr, tmp_path, monkeypatch, caplog):
    """run_net.py --eval-only on coco_2017_val_panoptic_separated (two small images in detectron2's directory layout, freshly
    initialised weights): the run ends with one log line per task instead of get_evaluator's NotImplementedError."""
    import logging
    import sys
    sys.path.insert(0, ROOT)
    import run_net
    make_dataset(tmp_path, None, [(96, 128), (80, 112)], [1, 2, 3, 5, 8], list(range(92, 92 + 53)), seed=10, coco_split="val")
    monkeypatch.setenv("DETECTRON2_DATASETS", str(tmp_path))
    out = str(tmp_path / "out")
    with caplog.at_level(logging.INFO, logger="openset_rcnn"):
        assert run_net.main(["--config-file", os.path.join(ROOT, "configs", "panoptic_fpn.yaml"), "--eval-only", "OUTPUT_DIR", out, "MODEL.WEIGHTS", "",
                             "DATASETS.TEST", "('coco_2017_val_panoptic_separated',)", "MODEL.ROI_HEADS.NUM_CLASSES", "5", "INPUT.MIN_SIZE_TEST", "0",
                             "MODEL.PANOPTIC_FPN.COMBINE.STUFF_AREA_LIMIT", "64"]) == 0
    lines = [r.getMessage() for r in caplog.records]
    assert any(m.strip().startswith("sem_seg:") and "mIoU=" in m and "pACC=" in m for m in lines), lines
    assert any(m.strip().startswith("panoptic_seg:") and "PQ=" in m and "RQ_st=" in m for m in lines), lines
    folder = os.path.join(out, "inference", "coco_2017_val_panoptic_separated", "Final")
    assert os.path.isfile(os.path.join(folder, "sem_seg_evaluation.json")) and os.path.isfile(os.path.join(folder, "panoptic_evaluation.json"))


@pytest.mark.gpu
def test_the_three_kernels_capture_and_replay(osr):
    ops = osr.ops
    rng = np.random.default_rng(9)
    h, w, c = 40, 52, 19
    labels = torch.from_numpy(blocky(rng, h, w, c).astype(np.int32)).to(DEV)
    gt = torch.from_numpy(blocky(rng, h, w, c).astype(np.uint8)).to(DEV)
    ids_map, pred = blocky(rng, h, w, 5) * 3, blocky(rng, h, w, 4, cell=6)
    rgb, gt_ids = torch.from_numpy(ids_to_rgb(ids_map)).to(DEV), torch.tensor([3, 6, 9, 12], dtype=torch.int32, device=DEV)
    pred_d = torch.from_numpy(pred.astype(np.int32)).to(DEV)
    area = [int((ids_map == v).sum()) for v in (3, 6, 9, 12)]
    meta = torch.tensor([[i % 2, 0, a, 0] for i, a in enumerate(area)], dtype=torch.int32, device=DEV)
    slots = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    state = [torch.zeros((c + 1, c + 1), dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
             torch.zeros((2, 3), dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)]
    table = torch.zeros((6, 4), dtype=torch.int32, device=DEV)

    def step():
        ops.semseg_confusion(labels, gt, c, 255, state[0], state[1])
        ops.panoptic_pair_counts(rgb, gt_ids, pred_d, 3, state[4], out=table)
        ops.pq_accumulate(table, meta, slots, state[2], state[3], state[4])
    step()
    torch.cuda.synchronize()
    eager = [t.clone() for t in state]
    for t in state:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in state:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(state, eager)) and int(eager[0].sum()) == h * w
