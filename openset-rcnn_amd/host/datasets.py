"""Dataset catalog + the VOC-COCO open-set splits (the data format either side of the hot path).

Mirrors /root/reference/openset_rcnn/data/voc_coco.py (category list :5-29, register_voc_coco :32-42) and data/custom.py
(register_opendet_voc_coco :32-51) on a minimal catalog of our own, plus [d2] load_voc_instances: one dict per image with
file_name, image_id, height, width and annotations [{category_id, bbox XYXY with xmin/ymin - 1}]."""
from __future__ import annotations

import os
import xml.etree.ElementTree as ET
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence

# the 20 VOC classes, the 60 remaining COCO classes in the order of the 20-40 / 40-60 / 60-80 splits, then "unknown"
VOC_COCO_CATEGORIES = [
    "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse", "motorbike",
    "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor",
    "truck", "traffic light", "fire hydrant", "stop sign", "parking meter", "bench", "elephant", "bear", "zebra", "giraffe", "backpack",
    "umbrella", "handbag", "tie", "suitcase", "microwave", "oven", "toaster", "sink", "refrigerator",
    "frisbee", "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard", "tennis racket",
    "banana", "apple", "sandwich", "orange", "broccoli", "carrot", "hot dog", "pizza", "donut", "cake",
    "bed", "toilet", "laptop", "mouse", "remote", "keyboard", "cell phone", "book", "clock", "vase", "scissors", "teddy bear", "hair drier",
    "toothbrush", "wine glass", "cup", "fork", "knife", "spoon", "bowl",
    "unknown",
]

VOC_COCO_SPLITS = ("voc_coco_20_40_test", "voc_coco_20_60_test", "voc_coco_20_80_test", "voc_coco_2500_test", "voc_coco_5000_test",
                   "voc_coco_10000_test", "voc_coco_20000_test", "voc_coco_val")


class _Catalog(dict):
    def register(self, name: str, value) -> None:
        assert name not in self, f"dataset '{name}' is already registered"
        self[name] = value


DatasetCatalog: Dict[str, Callable[[], List[dict]]] = _Catalog()
_METADATA: Dict[str, SimpleNamespace] = {}


class MetadataCatalog:
    @staticmethod
    def get(name: str) -> SimpleNamespace:
        if name not in _METADATA:
            _METADATA[name] = SimpleNamespace(name=name)
        return _METADATA[name]


def load_voc_instances(dirname: str, split: str, class_names: Sequence[str]) -> List[dict]:
    """[d2] detectron2.data.datasets.pascal_voc.load_voc_instances."""
    with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
        fileids = [x.strip() for x in f.readlines() if x.strip()]
    dicts = []
    for fid in fileids:
        tree = ET.parse(os.path.join(dirname, "Annotations", fid + ".xml"))
        rec = dict(file_name=os.path.join(dirname, "JPEGImages", fid + ".jpg"), image_id=fid,
                   height=int(tree.findall("./size/height")[0].text), width=int(tree.findall("./size/width")[0].text), annotations=[])
        for obj in tree.findall("object"):
            bb = obj.find("bndbox")
            box = [float(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]
            box[0] -= 1.0  # VOC pixel indices are 1-based; boxes become 0-based half-open (the evaluator adds the 1 back)
            box[1] -= 1.0
            rec["annotations"].append(dict(category_id=class_names.index(obj.find("name").text), bbox=box, bbox_mode="XYXY_ABS"))
        dicts.append(rec)
    return dicts


def register_voc_coco(name: str, dirname: str, split: str, year: int) -> None:
    class_names = VOC_COCO_CATEGORIES
    DatasetCatalog.register(name, lambda: load_voc_instances(dirname, split, class_names))
    meta = MetadataCatalog.get(name)
    meta.thing_classes, meta.dirname, meta.year, meta.split = list(class_names), dirname, year, split
    meta.thing_dataset_id_to_contiguous_id = {i: i for i in range(len(class_names))}
    meta.evaluator_type = "pascal_voc"


def register_opendet_voc_coco(root: str) -> None:
    for split in VOC_COCO_SPLITS:
        register_voc_coco(split, os.path.join(root, "voc_coco"), split, 2007 if "2007" in split else 2012)


def register_builtin_pascal_voc(root: str) -> None:
    """The PASCAL VOC names the VOC-COCO yaml trains on and tests first ('voc_2007_train', 'voc_2012_trainval', 'voc_2007_test'):
    detectron2 pre-registers them ([d2] data/datasets/builtin.py register_all_pascal_voc) as <root>/VOC{2007,2012} with the 20
    VOC class names, which are the first 20 entries of VOC_COCO_CATEGORIES."""
    names = list(VOC_COCO_CATEGORIES[:20])
    for year, splits in ((2007, ("trainval", "train", "val", "test")), (2012, ("trainval", "train", "val"))):
        for split in splits:
            name, dirname = f"voc_{year}_{split}", os.path.join(root, f"VOC{year}")
            DatasetCatalog.register(name, lambda d=dirname, s=split: load_voc_instances(d, s, names))
            meta = MetadataCatalog.get(name)
            meta.thing_classes, meta.dirname, meta.year, meta.split, meta.evaluator_type = list(names), dirname, year, split, "pascal_voc"
            meta.thing_dataset_id_to_contiguous_id = {i: i for i in range(len(names))}


# ---------------------------------------------------------------------------------------------------------------
# GraspNet open-set splits (COCO-format json): openset_rcnn/data/graspnet.py, graspnet_meta.py, custom.py:9-30
# ---------------------------------------------------------------------------------------------------------------
# the 28 known object categories of the benchmark (graspnet_meta.py:92-98); the full 88-entry category table is read from the
# annotation json itself
GRASPNET_KNOWN_CATEGORIES = [
    "cracker_box", "tomato_soup_can", "banana", "mug", "power_drill", "scissors", "strawberry", "peach", "plum", "knife", "flat_screwdriver",
    "racquetball", "b_cups", "d_toy_airplane", "f_toy_airplane", "i_toy_airplane", "j_toy_airplane", "dabao_sod", "darlie_toothpaste", "camel",
    "large_elephant", "rhinocero", "darlie_box", "black_mouse", "dabao_facewash", "pantene", "head_shoulders_supreme", "head_shoulders_care",
]
GRASPNET_SPLITS = {"graspnet_train": "graspnet_os_train.json", **{f"graspnet_test_{i}": f"graspnet_os_test_{i}.json" for i in range(1, 7)}}


def load_coco_json(json_file: str, image_root: str, dataset_name: Optional[str] = None) -> List[dict]:
    """[d2] load_coco_json without pycocotools: one dict per image with file_name, height, width, image_id and annotations
    [{bbox XYWH_ABS, category_id (contiguous), iscrowd, segmentation (when the json has one: polygons, RLE or whatever it holds,
    untouched -- DatasetMapper decodes what INPUT.MASK_FORMAT "bitmask" can train on)}]; records the category tables in the
    dataset's metadata."""
    import json
    with open(json_file) as f:
        data = json.load(f)
    cats = sorted(data["categories"], key=lambda c: c["id"])
    id_map = {c["id"]: i for i, c in enumerate(cats)}
    if dataset_name is not None:
        meta = MetadataCatalog.get(dataset_name)
        meta.thing_classes = [c["name"] for c in cats]
        meta.thing_dataset_id_to_contiguous_id = id_map
    by_img: Dict[int, List[dict]] = {}
    for a in data["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a)
    out = []
    for im in sorted(data["images"], key=lambda r: r["id"]):
        rec = dict(file_name=os.path.join(image_root, im["file_name"]), height=im["height"], width=im["width"], image_id=im["id"], annotations=[])
        for a in by_img.get(im["id"], []):
            if a.get("ignore", 0):
                continue
            x, y, w, h = a["bbox"]
            rec["annotations"].append(dict(bbox=[x, y, x + w, y + h], bbox_mode="XYXY_ABS", category_id=id_map[a["category_id"]],
                                           iscrowd=a.get("iscrowd", 0)))
            if a.get("segmentation") is not None:
                rec["annotations"][-1]["segmentation"] = a["segmentation"]
        out.append(rec)
    return out


def register_graspnet_instances(name: str, json_file: str, image_root: str) -> None:
    DatasetCatalog.register(name, lambda: load_coco_json(json_file, image_root, name))
    meta = MetadataCatalog.get(name)
    meta.json_file, meta.image_root, meta.evaluator_type = json_file, image_root, "coco"


def register_coco_instances(name: str, metadata: dict, json_file: str, image_root: str) -> None:
    """[d2] register_coco_instances: a plain COCO instances (or person-keypoints) dataset. `closed_set` tells get_evaluator that the
    name is scored with COCOEvaluator (box and keypoint AP); a GraspNet registration carries no such mark."""
    DatasetCatalog.register(name, lambda: load_coco_json(json_file, image_root, name))
    meta = MetadataCatalog.get(name)
    for k, v in dict(metadata).items():
        setattr(meta, k, v)
    meta.json_file, meta.image_root, meta.evaluator_type, meta.closed_set = json_file, image_root, "coco", True


def register_builtin_coco(root: str) -> None:
    """coco_2017_{train,val} and keypoints_coco_2017_{train,val} under detectron2's directory names, when their files exist:
    coco/{train,val}2017 with coco/annotations/instances_{split}2017.json and coco/annotations/person_keypoints_{split}2017.json."""
    coco = os.path.join(root, "coco")
    for split in ("train", "val"):
        for name, jf in ((f"coco_2017_{split}", f"instances_{split}2017.json"), (f"keypoints_coco_2017_{split}", f"person_keypoints_{split}2017.json")):
            jf = os.path.join(coco, "annotations", jf)
            if os.path.isfile(jf):
                register_coco_instances(name, {}, jf, os.path.join(coco, f"{split}2017"))


def load_lvis_json(json_file: str, image_root: str, dataset_name: Optional[str] = None) -> List[dict]:
    """[d2] load_lvis_json without lvis-api: one dict per image with file_name (the JSON's, else the last two path parts of coco_url:
    LVIS v1 names its images "val2017/000000000139.jpg" that way), height, width, image_id, the image's not_exhaustive_category_ids
    and neg_category_ids (dataset ids, as the JSON has them) and annotations [{bbox XYWH_ABS, category_id (contiguous, ascending
    dataset id), segmentation (when the json has one, untouched)}]; records the category tables in the dataset's metadata."""
    import json
    with open(json_file) as f:
        data = json.load(f)
    cats = sorted(data["categories"], key=lambda c: c["id"])
    id_map = {c["id"]: i for i, c in enumerate(cats)}
    if dataset_name is not None:
        meta = MetadataCatalog.get(dataset_name)
        meta.thing_classes = [c["name"] for c in cats]
        meta.thing_dataset_id_to_contiguous_id = id_map
    by_img: Dict[int, List[dict]] = {}
    for a in data["annotations"]:
        by_img.setdefault(a["image_id"], []).append(a)
    out = []
    for im in sorted(data["images"], key=lambda r: r["id"]):
        name = im["file_name"] if "file_name" in im else os.path.join(*im["coco_url"].split("/")[-2:])
        rec = dict(file_name=os.path.join(image_root, name), height=im["height"], width=im["width"], image_id=im["id"],
                   not_exhaustive_category_ids=list(im.get("not_exhaustive_category_ids", [])), neg_category_ids=list(im.get("neg_category_ids", [])),
                   annotations=[])
        for a in by_img.get(im["id"], []):
            rec["annotations"].append(dict(bbox=list(a["bbox"]), bbox_mode="XYWH_ABS", category_id=id_map[a["category_id"]]))
            if a.get("segmentation") is not None:
                rec["annotations"][-1]["segmentation"] = a["segmentation"]
        out.append(rec)
    return out


def register_lvis_instances(name: str, metadata: dict, json_file: str, image_root: str) -> None:
    """[d2] register_lvis_instances. `lvis_json` tells get_evaluator that the name is scored with LVISEvaluator: metadata that merely
    says evaluator_type "lvis" carries no such mark (and no JSON to score against)."""
    DatasetCatalog.register(name, lambda: load_lvis_json(json_file, image_root, name))
    meta = MetadataCatalog.get(name)
    for k, v in dict(metadata).items():
        setattr(meta, k, v)
    meta.json_file, meta.image_root, meta.evaluator_type, meta.lvis_json = json_file, image_root, "lvis", True


def register_builtin_lvis(root: str) -> None:
    """lvis_v1_{train,val} and lvis_v0.5_{train,val} under detectron2's directory names, when their files exist: lvis/lvis_<version>_
    <split>.json with the images under coco/ (the file names carry the split directory). thing_classes come from the JSON's
    categories, ascending id, when the dataset is loaded or its evaluator built."""
    for version in ("v1", "v0.5"):
        for split in ("train", "val"):
            jf = os.path.join(root, "lvis", f"lvis_{version}_{split}.json")
            if os.path.isfile(jf):
                register_lvis_instances(f"lvis_{version}_{split}", {}, jf, os.path.join(root, "coco"))


def register_graspnet_os(root: str) -> None:
    for name, jf in GRASPNET_SPLITS.items():
        register_graspnet_instances(name, os.path.join(root, "graspnet_os", "annotations", jf), os.path.join(root, "graspnet_os", "images"))


def graspnet_class_map(thing_classes: Sequence[str]):
    """Sorted contiguous ids of the known categories: the `class_id` tensor PLN / SoftMaxClassifier build
    (prototype_learning_network.py:80-86); pass it as `class_id` to build_model / OpensetRCNNEngine(class_map=...)."""
    import torch
    return torch.tensor(sorted(thing_classes.index(n) for n in GRASPNET_KNOWN_CATEGORIES if n in thing_classes), dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------
# Semantic and panoptic segmentation datasets ([d2] data/datasets/coco.py load_sem_seg, coco_panoptic.py
# register_coco_panoptic_separated, builtin.py register_all_coco; written from memory of detectron2 v0.6)
# ---------------------------------------------------------------------------------------------------------------
def _files_by_stem(root: str, ext: str) -> Dict[str, str]:
    out = {}
    for base, _, files in os.walk(root):
        for f in files:
            if f.lower().endswith(ext):
                full = os.path.join(base, f)
                out[os.path.splitext(os.path.relpath(full, root))[0]] = full
    return out


def load_sem_seg(gt_root: str, image_root: str, gt_ext: str = ".png", image_ext: str = ".jpg") -> List[dict]:
    """[d2] load_sem_seg: one dict {file_name, sem_seg_file_name} per image, the two directories paired by relative path without
    the extension; a file without its partner is left out, the rest is sorted by path."""
    images, gts = _files_by_stem(image_root, image_ext), _files_by_stem(gt_root, gt_ext)
    return [dict(file_name=images[k], sem_seg_file_name=gts[k]) for k in sorted(set(images) & set(gts))]


def register_sem_seg(name: str, gt_root: str, image_root: str, stuff_classes: Sequence[str], ignore_label: int = 255) -> None:
    DatasetCatalog.register(name, lambda: load_sem_seg(gt_root, image_root))
    meta = MetadataCatalog.get(name)
    meta.sem_seg_root, meta.image_root, meta.stuff_classes, meta.ignore_label = gt_root, image_root, list(stuff_classes), int(ignore_label)
    meta.evaluator_type = "sem_seg"


def panoptic_separated_tables(categories: Sequence[dict]) -> dict:
    """The metadata tables of detectron2's "separated" panoptic format from a panoptic JSON's `categories` ({id, name, isthing}):
    things get contiguous ids 0 .. in ascending dataset id; stuff contiguous id 0 is "things" (every thing pixel of the semantic
    ground truth; dataset id 0) and the stuff categories follow from 1 in ascending dataset id."""
    cats = sorted(categories, key=lambda c: c["id"])
    things, stuff = [c for c in cats if c["isthing"]], [c for c in cats if not c["isthing"]]
    return dict(thing_classes=[c["name"] for c in things], stuff_classes=["things"] + [c["name"] for c in stuff],
                thing_dataset_id_to_contiguous_id={c["id"]: i for i, c in enumerate(things)},
                stuff_dataset_id_to_contiguous_id={0: 0, **{c["id"]: i + 1 for i, c in enumerate(stuff)}})


def _read_json(path: str):
    import json
    with open(path) as f:
        return json.load(f)


def load_coco_panoptic_separated(name: str) -> List[dict]:
    """load_coco_json's dicts of the instances JSON plus sem_seg_file_name, pan_seg_file_name and segments_info (the panoptic
    JSON's, category ids made contiguous through the thing / stuff tables, with `isthing`)."""
    meta = MetadataCatalog.get(name)
    pan = {a["image_id"]: a for a in _read_json(meta.panoptic_json)["annotations"]}
    thing, stuff = meta.thing_dataset_id_to_contiguous_id, meta.stuff_dataset_id_to_contiguous_id
    out = []
    for rec in load_coco_json(meta.json_file, meta.image_root):
        a = pan[rec["image_id"]]
        rec["pan_seg_file_name"] = os.path.join(meta.panoptic_root, a["file_name"])
        rec["sem_seg_file_name"] = os.path.join(meta.sem_seg_root, os.path.splitext(os.path.basename(rec["file_name"]))[0] + ".png")
        rec["segments_info"] = [dict(s, isthing=s["category_id"] in thing, category_id=thing[s["category_id"]] if s["category_id"] in thing
                                     else stuff[s["category_id"]]) for s in a["segments_info"]]
        out.append(rec)
    return out


def register_coco_panoptic_separated(name: str, image_root: str, panoptic_root: str, panoptic_json: str, sem_seg_root: str, instances_json: str) -> None:
    """[d2] register_coco_panoptic_separated: the instances JSON for the detector, <sem_seg_root>/<image>.png for the semantic head
    (stuff ids as in panoptic_separated_tables, 255 = ignore), the panoptic PNGs + JSON for PQ. Reads the panoptic JSON's categories."""
    DatasetCatalog.register(name, lambda: load_coco_panoptic_separated(name))
    meta = MetadataCatalog.get(name)
    for k, v in panoptic_separated_tables(_read_json(panoptic_json)["categories"]).items():
        setattr(meta, k, v)
    meta.image_root, meta.panoptic_root, meta.panoptic_json, meta.sem_seg_root, meta.json_file = image_root, panoptic_root, panoptic_json, sem_seg_root, instances_json
    meta.ignore_label, meta.evaluator_type = 255, "coco_panoptic_seg"


def register_coco_panoptic(root: str) -> None:
    """coco_2017_{train,val}_panoptic_separated under detectron2's directory names, when the files exist:
    coco/{train,val}2017, coco/panoptic_{split}2017, coco/annotations/panoptic_{split}2017.json, coco/panoptic_stuff_{split}2017,
    coco/annotations/instances_{split}2017.json."""
    coco = os.path.join(root, "coco")
    for split in ("train", "val"):
        pj, ij = os.path.join(coco, "annotations", f"panoptic_{split}2017.json"), os.path.join(coco, "annotations", f"instances_{split}2017.json")
        if os.path.isfile(pj) and os.path.isfile(ij):
            register_coco_panoptic_separated(f"coco_2017_{split}_panoptic_separated", os.path.join(coco, f"{split}2017"), os.path.join(coco, f"panoptic_{split}2017"),
                                             pj, os.path.join(coco, f"panoptic_stuff_{split}2017"), ij)


def get_evaluator(cfg, dataset_name: str, output_folder=None):
    """train.py:57-78: "pascal_voc" -> open-set VOC evaluator, "coco" -> open-set COCO-style evaluator (GraspNet); [d2] train_net.py:
    "coco" on a register_coco_instances name (metadata closed_set) -> COCOEvaluator (box and keypoint AP; segm is not built),
    "sem_seg" -> SemSegEvaluator, "coco_panoptic_seg" -> SemSegEvaluator + COCOPanopticEvaluator (box AP is not wired into the
    panoptic datasets), "lvis" on a register_lvis_instances name (metadata lvis_json) -> LVISEvaluator (federated box AP)."""
    from .evaluation import PascalVOCDetectionEvaluator
    meta = MetadataCatalog.get(dataset_name)
    if getattr(meta, "evaluator_type", None) in ("sem_seg", "coco_panoptic_seg"):
        from .evaluation import DatasetEvaluators
        from .seg_evaluation import COCOPanopticEvaluator, SemSegEvaluator
        sem = SemSegEvaluator(dataset_name, len(meta.stuff_classes), meta.ignore_label, meta.stuff_classes, output_folder)
        if meta.evaluator_type == "sem_seg":
            return sem
        evaluators = [sem]
        if cfg.MODEL.PANOPTIC_FPN.COMBINE.ENABLED:
            evaluators.append(COCOPanopticEvaluator(dataset_name, output_folder))
        return DatasetEvaluators(evaluators)
    if getattr(meta, "evaluator_type", None) == "lvis" and getattr(meta, "lvis_json", False):
        from .lvis_evaluation import LVISEvaluator
        if not hasattr(meta, "thing_dataset_id_to_contiguous_id"):
            DatasetCatalog[dataset_name]()  # loading the json fills the category tables
        return LVISEvaluator(dataset_name, cfg, output_folder)
    if getattr(meta, "evaluator_type", None) == "coco" and getattr(meta, "closed_set", False):
        from .coco_evaluation import COCOEvaluator
        if not hasattr(meta, "thing_dataset_id_to_contiguous_id"):
            DatasetCatalog[dataset_name]()  # loading the json fills the category tables
        return COCOEvaluator(dataset_name, cfg, output_folder, max_dets_per_image=cfg.TEST.DETECTIONS_PER_IMAGE)
    if getattr(meta, "evaluator_type", None) == "coco":
        from .os_coco_evaluation import OpensetCOCOEvaluator
        if not hasattr(meta, "thing_dataset_id_to_contiguous_id"):
            DatasetCatalog[dataset_name]()  # loading the json fills the category tables
        rev = {v: k for k, v in meta.thing_dataset_id_to_contiguous_id.items()}
        return OpensetCOCOEvaluator(meta.json_file, GRASPNET_KNOWN_CATEGORIES, rev, max_dets_per_image=[10, 20, 30, 50, 100], output_dir=output_folder)
    if getattr(meta, "evaluator_type", None) != "pascal_voc":
        raise NotImplementedError(f"no Evaluator for the dataset {dataset_name} with the type {getattr(meta, 'evaluator_type', None)}")
    return PascalVOCDetectionEvaluator(meta.dirname, meta.split, meta.thing_classes, cfg.MODEL.ROI_HEADS.NUM_KNOWN_CLASSES,
                                       output_folder if output_folder is not None else getattr(cfg, "OUTPUT_DIR", None))
