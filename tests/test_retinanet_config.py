"""META_ARCHITECTURE "RetinaNet" on the host side, without a GPU: the MODEL.RETINANET defaults (detectron2 v0.6), configs/retinanet_fpn.yaml,
the model mirror's parameter names and shapes, checkpoint round trips, every refusal by name, and engine_std.cell_anchor_table with several
sizes per level."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(yaml="retinanet_fpn.yaml", *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    if yaml:
        cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def test_defaults_are_detectron2s(osr):
    rn = _cfg(None).MODEL.RETINANET
    want = dict(NUM_CLASSES=80, IN_FEATURES=["p3", "p4", "p5", "p6", "p7"], NUM_CONVS=4, PRIOR_PROB=0.01, SCORE_THRESH_TEST=0.05, TOPK_CANDIDATES_TEST=1000,
                NMS_THRESH_TEST=0.5, BBOX_REG_WEIGHTS=(1.0, 1.0, 1.0, 1.0), NORM="", IOU_THRESHOLDS=[0.4, 0.5], IOU_LABELS=[0, -1, 1], FOCAL_LOSS_GAMMA=2.0,
                FOCAL_LOSS_ALPHA=0.25, SMOOTH_L1_LOSS_BETA=0.1, BBOX_REG_LOSS_TYPE="smooth_l1")
    assert dict(rn) == want
    assert _cfg(None).MODEL.META_ARCHITECTURE == "GeneralizedRCNN"


def test_yaml_loads_and_restates_base_retinanet(osr):
    cfg = _cfg()
    m = cfg.MODEL
    assert m.META_ARCHITECTURE == "RetinaNet" and m.BACKBONE.NAME == "build_retinanet_resnet_fpn_backbone"
    assert list(m.RESNETS.OUT_FEATURES) == ["res3", "res4", "res5"] and list(m.FPN.IN_FEATURES) == ["res3", "res4", "res5"]
    assert [list(s) for s in m.ANCHOR_GENERATOR.SIZES] == [[x * 2 ** (i / 3) for i in range(3)] for x in (32, 64, 128, 256, 512)]  # (double precision, exactly)
    assert [list(r) for r in m.ANCHOR_GENERATOR.ASPECT_RATIOS] == [[0.5, 1.0, 2.0]]


@pytest.mark.parametrize("k", [80, 5])
def test_parameter_names_and_widths(osr, k):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.RETINANET.NUM_CLASSES", str(k)))
    assert type(model).__name__ == "RetinaNet"
    sd = model.state_dict()
    names = {n for n in sd if not n.startswith("backbone.bottom_up.")}
    want = {f"backbone.fpn_{kind}{l}.{leaf}" for kind in ("lateral", "output") for l in (3, 4, 5) for leaf in ("weight", "bias")}
    want |= {f"backbone.top_block.{p}.{leaf}" for p in ("p6", "p7") for leaf in ("weight", "bias")}
    want |= {f"head.{sub}.{i}.{leaf}" for sub in ("cls_subnet", "bbox_subnet") for i in (0, 2, 4, 6) for leaf in ("weight", "bias")}
    want |= {f"head.{n}.{leaf}" for n in ("cls_score", "bbox_pred") for leaf in ("weight", "bias")}
    assert names == want
    assert not [n for n in sd if "fpn_lateral2" in n or "fpn_output2" in n]
    assert tuple(sd["backbone.top_block.p6.weight"].shape) == (256, 2048, 3, 3) and tuple(sd["backbone.top_block.p7.weight"].shape) == (256, 256, 3, 3)
    assert tuple(sd["head.cls_score.weight"].shape) == (9 * k, 256, 3, 3) and tuple(sd["head.bbox_pred.weight"].shape) == (36, 256, 3, 3)
    assert tuple(sd["head.cls_subnet.6.weight"].shape) == (256, 256, 3, 3)
    assert torch.allclose(sd["head.cls_score.bias"], torch.full((9 * k,), -math.log(0.99 / 0.01)))
    assert float(sd["head.bbox_pred.bias"].abs().max()) == 0.0 and 0.008 < float(sd["head.cls_subnet.0.weight"].std()) < 0.012
    # the bottom-up trunk is the stock one
    stock = M.build_model(_cfg("base_rcnn_fpn.yaml")).state_dict()
    assert {n for n in sd if n.startswith("backbone.bottom_up.")} == {n for n in stock if n.startswith("backbone.bottom_up.")}


def test_unequal_anchor_counts_are_refused(osr):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match="MODEL.ANCHOR_GENERATOR.SIZES"):
        M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.ANCHOR_GENERATOR.SIZES", "[[32, 40], [64], [128], [256], [512]]"))


def test_state_dict_round_trips_through_pth_and_pkl(osr, tmp_path):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into
    torch.manual_seed(3)
    src = M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.RETINANET.NUM_CLASSES", "5"))
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    pth, pkl = str(tmp_path / "retinanet_R_50_FPN.pth"), str(tmp_path / "retinanet_R_50_FPN.pkl")
    torch.save({"model": sd, "iteration": 7}, pth)
    with open(pkl, "wb") as f:  # detectron2's model-zoo form
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "Detectron2 Model Zoo"}, f)
    for path in (pth, pkl):
        torch.manual_seed(4)
        dst = M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.RETINANET.NUM_CLASSES", "5"))
        state = load_checkpoint(path)
        assert state.origin == "d2"
        missing, unexpected = load_into(dst, state)
        assert not missing and not unexpected
        got = dst.state_dict()
        assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_refusals_name_their_keys(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    model = M.build_model(_cfg())
    model.train()
    with pytest.raises(NotImplementedError, match='MODEL.META_ARCHITECTURE "RetinaNet"'):
        model([{"image": torch.zeros(3, 32, 32, dtype=torch.uint8)}])
    with pytest.raises(NotImplementedError, match='MODEL.META_ARCHITECTURE "RetinaNet"'):
        model.make_trainer()
    with pytest.raises(NotImplementedError, match='MODEL.META_ARCHITECTURE "RetinaNet"'):
        model.trainer()
    with pytest.raises(NotImplementedError, match='MODEL.META_ARCHITECTURE "RetinaNet"'):
        model.losses_forward([{"image": torch.zeros(3, 32, 32, dtype=torch.uint8)}])
    model.eval()
    with pytest.raises(ValueError, match="META_ARCHITECTURE"):
        GeneralizedRCNNWithTTA(_cfg(), model)
    with pytest.raises(ValueError, match="META_ARCHITECTURE"):
        M.build_model(_cfg("retinanet_fpn.yaml", "TEST.AUG.ENABLED", "True"))
    with pytest.raises(ValueError, match="MODEL.RETINANET.NORM"):
        M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.RETINANET.NORM", "GN"))
    with pytest.raises(ValueError, match="MASK_ON"):
        M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.MASK_ON", "True"))
    with pytest.raises(ValueError, match="KEYPOINT_ON"):
        M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.KEYPOINT_ON", "True"))


def test_split_convolutions_are_refused(osr):
    from openset_rcnn_amd.host.engine_retinanet import RetinaNetEngine
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match="conv"):
        RetinaNetEngine({}, None, torch.float32, "cpu", conv="split")
    model = M.build_model(_cfg())
    model.conv_precision = "split"
    with pytest.raises(ValueError, match="split"):
        model.engine()


def _table(sizes, ratios):
    """The documented formula: per size then ratio, area = size^2, w = sqrt(area / ratio), h = ratio * w, [-w/2, -h/2, w/2, h/2] in double,
    rounded to fp32."""
    rows = []
    for level in sizes:
        cells = []
        for z in level:
            for r in ratios:
                w = math.sqrt(z * z / r)
                cells.append([-w / 2, -(r * w) / 2, w / 2, (r * w) / 2])
        rows.append(cells)
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def test_cell_anchor_table_is_size_major_and_unchanged_for_one_size(osr):
    from openset_rcnn_amd.host.engine_std import cell_anchor_table
    ratios = (0.5, 1.0, 2.0)
    three = [[x * 2 ** (i / 3) for i in range(3)] for x in (32, 64, 128, 256, 512)]
    got = cell_anchor_table(three, ratios)
    assert tuple(got.shape) == (5, 9, 4) and got.dtype == torch.float32
    assert np.array_equal(got.numpy(), _table(three, ratios))
    assert abs(float(got[0, 4, 2] - got[0, 4, 0]) - 32 * 2 ** (1 / 3)) < 1e-4  # row 4 = second size, ratio 1: a square of that size
    # one size per level, as the stock callers pass it (scalars) -- bit for bit what the formula gives, and what a one-entry list gives
    one = (32.0, 64.0, 128.0, 256.0, 512.0)
    want = _table([[z] for z in one], ratios)
    assert np.array_equal(cell_anchor_table(one, ratios).numpy(), want)
    assert np.array_equal(cell_anchor_table([[z] for z in one], ratios).numpy(), want)
    assert np.array_equal(cell_anchor_table((32, 64), (1.0,)).numpy(), _table([[32.0], [64.0]], (1.0,)))


def test_generalized_rcnn_keeps_its_parameter_names(osr, golden_dir):
    """base_rcnn_fpn.yaml under a configuration that now carries MODEL.RETINANET: the parameter names of the stock model, restated here."""
    from openset_rcnn_amd.host import modeling as M
    names = set(M.build_model(_cfg("base_rcnn_fpn.yaml")).state_dict())
    blocks = (3, 4, 6, 3)
    want = set()
    bn = ("weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var")
    want |= {f"backbone.bottom_up.stem.conv1.{l}" for l in bn}
    for si, nb in enumerate(blocks):
        for b in range(nb):
            for c in ("conv1", "conv2", "conv3") + (("shortcut",) if b == 0 else ()):
                want |= {f"backbone.bottom_up.res{si + 2}.{b}.{c}.{l}" for l in bn}
    want |= {f"backbone.fpn_{kind}{l}.{leaf}" for kind in ("lateral", "output") for l in (2, 3, 4, 5) for leaf in ("weight", "bias")}
    want |= {f"proposal_generator.rpn_head.{n}.{leaf}" for n in ("conv", "objectness_logits", "anchor_deltas") for leaf in ("weight", "bias")}
    want |= {f"roi_heads.{n}.{leaf}" for n in ("box_head.fc1", "box_head.fc2", "box_predictor.cls_score", "box_predictor.bbox_pred") for leaf in ("weight", "bias")}
    assert names == want
