"""MODEL.KEYPOINT_ON for the stock heads (configs/keypoint_rcnn_fpn.yaml), CPU side: the model builds with a [d2]-named keypoint head
(conv_fcn1..N, score_lowres), checkpoints round-trip, what the fused tail does not take is refused by key name when the model is
built, KEYPOINT_ON with any NUM_CLASSES but 1 stays refused, training is refused by name (the keypoint loss), and KEYPOINT_ON False
builds what it always built."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = "roi_heads.keypoint_head."


def _cfg(*opts, yaml="keypoint_rcnn_fpn.yaml"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _kp_keys(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith(PRE)}


def _want(dims, k, cin=256):
    want, cur = {}, cin
    for i, d in enumerate(dims):
        want[f"{PRE}conv_fcn{i + 1}.weight"] = (d, cur, 3, 3)
        want[f"{PRE}conv_fcn{i + 1}.bias"] = (d,)
        cur = d
    want[PRE + "score_lowres.weight"] = (cur, k, 4, 4)
    want[PRE + "score_lowres.bias"] = (k,)
    return want


def test_the_yaml_builds_with_detectron2_names(osr):
    from openset_rcnn_amd.host import modeling as M
    cfg = _cfg()
    kh = cfg.MODEL.ROI_KEYPOINT_HEAD
    assert (kh.NAME, kh.POOLER_RESOLUTION, kh.POOLER_SAMPLING_RATIO, kh.POOLER_TYPE) == ("KRCNNConvDeconvUpsampleHead", 14, 0, "ROIAlignV2")
    assert tuple(kh.CONV_DIMS) == (512,) * 8 and kh.NUM_KEYPOINTS == 17 and kh.MIN_KEYPOINTS_PER_IMAGE == 1
    assert kh.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS is True and kh.LOSS_WEIGHT == 1.0 and list(cfg.TEST.KEYPOINT_OKS_SIGMAS) == []
    assert cfg.MODEL.KEYPOINT_ON is True and cfg.MODEL.ROI_HEADS.NUM_CLASSES == 1 and cfg.MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA == 0.5
    assert cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN == 1500
    assert tuple(cfg.DATASETS.TRAIN) == ("keypoints_coco_2017_train",) and tuple(cfg.DATASETS.TEST) == ("keypoints_coco_2017_val",)
    model = M.build_model(cfg)
    assert _kp_keys(model) == _want((512,) * 8, 17)
    assert "KRCNNConvDeconvUpsampleHead" in M.ROI_KEYPOINT_HEAD_REGISTRY and model.roi_heads.keypoint_on is True
    sd = model.state_dict()
    assert sd["roi_heads.box_predictor.cls_score.weight"].shape[0] == 2  # one class + background
    for k in _kp_keys(model):
        if k.endswith(".bias"):
            assert float(sd[k].abs().max()) == 0.0, k
    # kaiming_normal_(fan_out, relu): std = sqrt(2 / (cout * kh * kw)); score_lowres' fan_out is size(0) * 16 as torch counts it
    w = sd[PRE + "conv_fcn2.weight"]
    assert abs(float(w.std()) / (2.0 / (512 * 9)) ** 0.5 - 1.0) < 0.02
    w = sd[PRE + "score_lowres.weight"]
    assert abs(float(w.std()) / (2.0 / (512 * 16)) ** 0.5 - 1.0) < 0.05
    # CONV_DIMS / NUM_KEYPOINTS are read
    small = M.build_model(_cfg("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(128, 64)", "MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS", "5"))
    assert _kp_keys(small) == _want((128, 64), 5)
    # the keypoint pooler's keys reach the engine configuration, the box pooler keeps its own
    alt = M.build_model(_cfg("MODEL.ROI_KEYPOINT_HEAD.POOLER_TYPE", "ROIAlign", "MODEL.ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO", "2",
                             "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", "12", "MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(64,)"))
    ec = alt.roi_heads._eng_cfg
    assert (ec["keypoint_pooler_resolution"], ec["keypoint_pooler_aligned"], ec["keypoint_pooler_sampling_ratio"]) == (12, False, 2)
    assert (ec["pooler_resolution"], ec["pooler_aligned"], ec["pooler_sampling_ratio"]) == (7, True, 0)
    # MASK_ON may be on as well
    both = M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(64,)"))
    assert _kp_keys(both) == _want((64,), 17) and "roi_heads.mask_head.deconv.weight" in both.state_dict()


def test_state_dict_round_trips_through_load_into(osr):
    from openset_rcnn_amd.host import checkpoint, modeling as M
    torch.manual_seed(3)
    opts = ("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(128, 64)")
    a = M.build_model(_cfg(*opts))
    state = {k: v.clone() for k, v in a.state_dict().items()}
    for k in _kp_keys(a):
        state[k] = torch.randn_like(state[k])
    b = M.build_model(_cfg(*opts))
    missing, unexpected = checkpoint.load_into(b, state)
    assert missing == [] and unexpected == []
    got = b.state_dict()
    for k in _kp_keys(a):
        assert torch.equal(got[k], state[k]), k
    # a box-only checkpoint leaves the keypoint head at its initial values and names what is missing
    box_only = {k: v for k, v in state.items() if not k.startswith(PRE)}
    missing, unexpected = checkpoint.load_into(M.build_model(_cfg(*opts)), box_only)
    assert sorted(missing) == sorted(_kp_keys(a)) and unexpected == []


@pytest.mark.parametrize("opts, word", [
    (("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(512, 96)"), "ROI_KEYPOINT_HEAD.CONV_DIMS"),
    (("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(576,)"), "ROI_KEYPOINT_HEAD.CONV_DIMS"),
    (("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "()"), "ROI_KEYPOINT_HEAD.CONV_DIMS"),
    (("MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS", "0"), "ROI_KEYPOINT_HEAD.NUM_KEYPOINTS"),
    (("MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS", "33"), "ROI_KEYPOINT_HEAD.NUM_KEYPOINTS"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", "7"), "ROI_KEYPOINT_HEAD.POOLER_RESOLUTION"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", "15"), "ROI_KEYPOINT_HEAD.POOLER_RESOLUTION"),
    (("MODEL.ROI_KEYPOINT_HEAD.NAME", "KRCNNConvHead"), "ROI_KEYPOINT_HEAD.NAME"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_TYPE", "ROIPool"), "ROI_KEYPOINT_HEAD.POOLER_TYPE"),
    (("MODEL.ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO", "-1"), "ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO"),
])
def test_what_the_kernels_do_not_take_is_refused_by_key_name(osr, opts, word):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match=word):
        M.build_model(_cfg(*opts))
    # ... and none of these keys matters while the branch is off
    M.build_model(_cfg("MODEL.KEYPOINT_ON", "False", *opts))


def test_other_class_counts_and_other_heads_stay_refused(osr):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match="KEYPOINT_ON") as e:
        M.build_model(_cfg("MODEL.ROI_HEADS.NUM_CLASSES", "80"))
    assert "MODEL.KEYPOINT_ON" in str(e.value) and "ROI_HEADS.NUM_CLASSES 1" in str(e.value)
    with pytest.raises(ValueError, match="KEYPOINT_ON"):
        M.build_model(_cfg("MODEL.ROI_HEADS.NUM_CLASSES", "2"))
    with pytest.raises(ValueError, match="KEYPOINT_ON"):  # Cascade R-CNN with one class: still no keypoint branch
        M.build_model(_cfg("MODEL.KEYPOINT_ON", "True", "MODEL.ROI_HEADS.NUM_CLASSES", "1", yaml="cascade_rcnn_fpn.yaml"))


def test_training_is_refused_naming_the_keypoint_loss(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Boxes, ImageList, Instances
    model = M.build_model(_cfg("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(64,)"))
    with pytest.raises(NotImplementedError, match="keypoint") as e:
        model.make_trainer()
    assert "keypoint_rcnn_loss" in str(e.value)
    with pytest.raises(NotImplementedError, match="keypoint"):
        model.trainer()
    gt = Instances((64, 64), gt_boxes=Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]])), gt_classes=torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="keypoint"):
        model.losses_forward([{"image": torch.zeros(3, 64, 64), "instances": gt}])
    model.train()
    with pytest.raises(NotImplementedError, match="keypoint"):
        model([{"image": torch.zeros(3, 64, 64), "instances": gt}])
    # the RoI heads' own training-mode forward
    prop = Instances((64, 64), proposal_boxes=Boxes(torch.tensor([[2.0, 2.0, 30.0, 30.0]])), objectness_logits=torch.tensor([1.0]))
    feats = {k: torch.zeros(1, 256, 64 // s, 64 // s) for k, s in (("p2", 4), ("p3", 8), ("p4", 16), ("p5", 32))}
    with pytest.raises(NotImplementedError, match="keypoint"):
        model.roi_heads(ImageList(torch.zeros(1, 3, 64, 64), [(64, 64)]), feats, [prop], [gt])
    # KEYPOINT_ON False trains as before (no GPU here, so the trainer stops at the device check)
    with pytest.raises(osr.OsrError):
        M.build_model(_cfg("MODEL.KEYPOINT_ON", "False")).make_trainer()


def test_keypoint_off_builds_the_parameter_set_it_built_before(osr):
    from openset_rcnn_amd.host import modeling as M
    off = M.build_model(_cfg("MODEL.KEYPOINT_ON", "False"))
    assert _kp_keys(off) == {} and not hasattr(off.roi_heads, "keypoint_head") and off.roi_heads.keypoint_on is False
    on = M.build_model(_cfg("MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS", "(64,)"))
    assert set(off.state_dict()) == {k for k in on.state_dict() if not k.startswith(PRE)}
    # the stock 80-class file: the same keys as a one-class model without the branch, and no keypoint entry anywhere
    base = M.build_model(_cfg(yaml="base_rcnn_fpn.yaml"))
    assert set(base.state_dict()) == set(off.state_dict()) and not any("keypoint" in k for k in base.state_dict())


def test_keypoint_deconv_packer_places_every_element(osr):
    from openset_rcnn_amd.host.weights import pack_keypoint_deconv_weight
    w = torch.arange(128 * 5 * 16, dtype=torch.float32).view(128, 5, 4, 4) + 1.0
    for dt, e in ((torch.float32, 4), (torch.float16, 8)):
        p = pack_keypoint_deconv_weight(w, dt).float()
        assert p.shape == (16, 128 // (2 * e), 2, 32, e)
        assert float(p[:, :, :, 5:].abs().max()) == 0.0  # the padding of k to the MFMA's N
        if dt == torch.float32:
            assert torch.equal(p[:, :, :, :5].flatten().sort().values, w.flatten())
        for (tap, kb, half, j, ke) in ((0, 0, 0, 0, 0), (15, 128 // (2 * e) - 1, 1, 4, e - 1), (6, 1, 0, 3, 2)):
            c = (kb * 2 + half) * e + ke
            assert p[tap, kb, half, j, ke] == w[c, j, tap // 4, tap % 4].to(dt).float()
    for bad in ((96, 5, 4, 4), (64, 33, 4, 4), (64, 5, 2, 2)):
        with pytest.raises(ValueError):
            pack_keypoint_deconv_weight(torch.zeros(bad), torch.float16)
