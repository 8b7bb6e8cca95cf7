"""MODEL.MASK_ON for the stock heads (Base-RCNN-FPN.yaml:29-33), CPU side: the model builds with a [d2]-named mask head
(mask_fcn1..N, deconv, predictor), checkpoints round-trip, what has no kernel is refused when the model is built (KEYPOINT_ON,
ROI_MASK_HEAD.NORM, a pooler the RoIAlign kernels do not have) and training is refused by name (the mask loss), while MASK_ON False
builds what it always built."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _mask_keys(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith("roi_heads.mask_head.")}


def test_mask_on_builds_with_detectron2_names(osr):
    from openset_rcnn_amd.host import modeling as M
    want = {}
    for i in range(1, 5):
        want[f"roi_heads.mask_head.mask_fcn{i}.weight"] = (256, 256, 3, 3)
        want[f"roi_heads.mask_head.mask_fcn{i}.bias"] = (256,)
    want["roi_heads.mask_head.deconv.weight"] = (256, 256, 2, 2)
    want["roi_heads.mask_head.deconv.bias"] = (256,)
    # the yaml's CLS_AGNOSTIC_MASK True: one map
    agn = M.build_model(_cfg("MODEL.MASK_ON", "True"))
    assert _mask_keys(agn) == {**want, "roi_heads.mask_head.predictor.weight": (1, 256, 1, 1), "roi_heads.mask_head.predictor.bias": (1,)}
    assert "MaskRCNNConvUpsampleHead" in M.ROI_MASK_HEAD_REGISTRY
    # class-specific: NUM_CLASSES maps
    spec = M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", "False", "MODEL.ROI_HEADS.NUM_CLASSES", "5"))
    assert _mask_keys(spec) == {**want, "roi_heads.mask_head.predictor.weight": (5, 256, 1, 1), "roi_heads.mask_head.predictor.bias": (5,)}
    # NUM_CONV / CONV_DIM are read
    small = M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.NUM_CONV", "1", "MODEL.ROI_MASK_HEAD.CONV_DIM", "128"))
    assert _mask_keys(small) == {"roi_heads.mask_head.mask_fcn1.weight": (128, 256, 3, 3), "roi_heads.mask_head.mask_fcn1.bias": (128,),
                                 "roi_heads.mask_head.deconv.weight": (128, 128, 2, 2), "roi_heads.mask_head.deconv.bias": (128,),
                                 "roi_heads.mask_head.predictor.weight": (1, 128, 1, 1), "roi_heads.mask_head.predictor.bias": (1,)}
    # the mask pooler's keys reach the engine configuration
    alt = M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.POOLER_TYPE", "ROIAlign", "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", "2",
                             "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", "12"))
    ec = alt.roi_heads._eng_cfg
    assert (ec["mask_pooler_resolution"], ec["mask_pooler_aligned"], ec["mask_pooler_sampling_ratio"]) == (12, False, 2)
    assert (ec["pooler_resolution"], ec["pooler_aligned"], ec["pooler_sampling_ratio"]) == (7, True, 0)  # the box pooler keeps its own


def test_mask_off_has_no_mask_parameters(osr):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg())
    assert _mask_keys(model) == {} and not hasattr(model.roi_heads, "mask_head") and model.roi_heads.mask_on is False
    on = M.build_model(_cfg("MODEL.MASK_ON", "True"))
    off_keys = set(model.state_dict())
    assert off_keys == {k for k in on.state_dict() if not k.startswith("roi_heads.mask_head.")}


def test_state_dict_round_trips_through_load_into(osr):
    from openset_rcnn_amd.host import checkpoint, modeling as M
    torch.manual_seed(3)
    a = M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", "False", "MODEL.ROI_HEADS.NUM_CLASSES", "5"))
    state = {k: v.clone() for k, v in a.state_dict().items()}
    for k in _mask_keys(a):
        state[k] = torch.randn_like(state[k])
    b = M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", "False", "MODEL.ROI_HEADS.NUM_CLASSES", "5"))
    missing, unexpected = checkpoint.load_into(b, state)
    assert missing == [] and unexpected == []
    got = b.state_dict()
    for k in _mask_keys(a):
        assert torch.equal(got[k], state[k]), k
    # a box-only checkpoint leaves the mask head at its initial values and names what is missing
    box_only = {k: v for k, v in state.items() if not k.startswith("roi_heads.mask_head.")}
    missing, unexpected = checkpoint.load_into(M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", "False",
                                                                   "MODEL.ROI_HEADS.NUM_CLASSES", "5")), box_only)
    assert sorted(missing) == sorted(_mask_keys(a)) and unexpected == []
    # a class-agnostic model refuses the class-specific predictor
    with pytest.raises(ValueError, match="predictor"):
        checkpoint.load_into(M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_HEADS.NUM_CLASSES", "5")), state)


def test_what_has_no_kernel_is_refused_at_build_time(osr):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match="KEYPOINT_ON"):
        M.build_model(_cfg("MODEL.KEYPOINT_ON", "True"))
    with pytest.raises(ValueError, match="KEYPOINT_ON"):
        M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.KEYPOINT_ON", "True"))
    with pytest.raises(ValueError, match="ROI_MASK_HEAD.NORM"):
        M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.NORM", "GN"))
    # the mask pooler goes through the box pooler's checks
    with pytest.raises(ValueError, match="ROI_MASK_HEAD.POOLER_TYPE"):
        M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.POOLER_TYPE", "ROIPool"))
    with pytest.raises(ValueError, match="ROI_MASK_HEAD.POOLER_SAMPLING_RATIO"):
        M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", "-1"))
    with pytest.raises(ValueError, match="ROI_MASK_HEAD.POOLER_RESOLUTION"):
        M.build_model(_cfg("MODEL.MASK_ON", "True", "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", "15"))
    # ... and none of these keys matters while the branch is off
    M.build_model(_cfg("MODEL.ROI_MASK_HEAD.NORM", "GN", "MODEL.ROI_MASK_HEAD.POOLER_TYPE", "ROIPool"))


def test_training_is_refused_naming_the_mask_loss(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Boxes, ImageList, Instances
    model = M.build_model(_cfg("MODEL.MASK_ON", "True"))
    with pytest.raises(NotImplementedError, match="mask loss"):
        model.make_trainer()
    model.train()
    gt = Instances((64, 64), gt_boxes=Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]])), gt_classes=torch.tensor([1]))
    with pytest.raises(NotImplementedError, match="mask loss"):
        model([{"image": torch.zeros(3, 64, 64), "instances": gt}])
    # the RoI heads' own training-mode forward
    prop = Instances((64, 64), proposal_boxes=Boxes(torch.tensor([[2.0, 2.0, 30.0, 30.0]])), objectness_logits=torch.tensor([1.0]))
    feats = {k: torch.zeros(1, 256, 64 // s, 64 // s) for k, s in (("p2", 4), ("p3", 8), ("p4", 16), ("p5", 32))}
    with pytest.raises(NotImplementedError, match="mask loss"):
        model.roi_heads(ImageList(torch.zeros(1, 3, 64, 64), [(64, 64)]), feats, [prop], [gt])
    # MASK_ON False trains as before: the refusal is the mask branch's (no GPU here, so the trainer stops at the device check)
    with pytest.raises(osr.OsrError):
        M.build_model(_cfg()).make_trainer()


def test_deconv_packer_is_a_permutation(osr):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    w = torch.arange(128 * 64 * 4, dtype=torch.float32).view(128, 64, 2, 2)
    for dt, e in ((torch.float32, 4), (torch.float16, 8)):
        p = pack_deconv_weight(w, dt).float()
        assert p.shape == (4, 2, 128 // (2 * e), 2, 32, e)
        if dt == torch.float32:  # (fp16 cannot hold the counter exactly)
            assert torch.equal(p.flatten().sort().values, w.flatten())
        for (t, nb, kb, half, nl, ke) in ((0, 0, 0, 0, 0, 0), (3, 1, 128 // (2 * e) - 1, 1, 31, e - 1), (2, 1, 1, 0, 7, 3)):
            n, k = nb * 32 + nl, (kb * 2 + half) * e + ke
            assert p[t, nb, kb, half, nl, ke] == w[k, n, t // 2, t % 2].to(dt).float()
    with pytest.raises(ValueError):
        pack_deconv_weight(torch.zeros(96, 64, 2, 2), torch.float16)
