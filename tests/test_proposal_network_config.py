"""MODEL.META_ARCHITECTURE "ProposalNetwork" on the host side, without a GPU: configs/rpn_R_50_FPN.yaml, the registered name, the
parameter names (the full model's minus roi_heads.*, so detectron2's rpn_R_50_FPN checkpoints load by name), a full model's checkpoint
loaded with its RoI-head keys reported as unexpected, and every refusal by its key."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 'MODEL.META_ARCHITECTURE "ProposalNetwork"'
VARIANTS = {
    "fpn": ("rpn_R_50_FPN.yaml", []),
    "c4": ("faster_rcnn_R_50_C4.yaml", ["MODEL.META_ARCHITECTURE", "ProposalNetwork"]),
    "clsfree": ("voc_coco.yaml", ["MODEL.META_ARCHITECTURE", "ProposalNetwork"]),
}


def _cfg(*opts, yaml="rpn_R_50_FPN.yaml"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _pair(variant):
    """-> (the ProposalNetwork, the full model of the same yaml)."""
    from openset_rcnn_amd.host import modeling as M
    yaml, opts = VARIANTS[variant]
    full_opts = ["MODEL.META_ARCHITECTURE", "GeneralizedRCNN"] if variant == "fpn" else []
    return M.build_model(_cfg(*opts, yaml=yaml)), M.build_model(_cfg(*full_opts, yaml=yaml))


def test_the_shipped_yaml_is_the_base_with_two_changes(osr):
    ours, base = _cfg(), _cfg(yaml="base_rcnn_fpn.yaml")
    assert ours.MODEL.META_ARCHITECTURE == "ProposalNetwork" and ours.MODEL.RPN.POST_NMS_TOPK_TEST == 2000
    assert base.MODEL.META_ARCHITECTURE == "GeneralizedRCNN" and base.MODEL.RPN.POST_NMS_TOPK_TEST == 1000
    base.MODEL.META_ARCHITECTURE, base.MODEL.RPN.POST_NMS_TOPK_TEST = "ProposalNetwork", 2000
    assert ours == base


def test_the_name_is_registered(osr):
    from openset_rcnn_amd.host import modeling as M
    assert "ProposalNetwork" in M.META_ARCH_REGISTRY
    assert not issubclass(M.ProposalNetwork, M.GeneralizedRCNN)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_state_dict_is_the_full_models_without_roi_heads(osr, variant):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.engine_c4 import C4RCNNEngine
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    model, full = _pair(variant)
    assert type(model) is M.ProposalNetwork and not hasattr(model, "roi_heads")
    sd, fsd = model.state_dict(), full.state_dict()
    assert [k for k in fsd if k.startswith("roi_heads.")]
    assert list(sd) == [k for k in fsd if not k.startswith("roi_heads.")]
    assert all(k.startswith(("backbone.", "proposal_generator.")) for k in sd)
    assert all(tuple(sd[k].shape) == tuple(fsd[k].shape) for k in sd)
    assert model._engine_cls is {"fpn": StandardRCNNEngine, "c4": C4RCNNEngine, "clsfree": OpensetRCNNEngine}[variant]
    assert model._engine_cls is model.proposal_generator.rpn_head._engine_cls
    if variant == "fpn":
        assert model._eng_cfg["post_nms_topk_test"] == 2000 and model._eng_cfg["pre_nms_topk_test"] == 1000
    if variant == "c4":
        assert model._eng_cfg["anchor_sizes"] == ((32.0, 64.0, 128.0, 256.0, 512.0),) and model._eng_cfg["pre_nms_topk_test"] == 6000


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_full_models_checkpoint_loads_with_its_roi_heads_unexpected(osr, variant, tmp_path):
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into
    torch.manual_seed(11)
    model, full = _pair(variant)
    fsd = {k: v.clone() for k, v in full.state_dict().items()}
    path = str(tmp_path / "full.pth")
    torch.save({"model": fsd, "iteration": 3}, path)
    missing, unexpected = load_into(model, load_checkpoint(path))
    assert not missing
    assert sorted(unexpected) == sorted(k for k in fsd if k.startswith("roi_heads."))
    got = model.state_dict()
    assert all(torch.equal(got[k], fsd[k]) for k in got)
    # its own checkpoint (what an rpn_R_50_FPN zoo file holds) loads by name, strictly
    own = str(tmp_path / "rpn.pth")
    torch.save({"model": {k: v.clone() for k, v in got.items()}}, own)
    torch.manual_seed(12)
    again, _ = _pair(variant)
    assert load_into(again, load_checkpoint(own), strict=True) == ([], [])
    assert all(torch.equal(again.state_dict()[k], fsd[k]) for k in got)


REFUSALS = [
    (["MODEL.MASK_ON", "True"], "MODEL.MASK_ON"),
    (["MODEL.KEYPOINT_ON", "True"], "MODEL.KEYPOINT_ON"),
    (["TEST.AUG.ENABLED", "True"], "TEST.AUG"),
]


@pytest.mark.parametrize("opts,key", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_refusals_name_their_key(osr, opts, key):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match=key):
        M.build_model(_cfg(*opts))


def test_the_c4_select_limit_is_refused_by_key(osr):
    from openset_rcnn_amd.host import modeling as M
    yaml, opts = VARIANTS["c4"]
    M.build_model(_cfg(*opts, "MODEL.RPN.PRE_NMS_TOPK_TEST", "8192", yaml=yaml))
    with pytest.raises(ValueError, match="MODEL.RPN.PRE_NMS_TOPK_TEST"):
        M.build_model(_cfg(*opts, "MODEL.RPN.PRE_NMS_TOPK_TEST", "12000", yaml=yaml))  # the zoo's rpn_R_50_C4 value


def test_training_is_refused_by_name(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.solver import build_optimizer
    cfg = _cfg()
    model = M.build_model(cfg)
    for call in (model.make_trainer, model.trainer, lambda: model.losses_forward([])):
        with pytest.raises(NotImplementedError, match=KEY):
            call()
    model.train()
    with pytest.raises(NotImplementedError, match=KEY):
        model([])
    with pytest.raises(NotImplementedError, match=KEY):
        build_optimizer(cfg, model).step()


def test_tta_wrapper_refuses_the_model(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    model = M.build_model(_cfg()).eval()
    with pytest.raises(ValueError, match="TEST.AUG"):
        GeneralizedRCNNWithTTA(_cfg(), model)


def test_no_engine_without_a_gpu(osr):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg()).eval()
    with pytest.raises(osr.OsrError):
        model([{"image": torch.zeros(3, 64, 64, dtype=torch.uint8)}])
