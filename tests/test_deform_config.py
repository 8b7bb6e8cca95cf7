"""MODEL.RESNETS.DEFORM_ON_PER_STAGE / DEFORM_MODULATED / DEFORM_NUM_GROUPS without a GPU: the defaults, configs/mask_rcnn_dconv_c3_c5.yaml,
the model mirror's `conv2_offset` parameters under detectron2's names, checkpoints, the refusals (each naming its key) and what reaches
the engine."""
import os
import pickle

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3_C5 = "[False, True, True, True]"
MID = {2: 64, 3: 128, 4: 256, 5: 512}
BLOCKS = {2: 3, 3: 4, 4: 6, 5: 3}


def _cfg(osr, *opts, yaml="base_rcnn_fpn.yaml"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _offset_names(stages):
    return sorted(f"backbone.bottom_up.res{s}.{b}.conv2_offset.{p}" for s in stages for b in range(BLOCKS[s]) for p in ("weight", "bias"))


def test_defaults(osr):
    from openset_rcnn_amd.host.config import get_cfg
    from openset_rcnn_amd.host.engine import DEFAULT_CFG
    r = get_cfg().MODEL.RESNETS
    assert list(r.DEFORM_ON_PER_STAGE) == [False] * 4 and r.DEFORM_MODULATED is False and r.DEFORM_NUM_GROUPS == 1
    assert tuple(DEFAULT_CFG["deform_on_per_stage"]) == (False,) * 4 and DEFAULT_CFG["deform_modulated"] is False and DEFAULT_CFG["deform_num_groups"] == 1


def test_the_shipped_yaml(osr):
    cfg = _cfg(osr, yaml="mask_rcnn_dconv_c3_c5.yaml")
    assert list(cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE) == [False, True, True, True]
    assert cfg.MODEL.RESNETS.DEFORM_MODULATED is False and cfg.MODEL.RESNETS.DEFORM_NUM_GROUPS == 1 and cfg.MODEL.MASK_ON is True
    assert cfg.MODEL.ROI_HEADS.NAME == "StandardROIHeads" and cfg.MODEL.ROI_BOX_HEAD.NUM_FC == 2  # the rest is base_rcnn_fpn.yaml's


@pytest.mark.parametrize("yaml", ["base_rcnn_fpn.yaml", "voc_coco.yaml", "cascade_rcnn_fpn.yaml"])
def test_every_family_builds_with_and_without_the_flags(osr, yaml):
    from openset_rcnn_amd.host import modeling as M
    plain = M.build_model(_cfg(osr, yaml=yaml))
    assert not [k for k in plain.state_dict() if "conv2_offset" in k]
    assert plain._eng_cfg["deform_on_per_stage"] == (False,) * 4
    model = M.build_model(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, yaml=yaml))
    assert sorted(k for k in model.state_dict() if "conv2_offset" in k) == _offset_names((3, 4, 5))
    assert sorted(k for k in model.state_dict() if "conv2_offset" not in k) == sorted(plain.state_dict())
    for m in (model, model.backbone, model.roi_heads, model.proposal_generator.rpn_head):
        assert m._eng_cfg["deform_on_per_stage"] == (False, True, True, True), type(m)


@pytest.mark.parametrize("modulated, groups", [(False, 1), (True, 1), (False, 2), (True, 4)])
def test_conv2_offset_parameters(osr, modulated, groups):
    """Exactly the extra conv2_offset.{weight,bias} keys, (18 G or 27 G, mid, 3, 3), zero; conv2 keeps its names, shape and FrozenBN."""
    from openset_rcnn_amd.host import modeling as M
    plain = M.build_model(_cfg(osr)).state_dict()
    sd = M.build_model(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, "MODEL.RESNETS.DEFORM_MODULATED", str(modulated),
                            "MODEL.RESNETS.DEFORM_NUM_GROUPS", str(groups))).state_dict()
    assert sorted(set(sd) - set(plain)) == _offset_names((3, 4, 5)) and not set(plain) - set(sd)
    ch = (27 if modulated else 18) * groups
    for s in (3, 4, 5):
        for b in range(BLOCKS[s]):
            pre = f"backbone.bottom_up.res{s}.{b}."
            assert tuple(sd[pre + "conv2_offset.weight"].shape) == (ch, MID[s], 3, 3) and tuple(sd[pre + "conv2_offset.bias"].shape) == (ch,)
            assert not sd[pre + "conv2_offset.weight"].any() and not sd[pre + "conv2_offset.bias"].any()
            assert tuple(sd[pre + "conv2.weight"].shape) == (MID[s], MID[s], 3, 3) and pre + "conv2.norm.running_var" in sd
    assert all(sd[k].shape == plain[k].shape for k in plain)


def test_all_false_leaves_the_key_set_unchanged(osr):
    from openset_rcnn_amd.host import modeling as M
    a = M.build_model(_cfg(osr)).state_dict()
    b = M.build_model(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[False, False, False, False]", "MODEL.RESNETS.DEFORM_MODULATED", "True",
                           "MODEL.RESNETS.DEFORM_NUM_GROUPS", "2")).state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)


def test_random_params_carry_the_offset_layers(osr):
    from openset_rcnn_amd.host.weights import deform_offset_params, random_params
    plain = random_params(0)
    p = random_params(0, deform_on_per_stage=(False, True, True, True), deform_modulated=True, deform_num_groups=2, deform_std=1.0)
    assert sorted(set(p) - set(plain)) == _offset_names((3, 4, 5)) and all(torch.equal(p[k], plain[k]) for k in plain)
    assert tuple(p["backbone.bottom_up.res4.5.conv2_offset.weight"].shape) == (54, 256, 3, 3) and p["backbone.bottom_up.res4.5.conv2_offset.weight"].any()
    zero = deform_offset_params((True, False, False, False))
    assert sorted(zero) == _offset_names((2,)) and not any(v.any() for v in zero.values())


def test_checkpoint_round_trip(osr, tmp_path):
    """A `.pth` as DetectionCheckpointer writes it and detectron2's own `.pkl` form, both with conv2_offset tensors, through
    load_checkpoint / load_into; a converted-torchvision style backbone name maps too."""
    from openset_rcnn_amd.host import checkpoint as CK
    from openset_rcnn_amd.host import modeling as M
    cfg = _cfg(osr, yaml="mask_rcnn_dconv_c3_c5.yaml")
    a, b, c = M.build_model(cfg), M.build_model(cfg), M.build_model(cfg)
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.randn(v.shape, generator=g) * 0.1 if "conv2_offset" in k else v.clone()) for k, v in a.state_dict().items()}
    pth = tmp_path / "model_final.pth"
    torch.save({"model": sd, "iteration": 1}, pth)
    assert CK.load_into(b, CK.load_checkpoint(str(pth)), strict=True) == ([], [])
    pkl = tmp_path / "model_final.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "test"}, f)
    assert CK.load_into(c, CK.load_checkpoint(str(pkl)), strict=True) == ([], [])
    for m in (b, c):
        got = m.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert got["backbone.bottom_up.res5.2.conv2_offset.weight"].any()
    assert CK.convert_d2_backbone_name("res3.1.conv2_offset.bias") == "backbone.bottom_up.res3.1.conv2_offset.bias"
    # a checkpoint without the offset layers leaves them at their zero initialisation and reports them missing
    plain = M.build_model(_cfg(osr, "MODEL.MASK_ON", "True")).state_dict()
    missing, unexpected = CK.load_into(M.build_model(cfg), {k: v for k, v in plain.items()})
    assert sorted(missing) == _offset_names((3, 4, 5)) and not unexpected


@pytest.mark.parametrize("opts, key", [
    (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[False, True, True]"), "DEFORM_ON_PER_STAGE"),
    (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[0, 1, 1, 1]"), "DEFORM_ON_PER_STAGE"),
    (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, "MODEL.RESNETS.DEFORM_NUM_GROUPS", "0"), "DEFORM_NUM_GROUPS"),
    (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, "MODEL.RESNETS.DEFORM_NUM_GROUPS", "3"), "DEFORM_NUM_GROUPS"),      # 128 % 3
    (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, "MODEL.RESNETS.DEFORM_NUM_GROUPS", "32"), "DEFORM_NUM_GROUPS"),     # 128 / 32 = 4 channels
    (("MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[True, False, False, False]", "MODEL.RESNETS.DEFORM_NUM_GROUPS", "16"), "DEFORM_NUM_GROUPS"),  # 64 / 16
], ids=["three-flags", "ints", "zero-groups", "indivisible", "four-channel-groups", "res2-groups"])
def test_bad_values_name_their_key(osr, opts, key):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match=key):
        M.build_model(_cfg(osr, *opts))


def test_group_counts_that_fit_build(osr):
    from openset_rcnn_amd.host import modeling as M
    M.build_model(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, "MODEL.RESNETS.DEFORM_NUM_GROUPS", "16"))   # 128 / 16 = 8
    M.build_model(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[False, False, False, True]", "MODEL.RESNETS.DEFORM_NUM_GROUPS", "64"))


def test_option_check_of_the_engine(osr):
    from openset_rcnn_amd.host.engine import check_deform_options
    assert check_deform_options([False, True, True, True], True, 2) == (False, True, True, True)
    with pytest.raises(ValueError, match="DEFORM_MODULATED"):
        check_deform_options((False,) * 4, 1, 1)
    with pytest.raises(ValueError, match="DEFORM_NUM_GROUPS"):
        check_deform_options((False,) * 4, False, True)


@pytest.mark.parametrize("yaml", ["mask_rcnn_dconv_c3_c5.yaml", "voc_coco.yaml", "cascade_rcnn_fpn.yaml"])
def test_training_is_refused_by_name(osr, yaml):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Boxes, Instances
    model = M.build_model(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, yaml=yaml))
    inst = Instances((64, 64), gt_boxes=Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]])), gt_classes=torch.tensor([1]))
    data = [{"image": torch.zeros(3, 64, 64, dtype=torch.uint8), "instances": inst}]
    with pytest.raises(NotImplementedError, match="MODEL.RESNETS.DEFORM_ON_PER_STAGE"):
        model.make_trainer()
    with pytest.raises(NotImplementedError, match="MODEL.RESNETS.DEFORM_ON_PER_STAGE"):
        model.losses_forward(data)
    model.train()
    with pytest.raises(NotImplementedError, match="MODEL.RESNETS.DEFORM_ON_PER_STAGE"):
        model(data)


def test_trainer_and_engine_refuse_a_deformable_stage(osr):
    """Below the model: the trainer's constructor and the engine's training forward refuse on their engine configuration alone."""
    from openset_rcnn_amd.host.engine import refuse_deform_training
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    with pytest.raises(NotImplementedError, match="MODEL.RESNETS.DEFORM_ON_PER_STAGE"):
        OpensetRCNNTrainer({}, dict(deform_on_per_stage=(False, False, False, True)))
    refuse_deform_training(dict(deform_on_per_stage=(False,) * 4))
    refuse_deform_training({})


def test_engine_cfg_carries_the_three_values(osr):
    from openset_rcnn_amd.host import modeling as M
    e = M.engine_cfg_from(_cfg(osr, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", C3_C5, "MODEL.RESNETS.DEFORM_MODULATED", "True",
                               "MODEL.RESNETS.DEFORM_NUM_GROUPS", "2"))
    assert e["deform_on_per_stage"] == (False, True, True, True) and e["deform_modulated"] is True and e["deform_num_groups"] == 2
    e = M.engine_cfg_from(_cfg(osr))
    assert e["deform_on_per_stage"] == (False,) * 4 and e["deform_modulated"] is False and e["deform_num_groups"] == 1


def test_split_convolutions_refuse_a_deformable_stage(osr):
    """conv="split" has no deformable form: ValueError when the engine is built, before anything is packed."""
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    with pytest.raises(ValueError, match="DEFORM_ON_PER_STAGE"):
        OpensetRCNNEngine({}, dict(deform_on_per_stage=(False, True, True, True)), torch.float32, "cpu", conv="split")
