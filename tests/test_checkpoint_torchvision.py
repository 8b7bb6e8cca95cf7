"""Checkpoint import of torchvision's ImageNet ResNet-50 (host/checkpoint.py): the raw resnet50 state dict saved as .pth and the
.pkl of detectron2's tools/convert-torchvision-to-d2.py, fabricated here with the right names and shapes; the MSRA .pkl and
d2 .pth paths are unchanged."""
import logging
import os
import pickle

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS, MID = (3, 4, 6, 3), (64, 128, 256, 512)


def torchvision_r50_state(seed=0):
    """{name: tensor} of torchvision.models.resnet50().state_dict() (names, shapes and dtypes), random values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def bn(pre, c):
        sd[pre + ".weight"] = torch.rand(c, generator=g) + 0.5
        sd[pre + ".bias"] = torch.randn(c, generator=g)
        sd[pre + ".running_mean"] = torch.randn(c, generator=g)
        sd[pre + ".running_var"] = torch.rand(c, generator=g) + 0.1
        sd[pre + ".num_batches_tracked"] = torch.tensor(7)
    sd["conv1.weight"] = torch.randn(64, 3, 7, 7, generator=g)
    bn("bn1", 64)
    cin = 64
    for li, (nb, mid) in enumerate(zip(BLOCKS, MID)):
        for b in range(nb):
            pre = f"layer{li + 1}.{b}"
            sd[pre + ".conv1.weight"] = torch.randn(mid, cin, 1, 1, generator=g)
            bn(pre + ".bn1", mid)
            sd[pre + ".conv2.weight"] = torch.randn(mid, mid, 3, 3, generator=g)
            bn(pre + ".bn2", mid)
            sd[pre + ".conv3.weight"] = torch.randn(mid * 4, mid, 1, 1, generator=g)
            bn(pre + ".bn3", mid * 4)
            if b == 0:
                sd[pre + ".downsample.0.weight"] = torch.randn(mid * 4, cin, 1, 1, generator=g)
                bn(pre + ".downsample.1", mid * 4)
            cin = mid * 4
    sd["fc.weight"] = torch.randn(1000, 2048, generator=g)
    sd["fc.bias"] = torch.randn(1000, generator=g)
    return sd


def d2_converted(sd):
    """What tools/convert-torchvision-to-d2.py writes: the same tensors under d2 backbone names without the prefix, as ndarrays."""
    out = {}
    for k, v in sd.items():
        old = k
        if "layer" not in k:
            k = "stem." + k
        for t in range(4):
            k = k.replace(f"layer{t + 1}", f"res{t + 2}")
        for t in range(3):
            k = k.replace(f"bn{t + 1}", f"conv{t + 1}.norm")
        k = k.replace("downsample.0", "shortcut").replace("downsample.1", "shortcut.norm")
        out[k] = v.numpy()
        assert old  # (every name is carried, fc and num_batches_tracked included)
    return {"model": out, "__author__": "torchvision", "matching_heuristics": True}


def _model(osr, stride_in_1x1):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "voc_coco.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.RESNETS.STRIDE_IN_1X1", str(stride_in_1x1)])
    return M.build_model(cfg)


def test_torchvision_name_mapping(osr):
    from openset_rcnn_amd.host.checkpoint import convert_d2_backbone_name, convert_torchvision_name
    bu = "backbone.bottom_up."
    assert convert_torchvision_name("conv1.weight") == bu + "stem.conv1.weight"
    assert convert_torchvision_name("bn1.running_var") == bu + "stem.conv1.norm.running_var"
    assert convert_torchvision_name("layer1.0.conv2.weight") == bu + "res2.0.conv2.weight"
    assert convert_torchvision_name("layer3.5.bn3.bias") == bu + "res4.5.conv3.norm.bias"
    assert convert_torchvision_name("layer4.0.downsample.0.weight") == bu + "res5.0.shortcut.weight"
    assert convert_torchvision_name("layer2.0.downsample.1.running_mean") == bu + "res3.0.shortcut.norm.running_mean"
    assert convert_torchvision_name("fc.weight") == "" and convert_torchvision_name("layer1.0.bn1.num_batches_tracked") == ""
    assert convert_d2_backbone_name("stem.conv1.norm.running_var") == bu + "stem.conv1.norm.running_var"
    assert convert_d2_backbone_name("res2.0.shortcut.weight") == bu + "res2.0.shortcut.weight"
    assert convert_d2_backbone_name("stem.fc.weight") == "" and convert_d2_backbone_name("res3.1.conv1.norm.num_batches_tracked") == ""
    for bad in ("layer5.0.conv1.weight", "bn4.weight"):
        with pytest.raises(KeyError):
            convert_torchvision_name(bad)
    with pytest.raises(KeyError):
        convert_d2_backbone_name("res6.0.conv1.weight")


@pytest.mark.parametrize("fmt", ["pth", "pkl"])
def test_torchvision_checkpoint_lands_on_the_backbone(osr, tmp_path, caplog, fmt):
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into
    sd = torchvision_r50_state()
    path = tmp_path / f"r50.{fmt}"
    if fmt == "pth":
        torch.save(sd, path)
    else:
        with open(path, "wb") as f:
            pickle.dump(d2_converted(sd), f)
    state = load_checkpoint(str(path))
    assert state.origin == "torchvision"
    assert not any("fc" in k.split(".")[-2:][0] or k.endswith("num_batches_tracked") for k in state)
    model = _model(osr, False)
    with caplog.at_level(logging.WARNING):
        missing, unexpected = load_into(model, state, strict=False)
    assert not caplog.records, "no warning for a torchvision checkpoint in the torchvision layout"
    assert unexpected == []
    assert not any(k.startswith("backbone.bottom_up.") for k in missing)
    own = model.state_dict()
    bu = "backbone.bottom_up."
    assert torch.equal(own[bu + "stem.conv1.weight"], sd["conv1.weight"])
    assert torch.equal(own[bu + "stem.conv1.norm.running_mean"], sd["bn1.running_mean"])
    assert torch.equal(own[bu + "stem.conv1.norm.running_var"], sd["bn1.running_var"])  # real statistics, kept
    assert torch.equal(own[bu + "res3.0.conv2.weight"], sd["layer2.0.conv2.weight"])
    assert torch.equal(own[bu + "res5.2.conv3.norm.weight"], sd["layer4.2.bn3.weight"])
    assert torch.equal(own[bu + "res4.0.shortcut.weight"], sd["layer3.0.downsample.0.weight"])
    assert torch.equal(own[bu + "res4.0.shortcut.norm.running_var"], sd["layer3.0.downsample.1.running_var"])
    n_tv = sum(1 for k in sd if not k.startswith("fc.") and not k.endswith("num_batches_tracked"))
    assert len(state) == n_tv == sum(1 for k in own if k.startswith(bu))


def test_torchvision_checkpoint_into_msra_layout_warns(osr, tmp_path, caplog):
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into
    path = tmp_path / "r50.pth"
    torch.save(torchvision_r50_state(), path)
    model = _model(osr, True)
    with caplog.at_level(logging.WARNING):
        load_into(model, load_checkpoint(str(path)), strict=False)
    assert any("STRIDE_IN_1X1" in r.getMessage() for r in caplog.records)
    assert torch.equal(model.state_dict()["backbone.bottom_up.res2.0.conv1.weight"], torchvision_r50_state()["layer1.0.conv1.weight"])


def test_msra_and_d2_formats_are_unchanged(osr, tmp_path, caplog):
    from openset_rcnn_amd.host import checkpoint as CK
    model = _model(osr, True)
    own = {k: v for k, v in model.state_dict().items()}
    names = CK.msra_names_for(k for k in own if k.startswith("backbone.bottom_up."))
    g = np.random.default_rng(0)
    blobs = {names[k]: g.standard_normal(tuple(own[k].shape)).astype(np.float32) for k in names if not k.endswith(("running_mean", "running_var"))}
    p = tmp_path / "R-50.pkl"
    with open(p, "wb") as f:
        pickle.dump({"blobs": blobs}, f)
    st = CK.load_checkpoint(str(p))
    assert st.origin == "msra"
    assert dict(st).keys() == CK.convert_msra_state(blobs).keys()
    assert all(torch.equal(st[k], v) for k, v in CK.convert_msra_state(blobs).items())
    d2 = tmp_path / "model_final.pth"
    torch.save({"model": own, "iteration": 3}, d2)
    st2 = CK.load_checkpoint(str(d2))
    assert st2.origin == "d2" and st2.keys() == own.keys() and all(torch.equal(st2[k], own[k].float()) for k in own if own[k].is_floating_point())
    with caplog.at_level(logging.WARNING):
        CK.load_into(model, st, strict=False)
        CK.load_into(model, st2, strict=False)
    assert not caplog.records
