"""Training the stock Faster R-CNN of Base-RCNN-FPN.yaml (BASELINE config 1) through the module surface: build_model in train mode on
the two-image COCO toy of test_standard_rcnn.py, model(batch) -> the four [d2] losses, sum().backward() + the solver step, the seven
EventStorage scalars, eval-mode detections with the trained weights, and a run_net.py run that trains and checkpoints."""
import os
import sys

import pytest
import torch

from tests.test_run_net import toy_voc_root  # noqa: F401  (fixture)
from tests.test_standard_rcnn import _cfg, coco_toy  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SCALARS = {"rpn/num_pos_anchors", "rpn/num_neg_anchors", "roi_head/num_fg_samples", "roi_head/num_bg_samples", "fast_rcnn/cls_accuracy",
           "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative"}


@pytest.mark.gpu
def test_model_trains_on_two_synthetic_coco_images(osr, coco_toy):  # noqa: F811
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host import solver
    from openset_rcnn_amd.host.data import DatasetMapper, build_detection_test_loader
    cfg = _cfg(osr, DEV)
    cfg.merge_from_list(["INPUT.MIN_SIZE_TEST", "480", "INPUT.MAX_SIZE_TEST", "640", "SOLVER.BASE_LR", "0.001", "SOLVER.WARMUP_ITERS", "0"])
    dicts = D.load_coco_json(os.path.join(coco_toy, "instances.json"), os.path.join(coco_toy, "images"))
    batch = next(iter(build_detection_test_loader(dicts, DatasetMapper(cfg, is_train=True), batch_size=2, rank=0, world=1)))
    model = M.build_model(cfg)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    opt = solver.build_optimizer(cfg, model)
    losses = model(batch)
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg"}
    total = sum(losses.values())
    assert torch.isfinite(total)
    total.backward()
    opt.step()
    assert set(model.event_scalars()) == SCALARS
    assert model.event_scalars()["roi_head/num_fg_samples"] > 0
    model.eval()
    after = model.state_dict()
    changed = [k for k in after if after[k].is_floating_point() and not torch.equal(after[k].cpu(), before[k].cpu())]
    assert any(k.startswith("proposal_generator.rpn_head.objectness_logits") for k in changed)
    assert any(k.startswith("roi_heads.box_predictor.cls_score") for k in changed)
    assert any(k.startswith("backbone.fpn_output2") for k in changed)
    out = model([{"image": b["image"], "height": 480, "width": 640} for b in batch])
    assert len(out) == 2 and all(len(o["instances"]) <= 100 for o in out)


@pytest.mark.gpu
def test_module_training_branches_return_losses(osr, coco_toy):  # noqa: F811
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.data import DatasetMapper, build_detection_test_loader
    cfg = _cfg(osr, DEV)
    dicts = D.load_coco_json(os.path.join(coco_toy, "instances.json"), os.path.join(coco_toy, "images"))
    batch = next(iter(build_detection_test_loader(dicts, DatasetMapper(cfg, is_train=True), batch_size=2, rank=0, world=1)))
    model = M.build_model(cfg)
    model.train()
    with torch.no_grad():
        images = model.preprocess_image(batch)
        feats = model.backbone(images.tensor)
        gts = [b["instances"].to(DEV) if hasattr(b["instances"], "to") else b["instances"] for b in batch]
        props, rl = model.proposal_generator(images, feats, gts)
        assert set(rl) == {"loss_rpn_cls", "loss_rpn_loc"} and all(torch.isfinite(v) for v in rl.values())
        assert all(0 < len(p) <= 1000 for p in props)
        smp, hl = model.roi_heads(images, feats, props, gts)
    assert set(hl) == {"loss_cls", "loss_box_reg"} and all(torch.isfinite(v) for v in hl.values())
    assert all(0 < len(p) <= 512 and hasattr(p, "gt_classes") for p in smp)


@pytest.mark.gpu
def test_run_net_trains_and_checkpoints_the_stock_config(osr, toy_voc_root, tmp_path, monkeypatch):  # noqa: F811
    sys.path.insert(0, ROOT)
    import run_net
    from openset_rcnn_amd.host import modeling as M
    monkeypatch.setenv("DETECTRON2_DATASETS", toy_voc_root)
    out = str(tmp_path / "out")
    args = ["--config-file", os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"), "OUTPUT_DIR", out, "SEED", "5",
            "DATASETS.TRAIN", "('voc_2007_train',)", "DATASETS.TEST", "()", "SOLVER.IMS_PER_BATCH", "2", "SOLVER.BASE_LR", "0.0001",
            "SOLVER.WARMUP_ITERS", "0", "SOLVER.CHECKPOINT_PERIOD", "0", "SOLVER.MAX_ITER", "3", "INPUT.MIN_SIZE_TRAIN", "(96,)",
            "INPUT.MAX_SIZE_TRAIN", "128"]
    assert run_net.main(args) == 0
    blob = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    assert blob["iteration"] == 2 and all(torch.isfinite(v).all() for v in blob["model"].values() if v.is_floating_point())
    cfg = _cfg(osr, DEV)
    model = M.build_model(cfg)
    model.load_state_dict({k: v for k, v in blob["model"].items()}, strict=False)
    sd = model.state_dict()
    assert torch.equal(sd["proposal_generator.rpn_head.objectness_logits.weight"].cpu(), blob["model"]["proposal_generator.rpn_head.objectness_logits.weight"])
