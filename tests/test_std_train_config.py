"""CPU: the yaml keys of the stock heads' training step reach the engine configuration, and stock options the HIP path does not
train are refused when the model is built (not at the first iteration)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def test_engine_cfg_maps_the_stock_training_keys(osr):
    from openset_rcnn_amd.host.modeling import engine_cfg_from
    c = engine_cfg_from(_cfg("MODEL.RPN.LOSS_WEIGHT", "2.0", "MODEL.RPN.BBOX_REG_LOSS_WEIGHT", "0.5", "MODEL.RPN.SMOOTH_L1_BETA", "0.25",
                             "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", "0.5", "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT", "3.0"))
    assert c["pre_nms_topk_train"] == 2000 and c["post_nms_topk_train"] == 1000
    assert c["rpn_iou_thresholds"] == (0.3, 0.7) and c["rpn_batch_size"] == 256 and c["rpn_positive_fraction"] == 0.5
    assert c["rpn_cls_weight"] == 2.0 and c["rpn_loc_weight"] == 1.0 and c["rpn_bbox_reg_weights"] == (1.0, 1.0, 1.0, 1.0)
    assert c["roi_batch_size"] == 512 and c["roi_positive_fraction"] == 0.25 and c["roi_iou_threshold"] == 0.5
    assert c["std_num_classes"] == 80 and c["cls_agnostic_bbox_reg"] is True and c["box_reg_weight"] == 3.0
    assert c["loss_types"]["rpn_box"] == ("smooth_l1", 0.25) and c["loss_types"]["roi_box"] == ("smooth_l1", 0.5)


@pytest.mark.parametrize("key", ["MODEL.RPN.BBOX_REG_LOSS_TYPE", "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE"])
def test_unsupported_stock_loss_types_are_refused_at_build_time(osr, key):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(NotImplementedError, match=key):
        M.build_model(_cfg(key, "giou"))
    M.build_model(_cfg(key, "smooth_l1"))  # the default builds
