"""TEST.AUG without a GPU: the config node, the augmentation list, the wrapper's and the new ops' refusals, the argument validation
of the four new entry points, and run_net.do_test's second pass."""
import ctypes
import importlib.util
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(osr, yaml="base_rcnn_fpn.yaml", *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


# ---- config ---------------------------------------------------------------------------------------------------------------------
def test_defaults(osr):
    from openset_rcnn_amd.host.config import get_cfg
    cfg = get_cfg()
    aug = cfg.TEST.AUG
    assert aug.ENABLED is False
    assert tuple(aug.MIN_SIZES) == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
    assert aug.MAX_SIZE == 4000
    assert aug.FLIP is True
    assert cfg.TEST.DETECTIONS_PER_IMAGE == 100 and cfg.TEST.EVAL_PERIOD == 0


def test_yaml_merges(osr, tmp_path):
    from openset_rcnn_amd.host.config import get_cfg
    path = tmp_path / "tta.yaml"
    path.write_text("TEST:\n  AUG:\n    ENABLED: True\n    MIN_SIZES: (64, 96)\n")
    cfg = get_cfg()
    cfg.merge_from_file(str(path))
    assert cfg.TEST.AUG.ENABLED is True and tuple(cfg.TEST.AUG.MIN_SIZES) == (64, 96)
    assert cfg.TEST.AUG.MAX_SIZE == 4000 and cfg.TEST.AUG.FLIP is True
    assert cfg.TEST.DETECTIONS_PER_IMAGE == 100
    cfg.merge_from_list(["TEST.AUG.FLIP", "False", "TEST.AUG.MAX_SIZE", "160"])
    assert cfg.TEST.AUG.FLIP is False and cfg.TEST.AUG.MAX_SIZE == 160


# ---- the augmentation list ----------------------------------------------------------------------------------------------------------
def test_augmentation_list(osr):
    from openset_rcnn_amd.host.tta import tta_augmentations
    got = tta_augmentations(96, 128, 120, 160, (64, 96, 128), 160, True)
    # the last pair: 128 -> 128 x 170.67, clamped by MAX_SIZE 160 to 120 x 160
    assert got == [(64, 85, False), (64, 85, True), (96, 128, False), (96, 128, True), (120, 160, False), (120, 160, True)]
    assert tta_augmentations(96, 128, 120, 160, (64, 96, 128), 160, False) == [(64, 85, False), (96, 128, False), (120, 160, False)]
    # portrait: h and w swap roles
    assert tta_augmentations(128, 96, 160, 120, (64, 96, 128), 160, True) == \
        [(85, 64, False), (85, 64, True), (128, 96, False), (128, 96, True), (160, 120, False), (160, 120, True)]
    # (ho, wo) does not enter the sizes: the resize acts on the model input image
    assert tta_augmentations(96, 128, 96, 128, (64,), 160, False) == tta_augmentations(96, 128, 480, 640, (64,), 160, False)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def std_model(osr):
    from openset_rcnn_amd.host import modeling as M
    return M.build_model(_cfg(osr)).eval()


def test_wrapper_accepts_the_stock_model(osr, std_model):
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    w = GeneralizedRCNNWithTTA(_cfg(osr, "base_rcnn_fpn.yaml", "TEST.AUG.MIN_SIZES", "(64, 96)", "TEST.AUG.FLIP", "False"), std_model)
    assert w.min_sizes == (64, 96) and w.flip is False and w.max_size == 4000


def test_wrapper_refuses_the_openset_heads(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    cfg = _cfg(osr, "voc_coco.yaml")
    model = M.build_model(cfg).eval()
    with pytest.raises(ValueError, match="StandardROIHeads"):
        GeneralizedRCNNWithTTA(cfg, model)


@pytest.mark.parametrize("key, word", [("MODEL.KEYPOINT_ON", "KEYPOINT_ON"), ("MODEL.LOAD_PROPOSALS", "LOAD_PROPOSALS")])
def test_wrapper_refuses_keypoints_and_loaded_proposals(osr, std_model, key, word):
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    with pytest.raises(ValueError, match=word):
        GeneralizedRCNNWithTTA(_cfg(osr, "base_rcnn_fpn.yaml", key, "True"), std_model)


def test_wrapper_refuses_training_mode(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    cfg = _cfg(osr)
    model = M.build_model(cfg)
    model.train()
    with pytest.raises(ValueError, match="training mode"):
        GeneralizedRCNNWithTTA(cfg, model)


def test_float_image_is_refused(osr, std_model):
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    w = GeneralizedRCNNWithTTA(_cfg(osr), std_model)
    with pytest.raises(ValueError, match="uint8"):
        w([{"image": torch.zeros(3, 32, 32, dtype=torch.float32)}])


def test_new_ops_refuse_cpu_tensors(osr):
    ops, OsrError = osr.ops, osr.OsrError
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)  # noqa: E731
    with pytest.raises(OsrError):
        ops.resize_bilinear_u8_planar(torch.zeros(3, 4, 4, dtype=torch.uint8), i32(4, 2), i32(4, 3), 3, i32(4, 2), i32(4, 3), 3, 0, 4, 4, 4)
    with pytest.raises(OsrError):
        ops.tta_boxes_to_original(f32(1, 2, 4), f32(1, 2), torch.zeros(1, 2, dtype=torch.int64), i32(1), i32(1, 4), 8, 8, False, 0,
                                  f32(1, 2, 4), f32(1, 2), i32(1, 2), i32(1, 2))
    with pytest.raises(OsrError):
        ops.tta_boxes_to_augmented(f32(1, 2, 4), i32(1), i32(1, 4), 8, 8, True)
    with pytest.raises(OsrError):
        ops.tta_reduce_masks(f32(1, 1, 2, 4, 4), i32(1), i32(1))


def test_model_inference_takes_detected_instances(osr, std_model):
    import inspect
    from openset_rcnn_amd.host import modeling as M
    sig = inspect.signature(M.GeneralizedRCNN.inference)
    assert list(sig.parameters)[1:] == ["batched_inputs", "detected_instances", "do_postprocess"]
    assert sig.parameters["detected_instances"].default is None and sig.parameters["do_postprocess"].default is True
    assert hasattr(M.StandardROIHeads, "forward_with_given_boxes")


# ---- argument validation of the four entry points (no GPU: nothing is launched) ---------------------------------------------------------
def test_argument_validation_needs_no_gpu(osr):
    lib = osr._lib.load()
    buf = (ctypes.c_uint8 * 4096)()  # host memory standing in for every non-null pointer: validation fails before any launch
    b = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.osr_last_error()  # noqa: E731

    # resize: null pointers, mirror not 0 / 1, rows outside the image, a short tmp
    assert lib.osr_resize_bilinear_u8_planar(None, 3, 4, 4, b, b, 3, b, b, 3, 0, 4, 4, 4, 0, b, 4096, b, None) == -1 and b"null pointer" in err()
    assert lib.osr_resize_bilinear_u8_planar(b, 3, 4, 4, b, b, 3, b, b, 3, 0, 4, 4, 4, 0, b, 4096, None, None) == -1 and b"null pointer" in err()
    assert lib.osr_resize_bilinear_u8_planar(b, 3, 4, 4, b, b, 3, b, b, 3, 0, 4, 4, 4, 2, b, 4096, b, None) == -1 and b"mirror" in err()
    assert lib.osr_resize_bilinear_u8_planar(b, 3, 4, 4, b, b, 3, b, b, 3, 0, 4, 4, 4, -1, b, 4096, b, None) == -1 and b"mirror" in err()
    assert lib.osr_resize_bilinear_u8_planar(b, 3, 4, 4, b, b, 3, b, b, 3, 2, 3, 4, 4, 0, b, 4096, b, None) == -1 and b"inside the image" in err()
    assert lib.osr_resize_bilinear_u8_planar(b, 3, 4, 4, b, b, 3, b, b, 3, 0, 4, 4, 4, 0, b, 47, b, None) == -1 and b"tmp" in err()
    assert lib.osr_resize_bilinear_u8_planar(b, 0, 4, 4, b, b, 3, b, b, 3, 0, 4, 4, 4, 0, b, 4096, b, None) == -1 and b"geometry" in err()

    # boxes -> original space
    ok = dict(n=1, topk=2, ha=8, wa=8, flip=0, slot=0, cap=2)

    def to_orig(boxes=b, c_cand=b, **kw):
        a = {**ok, **kw}
        return lib.osr_tta_boxes_to_original(boxes, b, b, b, b, a["n"], a["topk"], a["ha"], a["wa"], a["flip"], a["slot"], a["cap"], b, b, b, c_cand, None)
    assert to_orig(boxes=None) == -1 and b"null pointer" in err()
    assert to_orig(c_cand=None) == -1 and b"null pointer" in err()
    assert to_orig(flip=2) == -1 and b"flip" in err()
    assert to_orig(n=0) == -1 and b"geometry" in err()
    assert to_orig(wa=0) == -1 and b"geometry" in err()
    assert to_orig(slot=1) == -1 and b"slot" in err()  # rows [1, 3) do not fit a list of 2
    assert to_orig(slot=-1) == -1 and b"slot" in err()

    # boxes -> augmented space
    assert lib.osr_tta_boxes_to_augmented(None, b, b, 1, 2, 8, 8, 0, b, None) == -1 and b"null pointer" in err()
    assert lib.osr_tta_boxes_to_augmented(b, b, b, 1, 2, 8, 8, 0, None, None) == -1 and b"null pointer" in err()
    assert lib.osr_tta_boxes_to_augmented(b, b, b, 1, 2, 8, 8, 3, b, None) == -1 and b"flip" in err()
    assert lib.osr_tta_boxes_to_augmented(b, b, b, 1, 0, 8, 8, 0, b, None) == -1 and b"geometry" in err()

    # mask mean: A < 1
    assert lib.osr_tta_reduce_masks(None, b, 1, b, 1, 2, 4, b, None) == -1 and b"null pointer" in err()
    assert lib.osr_tta_reduce_masks(b, None, 1, b, 1, 2, 4, b, None) == -1 and b"null pointer" in err()
    assert lib.osr_tta_reduce_masks(b, b, 0, b, 1, 2, 4, b, None) == -1 and b"A >= 1" in err()
    assert lib.osr_tta_reduce_masks(b, b, -3, b, 1, 2, 4, b, None) == -1 and b"A >= 1" in err()
    assert lib.osr_tta_reduce_masks(b, b, 1, b, 1, 2, 0, b, None) == -1 and b"geometry" in err()


# ---- run_net.do_test -----------------------------------------------------------------------------------------------------------------
def _run_net():
    spec = importlib.util.spec_from_file_location("run_net_for_tta_test", os.path.join(ROOT, "run_net.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Evaluator:
    def __init__(self, log, folder):
        self.log, self.folder = log, folder

    def reset(self):
        pass

    def process(self, inputs, outputs):
        raise AssertionError("the stub dataset is empty")

    def evaluate(self):
        self.log.append(self.folder)
        return {"AP": float(len(self.log))}


def _stub_catalog(log):
    return types.SimpleNamespace(get_evaluator=lambda cfg, name, folder: _Evaluator(log, folder), DatasetCatalog={"setA": lambda: [], "setB": lambda: []})


@pytest.mark.parametrize("enabled", [False, True])
def test_do_test_runs_a_second_pass_when_enabled(osr, std_model, tmp_path, enabled):
    rn = _run_net()
    cfg = _cfg(osr, "base_rcnn_fpn.yaml", "TEST.AUG.ENABLED", str(enabled), "OUTPUT_DIR", str(tmp_path), "DATASETS.TEST", "('setA', 'setB')")
    log = []
    args = types.SimpleNamespace(resume_test=False, test_batch=1)
    res = rn.do_test(cfg, args, std_model, _stub_catalog(log))
    if not enabled:
        assert list(res) == ["setA", "setB"] and len(log) == 2
        assert all(os.sep + "inference" + os.sep in f for f in log)
    else:
        assert list(res) == ["setA", "setB", "setA_TTA", "setB_TTA"] and len(log) == 4
        assert [os.path.relpath(f, str(tmp_path)) for f in log] == [
            os.path.join("inference", "setA", "Final"), os.path.join("inference", "setB", "Final"),
            os.path.join("inference_TTA", "setA", "Final"), os.path.join("inference_TTA", "setB", "Final")]
        assert res["setA_TTA"] == {"AP": 3.0}


def test_do_test_stops_on_the_openset_heads(osr, tmp_path):
    from openset_rcnn_amd.host import modeling as M
    rn = _run_net()
    cfg = _cfg(osr, "voc_coco.yaml", "TEST.AUG.ENABLED", "True", "OUTPUT_DIR", str(tmp_path), "DATASETS.TEST", "('setA',)")
    model = M.build_model(cfg).eval()
    with pytest.raises(ValueError, match="StandardROIHeads"):
        rn.do_test(cfg, types.SimpleNamespace(resume_test=False, test_batch=1), model, _stub_catalog([]))
