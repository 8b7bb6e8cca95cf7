"""Shared by the TEST.AUG tests: the numpy fp32 restatement of [d2]'s box transform lists, and the small stock model of
tests/test_mask_rcnn_e2e.py (random_standard_params(0, num_classes=5), SCORE_THRESH_TEST 0.01, 8 detections per image, a mask
predictor scaled so that the probabilities spread over (0, 1)).

An augmentation of an input with image (hi, wi) and output resolution (ho, wo) is the list [resize (ho, wo) -> (hi, wi), only when
they differ], resize (hi, wi) -> (ha, wa), [hflip(wa)]. A resize multiplies x by f32(w'/w) and y by f32(h'/h) (ratio in double,
rounded once), a flip is f32(wa) - x; after each step the box is (min x, min y, max x, max y) of its corners; the inverse runs the
inverted steps in reverse order."""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEV = "cuda:0"
K = 5
TOPK = 8


# ---- box maps -------------------------------------------------------------------------------------------------------------------
def _ratio(num, den):
    return F(float(num) / float(den))


def _resize(b, h, w, h2, w2):
    out = b.copy()
    out[[0, 2]] = b[[0, 2]] * _ratio(w2, w)
    out[[1, 3]] = b[[1, 3]] * _ratio(h2, h)
    return out


def _flip(b, wa):
    x0, x1 = F(wa) - b[0], F(wa) - b[2]
    with np.errstate(invalid="ignore"):
        return np.array([np.minimum(x0, x1), b[1], np.maximum(x0, x1), b[3]], dtype=F)


def steps(size, ha, wa, flip):
    """size = (hi, wi, ho, wo) -> the transform list."""
    hi, wi, ho, wo = (int(v) for v in size)
    out = []
    if (ho, wo) != (hi, wi):
        out.append(("resize", ho, wo, hi, wi))
    out.append(("resize", hi, wi, ha, wa))
    if flip:
        out.append(("flip", wa))
    return out


def forward_box(b, size, ha, wa, flip):
    b = np.asarray(b, dtype=F)
    for s in steps(size, ha, wa, flip):
        b = _resize(b, *s[1:]) if s[0] == "resize" else _flip(b, s[1])
    return b


def inverse_box(b, size, ha, wa, flip):
    b = np.asarray(b, dtype=F)
    for s in reversed(steps(size, ha, wa, flip)):
        b = _resize(b, s[3], s[4], s[1], s[2]) if s[0] == "resize" else _flip(b, s[1])
    return b


# ---- the model --------------------------------------------------------------------------------------------------------------------
def cfg_for(mask_on: bool, agnostic: bool = False, *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.MASK_ON", str(mask_on), "MODEL.ROI_HEADS.NUM_CLASSES", str(K),
                         "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.01", "TEST.DETECTIONS_PER_IMAGE", str(TOPK),
                         "MODEL.RPN.POST_NMS_TOPK_TEST", "200", "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", str(agnostic),
                         "TEST.AUG.MIN_SIZES", "(64, 96, 128)", "TEST.AUG.MAX_SIZE", "160", "TEST.AUG.FLIP", "True"] + list(opts))
    return cfg


@functools.lru_cache(maxsize=None)
def params(mask_on: bool, agnostic: bool, seed: int = 0):
    """random_standard_params(seed, 5) + (mask_on) He-style mask_fcn / deconv and a unit-scale predictor."""
    from openset_rcnn_amd.host.weights import random_standard_params
    p = dict(random_standard_params(seed, num_classes=K))
    if not mask_on:
        return p
    g = torch.Generator().manual_seed(4000)
    pre = "roi_heads.mask_head."
    for i in range(1, 5):
        p[f"{pre}mask_fcn{i}.weight"] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        p[f"{pre}mask_fcn{i}.bias"] = torch.randn(256, generator=g) * 0.02
    p[pre + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (2.0 / 256) ** 0.5
    p[pre + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
    rows = 1 if agnostic else K
    p[pre + "predictor.weight"] = torch.randn(rows, 256, 1, 1, generator=g)
    p[pre + "predictor.bias"] = torch.randn(rows, generator=g) * 0.1
    return p


def _load(model, p):
    sd = model.state_dict()
    for k, v in p.items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)


def build(mask_on: bool, agnostic: bool, dtype, seed: int = 0):
    """-> (cfg, model in eval mode). With a mask head the predictor is rescaled so that the logits of the model's own detections on
    `images()` have unit spread ([d2]'s std = 0.001 initialiser would put every probability at 0.5, the unit-scale one saturates
    them); asserted: at least a fifth of the probabilities lie in (0.05, 0.95)."""
    from openset_rcnn_amd.host import modeling as M
    cfg = cfg_for(mask_on, agnostic)
    model = M.build_model(cfg)
    p = dict(params(mask_on, agnostic, seed))
    _load(model, p)
    model.kernel_dtype = dtype
    model.eval()
    if mask_on:
        pre = "roi_heads.mask_head.predictor."
        probs = torch.cat([o["instances"].pred_masks.flatten() for o in model.inference(inputs(), do_postprocess=False)]).double().cpu()
        assert probs.numel() > 0, "precondition: the plain pass detects something"
        z = torch.logit(probs.clamp(1e-9, 1 - 1e-9))
        p[pre + "weight"] = p[pre + "weight"] / float(z.std())
        p[pre + "bias"] = p[pre + "bias"] * 0.0
        _load(model, p)
        model.eval()
        probs = torch.cat([o["instances"].pred_masks.flatten() for o in model.inference(inputs(), do_postprocess=False)]).cpu()
        spread = float(((probs > 0.05) & (probs < 0.95)).float().mean())
        assert spread >= 0.2, f"precondition: mask probabilities spread over (0, 1), got {spread:.2f} inside (0.05, 0.95)"
    return cfg, model


IMAGE_SIZES = [(96, 128), (96, 128), (80, 112)]
OUT_SIZES = [(120, 160), (96, 128), (80, 112)]  # one group of two with two pre-transforms, one group of one


@functools.lru_cache(maxsize=None)
def images(seed: int = 11):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in IMAGE_SIZES)


def inputs(seed: int = 11):
    return [{"image": im, "height": oh, "width": ow} for im, (oh, ow) in zip(images(seed), OUT_SIZES)]
