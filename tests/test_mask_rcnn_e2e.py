"""MODEL.MASK_ON end to end on the stock heads: base_rcnn_fpn.yaml with MASK_ON True, NUM_CLASSES 5 and a low SCORE_THRESH_TEST, two
images of different sizes (96 x 128 and 80 x 112), both CLS_AGNOSTIC_MASK values.

Parity mode (kernel_dtype float32): the pred_masks probabilities are within 1e-4 (the fp32 engine's contract) of the torch-CPU fp32
chain -- oracle.roi_pooler_ref at 14, the four mask_fcn convolutions, the deconvolution, the predictor, the sigmoid of the class row --
run on the engine's own pyramid and detections; the pasted bitmasks equal [d2] _do_paste_mask (F.grid_sample, float64) of the
reference probabilities except where the reference value lies within 1.1e-4 of the threshold (bilinear sampling is a convex
combination, so a pasted value moves by at most the 1e-4 the probabilities may move, plus the paste's own 1e-5 band).

fp16 mode: shapes and dtypes, masks empty outside their boxes, a captured replay (engine.capture) equal to the eager pass, and the mean
IoU of the thresholded 28 x 28 masks against the parity mode's on the same boxes (_mask_head called on its own).
Measured on the MI355X: 1.0000 (class-agnostic) and 0.9994 (per-class) over 16 detections; asserted at the measured value minus 0.01
(IOU_MEASURED / IOU_FLOOR below).

The mask predictor is scaled so that the reference logits have a standard deviation of 1 (asserted >= 0.5): [d2]'s std = 0.001
initialiser would put every probability at 0.5."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K = 5
TOPK = 8
SIZES = [(96, 128), (80, 112)]
OUT_SIZES = [(120, 160), (80, 112)]  # the first image is pasted at 1.25 x its size
PROB_TOL = 1e-4
# mean IoU of the fp16 engine's thresholded 28 x 28 masks against the parity engine's on the same 16 boxes, measured on the MI355X per
# CLS_AGNOSTIC_MASK value (the probabilities themselves differ by up to 1.5e-3, so only pixels that close to the threshold can flip).
# The floor is the measured value minus 0.01: room for a few more flipped pixels under another compiler's rounding of the five layers
IOU_MEASURED = {True: 1.0000, False: 0.9994}
IOU_FLOOR = {k: v - 0.01 for k, v in IOU_MEASURED.items()}


def _cfg(agnostic: bool):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.MASK_ON", "True", "MODEL.ROI_HEADS.NUM_CLASSES", str(K),
                         "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.01", "TEST.DETECTIONS_PER_IMAGE", str(TOPK),
                         "MODEL.RPN.POST_NMS_TOPK_TEST", "200", "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", str(agnostic)])
    return cfg


@functools.lru_cache(maxsize=None)
def _images():
    g = torch.Generator().manual_seed(11)
    return tuple(torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in SIZES)


def _inputs():
    return [{"image": im, "height": oh, "width": ow} for im, (oh, ow) in zip(_images(), OUT_SIZES)]


@functools.lru_cache(maxsize=None)
def _state(agnostic: bool):
    """Seeded parameters: random_standard_params for the detector, He-style mask_fcn / deconv, a unit-scale predictor (rescaled by
    _setup once the reference chain has told how large the hidden state is)."""
    from openset_rcnn_amd.host.weights import random_standard_params
    p = dict(random_standard_params(0, num_classes=K))
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


def _model(agnostic: bool, dtype, params):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg(agnostic))
    sd = model.state_dict()
    for k, v in params.items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    model.kernel_dtype = dtype
    return model.eval()


def _engine_pass(model):
    """-> (engine, padded batch, image_hw, (hp, wp), the five outputs, the pyramid NHWC)."""
    eng = model.engine()
    batch, sizes = model._stack_images(list(_images()))
    keep = {}
    res = eng.forward(batch, sizes, keep=keep)
    torch.cuda.synchronize()
    hw = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    return eng, batch, hw, (int(batch.shape[-2]), int(batch.shape[-1])), res, keep["feats"]


def _cpu_chain(feats, boxes_per_image, classes, p, agnostic, scale=1.0):
    """The torch-CPU fp32 mask branch on a pyramid (NCHW fp32 per level) and per-image boxes -> (probs (m, 28, 28), logits)."""
    pre = "roi_heads.mask_head."
    x = O.roi_pooler_ref(feats, boxes_per_image, out_size=14)
    for i in range(1, 5):
        x = F.relu(F.conv2d(x, p[f"{pre}mask_fcn{i}.weight"], p[f"{pre}mask_fcn{i}.bias"], padding=1))
    x = F.relu(F.conv_transpose2d(x, p[pre + "deconv.weight"], p[pre + "deconv.bias"], stride=2))
    z = F.conv2d(x, p[pre + "predictor.weight"] * scale, p[pre + "predictor.bias"])
    idx = torch.zeros(len(classes), dtype=torch.int64) if agnostic else classes
    z = z[torch.arange(len(classes)), idx]
    return torch.sigmoid(z), z


@functools.lru_cache(maxsize=None)
def _setup(agnostic: bool):
    """The parity model with a predictor scaled to unit logit spread, its engine pass, and the CPU reference on the engine's own
    pyramid and detections."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    p = dict(_state(agnostic))
    model = _model(agnostic, torch.float32, p)
    eng, batch, hw, hpwp, res, pyr = _engine_pass(model)
    counts = [int(c) for c in res[3].cpu()]
    assert all(c >= 1 for c in counts), f"precondition: at least one detection per image, got {counts}"
    feats = [pyr[k].detach().cpu().float().permute(0, 3, 1, 2).contiguous() for k in ("p2", "p3", "p4", "p5")]
    boxes = [res[0][i, :c].cpu() for i, c in enumerate(counts)]
    classes = torch.cat([res[2][i, :c].cpu() for i, c in enumerate(counts)])
    _, z = _cpu_chain(feats, boxes, classes, p, agnostic)
    scale = 1.0 / float(z.std())
    pre = "roi_heads.mask_head."
    p[pre + "predictor.weight"] = p[pre + "predictor.weight"] * scale
    ref, z = _cpu_chain(feats, boxes, classes, p, agnostic)
    assert float(z.std()) >= 0.5
    # the scaled predictor goes into the model (load_state_dict drops the packed engine); detections do not depend on the mask head
    sd = model.state_dict()
    sd[pre + "predictor.weight"] = p[pre + "predictor.weight"]
    model.load_state_dict(sd)
    eng, batch, hw, hpwp, res2, pyr = _engine_pass(model)
    assert all(torch.equal(a, b) for a, b in zip(res[:4], res2[:4]))
    return dict(params=p, model=model, eng=eng, batch=batch, hw=hw, hpwp=hpwp, res=res2, counts=counts, boxes=boxes, classes=classes, ref=ref, z=z)


def _paste_reference(probs, boxes, h, w):
    """[d2] _do_paste_mask(skip_empty=False) in float64 -> sampled values (m, h, w)."""
    m, b = probs.double(), boxes.double()
    iy = ((torch.arange(0, h, dtype=torch.float64) + 0.5) - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * 2 - 1
    ix = ((torch.arange(0, w, dtype=torch.float64) + 0.5) - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * 2 - 1
    grid = torch.stack([ix[:, None, :].expand(len(b), h, w), iy[:, :, None].expand(len(b), h, w)], dim=3)
    return F.grid_sample(m[:, None], grid, align_corners=False)[:, 0]


@pytest.mark.parametrize("agnostic", [True, False], ids=["agnostic", "per-class"])
def test_parity_mode_against_the_cpu_chain(osr, agnostic):
    s = _setup(agnostic)
    res, counts = s["res"], s["counts"]
    assert len(res) == 5 and res[4].shape == (2, TOPK, 28, 28) and res[4].dtype == torch.float32
    got = torch.cat([res[4][i, :c].cpu() for i, c in enumerate(counts)])
    err = float((got - s["ref"]).abs().max())
    print(f"agnostic={agnostic}: {sum(counts)} detections {counts}, logit std {float(s['z'].std()):.3f}, max |probs - cpu| {err:.3e}")
    assert err <= PROB_TOL
    for i, c in enumerate(counts):  # rows beyond an image's detections are zeros
        assert float(res[4][i, c:].abs().max()) == 0.0 if c < TOPK else True
    if not agnostic:
        assert len(set(s["classes"].tolist())) > 1, "more than one class among the detections"
    # ---- model(batch): Instances with pasted bitmasks at the output resolution ----
    out = s["model"](_inputs())
    off = 0
    for i, (o, (oh, ow), (h, w)) in enumerate(zip(out, OUT_SIZES, SIZES)):
        inst = o["instances"]
        assert inst.image_size == (oh, ow)
        # the reference postprocess: scale, clip, drop empties
        b = s["boxes"][i] * torch.tensor([ow / w, oh / h, ow / w, oh / h])
        b = torch.stack((b[:, 0].clamp(0, ow), b[:, 1].clamp(0, oh), b[:, 2].clamp(0, ow), b[:, 3].clamp(0, oh)), dim=1)
        keep = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        b = b[keep]
        assert len(inst) == len(b) and torch.allclose(inst.pred_boxes.tensor.cpu(), b)
        masks = inst.pred_masks
        assert masks.shape == (len(b), oh, ow) and masks.dtype == torch.bool
        val = _paste_reference(s["ref"][off:off + counts[i]][keep], b, oh, ow)
        band = (val - 0.5).abs() < PROB_TOL + 1e-5
        diff = (masks.cpu() != (val >= 0.5)) & ~band
        print(f"image {i}: {int(masks.sum())} mask pixels, {int(band.sum())} in the band, {int(diff.sum())} differ")
        assert int(band.sum()) < 0.01 * max(int((val > 0).sum()), 1), "too many reference values at the threshold"
        assert int(diff.sum()) == 0
        off += counts[i]
    # ---- StandardROIHeads.forward (eval) attaches the probabilities as mask_rcnn_inference does ----
    from openset_rcnn_amd.host.structures import Boxes, ImageList, Instances
    model = s["model"]
    pyr = model.engine()._backbone(s["batch"], *s["hpwp"])
    feats = {k: pyr[k].permute(0, 3, 1, 2) for k in ("p2", "p3", "p4", "p5")}
    props = [Instances(sz, proposal_boxes=Boxes(s["boxes"][i].to(DEV)), objectness_logits=torch.zeros(counts[i], device=DEV))
             for i, sz in enumerate(SIZES)]
    insts, _ = model.roi_heads(ImageList(s["batch"], SIZES), feats, props)
    assert sum(len(inst) for inst in insts) > 0
    for inst in insts:
        assert inst.pred_masks.shape == (len(inst), 1, 28, 28) and inst.pred_masks.dtype == torch.float32
        if len(inst):
            assert float(inst.pred_masks.min()) >= 0.0 and float(inst.pred_masks.max()) <= 1.0


@functools.lru_cache(maxsize=None)
def _fp16(agnostic: bool):
    model = _model(agnostic, torch.float16, _setup(agnostic)["params"])
    return (model,) + _engine_pass(model)


@pytest.mark.parametrize("agnostic", [True, False], ids=["agnostic", "per-class"])
def test_fp16_mode(osr, agnostic):
    s = _setup(agnostic)
    model, eng, batch, hw, (hp, wp), res, pyr = _fp16(agnostic)
    assert len(res) == 5 and res[4].shape == (2, TOPK, 28, 28) and res[4].dtype == torch.float32
    assert res[0].shape == (2, TOPK, 4) and res[2].dtype == torch.int64 and res[3].dtype == torch.int32
    counts = [int(c) for c in res[3].cpu()]
    assert all(c >= 1 for c in counts)
    # masks are empty outside their boxes
    for o, (oh, ow) in zip(model(_inputs()), OUT_SIZES):
        inst = o["instances"]
        masks, b = inst.pred_masks.cpu(), inst.pred_boxes.tensor.cpu()
        assert masks.shape == (len(inst), oh, ow) and masks.dtype == torch.bool and int(masks.sum()) > 0
        ys = (torch.arange(oh) + 0.5)[None, :, None]
        xs = (torch.arange(ow) + 0.5)[None, None, :]
        bb = b[:, :, None, None]
        outside = (xs < bb[:, 0]) | (xs > bb[:, 2]) | (ys < bb[:, 1]) | (ys > bb[:, 3])
        assert int(masks[outside].sum()) == 0
    # the mask head on its own, on the parity mode's boxes: IoU of the thresholded masks
    pres = s["res"]
    probs = eng._mask_head(pyr, pres[0], pres[2], pres[3])
    torch.cuda.synchronize()
    a = torch.cat([probs[i, :c].cpu() for i, c in enumerate(s["counts"])]) >= 0.5
    b = torch.cat([pres[4][i, :c].cpu() for i, c in enumerate(s["counts"])]) >= 0.5
    inter, union = (a & b).flatten(1).sum(1).float(), (a | b).flatten(1).sum(1).float()
    iou = float((inter / union.clamp(min=1)).mean())
    dp = float((torch.cat([probs[i, :c].cpu() for i, c in enumerate(s["counts"])]) - s["ref"]).abs().max())
    print(f"agnostic={agnostic}: fp16 vs parity mean mask IoU {iou:.4f} over {len(a)} detections, max |dprob| {dp:.3e}")
    assert iou >= IOU_FLOOR[agnostic]


def test_captured_replay_equals_the_eager_pass(osr):
    model, eng, batch, hw, (hp, wp), res, _ = _fp16(False)
    eager = [t.clone() for t in eng.forward_device(batch, hw, hp, wp)]
    graph, out = eng.capture(batch, hw, hp, wp)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 5
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(eager, res))
