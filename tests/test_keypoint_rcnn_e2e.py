"""MODEL.KEYPOINT_ON end to end on the stock heads: configs/keypoint_rcnn_fpn.yaml as it stands (eight 512-channel conv_fcn layers, 17
keypoints), four 256 x 384 images, four detections per image at most, nine fixed boxes for the comparisons.

The reference (tests/keypoint_common.py + oracle.roi_pooler_ref at 14 x 14) runs on the engine's own pyramid and on the stored
parameters: RoIAlign (the oracle's, fp32), then in float64 the conv_fcn layers, score_lowres, bilinear x2 and [d2]
heatmaps_to_keypoints (0.3 s per layer on eight cores). score_lowres is scaled so that the reference heatmaps have unit spread
(asserted >= 0.5).

Parity mode (kernel_dtype float32), through forward_with_given_boxes on the fixed boxes: pred_keypoint_heatmaps within 1e-4 of the
chain (the fp32 engine's contract, the bound of tests/test_mask_rcnn_e2e.py's parity mode); pred_keypoints equal to the reference
decode of the reference heatmaps wherever the reference's gap between its two largest resized values exceeds 1e-3 -- x and y within
1e-4 px (the fp32 rounding of the affine map at coordinates below 512) and the score within 1e-3 relative; the share of
(RoI, keypoint) pairs below that gap is asserted <= 5 %.
The score bound: score = 1 / sum exp(map - U[p]). The engine's heatmaps may differ from the reference's by 1e-4 per value; a
bicubic sample is a combination of 16 of them whose weights' absolute sum is at most 1.89 (1.375 per axis, at t = 0.5), so every
exponent moves by at most (1 + 1.89) * 1e-4 = 2.9e-4 and the score by that relative amount, plus fp32's own part
(tests/test_heatmaps_to_keypoints.py: 2e-5); 1e-3 leaves a factor 3.
fp16 mode: the heatmaps within 4 * e16 of the float64 chain on the fp16 engine's pyramid and fp16-rounded weights, e16 = the error
of that chain with the output of RoIAlign and of every conv_fcn layer rounded to fp16 (measured here, printed); pred_keypoints
equal to the float64 decode of the engine's own heatmaps under the same rule (only fp32 arithmetic separates the two there)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O
from tests.keypoint_common import decode_chain, upsample_chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K, TOPK, N, SIZE = 17, 4, 4, (256, 384)
DIMS = (512,) * 8  # the yaml's own MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS
PRE = "roi_heads.keypoint_head."
HEAT_TOL = 1e-4
GAP, XY_TOL, SCORE_RTOL = 1e-3, 1e-4, 1e-3
# fixed boxes (x0, y0, w, h), binary fractions so that the sides are exact in fp32: person-like, wide, small, below the 1 x 1 clamp
FIXED = [[(16.5, 20.25, 60.0, 120.0), (100.0, 30.5, 33.5, 47.25), (150.25, 8.0, 200.75, 150.0)],
         [(5.0, 5.0, 17.0, 9.5), (200.5, 100.25, 0.5, 0.25), (40.0, 60.0, 120.0, 180.0)],
         [(300.0, 10.0, 80.0, 240.0)],
         [(0.0, 0.0, 384.0, 256.0), (64.25, 32.5, 56.0, 56.0)]]


def _cfg(*extra):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "keypoint_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.01",
                         "TEST.DETECTIONS_PER_IMAGE", str(TOPK), "MODEL.RPN.POST_NMS_TOPK_TEST", "200"] + list(extra))
    return cfg


@functools.lru_cache(maxsize=None)
def _images():
    g = torch.Generator().manual_seed(21)
    return tuple(torch.randint(0, 256, (3,) + SIZE, generator=g, dtype=torch.uint8) for _ in range(N))


def _boxes():
    return [torch.tensor([[x, y, x + w, y + h] for x, y, w, h in b], dtype=torch.float32) for b in FIXED]


def _model(dtype, params=None, *extra):
    """The yaml's model with random_standard_params for the detector (its scores spread) and the keypoint head's own initialiser."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.weights import random_standard_params
    torch.manual_seed(31)
    model = M.build_model(_cfg(*extra))
    sd = model.state_dict()
    for k, v in random_standard_params(0, num_classes=1).items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    for k, v in (params or {}).items():
        sd[k] = v
    model.load_state_dict(sd)
    model.kernel_dtype = dtype
    return model.eval()


def _pyramid(model):
    eng = model.engine()
    batch, sizes = model._stack_images(list(_images()))
    d = eng.cfg["size_divisibility"]
    hp, wp = (int(batch.shape[-2]) + d - 1) // d * d, (int(batch.shape[-1]) + d - 1) // d * d
    pyr = eng._backbone(batch, hp, wp)
    torch.cuda.synchronize()
    return eng, batch, sizes, (hp, wp), pyr


def _given(model, pyr):
    """forward_with_given_boxes on the fixed boxes -> (heatmaps (m, K, 56, 56), keypoints (m, K, 3)) on the CPU, RoIs in FIXED's order."""
    from openset_rcnn_amd.host.structures import Boxes, Instances
    feats = {k: pyr[k].permute(0, 3, 1, 2) for k in ("p2", "p3", "p4", "p5")}
    insts = [Instances(SIZE, pred_boxes=Boxes(b.to(DEV)), pred_classes=torch.zeros(len(b), dtype=torch.int64, device=DEV)) for b in _boxes()]
    out = model.roi_heads.forward_with_given_boxes(feats, insts)
    torch.cuda.synchronize()
    for o, b in zip(out, _boxes()):
        assert o.pred_keypoints.shape == (len(b), K, 3) and o.pred_keypoint_heatmaps.shape == (len(b), K, 56, 56)
        assert o.pred_keypoint_heatmaps.dtype == torch.float32 and torch.equal(o.pred_boxes.tensor.cpu(), b)
    return torch.cat([o.pred_keypoint_heatmaps.cpu() for o in out]), torch.cat([o.pred_keypoints.cpu() for o in out])


def _cpu_chain(pyr, p, wdtype, round_to=None):
    """The float64 keypoint branch on a pyramid (NHWC, any dtype) and the fixed boxes; parameters rounded to wdtype first (the stored
    operands). round_to: RoIAlign's and every conv_fcn layer's output rounded to that type (what an engine of that storage type keeps)."""
    rnd = (lambda t: t.to(round_to).double()) if round_to is not None else (lambda t: t)
    feats = [pyr[k].detach().cpu().float().permute(0, 3, 1, 2).contiguous() for k in ("p2", "p3", "p4", "p5")]
    x = rnd(O.roi_pooler_ref(feats, _boxes(), out_size=14).double())  # (the oracle's RoIAlign works in fp32; everything behind it is float64)
    for i in range(len(DIMS)):
        w, b = p[f"{PRE}conv_fcn{i + 1}.weight"].to(wdtype).double(), p[f"{PRE}conv_fcn{i + 1}.bias"].double()
        x = rnd(F.relu(F.conv2d(x, w, b, padding=1)))
    return upsample_chain(x.permute(0, 2, 3, 1), p[PRE + "score_lowres.weight"].to(wdtype), p[PRE + "score_lowres.bias"], torch.float64)


def _check_decode(kp, heat64, what):
    """kp (m, K, 3) against the float64 decode of heat64 (m, K, 56, 56) under the module docstring's rule."""
    ref = decode_chain(heat64, torch.cat(_boxes()), torch.float64)
    many = (ref["size"][:, 0] * ref["size"][:, 1] > 1)[:, None].expand_as(ref["gap"])
    clear = (ref["gap"] > GAP) | ~many
    share = 1.0 - float(clear.double().mean())
    o = kp.double()
    dx, dy = (o[..., 0] - ref["x"]).abs()[clear], (o[..., 1] - ref["y"]).abs()[clear]
    ds = ((o[..., 2] - ref["score"]).abs() / ref["score"])[clear]
    print(f"{what}: {int(clear.sum())} of {clear.numel()} pairs above the gap (share below {share:.3%}); |dx| {float(dx.max()):.2e} |dy| {float(dy.max()):.2e} px, "
          f"rel |dscore| {float(ds.max()):.2e}")
    assert share <= 0.05
    assert float(dx.max()) <= XY_TOL and float(dy.max()) <= XY_TOL and float(ds.max()) <= SCORE_RTOL


@functools.lru_cache(maxsize=None)
def _parity():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    model = _model(torch.float32)
    p = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith(PRE)}
    g = torch.Generator().manual_seed(41)
    for k in p:  # biases that are not zero, so that they are checked too
        if k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    eng, batch, sizes, hpwp, pyr = _pyramid(model)
    assert tuple(model.roi_heads.keypoint_head.state_dict()[f"conv_fcn{len(DIMS)}.weight"].shape) == (512, 512, 3, 3)
    # the tail is linear in (score_lowres.weight, score_lowres.bias): scaling both by 1 / std scales the heatmaps, exactly so in the
    # float64 chain, and the pyramid does not depend on the keypoint head
    scale = 1.0 / float(_cpu_chain(pyr, p, torch.float32).std())
    for k in (PRE + "score_lowres.weight", PRE + "score_lowres.bias"):
        p[k] = p[k] * scale
    model = _model(torch.float32, p)
    eng, batch, sizes, hpwp, pyr = _pyramid(model)
    ref = _cpu_chain(pyr, p, torch.float32)
    assert float(ref.std()) >= 0.5
    return dict(model=model, params=p, eng=eng, batch=batch, sizes=sizes, hpwp=hpwp, pyr=pyr, ref=ref)


def test_parity_mode_against_the_float64_chain(osr):
    s = _parity()
    heat, kp = _given(s["model"], s["pyr"])
    err = float((heat.double() - s["ref"]).abs().max())
    print(f"parity mode: {len(heat)} RoIs, heatmap std {float(s['ref'].std()):.3f}, max |heatmaps - float64| {err:.3e}")
    assert err <= HEAT_TOL
    _check_decode(kp, s["ref"], "parity mode, reference heatmaps")
    # the x, y of a keypoint lie inside its (clamped) box
    b = torch.cat(_boxes())
    x1, y1 = torch.maximum(b[:, 2], b[:, 0] + 1), torch.maximum(b[:, 3], b[:, 1] + 1)
    assert bool(((kp[..., 0] >= b[:, None, 0]) & (kp[..., 0] <= x1[:, None]) & (kp[..., 1] >= b[:, None, 1]) & (kp[..., 1] <= y1[:, None])).all())


def test_the_full_pass_and_the_postprocess(osr):
    from openset_rcnn_amd.host import modeling as M
    s = _parity()
    model = s["model"]
    res = s["eng"].forward(s["batch"], s["sizes"])
    torch.cuda.synchronize()
    assert len(res) == 6 and res[4].shape == (N, TOPK, K, 3) and res[5].shape == (N, TOPK, K, 56, 56)
    counts = [int(c) for c in res[3].cpu()]
    assert all(c >= 1 for c in counts), f"precondition: at least one detection per image, got {counts}"
    for i, c in enumerate(counts):  # rows beyond an image's detections are zeros
        if c < TOPK:
            assert float(res[4][i, c:].abs().max()) == 0.0 and float(res[5][i, c:].abs().max()) == 0.0
    raw = model.inference([{"image": im} for im in _images()], do_postprocess=False)
    out = model([{"image": im, "height": 2 * SIZE[0], "width": 3 * SIZE[1] // 2} for im in _images()])
    for i, (r, o) in enumerate(zip(raw, out)):
        r, o = r["instances"], o["instances"]
        assert len(r) == counts[i] and r.pred_keypoints.shape == (counts[i], K, 3) and r.pred_keypoint_heatmaps.shape == (counts[i], K, 56, 56)
        assert torch.equal(r.pred_keypoints.cpu(), res[4][i, :counts[i]].cpu())
        want = M.detector_postprocess(r, 2 * SIZE[0], 3 * SIZE[1] // 2)
        keep = ((r.pred_boxes.tensor[:, 2] > r.pred_boxes.tensor[:, 0]) & (r.pred_boxes.tensor[:, 3] > r.pred_boxes.tensor[:, 1])).cpu()
        assert len(o) == int(keep.sum()) == len(want) and o.image_size == (2 * SIZE[0], 3 * SIZE[1] // 2)
        rk = r.pred_keypoints.cpu()[keep]
        assert torch.allclose(o.pred_keypoints.cpu()[..., 0], rk[..., 0] * 1.5, rtol=1e-6, atol=0)
        assert torch.allclose(o.pred_keypoints.cpu()[..., 1], rk[..., 1] * 2.0, rtol=1e-6, atol=0)
        assert torch.equal(o.pred_keypoints.cpu()[..., 2], rk[..., 2])
        assert torch.equal(o.pred_keypoint_heatmaps.cpu(), r.pred_keypoint_heatmaps.cpu()[keep])
    # a keypoint row dropped with its box: a box that the clip empties
    from openset_rcnn_amd.host.structures import Boxes, Instances
    inst = Instances(SIZE, pred_boxes=Boxes(torch.tensor([[10.0, 10.0, 50.0, 60.0], [400.0, 10.0, 420.0, 60.0]])), scores=torch.tensor([0.9, 0.8]),
                     pred_classes=torch.zeros(2, dtype=torch.int64), pred_keypoints=torch.arange(2 * K * 3, dtype=torch.float32).view(2, K, 3),
                     pred_keypoint_heatmaps=torch.arange(2 * K * 4, dtype=torch.float32).view(2, K, 2, 2))
    pp = M.detector_postprocess(inst, SIZE[0], SIZE[1])
    assert len(pp) == 1 and torch.equal(pp.pred_keypoints, inst.pred_keypoints[:1]) and torch.equal(pp.pred_keypoint_heatmaps, inst.pred_keypoint_heatmaps[:1])


@functools.lru_cache(maxsize=None)
def _fp16():
    model = _model(torch.float16, _parity()["params"])
    return (model,) + _pyramid(model)


def test_fp16_mode(osr):
    p = _parity()["params"]
    model, eng, batch, sizes, hpwp, pyr = _fp16()
    heat, kp = _given(model, pyr)
    ref = _cpu_chain(pyr, p, torch.float16)
    e16 = float((_cpu_chain(pyr, p, torch.float16, round_to=torch.float16) - ref).abs().max())
    err = float((heat.double() - ref).abs().max())
    print(f"fp16 mode: max |heatmaps - float64| {err:.3e}, e16 {e16:.3e} (bound {4 * e16:.3e}), heatmap std {float(ref.std()):.3f}")
    assert err <= 4 * e16
    _check_decode(kp, heat.double(), "fp16 mode, the engine's own heatmaps")


def test_captured_replay_equals_the_eager_pass(osr):
    model, eng, batch, sizes, (hp, wp), _ = _fp16()
    hw = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    eager = [t.clone() for t in eng.forward_device(batch, hw, hp, wp)]
    graph, out = eng.capture(batch, hw, hp, wp)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 6 and int(eager[3].sum()) >= 1
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


def test_masks_and_keypoints_together(osr):
    model = _model(torch.float16, _parity()["params"], "MODEL.MASK_ON", "True")
    eng, batch, sizes, hpwp, pyr = _pyramid(model)
    res = eng.forward(batch, sizes)
    torch.cuda.synchronize()
    assert len(res) == 7 and res[4].shape == (N, TOPK, 28, 28) and res[5].shape == (N, TOPK, K, 3) and res[6].shape == (N, TOPK, K, 56, 56)
    heat, kp = _given(model, pyr)  # (forward_with_given_boxes attaches both branches' fields)
    _check_decode(kp, heat.double(), "MASK_ON + KEYPOINT_ON, the engine's own heatmaps")
    for o in model([{"image": im} for im in _images()]):
        inst = o["instances"]
        assert inst.pred_masks.shape == (len(inst),) + SIZE and inst.pred_masks.dtype == torch.bool
        assert inst.pred_keypoints.shape == (len(inst), K, 3) and inst.pred_keypoint_heatmaps.shape == (len(inst), K, 56, 56)
