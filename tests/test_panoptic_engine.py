"""META_ARCHITECTURE "PanopticFPN" / "SemanticSegmentor" on the engine (host/engine_panoptic.py) against a torch-CPU fp32 network written
here: the R-50 trunk with folded FrozenBN, the FPN on res2..res5, SemSegFPNHead with F.group_norm / F.interpolate, the predictor, and
detectron2's two interpolations behind it (tests/panoptic_common.py). Two images of different sizes within a 128 x 160 pad, 5 thing
classes, 54 stuff classes.

Bounds: max |got - ref| / max |ref| < 1e-4 per tensor for the fp32 engine (the project's fp32 contract) and < 2e-2 for the fp16 engine
(the project's fp16 trunk bound). The parity engine's labels equal the reference's outside pixels whose reference gap is under
1e-3 max |ref| (the engine's error may move both logits); tests/test_panoptic_reference.py asserts that this excludes at most 5 %.
panoptic_seg / segments_info equal detectron2's loop run on the engine's own masks, scores, classes and labels, exactly."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests.panoptic_common import combine_reference, resample_reference, segments_info_reference, top_two_gap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
R50_BLOCKS = (3, 4, 6, 3)
K, C, PITCH = 5, 54, 56
SIZES = [(128, 160), (112, 144)]
OUT_SIZES = [(160, 200), (90, 116)]  # an upscale and a downscale of the two inputs
HP, WP = 128, 160
MEAN = (103.53, 116.28, 123.675)
# the seed and the predictor's gain: chosen on the CPU so that the reference's top-two gap is under 1e-3 max |ref| on at most 5 % of
# the output pixels (asserted in tests/test_panoptic_reference.py)
SEED, PREDICTOR_GAIN = 7, 4.0
COMBINE = dict(overlap_thresh=0.5, stuff_area_limit=64, instances_confidence_thresh=0.3)
HEAD_LENGTHS = {"p2": 1, "p3": 1, "p4": 2, "p5": 3}


def rel(a, b):
    return float((a.detach().float().cpu() - b).abs().max() / b.abs().max())


def cpu_network(P, x, norm="GN"):
    """x (n, 3, HP, WP) normalised, zero padded -> (pyramid p2..p5 NCHW, head stages {name: conv output, name + ".out": after GN + ReLU + x2},
    the sum, the stride-4 logits (n, C, HP / 4, WP / 4))."""
    def conv(x, name, stride=1, pad=0, relu=False):
        y = F.conv2d(x, P[name + ".weight"], P.get(name + ".bias"), stride, pad)
        return F.relu(y) if relu else y
    bu = "backbone.bottom_up."
    x = F.max_pool2d(conv(x, bu + "stem.conv1", 2, 3, True), 3, 2, 1)
    feats = {}
    for si, nb in enumerate(R50_BLOCKS):
        for b in range(nb):
            pre, st = f"{bu}res{si + 2}.{b}", 2 if (b == 0 and si > 0) else 1
            sc = conv(x, pre + ".shortcut", st) if b == 0 else x
            o = conv(conv(conv(x, pre + ".conv1", st, 0, True), pre + ".conv2", 1, 1, True), pre + ".conv3")
            x = F.relu(o + sc)
        feats[si + 2] = x
    lat = conv(feats[5], "backbone.fpn_lateral5")
    pyr = {"p5": conv(lat, "backbone.fpn_output5", 1, 1)}
    for lvl in (4, 3, 2):
        lat = conv(feats[lvl], f"backbone.fpn_lateral{lvl}") + F.interpolate(lat, scale_factor=2, mode="nearest")
        pyr[f"p{lvl}"] = conv(lat, f"backbone.fpn_output{lvl}", 1, 1)
    stages, total = {}, None
    for feat, length in HEAD_LENGTHS.items():
        t = pyr[feat]
        for k in range(length):
            name = f"sem_seg_head.{feat}.{2 * k}"
            y = conv(t, name, 1, 1)
            stages[name] = y
            if norm == "GN":
                y = F.group_norm(y, 32, P[name + ".norm.weight"], P[name + ".norm.bias"], 1e-5)
            t = F.relu(y)
            if feat != "p2":
                t = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
            stages[name + ".out"] = t
        total = t if total is None else total + t
    return pyr, stages, total, conv(total, "sem_seg_head.predictor")


@functools.lru_cache(maxsize=None)
def setup():
    """The parameters, the images and the CPU reference, computed once and shared by the tests (read-only)."""
    from openset_rcnn_amd.host.weights import random_panoptic_params
    P = random_panoptic_params(SEED, num_classes=K, sem_classes=C, predictor_gain=PREDICTOR_GAIN)
    g = torch.Generator().manual_seed(21)
    images = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in SIZES]
    x = torch.zeros(len(images), 3, HP, WP)
    mean = torch.tensor(MEAN).view(3, 1, 1)
    for i, im in enumerate(images):
        x[i, :, : im.shape[1], : im.shape[2]] = im.float() - mean
    with torch.no_grad():
        pyr, stages, total, logits = cpu_network(P, x)
    sem = [resample_reference(logits[i].permute(1, 2, 0), s, o) for i, (s, o) in enumerate(zip(SIZES, OUT_SIZES))]
    return dict(P=P, images=images, pyr=pyr, stages=stages, total=total, logits=logits, sem=sem)


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "panoptic_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.NUM_CLASSES", str(K), "MODEL.PANOPTIC_FPN.COMBINE.STUFF_AREA_LIMIT", str(COMBINE["stuff_area_limit"]),
                         "MODEL.PANOPTIC_FPN.COMBINE.INSTANCES_CONFIDENCE_THRESH", str(COMBINE["instances_confidence_thresh"])] + list(opts))
    return cfg


@functools.lru_cache(maxsize=None)
def model_of(meta_arch, dtype):
    from openset_rcnn_amd.host import modeling as M
    s = setup()
    model = M.build_model(_cfg("MODEL.META_ARCHITECTURE", meta_arch))
    sd = model.state_dict()
    for k, v in s["P"].items():
        if k in sd:
            assert sd[k].shape == v.shape, k
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
        elif meta_arch == "PanopticFPN":
            raise AssertionError(k)
    model.load_state_dict(sd)
    model.eval()
    model.kernel_dtype = dtype
    return model


def _engine_pass(dtype):
    model = model_of("PanopticFPN", dtype)
    eng = model.engine()
    batch, sizes = model._stack_images(list(setup()["images"]))
    hw = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    keep = {}
    out = eng.forward_device(batch, hw, HP, WP, keep)
    torch.cuda.synchronize()
    return eng, batch, hw, out, keep


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float16, 2e-2)], ids=["fp32", "fp16"])
def test_head_stages_and_logits_match_the_cpu_network(osr, dtype, tol):
    s = setup()
    eng, _, _, out, keep = _engine_pass(dtype)
    assert type(eng).__name__ == "PanopticFPNEngine" and eng.sem_pitch == PITCH and len(out) == 6
    assert set(keep["sem_stages"]) == set(s["stages"]) - {f"sem_seg_head.{f}.{2 * (l - 1)}.out" for f, l in HEAD_LENGTHS.items()}
    for name, got in keep["sem_stages"].items():
        r = rel(got.permute(0, 3, 1, 2), s["stages"][name])
        print(f"[rel] {str(dtype)[6:]} {name}: {r:.3e} (bound {tol:g})")
        assert r < tol, (name, r)
    r = rel(keep["sem_sum"].permute(0, 3, 1, 2), s["total"])
    print(f"[rel] {str(dtype)[6:]} sum: {r:.3e} (bound {tol:g})")
    assert r < tol
    logits = out[-1]
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (2, HP // 4, WP // 4, PITCH)
    r = rel(logits[..., :C].permute(0, 3, 1, 2), s["logits"])
    print(f"[rel] {str(dtype)[6:]} logits: {r:.3e} (bound {tol:g})")
    assert r < tol
    assert float(logits[..., C:].abs().max()) == 0.0


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float16, 2e-2)], ids=["fp32", "fp16"])
def test_model_outputs_and_the_combine_loop_on_its_own_outputs(osr, dtype, tol):
    from openset_rcnn_amd.host.structures import Instances
    ops = osr.ops
    s = setup()
    model = model_of("PanopticFPN", dtype)
    outs = model([{"image": im, "height": h, "width": w} for im, (h, w) in zip(s["images"], OUT_SIZES)])
    logits = _engine_pass(dtype)[3][-1]
    things = stuff = 0
    for i, (o, size, out_hw) in enumerate(zip(outs, SIZES, OUT_SIZES)):
        assert set(o) == {"sem_seg", "instances", "panoptic_seg"}
        sem, inst, (pan, info) = o["sem_seg"], o["instances"], o["panoptic_seg"]
        assert sem.dtype == torch.float32 and tuple(sem.shape) == (C,) + out_hw
        ref = s["sem"][i]
        r = float((sem.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"[rel] {str(dtype)[6:]} sem_seg {i}: {r:.3e} (bound {tol:g})")
        assert r < tol
        labels = ops.semseg_resample(logits[i], C, size, out_hw, labels=True)
        if dtype == torch.float32:
            sure = top_two_gap(ref) >= 1e-3 * float(ref.abs().max())
            assert torch.equal(labels.cpu()[sure].long(), ref.argmax(dim=0)[sure])
        assert isinstance(inst, Instances) and inst.image_size == out_hw and inst.pred_masks.dtype == torch.bool
        assert tuple(inst.pred_masks.shape) == (len(inst),) + out_hw
        pan_ref, table, scores, events = combine_reference(inst.pred_masks.cpu(), inst.scores.cpu().float(), inst.pred_classes.cpu(), labels.cpu(), **COMBINE)
        assert pan.dtype == torch.int32 and torch.equal(pan.cpu(), pan_ref)
        assert info == segments_info_reference(table, [float(torch.tensor(v, dtype=torch.float32)) for v in scores])
        things += sum(1 for row in table if row[0])
        stuff += sum(1 for row in table if not row[0])
    print(f"[combine] {str(dtype)[6:]}: {things} thing and {stuff} stuff segments over the two images")
    assert things >= 1 and stuff >= 1  # (the comparison above is not vacuous)


def test_semantic_segmentor_returns_the_same_sem_seg(osr):
    s = setup()
    inputs = [{"image": im, "height": h, "width": w} for im, (h, w) in zip(s["images"], OUT_SIZES)]
    pan = model_of("PanopticFPN", torch.float32)(inputs)
    sem_model = model_of("SemanticSegmentor", torch.float32)
    assert not [k for k in sem_model.state_dict() if k.startswith(("proposal_generator.", "roi_heads."))]
    sem = sem_model(inputs)
    for a, b in zip(sem, pan):
        assert set(a) == {"sem_seg"} and torch.equal(a["sem_seg"], b["sem_seg"])
    eng = sem_model.engine()
    assert not eng.has_rpn and not eng.has_roi and not eng.has_mask and eng.has_sem_seg


def test_no_norm_head_matches_the_cpu_network(osr):
    """SEM_SEG_HEAD.NORM "": the convolutions carry a bias, the merge only rectifies and upsamples."""
    from openset_rcnn_amd.host.engine_panoptic import PanopticFPNEngine
    from openset_rcnn_amd.host.weights import random_panoptic_params
    P = random_panoptic_params(SEED, num_classes=K, sem_classes=C, norm="", rcnn=False)
    s = setup()
    x = torch.zeros(2, 3, HP, WP)
    batch = torch.tensor(MEAN).view(1, 3, 1, 1).expand(2, 3, HP, WP).clone()
    for i, im in enumerate(s["images"]):
        x[i, :, : im.shape[1], : im.shape[2]] = im.float() - torch.tensor(MEAN).view(3, 1, 1)
        batch[i, :, : im.shape[1], : im.shape[2]] = im.float()
    with torch.no_grad():
        _, _, total, logits = cpu_network(P, x, norm="")
    eng = PanopticFPNEngine(P, dict(sem_seg_norm="", pixel_mean=MEAN, pixel_std=(1.0, 1.0, 1.0)), torch.float32, DEV)
    keep = {}
    (got,) = eng.forward_device(batch.to(DEV), torch.tensor(SIZES, dtype=torch.int32, device=DEV), HP, WP, keep)
    assert rel(keep["sem_sum"].permute(0, 3, 1, 2), total) < 1e-4
    assert rel(got[..., :C].permute(0, 3, 1, 2), logits) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_eager_and_captured_passes_are_bit_identical(osr, dtype):
    eng, batch, hw, out, _ = _engine_pass(dtype)
    eager = [t.clone() for t in out]
    again = eng.forward_device(batch, hw, HP, WP)
    graph, cap = eng.capture(batch, hw, HP, WP)
    for t in cap:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(cap) == 6 and int(eager[3].sum()) > 0
    for a, b, c in zip(cap, eager, again):
        assert torch.equal(a, b) and torch.equal(c, b)
