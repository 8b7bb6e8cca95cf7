"""MODEL.RESNETS.DEFORM_ON_PER_STAGE on the engine: the trunk with deformable res3..res5 against a torch-CPU ResNet-50-FPN written here
(tests/test_stride_in_3x3.py's network and bounds, extended with the float64 deformable convolution of tests/test_deform_kernels.py), what
the flags leave untouched when they are all False, and one end-to-end pass of configs/mask_rcnn_dconv_c3_c5.yaml (stock and cascade heads)
eager and as a captured graph.

Bounds, as in test_stride_in_3x3.py::test_model_pyramid_matches_cpu_resnet: max |got - ref| / max |ref| per pyramid level < 1e-4 for the
fp32 engine (the correctness contract) and < 2e-2 for the fp16 engine."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests.test_deform_kernels import ref_cols
from tests.test_stride_in_3x3 import cpu_pyramid, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
R50_BLOCKS = (3, 4, 6, 3)
C3_C5 = (False, True, True, True)
TOLS = ((torch.float32, 1e-4), (torch.float16, 2e-2))


def _cfg(yaml, *opts, device="cpu"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", device, "OPENDET_BENCHMARK", "True"] + list(opts))
    return cfg


def dconv_ref(x, om, weight, bias, stride, groups, modulated):
    """The binding definition on NCHW fp32 tensors: float64 samples (ref_cols) contracted with weight (cout,cin,3,3) in float64."""
    n, c = x.shape[:2]
    cols, _ = ref_cols(x.permute(0, 2, 3, 1).contiguous(), om.permute(0, 2, 3, 1).contiguous(), stride, groups, modulated)
    wm = weight.double().permute(0, 2, 3, 1).reshape(weight.shape[0], 9 * c)  # (cout, tap, cin): cols' K order
    y = cols.view(-1, 9 * c) @ wm.t() + bias.double()
    return y.view(n, om.shape[2], om.shape[3], -1).permute(0, 3, 1, 2).float()


def cpu_deform_pyramid(P, x, stride_in_1x1, deform, groups, modulated, offset_std=None):
    """cpu_pyramid with a DeformBottleneckBlock in the stages `deform` flags: om = conv2_offset(o1), o2 = relu(dconv(o1, om) + b2).
    offset_std: each block's conv2_offset weight and bias in P are first rescaled, in place, so that its outputs on this input have
    that standard deviation (offsets in pixels, mask logits alike) -- the caller then loads P's values into the model."""
    def conv(x, name, stride=1, pad=0, relu=False):
        y = F.conv2d(x, P[name + ".weight"], P[name + ".bias"], stride, pad)
        return F.relu(y) if relu else y
    bu = "backbone.bottom_up."
    x = F.max_pool2d(conv(x, bu + "stem.conv1", 2, 3, True), 3, 2, 1)
    feats, spread = {}, []
    for si, nb in enumerate(R50_BLOCKS):
        for b in range(nb):
            pre, st = f"{bu}res{si + 2}.{b}", 2 if (b == 0 and si > 0) else 1
            s1, s2 = (st, 1) if stride_in_1x1 else (1, st)
            sc = conv(x, pre + ".shortcut", st) if b == 0 else x
            o1 = conv(x, pre + ".conv1", s1, 0, True)
            if deform[si]:
                if offset_std is not None:
                    scale = offset_std / float(conv(o1, pre + ".conv2_offset", s2, 1).std())
                    P[pre + ".conv2_offset.weight"] = P[pre + ".conv2_offset.weight"] * scale
                    P[pre + ".conv2_offset.bias"] = P[pre + ".conv2_offset.bias"] * scale
                om = conv(o1, pre + ".conv2_offset", s2, 1)
                spread.append(float(om[:, :18 * groups].std()))
                o = F.relu(dconv_ref(o1, om, P[pre + ".conv2.weight"], P[pre + ".conv2.bias"], s2, groups, modulated))
            else:
                o = conv(o1, pre + ".conv2", s2, 1, True)
            x = F.relu(conv(o, pre + ".conv3") + sc)
        feats[si + 2] = x
    lat = conv(feats[5], "backbone.fpn_lateral5")
    out = {"p5": conv(lat, "backbone.fpn_output5", 1, 1)}
    for lvl in (4, 3, 2):
        lat = conv(feats[lvl], f"backbone.fpn_lateral{lvl}") + F.interpolate(lat, scale_factor=2, mode="nearest")
        out[f"p{lvl}"] = conv(lat, f"backbone.fpn_output{lvl}", 1, 1)
    out["p6"] = F.max_pool2d(out["p5"], 1, 2)
    return out, spread


def _model_with_random_bn(*opts):
    """test_model_pyramid_matches_cpu_resnet's model: voc_coco.yaml, random FrozenBN statistics (seed 5) -> (model, backbone state, x)."""
    from openset_rcnn_amd.host import modeling as M
    torch.manual_seed(0)
    model = M.build_model(_cfg("voc_coco.yaml", "MODEL.RESNETS.DEFORM_ON_PER_STAGE", str(list(C3_C5)), *opts))
    g = torch.Generator().manual_seed(5)
    sd = model.backbone.state_dict()
    for k in sd:
        if k.endswith("norm.running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif k.endswith("norm.running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
        elif k.endswith("norm.weight"):
            sd[k] = torch.rand(sd[k].shape, generator=g) * 0.5 + 0.5
        elif k.endswith("norm.bias"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    x = torch.randn(2, 3, 128, 192, generator=g)
    return model, sd, x, g


def _compare(model, sd, x, ref, what):
    model.backbone.load_state_dict(sd)
    bb = model.backbone.to(DEV)
    for dtype, tol in TOLS:
        bb.kernel_dtype = dtype
        bb.refresh()
        with torch.no_grad():
            out = bb(x.to(DEV))
        for k in ("p2", "p3", "p4", "p5", "p6"):
            assert out[k].shape == ref[k].shape, k
            r = rel(out[k], ref[k])
            print(f"[rel] {what} {str(dtype)[6:]} {k}: {r:.3e} (bound {tol:g})")
            assert r < tol, (what, dtype, k, r)


@pytest.mark.parametrize("stride_in_1x1", [True, False], ids=["msra", "stride_in_3x3"])
def test_zero_offsets_give_the_plain_network(osr, stride_in_1x1):
    """conv2_offset at its zero initialisation: the deformable route (no fused res2 / chained res3 launch in the deformable stages) must
    give what the plain CPU network gives."""
    from openset_rcnn_amd.host.weights import fold_frozen_bn
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    model, sd, x, _ = _model_with_random_bn("MODEL.RESNETS.STRIDE_IN_1X1", str(stride_in_1x1))
    assert not any(sd[k].any() for k in sd if "conv2_offset" in k)
    P = fold_frozen_bn({"backbone." + k: v for k, v in sd.items()})
    _compare(model, sd, x, cpu_pyramid(P, x, stride_in_1x1), "zero offsets")
    assert model.backbone.engine().deform == C3_C5


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("stride_in_1x1", [True, False], ids=["msra", "stride_in_3x3"])
@pytest.mark.parametrize("modulated", [False, True], ids=["dcn", "modulated"])
def test_random_offsets_match_the_cpu_network(osr, modulated, stride_in_1x1, groups):
    """conv2_offset drawn so that every block's offsets have a standard deviation of 1 px on this input (on res5's 4 x 6 map many
    samples then fall outside), against the CPU network with the float64 deformable convolution."""
    from openset_rcnn_amd.host.weights import fold_frozen_bn
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    model, sd, x, g = _model_with_random_bn("MODEL.RESNETS.STRIDE_IN_1X1", str(stride_in_1x1), "MODEL.RESNETS.DEFORM_MODULATED", str(modulated),
                                            "MODEL.RESNETS.DEFORM_NUM_GROUPS", str(groups))
    for k in sd:
        if "conv2_offset" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g)
    P = fold_frozen_bn({"backbone." + k: v for k, v in sd.items()})
    ref, spread = cpu_deform_pyramid(P, x, stride_in_1x1, C3_C5, groups, modulated, offset_std=1.0)
    assert len(spread) == 13 and all(0.7 < s < 1.3 for s in spread), spread
    for k in sd:
        if "conv2_offset" in k:
            sd[k] = P["backbone." + k]  # (the rescaled values)
    _compare(model, sd, x, ref, f"random offsets modulated={modulated} G={groups}")


def _profiled_pyramid(params, cfg, images, dtype):
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    eng = OpensetRCNNEngine(params, cfg, dtype, DEV)
    eng.profile = []
    feats = eng._backbone(images, images.shape[2], images.shape[3])
    torch.cuda.synchronize()
    return feats, [e[0] for e in eng.profile]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_all_false_changes_no_launch_and_no_bit(osr, dtype):
    """An engine configured with the three keys, every stage False (modulated and grouped: both must be inert), launches what an engine
    built without the keys launches, name for name, and gives the same bits. With res3..res5 deformable the res2 blocks stay fused, the
    shortcut + conv1 pair launches stay, and every deformable block runs conv2_offset, the gather and the contraction in place of the
    chained or plain conv2."""
    from openset_rcnn_amd.host.weights import deform_offset_params, random_params
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    params = {k: v for k, v in random_params(0).items() if k.startswith("backbone.")}
    images = torch.randint(0, 256, (2, 3, 128, 192), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(DEV)
    base, names = _profiled_pyramid(params, None, images, dtype)
    off, names_off = _profiled_pyramid(params, dict(deform_on_per_stage=(False,) * 4, deform_modulated=True, deform_num_groups=2), images, dtype)
    assert names_off == names and not [n for n in names if "deform" in n or "conv2_offset" in n]
    assert all(torch.equal(off[k], base[k]) for k in base)
    fast = dtype != torch.float32
    fused, chained = sum("(fused block)" in n for n in names), sum("(chained)" in n for n in names)
    assert (fused, chained) == (3, 4) if fast else (fused, chained) == (0, 0), (fused, chained)  # res2's blocks; res3's conv2 -> conv3
    dparams = dict(params, **deform_offset_params(C3_C5))  # zero offsets: the same function, another route
    on, names_on = _profiled_pyramid(dparams, dict(deform_on_per_stage=C3_C5), images, dtype)
    assert sum("(fused block)" in n for n in names_on) == fused and not [n for n in names_on if "(chained)" in n]
    for tag in ("conv2_offset", "(deform gather)", "(deform contraction)"):
        assert sum(tag in n for n in names_on) == 13, tag
    assert sum("(one launch)" in n for n in names_on) == sum("(one launch)" in n for n in names)
    assert len(names_on) == len(names) + 13 * 2 + chained  # conv2 -> three launches; a chained launch also gives its conv3 back
    tol = 2e-2 if fast else 1e-4
    assert all(rel(on[k], base[k]) < tol for k in base)


K, TOPK = 5, 8
SIZES = [(96, 128), (80, 112)]


@functools.lru_cache(maxsize=None)
def _e2e_params(cascade: bool):
    from openset_rcnn_amd.host.weights import deform_offset_params, random_cascade_params, random_standard_params
    p = dict(random_cascade_params(0, stages=3, num_classes=K) if cascade else random_standard_params(0, num_classes=K))
    p.update(deform_offset_params(C3_C5, std=1.0, seed=1))
    g = torch.Generator().manual_seed(4000)
    pre = "roi_heads.mask_head."
    for i in range(1, 5):
        p[f"{pre}mask_fcn{i}.weight"] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        p[f"{pre}mask_fcn{i}.bias"] = torch.randn(256, generator=g) * 0.02
    p[pre + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (2.0 / 256) ** 0.5
    p[pre + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
    p[pre + "predictor.weight"] = torch.randn(1, 256, 1, 1, generator=g) * 0.05
    p[pre + "predictor.bias"] = torch.randn(1, generator=g) * 0.1
    return p


@pytest.mark.parametrize("cascade", [False, True], ids=["mask_rcnn", "cascade_mask_rcnn"])
def test_the_shipped_yaml_end_to_end_eager_and_captured(osr, cascade):
    """configs/mask_rcnn_dconv_c3_c5.yaml (with CascadeROIHeads: plus that key) on two small synthetic images through model.eval():
    Instances with boxes, classes and masks come back, and a captured (hipGraph) replay of the pass equals the eager pass bit for bit."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Instances
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    opts = ["MODEL.ROI_HEADS.NUM_CLASSES", str(K), "MODEL.ROI_HEADS.SCORE_THRESH_TEST", "0.01", "TEST.DETECTIONS_PER_IMAGE", str(TOPK),
            "MODEL.RPN.POST_NMS_TOPK_TEST", "200"] + (["MODEL.ROI_HEADS.NAME", "CascadeROIHeads"] if cascade else [])
    model = M.build_model(_cfg("mask_rcnn_dconv_c3_c5.yaml", *opts, device=DEV))
    assert type(model.roi_heads).__name__ == ("CascadeROIHeads" if cascade else "StandardROIHeads") and model.roi_heads.mask_on
    sd = model.state_dict()
    for k, v in _e2e_params(cascade).items():
        if k in sd:
            assert sd[k].shape == v.shape, k
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
        else:
            raise AssertionError(k)
    model.load_state_dict(sd)
    model.eval()
    g = torch.Generator().manual_seed(11)
    images = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in SIZES]
    outs = model([{"image": im, "height": h, "width": w} for im, (h, w) in zip(images, SIZES)])
    assert len(outs) == 2
    total = 0
    for o, (h, w) in zip(outs, SIZES):
        inst = o["instances"]
        assert isinstance(inst, Instances) and inst.image_size == (h, w)
        assert inst.pred_masks.shape == (len(inst), h, w) and inst.pred_masks.dtype == torch.bool
        assert bool(torch.isfinite(inst.pred_boxes.tensor).all()) and bool(torch.isfinite(inst.scores).all())
        total += len(inst)
    assert total > 0
    eng = model.engine()
    assert eng.deform == C3_C5 and "backbone.bottom_up.res3.0.conv2_offset.w" in eng.w and "backbone.bottom_up.res2.0.conv2_offset.w" not in eng.w
    batch, sizes = model._stack_images(images)
    hw = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    hp, wp = (int(batch.shape[-2]) + 31) // 32 * 32, (int(batch.shape[-1]) + 31) // 32 * 32
    eager = [t.clone() for t in eng.forward_device(batch, hw, hp, wp)]
    graph, out = eng.capture(batch, hw, hp, wp)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 5 and int(eager[3].sum()) >= total  # (the postprocess may drop a box that clips to nothing)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
