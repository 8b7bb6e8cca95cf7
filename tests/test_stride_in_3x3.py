"""MODEL.RESNETS.STRIDE_IN_1X1 False (torchvision's ResNet-50: the stride of res3-res5 in the first block's 3x3): the model's
pyramid and the training step's backbone gradients against a plain torch-CPU ResNet-50-FPN written here, and a few stock
config-1 iterations. The default layout (True, MSRA) is checked against the same CPU model with the stride in the 1x1."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.test_standard_rcnn import coco_toy  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
R50_BLOCKS = (3, 4, 6, 3)


def _cfg(yaml, *opts, device="cpu"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", device, "SOLVER.BASE_LR", "0.0001", "SOLVER.WARMUP_ITERS", "0", "OPENDET_BENCHMARK", "True"] + list(opts))
    return cfg


def cpu_pyramid(P, x, stride_in_1x1):
    """[d2] ResNet-50 + FPN on BN-folded parameters P (name.weight (cout,cin,kh,kw), name.bias), fp32: p2..p6 (NCHW)."""
    def conv(x, name, stride=1, pad=0, relu=False):
        y = F.conv2d(x, P[name + ".weight"], P[name + ".bias"], stride, pad)
        return F.relu(y) if relu else y
    bu = "backbone.bottom_up."
    x = F.max_pool2d(conv(x, bu + "stem.conv1", 2, 3, True), 3, 2, 1)
    feats = {}
    for si, nb in enumerate(R50_BLOCKS):
        for b in range(nb):
            pre, st = f"{bu}res{si + 2}.{b}", 2 if (b == 0 and si > 0) else 1
            s1, s2 = (st, 1) if stride_in_1x1 else (1, st)
            sc = conv(x, pre + ".shortcut", st) if b == 0 else x
            o = conv(conv(x, pre + ".conv1", s1, 0, True), pre + ".conv2", s2, 1, True)
            x = F.relu(conv(o, pre + ".conv3") + sc)
        feats[si + 2] = x
    lat = conv(feats[5], "backbone.fpn_lateral5")
    out = {"p5": conv(lat, "backbone.fpn_output5", 1, 1)}
    for lvl in (4, 3, 2):
        lat = conv(feats[lvl], f"backbone.fpn_lateral{lvl}") + F.interpolate(lat, scale_factor=2, mode="nearest")
        out[f"p{lvl}"] = conv(lat, f"backbone.fpn_output{lvl}", 1, 1)
    out["p6"] = F.max_pool2d(out["p5"], 1, 2)
    return out


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-6))


def test_config_flag_reaches_the_engine(osr):
    from openset_rcnn_amd.host import modeling as M
    for yaml in ("voc_coco.yaml", "base_rcnn_fpn.yaml"):
        assert M.build_model(_cfg(yaml))._eng_cfg["stride_in_1x1"] is True
        model = M.build_model(_cfg(yaml, "MODEL.RESNETS.STRIDE_IN_1X1", "False"))
        assert model._eng_cfg["stride_in_1x1"] is False and model.backbone._eng_cfg["stride_in_1x1"] is False
    with pytest.raises(AssertionError):
        M.build_model(_cfg("voc_coco.yaml", "MODEL.RESNETS.DEPTH", "101"))
    with pytest.raises(AssertionError):
        M.build_model(_cfg("voc_coco.yaml", "MODEL.RESNETS.NORM", "BN"))


@pytest.mark.gpu
@pytest.mark.parametrize("stride_in_1x1", [False, True], ids=["stride_in_3x3", "msra"])
def test_model_pyramid_matches_cpu_resnet(osr, stride_in_1x1):
    """Model built from the yaml with random FrozenBN statistics; p2..p6 of the fp16 kernels and of the fp32 parity kernels against
    the CPU network of the same layout."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.weights import fold_frozen_bn
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    torch.manual_seed(0)
    model = M.build_model(_cfg("voc_coco.yaml", "MODEL.RESNETS.STRIDE_IN_1X1", str(stride_in_1x1)))
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
    model.backbone.load_state_dict(sd)
    P = fold_frozen_bn({"backbone." + k: v for k, v in sd.items()})
    x = torch.randn(2, 3, 128, 192, generator=g)
    ref = cpu_pyramid(P, x, stride_in_1x1)
    bb = model.backbone.to(DEV)
    for dtype, tol in ((torch.float32, 1e-4), (torch.float16, 2e-2)):
        bb.kernel_dtype = dtype
        bb.refresh()
        with torch.no_grad():
            out = bb(x.to(DEV))
        for k in ("p2", "p3", "p4", "p5", "p6"):
            assert out[k].shape == ref[k].shape, k
            assert rel(out[k], ref[k]) < tol, (dtype, k, rel(out[k], ref[k]))


@pytest.fixture(scope="module")
def trunk_batch(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from openset_rcnn_amd.host.weights import random_params
    g = torch.Generator().manual_seed(31)
    n, h, w = 2, 256, 320
    images = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    return dict(params=random_params(0), images=images, n=n, h=h, w=w, g=g)


@pytest.mark.gpu
@pytest.mark.parametrize("freeze_at", [0, 2, 3])
def test_trunk_gradients_match_autograd(trunk_batch, freeze_at):
    """One training step's backbone half (forward trunk + backward trunk, upstream gradient dP on p2..p6) with the stride in the 3x3,
    against autograd of the CPU network. dP is dense random noise on every pixel of every level (the heads' real gradient is sparse),
    carried in fp16 through fp16 activations: every layer, the stride-1 blocks of res2 included, lands at cosine 0.997-0.999 and
    norm within 1 %; tolerance cosine >= 0.995 (0.99 for the stem, through the max pool's argmax) and norm within 2 %. A stride in
    the wrong layer or a lost pixel of a data gradient is far outside that."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.engine import DEFAULT_CFG
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_stem_weight
    b = trunk_batch
    P, n, h, w = b["params"], b["n"], b["h"], b["w"]
    tr = OpensetRCNNTrainer(P, dict(stride_in_1x1=False), dtype=torch.float16, device=DEV, lr=0.002, loss_scale=1.0, freeze_at=freeze_at)
    s = {}
    p = tr._forward_trunk(b["images"].to(DEV), h, w, s)
    # the CPU network on the same normalised batch; fp16-rounded weights, as the kernels read them
    mean = torch.tensor(DEFAULT_CFG["pixel_mean"]).view(1, 3, 1, 1)
    Pc = {k: (v.half().float() if k.endswith(".weight") else v.clone()).requires_grad_(True) for k, v in P.items() if k.startswith("backbone.")}
    ref = cpu_pyramid(Pc, b["images"].float() - mean, False)
    g = torch.Generator().manual_seed(7 + freeze_at)
    dP = {k: torch.randn(ref[k].shape, generator=g).half() for k in ref}
    for k in ref:
        assert tuple(p[k].shape) == (n, ref[k].shape[2], ref[k].shape[3], 256), k
        assert rel(p[k].permute(0, 3, 1, 2), ref[k]) < 2e-2, (k, rel(p[k].permute(0, 3, 1, 2), ref[k]))
    sum((ref[k] * dP[k].float()).sum() for k in ref).backward()
    tr._backward_begin(1.0, False)
    tr._backward_trunk(s, {k: v.permute(0, 2, 3, 1).contiguous().to(DEV) for k, v in dP.items()}, None)
    torch.cuda.synchronize()
    bad, seen = [], set()
    for k, gten in tr.grad.items():
        if not k.startswith("backbone."):
            continue
        name = k[:-2]
        want = Pc[name + (".weight" if k.endswith(".w") else ".bias")].grad
        if k == "backbone.bottom_up.stem.conv1.w":
            want = pack_stem_weight(want, torch.float32)
        elif k.endswith(".w"):
            want = pack_conv_weight(want, torch.float32)
        got = gten.detach().cpu()
        assert got.shape == want.shape, k
        cos = float(F.cosine_similarity(got.flatten(), want.flatten(), dim=0))
        ratio = float(got.norm() / want.norm().clamp(min=1e-20))
        cos_min = 0.99 if "stem" in k else 0.995
        if not (cos >= cos_min and 0.98 <= ratio <= 1.02):
            bad.append(f"{k}: cos {cos:.5f} |got|/|ref| {ratio:.4f}")
        seen.add(k.split(".")[2] if k.startswith("backbone.bottom_up.") else "fpn")
    assert seen == {f"res{st}" for st in range(max(2, freeze_at + 1), 6)} | {"fpn"} | ({"stem"} if freeze_at == 0 else set())
    assert not bad, "gradient mismatch:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_stock_config1_trainer_learns_with_stride_in_3x3(osr, coco_toy):  # noqa: F811
    """A few iterations of the config-1 trainer (Base-RCNN-FPN: StandardRCNNTrainer) with STRIDE_IN_1X1 False on one fixed batch of
    the two-image COCO toy: finite losses that go down."""
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host import solver
    from openset_rcnn_amd.host.data import DatasetMapper, build_detection_test_loader
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    torch.manual_seed(0)
    cfg = _cfg("base_rcnn_fpn.yaml", "MODEL.RESNETS.STRIDE_IN_1X1", "False", "INPUT.MIN_SIZE_TEST", "480", "INPUT.MAX_SIZE_TEST", "640",
               "SOLVER.BASE_LR", "0.001", device=DEV)
    dicts = D.load_coco_json(os.path.join(coco_toy, "instances.json"), os.path.join(coco_toy, "images"))
    batch = next(iter(build_detection_test_loader(dicts, DatasetMapper(cfg, is_train=True), batch_size=2, rank=0, world=1)))
    model = M.build_model(cfg)
    assert model._eng_cfg["stride_in_1x1"] is False
    model.train()
    opt = solver.build_optimizer(cfg, model)
    totals = []
    for _ in range(6):
        losses = model(batch)
        total = sum(losses.values())
        totals.append(float(total))
        total.backward()
        opt.step()
    assert all(torch.isfinite(torch.tensor(totals))), totals
    assert totals[-1] < totals[0], totals
