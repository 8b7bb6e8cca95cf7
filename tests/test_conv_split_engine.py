"""The split parity mode on the GPU: OpensetRCNNEngine(dtype=float32, conv="split") -- fp32 storage, the convolutions and FC1 / FC2 on
the bf16 matrix instruction (ops.conv2d_split, ops.stem_conv_split, ops.linear_split) -- held to the bars of the fp32 parity mode.

The world is that of tests/test_e2e_parity.py: N = 4 seeded 256 x 384 images (seed 2024), weights.random_params(0) +
with_known_unknown_mix, the fp32 oracle (O.detector_inference's stages, no quantisation anywhere) as the reference.
  * every dense stage within 1e-4 of the oracle on the engine's own inputs to that stage;
  * >= 95 % of the final detections agree with the oracle (same class, IoU >= 0.99, |score difference| <= 1e-2), class ids equal on
    every match, matched box corners within 1e-4 of the image extent and scores within 1e-4;
  * a captured pass replays to the eager pass's bits; the model mirror selects the mode with conv_precision."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import c_binding as CO
from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 4, 256, 384


def _dets(eng, out):
    return [(d["pred_boxes"], d["scores"], d["pred_classes"]) for d in eng.to_instances(out, N)]


@pytest.fixture(scope="module")
def world(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import random_params, with_known_unknown_mix
    ops = osr.ops
    g = torch.Generator().manual_seed(2024)
    images = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8)
    sizes = [(H, W), (H, W), (H - 16, W - 40), (H - 6, W)]
    base = random_params(0)
    keep = {}
    eng32 = OpensetRCNNEngine(base, dtype=torch.float32, device=DEV)
    eng32.forward(images.to(DEV), sizes, keep=keep)
    cnt = keep["cnt1"].cpu()
    emb = torch.cat([keep["emb"].view(N, 1000, -1)[i, :int(cnt[i])] for i in range(N)])
    params = with_known_unknown_mix(base, emb)
    del eng32, keep
    with torch.no_grad():  # O.detector_inference with the true image sizes the engine gets
        batch, _ = O.preprocess_images([im for im in images])
        feats = O.resnet_fpn_forward(batch, params)
        props, _ = O.rpn_inference(feats, sizes, params, 1000)
        ref, _ = O.roi_heads_inference(feats, [(b, s) for b, s, _ in props], sizes, params, roi_align_fn=CO.roi_align)
    eng = OpensetRCNNEngine(params, dtype=torch.float32, device=DEV, conv="split")
    keep = {}
    ops.CONV_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    ops.LINEAR_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    out = eng.forward(images.to(DEV), sizes, keep=keep)
    torch.cuda.synchronize()
    counts = dict(conv=ops.CONV_SPLIT_COUNT["launches"], linear=ops.LINEAR_SPLIT_COUNT["launches"])
    ops.CONV_SPLIT_COUNT = ops.LINEAR_SPLIT_COUNT = None
    return dict(images=images, sizes=sizes, params=params, ref=ref, feats=feats, batch=batch, eng=eng, keep=keep, out=out, counts=counts,
                Engine=OpensetRCNNEngine)


def test_the_split_layers_ran_on_the_split_kernels(world):
    # stem + 16 bottlenecks x 3 + 4 shortcuts + 4 laterals + 4 outputs + the CF-RPN 3x3 on five levels; FC1 + FC2
    assert world["counts"] == dict(conv=1 + 48 + 4 + 4 + 4 + 5, linear=2)
    eng = world["eng"]
    assert eng.conv == "split" and eng.fc1_w is None and eng.fc2_w is None
    for k, v in eng.w.items():  # the split layers keep no fp32 copy of their weights
        if k.endswith(".w"):
            assert isinstance(v, tuple) and len(v) == 2 and all(t.dtype == torch.bfloat16 for t in v), k
    assert all(t.dtype == torch.bfloat16 for t in eng.fc1_split + eng.fc2_split)
    assert world["keep"]["feats"]["p2"].dtype == torch.float32 and world["keep"]["h1"].dtype == torch.float32


def test_dense_stages_within_1e_4(world):
    """Every dense stage tests/test_e2e_parity.py checks in the parity mode, against the oracle ON THE ENGINE'S OWN INPUTS to that stage."""
    keep, p = world["keep"], world["params"]
    nchw = lambda t: t.detach().cpu().float().permute(0, 3, 1, 2).contiguous()  # noqa: E731
    rel = lambda a, b: float((a.detach().cpu().float() - b).abs().max() / b.abs().max().clamp(min=1e-6))  # noqa: E731
    shown = {}
    feats = world["feats"]
    for k in ("p2", "p3", "p4", "p5", "p6"):
        shown[k] = rel(nchw(keep["feats"][k]), feats[k])
    ef = {k: nchw(v) for k, v in keep["feats"].items()}
    ds, cs = [], []
    for k in ("p2", "p3", "p4", "p5", "p6"):
        d, c = O.cfrpn_head(ef[k], p)
        ds.append(d)
        cs.append(c)
    ds, cs = O.flatten_head_outputs(ds, cs)
    shown["rpn_deltas"] = rel(keep["rpn_deltas"], torch.cat([d.reshape(-1, 4) for d in ds]))
    shown["rpn_ctr (absolute)"] = float((keep["rpn_ctr"].cpu() - torch.cat([c.reshape(-1) for c in cs])).abs().max())
    sel = keep["sel"]
    cap = sel["cap"]
    counts = [int(c) for c in sel["counts"].cpu()]
    boxes = [sel["boxes"][i, :counts[i]].cpu() for i in range(N)]
    pooled_ref = O.roi_pooler_ref([ef[k] for k in ("p2", "p3", "p4", "p5")], boxes, roi_align_fn=CO.roi_align)
    pooled = keep["pooled"].view(N, cap, 7, 7, 256)
    pe = torch.cat([pooled[i, :counts[i]] for i in range(N)]).cpu().float().permute(0, 3, 1, 2)
    shown["pooled (of max(1, max))"] = float((pe - pooled_ref).abs().max()) / max(1.0, float(pooled_ref.abs().max()))
    x = torch.flatten(pe, 1)
    h1 = F.relu(F.linear(x, p["roi_heads.box_head.fc1.weight"], p["roi_heads.box_head.fc1.bias"]))
    h1e = torch.cat([keep["h1"].view(N, cap, -1)[i, :counts[i]] for i in range(N)]).cpu()
    shown["h1"] = rel(h1e, h1)
    bf = F.relu(F.linear(h1e, p["roi_heads.box_head.fc2.weight"], p["roi_heads.box_head.fc2.bias"]))
    bfe = torch.cat([keep["box_feats"].view(N, cap, -1)[i, :counts[i]] for i in range(N)]).cpu()
    shown["box_feats"] = rel(bfe, bf)
    d_ref, _ = O.box_predictor(bfe, p)
    pd = keep["pred"]["pred_deltas"].view(N, cap, 4)
    shown["pred_deltas"] = rel(torch.cat([pd[i, :counts[i]] for i in range(N)]), d_ref)
    cnt1 = keep["cnt1"].cpu()
    shown["emb"] = shown["rec"] = 0.0
    for i in range(N):
        c = int(cnt1[i])
        _, rec, _, emb = O.pln_inference(keep["det_feats"][i, :c].cpu(), p, 0.23, 80, 20)
        shown["emb"] = max(shown["emb"], rel(keep["emb"].view(N, 1000, -1)[i, :c], emb))
        shown["rec"] = max(shown["rec"], rel(keep["rec"].view(N, 1000, -1)[i, :c], rec))
    print("\n[split parity mode, dense stages] " + "; ".join(f"{k} {v:.3e}" for k, v in shown.items()))
    for k, v in shown.items():
        assert v < 1e-4, (k, v)


def test_detections_match_the_fp32_oracle(world):
    from openset_rcnn_amd.host.agreement import detection_agreement
    ref, eng = world["ref"], world["eng"]
    assert sum(int((r[2] != 80).sum()) for r in ref) > 20 and sum(int((r[2] == 80).sum()) for r in ref) > 20, "weights must give both kinds"
    dets = _dets(eng, world["out"])
    ag = detection_agreement(dets, ref)
    total = max(ag["reference_detections"], ag["returned_detections"], 1)
    extent = float(max(H, W))
    print(f"\n[split parity mode] detection agreement {ag['matched']}/{total} = {ag['matched'] / total:.4f} (IoU >= 0.99, |dscore| <= 1e-2); "
          f"max |box diff| {ag['max_box_abs_diff_px']:.3e} px ({ag['max_box_abs_diff_px'] / extent:.2e} of the image extent), "
          f"max |score diff| {ag['max_score_abs_diff']:.3e}")
    assert ag["matched"] / total >= 0.95, ag
    assert ag["same_class"] == ag["matched"], ag  # class ids equal on every match
    assert ag["max_box_abs_diff_px"] / extent <= 1e-4, ag
    assert ag["max_score_abs_diff"] <= 1e-4, ag
    # report only: agreement with the fp32 parity engine
    e32 = world["Engine"](world["params"], dtype=torch.float32, device=DEV)
    out32 = e32.forward(world["images"].to(DEV), world["sizes"])
    torch.cuda.synchronize()
    a2 = detection_agreement(dets, _dets(e32, out32))
    print(f"[split parity mode vs the fp32 parity engine] {a2['matched']}/{max(a2['reference_detections'], a2['returned_detections'])} = {a2['fraction']:.4f}")


def test_captured_pass_replays_the_eager_bits(world):
    eng = world["eng"]
    imgs = world["images"].to(DEV)
    hw = torch.tensor(world["sizes"], dtype=torch.int32, device=DEV)
    plain = [t.clone() for t in eng.forward_device(imgs, hw, H, W)]
    graph, gout = eng.capture(imgs, hw, H, W, nstreams=1)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(plain, gout):
        assert torch.equal(x, y)


def test_model_attribute_selects_the_mode(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import random_params
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "voc_coco.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "OPENDET_BENCHMARK", "True"])
    model = M.build_model(cfg).eval()
    p = random_params(0)
    sd = model.state_dict()
    for k, v in p.items():  # seeded BN-folded parameters through the state-dict surface (identity FrozenBN statistics)
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    model = model.to(DEV)
    assert model.conv_precision == "storage" and model.engine().conv == "storage"
    model.conv_precision = "split"
    with pytest.raises(ValueError):
        model.engine()  # needs kernel_dtype float32
    model.kernel_dtype = torch.float32
    eng = model.engine()
    assert eng.conv == "split" and eng.dtype == torch.float32 and model.roi_heads.engine() is eng
    with pytest.raises(ValueError):
        model.make_trainer()
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randint(0, 256, (3, 128, 160), generator=g, dtype=torch.uint8) for _ in range(2)]
    out = model([{"image": im, "height": 128, "width": 160} for im in imgs])
    direct = OpensetRCNNEngine(p, model._eng_cfg, torch.float32, DEV, model._class_map, conv="split")
    res = direct.to_instances(direct.forward(torch.stack(imgs).to(DEV)), 2)
    assert sum(len(r["scores"]) for r in res) > 0
    for r, o in zip(res, out):
        inst = o["instances"]
        assert torch.allclose(inst.pred_boxes.tensor.cpu(), r["pred_boxes"].cpu()) and torch.equal(inst.scores.cpu(), r["scores"].cpu())
        assert torch.equal(inst.pred_classes.cpu(), r["pred_classes"].cpu())
    model.conv_precision = "storage"
    eng2 = model.engine()
    assert eng2 is not eng and eng2.conv == "storage" and not isinstance(eng2.w["backbone.fpn_lateral5.w"], tuple)
