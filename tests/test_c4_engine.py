"""Faster R-CNN R50-C4 on the HIP path (host/engine_c4.py) against the CPU reference of tests/c4_common.py, stage by stage, each stage
fed the engine's own inputs to it: RPN logits and deltas, the proposals, the pooled rows (the strided slice of the full RoIAlign grid),
res5 + mean (box_feats), the predictor and the detections; then the fp32 engine against the whole fp32 reference, both
STRIDE_IN_1X1 layouts, a run without a detection, the model mirror's Instances and the COCO evaluator on them.

Two images, 96 x 128 and 128 x 160 (res4: 8 x 10 cells, 1200 anchors each: PRE_NMS_TOPK_TEST 6000 takes the wide select with the level
taken whole), POST_NMS_TOPK_TEST 100.

Cases: the three dtypes and both stride layouts on full lists (NMS at 0.7 keeps more than 100 of each image's 1200 anchors); the same with
RPN.NMS_THRESH 0.2, which leaves about 60 and 80 proposals, so that every per-image list ends in padding rows -- the convolutions' row
segments (49 and 196 rows per RoI), the unfilled padding rows of the pooler and the zero rows of the mean are all in play; and
POOLER_RESOLUTION 7, the full pool + subsample path with res5 on 4 x 4.

box_feats bounds, every RoI of both images. fp32: 1e-4 of max|ref| (the project's fp32 contract) against the fp32 CPU chain. fp16 / bf16:
the float64 chain of res5 + mean from the engine's pooled rows and stored weights, and the same chain with every layer's output rounded
to the storage dtype; the device may be 3 x as far from the float64 chain as the rounded chain is (the margin is for accumulation
order). Measured on an MI355X (rounded chain - float64 chain / device - float64 chain):
    fp16, STRIDE_IN_1X1 True    2.63e-4 / 2.38e-4     partial lists 2.63e-4 / 2.84e-4     POOLER_RESOLUTION 7  4.10e-4 / 4.41e-4
    fp16, STRIDE_IN_1X1 False   3.95e-4 / 3.65e-4     partial lists 4.51e-4 / 4.41e-4     P 7, partial lists   3.78e-4 / 3.86e-4
    bf16, STRIDE_IN_1X1 True    2.02e-3 / 2.11e-3     fp32: 7.2e-7 .. 8.3e-7 from the fp32 chain at max|ref| 1.69
(DESIGN.md 7 item 19 records the same.)"""
import functools
import json

import pytest
import torch

from oracle import osr_oracle as O
from tests import c4_common as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POST = 100
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
N = len(C.IMAGE_SIZES)


@pytest.fixture(scope="module", autouse=True)
def _package(osr):
    """The product package is importable once the session fixture has loaded it."""
    osr._lib.load()


@functools.lru_cache(maxsize=None)
def params():
    return C.make_c4_params(0)


@functools.lru_cache(maxsize=None)
def run(dtype_name, s1x1=True, score_thresh=0.05, nms=0.7, pooler=14):
    """One engine pass with `keep` -> (outputs on the CPU, keep, the engine)."""
    from openset_rcnn_amd.host.engine_c4 import C4RCNNEngine
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    eng = C4RCNNEngine(params(), dict(post_nms_topk_test=POST, stride_in_1x1=s1x1, score_thresh_test=score_thresh, rpn_nms_thresh=nms, pooler_resolution=pooler),
                       DTYPES[dtype_name], DEV)
    keep = {}
    res = eng.forward(C.stacked(C.images()).to(DEV), C.IMAGE_SIZES, keep=keep)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in res), keep, eng


def _nchw(t):
    return t.detach().cpu().float().permute(0, 3, 1, 2).contiguous()


def _quantised(p, dtype):
    """The parameters as the engine stores them: convolution weights in the storage dtype, biases and the fp32 heads as they are."""
    return {k: (v.to(dtype).float() if v.dim() == 4 and not k.startswith("proposal_generator.rpn_head.o") and not k.startswith("proposal_generator.rpn_head.a")
                else v) for k, v in p.items()}


# (dtype, STRIDE_IN_1X1, RPN.NMS_THRESH, POOLER_RESOLUTION)
CASES = [("f16", True, 0.7, 14), ("bf16", True, 0.7, 14), ("f32", True, 0.7, 14), ("f16", False, 0.7, 14), ("f32", False, 0.7, 14),
         ("f16", True, 0.2, 14), ("f16", False, 0.2, 14), ("f32", True, 0.2, 14), ("f16", True, 0.7, 7), ("f16", False, 0.2, 7)]


@pytest.mark.parametrize("dtype_name,s1x1,nms,P", CASES, ids=[f"{d}-{'1x1' if s else '3x3'}-nms{t}-p{r}" for d, s, t, r in CASES])
def test_stage_by_stage(dtype_name, s1x1, nms, P):
    dtype = DTYPES[dtype_name]
    res, keep, eng = run(dtype_name, s1x1, 0.05, nms, P)
    o = (P + 1) // 2  # res5's output side
    p = _quantised(params(), dtype)
    tol = 1e-4 if dtype == torch.float32 else 5e-3
    res4 = _nchw(keep["feats"]["res4"])
    assert tuple(res4.shape) == (N, 1024, 8, 10) and keep["rpn_shapes"] == [(8, 10)]
    # ---- StandardRPNHead on the engine's res4 ----
    lg_ref, dl_ref = C.rpn_head(res4, p)
    lg, dl = keep["rpn_logits"].cpu().view(N, -1), keep["rpn_deltas"].cpu().view(N, -1, 4)
    assert lg.shape[1] == 8 * 10 * C.A
    assert float((lg - lg_ref).abs().max()) < tol * max(1.0, float(lg_ref.abs().max()))
    assert float((dl - dl_ref).abs().max()) < tol * max(1.0, float(dl_ref.abs().max()))
    # ---- selection (the wide select: k = 6000 > 2048) + NMS + post-NMS top-k on the engine's logits / deltas: same boxes, same order ----
    assert eng.cfg["pre_nms_topk_test"] == 6000 and keep["rpn_pre"]["cap"] == 1200
    ref_props = C.proposals(lg, dl, (8, 10), C.IMAGE_SIZES, 6000, POST, nms)
    sel = keep["sel"]
    counts = [int(c) for c in sel["counts"].cpu()]
    for i, (rb, rs, _) in enumerate(ref_props):
        assert counts[i] == len(rb) and 0 < counts[i] <= POST, (counts[i], len(rb))
        assert torch.equal(sel["scores"][i, :counts[i]].cpu(), rs)
        assert torch.allclose(sel["boxes"][i, :counts[i]].cpu(), rb, rtol=1e-5, atol=1e-4)  # expf on the device vs libm: last-ulp differences
    assert int(sel["status_flags"].cpu()[0]) == 0
    if nms < 0.7:  # every list ends in padding rows
        assert all(c < POST - 10 for c in counts), counts
        assert bool((sel["batch_idx"].cpu().view(N, POST)[0, counts[0]:] == -1).all())
    else:
        assert counts == [POST] * N
    # ---- the pooler on the engine's res4 and proposals: the even bins of the full 14 x 14 grid (STRIDE_IN_1X1), or all of it ----
    boxes = [sel["boxes"][i, :counts[i]].cpu() for i in range(N)]
    full = C.pooled_full(res4, boxes, P)                                         # (M, 1024, P, P) fp32
    want = (full[:, :, ::2, ::2] if s1x1 else full).permute(0, 2, 3, 1)
    pooled = keep["pooled"].cpu().float().view(N, POST, *keep["pooled"].shape[1:])
    assert tuple(pooled.shape[2:]) == ((o, o, 1024) if s1x1 else (P, P, 1024))
    assert all(bool((pooled[i, counts[i]:] == 0).all()) for i in range(N))  # (`keep` asks for the padding rows zero-filled)
    got = torch.cat([pooled[i, :counts[i]] for i in range(N)])
    # one rounding to the storage dtype (half an ulp) on top of fp32 sums of a few taps in another order
    bound = (C.storage_eps(dtype) + 1e-5) * float(want.abs().max())
    assert float((got - want).abs().max()) <= bound, (float((got - want).abs().max()), bound)
    # ---- res5 + mean on the engine's pooled rows ----
    x = got.permute(0, 3, 1, 2).contiguous()
    chain = (lambda t, q=(lambda v: v): C.res5_on_even_bins(t, p, q)) if s1x1 else (lambda t, q=(lambda v: v): C.res5(t, p, False, q))
    ref32 = chain(x).mean(dim=(2, 3))
    bf = keep["box_feats"].cpu().view(N, POST, -1)
    bf = torch.cat([bf[i, :counts[i]] for i in range(N)])
    assert tuple(keep["res5_out"].shape) == (N * POST, o, o, 2048) and bf.dtype == torch.float32
    err32 = float((bf - ref32).abs().max())
    scale = float(ref32.abs().max())
    print(f"\n[C4 {dtype_name} stride_in_1x1={s1x1} nms {nms} P {P}] box_feats: max|ref| {scale:.4f}, device - fp32 chain {err32:.3e}")
    if dtype == torch.float32:
        assert err32 <= 1e-4 * scale
    else:
        q = lambda t: t.to(dtype).double()  # noqa: E731
        x64 = x.double()
        ref64 = chain(x64).mean(dim=(2, 3))
        rounded = chain(x64, q).mean(dim=(2, 3))
        e_chain = float((rounded - ref64).abs().max())
        e_dev = float((bf.double() - ref64).abs().max())
        print(f"[C4 {dtype_name} stride_in_1x1={s1x1} nms {nms} P {P}] box_feats on {len(bf)} RoIs: rounded chain - float64 chain {e_chain:.3e}, "
              f"device - float64 chain {e_dev:.3e}")
        assert e_dev <= 3 * e_chain
    # the RoIs that do not exist come out as zeros
    bf_all = keep["box_feats"].cpu().view(N, POST, -1)
    assert all(bool((bf_all[i, counts[i]:] == 0).all()) for i in range(N))
    # ---- the predictor on the engine's box features, then [d2] fast_rcnn_inference on its outputs ----
    logits_ref, deltas_ref = C.predictor(bf, p)
    logits = torch.cat([keep["logits"].cpu().view(N, POST, -1)[i, :counts[i]] for i in range(N)])
    deltas = torch.cat([keep["deltas"].cpu().view(N, POST, -1)[i, :counts[i]] for i in range(N)])
    assert float((logits - logits_ref).abs().max()) < 1e-4 * max(1.0, float(logits_ref.abs().max()))
    assert float((deltas - deltas_ref).abs().max()) < 1e-4 * max(1.0, float(deltas_ref.abs().max()))
    off = 0
    for i in range(N):
        rb, rs, rc, _ = O.fast_rcnn_inference_from_outputs(logits[off:off + counts[i]], deltas[off:off + counts[i]], boxes[i], C.IMAGE_SIZES[i])
        off += counts[i]
        m = int(res[3][i])
        assert m == len(rb) and m > 0
        # the same detections with the same scores; two detections whose scores agree to the comparison's tolerance may come in either order
        gb, gs, gc = res[0][i, :m], res[1][i, :m], res[2][i, :m]
        assert torch.allclose(gs, rs, atol=1e-6)
        used = torch.zeros(m, dtype=torch.bool)
        for j in range(m):
            ok = (gc == rc[j]) & ((gs - rs[j]).abs() <= 1e-6 + 1e-5 * rs[j].abs()) & ((gb - rb[j]).abs().amax(dim=1) <= 1e-4 + 1e-5 * rb[j].abs().max()) & ~used
            assert bool(ok.any()), (i, j, int(rc[j]), float(rs[j]))
            k = int(torch.nonzero(ok)[0])
            assert abs(k - j) <= 2, (j, k)  # (only neighbours in the sorted list can swap)
            used[k] = True


def test_strided_pool_and_full_pool_give_one_tensor():
    """The engine's two ways to the input of res5.0: the even bins pooled directly, or the full grid subsampled. Same bits, same result."""
    from openset_rcnn_amd.host import ops
    res, keep, eng = run("f16", True)
    sel, feats = keep["sel"], keep["feats"]
    a, sa = eng.pool_res5_rois(feats, sel["boxes"].view(-1, 4), sel["batch_idx"])
    eng.STRIDED_POOL = False
    try:
        b, sb = eng.pool_res5_rois(feats, sel["boxes"].view(-1, 4), sel["batch_idx"])
        again = eng.forward(C.stacked(C.images()).to(DEV), C.IMAGE_SIZES)
    finally:
        del eng.STRIDED_POOL
    assert sa == sb == 1 and torch.equal(a, b) and torch.equal(a, keep["pooled"])
    assert all(torch.equal(x.cpu(), y) for x, y in zip(again, res))
    assert ops.RPN_SELECT_MAXK == 2048 and ops.RPN_SELECT_WIDE_MAXK == 8192


@pytest.mark.parametrize("s1x1", [True, False], ids=["1x1", "3x3"])
def test_fp32_engine_against_the_whole_fp32_reference(s1x1):
    res, _, _ = run("f32", s1x1)
    ref = C.detect(C.images(), params(), s1x1, post=POST)
    matched = total = 0
    for i in range(N):
        m = int(res[3][i])
        gb, gs, gc = res[0][i, :m], res[1][i, :m], res[2][i, :m]
        rb, rs, rc, _ = ref[i]
        iou = O.pairwise_iou(rb, gb)
        used = torch.zeros(m, dtype=torch.bool)
        for j in range(len(rb)):
            ok = (iou[j] >= 0.99) & ((gs - rs[j]).abs() <= 1e-2) & (gc == rc[j]) & ~used
            if bool(ok.any()):
                used[int(torch.nonzero(ok)[0])] = True
                matched += 1
        total += max(m, len(rb))
    print(f"\n[C4 parity mode, stride_in_1x1={s1x1}] {matched}/{total} detections agree with the fp32 reference")
    assert total > 0 and matched >= 0.95 * total


@pytest.mark.parametrize("s1x1,nms", [(True, 0.7), (True, 0.2), (False, 0.2)], ids=["full-lists", "partial-lists", "partial-lists-3x3"])
def test_a_pass_without_keep_repeats_the_pass_with_it(s1x1, nms):
    """Without `keep` the pooler leaves the padding rows of the lists unwritten (whatever the buffer held): nothing downstream may
    read them, so the outputs are the bits of the pass that zero-filled them, twice over."""
    res, _, eng = run("f16", s1x1, 0.05, nms, 14)
    for _ in range(2):
        again = eng.forward(C.stacked(C.images()).to(DEV), C.IMAGE_SIZES)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(again, res))


def test_no_proposal_above_the_score_threshold():
    res, keep, _ = run("f16", True, 1.0)  # (no softmax probability exceeds 1)
    assert res[3].tolist() == [0, 0] and int(keep["cands"]["count"].sum()) == 0
    assert bool((res[0] == 0).all()) and bool((res[1] == 0).all())
    assert tuple(res[0].shape) == (N, 100, 4)


def test_split_convolutions_are_refused():
    from openset_rcnn_amd.host.engine_c4 import C4RCNNEngine
    with pytest.raises(ValueError, match="conv"):
        C4RCNNEngine(params(), None, torch.float32, DEV, conv="split")


def _model():
    """The model mirror from the shipped yaml (POST_NMS_TOPK_TEST 100) with the test's parameters, on the device, in eval mode."""
    import os
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(root, "configs", "faster_rcnn_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.RPN.POST_NMS_TOPK_TEST", str(POST)])
    model = M.build_model(cfg).to(DEV)
    C.load_folded(model, params())
    return model.eval(), cfg


def test_stage_level_modules_chain_to_the_models_detections():
    """backbone -> proposal generator -> RoI heads through the mirrored signatures (logical NCHW features, Instances in and out) give
    the detections of model.inference."""
    model, _ = _model()
    imgs = C.images()
    il = model.preprocess_image([{"image": im} for im in imgs])
    feats = model.backbone(il.tensor)
    assert list(feats) == ["res4"] and tuple(feats["res4"].shape) == (N, 1024, 8, 10)
    lg, dl = model.proposal_generator.rpn_head([feats["res4"]])
    assert tuple(lg[0].shape) == (N, C.A, 8, 10) and tuple(dl[0].shape) == (N, 4 * C.A, 8, 10)
    props, losses = model.proposal_generator(il, feats)
    assert losses == {} and all(0 < len(p) <= POST and p.has("proposal_boxes") and p.has("objectness_logits") for p in props)
    dets, losses = model.roi_heads(il, feats, props)
    assert losses == {}
    whole = model.inference([{"image": im} for im in imgs], do_postprocess=False)
    for dd, o in zip(dets, whole):
        w = o["instances"]
        assert len(dd) == len(w) > 0
        for j in range(len(dd)):  # the same detections (a near-tie may sort either way between the two routes)
            ok = (w.pred_classes == dd.pred_classes[j]) & ((w.scores - dd.scores[j]).abs() < 1e-3) & \
                ((w.pred_boxes.tensor - dd.pred_boxes.tensor[j]).abs().amax(dim=1) < 0.5)
            assert bool(ok.any()), j


def test_model_instances_through_detector_postprocess_and_the_coco_evaluator(osr, tmp_path):
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    from openset_rcnn_amd.host.structures import Instances
    from tests.coco_eval_common import coco_json
    model, cfg = _model()
    imgs = C.images()
    # each image is asked back at twice its size: detector_postprocess rescales the boxes
    inputs = [dict(image=im, height=2 * im.shape[1], width=2 * im.shape[2], image_id=7 + i) for i, im in enumerate(imgs)]
    out = model(inputs)
    res, _, _ = run("f16", True)
    assert len(out) == N
    for i, o in enumerate(out):
        inst = o["instances"]
        assert isinstance(inst, Instances) and tuple(inst.image_size) == (2 * C.IMAGE_SIZES[i][0], 2 * C.IMAGE_SIZES[i][1])
        m = int(res[3][i])
        assert 0 < len(inst) <= m  # (the postprocess drops boxes that are empty after the clip)
        if len(inst) == m:
            assert torch.allclose(inst.pred_boxes.tensor.cpu(), 2 * res[0][i, :m], atol=1e-3)
            assert torch.equal(inst.scores.cpu(), res[1][i, :m]) and torch.equal(inst.pred_classes.cpu(), res[2][i, :m])
    # ---- the COCO evaluator on the model's outputs (the path run_net.py --eval-only takes: D.get_evaluator on a registered COCO dataset) ----
    anns = []
    for i, o in enumerate(out):
        inst = o["instances"]
        for j in range(0, len(inst), 3):  # every third detection is a ground truth: AP is well above zero
            x1, y1, x2, y2 = inst.pred_boxes.tensor[j].cpu().tolist()
            anns.append(dict(image_id=7 + i, category_id=int(inst.pred_classes[j]) + 1, bbox=[x1, y1, x2 - x1, y2 - y1], area=(x2 - x1) * (y2 - y1), iscrowd=0))
    gt = coco_json([7, 8], list(range(1, 81)), anns)
    path = str(tmp_path / "c4_toy.json")
    with open(path, "w") as f:
        json.dump(gt, f)
    name = f"c4_toy_{tmp_path.name}"
    D.register_coco_instances(name, {}, path, str(tmp_path))
    ev = D.get_evaluator(cfg, name, None)
    assert isinstance(ev, COCOEvaluator) and ev.tasks == ("bbox",)
    ev.process([dict(image_id=x["image_id"]) for x in inputs], out)
    got = ev.evaluate()
    cpu = COCOEvaluator(name, output_dir=None)
    cpu.process([dict(image_id=x["image_id"]) for x in inputs], [dict(instances=o["instances"].to("cpu")) for o in out])
    want = cpu.evaluate()
    assert list(got) == ["bbox"] and got["bbox"]["AP"] > 10.0
    assert json.dumps(got) == json.dumps(want)
