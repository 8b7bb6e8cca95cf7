"""OpensetRCNNEngine(box_head="split"): the reference's fp32 arithmetic from the RoIAlign output on, FC1 / FC2 on the split-precision
kernel (ops.linear_split). On the four seeded 256 x 384 images and the weights of tests/test_e2e_parity.py (built here the same way):
the dense stages against float64, the mode against the fp32-kernel configuration it replaces (fp32_points=("pooled", "h1"): same
fp16 backbone, so the two differ only in how FC1 / FC2 multiply), the captured and multi-stream schedules, one image at the
benchmark's resolution, and the switch on the detectron2-shaped model."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, H, W = 4, 256, 384
A_BOUND = 1e-4


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _real_rows(t, counts, cap):
    v = t.reshape(len(counts), cap, -1)
    return torch.cat([v[i, :counts[i]] for i in range(len(counts))]).cpu()


def _dets(eng, out, n):
    return [(d["pred_boxes"], d["scores"], d["pred_classes"]) for d in eng.to_instances(out, n)]


@pytest.fixture(scope="module")
def world(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import random_params, with_known_unknown_mix
    g = torch.Generator().manual_seed(2024)
    images = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8)
    sizes = [(H, W), (H, W), (H - 16, W - 40), (H - 6, W)]
    base = random_params(0)
    keep = {}
    eng = OpensetRCNNEngine(base, dtype=torch.float32, device=DEV)
    eng.forward(images.to(DEV), sizes, keep=keep)
    cnt = keep["cnt1"].cpu()
    emb = torch.cat([keep["emb"].view(N, 1000, -1)[i, :int(cnt[i])] for i in range(N)])
    params = with_known_unknown_mix(base, emb)
    del eng, keep
    osr.ops.LINEAR_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    split = OpensetRCNNEngine(params, dtype=torch.float16, device=DEV, box_head="split")
    ks = {}
    split.profile = []
    out = split.forward(images.to(DEV), sizes, keep=ks)
    torch.cuda.synchronize()
    names = [e[0] for e in split.profile]
    split.profile = None
    launches = osr.ops.LINEAR_SPLIT_COUNT["launches"]
    osr.ops.LINEAR_SPLIT_COUNT = None
    return dict(images=images, sizes=sizes, params=params, Engine=OpensetRCNNEngine, split=split, keep=ks, out=out, names=names, launches=launches)


def test_both_fc_layers_ran_on_the_split_kernel(world):
    assert world["split"].box_head == "split"
    assert world["launches"] == 2  # FC1 and FC2, nothing else
    fc = [n for n in world["names"] if n.startswith("roi_heads.box_head.fc")]
    assert fc == ["roi_heads.box_head.fc1 (split)", "roi_heads.box_head.fc2 (split)"], fc


def test_dense_stages_meet_a_on_the_engines_own_rows(world):
    """h1 and box_feats against relu(linear) in float64 with the fp32 weights, on the engine's own fp32 pooled rows / h1."""
    from openset_rcnn_amd.host.weights import pack_fc1_weight
    keep, p = world["keep"], world["params"]
    sel = keep["sel"]
    cap, counts = sel["cap"], [int(c) for c in sel["counts"].cpu()]
    assert keep["pooled"].dtype == torch.float32 and keep["h1"].dtype == torch.float32 and keep["box_feats"].dtype == torch.float32
    x = _real_rows(keep["pooled"], counts, cap)  # (rows, 7*7*256) in the (ph, pw, c) order FC1's packed weight has
    w1 = pack_fc1_weight(p["roi_heads.box_head.fc1.weight"], 256, 7, torch.float32)
    h1 = F.relu(F.linear(x.double(), w1.double(), p["roi_heads.box_head.fc1.bias"].double()))
    h1e = _real_rows(keep["h1"], counts, cap)
    bf = F.relu(F.linear(h1e.double(), p["roi_heads.box_head.fc2.weight"].double(), p["roi_heads.box_head.fc2.bias"].double()))
    bfe = _real_rows(keep["box_feats"], counts, cap)
    e1, e2 = rel(h1e, h1), rel(bfe, bf)
    print(f"\n[box_head split, 256x384 x 4, {sum(counts)} real rows] e(h1) {e1:.3e}  e(box_feats) {e2:.3e}")
    assert e1 <= A_BOUND and e2 <= A_BOUND


def test_against_the_fp32_kernel_configuration(world):
    from openset_rcnn_amd.host.agreement import detection_agreement
    c5 = world["Engine"](world["params"], dtype=torch.float16, device=DEV, fp32_points=("pooled", "h1"))
    k5 = {}
    out5 = c5.forward(world["images"].to(DEV), world["sizes"], keep=k5)
    torch.cuda.synchronize()
    keep = world["keep"]
    assert torch.equal(keep["pooled"], k5["pooled"])
    sel = keep["sel"]
    cap, counts = sel["cap"], [int(c) for c in sel["counts"].cpu()]
    a, b = _real_rows(keep["box_feats"], counts, cap), _real_rows(k5["box_feats"], counts, cap)
    d = float((a - b).abs().max() / b.abs().max())
    ag = detection_agreement(_dets(world["split"], world["out"], N), _dets(c5, out5, N))
    print(f"\n[box_head split vs fp32_points=(pooled, h1)] box_feats differ by {d:.3e} of their maximum; detection agreement "
          f"{ag['matched']}/{max(ag['reference_detections'], ag['returned_detections'])} = {ag['fraction']:.4f}")
    assert d <= 2e-4
    assert ag["fraction"] >= 0.95, ag


def test_captured_and_multi_stream_schedules_match_forward(world):
    eng = world["split"]
    imgs = world["images"].to(DEV)
    hw = torch.tensor(world["sizes"], dtype=torch.int32, device=DEV)
    plain = [t.clone() for t in eng.forward_device(imgs, hw, H, W)]
    lanes = eng.forward_device_streams(imgs, hw, H, W, nstreams=4)
    torch.cuda.synchronize()
    for x, y in zip(plain, lanes):
        assert torch.equal(x, y)
    graph, gout = eng.capture(imgs, hw, H, W, nstreams=2)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(plain, gout):
        assert torch.equal(x, y)


def test_one_image_at_benchmark_resolution(osr, world):
    g = torch.Generator().manual_seed(77)
    image = torch.randint(0, 256, (1, 3, 800, 1333), generator=g, dtype=torch.uint8)
    eng = world["split"]
    keep = {}
    osr.ops.LINEAR_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    eng.forward(image.to(DEV), [(800, 1333)], keep=keep)
    torch.cuda.synchronize()
    launches = osr.ops.LINEAR_SPLIT_COUNT["launches"]
    osr.ops.LINEAR_SPLIT_COUNT = None
    assert launches == 2
    cnt = int(keep["sel"]["counts"][0])
    assert keep["sel"]["cap"] == 4273 and cnt > 512
    rows = torch.randperm(cnt, generator=g)[:512]
    p = world["params"]
    h1 = keep["h1"][rows.to(DEV)].cpu()
    bf = F.relu(F.linear(h1.double(), p["roi_heads.box_head.fc2.weight"].double(), p["roi_heads.box_head.fc2.bias"].double()))
    e = rel(keep["box_feats"][rows.to(DEV)], bf)
    print(f"\n[box_head split, 800x1333, {cnt} proposals] e(box_feats) on 512 sampled rows {e:.3e}")
    assert e <= A_BOUND


def test_model_attribute_selects_the_mode(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "voc_coco.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "OPENDET_BENCHMARK", "True"])
    model = M.build_model(cfg).to(DEV).eval()
    assert model.roi_heads.box_head_precision == "storage" and model.engine().box_head == "storage"
    model.roi_heads.box_head_precision = "split"
    eng = model.engine()
    assert eng.box_head == "split" and hasattr(eng, "fc1_split") and eng.fc1_split[0].dtype == torch.bfloat16
    assert model.roi_heads.engine() is eng  # the children share the model's engine
