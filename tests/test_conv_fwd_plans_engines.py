"""osr_conv2d_fwd at the launch plans of the engines that came after tests/test_conv_fwd_plans.py's table: the stock heads with the mask
branch (StandardRCNNEngine), the cascade, the deformable stages and RetinaNet. The helpers, the fp64 restatement and the two runs are
that file's, imported; what is new here is listed below.

Tables: `engine_tables(kind, n, H, W, streams, stride_in_1x1)` lists every single-layer ops.conv2d / ops.linear launch of one
forward_device pass with the fused forms off; the trunk comes from forward_table, the rest is what differs -- the stock RPN's hidden state
(3x3, ReLU, fp32, written through out= into row slices of one level-major buffer), FC1 / FC2 without row_seg (three pairs in the cascade),
the mask head's four 3x3 layers on (n * 100, 14, 14, 256), conv2_offset (3x3, 18 / 27 channels packed to 24 / 32, fp32, conv2's stride)
and the dense contraction over (1, m, 1, 9c) of a deformable block, RetinaNet's p6 (3x3 / 2 on res5, no ReLU) and p7, its towers per
level, cls_score (720, 16-bit) and bbox_pred (36 packed to 40, fp32) into out= slices. test_tables_are_the_engines_forward records one
real pass per (kind, geometry) -- the only production-size work of this file. The deformable configuration runs unmodulated and
modulated in both stride layouts: no combination is refused.

ENGINE_CASES: a reduced case for every plan key of these tables that CASES does not have (NEW_KEYS, 13 of them), with the partial-N
companions of the old rule, and, whatever their key, the production couts 720, 40, 24 and 32 on their own layers, many small images
(14 x 14 with n the smallest that keeps the tile of n = 1600 and of n = 200) and inputs smaller than the filter (1 x 1, 2 x 3, 1 x 2 under
3x3 / 2; 1 x 1 under 3x3 / 1 with couts 720 and 40). The latter cannot reach 2 BM rows at the layer's own n: TINY relaxes that one
assertion for them and n is raised until at least one M tile is full. Every case gets the integer run and the float run of the other
file in fp16 and bf16; the fp32-output case of every tile that has one also runs with weights x 64 (fp32 does not overflow: finite and
exact).

out= slices: the per-level loop of the engines over a five-level pyramid into one buffer with 64 sentinel rows on either side; every level
exact, every guard row untouched, the reverse order gives the same buffer.

Teeth (no GPU): on the inputs of the small-image, tiny-input and stride-2 cases, four wrong restatements -- padding that contributes
relu(bias), stride-2 taps from origin 2 o, image boundaries ignored, a ReLU that the flag does not ask for -- each differ from the right
one, so the exact runs would see a kernel that made the same mistake. These tests carry no gpu mark; every other test of the file does."""
import functools
import os
import zlib

import pytest
import torch

from tests.test_conv_fwd_plans import (BF16, BU, CASES, DEV, F16, F32, GEOMS, L, SENTINEL, _assert_same, _cid, _exact, _half_ulp, _inputs, _run,
                                       _saw_big_odd, _short, describe, expect, forward_table, ops, out_hw, plan_key, record_pass,
                                       stage_hw, tile_of)  # noqa: F401 (ops: a fixture)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POST_NMS_TOPK, DETECTIONS = 1000, 100  # MODEL.RPN.POST_NMS_TOPK_TEST of base_rcnn_fpn.yaml, TEST.DETECTIONS_PER_IMAGE
RPN_CONV, TOP_BLOCK, HEAD, MASK = "proposal_generator.rpn_head.conv", "backbone.top_block", "head", "roi_heads.mask_head.mask_fcn"
ENGINE_GEOMS = dict(GEOMS, b2_64x64=(2, 64, 64, 1))  # (RetinaNet: res5 is 2 x 2, p6 and p7 are 1 x 1)
# kind -> (yaml, options, geometries); the deformable trunk: DEFORM_MODULATED x STRIDE_IN_1X1
KINDS = {"std_mask": ("base_rcnn_fpn.yaml", ("MODEL.MASK_ON", "True"), ("b16_800x1344", "mb4of16_800x1344_4streams", "b2_256x352")),
         "cascade": ("cascade_rcnn_fpn.yaml", (), ("b16_800x1344", "b2_256x352")),
         "dconv": ("mask_rcnn_dconv_c3_c5.yaml", (), ("b16_800x1344", "b2_256x352")),
         "retinanet": ("retinanet_fpn.yaml", (), ("b16_800x1344", "b2_256x352", "b2_64x64"))}
# (kind, stride_in_1x1, modulated): the engines
VARIANTS = [("std_mask", True, False), ("cascade", True, False), ("retinanet", True, False)] + \
           [("dconv", layout, mod) for layout in (True, False) for mod in (False, True)]


def engine_tables(kind, n, H, W, streams=1, stride_in_1x1=True, modulated=False, dt=F16):
    """Every single-layer ops.conv2d / ops.linear launch of one forward_device pass of the kind's engine over n images padded to H x W
    under ops.concurrent_streams(streams), fuse_res2 = chain_res3 = fuse_levels = False, in the engine's order."""
    hw = stage_hw(H, W)
    base = forward_table(n, H, W, streams, stride_in_1x1, dt)
    trunk = [e for e in base if e[0].startswith(BU)]
    fpn = {e[0]: e for e in base if e[0].startswith("backbone.fpn_")}

    def c(name, x, w, stride=1, pad=0, relu=False, out=dt):
        return L(name, x, w, stride, pad, relu, 0, out, None, streams)
    T = []
    for e in trunk:
        if kind == "dconv" and e[0].endswith(".conv2") and not e[0].startswith(BU + "res2"):
            # DeformBottleneckBlock: conv2_offset in fp32 at conv2's stride, the gather (a kernel of its own), the dense contraction
            pre, mid = e[0][:-len(".conv2")], e[1][3]
            ho, wo = out_hw(e)
            T += [c(pre + ".conv2_offset", e[1], (32 if modulated else 24, 3, 3, mid), e[3], 1, False, F32),
                  c(pre + ".conv2 (deform contraction)", (1, n * ho * wo, 1, 9 * mid), (mid, 1, 1, 9 * mid), 1, 0, True)]
        else:
            T.append(e)
    if kind == "retinanet":
        T += [fpn[f"backbone.fpn_lateral{l}"] for l in (5, 4, 3)] + [fpn[f"backbone.fpn_output{l}"] for l in (3, 4, 5)]
        h7 = ((hw[6][0] - 1) // 2 + 1, (hw[6][1] - 1) // 2 + 1)
        T += [c(TOP_BLOCK + ".p6", (n,) + hw[5] + (2048,), (256, 3, 3, 2048), 2, 1), c(TOP_BLOCK + ".p7", (n,) + hw[6] + (256,), (256, 3, 3, 256), 2, 1)]
        levels = [hw[3], hw[4], hw[5], hw[6], h7]
        for sub in ("cls_subnet", "bbox_subnet"):
            for i in range(4):
                T += [c(f"{HEAD}.{sub}.{2 * i}", (n,) + s + (256,), (256, 3, 3, 256), 1, 1, True) for s in levels]
        for s in levels:
            T += [c(HEAD + ".cls_score", (n,) + s + (256,), (720, 3, 3, 256), 1, 1), c(HEAD + ".bbox_pred", (n,) + s + (256,), (40, 3, 3, 256), 1, 1, False, F32)]
        return T
    T += [fpn[f"backbone.fpn_lateral{l}"] for l in (5, 4, 3, 2)] + [fpn[f"backbone.fpn_output{l}"] for l in (2, 3, 4, 5)]
    T += [c(RPN_CONV, (n,) + hw[l] + (256,), (256, 3, 3, 256), 1, 1, True, F32) for l in (2, 3, 4, 5, 6)]
    m = n * POST_NMS_TOPK
    for s in (("0.", "1.", "2.") if kind == "cascade" else ("",)):
        T += [c(f"roi_heads.box_head.{s}fc1", (1, m, 1, 12544), (1024, 1, 1, 12544), 1, 0, True),
              c(f"roi_heads.box_head.{s}fc2", (1, m, 1, 1024), (1024, 1, 1, 1024), 1, 0, True, F32)]
    if kind in ("std_mask", "dconv"):
        T += [c(f"{MASK}{i + 1}", (n * DETECTIONS, 14, 14, 256), (256, 3, 3, 256), 1, 1, True) for i in range(4)]
    return T


def _vid(v):
    kind, layout, mod = v
    return kind + ("" if kind != "dconv" else f"-{'msra' if layout else 'tv'}-{'dcnv2' if mod else 'dcnv1'}")


def all_tables():
    """(variant id, geometry, table) of every engine and geometry."""
    for v in VARIANTS:
        kind, layout, mod = v
        for gname in KINDS[kind][2]:
            n, H, W, streams = ENGINE_GEOMS[gname]
            yield _vid(v), gname, engine_tables(kind, n, H, W, streams, layout, mod)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the tables against the engines
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _engine(variant):
    """The variant's engine as build_model makes it from the shipped yaml (the parameters as the modules initialise them: only the
    launches are looked at), the fused forms off. One at a time: the tests below ask variant by variant."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    kind, layout, mod = variant
    yaml, opts, _ = KINDS[kind]
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.RESNETS.STRIDE_IN_1X1", str(layout), "MODEL.RESNETS.DEFORM_MODULATED", str(mod)] + list(opts))
    torch.manual_seed(0)
    eng = M.build_model(cfg).eval().engine()
    eng.fuse_res2 = eng.chain_res3 = eng.fuse_levels = False
    return eng


@gpu
@pytest.mark.parametrize("vg", [(v, g) for v in VARIANTS for g in KINDS[v[0]][2]], ids=lambda vg: f"{_vid(vg[0])}-{vg[1]}")
def test_tables_are_the_engines_forward(ops, vg):
    variant, gname = vg
    kind, layout, mod = variant
    n, H, W, streams = ENGINE_GEOMS[gname]
    log = record_pass(ops, _engine(variant), n, H, W, streams)
    want = engine_tables(kind, n, H, W, streams, layout, mod)
    for i, ((got, via_linear), e) in enumerate(zip(log, want)):
        assert got == e[1:], f"{_vid(variant)} {gname}: launch {i} ({e[0]}): engine {got} != table {e[1:]}"
        assert via_linear == (e[0].endswith((".fc1", ".fc2"))), f"{_vid(variant)} {gname}: launch {i} ({e[0]}): ops.linear {via_linear}"
    assert len(log) == len(want), f"{_vid(variant)} {gname}: {len(log)} launches, table {len(want)}"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the cases
# ------------------------------------------------------------------------------------------------------------------------------
# (expected plan key, launch), reduced as CASES are: K and cout of the production layer, the smallest n x h x w of the old file's odd
# sizes that keeps the key (the 256-row tiles keep a reduced shape only under the 4-stream hint), rows and rows per image no multiple of
# BM, more than 2 BM rows, odd h and w under stride 2; cout 8 and 72 beside every new 64-wide key, 192 beside every new 128-wide one.
ENGINE_CASES = [
    # the stock RPN's hidden state: 3x3, ReLU, fp32 out
    (("256x256/2", True, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (3, 113, 387, 256), (256, 3, 3, 256), 1, 1, True, 0, F32, None, 4)),
    (("256x256/2", False, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (2, 113, 145, 256), (256, 3, 3, 256), 1, 1, True, 0, F32, None, 4)),
    (("128x128/1", False, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (2, 113, 145, 256), (256, 3, 3, 256), 1, 1, True, 0, F32, None, 1)),
    (("128x128/1", False, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (2, 97, 225, 256), (192, 3, 3, 256), 1, 1, True, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (2, 7, 19, 256), (256, 3, 3, 256), 1, 1, True, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (2, 7, 19, 256), (8, 3, 3, 256), 1, 1, True, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, True, False, "32", False), L("rpn_head.conv", (2, 7, 19, 256), (72, 3, 3, 256), 1, 1, True, 0, F32, None, 1)),
    # FC1 / FC2 without row_seg
    (("256x256/2", False, "1x1", 1, 0, True, True, "16", False), L("fc1", (1, 12301, 1, 12544), (1024, 1, 1, 12544), 1, 0, True, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", False), L("fc1", (1, 1357, 1, 12544), (1024, 1, 1, 12544), 1, 0, True, 0, F16, None, 1)),
    (("256x256/2", False, "1x1", 1, 0, True, True, "32", False), L("fc2", (1, 12301, 1, 1024), (1024, 1, 1, 1024), 1, 0, True, 0, F32, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "32", False), L("fc2", (1, 1357, 1, 1024), (1024, 1, 1, 1024), 1, 0, True, 0, F32, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "32", False), L("fc2", (1, 1357, 1, 1024), (8, 1, 1, 1024), 1, 0, True, 0, F32, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "32", False), L("fc2", (1, 1357, 1, 1024), (72, 1, 1, 1024), 1, 0, True, 0, F32, None, 1)),
    # the mask head: many small images. 251 is the smallest n on the tile of n = 1600 (256x256/2), 168 the smallest on that of n = 200
    (("256x256/2", False, "KxK", 1, 0, True, False, "16", False), L("mask_fcn1", (251, 14, 14, 256), (256, 3, 3, 256), 1, 1, True, 0, F16, None, 1)),
    (("128x128/1", False, "KxK", 1, 0, True, False, "16", False), L("mask_fcn1", (168, 14, 14, 256), (256, 3, 3, 256), 1, 1, True, 0, F16, None, 1)),
    # the deformable blocks: conv2_offset (24 / 32 channels, fp32) at stride 1 and 2, the dense contraction over 9 c
    (("128x64/2", False, "KxK", 1, 0, False, False, "32", False), L("res3.1.conv2_offset", (2, 7, 19, 128), (24, 3, 3, 128), 1, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "32", False), L("res3.1.conv2_offset", (2, 7, 19, 128), (32, 3, 3, 128), 1, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "32", False), L("res3.0.conv2_offset", (2, 19, 25, 128), (24, 3, 3, 128), 2, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "32", False), L("res5.0.conv2_offset", (2, 19, 25, 512), (32, 3, 3, 512), 2, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "32", False), L("res3.0.conv2_offset", (2, 19, 25, 128), (8, 3, 3, 128), 2, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "32", False), L("res3.0.conv2_offset", (2, 19, 25, 128), (72, 3, 3, 128), 2, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", False), L("res3.0.conv2 (deform contraction)", (1, 261, 1, 1152), (128, 1, 1, 1152), 1, 0, True, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", False), L("res5.0.conv2 (deform contraction)", (1, 261, 1, 4608), (512, 1, 1, 4608), 1, 0, True, 0, F16, None, 1)),
    # RetinaNet: p6 (K = 18432) and p7, 3x3 / 2 without ReLU; a tower layer; cls_score (720) and bbox_pred (40, fp32)
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p6", (2, 19, 25, 2048), (256, 3, 3, 2048), 2, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p6", (2, 19, 25, 2048), (8, 3, 3, 2048), 2, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p6", (2, 19, 25, 2048), (72, 3, 3, 2048), 2, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p7", (2, 19, 25, 256), (256, 3, 3, 256), 2, 1, False, 0, F16, None, 1)),
    (("256x256/2", True, "KxK", 1, 0, True, False, "16", False), L("head.cls_subnet.0", (3, 113, 387, 256), (256, 3, 3, 256), 1, 1, True, 0, F16, None, 4)),
    (("128x128/1", True, "KxK", 1, 0, False, False, "16", False), L("head.cls_score", (3, 149, 149, 256), (720, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x128/1", True, "KxK", 1, 0, False, False, "16", False), L("head.cls_score", (3, 247, 297, 256), (192, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("256x128/1", False, "KxK", 1, 0, False, False, "16", False), L("head.cls_score", (2, 55, 149, 256), (720, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("256x128/1", False, "KxK", 1, 0, False, False, "16", False), L("head.cls_score", (3, 113, 145, 256), (192, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "16", False), L("head.cls_score", (2, 7, 19, 256), (720, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "32", False), L("head.bbox_pred", (2, 7, 19, 256), (40, 3, 3, 256), 1, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "32", False), L("head.bbox_pred", (2, 7, 19, 256), (8, 3, 3, 256), 1, 1, False, 0, F32, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "32", False), L("head.bbox_pred", (2, 7, 19, 256), (72, 3, 3, 256), 1, 1, False, 0, F32, None, 1)),
]
# inputs smaller than the filter (p6 / p7 and the head on p6 / p7 of a small batch). One output pixel or two per image: 2 BM rows are out
# of reach at the layer's own n, so n is raised until one M tile is full and the last one ragged (131 or 2 x 67 rows on BM 128)
TINY = [
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p7", (131, 1, 1, 256), (256, 3, 3, 256), 2, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p7", (67, 2, 3, 256), (256, 3, 3, 256), 2, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, False, False, "16", False), L("top_block.p6", (131, 1, 2, 2048), (256, 3, 3, 2048), 2, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "16", False), L("head.cls_score", (131, 1, 1, 256), (720, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "32", False), L("head.bbox_pred", (131, 1, 1, 256), (40, 3, 3, 256), 1, 1, False, 0, F32, None, 1)),
]
ENGINE_CASES += TINY
OLD_KEYS = {k for k, _ in CASES}
NEW_KEYS = sorted({k for k, _ in ENGINE_CASES} - OLD_KEYS)  # the plan keys that no case had before this file


def _rows(e):
    ho, wo = out_hw(e)
    return e[1][0] * ho * wo


@gpu
def test_plans_reached(osr):
    have = {}
    for key, e in CASES:
        have.setdefault(key, []).append(e)
    for case in ENGINE_CASES:
        key, e = case
        got = plan_key(osr, e)
        assert got == key, f"case {_cid(case)}: osr_conv2d_fwd_describe gives {got} ({describe(osr, e)}), the case says {key}"
        bm, m = tile_of(key)[0], _rows(e)
        assert m % bm != 0 and m > (bm if case in TINY else 2 * bm), f"case {_cid(case)}: {m} rows on BM {bm}"
        have.setdefault(key, []).append(e)
    missing, own = [], {}
    for vid, gname, table in all_tables():
        keys = {}
        for e in table:
            k = plan_key(osr, e)
            keys.setdefault(k, []).append(f"{_short(e[0])} [{describe(osr, e)}]")
            if e[2][0] in (720, 40, 24, 32):
                own.setdefault(e[2][0], set()).add(k)
        print(f"[plan] {vid}, {gname}: {len(keys)} keys")
        for k, layers in keys.items():
            print(f"[plan]   {'* ' if k not in OLD_KEYS else '  '}{k} <- {'; '.join(layers)}")
            if k not in have:
                missing.append((vid, gname, k, layers[0]))
    assert not missing, "plan keys of the engines' forward passes that no case has:\n" + "\n".join(map(str, missing))
    print(f"[plan] {len(NEW_KEYS)} keys that no case of tests/test_conv_fwd_plans.py has")
    # partial last N tiles beside every new key, by the old rule
    for key in NEW_KEYS:
        couts = {e[2][0] for e in have[key]}
        bn = tile_of(key)[1]
        if bn == 64:
            assert {8, 72} <= couts, (key, couts)
        elif bn == 128 and key[0] != "128x128/2":
            assert 192 in couts, (key, couts)
    # the production widths with a partial last N tile, each on a key its own layer takes
    assert set(own) == {720, 40, 24, 32}
    for cout, keys in own.items():
        assert any(k in keys and e[2][0] == cout for k, e in ENGINE_CASES), f"no case has cout {cout} on one of {keys}"


def test_small_image_cases_are_the_smallest_on_their_tile(osr):
    """(n, 14, 14, 256): 251 and 168 are the smallest n on the tiles of the production n = 1600 and n = 200 (describe needs no GPU)."""
    def tile(n):
        return describe(osr, L("mask_fcn1", (n, 14, 14, 256), (256, 3, 3, 256), 1, 1, True, 0, F16, None, 1)).split(" ")[0]
    for small, full in ((251, 1600), (168, 200)):
        assert tile(small) == tile(full) and all(tile(n) != tile(full) for n in range(1, small)), (small, full)
        assert (small * 196) % int(tile(full).split("x")[0]) != 0


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the two runs of tests/test_conv_fwd_plans.py on every case
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ENGINE_CASES, ids=_cid)
def test_exact(osr, ops, case, dt):
    key, e = case
    ref64 = _exact(ops, osr, key, e, dt, 1000 + zlib.crc32(_cid(case).encode()) % 1000)
    if case not in TINY:  # (at most four taps of a tiny input are inside it: K does not allow results past 2048)
        _saw_big_odd(ref64, F32 if e[7] == F32 else dt, e[2][1] * e[2][2] * e[2][3])


def _one_fp32_per_tile():
    """The first fp32-output case of every tile that has one (K >= 512)."""
    seen, out = set(), []
    for key, e in ENGINE_CASES:
        if key[0] not in seen and e[7] == F32 and e[2][1] * e[2][2] * e[2][3] >= 512:
            seen.add(key[0])
            out.append((key, e))
    return out


def test_one_fp32_case_per_tile():
    assert {k[0] for k, _ in _one_fp32_per_tile()} == {k[0] for k, e in ENGINE_CASES if e[7] == F32} == {"256x256/2", "128x128/1", "128x64/2"}


@gpu
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", _one_fp32_per_tile(), ids=_cid)
def test_exact_fp32_output_does_not_overflow(osr, ops, case, dt):
    """Weights x 64: exact products, fp32 sums < 2^24. What a 16-bit output turns into Inf (past 65504) an fp32 output holds exactly."""
    key, e = case
    ref64 = _exact(ops, osr, key, e, dt, 77, scale=64.0)  # (bit-equal to ref64 rounded to fp32, which is finite)
    assert bool((ref64.abs() > 65520).any()) and bool(torch.isfinite(ref64.float()).all())


@gpu
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ENGINE_CASES, ids=_cid)
def test_float_vs_fp64(osr, ops, case, dt):
    key, e = case
    g = torch.Generator(device=DEV).manual_seed(3000 + zlib.crc32(_cid(case).encode()) % 1000)
    x, w, b, res = _inputs(e, dt, g, False)
    odt = F32 if e[7] == F32 else dt
    cout, kh, kw, cin = e[2]
    got = _run(ops, e, dt, x, w, b, res)
    ref, S = expect(e, x, w, b, res), expect(e, x, w, b, res, absolute=True)
    torch.cuda.synchronize()
    got = got.double()
    chain = kh * kw * cin
    tol = (chain + 2) * 2.0 ** -24 * S + _half_ulp(ref, odt)
    err = (got - ref).abs()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    ratio = float((err / tol.clamp(min=1e-300)).max())
    print(f"[err] {_cid(case)}: max |err| {err.max().item():.3e}, max |err| / bound {ratio:.3e} (chain {chain})")
    assert ratio <= 1.0, f"{_cid(case)}: |err| / bound {ratio:.3e} > 1"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. out= slices of one level-major buffer
# ------------------------------------------------------------------------------------------------------------------------------
PYRAMID = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 2)]
GUARD = 64
# (layer, cout, fp32 output, relu): the stock RPN's hidden state, RetinaNet's cls_score and bbox_pred
SLICE_LAYERS = [("rpn_head.conv", 256, True, True), ("head.cls_score", 720, False, False), ("head.bbox_pred", 40, True, False)]


@gpu
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", SLICE_LAYERS, ids=lambda l: l[0])
def test_out_slices_of_one_buffer(osr, ops, layer, dt):
    """The engines' per-level loop (engine_std._rpn, engine_retinanet._head): one shared weight, each level written through out= into its
    rows of one buffer. Integer data: every level equals its fp64 restatement bit for bit, the 64 rows before the first level and
    after the last still hold the sentinel's bits, and writing the levels in reverse order gives the same buffer."""
    name, cout, fp32, relu = layer
    n, odt = 2, F32 if fp32 else dt
    g = torch.Generator(device=DEV).manual_seed(4100 + cout)
    es = [L(name, (n, h, w, 256), (cout, 3, 3, 256), 1, 1, relu, 0, odt if fp32 else dt, None, 1) for h, w in PYRAMID]
    xs, w, b = [], None, None
    for e in es:
        x, w_, b_, _ = _inputs(e, dt, g, True)
        xs.append(x)
        w, b = (w_, b_) if w is None else (w, b)
    rows = [n * h * wd for h, wd in PYRAMID]
    offs = [GUARD + sum(rows[:i]) for i in range(len(rows))]
    refs64 = [expect(e, x, w, b, None) for e, x in zip(es, xs)]
    bufs = []
    for order in (range(len(es)), reversed(range(len(es)))):
        buf = torch.full((GUARD + sum(rows) + GUARD, cout), SENTINEL, dtype=odt, device=DEV)
        for i in order:
            out = ops.conv2d(xs[i], w, b, 1, 1, relu, None, 0, odt, buf[offs[i]:offs[i] + rows[i]])
            assert out.data_ptr() == buf[offs[i]:].data_ptr()
        torch.cuda.synchronize()
        bufs.append(buf)
    buf = bufs[0]
    for i, (e, r64) in enumerate(zip(es, refs64)):
        _assert_same(buf[offs[i]:offs[i] + rows[i]], r64.to(odt).view(rows[i], cout), r64.view(rows[i], cout), f"{name}, level {PYRAMID[i]}")
    bits = torch.int32 if odt == F32 else torch.int16
    guard = torch.full((GUARD, cout), SENTINEL, dtype=odt, device=DEV).view(bits)
    assert torch.equal(buf[:GUARD].view(bits), guard), "rows before the first level were written"
    assert torch.equal(buf[-GUARD:].view(bits), guard), "rows after the last level were written"
    assert torch.equal(bufs[1].view(bits), buf.view(bits)), "the levels in reverse order give another buffer"


# ------------------------------------------------------------------------------------------------------------------------------
# 5. teeth: wrong restatements differ from the right one on these cases' inputs (CPU, no gpu mark)
# ------------------------------------------------------------------------------------------------------------------------------
def _restate(x, w, b, stride, pad, relu, border=None, origin_2o=False, tall=False):
    """conv + bias (+ ReLU) in fp64 by index gathers, with three switches for the mistakes a kernel can make: border (cin,) -- the
    padding holds these values, not 0; origin_2o -- the taps of output o start at input stride * o, not stride * o - pad; tall --
    the n images are read as one image of n * h rows (a tap past an image's edge reads its neighbour)."""
    n, h, wd, ci = x.shape
    co, kh, kw, _ = w.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    src = x.double().reshape(1, n * h, wd, ci) if tall else x.double()
    N, H = src.shape[:2]
    xp = torch.zeros((N, H + 3 * pad + kh, wd + 3 * pad + kw, ci), dtype=torch.float64)  # (zeros beyond the padding: origin_2o reads past it)
    if border is not None:
        xp[:, :H + 2 * pad, :wd + 2 * pad] = border.double()
    xp[:, pad:pad + H, pad:pad + wd] = src
    off = pad if origin_2o else 0
    out = torch.zeros((n * ho * wo, co), dtype=torch.float64)
    for a in range(kh):
        ri = stride * torch.arange(ho) + a + off
        rows = xp[0][(torch.arange(n)[:, None] * h + ri[None, :]).reshape(-1)].view(n, ho, -1, ci) if tall else xp[:, ri]
        for c in range(kw):
            out += rows[:, :, stride * torch.arange(wo) + c + off].reshape(-1, ci) @ w[:, a, c, :].double().t()
    out = (out + b.double()).view(n, ho, wo, co)
    return out.clamp(min=0) if relu else out


def _cpu_inputs(e, seed):
    """The integer recipe of _inputs on the CPU: |v| <= 2 with zeros, the hot block of positive values, integer bias."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, e[1], generator=g).float()
    x[0, :4] = torch.randint(1, 3, x[0, :4].shape, generator=g).float()
    x[0, 0] = 2
    w = torch.randint(-2, 3, e[2], generator=g).float()
    w[:16] = torch.randint(1, 3, w[:16].shape, generator=g).float()
    w[:4] = 2
    return x, w, torch.randint(-2, 3, (e[2][0],), generator=g).float()


def _teeth_cases():
    """The small-image, tiny-input and stride-2 cases. The restatements are per image, so the many-image cases keep 3 images here."""
    out = []
    for case in ENGINE_CASES:
        key, e = case
        if e[0] == "mask_fcn1" or case in TINY or e[3] == 2:
            n = min(e[1][0], 3)
            out.append(e[:1] + ((n,) + e[1][1:],) + e[2:])
    return out


@pytest.mark.parametrize("e", _teeth_cases(), ids=lambda e: f"{e[0]}-{'x'.join(map(str, e[1]))}-co{e[2][0]}-s{e[3]}")
def test_wrong_restatements_differ(e):
    _, _, _, stride, pad, relu = e[:6]
    x, w, b = _cpu_inputs(e, 9000 + zlib.crc32(repr(e[:6]).encode()) % 1000)
    right = expect(e, x, w, b, None)
    assert torch.equal(_restate(x, w, b, stride, pad, relu), right)  # the gather form with no switch set is the restatement
    # padding that contributes relu(bias) (of the layer before: one value per input channel) instead of 0
    border = torch.arange(e[1][3]).remainder(3).float()  # relu of integer biases: 0, 1, 2
    assert not torch.equal(_restate(x, w, b, stride, pad, relu, border=border), right)
    # image boundaries ignored
    assert not torch.equal(_restate(x, w, b, stride, pad, relu, tall=True), right)
    if stride == 2:  # taps from origin 2 o instead of 2 o - pad
        assert not torch.equal(_restate(x, w, b, stride, pad, relu, origin_2o=True), right)
    if not relu:  # a ReLU the flag does not ask for (p6 has none)
        assert bool((right < 0).any()) and not torch.equal(_restate(x, w, b, stride, pad, True), right)
