"""osr_conv2d_fwd (csrc/osr_conv_gemm64.hip) at every launch plan the engine's forward pass takes, against an explicit fp64 restatement
(per-tap shifted-view GEMMs in torch.float64 on the GPU, the epilogue in fp64, one rounding; never a torch fp16 / fp32 convolution).

Launch table: `forward_table` lists every single-layer ops.conv2d / ops.linear launch of one fast-mode OpensetRCNNEngine.forward_device
pass with the fused forms off (fuse_res2 = chain_res3 = fuse_levels = False; the stem and the CF-RPN head have kernels of their own), for
batch 16 at 800 x 1344, a 4-image micro-batch under concurrent_streams(4), batch 8 at 768 x 1344 and 2 x 256 x 352, in the MSRA
(stride_in_1x1) and the torchvision layout. test_table_is_the_engines_forward records one real pass per geometry and layout and requires
the table, so it cannot drift from the engine. These passes are the only production-size work of this file.

Plan key of a launch (plan_key, from osr_conv2d_fwd_describe with the workspace offered as ops.conv2d offers it): tile "BMxBN/stages",
split-K tail or not, 1x1 / KxK, stride, res_mode, relu, dense 1 x 1 input (the pw_dense row shortcut), 16-bit / fp32 output, row_seg.
The eight tables hold 45 keys on all seven tiles. CASES has, for every key, K and cout of a production layer at the smallest awkward
shape that keeps the key; test_plans_reached asserts that every key of every table is the key of some case and every case has the key
written beside it, and prints the key -> layers map (pytest -s): when the cost model moves, it names the plan that lost its case.

Exact runs: x, w, residual and bias hold small integers (|v| <= 2, zeros mixed in), so every product is exact and every fp32 partial
sum stays below 2^24 (4 x 12544 + 4 for FC1): the kernel must equal the fp64 restatement BIT FOR BIT over the whole tensor -- a dropped,
duplicated or misaddressed row, tap, K slice, split or tile is a nonzero integer. A hot block of positive values pushes results past
2048 (fp16) / 256 (bf16), where odd integers round to even as .half() / .bfloat16() do; one case per tile runs with weights x 64, so
that fp16 results pass 65504 and must be +-Inf. res_mode 2 reads its source pixel at odd ho, wo; res_mode 3's mask holds +0.0 and -0.0.
Row segments (FC1 / FC2 on the 256x256/2 + split-K, 128x128/1 and 128x64/2 plans): counts BM + 1, 0, 1, full, BM - 1, BM and a last
segment shorter than a tile; the output is pre-filled with a sentinel, every row of an M tile with a data row must be exact and every
row of the other tiles must still hold the sentinel (include/osr.h: "its rows are left unwritten"). Every case launches twice.
Float runs: random data, x's even channels post-ReLU values of mixed magnitude; elementwise error against fp64 within
tests/test_backbone_bwd_full_size.py's rule, (chain + 2) * 2^-24 * sum|terms| (+ half an ulp of a 16-bit output), chain = kh * kw * cin.
The concurrency hint (include/osr.h: "Tile selection only; results do not depend on it"): per geometry a layer whose tile changes
with it, exact at both hints; no layer of 2 x 256 x 352 changes its tile."""
import ctypes as C
import inspect
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
# name -> (images of the pass, padded H, padded W, streams: the pass runs under ops.concurrent_streams(streams))
GEOMS = {"b16_800x1344": (16, 800, 1344, 1), "mb4of16_800x1344_4streams": (4, 800, 1344, 4), "b8_768x1344": (8, 768, 1344, 1),
         "b2_256x352": (2, 256, 352, 1)}
R50 = ((2, 3, 64, 256), (3, 4, 128, 512), (4, 6, 256, 1024), (5, 3, 512, 2048))  # stage, blocks, bottleneck width, output channels
PRE_NMS_TOPK = 1000  # the engine's pre_nms_topk_test
BU = "backbone.bottom_up."


def stage_hw(H, W):
    """(h, w) of res2..res5 (= p2..p5) and p6 for a padded H x W batch (engine.pyramid_shapes)."""
    h, w = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    out = {}
    for s in (2, 3, 4, 5, 6):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out[s] = (h, w)
    return out


def L(name, x, w, stride=1, pad=0, relu=False, res_mode=0, out_dt=None, row_seg=None, conc=1):
    """One launch: (layer, input shape, weight shape, stride, pad, relu, res_mode, output dtype, row_seg = (segments, rows each) or None,
    concurrency)."""
    return (name, tuple(x), tuple(w), stride, pad, bool(relu), res_mode, out_dt, row_seg, conc)


def forward_table(n, H, W, streams=1, stride_in_1x1=True, dt=F16):
    """Every single-layer ops.conv2d / ops.linear launch of one fast-mode OpensetRCNNEngine.forward_device pass over n images padded to
    H x W under ops.concurrent_streams(streams), fuse_res2 = chain_res3 = fuse_levels = False, in the engine's order. (The stem and
    the CF-RPN head run on kernels of their own.)"""
    hw = stage_hw(H, W)
    T = []
    cin = 64
    for stage, nb, mid, cout in R50:
        hy, wy = hw[stage]
        for b in range(nb):
            stride = 2 if b == 0 and stage > 2 else 1
            hx, wx = hw[stage - 1] if stride == 2 else hw[stage]
            s1, s2 = (stride, 1) if stride_in_1x1 else (1, stride)
            h1, w1 = (hy, wy) if s1 == stride else (hx, wx)  # conv1's output
            pre = f"{BU}res{stage}.{b}"
            if b == 0:
                T.append(L(pre + ".shortcut", (n, hx, wx, cin), (cout, 1, 1, cin), stride, 0, False, 0, dt, None, streams))
            T += [L(pre + ".conv1", (n, hx, wx, cin), (mid, 1, 1, cin), s1, 0, True, 0, dt, None, streams),
                  L(pre + ".conv2", (n, h1, w1, mid), (mid, 3, 3, mid), s2, 1, True, 0, dt, None, streams),
                  L(pre + ".conv3", (n, hy, wy, mid), (cout, 1, 1, mid), 1, 0, True, 1, dt, None, streams)]
            cin = cout
    for lvl in (5, 4, 3, 2):
        T.append(L(f"backbone.fpn_lateral{lvl}", (n,) + hw[lvl] + (R50[lvl - 2][3],), (256, 1, 1, R50[lvl - 2][3]), 1, 0, False, 0 if lvl == 5 else 2,
                   dt, None, streams))
    for lvl in (2, 3, 4, 5):
        T.append(L(f"backbone.fpn_output{lvl}", (n,) + hw[lvl] + (256,), (256, 3, 3, 256), 1, 1, False, 0, dt, None, streams))
    cap = sum(min(PRE_NMS_TOPK, hw[s][0] * hw[s][1]) for s in (2, 3, 4, 5, 6))  # slots of one image's padded proposal list
    m = n * cap
    T += [L("roi_heads.box_head.fc1", (1, m, 1, 12544), (1024, 1, 1, 12544), 1, 0, True, 0, dt, (n, cap), streams),
          L("roi_heads.box_head.fc2", (1, m, 1, 1024), (1024, 1, 1, 1024), 1, 0, True, 0, F32, (n, cap), streams)]
    return T


def out_hw(e):
    _, (n, h, w, cin), (cout, kh, kw, _), stride, pad = e[:5]
    return (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1


# ------------------------------------------------------------------------------------------------------------------------------
# plan keys
# ------------------------------------------------------------------------------------------------------------------------------
def describe(osr, e):
    """osr_conv2d_fwd_describe of the launch ops.conv2d makes for this entry (the workspace offered as ops.conv2d offers it)."""
    from openset_rcnn_amd.host import ops
    lib = osr._lib.load()
    name, (n, h, w, cin), (cout, kh, kw, _), stride, pad, relu, res_mode, out_dt, row_seg, conc = e
    ho, wo = out_hw(e)
    in_dt = out_dt if out_dt in (F16, BF16) else F16
    with ops.concurrent_streams(conc):
        p = ops._conv_params(n, h, w, cin, ho, wo, cout, kh, kw, stride, pad, in_dt, out_dt or in_dt)
    p.relu, p.res_mode = int(relu), res_mode
    ws = int(ops.SPLIT_K_TAIL and res_mode == 0 and stride == 1 and lib.osr_conv2d_fwd_workspace_bytes(C.byref(p)) > 0)
    buf = C.create_string_buffer(256)
    lib.osr_conv2d_fwd_describe(C.byref(p), ws, buf, 256)
    return buf.value.decode()


def plan_key(osr, e):
    """(tile "BMxBN/stages", split-K tail, "1x1" / "KxK", stride, res_mode, relu, dense 1 x 1 input, "16" / "32" output bits, row_seg)."""
    name, (n, h, w, cin), (cout, kh, kw, _), stride, pad, relu, res_mode, out_dt, row_seg, conc = e
    d = describe(osr, e)
    ho, wo = out_hw(e)
    dense = kh == 1 and kw == 1 and stride == 1 and pad == 0 and n * ho * wo * max(cin, cout) < 2 ** 31  # Conv64Args::pw_dense & 1
    return (d.split(" ")[0], "split-K" in d, "1x1" if kh * kw == 1 else "KxK", stride, res_mode, relu, dense, "32" if out_dt == F32 else "16",
            row_seg is not None)


def _short(name):
    return name.replace(BU, "").replace("backbone.", "").replace("roi_heads.box_head.", "")


def tile_of(key):
    """(BM, BN) of a plan key."""
    bm, bn = key[0].split("/")[0].split("x")
    return int(bm), int(bn)


# Reduced shapes, one or more per plan key: K and cout of a production layer that has the key, rows shrunk to the smallest
# n x h x w (odd h and w, n = 2 or 3, at least three M tiles) at which osr_conv2d_fwd_describe still gives the key, rows and rows per
# image no multiple of BM (the last M tile is ragged and an M tile spans an image boundary), odd h and w under stride 2, odd ho and wo
# under res_mode 2; a second (third) case with cout = BN + 64 (128-wide tiles) or 8 and 72 (64-wide tiles) wherever some shape keeps
# the tile at that width (none does for 128x128/2; the 256-wide tiles need cout % 256 == 0). FC cases: 7 row segments, the last one
# shorter than a tile. (expected plan key, launch): test_plans_reached holds every case to its key.
CASES = [
    (("128x128/1", False, "1x1", 1, 0, False, True, "16", False), L("res2.0.shortcut", (2, 113, 145, 64), (256, 1, 1, 64), 1, 0, False, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 0, False, True, "16", False), L("res2.0.shortcut", (2, 97, 225, 64), (192, 1, 1, 64), 1, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 0, True, True, "16", False), L("res2.0.conv1", (2, 7, 19, 64), (64, 1, 1, 64), 1, 0, True, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 0, True, True, "16", False), L("res2.0.conv1", (2, 7, 19, 64), (8, 1, 1, 64), 1, 0, True, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 0, True, True, "16", False), L("res2.0.conv1", (2, 7, 19, 64), (72, 1, 1, 64), 1, 0, True, 0, F16, None, 1)),
    (("128x64/1", False, "KxK", 1, 0, True, False, "16", False), L("res2.0.conv2", (2, 199, 247, 64), (64, 3, 3, 64), 1, 1, True, 0, F16, None, 1)),
    (("128x64/1", False, "KxK", 1, 0, True, False, "16", False), L("res2.0.conv2", (2, 199, 247, 64), (8, 3, 3, 64), 1, 1, True, 0, F16, None, 1)),
    (("128x64/1", False, "KxK", 1, 0, True, False, "16", False), L("res2.0.conv2", (3, 113, 145, 64), (72, 3, 3, 64), 1, 1, True, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 1, True, True, "16", False), L("res2.0.conv3", (2, 113, 145, 64), (256, 1, 1, 64), 1, 0, True, 1, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 1, True, True, "16", False), L("res2.0.conv3", (2, 97, 225, 64), (192, 1, 1, 64), 1, 0, True, 1, F16, None, 1)),
    (("128x128/1", False, "1x1", 2, 0, False, False, "16", False), L("res3.0.shortcut", (2, 109, 297, 256), (512, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 2, 0, False, False, "16", False), L("res3.0.shortcut", (3, 149, 387, 256), (192, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 2, 0, True, False, "16", False), L("res3.0.conv1", (3, 229, 379, 256), (128, 1, 1, 256), 2, 0, True, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 2, 0, True, False, "16", False), L("res3.0.conv1", (3, 149, 387, 256), (192, 1, 1, 256), 2, 0, True, 0, F16, None, 1)),
    (("128x128/1", False, "KxK", 1, 0, True, False, "16", False), L("res3.0.conv2", (2, 115, 285, 128), (128, 3, 3, 128), 1, 1, True, 0, F16, None, 1)),
    (("128x128/1", False, "KxK", 1, 0, True, False, "16", False), L("res3.0.conv2", (2, 97, 225, 128), (192, 3, 3, 128), 1, 1, True, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 0, True, True, "16", False), L("res3.1.conv1", (2, 115, 285, 512), (128, 1, 1, 512), 1, 0, True, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 0, True, True, "16", False), L("res3.1.conv1", (2, 97, 225, 512), (192, 1, 1, 512), 1, 0, True, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, False, True, "16", False), L("fpn_lateral5", (2, 7, 19, 2048), (256, 1, 1, 2048), 1, 0, False, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, False, True, "16", False), L("fpn_lateral5", (2, 7, 19, 2048), (8, 1, 1, 2048), 1, 0, False, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, False, True, "16", False), L("fpn_lateral5", (2, 7, 19, 2048), (72, 1, 1, 2048), 1, 0, False, 0, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral4", (2, 113, 145, 1024), (256, 1, 1, 1024), 1, 0, False, 2, F16, None, 1)),
    (("128x128/1", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral4", (2, 97, 225, 1024), (192, 1, 1, 1024), 1, 0, False, 2, F16, None, 1)),
    (("256x256/2", True, "KxK", 1, 0, False, False, "16", False), L("fpn_output2", (3, 199, 247, 256), (256, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x128/1", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output4", (2, 113, 145, 256), (256, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x128/1", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output4", (2, 97, 225, 256), (192, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output5", (2, 7, 19, 256), (256, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output5", (2, 7, 19, 256), (8, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output5", (2, 7, 19, 256), (72, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    (("256x256/2", True, "1x1", 1, 0, True, True, "16", True), L("fc1", (1, 36873, 1, 12544), (1024, 1, 1, 12544), 1, 0, True, 0, F16, (7, 6125), 1)),
    (("128x128/1", False, "1x1", 1, 0, True, True, "32", True), L("fc2", (1, 8201, 1, 1024), (1024, 1, 1, 1024), 1, 0, True, 0, F32, (7, 1357), 1)),
    (("128x128/1", False, "1x1", 1, 0, True, True, "32", True), L("fc2", (1, 43649, 1, 1024), (192, 1, 1, 1024), 1, 0, True, 0, F32, (7, 7265), 1)),
    (("128x64/2", False, "KxK", 1, 0, True, False, "16", False), L("res2.0.conv2", (2, 7, 19, 64), (64, 3, 3, 64), 1, 1, True, 0, F16, None, 4)),
    (("128x64/2", False, "KxK", 1, 0, True, False, "16", False), L("res2.0.conv2", (2, 7, 19, 64), (8, 3, 3, 64), 1, 1, True, 0, F16, None, 4)),
    (("128x64/2", False, "KxK", 1, 0, True, False, "16", False), L("res2.0.conv2", (2, 7, 19, 64), (72, 3, 3, 64), 1, 1, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 2, 0, True, False, "16", False), L("res4.0.conv1", (2, 19, 25, 512), (256, 1, 1, 512), 2, 0, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 2, 0, True, False, "16", False), L("res4.0.conv1", (2, 19, 25, 512), (8, 1, 1, 512), 2, 0, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 2, 0, True, False, "16", False), L("res4.0.conv1", (2, 19, 25, 512), (72, 1, 1, 512), 2, 0, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", False), L("res4.1.conv1", (2, 7, 19, 1024), (256, 1, 1, 1024), 1, 0, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", False), L("res4.1.conv1", (2, 7, 19, 1024), (8, 1, 1, 1024), 1, 0, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", False), L("res4.1.conv1", (2, 7, 19, 1024), (72, 1, 1, 1024), 1, 0, True, 0, F16, None, 4)),
    (("128x64/2", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral4", (2, 7, 19, 1024), (256, 1, 1, 1024), 1, 0, False, 2, F16, None, 4)),
    (("128x64/2", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral4", (2, 7, 19, 1024), (8, 1, 1, 1024), 1, 0, False, 2, F16, None, 4)),
    (("128x64/2", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral4", (2, 7, 19, 1024), (72, 1, 1, 1024), 1, 0, False, 2, F16, None, 4)),
    (("256x256/2", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output3", (2, 113, 145, 256), (256, 3, 3, 256), 1, 1, False, 0, F16, None, 4)),
    (("128x256/1", False, "1x1", 2, 0, False, False, "16", False), L("res3.0.shortcut", (3, 109, 297, 256), (512, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
    (("256x128/1", False, "1x1", 2, 0, True, False, "16", False), L("res3.0.conv1", (3, 337, 387, 256), (128, 1, 1, 256), 2, 0, True, 0, F16, None, 1)),
    (("256x128/1", False, "1x1", 2, 0, True, False, "16", False), L("res3.0.conv1", (3, 225, 289, 256), (192, 1, 1, 256), 2, 0, True, 0, F16, None, 1)),
    (("256x128/1", False, "KxK", 1, 0, True, False, "16", False), L("res3.0.conv2", (2, 199, 247, 128), (128, 3, 3, 128), 1, 1, True, 0, F16, None, 1)),
    (("256x128/1", False, "KxK", 1, 0, True, False, "16", False), L("res3.0.conv2", (3, 113, 145, 128), (192, 3, 3, 128), 1, 1, True, 0, F16, None, 1)),
    (("256x128/1", False, "1x1", 1, 0, True, True, "16", False), L("res3.1.conv1", (2, 199, 247, 512), (128, 1, 1, 512), 1, 0, True, 0, F16, None, 1)),
    (("256x128/1", False, "1x1", 1, 0, True, True, "16", False), L("res3.1.conv1", (3, 113, 145, 512), (192, 1, 1, 512), 1, 0, True, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 2, 0, True, False, "16", False), L("res4.0.conv1", (3, 109, 297, 512), (256, 1, 1, 512), 2, 0, True, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 2, 0, True, False, "16", False), L("res4.0.conv1", (3, 337, 387, 512), (8, 1, 1, 512), 2, 0, True, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 2, 0, True, False, "16", False), L("res4.0.conv1", (3, 225, 289, 512), (72, 1, 1, 512), 2, 0, True, 0, F16, None, 1)),
    (("128x128/2", False, "KxK", 1, 0, True, False, "16", False), L("res4.0.conv2", (3, 55, 149, 256), (256, 3, 3, 256), 1, 1, True, 0, F16, None, 1)),
    # (cout 192: no shape keeps 128x128/2)
    (("128x128/2", False, "1x1", 1, 0, True, True, "16", False), L("res4.1.conv1", (3, 55, 149, 1024), (256, 1, 1, 1024), 1, 0, True, 0, F16, None, 1)),
    # (cout 192: no shape keeps 128x128/2)
    (("256x256/2", False, "1x1", 2, 0, False, False, "16", False), L("res5.0.shortcut", (2, 105, 115, 1024), (2048, 1, 1, 1024), 2, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 1, True, True, "16", False), L("res5.0.conv3", (2, 29, 53, 512), (2048, 1, 1, 512), 1, 0, True, 1, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 1, True, True, "16", False), L("res5.0.conv3", (2, 199, 247, 512), (8, 1, 1, 512), 1, 0, True, 1, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 1, True, True, "16", False), L("res5.0.conv3", (3, 113, 145, 512), (72, 1, 1, 512), 1, 0, True, 1, F16, None, 1)),
    (("128x128/2", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral4", (3, 55, 149, 1024), (256, 1, 1, 1024), 1, 0, False, 2, F16, None, 1)),
    # (cout 192: no shape keeps 128x128/2)
    (("128x128/2", False, "KxK", 1, 0, False, False, "16", False), L("fpn_output4", (3, 55, 149, 256), (256, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    # (cout 192: no shape keeps 128x128/2)
    (("128x128/1", False, "1x1", 1, 0, True, True, "16", True), L("fc1", (1, 8201, 1, 12544), (1024, 1, 1, 12544), 1, 0, True, 0, F16, (7, 1357), 1)),
    (("128x128/1", False, "1x1", 1, 0, True, True, "16", True), L("fc1", (1, 43649, 1, 12544), (192, 1, 1, 12544), 1, 0, True, 0, F16, (7, 7265), 1)),
    (("128x64/1", False, "1x1", 1, 0, False, True, "16", False), L("res2.0.shortcut", (2, 7, 19, 64), (256, 1, 1, 64), 1, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 0, False, True, "16", False), L("res2.0.shortcut", (2, 7, 19, 64), (8, 1, 1, 64), 1, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 0, False, True, "16", False), L("res2.0.shortcut", (2, 7, 19, 64), (72, 1, 1, 64), 1, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 2, 0, False, False, "16", False), L("res3.0.shortcut", (2, 19, 25, 256), (512, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 2, 0, False, False, "16", False), L("res3.0.shortcut", (2, 19, 25, 256), (8, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
    (("128x64/1", False, "1x1", 2, 0, False, False, "16", False), L("res3.0.shortcut", (2, 19, 25, 256), (72, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 2, 0, False, False, "16", False), L("res4.0.shortcut", (2, 19, 25, 512), (1024, 1, 1, 512), 2, 0, False, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 2, 0, False, False, "16", False), L("res4.0.shortcut", (2, 19, 25, 512), (8, 1, 1, 512), 2, 0, False, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 2, 0, False, False, "16", False), L("res4.0.shortcut", (2, 19, 25, 512), (72, 1, 1, 512), 2, 0, False, 0, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 1, True, True, "16", False), L("res5.0.conv3", (2, 7, 19, 512), (2048, 1, 1, 512), 1, 0, True, 1, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 1, True, True, "16", False), L("res5.0.conv3", (2, 7, 19, 512), (8, 1, 1, 512), 1, 0, True, 1, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 1, True, True, "16", False), L("res5.0.conv3", (2, 7, 19, 512), (72, 1, 1, 512), 1, 0, True, 1, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral2", (2, 7, 19, 256), (256, 1, 1, 256), 1, 0, False, 2, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral2", (2, 7, 19, 256), (8, 1, 1, 256), 1, 0, False, 2, F16, None, 1)),
    (("128x64/1", False, "1x1", 1, 2, False, True, "16", False), L("fpn_lateral2", (2, 7, 19, 256), (72, 1, 1, 256), 1, 0, False, 2, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", True), L("fc1", (1, 2393, 1, 12544), (1024, 1, 1, 12544), 1, 0, True, 0, F16, (7, 389), 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", True), L("fc1", (1, 2393, 1, 12544), (8, 1, 1, 12544), 1, 0, True, 0, F16, (7, 389), 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "16", True), L("fc1", (1, 2393, 1, 12544), (72, 1, 1, 12544), 1, 0, True, 0, F16, (7, 389), 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "32", True), L("fc2", (1, 2393, 1, 1024), (1024, 1, 1, 1024), 1, 0, True, 0, F32, (7, 389), 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "32", True), L("fc2", (1, 2393, 1, 1024), (8, 1, 1, 1024), 1, 0, True, 0, F32, (7, 389), 1)),
    (("128x64/2", False, "1x1", 1, 0, True, True, "32", True), L("fc2", (1, 2393, 1, 1024), (72, 1, 1, 1024), 1, 0, True, 0, F32, (7, 389), 1)),
    (("128x128/1", False, "KxK", 2, 0, True, False, "16", False), L("res3.0.conv2", (3, 229, 379, 128), (128, 3, 3, 128), 2, 1, True, 0, F16, None, 1)),
    (("128x128/1", False, "KxK", 2, 0, True, False, "16", False), L("res3.0.conv2", (3, 149, 387, 128), (192, 3, 3, 128), 2, 1, True, 0, F16, None, 1)),
    (("128x64/2", False, "KxK", 2, 0, True, False, "16", False), L("res4.0.conv2", (2, 19, 25, 256), (256, 3, 3, 256), 2, 1, True, 0, F16, None, 4)),
    (("128x64/2", False, "KxK", 2, 0, True, False, "16", False), L("res4.0.conv2", (2, 19, 25, 256), (8, 3, 3, 256), 2, 1, True, 0, F16, None, 4)),
    (("128x64/2", False, "KxK", 2, 0, True, False, "16", False), L("res4.0.conv2", (2, 19, 25, 256), (72, 3, 3, 256), 2, 1, True, 0, F16, None, 4)),
    (("256x128/1", False, "KxK", 2, 0, True, False, "16", False), L("res3.0.conv2", (3, 337, 387, 128), (128, 3, 3, 128), 2, 1, True, 0, F16, None, 1)),
    (("256x128/1", False, "KxK", 2, 0, True, False, "16", False), L("res3.0.conv2", (3, 225, 289, 128), (192, 3, 3, 128), 2, 1, True, 0, F16, None, 1)),
    (("128x256/1", False, "1x1", 1, 0, True, True, "16", False), L("res4.0.conv1", (3, 113, 145, 512), (256, 1, 1, 512), 1, 0, True, 0, F16, None, 1)),
    (("128x128/2", False, "KxK", 2, 0, True, False, "16", False), L("res4.0.conv2", (3, 109, 297, 256), (256, 3, 3, 256), 2, 1, True, 0, F16, None, 1)),
    # (cout 192: no shape keeps 128x128/2)
    (("256x256/2", False, "1x1", 1, 0, True, True, "16", False), L("res5.0.conv1", (3, 55, 149, 1024), (512, 1, 1, 1024), 1, 0, True, 0, F16, None, 1)),
    # res_mode 3 (the ReLU mask of the data gradients; no forward launch has it): +0.0 / -0.0 in the mask
    (("128x64/1", False, "1x1", 1, 3, False, True, "16", False), L("res2.0.conv3", (2, 7, 19, 64), (256, 1, 1, 64), 1, 0, False, 3, F16, None, 1)),
    (("128x64/2", False, "1x1", 1, 3, False, True, "16", False), L("res5.0.conv3", (2, 7, 19, 512), (2048, 1, 1, 512), 1, 0, False, 3, F16, None, 1)),
]

# (geometry, hint k, tile at hint 1, tile at hint k, launch): a layer of the geometry's table whose tile changes with the concurrency
# hint, reduced as above. No layer of b2_256x352 changes its tile (test_concurrency_hint_changes_the_tile_not_the_result asserts that).
CONC_CASES = [
    ("b16_800x1344", 2, "128x256/1", "256x256/2", L("res4.0.shortcut", (2, 105, 231, 512), (1024, 1, 1, 512), 2, 0, False, 0, F16, None, 1)),
    ("mb4of16_800x1344_4streams", 4, "128x128/1", "256x256/2", L("fpn_output3", (2, 113, 145, 256), (256, 3, 3, 256), 1, 1, False, 0, F16, None, 1)),
    ("b8_768x1344", 2, "128x256/1", "256x256/2", L("res3.0.shortcut", (3, 109, 297, 256), (512, 1, 1, 256), 2, 0, False, 0, F16, None, 1)),
]


def _cid(c):
    key, e = c
    return f"{_short(e[0])}-{'x'.join(map(str, e[1]))}-co{e[2][0]}-s{e[3]}-r{e[6]}-c{e[9]}-{key[0].replace('/', 'b')}"


@pytest.fixture(scope="module")
def ops(osr):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    osr._lib.load()
    return osr.ops


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the table against the engine
# ------------------------------------------------------------------------------------------------------------------------------
def record_launches(ops, fn):
    """fn() with ops.conv2d / ops.linear wrapped -> [(the launch as an L(...) entry without its name, it came through ops.linear)], in
    launch order; synchronised. (tests/test_conv_fwd_plans_engines.py records the later engines with it.)"""
    real_conv, real_linear = ops.conv2d, ops.linear
    sig = inspect.signature(real_conv)
    log, depth = [], [0]

    def conv(*a, **k):
        b = sig.bind(*a, **k)
        b.apply_defaults()
        v = b.arguments
        assert v["post_mask"] is None
        seg = None if v["row_seg"] is None else (v["row_seg"][0].numel(), int(v["row_seg"][1]))
        log.append(((tuple(v["x"].shape), tuple(v["weight"].shape), v["stride"], v["pad"], bool(v["relu"]), v["res_mode"],
                     v["out_dtype"] or v["x"].dtype, seg, ops._CONCURRENCY[0]), depth[0] > 0))
        return real_conv(*a, **k)

    def linear(*a, **k):
        depth[0] += 1
        try:
            return real_linear(*a, **k)
        finally:
            depth[0] -= 1

    ops.conv2d, ops.linear = conv, linear
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.conv2d, ops.linear = real_conv, real_linear
    return log


def record_pass(ops, eng, n, H, W, streams):
    """record_launches of one eng.forward_device pass over n random uint8 images padded to H x W under concurrent_streams(streams)."""
    g = torch.Generator().manual_seed(n + H)
    images = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8).to(DEV)
    image_hw = torch.tensor([(H, W)] * n, dtype=torch.int32).to(DEV)

    def run():
        with ops.concurrent_streams(streams):
            eng.forward_device(images, image_hw, H, W)
    try:
        return record_launches(ops, run)
    finally:
        del images
        torch.cuda.empty_cache()


@pytest.mark.parametrize("stride_in_1x1", [True, False])
def test_table_is_the_engines_forward(ops, stride_in_1x1):
    from openset_rcnn_amd.host.engine import OpensetRCNNEngine
    from openset_rcnn_amd.host.weights import random_params

    eng = OpensetRCNNEngine(random_params(0), cfg=dict(stride_in_1x1=stride_in_1x1), dtype=F16, device=DEV)
    eng.fuse_res2 = eng.chain_res3 = eng.fuse_levels = False
    for gname, (n, H, W, streams) in GEOMS.items():
        log = record_pass(ops, eng, n, H, W, streams)
        want = forward_table(n, H, W, streams, stride_in_1x1)
        for i, ((got, via_linear), e) in enumerate(zip(log, want)):
            assert got == e[1:], f"{gname}: launch {i} ({e[0]}): engine {got} != table {e[1:]}"
            assert via_linear == (e[8] is not None), f"{gname}: launch {i} ({e[0]}): ops.linear {via_linear}"
        assert len(log) == len(want), f"{gname}: {len(log)} launches, table {len(want)}"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the plans the tables reach, and the cases that cover them
# ------------------------------------------------------------------------------------------------------------------------------
def test_plans_reached(osr):
    have = {}
    for key, e in CASES:
        got = plan_key(osr, e)
        assert got == key, f"case {_cid((key, e))}: osr_conv2d_fwd_describe gives {got} ({describe(osr, e)}), the case says {key}"
        bm, bn = tile_of(key)
        m = e[1][0] * out_hw(e)[0] * out_hw(e)[1]
        assert m % bm != 0 and m > 2 * bm, f"case {_cid((key, e))}: {m} rows on BM {bm}"
        have.setdefault(key, []).append(e)
    missing = []
    for layout in (True, False):
        for gname, (n, H, W, streams) in GEOMS.items():
            keys = {}
            for e in forward_table(n, H, W, streams, layout):
                keys.setdefault(plan_key(osr, e), []).append(f"{_short(e[0])} [{describe(osr, e)}]")
            print(f"[plan] {gname}, stride_in_1x1={layout}: {len(keys)} keys")
            for k, layers in keys.items():
                print(f"[plan]   {k} <- {'; '.join(layers)}")
                if k not in have:
                    missing.append((gname, layout, k, layers[0]))
    assert not missing, "plan keys of the engine's forward pass that no case of CASES has:\n" + "\n".join(map(str, missing))
    # partial last N tiles: every 64-wide key has cout 8 and 72, every 128-wide key but the 128x128/2 ones has cout 192
    for key, es in have.items():
        if key[4] == 3:
            continue
        couts = {e[2][0] for e in es}
        bm, bn = tile_of(key)
        if bn == 64:
            assert {8, 72} <= couts, (key, couts)
        elif bn == 128 and key[0] != "128x128/2":
            assert 192 in couts, (key, couts)


# ------------------------------------------------------------------------------------------------------------------------------
# fp64 restatement (NHWC, weights (cout, kh, kw, cin)); exact for integer data
# ------------------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, stride, pad):
    """(n, ho, wo, cout) fp64: per tap one GEMM of the shifted, strided view of the zero-padded x with w[:, a, b, :]."""
    n, h, wd, ci = x.shape
    co, kh, kw, _ = w.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    out = torch.zeros((n * ho * wo, co), dtype=torch.float64, device=x.device)
    if kh == 1 and kw == 1 and stride == 1 and pad == 0:
        x2, w2 = x.reshape(-1, ci), w.reshape(co, ci)
        for k0 in range(0, ci, 2048):  # (FC1: K = 12544 -- the fp64 copy of the rows in slices)
            out += x2[:, k0:k0 + 2048].double() @ w2[:, k0:k0 + 2048].double().t()
    else:
        xp = F.pad(x.double(), (0, 0, pad, pad, pad, pad))
        for a in range(kh):
            for b in range(kw):
                out += xp[:, a:a + stride * (ho - 1) + 1:stride, b:b + stride * (wo - 1) + 1:stride].reshape(-1, ci) @ w[:, a, b, :].double().t()
    return out.view(n, ho, wo, co)


def expect(e, x, w, b, res, absolute=False):
    """fp64 result of the launch: conv + bias, the residual epilogue, ReLU. absolute: the same sum on |operands| (no mask, no ReLU
    would change it: a masked element is an exact zero on both sides)."""
    _, _, _, stride, pad, relu, res_mode = e[:7]
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    v = conv_ref(f(x), f(w), stride, pad) + f(b).double()
    ho, wo = v.shape[1], v.shape[2]
    if res_mode == 1:
        v += f(res).double()
    elif res_mode == 2:  # nearest 2x upsample of the coarser level: source pixel (oh // 2, ow // 2)
        ih, iw = torch.arange(ho, device=v.device) // 2, torch.arange(wo, device=v.device) // 2
        v += f(res).double()[:, ih][:, :, iw]
    elif res_mode == 3:
        v = torch.where(res > 0, v, torch.zeros_like(v))
    if relu and not absolute:
        v = v.clamp(min=0)
    return v


def _ints(shape, g, dt, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV, dtype=torch.int8).to(dt)


def _relu_out(shape, g, dt):
    """A ReLU output: +0.0, -0.0 and positive integers, a quarter each of the zeros, half positive."""
    k = torch.randint(0, 4, shape, generator=g, device=DEV)
    v = torch.randint(1, 4, shape, generator=g, device=DEV).to(dt)
    v[k == 0] = 0.0
    v[k == 1] = -0.0
    return v


def _res_shape(e):
    n, cout = e[1][0], e[2][0]
    ho, wo = out_hw(e)
    return (n, (ho + 1) // 2, (wo + 1) // 2, cout) if e[6] == 2 else (n, ho, wo, cout)


def _inputs(e, dt, g, exact, scale=1.0):
    """x, w, bias, residual. exact: integers |v| <= 2 with zeros mixed in; the hot block -- image 0's pixel rows 0..3 of x hold {1, 2}
    (row 0: all 2), output channels 0..15 of w hold {1, 2} (0..3: all 2) -- sums same-signed terms: up to 4 K there, 2.25 K on average.
    else: random data; x's even channels are post-ReLU values of mixed magnitude (2^-6 .. 2^3), the odd ones normal."""
    _, xs, ws, stride, pad, relu, res_mode = e[:7]
    cout, kh, kw, cin = ws
    if exact:
        x = _ints(xs, g, dt)
        x[0, :4] = torch.randint(1, 3, x[0, :4].shape, generator=g, device=DEV).to(dt)
        x[0, 0] = 2
        w = _ints(ws, g, dt)
        w[:16] = torch.randint(1, 3, w[:16].shape, generator=g, device=DEV).to(dt)
        w[:4] = 2
        w = (w * scale).to(dt)
        b = _ints((cout,), g, F32)
        res = None if res_mode == 0 else (_relu_out(_res_shape(e), g, dt) if res_mode == 3 else _ints(_res_shape(e), g, dt))
    else:
        x = torch.randn(xs, generator=g, device=DEV)
        x[..., ::2] = x[..., ::2].clamp(min=0) * torch.exp2(torch.randint(-6, 4, x[..., ::2].shape, generator=g, device=DEV).float())
        x = x.to(dt)
        w = (torch.randn(ws, generator=g, device=DEV) / (kh * kw * cin) ** 0.5).to(dt)
        b = torch.randn((cout,), generator=g, device=DEV)
        res = None if res_mode == 0 else (_relu_out(_res_shape(e), g, dt) if res_mode == 3 else torch.randn(_res_shape(e), generator=g, device=DEV).to(dt))
    return x, w, b, res


def _seg_counts(e, bm):
    """Data rows per segment: BM + 1, 0, 1, full, BM - 1, BM, and the last segment, shorter than a tile, full."""
    segs, sr = e[8]
    m = e[1][1]
    last = m - (segs - 1) * sr
    assert segs == 7 and 0 < last < bm and sr >= 3 * bm
    return [bm + 1, 0, 1, sr, bm - 1, bm, last]


def _run(ops, e, dt, x, w, b, res, conc=None, out=None, counts=None):
    _, _, _, stride, pad, relu, res_mode, out_dt, row_seg, c = e
    seg = None if row_seg is None else (torch.tensor(counts, dtype=torch.int32, device=DEV), row_seg[1])
    with ops.concurrent_streams(c if conc is None else conc):
        return ops.conv2d(x, w, b, stride, pad, relu, res, res_mode, F32 if out_dt == F32 else dt, out, row_seg=seg)


def _assert_same(got, ref, ref64, what):
    if not torch.equal(got, ref):
        bad = (got.double() != ref.double()) & ~(got.isnan() & ref.isnan())
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {bad.sum().item()} of {got.numel()} elements differ; first at {i}: got {got[tuple(i)].item()} "
                             f"ref {ref[tuple(i)].item()} (fp64 {ref64[tuple(i)].item()})")


SENTINEL = 0.5  # no integer run gives it


def _exact(ops, osr, key, e, dt, seed, scale=1.0, conc=None):
    """Integer run of one case in storage dtype dt: the whole output equals the fp64 restatement rounded once; two launches agree.
    row_seg: every row of an M tile with a data row is exact, every row of the other tiles keeps the sentinel."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x, w, b, res = _inputs(e, dt, g, True, scale)
    cout, kh, kw, cin = e[2]
    assert 4 * kh * kw * cin * scale + 2 + 2 < 2 ** 24  # every fp32 partial sum is an exact integer
    odt = F32 if e[7] == F32 else dt
    ref64 = expect(e, x, w, b, res)
    assert ref64.abs().max().item() < 2 ** 24
    ref = ref64.to(odt)
    counts = None
    outs = [None, None]
    if e[8] is not None:
        bm = tile_of(key)[0]
        counts = _seg_counts(e, bm)
        outs = [torch.full(ref.shape, SENTINEL, dtype=odt, device=DEV) for _ in range(2)]
    got = _run(ops, e, dt, x, w, b, res, conc, outs[0], counts)
    again = _run(ops, e, dt, x, w, b, res, conc, outs[1], counts)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two launches differ"
    if counts is not None:
        segs, sr = e[8]
        m = e[1][1]
        data = torch.zeros(m, dtype=torch.bool, device=DEV)
        for s, c in enumerate(counts):
            data[s * sr:s * sr + c] = True
        tiles = (m + bm - 1) // bm
        live = F.pad(data, (0, tiles * bm - m)).view(tiles, bm).any(1).repeat_interleave(bm)[:m]  # rows of the M tiles that hold a data row
        assert bool((~live).any()) and bool((live & ~data).any())
        g2, r2 = got.view(m, cout), ref.view(m, cout)
        _assert_same(g2[live], r2[live], ref64.view(m, cout)[live], "rows of the tiles with a data row")
        assert bool((g2[~live] == SENTINEL).all()), f"{int((g2[~live] != SENTINEL).any(1).sum())} rows of tiles without a data row were written"
    else:
        _assert_same(got, ref, ref64, _cid((key, e)))
    return ref64


def _saw_big_odd(ref64, dt_out, K):
    lim = {F16: 2048, BF16: 256}.get(dt_out)
    if lim is not None and 2 * K >= lim:  # (2.25 K on average in the hot block)
        assert bool(((ref64.abs() > lim) & (torch.remainder(ref64, 2) == 1)).any()), f"no odd result above {lim}: the rounding to even is not exercised"


# ------------------------------------------------------------------------------------------------------------------------------
# 3. exact runs (integer data), the whole tensor
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_exact(osr, ops, case, dt):
    key, e = case
    ref64 = _exact(ops, osr, key, e, dt, 1000 + zlib.crc32(_cid(case).encode()) % 1000)
    _saw_big_odd(ref64, F32 if e[7] == F32 else dt, e[2][1] * e[2][2] * e[2][3])


def _one_per_tile():
    """The first case of every tile with K >= 512 (and no row segments: the whole tensor is compared)."""
    seen, out = set(), []
    for key, e in CASES:
        if key[0] not in seen and e[8] is None and e[7] != F32 and e[2][1] * e[2][2] * e[2][3] >= 512:
            seen.add(key[0])
            out.append((key, e))
    return out


def test_one_overflow_case_per_tile():
    assert {k[0] for k, _ in _one_per_tile()} == {"128x128/1", "128x128/2", "128x64/1", "128x64/2", "128x256/1", "256x128/1", "256x256/2"}


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", _one_per_tile(), ids=_cid)
def test_exact_overflows_to_inf(osr, ops, case, dt):
    """Weights x 64: exact products, fp32 sums < 2^24; fp16 results past 65504 must be +-Inf as .half() makes them, not 65504; bf16
    results round to 8 significant bits at magnitudes up to ~3e6."""
    key, e = case
    ref64 = _exact(ops, osr, key, e, dt, 77, scale=64.0)
    if dt == F16:
        assert bool((ref64.abs() > 65520).any()), "no result past fp16's range"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cc", CONC_CASES, ids=lambda c: f"{c[0]}-{_short(c[4][0])}")
def test_concurrency_hint_changes_the_tile_not_the_result(osr, ops, cc, dt):
    """include/osr.h: the concurrency hint selects the tile, "results do not depend on it": exact against fp64 at both hints."""
    gname, k, tile1, tilek, e = cc
    n, H, W, streams = GEOMS[gname]
    full = next(t for t in forward_table(n, H, W, streams) if _short(t[0]) == e[0])
    assert describe(osr, full[:9] + (1,)).split(" ")[0] != describe(osr, full[:9] + (k,)).split(" ")[0], f"{full[0]} of {gname} no longer changes its tile with the hint"
    k1, kk = plan_key(osr, e[:9] + (1,)), plan_key(osr, e[:9] + (k,))
    assert (k1[0], kk[0]) == (tile1, tilek), (k1, kk)
    _exact(ops, osr, k1, e, dt, 500, conc=1)
    _exact(ops, osr, kk, e, dt, 500, conc=k)


def test_no_layer_of_the_small_geometry_changes_its_tile(osr):
    n, H, W, streams = GEOMS["b2_256x352"]
    for e in forward_table(n, H, W, streams):
        for k in (2, 4):
            assert describe(osr, e[:9] + (1,)).split(" ")[0] == describe(osr, e[:9] + (k,)).split(" ")[0], (e[0], k)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. float runs (random data): rounding against sum|terms|
# ------------------------------------------------------------------------------------------------------------------------------
def _half_ulp(v, dt):
    if dt == torch.float32:
        return torch.zeros_like(v)
    bits = 11 if dt == F16 else 8
    return torch.maximum(v.abs() * 2.0 ** -bits, torch.full_like(v, 2.0 ** -25 if dt == F16 else 0.0))


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_float_vs_fp64(osr, ops, case, dt):
    key, e = case
    g = torch.Generator(device=DEV).manual_seed(3000 + zlib.crc32(_cid(case).encode()) % 1000)
    x, w, b, res = _inputs(e, dt, g, False)
    odt = F32 if e[7] == F32 else dt
    cout, kh, kw, cin = e[2]
    counts = None if e[8] is None else _seg_counts(e, tile_of(key)[0])
    got = _run(ops, e, dt, x, w, b, res, counts=counts)
    ref, S = expect(e, x, w, b, res), expect(e, x, w, b, res, absolute=True)
    torch.cuda.synchronize()
    got = got.double()
    if counts is not None:  # the data rows
        sr = e[8][1]
        data = torch.zeros(e[1][1], dtype=torch.bool, device=DEV)
        for s, c in enumerate(counts):
            data[s * sr:s * sr + c] = True
        got, ref, S = got.view(-1, cout)[data], ref.view(-1, cout)[data], S.view(-1, cout)[data]
    chain = kh * kw * cin
    tol = (chain + 2) * 2.0 ** -24 * S + _half_ulp(ref, odt)
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all())
    ratio = float((err / tol.clamp(min=1e-300)).max())
    print(f"[err] {_cid(case)}: max |err| {err.max().item():.3e}, max |err| / bound {ratio:.3e} (chain {chain})")
    assert ratio <= 1.0, f"{_cid(case)}: |err| / bound {ratio:.3e} > 1"
