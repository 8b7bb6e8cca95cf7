"""Parameter handling for the HIP path: detectron2-compatible state-dict names (checkpoint row),
FrozenBatchNorm folding, and the one-time repacking of weights into the layouts the kernels read.

No checkpoint is reachable offline, so ``random_params`` builds a seeded synthetic parameter set with the
reference's parameter names and shapes (He-style init scaled so that activations stay inside fp16 range)."""
from __future__ import annotations

import math
from typing import Dict

import torch

R50_BLOCKS = (3, 4, 6, 3)
R50_MID = (64, 128, 256, 512)


def fold_frozen_bn(state: Dict[str, torch.Tensor], eps: float = 1e-5) -> Dict[str, torch.Tensor]:
    """[d2] FrozenBatchNorm2d (y = x*w*rsqrt(var+eps) + (b - mean*w*rsqrt(var+eps))) folded into the preceding
    bias-free conv: '<conv>.norm.{weight,bias,running_mean,running_var}' keys are consumed and '<conv>.bias' produced."""
    out = dict(state)
    for k in list(state.keys()):
        if k.endswith(".norm.weight"):
            pre = k[: -len(".norm.weight")]
            if pre + ".norm.running_mean" not in state:
                continue  # (a GroupNorm: sem_seg_head.*.norm has no running statistics and is not folded)
            w, b = state[pre + ".norm.weight"], state[pre + ".norm.bias"]
            mean, var = state[pre + ".norm.running_mean"], state[pre + ".norm.running_var"]
            scale = w * (var + eps).rsqrt()
            out[pre + ".weight"] = state[pre + ".weight"] * scale.view(-1, 1, 1, 1)
            out[pre + ".bias"] = b - mean * scale
            for s in ("weight", "bias", "running_mean", "running_var"):
                out.pop(pre + ".norm." + s, None)
    return out


def deform_offset_params(deform_on_per_stage, modulated: bool = False, groups: int = 1, std: float = 0.0, seed: int = 0) -> Dict[str, torch.Tensor]:
    """`conv2_offset.{weight,bias}` of every block of the deformable stages (MODEL.RESNETS.DEFORM_ON_PER_STAGE, res2..res5) under
    detectron2's names: weight ((27 if modulated else 18) * groups, mid, 3, 3) and bias. std 0: zeros, [d2]'s initialisation (the layer
    then samples on the regular grid); std > 0: seeded normal weights and biases, scaled by the fan-in so that a unit-variance input
    gives offsets of about `std` pixels."""
    g = torch.Generator().manual_seed(seed + 3000)
    p: Dict[str, torch.Tensor] = {}
    ch = (27 if modulated else 18) * groups
    for si, (nb, mid) in enumerate(zip(R50_BLOCKS, R50_MID)):
        for b in range(nb if deform_on_per_stage[si] else 0):
            pre = f"backbone.bottom_up.res{si + 2}.{b}.conv2_offset"
            p[pre + ".weight"] = torch.randn(ch, mid, 3, 3, generator=g) * (std / math.sqrt(9.0 * mid)) if std else torch.zeros(ch, mid, 3, 3)
            p[pre + ".bias"] = torch.randn(ch, generator=g) * (0.5 * std) if std else torch.zeros(ch)
    return p


def random_params(seed: int = 0, num_known: int = 20, fc_dim: int = 1024, emd: int = 256, res_gain: float = 0.5,
                  spread: bool = True, deform_on_per_stage=(False, False, False, False), deform_modulated: bool = False,
                  deform_num_groups: int = 1, deform_std: float = 0.0) -> Dict[str, torch.Tensor]:
    """Seeded synthetic parameters (already BN-folded) for R50-FPN + CF-RPN head + Openset RoI heads; with deformable stages also
    their deform_offset_params (every other tensor is what the same seed gives without them)."""
    g = torch.Generator().manual_seed(seed)
    p: Dict[str, torch.Tensor] = deform_offset_params(deform_on_per_stage, deform_modulated, deform_num_groups, deform_std, seed)

    def conv(name, cout, cin, k, gain=1.0, bias_std=0.05):
        std = gain * math.sqrt(2.0 / (cout * k * k))
        p[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * std
        p[name + ".bias"] = torch.randn(cout, generator=g) * bias_std

    conv("backbone.bottom_up.stem.conv1", 64, 3, 7, gain=0.02)
    cin = 64
    for si, (nb, mid) in enumerate(zip(R50_BLOCKS, R50_MID)):
        cout = mid * 4
        for b in range(nb):
            pre = f"backbone.bottom_up.res{si + 2}.{b}"
            if b == 0:
                conv(pre + ".shortcut", cout, cin, 1, gain=0.7)
            conv(pre + ".conv1", mid, cin, 1)
            conv(pre + ".conv2", mid, mid, 3)
            conv(pre + ".conv3", cout, mid, 1, gain=res_gain)
            cin = cout
    for lvl, c in zip((2, 3, 4, 5), (256, 512, 1024, 2048)):
        conv(f"backbone.fpn_lateral{lvl}", 256, c, 1, gain=0.7)
        conv(f"backbone.fpn_output{lvl}", 256, 256, 3, gain=0.7)

    g2 = torch.Generator().manual_seed(seed + 1000)
    m = 30.0 if spread else 1.0

    def lin(name, o, i, std, bstd=0.0):
        p[name + ".weight"] = torch.randn(o, i, generator=g2) * std
        p[name + ".bias"] = torch.randn(o, generator=g2) * bstd if bstd else torch.zeros(o)

    in_dim = 256 * 49
    p["proposal_generator.rpn_head.conv.weight"] = torch.randn(256, 256, 3, 3, generator=g2) * 0.01 * (2 if spread else 1)
    p["proposal_generator.rpn_head.conv.bias"] = torch.zeros(256)
    p["proposal_generator.rpn_head.anchor_deltas.weight"] = torch.randn(4, 256, 1, 1, generator=g2) * 0.01 * m * 3
    p["proposal_generator.rpn_head.anchor_deltas.bias"] = torch.full((4,), 0.5 if spread else 0.0)
    p["proposal_generator.rpn_head.centerness.weight"] = torch.randn(1, 256, 1, 1, generator=g2) * 0.01 * m * 10
    p["proposal_generator.rpn_head.centerness.bias"] = torch.zeros(1)
    lin("roi_heads.box_head.fc1", fc_dim, in_dim, math.sqrt(2.0 / in_dim), 0.02)
    lin("roi_heads.box_head.fc2", fc_dim, fc_dim, math.sqrt(2.0 / fc_dim), 0.02)
    lin("roi_heads.box_predictor.bbox_pred", 4, fc_dim, 0.001 * m)
    lin("roi_heads.box_predictor.iou_pred", 1, fc_dim, 0.01 * (m / 3))
    lin("roi_heads.dml.encoder", emd, fc_dim, 0.01 * (m / 6))
    lin("roi_heads.dml.decoder", fc_dim, emd, 0.01 * (m / 6))
    p["roi_heads.dml.representatives"] = torch.randn(num_known, emd, generator=g2)
    lin("roi_heads.softmaxcls.cls_score", num_known + 1, fc_dim, 0.01 * (m / 3))
    return p


def pack_conv_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(cout,cin,kh,kw) -> (cout,kh,kw,cin): the GEMM K axis becomes contiguous per tap."""
    return w.permute(0, 2, 3, 1).contiguous().to(dtype)


def pack_stem_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(64,3,7,7) -> stem view (64,8,1,32): K slice kh holds 8 taps x 4 channels of one image row; the 8th tap,
    the 4th channel and the whole 8th row are zero (the row pads K to a multiple of 64 for the BK=64 kernel)."""
    cout = w.shape[0]
    v = torch.zeros(cout, 8, 8, 4, dtype=torch.float32)
    v[:, :7, :7, :3] = w.float().permute(0, 2, 3, 1)
    return v.view(cout, 8, 1, 32).contiguous().to(dtype)


def pack_fc1_weight(w: torch.Tensor, channels: int, pooled: int, dtype: torch.dtype) -> torch.Tensor:
    """fc1 (out, c*p*p) with the reference's (c,ph,pw) flatten order -> (out, p*p*c) matching RoIAlign's (ph,pw,c) output."""
    o = w.shape[0]
    return w.view(o, channels, pooled, pooled).permute(0, 2, 3, 1).reshape(o, pooled * pooled * channels).contiguous().to(dtype)


def pack_deconv_weight(w: torch.Tensor, dtype: torch.dtype, frag_elems: int = 0) -> torch.Tensor:
    """[d2] MaskRCNNConvUpsampleHead.deconv weight (cin, cmid, 2, 2) -> the B operand of ops.mask_upsample_predict (include/osr.h
    osr_mask_upsample_predict): one (cmid, cin) matrix per tap t = 2 dy + dx, cut into the MFMA fragments a wave loads -- blocks of 32
    output channels x 2E input channels, E = 8 (fp16 / bf16) or 4 (fp32), laid out [t][n / 32][k / 2E][(k / E) % 2][n % 32][k % E] so
    that the 64 lanes of a wave read one contiguous block. cin and cmid must be multiples of 64. frag_elems: E whatever the dtype
    (the trainer keeps its fp32 master and gradient in the fp16 / bf16 kernels' order, E = 8). The backward's second operand
    (ops.mask_upsample_predict_bwd w_packed_t) is this function on weight.transpose(0, 1)."""
    cin, cmid, kh, kw = w.shape
    if (kh, kw) != (2, 2) or cin % 64 or cmid % 64:
        raise ValueError(f"deconv weight {tuple(w.shape)}: (cin, cmid, 2, 2) with cin and cmid multiples of 64")
    e = frag_elems or (4 if dtype == torch.float32 else 8)
    wt = w.detach().permute(2, 3, 1, 0).reshape(4, cmid // 32, 32, cin // (2 * e), 2, e)  # [t][n / 32][n % 32][k / 2E][half][k % E]
    return wt.permute(0, 1, 3, 4, 2, 5).contiguous().to(dtype)


def unpack_deconv_weight(p: torch.Tensor) -> torch.Tensor:
    """The inverse of pack_deconv_weight: fragments (4, cmid / 32, cin / 2E, 2, 32, E) -> (cin, cmid, 2, 2), same dtype."""
    _, nb, kb, _, _, e = p.shape
    cmid, cin = nb * 32, kb * 2 * e
    return p.permute(0, 1, 4, 2, 3, 5).reshape(2, 2, cmid, cin).permute(3, 2, 0, 1).contiguous()


def pack_keypoint_deconv_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[d2] KRCNNConvDeconvUpsampleHead.score_lowres weight (cin, k, 4, 4) -> the B operand of ops.keypoint_upsample (include/osr.h
    osr_keypoint_upsample): one (32, cin) matrix per tap ky * 4 + kx -- the k keypoints padded with zero rows to the MFMA's N = 32 --
    cut into the fragments a wave loads: blocks of 2E input channels, E = 8 (fp16 / bf16) or 4 (fp32), laid out
    [ky * 4 + kx][c / 2E][(c / E) % 2][j][c % E], so that the 64 lanes of a wave read one contiguous block. cin a multiple of 64,
    k 1 .. 32."""
    cin, k, kh, kw = w.shape
    if (kh, kw) != (4, 4) or cin % 64 or not 1 <= k <= 32:
        raise ValueError(f"score_lowres weight {tuple(w.shape)}: (cin, k, 4, 4) with cin a multiple of 64 and k in 1 .. 32")
    e = 4 if dtype == torch.float32 else 8
    wt = torch.zeros((16, 32, cin), dtype=w.dtype)
    wt[:, :k] = w.detach().cpu().permute(2, 3, 1, 0).reshape(16, k, cin)
    wt = wt.reshape(16, 32, cin // (2 * e), 2, e)  # [tap][j][c / 2E][half][c % E]
    return wt.permute(0, 2, 3, 1, 4).contiguous().to(dtype)


def split_fp32_rows(w: torch.Tensor):
    """The operand format of the split-precision box head (ops.linear_split, include/osr.h osr_linear_split_fwd): an fp32 matrix as
    two bf16 planes, w = hi + lo to 2^-17 of each element's magnitude, hi = bf16(w), lo = bf16(w - hi), both rounded to nearest
    even (w - hi is exact in fp32). Returns (hi, lo, exp); exp is None: bf16 carries fp32's exponent range, so rows need no
    power-of-two scaling and there is no exponent to clamp -- a row of zeros, a row at 1e-30 and a row at 1e30 split like any
    other (a value beyond bf16's largest, about 3.39e38, would round hi to Inf)."""
    w = w.detach().to(torch.float32).contiguous()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo, None


def split_fp32_rows_t(w: torch.Tensor):
    """split_fp32_rows of the transpose: (rows, cols) fp32 -> the planes (cols, rows) that the split-precision data gradient reads
    (ops.linear_split_dgrad; ops.split_rows_bf16_t gives the same bits on the GPU). Returns (hi, lo, None)."""
    return split_fp32_rows(w.detach().to(torch.float32).t().contiguous())


def _split_packed(packed: torch.Tensor):
    hi, lo, _ = split_fp32_rows(packed.view(packed.shape[0], -1))
    return hi.view(packed.shape), lo.view(packed.shape)


def split_conv_weight(w: torch.Tensor):
    """The weight operand of the split-precision convolution (ops.conv2d_split, include/osr.h osr_conv2d_split_fwd):
    (cout,cin,kh,kw) -> pack_conv_weight in fp32 -> split_fp32_rows of its (cout, kh*kw*cin) rows. Returns (hi, lo), two bf16
    tensors shaped (cout,kh,kw,cin)."""
    return _split_packed(pack_conv_weight(w, torch.float32))


def split_stem_weight(w: torch.Tensor):
    """split_conv_weight for the stem: (64,3,7,7) -> pack_stem_weight in fp32 -> (hi, lo), bf16, shaped (64,8,1,32). The zero taps of
    the view (8th tap, 4th channel, 8th row) are zero in both planes."""
    return _split_packed(pack_stem_weight(w, torch.float32))


def pack_dgrad_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(cout,cin,kh,kw) -> (cin,kh,kw,cout), spatially flipped: the backward-data pass of a stride-1 convolution is the
    forward convolution of dy with these weights and padding k-1-pad; for a 1x1 layer it is the transposed matrix."""
    return w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(dtype)


def with_known_unknown_mix(params: Dict[str, torch.Tensor], embeddings: torch.Tensor, unk_thr: float = 0.23, known_fraction: float = 0.5,
                           proto: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic-weights helper (benchmarks / tests; no checkpoint is reachable offline). Random prototypes put every embedding
    ~0.85-1.0 away from all of them, so PLN.inference (prototype_learning_network.py:213-223) calls every detection "unknown" and
    the known-class leg (softmax over <= 20 000 candidates, per-class NMS) idles. This returns a copy of `params` whose PLN
    encoder bias is c * P_hat[proto]: with emb = W f + b, cos(emb, P_hat) = c / sqrt(c^2 + |W f|^2) (W f is nearly orthogonal to
    one fixed direction of 256), so the detections whose |W f| is below c * sqrt(1 / (1 - unk_thr)^2 - 1) become known. `c` is
    set from the `known_fraction` quantile of |embeddings| (rows = embeddings of a run with zero encoder bias, valid rows only).
    UNK_THR itself stays the yaml's value."""
    out = dict(params)
    p = params["roi_heads.dml.representatives"].float()
    ph = p[proto] / p[proto].norm().clamp(min=1e-12)
    norms = embeddings.detach().float().cpu().norm(dim=1)
    q = float(torch.quantile(norms, known_fraction))
    cos_thr = 1.0 - unk_thr
    c = q / math.sqrt(1.0 / (cos_thr * cos_thr) - 1.0)
    out["roi_heads.dml.encoder.bias"] = (c * ph).contiguous()
    return out


def random_standard_params(seed: int = 0, num_classes: int = 80, num_anchors: int = 3, cls_agnostic: bool = True, fc_dim: int = 1024) -> Dict[str, torch.Tensor]:
    """Seeded synthetic parameters (BN-folded backbone of random_params + the stock detectron2 heads of Base-RCNN-FPN.yaml):
    StandardRPNHead (conv, objectness_logits (A), anchor_deltas (4A)) and FastRCNNOutputLayers (cls_score (K+1), bbox_pred (4 or
    4K)), scaled so that logits and deltas spread (the [d2] initialisers, std 0.01 / 0.001, give near-constant outputs and
    degenerate top-k / NMS ties)."""
    p = {k: v for k, v in random_params(seed).items() if k.startswith("backbone.")}
    g = torch.Generator().manual_seed(seed + 2000)
    p["proposal_generator.rpn_head.conv.weight"] = torch.randn(256, 256, 3, 3, generator=g) * 0.02
    p["proposal_generator.rpn_head.conv.bias"] = torch.zeros(256)
    p["proposal_generator.rpn_head.objectness_logits.weight"] = torch.randn(num_anchors, 256, 1, 1, generator=g) * 0.5
    p["proposal_generator.rpn_head.objectness_logits.bias"] = torch.zeros(num_anchors)
    p["proposal_generator.rpn_head.anchor_deltas.weight"] = torch.randn(num_anchors * 4, 256, 1, 1, generator=g) * 0.1
    p["proposal_generator.rpn_head.anchor_deltas.bias"] = torch.zeros(num_anchors * 4)
    in_dim = 256 * 49
    p["roi_heads.box_head.fc1.weight"] = torch.randn(fc_dim, in_dim, generator=g) * math.sqrt(2.0 / in_dim)
    p["roi_heads.box_head.fc1.bias"] = torch.randn(fc_dim, generator=g) * 0.02
    p["roi_heads.box_head.fc2.weight"] = torch.randn(fc_dim, fc_dim, generator=g) * math.sqrt(2.0 / fc_dim)
    p["roi_heads.box_head.fc2.bias"] = torch.randn(fc_dim, generator=g) * 0.02
    p["roi_heads.box_predictor.cls_score.weight"] = torch.randn(num_classes + 1, fc_dim, generator=g) * 0.15
    p["roi_heads.box_predictor.cls_score.bias"] = torch.zeros(num_classes + 1)
    p["roi_heads.box_predictor.bbox_pred.weight"] = torch.randn(4 if cls_agnostic else 4 * num_classes, fc_dim, generator=g) * 0.03
    p["roi_heads.box_predictor.bbox_pred.bias"] = torch.zeros(4 if cls_agnostic else 4 * num_classes)
    return p


def random_c4_params(seed: int = 0, num_classes: int = 80, num_anchors: int = 15, cls_agnostic: bool = False) -> Dict[str, torch.Tensor]:
    """Seeded synthetic parameters for [d2] faster_rcnn_R_50_C4 under its names: random_params' BN-folded trunk with stem and res2..res4
    under backbone.* (no `bottom_up`) and res5 under roi_heads.res5.*, a StandardRPNHead on res4's 1024 channels (conv 1024 -> 1024,
    objectness_logits (A), anchor_deltas (4A)) and FastRCNNOutputLayers on res5's 2048 means, scaled so that logits and deltas spread."""
    p = {}
    for k, v in random_params(seed).items():
        if k.startswith("backbone.bottom_up.res5."):
            p["roi_heads.res5." + k[len("backbone.bottom_up.res5."):]] = v
        elif k.startswith("backbone.bottom_up."):
            p["backbone." + k[len("backbone.bottom_up."):]] = v
    g = torch.Generator().manual_seed(seed + 4000)
    rpn = "proposal_generator.rpn_head."
    p[rpn + "conv.weight"] = torch.randn(1024, 1024, 3, 3, generator=g) * 0.01
    p[rpn + "conv.bias"] = torch.zeros(1024)
    p[rpn + "objectness_logits.weight"] = torch.randn(num_anchors, 1024, 1, 1, generator=g) * 0.25
    p[rpn + "objectness_logits.bias"] = torch.zeros(num_anchors)
    p[rpn + "anchor_deltas.weight"] = torch.randn(num_anchors * 4, 1024, 1, 1, generator=g) * 0.05
    p[rpn + "anchor_deltas.bias"] = torch.zeros(num_anchors * 4)
    rows = 4 if cls_agnostic else 4 * num_classes
    p["roi_heads.box_predictor.cls_score.weight"] = torch.randn(num_classes + 1, 2048, generator=g) * 0.1
    p["roi_heads.box_predictor.cls_score.bias"] = torch.zeros(num_classes + 1)
    p["roi_heads.box_predictor.bbox_pred.weight"] = torch.randn(rows, 2048, generator=g) * 0.02
    p["roi_heads.box_predictor.bbox_pred.bias"] = torch.zeros(rows)
    return p


def random_cascade_params(seed: int = 0, stages: int = 3, num_classes: int = 80, num_anchors: int = 3, fc_dim: int = 1024) -> Dict[str, torch.Tensor]:
    """random_standard_params with [d2] CascadeROIHeads' box stages: roi_heads.box_head.{s}.* and roi_heads.box_predictor.{s}.* for
    s < stages (class-agnostic bbox_pred). Stage 0 carries random_standard_params(seed)'s box head and output layers, stage s > 0
    those of seed + 100 s, so a one-stage cascade computes what the stock heads compute."""
    p = {}
    for s in range(stages):
        for k, v in random_standard_params(seed + 100 * s, num_classes, num_anchors, True, fc_dim).items():
            if k.startswith("roi_heads.box_head."):
                p[f"roi_heads.box_head.{s}." + k[len("roi_heads.box_head."):]] = v
            elif k.startswith("roi_heads.box_predictor."):
                p[f"roi_heads.box_predictor.{s}." + k[len("roi_heads.box_predictor."):]] = v
            elif s == 0:
                p[k] = v
    return p


def random_retinanet_params(seed: int = 0, num_classes: int = 80, num_anchors: int = 9, num_convs: int = 4, cls_bias: float = -4.595) -> Dict[str, torch.Tensor]:
    """Seeded synthetic parameters for META_ARCHITECTURE "RetinaNet": random_params' BN-folded trunk with the FPN on res3..res5 only,
    [d2] LastLevelP6P7 (backbone.top_block.p6 from res5, .p7) and RetinaNetHead (cls_subnet / bbox_subnet .{0,2,..}, cls_score,
    bbox_pred), scaled so that the towers keep their input's scale and logits and deltas spread (the [d2] initialiser, std 0.01, gives
    near-constant outputs). cls_bias: cls_score's bias (-4.595 = [d2]'s PRIOR_PROB 0.01)."""
    p = {k: v for k, v in random_params(seed).items() if k.startswith("backbone.") and not k.startswith(("backbone.fpn_lateral2.", "backbone.fpn_output2."))}
    g = torch.Generator().manual_seed(seed + 3000)

    def conv(name, cout, cin, std, bias=0.0, bias_std=0.02):
        p[name + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * std
        p[name + ".bias"] = torch.randn(cout, generator=g) * bias_std + bias

    conv("backbone.top_block.p6", 256, 2048, 0.7 * math.sqrt(2.0 / (256 * 9)))
    conv("backbone.top_block.p7", 256, 256, 0.7 * math.sqrt(2.0 / (256 * 9)))
    for sub in ("cls_subnet", "bbox_subnet"):
        for i in range(num_convs):
            conv(f"head.{sub}.{2 * i}", 256, 256, math.sqrt(2.0 / (256 * 9)))
    conv("head.cls_score", num_anchors * num_classes, 256, 0.02, bias=cls_bias, bias_std=0.0)
    conv("head.bbox_pred", num_anchors * 4, 256, 0.004, bias_std=0.0)
    return p


SEM_SEG_FEATURES = (("p2", 4), ("p3", 8), ("p4", 16), ("p5", 32))


def sem_seg_head_lengths(common_stride: int = 4) -> Dict[str, int]:
    """[d2] SemSegFPNHead: head_length = max(1, log2(stride) - log2(COMMON_STRIDE)) 3x3 convolutions per input feature."""
    return {f: max(1, int(math.log2(s)) - int(math.log2(common_stride))) for f, s in SEM_SEG_FEATURES}


def random_panoptic_params(seed: int = 0, num_classes: int = 80, sem_classes: int = 54, convs_dim: int = 128, norm: str = "GN", mask_conv: int = 4,
                           predictor_gain: float = 1.0, rcnn: bool = True) -> Dict[str, torch.Tensor]:
    """Seeded synthetic parameters for META_ARCHITECTURE "PanopticFPN" (rcnn=False: "SemanticSegmentor", the backbone and the semantic
    head only): random_standard_params' detector, He-style MaskRCNNConvUpsampleHead parameters (class-agnostic predictor) and [d2]
    SemSegFPNHead under its names -- sem_seg_head.<feat>.<2k>.weight, with `.norm.weight` / `.norm.bias` (NORM "GN": no conv bias) or
    `.bias` (NORM ""), and sem_seg_head.predictor -- with affine parameters away from (1, 0) and a predictor whose logits spread."""
    base = random_standard_params(seed, num_classes=num_classes)
    p = dict(base) if rcnn else {k: v for k, v in base.items() if k.startswith("backbone.")}
    g = torch.Generator().manual_seed(seed + 5000)
    if rcnn:
        pre, cin = "roi_heads.mask_head.", 256
        for i in range(1, mask_conv + 1):
            p[f"{pre}mask_fcn{i}.weight"] = torch.randn(256, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
            p[f"{pre}mask_fcn{i}.bias"] = torch.randn(256, generator=g) * 0.02
        p[pre + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * math.sqrt(2.0 / 256)
        p[pre + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
        p[pre + "predictor.weight"] = torch.randn(1, 256, 1, 1, generator=g) * 0.5
        p[pre + "predictor.bias"] = torch.zeros(1)
    for feat, length in sem_seg_head_lengths().items():
        cin = 256
        for k in range(length):
            name = f"sem_seg_head.{feat}.{2 * k}"
            p[name + ".weight"] = torch.randn(convs_dim, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
            if norm == "GN":
                p[name + ".norm.weight"] = 1.0 + 0.2 * torch.randn(convs_dim, generator=g)
                p[name + ".norm.bias"] = 0.2 * torch.randn(convs_dim, generator=g)
            else:
                p[name + ".bias"] = torch.randn(convs_dim, generator=g) * 0.05
            cin = convs_dim
    p["sem_seg_head.predictor.weight"] = torch.randn(sem_classes, convs_dim, 1, 1, generator=g) * (predictor_gain / math.sqrt(convs_dim))
    p["sem_seg_head.predictor.bias"] = torch.randn(sem_classes, generator=g) * 0.1
    return p
