// [d2] Box2BoxTransform.apply_deltas, Boxes.clip, pairwise_iou and a pyramid cell's anchor: one definition each for every kernel that
// decodes, clips or matches a box -- the inference tails (osr_det_tail.hip, osr_cascade.hip, osr_rpn.hip, osr_retinanet.hip) and,
// through osr_box_loss.h, the losses.
//
// Header code takes its includer's contraction setting; every inference tail is built with -ffp-contract=off, so the decode rounds
// alike in all of them (and like the oracle's).
#pragma once
#include "osr_common.h"

#define OSR_B2B_SCALE_CLAMP 4.135166556742356f  // log(1000 / 16)

// The one place where the kernels differ from torch: torch.clamp(max=) keeps a NaN, fminf drops it.
//   KEEP_NAN false  fminf: a NaN size delta decodes as the clamp. The training kernels' form (osr_train_fwd.hip, osr_train_bwd.hip,
//                   osr_std_train.hip): their losses and gradients are defined by it, NaN rows included.
//   KEEP_NAN true   torch's rule: the NaN reaches the decoded size, so the box's x (dw) or y (dh) pair is NaN.
template <bool KEEP_NAN>
__device__ __forceinline__ float osr_b2b_clamp(float v) {
    return KEEP_NAN ? (v > OSR_B2B_SCALE_CLAMP ? OSR_B2B_SCALE_CLAMP : v) : fminf(v, OSR_B2B_SCALE_CLAMP);
}

// [d2] Box2BoxTransform.apply_deltas(d, src) with weights (wx, wy, ww, wh). Centre = d/w * size + centre, size = exp(min(d/w, clamp))
// * size; the decoded size also goes to *pw, *ph (the gradient through the exponential needs it, and it is zero where d/w reaches
// the clamp).
template <bool KEEP_NAN = false>
__device__ __forceinline__ float4 osr_b2b_apply_deltas(float4 s, const float* d, float wx, float wy, float ww, float wh, float* pw, float* ph) {
    const float sw = s.z - s.x, sh = s.w - s.y, scx = s.x + 0.5f * sw, scy = s.y + 0.5f * sh;
    *pw = expf(osr_b2b_clamp<KEEP_NAN>(d[2] / ww)) * sw; *ph = expf(osr_b2b_clamp<KEEP_NAN>(d[3] / wh)) * sh;
    const float pcx = d[0] / wx * sw + scx, pcy = d[1] / wy * sh + scy;
    return make_float4(pcx - 0.5f * *pw, pcy - 0.5f * *ph, pcx + 0.5f * *pw, pcy + 0.5f * *ph);
}

__device__ __forceinline__ bool osr_box_finite(float4 b) { return osr_finite(b.x) && osr_finite(b.y) && osr_finite(b.z) && osr_finite(b.w); }

// The inference decode: the box as torch computes it and whether a detection may be made of it. *valid: all four coordinates are
// finite -- which, the NaN being kept, also says that no size delta was NaN ([d2] drops such a row; a clamp that lost the NaN would
// hand on a finite box of the largest size instead).
__device__ __forceinline__ float4 osr_b2b_decode(float4 s, float4 d, float4 rw, bool* valid) {
    const float dd[4] = {d.x, d.y, d.z, d.w};
    float pw, ph;
    const float4 b = osr_b2b_apply_deltas<true>(s, dd, rw.x, rw.y, rw.z, rw.w, &pw, &ph);
    *valid = osr_box_finite(b);
    return b;
}

// [d2] Boxes.clip: x into [0, iw], y into [0, ih]. KEEP_NAN false: fminf / fmaxf, a NaN coordinate becomes 0 (for boxes whose
// validity was settled before the clip); true: clamp(min = 0, max = size) as torch orders it, a NaN stays a NaN.
template <bool KEEP_NAN = false>
__device__ __forceinline__ float osr_clip_coord(float v, float hi) {
    return KEEP_NAN ? (v < 0.f ? 0.f : (v > hi ? hi : v)) : fminf(fmaxf(v, 0.f), hi);
}
template <bool KEEP_NAN = false>
__device__ __forceinline__ float4 osr_box_clip(float4 b, float iw, float ih) {
    return make_float4(osr_clip_coord<KEEP_NAN>(b.x, iw), osr_clip_coord<KEEP_NAN>(b.y, ih), osr_clip_coord<KEEP_NAN>(b.z, iw),
                       osr_clip_coord<KEEP_NAN>(b.w, ih));
}

// [d2] pairwise_iou of two boxes in fp32: inter / (a1 + a2 - inter) where inter > 0, else 0 (the matchers of the RPN, the RoI heads
// and the cascade's stage transitions; built without FMA contraction wherever an index depends on it)
__device__ __forceinline__ float osr_pairwise_iou(const float4 g, const float4 b) {
    const float a1 = (g.z - g.x) * (g.w - g.y), a2 = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(g.z, b.z) - fmaxf(g.x, b.x), 0.f), h = fmaxf(fminf(g.w, b.w) - fmaxf(g.y, b.y), 0.f);
    const float inter = w * h;
    return inter > 0.f ? inter / (a1 + a2 - inter) : 0.f;
}

// [d2] DefaultAnchorGenerator: anchor a of cell `cell` (row-major in a level `w` cells wide) = the cell's shift + the level's cell
// anchor; cell_anchors is (levels, A, 4).
__device__ __forceinline__ float4 osr_cell_anchor(const float* __restrict__ cell_anchors, int level, int A, int a, int cell, int w, float stride) {
    const float sx = (float)(cell % w) * stride, sy = (float)(cell / w) * stride;
    const float* ca = cell_anchors + ((long long)level * A + a) * 4;
    return make_float4(sx + ca[0], sy + ca[1], sx + ca[2], sy + ca[3]);
}
