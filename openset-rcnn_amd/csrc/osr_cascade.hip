// [d2] CascadeROIHeads: what sits between the stages (osr_cascade_refine). The S-stage inference tail in front of the NMS,
// osr_cascade_candidates, is cand_kernel of osr_det_tail.hip. It works on the stock engine's fixed-capacity row lists: m = n x seg_rows
// rows, row r belongs to image r / seg_rows and exists iff batch_idx[r] >= 0. No compaction, no atomics, no host sync; every sum is
// taken in a fixed order, so a repeat is bit-identical. Built without FMA contraction, like osr_det_tail.hip: the decode of
// osr_boxes.h rounds alike in both.
//
// Launch shape: a latency-bound glue kernel (a few hundred to two thousand rows per image, tens of flops per row and ground-truth
// box). One workgroup per image, one thread per row and pass; the image's ground truth sits in LDS (16-byte boxes), the rows are read
// and written as float4. The per-image counts are integer sums over the workgroup: wave shuffles, then the wave partials in wave
// order by one thread.
//
// gmax is bounded by the static LDS table of the image's ground truth: CR_MAX_GT = 1024 boxes (16 KB) + their classes (8 KB), far
// above what a COCO / LVIS image carries; a larger gmax is refused with OSR_ERR_INVALID_ARG.
#include "osr_common.h"
#include "osr_boxes.h"

#define CR_MAX_GT 1024
#define CR_THREADS 256

__device__ __forceinline__ int cr_wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(CR_THREADS) void cascade_refine_kernel(const float* __restrict__ boxes, const int* __restrict__ batch_idx,
                                                                    const float* __restrict__ deltas, int seg_rows,
                                                                    const int* __restrict__ image_hw, float4 rw, int drop_empty,
                                                                    const float* __restrict__ gt, const long long* __restrict__ gt_classes,
                                                                    const int* __restrict__ gt_count, int gmax, int num_classes, float iou_thr,
                                                                    float* __restrict__ boxes_out, int* __restrict__ bidx_out,
                                                                    long long* __restrict__ cls_out, float* __restrict__ gt_out,
                                                                    int* __restrict__ gidx_out, int* __restrict__ counts) {
    __shared__ float4 s_gt[CR_MAX_GT];
    __shared__ long long s_cls[CR_MAX_GT];
    __shared__ int s_part[3][CR_THREADS / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const bool match = gt != nullptr;
    int G = 0;
    if (match) {
        G = min(max(gt_count[img], 0), gmax);
        for (int g = tid; g < G; g += CR_THREADS) {
            s_gt[g] = *reinterpret_cast<const float4*>(gt + ((long long)img * gmax + g) * 4);
            s_cls[g] = gt_classes[(long long)img * gmax + g];
        }
        __syncthreads();
    }
    const float ih = (float)image_hw[img * 2], iw = (float)image_hw[img * 2 + 1];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    int rows = 0, nfg = 0, nbg = 0;
    for (int j = tid; j < seg_rows; j += CR_THREADS) {
        const long long r = (long long)img * seg_rows + j;
        bool exists = batch_idx[r] >= 0;
        float4 b = zero;
        if (exists) {
            const float4 s = *reinterpret_cast<const float4*>(boxes + r * 4);
            const float4 d4 = *reinterpret_cast<const float4*>(deltas + r * 4);
            // a box that is not valid is handed on as torch computes it, its NaN kept through the clip: without drop_empty every row stays
            bool valid;
            b = osr_box_clip<true>(osr_b2b_decode(s, d4, rw, &valid), iw, ih);
            // [d2] Boxes.nonempty: width > 0 and height > 0 (false for a NaN)
            if (drop_empty && !((b.z - b.x) > 0.f && (b.w - b.y) > 0.f)) { exists = false; b = zero; }
        }
        *reinterpret_cast<float4*>(boxes_out + r * 4) = b;
        bidx_out[r] = exists ? img : -1;
        rows += exists;
        if (match) {
            long long cls = -1;
            int gi = -1;
            float4 mg = zero;
            if (exists) {
                float best = 0.f;
                int bi = 0;
                for (int g = 0; g < G; ++g) {
                    float v = osr_pairwise_iou(s_gt[g], b);
                    v = v == v ? v : 0.f;                          // (a NaN box -- kept only without drop_empty -- overlaps nothing)
                    if (g == 0 || v > best) { best = v; bi = g; }  // the lowest index among equal IoUs
                }
                const bool fg = G > 0 && best >= iou_thr;  // [d2] Matcher([thr], [0, 1]), no low-quality matches
                cls = fg ? s_cls[bi] : (long long)num_classes;
                gi = fg ? bi : -1;
                if (G > 0) mg = s_gt[bi];  // (also on background rows, as [d2] indexes gt_boxes[matched_idxs])
                nfg += fg; nbg += !fg;
            }
            cls_out[r] = cls;
            gidx_out[r] = gi;
            *reinterpret_cast<float4*>(gt_out + r * 4) = mg;
        }
    }
    rows = cr_wave_sum_int(rows); nfg = cr_wave_sum_int(nfg); nbg = cr_wave_sum_int(nbg);
    if ((tid & 63) == 0) { s_part[0][tid >> 6] = rows; s_part[1][tid >> 6] = nfg; s_part[2][tid >> 6] = nbg; }
    __syncthreads();
    if (tid < 3) {
        int t = 0;
        for (int w = 0; w < CR_THREADS / 64; ++w) t += s_part[tid][w];
        counts[img * 3 + tid] = t;
    }
}

extern "C" osr_status osr_cascade_refine(const float* boxes, const int32_t* batch_idx, const float* deltas, int32_t n, int32_t seg_rows,
                                         const int32_t* image_hw, const float reg_weights[4], int32_t drop_empty, const float* gt_boxes,
                                         const int64_t* gt_classes, const int32_t* gt_count, int32_t gmax, int32_t num_classes, float iou_thr,
                                         float* boxes_out, int32_t* batch_idx_out, int64_t* classes_out, float* gt_boxes_out, int32_t* gt_idx_out,
                                         int32_t* counts, void* stream) {
    OSR_REQUIRE(boxes && batch_idx && deltas && image_hw && reg_weights && boxes_out && batch_idx_out && counts, OSR_ERR_INVALID_ARG,
                "osr_cascade_refine: null pointer");
    OSR_REQUIRE(n >= 1 && seg_rows >= 1 && (int64_t)n * seg_rows < (1ll << 30), OSR_ERR_INVALID_ARG, "osr_cascade_refine: bad sizes");
    OSR_REQUIRE(reg_weights[0] > 0.f && reg_weights[1] > 0.f && reg_weights[2] > 0.f && reg_weights[3] > 0.f, OSR_ERR_INVALID_ARG,
                "osr_cascade_refine: regression weights must be positive");
    if (gt_boxes) {
        OSR_REQUIRE(gt_classes && gt_count && classes_out && gt_boxes_out && gt_idx_out, OSR_ERR_INVALID_ARG,
                    "osr_cascade_refine: ground truth needs gt_classes, gt_count and the three matching outputs");
        OSR_REQUIRE(gmax >= 1 && gmax <= CR_MAX_GT, OSR_ERR_INVALID_ARG, "osr_cascade_refine: gmax must be in 1..%d (the LDS table of an image's ground truth)",
                    CR_MAX_GT);
        OSR_REQUIRE(num_classes >= 1, OSR_ERR_INVALID_ARG, "osr_cascade_refine: bad num_classes");
        OSR_REQUIRE((((uintptr_t)gt_boxes | (uintptr_t)gt_boxes_out) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_cascade_refine: box arrays must be 16-byte aligned");
    }
    OSR_REQUIRE((((uintptr_t)boxes | (uintptr_t)deltas | (uintptr_t)boxes_out) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_cascade_refine: box arrays must be 16-byte aligned");
    hipLaunchKernelGGL(cascade_refine_kernel, dim3(n), dim3(CR_THREADS), 0, (hipStream_t)stream, boxes, batch_idx, deltas, seg_rows, image_hw,
                       make_float4(reg_weights[0], reg_weights[1], reg_weights[2], reg_weights[3]), drop_empty ? 1 : 0, gt_boxes,
                       (const long long*)gt_classes, gt_count, gmax, num_classes, iou_thr, boxes_out, batch_idx_out, (long long*)classes_out,
                       gt_boxes_out, gt_idx_out, counts);
    OSR_CHECK_LAUNCH("osr_cascade_refine");
    return OSR_OK;
}
