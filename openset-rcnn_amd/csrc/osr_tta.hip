// Test-time augmentation glue ([d2] modeling/test_time_augmentation.py: GeneralizedRCNNWithTTA._inverse_augment_boxes,
// _rescale_detected_boxes, _reduce_pred_masks) on the device, over the engine's padded detection lists. An augmentation is the
// transform list  [resize (ho, wo) -> (hi, wi)]  resize (hi, wi) -> (ha, wa)  [hflip(wa)]  of a model input whose image is (hi, wi) and
// whose output resolution is (ho, wo). Box arithmetic is [d2]'s, coordinate by coordinate in fp32: a resize multiplies by the ratio
// formed in double and rounded to fp32 once, a flip is wa - x, one rounding per step (this file is built with -ffp-contract=off, so a
// product is never fused into the difference that follows it) -- a numpy fp32 restatement gives the same bits.
// Memory-bound element-wise kernels: one 16-byte box (or four map samples) per thread.
#include "osr_common.h"

#define TTA_SCORE_THRESH 1e-8f  // [d2] GeneralizedRCNNWithTTA._merge_detections: fast_rcnn_inference_single_image(..., 1e-8, ...)

__device__ __forceinline__ float tta_ratio(int num, int den) { return (float)((double)num / (double)den); }

// (n, topk) detections of ONE augmentation -> rows [slot, slot + topk) of each image's candidate list (n, cap)
__global__ __launch_bounds__(256) void tta_boxes_to_original_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                                                                     const int64_t* __restrict__ classes, const int* __restrict__ counts,
                                                                     const int4* __restrict__ sizes, int n, int topk, int ha, int wa, int flip, int slot,
                                                                     int cap, float4* __restrict__ c_boxes, float* __restrict__ c_scores,
                                                                     int* __restrict__ c_cls, int* __restrict__ c_cand) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * topk) return;
    const int img = t / topk, j = t - img * topk;
    const long long o = (long long)img * cap + slot + j;
    if (j >= counts[img]) {
        c_boxes[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        c_scores[o] = 0.f;
        c_cls[o] = -1;
        c_cand[o] = 0;
        return;
    }
    const int4 s = sizes[img];  // hi, wi, ho, wo
    float4 b = boxes[t];
    if (flip) {  // the inverse of the flip is the flip
        const float fw = (float)wa, x0 = fw - b.x, x1 = fw - b.z;
        b.x = x0 < x1 ? x0 : x1; b.z = x0 < x1 ? x1 : x0;  // (a NaN survives in one of the two)
    }
    const float rx = tta_ratio(s.y, wa), ry = tta_ratio(s.x, ha);  // (ha, wa) -> (hi, wi)
    b.x *= rx; b.y *= ry; b.z *= rx; b.w *= ry;
    if (s.z != s.x || s.w != s.y) {  // (hi, wi) -> (ho, wo)
        const float qx = tta_ratio(s.w, s.y), qy = tta_ratio(s.z, s.x);
        b.x *= qx; b.y *= qy; b.z *= qx; b.w *= qy;
    }
    const float sc = scores[t];
    const bool fin = osr_finite(b.x) && osr_finite(b.y) && osr_finite(b.z) && osr_finite(b.w) && osr_finite(sc);
    const float W = (float)s.w, H = (float)s.z;  // [d2] Boxes.clip: clamp(min=0, max=size); a NaN stays a NaN (the row is no candidate)
    b.x = b.x < 0.f ? 0.f : (b.x > W ? W : b.x);
    b.y = b.y < 0.f ? 0.f : (b.y > H ? H : b.y);
    b.z = b.z < 0.f ? 0.f : (b.z > W ? W : b.z);
    b.w = b.w < 0.f ? 0.f : (b.w > H ? H : b.w);
    c_boxes[o] = b;
    c_scores[o] = sc;
    c_cls[o] = (int)classes[t];
    c_cand[o] = fin && sc > TTA_SCORE_THRESH ? 1 : 0;
}

// merged (n, topk) boxes in (ho, wo) space -> the augmentation's (ha, wa) space; rows beyond an image's count are zeros
__global__ __launch_bounds__(256) void tta_boxes_to_augmented_kernel(const float4* __restrict__ boxes, const int* __restrict__ counts,
                                                                      const int4* __restrict__ sizes, int n, int topk, int ha, int wa, int flip,
                                                                      float4* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * topk) return;
    const int img = t / topk, j = t - img * topk;
    if (j >= counts[img]) {
        out[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int4 s = sizes[img];
    float4 b = boxes[t];
    if (s.z != s.x || s.w != s.y) {  // (ho, wo) -> (hi, wi)
        const float qx = tta_ratio(s.y, s.w), qy = tta_ratio(s.x, s.z);
        b.x *= qx; b.y *= qy; b.z *= qx; b.w *= qy;
    }
    const float rx = tta_ratio(wa, s.y), ry = tta_ratio(ha, s.x);  // (hi, wi) -> (ha, wa)
    b.x *= rx; b.y *= ry; b.z *= rx; b.w *= ry;
    if (flip) {
        const float fw = (float)wa, x0 = fw - b.x, x1 = fw - b.z;
        b.x = x0 < x1 ? x0 : x1; b.z = x0 < x1 ? x1 : x0;  // (a NaN survives in one of the two)
    }
    out[t] = b;
}

// maps (A, rows, m, m) -> out (rows, m, m): the mean over a of the (mirrored when flip[a]) map; VEC samples of one map row per thread
template <int VEC>
__global__ __launch_bounds__(256) void tta_reduce_masks_kernel(const float* __restrict__ maps, const int* __restrict__ flip, int num_aug,
                                                                const int* __restrict__ counts, long long rows, int seg_rows, int m,
                                                                float* __restrict__ out) {
    const int per_row = m / VEC;  // (m % VEC == 0)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = rows * m * per_row;
    if (t >= total) return;
    const int xv = (int)(t % per_row);
    const long long line = t / per_row;  // (row, y)
    const long long row = line / m;
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    const bool live = (int)(row % seg_rows) < counts[row / seg_rows];
    if (live) {
        const long long plane = rows * m * m;
        for (int a = 0; a < num_aug; ++a) {  // fixed order: augmentation 0, 1, ...
            const float* src = maps + a * plane + line * m;
            if (VEC == 4) {
                if (flip[a]) {
                    const float4 q = *reinterpret_cast<const float4*>(src + (m - 4 - 4 * xv));
                    acc[0] += q.w; acc[1] += q.z; acc[2] += q.y; acc[3] += q.x;
                } else {
                    const float4 q = *reinterpret_cast<const float4*>(src + 4 * xv);
                    acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w;
                }
            } else {
                acc[0] += src[flip[a] ? m - 1 - xv : xv];
            }
        }
        const float d = (float)num_aug;
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / d;
    }
    float* dst = out + line * m + (long long)VEC * xv;
    if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else dst[0] = acc[0];
}

static bool tta_rows_ok(int32_t n, int32_t topk) { return n >= 1 && topk >= 1 && (int64_t)n * topk <= 0x7fffffffll - 256; }
static bool tta_aligned16(const void* a, const void* b, const void* c) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0; }

extern "C" osr_status osr_tta_boxes_to_original(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts,
                                                const int32_t* sizes, int32_t n, int32_t topk, int32_t ha, int32_t wa, int32_t flip,
                                                int32_t slot, int32_t cap, float* c_boxes, float* c_scores, int32_t* c_cls, int32_t* c_cand,
                                                void* stream) {
    OSR_REQUIRE(boxes && scores && classes && counts && sizes && c_boxes && c_scores && c_cls && c_cand, OSR_ERR_INVALID_ARG,
                "osr_tta_boxes_to_original: null pointer");
    OSR_REQUIRE(tta_rows_ok(n, topk) && ha >= 1 && wa >= 1, OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_original: bad geometry");
    OSR_REQUIRE(flip == 0 || flip == 1, OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_original: flip must be 0 or 1");
    OSR_REQUIRE(slot >= 0 && cap >= 1 && (int64_t)slot + topk <= cap, OSR_ERR_INVALID_ARG,
                "osr_tta_boxes_to_original: rows [slot, slot + topk) must lie inside the candidate list of cap rows");
    OSR_REQUIRE(tta_aligned16(boxes, sizes, c_boxes), OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_original: boxes, sizes and c_boxes must be 16-byte aligned");
    const int total = n * topk;
    hipLaunchKernelGGL(tta_boxes_to_original_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)boxes, scores,
                       classes, counts, (const int4*)sizes, n, topk, ha, wa, flip, slot, cap, (float4*)c_boxes, c_scores, c_cls, c_cand);
    OSR_CHECK_LAUNCH("osr_tta_boxes_to_original");
    return OSR_OK;
}

extern "C" osr_status osr_tta_boxes_to_augmented(const float* boxes, const int32_t* counts, const int32_t* sizes, int32_t n, int32_t topk,
                                                 int32_t ha, int32_t wa, int32_t flip, float* out, void* stream) {
    OSR_REQUIRE(boxes && counts && sizes && out, OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_augmented: null pointer");
    OSR_REQUIRE(tta_rows_ok(n, topk) && ha >= 1 && wa >= 1, OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_augmented: bad geometry");
    OSR_REQUIRE(flip == 0 || flip == 1, OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_augmented: flip must be 0 or 1");
    OSR_REQUIRE(tta_aligned16(boxes, sizes, out), OSR_ERR_INVALID_ARG, "osr_tta_boxes_to_augmented: boxes, sizes and out must be 16-byte aligned");
    const int total = n * topk;
    hipLaunchKernelGGL(tta_boxes_to_augmented_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)boxes, counts,
                       (const int4*)sizes, n, topk, ha, wa, flip, (float4*)out);
    OSR_CHECK_LAUNCH("osr_tta_boxes_to_augmented");
    return OSR_OK;
}

extern "C" osr_status osr_tta_reduce_masks(const float* maps, const int32_t* flip, int32_t num_aug, const int32_t* counts, int32_t n,
                                           int32_t topk, int32_t m, float* out, void* stream) {
    OSR_REQUIRE(maps && flip && counts && out, OSR_ERR_INVALID_ARG, "osr_tta_reduce_masks: null pointer");
    OSR_REQUIRE(num_aug >= 1, OSR_ERR_INVALID_ARG, "osr_tta_reduce_masks: at least one augmentation (A >= 1)");
    OSR_REQUIRE(tta_rows_ok(n, topk) && m >= 1 && m <= 1024, OSR_ERR_INVALID_ARG, "osr_tta_reduce_masks: bad geometry");
    const long long rows = (long long)n * topk;
    // 16-byte accesses when a map row is a whole number of float4 (then every row start is 16-byte aligned if the buffers are)
    const bool vec = m % 4 == 0 && ((uintptr_t)maps & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const long long total = rows * m * (vec ? m / 4 : m);
    OSR_REQUIRE((total + 255) / 256 <= 0x7fffffffll, OSR_ERR_INVALID_ARG, "osr_tta_reduce_masks: too many samples");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(tta_reduce_masks_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, maps, flip, num_aug, counts, rows, topk, m, out);
    else
        hipLaunchKernelGGL(tta_reduce_masks_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, maps, flip, num_aug, counts, rows, topk, m, out);
    OSR_CHECK_LAUNCH("osr_tta_reduce_masks");
    return OSR_OK;
}
