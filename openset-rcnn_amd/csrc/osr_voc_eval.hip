// Open-set PASCAL-VOC matching for gfx950 (include/osr.h: osr_voc_match, which states every rule): the per-detection half of
// host/evaluation.py's voc_eval for a batch of images and every class in ONE launch. Built with -ffp-contract=off: the record
// rounding and every overlap are fp64 and round like numpy's, so the flags equal the numpy specification's bit for bit.
//
// The grid is fixed: one workgroup of 1024 threads (16 waves) per (image row, class); a group without a detection of its class has
// nothing to write and leaves after the scan. What makes VOC's greedy matching parallel: a detection's ground truth is the argmax
// over ALL ground truths of its class, taken or not, so only "was it taken before me" depends on the other detections, and that is
// "am I the first in list order among the detections that chose it". Inside a group:
//   A. the rows of the group's class are compacted in row order with their rounded scores and ranked by them, stably
//      (osr_eval_match.h); non-finite rows are marked and left out;
//   B. one wave per detection: the lanes stride over the image's ground truths, keep the best overlap among those of the class (NaN
//      first, then the larger, equal ones to the lower index: np.argmax) and whether an "unknown" one overlaps, one wave reduction;
//      lane 0 notes the chosen ground truth and, unless it is difficult, lowers that ground truth's "first rank" in LDS (an integer
//      minimum inside the workgroup: the result does not depend on the order of arrival);
//   C. one thread per detection forms the flag byte: tp iff its rank is its ground truth's first rank.
// The group of class 0 also writes the rows that belong to no list (past counts, class outside 0 .. C - 1, image outside the table),
// so every output element has exactly ONE writer and repeats are bit-identical; `status` is preset by a memset on the same stream
// and every group that meets a non-finite row stores the same 1.
#include "osr_eval_match.h"
#include <limits.h>

#define VM_VALID 1
#define VM_TP 2
#define VM_FP 4
#define VM_UNK 8
#define VM_NONFINITE 16

struct VmParams {
    double thr;
    int n, cap, C, num_images, num_gt, max_img;
};

// The text record's numbers without the text: t[q] = rint(v * 10) of (x0 + 1, y0 + 1, x1, y1), the + 1 in fp32; *k = rint(s * 1000).
// false: a non-finite input, or a value that fits neither milli (int32) nor deci (int64).
__device__ __forceinline__ bool vm_record(const float* __restrict__ b, float s, double t[4], double* k) {
    const float x0 = b[0] + 1.0f, y0 = b[1] + 1.0f;
    t[0] = rint((double)x0 * 10.0), t[1] = rint((double)y0 * 10.0), t[2] = rint((double)b[2] * 10.0), t[3] = rint((double)b[3] * 10.0);
    *k = rint((double)s * 1000.0);
    bool ok = osr_finite(s) && osr_finite(b[0]) && osr_finite(b[1]) && osr_finite(b[2]) && osr_finite(b[3]) && fabs(*k) < 2147483648.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) ok = ok && fabs(t[q]) < 9223372036854775808.0;
    return ok;
}

// host/evaluation.py _overlaps: inclusive pixels (+ 1), fp64, in numpy's operation order
__device__ __forceinline__ double vm_iou(const double* __restrict__ g, const double bb[4]) {
    const double iw = fmax(fmin(g[2], bb[2]) - fmax(g[0], bb[0]) + 1.0, 0.0);
    const double ih = fmax(fmin(g[3], bb[3]) - fmax(g[1], bb[1]) + 1.0, 0.0);
    const double inter = iw * ih;
    const double uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (g[2] - g[0] + 1.0) * (g[3] - g[1] + 1.0) - inter;
    return inter / uni;
}

// np.argmax's order: does candidate (a, ja) come before (b, jb)? NaN is the maximum, equal values go to the lower index; j < 0: none
__device__ __forceinline__ bool vm_before(double a, int ja, double b, int jb) {
    if (ja < 0) return false;
    if (jb < 0) return true;
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return ja < jb;
}

__global__ __launch_bounds__(EM_THREADS) void vm_match_kernel(VmParams P, const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int64_t* __restrict__ classes, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ image_index, const int32_t* __restrict__ gt_img_off,
                                                             const double* __restrict__ gt_box, const int32_t* __restrict__ gt_cls,
                                                             const uint8_t* __restrict__ gt_difficult, uint8_t* __restrict__ flags,
                                                             int32_t* __restrict__ milli, int32_t* __restrict__ match, int64_t* __restrict__ deci,
                                                             int32_t* __restrict__ status) {
    __shared__ int c_row[EM_MAX_CAP];
    __shared__ int c_k[EM_MAX_CAP];
    __shared__ int c_rank[EM_MAX_CAP];
    __shared__ int c_j[EM_MAX_CAP];
    __shared__ uint8_t c_unk[EM_MAX_CAP];
    __shared__ int g_first[EM_MAX_G];  // per ground truth of the image: the lowest rank among the detections that chose it
    __shared__ int scan[17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x / P.C, c = blockIdx.x % P.C;
    const int img = image_index[i];
    const bool img_ok = img >= 0 && img < P.num_images;
    const int cnt = min(max(counts[i], 0), P.cap);
    const int64_t row0 = (int64_t)i * P.cap;
    if (c == 0) {  // the rows of no list
        for (int r = tid; r < P.cap; r += EM_THREADS) {
            bool listed = img_ok && r < cnt;
            if (listed) {
                const int64_t v = classes[row0 + r];
                listed = v >= 0 && v < (int64_t)P.C;
            }
            if (!listed) {
                flags[row0 + r] = 0, milli[row0 + r] = 0;
                if (match) match[row0 + r] = -1;
                if (deci) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) deci[(row0 + r) * 4 + q] = 0;
                }
            }
        }
    }
    if (!img_ok) return;  // (uniform)
    int g0, G;
    em_segment(gt_img_off, img, P.num_gt, P.max_img, &g0, &G);
    // A. the class's finite rows and their rounded scores, then their ranks
    const int D = em_compact(cnt, scan, c_row, c_k, [&](int r, int* key) {
        if (classes[row0 + r] != (int64_t)c) return false;
        double t[4], k;
        if (vm_record(boxes + (row0 + r) * 4, scores[row0 + r], t, &k)) {
            *key = (int)k;
            return true;
        }
        flags[row0 + r] = VM_VALID | VM_NONFINITE, milli[row0 + r] = 0;
        if (match) match[row0 + r] = -1;
        if (deci) {
#pragma unroll
            for (int q = 0; q < 4; ++q) deci[(row0 + r) * 4 + q] = 0;
        }
        status[0] = 1;  // (every writer stores the same word)
        return false;
    });
    if (D == 0) return;  // nothing more to write: no finite row of this image carries the class (uniform)
    __syncthreads();
    for (int m = tid; m < D; m += EM_THREADS) c_rank[m] = em_stable_before(c_k, D, m);
    for (int j = tid; j < G; j += EM_THREADS) g_first[j] = INT_MAX;
    __syncthreads();
    // B. per detection the first maximum among the class's ground truths and the overlap with an unknown one
    const int unknown = P.C - 1;
    for (int m = wave; m < D; m += EM_WAVES) {
        const int r = c_row[m];
        double t[4], k, bb[4];
        vm_record(boxes + (row0 + r) * 4, scores[row0 + r], t, &k);
#pragma unroll
        for (int q = 0; q < 4; ++q) bb[q] = t[q] / 10.0;
        double best = 0.0;
        int bj = -1;
        bool u_nan = false, u_over = false;
        for (int j = lane; j < G; j += 64) {
            const int cls = gt_cls[g0 + j];
            const bool own = cls == c, unk = c != unknown && cls == unknown;
            if (!own && !unk) continue;
            const double ov = vm_iou(gt_box + (int64_t)(g0 + j) * 4, bb);
            if (own && vm_before(ov, j, best, bj)) best = ov, bj = j;
            if (unk) {
                if (ov != ov) u_nan = true;
                else if (ov > P.thr) u_over = true;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const double ob = __shfl_xor(best, d, 64);
            const int oj = __shfl_xor(bj, d, 64);
            if (vm_before(ob, oj, best, bj)) best = ob, bj = oj;
        }
        const bool is_unk = __ballot(u_nan) == 0ull && __ballot(u_over) != 0ull;  // np.max(ov) > thr: a NaN overlap makes it false
        if (lane == 0) {
            const bool hit = bj >= 0 && best > P.thr;
            c_j[m] = hit ? bj : -1;
            c_unk[m] = is_unk ? 1 : 0;
            if (hit && !gt_difficult[g0 + bj]) atomicMin(&g_first[bj], c_rank[m]);
        }
    }
    __syncthreads();
    // C. the flag bytes
    for (int m = tid; m < D; m += EM_THREADS) {
        const int r = c_row[m], j = c_j[m];
        int f = VM_VALID | (c_unk[m] ? VM_UNK : 0);
        if (j < 0) f |= VM_FP;
        else if (!gt_difficult[g0 + j]) f |= g_first[j] == c_rank[m] ? VM_TP : VM_FP;
        flags[row0 + r] = (uint8_t)f;
        milli[row0 + r] = c_k[m];
        if (match) match[row0 + r] = j < 0 ? -1 : g0 + j;
        if (deci) {
            double t[4], k;
            vm_record(boxes + (row0 + r) * 4, scores[row0 + r], t, &k);
#pragma unroll
            for (int q = 0; q < 4; ++q) deci[(row0 + r) * 4 + q] = (int64_t)t[q];
        }
    }
}

extern "C" osr_status osr_voc_match(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts, const int32_t* image_index,
                                    int32_t n, int32_t cap, int32_t num_classes, const int32_t* gt_img_off, int32_t num_images, const double* gt_box,
                                    const int32_t* gt_cls, const uint8_t* gt_difficult, int32_t num_gt, int32_t max_gt_per_image, double ovthresh,
                                    uint8_t* flags, int32_t* milli, int32_t* match, int64_t* deci, int32_t* status, void* stream) {
    OSR_REQUIRE(n >= 0 && cap >= 0 && num_images >= 0 && num_gt >= 0 && max_gt_per_image >= 0, OSR_ERR_INVALID_ARG,
                "osr_voc_match: n %d, cap %d, num_images %d, num_gt %d, max_gt_per_image %d", n, cap, num_images, num_gt, max_gt_per_image);
    OSR_REQUIRE(cap <= EM_MAX_CAP, OSR_ERR_UNSUPPORTED, "osr_voc_match: cap %d, at most %d rows per image", cap, EM_MAX_CAP);
    OSR_REQUIRE(max_gt_per_image <= EM_MAX_G, OSR_ERR_UNSUPPORTED, "osr_voc_match: %d ground truths in one image, at most %d", max_gt_per_image, EM_MAX_G);
    OSR_REQUIRE(num_classes >= 1, OSR_ERR_UNSUPPORTED, "osr_voc_match: %d class names, at least 1 (\"unknown\")", num_classes);
    OSR_REQUIRE((int64_t)n * (int64_t)num_classes < (1LL << 31), OSR_ERR_UNSUPPORTED, "osr_voc_match: %d images x %d classes is no grid", n, num_classes);
    if (n == 0 || cap == 0) return OSR_OK;
    OSR_REQUIRE(boxes && scores && classes && counts && image_index && gt_img_off && flags && milli && status, OSR_ERR_INVALID_ARG,
                "osr_voc_match: null pointer");
    OSR_REQUIRE(num_gt == 0 || (gt_box && gt_cls && gt_difficult), OSR_ERR_INVALID_ARG, "osr_voc_match: null ground-truth pointer");
    OSR_REQUIRE(((uintptr_t)boxes & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)classes & 7) == 0 && ((uintptr_t)counts & 3) == 0 &&
                    ((uintptr_t)image_index & 3) == 0 && ((uintptr_t)gt_img_off & 3) == 0 && ((uintptr_t)gt_box & 7) == 0 && ((uintptr_t)gt_cls & 3) == 0 &&
                    ((uintptr_t)milli & 3) == 0 && ((uintptr_t)match & 3) == 0 && ((uintptr_t)deci & 7) == 0 && ((uintptr_t)status & 3) == 0,
                OSR_ERR_INVALID_ARG, "osr_voc_match: misaligned pointer");
    VmParams P;
    P.thr = ovthresh, P.n = n, P.cap = cap, P.C = num_classes, P.num_images = num_images, P.num_gt = num_gt, P.max_img = max_gt_per_image;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, 4, st) != hipSuccess) {
        osr_set_error("osr_voc_match: hipMemsetAsync failed");
        return OSR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(vm_match_kernel, dim3(n * num_classes), dim3(EM_THREADS), 0, st, P, boxes, scores, classes, counts, image_index, gt_img_off, gt_box,
                       gt_cls, gt_difficult, flags, milli, match, deci, status);
    OSR_CHECK_LAUNCH("osr_voc_match");
    return OSR_OK;
}
