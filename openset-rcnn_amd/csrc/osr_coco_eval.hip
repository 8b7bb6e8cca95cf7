// COCO detection / keypoint matching for gfx950 (include/osr.h: osr_coco_match): pycocotools' COCOeval.computeIoU / computeOks and
// evaluateImg for a batch of images in ONE launch. Built with -ffp-contract=off: every comparison and every similarity is fp64 and
// the bbox similarities round like numpy's, so the flags equal the numpy specification's bit for bit.
//
// The grid is fixed: one workgroup of 1024 threads (16 waves) per (image, category); a group without a detection of its class
// has nothing to write and leaves after the scan. Inside a group (osr_eval_match.h holds the shared steps A, D and E):
//   A. the rows of the group's class are compacted in row order and ranked by score key, stably;
//   B. per ranked detection its area, per ground truth one uint16 in LDS: bit a = "ignored in area range a", bit 8 = crowd;
//   C. the M x G similarity matrix, one thread per pair, into the caller's matrix (global memory: 128 x 4096 doubles fit no LDS);
//   D. the T x A greedy passes are independent, so the waves take them in turn (40 passes for bbox: 16 waves need three turns).
//      There are no sets and a tie goes to the higher position, the loop's `<`;
//   E. the bits of the T passes of an area range are packed into the flag words.
// No atomics anywhere and every address has one writer: repeats are bit-identical. rank, flags and match are preset by memsets on
// the same stream, so rows outside every list read -1 / 0 / -1.
#include "osr_eval_match.h"

#define CM_MAX_KP 32

struct CmParams {
    EmTables tb;
    int n, cap, K, Kp, T, A, max_det, mcap, task, num_gt, max_group;
};

__device__ __forceinline__ double cm_bbox_sim(const float* __restrict__ b, const double* __restrict__ g, bool crowd) {
    const double dx = (double)b[0], dy = (double)b[1], dw = (double)(b[2] - b[0]), dh = (double)(b[3] - b[1]);  // (fp32 differences, then widened)
    const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
    const double iw = fmax(fmin(dx + dw, gx + gw) - fmax(dx, gx), 0.0), ih = fmax(fmin(dy + dh, gy + gh) - fmax(dy, gy), 0.0);
    const double inter = iw * ih, da = dw * dh, ga = gw * gh;
    const double uni = crowd ? da : da + ga - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

__device__ __forceinline__ double cm_oks(const float* __restrict__ dk, const double* __restrict__ gk, const double* __restrict__ gb, double garea,
                                         const double* __restrict__ sigmas, int Kp) {
    int k1 = 0;
    for (int k = 0; k < Kp; ++k) k1 += gk[k * 3 + 2] > 0.0;
    const double x0 = gb[0] - gb[2], x1 = gb[0] + gb[2] * 2.0, y0 = gb[1] - gb[3], y1 = gb[1] + gb[3] * 2.0;
    const double den = garea + 2.220446049250313e-16;  // np.spacing(1)
    double sum = 0.0;
    for (int k = 0; k < Kp; ++k) {
        const double xd = (double)(dk[k * 3 + 0] - 0.5f), yd = (double)(dk[k * 3 + 1] - 0.5f);
        double dx, dy;
        if (k1 > 0) {
            if (!(gk[k * 3 + 2] > 0.0)) continue;
            dx = xd - gk[k * 3 + 0], dy = yd - gk[k * 3 + 1];
        } else {
            dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1), dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        }
        const double s2 = 2.0 * sigmas[k], e = (dx * dx + dy * dy) / (s2 * s2) / den / 2.0;
        sum += exp(-e);
    }
    return sum / (double)(k1 > 0 ? k1 : Kp);
}

__global__ __launch_bounds__(EM_THREADS) void cm_match_kernel(CmParams P, const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int64_t* __restrict__ classes, const int32_t* __restrict__ counts,
                                                             const float* __restrict__ keypoints, const int32_t* __restrict__ gt_seg_off,
                                                             const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                             const uint8_t* __restrict__ gt_flags, const double* __restrict__ gt_kpts,
                                                             const double* __restrict__ sigmas, uint32_t* __restrict__ flags, int32_t* __restrict__ rank,
                                                             int32_t* __restrict__ match, double* __restrict__ simm) {
    __shared__ int c_row[EM_MAX_CAP];
    __shared__ uint32_t c_key[EM_MAX_CAP];
    __shared__ int d_row[EM_MAX_DET];
    __shared__ double d_area[EM_MAX_DET];
    __shared__ uint16_t g_meta[EM_MAX_G];
    __shared__ uint8_t res[EM_MAX_T * EM_MAX_A][64];
    __shared__ int scan[17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x / P.K, c = blockIdx.x % P.K;
    const int cnt = min(max(counts[i], 0), P.cap);
    const int64_t row0 = (int64_t)i * P.cap;
    int g0, G;
    em_segment(gt_seg_off, blockIdx.x, P.num_gt, P.max_group, &g0, &G);
    // A. the class's rows, then their ranks
    const int D = em_compact(cnt, scan, c_row, c_key, [&](int r, uint32_t* key) {
        if (classes[row0 + r] != (int64_t)c) return false;
        *key = osr_float_key(scores[row0 + r]);
        return true;
    });
    if (D == 0) return;  // nothing to write: no row of this image carries the class (uniform)
    __syncthreads();
    const int M = min(D, P.max_det);
    for (int m = tid; m < D; m += EM_THREADS) {
        const int before = em_stable_before(c_key, D, m);
        if (before < M) {
            d_row[before] = c_row[m];
            rank[row0 + c_row[m]] = before;
        }
    }
    __syncthreads();
    // B. detection areas, ground-truth marks
    for (int d = tid; d < M; d += EM_THREADS) {
        const int64_t row = row0 + d_row[d];
        if (P.task == OSR_COCO_BBOX) {
            const float* b = boxes + row * 4;
            d_area[d] = (double)(b[2] - b[0]) * (double)(b[3] - b[1]);
        } else {
            const float* k = keypoints + row * P.Kp * 3;
            double xa = 0, xb = 0, ya = 0, yb = 0;
            for (int q = 0; q < P.Kp; ++q) {
                const double x = (double)(k[q * 3 + 0] - 0.5f), y = (double)(k[q * 3 + 1] - 0.5f);
                if (q == 0) xa = xb = x, ya = yb = y;
                else xa = fmin(xa, x), xb = fmax(xb, x), ya = fmin(ya, y), yb = fmax(yb, y);
            }
            d_area[d] = (xb - xa) * (yb - ya);
        }
    }
    for (int j = tid; j < G; j += EM_THREADS) {
        const int f = gt_flags[g0 + j];
        g_meta[j] = (uint16_t)((f & 1 ? EM_CROWD : 0) | em_ignored_bits(f & 2, gt_area[g0 + j], P.tb.rng, P.A));
    }
    // C. similarities: row d of the group's M x G block, which starts at g0 * mcap
    double* S = simm + (int64_t)g0 * P.mcap;
    for (int64_t p = tid; p < (int64_t)M * G; p += EM_THREADS) {
        const int d = (int)(p / G), j = (int)(p % G);
        const int64_t row = row0 + d_row[d];
        const double v = P.task == OSR_COCO_BBOX ? cm_bbox_sim(boxes + row * 4, gt_box + (int64_t)(g0 + j) * 4, gt_flags[g0 + j] & 1)
                                       : cm_oks(keypoints + row * P.Kp * 3, gt_kpts + (int64_t)(g0 + j) * P.Kp * 3, gt_box + (int64_t)(g0 + j) * 4,
                                                gt_area[g0 + j], sigmas, P.Kp);
        S[p] = v;
    }
    __threadfence_block();
    __syncthreads();
    // D. the passes
    for (int pass = wave; pass < P.A * P.T; pass += EM_WAVES) {
        const int a = pass / P.T, t = pass % P.T;
        res[pass][lane] = (uint8_t)em_greedy_pass<false>(
            g_meta, G, -1, P.tb.thr[t], a, P.tb.rng[a * 2], P.tb.rng[a * 2 + 1], d_area, d_row, M, [&](int d) { return S + (int64_t)d * G; },
            [](int j) { return j; }, match ? match + (row0 * P.A + a) * P.T + t : nullptr, (int64_t)P.A * P.T, g0);
    }
    __syncthreads();
    // E. the flag words
    for (int p = tid; p < M * P.A; p += EM_THREADS) {
        const int d = p / P.A, a = p % P.A;
        flags[(row0 + d_row[d]) * P.A + a] = em_flag_word(res, a * P.T, P.T, d);
    }
}

extern "C" int64_t osr_coco_match_workspace_bytes(int32_t cap, int32_t max_det, int32_t num_gt) {
    if (cap < 0 || max_det < 0 || num_gt < 0) return -1;
    return (int64_t)(cap < max_det ? cap : max_det) * num_gt * 8;
}

extern "C" osr_status osr_coco_match(int32_t task, const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts,
                                     const float* keypoints, int32_t n, int32_t cap, int32_t num_categories, int32_t num_keypoints,
                                     const int32_t* gt_seg_off, const double* gt_box, const double* gt_area, const uint8_t* gt_flags,
                                     const double* gt_kpts, const double* sigmas, int32_t num_gt, int32_t max_gt_per_group, const double* iou_thrs,
                                     int32_t num_thrs, const double* area_rng, int32_t num_areas, int32_t max_det, uint32_t* flags, int32_t* rank,
                                     int32_t* match, double* sim, void* workspace, int64_t workspace_bytes, void* stream) {
    const bool kp = task == OSR_COCO_KEYPOINTS;
    OSR_REQUIRE(task == OSR_COCO_BBOX || kp, OSR_ERR_INVALID_ARG, "osr_coco_match: task %d", task);
    OSR_REQUIRE(n >= 0 && cap >= 0 && num_categories >= 1 && num_gt >= 0 && max_gt_per_group >= 0 && max_det >= 1 && num_thrs >= 1 && num_areas >= 1,
                OSR_ERR_INVALID_ARG, "osr_coco_match: n %d, cap %d, categories %d, num_gt %d, max_gt_per_group %d, max_det %d, thresholds %d, area ranges %d", n, cap,
                num_categories, num_gt, max_gt_per_group, max_det, num_thrs, num_areas);
    OSR_REQUIRE(cap <= EM_MAX_CAP, OSR_ERR_UNSUPPORTED, "osr_coco_match: cap %d, at most %d rows per image", cap, EM_MAX_CAP);
    OSR_REQUIRE(max_det <= EM_MAX_DET, OSR_ERR_UNSUPPORTED, "osr_coco_match: max_det %d, at most %d", max_det, EM_MAX_DET);
    OSR_REQUIRE(num_thrs <= EM_MAX_T, OSR_ERR_UNSUPPORTED, "osr_coco_match: %d thresholds, at most %d", num_thrs, EM_MAX_T);
    OSR_REQUIRE(num_areas <= EM_MAX_A, OSR_ERR_UNSUPPORTED, "osr_coco_match: %d area ranges, at most %d", num_areas, EM_MAX_A);
    OSR_REQUIRE(max_gt_per_group <= EM_MAX_G, OSR_ERR_UNSUPPORTED, "osr_coco_match: %d ground truths in one (image, category), at most %d", max_gt_per_group,
                EM_MAX_G);
    OSR_REQUIRE(!kp || (num_keypoints >= 1 && num_keypoints <= CM_MAX_KP), kp && num_keypoints > CM_MAX_KP ? OSR_ERR_UNSUPPORTED : OSR_ERR_INVALID_ARG,
                "osr_coco_match: %d keypoints, 1 .. %d", num_keypoints, CM_MAX_KP);
    OSR_REQUIRE((int64_t)n * num_categories < (1LL << 31) - 1, OSR_ERR_INVALID_ARG, "osr_coco_match: %d images x %d categories", n, num_categories);
    OSR_REQUIRE(iou_thrs && area_rng, OSR_ERR_INVALID_ARG, "osr_coco_match: null pointer (thresholds / area ranges)");
    if (n == 0 || cap == 0) return OSR_OK;
    OSR_REQUIRE(boxes && scores && classes && counts && gt_seg_off && flags && rank && (!kp || (keypoints && sigmas)), OSR_ERR_INVALID_ARG,
                "osr_coco_match: null pointer");
    OSR_REQUIRE(num_gt == 0 || (gt_box && gt_area && gt_flags && (!kp || gt_kpts)), OSR_ERR_INVALID_ARG, "osr_coco_match: null ground-truth pointer");
    const int64_t need = osr_coco_match_workspace_bytes(cap, max_det, num_gt);
    double* simm = sim ? sim : (double*)workspace;
    OSR_REQUIRE(need == 0 || simm, OSR_ERR_WORKSPACE, "osr_coco_match: neither sim nor a workspace (%lld bytes)", (long long)need);
    OSR_REQUIRE(sim || need == 0 || workspace_bytes >= need, OSR_ERR_WORKSPACE, "osr_coco_match: workspace %lld bytes < %lld", (long long)workspace_bytes,
                (long long)need);
    OSR_REQUIRE(((uintptr_t)boxes & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)classes & 7) == 0 && ((uintptr_t)counts & 3) == 0 &&
                    ((uintptr_t)keypoints & 3) == 0 && ((uintptr_t)gt_seg_off & 3) == 0 && ((uintptr_t)gt_box & 7) == 0 && ((uintptr_t)gt_area & 7) == 0 &&
                    ((uintptr_t)gt_kpts & 7) == 0 && ((uintptr_t)sigmas & 7) == 0 && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)rank & 3) == 0 &&
                    ((uintptr_t)match & 3) == 0 && ((uintptr_t)simm & 7) == 0,
                OSR_ERR_INVALID_ARG, "osr_coco_match: misaligned pointer");
    CmParams P;
    em_fill_tables(&P.tb, iou_thrs, num_thrs, area_rng, num_areas);
    P.n = n, P.cap = cap, P.K = num_categories, P.Kp = kp ? num_keypoints : 0, P.T = num_thrs, P.A = num_areas, P.max_det = max_det;
    P.mcap = cap < max_det ? cap : max_det, P.task = task, P.num_gt = num_gt, P.max_group = max_gt_per_group;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)n * cap;
    if (!em_preset(flags, rows * num_areas, rank, rows, match, rows * num_areas * num_thrs, st)) {
        osr_set_error("osr_coco_match: hipMemsetAsync failed");
        return OSR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(cm_match_kernel, dim3(n * num_categories), dim3(EM_THREADS), 0, st, P, boxes, scores, classes, counts, keypoints, gt_seg_off, gt_box,
                       gt_area, gt_flags, gt_kpts, sigmas, flags, rank, match, simm);
    OSR_CHECK_LAUNCH("osr_coco_match");
    return OSR_OK;
}
