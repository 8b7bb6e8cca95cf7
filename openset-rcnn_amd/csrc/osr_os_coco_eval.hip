// Open-set COCO matching for gfx950 (include/osr.h: osr_os_coco_match, which states every rule): the per-image half of
// host/os_coco_evaluation.py's OpensetCOCOEval.evaluate for a batch of images in ONE launch. Built with -ffp-contract=off: every
// comparison and every similarity is fp64 and rounds like numpy's, so the flags equal the numpy specification's bit for bit.
//
// It differs from osr_coco_eval.hip in what a list is matched against: one detection list (a class slot of an image) meets up to
// THREE ground-truth sets of the same image (own slot, the other known slots, the unknown slot), each with its own "taken" state and
// one of them with its own tie order, and the detection geometry is formed from corners widened to fp64 first.
//
// The grid is fixed: one workgroup of 1024 threads (16 waves) per (image, slot), slots 0 .. K with K the unknown one; a group
// without a detection of its slot has nothing to write and leaves after the scan. Inside a group (osr_eval_match.h holds the shared
// steps A, D and E):
//   A. the rows of the group's slot are compacted in row order and ranked by score key, stably;
//   B. per ranked detection its area, per ground truth of the IMAGE one uint16 in LDS: bit a = "ignored in area range a", bit 8 =
//      crowd, bits 9-10 = the set it belongs to for this slot (3: none);
//   C. the M x G similarity matrix, one thread per pair, into the workspace (global memory: 128 x 4096 doubles fit no LDS). A row of
//      the padded list belongs to one slot only, so the image's groups share the image's cap x G block and index it by row: every
//      detection x ground-truth pair of an image is computed once. (Keeping a small matrix in LDS instead was measured on the
//      GraspNet-shaped set and changed nothing: 0.877 against 0.884 ms per batch.)
//   D. the sets x A x T greedy passes are independent chains, so the waves take them in turn (120 passes for a known slot: 16 waves
//      need eight turns). A pass skips the ground truths outside its set, and a tie goes to the higher position in the set's order;
//   E. the bits of the T passes of a (set, area range) are packed into the flag words.
// No atomics anywhere and every address has one writer: repeats are bit-identical. rank, flags and match are preset by memsets on
// the same stream, so rows outside every list read -1 / 0 / -1.
#include "osr_eval_match.h"

#define OM_SETS 3

struct OmParams {
    EmTables tb;
    int n, cap, K, L, T, A, max_det, num_gt, max_img;
};

// maskUtils.iou on xywh as host/os_coco_evaluation.py box_iou_xywh forms it; the detection's corners are widened BEFORE the differences
__device__ __forceinline__ double om_bbox_sim(const float* __restrict__ b, const double* __restrict__ g, bool crowd) {
    const double dx = (double)b[0], dy = (double)b[1], dw = (double)b[2] - (double)b[0], dh = (double)b[3] - (double)b[1];
    const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
    const double iw = fmax(fmin(dx + dw, gx + gw) - fmax(dx, gx), 0.0), ih = fmax(fmin(dy + dh, gy + gh) - fmax(dy, gy), 0.0);
    const double inter = iw * ih, da = dw * dh, ga = gw * gh;
    const double uni = crowd ? da : da + ga - inter;
    return uni > 0.0 ? inter / fmax(uni, 1e-300) : 0.0;
}

// (8 waves per SIMD: two groups share a CU. Stated, not left to the register allocator, which otherwise spreads over 105 scalar registers.)
__global__ __launch_bounds__(EM_THREADS, 8) void om_match_kernel(OmParams P, const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int64_t* __restrict__ classes, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ class_slot, const int32_t* __restrict__ gt_img_off,
                                                             const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                             const int32_t* __restrict__ gt_slot, const int32_t* __restrict__ gt_pos,
                                                             const uint8_t* __restrict__ gt_crowd, uint32_t* __restrict__ flags,
                                                             int32_t* __restrict__ rank, int32_t* __restrict__ match, double* __restrict__ simm) {
    __shared__ int c_row[EM_MAX_CAP];
    __shared__ uint32_t c_key[EM_MAX_CAP];
    __shared__ int d_row[EM_MAX_DET];
    __shared__ double d_area[EM_MAX_DET];
    __shared__ uint16_t g_meta[EM_MAX_G];
    __shared__ uint8_t res[OM_SETS * EM_MAX_A * EM_MAX_T][64];
    __shared__ int scan[17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slots = P.K + 1;
    const int i = blockIdx.x / slots, c = blockIdx.x % slots;
    const int cnt = min(max(counts[i], 0), P.cap);
    const int64_t row0 = (int64_t)i * P.cap;
    int g0, G;
    em_segment(gt_img_off, i, P.num_gt, P.max_img, &g0, &G);
    // A. the slot's rows, then their ranks
    const int D = em_compact(cnt, scan, c_row, c_key, [&](int r, uint32_t* key) {
        const int64_t v = classes[row0 + r];
        if (!(v >= 0 && v < (int64_t)P.L && class_slot[v] == c)) return false;  // (c is in 0 .. K, so a slot outside -1 .. K is dropped as well)
        *key = osr_float_key(scores[row0 + r]);
        return true;
    });
    if (D == 0) return;  // nothing to write: no row of this image carries the slot (uniform)
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
    const bool unknown = c == P.K;
    for (int d = tid; d < M; d += EM_THREADS) {
        const float* b = boxes + (row0 + d_row[d]) * 4;
        d_area[d] = ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]);
    }
    for (int j = tid; j < G; j += EM_THREADS) {
        const int crowd = gt_crowd[g0 + j] & 1, gs = gt_slot[g0 + j];
        int set = 3;
        if (gs == P.K) set = unknown ? 0 : 2;
        else if (gs >= 0 && gs < P.K) set = unknown ? 1 : (gs == c ? 0 : 1);
        g_meta[j] = (uint16_t)((crowd ? EM_CROWD : 0) | set << EM_SET_SHIFT | em_ignored_bits(crowd, gt_area[g0 + j], P.tb.rng, P.A));
    }
    // C. similarities: row r of the image's cap x G block, which starts at g0 * cap
    double* S = simm + (int64_t)g0 * P.cap;
    for (int64_t p = tid; p < (int64_t)M * G; p += EM_THREADS) {
        const int d = (int)(p / G), j = (int)(p % G);
        const int r = d_row[d];
        S[(int64_t)r * G + j] = om_bbox_sim(boxes + (row0 + r) * 4, gt_box + (int64_t)(g0 + j) * 4, gt_crowd[g0 + j] & 1);
    }
    __threadfence_block();
    __syncthreads();
    // D. the passes
    const int sets = unknown ? 2 : 3;
    for (int pass = wave; pass < sets * P.A * P.T; pass += EM_WAVES) {
        const int s = pass / (P.A * P.T), a = pass / P.T % P.A, t = pass % P.T;
        const bool by_pos = !unknown && s == 1;  // a known slot's other-known set stands in annotation order ACROSS the slots
        res[pass][lane] = (uint8_t)em_greedy_pass<true>(
            g_meta, G, s, P.tb.thr[t], a, P.tb.rng[a * 2], P.tb.rng[a * 2 + 1], d_area, d_row, M, [&](int d) { return S + (int64_t)d_row[d] * G; },
            [&](int j) { return by_pos ? gt_pos[g0 + j] : j; }, match ? match + ((row0 * P.A + a) * OM_SETS + s) * P.T + t : nullptr,
            (int64_t)P.A * OM_SETS * P.T, g0);
    }
    __syncthreads();
    // E. the flag words
    for (int p = tid; p < M * P.A * sets; p += EM_THREADS) {
        const int d = p / (P.A * sets), a = p / sets % P.A, s = p % sets;
        flags[((row0 + d_row[d]) * P.A + a) * OM_SETS + s] = em_flag_word(res, (s * P.A + a) * P.T, P.T, d);
    }
}

extern "C" int64_t osr_os_coco_match_workspace_bytes(int32_t cap, int32_t num_gt) {
    if (cap < 0 || num_gt < 0) return -1;
    return (int64_t)cap * num_gt * 8;
}

extern "C" osr_status osr_os_coco_match(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts, int32_t n, int32_t cap,
                                        const int32_t* class_slot, int32_t num_class_values, int32_t num_known, const int32_t* gt_img_off,
                                        const double* gt_box, const double* gt_area, const int32_t* gt_slot, const int32_t* gt_pos,
                                        const uint8_t* gt_crowd, int32_t num_gt, int32_t max_gt_per_image, const double* iou_thrs, int32_t num_thrs,
                                        const double* area_rng, int32_t num_areas, int32_t max_det, uint32_t* flags, int32_t* rank, int32_t* match,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    OSR_REQUIRE(n >= 0 && cap >= 0 && num_class_values >= 1 && num_known >= 0 && num_gt >= 0 && max_gt_per_image >= 0 && max_det >= 1 && num_thrs >= 1 &&
                    num_areas >= 1,
                OSR_ERR_INVALID_ARG,
                "osr_os_coco_match: n %d, cap %d, class values %d, known slots %d, num_gt %d, max_gt_per_image %d, max_det %d, thresholds %d, area ranges %d", n,
                cap, num_class_values, num_known, num_gt, max_gt_per_image, max_det, num_thrs, num_areas);
    OSR_REQUIRE(cap <= EM_MAX_CAP, OSR_ERR_UNSUPPORTED, "osr_os_coco_match: cap %d, at most %d rows per image", cap, EM_MAX_CAP);
    OSR_REQUIRE(max_det <= EM_MAX_DET, OSR_ERR_UNSUPPORTED, "osr_os_coco_match: max_det %d, at most %d", max_det, EM_MAX_DET);
    OSR_REQUIRE(num_thrs <= EM_MAX_T, OSR_ERR_UNSUPPORTED, "osr_os_coco_match: %d thresholds, at most %d", num_thrs, EM_MAX_T);
    OSR_REQUIRE(num_areas <= EM_MAX_A, OSR_ERR_UNSUPPORTED, "osr_os_coco_match: %d area ranges, at most %d", num_areas, EM_MAX_A);
    OSR_REQUIRE(max_gt_per_image <= EM_MAX_G, OSR_ERR_UNSUPPORTED, "osr_os_coco_match: %d ground truths in one image, at most %d", max_gt_per_image, EM_MAX_G);
    OSR_REQUIRE((int64_t)n * ((int64_t)num_known + 1) < (1LL << 31) - 1, OSR_ERR_UNSUPPORTED, "osr_os_coco_match: %d images x %lld slots is no grid", n,
                (long long)num_known + 1);
    OSR_REQUIRE(iou_thrs && area_rng, OSR_ERR_INVALID_ARG, "osr_os_coco_match: null pointer (thresholds / area ranges)");
    if (n == 0 || cap == 0) return OSR_OK;
    OSR_REQUIRE(boxes && scores && classes && counts && class_slot && gt_img_off && flags && rank, OSR_ERR_INVALID_ARG, "osr_os_coco_match: null pointer");
    OSR_REQUIRE(num_gt == 0 || (gt_box && gt_area && gt_slot && gt_pos && gt_crowd), OSR_ERR_INVALID_ARG, "osr_os_coco_match: null ground-truth pointer");
    const int64_t need = osr_os_coco_match_workspace_bytes(cap, num_gt);
    OSR_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), OSR_ERR_WORKSPACE, "osr_os_coco_match: workspace %lld bytes < %lld",
                (long long)(workspace ? workspace_bytes : 0), (long long)need);
    OSR_REQUIRE(((uintptr_t)boxes & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)classes & 7) == 0 && ((uintptr_t)counts & 3) == 0 &&
                    ((uintptr_t)class_slot & 3) == 0 && ((uintptr_t)gt_img_off & 3) == 0 && ((uintptr_t)gt_box & 7) == 0 && ((uintptr_t)gt_area & 7) == 0 &&
                    ((uintptr_t)gt_slot & 3) == 0 && ((uintptr_t)gt_pos & 3) == 0 && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)rank & 3) == 0 &&
                    ((uintptr_t)match & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
                OSR_ERR_INVALID_ARG, "osr_os_coco_match: misaligned pointer");
    OmParams P;
    em_fill_tables(&P.tb, iou_thrs, num_thrs, area_rng, num_areas);
    P.n = n, P.cap = cap, P.K = num_known, P.L = num_class_values, P.T = num_thrs, P.A = num_areas, P.max_det = max_det;
    P.num_gt = num_gt, P.max_img = max_gt_per_image;
    hipStream_t st = (hipStream_t)stream;
    const int64_t words = (int64_t)n * cap * num_areas * OM_SETS;
    if (!em_preset(flags, words, rank, (int64_t)n * cap, match, words * num_thrs, st)) {
        osr_set_error("osr_os_coco_match: hipMemsetAsync failed");
        return OSR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(om_match_kernel, dim3(n * (num_known + 1)), dim3(EM_THREADS), 0, st, P, boxes, scores, classes, counts, class_slot, gt_img_off, gt_box,
                       gt_area, gt_slot, gt_pos, gt_crowd, flags, rank, match, (double*)workspace);
    OSR_CHECK_LAUNCH("osr_os_coco_match");
    return OSR_OK;
}
