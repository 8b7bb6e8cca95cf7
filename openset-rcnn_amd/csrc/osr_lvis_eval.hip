// LVIS federated box matching for gfx950 (include/osr.h: osr_lvis_match): lvis-api's LVISResults cut, LVISEval._prepare's category
// filter and evaluate_img for a batch of images in TWO launches. Built with -ffp-contract=off: every comparison and every similarity is
// fp64 and the similarities are osr_coco_match's (cm_bbox_sim's arithmetic with crowd 0), so the flags equal the numpy LVISEval's bit
// for bit.
//
// The grid never is n x K (1203 categories, of which an image evaluates a dozen):
//   lv_group_kernel, one workgroup of 1024 threads per image:
//     1. every row < count is ranked by score key, stably (em_compact + em_stable_before), and the ranks >= max_dets are cut: the cut
//        is ACROSS the categories and comes first;
//     2. each kept row looks its class up in the image's ascending ev_cat slice (binary search): no entry, no listing;
//     3. the listed rows are ordered by (entry, image rank), which is (category, image rank): a count over at most max_dets rows;
//     4. one scan over the ordered list numbers the groups; the per-image group table {entry, first, M}, the ordered rows and the
//        group count go to the workspace, rank (the position in the group's list) to the caller.
//   lv_match_kernel, n x min(cap, max_dets) workgroups; those beyond the image's group count leave at once. A group runs steps B to E
//     of cm_match_kernel with osr_eval_match.h's pass and packer at LV_MAX_DET detections; an unmatched detection of a not
//     exhaustively annotated category becomes ignored where the flag words are packed.
// No atomics anywhere and every address has one writer: repeats are bit-identical. rank, flags and match are preset by memsets on the
// same stream, so rows outside every list read -1 / 0 / -1.
#include "osr_eval_match.h"

#define LV_MAX_DET 512  // detections kept per image, hence per group: a lane's results are 8 detections in a uint16

struct LvParams {
    EmTables tb;
    int n, cap, K, T, A, max_dets, mcap, num_ev, num_gt, max_group;
};

// the workspace's tables behind the similarities, int32: gcount (n), then g_ent, g_first, g_M and s_row, each (n, mcap)
struct LvTables {
    int32_t *gcount, *g_ent, *g_first, *g_M, *s_row;
};

static inline int64_t lv_table_words(int64_t n, int64_t mcap) { return (n + 4 * n * mcap + 1) / 2 * 2; }

// cm_bbox_sim (osr_coco_eval.hip) without its crowd branch: LVIS has no crowds
__device__ __forceinline__ double lv_bbox_sim(const float* __restrict__ b, const double* __restrict__ g) {
    const double dx = (double)b[0], dy = (double)b[1], dw = (double)(b[2] - b[0]), dh = (double)(b[3] - b[1]);  // (fp32 differences, then widened)
    const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
    const double iw = fmax(fmin(dx + dw, gx + gw) - fmax(dx, gx), 0.0), ih = fmax(fmin(dy + dh, gy + gh) - fmax(dy, gy), 0.0);
    const double inter = iw * ih, uni = dw * dh + gw * gh - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

__global__ __launch_bounds__(EM_THREADS) void lv_group_kernel(LvParams P, const float* __restrict__ scores, const int64_t* __restrict__ classes,
                                                             const int32_t* __restrict__ counts, const int32_t* __restrict__ img_off,
                                                             const int32_t* __restrict__ ev_cat, int32_t* __restrict__ rank, LvTables W) {
    __shared__ int c_row[EM_MAX_CAP];
    __shared__ uint32_t c_key[EM_MAX_CAP];
    __shared__ int k_ent[LV_MAX_DET], k_row[LV_MAX_DET];  // by image rank: the row's entry (-1: its category is not evaluated), the row
    __shared__ int s_ent[LV_MAX_DET], s_rank[LV_MAX_DET];  // by list position: the entry, the position in the group
    __shared__ int scan[17];
    const int tid = threadIdx.x, i = blockIdx.x;
    const int cnt = min(max(counts[i], 0), P.cap);
    const int64_t row0 = (int64_t)i * P.cap, tab0 = (int64_t)i * P.mcap;
    const int e0 = min(max(img_off[i], 0), P.num_ev), e1 = min(max(img_off[i + 1], e0), P.num_ev);
    // 1. every row of the image, ranked
    const int D = em_compact(cnt, scan, c_row, c_key, [&](int r, uint32_t* key) {
        *key = osr_float_key(scores[row0 + r]);
        return true;
    });
    if (D == 0 || e0 == e1) {  // nothing is listed (uniform)
        if (tid == 0) W.gcount[i] = 0;
        return;
    }
    __syncthreads();
    const int kept = min(D, P.max_dets);
    // 2. the cut, then the category filter
    for (int m = tid; m < D; m += EM_THREADS) {
        const int before = em_stable_before(c_key, D, m);
        if (before >= kept) continue;
        const int64_t c = classes[row0 + c_row[m]];
        int ent = -1;
        if (c >= 0 && c < (int64_t)P.K) {
            int lo = e0, hi = e1;  // the first entry whose category is >= c
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)ev_cat[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < e1 && (int64_t)ev_cat[lo] == c) ent = lo;
        }
        k_ent[before] = ent, k_row[before] = c_row[m];
    }
    __syncthreads();
    // 3. the listed rows by (entry, image rank); kept <= LV_MAX_DET < EM_THREADS: one thread per kept row
    const int ent = tid < kept ? k_ent[tid] : -1;
    int L;
    osr_block_excl_scan(ent >= 0 ? 1 : 0, scan, &L);
    if (L == 0) {
        if (tid == 0) W.gcount[i] = 0;
        return;
    }
    if (ent >= 0) {
        int pos = 0, in_group = 0;
        for (int q = 0; q < kept; ++q) {
            const int o = k_ent[q];
            pos += o >= 0 && (o < ent || (o == ent && q < tid));
            in_group += o == ent && q < tid;
        }
        s_ent[pos] = ent, s_rank[pos] = in_group;
        W.s_row[tab0 + pos] = k_row[tid];
        rank[row0 + k_row[tid]] = in_group;
    }
    __syncthreads();
    // 4. the groups: a head opens one, the last member knows M
    const bool head = tid < L && (tid == 0 || s_ent[tid - 1] != s_ent[tid]);
    int groups;
    const int g = osr_block_excl_scan(head ? 1 : 0, scan, &groups) + (head ? 1 : 0) - 1;  // the group of list position tid
    if (tid < L) {
        if (head) W.g_ent[tab0 + g] = s_ent[tid], W.g_first[tab0 + g] = tid;
        if (tid == L - 1 || s_ent[tid + 1] != s_ent[tid]) W.g_M[tab0 + g] = s_rank[tid] + 1;
    }
    if (tid == 0) W.gcount[i] = groups;
}

__global__ __launch_bounds__(EM_THREADS) void lv_match_kernel(LvParams P, const float* __restrict__ boxes, const int32_t* __restrict__ ev_gt_off,
                                                             const uint8_t* __restrict__ ev_flags, const double* __restrict__ gt_box,
                                                             const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_flags, LvTables W,
                                                             uint32_t* __restrict__ flags, int32_t* __restrict__ match, double* __restrict__ simm) {
    __shared__ int d_row[LV_MAX_DET];
    __shared__ double d_area[LV_MAX_DET];
    __shared__ uint16_t g_meta[EM_MAX_G];
    __shared__ em_res_t<LV_MAX_DET> res[EM_MAX_T * EM_MAX_A][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x / P.mcap, grp = blockIdx.x % P.mcap;
    if (grp >= min(W.gcount[i], P.mcap)) return;  // (uniform)
    const int64_t row0 = (int64_t)i * P.cap, tab0 = (int64_t)i * P.mcap;
    const int ent = min(max(W.g_ent[tab0 + grp], 0), P.num_ev - 1);
    const int first = min(max(W.g_first[tab0 + grp], 0), P.mcap - 1), M = min(max(W.g_M[tab0 + grp], 0), P.mcap - first);
    int g0, G;
    em_segment(ev_gt_off, ent, P.num_gt, P.max_group, &g0, &G);
    const bool not_exhaustive = ev_flags[ent] & 1;
    // B. the group's rows and their areas, ground-truth marks
    for (int d = tid; d < M; d += EM_THREADS) {
        const int r = min(max(W.s_row[tab0 + first + d], 0), P.cap - 1);
        const float* b = boxes + (row0 + r) * 4;
        d_row[d] = r;
        d_area[d] = (double)(b[2] - b[0]) * (double)(b[3] - b[1]);
    }
    for (int j = tid; j < G; j += EM_THREADS) g_meta[j] = (uint16_t)em_ignored_bits(gt_flags[g0 + j] & 2, gt_area[g0 + j], P.tb.rng, P.A);
    __syncthreads();
    // C. similarities: row d of the group's M x G block, which starts at g0 * mcap
    double* S = simm + (int64_t)g0 * P.mcap;
    for (int64_t p = tid; p < (int64_t)M * G; p += EM_THREADS) {
        const int d = (int)(p / G), j = (int)(p % G);
        S[p] = lv_bbox_sim(boxes + (row0 + d_row[d]) * 4, gt_box + (int64_t)(g0 + j) * 4);
    }
    __threadfence_block();
    __syncthreads();
    // D. the passes
    for (int pass = wave; pass < P.A * P.T; pass += EM_WAVES) {
        const int a = pass / P.T, t = pass % P.T;
        res[pass][lane] = (em_res_t<LV_MAX_DET>)em_greedy_pass<false, LV_MAX_DET>(
            g_meta, G, -1, P.tb.thr[t], a, P.tb.rng[a * 2], P.tb.rng[a * 2 + 1], d_area, d_row, M, [&](int d) { return S + (int64_t)d * G; },
            [](int j) { return j; }, match ? match + (row0 * P.A + a) * P.T + t : nullptr, (int64_t)P.A * P.T, g0);
    }
    __syncthreads();
    // E. the flag words; where the category is not exhaustively annotated an unmatched detection is ignored
    const uint32_t all_t = (1u << P.T) - 1u;
    for (int p = tid; p < M * P.A; p += EM_THREADS) {
        const int d = p / P.A, a = p % P.A;
        uint32_t w = em_flag_word<LV_MAX_DET>(res, a * P.T, P.T, d);
        if (not_exhaustive) w |= (~w & all_t) << 16;
        flags[(row0 + d_row[d]) * P.A + a] = w;
    }
}

extern "C" int64_t osr_lvis_match_workspace_bytes(int32_t n, int32_t cap, int32_t max_dets, int32_t num_gt) {
    if (n < 0 || cap < 0 || max_dets < 0 || num_gt < 0) return -1;
    const int64_t mcap = cap < max_dets ? cap : max_dets;
    return mcap * num_gt * 8 + lv_table_words(n, mcap) * 4;
}

extern "C" osr_status osr_lvis_match(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts, int32_t n, int32_t cap,
                                     int32_t num_categories, const int32_t* img_off, const int32_t* ev_cat, const int32_t* ev_gt_off,
                                     const uint8_t* ev_flags, int32_t num_entries, const double* gt_box, const double* gt_area, const uint8_t* gt_flags,
                                     int32_t num_gt, int32_t max_gt_per_group, const double* iou_thrs, int32_t num_thrs, const double* area_rng,
                                     int32_t num_areas, int32_t max_dets, uint32_t* flags, int32_t* rank, int32_t* match, double* sim, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    OSR_REQUIRE(n >= 0 && cap >= 0 && num_categories >= 1 && num_entries >= 0 && num_gt >= 0 && max_gt_per_group >= 0 && max_dets >= 1 && num_thrs >= 1 &&
                    num_areas >= 1,
                OSR_ERR_INVALID_ARG, "osr_lvis_match: n %d, cap %d, categories %d, entries %d, num_gt %d, max_gt_per_group %d, max_dets %d, thresholds %d, area ranges %d",
                n, cap, num_categories, num_entries, num_gt, max_gt_per_group, max_dets, num_thrs, num_areas);
    OSR_REQUIRE(cap <= EM_MAX_CAP, OSR_ERR_UNSUPPORTED, "osr_lvis_match: cap %d, at most %d rows per image", cap, EM_MAX_CAP);
    OSR_REQUIRE(max_dets <= LV_MAX_DET, OSR_ERR_UNSUPPORTED, "osr_lvis_match: max_dets %d, at most %d", max_dets, LV_MAX_DET);
    OSR_REQUIRE(num_thrs <= EM_MAX_T, OSR_ERR_UNSUPPORTED, "osr_lvis_match: %d thresholds, at most %d", num_thrs, EM_MAX_T);
    OSR_REQUIRE(num_areas <= EM_MAX_A, OSR_ERR_UNSUPPORTED, "osr_lvis_match: %d area ranges, at most %d", num_areas, EM_MAX_A);
    OSR_REQUIRE(max_gt_per_group <= EM_MAX_G, OSR_ERR_UNSUPPORTED, "osr_lvis_match: %d ground truths in one (image, category), at most %d", max_gt_per_group,
                EM_MAX_G);
    const int64_t mcap = cap < max_dets ? cap : max_dets;
    OSR_REQUIRE((int64_t)n * mcap < (1LL << 31) - 1, OSR_ERR_INVALID_ARG, "osr_lvis_match: %d images x %lld groups", n, (long long)mcap);
    OSR_REQUIRE(iou_thrs && area_rng, OSR_ERR_INVALID_ARG, "osr_lvis_match: null pointer (thresholds / area ranges)");
    if (n == 0 || cap == 0) return OSR_OK;
    OSR_REQUIRE(boxes && scores && classes && counts && img_off && ev_gt_off && flags && rank && workspace, OSR_ERR_INVALID_ARG, "osr_lvis_match: null pointer");
    OSR_REQUIRE(num_entries == 0 || (ev_cat && ev_flags), OSR_ERR_INVALID_ARG, "osr_lvis_match: null entry pointer");
    OSR_REQUIRE(num_gt == 0 || (gt_box && gt_area && gt_flags), OSR_ERR_INVALID_ARG, "osr_lvis_match: null ground-truth pointer");
    const int64_t sim_bytes = mcap * num_gt * 8, need = osr_lvis_match_workspace_bytes(n, cap, max_dets, num_gt);
    OSR_REQUIRE(workspace_bytes >= need, OSR_ERR_WORKSPACE, "osr_lvis_match: workspace %lld bytes < %lld", (long long)workspace_bytes, (long long)need);
    double* simm = sim ? sim : (double*)workspace;
    OSR_REQUIRE(((uintptr_t)boxes & 3) == 0 && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)classes & 7) == 0 && ((uintptr_t)counts & 3) == 0 &&
                    ((uintptr_t)img_off & 3) == 0 && ((uintptr_t)ev_cat & 3) == 0 && ((uintptr_t)ev_gt_off & 3) == 0 && ((uintptr_t)gt_box & 7) == 0 &&
                    ((uintptr_t)gt_area & 7) == 0 && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)rank & 3) == 0 && ((uintptr_t)match & 3) == 0 &&
                    ((uintptr_t)sim & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                OSR_ERR_INVALID_ARG, "osr_lvis_match: misaligned pointer");
    LvParams P;
    em_fill_tables(&P.tb, iou_thrs, num_thrs, area_rng, num_areas);
    P.n = n, P.cap = cap, P.K = num_categories, P.T = num_thrs, P.A = num_areas, P.max_dets = max_dets, P.mcap = (int)mcap, P.num_ev = num_entries;
    P.num_gt = num_gt, P.max_group = max_gt_per_group;
    LvTables W;
    W.gcount = (int32_t*)((char*)workspace + sim_bytes);
    W.g_ent = W.gcount + n, W.g_first = W.g_ent + n * mcap, W.g_M = W.g_first + n * mcap, W.s_row = W.g_M + n * mcap;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)n * cap;
    if (!em_preset(flags, rows * num_areas, rank, rows, match, rows * num_areas * num_thrs, st)) {
        osr_set_error("osr_lvis_match: hipMemsetAsync failed");
        return OSR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(lv_group_kernel, dim3(n), dim3(EM_THREADS), 0, st, P, scores, classes, counts, img_off, ev_cat, rank, W);
    OSR_CHECK_LAUNCH("osr_lvis_match (groups)");
    if (num_entries == 0) return OSR_OK;  // (every group count is 0)
    hipLaunchKernelGGL(lv_match_kernel, dim3((unsigned)(n * mcap)), dim3(EM_THREADS), 0, st, P, boxes, ev_gt_off, ev_flags, gt_box, gt_area, gt_flags, W, flags,
                       match, simm);
    OSR_CHECK_LAUNCH("osr_lvis_match (match)");
    return OSR_OK;
}
