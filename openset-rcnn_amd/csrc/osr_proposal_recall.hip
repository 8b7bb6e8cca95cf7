// Class-agnostic box-proposal recall for gfx950 (include/osr.h: osr_proposal_recall, which states every rule): the greedy one-to-one
// matching of an image's ranked proposals to its non-crowd ground truths, for every area range and every proposal limit of a batch,
// in ONE launch. Built with -ffp-contract=off: osr_pairwise_iou rounds like torch's fp32 pairwise_iou on the CPU, so the chosen
// indices, the recorded overlaps and the hit counts equal host/proposal_evaluation.py's bit for bit.
//
// The grid is fixed: one workgroup of 1024 threads (16 waves) per (image, area range, limit). Inside a group:
//   A. the ground truths of the area range are marked and counted (one thread per ground truth);
//   B. the image's rows are ranked: (logit key, ~row) pairs, the bitonic sort of osr_select.h (key descending, row ascending = a stable
//      descending sort), and the boxes of the first min(count, limit) ranks are staged in LDS. The pairs are dead then, and their
//      16 KB take the ground-truth boxes;
//   C. per valid ground truth one wave finds its best live proposal: the largest IoU, the lowest rank among equals. The IoUs are
//      recomputed from the LDS boxes whenever they are needed; no matrix is stored;
//   D. min(live proposals, valid ground truths) rounds. A block arg-max over the cached (IoU, ~ground-truth index) keys picks the
//      pair, the ground truth and the proposal retire, and only the columns whose cached best proposal has just retired are
//      recomputed, one wave per column;
//   E. per threshold the ground truths at or above it are counted with wave ballots.
// Every output address has one writer and the only atomics are integer adds in LDS: repeats are bit-identical.
#include "osr_boxes.h"
#include "osr_eval_match.h"  // (the clamped segment read only: the limits here are PR_*)
#include "osr_select.h"

#define PR_THREADS 1024
#define PR_WAVES (PR_THREADS / 64)
#define PR_MAX_CAP 2048
#define PR_MAX_GT 1024
#define PR_MAX_A 8
#define PR_MAX_L 8
#define PR_MAX_T 16

static_assert(PR_MAX_CAP <= SEL_MAXK, "the ranking is osr_select.h's bitonic sort over at most SEL_MAXK pairs");
static_assert(PR_MAX_GT <= PR_THREADS, "one thread per ground truth");
static_assert(PR_MAX_GT * 16 <= PR_MAX_CAP * 8, "the ground-truth boxes take the place of the sorted pairs");

struct PrParams {
    float rng[PR_MAX_A * 2];
    float thr[PR_MAX_T];
    int limit[PR_MAX_L];
    int n, cap, A, L, T, num_gt, max_gt;
};

// the best live proposal of ground truth g: the largest IoU, equal IoUs to the lowest rank. Called by one full wave; every lane returns
// the result. PRECONDITION: at least one rank < live is not retired.
__device__ __forceinline__ void pr_column_best(const float4 g, const float4* __restrict__ rbox, const unsigned long long* __restrict__ retired, int live,
                                               float* iou, int* rank) {
    const int lane = threadIdx.x & 63;
    float s = -1.f;
    int k = 0x7fffffff;
    for (int r = lane; r < live; r += 64) {
        if ((retired[r >> 6] >> (r & 63)) & 1ull) continue;
        const float v = osr_pairwise_iou(rbox[r], g);
        if (v > s) s = v, k = r;  // (ascending r: the first of equals stays)
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float os = __shfl_xor(s, d, 64);
        const int ok = __shfl_xor(k, d, 64);
        if (os > s || (os == s && ok < k)) s = os, k = ok;
    }
    *iou = s, *rank = k;
}

__global__ __launch_bounds__(PR_THREADS) void pr_recall_kernel(PrParams P, const float* __restrict__ boxes, const float* __restrict__ logits,
                                                              const int32_t* __restrict__ counts, const float* __restrict__ gt_boxes,
                                                              const float* __restrict__ gt_area, const int32_t* __restrict__ seg_off,
                                                              int32_t* __restrict__ hits, int32_t* __restrict__ num_pos, float* __restrict__ gt_overlap) {
    __shared__ unsigned long long s_pairs[PR_MAX_CAP];  // B: the sorted pairs; from C on the ground-truth boxes (float4 x PR_MAX_GT)
    __shared__ float4 s_rbox[PR_MAX_CAP];               // the ranked proposal boxes
    __shared__ float s_best[PR_MAX_GT];                 // per ground truth: the IoU of its best live proposal; after its round: its overlap
    __shared__ int s_rank[PR_MAX_GT];                   // that proposal's rank; -1: the ground truth is not in play (invalid or retired)
    __shared__ unsigned long long s_retired[PR_MAX_CAP / 64];
    __shared__ unsigned long long s_red[PR_WAVES];
    __shared__ int s_hits[PR_MAX_T];
    __shared__ int s_count;
    float4* s_gbox = reinterpret_cast<float4*>(s_pairs);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int al = blockIdx.x % (P.A * P.L), i = blockIdx.x / (P.A * P.L);
    const int a = al / P.L, l = al % P.L;
    const int cnt = min(max(counts[i], 0), P.cap);
    int g0, G;
    em_segment(seg_off, i, P.num_gt, P.max_gt, &g0, &G);
    int32_t* my_hits = hits + ((int64_t)(i * P.A + a) * P.L + l) * P.T;
    float* my_ov = gt_overlap ? gt_overlap + (int64_t)(a * P.L + l) * P.num_gt + g0 : nullptr;
    // A. the area range's ground truths
    const float lo = P.rng[a * 2], hi = P.rng[a * 2 + 1];
    const bool skip = cnt == 0 || G == 0;  // the image adds nothing, num_pos included
    bool valid = false;
    if (tid < G && !skip) {
        const float ar = gt_area[g0 + tid];
        valid = lo <= ar && ar <= hi;
    }
    if (tid == 0) s_count = 0;
    if (tid < PR_MAX_T) s_hits[tid] = 0;
    if (tid < PR_MAX_CAP / 64) s_retired[tid] = 0ull;
    __syncthreads();
    {
        const unsigned long long m = __ballot(valid);
        if (lane == 0 && m) atomicAdd(&s_count, __popcll(m));
    }
    __syncthreads();
    const int nvalid = s_count;
    if (l == 0 && tid == 0) num_pos[i * P.A + a] = nvalid;
    if (nvalid == 0) {  // (uniform) nothing to match
        if (tid < P.T) my_hits[tid] = 0;
        if (my_ov && tid < G) my_ov[tid] = -1.f;
        return;
    }
    // B. rank the rows, stage the live boxes
    for (int r = tid; r < cnt; r += PR_THREADS) s_pairs[r] = sel_pair(osr_float_key(logits[(int64_t)i * P.cap + r]), (unsigned)r);
    sel_pad_and_sort(s_pairs, cnt);
    const int live = min(cnt, P.limit[l]);
    for (int r = tid; r < live; r += PR_THREADS) {
        const float* b = boxes + ((int64_t)i * P.cap + sel_pair_index(s_pairs[r])) * 4;
        s_rbox[r] = make_float4(b[0], b[1], b[2], b[3]);
    }
    __syncthreads();  // the pairs are read: their place is the ground-truth boxes' now
    if (tid < G) {
        const float* g = gt_boxes + (int64_t)(g0 + tid) * 4;
        s_gbox[tid] = make_float4(g[0], g[1], g[2], g[3]);
        s_best[tid] = 0.f;  // a ground truth that is never chosen keeps 0
        s_rank[tid] = valid ? 0 : -1;
    }
    __syncthreads();
    // C. every valid column's best proposal
    for (int j = wave; j < G; j += PR_WAVES) {
        if (s_rank[j] < 0) continue;  // (uniform in the wave)
        float s;
        int k;
        pr_column_best(s_gbox[j], s_rbox, s_retired, live, &s, &k);
        if (lane == 0) s_best[j] = s, s_rank[j] = k;
    }
    __syncthreads();
    // D. the rounds
    const int rounds = min(live, nvalid);
    for (int round = 0; round < rounds; ++round) {
        // the pair: IoU descending, then ground-truth index ascending (an IoU is >= +0, so its bits order like the value)
        unsigned long long key = 0ull;
        if (tid < G && s_rank[tid] >= 0) key = ((unsigned long long)__float_as_uint(s_best[tid]) << 32) | (0xffffffffu - (unsigned)tid);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long o = __shfl_xor(key, d, 64);
            key = o > key ? o : key;
        }
        if (lane == 0) s_red[wave] = key;
        __syncthreads();
        key = s_red[0];
#pragma unroll
        for (int w = 1; w < PR_WAVES; ++w) key = s_red[w] > key ? s_red[w] : key;
        const int jw = (int)(0xffffffffu - (unsigned)key);  // (rounds <= valid ground truths: there is always one in play)
        const int kw = s_rank[jw];
        __syncthreads();  // s_rank[jw] and s_red are read by all
        if (tid == 0) {
            s_rank[jw] = -1;  // retired; s_best[jw] stays: it is the recorded overlap
            s_retired[kw >> 6] |= 1ull << (kw & 63);
        }
        __syncthreads();
        if (round + 1 == rounds) break;
        for (int j = wave; j < G; j += PR_WAVES) {
            if (s_rank[j] != kw) continue;  // (uniform in the wave; a retired or invalid column holds -1)
            float s;
            int k;
            pr_column_best(s_gbox[j], s_rbox, s_retired, live, &s, &k);
            if (lane == 0) s_best[j] = s, s_rank[j] = k;
        }
        __syncthreads();
    }
    // E. the overlaps and the hits. A column still in play was never chosen: its overlap is 0
    float ov = -1.f;
    if (tid < G && valid) ov = s_rank[tid] >= 0 ? 0.f : s_best[tid];
    if (my_ov && tid < G) my_ov[tid] = ov;
    for (int t = 0; t < P.T; ++t) {
        const unsigned long long m = __ballot(valid && ov >= P.thr[t]);
        if (lane == 0 && m) atomicAdd(&s_hits[t], __popcll(m));
    }
    __syncthreads();
    if (tid < P.T) my_hits[tid] = s_hits[tid];
}

extern "C" osr_status osr_proposal_recall(const float* boxes, const float* logits, const int32_t* counts, int32_t n, int32_t cap, const float* gt_boxes,
                                          const float* gt_area, const int32_t* seg_off, int32_t num_gt, int32_t max_gt_per_image,
                                          const float* area_ranges, int32_t num_areas, const int32_t* limits, int32_t num_limits,
                                          const float* thresholds, int32_t num_thrs, int32_t* hits, int32_t* num_pos, float* gt_overlap, void* stream) {
    OSR_REQUIRE(n >= 0 && cap >= 0 && num_gt >= 0 && max_gt_per_image >= 0, OSR_ERR_INVALID_ARG,
                "osr_proposal_recall: n %d, cap %d, num_gt %d, max_gt_per_image %d", n, cap, num_gt, max_gt_per_image);
    OSR_REQUIRE(num_areas >= 1 && num_areas <= PR_MAX_A, OSR_ERR_INVALID_ARG, "osr_proposal_recall: %d area ranges, 1 .. %d", num_areas, PR_MAX_A);
    OSR_REQUIRE(num_limits >= 1 && num_limits <= PR_MAX_L, OSR_ERR_INVALID_ARG, "osr_proposal_recall: %d limits, 1 .. %d", num_limits, PR_MAX_L);
    OSR_REQUIRE(num_thrs >= 1 && num_thrs <= PR_MAX_T, OSR_ERR_INVALID_ARG, "osr_proposal_recall: %d thresholds, 1 .. %d", num_thrs, PR_MAX_T);
    OSR_REQUIRE(area_ranges && limits && thresholds, OSR_ERR_INVALID_ARG, "osr_proposal_recall: null pointer (area ranges / limits / thresholds)");
    for (int l = 0; l < num_limits; ++l) OSR_REQUIRE(limits[l] >= 1, OSR_ERR_INVALID_ARG, "osr_proposal_recall: limit %d is %d, at least 1", l, limits[l]);
    OSR_REQUIRE(cap <= PR_MAX_CAP, OSR_ERR_UNSUPPORTED, "osr_proposal_recall: cap %d, at most %d rows per image", cap, PR_MAX_CAP);
    OSR_REQUIRE(max_gt_per_image <= PR_MAX_GT, OSR_ERR_UNSUPPORTED, "osr_proposal_recall: %d ground truths in one image, at most %d", max_gt_per_image,
                PR_MAX_GT);
    OSR_REQUIRE((int64_t)n * num_areas * num_limits < (1LL << 31) - 1, OSR_ERR_INVALID_ARG, "osr_proposal_recall: %d images x %d area ranges x %d limits", n,
                num_areas, num_limits);
    if (n == 0) return OSR_OK;
    OSR_REQUIRE(counts && seg_off && hits && num_pos && (cap == 0 || (boxes && logits)), OSR_ERR_INVALID_ARG, "osr_proposal_recall: null pointer");
    OSR_REQUIRE(num_gt == 0 || (gt_boxes && gt_area), OSR_ERR_INVALID_ARG, "osr_proposal_recall: null ground-truth pointer");
    OSR_REQUIRE(((uintptr_t)boxes & 3) == 0 && ((uintptr_t)logits & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)gt_boxes & 3) == 0 &&
                    ((uintptr_t)gt_area & 3) == 0 && ((uintptr_t)seg_off & 3) == 0 && ((uintptr_t)hits & 3) == 0 && ((uintptr_t)num_pos & 3) == 0 &&
                    ((uintptr_t)gt_overlap & 3) == 0,
                OSR_ERR_INVALID_ARG, "osr_proposal_recall: misaligned pointer");
    PrParams P;
    for (int a = 0; a < PR_MAX_A * 2; ++a) P.rng[a] = a < num_areas * 2 ? area_ranges[a] : 0.f;
    for (int t = 0; t < PR_MAX_T; ++t) P.thr[t] = t < num_thrs ? thresholds[t] : 2.f;
    for (int l = 0; l < PR_MAX_L; ++l) P.limit[l] = l < num_limits ? limits[l] : 1;
    P.n = n, P.cap = cap, P.A = num_areas, P.L = num_limits, P.T = num_thrs, P.num_gt = num_gt, P.max_gt = max_gt_per_image;
    hipLaunchKernelGGL(pr_recall_kernel, dim3(n * num_areas * num_limits), dim3(PR_THREADS), 0, (hipStream_t)stream, P, boxes, logits, counts, gt_boxes,
                       gt_area, seg_off, hits, num_pos, gt_overlap);
    OSR_CHECK_LAUNCH("osr_proposal_recall");
    return OSR_OK;
}
