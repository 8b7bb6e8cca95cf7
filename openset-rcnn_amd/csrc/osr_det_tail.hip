// Second-stage tail kernels for gfx950 (include/osr.h): box predictor tail, segmented stable sort + greedy
// per-class NMS + top-k, row gather, L2 normalise, PLN tail, softmax-classifier candidates, final assembly.
//
// Reference call sites (/root/reference/openset_rcnn/modeling/roi_heads/):
//   osrcnn_fast_rcnn.py:89-145,248-264,403-450   prototype_learning_network.py:189-230
//   softmax_classifier.py:47-168,287-346
// Compile with -ffp-contract=off: IoU / clip / threshold arithmetic must round like the oracle's so that
// kept-index lists are bit-exact.
#include "osr_common.h"
#include "osr_boxes.h"
#include "osr_loss_common.h"
#include "osr_pln_dist.h"
#include "osr_select.h"

// ------------------------------------------------------------------------------------------------------
// box predictor tail: wave per RoI row
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void box_pred_tail_kernel(const float* __restrict__ x, long long m, int k,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            const float* __restrict__ proposals, const float* __restrict__ ctr,
                                                            const int* __restrict__ batch_idx, const int* __restrict__ image_hw,
                                                            float wx, float wy, float ww, float wh, int mean_type, float score_thresh,
                                                            float* __restrict__ pred_deltas, float* __restrict__ pred_iou,
                                                            float* __restrict__ boxes, float* __restrict__ score, int* __restrict__ cand) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];  // [5][k]
    for (int i = threadIdx.x; i < 5 * k; i += blockDim.x) s_w[i] = w[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long r = (long long)blockIdx.x * nw + wid; r < m; r += (long long)gridDim.x * nw) {
        const int bi = batch_idx[r];
        if (bi < 0) {
            if (lane == 0) {
                *reinterpret_cast<float4*>(pred_deltas + r * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(boxes + r * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                pred_iou[r] = 0.f; score[r] = 0.f; cand[r] = 0;
            }
            continue;
        }
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, d4 = 0.f;
        const float* row = x + r * k;
        for (int c = lane * 4; c < k; c += 256) {
            const float4 q = *reinterpret_cast<const float4*>(row + c);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d0 += v[j] * s_w[c + j];
                d1 += v[j] * s_w[k + c + j];
                d2 += v[j] * s_w[2 * k + c + j];
                d3 += v[j] * s_w[3 * k + c + j];
                d4 += v[j] * s_w[4 * k + c + j];
            }
        }
        d0 = osr_wave_sum(d0); d1 = osr_wave_sum(d1); d2 = osr_wave_sum(d2); d3 = osr_wave_sum(d3); d4 = osr_wave_sum(d4);
        if (lane == 0) {
            d0 += b[0]; d1 += b[1]; d2 += b[2]; d3 += b[3];
            const float iou = 1.0f / (1.0f + expf(-(d4 + b[4])));
            const float4 p = *reinterpret_cast<const float4*>(proposals + r * 4);
            bool valid;
            const float4 box = osr_b2b_decode(p, make_float4(d0, d1, d2, d3), make_float4(wx, wy, ww, wh), &valid);
            const float c_ = ctr[r];
            const float s = mean_type == 0 ? sqrtf(iou * c_) : (iou + c_) / 2.0f;
            const float ih = (float)image_hw[bi * 2], iw = (float)image_hw[bi * 2 + 1];
            *reinterpret_cast<float4*>(pred_deltas + r * 4) = make_float4(d0, d1, d2, d3);
            pred_iou[r] = iou;
            *reinterpret_cast<float4*>(boxes + r * 4) = osr_box_clip(box, iw, ih);
            score[r] = s;
            cand[r] = (valid && osr_finite(s) && s > score_thresh) ? 1 : 0;
        }
    }
}

extern "C" osr_status osr_box_predictor_tail(const float* x, int64_t m, int32_t k, const float* w, const float* b,
                                             const float* proposals, const float* ctr, const int32_t* batch_idx,
                                             const int32_t* image_hw, const float reg_weights[4], int32_t mean_type,
                                             float score_thresh, float* pred_deltas, float* pred_iou, float* boxes,
                                             float* score, int32_t* cand, void* stream) {
    OSR_REQUIRE(x && w && b && proposals && ctr && batch_idx && image_hw && reg_weights && pred_deltas && pred_iou && boxes && score && cand,
                OSR_ERR_INVALID_ARG, "osr_box_predictor_tail: null pointer");
    OSR_REQUIRE(k > 0 && k % 4 == 0 && k <= 3072, OSR_ERR_UNSUPPORTED, "osr_box_predictor_tail: k must be a multiple of 4 and <= 3072, got %d", k);
    OSR_REQUIRE(m >= 0 && (mean_type == 0 || mean_type == 1), OSR_ERR_INVALID_ARG, "osr_box_predictor_tail: bad m / mean_type");
    if (m == 0) return OSR_OK;
    long long blocks = (m + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(box_pred_tail_kernel, dim3((unsigned)blocks), dim3(256), (size_t)5 * k * 4, (hipStream_t)stream, x, (long long)m, k, w, b,
                       proposals, ctr, batch_idx, image_hw, reg_weights[0], reg_weights[1], reg_weights[2], reg_weights[3], mean_type,
                       score_thresh, pred_deltas, pred_iou, boxes, score, cand);
    OSR_CHECK_LAUNCH("osr_box_predictor_tail");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// segmented stable sort (score desc, index asc) + greedy NMS + top-k
// ------------------------------------------------------------------------------------------------------
#define SORT_THREADS 1024
#define SORT_LDS_CAP 8192

static inline long long pow2ceil(long long v) { long long p = 1; while (p < v) p <<= 1; return p; }

// workspace per segment: order[seg_stride] int32, then (16-byte aligned) keys[pow2ceil(seg_stride)] u64
__global__ __launch_bounds__(SORT_THREADS) void seg_sort_kernel(const float* __restrict__ scores, const int* __restrict__ cand,
                                                                long long seg_stride, const int* __restrict__ seg_len,
                                                                int* __restrict__ ws_order, int* __restrict__ ws_count,
                                                                unsigned long long* __restrict__ ws_keys, long long keys_stride, int lds_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];  // [lds_cap] keys, then 32 ints of scan scratch
    int* s_scan = reinterpret_cast<int*>(s_keys + lds_cap);
    const int seg = blockIdx.x, tid = threadIdx.x;
    long long len = seg_len[seg];
    if (len > seg_stride) len = seg_stride;
    if (len < 0) len = 0;
    const float* sc = scores + seg * seg_stride;
    const int* cd = cand ? cand + seg * seg_stride : nullptr;
    int* order = ws_order + seg * seg_stride;
    int np = 1;
    while (np < len) np <<= 1;
    const bool in_lds = np <= lds_cap;
    unsigned long long* gk = ws_keys + seg * keys_stride;
    int nvalid = 0;
    for (int i = tid; i < np; i += blockDim.x) {
        unsigned long long key = 0ull;
        if (i < len && (!cd || cd[i])) {
            key = sel_pair(osr_float_key(sc[i]), (unsigned int)i);
            ++nvalid;
        }
        if (in_lds) s_keys[i] = key; else gk[i] = key;
    }
    int tot;
    osr_block_excl_scan(nvalid, s_scan, &tot);
    __syncthreads();
    if (in_lds) bitonic_desc(s_keys, np); else bitonic_desc(gk, np);
    for (int i = tid; i < tot; i += blockDim.x) order[i] = sel_pair_index(in_lds ? s_keys[i] : gk[i]);
    if (tid == 0) ws_count[seg] = tot;
}

// The kept boxes sit in LDS: 24 bytes each. Up to 1024 (every inference list, the stock RPN's POST_NMS_TOPK_TRAIN 1000) the kernel is the
// one it always was; a longer list -- [d2]'s cascade configs train on POST_NMS_TOPK_TRAIN 2000 proposals -- takes the 2048-entry
// instantiation (48 KB of static LDS for its one wave).
#define NMS_MAX_TOPK 2048

template <int CAP>
__global__ __launch_bounds__(64) void nms_greedy_kernel(const float* __restrict__ boxes, const int* __restrict__ cls, long long seg_stride,
                                                        const int* __restrict__ ws_order, const int* __restrict__ ws_count, float thr,
                                                        int topk, int* __restrict__ keep, int* __restrict__ keep_count) {
    __shared__ float4 s_box[CAP];
    __shared__ float s_area[CAP];
    __shared__ int s_cls[CAP];
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int n = ws_count[seg];
    const int* order = ws_order + seg * seg_stride;
    const float* bx = boxes + seg * seg_stride * 4;
    const int* cl = cls ? cls + seg * seg_stride : nullptr;
    int* kp = keep + (long long)seg * topk;
    if (thr >= 1.0f) {  // IoU > thr can never hold: pure sort + top-k
        const int nk = n < topk ? n : topk;
        for (int i = lane; i < nk; i += 64) kp[i] = order[i];
        for (int i = nk + lane; i < topk; i += 64) kp[i] = -1;
        if (lane == 0) keep_count[seg] = nk;
        return;
    }
    int nkept = 0;
    for (int base = 0; base < n && nkept < topk; base += 64) {
        const int j = base + lane;
        bool alive = j < n;
        int idx = -1, c = 0;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        float area = 0.f;
        if (alive) {
            idx = order[j];
            q = *reinterpret_cast<const float4*>(bx + (long long)idx * 4);
            c = cl ? cl[idx] : 0;
            area = (q.z - q.x) * (q.w - q.y);
            for (int t = 0; t < nkept; ++t) {
                if (s_cls[t] != c) continue;
                const float4 kq = s_box[t];
                const float xx1 = fmaxf(kq.x, q.x), yy1 = fmaxf(kq.y, q.y), xx2 = fminf(kq.z, q.z), yy2 = fminf(kq.w, q.w);
                const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
                const float inter = w * h;
                const float ovr = inter / (s_area[t] + area - inter);
                if (ovr > thr) { alive = false; break; }
            }
        }
        unsigned long long msk = __ballot(alive);
        while (msk && nkept < topk) {
            const int i = __ffsll((long long)msk) - 1;
            const float ix1 = __shfl(q.x, i, 64), iy1 = __shfl(q.y, i, 64), ix2 = __shfl(q.z, i, 64), iy2 = __shfl(q.w, i, 64);
            const float ia = __shfl(area, i, 64);
            const int ic = __shfl(c, i, 64), iidx = __shfl(idx, i, 64);
            if (lane == 0) {
                s_box[nkept] = make_float4(ix1, iy1, ix2, iy2);
                s_area[nkept] = ia;
                s_cls[nkept] = ic;
                kp[nkept] = iidx;
            }
            ++nkept;
            if (lane == i) alive = false;
            if (alive && lane > i && c == ic) {
                const float xx1 = fmaxf(ix1, q.x), yy1 = fmaxf(iy1, q.y), xx2 = fminf(ix2, q.z), yy2 = fminf(iy2, q.w);
                const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
                const float inter = w * h;
                const float ovr = inter / (ia + area - inter);
                if (ovr > thr) alive = false;
            }
            msk = __ballot(alive && lane > i);
        }
        __syncthreads();  // single wave: orders lane 0's LDS writes before the next chunk's reads
    }
    for (int i = nkept + lane; i < topk; i += 64) kp[i] = -1;
    if (lane == 0) keep_count[seg] = nkept;
}

static void nms_ws_layout(int num_segments, long long seg_stride, long long* off_count, long long* off_keys, long long* keys_stride, long long* total) {
    long long order_bytes = (long long)num_segments * seg_stride * 4;
    long long oc = (order_bytes + 15) / 16 * 16;
    long long ok = oc + ((long long)num_segments * 4 + 15) / 16 * 16;
    long long ks = pow2ceil(seg_stride);
    *off_count = oc; *off_keys = ok; *keys_stride = ks;
    *total = ok + (long long)num_segments * ks * 8;
}

extern "C" int64_t osr_nms_topk_workspace_bytes(int32_t num_segments, int64_t seg_stride) {
    if (num_segments < 1 || seg_stride < 1 || seg_stride > (1ll << 24)) { osr_set_error("osr_nms_topk_workspace_bytes: bad arguments"); return OSR_ERR_INVALID_ARG; }
    long long a, b, c, t;
    nms_ws_layout(num_segments, seg_stride, &a, &b, &c, &t);
    return t;
}

extern "C" osr_status osr_nms_topk(const float* boxes, const float* scores, const int32_t* cls, const int32_t* cand,
                                   int32_t num_segments, int64_t seg_stride, const int32_t* seg_len, float thr, int32_t topk,
                                   int32_t* keep, int32_t* keep_count, void* workspace, int64_t workspace_bytes, void* stream) {
    OSR_REQUIRE(boxes && scores && seg_len && keep && keep_count && workspace, OSR_ERR_INVALID_ARG, "osr_nms_topk: null pointer");
    OSR_REQUIRE(num_segments >= 1 && seg_stride >= 1 && seg_stride <= (1ll << 24), OSR_ERR_INVALID_ARG, "osr_nms_topk: bad segment geometry");
    OSR_REQUIRE(topk >= 1, OSR_ERR_INVALID_ARG, "osr_nms_topk: topk must be >= 1");
    OSR_REQUIRE(thr >= 1.0f || topk <= NMS_MAX_TOPK, OSR_ERR_UNSUPPORTED, "osr_nms_topk: topk > %d needs thr >= 1", NMS_MAX_TOPK);
    OSR_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)boxes & 15) == 0, OSR_ERR_INVALID_ARG, "osr_nms_topk: boxes/workspace must be 16-byte aligned");
    long long oc, ok, ks, total;
    nms_ws_layout(num_segments, seg_stride, &oc, &ok, &ks, &total);
    OSR_REQUIRE(workspace_bytes >= total, OSR_ERR_WORKSPACE, "osr_nms_topk: workspace %lld < %lld bytes", (long long)workspace_bytes, total);
    char* ws = (char*)workspace;
    int* ws_order = (int*)ws;
    int* ws_count = (int*)(ws + oc);
    unsigned long long* ws_keys = (unsigned long long*)(ws + ok);
    hipStream_t st = (hipStream_t)stream;
    long long np = pow2ceil(seg_stride);
    const int lds_cap = (int)(np <= SORT_LDS_CAP ? np : SORT_LDS_CAP);
    const size_t smem = (size_t)lds_cap * 8 + 128;
    static osr_dev_mask attr_set{0};
    osr_once_per_device(attr_set, [] {  // > 64 KB of dynamic LDS needs the opt-in (per device); 160 KB per CU on gfx950
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(seg_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SORT_LDS_CAP * 8 + 128);
    });
    hipLaunchKernelGGL(seg_sort_kernel, dim3(num_segments), dim3(SORT_THREADS), smem, st, scores, cand, (long long)seg_stride, seg_len, ws_order,
                       ws_count, ws_keys, ks, lds_cap);
    OSR_CHECK_LAUNCH("osr_nms_topk(sort)");
    if (topk <= 1024)
        hipLaunchKernelGGL(nms_greedy_kernel<1024>, dim3(num_segments), dim3(64), 0, st, boxes, cls, (long long)seg_stride, ws_order, ws_count, thr,
                           topk, keep, keep_count);
    else  // (thr >= 1 never touches the table: any topk)
        hipLaunchKernelGGL(nms_greedy_kernel<NMS_MAX_TOPK>, dim3(num_segments), dim3(64), 0, st, boxes, cls, (long long)seg_stride, ws_order, ws_count,
                           thr, topk, keep, keep_count);
    OSR_CHECK_LAUNCH("osr_nms_topk(nms)");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// gather rows
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, long long seg_stride, int row_elems,
                                                          const int* __restrict__ keep, const int* __restrict__ keep_count, int topk,
                                                          float* __restrict__ dst) {
    const int j = blockIdx.x, seg = blockIdx.y;
    float* d = dst + ((long long)seg * topk + j) * row_elems;
    const int cnt = keep_count[seg];
    const int idx = j < cnt ? keep[(long long)seg * topk + j] : -1;
    if (idx < 0) {
        for (int i = threadIdx.x; i < row_elems; i += blockDim.x) d[i] = 0.f;
        return;
    }
    const float* s = src + (seg * seg_stride + idx) * row_elems;
    if ((row_elems & 3) == 0) {
        for (int i = threadIdx.x * 4; i < row_elems; i += blockDim.x * 4)
            *reinterpret_cast<float4*>(d + i) = *reinterpret_cast<const float4*>(s + i);
    } else {
        for (int i = threadIdx.x; i < row_elems; i += blockDim.x) d[i] = s[i];
    }
}

extern "C" osr_status osr_gather_rows(const float* src, int64_t seg_stride, int32_t row_elems, const int32_t* keep,
                                      const int32_t* keep_count, int32_t num_segments, int32_t topk, float* dst, void* stream) {
    OSR_REQUIRE(src && keep && keep_count && dst, OSR_ERR_INVALID_ARG, "osr_gather_rows: null pointer");
    OSR_REQUIRE(num_segments >= 1 && num_segments <= 65535 && topk >= 1 && row_elems >= 1 && seg_stride >= 1, OSR_ERR_INVALID_ARG, "osr_gather_rows: bad sizes");
    OSR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_gather_rows: src/dst must be 16-byte aligned");
    const int threads = row_elems >= 1024 ? 256 : 64;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(topk, num_segments), dim3(threads), 0, (hipStream_t)stream, src, (long long)seg_stride, row_elems,
                       keep, keep_count, topk, dst);
    OSR_CHECK_LAUNCH("osr_gather_rows");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// L2 normalise rows (F.normalize): x / max(||x||, 1e-12); wave per row
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2norm_kernel(const float* __restrict__ x, int rows, int d, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    float ss = 0.f;
    for (int i = lane; i < d; i += 64) { float v = x[(long long)r * d + i]; ss += v * v; }
    ss = osr_wave_sum(ss);
    if (ss > 3.402823466e38f) {  // the sum of squares left fp32's range (wave-uniform): norm = max|x| * ||x / max|x|||
        float mx = 0.f;
        for (int i = lane; i < d; i += 64) mx = fmaxf(mx, fabsf(x[(long long)r * d + i]));
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
        if (osr_finite(mx)) {  // (a row that holds an Inf keeps the plain form below)
            float s2 = 0.f;
            for (int i = lane; i < d; i += 64) { float v = x[(long long)r * d + i] / mx; s2 += v * v; }
            const float nrm = sqrtf(osr_wave_sum(s2));
            for (int i = lane; i < d; i += 64) out[(long long)r * d + i] = x[(long long)r * d + i] / mx / nrm;
            return;
        }
    }
    const float den = fmaxf(sqrtf(ss), 1e-12f);
    for (int i = lane; i < d; i += 64) out[(long long)r * d + i] = x[(long long)r * d + i] / den;
}

extern "C" osr_status osr_l2_normalize_rows(const float* x, int32_t rows, int32_t d, float* out, void* stream) {
    OSR_REQUIRE(rows >= 0 && d >= 1, OSR_ERR_INVALID_ARG, "osr_l2_normalize_rows: bad arguments");
    if (rows == 0) return OSR_OK;  // (an empty tensor has no storage: its pointers may be null)
    OSR_REQUIRE(x && out, OSR_ERR_INVALID_ARG, "osr_l2_normalize_rows: null pointer");
    hipLaunchKernelGGL(l2norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, rows, d, out);
    OSR_CHECK_LAUNCH("osr_l2_normalize_rows");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// PLN tail: wave per embedding row
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pln_tail_kernel(const float* __restrict__ emb, long long rows, int d,
                                                       const float* __restrict__ protos, int num_known, int reps, int dist_type, float unk_thr,
                                                       long long unknown_id, const long long* __restrict__ class_map,
                                                       const int* __restrict__ rows_valid, int seg_rows,
                                                       long long* __restrict__ pred_class, float* __restrict__ min_dist) {
    extern __shared__ __attribute__((aligned(16))) float s_p[];  // [num_known*reps][d]
    const int np = num_known * reps;
    for (int i = threadIdx.x; i < np * d; i += blockDim.x) s_p[i] = protos[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long r = (long long)blockIdx.x * nw + wid; r < rows; r += (long long)gridDim.x * nw) {
        if (rows_valid) {
            const long long seg = r / seg_rows;
            if ((int)(r - seg * seg_rows) >= rows_valid[seg]) {
                if (lane == 0) { pred_class[r] = -1; min_dist[r] = 0.f; }
                continue;
            }
        }
        const float* e = emb + r * d;
        float ss = 0.f;
        for (int i = lane; i < d; i += 64) { float v = e[i]; ss += v * v; }
        ss = osr_wave_sum(ss);
        const float den = fmaxf(sqrtf(ss), 1e-12f);
        float best = 0.f;
        int best_c = -1;
        for (int c = 0; c < num_known; ++c) {
            float md = 0.f;
            for (int q = 0; q < reps; ++q) {
                const float* p = s_p + (long long)(c * reps + q) * d;
                const float dist = osr_pln_distance([&](int i) { return e[i] / den; }, p, d, lane, dist_type);
                md = (q == 0 || dist < md) ? dist : md;
            }
            if (best_c < 0 || md < best) { best = md; best_c = c; }  // strict <: lower class wins ties
        }
        if (lane == 0) {
            long long cls = class_map ? class_map[best_c] : (long long)best_c;
            if (best > unk_thr) cls = unknown_id;
            pred_class[r] = cls;
            min_dist[r] = best;
        }
    }
}

extern "C" osr_status osr_pln_tail_ex(const float* emb, int64_t rows, int32_t d, const float* protos_normed, int32_t num_known,
                                      int32_t reps, int32_t distance_type, float unk_thr, int64_t unknown_id, const int64_t* class_map,
                                      const int32_t* rows_valid, int32_t seg_rows, int64_t* pred_class, float* min_dist, void* stream) {
    OSR_REQUIRE(distance_type >= OSR_DIST_COS && distance_type <= OSR_DIST_L2, OSR_ERR_INVALID_ARG, "osr_pln_tail: distance_type %d", distance_type);
    OSR_REQUIRE(emb && protos_normed && pred_class && min_dist, OSR_ERR_INVALID_ARG, "osr_pln_tail: null pointer");
    OSR_REQUIRE(rows >= 0 && d >= 1 && num_known >= 1 && reps >= 1, OSR_ERR_INVALID_ARG, "osr_pln_tail: bad sizes");
    OSR_REQUIRE((long long)num_known * reps * d <= 36864, OSR_ERR_UNSUPPORTED, "osr_pln_tail: prototypes exceed the 144 KB LDS table");
    OSR_REQUIRE(!rows_valid || seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_pln_tail: seg_rows must be >= 1 with rows_valid");
    // (a trailing partial segment would index rows_valid past its last entry)
    OSR_REQUIRE(!rows_valid || rows % seg_rows == 0, OSR_ERR_INVALID_ARG, "osr_pln_tail: rows %lld is not a whole number of %d-row segments",
                (long long)rows, seg_rows);
    if (rows == 0) return OSR_OK;
    long long blocks = (rows + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    size_t smem = (size_t)num_known * reps * d * 4;
    if (smem > 64 * 1024) {
        static osr_dev_mask attr{0};
        osr_once_per_device(attr, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pln_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024); });
    }
    hipLaunchKernelGGL(pln_tail_kernel, dim3((unsigned)blocks), dim3(256), smem, (hipStream_t)stream, emb, (long long)rows, d, protos_normed,
                       num_known, reps, distance_type, unk_thr, (long long)unknown_id, (const long long*)class_map, rows_valid, seg_rows,
                       (long long*)pred_class, min_dist);
    OSR_CHECK_LAUNCH("osr_pln_tail");
    return OSR_OK;
}

extern "C" osr_status osr_pln_tail(const float* emb, int64_t rows, int32_t d, const float* protos_normed, int32_t num_known,
                                   int32_t reps, float unk_thr, int64_t unknown_id, const int64_t* class_map,
                                   const int32_t* rows_valid, int32_t seg_rows, int64_t* pred_class, float* min_dist, void* stream) {
    return osr_pln_tail_ex(emb, rows, d, protos_normed, num_known, reps, OSR_DIST_COS, unk_thr, unknown_id, class_map, rows_valid, seg_rows, pred_class,
                           min_dist, stream);
}

// ------------------------------------------------------------------------------------------------------
// softmax classifier candidates: block per image, thread per detection
// ------------------------------------------------------------------------------------------------------
#define SM_MAX_KNOWN 64

// The candidates of one row, written from slot q on: every class c < K with score(c) > thresh, in class order, as (box(c), score,
// class, row). The emit half of the scan-then-emit loop of softmax_cand_kernel and cand_kernel.
template <class Score, class Box>
__device__ __forceinline__ void cand_emit_row(int K, float thresh, Score score, Box box, long long q, int row, float* __restrict__ o_boxes,
                                              float* __restrict__ o_scores, int* __restrict__ o_cls, int* __restrict__ o_row) {
    for (int c = 0; c < K; ++c) {
        const float p = score(c);
        if (p > thresh) {
            *reinterpret_cast<float4*>(o_boxes + q * 4) = box(c);
            o_scores[q] = p; o_cls[q] = c; o_row[q] = row;
            ++q;
        }
    }
}

__global__ __launch_bounds__(1024) void softmax_cand_kernel(const float* __restrict__ logits, int K, const float* __restrict__ det_boxes,
                                                            const float* __restrict__ det_scores, const long long* __restrict__ pred_class,
                                                            const int* __restrict__ det_count, int seg_rows, long long unknown_id,
                                                            float known_thresh, float unknown_thresh, float* __restrict__ k_boxes,
                                                            float* __restrict__ k_scores, int* __restrict__ k_cls, int* __restrict__ k_det,
                                                            int* __restrict__ k_count, float* __restrict__ u_boxes, float* __restrict__ u_scores,
                                                            int* __restrict__ u_det, int* __restrict__ u_count) {
    __shared__ int s_scan[32];
    const int img = blockIdx.x, tid = threadIdx.x;
    int cnt = det_count[img];
    if (cnt > seg_rows) cnt = seg_rows;
    const long long kcap = (long long)seg_rows * K;
    int run_k = 0, run_u = 0;
    for (int j0 = 0; j0 < seg_rows; j0 += blockDim.x) {
        const int j = j0 + tid;
        const long long r = (long long)img * seg_rows + j;
        int nk = 0, nu = 0;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        float mx = 0.f, sum = 1.f;
        bool known = false, okbox = false;
        if (j < cnt) {
            bx = *reinterpret_cast<const float4*>(det_boxes + r * 4);
            okbox = osr_box_finite(bx);
            const long long pc = pred_class[r];
            known = pc != unknown_id;
            if (known) {
                const float* lg = logits + r * (K + 1);
                mx = osr_softmax_row(lg, K + 1, &sum);
                bool okp = true;
                for (int c = 0; c <= K; ++c) okp = okp && osr_finite(expf(lg[c] - mx) / sum);
                if (okbox && okp)
                    for (int c = 0; c < K; ++c) nk += (expf(lg[c] - mx) / sum) > known_thresh;
            } else {
                const float s = det_scores[r];
                nu = (okbox && osr_finite(s) && s > unknown_thresh) ? 1 : 0;
            }
        }
        int tk, tu;
        const int pk = run_k + osr_block_excl_scan(nk, s_scan, &tk);
        const int pu = run_u + osr_block_excl_scan(nu, s_scan, &tu);
        if (nk) {
            const float* lg = logits + r * (K + 1);
            cand_emit_row(K, known_thresh, [&](int c) { return expf(lg[c] - mx) / sum; }, [&](int) { return bx; }, (long long)img * kcap + pk, j,
                          k_boxes, k_scores, k_cls, k_det);
        }
        if (nu) {
            const long long q = (long long)img * seg_rows + pu;
            *reinterpret_cast<float4*>(u_boxes + q * 4) = bx;
            u_scores[q] = det_scores[r]; u_det[q] = j;
        }
        run_k += tk;
        run_u += tu;
    }
    if (tid == 0) { k_count[img] = run_k; u_count[img] = run_u; }
}

extern "C" osr_status osr_softmax_candidates(const float* logits, int32_t num_known, const float* det_boxes, const float* det_scores,
                                             const int64_t* pred_class, const int32_t* det_count, int32_t n, int32_t seg_rows,
                                             int64_t unknown_id, float known_thresh, float unknown_thresh, float* k_boxes,
                                             float* k_scores, int32_t* k_cls, int32_t* k_det, int32_t* k_count, float* u_boxes,
                                             float* u_scores, int32_t* u_det, int32_t* u_count, void* stream) {
    OSR_REQUIRE(logits && det_boxes && det_scores && pred_class && det_count && k_boxes && k_scores && k_cls && k_det && k_count && u_boxes &&
                    u_scores && u_det && u_count, OSR_ERR_INVALID_ARG, "osr_softmax_candidates: null pointer");
    OSR_REQUIRE(n >= 1 && seg_rows >= 1 && num_known >= 1 && num_known <= SM_MAX_KNOWN, OSR_ERR_INVALID_ARG, "osr_softmax_candidates: bad sizes");
    OSR_REQUIRE((((uintptr_t)det_boxes | (uintptr_t)k_boxes | (uintptr_t)u_boxes) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_softmax_candidates: box arrays must be 16-byte aligned");
    hipLaunchKernelGGL(softmax_cand_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, logits, num_known, det_boxes, det_scores,
                       (const long long*)pred_class, det_count, seg_rows, (long long)unknown_id, known_thresh, unknown_thresh, k_boxes, k_scores,
                       k_cls, k_det, k_count, u_boxes, u_scores, u_det, u_count);
    OSR_CHECK_LAUNCH("osr_softmax_candidates");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// [d2] FastRCNNOutputLayers.inference -> fast_rcnn_inference_single_image, everything before the NMS, for StandardROIHeads (BASELINE
// config 1: Base-RCNN-FPN.yaml) and, with S score sets, for CascadeROIHeads._forward_box behind its last stage: softmax over K+1
// logits (the mean of the S stages' softmax scores), Box2BoxTransform decode of the row's box (K*4 deltas per row, 4 when
// class-agnostic), rows with a non-finite box or score dropped, clip, (row, class) pairs with score > score_thresh emitted in
// row-major order (= nonzero()). Block per image, thread per row and pass; S is a compile-time constant.
// A row exists below the image's prefix count (prop_count, StandardROIHeads' lists) and where batch_idx is not negative (the
// cascade's lists, which keep every row's slot from stage to stage); either pointer may be null.
// ------------------------------------------------------------------------------------------------------
#define CAND_MAX_CLASSES 128

struct CandLogits { const float* p[OSR_CASCADE_MAX_STAGES]; };

template <int S>
__device__ __forceinline__ float cand_score(const CandLogits& lg, long long off, int c, const float (&mx)[S], const float (&sum)[S], float inv) {
    float acc = expf(lg.p[0][off + c] - mx[0]) / sum[0];
#pragma unroll
    for (int s = 1; s < S; ++s) acc += expf(lg.p[s][off + c] - mx[s]) / sum[s];
    return S == 1 ? acc : acc * inv;  // (one stage: the factor is exactly 1)
}

template <int S>
__global__ __launch_bounds__(1024) void cand_kernel(CandLogits lg, const float* __restrict__ deltas, int K, int kbox, const float* __restrict__ boxes,
                                                    const int* __restrict__ prop_count, const int* __restrict__ batch_idx, int seg_rows,
                                                    const int* __restrict__ image_hw, float4 rw, float score_thresh, float inv,
                                                    float* __restrict__ c_boxes, float* __restrict__ c_scores, int* __restrict__ c_cls,
                                                    int* __restrict__ c_row, int* __restrict__ c_count) {
    __shared__ int s_scan[32];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int cnt = prop_count ? min(prop_count[img], seg_rows) : seg_rows;
    const long long ccap = (long long)seg_rows * K;
    const float ih = (float)image_hw[img * 2], iw = (float)image_hw[img * 2 + 1];
    int run = 0;
    for (int j0 = 0; j0 < seg_rows; j0 += blockDim.x) {
        const int j = j0 + tid;
        const long long r = (long long)img * seg_rows + j, off = r * (K + 1);
        const float* dl = deltas + r * (long long)kbox * 4;
        const auto delta = [&](int c) { return make_float4(dl[c * 4], dl[c * 4 + 1], dl[c * 4 + 2], dl[c * 4 + 3]); };
        int nk = 0;
        float mx[S], sum[S];
        float4 pb = make_float4(0.f, 0.f, 0.f, 0.f), b0 = pb;
        if (j < cnt && (!batch_idx || batch_idx[r] >= 0)) {
#pragma unroll
            for (int s = 0; s < S; ++s) mx[s] = osr_softmax_row(lg.p[s] + off, K + 1, &sum[s]);
            // one walk over the classes: every score (the background's too) must be finite, the foreground ones are counted
            bool ok = true;
            int above = 0;
            for (int c = 0; c <= K; ++c) {
                const float p = cand_score<S>(lg, off, c, mx, sum, inv);
                ok = ok && osr_finite(p);
                above += c < K && p > score_thresh;
            }
            // every class's decoded box must be valid, or the whole row is dropped (valid_mask over dim 1); b0 ends as the
            // class-agnostic box
            pb = *reinterpret_cast<const float4*>(boxes + r * 4);
            for (int c = 0; c < kbox && ok; ++c) b0 = osr_b2b_decode(pb, delta(c), rw, &ok);
            nk = ok ? above : 0;
        }
        int tot;
        const int pos = run + osr_block_excl_scan(nk, s_scan, &tot);
        if (nk) {  // a class's own box is decoded again here, for the emitted pairs only (its verdict was settled above)
            bool v;
            const auto box = [&](int c) { return osr_box_clip(kbox > 1 ? osr_b2b_decode(pb, delta(c), rw, &v) : b0, iw, ih); };
            cand_emit_row(K, score_thresh, [&](int c) { return cand_score<S>(lg, off, c, mx, sum, inv); }, box, (long long)img * ccap + pos, j,
                          c_boxes, c_scores, c_cls, c_row);
        }
        run += tot;
    }
    if (tid == 0) c_count[img] = run;
}

template <int S>
static void cand_launch(const CandLogits& lg, const float* deltas, int K, int kbox, const float* boxes, const int* prop_count, const int* batch_idx,
                        int n, int seg_rows, const int* image_hw, const float reg_weights[4], float score_thresh, float* c_boxes, float* c_scores,
                        int* c_cls, int* c_row, int* c_count, void* stream) {
    const float inv = (float)(1.0 / (double)S);  // [d2]: sum(scores) * (1.0 / num_stages), the factor rounded to fp32
    hipLaunchKernelGGL(cand_kernel<S>, dim3(n), dim3(1024), 0, (hipStream_t)stream, lg, deltas, K, kbox, boxes, prop_count, batch_idx, seg_rows, image_hw,
                       make_float4(reg_weights[0], reg_weights[1], reg_weights[2], reg_weights[3]), score_thresh, inv, c_boxes, c_scores, c_cls, c_row,
                       c_count);
}

extern "C" osr_status osr_fastrcnn_candidates(const float* logits, const float* deltas, int32_t num_classes, int32_t num_bbox_reg_classes,
                                              const float* prop_boxes, const int32_t* prop_count, int32_t n, int32_t seg_rows,
                                              const int32_t* image_hw, const float reg_weights[4], float score_thresh, float* c_boxes,
                                              float* c_scores, int32_t* c_cls, int32_t* c_row, int32_t* c_count, void* stream) {
    OSR_REQUIRE(logits && deltas && prop_boxes && prop_count && image_hw && reg_weights && c_boxes && c_scores && c_cls && c_row && c_count,
                OSR_ERR_INVALID_ARG, "osr_fastrcnn_candidates: null pointer");
    OSR_REQUIRE(n >= 1 && seg_rows >= 1 && num_classes >= 1 && num_classes <= CAND_MAX_CLASSES && (num_bbox_reg_classes == 1 || num_bbox_reg_classes == num_classes),
                OSR_ERR_INVALID_ARG, "osr_fastrcnn_candidates: bad sizes (1..%d classes; box regression class-agnostic or per class)", CAND_MAX_CLASSES);
    OSR_REQUIRE(reg_weights[0] > 0.f && reg_weights[1] > 0.f && reg_weights[2] > 0.f && reg_weights[3] > 0.f, OSR_ERR_INVALID_ARG,
                "osr_fastrcnn_candidates: regression weights must be positive");
    OSR_REQUIRE((((uintptr_t)prop_boxes | (uintptr_t)c_boxes) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_fastrcnn_candidates: box arrays must be 16-byte aligned");
    CandLogits lg;
    for (int s = 0; s < OSR_CASCADE_MAX_STAGES; ++s) lg.p[s] = logits;
    cand_launch<1>(lg, deltas, num_classes, num_bbox_reg_classes, prop_boxes, prop_count, nullptr, n, seg_rows, image_hw, reg_weights, score_thresh,
                   c_boxes, c_scores, c_cls, c_row, c_count, stream);
    OSR_CHECK_LAUNCH("osr_fastrcnn_candidates");
    return OSR_OK;
}

extern "C" osr_status osr_cascade_candidates(const float* const* logits, int32_t num_stages, const float* deltas, int32_t num_classes,
                                             const float* boxes, const int32_t* batch_idx, int32_t n, int32_t seg_rows, const int32_t* image_hw,
                                             const float reg_weights[4], float score_thresh, float* c_boxes, float* c_scores, int32_t* c_cls,
                                             int32_t* c_row, int32_t* c_count, void* stream) {
    OSR_REQUIRE(logits && deltas && boxes && batch_idx && image_hw && reg_weights && c_boxes && c_scores && c_cls && c_row && c_count,
                OSR_ERR_INVALID_ARG, "osr_cascade_candidates: null pointer");
    OSR_REQUIRE(num_stages >= 1 && num_stages <= OSR_CASCADE_MAX_STAGES, OSR_ERR_INVALID_ARG, "osr_cascade_candidates: 1..%d stages", OSR_CASCADE_MAX_STAGES);
    OSR_REQUIRE(n >= 1 && seg_rows >= 1 && num_classes >= 1 && num_classes <= CAND_MAX_CLASSES && (int64_t)n * seg_rows * num_classes < (1ll << 31),
                OSR_ERR_INVALID_ARG, "osr_cascade_candidates: bad sizes (1..%d classes)", CAND_MAX_CLASSES);
    OSR_REQUIRE(reg_weights[0] > 0.f && reg_weights[1] > 0.f && reg_weights[2] > 0.f && reg_weights[3] > 0.f, OSR_ERR_INVALID_ARG,
                "osr_cascade_candidates: regression weights must be positive");
    OSR_REQUIRE((((uintptr_t)boxes | (uintptr_t)deltas | (uintptr_t)c_boxes) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_cascade_candidates: box arrays must be 16-byte aligned");
    CandLogits lg;
    for (int s = 0; s < OSR_CASCADE_MAX_STAGES; ++s) {
        lg.p[s] = s < num_stages ? logits[s] : logits[0];
        OSR_REQUIRE(lg.p[s], OSR_ERR_INVALID_ARG, "osr_cascade_candidates: null logits of stage %d", s);
    }
#define CAND_LAUNCH(S_) \
    cand_launch<S_>(lg, deltas, num_classes, 1, boxes, nullptr, batch_idx, n, seg_rows, image_hw, reg_weights, score_thresh, c_boxes, c_scores, c_cls, c_row, c_count, stream)
    switch (num_stages) {
        case 1: CAND_LAUNCH(1); break;
        case 2: CAND_LAUNCH(2); break;
        case 3: CAND_LAUNCH(3); break;
        default: CAND_LAUNCH(4); break;
    }
#undef CAND_LAUNCH
    OSR_CHECK_LAUNCH("osr_cascade_candidates");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// final assembly: [unknown..., known...]
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ k_boxes, const float* __restrict__ k_scores,
                                                       const int* __restrict__ k_cls, const int* __restrict__ k_keep,
                                                       const int* __restrict__ k_keep_count, long long k_stride, int k_topk,
                                                       const float* __restrict__ u_boxes, const float* __restrict__ u_scores,
                                                       const int* __restrict__ u_keep, const int* __restrict__ u_keep_count,
                                                       long long u_stride, int u_topk, long long unknown_id,
                                                       const long long* __restrict__ class_map, float* __restrict__ out_boxes,
                                                       float* __restrict__ out_scores, long long* __restrict__ out_classes,
                                                       int* __restrict__ out_count) {
    const int img = blockIdx.x, cap = u_topk + k_topk;
    int nu = u_keep_count[img], nk = k_keep_count[img];
    nu = nu < u_topk ? nu : u_topk;
    nk = nk < k_topk ? nk : k_topk;
    for (int i = threadIdx.x; i < cap; i += blockDim.x) {
        const long long o = (long long)img * cap + i;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float s = 0.f;
        long long c = -1;
        if (i < nu) {
            const long long q = img * u_stride + u_keep[(long long)img * u_topk + i];
            b = *reinterpret_cast<const float4*>(u_boxes + q * 4);
            s = u_scores[q];
            c = unknown_id;
        } else if (i < nu + nk) {
            const long long q = img * k_stride + k_keep[(long long)img * k_topk + (i - nu)];
            b = *reinterpret_cast<const float4*>(k_boxes + q * 4);
            s = k_scores[q];
            c = class_map ? class_map[k_cls[q]] : (long long)k_cls[q];
        }
        *reinterpret_cast<float4*>(out_boxes + o * 4) = b;
        out_scores[o] = s;
        out_classes[o] = c;
    }
    if (threadIdx.x == 0) out_count[img] = nu + nk;
}

extern "C" osr_status osr_assemble_detections(const float* k_boxes, const float* k_scores, const int32_t* k_cls, const int32_t* k_keep,
                                              const int32_t* k_keep_count, int64_t k_stride, int32_t k_topk, const float* u_boxes,
                                              const float* u_scores, const int32_t* u_keep, const int32_t* u_keep_count, int64_t u_stride,
                                              int32_t u_topk, int32_t n, int64_t unknown_id, const int64_t* class_map, float* out_boxes,
                                              float* out_scores, int64_t* out_classes, int32_t* out_count, void* stream) {
    OSR_REQUIRE(k_boxes && k_scores && k_cls && k_keep && k_keep_count && u_boxes && u_scores && u_keep && u_keep_count && out_boxes &&
                    out_scores && out_classes && out_count, OSR_ERR_INVALID_ARG, "osr_assemble_detections: null pointer");
    OSR_REQUIRE(n >= 1 && k_topk >= 1 && u_topk >= 1 && k_stride >= 1 && u_stride >= 1, OSR_ERR_INVALID_ARG, "osr_assemble_detections: bad sizes");
    hipLaunchKernelGGL(assemble_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, k_boxes, k_scores, k_cls, k_keep, k_keep_count,
                       (long long)k_stride, k_topk, u_boxes, u_scores, u_keep, u_keep_count, (long long)u_stride, u_topk, (long long)unknown_id,
                       (const long long*)class_map, out_boxes, out_scores, (long long*)out_classes, out_count);
    OSR_CHECK_LAUNCH("osr_assemble_detections");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// [d2] detector_postprocess: rescale to the requested output resolution, clip, drop empty boxes (order kept)
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                          const long long* __restrict__ classes, const int* __restrict__ count, int cap,
                                                          const float* __restrict__ scale_xy, const int* __restrict__ out_hw, float* __restrict__ o_boxes,
                                                          float* __restrict__ o_scores, long long* __restrict__ o_classes, int* __restrict__ o_count) {
    __shared__ int s_scan[32];
    const int img = blockIdx.x;
    const int n = min(count[img], cap);
    const float sx = scale_xy[img * 2], sy = scale_xy[img * 2 + 1];
    const float W = (float)out_hw[img * 2 + 1], H = (float)out_hw[img * 2];
    int base = 0;
    for (int i0 = 0; i0 < cap; i0 += blockDim.x) {
        const int i = i0 + threadIdx.x;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        bool keep = false;
        if (i < n) {
            b = *reinterpret_cast<const float4*>(boxes + ((long long)img * cap + i) * 4);
            // Boxes.scale then Boxes.clip: x in [0, W], y in [0, H]; nonempty: w > 0 and h > 0
            b.x = fminf(fmaxf(b.x * sx, 0.f), W); b.z = fminf(fmaxf(b.z * sx, 0.f), W);
            b.y = fminf(fmaxf(b.y * sy, 0.f), H); b.w = fminf(fmaxf(b.w * sy, 0.f), H);
            keep = (b.z - b.x) > 0.f && (b.w - b.y) > 0.f;
        }
        int tot;
        const int pos = base + osr_block_excl_scan(keep ? 1 : 0, s_scan, &tot);
        if (keep) {
            const long long o = (long long)img * cap + pos, q = (long long)img * cap + i;
            *reinterpret_cast<float4*>(o_boxes + o * 4) = b;
            o_scores[o] = scores[q];
            o_classes[o] = classes[q];
        }
        base += tot;
        __syncthreads();
    }
    for (int i = base + threadIdx.x; i < cap; i += blockDim.x) {
        const long long o = (long long)img * cap + i;
        *reinterpret_cast<float4*>(o_boxes + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        o_scores[o] = 0.f;
        o_classes[o] = -1;
    }
    if (threadIdx.x == 0) o_count[img] = base;
}

extern "C" osr_status osr_detector_postprocess(const float* boxes, const float* scores, const int64_t* classes, const int32_t* count, int32_t n,
                                               int32_t cap, const float* scale_xy, const int32_t* out_hw, float* out_boxes, float* out_scores,
                                               int64_t* out_classes, int32_t* out_count, void* stream) {
    OSR_REQUIRE(boxes && scores && classes && count && scale_xy && out_hw && out_boxes && out_scores && out_classes && out_count, OSR_ERR_INVALID_ARG,
                "osr_detector_postprocess: null pointer");
    OSR_REQUIRE(n >= 1 && cap >= 1, OSR_ERR_INVALID_ARG, "osr_detector_postprocess: bad n / cap");
    OSR_REQUIRE(boxes != out_boxes, OSR_ERR_INVALID_ARG, "osr_detector_postprocess: in-place operation is not supported");
    hipLaunchKernelGGL(postprocess_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, boxes, scores, (const long long*)classes, count, cap, scale_xy, out_hw,
                       out_boxes, out_scores, (long long*)out_classes, out_count);
    OSR_CHECK_LAUNCH("osr_detector_postprocess");
    return OSR_OK;
}
