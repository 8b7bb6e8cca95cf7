// CF-RPN head tail + proposal selection for gfx950 (include/osr.h: osr_cfrpn_head_tail, osr_rpn_select).
//
// Replaces, for all images and pyramid levels at once,
//   ClsFreeRPNHead.forward after the 3x3 conv     classification_free_rpn.py:159-161
//   ClsFreeRPN._decode_proposals                   classification_free_rpn.py:591-610
//   find_top_rpn_proposals                         find_top_proposals.py:60-127
// Compile with -ffp-contract=off: the decode/clip arithmetic must round exactly like the oracle's.
#include "osr_common.h"
#include "osr_boxes.h"
#include "osr_select.h"

// ------------------------------------------------------------------------------------------------------
// head tail: one wave per pixel row of t (c channels, channels-last). 5 dot products + sum of squares.
// ------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void cfrpn_tail_kernel(const T* __restrict__ t, long long rows, int c,
                                                         const float* __restrict__ w_delta, const float* __restrict__ b_delta,
                                                         const float* __restrict__ w_ctr, const float* __restrict__ b_ctr,
                                                         float* __restrict__ deltas, float* __restrict__ ctr) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];  // [5][c]
    for (int i = threadIdx.x; i < 5 * c; i += blockDim.x) s_w[i] = i < 4 * c ? w_delta[i] : w_ctr[i - 4 * c];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long r = (long long)blockIdx.x * nw + wid; r < rows; r += (long long)gridDim.x * nw) {
        float ss = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, d4 = 0.f;
        const T* row = t + r * c;
        for (int k = lane * 4; k < c; k += 256) {
            float v[4];
            if constexpr (sizeof(T) == 4) {
                float4 q = *reinterpret_cast<const float4*>(row + k);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                typedef T t4 __attribute__((ext_vector_type(4)));
                t4 q = *reinterpret_cast<const t4*>(row + k);
                v[0] = (float)q[0]; v[1] = (float)q[1]; v[2] = (float)q[2]; v[3] = (float)q[3];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ss += v[j] * v[j];
                d0 += v[j] * s_w[k + j];
                d1 += v[j] * s_w[c + k + j];
                d2 += v[j] * s_w[2 * c + k + j];
                d3 += v[j] * s_w[3 * c + k + j];
                d4 += v[j] * s_w[4 * c + k + j];
            }
        }
        ss = osr_wave_sum(ss); d0 = osr_wave_sum(d0); d1 = osr_wave_sum(d1);
        d2 = osr_wave_sum(d2); d3 = osr_wave_sum(d3); d4 = osr_wave_sum(d4);
        if (lane == 0) {
            // F.normalize: t / max(||t||_2, 1e-12); the 1x1 convs are linear, so scale the dot products
            const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
            float4 o = make_float4(d0 * inv + b_delta[0], d1 * inv + b_delta[1], d2 * inv + b_delta[2], d3 * inv + b_delta[3]);
            *reinterpret_cast<float4*>(deltas + r * 4) = o;
            const float z = d4 * inv + b_ctr[0];
            ctr[r] = 1.0f / (1.0f + expf(-z));
        }
    }
}

extern "C" osr_status osr_cfrpn_head_tail(const void* t, int32_t t_dtype, int64_t rows, int32_t c, const float* w_delta,
                                          const float* b_delta, const float* w_ctr, const float* b_ctr, float* deltas,
                                          float* ctr, void* stream) {
    OSR_REQUIRE(t && w_delta && b_delta && w_ctr && b_ctr && deltas && ctr, OSR_ERR_INVALID_ARG, "osr_cfrpn_head_tail: null pointer");
    OSR_REQUIRE(osr_dtype_ok(t_dtype), OSR_ERR_INVALID_ARG, "osr_cfrpn_head_tail: bad dtype %d", t_dtype);
    OSR_REQUIRE(c > 0 && c % 4 == 0 && c <= 2048, OSR_ERR_UNSUPPORTED, "osr_cfrpn_head_tail: c must be a multiple of 4 and <= 2048, got %d", c);
    OSR_REQUIRE(rows >= 0, OSR_ERR_INVALID_ARG, "osr_cfrpn_head_tail: rows < 0");
    if (rows == 0) return OSR_OK;
    long long blocks = (rows + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    size_t smem = (size_t)5 * c * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (t_dtype == OSR_F32)
        hipLaunchKernelGGL(cfrpn_tail_kernel<float>, dim3((unsigned)blocks), dim3(256), smem, st, (const float*)t, rows, c, w_delta, b_delta, w_ctr, b_ctr, deltas, ctr);
    else if (t_dtype == OSR_F16)
        hipLaunchKernelGGL(cfrpn_tail_kernel<f16_t>, dim3((unsigned)blocks), dim3(256), smem, st, (const f16_t*)t, rows, c, w_delta, b_delta, w_ctr, b_ctr, deltas, ctr);
    else
        hipLaunchKernelGGL(cfrpn_tail_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), smem, st, (const bf16_t*)t, rows, c, w_delta, b_delta, w_ctr, b_ctr, deltas, ctr);
    OSR_CHECK_LAUNCH("osr_cfrpn_head_tail");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// proposal selection
// ------------------------------------------------------------------------------------------------------

struct SelLevels {
    int num_levels, num_anchors;
    int h[OSR_MAX_LEVELS], w[OSR_MAX_LEVELS], stride[OSR_MAX_LEVELS];
    long long offset[OSR_MAX_LEVELS];
    int klevel[OSR_MAX_LEVELS];  // min(h*w*a, topk)
    int koff[OSR_MAX_LEVELS];    // prefix of klevel
    int aoff[OSR_MAX_LEVELS];    // prefix of h*w*a (index into the image's concatenated anchor list)
    int cap;
};

// Stage A: grid (level, image). Stable top-k by radix select + bitonic sort, ltrb decode, filters.
// Writes staging arrays st_box/st_score/st_src/st_flag at [img][koff[l] + rank].
// MAXK is the length of the pair list in LDS: SEL_MAXK for osr_rpn_select(_ex), SEL_WIDE_MAXK for osr_rpn_select_wide. Nothing else
// differs between the two instantiations, so for a k both serve they select, sort and decode alike, bit for bit.
#define SEL_WIDE_MAXK OSR_RPN_SELECT_WIDE_MAXK  // 8192 pairs = 64 KiB beside the 8 KiB histogram: 72 KiB of the 160 KiB a workgroup may hold
template <int MAXK>
__global__ __launch_bounds__(SEL_THREADS) void rpn_select_kernel(SelLevels lv, const float* __restrict__ cell_anchors,
                                                                 const float* __restrict__ ctr, const float* __restrict__ deltas,
                                                                 int n_img, const int* __restrict__ image_hw, float min_box_size,
                                                                 int decode_mode, float4 rw, float* __restrict__ st_box,
                                                                 float* __restrict__ st_score, int* __restrict__ st_src, int* __restrict__ st_flag,
                                                                 int* __restrict__ status_flags) {
    const int l = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const int A = lv.num_anchors, W = lv.w[l];
    const int cnt = lv.h[l] * W * A;
    const int k = lv.klevel[l];
    const float* sc = ctr + lv.offset[l] + (long long)img * cnt;
    const float* dl = deltas + (lv.offset[l] + (long long)img * cnt) * 4;

    __shared__ unsigned long long s_sel[MAXK];
    __shared__ __attribute__((aligned(16))) int s_hist[SEL_BINS];
    __shared__ int s_scan[32];
    __shared__ SelBcast<unsigned int> s_bc;

    // Four scores per thread and load (16 bytes per lane) where the segment allows it: the level's score run must be 16-byte
    // aligned and a multiple of 4 long (true for p2..p4 of every image; the small levels take the scalar form).
    const bool vec4 = (cnt & 3) == 0 && (((uintptr_t)sc) & 15) == 0;
    const int per = vec4 ? 4 : 1;
    const int nit = (cnt + SEL_THREADS * per - 1) / (SEL_THREADS * per);  // uniform trip count of the strided loops below

    // ---- 1. radix select: key T of the k-th largest element (3 passes: 11 + 11 + 10 key bits, MSB first). The scores of a level are sigmoid
    //      outputs: their leading key byte is the same for almost every anchor, so one LDS atomic per element would put all 67 200
    //      adds of a p2 pass on one histogram bin, one behind the other. sel_hist_add adds a wave's most common digits once per wave. ----
    SelRank<unsigned int> rank{0u, 0u, k};
    if (cnt > k) {  // (so the first histogram holds cnt > k = remaining elements, and every later one its prefix's bucket, which holds the rank)
        // three passes over the scores: 11 + 11 + 10 key bits, MSB first (four 8-bit passes read the 269 KB of a p2 level once more)
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            sel_radix_pass<SEL_BINS, 2>(rank, pass == 0 ? 21 : pass == 1 ? 10 : 0, pass == 2 ? 10 : 11, s_hist, &s_bc, [&](auto add) {
                for (int it = 0; it < nit; ++it) {
                    const int i = (it * SEL_THREADS + tid) * per;
                    unsigned int key[4] = {0u, 0u, 0u, 0u};
                    if (i < cnt) {
                        if (vec4) {
                            const float4 v = *reinterpret_cast<const float4*>(sc + i);
                            key[0] = sel_key(v.x); key[1] = sel_key(v.y); key[2] = sel_key(v.z); key[3] = sel_key(v.w);
                        } else key[0] = sel_key(sc[i]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < per) add(key[e], i < cnt);
                }
            });
        }
    }
    // Now: elements with key > prefix are all selected; of those with key == prefix the first `remaining`
    // in index order are selected (stable tie rule). If cnt <= k everything is selected.
    const unsigned int T = rank.prefix;
    const int remaining = rank.remaining;
    const bool all = cnt <= k;

    // ---- 2. ordered compaction into s_sel as (key << 32) | ~index: strictly greater keys to [0, ngt), ties to [ngt, k). The k-th
    //      largest key is T and `remaining` of its ties are needed, so exactly k - remaining keys are greater: no counting pass ----
    int base_gt = 0, base_eq = 0;  // running counts (uniform across the block)
    const int ngt_total = all ? 0 : k - remaining;
    for (int it = 0; it < nit; ++it) {
        const int i = (it * SEL_THREADS + tid) * per;
        unsigned int key[4] = {0u, 0u, 0u, 0u};
        int gt = 0, eq = 0;  // how many of this thread's (up to four, consecutive) elements are greater / tie
        if (i < cnt) {
            if (vec4) {
                const float4 v = *reinterpret_cast<const float4*>(sc + i);
                key[0] = sel_key(v.x); key[1] = sel_key(v.y); key[2] = sel_key(v.z); key[3] = sel_key(v.w);
            } else key[0] = sel_key(sc[i]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < per) { if (all) gt += 1; else { gt += key[e] > T; eq += key[e] == T; } }
        }
        int tot;
        const int packed = osr_block_excl_scan(gt | (eq << 16), s_scan, &tot);
        int pg = base_gt + (packed & 0xffff), pe = base_eq + (packed >> 16);
        if (i < cnt) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < per) {
                    const unsigned long long comp = sel_pair(key[e], (unsigned int)(i + e));
                    const bool g = all || key[e] > T, q = !all && key[e] == T;
                    if (g) { if (pg < MAXK) s_sel[pg] = comp; ++pg; }
                    if (q) { if (pe < remaining && ngt_total + pe < MAXK) s_sel[ngt_total + pe] = comp; ++pe; }
                }
        }
        base_gt += tot & 0xffff;
        base_eq += tot >> 16;
        if (!all && base_eq >= remaining && base_gt >= ngt_total) break;  // uniform
    }

    // ---- 3. sort the survivors: score descending, index ascending ----
    sel_pad_and_sort(s_sel, k);

    // ---- 4. decode + filters ----
    const float ih = (float)image_hw[img * 2 + 0], iw = (float)image_hw[img * 2 + 1];
    const float fstride = (float)lv.stride[l];
    bool bad = false;
    for (int j = tid; j < k; j += blockDim.x) {
        const int idx = sel_pair_index(s_sel[j]);
        const float s = sc[idx];
        const float4 d = *reinterpret_cast<const float4*>(dl + (long long)idx * 4);
        const float4 an = osr_cell_anchor(cell_anchors, l, A, idx % A, idx / A, W, fstride);
        float4 b;
        bool valid;
        if (decode_mode == 0) {
            // [d2] Box2BoxTransformLinear(normalize_by_size=True).apply_deltas (the CF-RPN, classification_free_rpn.py:607)
            const float aw = an.z - an.x, ah = an.w - an.y, cx = 0.5f * (an.x + an.z), cy = 0.5f * (an.y + an.w);
            b = make_float4(cx - fmaxf(d.x, 0.f) * aw, cy - fmaxf(d.y, 0.f) * ah, cx + fmaxf(d.z, 0.f) * aw, cy + fmaxf(d.w, 0.f) * ah);
            // relu(NaN) must stay NaN like torch's: fmaxf drops a NaN, so test the raw deltas too
            valid = osr_box_finite(b) && !((d.x != d.x) || (d.y != d.y) || (d.z != d.z) || (d.w != d.w));
        } else {
            // [d2] Box2BoxTransform(weights).apply_deltas (the stock RPN of Base-RCNN-FPN.yaml: weights 1,1,1,1)
            b = osr_b2b_decode(an, d, rw, &valid);
        }
        valid = valid && osr_finite(s);
        bad |= !valid;
        b = osr_box_clip(b, iw, ih);
        const bool keep = valid && (b.z - b.x > min_box_size) && (b.w - b.y > min_box_size);
        const long long o = (long long)img * lv.cap + lv.koff[l] + j;
        *reinterpret_cast<float4*>(st_box + o * 4) = b;
        st_score[o] = s;
        st_src[o] = lv.aoff[l] + idx;
        st_flag[o] = keep ? 1 : 0;
    }
    if (bad) atomicOr(status_flags, 1);
}

// Stage B: one block per image; order-preserving compaction of the staged slots.
__global__ __launch_bounds__(SEL_THREADS) void rpn_compact_kernel(int cap, const float* __restrict__ st_box,
                                                                  const float* __restrict__ st_score, const int* __restrict__ st_src,
                                                                  const int* __restrict__ st_flag, float* __restrict__ boxes,
                                                                  float* __restrict__ scores, int* __restrict__ src_index,
                                                                  int* __restrict__ batch_idx, int* __restrict__ counts, SelLevels lv,
                                                                  int* __restrict__ level_out) {
    const int img = blockIdx.x, tid = threadIdx.x;
    __shared__ int s_scan[32];
    const long long base = (long long)img * cap;
    int running = 0;
    for (int i0 = 0; i0 < cap; i0 += blockDim.x) {
        const int i = i0 + tid;
        const int f = i < cap ? st_flag[base + i] : 0;
        int tot;
        const int pos = running + osr_block_excl_scan(f, s_scan, &tot);
        if (f) {
            *reinterpret_cast<float4*>(boxes + (base + pos) * 4) = *reinterpret_cast<const float4*>(st_box + (base + i) * 4);
            scores[base + pos] = st_score[base + i];
            src_index[base + pos] = st_src[base + i];
            batch_idx[base + pos] = img;
            if (level_out) {  // slot i of the staging array belongs to the level whose [koff, koff + klevel) holds it
                int l = 0;
                while (l + 1 < lv.num_levels && i >= lv.koff[l + 1]) ++l;
                level_out[base + pos] = l;
            }
        }
        running += tot;
    }
    for (int i = running + tid; i < cap; i += blockDim.x) {
        *reinterpret_cast<float4*>(boxes + (base + i) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        scores[base + i] = 0.f;
        src_index[base + i] = -1;
        batch_idx[base + i] = -1;
        if (level_out) level_out[base + i] = -1;
    }
    if (tid == 0) counts[img] = running;
}

static bool fill_levels(const osr_rpn_levels* in, int topk, SelLevels* o, int maxk = SEL_MAXK) {
    if (!in || in->num_levels < 1 || in->num_levels > OSR_MAX_LEVELS || in->num_anchors < 1 || topk < 1 || topk > maxk) return false;
    o->num_levels = in->num_levels;
    o->num_anchors = in->num_anchors;
    int ko = 0;
    long long ao = 0;
    for (int l = 0; l < in->num_levels; ++l) {
        if (in->h[l] < 1 || in->w[l] < 1 || in->stride[l] < 1 || in->offset[l] < 0) return false;
        long long cnt = (long long)in->h[l] * in->w[l] * in->num_anchors;
        if (cnt > (1ll << 30) || ao + cnt > (1ll << 30)) return false;
        o->h[l] = in->h[l]; o->w[l] = in->w[l]; o->stride[l] = in->stride[l]; o->offset[l] = in->offset[l];
        o->klevel[l] = (int)(cnt < topk ? cnt : topk);
        o->koff[l] = ko;
        o->aoff[l] = (int)ao;
        ko += o->klevel[l];
        ao += cnt;
    }
    o->cap = ko;
    return true;
}

extern "C" int32_t osr_rpn_select_capacity(const osr_rpn_levels* lv, int32_t pre_nms_topk) {
    SelLevels s;
    if (!fill_levels(lv, pre_nms_topk, &s)) { osr_set_error("osr_rpn_select_capacity: bad level table / topk (1..%d)", SEL_MAXK); return OSR_ERR_INVALID_ARG; }
    return s.cap;
}

extern "C" int64_t osr_rpn_select_workspace_bytes(const osr_rpn_levels* lv, int32_t n, int32_t pre_nms_topk) {
    SelLevels s;
    if (!fill_levels(lv, pre_nms_topk, &s) || n < 1) { osr_set_error("osr_rpn_select_workspace_bytes: bad arguments"); return OSR_ERR_INVALID_ARG; }
    return (int64_t)n * s.cap * (4 * 4 + 4 + 4 + 4);
}

// The two launches behind osr_rpn_select_ex (MAXK = SEL_MAXK) and osr_rpn_select_wide (MAXK = SEL_WIDE_MAXK).
template <int MAXK>
static osr_status rpn_select_impl(const osr_rpn_levels* lv, const float* cell_anchors, const float* ctr, const float* deltas,
                                  int32_t n, const int32_t* image_hw, int32_t pre_nms_topk, float min_box_size, int32_t decode_mode,
                                  const float reg_weights[4], float* boxes, float* scores, int32_t* src_index, int32_t* batch_idx,
                                  int32_t* level_out, int32_t* counts, int32_t* status_flags, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    SelLevels s;
    OSR_REQUIRE(fill_levels(lv, pre_nms_topk, &s, MAXK), OSR_ERR_INVALID_ARG, "osr_rpn_select: bad level table / topk (1..%d)", MAXK);
    OSR_REQUIRE(cell_anchors && ctr && deltas && image_hw && boxes && scores && src_index && batch_idx && counts && status_flags && workspace,
                OSR_ERR_INVALID_ARG, "osr_rpn_select: null pointer");
    OSR_REQUIRE(n >= 1 && n <= 65535, OSR_ERR_INVALID_ARG, "osr_rpn_select: n out of range");
    OSR_REQUIRE(decode_mode == 0 || (decode_mode == 1 && reg_weights && reg_weights[0] > 0.f && reg_weights[1] > 0.f && reg_weights[2] > 0.f && reg_weights[3] > 0.f),
                OSR_ERR_INVALID_ARG, "osr_rpn_select: decode_mode 0 (ltrb) or 1 (Box2BoxTransform with positive weights)");
    const int64_t need = (int64_t)n * s.cap * 28;
    OSR_REQUIRE(workspace_bytes >= need, OSR_ERR_WORKSPACE, "osr_rpn_select: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    OSR_REQUIRE(((uintptr_t)workspace & 15) == 0, OSR_ERR_INVALID_ARG, "osr_rpn_select: workspace must be 16-byte aligned");
    char* ws = (char*)workspace;
    float* st_box = (float*)ws;
    float* st_score = (float*)(ws + (int64_t)n * s.cap * 16);
    int* st_src = (int*)(ws + (int64_t)n * s.cap * 20);
    int* st_flag = (int*)(ws + (int64_t)n * s.cap * 24);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status_flags, 0, sizeof(int32_t), st) != hipSuccess) { osr_set_error("osr_rpn_select: memset failed"); return OSR_ERR_LAUNCH; }
    const float4 rw = decode_mode == 1 ? make_float4(reg_weights[0], reg_weights[1], reg_weights[2], reg_weights[3]) : make_float4(1.f, 1.f, 1.f, 1.f);
    hipLaunchKernelGGL(rpn_select_kernel<MAXK>, dim3(s.num_levels, n), dim3(SEL_THREADS), 0, st, s, cell_anchors, ctr, deltas, n, image_hw,
                       min_box_size, decode_mode, rw, st_box, st_score, st_src, st_flag, status_flags);
    OSR_CHECK_LAUNCH("osr_rpn_select(select)");
    hipLaunchKernelGGL(rpn_compact_kernel, dim3(n), dim3(SEL_THREADS), 0, st, s.cap, st_box, st_score, st_src, st_flag, boxes, scores,
                       src_index, batch_idx, counts, s, level_out);
    OSR_CHECK_LAUNCH("osr_rpn_select(compact)");
    return OSR_OK;
}

extern "C" osr_status osr_rpn_select_ex(const osr_rpn_levels* lv, const float* cell_anchors, const float* ctr, const float* deltas,
                                        int32_t n, const int32_t* image_hw, int32_t pre_nms_topk, float min_box_size, int32_t decode_mode,
                                        const float reg_weights[4], float* boxes, float* scores, int32_t* src_index, int32_t* batch_idx,
                                        int32_t* level_out, int32_t* counts, int32_t* status_flags, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
    return rpn_select_impl<SEL_MAXK>(lv, cell_anchors, ctr, deltas, n, image_hw, pre_nms_topk, min_box_size, decode_mode, reg_weights, boxes,
                                     scores, src_index, batch_idx, level_out, counts, status_flags, workspace, workspace_bytes, stream);
}

// ---- osr_rpn_select_wide: the same selection with up to OSR_RPN_SELECT_WIDE_MAXK proposals per level (the single-level C4 RPN's
// PRE_NMS_TOPK_TEST 6000). One workgroup per (level, image) as above; its pair list takes 64 KiB of LDS, so one workgroup per CU. ----
extern "C" int32_t osr_rpn_select_wide_capacity(const osr_rpn_levels* lv, int32_t pre_nms_topk) {
    SelLevels s;
    if (pre_nms_topk > SEL_WIDE_MAXK) { osr_set_error("osr_rpn_select_wide_capacity: pre_nms_topk %d > %d", pre_nms_topk, SEL_WIDE_MAXK); return OSR_ERR_UNSUPPORTED; }
    if (!fill_levels(lv, pre_nms_topk, &s, SEL_WIDE_MAXK)) { osr_set_error("osr_rpn_select_wide_capacity: bad level table / topk (1..%d)", SEL_WIDE_MAXK); return OSR_ERR_INVALID_ARG; }
    return s.cap;
}

extern "C" int64_t osr_rpn_select_wide_workspace_bytes(const osr_rpn_levels* lv, int32_t n, int32_t pre_nms_topk) {
    SelLevels s;
    if (pre_nms_topk > SEL_WIDE_MAXK) { osr_set_error("osr_rpn_select_wide_workspace_bytes: pre_nms_topk %d > %d", pre_nms_topk, SEL_WIDE_MAXK); return OSR_ERR_UNSUPPORTED; }
    if (!fill_levels(lv, pre_nms_topk, &s, SEL_WIDE_MAXK) || n < 1) { osr_set_error("osr_rpn_select_wide_workspace_bytes: bad arguments"); return OSR_ERR_INVALID_ARG; }
    return (int64_t)n * s.cap * (4 * 4 + 4 + 4 + 4);
}

extern "C" osr_status osr_rpn_select_wide(const osr_rpn_levels* lv, const float* cell_anchors, const float* ctr, const float* deltas,
                                          int32_t n, const int32_t* image_hw, int32_t pre_nms_topk, float min_box_size, int32_t decode_mode,
                                          const float reg_weights[4], float* boxes, float* scores, int32_t* src_index, int32_t* batch_idx,
                                          int32_t* level_out, int32_t* counts, int32_t* status_flags, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
    OSR_REQUIRE(pre_nms_topk <= SEL_WIDE_MAXK, OSR_ERR_UNSUPPORTED, "osr_rpn_select_wide: pre_nms_topk %d > %d", pre_nms_topk, SEL_WIDE_MAXK);
    return rpn_select_impl<SEL_WIDE_MAXK>(lv, cell_anchors, ctr, deltas, n, image_hw, pre_nms_topk, min_box_size, decode_mode, reg_weights, boxes,
                                          scores, src_index, batch_idx, level_out, counts, status_flags, workspace, workspace_bytes, stream);
}

extern "C" osr_status osr_rpn_select(const osr_rpn_levels* lv, const float* cell_anchors, const float* ctr, const float* deltas,
                                     int32_t n, const int32_t* image_hw, int32_t pre_nms_topk, float min_box_size, float* boxes,
                                     float* scores, int32_t* src_index, int32_t* batch_idx, int32_t* counts, int32_t* status_flags,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    return osr_rpn_select_ex(lv, cell_anchors, ctr, deltas, n, image_hw, pre_nms_topk, min_box_size, 0, nullptr, boxes, scores, src_index, batch_idx,
                             nullptr, counts, status_flags, workspace, workspace_bytes, stream);
}
