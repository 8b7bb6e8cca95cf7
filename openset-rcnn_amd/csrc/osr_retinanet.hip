// RetinaNet inference tail for gfx950 (include/osr.h: osr_retinanet_select): per (image, level) the candidates `logit > thresh` of up
// to h*w*A*K class logits, the topk largest of them, their sigmoid scores and decoded boxes -- [d2] RetinaNet.inference_single_image
// before its batched NMS (osr_nms_topk follows).
//
// Two launches:
//   rn_filter_kernel   the whole grid streams the logits ONCE in 16-byte vectors; every element above the threshold is appended as
//                      (key << 32 | ~index) to its segment's survivor list. A workgroup counts the survivors of its 32 KB chunk,
//                      takes its slots with ONE integer atomic on the segment's counter and writes them; the order inside the list
//                      is free, the (key, ~index) pairs are unique and pass 2 orders them.
//   rn_select_kernel   one workgroup per segment: radix select of the topk-th largest pair over the survivor list (the 32 key bits
//                      first, the 32 index bits only while ties straddle the k-th place), bitonic sort, decode.
// When a segment's counter says its list overflowed (more survivors than its fixed capacity: untrained or hostile weights), three
// launches between the two -- whose workgroups return at once for every other segment -- raise that segment's threshold, all on the
// device: the grid histograms the candidates' leading 11 key bits (rn_filter_kernel, mode 1), one wave per segment finds the digit
// that holds the topk-th largest (rn_refine_kernel), and the grid filters the segment again at that digit (mode 2) into the same
// list. If even that overflows (more ties inside one digit than the list holds), rn_select_kernel reads the segment's logits
// themselves instead of the list: one workgroup, exact, slow.
// Compile with -ffp-contract=off: the decode rounds like rpn_select_kernel's decode_mode 1.
#include "osr_common.h"
#include "osr_boxes.h"
#include "osr_select.h"

#define RN_FILTER_THREADS 256
#define RN_FILTER_ITEMS 8  // 16-byte vectors per thread: a workgroup's chunk is 256 * 8 * 16 bytes = 32 KB of logits
#define RN_CHUNK_VECS (RN_FILTER_THREADS * RN_FILTER_ITEMS)
#define RN_MIN_SURVIVORS 4096  // a segment's survivor list holds max(this, 1/32 of the segment) pairs, never more than the segment
#define RN_DIGITS 2048         // bins of an overflowed segment's histogram: the leading 11 key bits
#define RN_DIGIT_SHIFT 21

struct RnLevels {
    int num_levels, A, K, AK;
    int pitch_cls, pitch_box, topk, n;
    int h[OSR_MAX_LEVELS], w[OSR_MAX_LEVELS], stride[OSR_MAX_LEVELS];
    int cnt[OSR_MAX_LEVELS];              // h * w * A * K: candidates' index range
    int span[OSR_MAX_LEVELS];             // h * w * pitch_cls: the segment's extent in the logits buffer
    long long cell_off[OSR_MAX_LEVELS];   // cells before level l (offset / A): x pitch_cls in logits, x pitch_box in deltas
    int caps[OSR_MAX_LEVELS];             // survivor list capacity of one segment
    long long surv_off[OSR_MAX_LEVELS];   // first pair of level l's lists (image img at + img * caps)
    int chunks[OSR_MAX_LEVELS];           // filter workgroups per segment
    int block_off[OSR_MAX_LEVELS + 1];    // prefix of n * chunks
};

template <class T> struct rn_vec;
template <> struct rn_vec<float> { static constexpr int N = 4; };
template <> struct rn_vec<f16_t> { static constexpr int N = 8; };
template <> struct rn_vec<bf16_t> { static constexpr int N = 8; };

template <class T>
__device__ __forceinline__ void rn_unpack(const uint4& q, float* v) {
    if constexpr (sizeof(T) == 4) {
        v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
    } else {
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (__is_same(T, bf16_t)) {
                v[2 * j] = __uint_as_float(u[j] << 16);
                v[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
            } else {
                union { uint32_t w; f16_t h[2]; } c;
                c.w = u[j];
                v[2 * j] = (float)c.h[0];
                v[2 * j + 1] = (float)c.h[1];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// pass 1: threshold filter over the whole grid
// ------------------------------------------------------------------------------------------------------
// MODE 0: every candidate into the segment's list (slots from surv_cnt). MODE 1 / 2 work on overflowed segments only (surv_cnt > caps):
// 1 adds the candidates' leading key digit to the segment's histogram, 2 writes the candidates with key >= thr2[segment] (slots from cnt2).
template <class T, int MODE>
__global__ __launch_bounds__(RN_FILTER_THREADS) void rn_filter_kernel(RnLevels lv, const T* __restrict__ logits, float thresh,
                                                                      unsigned long long* __restrict__ surv, int* __restrict__ surv_cnt,
                                                                      int* __restrict__ cnt2, const unsigned int* __restrict__ thr2,
                                                                      int* __restrict__ hist) {
    constexpr int VEC = rn_vec<T>::N;
    const int tid = threadIdx.x;
    int l = 0;
    while (l + 1 < lv.num_levels && (int)blockIdx.x >= lv.block_off[l + 1]) ++l;
    const int rem = (int)blockIdx.x - lv.block_off[l];
    const int img = rem / lv.chunks[l], chunk = rem - img * lv.chunks[l];
    const int segid = img * lv.num_levels + l;
    unsigned int key_min = 0u;
    if constexpr (MODE != 0) {
        if (surv_cnt[segid] <= lv.caps[l]) return;  // uniform: the segment's list holds all its candidates
        if constexpr (MODE == 2) key_min = thr2[segid];
    }
    const int span = lv.span[l], pitch = lv.pitch_cls, AK = lv.AK;
    // the segment is elements [seg0, seg0 + span) of the buffer; vectors are aligned to the BUFFER, so the first and the last vector
    // of a segment may hang over its ends (their outside elements belong to the neighbours and are masked here)
    const long long seg0 = (lv.cell_off[l] + (long long)img * lv.h[l] * lv.w[l]) * pitch;
    const long long vec0 = seg0 / VEC + (long long)chunk * RN_CHUNK_VECS;

    __shared__ int s_scan[32];
    __shared__ int s_base;
    __shared__ int s_dig[MODE == 1 ? RN_DIGITS : 1];
    if constexpr (MODE == 1) {
        for (int i = tid; i < RN_DIGITS; i += RN_FILTER_THREADS) s_dig[i] = 0;
        __syncthreads();
    }

    uint4 q[RN_FILTER_ITEMS];
    int rel[RN_FILTER_ITEMS];  // element of the segment that the vector's lane 0 holds (negative: before the segment)
    unsigned int pass[RN_FILTER_ITEMS];
    int mine = 0;
#pragma unroll
    for (int it = 0; it < RN_FILTER_ITEMS; ++it) {
        const long long e0 = (vec0 + it * RN_FILTER_THREADS + tid) * VEC;
        const long long r = e0 - seg0;  // > -VEC
        rel[it] = r < (long long)span ? (int)r : span;
        q[it] = make_uint4(0u, 0u, 0u, 0u);
        if (rel[it] >= 0 && rel[it] + VEC <= span) {
            q[it] = *reinterpret_cast<const uint4*>(logits + e0);
        } else if (rel[it] < span) {  // a vector over an end of the segment: element by element, inside the segment only
            T tmp[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int re = rel[it] + e;
                tmp[e] = (re >= 0 && re < span) ? logits[e0 + e] : (T)0.f;
            }
            q[it] = *reinterpret_cast<const uint4*>(tmp);
        }
    }
#pragma unroll
    for (int it = 0; it < RN_FILTER_ITEMS; ++it) {
        float v[VEC];
        rn_unpack<T>(q[it], v);
        unsigned int m = 0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            bool on = v[e] > thresh;  // (NaN never passes)
            if constexpr (MODE == 2) on = on && osr_float_key(v[e]) >= key_min;
            m |= on ? 1u << e : 0u;
        }
        if (m) {
            // drop what lies outside the segment or in the padding channels [AK, pitch) of a cell: one 32-bit division per vector
            const int r0 = rel[it] > 0 ? rel[it] : 0;
            int c = rel[it] - (int)((unsigned)r0 / (unsigned)pitch) * pitch;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                while (c >= pitch) c -= pitch;
                const int re = rel[it] + e;
                if (re < 0 || re >= span || c >= AK) m &= ~(1u << e);
                ++c;
            }
        }
        pass[it] = m;
        mine += __popc(m);
        if constexpr (MODE == 1) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) sel_hist_add<2>(s_dig, (int)(osr_float_key(v[e]) >> RN_DIGIT_SHIFT), (m >> e) & 1u);  // (all lanes call it)
        }
    }
    if constexpr (MODE == 1) {
        __syncthreads();
        for (int i = tid; i < RN_DIGITS; i += RN_FILTER_THREADS)
            if (s_dig[i]) atomicAdd(&hist[(long long)segid * RN_DIGITS + i], s_dig[i]);
        return;
    }
    int total;
    int pos = osr_block_excl_scan(mine, s_scan, &total);
    if (total == 0) return;  // uniform
    if (tid == 0) s_base = atomicAdd(MODE == 2 ? &cnt2[segid] : &surv_cnt[segid], total);
    __syncthreads();
    pos += s_base;
    const int cap = lv.caps[l];
    if (pos >= cap) return;  // (the counter keeps the true number of candidates: pass 2 sees the overflow)
    unsigned long long* out = surv + lv.surv_off[l] + (long long)img * cap;
#pragma unroll
    for (int it = 0; it < RN_FILTER_ITEMS; ++it) {
        if (!pass[it]) continue;
        float v[VEC];
        rn_unpack<T>(q[it], v);
        const int r0 = rel[it] > 0 ? rel[it] : 0;
        int row = (int)((unsigned)r0 / (unsigned)pitch);
        int c = rel[it] - row * pitch;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            while (c >= pitch) { c -= pitch; ++row; }
            if ((pass[it] >> e) & 1u) {
                const unsigned int i = (unsigned)(row * AK + c);
                if (pos < cap) out[pos] = sel_pair(osr_float_key(v[e]), i);
                ++pos;
            }
            ++c;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// an overflowed segment's new threshold: the leading digit d of the topk-th largest candidate key (the largest d with
// sum(hist[d..]) >= topk); the second filter keeps key >= d << 21. One wave per segment.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rn_refine_kernel(RnLevels lv, const int* __restrict__ surv_cnt, const int* __restrict__ hist,
                                                       unsigned int* __restrict__ thr2) {
    const int l = blockIdx.x, img = blockIdx.y;
    const int segid = img * lv.num_levels + l;
    if (surv_cnt[segid] <= lv.caps[l]) return;
    int d, above, bucket;  // (an overflowed segment has more than caps >= RN_MIN_SURVIVORS > topk >= 1 candidates, all in its histogram)
    if (sel_digit_of_rank<RN_DIGITS>(hist + (long long)segid * RN_DIGITS, lv.topk, &d, &above, &bucket)) thr2[segid] = (unsigned int)d << RN_DIGIT_SHIFT;
}

// ------------------------------------------------------------------------------------------------------
// pass 2: one workgroup per segment
// ------------------------------------------------------------------------------------------------------

template <class T>
__global__ __launch_bounds__(SEL_THREADS) void rn_select_kernel(RnLevels lv, const float* __restrict__ cell_anchors, const T* __restrict__ logits,
                                                                const float* __restrict__ deltas, float thresh, float4 rw,
                                                                const unsigned long long* __restrict__ surv, const int* __restrict__ surv_cnt,
                                                                const int* __restrict__ cnt2, float* __restrict__ c_boxes, float* __restrict__ c_scores, int* __restrict__ c_cls,
                                                                int* __restrict__ c_cand, int* __restrict__ c_src, int* __restrict__ counts,
                                                                int* __restrict__ status_flags) {
    const int l = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const int A = lv.A, K = lv.K, AK = lv.AK, W = lv.w[l], topk = lv.topk;
    const long long cell0 = lv.cell_off[l] + (long long)img * lv.h[l] * W;
    const T* seg = logits + cell0 * lv.pitch_cls;
    const int ncand = surv_cnt[img * lv.num_levels + l];  // every element above the threshold, kept or not
    const bool over = ncand > lv.caps[l];                  // the list overflowed: it now holds the candidates of the raised threshold
    const int n2 = over ? cnt2[img * lv.num_levels + l] : 0;
    const bool fallback = over && n2 > lv.caps[l];         // ... unless they overflowed it too: read the logits themselves
    const int m = fallback ? lv.cnt[l] : over ? n2 : ncand;  // elements to look at
    const int nsrc = fallback ? ncand : m;                   // candidates among them (the list holds nothing else)
    const int k = ncand < topk ? ncand : topk;
    const unsigned long long* list = surv + lv.surv_off[l] + (long long)img * lv.caps[l];

    __shared__ unsigned long long s_sel[SEL_MAXK];
    __shared__ __attribute__((aligned(16))) int s_hist[SEL_BINS];
    __shared__ SelBcast<unsigned long long> s_bc;
    __shared__ int s_fill;

    // element j of the segment's source as its (key, ~index) pair; 0 = not a candidate
    auto load = [&](int j) -> unsigned long long {
        if (j >= m) return 0ull;
        if (!fallback) return list[j];
        const int row = (int)((unsigned)j / (unsigned)AK);
        const float v = osr_to_float(seg[(long long)row * lv.pitch_cls + (j - row * AK)]);
        return v > thresh ? sel_pair(osr_float_key(v), (unsigned)j) : 0ull;
    };
    const int nit = (m + SEL_THREADS - 1) / SEL_THREADS;

    // ---- 1. radix select of the k-th largest pair, MSB first: 11 + 11 + 10 key bits, then 11 + 11 + 10 index bits. It stops as soon
    //      as the bucket of the current prefix holds exactly the elements still wanted: with distinct logits after the key bits. ----
    SelRank<unsigned long long> rank{0ull, 0ull, k};
    if (nsrc > k) {  // (nsrc candidates reach the first histogram: more than k = remaining >= 1)
#pragma unroll 1
        for (int pass = 0; pass < 6; ++pass) {
            const int shift = pass == 0 ? 53 : pass == 1 ? 42 : pass == 2 ? 32 : pass == 3 ? 21 : pass == 4 ? 10 : 0;
            const int bucket = sel_radix_pass<SEL_BINS, 2>(rank, shift, (pass == 2 || pass == 5) ? 10 : 11, s_hist, &s_bc, [&](auto add) {
                for (int it = 0; it < nit; ++it) {
                    const unsigned long long c = load(it * SEL_THREADS + tid);
                    add(c, c != 0ull);
                }
            });
            if (bucket == rank.remaining) break;  // uniform: every element of the bucket is selected
        }
    }
    // Now: the selected elements are the candidates with (pair & mask) >= prefix -- exactly k of them (all, when ncand <= k).

    // ---- 2. compaction into LDS [0, k): the order is free (integer atomics), the sort below fixes it ----
    if (tid == 0) s_fill = 0;
    __syncthreads();
    for (int it = 0; it < nit; ++it) {
        const unsigned long long c = load(it * SEL_THREADS + tid);
        if (c != 0ull && (c & rank.mask) >= rank.prefix) {
            const int p = atomicAdd(&s_fill, 1);
            if (p < SEL_MAXK) s_sel[p] = c;
        }
    }

    // ---- 3. logit descending, index ascending ----
    sel_pad_and_sort(s_sel, k);

    // ---- 4. score, class, decode ----
    const float fstride = (float)lv.stride[l];
    const float* dl = deltas + cell0 * lv.pitch_box;
    const long long obase = (long long)img * lv.num_levels * topk + (long long)l * topk;
    bool bad = false;
    for (int j = tid; j < topk; j += blockDim.x) {
        const long long o = obase + j;
        if (j >= k) {
            *reinterpret_cast<float4*>(c_boxes + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            c_scores[o] = 0.f; c_cls[o] = -1; c_cand[o] = 0; c_src[o] = -1;
            continue;
        }
        const unsigned long long comp = s_sel[j];
        const int idx = sel_pair_index(comp);
        const float z = sel_pair_key_float(comp);
        const int t = idx / K, kc = idx - t * K;
        const int cell = t / A, a = t - cell * A;
        const float4 d = *reinterpret_cast<const float4*>(dl + (long long)cell * lv.pitch_box + a * 4);
        // [d2] Box2BoxTransform(weights).apply_deltas, as rpn_select_kernel's decode_mode 1
        bool valid;
        const float4 b = osr_b2b_decode(osr_cell_anchor(cell_anchors, l, A, a, cell, W, fstride), d, rw, &valid);
        valid = valid && osr_box_finite(d);  // dfin: an infinite size delta gives a finite box (the clamp, or exp(-Inf) = 0)
        bad |= !valid;
        *reinterpret_cast<float4*>(c_boxes + o * 4) = valid ? b : make_float4(0.f, 0.f, 0.f, 0.f);
        c_scores[o] = 1.0f / (1.0f + expf(-z));
        c_cls[o] = kc;
        c_cand[o] = valid ? 1 : 0;
        c_src[o] = idx;
    }
    if (tid == 0) counts[img * lv.num_levels + l] = k;
    if (bad) atomicOr(status_flags, 1);
}

// ------------------------------------------------------------------------------------------------------
static osr_status rn_fill(const osr_rpn_levels* in, int n, int K, int topk, long long pitch_cls, long long pitch_box, int elem_bytes, RnLevels* o,
                          long long* surv_total) {
    OSR_REQUIRE(in && in->num_levels >= 1 && in->num_levels <= OSR_MAX_LEVELS && in->num_anchors >= 1 && K >= 1 && topk >= 1 && n >= 1 && n <= 65535,
                OSR_ERR_INVALID_ARG, "osr_retinanet_select: bad level table / num_classes / topk / n");
    OSR_REQUIRE(topk <= SEL_MAXK, OSR_ERR_UNSUPPORTED, "osr_retinanet_select: topk %d > %d", topk, SEL_MAXK);
    const long long AK = (long long)in->num_anchors * K;
    OSR_REQUIRE(AK < (1ll << 24), OSR_ERR_UNSUPPORTED, "osr_retinanet_select: A * K too large");
    OSR_REQUIRE(pitch_cls >= AK && pitch_box >= 4ll * in->num_anchors, OSR_ERR_INVALID_ARG,
                "osr_retinanet_select: pitch_cls %lld < A*K = %lld or pitch_box %lld < 4A = %d", pitch_cls, AK, pitch_box, 4 * in->num_anchors);
    OSR_REQUIRE(pitch_cls < (1ll << 24) && pitch_box < (1ll << 24), OSR_ERR_UNSUPPORTED, "osr_retinanet_select: pitch too large");
    OSR_REQUIRE(pitch_box % 4 == 0, OSR_ERR_UNSUPPORTED, "osr_retinanet_select: pitch_box %lld is not a multiple of 4 (16-byte delta rows)", pitch_box);
    o->num_levels = in->num_levels; o->A = in->num_anchors; o->K = K; o->AK = (int)AK;
    o->pitch_cls = (int)pitch_cls; o->pitch_box = (int)pitch_box; o->topk = topk; o->n = n;
    const int vec = 16 / elem_bytes;
    long long so = 0, bo = 0;
    for (int l = 0; l < in->num_levels; ++l) {
        OSR_REQUIRE(in->h[l] >= 1 && in->w[l] >= 1 && in->stride[l] >= 1 && in->offset[l] >= 0 && in->offset[l] % in->num_anchors == 0,
                    OSR_ERR_INVALID_ARG, "osr_retinanet_select: bad level %d", l);
        const long long cells = (long long)in->h[l] * in->w[l];
        const long long cnt = cells * AK, span = cells * pitch_cls;
        OSR_REQUIRE(cnt < (1ll << 31) - 64 && span < (1ll << 31) - 64, OSR_ERR_UNSUPPORTED,
                    "osr_retinanet_select: level %d has %lld elements per image (>= 2^31)", l, span);
        o->h[l] = in->h[l]; o->w[l] = in->w[l]; o->stride[l] = in->stride[l];
        o->cnt[l] = (int)cnt; o->span[l] = (int)span;
        o->cell_off[l] = in->offset[l] / in->num_anchors;
        long long caps = cnt / 32 + 1;
        if (caps < RN_MIN_SURVIVORS) caps = RN_MIN_SURVIVORS;
        if (caps > cnt) caps = cnt;
        o->caps[l] = (int)caps;
        o->surv_off[l] = so;
        so += caps * n;
        const long long vecs = span / vec + 2;  // the vectors that can touch a segment, whatever its alignment in the buffer
        o->chunks[l] = (int)((vecs + RN_CHUNK_VECS - 1) / RN_CHUNK_VECS);
        o->block_off[l] = (int)bo;
        bo += (long long)o->chunks[l] * n;
        OSR_REQUIRE(bo < (1ll << 31) - 1, OSR_ERR_UNSUPPORTED, "osr_retinanet_select: too many workgroups");
    }
    o->block_off[in->num_levels] = (int)bo;
    *surv_total = so;
    return OSR_OK;
}

// per segment: the list's counter, the second filter's counter, its key threshold, the histogram of the leading key digit
static int64_t rn_counter_bytes(int n, int num_levels) { return ((int64_t)n * num_levels * (3 + RN_DIGITS) * 4 + 15) & ~15ll; }

extern "C" int32_t osr_retinanet_select_capacity(const osr_rpn_levels* lv, int32_t topk) {
    if (!lv || lv->num_levels < 1 || lv->num_levels > OSR_MAX_LEVELS || topk < 1) {
        osr_set_error("osr_retinanet_select_capacity: bad level table / topk");
        return OSR_ERR_INVALID_ARG;
    }
    if (topk > SEL_MAXK) {
        osr_set_error("osr_retinanet_select_capacity: topk %d > %d", topk, SEL_MAXK);
        return OSR_ERR_UNSUPPORTED;
    }
    return lv->num_levels * topk;
}

extern "C" int64_t osr_retinanet_select_workspace_bytes(const osr_rpn_levels* lv, int32_t n, int32_t num_classes, int32_t topk) {
    RnLevels s;
    long long surv;
    // (the capacities depend on neither the pitches nor the dtype: the real widths stand in)
    const osr_status st = rn_fill(lv, n, num_classes, topk, lv ? (long long)lv->num_anchors * num_classes : 0, lv ? 4ll * lv->num_anchors : 0, 2, &s, &surv);
    if (st != OSR_OK) return st;
    return (int64_t)surv * 8 + rn_counter_bytes(n, s.num_levels);
}

extern "C" osr_status osr_retinanet_select(const osr_rpn_levels* lv, const float* cell_anchors, const void* logits, int32_t logits_dtype,
                                           int64_t pitch_cls, const float* deltas, int64_t pitch_box, int32_t n, int32_t num_classes, int32_t topk,
                                           float logit_thresh, const float reg_weights[4], float* c_boxes, float* c_scores, int32_t* c_cls,
                                           int32_t* c_cand, int32_t* c_src, int32_t* counts, int32_t* status_flags, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
    OSR_REQUIRE(osr_dtype_ok(logits_dtype), OSR_ERR_INVALID_ARG, "osr_retinanet_select: bad dtype %d", logits_dtype);
    RnLevels s;
    long long surv_total;
    const osr_status fs = rn_fill(lv, n, num_classes, topk, pitch_cls, pitch_box, osr_dtype_size(logits_dtype), &s, &surv_total);
    if (fs != OSR_OK) return fs;
    OSR_REQUIRE(cell_anchors && logits && deltas && reg_weights && c_boxes && c_scores && c_cls && c_cand && c_src && counts && status_flags && workspace,
                OSR_ERR_INVALID_ARG, "osr_retinanet_select: null pointer");
    OSR_REQUIRE(reg_weights[0] > 0.f && reg_weights[1] > 0.f && reg_weights[2] > 0.f && reg_weights[3] > 0.f, OSR_ERR_INVALID_ARG,
                "osr_retinanet_select: reg_weights must be positive");
    OSR_REQUIRE(!(logit_thresh != logit_thresh), OSR_ERR_INVALID_ARG, "osr_retinanet_select: logit_thresh is NaN");
    OSR_REQUIRE((((uintptr_t)logits | (uintptr_t)deltas | (uintptr_t)c_boxes | (uintptr_t)workspace) & 15) == 0, OSR_ERR_UNSUPPORTED,
                "osr_retinanet_select: logits, deltas, c_boxes and workspace must be 16-byte aligned");
    const int64_t cnt_bytes = rn_counter_bytes(n, s.num_levels);
    const int64_t need = (int64_t)surv_total * 8 + cnt_bytes;
    OSR_REQUIRE(workspace_bytes >= need, OSR_ERR_WORKSPACE, "osr_retinanet_select: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    // the histograms first: rn_refine_kernel reads them 16 bytes at a time
    const int nseg = n * s.num_levels;
    int* hist = (int*)workspace;
    int* surv_cnt = hist + (int64_t)nseg * RN_DIGITS;
    int* cnt2 = surv_cnt + nseg;
    unsigned int* thr2 = (unsigned int*)(cnt2 + nseg);
    unsigned long long* surv = (unsigned long long*)((char*)workspace + cnt_bytes);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status_flags, 0, sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(workspace, 0, (size_t)cnt_bytes, st) != hipSuccess) {
        osr_set_error("osr_retinanet_select: memset failed");
        return OSR_ERR_LAUNCH;
    }
    const float4 rw = make_float4(reg_weights[0], reg_weights[1], reg_weights[2], reg_weights[3]);
    const dim3 g1((unsigned)s.block_off[s.num_levels]), g2(s.num_levels, n);
#define RN_LAUNCH(T)                                                                                                                     \
    do {                                                                                                                                 \
        hipLaunchKernelGGL((rn_filter_kernel<T, 0>), g1, dim3(RN_FILTER_THREADS), 0, st, s, (const T*)logits, logit_thresh, surv, surv_cnt, cnt2, thr2, hist); \
        OSR_CHECK_LAUNCH("osr_retinanet_select(filter)");                                                                                \
        hipLaunchKernelGGL((rn_filter_kernel<T, 1>), g1, dim3(RN_FILTER_THREADS), 0, st, s, (const T*)logits, logit_thresh, surv, surv_cnt, cnt2, thr2, hist); \
        OSR_CHECK_LAUNCH("osr_retinanet_select(histogram)");                                                                             \
        hipLaunchKernelGGL(rn_refine_kernel, g2, dim3(64), 0, st, s, surv_cnt, hist, thr2);                                             \
        OSR_CHECK_LAUNCH("osr_retinanet_select(refine)");                                                                                \
        hipLaunchKernelGGL((rn_filter_kernel<T, 2>), g1, dim3(RN_FILTER_THREADS), 0, st, s, (const T*)logits, logit_thresh, surv, surv_cnt, cnt2, thr2, hist); \
        OSR_CHECK_LAUNCH("osr_retinanet_select(second filter)");                                                                         \
        hipLaunchKernelGGL(rn_select_kernel<T>, g2, dim3(SEL_THREADS), 0, st, s, cell_anchors, (const T*)logits, deltas, logit_thresh, rw, \
                           surv, surv_cnt, cnt2, c_boxes, c_scores, c_cls, c_cand, c_src, counts, status_flags);                         \
        OSR_CHECK_LAUNCH("osr_retinanet_select(select)");                                                                                \
    } while (0)
    if (logits_dtype == OSR_F32) RN_LAUNCH(float);
    else if (logits_dtype == OSR_F16) RN_LAUNCH(f16_t);
    else RN_LAUNCH(bf16_t);
#undef RN_LAUNCH
    return OSR_OK;
}
