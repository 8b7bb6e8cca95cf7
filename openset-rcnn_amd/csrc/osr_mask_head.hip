// The tail of [d2] MaskRCNNConvUpsampleHead at test time, and detector_postprocess's mask pasting, for gfx950 (include/osr.h:
// osr_mask_upsample_predict, osr_paste_masks).
//
// osr_mask_upsample_predict: deconv = ConvTranspose2d(Cin -> Cmid, 2 x 2, stride 2) + bias + ReLU, predictor = Conv2d(Cmid -> K, 1 x 1),
// mask_rcnn_inference = the sigmoid of the RoI's class row (row 0 when class-agnostic). A stride-2 2 x 2 transposed convolution has no
// overlap: output pixel (2y + dy, 2x + dx) is the product of input pixel (y, x) with the (Cin, Cmid) matrix of tap (dy, dx). So the
// layer is four independent GEMMs with M = R S S rows, K = Cin, N = Cmid, and the predictor is a dot product over the Cmid outputs of
// ONE (row, tap): it is taken in the epilogue from the fp32 accumulators, and the (R, 2S, 2S, Cmid) intermediate is never stored.
//
// One workgroup (4 waves) per tile of BM rows: the tile's Cin-deep rows are loaded into LDS once and stay there; wave t owns tap t and
// walks the Cmid columns in chunks of 64 (two 32 x 32 MFMA column blocks), so the dot product is wave-local and the summation order is
// fixed (repeats are bit-identical; no atomics). The weights come from global memory (4 Cin Cmid elements, L2-resident) in fragment
// order -- host/weights.py pack_deconv_weight lays them out so that a wave's B fragment is one contiguous load. fp16 / bf16:
// v_mfma_f32_32x32x16 with fp32 accumulation, BM = 64. fp32 (the parity mode): v_mfma_f32_32x32x2_f32, an exact fp32 FMA chain, BM = 32.
#include "osr_common.h"
#include "osr_mask_mfma.h"

#define MH_MAX_LDS 65536  // static limit of a workgroup's LDS without an opt-in

struct MaskHeadArgs {
    const void* x;
    const void* w;
    const float* bias;
    const float* pred_w;
    const float* pred_b;
    const long long* classes;
    const int* rows_valid;
    float* probs;   // sigmoid of the class row's logit, or null
    float* logits;  // the logit itself (training: the loss reads it), or null
    long long M;  // r * s * s
    int s, cin, cmid, num_rows, seg_rows;
};

template <class T>
__global__ __launch_bounds__(256) void mask_upsample_predict_kernel(MaskHeadArgs a) {
    typedef typename MhFrag<T>::type frag_t;
    constexpr int BM = MhFrag<T>::BM, TM = BM / 32, E = MhFrag<T>::E;
    extern __shared__ __attribute__((aligned(16))) unsigned char mh_lds[];
    __shared__ int s_off[BM];  // per tile row: element offset of its class row in pred_w, -1 = the row is written as zeros
    const int tid = threadIdx.x, lane = tid & 63, tap = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ss = a.s * a.s, os = 2 * a.s;
    const long long m0 = (long long)blockIdx.x * BM;
    const int rowb = a.cin * (int)sizeof(T) + MH_PAD;

    int valid = 0;
    if (tid < BM) {
        const long long m = m0 + tid;
        int off = -1;
        if (m < a.M) {
            const int row = mt_row_class(m / ss, a.num_rows, a.classes, a.rows_valid, a.seg_rows);
            if (row >= 0) off = row * a.cmid;
        }
        s_off[tid] = off;
        valid = off >= 0;
    }
    const int any = __syncthreads_or(valid);  // (also publishes s_off)

    // this lane's output pixels: accumulator register q of row block i is tile row i * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5); after
    // the reduction over the 32 columns, lane (lane & 31) == q of each half stores it
    const int dy = tap >> 1, dx = tap & 1;
    const int q_own = lane & 31;
    if (!any) {  // nothing but padding rows: zeros, no loads
        if (q_own < 16) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const long long m = m0 + i * 32 + (q_own & 3) + 8 * (q_own >> 2) + 4 * (lane >> 5);
                if (m < a.M) {
                    const long long roi = m / ss;
                    const int rem = (int)(m - roi * ss), y = rem / a.s, xx = rem - y * a.s;
                    const long long o = roi * (long long)(os * os) + (long long)(2 * y + dy) * os + 2 * xx + dx;
                    if (a.probs) a.probs[o] = 0.f;
                    if (a.logits) a.logits[o] = 0.f;
                }
            }
        }
        return;
    }

    // ---- the tile's rows -> LDS (16-byte pieces; rows past M as zeros) ----
    {
        const int ppr = a.cin * (int)sizeof(T) / 16;  // pieces per row
        const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x);
        for (int e = tid; e < BM * ppr; e += 256) {
            const int row = e / ppr, pc = e - row * ppr;
            const long long m = m0 + row;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (m < a.M) v = *reinterpret_cast<const uint4*>(xb + (size_t)m * a.cin * sizeof(T) + (size_t)pc * 16);
            *reinterpret_cast<uint4*>(mh_lds + row * rowb + pc * 16) = v;
        }
    }
    __syncthreads();

    int poff[TM][16];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) poff[i][q] = s_off[i * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)];

    float dot[TM][16];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) dot[i][q] = 0.f;

    const int nkb = a.cin / (2 * E);  // K blocks
    const frag_t* __restrict__ wf = reinterpret_cast<const frag_t*>(a.w);  // [tap][cmid / 32][nkb][64 lanes] fragments
    const unsigned char* arow = mh_lds + (lane & 31) * rowb + (lane >> 5) * E * (int)sizeof(T);
    for (int n0 = 0; n0 < a.cmid; n0 += 64) {
        mh_f32x16 acc[TM][2];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
        const frag_t* w0 = wf + ((size_t)(tap * (a.cmid >> 5) + (n0 >> 5)) * nkb) * 64 + lane;
        const frag_t* w1 = w0 + (size_t)nkb * 64;
        for (int kb4 = 0; kb4 < nkb; kb4 += 4) {  // (cin % 64 == 0: nkb is a multiple of 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kb = kb4 + u;
                const frag_t fb0 = w0[(size_t)kb * 64], fb1 = w1[(size_t)kb * 64];
                frag_t fa[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const frag_t*>(arow + i * 32 * rowb + kb * 2 * E * (int)sizeof(T));
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    acc[i][0] = MhFrag<T>::mfma(fa[i], fb0, acc[i][0]);
                    acc[i][1] = MhFrag<T>::mfma(fa[i], fb1, acc[i][1]);
                }
            }
        }
        // bias + ReLU in fp32, then this chunk's share of the predictor's dot product (column = n0 + j * 32 + (lane & 31))
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + j * 32 + (lane & 31);
            const float bv = a.bias[col];
            const bool agnostic = a.num_rows == 1;  // one predictor row for every RoI: one load per column
            const float pw0 = a.pred_w[col];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float h = fmaxf(acc[i][j][q] + bv, 0.f);
                    const float pw = agnostic ? pw0 : (poff[i][q] >= 0 ? a.pred_w[poff[i][q] + col] : 0.f);
                    dot[i][q] += h * pw;
                }
        }
    }

    // ---- sum over the 32 columns a half-wave holds, sigmoid, store ----
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        float mine = 0.f;
        int moff = -1;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float v = dot[i][q];
#pragma unroll
            for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
            if (q_own == q) { mine = v; moff = poff[i][q]; }
        }
        if (q_own < 16) {
            const long long m = m0 + i * 32 + (q_own & 3) + 8 * (q_own >> 2) + 4 * (lane >> 5);
            if (m < a.M) {
                float p = 0.f, z = 0.f;
                if (moff >= 0) {
                    z = mine + a.pred_b[moff / a.cmid];
                    p = 1.0f / (1.0f + expf(-z));
                }
                const long long roi = m / ss;
                const int rem = (int)(m - roi * ss), y = rem / a.s, xx = rem - y * a.s;
                const long long o = roi * (long long)(os * os) + (long long)(2 * y + dy) * os + 2 * xx + dx;
                if (a.probs) a.probs[o] = p;
                if (a.logits) a.logits[o] = z;
            }
        }
    }
}

template <class T>
static osr_status mask_head_launch(const MaskHeadArgs& a, hipStream_t st) {
    constexpr int BM = MhFrag<T>::BM;
    const size_t lds = (size_t)BM * (a.cin * sizeof(T) + MH_PAD);
    OSR_REQUIRE(lds + BM * sizeof(int) <= MH_MAX_LDS, OSR_ERR_UNSUPPORTED, "osr_mask_upsample_predict: cin %d: the row tile does not fit 64 KB of LDS (at most 448)", a.cin);
    const long long tiles = (a.M + BM - 1) / BM;
    OSR_REQUIRE(tiles < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_mask_upsample_predict: too many rows");
    hipLaunchKernelGGL((mask_upsample_predict_kernel<T>), dim3((unsigned)tiles), dim3(256), lds, st, a);
    OSR_CHECK_LAUNCH("osr_mask_upsample_predict");
    return OSR_OK;
}

extern "C" osr_status osr_mask_upsample_predict_ex(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t cmid,
                                                   const void* w_packed, const float* bias, const float* pred_w, const float* pred_b,
                                                   int32_t num_rows, const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows,
                                                   float* probs, float* logits, void* stream) {
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: bad dtype");
    OSR_REQUIRE(r >= 0 && s >= 1 && s <= 1024, OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: bad r / s");
    OSR_REQUIRE(cin >= 64 && cin % 64 == 0 && cmid >= 64 && cmid % 64 == 0, OSR_ERR_UNSUPPORTED,
                "osr_mask_upsample_predict: cin and cmid must be multiples of 64, got %d and %d", cin, cmid);
    OSR_REQUIRE(num_rows >= 1 && (int64_t)num_rows * cmid < (1ll << 31), OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: bad num_rows");
    OSR_REQUIRE(!rows_valid || seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: rows_valid needs seg_rows >= 1");
    if (r == 0) return OSR_OK;
    OSR_REQUIRE(num_rows == 1 || classes, OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: a class-specific predictor needs classes");
    OSR_REQUIRE(x && w_packed && bias && pred_w && pred_b && (probs || logits), OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: null pointer");
    OSR_REQUIRE((((uintptr_t)x | (uintptr_t)w_packed) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: x / w_packed must be 16-byte aligned");
    OSR_REQUIRE(r <= (1ll << 31) / ((int64_t)4 * s * s), OSR_ERR_UNSUPPORTED, "osr_mask_upsample_predict: too many RoIs");
    MaskHeadArgs a;
    a.x = x; a.w = w_packed; a.bias = bias; a.pred_w = pred_w; a.pred_b = pred_b;
    a.classes = reinterpret_cast<const long long*>(classes); a.rows_valid = rows_valid; a.probs = probs; a.logits = logits;
    a.M = (long long)r * s * s; a.s = s; a.cin = cin; a.cmid = cmid; a.num_rows = num_rows; a.seg_rows = rows_valid ? seg_rows : 1;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case OSR_F32: return mask_head_launch<float>(a, st);
        case OSR_F16: return mask_head_launch<f16_t>(a, st);
        default: return mask_head_launch<bf16_t>(a, st);
    }
}

extern "C" osr_status osr_mask_upsample_predict(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t cmid,
                                                const void* w_packed, const float* bias, const float* pred_w, const float* pred_b,
                                                int32_t num_rows, const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows,
                                                float* probs, void* stream) {
    OSR_REQUIRE(probs || r == 0, OSR_ERR_INVALID_ARG, "osr_mask_upsample_predict: null pointer");
    return osr_mask_upsample_predict_ex(x, dtype, r, s, cin, cmid, w_packed, bias, pred_w, pred_b, num_rows, classes, rows_valid, seg_rows, probs,
                                        nullptr, stream);
}

// ------------------------------------------------------------------------------------------------------
// [d2] paste_masks_in_image / _do_paste_mask(skip_empty=False) for one image: output pixel (x, y) samples mask r at
//   u = (x + 0.5 - x0) / (x1 - x0) * M - 0.5,  v = (y + 0.5 - y0) / (y1 - y0) * M - 0.5
// (grid_sample, align_corners=False, on the normalised coordinate 2 (x + 0.5 - x0) / (x1 - x0) - 1), bilinear with zeros outside
// the M x M map, and is 1 where the value >= threshold. One thread per output pixel writes its byte whatever it is; only pixels
// whose (u, v) lies inside (-1, M) on both axes -- the box's pixel range plus the half-texel rim -- read the mask.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paste_masks_kernel(const float* __restrict__ probs, const float* __restrict__ boxes, int M, int out_h,
                                                          int out_w, float thr, unsigned char* __restrict__ out) {
    const int r = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= out_w || y >= out_h) return;
    const float x0 = boxes[r * 4 + 0], y0 = boxes[r * 4 + 1], x1 = boxes[r * 4 + 2], y1 = boxes[r * 4 + 3];
    const float u = ((float)x + 0.5f - x0) / (x1 - x0) * (float)M - 0.5f;
    const float v = ((float)y + 0.5f - y0) / (y1 - y0) * (float)M - 0.5f;
    unsigned char bit = 0;
    if (u > -1.0f && u < (float)M && v > -1.0f && v < (float)M) {  // (false for NaN / inf: a degenerate box pastes nothing)
        const float fu = floorf(u), fv = floorf(v);
        const int iu = (int)fu, iv = (int)fv;
        const float au = u - fu, av = v - fv;
        const float* mk = probs + (size_t)r * M * M;
        const bool l = iu >= 0, rr = iu + 1 < M, t = iv >= 0, b = iv + 1 < M;
        const float p00 = (l && t) ? mk[iv * M + iu] : 0.f, p01 = (rr && t) ? mk[iv * M + iu + 1] : 0.f;
        const float p10 = (l && b) ? mk[(iv + 1) * M + iu] : 0.f, p11 = (rr && b) ? mk[(iv + 1) * M + iu + 1] : 0.f;
        const float val = (1.f - av) * ((1.f - au) * p00 + au * p01) + av * ((1.f - au) * p10 + au * p11);
        bit = val >= thr ? 1 : 0;
    }
    out[((size_t)r * out_h + y) * out_w + x] = bit;
}

extern "C" osr_status osr_paste_masks(const float* probs, const float* boxes, int64_t r, int32_t m, int32_t out_h, int32_t out_w,
                                      float threshold, uint8_t* out, void* stream) {
    OSR_REQUIRE(r >= 0 && r <= 65535, OSR_ERR_UNSUPPORTED, "osr_paste_masks: 0 .. 65535 masks per call, got %lld", (long long)r);
    OSR_REQUIRE(m >= 1 && m <= 4096 && out_h >= 1 && out_w >= 1, OSR_ERR_INVALID_ARG, "osr_paste_masks: bad mask or output size");
    OSR_REQUIRE((out_h + 3) / 4 <= 65535, OSR_ERR_UNSUPPORTED, "osr_paste_masks: output too high");
    if (r == 0) return OSR_OK;
    OSR_REQUIRE(probs && boxes && out, OSR_ERR_INVALID_ARG, "osr_paste_masks: null pointer");
    dim3 grid((out_w + 63) / 64, (out_h + 3) / 4, (unsigned)r);
    hipLaunchKernelGGL(paste_masks_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, boxes, m, out_h, out_w, threshold, out);
    OSR_CHECK_LAUNCH("osr_paste_masks");
    return OSR_OK;
}
