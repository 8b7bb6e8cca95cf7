// Training side of the mask branch of the stock heads ([d2] mask_rcnn_loss; include/osr.h "mask branch, training"):
//   osr_mask_targets                       [d2] BitMasks.crop_and_resize: the ground-truth bitmask of each foreground row's matched
//                                          instance, RoIAlign-ed into the row's proposal box at M x M and thresholded at 0.5
//   osr_mask_loss_fwd / osr_mask_loss_bwd  binary_cross_entropy_with_logits(mean) over the foreground rows' M x M logits, the five
//                                          counts behind mask_rcnn/{accuracy, false_positive, false_negative}, and its gradient
// The mask rows are segments of seg_rows rows (one segment per image) of which the first rows_valid[segment] exist -- the
// convention of osr_mask_upsample_predict. A row that does not exist, or whose class is not a predictor row, counts nowhere: its
// targets and its gradient are exact zeros and it enters no normaliser.
// Reductions are two-stage in a fixed order (per-workgroup partials, then one wave): repeats are bit-identical. Compiled with
// -ffp-contract=off so that a target's bilinear average rounds as the reference loop's.
#include "osr_common.h"
#include "osr_loss_common.h"
#include "osr_mask_mfma.h"

#define MT_THREADS 256
#define MT_NV 6

// One sample coordinate of torchvision's pre_calc_for_bilinear_interpolate along one axis (the rule csrc/osr_roi_align.hip
// documents): outside [-1, size] the sample contributes nothing, below 0 it is clamped to 0, the last pixel has no upper neighbour.
__device__ __forceinline__ bool mt_axis_sample(float start, int bin, float bin_size, int i, int grid, int size, int* lo, int* hi, float* wl, float* wh) {
    float v = start + bin * bin_size + ((float)i + .5f) * bin_size / (float)grid;
    if (v < -1.0f || v > (float)size) return false;
    if (v <= 0.f) v = 0.f;
    int l = (int)v, h;
    if (l >= size - 1) { h = l = size - 1; v = (float)l; } else h = l + 1;
    const float f = v - (float)l;
    *lo = l; *hi = h; *wh = f; *wl = 1.f - f;
    return true;
}

// ------------------------------------------------------------------------------------------------------
// osr_mask_targets: one workgroup per mask row, one thread per target pixel (M * M of them, in strides of the workgroup)
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_THREADS) void mask_targets_kernel(const unsigned char* __restrict__ planes, int gmax, int hm, int wm,
                                                                  const int* __restrict__ image_hw, const float* __restrict__ boxes,
                                                                  const int* __restrict__ gt_idx, const int* __restrict__ rows_valid,
                                                                  int seg_rows, int M, unsigned char* __restrict__ out) {
    const long long r = blockIdx.x;
    const int img = (int)(r / seg_rows), j = (int)(r % seg_rows);
    unsigned char* o = out + r * M * M;
    const int g = gt_idx[r];
    const float bx1 = boxes[r * 4 + 0], by1 = boxes[r * 4 + 1], bx2 = boxes[r * 4 + 2], by2 = boxes[r * 4 + 3];
    // (a box that is not finite has no sample grid to walk: zeros, like a row that does not exist)
    if (j >= rows_valid[img] || g < 0 || g >= gmax || !osr_finite(bx1) || !osr_finite(by1) || !osr_finite(bx2) || !osr_finite(by2)) {
        for (int e = threadIdx.x; e < M * M; e += MT_THREADS) o[e] = 0;
        return;
    }
    // the image's own size rules validity and clamps (its plane is padded to the batch's size with zeros)
    const int H = image_hw ? min(max(image_hw[img * 2], 1), hm) : hm, W = image_hw ? min(max(image_hw[img * 2 + 1], 1), wm) : wm;
    const unsigned char* p = planes + ((long long)img * gmax + g) * hm * wm;
    // roi_align(spatial_scale 1, sampling_ratio 0, aligned): offset 0.5, no minimum size, ceil(roi / M) samples per bin and axis
    const float sw = bx1 - 0.5f, sh = by1 - 0.5f, rw = (bx2 - 0.5f) - sw, rh = (by2 - 0.5f) - sh;
    const float bw = rw / (float)M, bh = rh / (float)M;
    const int gh = (int)ceilf(rh / (float)M), gw = (int)ceilf(rw / (float)M);
    const float count = (float)max(gh * gw, 1);
    for (int e = threadIdx.x; e < M * M; e += MT_THREADS) {
        const int ph = e / M, pw = e - ph * M;
        float acc = 0.f;
        for (int iy = 0; iy < gh; ++iy) {
            int yl, yh; float hy, ly;
            if (!mt_axis_sample(sh, ph, bh, iy, gh, H, &yl, &yh, &hy, &ly)) continue;
            for (int ix = 0; ix < gw; ++ix) {
                int xl, xh; float hx, lx;
                if (!mt_axis_sample(sw, pw, bw, ix, gw, W, &xl, &xh, &hx, &lx)) continue;
                const float v1 = p[(long long)yl * wm + xl] ? 1.f : 0.f, v2 = p[(long long)yl * wm + xh] ? 1.f : 0.f;
                const float v3 = p[(long long)yh * wm + xl] ? 1.f : 0.f, v4 = p[(long long)yh * wm + xh] ? 1.f : 0.f;
                acc += hy * hx * v1 + hy * lx * v2 + ly * hx * v3 + ly * lx * v4;
            }
        }
        o[e] = acc / count >= 0.5f ? 1 : 0;
    }
}

extern "C" osr_status osr_mask_targets(const uint8_t* gt_masks, int32_t n, int32_t gmax, int32_t hm, int32_t wm, const int32_t* image_hw,
                                       const float* boxes, const int32_t* gt_idx, const int32_t* rows_valid, int32_t seg_rows, int32_t m_side,
                                       uint8_t* targets, void* stream) {
    OSR_REQUIRE(n >= 1 && gmax >= 1 && hm >= 1 && wm >= 1 && seg_rows >= 1 && m_side >= 1 && m_side <= 256, OSR_ERR_INVALID_ARG,
                "osr_mask_targets: bad n / gmax / plane size / seg_rows / m_side");
    OSR_REQUIRE((int64_t)n * seg_rows < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_mask_targets: too many rows");
    OSR_REQUIRE(gt_masks && boxes && gt_idx && rows_valid && targets, OSR_ERR_INVALID_ARG, "osr_mask_targets: null pointer");
    hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)(n * seg_rows)), dim3(MT_THREADS), 0, (hipStream_t)stream, gt_masks, gmax, hm, wm, image_hw,
                       boxes, gt_idx, rows_valid, seg_rows, m_side, targets);
    OSR_CHECK_LAUNCH("osr_mask_targets");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// osr_mask_loss_fwd: {loss_mask, foreground rows, incorrect, positive, false positive, false negative}
// ------------------------------------------------------------------------------------------------------
struct MaskLoss {
    const float* logits; const unsigned char* targets; const long long* classes; const int* rows_valid;
    long long rows; int mm, num_rows, seg_rows;
};

__global__ __launch_bounds__(MT_THREADS) void mask_loss_kernel(MaskLoss p, float* __restrict__ partial /* [OSR_LOSS_RED_BLOCKS][MT_NV] */) {
    float v[MT_NV] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // bce, pixels of foreground rows, incorrect, positive, false positive, false negative
    const long long total = p.rows * p.mm;
    for (long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * MT_THREADS) {
        if (mt_row_class(i / p.mm, p.num_rows, p.classes, p.rows_valid, p.seg_rows) < 0) continue;
        const float x = p.logits[i];
        const bool t = p.targets[i] != 0, wrong = (x > 0.f) != t;
        v[0] += osr_bce_with_logits(x, t ? 1.f : 0.f);
        v[1] += 1.f;
        v[2] += wrong ? 1.f : 0.f;
        v[3] += t ? 1.f : 0.f;
        v[4] += wrong && !t ? 1.f : 0.f;
        v[5] += wrong && t ? 1.f : 0.f;
    }
    osr_loss_block_reduce_store<MT_NV>(v, partial);
}

__global__ __launch_bounds__(64) void mask_loss_final(const float* __restrict__ partial, int mm, float weight, float* __restrict__ out) {
    float s[MT_NV];
    for (int q = 0; q < MT_NV; ++q) s[q] = osr_loss_column_sum(partial, OSR_LOSS_RED_BLOCKS, MT_NV, q);
    if (threadIdx.x == 0) {
        out[0] = s[0] / fmaxf(s[1], 1.0f) * weight;  // (no foreground row: 0 / 1)
        out[1] = s[1] / (float)mm;
        out[2] = s[2]; out[3] = s[3]; out[4] = s[4]; out[5] = s[5];
    }
}

static const char* mask_loss_fill(MaskLoss* p, const float* logits, const uint8_t* targets, int64_t rows, int32_t m_side, int32_t num_rows,
                                  const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows) {
    if (rows < 0 || m_side < 1 || m_side > 256 || num_rows < 1) return "bad rows / m_side / num_rows";
    if (rows > 0 && (!logits || !targets)) return "null pointer";
    if (rows_valid && seg_rows < 1) return "rows_valid needs seg_rows >= 1";
    if (rows > 0 && num_rows > 1 && !classes) return "a class-specific predictor needs classes";
    *p = MaskLoss{logits, targets, (const long long*)classes, rows_valid, (long long)rows, m_side * m_side, num_rows, seg_rows};
    return nullptr;
}

extern "C" osr_status osr_mask_loss_fwd(const float* logits, const uint8_t* targets, int64_t rows, int32_t m_side, int32_t num_rows,
                                        const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows, float loss_weight, float* out6,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    MaskLoss p;
    const char* bad = mask_loss_fill(&p, logits, targets, rows, m_side, num_rows, classes, rows_valid, seg_rows);
    OSR_REQUIRE(!bad, OSR_ERR_INVALID_ARG, "osr_mask_loss_fwd: %s", bad ? bad : "");
    // (the counts are summed as fp32 integers: exact up to 2^24 pixels)
    OSR_REQUIRE(rows * p.mm <= (1ll << 24), OSR_ERR_UNSUPPORTED, "osr_mask_loss_fwd: more than 2^24 mask pixels");
    OSR_REQUIRE(out6 && workspace, OSR_ERR_INVALID_ARG, "osr_mask_loss_fwd: null pointer");
    OSR_REQUIRE(workspace_bytes >= (int64_t)OSR_LOSS_RED_BLOCKS * MT_NV * 4, OSR_ERR_WORKSPACE, "osr_mask_loss_fwd: workspace needs %d bytes", OSR_LOSS_RED_BLOCKS * MT_NV * 4);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mask_loss_kernel, dim3(OSR_LOSS_RED_BLOCKS), dim3(MT_THREADS), 0, st, p, (float*)workspace);
    OSR_CHECK_LAUNCH("osr_mask_loss_fwd");
    hipLaunchKernelGGL(mask_loss_final, dim3(1), dim3(64), 0, st, (const float*)workspace, p.mm, loss_weight, out6);
    OSR_CHECK_LAUNCH("osr_mask_loss_fwd(final)");
    return OSR_OK;
}

// foreground rows for osr_loss_count_rows_kernel: the backward's normaliser is the forward's
struct MaskRowIsForeground {
    MaskLoss p;
    __device__ bool operator()(long long r) const { return mt_row_class(r, p.num_rows, p.classes, p.rows_valid, p.seg_rows) >= 0; }
};

__global__ __launch_bounds__(MT_THREADS) void mask_loss_bwd_kernel(MaskLoss p, float scale, const float* __restrict__ count, float* __restrict__ d_logits) {
    const float s = scale / fmaxf(count[0] * (float)p.mm, 1.0f);
    const long long total = p.rows * p.mm;
    for (long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * MT_THREADS) {
        const bool fg = mt_row_class(i / p.mm, p.num_rows, p.classes, p.rows_valid, p.seg_rows) >= 0;
        d_logits[i] = fg ? (osr_sigmoid(p.logits[i]) - (p.targets[i] ? 1.f : 0.f)) * s : 0.f;
    }
}

extern "C" osr_status osr_mask_loss_bwd(const float* logits, const uint8_t* targets, int64_t rows, int32_t m_side, int32_t num_rows,
                                        const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows, float scale, float* d_logits,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    MaskLoss p;
    const char* bad = mask_loss_fill(&p, logits, targets, rows, m_side, num_rows, classes, rows_valid, seg_rows);
    OSR_REQUIRE(!bad, OSR_ERR_INVALID_ARG, "osr_mask_loss_bwd: %s", bad ? bad : "");
    OSR_REQUIRE(rows * p.mm <= (1ll << 24), OSR_ERR_UNSUPPORTED, "osr_mask_loss_bwd: more than 2^24 mask pixels");
    OSR_REQUIRE((rows == 0 || d_logits) && workspace, OSR_ERR_INVALID_ARG, "osr_mask_loss_bwd: null pointer");
    OSR_REQUIRE(workspace_bytes >= 16, OSR_ERR_WORKSPACE, "osr_mask_loss_bwd: workspace needs 16 bytes");
    if (rows == 0) return OSR_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(osr_loss_count_rows_kernel<MaskRowIsForeground>, dim3(1), dim3(256), 0, st, MaskRowIsForeground{p}, p.rows, (float*)workspace);
    OSR_CHECK_LAUNCH("osr_mask_loss_bwd(count)");
    const long long total = p.rows * p.mm;
    const unsigned blocks = (unsigned)((total + MT_THREADS - 1) / MT_THREADS < 4096 ? (total + MT_THREADS - 1) / MT_THREADS : 4096);
    hipLaunchKernelGGL(mask_loss_bwd_kernel, dim3(blocks), dim3(MT_THREADS), 0, st, p, scale, (const float*)workspace, d_logits);
    OSR_CHECK_LAUNCH("osr_mask_loss_bwd");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// osr_mask_upsample_predict_bwd: the backward of osr_mask_upsample_predict's deconv + ReLU + predictor (csrc/osr_mask_head.hip).
// One workgroup (4 waves) per tile of 64 rows of x, as in the forward, whose loop it repeats: the tile's rows stay in LDS, wave t
// owns tap t and walks the Cmid columns in chunks of 64, and u = deconv(x) + b comes out of the same MFMA sequence in the same
// registers. Per chunk, from the fp32 accumulators:
//   g[pix, n]   = d_logit[pix] * pred_w[class][n] * (u > 0)          the gradient of the (never stored) upsampled activation
//   column sums of g (d_deconv_b) and of d_logit * relu(u), the latter apart for the at most two RoIs a tile touches (d_pred_w)
// g goes to LDS in the storage type, row-major (the accumulator holds it column-major: this is the transpose the second contraction
// needs), and from there (a) to global memory in tap-major order for the weight gradient (four 1 x 1 osr_conv2d_wgrad calls) and
// (b) into the second contraction dx[m, c] = sum over taps and n of g_t[m, n] W_t[c, n]: K = 4 taps x 64 columns per chunk, wave w
// accumulating the 32-column blocks w, w + 4, ... of dx over all chunks. Its B operand is the deconv weight packed with the roles of
// Cin and Cmid exchanged (host/weights.py pack_deconv_weight of the transposed weight).
// The column sums leave the workgroup as one partial per tile in a workspace; two small kernels reduce them in a fixed order
// (per RoI, then per class): no atomics, repeats are bit-identical.
// ------------------------------------------------------------------------------------------------------
#define MB_BM 64
#define MB_GROW (64 * 2 + 16)  // bytes per row of a tap's g chunk in LDS: 64 storage elements + padding (16-byte aligned rows)
#define MB_MAX_LDS (160 * 1024 - 1024)  // dynamic LDS the kernel may ask for: the CU's 160 KB less its static arrays

struct MaskBwdArgs {
    const void* x; const void* w; const void* wt;
    const float* bias; const float* pred_w;
    const long long* classes; const int* rows_valid;
    const float* d_logits;
    void* dx; void* g_out;     // g_out may be null
    int dx_f32;                // dx is fp32 instead of the storage type
    float* partial;            // [tiles][3][cmid]: d_pred_w share of the tile's first RoI, of its second RoI, d_deconv_b share
    long long M;
    int s, cin, cmid, num_rows, seg_rows;
};

// planes: 1 (fp16) or 2 (bf16: g as hi + lo, see the kernel)
static size_t mask_bwd_lds(int cin, int cmid, int planes) {
    return (size_t)MB_BM * (cin * 2 + MH_PAD) + (size_t)planes * 4 * MB_BM * MB_GROW + (size_t)4 * 3 * cmid * 4 + (size_t)4 * MB_BM * 4;
}

// PL = 2 (bf16): g enters both contractions as two planes, hi = bf16(g) and lo = bf16(g - hi) -- 16 significant bits instead of 8, which
// alone would cost 2e-3 of the gradients' magnitude; the second contraction runs over both, g_out holds both (plane-major).
template <class T, int NB, int PL>
__global__ __launch_bounds__(256) void mask_upsample_predict_bwd_kernel(MaskBwdArgs a) {
    typedef typename MhFrag<T>::type frag_t;
    constexpr int BM = MB_BM, TM = 2, E = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char mb_lds[];
    __shared__ int s_off[BM];   // per tile row: element offset of its class row in pred_w, -1 = the row does not count
    __shared__ int s_slot[BM];  // 0: the row belongs to the tile's first RoI, 1: to the next one
    __shared__ int s_soff[2];   // the class-row offset of the tile's first / second RoI (-1: it does not count or does not exist)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tap = wave;
    const int ss = a.s * a.s, os = 2 * a.s;
    const long long m0 = (long long)blockIdx.x * BM;
    const int rowb = a.cin * 2 + MH_PAD;
    unsigned char* xl = mb_lds;
    unsigned char* gl = xl + (size_t)BM * rowb;
    float* sp = reinterpret_cast<float*>(gl + (size_t)PL * 4 * BM * MB_GROW);  // [tap][3][cmid]; gl: [plane][tap][row]
    float* sdl = sp + (size_t)4 * 3 * a.cmid;                             // [tap][BM]: d_logit of (row, tap), 0 on rows that do not count
    const long long roi0 = m0 / ss;

    int valid = 0;
    if (tid < BM) {
        const long long m = m0 + tid;
        int off = -1, slot = 0;
        if (m < a.M) {
            const long long roi = m / ss;
            const long long cls = a.classes ? a.classes[roi] : 0;
            const bool live = !a.rows_valid || (int)(roi % a.seg_rows) < a.rows_valid[roi / a.seg_rows];
            if (live && cls >= 0 && (a.num_rows == 1 || cls < a.num_rows)) off = (a.num_rows == 1 ? 0 : (int)cls) * a.cmid;
            slot = (int)(roi - roi0);  // 0 or 1: s * s >= 64
        }
        s_off[tid] = off; s_slot[tid] = slot;
        valid = off >= 0;
        if (tid < 2) {  // the tile's (at most) two RoIs themselves
            const long long roi = roi0 + tid;
            int so = -1;
            if (roi * ss < a.M) {
                const long long cls = a.classes ? a.classes[roi] : 0;
                const bool live = !a.rows_valid || (int)(roi % a.seg_rows) < a.rows_valid[roi / a.seg_rows];
                if (live && cls >= 0 && (a.num_rows == 1 || cls < a.num_rows)) so = (a.num_rows == 1 ? 0 : (int)cls) * a.cmid;
            }
            s_soff[tid] = so;
        }
    }
    const int any = __syncthreads_or(valid);  // (also publishes s_off / s_slot / s_soff)
    T* dxp = reinterpret_cast<T*>(a.dx);
    T* gop = reinterpret_cast<T*>(a.g_out);
    if (!any) {  // nothing but rows that do not count: zeros everywhere, no loads
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        const int ppr = a.cin / (a.dx_f32 ? 4 : 8);  // 16-byte pieces per row of dx
        for (int e = tid; e < BM * ppr; e += 256) {
            const int row = e / ppr, pc = e - row * ppr;
            if (m0 + row < a.M) *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(a.dx) + ((size_t)(m0 + row) * ppr + pc) * 16) = z;
        }
        if (gop) {
            const int gpr = a.cmid / 8;
            for (int e = tid; e < PL * 4 * BM * gpr; e += 256) {
                const int t = e / (BM * gpr), rem = e - t * (BM * gpr), row = rem / gpr, pc = rem - row * gpr;
                if (m0 + row < a.M) *reinterpret_cast<uint4*>(gop + ((size_t)t * a.M + (m0 + row)) * a.cmid + pc * 8) = z;
            }
        }
        for (int e = tid; e < 3 * a.cmid; e += 256) a.partial[(size_t)blockIdx.x * 3 * a.cmid + e] = 0.f;
        return;
    }

    // ---- the tile's rows -> LDS (rows past M as zeros), and the d_logit of every (row, tap) ----
    {
        const int ppr = a.cin * 2 / 16;
        const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x);
        for (int e = tid; e < BM * ppr; e += 256) {
            const int row = e / ppr, pc = e - row * ppr;
            const long long m = m0 + row;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (m < a.M) v = *reinterpret_cast<const uint4*>(xb + (size_t)m * a.cin * 2 + (size_t)pc * 16);
            *reinterpret_cast<uint4*>(xl + row * rowb + pc * 16) = v;
        }
        {   // thread (t, row)
            const int t = tid >> 6, row = tid & 63;
            const long long m = m0 + row;
            float v = 0.f;
            if (m < a.M && s_off[row] >= 0) {
                const long long roi = m / ss;
                const int rem = (int)(m - roi * ss), y = rem / a.s, xx = rem - y * a.s;
                v = a.d_logits[roi * (long long)(os * os) + (long long)(2 * y + (t >> 1)) * os + 2 * xx + (t & 1)];
            }
            sdl[t * BM + row] = v;
        }
    }
    __syncthreads();

    mh_f32x16 dacc[TM][NB];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int q = 0; q < 16; ++q) dacc[i][b][q] = 0.f;

    const int nkb = a.cin / (2 * E), nblk = a.cin >> 5, ngb = a.cmid / (2 * E);
    const frag_t* __restrict__ wf = reinterpret_cast<const frag_t*>(a.w);    // [tap][cmid / 32][cin / 16][64 lanes]
    const frag_t* __restrict__ wtf = reinterpret_cast<const frag_t*>(a.wt);  // [tap][cin / 32][cmid / 16][64 lanes]
    const unsigned char* arow = xl + (lane & 31) * rowb + (lane >> 5) * E * 2;
    const bool agnostic = a.num_rows == 1;
    const int half = lane >> 5;
    for (int n0 = 0; n0 < a.cmid; n0 += 64) {
        // ---- phase 1: u of this tap's 64 x 64 chunk, exactly as the forward computes it ----
        mh_f32x16 acc[TM][2];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
        const frag_t* w0 = wf + ((size_t)(tap * (a.cmid >> 5) + (n0 >> 5)) * nkb) * 64 + lane;
        const frag_t* w1 = w0 + (size_t)nkb * 64;
        for (int kb4 = 0; kb4 < nkb; kb4 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kb = kb4 + u;
                const frag_t fb0 = w0[(size_t)kb * 64], fb1 = w1[(size_t)kb * 64];
                frag_t fa[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const frag_t*>(arow + i * 32 * rowb + kb * 2 * E * 2);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    acc[i][0] = MhFrag<T>::mfma(fa[i], fb0, acc[i][0]);
                    acc[i][1] = MhFrag<T>::mfma(fa[i], fb1, acc[i][1]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cl = j * 32 + (lane & 31), col = n0 + cl;
            const float bv = a.bias[col];
            // the predictor weight of this column for each of the tile's two RoIs: two loads per column, not one per element
            const int so0 = s_soff[0], so1 = s_soff[1];
            const float pwa = agnostic ? a.pred_w[col] : (so0 >= 0 ? a.pred_w[so0 + col] : 0.f);
            const float pwb = agnostic ? pwa : (so1 >= 0 ? a.pred_w[so1 + col] : 0.f);
            float sg = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = i * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                    const int off = s_off[row];
                    const float dl = sdl[tap * BM + row];
                    const float u = acc[i][j][q] + bv;
                    const bool first = s_slot[row] == 0;
                    const float g = (off >= 0 && u > 0.f) ? dl * (first ? pwa : pwb) : 0.f;
                    const float hd = off >= 0 ? dl * fmaxf(u, 0.f) : 0.f;
                    sg += g;
                    if (first) s0 += hd; else s1 += hd;
                    const T ghi = osr_from_float<T>(g);
                    *reinterpret_cast<T*>(gl + ((size_t)tap * BM + row) * MB_GROW + cl * 2) = ghi;
                    if (PL == 2)
                        *reinterpret_cast<T*>(gl + ((size_t)(4 + tap) * BM + row) * MB_GROW + cl * 2) = osr_from_float<T>(g - osr_to_float(ghi));
                }
            // the two halves of the wave hold different rows of the same column
            sg += __shfl_xor(sg, 32, 64); s0 += __shfl_xor(s0, 32, 64); s1 += __shfl_xor(s1, 32, 64);
            if (half == 0) {
                sp[(tap * 3 + 0) * a.cmid + col] = s0; sp[(tap * 3 + 1) * a.cmid + col] = s1; sp[(tap * 3 + 2) * a.cmid + col] = sg;
            }
        }
        __syncthreads();
        // ---- phase 2: g of the four taps -> global (tap `wave`), and into dx (column blocks wave, wave + 4, ...) ----
        if (gop) {
            for (int e = lane; e < PL * BM * 8; e += 64) {
                const int pt = (e >> 9) * 4 + tap, row = (e >> 3) & 63, pc = e & 7;
                if (m0 + row < a.M)
                    *reinterpret_cast<uint4*>(gop + ((size_t)pt * a.M + (m0 + row)) * a.cmid + n0 + pc * 8) =
                        *reinterpret_cast<const uint4*>(gl + ((size_t)pt * BM + row) * MB_GROW + pc * 16);
            }
        }
        for (int t = 0; t < 4 * PL; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                frag_t fa[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    fa[i] = *reinterpret_cast<const frag_t*>(gl + ((size_t)t * BM + i * 32 + (lane & 31)) * MB_GROW + (kk * 16 + half * E) * 2);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int blk = wave + 4 * b;
                    if (blk < nblk) {
                        const frag_t fb = wtf[((size_t)((t & 3) * nblk + blk) * ngb + (n0 >> 4) + kk) * 64 + lane];
#pragma unroll
                        for (int i = 0; i < TM; ++i) dacc[i][b] = MhFrag<T>::mfma(fa[i], fb, dacc[i][b]);
                    }
                }
            }
        __syncthreads();  // (the next chunk overwrites gl)
    }

    // ---- dx: the storage type (or fp32), rows past M not written ----
    float* dxf = reinterpret_cast<float*>(a.dx);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int blk = wave + 4 * b;
        if (blk < nblk) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const long long m = m0 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                    if (m >= a.M) continue;
                    if (a.dx_f32) dxf[(size_t)m * a.cin + blk * 32 + (lane & 31)] = dacc[i][b][q];
                    else dxp[(size_t)m * a.cin + blk * 32 + (lane & 31)] = osr_from_float<T>(dacc[i][b][q]);
                }
        }
    }
    // ---- the tile's column sums, the four taps in order ----
    for (int e = tid; e < 3 * a.cmid; e += 256)
        a.partial[(size_t)blockIdx.x * 3 * a.cmid + e] =
            ((sp[e] + sp[3 * a.cmid + e]) + sp[6 * a.cmid + e]) + sp[9 * a.cmid + e];
}

// per RoI: s_roi[r][n] = the shares of the tiles r reaches, in tile order; sb_roi[r] = the sum of its d_logits (0 when it does not count)
__global__ __launch_bounds__(256) void mask_bwd_roi_reduce(const float* __restrict__ partial, const float* __restrict__ d_logits,
                                                           const long long* __restrict__ classes, const int* __restrict__ rows_valid, int seg_rows,
                                                           int num_rows, int ss, int cmid, float* __restrict__ s_roi, float* __restrict__ sb_roi) {
    __shared__ float s_red[256];
    const long long r = blockIdx.x;
    const bool counts = mt_row_class(r, num_rows, classes, rows_valid, seg_rows) >= 0;
    const long long t_first = r * ss / MB_BM, t_last = ((r + 1) * ss - 1) / MB_BM;
    for (int n = threadIdx.x; n < cmid; n += 256) {
        float v = 0.f;
        for (long long t = t_first; t <= t_last; ++t) {
            const int slot = (int)(r - t * MB_BM / ss);
            v += partial[((size_t)t * 3 + slot) * cmid + n];
        }
        s_roi[r * cmid + n] = counts ? v : 0.f;
    }
    float b = 0.f;
    if (counts)
        for (int e = threadIdx.x; e < 4 * ss; e += 256) b += d_logits[r * 4 * ss + e];
    s_red[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) sb_roi[r] = s_red[0];
}

// d_deconv_b[n] over the tiles: one workgroup per 16 columns, 16 threads per column each summing every 16th tile in tile order, the 16
// sums added in thread order -- a fixed order, 16 times shorter than one thread per column walking every tile
__global__ __launch_bounds__(256) void mask_bwd_bias_reduce(const float* __restrict__ partial, long long tiles, int cmid, float* __restrict__ d_deconv_b) {
    __shared__ float s_part[16][16];
    const int c = threadIdx.x & 15, grp = threadIdx.x >> 4, n = blockIdx.x * 16 + c;
    float v = 0.f;
    if (n < cmid)
        for (long long t = grp; t < tiles; t += 16) v += partial[((size_t)t * 3 + 2) * cmid + n];
    s_part[grp][c] = v;
    __syncthreads();
    if (grp == 0 && n < cmid) {
        float sum = 0.f;
        for (int k = 0; k < 16; ++k) sum += s_part[k][c];
        d_deconv_b[n] = sum;
    }
}

// per class: d_pred_w[k][n] and d_pred_b[k] over the RoIs of class k in RoI order
__global__ __launch_bounds__(256) void mask_bwd_class_reduce(const float* __restrict__ s_roi, const float* __restrict__ sb_roi,
                                                             const long long* __restrict__ classes,
                                                             const int* __restrict__ rows_valid, int seg_rows, int num_rows, long long rois,
                                                             int cmid, float* __restrict__ d_pred_w, float* __restrict__ d_pred_b) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nw = (long long)num_rows * cmid;
    if (i < nw) {
        const int k = (int)(i / cmid), n = (int)(i - (long long)k * cmid);
        float v = 0.f;
        for (long long r = 0; r < rois; ++r)
            if (mt_row_class(r, num_rows, classes, rows_valid, seg_rows) == k) v += s_roi[r * cmid + n];
        d_pred_w[i] = v;
    } else if (i < nw + num_rows) {
        const int k = (int)(i - nw);
        float v = 0.f;
        for (long long r = 0; r < rois; ++r)
            if (mt_row_class(r, num_rows, classes, rows_valid, seg_rows) == k) v += sb_roi[r];
        d_pred_b[k] = v;
    }
}

extern "C" int64_t osr_mask_upsample_predict_bwd_workspace_bytes(int64_t r, int32_t s, int32_t cmid) {
    if (r < 0 || s < 1 || cmid < 1) { osr_set_error("osr_mask_upsample_predict_bwd_workspace_bytes: bad arguments"); return OSR_ERR_INVALID_ARG; }
    const int64_t tiles = (r * s * s + MB_BM - 1) / MB_BM;
    return (tiles * 3 * cmid + r * cmid + r) * 4 + 16;
}

template <class T, int PL>
static void mask_bwd_launch(const MaskBwdArgs& a, long long tiles, hipStream_t st) {
    const size_t lds = mask_bwd_lds(a.cin, a.cmid, PL);
    static osr_dev_mask attr{0};  // (one per instantiation of this function template)
    osr_once_per_device(attr, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mask_upsample_predict_bwd_kernel<T, 2, PL>), hipFuncAttributeMaxDynamicSharedMemorySize, MB_MAX_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mask_upsample_predict_bwd_kernel<T, 4, PL>), hipFuncAttributeMaxDynamicSharedMemorySize, MB_MAX_LDS);
    });
    if (a.cin <= 256) hipLaunchKernelGGL((mask_upsample_predict_bwd_kernel<T, 2, PL>), dim3((unsigned)tiles), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((mask_upsample_predict_bwd_kernel<T, 4, PL>), dim3((unsigned)tiles), dim3(256), lds, st, a);
}

extern "C" osr_status osr_mask_upsample_predict_bwd(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t cmid,
                                                    const void* w_packed, const void* w_packed_t, const float* bias, const float* pred_w,
                                                    int32_t num_rows, const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows,
                                                    const float* d_logits, void* dx, int32_t dx_dtype, void* g_out, float* d_pred_w, float* d_pred_b,
                                                    float* d_deconv_b, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "osr_mask_upsample_predict_bwd";
    OSR_REQUIRE(dtype == OSR_F16 || dtype == OSR_BF16, OSR_ERR_UNSUPPORTED, "%s: fp16 / bf16 only", who);
    OSR_REQUIRE(dx_dtype == dtype || dx_dtype == OSR_F32, OSR_ERR_UNSUPPORTED, "%s: dx must be fp32 or x's type", who);
    OSR_REQUIRE(r >= 0 && s >= 1 && s <= 1024, OSR_ERR_INVALID_ARG, "%s: bad r / s", who);
    OSR_REQUIRE(s >= 8, OSR_ERR_UNSUPPORTED, "%s: s %d: a tile of 64 rows must reach at most two RoIs (s >= 8)", who, s);
    OSR_REQUIRE(cin >= 64 && cin % 64 == 0 && cin <= 448 && cmid >= 64 && cmid % 64 == 0, OSR_ERR_UNSUPPORTED,
                "%s: cin and cmid must be multiples of 64, cin at most 448, got %d and %d", who, cin, cmid);
    OSR_REQUIRE(mask_bwd_lds(cin, cmid, dtype == OSR_BF16 ? 2 : 1) <= MB_MAX_LDS, OSR_ERR_UNSUPPORTED, "%s: cin %d, cmid %d: the tile does not fit 160 KB of LDS", who, cin, cmid);
    OSR_REQUIRE(num_rows >= 1 && (int64_t)num_rows * cmid < (1ll << 31), OSR_ERR_INVALID_ARG, "%s: bad num_rows", who);
    OSR_REQUIRE(!rows_valid || seg_rows >= 1, OSR_ERR_INVALID_ARG, "%s: rows_valid needs seg_rows >= 1", who);
    OSR_REQUIRE(d_pred_w && d_pred_b && d_deconv_b && workspace, OSR_ERR_INVALID_ARG, "%s: null pointer", who);
    const int64_t need = osr_mask_upsample_predict_bwd_workspace_bytes(r, s, cmid);
    OSR_REQUIRE(workspace_bytes >= need, OSR_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes, (long long)need);
    OSR_REQUIRE(r == 0 || num_rows == 1 || classes, OSR_ERR_INVALID_ARG, "%s: a class-specific predictor needs classes", who);
    OSR_REQUIRE(r == 0 || (x && w_packed && w_packed_t && bias && pred_w && d_logits && dx), OSR_ERR_INVALID_ARG, "%s: null pointer", who);
    OSR_REQUIRE((((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)w_packed_t | (uintptr_t)dx | (uintptr_t)g_out) & 15) == 0, OSR_ERR_INVALID_ARG,
                "%s: x / w_packed / w_packed_t / dx / g must be 16-byte aligned", who);
    OSR_REQUIRE(r <= (1ll << 31) / ((int64_t)4 * s * s), OSR_ERR_UNSUPPORTED, "%s: too many RoIs", who);
    hipStream_t st = (hipStream_t)stream;
    MaskBwdArgs a;
    a.x = x; a.w = w_packed; a.wt = w_packed_t; a.bias = bias; a.pred_w = pred_w;
    a.classes = reinterpret_cast<const long long*>(classes); a.rows_valid = rows_valid; a.d_logits = d_logits;
    a.dx = dx; a.g_out = g_out; a.dx_f32 = dx_dtype == OSR_F32 ? 1 : 0;
    a.M = (long long)r * s * s; a.s = s; a.cin = cin; a.cmid = cmid; a.num_rows = num_rows; a.seg_rows = rows_valid ? seg_rows : 1;
    const long long tiles = (a.M + MB_BM - 1) / MB_BM;
    float* partial = (float*)workspace;
    float* s_roi = partial + tiles * 3 * cmid;
    float* sb_roi = s_roi + (long long)r * cmid;
    a.partial = partial;
    if (r > 0) {
        if (dtype == OSR_F16) mask_bwd_launch<f16_t, 1>(a, tiles, st);
        else mask_bwd_launch<bf16_t, 2>(a, tiles, st);
        OSR_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(mask_bwd_roi_reduce, dim3((unsigned)r), dim3(256), 0, st, (const float*)partial, d_logits, a.classes, rows_valid, a.seg_rows,
                           num_rows, s * s, cmid, s_roi, sb_roi);
        OSR_CHECK_LAUNCH("osr_mask_upsample_predict_bwd(per RoI)");
    }
    const long long outs = (long long)num_rows * cmid + num_rows;
    hipLaunchKernelGGL(mask_bwd_class_reduce, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, (const float*)s_roi, (const float*)sb_roi,
                       a.classes, rows_valid, a.seg_rows, num_rows, (long long)r, cmid, d_pred_w, d_pred_b);
    OSR_CHECK_LAUNCH("osr_mask_upsample_predict_bwd(per class)");
    hipLaunchKernelGGL(mask_bwd_bias_reduce, dim3((unsigned)((cmid + 15) / 16)), dim3(256), 0, st, (const float*)partial, tiles, cmid, d_deconv_b);
    OSR_CHECK_LAUNCH("osr_mask_upsample_predict_bwd(bias)");
    return OSR_OK;
}
