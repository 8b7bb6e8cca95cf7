// Training step of the stock detectron2 heads that Base-RCNN-FPN.yaml selects (BASELINE config 1): [d2] RPN.losses,
// FastRCNNOutputLayers.losses and the backward of StandardRPNHead's two 1x1 convolutions -- include/osr.h "stock heads".
//
// [d2] RPN.losses: BCE-with-logits over the sampled anchors (label >= 0) and smooth L1 of the deltas of the positive anchors
// against Box2BoxTransform(RPN.BBOX_REG_WEIGHTS).get_deltas(anchor, matched GT), both divided by BATCH_SIZE_PER_IMAGE * n.
// [d2] FastRCNNOutputLayers.losses: mean cross entropy over the (K+1) logits of the sampled rows, smooth L1 of the foreground
// rows' deltas (class-agnostic 4-vector or the GT class's group of 4K) against Box2BoxTransform(10,10,5,5), divided by the number
// of sampled rows. Padding rows (class -1) count nowhere.
// Reductions are two-stage in a fixed order (per-workgroup partials, then one wave): bitwise reproducible. Compiled with
// -ffp-contract=off like the other loss kernels.
#include "osr_common.h"
#include "osr_box_loss.h"
#include "osr_loss_common.h"

// ------------------------------------------------------------------------------------------------------
// [d2] RPN.losses, forward: {loss_rpn_cls, loss_rpn_loc, num_pos, num_neg}
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void std_rpn_losses_kernel(OsrLossLevels lv, const float* __restrict__ cell, int n, const float* __restrict__ logits,
                                                             const float* __restrict__ deltas, const signed char* __restrict__ labels,
                                                             const float* __restrict__ matched, float4 bw, float beta, float* __restrict__ partial) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const long long total = (long long)n * lv.R;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const signed char lb = labels[i];
        if (lb < 0) continue;
        const int img = (int)(i / lv.R), r = (int)(i - (long long)img * lv.R);
        int l, ci;
        const float4 a = osr_loss_anchor(lv, cell, r, &l, &ci);
        const long long pi = osr_loss_pred_index(lv, l, img, ci);
        v[0] += osr_bce_with_logits(logits[pi], (float)lb);
        if (lb == 1) {
            v[2] += 1.f;
            const float4 t = osr_b2b_get_deltas(a, *reinterpret_cast<const float4*>(matched + i * 4), bw.x, bw.y, bw.z, bw.w);
            const float4 d = *reinterpret_cast<const float4*>(deltas + pi * 4);
            v[1] += osr_smooth_l1(d.x - t.x, beta) + osr_smooth_l1(d.y - t.y, beta) + osr_smooth_l1(d.z - t.z, beta) + osr_smooth_l1(d.w - t.w, beta);
        } else {
            v[3] += 1.f;
        }
    }
    osr_loss_block_reduce_store<4>(v, partial);
}

static const char* std_rpn_check(const osr_rpn_levels* lvl, OsrLossLevels* lv, const float* cell, const float* logits, const float* deltas,
                                 const int8_t* labels, const float* matched, const float* bw, int n, int batch, float beta) {
    if (!osr_loss_levels_fill(lvl, lv) || !osr_loss_levels_whole_pixels(lvl, 8)) return "bad level table (1 <= A <= 8, offsets in whole pixels)";
    if (!cell || !logits || !deltas || !labels || !matched || !bw) return "null pointer";
    if (n < 1 || batch < 1 || !(beta >= 0.f)) return "bad n / batch size / beta";
    if ((((uintptr_t)deltas | (uintptr_t)matched) & 15) != 0) return "deltas and matched boxes must be 16-byte aligned";
    return nullptr;
}

extern "C" osr_status osr_std_rpn_losses_fwd(const osr_rpn_levels* lvl, const float* cell_anchors, int32_t n, const float* pred_logits,
                                             const float* pred_deltas, const int8_t* labels, const float* matched_boxes, const float b2b_weights[4],
                                             float smooth_l1_beta, float cls_weight, float loc_weight, int32_t batch_size_per_image, float* out4,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
    OsrLossLevels lv;
    const char* bad = std_rpn_check(lvl, &lv, cell_anchors, pred_logits, pred_deltas, labels, matched_boxes, b2b_weights, n, batch_size_per_image,
                                    smooth_l1_beta);
    OSR_REQUIRE(!bad, OSR_ERR_INVALID_ARG, "osr_std_rpn_losses_fwd: %s", bad ? bad : "");
    OSR_REQUIRE(out4 && workspace, OSR_ERR_INVALID_ARG, "osr_std_rpn_losses_fwd: null pointer");
    OSR_REQUIRE(workspace_bytes >= (int64_t)OSR_LOSS_RED_BLOCKS * 4 * 4, OSR_ERR_WORKSPACE, "osr_std_rpn_losses_fwd: workspace needs %d bytes", OSR_LOSS_RED_BLOCKS * 16);
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const float norm = (float)batch_size_per_image * (float)n;
    const OsrLossScale scale = {{cls_weight / norm, loc_weight / norm, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f}};
    hipLaunchKernelGGL(std_rpn_losses_kernel, dim3(OSR_LOSS_RED_BLOCKS), dim3(256), 0, st, lv, cell_anchors, n, pred_logits, pred_deltas,
                       (const signed char*)labels, matched_boxes, make_float4(b2b_weights[0], b2b_weights[1], b2b_weights[2], b2b_weights[3]),
                       smooth_l1_beta, partial);
    OSR_CHECK_LAUNCH("osr_std_rpn_losses_fwd");
    hipLaunchKernelGGL(osr_loss_final_reduce, dim3(1), dim3(64), 0, st, partial, OSR_LOSS_RED_BLOCKS, 4, scale, -1, out4);
    OSR_CHECK_LAUNCH("osr_std_rpn_losses_fwd(final)");
    return OSR_OK;
}

// backward: every anchor writes its A-column logit gradient and its four delta gradients into d_rows (pixel rows, 5A columns)
__global__ __launch_bounds__(256) void std_rpn_losses_bwd_kernel(OsrLossLevels lv, const float* __restrict__ cell, int n, const float* __restrict__ logits,
                                                                 const float* __restrict__ deltas, const signed char* __restrict__ labels,
                                                                 const float* __restrict__ matched, float4 bw, float beta, float s_cls, float s_loc,
                                                                 float* __restrict__ d_rows) {
    const int A = lv.num_anchors, W = 5 * A;
    const long long total = (long long)n * lv.R;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int img = (int)(i / lv.R), r = (int)(i - (long long)img * lv.R);
        const signed char lb = labels[i];
        int l, ci;
        const float4 a = osr_loss_anchor(lv, cell, r, &l, &ci);
        const long long pi = osr_loss_pred_index(lv, l, img, ci);
        const long long row = pi / A;
        const int ai = (int)(pi - row * A);
        float* d = d_rows + row * W;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (lb == 1) {
            const float4 t = osr_b2b_get_deltas(a, *reinterpret_cast<const float4*>(matched + i * 4), bw.x, bw.y, bw.z, bw.w);
            const float4 p = *reinterpret_cast<const float4*>(deltas + pi * 4);
            g[0] = s_loc * osr_smooth_l1_grad(p.x - t.x, beta); g[1] = s_loc * osr_smooth_l1_grad(p.y - t.y, beta);
            g[2] = s_loc * osr_smooth_l1_grad(p.z - t.z, beta); g[3] = s_loc * osr_smooth_l1_grad(p.w - t.w, beta);
        }
        d[ai] = lb >= 0 ? s_cls * osr_bce_with_logits_grad(logits[pi], (float)lb) : 0.f;
        // (row stride 5A floats: not 16-byte aligned for A = 3)
        d[A + 4 * ai] = g[0]; d[A + 4 * ai + 1] = g[1]; d[A + 4 * ai + 2] = g[2]; d[A + 4 * ai + 3] = g[3];
    }
}

extern "C" osr_status osr_std_rpn_losses_bwd(const osr_rpn_levels* lvl, const float* cell_anchors, int32_t n, const float* pred_logits,
                                             const float* pred_deltas, const int8_t* labels, const float* matched_boxes, const float b2b_weights[4],
                                             float smooth_l1_beta, float cls_weight, float loc_weight, int32_t batch_size_per_image, float loss_scale,
                                             float* d_rows, void* stream) {
    OsrLossLevels lv;
    const char* bad = std_rpn_check(lvl, &lv, cell_anchors, pred_logits, pred_deltas, labels, matched_boxes, b2b_weights, n, batch_size_per_image,
                                    smooth_l1_beta);
    OSR_REQUIRE(!bad, OSR_ERR_INVALID_ARG, "osr_std_rpn_losses_bwd: %s", bad ? bad : "");
    OSR_REQUIRE(d_rows, OSR_ERR_INVALID_ARG, "osr_std_rpn_losses_bwd: null pointer");
    const float norm = (float)batch_size_per_image * (float)n;
    const long long total = (long long)n * lv.R;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(std_rpn_losses_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, lv, cell_anchors, n, pred_logits, pred_deltas,
                       (const signed char*)labels, matched_boxes, make_float4(b2b_weights[0], b2b_weights[1], b2b_weights[2], b2b_weights[3]),
                       smooth_l1_beta, loss_scale * cls_weight / norm, loss_scale * loc_weight / norm, d_rows);
    OSR_CHECK_LAUNCH("osr_std_rpn_losses_bwd");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// [d2] FastRCNNOutputLayers.losses, forward:
// {loss_cls, loss_box_reg, rows, correct, foreground, foreground correct, foreground predicted as background}
// ------------------------------------------------------------------------------------------------------
struct StdRoi {
    const float* logits; const float* deltas; int delta_stride; int agnostic;
    const float* prop; const float* gtb; const long long* cls;
    long long m; int K; float wx, wy, ww, wh, beta;
};

__device__ __forceinline__ int std_roi_target(const StdRoi& p, long long i) {
    const long long c = p.cls[i];
    return c < 0 || c > p.K ? -1 : (int)c;
}

__device__ __forceinline__ const float* std_roi_delta(const StdRoi& p, long long i, int c) {
    return p.deltas + i * p.delta_stride + (p.agnostic ? 0 : 4 * c);
}

__global__ __launch_bounds__(256) void fastrcnn_losses_kernel(StdRoi p, float* __restrict__ partial) {
    float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // ce, box, rows, correct, fg, fg correct, fg as background
    const int nc = p.K + 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.m; i += (long long)gridDim.x * blockDim.x) {
        const int c = std_roi_target(p, i);
        if (c < 0) continue;
        const float* lg = p.logits + i * nc;
        float mx = lg[0];
        int arg = 0;
        for (int j = 1; j < nc; ++j)
            if (lg[j] > mx) { mx = lg[j]; arg = j; }  // (first maximum, as torch.argmax; not osr_softmax_row's fmaxf: they differ on a NaN logit)
        const float sum = osr_softmax_sum(lg, nc, mx);
        v[0] += logf(sum) + mx - lg[c];
        v[2] += 1.f;
        v[3] += arg == c ? 1.f : 0.f;
        if (c == p.K) continue;
        v[4] += 1.f;
        v[5] += arg == c ? 1.f : 0.f;
        v[6] += arg == p.K ? 1.f : 0.f;
        const float4 t = osr_b2b_get_deltas(*reinterpret_cast<const float4*>(p.prop + i * 4), *reinterpret_cast<const float4*>(p.gtb + i * 4), p.wx, p.wy, p.ww, p.wh);
        const float* d = std_roi_delta(p, i, c);
        v[1] += osr_smooth_l1(d[0] - t.x, p.beta) + osr_smooth_l1(d[1] - t.y, p.beta) + osr_smooth_l1(d[2] - t.z, p.beta) + osr_smooth_l1(d[3] - t.w, p.beta);
    }
    osr_loss_block_reduce_store<7>(v, partial);
}

static const char* std_roi_fill(StdRoi* p, const float* logits, const float* deltas, int32_t delta_stride, int32_t agnostic, const float* prop,
                                const float* gtb, const int64_t* cls, int64_t m, int32_t K, const float* rw, float beta) {
    // (an empty batch, m = 0, may come with null data pointers -- torch's empty tensors: no row is read)
    if ((m > 0 && (!logits || !deltas || !prop || !gtb || !cls)) || !rw) return "null pointer";
    if (m < 0 || K < 1 || !(beta >= 0.f)) return "bad m / num_classes / beta";
    if (delta_stride < (agnostic ? 4 : 4 * K)) return "delta_stride below 4 (class-agnostic) / 4K (class-specific)";
    if ((((uintptr_t)prop | (uintptr_t)gtb) & 15) != 0) return "box arrays must be 16-byte aligned";
    *p = StdRoi{logits, deltas, delta_stride, agnostic ? 1 : 0, prop, gtb, (const long long*)cls, (long long)m, K, rw[0], rw[1], rw[2], rw[3], beta};
    return nullptr;
}

extern "C" osr_status osr_fastrcnn_losses_fwd(const float* logits, const float* pred_deltas, int32_t delta_stride, int32_t cls_agnostic,
                                              const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_classes, int64_t m,
                                              int32_t num_classes, const float reg_weights[4], float smooth_l1_beta, float cls_weight,
                                              float box_weight, float* out7, void* workspace, int64_t workspace_bytes, void* stream) {
    StdRoi p;
    const char* bad = std_roi_fill(&p, logits, pred_deltas, delta_stride, cls_agnostic, proposal_boxes, gt_boxes, gt_classes, m, num_classes, reg_weights,
                                   smooth_l1_beta);
    OSR_REQUIRE(!bad, OSR_ERR_INVALID_ARG, "osr_fastrcnn_losses_fwd: %s", bad ? bad : "");
    OSR_REQUIRE(out7 && workspace, OSR_ERR_INVALID_ARG, "osr_fastrcnn_losses_fwd: null pointer");
    OSR_REQUIRE(workspace_bytes >= (int64_t)OSR_LOSS_RED_BLOCKS * 7 * 4, OSR_ERR_WORKSPACE, "osr_fastrcnn_losses_fwd: workspace needs %d bytes", OSR_LOSS_RED_BLOCKS * 28);
    hipStream_t st = (hipStream_t)stream;
    const OsrLossScale scale = {{cls_weight, box_weight, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f}};
    hipLaunchKernelGGL(fastrcnn_losses_kernel, dim3(OSR_LOSS_RED_BLOCKS), dim3(256), 0, st, p, (float*)workspace);
    OSR_CHECK_LAUNCH("osr_fastrcnn_losses_fwd");
    hipLaunchKernelGGL(osr_loss_final_reduce, dim3(1), dim3(64), 0, st, (const float*)workspace, OSR_LOSS_RED_BLOCKS, 7, scale, 2, out7);
    OSR_CHECK_LAUNCH("osr_fastrcnn_losses_fwd(final)");
    return OSR_OK;
}

// rows that count (class in 0..K) for osr_loss_count_rows_kernel: the backward's normaliser is the forward's
struct StdRoiHasTarget {
    StdRoi p;
    __device__ bool operator()(long long i) const { return std_roi_target(p, i) >= 0; }
};

__global__ __launch_bounds__(256) void fastrcnn_losses_bwd_kernel(StdRoi p, float s_cls, float s_box, const float* __restrict__ count,
                                                                  float* __restrict__ d_logits, float* __restrict__ d_deltas) {
    const float inv = 1.0f / fmaxf(count[0], 1.0f);
    const int nc = p.K + 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.m; i += (long long)gridDim.x * blockDim.x) {
        const int c = std_roi_target(p, i);
        float* dl = d_logits + i * nc;
        float* dd = d_deltas + i * p.delta_stride;
        for (int j = 0; j < p.delta_stride; ++j) dd[j] = 0.f;
        if (c < 0) {
            for (int j = 0; j < nc; ++j) dl[j] = 0.f;
            continue;
        }
        const float* lg = p.logits + i * nc;
        float sum;
        const float mx = osr_softmax_row(lg, nc, &sum);
        for (int j = 0; j < nc; ++j) dl[j] = (expf(lg[j] - mx) / sum - (j == c ? 1.f : 0.f)) * s_cls * inv;
        if (c == p.K) continue;
        const float4 t = osr_b2b_get_deltas(*reinterpret_cast<const float4*>(p.prop + i * 4), *reinterpret_cast<const float4*>(p.gtb + i * 4), p.wx, p.wy, p.ww, p.wh);
        const float* d = std_roi_delta(p, i, c);
        float* g = dd + (p.agnostic ? 0 : 4 * c);
        g[0] = s_box * inv * osr_smooth_l1_grad(d[0] - t.x, p.beta); g[1] = s_box * inv * osr_smooth_l1_grad(d[1] - t.y, p.beta);
        g[2] = s_box * inv * osr_smooth_l1_grad(d[2] - t.z, p.beta); g[3] = s_box * inv * osr_smooth_l1_grad(d[3] - t.w, p.beta);
    }
}

extern "C" osr_status osr_fastrcnn_losses_bwd(const float* logits, const float* pred_deltas, int32_t delta_stride, int32_t cls_agnostic,
                                              const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_classes, int64_t m,
                                              int32_t num_classes, const float reg_weights[4], float smooth_l1_beta, float cls_weight,
                                              float box_weight, float loss_scale, float* d_logits, float* d_deltas, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
    StdRoi p;
    const char* bad = std_roi_fill(&p, logits, pred_deltas, delta_stride, cls_agnostic, proposal_boxes, gt_boxes, gt_classes, m, num_classes, reg_weights,
                                   smooth_l1_beta);
    OSR_REQUIRE(!bad, OSR_ERR_INVALID_ARG, "osr_fastrcnn_losses_bwd: %s", bad ? bad : "");
    OSR_REQUIRE((m == 0 || (d_logits && d_deltas)) && workspace, OSR_ERR_INVALID_ARG, "osr_fastrcnn_losses_bwd: null pointer");
    OSR_REQUIRE(workspace_bytes >= 16, OSR_ERR_WORKSPACE, "osr_fastrcnn_losses_bwd: workspace needs 16 bytes");
    if (m == 0) return OSR_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(osr_loss_count_rows_kernel<StdRoiHasTarget>, dim3(1), dim3(256), 0, st, StdRoiHasTarget{p}, p.m, (float*)workspace);
    OSR_CHECK_LAUNCH("osr_fastrcnn_losses_bwd(count)");
    const unsigned blocks = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(fastrcnn_losses_bwd_kernel, dim3(blocks), dim3(256), 0, st, p, loss_scale * cls_weight, loss_scale * box_weight,
                       (const float*)workspace, d_logits, d_deltas);
    OSR_CHECK_LAUNCH("osr_fastrcnn_losses_bwd");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------
// StandardRPNHead tail backward: o = t . W^T + b with W = [W_obj (A,256); W_delta (4A,256)] (the 5A output columns of d_rows).
// dt = (d . W) masked by t > 0 (the 3x3 conv's ReLU), dW = d^T . t, db = column sums of d. One wave per row, 4 channels per lane;
// per-wave partials reduced in a fixed order.
// ------------------------------------------------------------------------------------------------------
#define STDT_BLOCKS 64
#define STDT_MAXQ 40
#define STDT_PSTRIDE (STDT_MAXQ * 256 + 64)

// Q = 5A output columns, a compile-time constant: the wave's dW (Q x 4 channels per lane) stays in registers, lane q < Q carries
// column q's bias sum. Each wave writes its partial once, at the end.
template <class TO, int Q>
__global__ __launch_bounds__(256) void std_tail_bwd_kernel(const float* __restrict__ t, long long T, const float* __restrict__ w,
                                                           const float* __restrict__ d, TO* __restrict__ dt, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    float dw[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) dw[q][0] = dw[q][1] = dw[q][2] = dw[q][3] = 0.f;
    float db = 0.f;
    for (long long r = gw; r < T; r += nw) {
        const float4 tv = *reinterpret_cast<const float4*>(t + r * 256 + lane * 4);
        const float gl = lane < Q ? d[r * Q + lane] : 0.f;
        db += gl;
        float du[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float g = __shfl(gl, q, 64);
            const float4 wq = *reinterpret_cast<const float4*>(w + q * 256 + lane * 4);
            du[0] += g * wq.x; du[1] += g * wq.y; du[2] += g * wq.z; du[3] += g * wq.w;
            dw[q][0] += g * tv.x; dw[q][1] += g * tv.y; dw[q][2] += g * tv.z; dw[q][3] += g * tv.w;
        }
        TO* o = dt + r * 256 + lane * 4;
        o[0] = osr_from_float<TO>(tv.x > 0.f ? du[0] : 0.f); o[1] = osr_from_float<TO>(tv.y > 0.f ? du[1] : 0.f);
        o[2] = osr_from_float<TO>(tv.z > 0.f ? du[2] : 0.f); o[3] = osr_from_float<TO>(tv.w > 0.f ? du[3] : 0.f);
    }
    float* pw = partial + (long long)gw * STDT_PSTRIDE;
#pragma unroll
    for (int q = 0; q < Q; ++q) *reinterpret_cast<float4*>(pw + q * 256 + lane * 4) = make_float4(dw[q][0], dw[q][1], dw[q][2], dw[q][3]);
    if (lane < Q) pw[STDT_MAXQ * 256 + lane] = db;
}

// one thread per output element, partials summed in wave order: deterministic
__global__ __launch_bounds__(256) void std_tail_bwd_reduce(const float* __restrict__ partial, int nparts, int Q, float* __restrict__ dw, float* __restrict__ db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q * 257) return;
    const long long col = i < Q * 256 ? i : (long long)STDT_MAXQ * 256 + (i - Q * 256);
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += partial[(long long)p * STDT_PSTRIDE + col];
    if (i < Q * 256) dw[i] = s;
    else db[i - Q * 256] = s;
}

template <class TO>
static void std_tail_launch(int width, hipStream_t st, const float* t, long long rows, const float* w, const float* d, void* dt, float* ws) {
    const dim3 g(STDT_BLOCKS), b(256);
    TO* o = (TO*)dt;
    switch (width) {
        case 5: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 5>), g, b, 0, st, t, rows, w, d, o, ws); break;
        case 10: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 10>), g, b, 0, st, t, rows, w, d, o, ws); break;
        case 15: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 15>), g, b, 0, st, t, rows, w, d, o, ws); break;
        case 20: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 20>), g, b, 0, st, t, rows, w, d, o, ws); break;
        case 25: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 25>), g, b, 0, st, t, rows, w, d, o, ws); break;
        case 30: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 30>), g, b, 0, st, t, rows, w, d, o, ws); break;
        case 35: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 35>), g, b, 0, st, t, rows, w, d, o, ws); break;
        default: hipLaunchKernelGGL((std_tail_bwd_kernel<TO, 40>), g, b, 0, st, t, rows, w, d, o, ws); break;
    }
}

extern "C" int64_t osr_std_rpn_tail_bwd_workspace_bytes(void) { return (int64_t)STDT_BLOCKS * 4 * STDT_PSTRIDE * 4; }

extern "C" osr_status osr_std_rpn_tail_bwd(const float* t, int64_t rows, const float* w_tail, int32_t width, const float* d_rows, void* dt, int32_t dt_dtype,
                                           float* dw_tail, float* db_tail, void* workspace, int64_t workspace_bytes, void* stream) {
    OSR_REQUIRE(t && w_tail && d_rows && dt && dw_tail && db_tail && workspace, OSR_ERR_INVALID_ARG, "osr_std_rpn_tail_bwd: null pointer");
    OSR_REQUIRE(rows >= 1 && width >= 5 && width <= STDT_MAXQ && width % 5 == 0, OSR_ERR_INVALID_ARG,
                "osr_std_rpn_tail_bwd: bad rows / width (5A, A = 1..8)");
    OSR_REQUIRE(dt_dtype == OSR_F16 || dt_dtype == OSR_BF16, OSR_ERR_UNSUPPORTED, "osr_std_rpn_tail_bwd: dt must be fp16 / bf16");
    OSR_REQUIRE((((uintptr_t)t | (uintptr_t)w_tail) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_std_rpn_tail_bwd: t and w_tail must be 16-byte aligned");
    OSR_REQUIRE(workspace_bytes >= osr_std_rpn_tail_bwd_workspace_bytes(), OSR_ERR_WORKSPACE, "osr_std_rpn_tail_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (dt_dtype == OSR_F16) std_tail_launch<f16_t>(width, st, t, (long long)rows, w_tail, d_rows, dt, (float*)workspace);
    else std_tail_launch<bf16_t>(width, st, t, (long long)rows, w_tail, d_rows, dt, (float*)workspace);
    OSR_CHECK_LAUNCH("osr_std_rpn_tail_bwd");
    hipLaunchKernelGGL(std_tail_bwd_reduce, dim3((width * 257 + 255) / 256), dim3(256), 0, st, (const float*)workspace, STDT_BLOCKS * 4, width, dw_tail, db_tail);
    OSR_CHECK_LAUNCH("osr_std_rpn_tail_bwd(reduce)");
    return OSR_OK;
}
