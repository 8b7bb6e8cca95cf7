// Building blocks shared by the loss kernels (csrc/osr_train_fwd.hip, osr_train_bwd.hip, osr_std_train.hip, osr_mask_train.hip):
// the anchor level table, the two-stage fixed-order reduction, the one-workgroup row counter, BCE-with-logits and the softmax row.
// One definition each, so that a fix to an overflow bound, a NaN rule or a summation order reaches every loss.
//
// Header code takes its includer's contraction setting: osr_train_bwd.hip is built with the default FMA contraction, the other three
// with -ffp-contract=off. That is on purpose -- it is what each file's own copy did.
#pragma once
#include "osr_common.h"

// ------------------------------------------------------------------------------------------------------
// anchor level table
// ------------------------------------------------------------------------------------------------------
struct OsrLossLevels {
    int num_levels, num_anchors;
    int h[OSR_MAX_LEVELS], w[OSR_MAX_LEVELS], stride[OSR_MAX_LEVELS];  // (the stock heads' kernels never read h[]: 32 bytes of kernel argument)
    long long pred_off[OSR_MAX_LEVELS];  // element offset of level l in the level-major prediction buffers
    int aoff[OSR_MAX_LEVELS + 1];        // prefix of h*w*a: index base inside an image's concatenated anchor list
    int R;
};

// false: "bad level table" in the caller's own words. At most 2^30 anchors per image (the kernels index them with an int).
// The stock heads add osr_loss_levels_whole_pixels() at their call sites; the CF-RPN entry points take any A >= 1 and any offset.
static bool osr_loss_levels_fill(const osr_rpn_levels* in, OsrLossLevels* o) {
    if (!in || in->num_levels < 1 || in->num_levels > OSR_MAX_LEVELS || in->num_anchors < 1) return false;
    o->num_levels = in->num_levels; o->num_anchors = in->num_anchors;
    long long a = 0;
    for (int l = 0; l < in->num_levels; ++l) {
        if (in->h[l] < 1 || in->w[l] < 1 || in->stride[l] < 1) return false;
        o->h[l] = in->h[l]; o->w[l] = in->w[l]; o->stride[l] = in->stride[l]; o->pred_off[l] = in->offset[l];
        o->aoff[l] = (int)a;
        a += (long long)in->h[l] * in->w[l] * in->num_anchors;
        if (a > (1ll << 30)) return false;
    }
    o->aoff[in->num_levels] = (int)a;
    o->R = (int)a;
    return true;
}

// the stock heads' extra conditions on a table that osr_loss_levels_fill accepted: 1 <= A <= max_anchors, offsets in whole pixels
static bool osr_loss_levels_whole_pixels(const osr_rpn_levels* in, int max_anchors) {
    if (in->num_anchors > max_anchors) return false;
    for (int l = 0; l < in->num_levels; ++l)
        if (in->offset[l] % in->num_anchors != 0) return false;
    return true;
}

// anchor r of an image's list (level, y, x, a -- a minor): the box, its level and its index inside the level
__device__ __forceinline__ float4 osr_loss_anchor(const OsrLossLevels& lv, const float* __restrict__ cell, int r, int* level, int* cell_idx) {
    int l = 0;
    while (l + 1 < lv.num_levels && r >= lv.aoff[l + 1]) ++l;
    const int idx = r - lv.aoff[l], A = lv.num_anchors, a = idx % A, c = idx / A;
    const float sx = (float)(c % lv.w[l]) * (float)lv.stride[l], sy = (float)(c / lv.w[l]) * (float)lv.stride[l];
    const float* ca = cell + ((long long)l * A + a) * 4;
    *level = l; *cell_idx = idx;
    return make_float4(sx + ca[0], sy + ca[1], sx + ca[2], sy + ca[3]);
}

// element index of (image, level, in-level index) in the level-major prediction buffers
__device__ __forceinline__ long long osr_loss_pred_index(const OsrLossLevels& lv, int level, int img, int cell_idx) {
    return lv.pred_off[level] + (long long)img * (lv.aoff[level + 1] - lv.aoff[level]) + cell_idx;
}

// ------------------------------------------------------------------------------------------------------
// deterministic two-stage reduction: per-workgroup partials, then one wave.
// The order is the contract ("bitwise reproducible losses"): a workgroup adds its waves' sums in wave order; the partials of a column
// are added lane-strided (lane l: workgroups l, l + 64, ...) and the 64 lane sums go down a __shfl_down tree. Every accumulator starts
// at +0 and adds never produce -0 from it, so starting a sum at 0.f or at its first element gives the same bits.
// ------------------------------------------------------------------------------------------------------
#define OSR_LOSS_RED_BLOCKS 256  // workgroups of a loss kernel = partials per column
#define OSR_LOSS_MAXV 8          // columns at most

// any workgroup of whole waves, up to 16 of them
template <int NV>
__device__ __forceinline__ void osr_loss_block_reduce_store(float v[NV], float* __restrict__ partial /* [gridDim.x][NV] */) {
    static_assert(NV <= OSR_LOSS_MAXV, "more columns than OsrLossScale holds");
    __shared__ float s_red[OSR_LOSS_MAXV][16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        float x = v[q];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
        if (lane == 0) s_red[q][wid] = x;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        float x = 0.f;
        for (int w = 0; w < nw; ++w) x += s_red[threadIdx.x][w];
        partial[(long long)blockIdx.x * NV + threadIdx.x] = x;
    }
}

// sum_b partial[b][q], in every lane of the (one) wave that calls it. (One thread walking all the workgroups' partials was a 16-30 us
// dependent chain per loss, four times on the training step's critical stream.)
__device__ __forceinline__ float osr_loss_column_sum(const float* __restrict__ partial, int nblocks, int nv, int q) {
    const int lane = threadIdx.x & 63;
    float x = 0.f;
#pragma unroll 4
    for (int b = lane; b < nblocks; b += 64) x += partial[(long long)b * nv + q];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
    return __shfl(x, 0, 64);
}

struct OsrLossScale { float s[OSR_LOSS_MAXV]; };

// out[q] = scale[q] * sum_b partial[b][q]; with norm_col >= 0 every column q < norm_col is also divided by
// max(sum_b partial[b][norm_col], 1) -- the "rows that count" normaliser when the row list is padded.
// (static: the header is included by several translation units. Losses with an output formula of their own -- pln_finish, ce_finish,
// mask_loss_final -- keep their finisher and read their columns through osr_loss_column_sum.)
static __global__ __launch_bounds__(64) void osr_loss_final_reduce(const float* __restrict__ partial, int nblocks, int nv, OsrLossScale scale, int norm_col,
                                                                   float* __restrict__ out) {
    const float c = norm_col >= 0 ? osr_loss_column_sum(partial, nblocks, nv, norm_col) : 1.0f;
    for (int q = 0; q < nv; ++q) {
        float x = osr_loss_column_sum(partial, nblocks, nv, q);
        if (norm_col >= 0 && q < norm_col) x = x / fmaxf(c, 1.0f);
        if (threadIdx.x == 0) out[q] = x * scale.s[q];
    }
}

// ------------------------------------------------------------------------------------------------------
// "rows that count": out[0] = number of rows i < m with counts(i). One workgroup of 256 threads, so that a backward's normaliser is
// its forward's. The predicate is the only thing the losses differ in; what a zero count means (max(count, 1), cnt <= 0) stays with
// the kernel that reads it.
// ------------------------------------------------------------------------------------------------------
template <class RowCounts>
__global__ __launch_bounds__(256) void osr_loss_count_rows_kernel(RowCounts counts, long long m, float* __restrict__ out) {
    __shared__ int s_cnt[256];
    int c = 0;
    for (long long i = threadIdx.x; i < m; i += blockDim.x) c += counts(i) ? 1 : 0;
    s_cnt[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)s_cnt[0];
}

// ------------------------------------------------------------------------------------------------------
// F.binary_cross_entropy_with_logits in its stable form, the stable sigmoid, and the loss's derivative w.r.t. x
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float osr_bce_with_logits(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float osr_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}
__device__ __forceinline__ float osr_bce_with_logits_grad(float x, float y) { return osr_sigmoid(x) - y; }

// ------------------------------------------------------------------------------------------------------
// softmax row: returns the row's maximum, *sum = sum_j exp(lg[j] - max), both in index order.
// The maximum is taken with fmaxf, which skips a NaN logit. [d2] FastRCNNOutputLayers' forward (fastrcnn_losses_kernel) also needs
// the first argmax and keeps its own `lg[j] > mx` loop -- the two differ when a logit is NaN -- and takes only the sum from here.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float osr_softmax_sum(const float* lg, int nc, float mx) {
    float s = 0.f;
    for (int j = 0; j < nc; ++j) s += expf(lg[j] - mx);
    return s;
}
__device__ __forceinline__ float osr_softmax_row(const float* lg, int nc, float* sum) {
    float mx = lg[0];
    for (int j = 1; j < nc; ++j) mx = fmaxf(mx, lg[j]);
    *sum = osr_softmax_sum(lg, nc, mx);
    return mx;
}
