// The SGD of a training step ([d2] build_optimizer -> torch.optim.SGD.step over every parameter), the library's only one: momentum
// and weight decay on the fp32 masters, the low-precision working copy written in the same pass, and the solver options beyond one
// SGD group -- per-parameter gradient clipping (maybe_add_gradient_clipping, CLIP_TYPE "value" / "norm"), per-group learning-rate
// factor and weight decay (BIAS_LR_FACTOR, WEIGHT_DECAY_BIAS), Nesterov momentum. One launch over the flat fp32 gradient, a second
// in front of it when norm clipping is on:
//   osr_grad_norm_partials  one read of the gradient: per chunk, sum |g*gs*rs|^p (or max |.| for p = inf) into partials[chunk],
//                           and the overflow flag cleared where a gradient is inf / NaN (it replaces osr_check_finite there)
//   osr_sgd_step_multi_ex   the multi-tensor SGD over SEGMENTS (one parameter each: a row range of a master), a table and a chunk
//                           list the caller builds once and keeps on the device: with norm clipping every workgroup first sums
//                           its parameter's partials in a fixed order; then it clips g*gs*rs, adds weight decay and applies
//                           (Nesterov) momentum
// row_scale (nullable, one value per leading-dimension row) is the folded FrozenBN scale of a conv: the master weight is the un-folded
// one, the kernels read w * scale, and the chain rule multiplies the gradient by it.
// No atomics: the partials and their sums are in a fixed order, so repeated steps give identical bits.
#include <cmath>

#include "osr_common.h"

namespace {

enum { NORM_L1 = 0, NORM_L2 = 1, NORM_INF = 2, NORM_P = 3 };

__device__ __forceinline__ int norm_kind(float p) { return p == 1.0f ? NORM_L1 : p == 2.0f ? NORM_L2 : isinf(p) ? NORM_INF : NORM_P; }

// Row of element i of a segment, advanced without a division per element (threads stride by blockDim.x).
struct RowCursor {
    long long r, rem, re;
    __device__ RowCursor(long long i, long long row_elems) : re(row_elems) { r = i / re; rem = i - r * re; }
    __device__ __forceinline__ void advance(int by) {
        rem += by;
        while (rem >= re) { rem -= re; ++r; }
    }
};

__device__ __forceinline__ double block_reduce(double v, bool take_max, double* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = take_max ? fmax(v, o) : v + o;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = take_max ? fmax(t, red[w]) : t + red[w];
    __syncthreads();
    return t;
}

template <int KIND>
__global__ __launch_bounds__(256) void norm_partials_kernel(const osr_sgd_segment* __restrict__ table, const int2* __restrict__ chunks, int chunk_elems,
                                                            float gs, float p, double* __restrict__ partials, int* __restrict__ flag) {
    __shared__ double red[4];
    const int2 c = chunks[blockIdx.x];
    const osr_sgd_segment s = table[c.x];
    const long long i0 = (long long)c.y * chunk_elems, i1 = i0 + chunk_elems < s.n ? i0 + chunk_elems : s.n;
    const float* __restrict__ g = s.grad;
    double acc = 0.0;
    bool bad = false;
    long long i = i0 + threadIdx.x;
    RowCursor rc(i, s.row_scale ? s.row_elems : 1);
    for (; i < i1; i += blockDim.x) {
        const float x = g[i];
        float rs = 1.0f;
        if (s.row_scale) {
            rs = s.row_scale[rc.r];
            rc.advance(blockDim.x);
        }
        bad |= !osr_finite(x);
        const float a = fabsf(x * gs * rs);  // (the product sgd_element forms, in its order)
        if (KIND == NORM_L1) acc += (double)a;
        else if (KIND == NORM_L2) acc += (double)a * (double)a;
        else if (KIND == NORM_INF) acc = fmax(acc, (double)a);
        else acc += (double)powf(a, p);
    }
    if (flag && __any(bad) && (threadIdx.x & 63) == 0) *flag = 0;  // every racing writer stores the same value
    const double t = block_reduce(acc, KIND == NORM_INF, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// [d2] clip_grad_norm_ of one parameter: c = max_norm / (||g||_p + 1e-6) in fp32, applied when c < 1. Returns 1 when it is not.
__device__ float segment_clip_coef(const osr_sgd_segment& s, const double* __restrict__ partials, float clip_value, float p, double* red) {
    const bool take_max = norm_kind(p) == NORM_INF;
    double a = 0.0;
    for (int k = threadIdx.x; k < s.nchunks; k += blockDim.x) a = take_max ? fmax(a, partials[s.chunk0 + k]) : a + partials[s.chunk0 + k];
    const double t = block_reduce(a, take_max, red);
    const int kind = norm_kind(p);
    const double nrm = kind == NORM_L1 || kind == NORM_INF ? t : kind == NORM_L2 ? sqrt(t) : pow(t, 1.0 / (double)p);
    const float c = clip_value / ((float)nrm + 1e-6f);
    return c < 1.0f ? c : 1.0f;
}

// One element of the update. Contraction into fused multiply-adds is off: every product and sum rounds on its own, as the recorded
// results of tests/golden/update_pin_v1.npz do, whatever the compiler would make of the surrounding loop.
__device__ __forceinline__ void sgd_element(float& p, float& v, float g, float rs, float lr, float mu, float wd, float gs, int clip_mode, float cv,
                                               float coef, bool nesterov) {
#pragma clang fp contract(off)
    float d = g * gs * rs;
    if (clip_mode == OSR_CLIP_VALUE) d = fminf(fmaxf(d, -cv), cv);
    else if (clip_mode == OSR_CLIP_NORM && coef < 1.0f) d = d * coef;
    d = d + wd * p;  // torch.optim.SGD adds the weight decay to the (clipped) gradient
    const float vi = mu * v + d;
    if (nesterov) d = d + mu * vi;
    else d = vi;
    p = p - lr * d;
    v = vi;
}

template <class T>
__device__ __forceinline__ void sgd_ex_run(const osr_sgd_segment& s, long long i0, long long i1, float lr, float mu, float gs, int clip_mode, float cv, float coef) {
    float* __restrict__ p = s.param;
    const float* __restrict__ g = s.grad;
    float* __restrict__ v = s.momentum;
    T* __restrict__ lp = reinterpret_cast<T*>(s.lowp);
    const float lr_s = lr * s.lr_factor, wd = s.weight_decay;
    const bool nesterov = s.nesterov != 0;
    long long i = i0 + threadIdx.x;
    RowCursor rc(i, s.row_scale ? s.row_elems : 1);
    for (; i < i1; i += blockDim.x) {
        float rs = 1.0f;
        if (s.row_scale) {
            rs = s.row_scale[rc.r];
            rc.advance(blockDim.x);
        }
        float pi = p[i], vi = v[i];
        sgd_element(pi, vi, g[i], rs, lr_s, mu, wd, gs, clip_mode, cv, coef, nesterov);
        v[i] = vi;
        p[i] = pi;
        if (lp) lp[i] = osr_from_float<T>(pi * rs);
    }
}

__global__ __launch_bounds__(256) void sgd_multi_ex_kernel(const osr_sgd_segment* __restrict__ table, const int2* __restrict__ chunks, int chunk_elems,
                                                           float lr, float mu, float gs, int clip_mode, float cv, float norm_type,
                                                           const double* __restrict__ partials, const int* __restrict__ gate) {
    __shared__ double red[4];
    if (gate && *gate == 0) return;  // this iteration's gradients held an inf / NaN: leave parameters and momentum alone
    const int2 c = chunks[blockIdx.x];
    const osr_sgd_segment s = table[c.x];
    const float coef = clip_mode == OSR_CLIP_NORM ? segment_clip_coef(s, partials, cv, norm_type, red) : 1.0f;
    const long long i0 = (long long)c.y * chunk_elems, i1 = i0 + chunk_elems < s.n ? i0 + chunk_elems : s.n;
    if (!s.lowp || s.lowp_dtype == OSR_F32) sgd_ex_run<float>(s, i0, i1, lr, mu, gs, clip_mode, cv, coef);
    else if (s.lowp_dtype == OSR_F16) sgd_ex_run<f16_t>(s, i0, i1, lr, mu, gs, clip_mode, cv, coef);
    else sgd_ex_run<bf16_t>(s, i0, i1, lr, mu, gs, clip_mode, cv, coef);
}

}  // namespace

extern "C" osr_status osr_grad_norm_partials(const osr_sgd_segment* table, const int32_t* chunks, int32_t num_chunks, int32_t chunk_elems, float grad_scale,
                                             float norm_type, double* partials, int32_t* finite_flag, void* stream) {
    OSR_REQUIRE(table && chunks && partials && num_chunks >= 0 && chunk_elems >= 256, OSR_ERR_INVALID_ARG,
                "osr_grad_norm_partials: null table / partials or bad chunk size");
    OSR_REQUIRE(norm_type > 0.0f, OSR_ERR_INVALID_ARG, "osr_grad_norm_partials: norm_type must be > 0 (inf for the max norm)");
    if (num_chunks == 0) return OSR_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_chunks), block(256);
    const auto c2 = reinterpret_cast<const int2*>(chunks);
    if (norm_type == 1.0f) hipLaunchKernelGGL(norm_partials_kernel<NORM_L1>, grid, block, 0, st, table, c2, chunk_elems, grad_scale, norm_type, partials, finite_flag);
    else if (norm_type == 2.0f) hipLaunchKernelGGL(norm_partials_kernel<NORM_L2>, grid, block, 0, st, table, c2, chunk_elems, grad_scale, norm_type, partials, finite_flag);
    else if (std::isinf(norm_type)) hipLaunchKernelGGL(norm_partials_kernel<NORM_INF>, grid, block, 0, st, table, c2, chunk_elems, grad_scale, norm_type, partials, finite_flag);
    else hipLaunchKernelGGL(norm_partials_kernel<NORM_P>, grid, block, 0, st, table, c2, chunk_elems, grad_scale, norm_type, partials, finite_flag);
    OSR_CHECK_LAUNCH("osr_grad_norm_partials");
    return OSR_OK;
}

extern "C" osr_status osr_sgd_step_multi_ex(const osr_sgd_segment* table, const int32_t* chunks, int32_t num_chunks, int32_t chunk_elems, float lr, float momentum,
                                            float grad_scale, int32_t clip_mode, float clip_value, float norm_type, const double* partials,
                                            const int32_t* apply_flag, void* stream) {
    OSR_REQUIRE(table && chunks && num_chunks >= 0 && chunk_elems >= 256, OSR_ERR_INVALID_ARG, "osr_sgd_step_multi_ex: null table / bad chunk size");
    OSR_REQUIRE(clip_mode == OSR_CLIP_NONE || clip_mode == OSR_CLIP_VALUE || clip_mode == OSR_CLIP_NORM, OSR_ERR_INVALID_ARG,
                "osr_sgd_step_multi_ex: bad clip mode");
    OSR_REQUIRE(clip_mode != OSR_CLIP_NORM || (partials && norm_type > 0.0f), OSR_ERR_INVALID_ARG,
                "osr_sgd_step_multi_ex: norm clipping needs the partials of osr_grad_norm_partials and norm_type > 0");
    if (num_chunks == 0) return OSR_OK;
    hipLaunchKernelGGL(sgd_multi_ex_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<const int2*>(chunks), chunk_elems,
                       lr, momentum, grad_scale, (int)clip_mode, clip_value, norm_type, partials, apply_flag);
    OSR_CHECK_LAUNCH("osr_sgd_step_multi_ex");
    return OSR_OK;
}
