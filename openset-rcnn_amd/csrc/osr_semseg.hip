// The elementwise and resampling kernels of [d2] SemSegFPNHead at test time for gfx950 (include/osr.h: osr_group_norm_stats,
// osr_gn_relu_merge, osr_semseg_resample). All three are memory bound: NHWC rows are read and written as 8-channel vectors (16 bytes
// in fp16 / bf16), arithmetic is fp32, there are no floating-point atomics and every sum has a fixed order, so repeats are bit-identical.
//
// osr_group_norm_stats: GroupNorm(32) statistics of (n, h, w, c), c in {64, 128, 256}: a group is c / 32 consecutive channels of every
// pixel, so an 8-channel vector holds 1, 2 or 4 whole groups. Pass 1, one workgroup per (chunk of GN_CHUNK pixels, image): a thread
// walks the pixels of its vector slot, sums (x - K) and (x - K)^2 per group with K = the first value it meets (the shift keeps the
// difference of squares away from cancellation whatever mean / std is), turns them into (count, mean, M2), and 32 threads merge the
// threads' triples in thread order with Chan's formula; the chunk's 32 triples go to the workspace. Pass 2, one workgroup per image:
// thread g merges group g's chunk triples in chunk order and writes mean and 1 / sqrt(M2 / count + eps).
//
// osr_gn_relu_merge: out = sum_t up_t(relu(gn_t(x_t))) over up to four terms, the sum in fp32 in term order, rounded once.
// A thread owns one 8-channel vector slot and walks pixels; a workgroup forms the per-channel mean, rstd * gamma and beta of its image
// once, in LDS, and walks several chunks of pixels with them.
//
// osr_semseg_resample: [d2]'s F.interpolate(x4) -> crop -> F.interpolate(output size) composed per output pixel. The two second-stage
// rows y0, y0 + 1 of the x4 map read the stride-4 rows a, a + 1, a + 2 at most (a = first-stage floor of y0), so a pixel is a
// 3 x 3 weighted sum of stride-4 logits per class; the x4 map is never formed. One thread per output pixel; a wave is 64 pixels of
// one output row, combines the rows once per stride-4 column into LDS and then the columns per pixel (semseg_resample_kernel). Label
// mode keeps a running argmax (strict >, so the lowest class wins a tie and NaN never wins), value mode writes the C planes (lanes
// of a wave write consecutive x: coalesced).
#include "osr_common.h"

#define GN_GROUPS 32
#define GN_THREADS 256
#define GN_CHUNK 1024  // pixels per pass-1 workgroup

struct Vec8 {
    float v[8];
};

template <class T> __device__ __forceinline__ Vec8 load8(const T* p);
template <> __device__ __forceinline__ Vec8 load8<float>(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    return Vec8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
template <> __device__ __forceinline__ Vec8 load8<f16_t>(const f16_t* p) {
    union { uint4 u; f16_t h[8]; } r;
    r.u = *reinterpret_cast<const uint4*>(p);
    Vec8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = (float)r.h[j];
    return o;
}
template <> __device__ __forceinline__ Vec8 load8<bf16_t>(const bf16_t* p) {
    union { uint4 u; bf16_t h[8]; } r;
    r.u = *reinterpret_cast<const uint4*>(p);
    Vec8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.v[j] = (float)r.h[j];
    return o;
}

template <class T> __device__ __forceinline__ void store8(T* p, const Vec8& o);
template <> __device__ __forceinline__ void store8<float>(float* p, const Vec8& o) {
    *reinterpret_cast<float4*>(p) = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(o.v[4], o.v[5], o.v[6], o.v[7]);
}
template <> __device__ __forceinline__ void store8<f16_t>(f16_t* p, const Vec8& o) {
    union { uint4 u; f16_t h[8]; } r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.h[j] = (f16_t)o.v[j];
    *reinterpret_cast<uint4*>(p) = r.u;
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const Vec8& o) {
    union { uint4 u; bf16_t h[8]; } r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.h[j] = (bf16_t)o.v[j];
    *reinterpret_cast<uint4*>(p) = r.u;
}

// (count, mean, M2) of b merged into a: Chan, Golub, LeVeque
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& sa, float nb, float mb, float sb) {
    if (nb == 0.f) return;
    if (na == 0.f) {
        na = nb, ma = mb, sa = sb;
        return;
    }
    const float n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    sa += sb + d * d * (na * (nb / n));
    na = n;
}

// ------------------------------------------------------------------------------------------------------------------------------
// GroupNorm statistics
// ------------------------------------------------------------------------------------------------------------------------------
// partials: (n, chunks, 32, 3) fp32 triples
template <class T, int CPG>
__global__ __launch_bounds__(GN_THREADS) void gn_partials_kernel(const T* __restrict__ x, int64_t pixels, int c, int chunks, float* __restrict__ partials) {
    constexpr int GPV = 8 / CPG;  // groups per 8-channel vector
    __shared__ float sh[GN_THREADS * GPV * 3];
    const int img = blockIdx.y, chunk = blockIdx.x;
    const int V = c >> 3, lanes = GN_THREADS / V;  // vector slots per pixel; pixels in flight per workgroup
    const int slot = threadIdx.x % V, pl = threadIdx.x / V;
    const int64_t p0 = (int64_t)chunk * GN_CHUNK, p1 = p0 + GN_CHUNK < pixels ? p0 + GN_CHUNK : pixels;
    const T* base = x + ((int64_t)img * pixels) * c + slot * 8;
    float s1[GPV], s2[GPV], shift[GPV];
    int cnt = 0;
#pragma unroll
    for (int g = 0; g < GPV; ++g) s1[g] = s2[g] = shift[g] = 0.f;
    for (int64_t p = p0 + pl; p < p1; p += lanes) {
        const Vec8 v = load8<T>(base + p * c);
        if (cnt == 0) {
#pragma unroll
            for (int g = 0; g < GPV; ++g) shift[g] = v.v[g * CPG];
        }
#pragma unroll
        for (int g = 0; g < GPV; ++g)
#pragma unroll
            for (int j = 0; j < CPG; ++j) {
                const float d = v.v[g * CPG + j] - shift[g];
                s1[g] += d;
                s2[g] += d * d;
            }
        ++cnt;
    }
#pragma unroll
    for (int g = 0; g < GPV; ++g) {
        const float nn = (float)(cnt * CPG);
        const float dm = cnt ? s1[g] / nn : 0.f;
        float* o = sh + (threadIdx.x * GPV + g) * 3;
        o[0] = nn;
        o[1] = shift[g] + dm;
        o[2] = cnt ? fmaxf(s2[g] - s1[g] * dm, 0.f) : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < GN_GROUPS) {
        const int g = threadIdx.x, vs = g / GPV, gi = g % GPV;  // group g lives in vector slot vs, sub-group gi
        float na = 0.f, ma = 0.f, sa = 0.f;
        for (int l = 0; l < lanes; ++l) {
            const float* o = sh + ((l * V + vs) * GPV + gi) * 3;
            chan_merge(na, ma, sa, o[0], o[1], o[2]);
        }
        float* dst = partials + (((int64_t)img * chunks + chunk) * GN_GROUPS + g) * 3;
        dst[0] = na, dst[1] = ma, dst[2] = sa;
    }
}

__global__ __launch_bounds__(64) void gn_finalize_kernel(const float* __restrict__ partials, int chunks, float eps, float* __restrict__ mean,
                                                         float* __restrict__ rstd) {
    const int img = blockIdx.x, g = threadIdx.x;
    if (g >= GN_GROUPS) return;
    float na = 0.f, ma = 0.f, sa = 0.f;
    for (int ch = 0; ch < chunks; ++ch) {
        const float* o = partials + (((int64_t)img * chunks + ch) * GN_GROUPS + g) * 3;
        chan_merge(na, ma, sa, o[0], o[1], o[2]);
    }
    mean[img * GN_GROUPS + g] = ma;
    rstd[img * GN_GROUPS + g] = 1.0f / sqrtf(sa / na + eps);
}

static inline int gn_chunks(int64_t pixels) { return (int)((pixels + GN_CHUNK - 1) / GN_CHUNK); }

static bool gn_shape_ok(int32_t n, int32_t h, int32_t w, int32_t c) {
    return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (c == 64 || c == 128 || c == 256) && (int64_t)h * w <= (1LL << 30);
}

extern "C" int64_t osr_group_norm_stats_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
    if (!gn_shape_ok(n, h, w, c)) {
        osr_set_error("osr_group_norm_stats: n %d h %d w %d c %d (c must be 64, 128 or 256: 32 groups of 2, 4 or 8 channels)", n, h, w, c);
        return OSR_ERR_INVALID_ARG;
    }
    return (int64_t)n * gn_chunks((int64_t)h * w) * GN_GROUPS * 3 * (int64_t)sizeof(float);
}

template <class T>
static void gn_partials_launch(const void* x, int64_t pixels, int c, int chunks, int n, float* partials, hipStream_t st) {
    const dim3 grid(chunks, n);
    switch (c / GN_GROUPS) {
        case 2: hipLaunchKernelGGL((gn_partials_kernel<T, 2>), grid, dim3(GN_THREADS), 0, st, (const T*)x, pixels, c, chunks, partials); break;
        case 4: hipLaunchKernelGGL((gn_partials_kernel<T, 4>), grid, dim3(GN_THREADS), 0, st, (const T*)x, pixels, c, chunks, partials); break;
        default: hipLaunchKernelGGL((gn_partials_kernel<T, 8>), grid, dim3(GN_THREADS), 0, st, (const T*)x, pixels, c, chunks, partials); break;
    }
}

extern "C" osr_status osr_group_norm_stats(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, float eps, float* mean,
                                           float* rstd, void* workspace, int64_t workspace_bytes, void* stream) {
    OSR_REQUIRE(x && mean && rstd && workspace, OSR_ERR_INVALID_ARG, "osr_group_norm_stats: null pointer");
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_group_norm_stats: bad dtype %d", dtype);
    const int64_t need = osr_group_norm_stats_workspace_bytes(n, h, w, c);
    if (need < 0) return (osr_status)need;
    OSR_REQUIRE(workspace_bytes >= need, OSR_ERR_INVALID_ARG, "osr_group_norm_stats: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    OSR_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)workspace & 3) == 0, OSR_ERR_UNSUPPORTED, "osr_group_norm_stats: x must be 16-byte aligned");
    OSR_REQUIRE(eps > 0.f, OSR_ERR_INVALID_ARG, "osr_group_norm_stats: eps must be positive");
    const int64_t pixels = (int64_t)h * w;
    const int chunks = gn_chunks(pixels);
    hipStream_t st = (hipStream_t)stream;
    float* partials = (float*)workspace;
    switch (dtype) {
        case OSR_F32: gn_partials_launch<float>(x, pixels, c, chunks, n, partials, st); break;
        case OSR_F16: gn_partials_launch<f16_t>(x, pixels, c, chunks, n, partials, st); break;
        default: gn_partials_launch<bf16_t>(x, pixels, c, chunks, n, partials, st); break;
    }
    OSR_CHECK_LAUNCH("osr_group_norm_stats (partials)");
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(n), dim3(64), 0, st, partials, chunks, eps, mean, rstd);
    OSR_CHECK_LAUNCH("osr_group_norm_stats (finalize)");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// GroupNorm + ReLU (+ bilinear x2) of up to four terms, summed
// ------------------------------------------------------------------------------------------------------------------------------
struct MergeArgs {
    osr_gn_term t[OSR_GN_MAX_TERMS];
    int nterms, n, ho, wo, c;
};

#define GM_THREADS 256
#define GM_ITERS 4    // pixels per thread and chunk
#define GM_CHUNKS 8   // chunks per workgroup: the per-channel parameters are formed once per workgroup

template <class T>
__global__ __launch_bounds__(GM_THREADS) void gn_relu_merge_kernel(const MergeArgs a, T* __restrict__ out) {
    // per term and channel: mean, rstd * gamma, beta of this workgroup's image (a term without statistics: 0, 1, 0)
    __shared__ __attribute__((aligned(16))) float prm[OSR_GN_MAX_TERMS][3][256];
    const int img = blockIdx.y, c = a.c;
    const int V = c >> 3, lanes = GM_THREADS / V;
    const int slot = threadIdx.x % V, pl = threadIdx.x / V, ch0 = slot * 8;
    const int cpg = c / GN_GROUPS;
    for (int i = threadIdx.x; i < a.nterms * c; i += GM_THREADS) {
        const int ti = i / c, ch = i - ti * c;
        const osr_gn_term& t = a.t[ti];
        float mu = 0.f, sc = 1.f, be = 0.f;
        if (t.mean != nullptr) {
            const int g = ch / cpg;
            mu = t.mean[img * GN_GROUPS + g];
            sc = t.rstd[img * GN_GROUPS + g] * t.gamma[ch];
            be = t.beta[ch];
        }
        prm[ti][0][ch] = mu, prm[ti][1][ch] = sc, prm[ti][2][ch] = be;
    }
    __syncthreads();
    const int64_t pixels = (int64_t)a.ho * a.wo;
    T* o = out + (int64_t)img * pixels * c + ch0;
    for (int chunk = 0; chunk < GM_CHUNKS; ++chunk) {
        const int64_t pbase = ((int64_t)blockIdx.x * GM_CHUNKS + chunk) * lanes * GM_ITERS;
        if (pbase >= pixels) break;
        Vec8 acc[GM_ITERS];
#pragma unroll
        for (int it = 0; it < GM_ITERS; ++it)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[it].v[j] = 0.f;
        for (int ti = 0; ti < a.nterms; ++ti) {
            const osr_gn_term& t = a.t[ti];
            float mu[8], sc[8], be[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) mu[j] = prm[ti][0][ch0 + j], sc[j] = prm[ti][1][ch0 + j], be[j] = prm[ti][2][ch0 + j];
            const T* x = (const T*)t.x + (int64_t)img * t.h * t.w * c + ch0;
#pragma unroll
            for (int it = 0; it < GM_ITERS; ++it) {
                const int64_t p = pbase + (int64_t)it * lanes + pl;
                if (p >= pixels) continue;
                const int y = (int)(p / a.wo), xo = (int)(p % a.wo);
                if (!t.up2) {
                    const Vec8 v = load8<T>(x + ((int64_t)y * t.w + xo) * c);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[it].v[j] += fmaxf((v.v[j] - mu[j]) * sc[j] + be[j], 0.f);
                } else {
                    // torch upsample_bilinear2d, scale 1/2, align_corners=False: src = max(0, (dst + 0.5) / 2 - 0.5)
                    const float sy = fmaxf(0.5f * ((float)y + 0.5f) - 0.5f, 0.f), sx = fmaxf(0.5f * ((float)xo + 0.5f) - 0.5f, 0.f);
                    const int y0 = (int)sy, x0 = (int)sx;
                    const int y1 = y0 + 1 < t.h ? y0 + 1 : t.h - 1, x1 = x0 + 1 < t.w ? x0 + 1 : t.w - 1;
                    const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
                    const Vec8 v00 = load8<T>(x + ((int64_t)y0 * t.w + x0) * c), v01 = load8<T>(x + ((int64_t)y0 * t.w + x1) * c);
                    const Vec8 v10 = load8<T>(x + ((int64_t)y1 * t.w + x0) * c), v11 = load8<T>(x + ((int64_t)y1 * t.w + x1) * c);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float r00 = fmaxf((v00.v[j] - mu[j]) * sc[j] + be[j], 0.f), r01 = fmaxf((v01.v[j] - mu[j]) * sc[j] + be[j], 0.f);
                        const float r10 = fmaxf((v10.v[j] - mu[j]) * sc[j] + be[j], 0.f), r11 = fmaxf((v11.v[j] - mu[j]) * sc[j] + be[j], 0.f);
                        acc[it].v[j] += ly0 * (lx0 * r00 + lx1 * r01) + ly1 * (lx0 * r10 + lx1 * r11);
                    }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < GM_ITERS; ++it) {
            const int64_t p = pbase + (int64_t)it * lanes + pl;
            if (p < pixels) store8<T>(o + p * c, acc[it]);
        }
    }
}

extern "C" osr_status osr_gn_relu_merge(const osr_gn_term* terms, int32_t num_terms, int32_t dtype, int32_t n, int32_t ho, int32_t wo, int32_t c,
                                        void* out, void* stream) {
    OSR_REQUIRE(terms && out, OSR_ERR_INVALID_ARG, "osr_gn_relu_merge: null pointer");
    OSR_REQUIRE(num_terms >= 1 && num_terms <= OSR_GN_MAX_TERMS, OSR_ERR_INVALID_ARG, "osr_gn_relu_merge: 1 .. %d terms, got %d", OSR_GN_MAX_TERMS, num_terms);
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_gn_relu_merge: bad dtype %d", dtype);
    OSR_REQUIRE(gn_shape_ok(n, ho, wo, c), OSR_ERR_INVALID_ARG, "osr_gn_relu_merge: n %d ho %d wo %d c %d (c must be 64, 128 or 256)", n, ho, wo, c);
    OSR_REQUIRE(((uintptr_t)out & 15) == 0, OSR_ERR_UNSUPPORTED, "osr_gn_relu_merge: out must be 16-byte aligned");
    MergeArgs a;
    a.nterms = num_terms, a.n = n, a.ho = ho, a.wo = wo, a.c = c;
    for (int i = 0; i < num_terms; ++i) {
        const osr_gn_term& t = terms[i];
        OSR_REQUIRE(t.x, OSR_ERR_INVALID_ARG, "osr_gn_relu_merge: term %d has no input", i);
        OSR_REQUIRE(((uintptr_t)t.x & 15) == 0, OSR_ERR_UNSUPPORTED, "osr_gn_relu_merge: term %d's input must be 16-byte aligned", i);
        const int f = t.up2 ? 2 : 1;
        OSR_REQUIRE(t.h >= 1 && t.w >= 1 && t.h * f == ho && t.w * f == wo, OSR_ERR_INVALID_ARG,
                    "osr_gn_relu_merge: term %d is %d x %d%s, the output %d x %d", i, t.h, t.w, t.up2 ? " (up2)" : "", ho, wo);
        const bool all = t.mean && t.rstd && t.gamma && t.beta, none = !t.mean && !t.rstd && !t.gamma && !t.beta;
        OSR_REQUIRE(all || none, OSR_ERR_INVALID_ARG, "osr_gn_relu_merge: term %d needs mean, rstd, gamma and beta together, or none of them", i);
        a.t[i] = t;
    }
    const int lanes = GM_THREADS / (c / 8);
    const int64_t per_block = (int64_t)lanes * GM_ITERS * GM_CHUNKS, blocks = ((int64_t)ho * wo + per_block - 1) / per_block;
    OSR_REQUIRE(blocks <= 2147483647LL, OSR_ERR_UNSUPPORTED, "osr_gn_relu_merge: map too large");
    const dim3 grid((unsigned)blocks, n);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case OSR_F32: hipLaunchKernelGGL(gn_relu_merge_kernel<float>, grid, dim3(GM_THREADS), 0, st, a, (float*)out); break;
        case OSR_F16: hipLaunchKernelGGL(gn_relu_merge_kernel<f16_t>, grid, dim3(GM_THREADS), 0, st, a, (f16_t*)out); break;
        default: hipLaunchKernelGGL(gn_relu_merge_kernel<bf16_t>, grid, dim3(GM_THREADS), 0, st, a, (bf16_t*)out); break;
    }
    OSR_CHECK_LAUNCH("osr_gn_relu_merge");
    return OSR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// x4 bilinear -> crop -> bilinear resize, composed; argmax or planes
// ------------------------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ float4 load4(const T* p);
template <> __device__ __forceinline__ float4 load4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 load4<f16_t>(const f16_t* p) {
    union { uint2 u; f16_t h[4]; } r;
    r.u = *reinterpret_cast<const uint2*>(p);
    return make_float4((float)r.h[0], (float)r.h[1], (float)r.h[2], (float)r.h[3]);
}
template <> __device__ __forceinline__ float4 load4<bf16_t>(const bf16_t* p) {
    union { uint2 u; bf16_t h[4]; } r;
    r.u = *reinterpret_cast<const uint2*>(p);
    return make_float4((float)r.h[0], (float)r.h[1], (float)r.h[2], (float)r.h[3]);
}

// One axis: output index o of `out` over a crop of `in` fine pixels of the x4 map over `coarse` stride-4 cells. -> the first
// coarse index `a` and the weights of a, a + 1, a + 2 (indices clamped to coarse - 1 by the caller; a weight is 0 where unused).
__device__ __forceinline__ void axis_weights(int o, int in, int out, int coarse, int& a, float wgt[3]) {
    const float scale = (float)in / (float)out;
    const float s = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);
    int f0 = (int)s;
    if (f0 > in - 1) f0 = in - 1;  // (cannot happen for finite inputs; keeps the index inside whatever the rounding)
    const int f1 = f0 + 1 < in ? f0 + 1 : in - 1;
    const float l1 = s - (float)f0, l0 = 1.f - l1;
    wgt[0] = wgt[1] = wgt[2] = 0.f;
    a = 0;
    const int fine[2] = {f0, f1};
    const float lam[2] = {l0, l1};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        // first stage, scale 1/4: src = max(0, (f + 0.5) / 4 - 0.5)
        const float q = fmaxf(0.25f * ((float)fine[k] + 0.5f) - 0.5f, 0.f);
        const int c0 = (int)q, c1 = c0 + 1 < coarse ? c0 + 1 : coarse - 1;
        const float m1 = q - (float)c0, m0 = 1.f - m1;
        if (k == 0) a = c0;
        // c0 - a and c1 - a lie in 0 .. 2: f1 <= f0 + 1 moves the first-stage floor by at most one cell
        const int d0 = c0 - a, d1 = c1 - a;
        const float u0 = lam[k] * m0, u1 = lam[k] * m1;
        wgt[0] += (d0 == 0 ? u0 : 0.f) + (d1 == 0 ? u1 : 0.f);
        wgt[1] += (d0 == 1 ? u0 : 0.f) + (d1 == 1 ? u1 : 0.f);
        wgt[2] += (d0 >= 2 ? u0 : 0.f) + (d1 >= 2 ? u1 : 0.f);
    }
}

// The general path: one thread, one output pixel, the 3 x 3 stride-4 taps read from global memory.
template <class T, int MODE>
__device__ __forceinline__ void resample_direct(const T* __restrict__ logits, int h4, int w4, int pitch, int classes, int ra, int ca, const float rw[3],
                                                const float cw[3], int64_t plane, int64_t pix, void* __restrict__ out_) {
    const T* tap[9];
    float wt[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int rr = ra + r < h4 ? ra + r : h4 - 1, cc = ca + c < w4 ? ca + c : w4 - 1;
            wt[r * 3 + c] = rw[r] * cw[c];
            // (a tap of weight zero re-reads tap 0, whose weight is never zero: 0 x its value cannot bring in a foreign Inf / NaN)
            tap[r * 3 + c] = wt[r * 3 + c] != 0.f ? logits + ((int64_t)rr * w4 + cc) * pitch : tap[0];
        }
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < classes; k += 4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float4 v = load4<T>(tap[i] + k);
            s.x += wt[i] * v.x, s.y += wt[i] * v.y, s.z += wt[i] * v.z, s.w += wt[i] * v.w;
        }
        const float e[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k + j >= classes) break;
            if (MODE == 0) {
                if ((k + j == 0) || e[j] > best) best = e[j], arg = k + j;
            } else {
                ((float*)out_)[(int64_t)(k + j) * plane + pix] = e[j];
            }
        }
    }
    if (MODE == 0) ((int32_t*)out_)[pix] = arg;
}

#define RS_CAP 40  // stride-4 columns that the 64 output pixels of a wave may span on the tiled path
#define RS_CH 56   // channels per pass through LDS
#define RS_LD 60   // LDS floats per column: 56 + 4, so that the 16-byte reads of 16 neighbouring columns fall on distinct banks

__device__ __forceinline__ float4 scaled(float w, float4 v) { return make_float4(w * v.x, w * v.y, w * v.z, w * v.w); }
__device__ __forceinline__ float4 madd(float4 a, float w, float4 v) { return make_float4(a.x + w * v.x, a.y + w * v.y, a.z + w * v.z, a.w + w * v.w); }

// A workgroup is 4 waves, a wave 64 consecutive pixels of ONE output row: its row weights are the same in every lane and its columns
// ca .. ca + 2 span few stride-4 columns (19 at scale 1). Tiled path (the span fits RS_CAP): the wave first combines the two or three
// stride-4 rows with the row weights for every column of the span, lanes along the channels (coalesced 16-byte loads, each logit
// read once per wave), into its LDS tile; then every lane combines its three columns from LDS. A wider span (a strong downscale)
// takes resample_direct. Which path a wave takes depends on the shapes only, so repeats are bit-identical.
template <class T, int MODE>
__global__ __launch_bounds__(256) void semseg_resample_kernel(const T* __restrict__ logits, int h4, int w4, int pitch, int classes, int ih, int iw, int oh,
                                                              int ow, void* __restrict__ out_) {
    __shared__ __attribute__((aligned(16))) float tile[4][RS_CAP * RS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ox = blockIdx.x * 64 + lane, oy = blockIdx.y * 4 + wave;
    const bool row_ok = oy < oh, ok = row_ok && ox < ow;
    int ra, ca;
    float rw[3], cw[3];
    axis_weights(row_ok ? oy : oh - 1, ih, oh, h4, ra, rw);
    axis_weights(ox < ow ? ox : ow - 1, iw, ow, w4, ca, cw);  // (lanes past the row's end repeat its last pixel: ca never decreases along the wave)
    const int cmin = __shfl(ca, 0, 64);
    int cmax = __shfl(ca, 63, 64) + 2;
    cmax = cmax < w4 ? cmax : w4 - 1;
    const int ncols = cmax - cmin + 1;
    const bool tiled = ncols <= RS_CAP;  // the same in every lane of the wave
    const int64_t plane = (int64_t)oh * ow, pix = (int64_t)oy * ow + ox;
    if (!tiled && ok) resample_direct<T, MODE>(logits, h4, w4, pitch, classes, ra, ca, rw, cw, plane, pix, out_);
    const T* rows[3];
    int col[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int rr = ra + r < h4 ? ra + r : h4 - 1, cc = ca + r < w4 ? ca + r : w4 - 1;
        rows[r] = logits + ((int64_t)rr * w4 + cmin) * pitch;
        col[r] = (cc - cmin) * RS_LD;  // cmin <= ca <= cc <= cmax
    }
    float* my = tile[wave];
    const int cpad = (classes + 3) & ~3;  // <= pitch: the pitch is a multiple of 4
    float best = 0.f;
    int arg = 0;
    for (int c0 = 0; c0 < cpad; c0 += RS_CH) {
        const int q = (cpad - c0 < RS_CH ? cpad - c0 : RS_CH) >> 2;  // 4-channel groups in this pass
        if (tiled && row_ok) {
            for (int it = lane; it < ncols * q; it += 64) {
                const int cl = it / q, qd = it - cl * q;
                const int64_t off = (int64_t)cl * pitch + c0 + qd * 4;
                float4 v = scaled(rw[0], load4<T>(rows[0] + off));  // (a weight of zero is skipped: 0 x Inf must not appear)
                if (rw[1] != 0.f) v = madd(v, rw[1], load4<T>(rows[1] + off));
                if (rw[2] != 0.f) v = madd(v, rw[2], load4<T>(rows[2] + off));
                *reinterpret_cast<float4*>(my + cl * RS_LD + qd * 4) = v;
            }
        }
        __syncthreads();
        if (tiled && ok) {
            for (int qd = 0; qd < q; ++qd) {
                float4 s = scaled(cw[0], *reinterpret_cast<const float4*>(my + col[0] + qd * 4));
                if (cw[1] != 0.f) s = madd(s, cw[1], *reinterpret_cast<const float4*>(my + col[1] + qd * 4));
                if (cw[2] != 0.f) s = madd(s, cw[2], *reinterpret_cast<const float4*>(my + col[2] + qd * 4));
                const float e[4] = {s.x, s.y, s.z, s.w};
                const int k = c0 + qd * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k + j >= classes) break;
                    if (MODE == 0) {
                        if ((k + j == 0) || e[j] > best) best = e[j], arg = k + j;
                    } else {
                        ((float*)out_)[(int64_t)(k + j) * plane + pix] = e[j];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (MODE == 0 && tiled && ok) ((int32_t*)out_)[pix] = arg;
}

template <class T>
static void semseg_resample_launch(const void* logits, int h4, int w4, int pitch, int classes, int ih, int iw, int oh, int ow, int mode, void* out,
                                   hipStream_t st) {
    const dim3 grid((ow + 63) / 64, (oh + 3) / 4);
    if (mode == 0)
        hipLaunchKernelGGL((semseg_resample_kernel<T, 0>), grid, dim3(256), 0, st, (const T*)logits, h4, w4, pitch, classes, ih, iw, oh, ow, out);
    else
        hipLaunchKernelGGL((semseg_resample_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)logits, h4, w4, pitch, classes, ih, iw, oh, ow, out);
}

extern "C" osr_status osr_semseg_resample(const void* logits, int32_t dtype, int32_t h4, int32_t w4, int32_t pitch, int32_t num_classes, int32_t ih,
                                          int32_t iw, int32_t oh, int32_t ow, int32_t mode, void* out, void* stream) {
    OSR_REQUIRE(logits && out, OSR_ERR_INVALID_ARG, "osr_semseg_resample: null pointer");
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_semseg_resample: bad dtype %d", dtype);
    OSR_REQUIRE(mode == OSR_SEMSEG_LABELS || mode == OSR_SEMSEG_VALUES, OSR_ERR_INVALID_ARG, "osr_semseg_resample: mode %d", mode);
    OSR_REQUIRE(h4 >= 1 && w4 >= 1 && h4 <= 16384 && w4 <= 16384, OSR_ERR_INVALID_ARG, "osr_semseg_resample: stride-4 map %d x %d", h4, w4);
    OSR_REQUIRE(num_classes >= 1 && pitch >= num_classes && pitch % 4 == 0, OSR_ERR_INVALID_ARG,
                "osr_semseg_resample: %d classes in a pitch of %d (the pitch must be a multiple of 4 and hold the classes)", num_classes, pitch);
    OSR_REQUIRE(ih >= 1 && iw >= 1 && ih <= 4 * h4 && iw <= 4 * w4, OSR_ERR_INVALID_ARG, "osr_semseg_resample: crop %d x %d of a %d x %d map", ih, iw,
                4 * h4, 4 * w4);
    OSR_REQUIRE(oh >= 1 && ow >= 1 && oh <= 65535 * 4 && ow <= 65536, OSR_ERR_INVALID_ARG, "osr_semseg_resample: output %d x %d", oh, ow);
    OSR_REQUIRE(((uintptr_t)logits & 15) == 0 && (pitch * osr_dtype_size(dtype)) % 8 == 0, OSR_ERR_UNSUPPORTED,
                "osr_semseg_resample: logits must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case OSR_F32: semseg_resample_launch<float>(logits, h4, w4, pitch, num_classes, ih, iw, oh, ow, mode, out, st); break;
        case OSR_F16: semseg_resample_launch<f16_t>(logits, h4, w4, pitch, num_classes, ih, iw, oh, ow, mode, out, st); break;
        default: semseg_resample_launch<bf16_t>(logits, h4, w4, pitch, num_classes, ih, iw, oh, ow, mode, out, st); break;
    }
    OSR_CHECK_LAUNCH("osr_semseg_resample");
    return OSR_OK;
}
