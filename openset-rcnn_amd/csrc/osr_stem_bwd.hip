// Backward of the ResNet stem for training with MODEL.BACKBONE.FREEZE_AT 0: [d2] BasicStem = conv1 (7x7/2, pad 3, 3 -> 64, FrozenBN
// folded) -> ReLU -> max_pool2d(3, 2, 1).
//   osr_stem_pool_bwd   the max pool's and the ReLU's backward in one pass: dS[p][c] = sum of dpool over the (<= 4) windows whose first
//                       maximum (torch's scan: ky then kx, (v > max) || isnan(v)) is p, zero where the stem output S[p][c] <= 0. A
//                       gather (each stem pixel visits its windows in a fixed order): no atomics, repeats are bit-identical.
//   osr_stem_wgrad      dW of the stem view (64, 8, 1, 32) = sum over stem pixels p of dS[p][co] * xpad[patch(p)][k] on the f16 / bf16
//                       MFMA (16x16x32), K = 8 rows x 8 taps x 4 channels. The pixels are split into a fixed number of contiguous ranges
//                       (a function of the pixel count only); each range writes its fp32 partial tile to the workspace and a second
//                       launch sums the partials in range order: no float atomics, bit-identical repeats. The 8th row, the 8th tap
//                       and the 4th channel (they multiply real halo / image pixels in the forward view) are written as exact zeros.
#include "osr_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

template <class T> struct StemMfma;
template <> struct StemMfma<f16_t> {
    typedef f16x8_t frag;
    static __device__ __forceinline__ f32x4_t mfma(frag a, frag b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct StemMfma<bf16_t> {
    typedef bf16x8_t frag;
    static __device__ __forceinline__ f32x4_t mfma(frag a, frag b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

constexpr int kCout = 64;       // stem output channels
constexpr int kK = 256;         // stem view: 8 rows x 8 taps x 4 channels
constexpr int kChunk = 32;      // pixels per MFMA k-step
constexpr int kLdsRow = 40;     // halves per LDS row (32 + 8 pad: 80-byte rows keep the 16-byte fragment reads aligned)
constexpr int kMaxRanges = 512; // pixel ranges of the weight gradient (partials in the workspace)

// One thread per pixel and 8 channels (16-byte loads): the windows' maxima are recomputed from the stem output, each window's 9 values
// read once per visiting pixel (L2 / L1 hits: the pixel's neighbours read the same rows).
template <class T>
__global__ void __launch_bounds__(256) stem_pool_bwd_kernel(const T* __restrict__ s, const T* __restrict__ dpool, T* __restrict__ ds, int n, int hs,
                                                            int ws, int c) {
    const int cg = c >> 3;
    const int64_t total = (int64_t)n * hs * ws * cg;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % cg) * 8;
    int64_t r = i / cg;
    const int x = (int)(r % ws);
    r /= ws;
    const int y = (int)(r % hs);
    const int ni = (int)(r / hs);
    const int64_t pix = ((int64_t)ni * hs + y) * ws + x;
    T sv[8];
    *reinterpret_cast<uint4*>(sv) = *reinterpret_cast<const uint4*>(s + pix * c + ch);
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    const int ho = (hs - 1) / 2 + 1, wo = (ws - 1) / 2 + 1;
    const T* sn = s + (int64_t)ni * hs * ws * c + ch;
    const int py1 = min(ho - 1, (y + 1) >> 1), px1 = min(wo - 1, (x + 1) >> 1);
    const int me = y * ws + x;
    for (int py = y >> 1; py <= py1; ++py) {
        for (int px = x >> 1; px <= px1; ++px) {
            float m[8];
            int am[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { m[k] = -INFINITY; am[k] = -1; }
            for (int ky = max(0, 2 * py - 1); ky <= min(hs - 1, 2 * py + 1); ++ky) {
                for (int kx = max(0, 2 * px - 1); kx <= min(ws - 1, 2 * px + 1); ++kx) {
                    T v8[8];
                    *reinterpret_cast<uint4*>(v8) = *reinterpret_cast<const uint4*>(sn + ((int64_t)ky * ws + kx) * c);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float v = osr_to_float(v8[k]);
                        if (am[k] < 0 || v > m[k] || isnan(v)) {  // (am < 0: the first valid position starts the scan, as torch's maxindex)
                            m[k] = v;
                            am[k] = ky * ws + kx;
                        }
                    }
                }
            }
            T d8[8];
            *reinterpret_cast<uint4*>(d8) = *reinterpret_cast<const uint4*>(dpool + (((int64_t)ni * ho + py) * wo + px) * c + ch);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (am[k] == me) acc[k] += osr_to_float(d8[k]);
        }
    }
    T o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = osr_from_float<T>(osr_to_float(sv[k]) <= 0.f ? 0.f : acc[k]);  // the ReLU's mask (a NaN output passes)
    *reinterpret_cast<uint4*>(ds + pix * c + ch) = *reinterpret_cast<const uint4*>(o);
}

// One workgroup (4 waves) per pixel range; every wave owns 4 x 4 16x16 tiles of the (64, 256) result: co tiles 0..3, K tiles 4w..4w+3.
template <class T>
__global__ void __launch_bounds__(256) stem_wgrad_partial_kernel(const T* __restrict__ xpad, const T* __restrict__ ds, float* __restrict__ part,
                                                                 int hs, int ws, int hd, int wd, int64_t P, int64_t chunks_per_range,
                                                                 int64_t nchunks) {
    typedef typename StemMfma<T>::frag frag;
    __shared__ __align__(16) T dsT[kCout * kLdsRow];
    __shared__ __align__(16) T aT[kK * kLdsRow];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int64_t c0 = (int64_t)blockIdx.x * chunks_per_range;
    const int64_t c1 = min(nchunks, c0 + chunks_per_range);
    const int px = t >> 3, sub = t & 7;
    for (int64_t ck = c0; ck < c1; ++ck) {
        const int64_t p = ck * kChunk + px;
        // dS: 8 channels of one pixel per thread -> dsT[co][px]
        T dv[8];
        // image patch: one of the 8 rows (32 halves = 8 taps x 4 channels) of one pixel per thread -> aT[row * 32 + j][px]
        T av[32];
        if (p < P) {
            const uint4 d4 = *reinterpret_cast<const uint4*>(ds + p * kCout + sub * 8);
            *reinterpret_cast<uint4*>(dv) = d4;
            const int ox = (int)(p % ws);
            const int64_t q = p / ws;
            const int oy = (int)(q % hs);
            const int64_t ni = q / hs;
            const T* src = xpad + ((ni * hd + 2 * oy + sub) * (int64_t)wd + 2 * ox) * 4;
#pragma unroll
            for (int j = 0; j < 8; ++j) *reinterpret_cast<uint2*>(av + 4 * j) = *reinterpret_cast<const uint2*>(src + 4 * j);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) dv[j] = osr_from_float<T>(0.f);
#pragma unroll
            for (int j = 0; j < 32; ++j) av[j] = osr_from_float<T>(0.f);
        }
        __syncthreads();  // (the previous chunk's fragment reads are done)
#pragma unroll
        for (int j = 0; j < 8; ++j) dsT[(sub * 8 + j) * kLdsRow + px] = dv[j];
#pragma unroll
        for (int j = 0; j < 32; ++j) aT[(sub * 32 + j) * kLdsRow + px] = av[j];
        __syncthreads();
        frag fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const frag*>(&dsT[(i * 16 + (lane & 15)) * kLdsRow + (lane >> 4) * 8]);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const frag*>(&aT[((wave * 4 + j) * 16 + (lane & 15)) * kLdsRow + (lane >> 4) * 8]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = StemMfma<T>::mfma(fa[i], fb[j], acc[i][j]);
    }
    float* out = part + (int64_t)blockIdx.x * kCout * kK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(i * 16 + (lane >> 4) * 4 + r) * kK + (wave * 4 + j) * 16 + (lane & 15)] = acc[i][j][r];
}

__global__ void __launch_bounds__(256) stem_wgrad_reduce_kernel(const float* __restrict__ part, int ranges, float* __restrict__ dw, int accumulate) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= kCout * kK) return;
    const int k = idx % kK, row = k >> 5, tap = (k >> 2) & 7, ch = k & 3;
    float v = 0.f;
    if (row < 7 && tap < 7 && ch < 3) {
        for (int b = 0; b < ranges; ++b) v += part[(int64_t)b * kCout * kK + idx];  // range order: fixed
        if (accumulate) v += dw[idx];
    }
    dw[idx] = v;
}

int64_t stem_ranges(int64_t P) {
    const int64_t nchunks = (P + kChunk - 1) / kChunk;
    return nchunks < kMaxRanges ? nchunks : kMaxRanges;
}

}  // namespace

extern "C" osr_status osr_stem_pool_bwd(const void* s, const void* dpool, int32_t n, int32_t hs, int32_t ws, int32_t c, void* ds, int32_t dtype,
                                        void* stream) {
    OSR_REQUIRE(s && dpool && ds, OSR_ERR_INVALID_ARG, "osr_stem_pool_bwd: null pointer");
    OSR_REQUIRE(n > 0 && hs > 0 && ws > 0 && c > 0 && c % 8 == 0, OSR_ERR_INVALID_ARG, "osr_stem_pool_bwd: bad shape (c a multiple of 8)");
    OSR_REQUIRE(dtype == OSR_F16 || dtype == OSR_BF16, OSR_ERR_UNSUPPORTED, "osr_stem_pool_bwd: dtype must be f16 / bf16");
    const int64_t total = (int64_t)n * hs * ws * (c / 8);
    const int64_t blocks = (total + 255) / 256;
    OSR_REQUIRE(blocks < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_stem_pool_bwd: too large");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == OSR_F16)
        hipLaunchKernelGGL(stem_pool_bwd_kernel<f16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const f16_t*)s, (const f16_t*)dpool, (f16_t*)ds, n, hs, ws, c);
    else
        hipLaunchKernelGGL(stem_pool_bwd_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)s, (const bf16_t*)dpool, (bf16_t*)ds, n, hs, ws,
                           c);
    OSR_CHECK_LAUNCH("osr_stem_pool_bwd");
    return OSR_OK;
}

extern "C" int64_t osr_stem_wgrad_workspace_bytes(int32_t n, int32_t hp, int32_t wp) {
    if (n <= 0 || hp <= 0 || wp <= 0) return OSR_ERR_INVALID_ARG;
    const int64_t P = (int64_t)n * (hp / 2) * (wp / 2);
    return stem_ranges(P) * kCout * kK * (int64_t)sizeof(float);
}

extern "C" osr_status osr_stem_wgrad(const void* xpad, const void* ds, int32_t n, int32_t hp, int32_t wp, float* dw, int32_t accumulate, void* workspace,
                                     int64_t workspace_bytes, int32_t dtype, void* stream) {
    OSR_REQUIRE(xpad && ds && dw, OSR_ERR_INVALID_ARG, "osr_stem_wgrad: null pointer");
    OSR_REQUIRE(n > 0 && hp > 0 && wp > 0 && hp % 2 == 0 && wp % 2 == 0, OSR_ERR_INVALID_ARG, "osr_stem_wgrad: n > 0, hp and wp even");
    OSR_REQUIRE(dtype == OSR_F16 || dtype == OSR_BF16, OSR_ERR_UNSUPPORTED, "osr_stem_wgrad: dtype must be f16 / bf16");
    const int64_t need = osr_stem_wgrad_workspace_bytes(n, hp, wp);
    OSR_REQUIRE(workspace && workspace_bytes >= need, OSR_ERR_INVALID_ARG, "osr_stem_wgrad: workspace of %lld bytes needed", (long long)need);
    const int hs = hp / 2, ws = wp / 2, hd = hp + 6, wd = osr_stem_padded_width(wp);
    OSR_REQUIRE(wd >= wp + 6, OSR_ERR_INVALID_ARG, "osr_stem_wgrad: padded width");
    const int64_t P = (int64_t)n * hs * ws;
    const int64_t nchunks = (P + kChunk - 1) / kChunk;
    const int64_t ranges = stem_ranges(P);
    const int64_t per = (nchunks + ranges - 1) / ranges;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (dtype == OSR_F16)
        hipLaunchKernelGGL(stem_wgrad_partial_kernel<f16_t>, dim3((unsigned)ranges), dim3(256), 0, st, (const f16_t*)xpad, (const f16_t*)ds, part, hs, ws, hd, wd,
                           P, per, nchunks);
    else
        hipLaunchKernelGGL(stem_wgrad_partial_kernel<bf16_t>, dim3((unsigned)ranges), dim3(256), 0, st, (const bf16_t*)xpad, (const bf16_t*)ds, part, hs, ws, hd,
                           wd, P, per, nchunks);
    OSR_CHECK_LAUNCH("osr_stem_wgrad(partials)");
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(kCout * kK / 256), dim3(256), 0, st, part, (int)ranges, dw, accumulate);
    OSR_CHECK_LAUNCH("osr_stem_wgrad(reduce)");
    return OSR_OK;
}
