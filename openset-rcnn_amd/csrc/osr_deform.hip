// Deformable convolution, the gather half (include/osr.h osr_deform_cols): the masked bilinear samples of a 3x3 deformable
// convolution's nine taps, written as the (pixels, 9, c) matrix that the 1x1 MFMA contraction then multiplies with the layer's
// (cout, 3, 3, c) weight. Built with -ffp-contract=off: the only fused multiply-adds are the three written out below.
//
// Work split: one lane owns 8 consecutive channels of one (output pixel, tap); consecutive lanes take consecutive channel vectors,
// so each of the four corner reads of a wave is one contiguous segment of an input row (16 B per lane for f16 / bf16, 32 B for
// fp32) and the store is one contiguous segment of cols. The lanes of one (pixel, tap, group) read the same two offsets (and the
// same mask logit): one address per wave and group, served as one request.
//
// Arithmetic. The sample position of tap (i, j) at output pixel (y, x) is h = y * stride - 1 + i + dy: an integer plus an fp32
// offset. It is never rounded to fp32: the in-range test compares dy with the two integers -1 - base and H - base (exact), and the
// cell and the fraction come from dy alone -- for dy >= 0, floor and dy - floor(dy) are exact; for dy < 0 the exact quantity is
// 1 - lh = |dy| - floor(|dy|). So of the pair (lh, 1 - lh) one is exact and the other carries one rounding (relative 2^-24), never an
// absolute error of the fraction that a small corner value would not cover. The modulation scalar is a sigmoid evaluated in fp64 and
// rounded once (one value per pixel, tap and group; the kernel is bound by its reads and writes). Per element: three roundings
// in a corner's weight, four in the blend (a product and three fused multiply-adds), one for the mask, one to the storage dtype.
#include "osr_common.h"

namespace {

// d = an offset with base + d inside (-1, size): cell index (relative to base) and the two interpolation factors.
__device__ __forceinline__ void deform_split(float d, int& cell, float& lo, float& hi) {
    const float a = fabsf(d), fa = floorf(a), r = a - fa;  // exact
    if (d >= 0.f) {
        cell = (int)fa; hi = r; lo = 1.f - r;
    } else if (r == 0.f) {
        cell = -(int)fa; hi = 0.f; lo = 1.f;
    } else {
        cell = -(int)fa - 1; lo = r; hi = 1.f - r;
    }
}

// One work item: 8 channels (from cc) of row pk = (pixel, tap) of cols. `inside` false: the sample is zero and nothing is read.
struct deform_item {
    unsigned pk;
    int cc;
    bool live, inside, r0, r1, q0, q1;
    long long at;  // element offset of corner (y0, x0): formed, read only where r0 && q0
    float w00, w01, w10, w11, m;
};

template <bool MOD>
__device__ __forceinline__ deform_item deform_setup(unsigned i, unsigned total, const float* __restrict__ om, int h, int w, int c, unsigned c8, int ho,
                                                    int wo, int ch, int stride, int cg, int groups) {
    deform_item it;
    it.live = i < total;
    it.inside = false;
    it.pk = 0; it.cc = 0; it.at = 0;
    it.r0 = it.r1 = it.q0 = it.q1 = false;
    it.w00 = it.w01 = it.w10 = it.w11 = 0.f;
    it.m = 1.f;
    if (!it.live) return it;
    const unsigned pk = i / c8;
    const int cc = (int)(i - pk * c8) * 8;
    const unsigned p = pk / 9, py = p / (unsigned)wo, pb = py / (unsigned)ho;
    const int k = (int)(pk - p * 9);
    const int ox = (int)(p - py * (unsigned)wo), oy = (int)(py - pb * (unsigned)ho), b = (int)pb;
    const int g = groups == 1 ? 0 : cc / cg;
    const float* o = om + (long long)p * ch;
    const float dy = o[2 * (9 * g + k)], dx = o[2 * (9 * g + k) + 1];
    const int by = oy * stride - 1 + k / 3, bx = ox * stride - 1 + k % 3;
    it.pk = pk;
    it.cc = cc;
    // h > -1, w > -1, h < H, w < W; false for NaN and +-inf
    it.inside = dy > (float)(-1 - by) && dy < (float)(h - by) && dx > (float)(-1 - bx) && dx < (float)(w - bx);
    if (it.inside) {
        int y0, x0;
        float ly0, ly1, lx0, lx1;  // weights of row y0 / y0 + 1 and of column x0 / x0 + 1
        deform_split(dy, y0, ly0, ly1);
        deform_split(dx, x0, lx0, lx1);
        y0 += by;
        x0 += bx;
        // a corner outside the map contributes zero and is not read (a predicate, not a clamp: the value never moves)
        it.r0 = y0 >= 0; it.r1 = y0 + 1 <= h - 1; it.q0 = x0 >= 0; it.q1 = x0 + 1 <= w - 1;
        it.at = (((long long)b * h + y0) * w + x0) * c + cc;
        it.w00 = ly0 * lx0; it.w01 = ly0 * lx1; it.w10 = ly1 * lx0; it.w11 = ly1 * lx1;
        if (MOD) it.m = (float)(1.0 / (1.0 + exp(-(double)o[18 * groups + 9 * g + k])));
    }
    return it;
}

// Two items per lane and pass (this grid-stride step's and the next one's): their offset reads, then their eight corner reads, are in
// flight together -- the kernel is two dependent round trips per item and little else.
template <class T, bool MOD>
__global__ __launch_bounds__(256) void deform_cols_kernel(const T* __restrict__ x, const float* __restrict__ om, int n, int h, int w, int c,
                                                          int ho, int wo, int ch, int stride, int cg, int groups, T* __restrict__ cols) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    // (the work items fit 31 bits, the entry point sees to it: a 64-bit division per index would cost more than the four loads)
    const unsigned c8 = c / 8, total = (unsigned)n * ho * wo * 9 * c8, step = gridDim.x * blockDim.x;
    const long long row = (long long)w * c;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += 2 * step) {
        deform_item it[2];
        t8 v[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) it[u] = deform_setup<MOD>(i + u * step, total, om, h, w, c, c8, ho, wo, ch, stride, cg, groups);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) v[u][q][e] = (T)0.f;
            if (it[u].r0 && it[u].q0) v[u][0] = *reinterpret_cast<const t8*>(x + it[u].at);
            if (it[u].r0 && it[u].q1) v[u][1] = *reinterpret_cast<const t8*>(x + it[u].at + c);
            if (it[u].r1 && it[u].q0) v[u][2] = *reinterpret_cast<const t8*>(x + it[u].at + row);
            if (it[u].r1 && it[u].q1) v[u][3] = *reinterpret_cast<const t8*>(x + it[u].at + row + c);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!it[u].live) continue;
            t8 out;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float s = it[u].w00 * (float)v[u][0][e];
                s = fmaf(it[u].w01, (float)v[u][1][e], s);
                s = fmaf(it[u].w10, (float)v[u][2][e], s);
                s = fmaf(it[u].w11, (float)v[u][3][e], s);
                out[e] = (T)(MOD ? s * it[u].m : s);
            }
            *reinterpret_cast<t8*>(cols + (long long)it[u].pk * c + it[u].cc) = out;
        }
    }
}

}  // namespace

extern "C" osr_status osr_deform_cols(const void* x, const float* om, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo,
                                      int32_t ch, int32_t stride, int32_t groups, int32_t modulated, void* cols, int32_t dtype, void* stream) {
    OSR_REQUIRE(x && om && cols, OSR_ERR_INVALID_ARG, "osr_deform_cols: null pointer");
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_deform_cols: bad dtype");
    OSR_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1 && groups >= 1, OSR_ERR_INVALID_ARG, "osr_deform_cols: bad sizes");
    OSR_REQUIRE(stride == 1 || stride == 2, OSR_ERR_INVALID_ARG, "osr_deform_cols: stride must be 1 or 2, got %d", stride);
    OSR_REQUIRE(ho == (h - 1) / stride + 1 && wo == (w - 1) / stride + 1, OSR_ERR_INVALID_ARG,
                "osr_deform_cols: ho / wo must be those of a 3x3 convolution with padding 1 (%d x %d for %d x %d at stride %d)",
                (h - 1) / stride + 1, (w - 1) / stride + 1, h, w, stride);
    OSR_REQUIRE(c % 8 == 0 && c % groups == 0 && (c / groups) % 8 == 0, OSR_ERR_UNSUPPORTED,
                "osr_deform_cols: c, and c / groups, must be multiples of 8 (c %d, groups %d)", c, groups);
    const long long need = (long long)(modulated ? 27 : 18) * groups;
    OSR_REQUIRE(ch >= need, OSR_ERR_INVALID_ARG, "osr_deform_cols: om has %d channels per pixel, %lld are read", ch, need);
    OSR_REQUIRE((((uintptr_t)x | (uintptr_t)cols) & 15) == 0 && (((uintptr_t)om) & 3) == 0, OSR_ERR_INVALID_ARG,
                "osr_deform_cols: x and cols must be 16-byte aligned");
    const long long total = (long long)n * ho * wo * 9 * (c / 8);
    OSR_REQUIRE(total < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_deform_cols: problem too large (%lld 8-channel samples, at most 2^31 - 1)", total);
    long long blocks = (total + 511) / 512;  // two items per lane and pass
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipStream_t st = (hipStream_t)stream;
    const int cg = c / groups;
#define OSR_DC(T)                                                                                                                            \
    do {                                                                                                                                     \
        if (modulated) hipLaunchKernelGGL((deform_cols_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, om, n, h, w, c, ho, wo, ch, \
                                          stride, cg, groups, (T*)cols);                                                                     \
        else hipLaunchKernelGGL((deform_cols_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, om, n, h, w, c, ho, wo, ch, stride, \
                                cg, groups, (T*)cols);                                                                                       \
    } while (0)
    if (dtype == OSR_F16) OSR_DC(f16_t);
    else if (dtype == OSR_BF16) OSR_DC(bf16_t);
    else OSR_DC(float);
#undef OSR_DC
    OSR_CHECK_LAUNCH("osr_deform_cols");
    return OSR_OK;
}
