// Split-precision convolution (include/osr.h: osr_conv2d_split_fwd): the fp32 layers of the parity mode -- ResNet-50 + FPN and the
// CF-RPN head's 3x3 -- at fp32 quality on the bf16 matrix instruction.
//
// The arithmetic is that of osr_linear_split.hip: every fp32 value is the sum of two bf16 terms to 2^-17 of its magnitude,
//     x = x0 + x1,  W = w0 + w1        x0 = bf16(x), x1 = bf16(x - x0)
//     acc = x0 w1 + x1 w0 + x0 w0      three v_mfma_f32_32x32x16_bf16 per K step into ONE fp32 accumulator tile
// (the x1 w1 term is dropped). The weights are static and arrive split (two bf16 planes of [cout][kh][kw][cin]); the activations are
// NHWC fp32 and are split on the way from global memory to LDS.
//
// Implicit GEMM: M = n*ho*wo output pixels, N = cout, K = kh*kw*cin. A 32-wide K slice is 128 contiguous bytes of one tap of one input
// pixel (cin % 32 == 0); the 7x7 stem runs as the (kh = 8, kw = 1, cin = 32) view of the pre-padded NHWC4 image (pad_mode 1), as in
// conv_f32_kernel. Tile: 128 x 128 x 32 per 256-thread workgroup (2 x 2 waves, 64 x 64 per wave), 128 x 64 when cout == 64; the K loop
// is linear_split_kernel's: LDS double buffer with 80-byte rows, the next two K slices in registers behind the current slice's MFMAs,
// one barrier per K step.
//
// Zero padding: the predicate of a tap (inside the image? a row of this launch? a slice of this layer?) selects the ADDRESS of the
// load, never its value: a tap outside the image reads a constant line of zeros, and a padding tap contributes exactly zero. Both
// addresses are held as address-space-1 pointers, so the selected load is a global_load_dwordx4 (a select between generic pointers
// compiles to flat loads, which count on the LDS counter too and are waited for in front of the first MFMA of the K step). In the
// gfx950 ISA the K loop has no vmcnt wait in front of its MFMAs; the LDS stores of a slice wait with vmcnt(9) / vmcnt(8), that is
// with the eight loads of the following slice still in flight.
//
// No split-K and no atomics: one workgroup owns an output tile and sums its K axis in order, slice by slice, whatever the tile's place
// in the launch -- a launch is bitwise reproducible and an output pixel's bits do not depend on the batch size.
//
// Workgroup order: as linear_split_kernel (consecutive ids round-robin over 8 XCDs; each XCD walks a contiguous range of the row-major
// tile list, so the column tiles that share a slice of the activations meet in one L2).
#include "osr_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// a pointer the compiler knows to be global memory: a select between two of them stays a global_load (a select between generic pointers
// is a flat load, which counts on the LDS counter as well and is waited for in front of the K step's first fragment read)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) f32x4* gf4_ptr;

#define CS_BM 128
#define CS_BK 32
#define CS_ROWB 80  // LDS bytes per tile row: 64 data + 16 pad
#define CS_XCDS 8

// what a tap outside the image reads (one K slice of one pixel: 32 floats)
__device__ __attribute__((aligned(128))) const float cs_zero_line[CS_BK] = {};

struct ConvSplitArgs {
    const float* in;
    const bf16_t* w0;
    const bf16_t* w1;
    const float* bias;
    const float* res;
    float* out;
    long long in_stride_n, out_stride_n, res_stride_n;
    int in_stride_h, in_stride_w, out_stride_h, out_stride_w, res_stride_h, res_stride_w;
    int hi, wi, cin, ho, wo, cout, kw;
    int stride_h, stride_w, pad_h, pad_w;
    int relu, res_mode;
    int m, k;
    int tiles_m, tiles_n, per_xcd;
};

template <int TN>  // 32 x 32 accumulator tiles per wave along cout: the tile is 128 x (64 * TN)
__global__ __launch_bounds__(256) void conv_split_kernel(ConvSplitArgs a) {
    constexpr int TM = 2;
    constexpr int BN = 64 * TN;
    constexpr int A_TILE = CS_BM * CS_ROWB, B_TILE = BN * CS_ROWB;
    constexpr int STAGE = 2 * A_TILE + 2 * B_TILE;  // x0, x1, w0, w1
    constexpr int A_CH = CS_BM * 8 / 256;           // float4 chunks of activations per thread per K step (8 per row)
    constexpr int B_CH = BN * 4 / 256;              // 16-byte chunks of one weight plane per thread per K step (4 per row)
    constexpr int EPI_LD = TN * 32 + 4;             // floats per staged row
    static_assert(4 * 32 * EPI_LD * 4 <= 2 * STAGE, "epilogue slabs fit the K loop's LDS");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int logical = (int)(blockIdx.x % CS_XCDS) * a.per_xcd + (int)(blockIdx.x / CS_XCDS);
    if (logical >= a.tiles_m * a.tiles_n) return;
    const int tile_n = logical % a.tiles_n, tile_m = logical / a.tiles_n;
    const int m0 = tile_m * CS_BM, n0 = tile_n * BN;

    const bf16_t* __restrict__ w0 = a.w0;
    const bf16_t* __restrict__ w1 = a.w1;

    // ---- per-thread load descriptors (fixed over the K loop): thread -> 4 output pixels (tile rows tid/8 + 32 i) x one 4-float chunk of
    //      the slice. A tile row beyond m gets an input row far outside the image: every tap of it reads the zero line. ----
    gf4_ptr a_img[A_CH];
    int a_ih0[A_CH], a_iw0[A_CH];
    const int chunk = (tid & 7) * 4;
    const int howo = a.ho * a.wo;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int m = m0 + (tid >> 3) + 32 * i;
        const bool ok = m < a.m;
        const int mm = ok ? m : 0;
        const int ni = mm / howo, rem = mm - ni * howo;
        const int oh = rem / a.wo, ow = rem - oh * a.wo;
        a_img[i] = (gf4_ptr)(a.in + (long long)ni * a.in_stride_n + chunk);
        a_ih0[i] = ok ? oh * a.stride_h - a.pad_h : -(1 << 29);
        a_iw0[i] = ow * a.stride_w - a.pad_w;
    }
    long long b_off[B_CH];
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        const int q = tid + 256 * i, row = q >> 2;
        b_off[i] = (long long)(n0 + row < a.cout ? n0 + row : 0) * a.k + (q & 3) * 8;  // (a weight row beyond cout: row 0, never stored)
    }
    const gf4_ptr zero_src = (gf4_ptr)(cs_zero_line + chunk);

    // the slice the next LOAD fetches: tap (kh, kw), channel origin c0, flat K index kf. Workgroup-uniform (scalar registers). Beyond the
    // last slice (kf >= k: the tail loads of the pipeline, and the second half of the last trip when the slice count is odd) the
    // activations read the zero line and the weights the last slice again: such a slice adds exactly zero.
    int l_kh = 0, l_kw = 0, l_c0 = 0, l_kf = 0;
    const int klast = a.k - CS_BK;

    f32x4 raE[A_CH], raO[A_CH];
    u32x4 rb0E[B_CH], rb1E[B_CH], rb0O[B_CH], rb1O[B_CH];

    // (macros, not lambdas: by-reference captures of the register arrays would force them into scratch)
#define CS_LOAD_TILES(ra, rb0, rb1)                                                              \
    {                                                                                            \
        const bool live_ = l_kf < a.k;                                                           \
        _Pragma("unroll") for (int i = 0; i < A_CH; ++i) {                                       \
            const int ih = a_ih0[i] + l_kh, iw = a_iw0[i] + l_kw;                                \
            const bool ok = live_ && (unsigned)ih < (unsigned)a.hi && (unsigned)iw < (unsigned)a.wi; \
            const unsigned off = (unsigned)ih * (unsigned)a.in_stride_h + (unsigned)iw * (unsigned)a.in_stride_w + (unsigned)l_c0; \
            const gf4_ptr src = ok ? (gf4_ptr)((const __attribute__((address_space(1))) float*)a_img[i] + off) : zero_src; \
            ra[i] = *src;                                                                        \
        }                                                                                        \
        const int kfw_ = min(l_kf, klast);                                                       \
        _Pragma("unroll") for (int i = 0; i < B_CH; ++i) {                                       \
            rb0[i] = *reinterpret_cast<const u32x4*>(w0 + b_off[i] + kfw_);                      \
            rb1[i] = *reinterpret_cast<const u32x4*>(w1 + b_off[i] + kfw_);                      \
        }                                                                                        \
        l_kf += CS_BK;                                                                           \
        l_c0 += CS_BK;                                                                           \
        if (l_c0 >= a.cin) {                                                                     \
            l_c0 = 0;                                                                            \
            if (++l_kw >= a.kw) { l_kw = 0; ++l_kh; }                                            \
        }                                                                                        \
    }
    // the split of the activations: x0 = bf16(x) (round to nearest even), x1 = bf16(x - x0) (the subtraction is exact)
#define CS_STORE_TILES(buf, ra, rb0, rb1)                                                        \
    {                                                                                            \
        unsigned char* s_ = lds + (buf) * STAGE;                                                 \
        _Pragma("unroll") for (int i = 0; i < A_CH; ++i)                                         \
            asm volatile("" : "+v"(ra[i]));                                                      \
        _Pragma("unroll") for (int i = 0; i < A_CH; ++i) {                                       \
            const int q = tid + 256 * i;                                                         \
            const float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};                             \
            bf16x4 h, l;                                                                         \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                      \
                h[e] = (bf16_t)v[e];                                                             \
                l[e] = (bf16_t)(v[e] - (float)h[e]);                                             \
            }                                                                                    \
            *reinterpret_cast<bf16x4*>(s_ + (q >> 3) * CS_ROWB + (q & 7) * 8) = h;               \
            *reinterpret_cast<bf16x4*>(s_ + A_TILE + (q >> 3) * CS_ROWB + (q & 7) * 8) = l;      \
        }                                                                                        \
        _Pragma("unroll") for (int i = 0; i < B_CH; ++i) {                                       \
            const int q = tid + 256 * i;                                                         \
            *reinterpret_cast<u32x4*>(s_ + 2 * A_TILE + (q >> 2) * CS_ROWB + (q & 3) * 16) = rb0[i]; \
            *reinterpret_cast<u32x4*>(s_ + 2 * A_TILE + B_TILE + (q >> 2) * CS_ROWB + (q & 3) * 16) = rb1[i]; \
        }                                                                                        \
    }
    // one K slice out of LDS stage buf: per 16 columns of K, x0 w1 and x1 w0 (the small terms) first, x0 w0 last
#define CS_MULTIPLY(buf)                                                                         \
    {                                                                                            \
        const unsigned char* s = lds + (buf) * STAGE;                                            \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                       \
            bf16x8 fa0[TM], fa1[TM], fb0[TN], fb1[TN];                                           \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                     \
                const int off = ((wr * TM + i) * 32 + (lane & 31)) * CS_ROWB + kk * 32 + (lane >> 5) * 16; \
                fa0[i] = *reinterpret_cast<const bf16x8*>(s + off);                              \
                fa1[i] = *reinterpret_cast<const bf16x8*>(s + A_TILE + off);                     \
            }                                                                                    \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                     \
                const int off = ((wc * TN + j) * 32 + (lane & 31)) * CS_ROWB + kk * 32 + (lane >> 5) * 16; \
                fb0[j] = *reinterpret_cast<const bf16x8*>(s + 2 * A_TILE + off);                 \
                fb1[j] = *reinterpret_cast<const bf16x8*>(s + 2 * A_TILE + B_TILE + off);        \
            }                                                                                    \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                       \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                   \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0[i], fb1[j], acc[i][j], 0, 0, 0); \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                       \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                   \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa1[i], fb0[j], acc[i][j], 0, 0, 0); \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                       \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                   \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa0[i], fb0[j], acc[i][j], 0, 0, 0); \
        }                                                                                        \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // two K slices per trip -- even slices through register set E and LDS stage 0, odd ones through set O and stage 1 (no branch around
    // a load or a store, and the scheduling fences: see linear_split_kernel)
    const int nk = a.k / CS_BK;
    CS_LOAD_TILES(raE, rb0E, rb1E);
    CS_LOAD_TILES(raO, rb0O, rb1O);
    CS_STORE_TILES(0, raE, rb0E, rb1E);
    __syncthreads();
    for (int ks = 0; ks < nk; ks += 2) {
        CS_LOAD_TILES(raE, rb0E, rb1E);
        __builtin_amdgcn_sched_barrier(0);
        CS_MULTIPLY(0);
        __builtin_amdgcn_sched_barrier(0);
        CS_STORE_TILES(1, raO, rb0O, rb1O);
        __syncthreads();
        CS_LOAD_TILES(raO, rb0O, rb1O);
        __builtin_amdgcn_sched_barrier(0);
        CS_MULTIPLY(1);
        __builtin_amdgcn_sched_barrier(0);
        CS_STORE_TILES(0, raE, rb0E, rb1E);
        __syncthreads();
    }
#undef CS_LOAD_TILES
#undef CS_STORE_TILES
#undef CS_MULTIPLY

    // ---- epilogue: acc -> wave-private LDS slab (32 rows x 32 TN fp32) -> bias, residual, ReLU on 8 channels per lane, coalesced
    //      stores. (The last K step ended with a barrier: nobody reads the K loop's LDS any more.) ----
    float* slab = reinterpret_cast<float*>(lds) + wid * 32 * EPI_LD;
    constexpr int LPR = TN * 4;    // lanes per staged row (8 channels each)
    constexpr int RPP = 64 / LPR;  // rows per pass
    const int cseg = (lane % LPR) * 8;
    const int co = n0 + wc * TN * 32 + cseg;
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (co < a.cout) {
        const float4 b0 = *reinterpret_cast<const float4*>(a.bias + co);
        const float4 b1 = *reinterpret_cast<const float4*>(a.bias + co + 4);
        bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                slab[row * EPI_LD + j * 32 + (lane & 31)] = acc[i][j][r];
            }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): wave-private slab, no barrier needed
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int pass = 0; pass < 32 / RPP; ++pass) {
            const int row = pass * RPP + lane / LPR;
            const int m = m0 + (wr * TM + i) * 32 + row;
            if (m < a.m && co < a.cout) {
                const float4 v0 = *reinterpret_cast<const float4*>(slab + row * EPI_LD + cseg);
                const float4 v1 = *reinterpret_cast<const float4*>(slab + row * EPI_LD + cseg + 4);
                float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                const int ni = m / howo, rem = m - ni * howo;
                const int yo = rem / a.wo, xo = rem - yo * a.wo;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += bv[e];
                if (a.res_mode != 0) {
                    const int rh = a.res_mode == 2 ? (yo >> 1) : yo, rw = a.res_mode == 2 ? (xo >> 1) : xo;
                    const float* rp = a.res + (long long)ni * a.res_stride_n + (long long)rh * a.res_stride_h + (long long)rw * a.res_stride_w + co;
                    const float4 r0 = *reinterpret_cast<const float4*>(rp);
                    const float4 r1 = *reinterpret_cast<const float4*>(rp + 4);
                    const float rv[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
                    if (a.res_mode == 3) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = rv[e] > 0.f ? v[e] : 0.f;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += rv[e];
                    }
                }
                if (a.relu) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                float* o = a.out + (long long)ni * a.out_stride_n + (long long)yo * a.out_stride_h + (long long)xo * a.out_stride_w + co;
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int TN>
static osr_status conv_split_launch(ConvSplitArgs& a, hipStream_t st) {
    constexpr int BN = 64 * TN;
    constexpr int LDS = 2 * (2 * CS_BM + 2 * BN) * CS_ROWB;
    a.tiles_m = (a.m + CS_BM - 1) / CS_BM;
    a.tiles_n = (a.cout + BN - 1) / BN;
    const long long tiles = (long long)a.tiles_m * a.tiles_n;
    OSR_REQUIRE(tiles <= (1ll << 30), OSR_ERR_UNSUPPORTED, "osr_conv2d_split_fwd: problem too large");
    a.per_xcd = (int)((tiles + CS_XCDS - 1) / CS_XCDS);
    static osr_dev_mask once{0};
    osr_once_per_device(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_split_kernel<TN>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS); });
    hipLaunchKernelGGL(conv_split_kernel<TN>, dim3((unsigned)(a.per_xcd * CS_XCDS)), dim3(256), LDS, st, a);
    OSR_CHECK_LAUNCH("osr_conv2d_split_fwd");
    return OSR_OK;
}

extern "C" osr_status osr_conv2d_split_fwd(const osr_conv_params* p, const float* in, const void* w_hi, const void* w_lo, const float* bias,
                                           const float* residual, float* out, void* stream) {
    OSR_REQUIRE(p && in && w_hi && w_lo && bias && out, OSR_ERR_INVALID_ARG, "osr_conv2d_split_fwd: null pointer");
    OSR_REQUIRE(p->in_dtype == OSR_F32 && p->out_dtype == OSR_F32, OSR_ERR_UNSUPPORTED, "osr_conv2d_split_fwd: in_dtype and out_dtype must be f32");
    OSR_REQUIRE(p->n >= 1 && p->hi >= 1 && p->wi >= 1 && p->ho >= 1 && p->wo >= 1 && p->cin >= 1 && p->cout >= 1, OSR_ERR_INVALID_ARG,
                "osr_conv2d_split_fwd: bad shape");
    OSR_REQUIRE(p->res_mode >= 0 && p->res_mode <= 3 && (p->res_mode == 0 || residual), OSR_ERR_INVALID_ARG,
                "osr_conv2d_split_fwd: res_mode %d needs a residual (modes 0..3)", p->res_mode);
    OSR_REQUIRE(p->cin % 32 == 0, OSR_ERR_UNSUPPORTED, "osr_conv2d_split_fwd: cin must be a multiple of 32, got %d", p->cin);
    OSR_REQUIRE(p->cout % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_conv2d_split_fwd: cout must be a multiple of 64, got %d", p->cout);
    const bool stem = p->pad_mode == 1 && p->kh == 8 && p->kw == 1 && p->cin == 32 && p->stride_h == 2 && p->stride_w == 2 && p->pad_h == 0 && p->pad_w == 0;
    const bool square = p->pad_mode == 0 && p->kh == p->kw && (p->kh == 1 || p->kh == 3) && p->stride_h == p->stride_w &&
                        (p->stride_h == 1 || p->stride_h == 2) && p->pad_h == p->pad_w && p->pad_h >= 0 && p->pad_h < p->kh;
    OSR_REQUIRE(stem || square, OSR_ERR_UNSUPPORTED,
                "osr_conv2d_split_fwd: 1x1 / 3x3 at stride 1 / 2 or the stem view (kh 8, kw 1, cin 32, pad_mode 1), got %dx%d stride %d,%d pad %d,%d pad_mode %d",
                p->kh, p->kw, p->stride_h, p->stride_w, p->pad_h, p->pad_w, p->pad_mode);
    // every tap the launch reads lies inside the input the strides describe
    if (stem) {
        OSR_REQUIRE((long long)(p->ho - 1) * 2 + 8 <= p->hi && ((long long)(p->wo - 1) * 2 + 8) * p->in_stride_w <= p->in_stride_h, OSR_ERR_INVALID_ARG,
                    "osr_conv2d_split_fwd: the stem view reads beyond the padded image");
    } else {
        OSR_REQUIRE((long long)(p->ho - 1) * p->stride_h - p->pad_h + p->kh - 1 < (long long)p->hi + p->pad_h &&
                        (long long)(p->wo - 1) * p->stride_w - p->pad_w + p->kw - 1 < (long long)p->wi + p->pad_w,
                    OSR_ERR_INVALID_ARG, "osr_conv2d_split_fwd: output size does not fit the input");
        OSR_REQUIRE(p->in_stride_w >= p->cin && p->in_stride_h >= (long long)p->wi * p->in_stride_w, OSR_ERR_INVALID_ARG, "osr_conv2d_split_fwd: bad input strides");
    }
    OSR_REQUIRE(p->in_stride_n >= (long long)p->hi * p->in_stride_h, OSR_ERR_INVALID_ARG, "osr_conv2d_split_fwd: bad input strides");
    OSR_REQUIRE(p->in_stride_w % 4 == 0 && p->in_stride_h % 4 == 0 && p->in_stride_n % 4 == 0 && p->out_stride_w % 4 == 0 && p->out_stride_h % 4 == 0 &&
                    p->out_stride_n % 4 == 0 && (p->res_mode == 0 || (p->res_stride_w % 4 == 0 && p->res_stride_h % 4 == 0 && p->res_stride_n % 4 == 0)),
                OSR_ERR_INVALID_ARG, "osr_conv2d_split_fwd: strides must be multiples of 4 elements (16-byte accesses)");
    OSR_REQUIRE(p->out_stride_w >= p->cout && p->out_stride_h > 0 && p->out_stride_n > 0, OSR_ERR_INVALID_ARG, "osr_conv2d_split_fwd: bad output strides");
    OSR_REQUIRE((((uintptr_t)in | (uintptr_t)w_hi | (uintptr_t)w_lo | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_conv2d_split_fwd: pointers must be 16-byte aligned");
    const long long M = (long long)p->n * p->ho * p->wo, K = (long long)p->kh * p->kw * p->cin;
    // (32-bit offsets inside one image and 32-bit pixel counts in the kernel)
    OSR_REQUIRE(M <= (1ll << 30) && K <= (1ll << 30) && p->in_stride_n < (1ll << 31) && p->in_stride_h < (1ll << 31) && p->out_stride_h < (1ll << 31) &&
                    p->out_stride_w < (1ll << 31) && p->res_stride_h < (1ll << 31) && p->res_stride_w < (1ll << 31) && p->hi < (1 << 28) && p->wi < (1 << 28),
                OSR_ERR_UNSUPPORTED, "osr_conv2d_split_fwd: problem too large");
    ConvSplitArgs a;
    a.in = in; a.w0 = (const bf16_t*)w_hi; a.w1 = (const bf16_t*)w_lo; a.bias = bias; a.res = residual; a.out = out;
    a.in_stride_n = p->in_stride_n; a.out_stride_n = p->out_stride_n; a.res_stride_n = p->res_stride_n;
    a.in_stride_h = (int)p->in_stride_h; a.in_stride_w = (int)p->in_stride_w;
    a.out_stride_h = (int)p->out_stride_h; a.out_stride_w = (int)p->out_stride_w;
    a.res_stride_h = (int)p->res_stride_h; a.res_stride_w = (int)p->res_stride_w;
    // (the stem view holds its own halo: every tap of a live row is inside the buffer, so the bounds are those of the buffer)
    a.hi = p->hi; a.wi = stem ? (int)(p->in_stride_h / p->in_stride_w) : p->wi;
    a.cin = p->cin; a.ho = p->ho; a.wo = p->wo; a.cout = p->cout; a.kw = p->kw;
    a.stride_h = p->stride_h; a.stride_w = p->stride_w; a.pad_h = p->pad_h; a.pad_w = p->pad_w;
    a.relu = p->relu; a.res_mode = p->res_mode;
    a.m = (int)M; a.k = (int)K;
    return p->cout == 64 ? conv_split_launch<1>(a, (hipStream_t)stream) : conv_split_launch<2>(a, (hipStream_t)stream);
}
