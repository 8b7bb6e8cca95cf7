// Backward-data of a stride-2 3x3 convolution with pad 1 (the first block of res3-res5 when MODEL.RESNETS.STRIDE_IN_1X1 is
// False: torchvision's layout, stride in the 3x3).
//
//   dx[n, ih, iw, ci] = sum dy[n, oh, ow, co] * w[co, kh, kw, ci]  over  2*oh - 1 + kh = ih,  2*ow - 1 + kw = iw.
//
// A zero-inserted dy run through the stride-1 data gradient would spend 9 taps on every dx pixel, 3 of 4 of them on zeros. Split
// by pixel parity instead: an even ih sees only kh = 1 (oh = ih / 2), an odd ih sees kh = 0 (oh = (ih + 1) / 2) and kh = 2
// (oh = (ih - 1) / 2), and likewise for iw -- four phases of 1, 1x2, 2x1 and 2x2 taps, 9 in all. One launch covers the four:
// a workgroup takes a tile of one phase (128 of its pixels x 128 input channels) and its K loop runs over that phase's taps x cout
// only, 64 output channels of one tap per step. The heaviest phase is dispatched first.
//
// The GEMM of a tile is C[ci][pixel] = sum_k w[ci][k] * dy[pixel][k] with k = (tap, co): both operands are k-contiguous in memory
// (dy rows of cout channels, and the repacked data-gradient weights (cin, 3, 3, cout) of host/weights.py pack_dgrad_weight), staged
// row-major in LDS and read with ds_read_b128. The weight rows are placed in LDS in a permuted order so that the MFMA result a
// lane holds is 16 CONSECUTIVE input channels of one pixel: the epilogue reads the mask / addend and writes dx with 16-byte
// accesses. Every dx pixel belongs to exactly one tile and is written once (no zero fill: with pad 1 every pixel has a tap).
#include "osr_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f16_t f16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));

template <class T> struct FragS2;
template <> struct FragS2<f16_t> {
    typedef f16x8 type;
    static __device__ __forceinline__ f32x4 mfma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct FragS2<bf16_t> {
    typedef bf16x8 type;
    static __device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

#define S2_BM 128    // pixels of one phase per workgroup
#define S2_BN 128    // input channels per workgroup
#define S2_BK 64     // contraction step: 64 output channels of one tap
// LDS row pitch in elements: 160 B. ds_read_b128 serves a wave in four 16-lane groups ({0-3, 12-15, 20-27}, ...: rows 0-3 and
// 12-15 at one k offset, rows 4-11 at the next); with 10 16-byte slots per row those 16 reads land on 16 different slots of the
// 256-B bank row (a 144-B pitch puts rows r and r + 16 / r + 9 on one slot).
#define S2_PITCH 80
#define S2_THREADS 256

struct DgradS2Args {
    const void* dy;
    const void* w;     // (cin, 3, 3, cout): w[ci][2 - kh][2 - kw][co] = forward weight[co][kh][kw][ci]
    const void* mask;  // (n, hi, wi, cin) or null: dx = mask > 0 ? value : 0
    const void* add;   // (n, hi, wi, cin) or null: value = conv + add
    void* dx;          // (n, hi, wi, cin)
    int n, hi, wi, cin, ho, wo, cout;
    int tiles_ci;
    long long tile_begin[5];  // first workgroup of the phase in dispatch slot s; [4] = grid size
    int phase_of[4];          // dispatch slot -> phase (row parity * 2 + column parity)
};

template <class T> struct S2Out;
template <> struct S2Out<float> {
    static __device__ __forceinline__ void store16(float* dst, const float* v) {
#pragma unroll
        for (int q = 0; q < 4; ++q) reinterpret_cast<float4*>(dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
};
template <> struct S2Out<f16_t> {
    static __device__ __forceinline__ void store16(f16_t* dst, const float* v) {
        f16x8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] = (f16_t)v[e]; b[e] = (f16_t)v[8 + e]; }
        reinterpret_cast<f16x8*>(dst)[0] = a;
        reinterpret_cast<f16x8*>(dst)[1] = b;
    }
};
template <> struct S2Out<bf16_t> {
    static __device__ __forceinline__ void store16(bf16_t* dst, const float* v) {
        bf16x8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] = (bf16_t)v[e]; b[e] = (bf16_t)v[8 + e]; }
        reinterpret_cast<bf16x8*>(dst)[0] = a;
        reinterpret_cast<bf16x8*>(dst)[1] = b;
    }
};

template <class T, class TO>
__global__ __launch_bounds__(S2_THREADS) void conv_dgrad_s2_kernel(DgradS2Args a) {
    typedef typename FragS2<T>::type frag_t;
    typedef T t8 __attribute__((ext_vector_type(8)));
    __shared__ __attribute__((aligned(16))) T s_w[S2_BN * S2_PITCH];
    __shared__ __attribute__((aligned(16))) T s_y[S2_BM * S2_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid & 1, wn = wid >> 1;  // wave: 64 pixels (half wm of the tile) x 64 input channels (half wn)

    // ---- tile decode: dispatch slot (phase), input-channel tile, pixel tile ----
    const long long bid = blockIdx.x;
    int slot = 0;
    while (slot < 3 && bid >= a.tile_begin[slot + 1]) ++slot;
    const int phase = a.phase_of[slot], ph = phase >> 1, pw = phase & 1;
    const long long t = bid - a.tile_begin[slot];
    const int tile_ci = (int)(t % a.tiles_ci);
    const int m0 = (int)(t / a.tiles_ci) * S2_BM, ci0 = tile_ci * S2_BN;
    const int Hp = (a.hi - ph + 1) >> 1, Wp = (a.wi - pw + 1) >> 1, HWp = Hp * Wp;
    const int M = a.n * HWp;  // pixels of this phase
    const int ntw = pw ? 2 : 1, ntaps = (ph ? 2 : 1) * ntw, cpt = a.cout / S2_BK, nk = ntaps * cpt;

    // ---- staging: thread tid moves 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 q, q = 0..3, of both tiles ----
    const int kc8 = (tid & 7) * 8;
    const T* __restrict__ dy = (const T*)a.dy;
    const T* __restrict__ w = (const T*)a.w;
    int ybase[4];      // dy pixel index (n, i, j) at tap offset (0, 0), -1 past the phase's last pixel
    int ylast[4];      // bit 0: i + 1 == ho (no row below), bit 1: j + 1 == wo
    int wrow[4];       // input channel of the weight row, -1 past cin
    int lrow_w[4];     // LDS row of that weight row (permuted: see the epilogue)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (tid >> 3) + 32 * q;
        const int m = m0 + r;
        if (m < M) {
            const int ni = m / HWp, rem = m - ni * HWp, i = rem / Wp, j = rem - i * Wp;
            ybase[q] = (ni * a.ho + i) * a.wo + j;
            ylast[q] = (i + 1 >= a.ho ? 1 : 0) | (j + 1 >= a.wo ? 2 : 0);
        } else {
            ybase[q] = -1;
            ylast[q] = 3;
        }
        wrow[q] = ci0 + r < a.cin ? ci0 + r : -1;
        // input channel c = 64 h + 16 G + 4 i + e of the tile -> LDS row 64 h + 16 i + 4 G + e
        lrow_w[q] = (r & 64) | (((r >> 2) & 3) << 4) | (((r >> 4) & 3) << 2) | (r & 3);
    }
    t8 ry[4], rw[4];
    auto load = [&](int kc) {
        const int tap = kc / cpt, co0 = (kc - tap * cpt) * S2_BK;
        const int th = tap / ntw, tw = tap - th * ntw;
        // phase row parity 1: taps kh = 0 (oh = i + 1) and kh = 2 (oh = i); parity 0: kh = 1 (oh = i). Same for the columns.
        const int dh = ph ? 1 - th : 0, dw = pw ? 1 - tw : 0;
        const int kh = ph ? 2 * th : 1, kw = pw ? 2 * tw : 1;
        const int tap9 = (2 - kh) * 3 + (2 - kw);
        const int need = (dh ? 1 : 0) | (dw ? 2 : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ybase[q] >= 0 && !(ylast[q] & need))
                ry[q] = *reinterpret_cast<const t8*>(dy + (long long)(ybase[q] + dh * a.wo + dw) * a.cout + co0 + kc8);
            else
                ry[q] = t8{};
            if (wrow[q] >= 0)
                rw[q] = *reinterpret_cast<const t8*>(w + ((long long)wrow[q] * 9 + tap9) * a.cout + co0 + kc8);
            else
                rw[q] = t8{};
        }
    };

    f32x4 acc[4][4];  // [input-channel sub-tile][pixel sub-tile]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fk = (lane >> 4) * 8;
    load(0);
    for (int kc = 0; kc < nk; ++kc) {
        if (kc) __syncthreads();  // every wave is done reading the previous step
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (tid >> 3) + 32 * q;
            *reinterpret_cast<t8*>(s_y + r * S2_PITCH + kc8) = ry[q];
            *reinterpret_cast<t8*>(s_w + lrow_w[q] * S2_PITCH + kc8) = rw[q];
        }
        __syncthreads();
        if (kc + 1 < nk) load(kc + 1);  // in flight under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < S2_BK / 32; ++kk) {
            frag_t fw[4], fy[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fw[i] = *reinterpret_cast<const frag_t*>(s_w + (wn * 64 + i * 16 + fr) * S2_PITCH + kk * 32 + fk);
#pragma unroll
            for (int j = 0; j < 4; ++j) fy[j] = *reinterpret_cast<const frag_t*>(s_y + (wm * 64 + j * 16 + fr) * S2_PITCH + kk * 32 + fk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = FragS2<T>::mfma(fw[i], fy[j], acc[i][j]);
        }
    }

    // ---- epilogue. MFMA row R = 4 (lane >> 4) + e of sub-tile i is LDS weight row 64 wn + 16 i + R, i.e. input channel
    // 64 wn + 16 (lane >> 4) + 4 i + e: the lane holds 16 consecutive channels of pixel (lane & 15) of each pixel sub-tile ----
    const int cb = ci0 + wn * 64 + (lane >> 4) * 16;
    if (cb >= a.cin) return;  // (cin % 16 == 0: a lane's 16 channels are all in range or all out)
    const T* __restrict__ mk = (const T*)a.mask;
    const T* __restrict__ ad = (const T*)a.add;
    TO* __restrict__ dx = (TO*)a.dx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + fr;
        if (m >= M) continue;
        const int ni = m / HWp, rem = m - ni * HWp, i = rem / Wp, jj = rem - i * Wp;
        const long long off = ((long long)(ni * a.hi + 2 * i + ph) * a.wi + 2 * jj + pw) * a.cin + cb;
        float v[16];
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i4 * 4 + e] = acc[i4][j][e];
        if (ad) {
            const t8 a0 = reinterpret_cast<const t8*>(ad + off)[0], a1 = reinterpret_cast<const t8*>(ad + off)[1];
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[e] += (float)a0[e]; v[8 + e] += (float)a1[e]; }
        }
        if (mk) {
            const t8 k0 = reinterpret_cast<const t8*>(mk + off)[0], k1 = reinterpret_cast<const t8*>(mk + off)[1];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] = (float)k0[e] > 0.f ? v[e] : 0.f;
                v[8 + e] = (float)k1[e] > 0.f ? v[8 + e] : 0.f;
            }
        }
        S2Out<TO>::store16(dx + off, v);
    }
}

extern "C" osr_status osr_conv2d_dgrad_s2(const osr_conv_params* p, const void* dy, const void* w_dgrad, const void* mask, const void* add,
                                          void* dx, void* stream) {
    OSR_REQUIRE(p && dy && w_dgrad && dx, OSR_ERR_INVALID_ARG, "osr_conv2d_dgrad_s2: null pointer");
    OSR_REQUIRE(p->kh == 3 && p->kw == 3 && p->stride_h == 2 && p->stride_w == 2 && p->pad_h == 1 && p->pad_w == 1, OSR_ERR_UNSUPPORTED,
                "osr_conv2d_dgrad_s2: the layer must be a 3x3 convolution with stride 2 and pad 1");
    OSR_REQUIRE(p->n >= 1 && p->hi >= 1 && p->wi >= 1 && p->ho == (p->hi - 1) / 2 + 1 && p->wo == (p->wi - 1) / 2 + 1, OSR_ERR_INVALID_ARG,
                "osr_conv2d_dgrad_s2: ho/wo inconsistent with hi/wi (3x3, stride 2, pad 1)");
    OSR_REQUIRE(p->cin >= 16 && p->cin % 16 == 0 && p->cout >= 64 && p->cout % 64 == 0, OSR_ERR_UNSUPPORTED,
                "osr_conv2d_dgrad_s2: cin must be a multiple of 16 and cout a multiple of 64");
    OSR_REQUIRE(p->in_dtype == OSR_F16 || p->in_dtype == OSR_BF16, OSR_ERR_UNSUPPORTED, "osr_conv2d_dgrad_s2: dy / weights must be f16 or bf16");
    OSR_REQUIRE(p->out_dtype == p->in_dtype || p->out_dtype == OSR_F32, OSR_ERR_UNSUPPORTED, "osr_conv2d_dgrad_s2: dx must be in_dtype or f32");
    OSR_REQUIRE(p->in_stride_w == p->cin && p->in_stride_h == (int64_t)p->wi * p->cin && p->in_stride_n == (int64_t)p->hi * p->wi * p->cin &&
                    p->out_stride_w == p->cout && p->out_stride_h == (int64_t)p->wo * p->cout && p->out_stride_n == (int64_t)p->ho * p->wo * p->cout,
                OSR_ERR_UNSUPPORTED, "osr_conv2d_dgrad_s2: dx (n, hi, wi, cin) and dy (n, ho, wo, cout) must be dense");
    OSR_REQUIRE((((uintptr_t)dy | (uintptr_t)w_dgrad | (uintptr_t)mask | (uintptr_t)add | (uintptr_t)dx) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_conv2d_dgrad_s2: pointers must be 16-byte aligned");
    const long long dx_elems = (long long)p->n * p->hi * p->wi, dy_rows = (long long)p->n * p->ho * p->wo;
    OSR_REQUIRE(dx_elems < (1ll << 31) && dy_rows < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_conv2d_dgrad_s2: too many pixels for 32-bit indices");
    DgradS2Args a;
    a.dy = dy; a.w = w_dgrad; a.mask = mask; a.add = add; a.dx = dx;
    a.n = p->n; a.hi = p->hi; a.wi = p->wi; a.cin = p->cin; a.ho = p->ho; a.wo = p->wo; a.cout = p->cout;
    a.tiles_ci = (p->cin + S2_BN - 1) / S2_BN;
    // dispatch order: the 4-tap phase (odd, odd) first, then the two 2-tap phases, then the 1-tap phase
    static const int order[4] = {3, 1, 2, 0};
    long long total = 0;
    for (int s = 0; s < 4; ++s) {
        const int ph = order[s] >> 1, pw = order[s] & 1;
        const long long pix = (long long)p->n * ((p->hi - ph + 1) / 2) * ((p->wi - pw + 1) / 2);
        a.phase_of[s] = order[s];
        a.tile_begin[s] = total;
        total += (pix + S2_BM - 1) / S2_BM * a.tiles_ci;
    }
    a.tile_begin[4] = total;
    OSR_REQUIRE(total < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_conv2d_dgrad_s2: grid too large");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)total), block(S2_THREADS);
    if (p->in_dtype == OSR_F16) {
        if (p->out_dtype == OSR_F32) hipLaunchKernelGGL((conv_dgrad_s2_kernel<f16_t, float>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((conv_dgrad_s2_kernel<f16_t, f16_t>), grid, block, 0, st, a);
    } else {
        if (p->out_dtype == OSR_F32) hipLaunchKernelGGL((conv_dgrad_s2_kernel<bf16_t, float>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((conv_dgrad_s2_kernel<bf16_t, bf16_t>), grid, block, 0, st, a);
    }
    OSR_CHECK_LAUNCH("osr_conv2d_dgrad_s2");
    return OSR_OK;
}
