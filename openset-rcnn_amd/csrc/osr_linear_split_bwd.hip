// Weight gradient of the split-precision fully connected layer (include/osr.h: osr_linear_split_wgrad):
//     dW[n][k] = sum_r dy[r][n] * x[r][k]          dy (m, n), x (m, k), dW (n, k), all fp32 row-major
// at fp32 quality on the bf16 matrix instruction. Both operands are dynamic, so both are split on their way from global memory to
// LDS exactly as osr_linear_split_fwd splits its rows: v0 = bf16(v), v1 = bf16(v - v0), round to nearest even, and each step sums
//     dy0 x0 + dy1 x0 + dy0 x1                      three v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator tile
// (the dy1 x1 term is dropped).
//
// The reduction axis r is the slow axis of both operands, and the MFMA wants it contiguous per lane: the tiles are transposed while
// they are staged. A thread loads the same four columns of four consecutive rows (4 x float4 per operand: a wave reads whole 128-byte
// lines), splits them, and writes per column the four rows' terms as ONE 8-byte LDS store. The LDS image is the forward's: one tile row
// per output row / column (128 of them), 32 reduction steps x bf16 = 64 bytes + 16 pad, so the K loop's ds_read_b128 fragment reads are
// the forward's, conflict-free. The stores: 16 contiguous lanes (8 row groups x 2 column groups, 80 dwords apart) cover the 32 banks
// once.
//
// Tile 128 (n) x 128 (k) x 32 (rows) per 256-thread workgroup, 2 x 2 waves, LDS double buffer (80 KB: two workgroups per CU), the next
// two row slices prefetched into registers behind the current slice's 24 MFMAs per wave -- the forward's pipeline. Rows that take no
// part (beyond m, beyond this workgroup's share of the rows, padding of a per-image list) are loaded from a row that exists and
// replaced by zeros when they are split: no load is masked, and nothing a padding row holds (NaN) reaches dW.
//
// A layer with few output tiles (FC2: 64) cuts the row axis over workgroups: every cut writes its partial tile to the caller's
// workspace and a second launch adds the partials in cut order. No atomics: a launch is bitwise reproducible.
#include "osr_common.h"

#include <algorithm>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));

#define LW_BT 128   // tile side (output rows = columns of dy, output columns = columns of x)
#define LW_BR 32    // rows of dy / x per step
#define LW_ROWB 80  // LDS bytes per tile row: 64 data + 16 pad
#define LW_TILE (LW_BT * LW_ROWB)
#define LW_STAGE (4 * LW_TILE)  // dy0, dy1, x0, x1
#define LW_LDS (2 * LW_STAGE)
#define LW_XCDS 8
#define LW_SLOTS 512      // workgroups the device holds at once (256 CUs x 2)
#define LW_MAX_SPLITS 16

struct LinearSplitWgradArgs {
    const float* dy;
    const float* x;
    float* out;  // dW, or the partial tiles (splits, n, k) in the workspace
    const int* seg_counts;
    long long lddy, ldx, ldo, split_stride;
    int m, n, k, seg_rows;
    int tiles_n, tiles_k, splits, slices_per_split, per_xcd;
};

template <bool SEG>
__global__ __launch_bounds__(256) void linear_split_wgrad_kernel(LinearSplitWgradArgs a) {
    constexpr int TM = 2, TN = 2;         // 32 x 32 accumulator tiles per wave
    constexpr int EPI_LD = TN * 32 + 4;   // floats per staged row
    static_assert(4 * 32 * EPI_LD * 4 <= LW_LDS, "epilogue slabs fit the K loop's LDS");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    // workgroup id -> (cut, k tile, n tile), n tile fastest: one XCD (id % 8) walks a contiguous range of that list, so the workgroups
    // that share a column slice of x, and all of them the slice of dy, meet in one L2
    const int logical = (int)(blockIdx.x % LW_XCDS) * a.per_xcd + (int)(blockIdx.x / LW_XCDS);
    if (logical >= a.tiles_n * a.tiles_k * a.splits) return;
    const int tile_n = logical % a.tiles_n, rest = logical / a.tiles_n;
    const int tile_k = rest % a.tiles_k, split = rest / a.tiles_k;
    const int n0 = tile_n * LW_BT, k0 = tile_k * LW_BT;
    const int s_begin = split * a.slices_per_split;
    const int r_end = min(a.m, (s_begin + a.slices_per_split) * LW_BR);  // this workgroup sums rows [s_begin * 32, r_end)
    const int nk = ((r_end - s_begin * LW_BR + LW_BR - 1) / LW_BR + 1) & ~1;  // slices, rounded up to even: the slice beyond is all zeros

    const float* __restrict__ dy = a.dy;
    const float* __restrict__ x = a.x;
    const int* __restrict__ segc = a.seg_counts;

    // thread -> rows 4 rg .. 4 rg + 3 of the slice, columns 4 cg .. 4 cg + 3 of the tile. A column group beyond the matrix (n, k are
    // multiples of 64, the tile is 128) reads the tile's first columns instead; what it computes is never stored.
    const int rg = tid & 7, cg = tid >> 3;
    const long long a_col = n0 + (n0 + cg * 4 < a.n ? cg * 4 : 0);
    const long long b_col = k0 + (k0 + cg * 4 < a.k ? cg * 4 : 0);
    const int m_last = a.m - 1, seg_rows = a.seg_rows;

    float4 raE[4], rbE[4], raO[4], rbO[4];
    [[maybe_unused]] int limE[4], limO[4];  // SEG: the data rows of the row's segment (its image's list)

#define LW_LOAD_TILES(ra, rb, lim, sl)                                                           \
    {                                                                                            \
        const int rbase_ = (s_begin + (sl)) * LW_BR + rg * 4;                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                          \
            const int rc_ = min(rbase_ + i, m_last);                                             \
            ra[i] = *reinterpret_cast<const float4*>(dy + (long long)rc_ * a.lddy + a_col);      \
            rb[i] = *reinterpret_cast<const float4*>(x + (long long)rc_ * a.ldx + b_col);        \
            if constexpr (SEG) lim[i] = segc[rc_ / seg_rows];                                    \
        }                                                                                        \
    }
    // the split, with the rows that take no part replaced by zeros, and the transposition: per column the four rows' terms as 8 bytes
#define LW_STORE_TILES(buf, ra, rb, lim, sl)                                                     \
    {                                                                                            \
        unsigned char* s_ = lds + (buf) * LW_STAGE + (cg * 4) * LW_ROWB + rg * 8;                \
        const int rbase_ = (s_begin + (sl)) * LW_BR + rg * 4;                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                            \
            asm volatile("" : "+v"(ra[i].x), "+v"(ra[i].y), "+v"(ra[i].z), "+v"(ra[i].w),       \
                              "+v"(rb[i].x), "+v"(rb[i].y), "+v"(rb[i].z), "+v"(rb[i].w));      \
        float va_[4][4], vb_[4][4];                                                              \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                          \
            const int r_ = rbase_ + i;                                                           \
            bool ok_ = r_ < r_end;                                                               \
            if constexpr (SEG) ok_ = ok_ && (r_ % seg_rows) < lim[i];                            \
            va_[i][0] = ok_ ? ra[i].x : 0.f; va_[i][1] = ok_ ? ra[i].y : 0.f;                    \
            va_[i][2] = ok_ ? ra[i].z : 0.f; va_[i][3] = ok_ ? ra[i].w : 0.f;                    \
            vb_[i][0] = ok_ ? rb[i].x : 0.f; vb_[i][1] = ok_ ? rb[i].y : 0.f;                    \
            vb_[i][2] = ok_ ? rb[i].z : 0.f; vb_[i][3] = ok_ ? rb[i].w : 0.f;                    \
        }                                                                                        \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                          \
            bf16x4 ah, al, bh, bl;                                                               \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                      \
                ah[i] = (bf16_t)va_[i][e];                                                       \
                al[i] = (bf16_t)(va_[i][e] - (float)ah[i]);                                      \
                bh[i] = (bf16_t)vb_[i][e];                                                       \
                bl[i] = (bf16_t)(vb_[i][e] - (float)bh[i]);                                      \
            }                                                                                    \
            *reinterpret_cast<bf16x4*>(s_ + e * LW_ROWB) = ah;                                   \
            *reinterpret_cast<bf16x4*>(s_ + LW_TILE + e * LW_ROWB) = al;                         \
            *reinterpret_cast<bf16x4*>(s_ + 2 * LW_TILE + e * LW_ROWB) = bh;                     \
            *reinterpret_cast<bf16x4*>(s_ + 3 * LW_TILE + e * LW_ROWB) = bl;                     \
        }                                                                                        \
    }
    // one row slice out of LDS stage buf: per 16 rows, dy0 x1 and dy1 x0 (the small terms) first, dy0 x0 last
#define LW_MULTIPLY(buf)                                                                         \
    {                                                                                            \
        const unsigned char* s = lds + (buf) * LW_STAGE;                                         \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                       \
            bf16x8 fa0[TM], fa1[TM], fb0[TN], fb1[TN];                                           \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                     \
                const int off = ((wr * TM + i) * 32 + (lane & 31)) * LW_ROWB + kk * 32 + (lane >> 5) * 16; \
                fa0[i] = *reinterpret_cast<const bf16x8*>(s + off);                              \
                fa1[i] = *reinterpret_cast<const bf16x8*>(s + LW_TILE + off);                    \
            }                                                                                    \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                     \
                const int off = ((wc * TN + j) * 32 + (lane & 31)) * LW_ROWB + kk * 32 + (lane >> 5) * 16; \
                fb0[j] = *reinterpret_cast<const bf16x8*>(s + 2 * LW_TILE + off);                \
                fb1[j] = *reinterpret_cast<const bf16x8*>(s + 3 * LW_TILE + off);                \
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

    // two slices per trip: even ones through register set E and LDS stage 0, odd ones through set O and stage 1. A slice index
    // beyond nk loads the clamped last row and splits to zeros (its rows are >= r_end); it lands in a stage nothing reads any more.
    LW_LOAD_TILES(raE, rbE, limE, 0);
    LW_LOAD_TILES(raO, rbO, limO, 1);
    LW_STORE_TILES(0, raE, rbE, limE, 0);
    __syncthreads();
    for (int ks = 0; ks < nk; ks += 2) {
        LW_LOAD_TILES(raE, rbE, limE, ks + 2);
        __builtin_amdgcn_sched_barrier(0);
        LW_MULTIPLY(0);
        __builtin_amdgcn_sched_barrier(0);
        LW_STORE_TILES(1, raO, rbO, limO, ks + 1);
        __syncthreads();
        LW_LOAD_TILES(raO, rbO, limO, ks + 3);
        __builtin_amdgcn_sched_barrier(0);
        LW_MULTIPLY(1);
        __builtin_amdgcn_sched_barrier(0);
        LW_STORE_TILES(0, raE, rbE, limE, ks + 2);
        __syncthreads();
    }
#undef LW_LOAD_TILES
#undef LW_STORE_TILES
#undef LW_MULTIPLY

    // ---- epilogue: acc -> wave-private LDS slab (32 rows x 64 fp32) -> coalesced row stores of 8 columns per lane ----
    float* slab = reinterpret_cast<float*>(lds) + wid * 32 * EPI_LD;
    float* __restrict__ out = a.out + (long long)split * a.split_stride;
    constexpr int LPR = TN * 4;    // lanes per staged row (8 columns each)
    constexpr int RPP = 64 / LPR;  // rows per pass
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
        const int cseg = (lane % LPR) * 8;
        const int co = k0 + wc * TN * 32 + cseg;
#pragma unroll
        for (int pass = 0; pass < 32 / RPP; ++pass) {
            const int row = pass * RPP + lane / LPR;
            const int nr = n0 + (wr * TM + i) * 32 + row;
            if (nr < a.n && co < a.k) {
                float* o = out + (long long)nr * a.ldo + co;
                *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(slab + row * EPI_LD + cseg);
                *reinterpret_cast<float4*>(o + 4) = *reinterpret_cast<const float4*>(slab + row * EPI_LD + cseg + 4);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// dW = the partial tiles added in cut order (4 elements per thread)
__global__ __launch_bounds__(256) void linear_split_wgrad_reduce(const float* __restrict__ part, long long split_stride, int splits, float* __restrict__ dw,
                                                                 long long lddw, int n, int k) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const int kq = k / 4;
    if (q >= (long long)n * kq) return;
    const long long row = q / kq, col = (q % kq) * 4;
    const float* p = part + row * k + col;
    float4 s = *reinterpret_cast<const float4*>(p);
    for (int i = 1; i < splits; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(p + i * split_stride);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(dw + row * lddw + col) = s;
}

// how many cuts of the row axis: as many as fill the device once, each at least four slices long
static int wgrad_splits(int m, int n, int k) {
    const long long tiles = (long long)((n + LW_BT - 1) / LW_BT) * ((k + LW_BT - 1) / LW_BT);
    const int slices = (m + LW_BR - 1) / LW_BR;
    long long s = LW_SLOTS / tiles;
    s = std::min<long long>(s, std::min(LW_MAX_SPLITS, slices / 4));
    return (int)std::max<long long>(s, 1);
}

extern "C" int64_t osr_linear_split_wgrad_workspace_bytes(int32_t m, int32_t n, int32_t k) {
    if (m <= 0 || n <= 0 || k <= 0) return 0;
    const int s = wgrad_splits(m, n, k);
    return s > 1 ? (int64_t)s * n * k * 4 : 0;
}

extern "C" osr_status osr_linear_split_wgrad(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dw, int64_t lddw, int32_t m, int32_t n,
                                             int32_t k, const int32_t* row_seg_counts, int32_t row_seg_rows, void* workspace, int64_t workspace_bytes,
                                             void* stream) {
    OSR_REQUIRE(dy && x && dw, OSR_ERR_INVALID_ARG, "osr_linear_split_wgrad: null pointer");
    OSR_REQUIRE(m >= 1 && n >= 1 && k >= 1, OSR_ERR_INVALID_ARG, "osr_linear_split_wgrad: bad shape");
    OSR_REQUIRE(n % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_linear_split_wgrad: n must be a multiple of 64, got %d", n);
    OSR_REQUIRE(k % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_linear_split_wgrad: k must be a multiple of 64, got %d", k);
    OSR_REQUIRE(lddy >= n && lddy % 4 == 0 && ldx >= k && ldx % 4 == 0 && lddw >= k && lddw % 4 == 0, OSR_ERR_INVALID_ARG,
                "osr_linear_split_wgrad: bad leading dimensions");
    OSR_REQUIRE(!row_seg_counts || row_seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_linear_split_wgrad: row_seg_rows must be positive with row_seg_counts");
    OSR_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)workspace) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_linear_split_wgrad: pointers must be 16-byte aligned");
    OSR_REQUIRE(m <= (1 << 30), OSR_ERR_UNSUPPORTED, "osr_linear_split_wgrad: m too large");
    LinearSplitWgradArgs a;
    a.dy = dy; a.x = x; a.seg_counts = row_seg_counts; a.seg_rows = row_seg_counts ? row_seg_rows : 1;
    a.lddy = lddy; a.ldx = ldx; a.m = m; a.n = n; a.k = k;
    a.tiles_n = (n + LW_BT - 1) / LW_BT;
    a.tiles_k = (k + LW_BT - 1) / LW_BT;
    const int slices = (m + LW_BR - 1) / LW_BR;
    const int64_t per = (int64_t)n * k * 4;
    int splits = wgrad_splits(m, n, k);
    if (!workspace || workspace_bytes < 2 * per) splits = 1;
    else splits = (int)std::min<int64_t>(splits, workspace_bytes / per);
    a.slices_per_split = (slices + splits - 1) / splits;
    a.splits = (slices + a.slices_per_split - 1) / a.slices_per_split;  // every cut has rows
    if (a.splits > 1) { a.out = (float*)workspace; a.ldo = k; a.split_stride = (long long)n * k; }
    else { a.out = dw; a.ldo = lddw; a.split_stride = 0; }
    const long long wgs = (long long)a.tiles_n * a.tiles_k * a.splits;
    OSR_REQUIRE(wgs <= (1ll << 30), OSR_ERR_UNSUPPORTED, "osr_linear_split_wgrad: problem too large");
    a.per_xcd = (int)((wgs + LW_XCDS - 1) / LW_XCDS);
    static osr_dev_mask once{0};
    osr_once_per_device(once, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(linear_split_wgrad_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LW_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(linear_split_wgrad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LW_LDS);
    });
    if (row_seg_counts) hipLaunchKernelGGL(linear_split_wgrad_kernel<true>, dim3((unsigned)(a.per_xcd * LW_XCDS)), dim3(256), LW_LDS, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(linear_split_wgrad_kernel<false>, dim3((unsigned)(a.per_xcd * LW_XCDS)), dim3(256), LW_LDS, (hipStream_t)stream, a);
    OSR_CHECK_LAUNCH("osr_linear_split_wgrad");
    if (a.splits > 1) {
        const long long quads = (long long)n * (k / 4);
        hipLaunchKernelGGL(linear_split_wgrad_reduce, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace,
                           a.split_stride, a.splits, dw, (long long)lddw, n, k);
        OSR_CHECK_LAUNCH("osr_linear_split_wgrad(reduce)");
    }
    return OSR_OK;
}
