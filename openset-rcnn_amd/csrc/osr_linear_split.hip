// Split-precision fully connected layer (include/osr.h: osr_linear_split_fwd, osr_split_rows_bf16): fp32 rows times fp32 weights
// at fp32 quality on the bf16 matrix instruction. The layer's data gradient (osr_linear_split_dgrad, osr_split_rows_bf16_t) is the same
// kernel with another epilogue; its weight gradient is csrc/osr_linear_split_bwd.hip.
//
// FastRCNNConvFCHead fc1 / fc2 (osrcnn_roi_heads.py:308) with the reference's fp32 operands. Every fp32 value is the sum of
// two bf16 terms to 2^-17 of its magnitude (bf16 has fp32's exponent range: no scaling, no exponents, no range cases):
//     x = x0 + x1,  W = w0 + w1        x0 = bf16(x), x1 = bf16(x - x0)
//     acc = x0 w0 + x1 w0 + x0 w1      three v_mfma_f32_32x32x16_bf16 per K step into ONE fp32 accumulator tile
// (the x1 w1 term, <= 2^-16 of the product, is dropped). The weights are static and arrive split (two bf16 planes); the rows are
// dynamic and are split on the way from global memory to LDS: fp32 loads -> registers -> two bf16 LDS tiles.
//
// Tile: 128 x 128 x 32 per 256-thread workgroup (2 x 2 waves, 64 x 64 per wave), the K loop of conv_igemm_kernel
// (osr_conv_gemm.hip): LDS double buffer with 80-byte rows (conflict-free ds_read_b128 of the 32x32x16 fragments), the next two K
// slices prefetched into registers behind the current slice's 24 MFMAs per wave, one barrier per K step. Four LDS tiles per
// stage (x0, x1, w0, w1: 40 KB), 80 KB in all: two workgroups per CU. No split-K and no atomics: one workgroup owns an output
// tile and sums K in order, so a launch is bitwise reproducible.
//
// Workgroup order: consecutive workgroup ids land on different XCDs (round robin over 8), each with its own L2. The ids are
// re-mapped so that one XCD walks the column tiles of one row tile after the other: the eight column tiles that share a slice
// of x (the large operand, 4 bytes per element) meet in one L2 instead of fetching it eight times.
#include "osr_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef bf16_t bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define LS_BM 128
#define LS_BN 128
#define LS_BK 32
#define LS_ROWB 80  // LDS bytes per tile row: 64 data + 16 pad
#define LS_TILE (LS_BM * LS_ROWB)
#define LS_STAGE (4 * LS_TILE)  // x0, x1, w0, w1
#define LS_LDS (2 * LS_STAGE)
#define LS_XCDS 8
static_assert(LS_BM == LS_BN, "one tile size for the four LDS tiles");

struct LinearSplitArgs {
    const float* x;
    const bf16_t* w0;
    const bf16_t* w1;
    const float* bias;
    float* out;
    const int* seg_counts;
    long long ldx, ldo;
    int m, n, k, relu;
    int seg_rows, tiles_m, tiles_n, per_xcd;
    const float* mask;  // DGRAD only (may be null): out is exactly 0 where mask <= 0
    long long ldmask;
};

// DGRAD: the same contraction as the data gradient of the layer (osr_linear_split_dgrad): x = dy (m, n_layer), the weight planes those
// of W^T (k_layer, n_layer), no bias, and the ReLU mask of the layer below in the epilogue. The K loop is the forward's, instruction for
// instruction.
template <bool DGRAD>
__global__ __launch_bounds__(256) void linear_split_kernel(LinearSplitArgs a) {
    constexpr int TM = 2, TN = 2;                     // 32 x 32 accumulator tiles per wave
    constexpr int A_CH = LS_BM * 8 / 256;             // float4 chunks of x per thread per K step (8 per row)
    constexpr int B_CH = LS_BN * 4 / 256;             // 16-byte chunks of one weight plane per thread per K step (4 per row)
    constexpr int EPI_LD = TN * 32 + 4;               // floats per staged row
    static_assert(4 * 32 * EPI_LD * 4 <= LS_LDS, "epilogue slabs fit the K loop's LDS");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    // workgroup id -> tile: XCD (id % 8) takes the contiguous range [xcd * per_xcd, (xcd + 1) * per_xcd) of the row-major tile list
    const int logical = (int)(blockIdx.x % LS_XCDS) * a.per_xcd + (int)(blockIdx.x / LS_XCDS);
    if (logical >= a.tiles_m * a.tiles_n) return;
    const int tile_n = logical % a.tiles_n, tile_m = logical / a.tiles_n;
    const int m0 = tile_m * LS_BM, n0 = tile_n * LS_BN;
    if (a.seg_counts) {  // padded per-image lists: a tile without a single data row has nothing to do (workgroup-uniform)
        const int sr = a.seg_rows, mend = min(m0 + LS_BM, a.m);
        bool any = false;
        for (int sg = m0 / sr; sg * sr < mend; ++sg) {
            const int lo = max(m0, sg * sr), hi = sg * sr + a.seg_counts[sg];
            any |= min(hi, mend) > lo;
        }
        if (!any) return;
    }

    const float* __restrict__ x = a.x;
    const bf16_t* __restrict__ w0 = a.w0;
    const bf16_t* __restrict__ w1 = a.w1;

    // ---- per-thread load descriptors (fixed over the K loop). Rows are independent in x W^T: output (r, c) reads row r of x and
    //      row c of W and nothing else. So a tile row beyond m (a weight row beyond n) loads row 0 in its place -- memory that
    //      exists -- and what it computes is never stored; and a padding row inside a live tile is read as it lies: whatever it
    //      holds (uninitialised memory, NaN) stays in its own output row. No load is masked, so none is waited for before the
    //      K step's MFMAs. ----
    long long a_off[A_CH], b_off[B_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int q = tid + 256 * i, row = q >> 3;
        a_off[i] = (long long)(m0 + row < a.m ? m0 + row : 0) * a.ldx + (q & 7) * 4;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        const int q = tid + 256 * i, row = q >> 2;
        b_off[i] = (long long)(n0 + row < a.n ? n0 + row : 0) * a.k + (q & 3) * 8;
    }

    // two register sets: while K slice ks is multiplied out of LDS, slice ks + 1 sits in one set (its loads were issued a whole K
    // step ago) and the loads of slice ks + 2 are issued into the other -- a load has two K steps (48 MFMAs per wave) to land
    float4 raE[A_CH], raO[A_CH];
    u32x4 rb0E[B_CH], rb1E[B_CH], rb0O[B_CH], rb1O[B_CH];

    // (macros, not lambdas: by-reference captures of the register arrays would force them into scratch)
#define LS_LOAD_TILES(ra, rb0, rb1, kflat)                                                       \
    {                                                                                            \
        _Pragma("unroll") for (int i = 0; i < A_CH; ++i)                                         \
            ra[i] = *reinterpret_cast<const float4*>(x + a_off[i] + (kflat));                    \
        _Pragma("unroll") for (int i = 0; i < B_CH; ++i) {                                       \
            rb0[i] = *reinterpret_cast<const u32x4*>(w0 + b_off[i] + (kflat));                   \
            rb1[i] = *reinterpret_cast<const u32x4*>(w1 + b_off[i] + (kflat));                   \
        }                                                                                        \
    }
    // the split of the activation rows: x0 = bf16(x) (round to nearest even), x1 = bf16(x - x0) (the subtraction is exact)
#define LS_STORE_TILES(buf, ra, rb0, rb1)                                                        \
    {                                                                                            \
        unsigned char* s_ = lds + (buf) * LS_STAGE;                                              \
        _Pragma("unroll") for (int i = 0; i < A_CH; ++i)                                         \
            asm volatile("" : "+v"(ra[i].x), "+v"(ra[i].y), "+v"(ra[i].z), "+v"(ra[i].w));      \
        _Pragma("unroll") for (int i = 0; i < A_CH; ++i) {                                       \
            const int q = tid + 256 * i;                                                         \
            const float v[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};                             \
            bf16x4 h, l;                                                                         \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                      \
                h[e] = (bf16_t)v[e];                                                             \
                l[e] = (bf16_t)(v[e] - (float)h[e]);                                             \
            }                                                                                    \
            *reinterpret_cast<bf16x4*>(s_ + (q >> 3) * LS_ROWB + (q & 7) * 8) = h;               \
            *reinterpret_cast<bf16x4*>(s_ + LS_TILE + (q >> 3) * LS_ROWB + (q & 7) * 8) = l;     \
        }                                                                                        \
        _Pragma("unroll") for (int i = 0; i < B_CH; ++i) {                                       \
            const int q = tid + 256 * i;                                                         \
            *reinterpret_cast<u32x4*>(s_ + 2 * LS_TILE + (q >> 2) * LS_ROWB + (q & 3) * 16) = rb0[i]; \
            *reinterpret_cast<u32x4*>(s_ + 3 * LS_TILE + (q >> 2) * LS_ROWB + (q & 3) * 16) = rb1[i]; \
        }                                                                                        \
    }
    // one K slice out of LDS stage buf: per 16 columns of K, x0 w1 and x1 w0 (the small terms) first, x0 w0 last
#define LS_MULTIPLY(buf)                                                                         \
    {                                                                                            \
        const unsigned char* s = lds + (buf) * LS_STAGE;                                         \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                       \
            bf16x8 fa0[TM], fa1[TM], fb0[TN], fb1[TN];                                           \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                     \
                const int off = ((wr * TM + i) * 32 + (lane & 31)) * LS_ROWB + kk * 32 + (lane >> 5) * 16; \
                fa0[i] = *reinterpret_cast<const bf16x8*>(s + off);                              \
                fa1[i] = *reinterpret_cast<const bf16x8*>(s + LS_TILE + off);                    \
            }                                                                                    \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                     \
                const int off = ((wc * TN + j) * 32 + (lane & 31)) * LS_ROWB + kk * 32 + (lane >> 5) * 16; \
                fb0[j] = *reinterpret_cast<const bf16x8*>(s + 2 * LS_TILE + off);                \
                fb1[j] = *reinterpret_cast<const bf16x8*>(s + 3 * LS_TILE + off);                \
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

    // k is a multiple of 64: an even number (>= 2) of K slices, two per trip -- even slices through register set E and LDS
    // stage 0, odd ones through set O and stage 1
    const int nk = a.k / LS_BK;
    LS_LOAD_TILES(raE, rb0E, rb1E, 0);
    LS_LOAD_TILES(raO, rb0O, rb1O, LS_BK);
    LS_STORE_TILES(0, raE, rb0E, rb1E);
    __syncthreads();
    // (no branch around a load or a store: the wait counters are set at compile time, and a load that may or may not have been
    // issued makes every later wait a wait for all of them. The last trip re-loads the last slice and stores it where nothing
    // reads it any more.)
    // (the scheduling fences, and the empty asm that LS_STORE_TILES passes the loaded rows through, keep the three phases of a K
    // step in program order: left alone, the compiler moves the split of a slice up in front of the MFMAs or to its loads --
    // fewer live registers -- and so waits for loads that should have had the MFMAs' time to land.)
    const int klast = a.k - LS_BK;
    for (int ks = 0; ks < nk; ks += 2) {
        LS_LOAD_TILES(raE, rb0E, rb1E, min((ks + 2) * LS_BK, klast));
        __builtin_amdgcn_sched_barrier(0);
        LS_MULTIPLY(0);
        __builtin_amdgcn_sched_barrier(0);
        LS_STORE_TILES(1, raO, rb0O, rb1O);
        __syncthreads();
        LS_LOAD_TILES(raO, rb0O, rb1O, min((ks + 3) * LS_BK, klast));
        __builtin_amdgcn_sched_barrier(0);
        LS_MULTIPLY(1);
        __builtin_amdgcn_sched_barrier(0);
        LS_STORE_TILES(0, raE, rb0E, rb1E);
        __syncthreads();
    }
#undef LS_LOAD_TILES
#undef LS_STORE_TILES
#undef LS_MULTIPLY

    // ---- epilogue: acc -> wave-private LDS slab (32 rows x 64 fp32) -> bias + ReLU on 8 columns per lane, coalesced row stores ----
    float* slab = reinterpret_cast<float*>(lds) + wid * 32 * EPI_LD;
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
        const int co = n0 + wc * TN * 32 + cseg;
#pragma unroll
        for (int pass = 0; pass < 32 / RPP; ++pass) {
            const int row = pass * RPP + lane / LPR;
            const int m = m0 + (wr * TM + i) * 32 + row;
            if (m < a.m && co < a.n) {
                const float4 v0 = *reinterpret_cast<const float4*>(slab + row * EPI_LD + cseg);
                const float4 v1 = *reinterpret_cast<const float4*>(slab + row * EPI_LD + cseg + 4);
                float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                if constexpr (DGRAD) {
                    if (a.mask) {  // the saved forward output of the layer below: its ReLU passed nothing where it is <= 0
                        const float4 k0 = *reinterpret_cast<const float4*>(a.mask + (long long)m * a.ldmask + co);
                        const float4 k1 = *reinterpret_cast<const float4*>(a.mask + (long long)m * a.ldmask + co + 4);
                        const float k[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = k[e] > 0.f ? v[e] : 0.f;
                    }
                } else {
                    const float4 b0 = *reinterpret_cast<const float4*>(a.bias + co);
                    const float4 b1 = *reinterpret_cast<const float4*>(a.bias + co + 4);
                    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
                    v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
                    if (a.relu) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : (v[e] == v[e] ? 0.f : v[e]);  // (a NaN stays a NaN)
                    }
                }
                float* o = a.out + (long long)m * a.ldo + co;
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// w (rows, cols) fp32 -> the two bf16 planes of the split, element by element (host/weights.py split_fp32_rows states the format)
__global__ __launch_bounds__(256) void split_rows_bf16_kernel(const float* __restrict__ w, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, long long count) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float v = w[i];
    const bf16_t h = (bf16_t)v;
    hi[i] = h;
    lo[i] = (bf16_t)(v - (float)h);
}

extern "C" osr_status osr_split_rows_bf16(const float* w, int32_t rows, int32_t cols, void* hi, void* lo, void* stream) {
    OSR_REQUIRE(w && hi && lo, OSR_ERR_INVALID_ARG, "osr_split_rows_bf16: null pointer");
    OSR_REQUIRE(rows >= 1 && cols >= 1, OSR_ERR_INVALID_ARG, "osr_split_rows_bf16: bad shape");
    const long long count = (long long)rows * cols;
    OSR_REQUIRE(count <= (1ll << 38), OSR_ERR_UNSUPPORTED, "osr_split_rows_bf16: matrix too large");
    hipLaunchKernelGGL(split_rows_bf16_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)hi, (bf16_t*)lo, count);
    OSR_CHECK_LAUNCH("osr_split_rows_bf16");
    return OSR_OK;
}

// w (rows, cols) fp32 -> the two bf16 planes of its transpose (cols, rows): 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void split_rows_bf16_t_kernel(const float* __restrict__ w, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int rows, int cols) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 8 * i][tx] = w[(long long)r * cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < rows && c < cols) {
            const float v = tile[tx][ty + 8 * i];
            const bf16_t h = (bf16_t)v;
            hi[(long long)c * rows + r] = h;
            lo[(long long)c * rows + r] = (bf16_t)(v - (float)h);
        }
    }
}

extern "C" osr_status osr_split_rows_bf16_t(const float* w, int32_t rows, int32_t cols, void* hi, void* lo, void* stream) {
    OSR_REQUIRE(w && hi && lo, OSR_ERR_INVALID_ARG, "osr_split_rows_bf16_t: null pointer");
    OSR_REQUIRE(rows >= 1 && cols >= 1, OSR_ERR_INVALID_ARG, "osr_split_rows_bf16_t: bad shape");
    OSR_REQUIRE((rows + 31) / 32 <= 65535, OSR_ERR_UNSUPPORTED, "osr_split_rows_bf16_t: too many rows");
    hipLaunchKernelGGL(split_rows_bf16_t_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, (hipStream_t)stream, w,
                       (bf16_t*)hi, (bf16_t*)lo, rows, cols);
    OSR_CHECK_LAUNCH("osr_split_rows_bf16_t");
    return OSR_OK;
}

extern "C" osr_status osr_linear_split_fwd(const osr_linear_split_params* p, const float* x, const void* w_hi, const void* w_lo, const float* bias,
                                           float* out, void* stream) {
    OSR_REQUIRE(p && x && w_hi && w_lo && bias && out, OSR_ERR_INVALID_ARG, "osr_linear_split_fwd: null pointer");
    OSR_REQUIRE(p->m >= 1 && p->n >= 1 && p->k >= 1, OSR_ERR_INVALID_ARG, "osr_linear_split_fwd: bad shape");
    OSR_REQUIRE(p->k % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_linear_split_fwd: k must be a multiple of 64, got %d", p->k);
    OSR_REQUIRE(p->n % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_linear_split_fwd: n must be a multiple of 64, got %d", p->n);
    OSR_REQUIRE(p->ldx >= p->k && p->ldx % 4 == 0 && p->ldo >= p->n && p->ldo % 4 == 0, OSR_ERR_INVALID_ARG, "osr_linear_split_fwd: bad leading dimensions");
    OSR_REQUIRE(!p->row_seg_counts || p->row_seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_linear_split_fwd: row_seg_rows must be positive with row_seg_counts");
    OSR_REQUIRE((((uintptr_t)x | (uintptr_t)w_hi | (uintptr_t)w_lo | (uintptr_t)bias | (uintptr_t)out) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_linear_split_fwd: pointers must be 16-byte aligned");
    OSR_REQUIRE(p->m <= (1 << 30), OSR_ERR_UNSUPPORTED, "osr_linear_split_fwd: m too large");
    LinearSplitArgs a;
    a.x = x; a.w0 = (const bf16_t*)w_hi; a.w1 = (const bf16_t*)w_lo; a.bias = bias; a.out = out;
    a.seg_counts = p->row_seg_counts; a.seg_rows = p->row_seg_rows; a.mask = nullptr; a.ldmask = 0;
    a.ldx = p->ldx; a.ldo = p->ldo; a.m = p->m; a.n = p->n; a.k = p->k; a.relu = p->relu;
    a.tiles_m = (p->m + LS_BM - 1) / LS_BM;
    a.tiles_n = (p->n + LS_BN - 1) / LS_BN;
    const long long tiles = (long long)a.tiles_m * a.tiles_n;
    OSR_REQUIRE(tiles <= (1ll << 30), OSR_ERR_UNSUPPORTED, "osr_linear_split_fwd: problem too large");
    a.per_xcd = (int)((tiles + LS_XCDS - 1) / LS_XCDS);
    static osr_dev_mask mask{0};
    osr_once_per_device(mask, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(linear_split_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS); });
    hipLaunchKernelGGL(linear_split_kernel<false>, dim3((unsigned)(a.per_xcd * LS_XCDS)), dim3(256), LS_LDS, (hipStream_t)stream, a);
    OSR_CHECK_LAUNCH("osr_linear_split_fwd");
    return OSR_OK;
}

// dx (m, k) = (dy (m, n) . W (n, k)) masked: the forward's contraction with dy as the rows and the planes of W^T (k, n) as the weight
extern "C" osr_status osr_linear_split_dgrad(const float* dy, int64_t lddy, const void* wt_hi, const void* wt_lo, const float* mask, int64_t ldmask,
                                             float* dx, int64_t lddx, int32_t m, int32_t n, int32_t k, const int32_t* row_seg_counts, int32_t row_seg_rows,
                                             void* stream) {
    OSR_REQUIRE(dy && wt_hi && wt_lo && dx, OSR_ERR_INVALID_ARG, "osr_linear_split_dgrad: null pointer");
    OSR_REQUIRE(m >= 1 && n >= 1 && k >= 1, OSR_ERR_INVALID_ARG, "osr_linear_split_dgrad: bad shape");
    OSR_REQUIRE(n % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_linear_split_dgrad: n must be a multiple of 64, got %d", n);
    OSR_REQUIRE(k % 64 == 0, OSR_ERR_UNSUPPORTED, "osr_linear_split_dgrad: k must be a multiple of 64, got %d", k);
    OSR_REQUIRE(lddy >= n && lddy % 4 == 0 && lddx >= k && lddx % 4 == 0 && (!mask || (ldmask >= k && ldmask % 4 == 0)), OSR_ERR_INVALID_ARG,
                "osr_linear_split_dgrad: bad leading dimensions");
    OSR_REQUIRE(!row_seg_counts || row_seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_linear_split_dgrad: row_seg_rows must be positive with row_seg_counts");
    OSR_REQUIRE((((uintptr_t)dy | (uintptr_t)wt_hi | (uintptr_t)wt_lo | (uintptr_t)mask | (uintptr_t)dx) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_linear_split_dgrad: pointers must be 16-byte aligned");
    OSR_REQUIRE(m <= (1 << 30), OSR_ERR_UNSUPPORTED, "osr_linear_split_dgrad: m too large");
    LinearSplitArgs a;
    a.x = dy; a.w0 = (const bf16_t*)wt_hi; a.w1 = (const bf16_t*)wt_lo; a.bias = nullptr; a.out = dx;
    a.seg_counts = row_seg_counts; a.seg_rows = row_seg_rows; a.mask = mask; a.ldmask = ldmask;
    a.ldx = lddy; a.ldo = lddx; a.m = m; a.n = k; a.k = n; a.relu = 0;  // (the kernel's n is its output width, its k the reduction length)
    a.tiles_m = (m + LS_BM - 1) / LS_BM;
    a.tiles_n = (k + LS_BN - 1) / LS_BN;
    const long long tiles = (long long)a.tiles_m * a.tiles_n;
    OSR_REQUIRE(tiles <= (1ll << 30), OSR_ERR_UNSUPPORTED, "osr_linear_split_dgrad: problem too large");
    a.per_xcd = (int)((tiles + LS_XCDS - 1) / LS_XCDS);
    static osr_dev_mask once{0};
    osr_once_per_device(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(linear_split_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS); });
    hipLaunchKernelGGL(linear_split_kernel<true>, dim3((unsigned)(a.per_xcd * LS_XCDS)), dim3(256), LS_LDS, (hipStream_t)stream, a);
    OSR_CHECK_LAUNCH("osr_linear_split_dgrad");
    return OSR_OK;
}
