// The tail of [d2] KRCNNConvDeconvUpsampleHead at test time and [d2] heatmaps_to_keypoints, for gfx950 (include/osr.h:
// osr_keypoint_upsample, osr_heatmaps_to_keypoints).
//
// osr_keypoint_upsample: score_lowres = ConvTranspose2d(Cin -> K, 4 x 4, stride 2, pad 1), then bilinear x2 (align_corners=False).
// Output pixel (oy, ox) of the transposed convolution takes the taps with oy = 2 iy - 1 + ky: two per axis, and which two depends on
// the parity of oy alone. Output pixel (2a + py, 2b + px) of parity class (py, px) is therefore
//   sum over ty, tx in {0, 1} of x[a + py - ty, b + px - tx, :] . w[:, :, 1 - py + 2 ty, 1 - px + 2 tx]
// (input pixels outside the S x S map contribute nothing): a GEMM with M = S S pixels, K = 4 Cin, N = K keypoints padded to 32. One
// workgroup (4 waves) per RoI, wave p = parity class p = 2 py + px, so a wave's ceil(S S / 32) accumulator tiles (32 x 32 MFMA) hold
// one quarter of the 2S x 2S map in fp32 registers. A RoI's input (14 x 14 x 512 fp16 = 200 KB) does not fit the LDS: it is streamed
// over channels in chunks of 128 bytes per pixel (64 fp16 / bf16 channels, 32 fp32), the next chunk prefetched into registers while
// the MFMAs run on this one; the shifted A rows of a tap are LDS row offsets, a row of zeros stands for the pixels outside. The
// weights come from global memory (16 Cin 32 elements, L2-resident) in fragment order (host/weights.py pack_keypoint_deconv_weight).
// The epilogue adds the bias, lays 16 keypoints' 2S x 2S maps at a time into the LDS the stream used (fp32), and every thread
// interpolates its share of the 4S x 4S outputs: the low-resolution map never leaves the chip. The summation order is fixed: repeats
// are bit-identical.
//
// osr_heatmaps_to_keypoints: see the comment at the kernel.
#include "osr_common.h"
#include "osr_mask_mfma.h"

#define KP_CHUNK_BYTES 128                     // bytes of channels per pixel and streamed chunk
#define KP_ROWB (KP_CHUNK_BYTES + MH_PAD)      // LDS row pitch of a chunk
#define KP_MAX_S 14
#define KP_MAX_MB 7                            // ceil(14 * 14 / 32) M blocks
#define KP_HALF 16                             // keypoint maps per interpolation pass
#define KP_PF 7                                // 16-byte pieces a thread prefetches: ceil(14 * 14 * 8 / 256)

struct KpUpArgs {
    const void* x;
    const void* w;
    const float* bias;
    const int* rows_valid;
    float* out;
    int s, cin, k, seg_rows;
};

template <class T>
__global__ __launch_bounds__(256) void keypoint_upsample_kernel(KpUpArgs a) {
    typedef typename MhFrag<T>::type frag_t;
    constexpr int E = MhFrag<T>::E;
    extern __shared__ __attribute__((aligned(16))) unsigned char kp_lds[];
    const int tid = threadIdx.x, lane = tid & 63, par = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = a.s, ss = s * s, os = 2 * s, hs = 4 * s;
    const long long roi = blockIdx.x;
    float* __restrict__ out = a.out + roi * (long long)a.k * hs * hs;

    if (a.rows_valid && (int)(roi % a.seg_rows) >= a.rows_valid[roi / a.seg_rows]) {  // a RoI that does not exist: zeros, no loads
        float4* o4 = reinterpret_cast<float4*>(out);  // (k 16 s s floats per RoI: every RoI starts 16-byte aligned)
        const int n4 = a.k * hs * hs / 4;
        for (int e = tid; e < n4; e += 256) o4[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }

    const int py = par >> 1, px = par & 1;
    const int nmb = (ss + 31) >> 5;
    const float inv_s = 1.0f / (float)s;

    // byte offsets of this lane's A rows: M block i, tap t = 2 ty + tx reads input pixel (a + py - ty, b + px - tx); row ss is zeros
    int aoff[4][KP_MAX_MB];
#pragma unroll
    for (int i = 0; i < KP_MAX_MB; ++i) {
        const int m = i * 32 + (lane & 31);
        const int ya = (int)(((float)m + 0.5f) * inv_s), xb = m - ya * s;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int iy = ya + py - (t >> 1), ix = xb + px - (t & 1);
            const bool in = m < ss && iy >= 0 && iy < s && ix >= 0 && ix < s;
            aoff[t][i] = (in ? iy * s + ix : ss) * KP_ROWB + (lane >> 5) * 16;  // (E elements of T are 16 bytes)
        }
    }

    mh_f32x16 acc[KP_MAX_MB];
#pragma unroll
    for (int i = 0; i < KP_MAX_MB; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;

    const int rowbytes = a.cin * (int)sizeof(T);
    const int nch = rowbytes / KP_CHUNK_BYTES;
    const int nkb = a.cin / (2 * E);  // K blocks of the whole weight; a chunk holds 4
    const int npc = ss * 8;           // 16-byte pieces of a chunk
    const unsigned char* xb0 = reinterpret_cast<const unsigned char*>(a.x) + (size_t)roi * ss * rowbytes;
    const frag_t* __restrict__ wf = reinterpret_cast<const frag_t*>(a.w);  // [ky * 4 + kx][nkb][64 lanes] fragments

    uint4 pf[KP_PF];
#pragma unroll
    for (int u = 0; u < KP_PF; ++u) {
        const int e = tid + u * 256;
        pf[u] = make_uint4(0u, 0u, 0u, 0u);
        if (e < npc) pf[u] = *reinterpret_cast<const uint4*>(xb0 + (size_t)(e >> 3) * rowbytes + (e & 7) * 16);
    }
    if (tid < KP_ROWB / 16) *reinterpret_cast<uint4*>(kp_lds + ss * KP_ROWB + tid * 16) = make_uint4(0u, 0u, 0u, 0u);

    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();  // every wave is done with the previous chunk
#pragma unroll
        for (int u = 0; u < KP_PF; ++u) {
            const int e = tid + u * 256;
            if (e < npc) *reinterpret_cast<uint4*>(kp_lds + (e >> 3) * KP_ROWB + (e & 7) * 16) = pf[u];
        }
        __syncthreads();
        if (ch + 1 < nch) {
#pragma unroll
            for (int u = 0; u < KP_PF; ++u) {
                const int e = tid + u * 256;
                if (e < npc) pf[u] = *reinterpret_cast<const uint4*>(xb0 + (size_t)(e >> 3) * rowbytes + (size_t)(ch + 1) * KP_CHUNK_BYTES + (e & 7) * 16);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int tap = (1 - py + 2 * (t >> 1)) * 4 + (1 - px + 2 * (t & 1));
            const frag_t* wt = wf + ((size_t)tap * nkb + (size_t)ch * 4) * 64 + lane;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const frag_t fb = wt[u * 64];
#pragma unroll
                for (int i = 0; i < KP_MAX_MB; ++i)
                    if (i < nmb) {
                        const frag_t fa = *reinterpret_cast<const frag_t*>(kp_lds + aoff[t][i] + u * 32);
                        acc[i] = MhFrag<T>::mfma(fa, fb, acc[i]);
                    }
            }
        }
    }

    // ---- bias, the 2S x 2S maps of 16 keypoints at a time -> LDS (fp32), bilinear x2 -> global ----
    float* low = reinterpret_cast<float*>(kp_lds);
    const int plane = os * os + 1;  // (odd pitch: the 16 keypoints of a pixel land on different banks)
    const int col = lane & 31;
    const float bv = col < a.k ? a.bias[col] : 0.f;
    const float inv_hs = 1.0f / (float)hs, inv_hh = 1.0f / (float)(hs * hs);
    for (int j0 = 0; j0 < a.k; j0 += KP_HALF) {
        __syncthreads();  // the stream's last chunk, or the previous pass's maps, are read
        if (col >= j0 && col < j0 + KP_HALF && col < a.k) {
            float* lp = low + (col - j0) * plane;
#pragma unroll
            for (int i = 0; i < KP_MAX_MB; ++i)
                if (i < nmb) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int m = i * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
                        if (m < ss) {
                            const int ya = (int)(((float)m + 0.5f) * inv_s), xa = m - ya * s;
                            lp[(2 * ya + py) * os + 2 * xa + px] = acc[i][q] + bv;
                        }
                    }
                }
        }
        __syncthreads();
        const int nj = min(KP_HALF, a.k - j0);
        const int total = nj * hs * hs;
        float* o = out + (long long)j0 * hs * hs;
        for (int e = tid; e < total; e += 256) {
            const int jj = (int)(((float)e + 0.5f) * inv_hh), rem = e - jj * hs * hs;
            const int y = (int)(((float)rem + 0.5f) * inv_hs), xx = rem - y * hs;
            const float sy = fmaxf(((float)y + 0.5f) * 0.5f - 0.5f, 0.f), sx = fmaxf(((float)xx + 0.5f) * 0.5f - 0.5f, 0.f);
            const int y0 = (int)sy, x0 = (int)sx;
            const int y1 = min(y0 + 1, os - 1), x1 = min(x0 + 1, os - 1);
            const float ly = sy - (float)y0, lx = sx - (float)x0;
            const float* lp = low + jj * plane;
            const float top = (1.f - lx) * lp[y0 * os + x0] + lx * lp[y0 * os + x1];
            const float bot = (1.f - lx) * lp[y1 * os + x0] + lx * lp[y1 * os + x1];
            o[e] = (1.f - ly) * top + ly * bot;
        }
    }
}

template <class T>
static osr_status keypoint_upsample_launch(const KpUpArgs& a, long long r, hipStream_t st) {
    const int ss = a.s * a.s, os = 2 * a.s;
    const size_t stream_bytes = (size_t)(ss + 1) * KP_ROWB, low_bytes = (size_t)KP_HALF * (os * os + 1) * sizeof(float);
    const size_t lds = stream_bytes > low_bytes ? stream_bytes : low_bytes;  // (at most 50 240 bytes: S = 14)
    hipLaunchKernelGGL((keypoint_upsample_kernel<T>), dim3((unsigned)r), dim3(256), lds, st, a);
    OSR_CHECK_LAUNCH("osr_keypoint_upsample");
    return OSR_OK;
}

extern "C" osr_status osr_keypoint_upsample(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t k,
                                            const void* w_packed, const float* bias, const int32_t* rows_valid, int32_t seg_rows,
                                            float* heatmaps, void* stream) {
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_keypoint_upsample: bad dtype");
    OSR_REQUIRE(r >= 0, OSR_ERR_INVALID_ARG, "osr_keypoint_upsample: bad r");
    OSR_REQUIRE(s >= 8 && s <= KP_MAX_S, OSR_ERR_UNSUPPORTED, "osr_keypoint_upsample: s must be 8 .. 14, got %d", s);
    OSR_REQUIRE(cin >= 64 && cin % 64 == 0 && cin <= 512, OSR_ERR_UNSUPPORTED, "osr_keypoint_upsample: cin must be a multiple of 64, at most 512, got %d", cin);
    OSR_REQUIRE(k >= 1 && k <= 32, OSR_ERR_UNSUPPORTED, "osr_keypoint_upsample: k must be 1 .. 32, got %d", k);
    OSR_REQUIRE(!rows_valid || seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_keypoint_upsample: rows_valid needs seg_rows >= 1");
    if (r == 0) return OSR_OK;
    OSR_REQUIRE(x && w_packed && bias && heatmaps, OSR_ERR_INVALID_ARG, "osr_keypoint_upsample: null pointer");
    OSR_REQUIRE((((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)heatmaps) & 15) == 0, OSR_ERR_INVALID_ARG,
                "osr_keypoint_upsample: x / w_packed / heatmaps must be 16-byte aligned");
    OSR_REQUIRE(r < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_keypoint_upsample: too many RoIs");
    KpUpArgs a;
    a.x = x; a.w = w_packed; a.bias = bias; a.rows_valid = rows_valid; a.out = heatmaps;
    a.s = s; a.cin = cin; a.k = k; a.seg_rows = rows_valid ? seg_rows : 1;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case OSR_F32: return keypoint_upsample_launch<float>(a, r, st);
        case OSR_F16: return keypoint_upsample_launch<f16_t>(a, r, st);
        default: return keypoint_upsample_launch<bf16_t>(a, r, st);
    }
}

// ------------------------------------------------------------------------------------------------------
// [d2] heatmaps_to_keypoints for one (RoI, keypoint) per workgroup: the position of the maximum of the M x M map resized bicubically
// (A = -0.75, align_corners=False, F.interpolate's rules) to ceil(h) x ceil(w) of the RoI, without the resized map. The map is staged
// in LDS. Bicubic resampling is separable: each wave takes the output rows wave, wave + 4, ...; its lanes blend the four source rows
// of an output row into the wave's own LDS row of M values (the vertical taps), then each lane walks the output columns lane,
// lane + 64, ... with the four horizontal taps on that row and keeps a running (max, lowest row-major index). A wave's row buffer is
// written and read by that wave alone, so the rows need no workgroup barrier: a wave's LDS accesses complete in order, and a
// wavefront fence keeps the compiler from moving them across the hand-over. The workgroup's 256 candidates are reduced with the
// same (larger value, then lower index) rule, which makes the result independent of the order: the first row-major maximum, bit-identical between runs. The score is
// 1 / sum over the M x M INPUT map of exp(map - max), [d2]'s expression, summed in a fixed tree.
//
// Why one workgroup per (RoI, keypoint): the work is ceil(h) ceil(w) outputs, 1 to about 10^6, unknown on the host. 1 600 RoIs x 17
// keypoints are 27 200 workgroups of uneven length for 256 CUs: the dispatcher balances them, a map is read from global memory once,
// and four rows in flight hide the LDS latency of the taps. A wave per map would leave the large boxes as stragglers; several
// workgroups per map would need a second reduction pass.
// ------------------------------------------------------------------------------------------------------
#define KH_MAX_M 56
#define KH_MAX_SIDE 16384

__device__ __forceinline__ void kh_cubic(float t, float c[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x3 = 2.0f - t, x2 = 1.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__device__ __forceinline__ void kh_better(float& v, int& idx, float ov, int oidx) {
    if (ov > v || (ov == v && oidx < idx)) { v = ov; idx = oidx; }
}

// hand-over of a wave-private LDS row between the lanes of one wave (no other wave touches it)
__device__ __forceinline__ void kh_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void heatmaps_to_keypoints_kernel(const float* __restrict__ maps, const float* __restrict__ rois, int k, int m,
                                                                    const int* __restrict__ rows_valid, int seg_rows, float* __restrict__ out) {
    __shared__ float s_map[KH_MAX_M * KH_MAX_M];
    __shared__ float s_row[4][64];
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x, roi = b / k;
    float* o = out + b * 4;
    if (rows_valid && (int)(roi % seg_rows) >= rows_valid[roi / seg_rows]) {
        if (tid < 4) o[tid] = 0.f;
        return;
    }
    const int mm = m * m;
    const float* mp = maps + b * mm;
    for (int e = tid; e < mm; e += 256) s_map[e] = mp[e];

    const float bx0 = rois[roi * 4 + 0], by0 = rois[roi * 4 + 1];
    const float w = fmaxf(rois[roi * 4 + 2] - bx0, 1.0f), h = fmaxf(rois[roi * 4 + 3] - by0, 1.0f);
    const int wc = (int)fminf(ceilf(w), (float)KH_MAX_SIDE), hc = (int)fminf(ceilf(h), (float)KH_MAX_SIDE);
    const float scx = (float)m / (float)wc, scy = (float)m / (float)hc;
    __syncthreads();

    float best = -INFINITY;
    int bidx = 0x7fffffff;
    float* row = s_row[wave];
    for (int y = wave; y < hc; y += 4) {
        if (lane < m) {
            const float src = scy * ((float)y + 0.5f) - 0.5f, fl = floorf(src);
            float c[4];
            kh_cubic(src - fl, c);
            const int i0 = (int)fl - 1;
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) v += c[t] * s_map[min(max(i0 + t, 0), m - 1) * m + lane];
            row[lane] = v;
        }
        kh_wave_sync();  // the row is written: the wave's lanes read each other's values
        for (int x = lane; x < wc; x += 64) {
            const float src = scx * ((float)x + 0.5f) - 0.5f, fl = floorf(src);
            float c[4];
            kh_cubic(src - fl, c);
            const int i0 = (int)fl - 1;
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) v += c[t] * row[min(max(i0 + t, 0), m - 1)];
            kh_better(best, bidx, v, y * wc + x);
        }
        kh_wave_sync();  // the row is read: the next output row overwrites it
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(best, d, 64);
        const int oi = __shfl_xor(bidx, d, 64);
        kh_better(best, bidx, ov, oi);
    }
    if (lane == 0) { s_v[wave] = best; s_i[wave] = bidx; }
    __syncthreads();
    best = s_v[0]; bidx = s_i[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) kh_better(best, bidx, s_v[q], s_i[q]);
    if (bidx == 0x7fffffff) bidx = 0;  // (a map without one comparable value)
    __syncthreads();

    float sum = 0.f;
    for (int e = tid; e < mm; e += 256) sum += expf(s_map[e] - best);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) s_v[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const float total = (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
        const int pyi = bidx / wc, pxi = bidx - pyi * wc;
        o[0] = fmaf((float)pxi + 0.5f, w / (float)wc, bx0);
        o[1] = fmaf((float)pyi + 0.5f, h / (float)hc, by0);
        o[2] = best;
        o[3] = 1.0f / total;
    }
}

extern "C" osr_status osr_heatmaps_to_keypoints(const float* maps, const float* rois, int64_t r, int32_t k, int32_t m,
                                                const int32_t* rows_valid, int32_t seg_rows, float* out, void* stream) {
    OSR_REQUIRE(r >= 0 && k >= 1, OSR_ERR_INVALID_ARG, "osr_heatmaps_to_keypoints: bad r / k");
    OSR_REQUIRE(m >= 1 && m <= KH_MAX_M, OSR_ERR_UNSUPPORTED, "osr_heatmaps_to_keypoints: m must be 1 .. 56, got %d", m);
    OSR_REQUIRE(!rows_valid || seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_heatmaps_to_keypoints: rows_valid needs seg_rows >= 1");
    if (r == 0) return OSR_OK;
    OSR_REQUIRE(maps && rois && out, OSR_ERR_INVALID_ARG, "osr_heatmaps_to_keypoints: null pointer");
    OSR_REQUIRE(r * (int64_t)k < (1ll << 31), OSR_ERR_UNSUPPORTED, "osr_heatmaps_to_keypoints: too many maps");
    hipLaunchKernelGGL(heatmaps_to_keypoints_kernel, dim3((unsigned)(r * k)), dim3(256), 0, (hipStream_t)stream, maps, rois, k, m, rows_valid,
                       rows_valid ? seg_rows : 1, out);
    OSR_CHECK_LAUNCH("osr_heatmaps_to_keypoints");
    return OSR_OK;
}
