// Mean over the positions of a RoI for gfx950 (include/osr.h: osr_avgpool_rows).
//
// Replaces [d2] Res5ROIHeads.forward's box_features.mean(dim=[2, 3]): res5's (R, 7, 7, 2048) output, channels last, to the (R, 2048)
// fp32 rows box_predictor reads. One lane owns 16 bytes of channels of one RoI and walks the RoI's positions in ascending order, so a
// wave reads one contiguous 1 KiB run per position and a channel's sum has one order whatever the launch: no atomics, no LDS, no
// cross-lane step. The kernel is a read of x at HBM rate; the positions are unrolled so that several loads are in flight per lane.
#include "osr_common.h"

#define AP_THREADS 256
#define AP_MAX_S 196  // 14 x 14: the largest grid a pooler of this library produces

// V elements of T (16 bytes, or 8 for 16-bit rows whose width is not a multiple of 8) added into acc
template <class T, int V>
__device__ __forceinline__ void ap_add(const T* p, float* acc) {
    if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w;
    } else {
        typedef T tv __attribute__((ext_vector_type(V)));
        const tv q = *reinterpret_cast<const tv*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += (float)q[j];
    }
}

template <class T, int V>
__global__ __launch_bounds__(AP_THREADS) void avgpool_rows_kernel(const T* __restrict__ x, long long r, int s, int c,
                                                                  const int* __restrict__ rows_valid, int seg_rows,
                                                                  float* __restrict__ out) {
    const int cv = c / V;
    const long long items = r * cv;
    const float fs = (float)s;
    for (long long it = (long long)blockIdx.x * AP_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * AP_THREADS) {
        const long long row = it / cv;
        const int c0 = (int)(it - row * cv) * V;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        const bool exists = !rows_valid || (int)(row % seg_rows) < rows_valid[row / seg_rows];
        if (exists) {
            const T* p = x + (size_t)row * s * c + c0;
#pragma unroll 7
            for (int i = 0; i < s; ++i) ap_add<T, V>(p + (size_t)i * c, acc);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = acc[j] / fs;
        }
        float* o = out + (size_t)row * c + c0;
#pragma unroll
        for (int j = 0; j < V; j += 4) *reinterpret_cast<float4*>(o + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
    }
}

template <class T, int V>
static void ap_launch(const void* x, int64_t r, int s, int c, const int32_t* rows_valid, int seg_rows, float* out, hipStream_t st) {
    const long long items = (long long)r * (c / V);
    long long blocks = (items + AP_THREADS - 1) / AP_THREADS;
    if (blocks > 256 * 64) blocks = 256 * 64;  // grid-stride beyond 64 workgroups per CU
    hipLaunchKernelGGL((avgpool_rows_kernel<T, V>), dim3((unsigned)blocks), dim3(AP_THREADS), 0, st, (const T*)x, (long long)r, s, c,
                       rows_valid, seg_rows, out);
}

extern "C" osr_status osr_avgpool_rows(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t c, const int32_t* rows_valid,
                                       int32_t seg_rows, float* out, void* stream) {
    OSR_REQUIRE(osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_avgpool_rows: bad dtype %d", dtype);
    OSR_REQUIRE(r >= 0 && r < (1ll << 31), OSR_ERR_INVALID_ARG, "osr_avgpool_rows: bad r");
    OSR_REQUIRE(c > 0 && c % 4 == 0, OSR_ERR_UNSUPPORTED, "osr_avgpool_rows: c must be a multiple of 4, got %d", c);
    OSR_REQUIRE(s >= 1 && s <= AP_MAX_S, OSR_ERR_UNSUPPORTED, "osr_avgpool_rows: s must be 1..%d, got %d", AP_MAX_S, s);
    OSR_REQUIRE(!rows_valid || seg_rows >= 1, OSR_ERR_INVALID_ARG, "osr_avgpool_rows: rows_valid needs seg_rows >= 1");
    if (r == 0) return OSR_OK;
    OSR_REQUIRE(x && out, OSR_ERR_INVALID_ARG, "osr_avgpool_rows: null pointer");
    OSR_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, OSR_ERR_INVALID_ARG, "osr_avgpool_rows: x and out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int sr = rows_valid ? seg_rows : 1;
    if (dtype == OSR_F32) ap_launch<float, 4>(x, r, s, c, rows_valid, sr, out, st);
    else if (dtype == OSR_F16) { if (c % 8 == 0) ap_launch<f16_t, 8>(x, r, s, c, rows_valid, sr, out, st); else ap_launch<f16_t, 4>(x, r, s, c, rows_valid, sr, out, st); }
    else { if (c % 8 == 0) ap_launch<bf16_t, 8>(x, r, s, c, rows_valid, sr, out, st); else ap_launch<bf16_t, 4>(x, r, s, c, rows_valid, sr, out, st); }
    OSR_CHECK_LAUNCH("osr_avgpool_rows");
    return OSR_OK;
}
