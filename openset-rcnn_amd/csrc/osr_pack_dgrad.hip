// Backward-data weight of a convolution from its forward weight, once per SGD step (instead of flip + permute + copy kernels of
// the tensor library every iteration): dst[ci][kh-1-y][kw-1-x][co] = src[co][y][x][ci]. For 1x1 layers and FC matrices this is
// the plain transpose. One 32 x 32 (co, ci) tile of one tap per workgroup, through LDS, both sides coalesced; 2- or 4-byte elements.
//   osr_pack_dgrad_weight        one tensor per launch (first allocation, the narrow fp32 heads, the cascade's later stages)
//   osr_pack_dgrad_weight_multi  every convolution / FC weight of a training step in ONE launch instead of ~70: the caller builds a
//                                table (one entry per tensor) and a chunk list ((tensor index, tile index) per workgroup) once --
//                                the pointers of the trainer's buffers are stable -- uploads them, and passes them every step
// Both run the same pack_tile.
#include "osr_common.h"

namespace {

template <class T>
__device__ __forceinline__ void pack_tile(const osr_pack_tensor& t, int bx, int by, int tap, T (*buf)[33]) {
    const int y = tap / t.kw, x = tap % t.kw;
    const int ci0 = bx * 32, co0 = by * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const long long taps = (long long)t.kh * t.kw;
    const T* __restrict__ src = reinterpret_cast<const T*>(t.src);
    T* __restrict__ dst = reinterpret_cast<T*>(t.dst);
    for (int r = ty; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + tx;
        if (co < t.cout && ci < t.cin) buf[r][tx] = src[((long long)co * taps + tap) * t.cin + ci];
    }
    __syncthreads();
    const int ftap = (t.kh - 1 - y) * t.kw + (t.kw - 1 - x);
    for (int r = ty; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + tx;
        if (ci < t.cin && co < t.cout) dst[((long long)ci * taps + ftap) * t.cout + co] = buf[tx][r];
    }
}

// grid: (ci tiles, co tiles, taps)
template <class T>
__global__ __launch_bounds__(256) void pack_dgrad_kernel(osr_pack_tensor t) {
    __shared__ T buf[32][33];
    pack_tile<T>(t, blockIdx.x, blockIdx.y, blockIdx.z, buf);
}

// chunk = (tensor index, (tap * ceil(cout / 32) + co tile) * ceil(cin / 32) + ci tile)
__global__ __launch_bounds__(256) void pack_multi_kernel(const osr_pack_tensor* __restrict__ table, const int2* __restrict__ chunks) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[32 * 33 * 4];
    const int2 c = chunks[blockIdx.x];
    const osr_pack_tensor t = table[c.x];
    const int tiles_ci = (t.cin + 31) >> 5, tiles_co = (t.cout + 31) >> 5;
    const int bx = c.y % tiles_ci, rest = c.y / tiles_ci, by = rest % tiles_co, tap = rest / tiles_co;
    if (t.elem_bytes == 4) pack_tile(t, bx, by, tap, reinterpret_cast<float (*)[33]>(smem));
    else pack_tile(t, bx, by, tap, reinterpret_cast<unsigned short (*)[33]>(smem));
}

}  // namespace

extern "C" osr_status osr_pack_dgrad_weight(const void* weight, void* out, int32_t cout, int32_t kh, int32_t kw, int32_t cin, int32_t dtype, void* stream) {
    OSR_REQUIRE(weight && out && weight != out, OSR_ERR_INVALID_ARG, "osr_pack_dgrad_weight: null or aliased pointers");
    OSR_REQUIRE(cout >= 1 && cin >= 1 && kh >= 1 && kw >= 1 && kh * kw <= 65535 && osr_dtype_ok(dtype), OSR_ERR_INVALID_ARG, "osr_pack_dgrad_weight: bad sizes / dtype");
    const dim3 grid((cin + 31) / 32, (cout + 31) / 32, kh * kw);
    OSR_REQUIRE(grid.y <= 65535, OSR_ERR_UNSUPPORTED, "osr_pack_dgrad_weight: cout too large");
    hipStream_t st = (hipStream_t)stream;
    const osr_pack_tensor t = {weight, out, cout, kh, kw, cin, dtype == OSR_F32 ? 4 : 2, 0};
    if (dtype == OSR_F32) hipLaunchKernelGGL(pack_dgrad_kernel<float>, grid, dim3(256), 0, st, t);
    else hipLaunchKernelGGL(pack_dgrad_kernel<unsigned short>, grid, dim3(256), 0, st, t);
    OSR_CHECK_LAUNCH("osr_pack_dgrad_weight");
    return OSR_OK;
}

extern "C" osr_status osr_pack_dgrad_weight_multi(const osr_pack_tensor* table, const int32_t* chunks, int32_t num_chunks, void* stream) {
    OSR_REQUIRE(table && chunks && num_chunks >= 0, OSR_ERR_INVALID_ARG, "osr_pack_dgrad_weight_multi: null table");
    if (num_chunks == 0) return OSR_OK;
    hipLaunchKernelGGL(pack_multi_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<const int2*>(chunks));
    OSR_CHECK_LAUNCH("osr_pack_dgrad_weight_multi");
    return OSR_OK;
}
