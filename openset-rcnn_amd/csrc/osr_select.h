// Selection helpers shared by the top-k kernels (osr_rpn.hip: osr_rpn_select; osr_retinanet.hip: osr_retinanet_select).
#pragma once
#include "osr_common.h"

#define SEL_THREADS 1024
#define SEL_MAXK 2048
#define SEL_BINS 2048  // histogram bins of a radix-select pass (11 key bits)

// descending bitonic sort of 64-bit keys in LDS, n power of two
__device__ __forceinline__ void bitonic_desc(unsigned long long* buf, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                int ixj = i ^ j;
                if (ixj > i) {
                    unsigned long long a = buf[i], b = buf[ixj];
                    bool desc = (i & k) == 0;
                    if (desc ? (a < b) : (a > b)) { buf[i] = b; buf[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// osr_float_key with every NaN mapped to the largest key. torch.sort(descending=True), which find_top_rpn_proposals selects with, puts
// a NaN score first whatever its sign bit; osr_float_key orders a sign-set NaN (0xffc00000, an x86 host's inf - inf) below -inf, so
// the anchor would never be selected, never reach the finite filter and never raise status_flags. NaNs tie with each other: lower
// index first, like every other tie.
__device__ __forceinline__ uint32_t sel_key(float f) { return f != f ? 0xffffffffu : osr_float_key(f); }

// hist[digit] += 1 for the lanes with `on`, called by all 64 lanes of a wave. Two rounds of "the first pending lane's digit: every
// lane that shares it is added by ONE atomic", then one atomic per lane that is still pending. Same histogram as 64 plain atomics.
__device__ __forceinline__ void sel_hist_add(int* hist, int digit, bool on) {
    const int lane = threadIdx.x & 63;
    unsigned long long act = __ballot(on);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (!act) return;  // wave-uniform
        const int leader = __ffsll((long long)act) - 1;
        const int d0 = __shfl(digit, leader, 64);
        const bool mine = on && digit == d0;
        const unsigned long long m = __ballot(mine);
        if (lane == leader) atomicAdd(&hist[d0], __popcll(m));
        if (mine) on = false;
        act &= ~m;
    }
    if (on) atomicAdd(&hist[digit], 1);
}
