// Selection helpers shared by the top-k kernels: the k best of a list by a float key, ties to the lower index, sorted. Users:
//   osr_rpn.hip        rpn_select_kernel (osr_rpn_select)
//   osr_retinanet.hip  rn_filter_kernel, rn_refine_kernel, rn_select_kernel (osr_retinanet_select)
//   osr_train_fwd.hip  tr_select_smallest (subsample_kernel, roi_match_sample_kernel)
//   osr_det_tail.hip   seg_sort_kernel
// One pair format, one bitonic sort, one wave-aggregated histogram add, one digit walk and one radix pass. What a kernel keeps for
// itself is what differs for a measured reason: its memory walk, its compaction, its pass schedule and its LDS budget.
#pragma once
#include "osr_common.h"

#define SEL_THREADS 1024
#define SEL_MAXK 2048
#define SEL_BINS 2048  // histogram bins of a radix-select pass (11 key bits)

// ---- the (key, ~index) pair: pairs are unique, and descending pair order is key descending, then index ascending. 0 is no element. ----
__device__ __forceinline__ unsigned long long sel_pair(uint32_t key, unsigned index) {
    return ((unsigned long long)key << 32) | (0xffffffffu - index);
}
__device__ __forceinline__ int sel_pair_index(unsigned long long pair) { return (int)(0xffffffffu - (unsigned int)pair); }
// the float whose osr_float_key is the pair's key
__device__ __forceinline__ float sel_pair_key_float(unsigned long long pair) {
    const uint32_t key = (uint32_t)(pair >> 32);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// osr_float_key with every NaN mapped to the largest key. torch.sort(descending=True), which find_top_rpn_proposals selects with, puts
// a NaN score first whatever its sign bit; osr_float_key orders a sign-set NaN (0xffc00000, an x86 host's inf - inf) below -inf, so
// the anchor would never be selected, never reach the finite filter and never raise status_flags. NaNs tie with each other: lower
// index first, like every other tie.
__device__ __forceinline__ uint32_t sel_key(float f) { return f != f ? 0xffffffffu : osr_float_key(f); }

// ---- descending bitonic sort of 64-bit pairs, n a power of two; P points into LDS or global memory. Called by the whole block. ----
template <class P>
__device__ __forceinline__ void bitonic_desc(P buf, int n) {
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

// buf[0, k) holds the selected pairs in any order (written before the call, no barrier needed): pad to a power of two with zeros, which
// sort last, and sort. buf must hold pow2ceil(k) pairs.
template <class P>
__device__ __forceinline__ void sel_pad_and_sort(P buf, int k) {
    int kp = 1;
    while (kp < k) kp <<= 1;
    for (int i = k + threadIdx.x; i < kp; i += blockDim.x) buf[i] = 0ull;
    __syncthreads();
    bitonic_desc(buf, kp);
}

// ---- hist[digit] += 1 for the lanes with `on`. The lanes of a wave that call it call it together, `on` or not (the tail of a walk may
// leave some out). ROUNDS times "the first pending lane's digit: every lane that shares it is added by ONE atomic", then one atomic per
// lane that is still pending. Same histogram as 64 plain atomics whatever ROUNDS is: keys of a narrow range share their leading digit
// (sigmoid outputs, uniform keys in [0.5, 1): one exponent), and a plain LDS atomic per lane would serialise 64 ways on one address. ----
template <int ROUNDS>
__device__ __forceinline__ void sel_hist_add(int* hist, int digit, bool on) {
    const int lane = threadIdx.x & 63;
    unsigned long long act = __ballot(on);
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
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

// ---- the digit whose bucket holds a rank: the largest d with sum(hist[d..]) >= remaining. Called by one full wave; returns true in the
// ONE lane that finds it, and only there *digit = d, *above = sum(hist[d + 1..]) and *bucket = hist[d]: that lane publishes them.
// hist (LDS or global, 16-byte aligned) has BINS entries.
// PRECONDITION: sum(hist) >= remaining >= 1. Then exactly one lane holds the crossing; no exit for an emptier histogram exists.
// Lane l owns bins [l * BINS / 64, (l + 1) * BINS / 64): 16-byte reads, suffix sums over the lanes, then the one lane that holds the
// crossing walks its own bins (a serial walk over all bins is dependent reads, 7 us per 256 of them in LDS). ----
template <int BINS>
__device__ __forceinline__ bool sel_digit_of_rank(const int* hist, int remaining, int* digit, int* above, int* bucket) {
    constexpr int BPL = BINS / 64;
    static_assert(BINS % 256 == 0, "sel_digit_of_rank: 64 lanes x whole int4 reads");
    const int lane = threadIdx.x & 63;
    const int* h = hist + lane * BPL;
    int sum = 0;
#pragma unroll
    for (int j = 0; j < BPL; j += 4) {
        const int4 h4 = *reinterpret_cast<const int4*>(h + j);
        sum += h4.x + h4.y + h4.z + h4.w;
    }
    int inc = sum;  // becomes the sum over this lane's bins and all higher lanes'
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        const int t = __shfl_down(inc, dd, 64);
        if (lane + dd < 64) inc += t;
    }
    const bool here = inc - sum < remaining && remaining <= inc;
    if (here) {
        int acc = inc - sum;
        for (int j = BPL - 1; j >= 0; --j) {
            const int hj = h[j];
            if (acc + hj >= remaining) { *digit = lane * BPL + j; *bucket = hj; break; }
            acc += hj;
        }
        *above = acc;
    }
    return here;
}

// ---- one pass of a radix select of the `remaining`-th largest key, MSB first. K is the key type: uint32_t float keys, or the 64-bit
// pairs themselves where the index bits take part. ----
template <class K>
struct SelRank {  // the search so far, in registers (uniform across the block)
    K prefix, mask;  // the wanted key's bits under mask are prefix
    int remaining;   // rank (1-based, from the top) still to resolve among the keys that match the prefix
};
template <class K>
struct SelBcast { K prefix; int remaining, bucket; };  // a pass's result on its way from wave 0 to the block, in LDS

// Refines `r` by the `bits` key bits at `shift`: zero the histogram, barrier, walk(add) -- the kernel's own walk over its list, calling
// add(key, member) for every element as sel_hist_add is called -- barrier, digit walk on wave 0, broadcast through *s_bc, barrier.
// Returns hist[digit], the size of the new prefix's bucket. Called by the whole block; s_hist has BINS >= 1 << bits entries, 16-byte
// aligned. PRECONDITION (sel_digit_of_rank's): at least r.remaining >= 1 members match r's prefix.
template <int BINS, int ROUNDS, class K, class Walk>
__device__ __forceinline__ int sel_radix_pass(SelRank<K>& r, int shift, int bits, int* s_hist, SelBcast<K>* s_bc, Walk walk) {
    const K digits = (K)((1 << bits) - 1);
    for (int i = threadIdx.x; i < BINS; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
    walk([&](K key, bool member) { sel_hist_add<ROUNDS>(s_hist, (int)((key >> shift) & digits), member && (key & r.mask) == r.prefix); });
    __syncthreads();
    if (threadIdx.x < 64) {
        int d, above, bucket;
        if (sel_digit_of_rank<BINS>(s_hist, r.remaining, &d, &above, &bucket))
            *s_bc = SelBcast<K>{r.prefix | ((K)d << shift), r.remaining - above, bucket};
    }
    __syncthreads();
    r.prefix = s_bc->prefix;
    r.remaining = s_bc->remaining;
    const int bucket = s_bc->bucket;
    r.mask |= digits << shift;
    __syncthreads();
    return bucket;
}
