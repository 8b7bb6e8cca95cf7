// The MFMA fragments of the mask head's tail (csrc/osr_mask_head.hip: forward; csrc/osr_mask_train.hip: backward), shared so that the
// backward recomputes the deconvolution with the very instructions of the forward, and the one rule for which mask rows are live.
#pragma once
#include "osr_common.h"

typedef float mh_f32x16 __attribute__((ext_vector_type(16)));
typedef f16_t mh_f16x8 __attribute__((ext_vector_type(8)));
typedef bf16_t mh_bf16x8 __attribute__((ext_vector_type(8)));

// E: elements of K a lane holds per fragment; a K block is 2 E deep (lanes 0..31 the first E, lanes 32..63 the second).
template <class T> struct MhFrag;
template <> struct MhFrag<f16_t> {
    typedef mh_f16x8 type;
    static constexpr int BM = 64, E = 8;
    static __device__ __forceinline__ mh_f32x16 mfma(type a, type b, mh_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct MhFrag<bf16_t> {
    typedef mh_bf16x8 type;
    static constexpr int BM = 64, E = 8;
    static __device__ __forceinline__ mh_f32x16 mfma(type a, type b, mh_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MhFrag<float> {
    typedef float4 type;
    static constexpr int BM = 32, E = 4;
    static __device__ __forceinline__ mh_f32x16 mfma(type a, type b, mh_f32x16 c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
    }
};

#define MH_PAD 16         // bytes of padding per LDS row (rows of Cin elements are a multiple of 128 bytes: all on one bank otherwise)

// does mask row r exist (its segment's count: the first rows_valid[segment] rows of every seg_rows), and which predictor row does it
// take (-1: none; row 0 when class-agnostic). Forward, loss and backward agree on it: a row that is not live counts nowhere.
__device__ __forceinline__ int mt_row_class(long long r, int num_rows, const long long* __restrict__ classes, const int* __restrict__ rows_valid, int seg_rows) {
    if (rows_valid && (int)(r % seg_rows) >= rows_valid[r / seg_rows]) return -1;
    if (!classes) return 0;
    const long long c = classes[r];
    if (c < 0) return -1;
    if (num_rows == 1) return 0;
    return c < num_rows ? (int)c : -1;
}
