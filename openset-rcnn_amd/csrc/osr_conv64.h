// The BK=64 convolution path (osr_conv_gemm64.hip) as osr_conv2d_fwd (osr_conv_gemm.hip) sees it.
#pragma once
#include "osr_common.h"

// 1 when the BK=64 kernel can take the problem (all arguments already validated by osr_conv2d_fwd).
int osr_conv64_eligible(const osr_conv_params* p, long long in_bytes, long long w_bytes);
// Bytes of workspace with which osr_conv2d_fwd cuts this layer's partial last dispatch round along K (0: not applicable).
long long osr_conv64_split_workspace_bytes(const osr_conv_params* p);
// Host-side description of how osr_conv2d_fwd covers this layer (tests, docs/CONV_FWD_PLANS.md).
int osr_conv64_describe(const osr_conv_params* p, int has_workspace, char* buf, int n);
osr_status osr_conv64_run(const osr_conv_params* p, const void* in, const void* weight, const float* bias, const void* residual, const void* mask,
                          void* out, long long in_bytes, long long w_bytes, hipStream_t st);
