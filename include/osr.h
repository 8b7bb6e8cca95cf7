/*
 * osr.h -- C ABI of libosr_hip.so: the MI355X (gfx950) implementation of Openset R-CNN's per-image
 * detection hot path.
 *
 * The reference (Yifei-Y/Openset-RCNN) has NO FFI of its own: its boundary is detectron2's registries and
 * nn.Module call signatures. Each entry point below therefore cites the reference call site
 * (file:line under /root/reference) -- or the un-vendored detectron2/torchvision primitive invoked there,
 * marked [d2] -- whose arithmetic it replaces. INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer unless named host_*;
 *   - the caller owns every buffer including workspace (sizes from osr_*_workspace_bytes); the library never
 *     allocates, frees or synchronises; all work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 = OSR_OK, negative = error (osr_last_error() gives a thread-local message);
 *     no C++ exception crosses the boundary; no global mutable state (re-entrant across threads/streams);
 *   - activations are NHWC ("channels last"); element types are named by osr_dtype.
 */
#ifndef OSR_H_
#define OSR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSR_ABI_VERSION 1

typedef int32_t osr_status;
enum {
    OSR_OK = 0,
    OSR_ERR_INVALID_ARG = -1,
    OSR_ERR_UNSUPPORTED = -2,
    OSR_ERR_LAUNCH = -3,
    OSR_ERR_WORKSPACE = -4
};

typedef enum { OSR_F32 = 0, OSR_F16 = 1, OSR_BF16 = 2 } osr_dtype;

#define OSR_MAX_LEVELS 8

int32_t osr_abi_version(void);
const char* osr_last_error(void);

/* ---------------------------------------------------------------------------------------------------------
 * Pre-processing  ([d2] GeneralizedRCNN.preprocess_image + ImageList.from_tensors, called from train.py:135)
 * src: (n,3,h,w) NCHW, uint8 (src_is_u8=1) or float32. dst: (n, hp+6, wpad, 4) NHWC fp16/bf16 where the
 * normalised image sits at row offset 3 / column offset 3, everything else (3-pixel halo, the /32 padding,
 * the 4th channel) is zero. wpad = osr_stem_padded_width(wp). This is the layout the 7x7/s2 stem reads
 * without bounds checks.
 * --------------------------------------------------------------------------------------------------------- */
int32_t osr_stem_padded_width(int32_t wp);
osr_status osr_preprocess(const void* src, int32_t src_is_u8, int32_t n, int32_t h, int32_t w, int32_t hp, int32_t wp,
                          const float mean[3], const float std[3], void* dst, int32_t dst_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Dense contractions on MFMA  ([d2] Conv2d / FrozenBatchNorm2d (folded) / nn.Linear of build_resnet_fpn_backbone
 * (Base-RCNN-FPN.yaml:3-8), ClsFreeRPNHead.conv (classification_free_rpn.py:158), FastRCNNConvFCHead
 * (osrcnn_roi_heads.py:308)).  Implicit GEMM:  out[n,oh,ow,co] = act( sum_{kh,kw,ci} in[n,oh*sh-ph+kh,
 * ow*sw-pw+kw,ci] * w[co,kh,kw,ci] + bias[co] (+ residual) ).
 * in/weight: fp16 or bf16; accumulate fp32; out: fp16/bf16/fp32. cin must be a multiple of 32, cout of 8.
 * A fully connected layer is the 1x1 case with hi=rows, wi=1.
 * res_mode: 0 none; 1 residual[n,oh,ow,co] (bottleneck shortcut); 2 residual[n,oh/2,ow/2,co]
 * (FPN top-down nearest-2x upsample-add); 3 residual[n,oh,ow,co] is a forward activation used as a ReLU mask
 * (out = residual > 0 ? value : 0; the backward-data pass, see osr_conv2d_wgrad below).
 * Strides are in ELEMENTS; the channel stride is 1.
 * pad_mode: 0 = bounds-checked zero padding; 1 = the input buffer already holds the halo (stem view).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct osr_conv_params {
    int32_t n, hi, wi, cin;
    int32_t ho, wo, cout;
    int32_t kh, kw, stride_h, stride_w, pad_h, pad_w;
    int64_t in_stride_n, in_stride_h, in_stride_w;
    int64_t out_stride_n, out_stride_h, out_stride_w;
    int64_t res_stride_n, res_stride_h, res_stride_w;
    int32_t relu;
    int32_t res_mode;
    int32_t pad_mode;
    int32_t in_dtype;  /* osr_dtype of in, weight, residual */
    int32_t out_dtype; /* osr_dtype of out */
    int32_t concurrency; /* scheduling hint: number of streams of the caller that launch onto the GPU at the same time (0 or 1:
                          * this launch has the GPU to itself). Tile selection only; results do not depend on it. */
    void* workspace;         /* optional (may be null), caller-owned, 16-byte aligned: with at least                      */
    int64_t workspace_bytes; /* osr_conv2d_fwd_workspace_bytes(p) bytes the partial last dispatch round of a deep-K 1x1 / FC
                              * layer is cut along K (fixed-order fp32 partial sums: bitwise reproducible, but not bitwise
                              * equal to the un-split sum) */
    const int32_t* row_seg_counts; /* optional (may be null), device memory: the output rows (n*ho*wo of them) come in segments */
    int32_t row_seg_rows;          /* of row_seg_rows rows of which only the first row_seg_counts[s] carry data (a padded per-image
                                    * proposal list: the box head's FC layers). A tile of output rows without any such row is
                                    * skipped and its rows are left unwritten; all other rows are computed as usual. */
} osr_conv_params;

/* Workspace with which osr_conv2d_fwd splits the tail round of this layer along K; 0 when the layer does not qualify (then a
 * null workspace costs nothing). Host-side arithmetic only. */
int64_t osr_conv2d_fwd_workspace_bytes(const osr_conv_params* p);
/* How osr_conv2d_fwd covers this layer: the tile shape of a single launch, or full rounds + split-K tail + reduction
 * (has_workspace != 0). Writes a short text ("256x256/2 rows [0,65536) + split-K x5 tail rows [65536,68368) + reduce") and
 * returns its length; host-side only (diagnostics, tests). */
int32_t osr_conv2d_fwd_describe(const osr_conv_params* p, int32_t has_workspace, char* buf, int32_t buf_bytes);

osr_status osr_conv2d_fwd(const osr_conv_params* p, const void* in, const void* weight, const float* bias,
                          const void* residual, void* out, void* stream);
/* osr_conv2d_fwd followed, in the same epilogue, by a ReLU mask: out = mask > 0 ? (conv + bias [+ residual]) : 0.
 * `mask` has in_dtype and out's logical layout (addressed with out_stride_*). This is the join of a residual block in the
 * backward pass -- data gradient of one branch + the gradient of the other (res_mode 1), through the ReLU of the layer
 * below ([d2] BottleneckBlock.forward's `F.relu_(out + shortcut)`, entered from train.py:145 `losses.backward()`) -- in one
 * launch. res_mode 0 or 1. Returns OSR_ERR_UNSUPPORTED (nothing launched) outside the BK=64 kernel's envelope
 * (cin % 64 != 0): run osr_conv2d_fwd + osr_relu_mask instead. */
osr_status osr_conv2d_fwd_masked(const osr_conv_params* p, const void* in, const void* weight, const float* bias,
                                 const void* residual, const void* mask, void* out, void* stream);

/* A bottleneck's 3x3 convolution and the 1x1 convolution behind it in ONE launch ([d2] BottleneckBlock.forward: conv2 -> conv3 ->
 * `out += shortcut; relu`, /root/reference/configs/Base-RCNN-FPN.yaml:3-8):
 *     out = relu(conv1x1(act(conv(in, weight) + bias), w3) + bias3 + residual),   act = ReLU when p->relu.
 * p describes the FIRST convolution (its output, cout channels, never reaches HBM; out_dtype == in_dtype f16/bf16; res_mode,
 * out_stride_* and row_seg_* are ignored); w3 is [cout3][cout] in the same dtype, bias3 fp32; residual and out are dense
 * (n*ho*wo, cout3) tensors of that dtype. Same K order and rounding points as osr_conv2d_fwd twice: bit-identical results.
 * Fused shapes: cout == 128, cout3 == 512 (the res3 blocks); anything else returns OSR_ERR_UNSUPPORTED, nothing launched. */
osr_status osr_conv2d_chain_fwd(const osr_conv_params* p, const void* in, const void* weight, const float* bias, const void* w3,
                                const float* bias3, int32_t cout3, const void* residual, void* out, void* stream);
/* The same, also writing the first convolution's activated output (what the separate launch would have stored), dense
 * (n*ho*wo, cout) rows in the storage dtype, to mid_out (nullable): the training step keeps it for the block's backward (ReLU mask of
 * conv3's data gradient, input of conv3's weight gradient) and still saves the second launch and its re-read. */
osr_status osr_conv2d_chain_fwd_ex(const osr_conv_params* p, const void* in, const void* weight, const float* bias, const void* w3,
                                   const float* bias3, int32_t cout3, const void* residual, void* out, void* mid_out,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * One whole ResNet bottleneck block in ONE launch: y = relu(conv3(relu(conv2(relu(conv1(x))))) + shortcut(x)),
 * 1x1 -> 3x3 (pad 1) -> 1x1, stride 1, FrozenBN folded into weights / biases ([d2] BottleneckBlock.forward, built by
 * build_resnet_fpn_backbone for /root/reference/configs/Base-RCNN-FPN.yaml:3-8). The two cmid-channel intermediates never
 * leave the chip: the block reads x once and writes y once (the three separate convolutions of a res2 block are HBM-bound
 * and move twice the bytes). Fused shapes: the res2 blocks -- cmid 64, cout 256, and either cin 256 with the identity
 * shortcut (has_proj 0) or cin 64 with a 1x1 projection shortcut wsc / bsc (has_proj 1). Anything else returns
 * OSR_ERR_UNSUPPORTED with nothing launched: run osr_conv2d_fwd three (four) times instead.
 * in (n,h,w,cin), out (n,h,w,cout) NHWC contiguous, dtype f16/bf16; weights packed [cout][kh][kw][cin] in the same dtype,
 * biases fp32. Same K order and the same rounding points as the separate launches; with has_proj the shortcut's output
 * is accumulated in fp32 with conv3 instead of being rounded to the storage dtype first (one rounding fewer).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct osr_bottleneck_params {
    int32_t n, h, w;
    int32_t cin, cmid, cout;
    int32_t dtype;    /* osr_dtype of in, out and the weights */
    int32_t has_proj; /* 1: projection shortcut (wsc, bsc); 0: identity (cin == cout) */
} osr_bottleneck_params;
osr_status osr_bottleneck_fwd(const osr_bottleneck_params* p, const void* in, const void* w1, const float* b1,
                              const void* w2, const float* b2, const void* w3, const float* b3, const void* wsc,
                              const float* bsc, void* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * ResizeShortestEdge on the device for uint8 images: [d2] ResizeTransform.apply_image = PIL Image.resize(BILINEAR)
 * (INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST, /root/reference/configs/Base-RCNN-FPN.yaml:43; the loader the reference builds
 * at train.py:129 does it on the host). Pillow's algorithm (Resample.c): separable triangle filter whose support grows
 * with the down-scaling factor, horizontal pass into an 8-bit intermediate, then the vertical pass, 22-bit fixed-point
 * coefficients. The caller computes the tables on the host from the two sizes (Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc: bounds (n,2) = first input index and tap count per output index, coef (n,k) int32); the result
 * is the PIL image bit for bit.
 * in: (h, w, 3) uint8 interleaved (row stride in bytes); out: (3, nh, nw) uint8 planar -- the "image" tensor of a model
 * input dict; tmp: osr_resize_tmp_bytes(y_rows, nw) bytes, rows [y_first, y_first + y_rows) = the input rows the vertical
 * pass reads (Pillow resamples only those horizontally).
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_resize_tmp_bytes(int32_t rows, int32_t nw);
osr_status osr_resize_bilinear_u8(const uint8_t* in, int32_t h, int32_t w, int64_t in_row_stride, const int32_t* xbounds,
                                  const int32_t* xcoef, int32_t kx, const int32_t* ybounds, const int32_t* ycoef,
                                  int32_t ky, int32_t y_first, int32_t y_rows, int32_t nh, int32_t nw, uint8_t* tmp,
                                  int64_t tmp_bytes, uint8_t* out, void* stream);

/* The same resampling of PLANAR images with an optional mirrored store: the "resize" and "resize + horizontal flip" of test-time
 * augmentation ([d2] DatasetMapperTTA: ResizeShortestEdge(s, TEST.AUG.MAX_SIZE) [+ RandomFlip(prob=1.0)] applied to the model input
 * image). in: (planes, h, w) uint8 -- planes = 3 for one image dict's "image", 3n for a stacked batch of n; out: (planes, nh, nw).
 * Same tables, same two passes and 8-bit intermediate as osr_resize_bilinear_u8: on the transposed data the two give the same bits.
 * mirror (0 / 1): the last pass stores column x at nw - 1 - x. tmp: planes * y_rows * nw bytes. */
osr_status osr_resize_bilinear_u8_planar(const uint8_t* in, int32_t planes, int32_t h, int32_t w, const int32_t* xbounds,
                                         const int32_t* xcoef, int32_t kx, const int32_t* ybounds, const int32_t* ycoef,
                                         int32_t ky, int32_t y_first, int32_t y_rows, int32_t nh, int32_t nw, int32_t mirror,
                                         uint8_t* tmp, int64_t tmp_bytes, uint8_t* out, void* stream);

/* The whole ResNet stem in ONE launch (csrc/osr_stem_pool.hip): [d2] BasicStem.forward = conv1 (7x7, stride 2, pad 3, 3 -> 64,
 * FrozenBN folded) -> ReLU -> F.max_pool2d(3, 2, 1), built by build_resnet_fpn_backbone (/root/reference/configs/Base-RCNN-FPN.yaml:3-8).
 * xpad: osr_preprocess' (n, hp + 6, osr_stem_padded_width(wp), 4) image; w_view: the stem view (64, w_rows, 1, 32) of
 * osr_conv2d_fwd's stem path (w_rows 7 or 8; row ky holds 8 taps x 4 channels, the 8th tap and the 4th channel zero); out:
 * (n, hp / 4, wp / 4, 64) (odd halves round up as the two layers do). The 64-channel stem output never reaches HBM. Same K order and
 * rounding points as osr_conv2d_fwd(stem view) followed by osr_maxpool3x3s2. dtype f16 / bf16 (hp, wp even). */
osr_status osr_stem_maxpool_fwd(const void* xpad, int32_t n, int32_t hp, int32_t wp, const void* w_view, int32_t w_rows, const float* bias,
                                void* out, int32_t dtype, void* stream);
/* The same from the RAW batch: osr_preprocess' normalisation, halo and /32 padding are applied while the kernel stages its input patch
 * (src (n,3,h,w) NCHW uint8 or float32, mean / std as osr_preprocess): same bits, no pre-padded copy of the batch in HBM. */
osr_status osr_stem_maxpool_fwd_raw(const void* src, int32_t src_is_u8, int32_t n, int32_t h, int32_t w, int32_t hp, int32_t wp,
                                    const float mean[3], const float std[3], const void* w_view, int32_t w_rows, const float* bias,
                                    void* out, int32_t dtype, void* stream);
/* Backward of the stem for a trainable stem (MODEL.BACKBONE.FREEZE_AT 0; csrc/osr_stem_bwd.hip). The training forward keeps the
 * stem output: osr_conv2d_fwd(stem view, ReLU) -> s, osr_maxpool3x3s2(s) -> pooled (same bits as osr_stem_maxpool_fwd).
 * osr_stem_pool_bwd: the max pool's and the ReLU's backward, s (n, hs, ws, c), dpool (n, (hs-1)/2+1, (ws-1)/2+1, c) -> ds (n, hs, ws, c):
 * ds[p] = sum of dpool over the windows whose first maximum is p (scan ky then kx, (v > max) || isnan(v): torch's max_pool2d
 * indices), 0 where s[p] <= 0. A gather in a fixed order: no atomics, repeats bit-identical. c % 8 == 0, dtype f16 / bf16. */
osr_status osr_stem_pool_bwd(const void* s, const void* dpool, int32_t n, int32_t hs, int32_t ws, int32_t c, void* ds, int32_t dtype,
                             void* stream);
/* osr_stem_wgrad: dw (64, 8, 1, 32) fp32 in the stem view's layout = sum over the n * hp/2 * wp/2 stem pixels of ds[p][co] times the
 * pixel's patch of xpad (osr_preprocess' image; row ky of the view: 8 taps x 4 channels of image row 2 oy + ky). MFMA with fp32
 * accumulation; the pixels are cut into a fixed number of ranges (a function of the pixel count only) whose partials go to the
 * caller's workspace (osr_stem_wgrad_workspace_bytes) and are summed in range order: no float atomics, repeats bit-identical. The
 * 8th row, the 8th tap and the 4th channel are written as exact zeros (accumulate: dw += the gradient). ds (n, hp/2, wp/2, 64). */
int64_t osr_stem_wgrad_workspace_bytes(int32_t n, int32_t hp, int32_t wp);
osr_status osr_stem_wgrad(const void* xpad, const void* ds, int32_t n, int32_t hp, int32_t wp, float* dw, int32_t accumulate, void* workspace,
                          int64_t workspace_bytes, int32_t dtype, void* stream);
/* [d2] F.max_pool2d(k=3,s=2,p=1) of the ResNet stem, NHWC contiguous. Non-finite inputs included: the maximum starts at -inf and is
 * replaced when (v > max) || isnan(v), scanning ky then kx -- a window of -inf gives -inf, +inf wins, a NaN once seen stays: the rule
 * osr_stem_pool_bwd uses to find the same maximum. */
osr_status osr_maxpool3x3s2(const void* in, int32_t n, int32_t hi, int32_t wi, int32_t c, void* out, int32_t dtype,
                            void* stream);
/* [d2] LastLevelMaxPool: p6 = max_pool2d(p5, k=1, s=2) = stride-2 subsample, NHWC contiguous. */
osr_status osr_subsample2(const void* in, int32_t n, int32_t hi, int32_t wi, int32_t c, void* out, int32_t dtype,
                          void* stream);

/* The gather half of a 3x3 deformable convolution, padding 1, dilation 1 ([d2] DeformConv / ModulatedDeformConv as
 * DeformBottleneckBlock's conv2; MODEL.RESNETS.DEFORM_ON_PER_STAGE): cols (n*ho*wo, 9, c), x's dtype, holds for output pixel
 * p = (b, y, x), tap k = 3 i + j and channel ch (group g = ch / (c / groups)) the masked bilinear sample
 *     cols[p][k][ch] = m * bilinear(x[b, :, :, ch], y * stride - 1 + i + dy, x * stride - 1 + j + dx),
 *     dy = om[p][2 (9 g + k)], dx = om[p][2 (9 g + k) + 1], m = sigmoid(om[p][18 groups + 9 g + k]) when modulated, else 1;
 * the layer is then the 1x1 convolution of cols (as (1, n*ho*wo, 1, 9 c)) with the (cout, 3, 3, c) weight. x (n,h,w,c) NHWC
 * contiguous f16 / bf16 / f32; om (n,ho,wo,ch) fp32, ch >= 18 groups (27 groups when modulated) the row pitch (channels beyond are
 * padding, not read); ho = (h - 1) / stride + 1, wo likewise; stride 1 or 2.
 * Bilinear rule at (hs, ws) on the h x w map: unless hs > -1, ws > -1, hs < h and ws < w the sample is 0 and nothing is read (NaN
 * and +-Inf coordinates included); else with h0 = floor(hs), lh = hs - h0 (w alike) the corners (h0,w0), (h0,w0+1), (h0+1,w0),
 * (h0+1,w0+1) weigh (1-lh)(1-lw), (1-lh) lw, lh (1-lw), lh lw, and a corner outside [0,h-1] x [0,w-1] contributes 0 and is not
 * read. Blend and mask multiply in fp32, one rounding to the storage dtype. No atomics, no workspace; one launch on `stream`.
 * c % 8 != 0, c % groups != 0, (c / groups) % 8 != 0, or n*ho*wo*9*c/8 >= 2^31: OSR_ERR_UNSUPPORTED with nothing launched. x and
 * cols 16-byte aligned. */
osr_status osr_deform_cols(const void* x, const float* om, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ho, int32_t wo,
                           int32_t ch, int32_t stride, int32_t groups, int32_t modulated, void* cols, int32_t dtype, void* stream);

/* fp32 GEMM out[m,n] = a[m,k] * w[n,k]^T + bias[n] on the exact-f32 MFMA (PLN encoder/decoder,
 * prototype_learning_network.py:204-205; cls_score, softmax_classifier.py:306). lda/ldo in elements. */
osr_status osr_gemm_f32(const float* a, int64_t lda, const float* w, const float* bias, float* out, int64_t ldo,
                        int32_t m, int32_t n, int32_t k, int32_t relu, void* stream);
/* fp32 out[m,n] = sum_k a[k,m] * b[k,n] on the exact-f32 MFMA: dW = dy^T x of the same layers in the training step (the
 * autograd backward of F.linear at prototype_learning_network.py:204-205, softmax_classifier.py:306), operands as they lie
 * (row = sample). The sample axis is split over workgroups when `workspace` holds osr_gemm_f32_tn_workspace_bytes(m,n,k);
 * the partial sums are added in split order. */
int64_t osr_gemm_f32_tn_workspace_bytes(int32_t m, int32_t n, int32_t k);
osr_status osr_gemm_f32_tn(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int32_t m,
                           int32_t n, int32_t k, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Split-precision fully connected layer: FastRCNNConvFCHead fc1 / fc2 (osrcnn_roi_heads.py:308) with the reference's fp32
 * operands, on the bf16 matrix instruction.   out = act(x * W^T + bias),  x (m, k) fp32, W (n, k) fp32, out (m, n) fp32.
 * Every fp32 value is carried as two bf16 terms, v = v0 + v1 with v0 = bf16(v), v1 = bf16(v - v0), both rounded to nearest
 * even (bf16 has fp32's exponent range: no scaling and no exponents), and the layer sums x0 w0 + x1 w0 + x0 w1 in fp32;
 * the x1 w1 term is dropped. Error against the exact product: about 2^-16 per product before the cancellation of the sum
 * (measured 4e-6 of the largest output at k = 12544: DESIGN.md section 4), inside the 1e-4 of the fp32 parity mode.
 *   osr_split_rows_bf16  splits a (rows, cols) fp32 matrix into its two (rows, cols) bf16 planes hi, lo: the static operand
 *                        W, once. host/weights.py split_fp32_rows is the same format in torch.
 *   osr_linear_split_fwd takes W as those planes and splits the rows of x on their way to the matrix cores.
 * k and n must be multiples of 64, anything else returns OSR_ERR_UNSUPPORTED with nothing launched; any m >= 1. ldx / ldo are
 * row strides in elements (multiples of 4); all pointers 16-byte aligned. row_seg_counts / row_seg_rows describe padded
 * per-image row lists exactly as in osr_conv_params: a 128-row tile without a data row is skipped and its output rows are left
 * unwritten; every other row is computed. Rows are independent: what a padding row of x holds (uninitialised memory, NaN)
 * reaches its own output row only. One workgroup sums the whole K axis of its tile in order (no atomics, no split-K): a launch
 * is bitwise reproducible. Non-finite inputs: an Inf or NaN in a row of x makes that output row non-finite, one in a row of W
 * that output column, and so does a finite value beyond bf16's largest (about 3.39e38), whose leading term rounds to Inf;
 * which elements exactly become Inf and which NaN is not specified. ReLU keeps a NaN.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct osr_linear_split_params {
    int32_t m, n, k;
    int32_t relu;
    int64_t ldx, ldo;
    const int32_t* row_seg_counts; /* optional (may be null), device memory */
    int32_t row_seg_rows;
    int32_t reserved;
} osr_linear_split_params;
osr_status osr_split_rows_bf16(const float* w, int32_t rows, int32_t cols, void* hi, void* lo, void* stream);
osr_status osr_linear_split_fwd(const osr_linear_split_params* p, const float* x, const void* w_hi, const void* w_lo,
                                const float* bias, float* out, void* stream);

/* The training half of the split-precision layer: the reference's fp32 backward of F.linear (FastRCNNConvFCHead fc1 / fc2) on the
 * same three bf16 products. Shapes name the LAYER: dy (m, n), x (m, k), W (n, k), all fp32 row-major, ld* in elements (multiples
 * of 4), pointers 16-byte aligned; n and k multiples of 64 or OSR_ERR_UNSUPPORTED with nothing launched; any m >= 1.
 *   osr_split_rows_bf16_t  w (rows, cols) fp32 -> the bf16 planes hi, lo of its TRANSPOSE (cols, rows): the operand of the data
 *                          gradient, refreshed from the fp32 master after an update (host/weights.py split_fp32_rows_t).
 *   osr_linear_split_dgrad dx[r][k] = (sum_n dy[r][n] W[n][k]) where mask[r][k] > 0, exactly 0 elsewhere (mask: the saved forward
 *                          output of the layer below, fp32, optional). dy is split on the fly; wt_hi / wt_lo are the (k, n) planes
 *                          of osr_split_rows_bf16_t, so both operands are contiguous along the reduction. Rows are independent
 *                          and row lists are handled as in osr_linear_split_fwd (all-padding 128-row tiles are skipped, their rows
 *                          of dx left unwritten).
 *   osr_linear_split_wgrad dW[n][k] = sum_r dy[r][n] x[r][k], dW fp32 in the forward layout. Both operands are split on the fly
 *                          (dy0 x0 + dy1 x0 + dy0 x1). With row_seg_counts (device, one count per row_seg_rows rows, covering
 *                          m) the rows at or beyond their segment's count contribute nothing whatever they hold (NaN included).
 *                          When `workspace` holds osr_linear_split_wgrad_workspace_bytes(m, n, k) the row axis is cut over
 *                          workgroups and the partial sums are added in cut order; without it one workgroup sums all rows of its
 *                          tile. No atomics either way: a launch is bitwise reproducible. */
osr_status osr_split_rows_bf16_t(const float* w, int32_t rows, int32_t cols, void* hi, void* lo, void* stream);
osr_status osr_linear_split_dgrad(const float* dy, int64_t lddy, const void* wt_hi, const void* wt_lo, const float* mask,
                                  int64_t ldmask, float* dx, int64_t lddx, int32_t m, int32_t n, int32_t k,
                                  const int32_t* row_seg_counts, int32_t row_seg_rows, void* stream);
int64_t osr_linear_split_wgrad_workspace_bytes(int32_t m, int32_t n, int32_t k);
osr_status osr_linear_split_wgrad(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dw, int64_t lddw,
                                  int32_t m, int32_t n, int32_t k, const int32_t* row_seg_counts, int32_t row_seg_rows,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Split-precision convolution: the Conv2d / FrozenBatchNorm2d (folded) layers of build_resnet_fpn_backbone and
 * ClsFreeRPNHead.conv (classification_free_rpn.py:158) with the reference's fp32 operands, on the bf16 matrix instruction.
 * The implicit GEMM of osr_conv2d_fwd with the arithmetic of osr_linear_split_fwd: in, out and residual are fp32 NHWC
 * (p->in_dtype and p->out_dtype must be OSR_F32), w_hi / w_lo are the two bf16 planes of the [cout][kh][kw][cin] fp32 weight
 * (osr_split_rows_bf16 / host/weights.py split_fp32_rows on its (cout, kh*kw*cin) matrix). The activations are split on their
 * way to the matrix cores, x0 = bf16(x), x1 = bf16(x - x0), and every K step sums x0 w1 + x1 w0 + x0 w0 into one fp32
 * accumulator; the x1 w1 term is dropped. Strides, padding, pad_mode, relu and res_mode mean what they mean for osr_conv2d_fwd
 * with fp32 operands; concurrency, workspace and row_seg_* are ignored.
 * Shapes: cin a multiple of 32, cout of 64; 1x1 and 3x3 kernels (pad < kernel size) at stride 1 or 2 with pad_mode 0, or the stem's
 * (kh = 8, kw = 1, cin = 32, stride 2, pad_mode 1) view of the pre-padded NHWC4 image osr_preprocess writes in fp32; any
 * n*ho*wo >= 1. Anything else returns OSR_ERR_UNSUPPORTED with nothing launched. Strides are multiples of 4 elements and all
 * pointers 16-byte aligned (OSR_ERR_INVALID_ARG otherwise).
 * A tap outside the image contributes exactly zero. One workgroup sums the whole K axis of its output tile in order (no
 * split-K, no atomics): a launch is bitwise reproducible and an output pixel's bits do not depend on the batch size. The
 * library allocates nothing. Non-finite inputs: an Inf or NaN in an input pixel makes every output pixel that reads it
 * non-finite, one in a weight row that output channel, and so does a finite value beyond bf16's largest (about 3.39e38),
 * whose leading term rounds to Inf; which elements exactly become Inf and which NaN is not specified. ReLU maps a NaN to 0,
 * as the fp32 kernel's does.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_conv2d_split_fwd(const osr_conv_params* p, const float* in, const void* w_hi, const void* w_lo,
                                const float* bias, const float* residual, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * CF-RPN head tail: ClsFreeRPNHead.forward after the 3x3 conv+ReLU (classification_free_rpn.py:159-161):
 * t/max(||t||_2,1e-12) over channels, 1x1 -> 4 ltrb deltas, 1x1 -> centerness, sigmoid.
 * t: (rows, c) channels-last hidden state; w_delta (4,c), w_ctr (1,c) fp32. Outputs fp32.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_cfrpn_head_tail(const void* t, int32_t t_dtype, int64_t rows, int32_t c, const float* w_delta,
                               const float* b_delta, const float* w_ctr, const float* b_ctr, float* deltas,
                               float* ctr, void* stream);

/* The whole ClsFreeRPNHead.forward for one pyramid level in ONE launch (classification_free_rpn.py:157-161):
 * 3x3 conv + bias + ReLU on MFMA, then -- without the hidden state ever leaving the chip -- the channel
 * L2-normalise, both 1x1 convs and the sigmoid. p describes the 3x3 convolution (cout must be 256, cin %% 64 == 0,
 * no residual; p->relu/out_* are ignored). w_tail: (5, 256) fp32, rows 0-3 = anchor_deltas, row 4 = centerness;
 * b_tail: (5). deltas/ctr are indexed by pixel (n*ho + oh)*wo + ow. Returns OSR_ERR_UNSUPPORTED outside that
 * envelope: run osr_conv2d_fwd + osr_cfrpn_head_tail instead. The tail's dot products and ||t||^2 also run on the matrix
 * cores (each tail row scaled by a power of two, then its fp32 weights as three storage-dtype terms each -- exact for every weight
 * within 2^-11 of its row's largest, at most 2^-35 of that largest off below --, fp32 accumulation, the scale undone on the
 * sums; subnormal fp16 terms are multiplied as they are): equal to the un-fused pair up to the fp32 summation order (1e-7
 * absolute on O(1) outputs), not bit for bit. */
osr_status osr_cfrpn_head_fwd(const osr_conv_params* p, const void* in, const void* weight, const float* bias,
                              const float* w_tail, const float* b_tail, float* deltas, float* ctr, void* stream);
/* TWO convolutions of the same input and geometry in ONE launch: [d2] BottleneckBlock.forward of a stage's first block applies
 * `self.conv1` (1x1, stride s, FrozenBN folded, ReLU) and `self.shortcut` (1x1, stride s, no ReLU) to the same x
 * (build_resnet_fpn_backbone selected by /root/reference/configs/Base-RCNN-FPN.yaml:3-8). p gives the shared geometry (n, hi, wi, cin,
 * ho, wo, kernel, stride, pad, input strides, dtypes); its cout / relu / out strides / residual fields are ignored. Convolution A
 * (w_a (cout_a, kh, kw, cin), bias_a, relu_a) writes the dense (n, ho, wo, cout_a) tensor out_a, B likewise; cout_a and cout_b are
 * multiples of 128, cin of 64, storage f16 / bf16. Bit-identical to two osr_conv2d_fwd launches that run on the 128 x 128 tile.
 * Returns OSR_ERR_UNSUPPORTED (nothing launched) outside that envelope. */
osr_status osr_conv2d_fwd_pair(const osr_conv_params* p, const void* in, const void* w_a, const float* bias_a, int32_t cout_a,
                               int32_t relu_a, void* out_a, const void* w_b, const float* bias_b, int32_t cout_b, int32_t relu_b,
                               void* out_b, void* stream);

/* One pyramid level of a multi-level launch: a dense NHWC input (n, hi, wi, cin) of the storage dtype and where its results go. */
typedef struct osr_conv_level {
    const void* in;   /* (n, hi, wi, cin), dense */
    void* out;        /* osr_conv2d_fwd_levels: (n, hi, wi, cout), dense, storage dtype. osr_cfrpn_head_fwd_levels: the hidden state
                       * t = relu(conv + bias), (n*hi*wi, 256) rows, or NULL */
    float* deltas;    /* osr_cfrpn_head_fwd_levels: (n*hi*wi, 4) ltrb deltas (osr_conv2d_fwd_levels: ignored) */
    float* ctr;       /* osr_cfrpn_head_fwd_levels: (n*hi*wi) centerness */
    const void* weight; /* the level's own (cout, kh, kw, cin) weights and (cout) fp32 bias -- the FPN has one output conv per level --, */
    const float* bias;  /* or NULL: the shared `weight` / `bias` arguments of the call */
    int32_t n, hi, wi;
    int32_t reserved;
} osr_conv_level;
#define OSR_MAX_CONV_LEVELS 6
/* Stride-1, same-padding K x K convolutions of ONE shape (kernel size, cin, cout) applied to several feature maps in ONE launch, each
 * level with its own weights (osr_conv_level.weight / .bias) or the shared `weight` / `bias` (may be NULL when every level brings its
 * own): [d2] FPN.forward's `output_conv(prev_features)` per level (the backbone build_resnet_fpn_backbone selected by
 * /root/reference/configs/Base-RCNN-FPN.yaml:3-8). p gives kh == kw (odd), pad == kh / 2, stride 1, cin, cout (multiple of 256),
 * dtypes (f16 / bf16 in and out) and relu; its n / hi / wi / ho / wo / strides / residual fields are ignored: every level is a dense
 * tensor described by its osr_conv_level. Outputs are bit-identical to osr_conv2d_fwd per level whenever that picks its 256 x 256 tile
 * (and equal within fp32 summation order otherwise: the split-K tail of a single-level launch adds its K ranges separately).
 * Why: at batch 16 the levels p2..p5 are 4200 + 1050 + 263 + 66 tiles of 256 x 256 rows x channels; launched one by one each level pays
 * its own partial last dispatch round on 256 CUs and the small levels leave most of the chip idle; one grid pays one. */
osr_status osr_conv2d_fwd_levels(const osr_conv_params* p, int32_t nlevels, const osr_conv_level* levels, const void* weight,
                                 const float* bias, void* stream);
/* ClsFreeRPNHead.forward over ALL pyramid levels in ONE launch (classification_free_rpn.py:157-161: `for x in features:` applies the
 * same conv / anchor_deltas / centerness weights to every level): osr_cfrpn_head_fwd's fused kernel on the 256-row tile with a level
 * table. Same envelope as osr_cfrpn_head_fwd (cout == 256, cin %% 64 == 0, >= 8 K slices); bit-identical to it per level whenever it
 * runs its 256-row tile (levels of >= 512 tiles), equal within fp32 summation order to its 128-row tile otherwise. */
osr_status osr_cfrpn_head_fwd_levels(const osr_conv_params* p, int32_t nlevels, const osr_conv_level* levels, const void* weight,
                                     const float* bias, const float* w_tail, const float* b_tail, void* stream);
/* The same, also writing the hidden state t = relu(conv + bias) in the storage dtype, (n*ho*wo, 256) rows (hidden_out may be
 * NULL): the training step keeps it for the head's backward (osr_cfrpn_tail_bwd, the 3x3 conv's weight gradient) instead of
 * running the un-fused pair that writes t and reads it back. */
osr_status osr_cfrpn_head_fwd_ex(const osr_conv_params* p, const void* in, const void* weight, const float* bias,
                                 const float* w_tail, const float* b_tail, float* deltas, float* ctr, void* hidden_out,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Proposal selection: ClsFreeRPN.predict_proposals -> _decode_proposals (classification_free_rpn.py:558-610)
 * + find_top_rpn_proposals (find_top_proposals.py:60-127) for all images and levels in two launches.
 * Level l holds ctr[l_off + img*hw_l*a + i] and deltas[(same)*4]. Per (image, level): stable top-k of
 * centerness (value-descending, lower index first), ltrb decode of the k survivors around their anchors
 * ([d2] DefaultAnchorGenerator + Box2BoxTransformLinear), finite filter, clip to the image, drop empty boxes;
 * levels concatenated level-major (no NMS, no cross-level re-sort: the reference has both commented out).
 * Outputs are padded to cap = osr_rpn_select_capacity(): boxes (n,cap,4), scores (n,cap), src_index (n,cap)
 * (index into the image's concatenated anchor list), batch_idx (n*cap: image id, -1 for padding), counts (n).
 * status_flags[0] is set non-zero when any non-finite prediction was met (training raises on it). A NaN score of
 * either sign ranks above every number in the top-k (torch.sort's order), so it is met, dropped and flagged.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct osr_rpn_levels {
    int32_t num_levels;
    int32_t num_anchors;            /* A: cell anchors per location */
    int32_t h[OSR_MAX_LEVELS];
    int32_t w[OSR_MAX_LEVELS];
    int32_t stride[OSR_MAX_LEVELS];
    int64_t offset[OSR_MAX_LEVELS]; /* element offset of level l in ctr (x4 in deltas) */
} osr_rpn_levels;

int32_t osr_rpn_select_capacity(const osr_rpn_levels* lv, int32_t pre_nms_topk);
int64_t osr_rpn_select_workspace_bytes(const osr_rpn_levels* lv, int32_t n, int32_t pre_nms_topk);
osr_status osr_rpn_select(const osr_rpn_levels* lv, const float* cell_anchors /* (L,A,4) */, const float* ctr,
                          const float* deltas, int32_t n, const int32_t* image_hw /* (n,2) */, int32_t pre_nms_topk,
                          float min_box_size, float* boxes, float* scores, int32_t* src_index, int32_t* batch_idx,
                          int32_t* counts, int32_t* status_flags, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* osr_rpn_select with the decode rule and an extra output selectable -- what the stock detectron2 RPN of
 * /root/reference/configs/Base-RCNN-FPN.yaml:9-21 (BASELINE config 1) needs next to the CF-RPN:
 * decode_mode 0 = [d2] Box2BoxTransformLinear (ltrb, the CF-RPN; reg_weights ignored), 1 = [d2] Box2BoxTransform with
 * reg_weights (dx,dy,dw,dh; dw/dh clamped at log(1000/16)) -- MODEL.RPN.BBOX_REG_WEIGHTS. `ctr` is then the objectness LOGIT
 * (top-k on the raw value, as [d2] find_top_rpn_proposals does). level_out (nullable): (n,cap) pyramid level of every kept
 * slot (-1 padding): the category of the per-level batched NMS that follows (osr_nms_topk, thr MODEL.RPN.NMS_THRESH). */
osr_status osr_rpn_select_ex(const osr_rpn_levels* lv, const float* cell_anchors, const float* ctr, const float* deltas,
                             int32_t n, const int32_t* image_hw, int32_t pre_nms_topk, float min_box_size,
                             int32_t decode_mode, const float reg_weights[4], float* boxes, float* scores,
                             int32_t* src_index, int32_t* batch_idx, int32_t* level_out, int32_t* counts,
                             int32_t* status_flags, void* workspace, int64_t workspace_bytes, void* stream);

/* osr_rpn_select_ex for a single-scale RPN ([d2] Base-RCNN-C4.yaml: one level, 15 anchors per cell, PRE_NMS_TOPK_TEST 6000): the
 * same contract word for word -- stable top-k (value descending, lower index first), NaN first and flagged, both decode modes,
 * level_out, padding -- with pre_nms_topk 1 .. OSR_RPN_SELECT_WIDE_MAXK. Above that: OSR_ERR_UNSUPPORTED, nothing launched (the
 * capacity / workspace queries return it too). For pre_nms_topk <= 2048 every output is bit-identical to osr_rpn_select_ex: the two
 * run one kernel, instantiated with a 2048-pair and an 8192-pair list in LDS (16 KiB / 64 KiB beside the 8 KiB histogram). */
#define OSR_RPN_SELECT_WIDE_MAXK 8192
int32_t osr_rpn_select_wide_capacity(const osr_rpn_levels* lv, int32_t pre_nms_topk);
int64_t osr_rpn_select_wide_workspace_bytes(const osr_rpn_levels* lv, int32_t n, int32_t pre_nms_topk);
osr_status osr_rpn_select_wide(const osr_rpn_levels* lv, const float* cell_anchors, const float* ctr, const float* deltas,
                               int32_t n, const int32_t* image_hw, int32_t pre_nms_topk, float min_box_size,
                               int32_t decode_mode, const float reg_weights[4], float* boxes, float* scores,
                               int32_t* src_index, int32_t* batch_idx, int32_t* level_out, int32_t* counts,
                               int32_t* status_flags, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * RoIAlign over the pyramid: [d2] ROIPooler.forward (level = floor(4+log2(sqrt(area)/224+1e-8)) clamped to
 * [min,max]) -> torchvision roi_align(aligned=True, sampling_ratio=0) (osrcnn_roi_heads.py:108-113,306).
 * feats[l]: (n, h_l, w_l, c) NHWC. boxes (m,4) fp32, batch_idx (m) (<0 => row of zeros).
 * out: (m, p, p, c) i.e. out[m][(ph*p+pw)*c + ch]  (the reference's (m,c,p,p) is the same data permuted;
 * the FC1 weight is permuted once at load time instead).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct osr_pyramid {
    int32_t num_levels;
    int32_t c;
    int32_t h[OSR_MAX_LEVELS];
    int32_t w[OSR_MAX_LEVELS];
    float scale[OSR_MAX_LEVELS];
    const void* data[OSR_MAX_LEVELS];
} osr_pyramid;

/* pooled: 1 .. OSR_ROI_MAX_POOLED_FWD for the four forward entry points (1..7: the box pooler's kernels; 8..14, the mask head's 14 x 14
 * pooler: a per-sample kernel of its own, same options, same order independence) and for the scatter backward (osr_roi_align_bwd /
 * _opt: 8..14 likewise through a per-sample kernel); the pixel-centric backward (osr_roi_align_bwd_dense / _opt) takes 1..7. */
#define OSR_ROI_MAX_POOLED_FWD 14
osr_status osr_roi_align_fwd(const osr_pyramid* feats, int32_t feat_dtype, int32_t n, const float* boxes,
                             const int32_t* batch_idx, int64_t m, int32_t pooled, int32_t canonical_level,
                             int32_t canonical_size, int32_t min_level, void* out, int32_t out_dtype, void* stream);

/* The same with an explicit processing order: `order` is a permutation of 0..m-1 (or NULL = list order); workgroup i pools RoI
 * order[i] into ITS OWN row out[order[i]], so the result is bit-identical for every order. `order_nvalid` (device pointer, may
 * be NULL): the number of leading entries of `order` that are real RoIs, the rest being padding rows (batch index -1): the
 * kernel then gives every XCD the same share of the real work. osr_roi_locality_order fills both so that RoIs that are
 * neighbours in the image are neighbours in time on one XCD (bucket sort by image, pyramid level and 32x32-pixel tile of the box
 * centre; the level rule is the one of osr_roi_align_fwd; padding rows last): the proposals of an image overlap each other
 * several times over, and in score order every overlap is a re-read from HBM.
 * workspace: osr_roi_locality_order_workspace_bytes(n, m) bytes. */
osr_status osr_roi_align_fwd_ordered(const osr_pyramid* feats, int32_t feat_dtype, int32_t n, const float* boxes,
                                     const int32_t* batch_idx, int64_t m, int32_t pooled, int32_t canonical_level,
                                     int32_t canonical_size, int32_t min_level, const int32_t* order,
                                     const int32_t* order_nvalid, void* out, int32_t out_dtype, void* stream);
/* osr_roi_align_fwd_ordered with flags. OSR_ROI_NO_PADDING_FILL: padding rows (batch index -1) are left UNWRITTEN instead of
 * zero-filled -- for a caller whose consumers never read them (the engine: the box head skips or ignores those rows; a fifth of the
 * benchmark's list, 0.37 GB of zeros per step). */
#define OSR_ROI_NO_PADDING_FILL 1
osr_status osr_roi_align_fwd_ordered_ex(const osr_pyramid* feats, int32_t feat_dtype, int32_t n, const float* boxes,
                                        const int32_t* batch_idx, int64_t m, int32_t pooled, int32_t canonical_level,
                                        int32_t canonical_size, int32_t min_level, const int32_t* order,
                                        const int32_t* order_nvalid, int32_t flags, void* out, int32_t out_dtype, void* stream);
/* Pooler options: the two ROI_BOX_HEAD keys beside the resolution that [d2] ROIPooler hands to roi_align.
 * aligned: 1 = POOLER_TYPE "ROIAlignV2" (pixel centres at +0.5: box * scale - 0.5, no minimum size); 0 = "ROIAlign" (no offset, and the
 *   RoI's width and height in level pixels are clamped to at least 1 before the bin size is taken).
 * sampling_ratio: 0 = adaptive grid, ceil(roi / pooled) samples per bin and axis; S > 0 = a fixed S x S grid per bin, whose divisor is
 *   S * S whether or not a sample is valid.
 * A zero-area box pools to zeros under {1, 0} (its adaptive grid is 0 x 0) and to the bilinear value at its point under every other
 * pair. NULL means {1, 0}, for which every _opt entry point computes bit for bit what the entry point without options computes (it
 * runs the same kernel). Any other `aligned`, or a sampling_ratio outside 0 .. OSR_ROI_MAX_SAMPLING_RATIO (the sample loops are
 * O(S) per table entry and S * S is the divisor): OSR_ERR_INVALID_ARG, nothing launched. Level assignment,
 * the validity rule (a sample outside [-1, size] on an axis contributes nothing) and the edge clamps do not depend on the options. */
#define OSR_ROI_MAX_SAMPLING_RATIO 64
typedef struct osr_roi_options {
    int32_t aligned;
    int32_t sampling_ratio;
} osr_roi_options;
/* osr_roi_align_fwd_ordered_ex with pooler options. */
osr_status osr_roi_align_fwd_ordered_opt(const osr_pyramid* feats, int32_t feat_dtype, int32_t n, const float* boxes,
                                         const int32_t* batch_idx, int64_t m, int32_t pooled, int32_t canonical_level,
                                         int32_t canonical_size, int32_t min_level, const int32_t* order,
                                         const int32_t* order_nvalid, int32_t flags, const osr_roi_options* options, void* out,
                                         int32_t out_dtype, void* stream);
/* osr_roi_align_fwd_ordered_opt for a consumer that reads every bin_stride-th bin only ([d2] Res5ROIHeads with STRIDE_IN_1X1: res5's
 * first block enters through two 1 x 1 convolutions of stride 2, which read the even bins of the 14 x 14 grid and nothing else).
 * out is (m, q, q, c) with q = ceil(pooled / bin_stride) and holds bins (bin_stride * i, bin_stride * j) of the pooled x pooled grid,
 * each bit-identical to the same bin of osr_roi_align_fwd_ordered_opt; the other bins are neither sampled nor written.
 * bin_stride 1 is that call. bin_stride 2 is served for pooled 8 .. OSR_ROI_MAX_POOLED_FWD (the per-sample kernel); any other
 * pair returns OSR_ERR_UNSUPPORTED with nothing launched. Options, flags, padding rule and order independence as there. */
osr_status osr_roi_align_fwd_strided(const osr_pyramid* feats, int32_t feat_dtype, int32_t n, const float* boxes,
                                     const int32_t* batch_idx, int64_t m, int32_t pooled, int32_t bin_stride, int32_t canonical_level,
                                     int32_t canonical_size, int32_t min_level, const int32_t* order,
                                     const int32_t* order_nvalid, int32_t flags, const osr_roi_options* options, void* out,
                                     int32_t out_dtype, void* stream);
/* Mean over the positions of a RoI ([d2] Res5ROIHeads: res5's output .mean(dim=[2, 3]), the input of box_predictor).
 * x: (r, s, c) in `dtype`, the s positions of a RoI, channels last. out: (r, c) fp32 = (the sum over the positions in ascending
 * order, accumulated in fp32) / s. rows_valid / seg_rows: as osr_mask_upsample_predict; RoIs that do not exist are written as zeros
 * and their x is not read. c a multiple of 4, s 1 .. 196: anything else is OSR_ERR_UNSUPPORTED with nothing launched. x and out
 * 16-byte aligned. r == 0 launches nothing. No atomics: repeats are bit-identical. */
osr_status osr_avgpool_rows(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t c, const int32_t* rows_valid,
                            int32_t seg_rows, float* out, void* stream);
int64_t osr_roi_locality_order_workspace_bytes(int32_t n, int64_t m);
osr_status osr_roi_locality_order(const osr_pyramid* feats, int32_t n, const float* boxes, const int32_t* batch_idx, int64_t m,
                                  int32_t canonical_level, int32_t canonical_size, int32_t min_level, int32_t* order,
                                  int32_t* nvalid, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Box predictor tail: OpensetFastRCNNOutputLayers.forward + predict_boxes + predict_ious
 * (osrcnn_fast_rcnn.py:262-263,423,443-446) and the per-row part of fast_rcnn_inference_single_image
 * (:109-126): deltas = x W_b^T + b, iou = sigmoid(x w_i + b), box = Box2BoxTransform.apply_deltas (weights
 * wx,wy,ww,wh; scale clamp log(1000/16)), score = sqrt(iou*ctr) (mean_type 0) or (iou+ctr)/2 (1), finite filter,
 * clip, score > thresh. x: (m, k) fp32 box-head features. w: (5,k): rows 0-3 bbox_pred, row 4 iou_pred.
 * Outputs: pred_deltas (m,4) raw, pred_iou (m), boxes (m,4) clipped, score (m), cand (m) int32 0/1.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_box_predictor_tail(const float* x, int64_t m, int32_t k, const float* w, const float* b,
                                  const float* proposals, const float* ctr, const int32_t* batch_idx,
                                  const int32_t* image_hw, const float reg_weights[4], int32_t mean_type,
                                  float score_thresh, float* pred_deltas, float* pred_iou, float* boxes,
                                  float* score, int32_t* cand, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Segmented stable sort + greedy per-class NMS + top-k: [d2] detectron2.layers.batched_nms -> torchvision
 * nms (osrcnn_fast_rcnn.py:135-137; softmax_classifier.py:93-95,154-156), vanilla per-class semantics:
 * candidates ordered by score descending (ties: lower index first); a candidate is suppressed by an already
 * kept one of the same class when inter/(a_i+a_j-inter) > thr; the first `topk` kept are returned, in order.
 * thr >= 1 suppresses nothing (pure sort + top-k). Segment s covers elements
 * [s*seg_stride, s*seg_stride + seg_len[s]) of boxes/scores/cls/cand; cand==0 elements are skipped.
 * keep: (num_segments, topk) indices relative to the segment start; keep_count: (num_segments).
 * With thr < 1 the kept boxes sit in LDS: topk <= 2048 (OSR_ERR_UNSUPPORTED above; up to 1024 the kernel with the 1024-entry table).
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_nms_topk_workspace_bytes(int32_t num_segments, int64_t seg_stride);
osr_status osr_nms_topk(const float* boxes, const float* scores, const int32_t* cls /* nullable: one class */,
                        const int32_t* cand /* nullable: all */, int32_t num_segments, int64_t seg_stride,
                        const int32_t* seg_len, float thr, int32_t topk, int32_t* keep, int32_t* keep_count,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Gather rows: dst[s, j, :] = src[s*seg_stride + keep[s, j], :] for j < keep_count[s], else 0
 * (boxes[keep], scores[keep], feats[keep] at osrcnn_fast_rcnn.py:138). row_elems fp32 elements per row. */
osr_status osr_gather_rows(const float* src, int64_t seg_stride, int32_t row_elems, const int32_t* keep,
                           const int32_t* keep_count, int32_t num_segments, int32_t topk, float* dst, void* stream);

/* Row-wise L2 normalisation x/max(||x||,1e-12) (F.normalize; prototype_learning_network.py:199). */
osr_status osr_l2_normalize_rows(const float* x, int32_t rows, int32_t d, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * PLN inference tail (prototype_learning_network.py:206-223, COS distance): normalise each embedding, cosine
 * distance to the (already normalised) prototypes, min over reps then min/argmin over classes (ties: lower
 * class), unknown if min > unk_thr. class_map (nullable, (num_known)): GraspNet class_id remap (:222).
 * emb: (rows, d). rows_valid (nullable): per-segment valid counts for padded (segments, seg_rows) layouts
 * (rows must then be a multiple of seg_rows: OSR_ERR_INVALID_ARG otherwise); padded rows get class -1 and
 * distance 0. Outputs: pred_class (rows) int64, min_dist (rows).
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_pln_tail(const float* emb, int64_t rows, int32_t d, const float* protos_normed, int32_t num_known,
                        int32_t reps, float unk_thr, int64_t unknown_id, const int64_t* class_map,
                        const int32_t* rows_valid, int32_t seg_rows, int64_t* pred_class, float* min_dist,
                        void* stream);
/* MODEL.PLN.DISTANCE_TYPE (prototype_learning_network.py:155-160, 213-218): the distance between the normalised embedding and
 * the normalised prototypes. osr_pln_tail / osr_pln_loss_fwd / osr_pln_loss_bwd are the COS forms with one prototype per class. */
enum { OSR_PLN_DIST_COS = 0, OSR_PLN_DIST_L1 = 1, OSR_PLN_DIST_L2 = 2 };
osr_status osr_pln_tail_ex(const float* emb, int64_t rows, int32_t d, const float* protos_normed, int32_t num_known,
                           int32_t reps, int32_t distance_type, float unk_thr, int64_t unknown_id,
                           const int64_t* class_map, const int32_t* rows_valid, int32_t seg_rows, int64_t* pred_class,
                           float* min_dist, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Softmax classifier candidates: SoftMaxClassifier.inference up to the NMS calls (softmax_classifier.py:300-307,
 * 66-88, 126-149). Per image (segment of seg_rows detections, det_count[s] valid): known detections
 * (pred_class != unknown_id): softmax over num_known+1 logits, drop the background column, candidate for every
 * (det, class) with prob > known_thresh in row-major order; unknown detections: candidate if objectness score >
 * unknown_thresh. Candidate arrays are padded per image: known cap = seg_rows*num_known, unknown cap = seg_rows.
 * Outputs (k = known, u = unknown): *_boxes (n,cap,4), *_scores (n,cap), k_cls (n,cap) int32, *_det (n,cap)
 * int32 source detection, *_count (n).
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_softmax_candidates(const float* logits, int32_t num_known, const float* det_boxes,
                                  const float* det_scores, const int64_t* pred_class, const int32_t* det_count,
                                  int32_t n, int32_t seg_rows, int64_t unknown_id, float known_thresh,
                                  float unknown_thresh, float* k_boxes, float* k_scores, int32_t* k_cls, int32_t* k_det,
                                  int32_t* k_count, float* u_boxes, float* u_scores, int32_t* u_det, int32_t* u_count,
                                  void* stream);

/* [d2] FastRCNNOutputLayers.inference -> fast_rcnn_inference_single_image up to (not including) the NMS, for the stock
 * StandardROIHeads of /root/reference/configs/Base-RCNN-FPN.yaml:22-28 (BASELINE config 1). logits (n*seg_rows, K+1),
 * deltas (n*seg_rows, R*4) with R = num_bbox_reg_classes (K, or 1 when class-agnostic), prop_boxes (n, seg_rows, 4) padded with
 * prop_count (n) valid rows. Per valid row: softmax; Box2BoxTransform(reg_weights) decode of every class's box; the row is
 * dropped when any box coordinate or probability is non-finite; boxes clipped to image_hw; every (row, class < K) with
 * p > score_thresh becomes a candidate, row-major. Outputs padded to seg_rows*K per image: c_boxes (n,cap,4), c_scores,
 * c_cls, c_row (proposal row of the candidate), c_count (n). Follow with osr_nms_topk(cls = c_cls, thr NMS_THRESH_TEST,
 * topk DETECTIONS_PER_IMAGE). */
osr_status osr_fastrcnn_candidates(const float* logits, const float* deltas, int32_t num_classes,
                                   int32_t num_bbox_reg_classes, const float* prop_boxes, const int32_t* prop_count,
                                   int32_t n, int32_t seg_rows, const int32_t* image_hw, const float reg_weights[4],
                                   float score_thresh, float* c_boxes, float* c_scores, int32_t* c_cls, int32_t* c_row,
                                   int32_t* c_count, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * [d2] CascadeROIHeads (Cascade R-CNN; csrc/osr_cascade.hip, csrc/osr_det_tail.hip): the glue between the stages, on the stock engine's fixed-capacity
 * row lists. m = n * seg_rows rows; row r belongs to image r / seg_rows and exists iff batch_idx[r] >= 0. No compaction, no
 * atomics, no host sync; repeats are bit-identical.
 *
 * osr_cascade_refine: one launch per stage transition ([d2] predict_boxes + _create_proposals_from_boxes +
 * _match_and_label_boxes). Per existing row: Box2BoxTransform(reg_weights).apply_deltas of the stage's class-agnostic deltas (m,4)
 * on the stage's input box, clipped to the row's image_hw (a NaN stays a NaN). drop_empty (training): a row whose clipped box has
 * width <= 0 or height <= 0 (or a NaN there) stops existing: batch_idx_out -1, class -1, a zero box. Without it (inference) every
 * existing row stays, so the stages' scores stay aligned. gt_boxes (n,gmax,4) / gt_classes (n,gmax) / gt_count (n) -- all NULL at
 * inference, the three matching outputs are then not written and may be NULL --: pairwise_iou in fp32 against the image's boxes
 * (inter / (a1 + a2 - inter) where inter > 0, else 0), the maximum with the lowest index among equal IoUs; foreground iff the
 * maximum >= iou_thr (Matcher([thr], [0, 1]), no low-quality matches): classes_out int64 = the matched class (background:
 * num_classes), gt_boxes_out = the matched box (on background rows too; zeros when gt_count is 0), gt_idx_out = the matched index
 * (-1 off foreground). counts (n,3) = {rows, foreground, background} (foreground / background 0 without ground truth).
 * gmax <= 1024: an image's ground truth sits in a static LDS table; OSR_ERR_INVALID_ARG above it. Not in place.
 *
 * osr_cascade_candidates: osr_fastrcnn_candidates for num_stages <= OSR_CASCADE_MAX_STAGES stages. logits[s] (m, K+1) for
 * s < num_stages (a host array of device pointers), the last stage's deltas (m,4) and input boxes (m,4). Per existing row: softmax
 * of each stage in fp32, score = ((p0 + p1) + p2 ...) * (float)(1.0 / num_stages); decode with reg_weights, clip; the row is
 * dropped when any box coordinate or score is non-finite; every (row, class < K) with score > score_thresh becomes a candidate,
 * row-major. Outputs and padding as osr_fastrcnn_candidates; with one stage they are bit-identical to it.
 * --------------------------------------------------------------------------------------------------------- */
#define OSR_CASCADE_MAX_STAGES 4
osr_status osr_cascade_refine(const float* boxes, const int32_t* batch_idx, const float* deltas, int32_t n, int32_t seg_rows,
                              const int32_t* image_hw, const float reg_weights[4], int32_t drop_empty, const float* gt_boxes,
                              const int64_t* gt_classes, const int32_t* gt_count, int32_t gmax, int32_t num_classes,
                              float iou_thr, float* boxes_out, int32_t* batch_idx_out, int64_t* classes_out,
                              float* gt_boxes_out, int32_t* gt_idx_out, int32_t* counts, void* stream);
osr_status osr_cascade_candidates(const float* const* logits, int32_t num_stages, const float* deltas, int32_t num_classes,
                                  const float* boxes, const int32_t* batch_idx, int32_t n, int32_t seg_rows,
                                  const int32_t* image_hw, const float reg_weights[4], float score_thresh, float* c_boxes,
                                  float* c_scores, int32_t* c_cls, int32_t* c_row, int32_t* c_count, void* stream);

/* Final assembly: output order [unknown..., known...] (softmax_classifier.py:328-334), class ids int64
 * (unknown_id for the unknown group, class_map[c] or c for known). out_* padded to (n, u_topk + k_topk). */
osr_status osr_assemble_detections(const float* k_boxes, const float* k_scores, const int32_t* k_cls,
                                   const int32_t* k_keep, const int32_t* k_keep_count, int64_t k_stride, int32_t k_topk,
                                   const float* u_boxes, const float* u_scores, const int32_t* u_keep,
                                   const int32_t* u_keep_count, int64_t u_stride, int32_t u_topk, int32_t n,
                                   int64_t unknown_id, const int64_t* class_map, float* out_boxes, float* out_scores,
                                   int64_t* out_classes, int32_t* out_count, void* stream);

/* [d2] detector_postprocess on the device (the step after the path): per image, boxes * (scale_x, scale_y),
 * clip to (out_h, out_w), drop boxes without positive width and height, keep the order. In/out: padded (n, cap, .) + counts;
 * scale_xy (n,2) = {out_w / w, out_h / h}; out_hw (n,2) = {out_h, out_w}. Not in place. */
osr_status osr_detector_postprocess(const float* boxes, const float* scores, const int64_t* classes, const int32_t* count,
                                    int32_t n, int32_t cap, const float* scale_xy, const int32_t* out_hw, float* out_boxes,
                                    float* out_scores, int64_t* out_classes, int32_t* out_count, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Mask head tail ([d2] MaskRCNNConvUpsampleHead.deconv + ReLU + predictor, mask_rcnn_inference; csrc/osr_mask_head.hip).
 * x: (r, s, s, cin) NHWC in `dtype` (the output of the mask_fcn convolutions). One launch computes
 * ConvTranspose2d(cin -> cmid, 2 x 2, stride 2) + bias + ReLU, the 1 x 1 predictor row of each RoI's class and the sigmoid:
 * probs (r, 2s, 2s) fp32. The (r, 2s, 2s, cmid) intermediate is never stored; it stays in fp32 up to the dot product.
 * w_packed: the deconv weight in `dtype`, in MFMA fragment order (host/weights.py pack_deconv_weight): with t = 2 dy + dx and
 *   E = 8 (f16 / bf16) or 4 (f32), element [t][n / 32][k / 2E][(k / E) % 2][n % 32][k % E] = weight[k][n][dy][dx].
 * bias (cmid), pred_w (num_rows, cmid), pred_b (num_rows): fp32. num_rows == 1: class-agnostic, row 0 for every RoI with class >= 0
 * (classes may be NULL: every RoI); otherwise row classes[i].
 * rows_valid / seg_rows: as osr_pln_tail -- the RoIs are segments of seg_rows of which the first rows_valid[segment] exist (NULL:
 * all exist). RoIs that do not exist, and RoIs whose class is negative or not a predictor row, are written as zeros.
 * cin, cmid: multiples of 64, cin <= 448. r == 0: OSR_OK without a launch. Repeats are bit-identical. */
osr_status osr_mask_upsample_predict(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t cmid,
                                     const void* w_packed, const float* bias, const float* pred_w, const float* pred_b,
                                     int32_t num_rows, const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows,
                                     float* probs, void* stream);
/* The same launch with a second output, logits (r, 2s, 2s) fp32: the class row's logit before the sigmoid (zeros where probs are
 * zeros) -- what the training loss reads. Either of probs / logits may be NULL, not both; probs are bit-identical to the call above. */
osr_status osr_mask_upsample_predict_ex(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t cmid,
                                        const void* w_packed, const float* bias, const float* pred_w, const float* pred_b,
                                        int32_t num_rows, const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows,
                                        float* probs, float* logits, void* stream);
/* [d2] paste_masks_in_image (_do_paste_mask, skip_empty=False) for ONE image: probs (r, m, m) fp32, boxes (r, 4) at the output
 * resolution -> out (r, out_h, out_w) uint8, 1 where the bilinear sample (zeros outside the map) of mask i at
 * u = (x + 0.5 - x0) / (x1 - x0) * m - 0.5, v likewise, is >= threshold, else 0. Every byte of out is written. r <= 65535. */
osr_status osr_paste_masks(const float* probs, const float* boxes, int64_t r, int32_t m, int32_t out_h, int32_t out_w,
                           float threshold, uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Keypoint branch ([d2] KRCNNConvDeconvUpsampleHead's tail and heatmaps_to_keypoints; csrc/osr_keypoint.hip). detectron2 is not at
 * hand: the semantics are stated here and are the contract.
 *
 * osr_keypoint_upsample: x (r, s, s, cin) NHWC in `dtype` (the output of the last conv_fcn). One launch computes
 *   low[r, j, oy, ox] = bias[j] + sum over c, ky, kx of x[r, iy, ix, c] * w[c, j, ky, kx]   over the taps with oy = 2 iy - 1 + ky,
 *   ox = 2 ix - 1 + kx, 0 <= iy, ix < s  (ConvTranspose2d(cin -> k, 4 x 4, stride 2, padding 1): a 2s x 2s map),
 * then bilinear x2 with align_corners = false (source (d + 0.5) / 2 - 0.5 clamped below at 0, second tap min(i0 + 1, 2s - 1)):
 * heatmaps (r, k, 4s, 4s) fp32. The 2s x 2s map stays on chip in fp32; the contraction runs on the MFMA with k padded to 32.
 * w_packed: the score_lowres weight (cin, k, 4, 4) in `dtype`, in MFMA fragment order (host/weights.py
 *   pack_keypoint_deconv_weight): with E = 8 (f16 / bf16) or 4 (f32), element [ky * 4 + kx][c / 2E][(c / E) % 2][j (32)][c % E] =
 *   w[c][j][ky][kx], zeros for j >= k: 16 * cin * 32 elements.
 * bias (k) fp32. rows_valid / seg_rows: as osr_mask_upsample_predict; RoIs that do not exist are written as zeros.
 * cin a multiple of 64, at most 512; k 1 .. 32; s 8 .. 14: anything else is OSR_ERR_UNSUPPORTED with nothing launched. x, w_packed
 * and heatmaps are 16-byte aligned. r == 0: OSR_OK without a launch. Repeats are bit-identical.
 *
 * osr_heatmaps_to_keypoints: maps (r, k, m, m) fp32, m <= 56; rois (r, 4) xyxy; out (r, k, 4) = {x, y, logit, score}. Per RoI
 * w = max(x1 - x0, 1), h likewise, wc = ceil(w), hc = ceil(h) (a side above 16384 px counts as 16384). U is the bicubic resize of
 * the map to hc x wc by F.interpolate(mode="bicubic", align_corners=False)'s rules: source (m / wc) * (d + 0.5) - 0.5 (not clamped),
 * t = src - floor(src), Keys' cubic convolution with A = -0.75 over the taps floor(src) - 1 .. + 2, tap indices clamped to
 * [0, m - 1]. p = the first row-major position of max U (ties: the lowest y * wc + x);
 *   x = (px + 0.5) * (w / wc) + x0,  y = (py + 0.5) * (h / hc) + y0,  logit = U[p],
 *   score = 1 / sum over the m x m INPUT map of exp(map - U[p]).
 * U is never stored. RoIs that do not exist (rows_valid / seg_rows as above) are written as zeros. r == 0 launches nothing. Repeats
 * are bit-identical.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_keypoint_upsample(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t k,
                                 const void* w_packed, const float* bias, const int32_t* rows_valid, int32_t seg_rows,
                                 float* heatmaps, void* stream);
osr_status osr_heatmaps_to_keypoints(const float* maps, const float* rois, int64_t r, int32_t k, int32_t m,
                                     const int32_t* rows_valid, int32_t seg_rows, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Mask branch, training ([d2] mask_rcnn_loss; csrc/osr_mask_train.hip). The mask rows are the foreground prefix of each image's
 * sampled proposals: n segments of seg_rows rows of which the first rows_valid[image] exist (osr_roi_match_and_sample_ex writes an
 * image's foreground rows first; rows_valid = its foreground count, seg_rows = int(batch_size * positive_fraction)).
 *
 * osr_mask_targets ([d2] BitMasks.crop_and_resize): gt_masks (n, gmax, hm, wm) uint8 planes (non-zero = inside), padded with zeros
 * to the batch's image size; image_hw (n, 2) int32 {h, w} of each image (NULL: every image is hm x wm) -- the validity and clamp
 * rules of the samples are those of the image's own bitmask. boxes (n * seg_rows, 4), gt_idx (n * seg_rows) int32.
 * targets[r] (m_side, m_side) uint8 = roi_align(plane[image][gt_idx[r]] as float, boxes[r], m_side x m_side, scale 1,
 * sampling_ratio 0, aligned) >= 0.5, evaluated in fp32 in the reference loop's order. Rows that do not exist, rows whose gt_idx is
 * outside [0, gmax) and rows whose box is not finite are zeros. m_side <= 256.
 *
 * osr_mask_loss_fwd: logits (rows, m_side, m_side) fp32 (each row's own predictor channel), targets as above. A row counts when
 * it exists (rows_valid / seg_rows; NULL: all exist) and its class is a predictor row: classes[r] in [0, num_rows), or >= 0 when
 * num_rows == 1 (class-agnostic; classes may then be NULL). out6 = {loss_mask, foreground rows, incorrect, positive,
 * false positive, false negative}: loss_mask = loss_weight * sum of max(l,0) - l*t + log1p(exp(-|l|)) over the counted rows'
 * pixels / max(their number, 1) -- exactly 0 without a counted row; the other four count pixels with (l > 0) != t, t, both without
 * t and both with t. workspace 6 KiB. At most 2^24 pixels in all (the counts are exact). Repeats are bit-identical.
 * osr_mask_loss_bwd: d_logits (rows, m_side, m_side) = (sigmoid(l) - t) * scale / max(foreground rows * m_side^2, 1) on counted
 * rows, exact zeros elsewhere; every element written. workspace 16 bytes.
 * rows == 0 (logits, targets and classes may then be NULL whatever num_rows): out6 is six zeros, d_logits is not touched.
 *
 * osr_mask_upsample_predict_bwd: the backward of osr_mask_upsample_predict_ex's logits, same x / w_packed / bias / pred_w /
 * num_rows / classes / rows_valid / seg_rows contract, fp16 / bf16, cin <= 448, s >= 8 (a tile of 64 rows reaches at most two RoIs).
 * It recomputes u = deconv(x) + bias per tile on the MFMA exactly as the forward does and, with
 * g[pix, n] = d_logits[pix] * pred_w[class][n] * (u > 0) taken from the fp32 accumulators, writes
 *   dx (r, s, s, cin) in dx_dtype (`dtype`, or OSR_F32): sum over the four taps and n of g W -- a second MFMA contraction, g rounded to `dtype`; its B
 *     operand w_packed_t is the deconv weight packed with cin and cmid exchanged (pack_deconv_weight of weight.transpose(0, 1));
 *   g_out (P * 4, r * s * s, cmid) in `dtype`, plane- then tap-major (t = 2 dy + dx), or NULL. P = 1 for fp16; P = 2 for bf16, whose g
 *     enters both contractions as hi = bf16(g) and lo = bf16(g - hi) (8 bits alone cost 2e-3 of the gradients' magnitude). The
 *     deconv weight gradient is then 1 x 1 osr_conv2d_wgrad calls of x against g_out[p * 4 + t], summed over p;
 *   d_pred_w (num_rows, cmid), d_pred_b (num_rows), d_deconv_b (cmid) fp32: per-workgroup partials in the workspace reduced in a
 *     fixed order (per RoI in tile order, per class in RoI order) -- no atomics, repeats are bit-identical.
 * RoIs that do not exist or whose class is not a predictor row contribute exact zeros everywhere. r == 0: zeros in the three
 * parameter gradients.
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_mask_upsample_predict_bwd_workspace_bytes(int64_t r, int32_t s, int32_t cmid);
osr_status osr_mask_upsample_predict_bwd(const void* x, int32_t dtype, int64_t r, int32_t s, int32_t cin, int32_t cmid,
                                         const void* w_packed, const void* w_packed_t, const float* bias, const float* pred_w,
                                         int32_t num_rows, const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows,
                                         const float* d_logits, void* dx, int32_t dx_dtype, void* g_out, float* d_pred_w, float* d_pred_b,
                                         float* d_deconv_b, void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_mask_targets(const uint8_t* gt_masks, int32_t n, int32_t gmax, int32_t hm, int32_t wm, const int32_t* image_hw,
                            const float* boxes, const int32_t* gt_idx, const int32_t* rows_valid, int32_t seg_rows,
                            int32_t m_side, uint8_t* targets, void* stream);
osr_status osr_mask_loss_fwd(const float* logits, const uint8_t* targets, int64_t rows, int32_t m_side, int32_t num_rows,
                             const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows, float loss_weight, float* out6,
                             void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_mask_loss_bwd(const float* logits, const uint8_t* targets, int64_t rows, int32_t m_side, int32_t num_rows,
                             const int64_t* classes, const int32_t* rows_valid, int32_t seg_rows, float scale, float* d_logits,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Test-time augmentation glue ([d2] modeling/test_time_augmentation.py GeneralizedRCNNWithTTA; csrc/osr_tta.hip), over the padded
 * detection lists (n, topk, .) + counts (n) of one engine pass. An augmentation of an input with image (hi, wi) and output resolution
 * (ho, wo) is the transform list [resize (ho, wo) -> (hi, wi), only when the two differ], resize (hi, wi) -> (ha, wa), [hflip(wa)].
 * sizes: (n, 4) int32 {hi, wi, ho, wo} per image. fp32 arithmetic per coordinate as [d2]'s numpy: a resize multiplies x by
 * (float)((double)w' / w) and y by (float)((double)h' / h), a flip is (float)wa - x, the box is (min x, min y, max x, max y) of its
 * corners after each step, nothing is fused across steps. boxes, sizes and the box outputs are 16-byte aligned.
 *
 * osr_tta_boxes_to_original (_inverse_augment_boxes + the per-row part of fast_rcnn_inference_single_image(.., 1e-8, ..)): the inverse
 * list, then clip x to [0, wo] and y to [0, ho]. Writes rows [slot, slot + topk) of every image's candidate list of `cap` rows
 * (cap >= slot + topk; A augmentations fill cap = A * topk): c_boxes (n, cap, 4), c_scores (n, cap), c_cls (n, cap) int32,
 * c_cand (n, cap) int32 = the row exists && every mapped coordinate and the score are finite && score > 1e-8. Rows beyond an
 * image's count: zeros, class -1, cand 0. Follow with osr_nms_topk(cls = c_cls, cand = c_cand, thr NMS_THRESH_TEST, topk
 * DETECTIONS_PER_IMAGE) and osr_gather_rows.
 * osr_tta_boxes_to_augmented (_rescale_detected_boxes): boxes in (ho, wo) space through the forward list, not clipped; rows beyond
 * an image's count are zeros.
 * osr_tta_reduce_masks (_reduce_pred_masks): maps (A, n, topk, m, m) fp32, flip (A) int32 0 / 1 in device memory -> out (n, topk, m, m):
 * the maps of flipped augmentations mirrored along their last axis, summed in fp32 in augmentation order, divided by A; rows beyond
 * an image's count are zeros. Repeats are bit-identical.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_tta_boxes_to_original(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts,
                                     const int32_t* sizes, int32_t n, int32_t topk, int32_t ha, int32_t wa, int32_t flip,
                                     int32_t slot, int32_t cap, float* c_boxes, float* c_scores, int32_t* c_cls,
                                     int32_t* c_cand, void* stream);
osr_status osr_tta_boxes_to_augmented(const float* boxes, const int32_t* counts, const int32_t* sizes, int32_t n, int32_t topk,
                                      int32_t ha, int32_t wa, int32_t flip, float* out, void* stream);
osr_status osr_tta_reduce_masks(const float* maps, const int32_t* flip, int32_t num_aug, const int32_t* counts, int32_t n,
                                int32_t topk, int32_t m, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * RetinaNet inference tail: [d2] RetinaNet.inference_single_image before its batched NMS, for all images and levels in two
 * launches (csrc/osr_retinanet.hip). detectron2 is not at hand: the semantics are written from memory of detectron2 v0.6, and
 * THIS TEXT is the contract the tests check.
 * Inputs: lv with num_anchors = A (offset[l] counts anchors, a multiple of A: level l starts offset[l] / A cells into both
 * buffers); cell_anchors (L,A,4) fp32; logits, level-major, per level (n, h, w, pitch_cls) of logits_dtype (f16 / bf16 / f32) with
 * channel a*K + k, pitch_cls >= A*K; deltas, level-major, per level (n, h, w, pitch_box) fp32 with channel a*4 + j, pitch_box >= 4A
 * and a multiple of 4. The channels [A*K, pitch_cls) and [4A, pitch_box) are padding and are never read as candidates.
 * Candidates: per (image, level) the flat index is i = (cell*A + a)*K + k over the real channels; element i is a candidate iff
 * logit > logit_thresh (the caller passes log(t / (1 - t)) of SCORE_THRESH_TEST, evaluated in double and rounded once to fp32).
 * NaN never passes, +Inf does.
 * Selection: the min(topk, #candidates) candidates with the largest logit, equal logits lower i first; output order is logit
 * descending, then i ascending. (Ordering by the raw logit refines [d2]'s ordering by sigmoid in fp32: the two differ only where
 * distinct logits round to one probability, an order [d2]'s unstable sort leaves open.)
 * Per selected element: score 1 / (1 + expf(-logit)) in fp32; class i % K; the anchor shift + cell_anchor in fp32 as
 * osr_rpn_select forms it; Box2BoxTransform(reg_weights).apply_deltas exactly as osr_rpn_select_ex's decode_mode 1 (dw, dh clamped
 * at log(1000/16)); NOT clipped to the image ([d2] v0.6 does not clip before the NMS; osr_detector_postprocess clips later).
 * c_cand = 0 (and the row's box zeroed, bit 0 of status_flags[0] set) when a decoded coordinate or one of the four deltas is
 * non-finite; the row keeps its score, class and index.
 * Outputs, padded to cap = osr_retinanet_select_capacity() = L * topk rows per image, level l's rows at [l*topk, l*topk + count_l):
 * c_boxes (n,cap,4) fp32, c_scores (n,cap), c_cls (n,cap) int32 (-1 padding), c_cand (n,cap) int32 (0 padding), c_src (n,cap)
 * int32 (the flat index i; -1 padding), counts (n,L) int32. osr_nms_topk(cls = c_cls, cand = c_cand, seg_len = cap) consumes them.
 * Repeats are bit-identical for any input; no host sync; capturable; integer atomics only. OSR_ERR_UNSUPPORTED, nothing launched,
 * for topk > 2048, a level of >= 2^31 elements per image, or logits / deltas / c_boxes / workspace not 16-byte aligned;
 * OSR_ERR_INVALID_ARG for a pitch below the real width.
 * --------------------------------------------------------------------------------------------------------- */
int32_t osr_retinanet_select_capacity(const osr_rpn_levels* lv, int32_t topk);
int64_t osr_retinanet_select_workspace_bytes(const osr_rpn_levels* lv, int32_t n, int32_t num_classes, int32_t topk);
osr_status osr_retinanet_select(const osr_rpn_levels* lv, const float* cell_anchors, const void* logits, int32_t logits_dtype,
                                int64_t pitch_cls, const float* deltas, int64_t pitch_box, int32_t n, int32_t num_classes,
                                int32_t topk, float logit_thresh, const float reg_weights[4], float* c_boxes, float* c_scores,
                                int32_t* c_cls, int32_t* c_cand, int32_t* c_src, int32_t* counts, int32_t* status_flags,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Panoptic FPN at inference: the elementwise half of [d2] SemSegFPNHead, its output path, and
 * combine_semantic_and_instance_outputs (csrc/osr_semseg.hip, csrc/osr_panoptic.hip). detectron2 is not at hand: the semantics are
 * written from memory of detectron2 v0.6, and THIS TEXT is the contract the tests check. Tensors are NHWC in f16 / bf16 / f32, all
 * arithmetic is fp32, every launch is deterministic (integer atomics only, fixed summation orders: repeats are bit-identical),
 * nothing syncs with the host, every function is capturable.
 *
 * osr_group_norm_stats: x (n, h, w, c), c in {64, 128, 256}, 32 groups of c / 32 consecutive channels of every pixel ->
 * mean, rstd (n, 32) fp32, rstd = 1 / sqrt(biased variance + eps). Two launches: per-chunk (count, mean, M2) partials (shifted sums
 * per thread, Chan merges in thread order) into the workspace, then a merge of the chunks in chunk order. x 16-byte aligned.
 *
 * osr_gn_relu_merge: out (n, ho, wo, c) = sum over the terms, in order, of up_t(relu(gn_t(x_t))), summed in fp32 and rounded once
 * to dtype. A term's input is (n, h, w, c) of dtype; with mean / rstd (n, 32) and gamma / beta (c) fp32 it is normalised as
 * (x - mean) * rstd * gamma + beta, with all four NULL it is only rectified. up2 != 0: torch's bilinear x2 with
 * align_corners=False applied after the ReLU (src = max(0, (dst + 0.5) / 2 - 0.5), second tap clamped to the last row / column),
 * h = ho / 2, w = wo / 2; up2 == 0: h = ho, w = wo. 1 .. OSR_GN_MAX_TERMS terms; c in {64, 128, 256}.
 *
 * osr_semseg_resample: ONE image. logits (h4, w4, pitch) of dtype, channels [0, num_classes) real, [num_classes, pitch) padding
 * that is never compared or written; pitch a multiple of 4. Per output pixel and class: bilinear x4 to (4 h4, 4 w4), crop to
 * (ih, iw), bilinear resize of the crop to (oh, ow), both align_corners=False without antialiasing, composed without forming the
 * x4 map; second-stage coordinates src = max(0, ((float)ih / oh) * (dst + 0.5) - 0.5), second taps clamped to the crop's last row /
 * column. mode OSR_SEMSEG_LABELS: out (oh, ow) int32, the argmax over the real classes, the lowest class on a tie (strict
 * comparisons: NaN never wins). mode OSR_SEMSEG_VALUES: out (num_classes, oh, ow) fp32. 1 <= ih <= 4 h4, 1 <= iw <= 4 w4.
 *
 * osr_panoptic_combine: ONE image. masks (k, h, w) bytes (non-zero = set; torch bool), scores (k) fp32, classes (k) int64, count
 * (device int32, NULL = k): the first min(count, k) instances are walked by descending score (equal scores: lower index first,
 * whatever the input order), stopping at the first score < instances_confidence_thresh; an instance of area 0 is skipped; with
 * inter = its pixels already painted it is skipped when (double)inter / area > (double)overlap_thresh, else its unpainted pixels
 * get the next id (1, 2, ..). Then the labels (h, w) int32 present in the map, ascending, without label 0 (labels outside
 * 0 .. 255 are ignored): a label with at least stuff_area_limit unpainted pixels paints them with the next id. Outputs:
 * panoptic_seg (h, w) int32 (0 = none), seg_table (k + 255, 4) int32 rows {isthing, category_id, instance_id or -1, area (painted
 * pixels)}, seg_scores (k + 255) fp32 (0 for stuff), seg_count (1) int32; row r describes id r + 1. Six launches whatever k is.
 * k > 1024: OSR_ERR_UNSUPPORTED, nothing launched. h * w <= 2^30.
 * --------------------------------------------------------------------------------------------------------- */
#define OSR_GN_MAX_TERMS 4
typedef struct osr_gn_term {
    const void* x;
    const float* mean;
    const float* rstd;
    const float* gamma;
    const float* beta;
    int32_t h, w;
    int32_t up2;
    int32_t reserved;
} osr_gn_term;
#define OSR_SEMSEG_LABELS 0
#define OSR_SEMSEG_VALUES 1
int64_t osr_group_norm_stats_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
osr_status osr_group_norm_stats(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, float eps, float* mean,
                                float* rstd, void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_gn_relu_merge(const osr_gn_term* terms, int32_t num_terms, int32_t dtype, int32_t n, int32_t ho, int32_t wo, int32_t c,
                             void* out, void* stream);
osr_status osr_semseg_resample(const void* logits, int32_t dtype, int32_t h4, int32_t w4, int32_t pitch, int32_t num_classes, int32_t ih,
                               int32_t iw, int32_t oh, int32_t ow, int32_t mode, void* out, void* stream);
int64_t osr_panoptic_combine_workspace_bytes(int32_t k, int32_t h, int32_t w);
osr_status osr_panoptic_combine(const uint8_t* masks, const float* scores, const int64_t* classes, const int32_t* count, int32_t k,
                                const int32_t* labels, int32_t h, int32_t w, float overlap_thresh, int32_t stuff_area_limit,
                                float instances_confidence_thresh, int32_t* panoptic_seg, int32_t* seg_table, float* seg_scores,
                                int32_t* seg_count, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Scoring what the two models above produce: the pixel passes of [d2] SemSegEvaluator (mIoU) and of panopticapi's
 * pq_compute_single_core (PQ), csrc/osr_seg_eval.hip. Neither detectron2 nor panopticapi is at hand: the rules are written from
 * memory of detectron2 v0.6 and panopticapi, and THIS TEXT is the contract the tests check. Common to the three: integer arithmetic
 * and integer atomics only (no float atomics), repeats give identical bits, nothing syncs with the host, every function is
 * capturable, every argument is validated before anything is launched (no GPU needed for a refusal), h * w <= 2^30.
 *
 * osr_semseg_confusion: ONE image, one launch. Adds the image into conf (C + 1, C + 1) int64, indexed [pred][gt]; conf is
 * accumulated in place and never zeroed by the call. 1 <= C <= 255. mode OSR_CONF_LABELS: pred (h, w) int32 (what
 * osr_semseg_resample's label mode gives). mode OSR_CONF_VALUES: pred (C, h, w) fp32 (the models' "sem_seg"); the argmax is fused,
 * with osr_semseg_resample's rule (strict comparisons from class 0 up: the lowest class wins a tie, NaN never wins). gt (h, w)
 * uint8; a value equal to ignore_value goes to column C. A ground-truth value in [C, 255] other than ignore_value, or a predicted
 * label outside [0, C), is not counted in conf: each such pixel adds 1 to invalid[0], a device int64 also accumulated in place.
 * The grid is sized by the CUs; per workgroup an LDS histogram for C <= 126, above that per-thread runs of equal (pred, gt)
 * flushed with 64-bit integer atomics.
 *
 * osr_panoptic_pair_counts: ONE image; panopticapi's np.unique(gt * OFFSET + pred, return_counts=True). gt_rgb (h, w, 3) uint8,
 * the ground-truth PNG as decoded: segment id = R + 256 G + 65536 B. gt_ids (num_gt) int32, strictly ascending: the ids of the
 * image's segments_info. pred (h, w) int32: ids 0 .. num_pred, 0 = VOID. counts (num_gt + 2, num_pred + 1) int32, zeroed by the
 * call: row 0 is ground-truth id 0 (VOID), row 1 + i is gt_ids[i], row num_gt + 1 every other id ("unlisted"); the column is the
 * predicted id. A predicted id outside 0 .. num_pred is not counted and adds 1 to flags[0] (device int64, accumulated in place).
 * The id decode and the search in gt_ids run on the device, the search once per run of equal ids. 0 <= num_gt <= 1023,
 * 0 <= num_pred <= 2047; beyond either: OSR_ERR_UNSUPPORTED, nothing launched.
 *
 * osr_pq_accumulate: ONE image, one workgroup. Adds the image's matches into the running per-category statistics pq_counts
 * (num_categories, 3) int64 {tp, fp, fn} and pq_iou (num_categories) float64, both accumulated in place. counts: as written by
 * osr_panoptic_pair_counts. gt_meta (num_gt, 4) int32 {category slot, iscrowd, area as the JSON states it, crowd_pick};
 * crowd_pick marks the LAST crowd segment of its category in the JSON's segments_info order (panopticapi's crowd_labels_dict
 * overwrites), at most one row per slot. pred_slot (num_pred) int32: the category slot of predicted id p + 1.
 *   - the area of predicted id p is its column sum (counted from the map; VOID and unlisted rows included);
 *   - for every row g in 1 .. num_gt and column p in 1 .. num_pred with counts[g][p] > 0, ground truth not crowd and equal slots:
 *     union = area_p + area_g - inter - counts[0][p]; iou = (double)inter / (double)union; iou > 0.5 (strictly): tp += 1 and
 *     pq_iou += iou for the slot, both sides are matched. Pairs are tested independently of each other;
 *   - every unmatched ground-truth row that is not crowd adds fn for its slot;
 *   - every unmatched predicted id adds fp for its slot, unless (double)(counts[0][p] + counts[row of the slot's crowd_pick, if
 *     any][p]) / area_p > 0.5 (strictly);
 *   - row num_gt + 1 takes part in nothing but the areas.
 * The adds to pq_iou[slot] happen in ascending (g, p) order onto the running sum: the result is bit-equal to a float64 reference
 * that adds in (image, gt id, pred id) order. What the reference raises on becomes a counter: flags[1] += predicted ids with a
 * valid slot and area 0, flags[2] += predicted ids (and ground-truth rows) whose slot is outside [0, num_categories); such an id
 * or row counts as nothing else. Same limits on num_gt / num_pred as above; num_categories >= 1.
 * --------------------------------------------------------------------------------------------------------- */
#define OSR_CONF_LABELS 0
#define OSR_CONF_VALUES 1
osr_status osr_semseg_confusion(const void* pred, int32_t mode, const uint8_t* gt, int32_t h, int32_t w, int32_t num_classes,
                                int32_t ignore_value, int64_t* conf, int64_t* invalid, void* stream);
osr_status osr_panoptic_pair_counts(const uint8_t* gt_rgb, const int32_t* gt_ids, int32_t num_gt, const int32_t* pred, int32_t num_pred,
                                    int32_t h, int32_t w, int32_t* counts, int64_t* flags, void* stream);
osr_status osr_pq_accumulate(const int32_t* counts, int32_t num_gt, int32_t num_pred, const int32_t* gt_meta, const int32_t* pred_slot,
                             int32_t num_categories, int64_t* pq_counts, double* pq_iou, int64_t* flags, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * COCO box and keypoint AP: the per-image half of pycocotools' COCOeval (computeIoU / computeOks and evaluateImg),
 * csrc/osr_coco_eval.hip. pycocotools is not at hand: the rules are written from memory of pycocotools 2.0 and detectron2 v0.6, and
 * THIS TEXT is the contract; host/coco_evaluation.py's numpy COCOeval states the same rules as a literal sequential loop and the
 * tests hold the two against each other.
 *
 * osr_coco_match: ONE launch scores n images against their ground truth, for every (image, category) group, every area range and
 * every IoU threshold. No host sync, no atomics, capturable, repeats are bit-identical. Every argument is validated before anything
 * is launched (no GPU needed for a refusal); n == 0 or cap == 0 is OSR_OK without a launch.
 *
 * Detections, the engines' padded lists (need not be sorted): boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap)
 * int64 contiguous ids, counts (n) int32 (clamped to 0 .. cap); task OSR_COCO_KEYPOINTS also keypoints (n, cap, Kp, 3) fp32
 * {x, y, score} (NULL for OSR_COCO_BBOX, where num_keypoints is not read).
 * Ground truth, built by the host from the JSON, grouped by (image, category) in the JSON's annotation order: gt_seg_off
 * (n * K + 1) int32, group i * K + c owns entries gt_seg_off[i * K + c] .. gt_seg_off[i * K + c + 1]; gt_box (NG, 4) fp64 xywh;
 * gt_area (NG) fp64; gt_flags (NG) uint8, bit 0 iscrowd, bit 1 ignore; keypoints only: gt_kpts (NG, Kp, 3) fp64 {x, y, v} and
 * sigmas (Kp) fp64. max_gt_per_group: the largest group, which the host knows since it built the table (a longer group is cut there).
 * Host arrays: iou_thrs (T) fp64, passed as the doubles np.linspace(.5, .95, 10) gives and never recomputed; area_rng (A, 2) fp64
 * {lo, hi}; max_det.
 *
 * Per (image i, category c):
 *   - the detection list is the rows r < counts[i] with classes[i][r] == c, by descending score, equal scores the lower row first
 *     (mergesort's stable order; scores compare by their order-preserving bit key, -0 == +0), cut to max_det. rank (n, cap) int32
 *     is the row's position in that list, -1 for rows >= counts[i], rows whose class is outside [0, K) and rows beyond max_det;
 *   - detection geometry, as detectron2's instances_to_coco_json followed by COCO.loadRes. bbox: x = x0, y = y0, w = x1 - x0 and
 *     h = y1 - y0 in fp32, then widened to fp64, area = w * h in fp64. keypoints: x - 0.5 and y - 0.5 in fp32, then widened,
 *     area = (max x - min x) * (max y - min y) over the Kp points;
 *   - similarity, fp64. bbox, maskUtils.iou on xywh: iw = max(min(dx + dw, gx + gw) - max(dx, gx), 0), ih likewise,
 *     inter = iw * ih, union = (dw * dh + gw * gh) - inter, or dw * dh for a crowd ground truth; inter / union, 0 where the union
 *     is not positive. keypoints, computeOks: k1 = the ground truth's points with v > 0; if k1 > 0: dx = xd - xg, dy = yd - yg;
 *     otherwise with its bbox (bx, by, bw, bh): x0 = bx - bw, x1 = bx + bw * 2, y0 and y1 likewise, dx = max(0, x0 - xd) +
 *     max(0, xd - x1), dy likewise; e = (dx * dx + dy * dy) / (2 sigma)^2 / (gt_area + 2^-52) / 2; oks = the sum of exp(-e) over
 *     the points with v > 0, in ascending point order, divided by k1; over all Kp points and divided by Kp when k1 == 0;
 *   - in area range a a ground truth is ignored when its ignore bit is set or its area is outside [lo, hi];
 *   - per threshold t the detections are matched in list order. thr = min(t, 1 - 1e-10). A ground truth is available when no
 *     earlier detection of this (t, a) took it, or it is crowd. Among the available, not ignored ground truths with similarity >=
 *     thr the detection takes the largest similarity, equal similarities going to the HIGHEST position in the group (pycocotools'
 *     loop replaces on `not <`); if there is none, the same rule among the available ignored ones; else it stays unmatched. This
 *     equals pycocotools' loop over the ground truths sorted ignored-last (stably) with its break;
 *   - a matched detection is ignored iff its ground truth is ignored at a; an unmatched one iff its own area is outside [lo, hi].
 *
 * Outputs (all written in full by the call): flags (n, cap, A) uint32, bit t = matched at threshold t, bit 16 + t = ignored at
 * threshold t, 0 where rank is -1; rank; match (n, cap, A, T) int32 or NULL: the matched ground truth's index into gt_*, else -1.
 * The similarity matrix goes to `sim` when given, else to `workspace` (sim NULL): either holds
 * osr_coco_match_workspace_bytes(cap, max_det, NG) = min(cap, max_det) * NG * 8 bytes. Layout: group (i, c) with G ground truths
 * starting at g0 = gt_seg_off[i * K + c] and M listed detections owns the doubles from g0 * min(cap, max_det); entry
 * [rank d][position j] is at d * G + j. Entries outside the groups' M x G blocks are not written.
 *
 * Limits, OSR_ERR_UNSUPPORTED with nothing launched beyond them: cap <= 1024, max_det <= 128, T <= 16, A <= 8, Kp <= 32,
 * max_gt_per_group <= 4096. K >= 1, n * K < 2^31. A NaN score orders by its bit pattern; NaN similarities match nothing.
 * --------------------------------------------------------------------------------------------------------- */
#define OSR_COCO_BBOX 0
#define OSR_COCO_KEYPOINTS 1
int64_t osr_coco_match_workspace_bytes(int32_t cap, int32_t max_det, int32_t num_gt);
osr_status osr_coco_match(int32_t task, const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts,
                          const float* keypoints, int32_t n, int32_t cap, int32_t num_categories, int32_t num_keypoints,
                          const int32_t* gt_seg_off, const double* gt_box, const double* gt_area, const uint8_t* gt_flags,
                          const double* gt_kpts, const double* sigmas, int32_t num_gt, int32_t max_gt_per_group, const double* iou_thrs,
                          int32_t num_thrs, const double* area_rng, int32_t num_areas, int32_t max_det, uint32_t* flags, int32_t* rank,
                          int32_t* match, double* sim, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Open-set COCO matching (known and unknown AP / AR, wilderness impact, A-OSE): the per-image half of OpensetCOCOEval.evaluate,
 * csrc/osr_os_coco_eval.hip. The rules below restate host/os_coco_evaluation.py (itself a restatement of the reference's
 * os_cocoeval.py:242-555), and THIS TEXT is the contract; the numpy class states the same rules as literal sequential loops and the
 * tests hold the two against each other bit for bit.
 *
 * osr_os_coco_match: ONE launch scores n images for every class slot, every area range and every IoU threshold; each slot's
 * detection list is matched against up to THREE ground-truth sets of its image. No host sync, no atomics, capturable, repeats are
 * bit-identical. Every argument is validated before anything is launched (no GPU needed for a refusal); n == 0 or cap == 0 is
 * OSR_OK without a launch.
 *
 * Detections, the engines' padded lists (need not be sorted): boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap)
 * int64, counts (n) int32 (clamped to 0 .. cap).
 * Class slots: class_slot (L) int32, built by the host, maps a class VALUE v to a slot: 0 .. K - 1 the known categories in ascending
 * dataset id, K the unknown class (prediction value 1000, with or without a contiguous-id map), -1 dropped. A value outside [0, L)
 * and an entry outside -1 .. K are dropped as well.
 * Ground truth, built by the host from the JSON for the batch's images, one table with per-image offsets: gt_img_off (n + 1) int32,
 * image i owns entries gt_img_off[i] .. gt_img_off[i + 1]; WITHIN an image the entries are sorted by (slot ascending, then annotation
 * order). gt_box (NG, 4) fp64 xywh; gt_area (NG) fp64 (the JSON's area, else w * h); gt_slot (NG) int32: the known slot or K (any
 * other value belongs to no set); gt_pos (NG) int32: the entry's position in the JSON's annotation order within its image (distinct
 * within an image); gt_crowd (NG) uint8, bit 0 iscrowd (ignore = iscrowd). max_gt_per_image: the largest image, which the host knows
 * since it built the table (a longer one is cut there).
 * Host arrays: iou_thrs (T) fp64, passed as the doubles np.linspace(.5, .95, 10) gives and never recomputed; area_rng (A, 2) fp64
 * {lo, hi}; max_det.
 *
 * Per (image i, slot c):
 *   - the detection list is the rows r < counts[i] whose class maps to c, by descending score, equal scores the lower row first
 *     (mergesort's stable order; scores compare by their order-preserving bit key, -0 == +0), cut to max_det. rank (n, cap) int32
 *     is the row's position in that list, -1 for rows >= counts[i], dropped classes and rows beyond max_det;
 *   - detection geometry, as instances_to_coco_json followed by loadRes: the four fp32 corners are widened to fp64 FIRST, then
 *     w = x1 - x0, h = y1 - y0 and area = w * h in fp64. (osr_coco_match subtracts in fp32 and widens afterwards: the two differ
 *     in the last bits for corners off a coarse grid, each as its own evaluator's records do);
 *   - similarity, fp64 maskUtils.iou on xywh exactly as box_iou_xywh: iw = max(min(dx + dw, gx + gw) - max(dx, gx), 0), ih likewise,
 *     inter = iw * ih, union = (dw * dh + gw * gh) - inter, or dw * dh for a crowd ground truth; inter / union, 0 where the union
 *     is not positive;
 *   - the sets. A known slot c < K: S0 the ground truths of slot c in annotation order; S1 those of the OTHER known slots in
 *     annotation order across the slots (position = gt_pos); S2 the unknown ones in annotation order. The unknown slot K: S0 the
 *     unknown ground truths in annotation order; S1 ALL known ones ordered by (slot ascending, then annotation order), i.e. in table
 *     order, which is NOT a known slot's S1 order; no S2. With the table sorted as above, a set's order is the table's except for a
 *     known slot's S1;
 *   - the matching rule per set is pycocotools' as osr_coco_match states it. In area range a a ground truth is ignored when it is
 *     crowd or its area is outside [lo, hi]. Per threshold t the detections are matched in list order, thr = min(t, 1 - 1e-10). A
 *     ground truth is available unless an earlier detection of this (set, t, a) took it, or it is crowd. Among the available, not
 *     ignored ground truths of the set with similarity >= thr the detection takes the largest similarity, equal similarities going
 *     to the HIGHEST position in the set's order; if there is none, the same rule among the available ignored ones; else it stays
 *     unmatched;
 *   - a matched detection is ignored iff its ground truth is ignored at a; an unmatched one iff its own area is outside [lo, hi],
 *     decided separately for each set.
 *
 * Outputs (all written in full by the call): rank; flags (n, cap, A, 3) uint32, word s belongs to set s: bit t = matched at
 * threshold t, bit 16 + t = ignored at threshold t; a word is 0 where rank is -1, and word 2 is 0 for the unknown slot; match
 * (n, cap, A, 3, T) int32 or NULL: the matched ground truth's index into gt_*, else -1.
 * workspace: osr_os_coco_match_workspace_bytes(cap, NG) = cap * NG * 8 bytes for the similarities (image i's rows x ground truths
 * from gt_img_off[i] * cap doubles on); OSR_ERR_WORKSPACE when it is smaller.
 *
 * Limits, OSR_ERR_UNSUPPORTED with nothing launched beyond them: cap <= 1024, max_det <= 128, T <= 16, A <= 8, max_gt_per_image <=
 * 4096, n * (K + 1) < 2^31 - 1. L >= 1, K >= 0. A NaN score orders by its bit pattern; NaN similarities match nothing.
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_os_coco_match_workspace_bytes(int32_t cap, int32_t num_gt);
osr_status osr_os_coco_match(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts, int32_t n, int32_t cap,
                             const int32_t* class_slot, int32_t num_class_values, int32_t num_known, const int32_t* gt_img_off,
                             const double* gt_box, const double* gt_area, const int32_t* gt_slot, const int32_t* gt_pos,
                             const uint8_t* gt_crowd, int32_t num_gt, int32_t max_gt_per_image, const double* iou_thrs, int32_t num_thrs,
                             const double* area_rng, int32_t num_areas, int32_t max_det, uint32_t* flags, int32_t* rank, int32_t* match,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * LVIS federated box AP: lvis-api's LVISResults cut, LVISEval._prepare's category filter and LVISEval.evaluate_img,
 * csrc/osr_lvis_eval.hip. Neither lvis-api nor detectron2 is at hand: the rules are written from memory of lvis-api 0.5.x and
 * detectron2 v0.6's LVISEvaluator, and THIS TEXT is the contract; host/lvis_evaluation.py's numpy LVISEval states the same rules as
 * a literal sequential loop and the tests hold the two against each other bit for bit.
 *
 * osr_lvis_match: TWO launches (after the memsets that preset the outputs) score n images against their sparse ground truth: a
 * first kernel cuts and groups each image's detections, a second matches every group for every area range and IoU threshold. The
 * grid does not grow with the number of categories. No host sync, no atomics, capturable, repeats are bit-identical. Every argument
 * is validated before anything is launched (no GPU needed for a refusal); n == 0 or cap == 0 is OSR_OK without a launch.
 *
 * Detections, the engines' padded lists (need not be sorted): boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap)
 * int64 contiguous ids, counts (n) int32 (clamped to 0 .. cap).
 * Ground truth, built by the host from the JSON, sparse: an ENTRY is one evaluated (image, category): the image has a ground truth
 * of the category (positive) or lists it in neg_category_ids. img_off (n + 1) int32: image i owns entries img_off[i] .. img_off[i + 1];
 * ev_cat (NE) int32: the entry's contiguous category, STRICTLY ASCENDING within an image (the kernel looks a class up by binary
 * search); ev_gt_off (NE + 1) int32: entry e owns ground truths ev_gt_off[e] .. ev_gt_off[e + 1], so the ground truths are stored in
 * entry order, within an entry in the JSON's annotation order, and a negative entry owns none; ev_flags (NE) uint8: bit 0 = the
 * category is in the image's not_exhaustive_category_ids. gt_box (NG, 4) fp64 xywh; gt_area (NG) fp64, the JSON's area; gt_flags
 * (NG) uint8, bit 1 = the annotation's `ignore` field (bit 0, osr_coco_match's crowd bit, is not read: LVIS has no crowds).
 * max_gt_per_group: the largest entry, which the host knows since it built the table (a longer one is cut there). Every offset is
 * clamped to its table. Host arrays: iou_thrs (T) fp64, passed as the doubles np.linspace(.5, .95, 10) gives and never recomputed;
 * area_rng (A, 2) fp64 {lo, hi}; max_dets (lvis-api's 300).
 *
 * Per image i:
 *   - the cut (LVISResults): ALL rows r < counts[i], whatever their class, are ordered by descending score, equal scores the lower
 *     row first (Python's stable sorted(reverse=True); scores compare by their order-preserving bit key, -0 == +0), and the first
 *     max_dets are kept. The cut comes BEFORE the category filter;
 *   - the category filter (_prepare): a kept row of class c is LISTED iff 0 <= c < K and the image has an entry of c. A row that is
 *     not listed is neither a false positive nor ignored: it does not exist for the evaluation;
 *   - a group is the listed rows of one entry in the order of the cut. There is no further cut per group. rank (n, cap) int32 is
 *     the row's position in its group's list, -1 for rows >= counts[i], rows beyond the cut, classes outside [0, K) and categories
 *     without an entry;
 *   - detection geometry and similarity are osr_coco_match's for bbox with no crowd: x = x0, y = y0, w = x1 - x0 and h = y1 - y0 in
 *     fp32, then widened to fp64, area = w * h in fp64; iw = max(min(dx + dw, gx + gw) - max(dx, gx), 0), ih likewise, inter = iw * ih,
 *     union = (dw * dh + gw * gh) - inter, inter / union, 0 where the union is not positive;
 *   - in area range a a ground truth is ignored when its ignore bit is set or its area is outside [lo, hi];
 *   - per threshold t the detections of a group are matched in list order by the rule osr_coco_match states: thr = min(t, 1 - 1e-10);
 *     a ground truth is available when no earlier detection of this (t, a) took it (there is no crowd re-use); among the available,
 *     not ignored ones with similarity >= thr the largest similarity wins, equal similarities going to the HIGHEST position in the
 *     group; if there is none, the same rule among the available ignored ones; else the detection stays unmatched. This equals
 *     lvis-api's loop over the ground truths sorted ignored-last (stably) with its break;
 *   - a matched detection is ignored iff its ground truth is ignored at a; an unmatched one iff its own area is outside [lo, hi] OR
 *     its entry's not-exhaustive bit is set.
 *
 * Outputs (all written in full by the call): rank; flags (n, cap, A) uint32 in osr_coco_match's layout, bit t = matched at
 * threshold t, bit 16 + t = ignored at threshold t, 0 where rank is -1; match (n, cap, A, T) int32 or NULL: the matched ground
 * truth's index into gt_*, else -1. The similarity blocks go to `sim` when given, else to the head of `workspace`: min(cap,
 * max_dets) * NG doubles, entry e with G ground truths from g0 = ev_gt_off[e] and M listed detections owns the doubles from
 * g0 * min(cap, max_dets), [position in the group d][ground truth j] at d * G + j; what lies outside the blocks is not written.
 * workspace is ALWAYS needed (the group tables the first kernel hands to the second stand behind the similarities):
 * osr_lvis_match_workspace_bytes(n, cap, max_dets, NG) bytes, 8-byte aligned, OSR_ERR_WORKSPACE when it is smaller.
 *
 * Limits, OSR_ERR_UNSUPPORTED with nothing launched beyond them: cap <= 1024, max_dets <= 512, T <= 16, A <= 8, max_gt_per_group
 * <= 4096. K >= 1 has no upper limit (nothing is sized by it). A NaN score orders by its bit pattern; NaN similarities match nothing.
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_lvis_match_workspace_bytes(int32_t n, int32_t cap, int32_t max_dets, int32_t num_gt);
osr_status osr_lvis_match(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts, int32_t n, int32_t cap,
                          int32_t num_categories, const int32_t* img_off, const int32_t* ev_cat, const int32_t* ev_gt_off,
                          const uint8_t* ev_flags, int32_t num_entries, const double* gt_box, const double* gt_area, const uint8_t* gt_flags,
                          int32_t num_gt, int32_t max_gt_per_group, const double* iou_thrs, int32_t num_thrs, const double* area_rng,
                          int32_t num_areas, int32_t max_dets, uint32_t* flags, int32_t* rank, int32_t* match, double* sim, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Open-set PASCAL-VOC matching (AP@K, AP@U, wilderness impact, A-OSE): the per-detection half of voc_eval for every class,
 * csrc/osr_voc_eval.hip. The rules below restate host/evaluation.py (PascalVOCDetectionEvaluator.process and voc_eval, themselves a
 * restatement of the reference's pascal_voc_evaluation.py:53-70 and :264-379), and THIS TEXT is the contract; voc_match_reference
 * states the same rules as a literal numpy loop and the tests hold the two against each other bit for bit.
 *
 * osr_voc_match: ONE launch scores the n images of a batch against their ground truth for every class. No host sync, no atomics
 * across workgroups, capturable, repeats are bit-identical. Every argument is validated before anything is launched (no GPU needed
 * for a refusal); n == 0 or cap == 0 is OSR_OK without a launch (and nothing is written).
 *
 * Detections, the engines' padded lists (need not be sorted): boxes (n, cap, 4) fp32 xyxy, scores (n, cap) fp32, classes (n, cap)
 * int64, counts (n) int32 (clamped to 0 .. cap), image_index (n) int32: the row's image in the ground-truth table.
 * Ground truth, built ONCE by the host for the whole dataset: gt_img_off (num_images + 1) int32, image m owns entries
 * gt_img_off[m] .. gt_img_off[m + 1] in annotation order; gt_box (NG, 4) fp64, the XML's integers (finite); gt_cls (NG) int32, an
 * index into the evaluator's class names: a known index, or C - 1 for "unknown" exactly as parse_voc_xml renames (any other value
 * belongs to no class); gt_difficult (NG) uint8, non-zero = difficult. max_gt_per_image: the largest image, which the host knows
 * since it built the table (a longer one is cut there). ovthresh: a double, used as given. C = the number of class names.
 *
 * Per detection row r of batch row i:
 *   - the row is VALID when r < counts[i], 0 <= class < C and 0 <= image_index[i] < num_images;
 *   - record geometry, what the evaluator's text record holds: x0' = fp32(x0 + 1.0f) and y0' likewise IN FP32 (the evaluator adds a
 *     Python int to an np.float32); each of x0', y0', x1, y1 then becomes t = rint((double)v * 10.0) and the record's value t / 10.0;
 *     the score becomes k = rint((double)s * 1000.0) and conf = k / 1000.0. This IS the "{:.1f}" / "{:.3f}" text round trip: the
 *     products are exact in fp64 for any fp32 input, rint is half-even like the formatting, and the division is correctly rounded
 *     like float("...");
 *   - a valid row is NON-FINITE when its score or a coordinate is not finite, |s * 1000| >= 2^31 or a |v * 10| >= 2^63 (k and t have
 *     to fit milli and deci). It gets the valid and the non-finite bit and nothing else (milli 0, deci 0, match -1), belongs to no
 *     list, and status becomes 1; the host then abandons the device result;
 *   - the list of (image, class c) is its valid finite rows by descending k, equal k going to the lower row first (the stable
 *     order; the ROUNDED score orders, not the raw one);
 *   - overlap, fp64 with the inclusive + 1 convention exactly as _overlaps: iw = max(min(gx1, bx1) - max(gx0, bx0) + 1, 0), ih
 *     likewise, inter = iw * ih, union = (bx1 - bx0 + 1) * (by1 - by0 + 1) + (gx1 - gx0 + 1) * (gy1 - gy0 + 1) - inter, ov = inter /
 *     union, with b the record's values. A union of zero gives a NaN or an infinite ov, which count as numpy counts them: NaN is the
 *     maximum of np.argmax and np.max and is not > ovthresh;
 *   - matching: the detections of a list meet, in list order, the image's ground truths with gt_cls == c in annotation order; jmax
 *     is the FIRST maximum of ov. If ov[jmax] > ovthresh (strictly): a difficult ground truth gives neither tp nor fp; a ground
 *     truth no earlier detection of the list has taken gives tp and is taken; a taken one gives fp. Otherwise, and with no ground
 *     truth of the class, fp;
 *   - unknown overlap, for every class except C - 1: is_unk is set when the maximum of ov over the image's ground truths with
 *     gt_cls == C - 1 is > ovthresh, independent of the matching; difficult ones count.
 *
 * Outputs (all written in full by the call): flags (n, cap) uint8: bit 0 valid, bit 1 tp, bit 2 fp, bit 3 is_unk, bit 4 non-finite;
 * 0 for rows that are not valid. milli (n, cap) int32: k, 0 for rows in no list. match (n, cap) int32 or NULL: jmax as an index into
 * gt_* where ov[jmax] > ovthresh (tp, fp on a taken one, or difficult), else -1. deci (n, cap, 4) int64 or NULL: the four t, 0 for
 * rows in no list. status (1) int32: 1 when a non-finite row was met, else 0.
 *
 * Limits, OSR_ERR_UNSUPPORTED with nothing launched beyond them: cap <= 1024, max_gt_per_image <= 4096, C >= 1, n * C < 2^31.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_voc_match(const float* boxes, const float* scores, const int64_t* classes, const int32_t* counts, const int32_t* image_index,
                         int32_t n, int32_t cap, int32_t num_classes, const int32_t* gt_img_off, int32_t num_images, const double* gt_box,
                         const int32_t* gt_cls, const uint8_t* gt_difficult, int32_t num_gt, int32_t max_gt_per_image, double ovthresh,
                         uint8_t* flags, int32_t* milli, int32_t* match, int64_t* deci, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Class-agnostic box-proposal recall (AR@limit per area range), csrc/osr_proposal_recall.hip: what the reference's evaluator
 * computes per image before it sums, for a batch of images, every area range and every proposal limit in ONE launch.
 * host/proposal_evaluation.py's evaluate_box_proposals states the same rules as a torch-CPU loop and the tests hold the two against
 * each other bit for bit. No host sync, no floating-point atomics, capturable, repeats are bit-identical. Every argument is validated
 * before anything is launched (no GPU needed for a refusal); n == 0 is OSR_OK without a launch.
 *
 * Device inputs, all finite: boxes (n, cap, 4) fp32 xyxy, logits (n, cap) fp32, counts (n) int32 (clamped to 0 .. cap; rows past
 * counts[i] hold anything and do not count). The batch's NON-CROWD ground truth in annotation order: gt_boxes (num_gt, 4) fp32 xyxy,
 * gt_area (num_gt) fp32 (the annotation's area), seg_off (n + 1) int32: image i owns entries seg_off[i] .. seg_off[i + 1].
 * max_gt_per_image: the largest segment, which the host knows since it built the table (a longer one is cut there).
 * Host arrays: area_ranges (A, 2) fp32 {lo, hi}, limits (L) int32 >= 1, thresholds (T) fp32, used bit for bit as given.
 *
 *   - An image with counts[i] == 0, or with no non-crowd ground truth, adds nothing. That includes num_pos, since the reference skips
 *     the image before it counts. All its gt_overlap entries are -1.
 *   - Otherwise rank the proposals by logit, descending. Equal logits keep row order, so the sort is stable (-0 == +0).
 *   - For area range a, the valid ground truths are those with lo <= area <= hi in fp32, both ends inclusive. An area of exactly 1024
 *     is therefore both small and medium. num_pos[i, a] is their number. An invalid ground truth has gt_overlap -1.
 *   - For limit l, the live proposals are the first min(counts[i], limit) ranks. The area filter comes before the limit.
 *   - Then run min(live proposals, valid ground truths) rounds. Among live pairs take the largest osr_pairwise_iou (csrc/osr_boxes.h,
 *     fp32, no FMA contraction). Ties go to the lowest ground-truth index in annotation order, then to the lowest rank. Record that IoU
 *     at the chosen ground truth, then retire that ground truth and that proposal. A zero IoU is a legitimate choice. Ground truths
 *     never chosen keep 0.
 *   - hits[i, a, l, t] is the number of valid ground truths with gt_overlap >= thresholds[t], compared in fp32.
 *
 * Outputs: hits (n, A, L, T) int32 and num_pos (n, A) int32, written in full; gt_overlap (A, L, num_gt) fp32 or NULL, written at the
 * entries the segments cover.
 * Limits, OSR_ERR_UNSUPPORTED with nothing launched beyond them: cap <= 2048, max_gt_per_image <= 1024. A in 1 .. 8, L in 1 .. 8,
 * T in 1 .. 16, limits >= 1, or OSR_ERR_INVALID_ARG.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_proposal_recall(const float* boxes, const float* logits, const int32_t* counts, int32_t n, int32_t cap, const float* gt_boxes,
                               const float* gt_area, const int32_t* seg_off, int32_t num_gt, int32_t max_gt_per_image,
                               const float* area_ranges, int32_t num_areas, const int32_t* limits, int32_t num_limits,
                               const float* thresholds, int32_t num_thrs, int32_t* hits, int32_t* num_pos, float* gt_overlap, void* stream);

/* =========================================================================================================
 * Training step, forward half: targets and losses. Gradients are not
 * produced by this library yet; every function below is a forward kernel whose outputs equal the reference's
 * forward values. Random subsampling takes caller-supplied uniform keys: the k smallest keys of a class are
 * kept (ties: lower index) -- the role torch.randperm plays in [d2] subsample_labels -- so that runs are
 * reproducible and the selected lists are comparable bit for bit.
 * ========================================================================================================= */

/* ---------------------------------------------------------------------------------------------------------
 * Anchor <-> GT matching: ClsFreeRPN.label_and_sample_anchors up to the subsampling
 * (classification_free_rpn.py:359-371): pairwise IoU (GT x anchors), argmax over GT (first maximum),
 * Matcher(reg thresholds, labels [0,-1,1], allow_low_quality_matches) and the same for the objectness
 * thresholds. Anchors are generated in-kernel from the level table (image-major list of R = sum h*w*a).
 * gt_boxes: (n, gmax, 4) padded, gt_count (n). Images without GT get label 0 everywhere and matched_idx 0.
 * Outputs: matched_idx (n,R) int32, matched_iou (n,R), labels_reg / labels_obj (n,R) int8 in {-1,0,1}.
 * workspace: n*gmax*4 bytes.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_rpn_match_anchors(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n,
                                 const float* gt_boxes, const int32_t* gt_count, int32_t gmax, float reg_lo,
                                 float reg_hi, float obj_lo, float obj_hi, int32_t* matched_idx, float* matched_iou,
                                 int8_t* labels_reg, int8_t* labels_obj, void* workspace, int64_t workspace_bytes,
                                 void* stream);

/* [d2] subsample_labels + ClsFreeRPN._subsample_labels (classification_free_rpn.py:299-316), in place: keep
 * min(int(num_samples*positive_fraction), #pos) positives and min(num_samples - kept_pos, #neg) negatives with
 * the smallest keys, everything else becomes -1. labels, keys: (n, r). num_samples <= 512. */
osr_status osr_subsample_labels(int8_t* labels, const float* keys, int32_t n, int64_t r, int32_t num_samples,
                                float positive_fraction, int32_t* num_pos_out, int32_t* num_neg_out, void* stream);

/* Matched GT box per anchor and the centerness target (classification_free_rpn.py:386-402): ltrb deltas of the
 * anchor against its matched GT, zero unless the anchor centre lies inside, sqrt(min(l,r)/max(l,r) *
 * min(t,b)/max(t,b)), zero where the (subsampled) objectness label is 0. matched_boxes (n,R,4), ctr_target (n,R). */
osr_status osr_rpn_anchor_targets(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n,
                                  const float* gt_boxes, const int32_t* gt_count, int32_t gmax,
                                  const int32_t* matched_idx, const int8_t* labels_obj, float* matched_boxes,
                                  float* ctr_target, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * ClsFreeRPN.losses, BBOX_REG_LOSS_TYPE "iou" (classification_free_rpn.py:446-490, box_regression_w_iou.py:49-61).
 * pred_deltas / pred_ctr: the level-major buffers osr_cfrpn_head_tail writes (levels->offset). Targets are
 * image-major (n, R). out6 = {loss_rpn_loc, loss_rpn_ctr, num_pos, num_neg, obj_num_pos, obj_num_neg}; both
 * losses are divided by batch_size_per_image * n and multiplied by their weight. workspace: 6 KiB.
 * --------------------------------------------------------------------------------------------------------- */
osr_status osr_rpn_losses_fwd(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n,
                              const float* pred_deltas, const float* pred_ctr, const int8_t* labels_reg,
                              const int8_t* labels_obj, const float* matched_boxes, const float* ctr_target,
                              float loc_weight, float ctr_weight, int32_t batch_size_per_image, float* out6,
                              void* workspace, int64_t workspace_bytes, void* stream);
/* The loss functions the reference selects by name (box_regression_w_iou.py:13-85: BBOX_REG_LOSS_TYPE "smooth_l1" | "iou" |
 * "giou" | "diou" | "ciou" with SMOOTH_L1_BETA; classification_free_rpn.py:475-481 and osrcnn_fast_rcnn.py:368: smooth L1 with
 * its own beta for the centerness / IoU regression). NULL options = what both Openset yaml files select: "iou" for the CF-RPN
 * boxes, "smooth_l1" for the RoI boxes, every beta 0 (= L1). */
enum { OSR_BOX_LOSS_IOU = 0, OSR_BOX_LOSS_SMOOTH_L1 = 1, OSR_BOX_LOSS_GIOU = 2, OSR_BOX_LOSS_DIOU = 3, OSR_BOX_LOSS_CIOU = 4 };
typedef struct osr_loss_options {
    int32_t box_loss_type;     /* OSR_BOX_LOSS_* */
    float box_smooth_l1_beta;  /* used by OSR_BOX_LOSS_SMOOTH_L1 */
    float aux_smooth_l1_beta;  /* centerness loss (CF-RPN) / IoU regression loss (RoI head) */
} osr_loss_options;
osr_status osr_rpn_losses_fwd_ex(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n,
                                 const float* pred_deltas, const float* pred_ctr, const int8_t* labels_reg,
                                 const int8_t* labels_obj, const float* matched_boxes, const float* ctr_target,
                                 float loc_weight, float ctr_weight, int32_t batch_size_per_image,
                                 const osr_loss_options* options, float* out6, void* workspace, int64_t workspace_bytes,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * OpensetROIHeads.label_and_sample_proposals (osrcnn_roi_heads.py:177-216): append the GT boxes to the
 * proposals ([d2] add_ground_truth_to_proposals, logit log((1-1e-10)/1e-10)), IoU against GT,
 * Matcher([iou_thr],[0,1]), class = GT class or num_classes (background), matched IoU, then keep batch_size
 * candidates, at most int(batch_size*positive_fraction) foreground. Candidates of image i are
 * [proposals 0..prop_count[i]), GT 0..gt_count[i])]; keys is (n, pcap+gmax): the key of proposal j is keys[i][j],
 * the key of GT g is keys[i][pcap+g], whatever the counts are.
 * Output rows per image: foreground by ascending key, then background by ascending key, padded to batch_size
 * (class -1, src -1, batch index -1; the loss kernels below skip rows with class < 0 and leave them out of their
 * normalisers, RoIAlign skips rows with batch index -1). out_src: candidate index of each row; out_batch_idx: image
 * of each row; out_counts: (n,3) = {rows, foreground, background}. batch_size <= 512.
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_roi_match_sample_workspace_bytes(int32_t n, int64_t pcap, int32_t gmax);
osr_status osr_roi_match_and_sample(const float* prop_boxes, const float* prop_logits, const int32_t* prop_count,
                                    int64_t pcap, const float* gt_boxes, const int64_t* gt_classes,
                                    const int32_t* gt_count, int32_t gmax, int32_t n, const float* keys,
                                    int32_t num_classes, int32_t batch_size, float positive_fraction, float iou_thr,
                                    float* out_boxes, float* out_logits, int64_t* out_classes, float* out_ious,
                                    float* out_gt_boxes, int32_t* out_src, int32_t* out_batch_idx, int32_t* out_counts,
                                    void* workspace, int64_t workspace_bytes, void* stream);
/* The same with one more output, out_gt_idx (n, batch_size) int32 (may be NULL: the call above): the index of the matched ground-truth
 * box inside its image's list (the lowest index among equal IoUs) on foreground rows, -1 on background and padding rows -- what the
 * mask target of a row is cut from (osr_mask_targets). Every other output is bit-identical to the call above. */
osr_status osr_roi_match_and_sample_ex(const float* prop_boxes, const float* prop_logits, const int32_t* prop_count,
                                       int64_t pcap, const float* gt_boxes, const int64_t* gt_classes,
                                       const int32_t* gt_count, int32_t gmax, int32_t n, const float* keys,
                                       int32_t num_classes, int32_t batch_size, float positive_fraction, float iou_thr,
                                       float* out_boxes, float* out_logits, int64_t* out_classes, float* out_ious,
                                       float* out_gt_boxes, int32_t* out_src, int32_t* out_batch_idx, int32_t* out_counts,
                                       int32_t* out_gt_idx, void* workspace, int64_t workspace_bytes, void* stream);

/* OpensetFastRCNNOutputLayers.losses (osrcnn_fast_rcnn.py:266-370): L1 between the predicted deltas and
 * Box2BoxTransform(reg_weights).get_deltas(proposal, gt), and L1 between the predicted and the matched IoU, over
 * rows with 0 <= class < num_classes; both divided by the number of rows with class >= 0 (the reference's
 * gt_classes.numel(): its row list has no padding). Predictions are read in place from the predictor GEMM output:
 * row i's deltas at pred_deltas[i*delta_stride .. +4), its IoU at pred_iou[i*iou_stride]; iou_is_logit applies the
 * sigmoid of OpensetFastRCNNOutputLayers.forward (:262) in the kernel.
 * out3 = {loss_box_reg, loss_iou, rows counted}. workspace 3 KiB. */
osr_status osr_roi_box_losses_fwd(const float* pred_deltas, int32_t delta_stride, const float* pred_iou,
                                  int32_t iou_stride, int32_t iou_is_logit, const float* proposal_boxes,
                                  const float* gt_boxes, const int64_t* gt_classes, const float* gt_iou, int64_t m,
                                  int32_t num_classes, const float reg_weights[4], float box_weight, float iou_weight,
                                  float* out3, void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_roi_box_losses_fwd_ex(const float* pred_deltas, int32_t delta_stride, const float* pred_iou,
                                     int32_t iou_stride, int32_t iou_is_logit, const float* proposal_boxes,
                                     const float* gt_boxes, const int64_t* gt_classes, const float* gt_iou, int64_t m,
                                     int32_t num_classes, const float reg_weights[4], float box_weight, float iou_weight,
                                     const osr_loss_options* options, float* out3, void* workspace,
                                     int64_t workspace_bytes, void* stream);

/* PLN.loss, COS distance, one prototype per class (prototype_learning_network.py:133-187): rows with a known
 * class and IoU > iou_thr contribute relu(d_own - alpha) + relu(beta - min d_other); the prototypes contribute
 * sum_k relu(alpha + beta - min_{j!=k} d(p_k,p_j)); total * loss_weight / (rows with class >= 0). emb: (m,d)
 * un-normalised encoder output; protos_normed (num_known, d). workspace 4 KiB. */
osr_status osr_pln_loss_fwd(const float* emb, int64_t m, int32_t d, const float* protos_normed, int32_t num_known,
                            const int64_t* gt_classes, const float* ious, float iou_thr, float alpha, float beta,
                            float loss_weight, float* out1, void* workspace, int64_t workspace_bytes, void* stream);
/* The same with REPS_PER_CLASS prototypes per class (protos_normed: (num_known * reps, d), class-major; a class's distance is
 * the minimum over its prototypes, the prototype term runs over all of them with the own-class block excluded,
 * prototype_learning_network.py:163-180) and any DISTANCE_TYPE. */
osr_status osr_pln_loss_fwd_ex(const float* emb, int64_t m, int32_t d, const float* protos_normed, int32_t num_known,
                               int32_t reps, int32_t distance_type, const int64_t* gt_classes, const float* ious,
                               float iou_thr, float alpha, float beta, float loss_weight, float* out1, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* SoftMaxClassifier.loss (softmax_classifier.py:266-285): id_map (known c -> c, num_classes -> num_known, any
 * other class is ignored), mean cross entropy over num_known+1 logits, times loss_weight. workspace 2 KiB. */
osr_status osr_softmax_ce_loss_fwd(const float* logits, int64_t m, int32_t num_known, const int64_t* gt_classes,
                                   int32_t num_classes, float loss_weight, float* out1, void* workspace,
                                   int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of osr_conv2d_fwd (training step, backward half). `p` describes the FORWARD layer.
 *  - data gradient: dx = osr_conv2d_fwd(dy, flipped/transposed weights) with stride 1, pad' = k-1-pad
 *    (host/weights.py pack_dgrad_weight); a stride-2 1x1 layer writes every second pixel of a zeroed dx through the output
 *    strides; res_mode 3 applies the ReLU mask of the layer below, res_mode 1 adds a second gradient. A stride-2 3x3 layer
 *    (pad 1) has an entry of its own, osr_conv2d_dgrad_s2.
 *  - weight gradient: dw[cout][kh][kw][cin] (fp32, the packed forward layout) = sum over output pixels of
 *    dy[n,oh,ow,co] * x[n, oh*sh-ph+kh, ow*sw-pw+kw, ci]; x, dy fp16/bf16 (dy dense (n,ho,wo,cout)), fp32 accumulate,
 *    split over the pixel axis with partials in the workspace and a fixed-order reduction (bitwise reproducible).
 *    accumulate != 0 adds to dw.
 *  - bias gradient: db[co] = sum_m dy[m][co]; workspace 512*cout*4 bytes.
 * --------------------------------------------------------------------------------------------------------- */
int64_t osr_conv2d_wgrad_workspace_bytes(const osr_conv_params* p);
osr_status osr_conv2d_wgrad(const osr_conv_params* p, const void* x, const void* dy, float* dw, int32_t accumulate,
                            void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_bias_grad(const void* dy, int32_t dtype, int64_t m, int32_t cout, float* db, int32_t accumulate,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* Data gradient of a 3x3 convolution with stride 2 and pad 1 (the first block of res3-res5 with MODEL.RESNETS.STRIDE_IN_1X1
 * False: torchvision's layout), `p` describing the FORWARD layer (n, hi, wi, cin of x; ho, wo, cout of dy; kh = kw = 3,
 * stride 2, pad 1; in_stride_* / out_stride_* the dense strides of dx / dy):
 *     dx[n,ih,iw,ci] = sum dy[n,oh,ow,co] * w[co,kh,kw,ci] over 2*oh-1+kh = ih, 2*ow-1+kw = iw,
 * computed per pixel-parity phase (1, 1x2, 2x1 and 2x2 taps) in one launch. w_dgrad = pack_dgrad_weight(w), (cin,3,3,cout).
 * add (nullable, dx's shape, in_dtype) is summed in; mask (nullable, dx's shape, in_dtype) is a ReLU mask applied after the
 * sum: dx = mask > 0 ? conv + add : 0. Every pixel of dx is written once (no zero fill needed). dy, w_dgrad, mask, add f16 /
 * bf16 (in_dtype), dx in_dtype or f32 (out_dtype); cin % 16 == 0, cout % 64 == 0; fp32 accumulation, fixed order
 * (bitwise reproducible). */
osr_status osr_conv2d_dgrad_s2(const osr_conv_params* p, const void* dy, const void* w_dgrad, const void* mask,
                               const void* add, void* dx, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Training step, backward half: losses and per-row stages. Every gradient is d(sum of weighted losses)/d(tensor)
 * times `loss_scale` (static loss scaling for fp16 gradient tensors; osr_sgd_step_multi_ex divides it out via grad_scale).
 * --------------------------------------------------------------------------------------------------------- */

/* Gradient of osr_rpn_losses_fwd w.r.t. the head's five pre-activation outputs per anchor: d_out5 (rows, 5) level-major
 * like the predictions = {d ltrb deltas (through decode + IoU), d centerness logit (through the sigmoid)}. */
osr_status osr_rpn_losses_bwd(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n,
                              const float* pred_deltas, const float* pred_ctr, const int8_t* labels_reg,
                              const int8_t* labels_obj, const float* matched_boxes, const float* ctr_target,
                              float loc_weight, float ctr_weight, int32_t batch_size_per_image, float loss_scale,
                              float* d_out5, void* stream);
osr_status osr_rpn_losses_bwd_ex(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n,
                                 const float* pred_deltas, const float* pred_ctr, const int8_t* labels_reg,
                                 const int8_t* labels_obj, const float* matched_boxes, const float* ctr_target,
                                 float loc_weight, float ctr_weight, int32_t batch_size_per_image, float loss_scale,
                                 const osr_loss_options* options, float* d_out5, void* stream);

/* ClsFreeRPNHead tail backward (classification_free_rpn.py:159-161): t (rows,256) is the hidden state after the 3x3 conv's
 * ReLU; outputs dt (rows,256, same dtype, already masked by t > 0), dw_tail (5,256), db_tail (5). */
int64_t osr_cfrpn_tail_bwd_workspace_bytes(void);
osr_status osr_cfrpn_tail_bwd(const void* t, int32_t dtype, int64_t rows, const float* w_tail, const float* d_out5, void* dt,
                              float* dw_tail, float* db_tail, int32_t accumulate, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* Sparse backward of the CF-RPN head's shared 3x3 convolution. ClsFreeRPN.losses (classification_free_rpn.py:446-490) sums over
 * the sampled anchors only (:299-316: <= 2 * BATCH_SIZE_PER_IMAGE per image), so d_out5 -- and the gradient of the hidden state
 * t = relu(conv3x3(p_l)) (:159-161) -- is zero on every other anchor row; autograd runs the conv's two gradients over the dense,
 * almost-all-zero tensor. These three entry points restate them on the non-zero rows (csrc/osr_rpn_sparse.hip):
 *  osr_rpn_sparse_rows: row_ids (cap) = the rows of d_out5 (rows,5) with a non-zero entry, ascending, -1 behind them; row_map
 *    (rows) = list slot of a row or -1; count2 = {min(found, cap), found}. Rows found beyond cap are dropped (the caller sizes cap
 *    by the sampling bound and may check count2[1]).
 *  osr_rpn_gather_cols: cols (cap, 9, 256) in the feature dtype = the im2col row of every listed anchor (tap-major, the 3x3 conv's
 *    K order; zero outside the map and for the -1 slots) from its level of `feats` (levels as in lv: level-major rows
 *    (img * h + y) * w + x), and d_out5_rows (cap, 5) = its five gradients. With the head's weight W viewed as (256, 2304):
 *    t_rows = relu(cols . W^T + b), dW = dt_rows^T . cols, y = dt_rows . W.
 *  osr_rpn_scatter_cols_add: grads[l] (n, h_l, w_l, 256), in place: every pixel adds, in tap order and in fp32, the rows
 *    y[row_map[q - tap offset]][tap] of its (<= 9) listed neighbours to the value already there and rounds once (no atomics; a pixel
 *    that no listed anchor reaches is not touched). y: (cap, 9, 256) fp32. */
int64_t osr_rpn_sparse_rows_workspace_bytes(void);
osr_status osr_rpn_sparse_rows(const float* d_out5, int64_t rows, int32_t cap, int32_t* row_ids, int32_t* row_map,
                               int32_t* count2, void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_rpn_gather_cols(const osr_rpn_levels* lv, const osr_pyramid* feats, int32_t feat_dtype, int32_t n,
                               const int32_t* row_ids, int32_t cap, const float* d_out5, void* cols, float* d_out5_rows,
                               void* stream);
osr_status osr_rpn_scatter_cols_add(const osr_rpn_levels* lv, int32_t n, const int32_t* row_map, const float* y,
                                    void* const* grads, int32_t grad_dtype, void* stream);

/* The same two with the gradient row width as a parameter (1..64): the stock RPN head's backward lists the rows of its
 * (rows, 5A) gradient (osr_std_rpn_losses_bwd) -- lv is then the PIXEL level table (num_anchors 1). osr_rpn_sparse_rows(...) =
 * osr_rpn_sparse_rows_ex(..., width 5, ...), osr_rpn_gather_cols likewise; d_rows_listed is (cap, width). */
osr_status osr_rpn_sparse_rows_ex(const float* d_rows, int64_t rows, int32_t width, int32_t cap, int32_t* row_ids, int32_t* row_map,
                                  int32_t* count2, void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_rpn_gather_cols_ex(const osr_rpn_levels* lv, const osr_pyramid* feats, int32_t feat_dtype, int32_t n,
                                  const int32_t* row_ids, int32_t cap, const float* d_rows, int32_t width, void* cols,
                                  float* d_rows_listed, void* stream);

/* Gradient of osr_roi_box_losses_fwd w.r.t. the (m,5) predictor output {4 deltas, IoU logit}. workspace 16 bytes. */
osr_status osr_roi_box_losses_bwd(const float* pred5, const float* proposal_boxes, const float* gt_boxes,
                                  const int64_t* gt_classes, const float* gt_iou, int64_t m, int32_t num_classes,
                                  const float reg_weights[4], float box_weight, float iou_weight, float loss_scale,
                                  float* d_pred5, void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_roi_box_losses_bwd_ex(const float* pred5, const float* proposal_boxes, const float* gt_boxes,
                                     const int64_t* gt_classes, const float* gt_iou, int64_t m, int32_t num_classes,
                                     const float reg_weights[4], float box_weight, float iou_weight, float loss_scale,
                                     const osr_loss_options* options, float* d_pred5, void* workspace,
                                     int64_t workspace_bytes, void* stream);

/* Gradient of osr_softmax_ce_loss_fwd w.r.t. the logits (m, num_known+1). workspace 16 bytes. */
osr_status osr_softmax_ce_loss_bwd(const float* logits, int64_t m, int32_t num_known, const int64_t* gt_classes,
                                   int32_t num_classes, float loss_weight, float loss_scale, float* d_logits,
                                   void* workspace, int64_t workspace_bytes, void* stream);

/* Gradient of osr_pln_loss_fwd w.r.t. the embeddings (m,d) and the RAW prototypes (num_known,d) (the forward normalises
 * them, prototype_learning_network.py:136). */
int64_t osr_pln_loss_bwd_workspace_bytes(int64_t m);
osr_status osr_pln_loss_bwd(const float* emb, int64_t m, int32_t d, const float* protos_raw, int32_t num_known,
                            const int64_t* gt_classes, const float* ious, float iou_thr, float alpha, float beta,
                            float loss_weight, float loss_scale, float* d_emb, float* d_protos, int32_t accumulate_protos,
                            void* workspace, int64_t workspace_bytes, void* stream);
osr_status osr_pln_loss_bwd_ex(const float* emb, int64_t m, int32_t d, const float* protos_raw, int32_t num_known,
                               int32_t reps, int32_t distance_type, const int64_t* gt_classes, const float* ious,
                               float iou_thr, float alpha, float beta, float loss_weight, float loss_scale, float* d_emb,
                               float* d_protos, int32_t accumulate_protos, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Training step of the stock detectron2 heads (Base-RCNN-FPN.yaml: RPN + StandardRPNHead, StandardROIHeads +
 * FastRCNNOutputLayers; csrc/osr_std_train.hip). Deterministic two-stage reductions as above.
 * --------------------------------------------------------------------------------------------------------- */
/* [d2] RPN.losses. pred_logits (rows*A) / pred_deltas (rows*A, 4): level-major as the head's GEMMs write them (levels->offset
 * counts anchors); labels (n,R) int8 in {-1,0,1} and matched_boxes (n,R,4): image-major, as osr_rpn_match_anchors /
 * osr_subsample_labels / osr_rpn_anchor_targets write them. loss_rpn_cls = sum_{label>=0} BCEWithLogits(logit, label) *
 * cls_weight / (batch_size_per_image * n); loss_rpn_loc = sum_{label=1} smooth_l1(delta - get_deltas(anchor, gt; b2b_weights),
 * beta) * loc_weight / (batch_size_per_image * n). out4 = {loss_rpn_cls, loss_rpn_loc, num_pos, num_neg}. workspace 4 KiB. */
osr_status osr_std_rpn_losses_fwd(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n, const float* pred_logits,
                                  const float* pred_deltas, const int8_t* labels, const float* matched_boxes,
                                  const float b2b_weights[4], float smooth_l1_beta, float cls_weight, float loc_weight,
                                  int32_t batch_size_per_image, float* out4, void* workspace, int64_t workspace_bytes,
                                  void* stream);
/* Its gradient, times loss_scale, as ONE (rows, 5A) fp32 buffer over the pixel rows: columns [0, A) the logits, [A, 5A) the
 * deltas (anchor a at A + 4a). Every element is written; only sampled anchors are non-zero. */
osr_status osr_std_rpn_losses_bwd(const osr_rpn_levels* levels, const float* cell_anchors, int32_t n, const float* pred_logits,
                                  const float* pred_deltas, const int8_t* labels, const float* matched_boxes,
                                  const float b2b_weights[4], float smooth_l1_beta, float cls_weight, float loc_weight,
                                  int32_t batch_size_per_image, float loss_scale, float* d_rows, void* stream);
/* [d2] FastRCNNOutputLayers.losses over m sampled rows (gt_classes: 0..K-1 foreground, K background, -1 padding -- skipped and
 * not counted). logits (m, K+1); pred_deltas rows of delta_stride floats: the 4 deltas at column 0 (cls_agnostic) or at 4c for
 * GT class c. loss_cls = mean cross entropy * cls_weight; loss_box_reg = sum_fg smooth_l1(delta - get_deltas(proposal, gt;
 * reg_weights), beta) * box_weight / max(rows, 1). out7 = {loss_cls, loss_box_reg, rows, correct, foreground, foreground
 * correct, foreground predicted as background} (argmax: first maximum). workspace 7 KiB. m = 0 gives zeros; the row arrays may
 * then be null. */
osr_status osr_fastrcnn_losses_fwd(const float* logits, const float* pred_deltas, int32_t delta_stride, int32_t cls_agnostic,
                                   const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_classes, int64_t m,
                                   int32_t num_classes, const float reg_weights[4], float smooth_l1_beta, float cls_weight,
                                   float box_weight, float* out7, void* workspace, int64_t workspace_bytes, void* stream);
/* Its gradient times loss_scale: d_logits (m, K+1), d_deltas (m, delta_stride); every element written. workspace 16 bytes. */
osr_status osr_fastrcnn_losses_bwd(const float* logits, const float* pred_deltas, int32_t delta_stride, int32_t cls_agnostic,
                                   const float* proposal_boxes, const float* gt_boxes, const int64_t* gt_classes, int64_t m,
                                   int32_t num_classes, const float reg_weights[4], float smooth_l1_beta, float cls_weight,
                                   float box_weight, float loss_scale, float* d_logits, float* d_deltas, void* workspace,
                                   int64_t workspace_bytes, void* stream);
/* StandardRPNHead tail backward: t (rows,256) fp32 hidden state after the 3x3 conv's ReLU, w_tail (width,256) = [W_obj; W_delta],
 * d_rows (rows, width). dt (rows,256) fp16/bf16 = (d_rows . w_tail) masked by t > 0; dw_tail (width,256) = d_rows^T . t;
 * db_tail (width) = column sums of d_rows. width = 5A, A = 1..8. */
int64_t osr_std_rpn_tail_bwd_workspace_bytes(void);
osr_status osr_std_rpn_tail_bwd(const float* t, int64_t rows, const float* w_tail, int32_t width, const float* d_rows, void* dt,
                                int32_t dt_dtype, float* dw_tail, float* db_tail, void* workspace, int64_t workspace_bytes,
                                void* stream);

/* RoIAlign backward: d feature pyramid (fp32 NHWC per level, zero-initialised by the caller; `dfeat->data` are written)
 * += scatter of dout (m,P,P,c) with the forward's geometry; fp32 atomic adds (the sums depend on their order: not bitwise
 * reproducible). pooled 1..7: one wave per RoI over per-axis weight tables; 8..OSR_ROI_MAX_POOLED_FWD: one workgroup per RoI,
 * torchvision's loop over every sample. Rows with batch_idx < 0 are not read. */
osr_status osr_roi_align_bwd(const osr_pyramid* dfeat, int32_t n, const float* boxes, const int32_t* batch_idx, int64_t m,
                             int32_t pooled, int32_t canonical_level, int32_t canonical_size, int32_t min_level,
                             const void* dout, int32_t dout_dtype, void* stream);

/* osr_roi_align_bwd with pooler options (osr_roi_options above; NULL = {1, 0}). */
osr_status osr_roi_align_bwd_opt(const osr_pyramid* dfeat, int32_t n, const float* boxes, const int32_t* batch_idx, int64_t m,
                                 int32_t pooled, int32_t canonical_level, int32_t canonical_size, int32_t min_level,
                                 const void* dout, int32_t dout_dtype, const osr_roi_options* options, void* stream);

/* The same gradient in pixel-centric form: one workgroup per 8 x 8 pixel tile of a level GATHERS the contributions of the image's RoIs
 * -- no atomics, no zero-initialised output (every element of dfeat is written exactly once, zeros where no RoI reaches), bitwise
 * reproducible (fixed summation order: list order, bin row, bin column). The RoI list must be image-major with a fixed stride:
 * rows [b * rois_per_image, (b + 1) * rois_per_image) belong to image b (batch_idx == b) or are padding (batch_idx < 0);
 * m == n * rois_per_image, rois_per_image <= 1024, c <= 256. Otherwise OSR_ERR_UNSUPPORTED with nothing launched: zero dfeat and
 * call osr_roi_align_bwd. out_dtype: OSR_F32, or dout's dtype -- the fp32 sums are then rounded once on the way out (what a separate
 * cast of the fp32 pyramid would give), dfeat->data pointing at tensors of that type. Same reference lines as osr_roi_align_bwd.
 * Non-finite dout: a bin's weights are not tested before they multiply, so an Inf or NaN in dout[r][by][bx][ch] reaches channel ch of
 * every pixel that bin weighs (as in the reference) and may also turn into NaN (0 * Inf) elsewhere in the 8 x 8 tiles RoI r reaches,
 * never outside them and never in another channel. It is never dropped: the training step's overflow check (osr_check_finite) relies
 * on that. Rows with batch_idx < 0 are not read at all. */
osr_status osr_roi_align_bwd_dense(const osr_pyramid* dfeat, int32_t n, const float* boxes, const int32_t* batch_idx, int64_t m,
                                   int32_t rois_per_image, int32_t pooled, int32_t canonical_level, int32_t canonical_size, int32_t min_level,
                                   const void* dout, int32_t dout_dtype, int32_t out_dtype, void* stream);
/* osr_roi_align_bwd_dense with pooler options (NULL = {1, 0}); same envelope, same summation order. */
osr_status osr_roi_align_bwd_dense_opt(const osr_pyramid* dfeat, int32_t n, const float* boxes, const int32_t* batch_idx, int64_t m,
                                       int32_t rois_per_image, int32_t pooled, int32_t canonical_level, int32_t canonical_size,
                                       int32_t min_level, const void* dout, int32_t dout_dtype, int32_t out_dtype,
                                       const osr_roi_options* options, void* stream);

/* g[i] = act[i] > 0 ? g[i] : 0, in place (gradient through a ReLU whose output is act). */
osr_status osr_relu_mask(void* g, int32_t g_dtype, const void* act, int32_t act_dtype, int64_t n, void* stream);
/* out[i] = (T)(a_f32[i] + b[i]); either addend may be null. */
osr_status osr_add_cast(const float* a_f32, const void* b, void* out, int32_t dtype, int64_t n, void* stream);
/* mode 0: FPN nearest-2x upsample-add backward, out (n,ho,wo,c) = base + 2x2 sums of src (n,hs,ws,c), ho = ceil(hs/2);
 * mode 1: LastLevelMaxPool (p6 = p5[::2,::2]) backward, out (n,ho,wo,c) = base, plus src[y/2][x/2] at even (y,x). */
osr_status osr_pool_bwd(const void* src, int32_t hs, int32_t ws, const void* base, void* out, int32_t n, int32_t ho,
                        int32_t wo, int32_t c, int32_t mode, int32_t dtype, void* stream);

/* Backward-data weight of a convolution, (cout,kh,kw,cin) -> (cin,kh,kw,cout) spatially flipped (the forward MFMA kernel run on
 * it with padding k-1-pad is the data gradient; a 1x1 layer / FC matrix is transposed). Run once per SGD step on the refreshed
 * working copies. dtype: element type of both tensors (f16/bf16/f32). out must not alias weight. */
osr_status osr_pack_dgrad_weight(const void* weight, void* out, int32_t cout, int32_t kh, int32_t kw, int32_t cin,
                                 int32_t dtype, void* stream);

/* osr_pack_dgrad_weight over every entry of a DEVICE-resident table, one launch (csrc/osr_pack_dgrad.hip; the same tile body).
 * `chunks`: (tensor index, tile index) int32 pairs, one per workgroup, on the device; the tile index of a 32 x 32 tile is
 * (tap * ceil(cout / 32) + co_tile) * ceil(cin / 32) + ci_tile. The caller builds both once (the buffers' addresses are stable
 * across steps). */
typedef struct osr_pack_tensor {
    const void* src;        /* (cout, kh, kw, cin) */
    void* dst;              /* (cin, kh, kw, cout), spatially flipped */
    int32_t cout, kh, kw, cin;
    int32_t elem_bytes;     /* 2 or 4 */
    int32_t reserved;
} osr_pack_tensor;
osr_status osr_pack_dgrad_weight_multi(const osr_pack_tensor* table, const int32_t* chunks, int32_t num_chunks, void* stream);

/* The SGD of a training step ([d2] build_optimizer -> torch.optim.SGD, csrc/osr_solver.hip): momentum and weight decay on the fp32
 * masters, with the solver options beyond one SGD group -- per-parameter gradient clipping (SOLVER.CLIP_GRADIENTS, CLIP_TYPE
 * "value" / "norm"), a learning-rate factor and weight decay per parameter group (BIAS_LR_FACTOR, WEIGHT_DECAY_BIAS) and Nesterov
 * momentum. The whole update is ONE launch, osr_sgd_step_multi_ex, over a DEVICE-resident table the caller builds once; norm
 * clipping puts the norm pass, osr_grad_norm_partials, in front of it. The table entries are SEGMENTS: one parameter each, a
 * row-aligned element range of a master (param / grad / momentum / row_scale / lowp already offset to its first row).
 * `chunks`: (segment index, chunk index) int32 pairs, one per workgroup, on the device; chunk c of a segment is its elements
 * [c * chunk_elems, min((c + 1) * chunk_elems, n)), and the chunks of a segment are the contiguous run [chunk0, chunk0 + nchunks)
 * of the list. row_scale (nullable): the folded FrozenBN scale per leading-dimension row of row_elems elements.
 * Per element, with d = grad*grad_scale*row_scale:
 *   clip_mode VALUE: d = clamp(d, -clip_value, clip_value); NORM: d *= c when c = clip_value / (||d||_norm_type + 1e-6) < 1,
 *   the norm over the segment's elements (inf: max |d|);
 *   d += weight_decay*param; buf = momentum*buf + d; d = nesterov ? d + momentum*buf : buf; param -= lr*lr_factor*d;
 *   lowp (nullable) = (T)(param*row_scale).
 * Every product and sum is rounded to fp32 on its own (no fused multiply-add): with clip_mode NONE, lr_factor 1, nesterov 0 this
 * is torch.optim.SGD's plain step, and how the table is cut into segments and chunks does not change a bit of the result. */
typedef enum { OSR_CLIP_NONE = 0, OSR_CLIP_VALUE = 1, OSR_CLIP_NORM = 2 } osr_clip_mode;
typedef struct osr_sgd_segment {
    float* param;
    const float* grad;
    float* momentum;
    const float* row_scale; /* nullable: one value per row of row_elems elements, from the segment's first row */
    void* lowp;             /* nullable: low-precision working copy, lowp_dtype */
    int64_t n;              /* elements of the segment */
    int64_t row_elems;      /* >= 1 */
    int32_t lowp_dtype;
    int32_t chunk0;         /* first chunk of this segment in `chunks` (and in the norm partials) */
    int32_t nchunks;
    float lr_factor;
    float weight_decay;
    int32_t nesterov;
} osr_sgd_segment;
/* Norm pass: partials[c] (double, one per chunk) = sum over chunk c of |grad*grad_scale*row_scale|^norm_type, or its max for
 * norm_type = inf (1, 2 and inf special-cased; any other norm_type > 0 through powf). One read of every segment's gradient;
 * finite_flag (nullable, device int32, preset to 1) is cleared when any of it is inf or NaN, as osr_check_finite would. No atomics. */
osr_status osr_grad_norm_partials(const osr_sgd_segment* table, const int32_t* chunks, int32_t num_chunks, int32_t chunk_elems,
                                  float grad_scale, float norm_type, double* partials, int32_t* finite_flag, void* stream);
/* SGD over every segment, one launch; clip_mode NORM reads the partials of osr_grad_norm_partials (same table and chunks) and
 * sums each segment's in a fixed order. apply_flag (nullable): when it reads 0 the launch changes nothing. */
osr_status osr_sgd_step_multi_ex(const osr_sgd_segment* table, const int32_t* chunks, int32_t num_chunks, int32_t chunk_elems,
                                 float lr, float momentum, float grad_scale, int32_t clip_mode, float clip_value, float norm_type,
                                 const double* partials, const int32_t* apply_flag, void* stream);

/* Overflow guard: *flag (device int32, preset to 1 by the caller) is cleared when any of the n floats of x is inf or NaN.
 * The reference trains in fp32 and has no such step (train.py:135-146); the fp16 gradients of this build do, and an
 * overflowed iteration must not reach the fp32 masters or a checkpoint. x 16-byte aligned. Asynchronous, no host sync. */
osr_status osr_check_finite(const float* x, int64_t n, int32_t* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSR_H_ */
